"""The keyed audio watermark without a GPU: the surface (header, struct, bindings, keywords, refusals) and the properties of the float64
restatement tests/watermark_ref.py -- the hash, depth 0, streams that concatenate to the whole call, and what the detector decides on seeded
synthetic voiced signals.  The restatement is the reference of tests/test_watermark_gpu.py; these tests are what show the scheme works."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import denoise_ref as D
import watermark_ref as W
from stream_util import cut, header, supported
from zerovox_amd import _lib, watermark as WM

KEY = 0xC0FFEE1234567
M64 = (1 << 64) - 1
_sig = {}


def voiced(seconds, seed):
    if (seconds, seed) not in _sig:
        x = W.voiced_signal(seconds, seed)
        y = W.embed(x, KEY).astype(np.float32)               # the defaults, depth 1 dB; f32 as the device delivers it
        x.setflags(write=False); y.setflags(write=False)
        _sig[(seconds, seed)] = (x, y)
    return _sig[(seconds, seed)]


# ---- surface --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    h = header()
    decl = re.search(r"zvx_status\s+zvx_watermark\s*\(([^;]*)\)\s*;", h).group(1)
    names = lambda d: [a.strip().split()[-1].lstrip("*") for a in d.split(",")]      # noqa: E731
    assert names(decl) == ["ctx", "in", "nsamples", "B", "Nmax", "params", "out", "out_stride", "flags"]
    decl = re.search(r"zvx_status\s+zvx_watermark_ex\s*\(([^;]*)\)\s*;", h).group(1)
    assert names(decl)[-4:] == ["in_origin", "out_begin", "out_count", "last"] and names(decl)[:9] == ["ctx", "in", "nsamples", "B", "Nmax", "params", "out", "out_stride", "flags"]
    decl = re.search(r"zvx_status\s+zvx_watermark_detect\s*\(([^;]*)\)\s*;", h).group(1)
    assert names(decl) == ["ctx", "in", "nsamples", "B", "Nmax", "params", "window_frames", "score", "offset", "window", "win_score", "win_offset",
                           "NWmax", "flags"]
    assert re.search(r"typedef struct zvx_watermark_params\s*\{\s*uint64_t\s+key;[^}]*float\s+depth_db;[^}]*float\s+lo_hz, hi_hz;[^}]*int32_t\s+block_frames;"
                     r"[^}]*int32_t\s+band_bins;[^}]*int32_t\s+period_blocks;[^}]*int32_t\s+reserved;[^}]*\}\s*zvx_watermark_params;", h)
    assert "post.watermark" in h and "post.wmdetect" in h and "0x9E3779B97F4A7C15" in h
    sec = h[h.index("Keyed audio watermark on the device"):h.index("typedef struct zvx_watermark_params")]
    assert "Not here:" in sec and "_rows" in sec and "sessions" in sec and "codecs" in sec and "time-stretching" in sec and "inaudible" in sec
    assert "NOT reliably detectable" in sec                  # the caveat about short telephone-band clips


def test_struct_bindings_and_exports():
    f = _lib.WatermarkParams._fields_
    assert [n for n, _ in f] == ["key", "depth_db", "lo_hz", "hi_hz", "block_frames", "band_bins", "period_blocks", "reserved"]
    assert C.sizeof(_lib.WatermarkParams) == 40 and _lib.WatermarkParams.key.offset == 0 and _lib.WatermarkParams.depth_db.offset == 8
    assert _lib.WatermarkParams.reserved.offset == 32 and dict(f)["key"] is C.c_uint64
    assert {"zvx_watermark", "zvx_watermark_ex", "zvx_watermark_detect"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert len(lib.zvx_watermark.argtypes) == 9 and len(lib.zvx_watermark_ex.argtypes) == 13 and len(lib.zvx_watermark_detect.argtypes) == 14
    assert lib.zvx_watermark_ex.argtypes[-4:] == [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    # a NULL context is refused before anything else is looked at
    assert lib.zvx_watermark(None, None, None, 0, 0, None, None, 0, 0) == _lib.ZVX_E_INVALID
    assert lib.zvx_watermark_ex(None, None, None, 0, 0, None, None, 0, 0, 0, 0, -1, 1) == _lib.ZVX_E_INVALID
    assert lib.zvx_watermark_detect(None, None, None, 0, 0, None, 0, None, None, None, None, None, 0, 0) == _lib.ZVX_E_INVALID
    for name in ("watermark", "watermark_window", "watermark_detect", "watermark_device"):
        assert callable(getattr(_lib.Context, name))
    p = inspect.signature(_lib.Context.watermark_window).parameters
    assert [p[k].default for k in ("in_origin", "out_begin", "out_count", "last")] == [0, 0, -1, True]
    assert inspect.signature(_lib.Context.watermark_detect).parameters["window_frames"].default == 256 == WM.WINDOW_FRAMES


def test_keyword_defaults_and_kinds():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    for f in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long, ZeroVoxTTS.tts_stream, ZeroVoxTTS.tts_stream_many):
        p = inspect.signature(f).parameters["watermark"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, f
    assert inspect.signature(ZeroVox.inference_ex).parameters["watermark"].default is None
    assert inspect.signature(ZeroVox.vocode_stream).parameters["watermark"].default is None
    p = inspect.signature(ZeroVoxTTS.detect_watermark).parameters
    assert list(p)[1:4] == ["wav", "key", "sampling_rate"] and p["sampling_rate"].default is None
    assert WM.EMBED_DEFAULTS == dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64) == W.DEFAULTS
    assert WM.WatermarkResult._fields == ("score", "offset", "window", "detected", "threshold", "windows")
    assert ZeroVoxTTS._watermark(None) is None
    assert ZeroVoxTTS._watermark(7) == dict(WM.EMBED_DEFAULTS, key=7) == ZeroVoxTTS._watermark({"key": 7})
    assert ZeroVoxTTS._watermark({"key": 7, "depth_db": 2.0})["depth_db"] == 2.0
    assert WM.sign_table(KEY, 3, 5) == W.sign_table(KEY, 3, 5).tolist() and WM.mix64(12345) == W.mix64(12345)
    from zerovox_amd import stream
    assert issubclass(WM.WatermarkPlanner, stream.ReachPlanner) and WM.WatermarkPlanner(1024).R == 1023 == WM.reach(1024) == W.reach(1024)
    assert WM.stream_watermark is stream.stream_windows


def test_refusals_come_before_the_model_is_touched():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                    # no model, no device: a refusal must not need either
    bad = [dict(key=1, depth_db=-0.5), dict(key=1, depth_db=6.5), dict(key=1, depth_db=float("nan")), dict(key=1, lo_hz=-1.0),
           dict(key=1, lo_hz=9000.0), dict(key=1, hi_hz=float("inf")), dict(key=1, block_frames=0), dict(key=1, band_bins=0),
           dict(key=1, period_blocks=0), dict(key=1, period_blocks=257), dict(key=1, reserved=1), dict(depth_db=1.0), dict(key=-1), dict(key=1 << 64),
           True, "key", 1.5]
    for w in bad:
        for call in (synth.tts, synth.tts_ex, synth.tts_long):
            with pytest.raises(ValueError, match="watermark"):
                call("hello there", None, watermark=w)
        with pytest.raises(ValueError, match="watermark"):
            synth.tts_stream("hello there", None, watermark=w)
    with pytest.raises(ValueError, match="no watermark stage yet"):
        synth.tts_stream("hello there", None, watermark=KEY, resident=True)
    with pytest.raises(ValueError, match="no watermark stage yet"):
        next(synth.tts_stream_many(["hello there"], None, watermark=KEY))
    with pytest.raises(ValueError, match="watermark"):
        synth.detect_watermark(np.zeros(8, np.float32), KEY, period_blocks=300)


# ---- the restatement's own properties ---------------------------------------------------------------------------------------------------------
def test_mix64_against_hand_computed_values():
    """the splitmix64 generator seeded with 0 emits mix64(0), mix64(g), mix64(2 g), g = 0x9E3779B97F4A7C15: its published first outputs"""
    g = 0x9E3779B97F4A7C15
    assert W.mix64(0) == 0xE220A8397B1DCDAF
    assert W.mix64(g) == 0x6E789E6AA1B965F4
    assert W.mix64((2 * g) & M64) == 0x06C45D188009454F
    assert W.bands(250.0, 8000.0, 4, 1024, 22050) == (12, 89) and W.bands(250.0, 3400.0, 4, 1024, 22050) == (12, 36)
    assert W.bands(0.0, 20000.0, 1, 1024, 22050) == (0, 512)                          # hi is clipped to rate / 2
    s = W.sign_table(KEY, 64, 89)
    assert set(np.unique(s)) == {-1, 1} and abs(int(s.sum())) < 4 * np.sqrt(s.size) and not np.array_equal(s, W.sign_table(KEY + 1, 64, 89))
    assert W.windows(259, 256) == [(0, 256), (128, 259)] and W.windows(256, 256) == [(0, 256)] and W.windows(5, 0) == [(0, 5)] and W.windows(0, 8) == []


def test_depth_zero_is_a_copy_and_the_mark_is_what_the_gain_says():
    x = voiced(1.5, 11)[0]
    assert np.array_equal(W.embed(x, KEY, depth_db=0.0), x.astype(np.float64))
    assert np.array_equal(W.embed_window(x[100:5000], KEY, 100, 100 + 1023, 500, False, depth_db=0.0), x[1123:1623].astype(np.float64))
    # a sine on the centre of a band, long enough for its middle to lie under whole blocks: it is scaled by g_up or g_dn, block by block
    k_lo, J = W.bands(250.0, 8000.0, 4, 1024, 22050)
    j, TB, P = 20, 8, 64
    kbin = k_lo + 4 * j + 1
    n = 256 * 56
    tone = 0.5 * np.sin(2 * np.pi * kbin * np.arange(n) / 1024)
    y = W.embed(tone, KEY, depth_db=3.0)
    g_up, g_dn = W.gains(3.0)
    assert abs(g_up * g_dn - 1.0) < 1e-6 and abs(20 * np.log10(g_up) - 3.0) < 1e-5
    sg = W.sign_table(KEY, P, J)
    pad = (1024 - 256) // 2
    for c in range(1, 6):                                    # between the centres of frames c TB + 3 and c TB + 4: under frames of block c only
        mid = (c * TB + TB // 2) * 256 - pad + 512 - 128
        seg = slice(mid - 128, mid + 128)
        ratio = np.sqrt(np.mean(y[seg] ** 2) / np.mean(tone[seg] ** 2))
        assert abs(ratio - (g_up if sg[c, j] > 0 else g_dn)) < 1e-6, (c, ratio)      # (a Hann spreads a bin-centred tone over 3 bins: all in band j)
    assert len({int(sg[c, j]) for c in range(1, 6)}) == 2    # both gains occur


@pytest.mark.parametrize("p", [dict(block_frames=2, band_bins=2, period_blocks=2), {}])
def test_planned_stream_concatenates_exactly_to_the_whole_call(p):
    """odd chunk sizes, a chunk shorter than the reach, `last`: the pieces are the whole call's samples to the last bit of float64"""
    rng = np.random.default_rng(5)
    R = WM.reach(1024)
    x = voiced(1.5, 11)[0][:9 * 256 + 77].astype(np.float64)
    want = W.embed(x, KEY, **p)
    assert np.max(np.abs(want - x)) > 1e-3
    for name, sizes in {"odd": [257, 1001, 333], "shorter than R": [341], "one chunk": [len(x)], "random": [int(v) for v in rng.integers(1, 2048, 64)]}.items():
        windows = []

        def window_fn(samples, in_origin, out_begin, out_count, last):
            windows.append((in_origin, len(samples), out_begin, out_count, last))
            return W.embed_window(samples, KEY, in_origin, out_begin, out_count, last, **p)

        got = np.concatenate(list(WM.stream_watermark(cut(x, sizes), WM.WatermarkPlanner(1024), window_fn)))
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert all(supported(R, *w) for w in windows) and windows[-1][4], name
        assert max(k for (_, k, _, _, _) in windows) <= max(sizes) + 2 * R


def test_detection_on_synthetic_voiced_signals():
    """At the defaults and depth 1 dB, on seeded synthetic voiced signals with pauses, 1.5 s (two seeds) and 3 s at 22.05 kHz.
    Choosing the threshold (measured with this restatement): the largest null score over 256 wrong keys x all 512 offsets x every window
    on the marked, the cut and the unmarked signals (and the join below) is 4.75; the smallest score with the right key, aligned or cut by
    5000 samples, is 7.10 (1.5 s; 12.2 at 3 s).  watermark.THRESHOLD = 5.5 lies between them, nearer the null side, 0.75 above it.
    This test keeps 32 wrong keys."""
    thr = WM.THRESHOLD
    assert 4.75 + 0.5 <= thr < (4.75 + 7.10) / 2
    wrong = [KEY ^ (1 << k) for k in range(16)] + [(KEY * (2 * k + 3)) & M64 for k in range(16)]
    for seconds, seed in ((1.5, 11), (1.5, 12), (3.0, 13)):
        x, y = voiced(seconds, seed)
        score, off, win, per = W.detect(y, KEY)
        cscore, coff, _, _ = W.detect(y[5000:], KEY)
        null = float(max(W.null_scores(y, wrong).max(), W.null_scores(x, wrong + [KEY]).max()))
        print(f"{seconds} s seed {seed}: right key {score:.2f} (offset {off}), cut by 5000 {cscore:.2f} (offset {coff}), largest null {null:.2f}")
        assert score >= thr and off == 0
        assert cscore >= thr and abs(coff - 5000 / 256) <= 1.0          # the true offset, 19.5 frames, within one frame
        assert null < thr


def test_a_join_of_two_sentences_is_detected_through_the_windows():
    thr = WM.THRESHOLD
    ya, yb = voiced(1.5, 11)[1], voiced(1.5, 12)[1]
    joined = np.concatenate([ya[3000:], np.zeros(2000, np.float32), yb[7001:]])
    score, off, win, per = W.detect(joined, KEY, window_frames=128)
    T = 8 * 64
    cuts = [3000 / 256, (7001 - (len(ya) - 3000 + 2000)) / 256]            # each sentence's own cut, in frames
    hits = [(s, o) for s, o in per if s >= thr]
    print(f"joined: {[(round(s, 2), o) for s, o in per]}; cuts {cuts}")
    assert score >= thr and len(per) == 3
    for c in cuts:
        assert any(min((o - c) % T, (c - o) % T) <= 1.0 for _, o in hits), (c, hits)
    assert W.null_scores(joined, [KEY ^ 1, KEY ^ 2, KEY + 99], window_frames=128).max() < thr
    # a detector band narrower than the embedder's: bands are counted from k_lo
    narrow = W.detect(ya, KEY, hi_hz=3400.0)
    assert narrow[1] == 0 and 0 < narrow[0] < W.detect(ya, KEY)[0]
