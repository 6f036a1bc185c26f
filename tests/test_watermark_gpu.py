"""The keyed audio watermark on the MI355X: zvx_watermark / zvx_watermark_ex / zvx_watermark_detect against tests/watermark_ref.py (float64
NumPy, never the library), the exact corners of include/zvx.h, row independence, the windows, the detector's decisions end to end, and the
watermark keyword of ZeroVoxTTS.tts / tts_stream.
Small parameters (TB = 2, P = 2, KB = 2) stand next to the defaults so that every boundary -- the edge of the 4-frame workgroup, block and
period wrap -- occurs on rows of a few frames.
The bounds.  The parity tests take rule (c) of tests/spectral_ref.py on their own data -- twice the largest element error of two f32
restatements of the pipeline (embed) or of the detector's two launches (the z of every offset) over 8 data seeds, nothing of it measured
on a device -- and never more than the earlier constants, which stay as caps.  Those were: embed, an f32 FFT pair of 1024 points, one
multiply per marked bin and an overlap-add of 4 frames, as the denoiser: 4x the largest error MEASURED over the parity cases (2.5e-7,
the denoiser's figure; see MEASURED_EMBED); detect, sums of some 10^4 f32 band log-energies normalised to unit variance: 4x the largest
|score - ref| MEASURED over the cases below.  The other tests keep the constants."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import denoise_ref as D
import spectral_ref as S
import watermark_ref as W
from stream_util import err, same_bits, supported, vp, window_of
from zerovox_amd import _lib, config as zcfg, pack, watermark as WM, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
N_FFT, HOP, RATE = 1024, 256, 22050
PAD = (N_FFT - HOP) // 2
KEY = 0xC0FFEE1234567
SMALL = dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=2, band_bins=2, period_blocks=2)
DEFAULT = dict(WM.EMBED_DEFAULTS)
INV, BUF, UNSUP = 1, 5, 6


def length_for(F):
    """the shortest row of F frames, plus an odd bit"""
    return (F - 1) * HOP + N_FFT - 2 * PAD + 37


# F = 3, 4, 5: the edge of the 4-frame workgroup; 8, 9: block and period wrap (TB = 2, P = 2: the period is 4 frames); the minimum length
BATCHES = [(length_for(3), length_for(4), length_for(5)), (length_for(8), length_for(9), D.min_samples(N_FFT, HOP))]
# Largest |out - ref| measured over both batches and both parameter sets (MI355X, rows with |x| <= 1): 2.521e-7 (TB = 2 / P = 2 / KB = 2, the
# row of 5 frames; per case 2.52e-7 / 2.02e-7 / 2.21e-7 / 2.32e-7).  LIMIT = 4x that: 1.008e-6.  The denoiser measures 2.475e-7 on the same
# transform pair with gains <= 1; here half the marked bins are scaled UP by 1.122 (1 dB), and the inverse transform's round-off scales with
# them -- 2 % above the denoiser's figure, the same order.
MEASURED_EMBED = 2.521e-7
LIMIT_EMBED = 4.0 * MEASURED_EMBED
assert LIMIT_EMBED <= 1e-4                                   # the denoiser's ceiling: a 1024-point f32 FFT pair cannot justify more
# Largest |score - ref| measured over test_detector_scores_against_the_reference's cases (scores of 2 .. 13.5): 7.745e-6.  LIMIT = 4x that.
MEASURED_DETECT = 7.745e-6
LIMIT_DETECT = 4.0 * MEASURED_DETECT
_ctx, _sig, _ref = {}, {}, {}


def ctx_for():
    if "c" not in _ctx:
        cfg = zcfg.reduced_modelcfg("styletts")
        cfg["audio"].update(fft_size=N_FFT, hop_size=HOP, win_length=N_FFT)
        h = zcfg.hifigan_config("tiny")
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
        _ctx["c"] = _lib.Context(man, blob, 0)
        assert _ctx["c"].get_int("fft_size") == N_FFT and _ctx["c"].hop == HOP and _ctx["c"].get_int("sampling_rate") == RATE
    return _ctx["c"]


def signal(rng, n):
    i = np.arange(n)
    x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 37.3 * i / N_FFT + 0.4) + 0.2 * np.sin(2 * np.pi * 120.0 * i / N_FFT + 1.1)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def rows_of(lengths, seed=0):
    """seed 0 is what the device runs; the other seeds feed rule (c)"""
    if (lengths, seed) not in _sig:
        rng = np.random.default_rng(4242 + sum(lengths) + 7919 * seed)
        _sig[(lengths, seed)] = [signal(rng, k) for k in lengths]
        for r in _sig[(lengths, seed)]:
            r.setflags(write=False)
    return _sig[(lengths, seed)]


def rule_c_embed(lengths, name):
    """spectral_ref's rule (c) on this case's own rows: the largest-element limit of the errors divided by spectral_ref.ola_scale"""
    if ("c", lengths, name) not in _ref:
        _ref[("c", lengths, name)] = S.embed_margin_of(lambda s: rows_of(lengths, s), SMALL if name == "small" else DEFAULT, N_FFT, HOP, N_FFT, RATE, KEY)
    return _ref[("c", lengths, name)]


def padded(rows):
    n = np.array([len(r) for r in rows], np.int32)
    nmax = int(n.max())
    x = np.full((len(rows), nmax + (nmax % 2 == 0)), SENTINEL32, np.uint32).view(np.float32)       # nothing behind a row's end may be read
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def prm_of(p, key=KEY):
    return _lib.WatermarkParams(key, p["depth_db"], p["lo_hz"], p["hi_hz"], p["block_frames"], p["band_bins"], p["period_blocks"], 0)


def raw(ctx, x, n, Nmax, prm, out, stride, flags=0, win=None, B=None):
    B = len(n) if B is None else B
    p = C.byref(prm) if prm is not None else None
    if win is None:
        return ctx._lib.zvx_watermark(ctx._h, vp(x), vp(n), B, Nmax, p, vp(out), stride, flags)
    return ctx._lib.zvx_watermark_ex(ctx._h, vp(x), vp(n), B, Nmax, p, vp(out), stride, flags, *[int(v) for v in win])


def run(ctx, x, n, p, pcm16=False, key=KEY):
    B, Nmax = x.shape
    stride = Nmax + 3
    out = np.full((B, stride), 0x5A5B, np.int16) if pcm16 else np.full((B, stride), SENTINEL32, np.uint32).view(np.float32)
    rc = raw(ctx, x, n, Nmax, prm_of(p, key), out, stride, _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, err(ctx)
    tail = out if pcm16 else out.view(np.uint32)
    assert all(np.all(tail[b, n[b]:] == (0x5A5B if pcm16 else SENTINEL32)) for b in range(B))        # nothing behind a row is touched
    return out


def reference(lengths, name):
    if (lengths, name) not in _ref:
        p = SMALL if name == "small" else DEFAULT
        _ref[(lengths, name)] = [W.embed(r, KEY, n_fft=N_FFT, hop=HOP, win_length=N_FFT, rate=RATE, **p) for r in rows_of(lengths)]
    return _ref[(lengths, name)]


@pytest.mark.parametrize("name", ["small", "default"])
@pytest.mark.parametrize("lengths", BATCHES)
def test_embed_against_the_float64_reference(lengths, name):
    ctx = ctx_for()
    p = SMALL if name == "small" else DEFAULT
    rows = rows_of(lengths)
    x, n = padded(rows)
    assert [D.geometry(k, N_FFT, HOP)[1] for k in lengths] in ([3, 4, 5], [8, 9, 1])
    out = run(ctx, x, n, p)
    mg = rule_c_embed(lengths, name)
    print(mg.line(f"embed {name} {lengths}"))
    worst, share = 0.0, 0.0
    for b, r in enumerate(reference(lengths, name)):
        ev = np.abs(out[b, :n[b]].astype(np.float64) - r)
        bound = np.minimum(LIMIT_EMBED, mg.max_limit * S.ola_scale(int(n[b]), N_FFT, HOP, N_FFT))
        e = float(ev.max())
        moved = float(np.max(np.abs(r - rows[b].astype(np.float64))))
        print(f"{name} row {b} (n = {n[b]}): max |out - ref| = {e:.3e}, the mark moves the row by up to {moved:.4f}")
        assert moved > 1e-3, (b, moved)                      # the mark acts: 1 dB on broadband rows
        worst, share = max(worst, e), max(share, float(np.max(ev / bound)))
        assert np.all(ev <= bound), (name, lengths, b, float(np.max(ev / bound)))
    print(f"{name} {lengths}: worst {worst:.3e}; worst err / min(LIMIT_EMBED {LIMIT_EMBED:.3e}, rule (c) {mg.max_limit:.3e} x its scale) = {share:.3f}")
    assert worst <= LIMIT_EMBED, (name, lengths, worst)


def test_depth_zero_batch_row_alone_in_place_and_pcm16():
    ctx = ctx_for()
    rows = rows_of(BATCHES[0])
    x, n = padded(rows)
    zero = run(ctx, x, n, {**SMALL, "depth_db": 0.0})
    assert all(same_bits(zero[b, :n[b]], rows[b]) for b in range(3))                                  # depth 0: the bits of x
    out = run(ctx, x, n, SMALL)
    for b, r in enumerate(rows):                                                                       # a row in a batch equals the row alone
        x1, n1 = padded([r])
        assert same_bits(run(ctx, x1, n1, SMALL)[0, :n[b]], out[b, :n[b]]), b
    xin = np.array(x)                                                                                  # in place equals out of place
    assert raw(ctx, xin, n, x.shape[1], prm_of(SMALL), xin, x.shape[1]) == 0, err(ctx)
    assert all(same_bits(xin[b, :n[b]], out[b, :n[b]]) and np.all(xin.view(np.uint32)[b, n[b]:] == SENTINEL32) for b in range(3))
    pcm = run(ctx, x, n, SMALL, pcm16=True)                                                            # the resampler's rule on the f32 result
    assert all(np.array_equal(pcm[b, :n[b]], D.pcm16(out[b, :n[b]])) for b in range(3))
    # another key, another mark; the same key, the same bits
    assert not same_bits(run(ctx, x, n, SMALL, key=KEY + 1)[0, :n[0]], out[0, :n[0]]) and same_bits(run(ctx, x, n, SMALL), out)


def test_a_non_finite_row_leaves_the_others_untouched():
    """zvx_vocode_mel's rule: the call succeeds, nothing faults, that row is unspecified, every other row is bit for bit what it is
    without it -- for the embedder and for the detector"""
    ctx = ctx_for()
    rows = rows_of(BATCHES[1])
    x, n = padded(rows)
    want = run(ctx, x, n, SMALL)
    bad = np.array(x)
    bad[0, 5] = np.nan
    bad[0, 900] = np.inf
    out = run(ctx, bad, n, SMALL)
    assert all(same_bits(out[b, :n[b]], want[b, :n[b]]) for b in (1, 2))
    kw = {k: v for k, v in SMALL.items() if k != "depth_db"}
    clean = ctx.watermark_detect(x, KEY, lengths=n, window_frames=4, **kw)
    dirty = ctx.watermark_detect(bad, KEY, lengths=n, window_frames=4, **kw)
    assert dirty[1] == clean[1] and dirty[2] == clean[2]
    assert ctx.watermark_detect(x, KEY, lengths=n, window_frames=4, **kw) == clean           # ... and the context goes on as before


def test_bins_outside_the_band_are_not_touched():
    """a band above all content (two tones under a smooth envelope: the float64 reference moves the row by less than 1e-8 at 6 dB): the
    marked row equals the unmarked one within the FFT pair's error -- the bins below the band go through the transform pair with no
    multiply -- while the same row with the band over the tones moves by tenths"""
    ctx = ctx_for()
    k = length_for(9)
    i = np.arange(k)
    rows = [(np.hanning(k) ** 2 * (0.5 * np.sin(2 * np.pi * 300.0 * i / RATE) + 0.3 * np.sin(2 * np.pi * 1234.5 * i / RATE + 1.0))).astype(np.float32)]
    x, n = padded(rows)
    high = {**SMALL, "depth_db": 6.0, "lo_hz": 9000.0, "hi_hz": 11000.0}
    ref = W.embed(rows[0], KEY, n_fft=N_FFT, hop=HOP, win_length=N_FFT, rate=RATE, **high)
    assert float(np.max(np.abs(ref - rows[0]))) < 1e-8
    out = run(ctx, x, n, high)
    e = float(np.max(np.abs(out[0, :k].astype(np.float64) - rows[0])))
    print(f"band above the content: max |out - x| = {e:.3e}")
    assert e <= LIMIT_EMBED
    inside = run(ctx, x, n, {**SMALL, "depth_db": 6.0})
    assert float(np.max(np.abs(inside[0, :k] - rows[0]))) > 0.05


def test_windows_concatenate_to_the_whole_call():
    ctx = ctx_for()
    R = WM.reach(N_FFT)
    for p in (SMALL, DEFAULT):
        rows = rows_of(BATCHES[1][:2])
        x, n = padded(rows)
        want = run(ctx, x, n, p)
        prm = prm_of(p)
        for b, r in enumerate(rows):
            k_all = len(r)
            edges = sorted({0, 1, HOP - 1, HOP + 1, N_FFT + 1, k_all // 2 + 1, k_all - 1, k_all})
            for begin, end in zip(edges[:-1], edges[1:]):
                o, w_end, last = window_of(k_all, begin, end, R)
                xin = np.ascontiguousarray(r[o:w_end])
                k, cnt = len(xin), end - begin
                assert supported(R, o, k, begin, cnt, last)
                out = np.full((2, k + 5), SENTINEL32, np.uint32)
                assert raw(ctx, xin, np.array([k], np.int32), k, prm, out, k + 5, win=(o, begin, cnt, last)) == 0, (b, begin, end, err(ctx))
                assert np.array_equal(out[0, :cnt], want[b, begin:end].view(np.uint32)), (p, b, begin, end)
                assert np.all(out[0, cnt:] == SENTINEL32) and np.all(out[1] == SENTINEL32)
    # an origin beyond 2^32: the block index comes from the absolute frame index, in 64 bits.  far is a whole number of pattern periods.
    far = HOP * 2 ** 24
    assert far == 2 ** 32 and (far // HOP) % (4 * DEFAULT["block_frames"] * DEFAULT["period_blocks"]) == 0
    r = rows_of((4001,))[0]
    o, begin, cnt = 301, 301 + R, 700
    xin = np.ascontiguousarray(r[o:begin + cnt + R])
    k = len(xin)
    near, farr = np.full((1, k), SENTINEL32, np.uint32), np.full((1, k), SENTINEL32, np.uint32)
    for p in (SMALL, DEFAULT):
        prm = prm_of(p)
        assert raw(ctx, xin, np.array([k], np.int32), k, prm, near, k, win=(o, begin, cnt, 0)) == 0, err(ctx)
        assert raw(ctx, xin, np.array([k], np.int32), k, prm, farr, k, win=(o + far, begin + far, cnt, 0)) == 0, err(ctx)
        assert np.array_equal(near, farr) and not np.any(near[0, :cnt] == SENTINEL32)
    one_block = DEFAULT["block_frames"] * HOP                # the same slots (a multiple of 4 frames), the next row of the pattern
    assert raw(ctx, xin, np.array([k], np.int32), k, prm, farr, k, win=(o + far + one_block, begin + far + one_block, cnt, 0)) == 0, err(ctx)
    assert not np.array_equal(near[0, :cnt], farr[0, :cnt])
    # the support condition, with the row named
    out = np.zeros((1, k), np.float32)
    assert raw(ctx, xin, np.array([k], np.int32), k, prm, out, k, win=(o, begin - 1, cnt, 0)) == INV and b"row 0" in err(ctx) and b"in front" in err(ctx)
    assert raw(ctx, xin, np.array([k], np.int32), k, prm, out, k, win=(o, begin, cnt + 1, 0)) == INV and b"row 0" in err(ctx) and b"behind" in err(ctx)
    assert raw(ctx, xin, np.array([k], np.int32), k, prm, out, k, win=(o, begin, cnt, 0)) == 0


def test_errors_leave_the_context_usable():
    ctx = ctx_for()
    rows = rows_of(BATCHES[0])
    x, n = padded(rows)
    Nmax = x.shape[1]
    want = run(ctx, x, n, SMALL)
    out = np.zeros((3, Nmax), np.float32)

    def bad(**kw):
        f = {**SMALL, **{k: v for k, v in kw.items() if k != "reserved"}}
        prm = prm_of(f)
        prm.reserved = kw.get("reserved", 0)
        return raw(ctx, x, n, Nmax, prm, out, Nmax)

    for kw in (dict(depth_db=-0.1), dict(depth_db=6.5), dict(depth_db=float("nan")), dict(lo_hz=-1.0), dict(lo_hz=8000.0), dict(hi_hz=float("inf")),
               dict(block_frames=0), dict(band_bins=0), dict(period_blocks=0), dict(period_blocks=257), dict(reserved=1),
               dict(lo_hz=1000.0, hi_hz=1100.0)):               # (the last: J = 2 bands)
        assert bad(**kw) == INV, (kw, err(ctx))
    assert bad(band_bins=1, lo_hz=0.0, hi_hz=11025.0) == 0      # J = 512
    short = np.array([n[0], 300, n[2]], np.int32)
    assert raw(ctx, x, short, Nmax, prm_of(SMALL), out, Nmax) == INV and b"row 1" in err(ctx)
    assert raw(ctx, x, n, Nmax, None, out, Nmax) == INV and raw(ctx, x, n, Nmax, prm_of(SMALL), None, Nmax) == INV
    assert raw(ctx, x, n, Nmax, prm_of(SMALL), out, Nmax - 1) == INV and raw(ctx, x, n, Nmax, prm_of(SMALL), out, Nmax, flags=64) == INV
    sc, of, wi = np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    lib, h = ctx._lib, ctx._h
    det = lambda wf=0, s=sc, ws=None, wo=None, nw=0, flags=0, prm=prm_of(SMALL): lib.zvx_watermark_detect(  # noqa: E731
        h, vp(x), vp(n), 3, Nmax, C.byref(prm), wf, vp(s), vp(of), vp(wi), vp(ws), vp(wo), nw, flags)
    assert det() == 0, err(ctx)
    assert det(wf=1) == INV and det(wf=-1) == INV and det(s=None) == INV and det(flags=_lib.ZVX_PCM16) == INV
    assert det(ws=np.zeros((3, 4), np.float32)) == INV
    assert det(wf=2, ws=np.zeros((3, 1), np.float32), wo=np.zeros((3, 1), np.int32), nw=1) == BUF
    assert det(prm=prm_of({**SMALL, "period_blocks": 300})) == INV
    out[:] = 0
    assert raw(ctx, x, n, Nmax, prm_of(SMALL), out, Nmax) == 0 and all(same_bits(out[b, :n[b]], want[b, :n[b]]) for b in range(3))


# ---- the detector ---------------------------------------------------------------------------------------------------------------------------
def voiced(seconds, seed):
    key = ("voiced", seconds, seed)
    if key not in _sig:
        _sig[key] = W.voiced_signal(seconds, seed)
        _sig[key].setflags(write=False)
    return _sig[key]


def test_detector_scores_against_the_reference():
    """scores within LIMIT_DETECT; offsets and windows equal wherever the reference's best score leads its runner-up outside +-1 frame by
    more than that bound"""
    ctx = ctx_for()
    worst = 0.0
    cases = []
    small_rows = rows_of(BATCHES[1])
    marked_small = run(ctx, *padded(small_rows), SMALL)
    cases.append(("small", SMALL, [marked_small[b, :len(r)] for b, r in enumerate(small_rows)], 0))
    cases.append(("small windows", SMALL, [marked_small[b, :len(r)] for b, r in enumerate(small_rows)], 4))
    y = ctx.watermark([voiced(1.5, 11)], KEY)[0]
    cases.append(("default", DEFAULT, [y, y[5000:], voiced(1.5, 11)], 0))
    cases.append(("default windows", DEFAULT, [y, y[5000:]], 64))
    # the case's own bound: rule (c) of spectral_ref on rows marked by the float64 reference (the short rows of the batch; one voiced
    # row of 1.5 s per seed), under today's constant as a cap
    geo = (N_FFT, HOP, N_FFT)
    mark = lambda r, p: W.embed(r, KEY, n_fft=N_FFT, hop=HOP, win_length=N_FFT, rate=RATE, **p).astype(np.float32)      # noqa: E731
    mg_small = S.detect_margin_of(lambda s: [mark(r, SMALL) for r in rows_of(BATCHES[1], s)], SMALL, *geo, (0, 4), RATE, KEY)
    mg_default = S.detect_margin_of(lambda s: [mark(W.voiced_signal(1.5, 11 + 100 * s), DEFAULT)], DEFAULT, *geo, (0, 64), RATE, KEY)
    print(mg_small.line("detect small") + "\n" + mg_default.line("detect default"))
    for name, p, rows, wf in cases:
        limit = min(LIMIT_DETECT, (mg_small if p is SMALL else mg_default).max_limit)
        kw = {k: v for k, v in p.items() if k != "depth_db"}
        got = ctx.watermark_detect(rows, KEY, window_frames=wf, **kw)
        for b, r in enumerate(rows):
            score, off, win, zs = W.detect(r, KEY, window_frames=wf, n_fft=N_FFT, hop=HOP, win_length=N_FFT, rate=RATE, full=True, **kw)
            assert len(got[b].windows) == len(zs), (name, b)
            for w, z in enumerate(zs):
                e = abs(got[b].windows[w][0] - float(z.max()))
                worst = max(worst, e)
                o = int(np.argmax(z))
                T = len(z)
                away = np.array([min((q - o) % T, (o - q) % T) > 1 for q in range(T)])
                lead = float(z[o] - z[away].max()) if away.any() else np.inf
                print(f"{name} row {b} window {w}: score {got[b].windows[w][0]:.5f} ref {z[o]:.5f} |diff| {e:.2e}; offset {got[b].windows[w][1]} ref {o} (lead {lead:.3f})")
                assert e <= limit, (name, b, w, e)
                if lead > limit:
                    assert min((got[b].windows[w][1] - o) % T, (o - got[b].windows[w][1]) % T) <= 1, (name, b, w)
                    if np.sum(z >= z[o] - limit) == 1:
                        assert got[b].windows[w][1] == o, (name, b, w)
            assert abs(got[b].score - score) <= limit
            runner = sorted(float(z.max()) for z in zs)
            if len(runner) < 2 or runner[-1] - runner[-2] > limit:
                assert got[b].window == win, (name, b)
    print(f"detector: worst |score - ref| {worst:.3e} against the limits {min(LIMIT_DETECT, mg_small.max_limit):.3e} (small) and {min(LIMIT_DETECT, mg_default.max_limit):.3e} (default)")
    empty = ctx.watermark_detect(np.zeros((2, 4000), np.float32), KEY, lengths=[0, 4000])
    assert empty[0].score == 0.0 and empty[0].offset == 0 and empty[0].windows == [] and empty[1].score == 0.0     # no samples; silence: 0 / 0


def test_detection_end_to_end_on_the_device():
    """the right-key / wrong-key / cut / joined cases of tests/test_watermark.py on 1.5 s rows, embedded and detected on the device"""
    ctx = ctx_for()
    a, b = voiced(1.5, 11), voiced(1.5, 12)
    ya, yb = ctx.watermark([a], KEY)[0], ctx.watermark([b], KEY)[0]
    thr = WM.THRESHOLD
    right, cut_, plain = ctx.watermark_detect([ya, ya[5000:], a], KEY)
    print(f"right key {right.score:.2f} offset {right.offset}; cut {cut_.score:.2f} offset {cut_.offset}; unmarked {plain.score:.2f}")
    assert right.detected and right.score >= thr and right.offset == 0
    assert cut_.detected and cut_.offset in (19, 20)         # 5000 / 256 = 19.5 frames
    assert not plain.detected and plain.score < thr
    wrong = [ctx.watermark_detect([ya], KEY ^ (1 << k))[0].score for k in range(8)]
    print(f"wrong keys: largest {max(wrong):.2f}")
    assert max(wrong) < thr
    joined = np.concatenate([ya[3000:], np.zeros(2000, np.float32), yb[7001:]])
    res = ctx.watermark_detect([joined], KEY, window_frames=128)[0]
    T = DEFAULT["block_frames"] * DEFAULT["period_blocks"]
    want = [3000 / HOP, (7001 - (len(ya) - 3000 + 2000)) / HOP]              # the cut of each sentence, in frames
    hits = [(w, s, o) for w, (s, o) in enumerate(res.windows) if s >= thr]
    print(f"joined: windows {[(w, round(s, 2), o) for w, s, o in hits]} of {len(res.windows)}; cuts {want}")
    near = lambda o, c: min((o - c) % T, (c - o) % T) <= 1.0                  # noqa: E731
    assert res.detected and all(any(near(o, c) for _, _, o in hits) for c in want)


# ---- the keyword of ZeroVoxTTS ----------------------------------------------------------------------------------------------------------------
TEXT = "The quick brown fox jumps over the lazy dog, and then it runs back home again before the night falls"


def test_tts_tts_long_and_tts_stream_keyword():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    try:
        ctx = synth.model.ctx
        spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
        plain = synth.tts(TEXT, spk)[0]
        assert same_bits(synth.tts(TEXT, spk, watermark=None)[0], plain)                  # None changes nothing, bit for bit
        marked = synth.tts(TEXT, spk, watermark=KEY)[0]
        assert same_bits(marked, ctx.watermark([plain], KEY)[0]) and not same_bits(marked, plain)
        print(f"tts: {len(plain)} samples ({len(plain) // HOP} frames), peak {np.abs(plain).max():.3f}, rms {np.sqrt(np.mean(plain ** 2)):.4f}")
        res, none, other = synth.detect_watermark(marked, KEY), synth.detect_watermark(plain, KEY), synth.detect_watermark(marked, KEY + 1)
        print(f"tts: marked {res.score:.2f} (offset {res.offset}), unmarked {none.score:.2f}, wrong key {other.score:.2f}; threshold {res.threshold}")
        assert res.detected and res.offset == 0 and not none.detected and not other.detected
        # behind the denoiser, before the gain and the limiter
        chain = synth.tts(TEXT, spk, watermark=KEY, denoise=0.5, loudness=-20.0, limiter=True)[0]
        assert synth.detect_watermark(chain, KEY).detected and not same_bits(chain, marked)
        # at another rate: converted to the model's first, hi_hz lowered to what survived
        synth.output_rate = 16000
        try:
            low = synth.tts(TEXT, spk, watermark=KEY)[0]
            r16 = synth.detect_watermark(low, KEY, sampling_rate=16000)
            print(f"tts at 16 kHz: {r16.score:.2f} (offset {r16.offset})")
            assert r16.detected and r16.offset in (0, 1, 511)
        finally:
            synth.output_rate = None
        # tts_long: ONE call over all sentence rows; every sentence carries the mark from its own first frame
        two = TEXT + ". " + TEXT + "."
        wav0, seg0 = synth.tts_long(two, spk, trim_db=0)
        wav1, seg1 = synth.tts_long(two, spk, trim_db=0, watermark=KEY)
        assert len(wav1) == len(wav0) and [s["start"] for s in seg1] == [s["start"] for s in seg0] and not same_bits(wav1, wav0)
        assert same_bits(synth.tts_long(two, spk, trim_db=0, watermark=None)[0], wav0)
        long_res = synth.detect_watermark(wav1, KEY)
        print(f"tts_long: {long_res.score:.2f} over {len(long_res.windows)} windows: {[(round(s, 2), o) for s, o in long_res.windows]}")
        assert long_res.detected and not synth.detect_watermark(wav0, KEY).detected
        # tts_stream: the pieces concatenate to zvx_watermark of the unwatermarked stream, n_fft - 1 samples behind it
        plain_pieces = list(synth.tts_stream(TEXT, spk, chunk_frames=16))
        stream = np.concatenate(plain_pieces)
        pieces = list(synth.tts_stream(TEXT, spk, chunk_frames=16, watermark=KEY))
        got = np.concatenate(pieces)
        assert len(pieces) >= 2 and same_bits(got, ctx.watermark([stream], KEY)[0]) and not same_bits(got, stream)
        R = WM.reach(N_FFT)
        received, emitted = np.cumsum([len(p) for p in plain_pieces]), np.cumsum([len(p) for p in pieces])
        assert all(emitted[j] == max(0, received[j] - R) for j in range(len(plain_pieces))) and emitted[-1] == received[-1]
        # the chain: denoise, watermark, limit
        both = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, watermark=KEY, denoise_strength=0.5, peak_db=-20.0)))
        want = ctx.limit([ctx.watermark([ctx.denoise([stream], synth.denoise_bias, 0.5)[0]], KEY)[0]], 10 ** (-20 / 20), 5.0, 4)[0][0]
        assert same_bits(both, want)
        assert same_bits(np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16))), stream)       # the plain stream is as it was
        with pytest.raises(ValueError, match="no watermark stage yet"):
            synth.tts_stream(TEXT, spk, watermark=KEY, resident=True)
    finally:
        synth.model.close()
