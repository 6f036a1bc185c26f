"""Sample-rate conversion on the MI355X: zvx_resample / zvx_resample_ex, the "out_rate" switch through the waveform calls, the
streaming path and reference audio.  The reference is tests/resample_ref.py (float64) on the same f32 input, never the library;
the bound per float sample is (T + 2) 2^-24 A[n] (resample_ref.bound), nothing is tuned on the GPU."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resample_ref as R
from stream_util import _ragged_case
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

PAIRS = [(22050, 48000), (22050, 44100), (22050, 24000), (22050, 16000), (22050, 8000),
         (16000, 22050), (24000, 22050), (44100, 22050), (48000, 22050), (22050, 32000), (32000, 22050)]
LENGTHS = [1, 300, 4097, 22050, 66151]
SQUARE_ROW = 3
SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
_ctx = {}


def ctx_for(voc, prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def rows_for(rate_in, seed=3):
    rng = np.random.default_rng(seed)
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for n in LENGTHS]
    t = np.arange(LENGTHS[SQUARE_ROW]) / float(rate_in)
    rows[SQUARE_ROW] = np.where(np.sin(2 * np.pi * 300.0 * t) >= 0, 1.0, -1.0).astype(np.float32)     # full-scale 300 Hz square wave
    return rows


def padded(rows):
    n = np.array([len(r) for r in rows], np.int32)
    x = np.zeros((len(rows), int(n.max())), np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def check_float(got, x, rate_in, rate_out, what):
    ref, A = R.resample_ref(x, rate_in, rate_out, want_mag=True)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, lim = np.abs(got.astype(np.float64) - ref), R.bound(rate_in, rate_out, A)
    frac = float((err / np.maximum(lim, 1e-300)).max()) if len(err) else 0.0
    print(f"{what}: {rate_in} -> {rate_out}, {len(ref)} samples, max |err| {err.max() if len(err) else 0:.3e}, worst fraction of the bound {frac:.3f}")
    assert np.all(err <= lim), (what, frac)
    return ref


def raw_resample(ctx, x, n, rate_in, rate_out, out, stride, flags=0, out_len=None, ex=None):
    """the C call itself: x / out are ndarrays (host) or integer device pointers"""
    p = lambda a: C.c_void_p(int(a)) if isinstance(a, (int, np.integer)) else a.ctypes.data_as(C.c_void_p)
    B = len(n)
    Nmax = x.shape[1] if hasattr(x, "shape") else int(max(n.max(), 1))
    args = [ctx._h, p(x), p(n), B, Nmax, rate_in, rate_out, p(out), stride, None if out_len is None else p(out_len), flags]
    if ex is None:
        return ctx._lib.zvx_resample(*args)
    return ctx._lib.zvx_resample_ex(*args, *ex)


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_resample_ragged_batch_host_device_and_pcm16(rate_in, rate_out):
    ctx = ctx_for("tiny")
    rows = rows_for(rate_in)
    x, n = padded(rows)
    B = len(rows)
    want_len = np.array([_lib.resampled_len(v, rate_in, rate_out) for v in n], np.int32)
    nmax = int(want_len.max())
    stride = nmax + 37
    # host rows
    out = np.full((B, stride), SENTINEL32, np.uint32).view(np.float32)
    out_len = np.zeros(B, np.int32)
    assert raw_resample(ctx, x, n, rate_in, rate_out, out, stride, 0, out_len) == 0, ctx._lib.zvx_last_error(ctx._h)
    assert np.array_equal(out_len, want_len)
    refs = []
    for b in range(B):
        refs.append(check_float(out[b, :want_len[b]], rows[b], rate_in, rate_out, f"row {b}"))
        assert np.all(out[b, want_len[b]:nmax].view(np.uint32) == 0), f"row {b}: tail not zero"
        assert np.all(out[b, nmax:].view(np.uint32) == SENTINEL32), f"row {b}: written past the longest row"
    # device in, device out
    xin, dout = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(B * stride * 4)
    try:
        ctx.dev_from_host(xin, x)
        ctx.dev_from_host(dout, np.full((B, stride), SENTINEL32, np.uint32))
        assert raw_resample(ctx, xin, n, rate_in, rate_out, dout, stride, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT, None) == 0
        dev = ctx.dev_to_host(dout, (B, stride), np.float32)
        assert np.array_equal(dev.view(np.uint32), out.view(np.uint32)), "device rows differ from host rows"
    finally:
        ctx.dev_free(xin); ctx.dev_free(dout)
    # int16: bit-equal to the conversion of the float rows of the same call, within 1 LSB of the conversion of the reference
    pcm = np.full((B, stride), SENTINEL16, np.int16)
    assert raw_resample(ctx, x, n, rate_in, rate_out, pcm, stride, _lib.ZVX_PCM16, out_len) == 0
    assert np.array_equal(out_len, want_len)
    for b in range(B):
        assert np.array_equal(pcm[b, :want_len[b]], R.pcm16(out[b, :want_len[b]])), f"row {b}"
        want = np.trunc(np.clip(refs[b] * 32760.0, -32768, 32767))
        assert np.abs(pcm[b, :want_len[b]].astype(np.float64) - want).max() <= 1, f"row {b}"
        assert np.all(pcm[b, want_len[b]:nmax] == 0) and np.all(pcm[b, nmax:] == SENTINEL16), f"row {b}"
    if (rate_in, rate_out) == (22050, 48000):
        assert refs[SQUARE_ROW].max() > 1.0 and refs[SQUARE_ROW].min() < -1.0         # the interpolated square wave overshoots full scale ...
        sq = pcm[SQUARE_ROW, :want_len[SQUARE_ROW]]
        assert (sq == 32767).sum() > 0 and (sq == -32768).sum() > 0                    # ... and the int16 rows saturate instead of wrapping


@pytest.mark.parametrize("rate_in,rate_out", [(22050, 48000), (22050, 8000), (48000, 22050)])
def test_a_row_does_not_depend_on_its_batch(rate_in, rate_out):
    ctx = ctx_for("tiny")
    rows = rows_for(rate_in, seed=8)
    out, out_len = ctx.resample(rows, rate_in, rate_out)
    for b, r in enumerate(rows):
        one, l1 = ctx.resample([r], rate_in, rate_out)
        assert l1[0] == out_len[b]
        assert np.array_equal(one[0].view(np.uint32), out[b, :out_len[b]].view(np.uint32)), b
    x, n = padded(rows)
    out2, _ = ctx.resample(x, rate_in, rate_out, lengths=n)                           # the padded-array form
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))
    same, ls = ctx.resample(rows, rate_in, rate_in)                                    # equal rates: a copy
    assert np.array_equal(ls, n) and np.array_equal(same.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("rate_in,rate_out", [(22050, 48000), (22050, 8000)])
def test_windows_concatenate_to_the_one_call_result(rate_in, rate_out):
    from zerovox_amd.resample import rate_pair
    ctx = ctx_for("tiny")
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, 3 * rate_in).astype(np.float32)
    whole, wl = ctx.resample([x], rate_in, rate_out)
    whole = whole[0, :wl[0]]
    L, M, half = rate_pair(rate_in, rate_out)
    W = len(whole)
    cuts = [0, 1, 777, W // 3, W // 3 + 1, (5 * W) // 7, W - 5, W]                      # output positions, arbitrary
    got = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        k_lo = max(0, -(-(lo * M - half) // L))                                       # the samples under the filter of outputs [lo, hi)
        k_hi = min(len(x), ((hi - 1) * M + half) // L + 1)
        piece, _ = ctx.resample_window([x[k_lo:k_hi]], rate_in, rate_out, in_origin=k_lo, out_begin=lo, out_count=hi - lo)
        assert piece.shape == (1, hi - lo)
        got.append(piece[0])
    got = np.concatenate(got)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    k_need = -(-(cuts[4] * M - half) // L)
    assert k_need > 3
    tail, tl = ctx.resample_window([x[k_need - 3:]], rate_in, rate_out, in_origin=k_need - 3, out_begin=cuts[4], out_count=-1)      # "to the end"
    assert tl[0] == len(whole) - cuts[4]
    assert np.array_equal(tail[0].view(np.uint32), whole[cuts[4]:].view(np.uint32))


def test_a_row_that_emits_nothing_next_to_one_that_does():
    """zvx_resample_ex, one window for two rows of 40 and 2000 samples, outputs from 100 on: row 0 has only 15 outputs at 8 kHz and emits
    nothing, yet it is zero-filled up to row 1's count and its 40 input samples count as read, as for every row of a call that writes."""
    ctx = ctx_for("tiny")
    rate_in, rate_out, begin = 22050, 8000, 100
    rng = np.random.default_rng(21)
    rows = [rng.uniform(-1, 1, k).astype(np.float32) for k in (40, 2000)]
    x, n = padded(rows)
    full = [_lib.resampled_len(int(v), rate_in, rate_out) for v in n]
    assert full[0] == 15 and full[0] < begin < full[1]
    want_len = np.array([0, full[1] - begin], np.int32)
    nmax = int(want_len[1])
    stride = nmax + 37
    out_len = np.full(2, -1, np.int32)
    dout = ctx.dev_alloc(2 * stride * 4)
    try:
        ctx.dev_from_host(dout, np.full((2, stride), SENTINEL32, np.uint32))
        ctx.set_int("profile", 2)
        try:
            ctx.reset_stats()
            assert raw_resample(ctx, x, n, rate_in, rate_out, dout, stride, _lib.ZVX_DEVICE_OUT, out_len, ex=(0, begin, -1)) == 0, ctx._lib.zvx_last_error(ctx._h)
            tags = {t["name"]: t for t in ctx.tag_stats()}
        finally:
            ctx.set_int("profile", 0)
        got = ctx.dev_to_host(dout, (2, stride), np.uint32)
    finally:
        ctx.dev_free(dout)
    assert np.array_equal(out_len, want_len)
    assert np.all(got[0, :nmax] == 0), "row 0: not zero up to the longest row's count"
    assert np.all(got[:, nmax:] == SENTINEL32), "written past the longest row's count"
    alone, l1 = ctx.resample_window([rows[1]], rate_in, rate_out, in_origin=0, out_begin=begin, out_count=-1)
    assert l1[0] == want_len[1] and np.array_equal(got[1, :nmax], alone[0].view(np.uint32))
    assert [t for t in tags if t != "voc.resample" and tags[t]["launches"]] == [] and tags["voc.resample"]["launches"] == 1, tags
    assert tags["voc.resample"]["bytes"] == 4.0 * (40 + 2000) + 4.0 * int(want_len[1]), tags["voc.resample"]


def test_errors_leave_the_context_usable():
    ctx = ctx_for("tiny")
    x = np.zeros((1, 100), np.float32); n = np.array([100], np.int32)
    out = np.zeros((1, 400), np.float32)
    for bad in (0, 3999, 192001):
        assert raw_resample(ctx, x, n, bad, 22050, out, 400) == _lib.ZVX_E_INVALID
        assert raw_resample(ctx, x, n, 22050, bad, out, 400) == _lib.ZVX_E_INVALID
    assert raw_resample(ctx, x, n, 22050, 22051, out, 400) == _lib.ZVX_E_UNSUPPORTED
    msg = ctx._lib.zvx_last_error(ctx._h).decode()
    assert "22051" in msg and "22050" in msg and "L" in msg and "M" in msg, msg
    need = _lib.resampled_len(100, 22050, 48000)
    assert raw_resample(ctx, x, n, 22050, 48000, out, need - 1) == _lib.ZVX_E_BUFFER
    assert raw_resample(ctx, x, n, 22050, 48000, out, need) == 0
    assert raw_resample(ctx, x, np.array([101], np.int32), 22050, 48000, out, 400) == _lib.ZVX_E_INVALID
    for fl in (_lib.ZVX_NO_SYNC, 64):                         # ZVX_NO_SYNC without ZVX_DEVICE_OUT; a flag the call does not know
        assert raw_resample(ctx, x, n, 22050, 48000, out, 400, fl) == _lib.ZVX_E_INVALID, fl
        assert b"zvx_resample" in ctx._lib.zvx_last_error(ctx._h), fl
    assert ctx.get_int("out_rate") == 0
    ctx.set_int("out_rate", 16000)
    try:
        for bad, code in ((22051, _lib.ZVX_E_UNSUPPORTED), (3999, _lib.ZVX_E_INVALID), (192001, _lib.ZVX_E_INVALID), (-1, _lib.ZVX_E_INVALID)):
            with pytest.raises(_lib.ZvxError) as e:
                ctx.set_int("out_rate", bad)
            assert e.value.code == code and ctx.get_int("out_rate") == 16000
    finally:
        ctx.set_int("out_rate", 0)
    assert ctx.get_int("out_rate") == 0
    got, _ = ctx.resample([np.ones(50, np.float32)], 22050, 48000)
    check_float(got[0], np.ones(50, np.float32), 22050, 48000, "after the errors")


@pytest.mark.parametrize("voc", ["tiny", "v1"])
def test_output_rate_through_the_waveform_calls(voc):
    ctx = ctx_for(voc)
    hop, native = ctx.hop, ctx.get_int("sampling_rate")
    case = _ragged_case(3, 20, 41)
    ctx.set_int("out_rate", 0)
    first = ctx.synthesize(*case, None, want_mel=False)
    ml = first["mel_len"]
    assert len(set(int(v) for v in ml)) == 3                                          # a ragged batch
    nat = [first["wav"][b, :int(ml[b]) * hop] for b in range(3)]
    try:
        for rate in (48000, 8000):
            ctx.set_int("out_rate", rate)
            assert ctx.get_int("out_rate") == rate
            lens = [_lib.resampled_len(int(ml[b]) * hop, native, rate) for b in range(3)]
            nmax = max(lens)
            r = ctx.synthesize(*case, None, want_mel=False)
            assert np.array_equal(r["mel_len"], ml) and r["wav"].shape == (3, nmax)
            for b in range(3):
                check_float(r["wav"][b, :lens[b]], nat[b], native, rate, f"{voc} utterance {b}")
                assert np.all(r["wav"][b, lens[b]:].view(np.uint32) == 0)
            # int16
            p = ctx.synthesize(*case, None, want_mel=False, pcm16=True)
            assert p["wav"].dtype == np.int16 and p["wav"].shape == (3, nmax)
            assert np.array_equal(p["wav"], R.pcm16(r["wav"]))
            # a short stride is refused, in output samples
            wbad = np.zeros((3, nmax - 1), np.float32)
            rc = ctx._lib.zvx_vocode(ctx._h, None, wbad.ctypes.data_as(C.c_void_p), nmax - 1, 0)
            assert rc == _lib.ZVX_E_BUFFER
            # queued, device rows
            stride = nmax + 11
            dptr = ctx.dev_alloc(3 * stride * 4)
            try:
                ctx.dev_from_host(dptr, np.full((3, stride), SENTINEL32, np.uint32))
                ctx.synthesize(*case, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True)
                ctx.sync()
                d = ctx.dev_to_host(dptr, (3, stride), np.float32)
                assert np.array_equal(d[:, :nmax].view(np.uint32), r["wav"].view(np.uint32))
                assert np.all(d[:, nmax:].view(np.uint32) == SENTINEL32)
            finally:
                ctx.dev_free(dptr)
            # asynchronous host delivery: `valid` in output samples
            for pcm in (False, True):
                a = ctx.synthesize(*case, None, want_mel=False, host_async=True, pcm16=pcm)
                got = ctx.wait_host(a["slot"], pcm16=pcm)
                assert got.shape == (3, nmax)
                assert np.array_equal(got, p["wav"] if pcm else r["wav"])
            # the staged calls and the per-call opt-out
            v = ctx.vocode(3, ml)
            assert v.shape == (3, nmax) and np.array_equal(v.view(np.uint32), r["wav"].view(np.uint32))
            vn = ctx.vocode(3, ml, native_rate=True)
            assert np.array_equal(vn.view(np.uint32), first["wav"].view(np.uint32))
            # accounting: one launch under its own tag, with its algorithmic bytes; Context.stage_times() keeps its six names
            ctx.set_int("profile", 2); ctx.reset_stats()
            ctx.synthesize(*case, None, want_mel=False)
            tags = {t["name"]: t for t in ctx.tag_stats()}
            assert tags["voc.resample"]["launches"] == 1
            assert tags["voc.resample"]["bytes"] == 4.0 * sum(int(m) * hop for m in ml) + 4.0 * sum(lens)
            assert ctx.resample_ms() > 0 and set(ctx.stage_times()) == set(_lib.STAGES)
            ctx.set_int("profile", 0)
        # back to the model's rate: the rows of the first run bit for bit, and no resample launch
        ctx.set_int("out_rate", 0)
        ctx.set_int("profile", 2); ctx.reset_stats()
        again = ctx.synthesize(*case, None, want_mel=False)
        assert np.array_equal(again["wav"].view(np.uint32), first["wav"].view(np.uint32))
        assert "voc.resample" not in {t["name"] for t in ctx.tag_stats()} and ctx.resample_ms() == 0.0
        ctx.set_int("out_rate", native)                                               # the model's own rate spelled out: the same
        same = ctx.synthesize(*case, None, want_mel=False)
        assert np.array_equal(same["wav"].view(np.uint32), first["wav"].view(np.uint32))
        assert "voc.resample" not in {t["name"] for t in ctx.tag_stats()}
    finally:
        ctx.set_int("profile", 0); ctx.set_int("out_rate", 0)


def test_streams_under_an_output_rate_equal_the_whole_conversion():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    ctx = ctx_for("v1")
    zv = ZeroVox.__new__(ZeroVox)
    zv._ctx, zv._hop_length = ctx, 256
    mel = np.random.default_rng(21).standard_normal((150, 80)).astype(np.float32)
    ctx.set_int("out_rate", 0)
    native = np.concatenate(list(zv.vocode_stream(mel, chunk_frames=40)))
    want, wl = ctx.resample([native], 22050, 16000)
    try:
        ctx.set_int("out_rate", 16000)
        for cf, cpc in ((40, 1), (7, 3), (1, 8)):
            parts = list(zv.vocode_stream(mel, chunk_frames=cf, chunks_per_call=cpc))
            got = np.concatenate(parts)
            assert len(got) == wl[0] == _lib.resampled_len(150 * 256, 22050, 16000)
            if cf == 40:
                assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
            else:                                                                     # other chunk sizes change the native stream only to f32/bf16 halo equality, see the streaming test
                nat2 = np.concatenate(list(zv._vocode_stream_native(mel, cf, zv.STREAM_HALO, cpc, True)))
                w2, _ = ctx.resample([nat2], 22050, 16000)
                assert np.array_equal(got.view(np.uint32), w2[0].view(np.uint32))
    finally:
        ctx.set_int("out_rate", 0)
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    text = "hello world, this is a test."
    nat = np.concatenate(list(synth.tts_stream(text, spk, chunk_frames=16)))
    assert synth.output_rate == 22050
    synth.output_rate = 16000
    assert synth.output_rate == 16000 and synth.model.ctx.get_int("out_rate") == 16000
    got = np.concatenate(list(synth.tts_stream(text, spk, chunk_frames=16)))
    want, wl = synth.model.ctx.resample([nat], 22050, 16000)
    assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    wav, _, length = synth.tts(text, spk)
    assert len(wav) == _lib.resampled_len(length * 256, 22050, 16000)
    synth.output_rate = 22050
    assert synth.model.ctx.get_int("out_rate") == 0
    wav_n, _, length_n = synth.tts(text, spk)
    assert length_n == length and len(wav_n) == length * 256
    synth.model.close()


def test_reference_audio_at_another_rate(tmp_path):
    from zerovox_amd.synthesize import ZeroVoxTTS
    pytest.importorskip("scipy")
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="f32")
    ctx = synth.model.ctx
    rng = np.random.default_rng(17)
    sr = 16000
    n = sr * 2
    t = np.arange(n) / float(sr)
    voiced = (0.25 * np.sin(2 * np.pi * 140 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(n)).astype(np.float32)
    x16k = np.concatenate([np.zeros(4350, np.float32), voiced, 1e-4 * rng.standard_normal(6530).astype(np.float32)])
    res, rl = ctx.resample([x16k], sr, 22050)
    check_float(res[0, :rl[0]], x16k, sr, 22050, "reference audio")
    e1 = synth.speaker_embed(x16k, sampling_rate=sr)
    e2 = synth.speaker_embed(res[0, :rl[0]])
    assert e1.shape == (1, 1, 528) and np.abs(e1 - e2).max() <= 5e-5
    path = os.path.join(tmp_path, "ref16k.wav")
    pcm = (x16k * 32760).astype(np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(pcm.tobytes())
    host = ZeroVoxTTS.get_speakerref(path, 22050)                                     # scipy on the host: the path that exists today
    dev = synth.speakerref_samples(path)
    assert dev.shape == host.shape and dev.dtype == np.float32
    xin = pcm.astype(np.float32) / 32768.0
    ref, A = R.resample_ref(xin, sr, 22050, want_mag=True)
    lim = R.bound(sr, 22050, A) + 2.0 ** -24 * np.abs(ref)                             # + the host path's own rounding to f32
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    print(f"device vs scipy host path: max |err| {err.max():.3e}, worst fraction of the bound {(err / np.maximum(lim, 1e-300)).max():.3f}")
    assert np.all(err <= lim)
    ef = synth.speaker_embed_file(path)
    assert np.abs(ef - synth.speaker_embed(host)).max() <= 5e-5
    synth.model.close()
