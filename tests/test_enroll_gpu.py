"""Speaker enrolment on the MI355X: zvx_spkemb_wav against the chain of calls include/zvx.h defines it by (bit for bit) and against the
float reference of tests/enroll_ref.py (never the library), its placement and error behaviour, a device-resident embedding into
zvx_synthesize (ZVX_DEVICE_SPK), and ZeroVoxTTS.speaker_embed_batch.  Every test first asserts, from the reference alone, that no clip has
a frame inside the ambiguity band of the trim threshold."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import enroll_ref as E
import join_ref as J
from stream_util import vp
from zerovox_amd import _lib, config as zcfg, pack, synthetic, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
NATIVE, N_FFT, HOP = 22050, 1024, 256
MIN_WINDOW = 2 * HOP                                      # fewer samples give fewer than the 2 frames zvx_spkemb needs
# (frame, hop, top_db, keep): begin = first * hop - keep lands on every residue mod 4; the last row is trimming off
GRID = [(2048, 512, 40.0, 0), (2048, 512, 40.0, 441), (1024, 256, 25.0, 1002), (400, 160, 60.0, 3), (2048, 512, 0.0, 0)]
_ctx, _sd, _oracle = {}, {}, {}


def model_sd():
    if not _sd:
        cfg = zcfg.medium_modelcfg("styletts")
        _sd["v"] = (cfg, zw.tts_state_dict(cfg, 0))
    return _sd["v"]


def ctx_for(voc, prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg, sd = model_sd()
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, sd, h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def padded(rows, odd=False):
    n = np.array([len(r) for r in rows], np.int32)
    nmax = max(int(n.max()), 1)
    x = np.zeros((len(rows), nmax + (odd and nmax % 2 == 0)), np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def params(frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0):
    return _lib.RefParams(frame, hop, top_db, keep, max_samples)


def raw(ctx, x, n, Nmax, rate, prm, out, flags=0, B=None, extra=0):
    """the C call itself: x / out are ndarrays (host) or integer device pointers -> (rc, begin, end, frames), the three with `extra`
    sentinel words behind index B - 1"""
    B = len(n) if B is None else B
    begin, end, frames = (np.full(max(B, 1) + extra, -7, np.int32) for _ in range(3))
    rc = ctx._lib.zvx_spkemb_wav(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if prm is not None else None, vp(out), vp(begin), vp(end),
                                 vp(frames), flags)
    return rc, begin, end, frames


def err(ctx):
    return ctx._lib.zvx_last_error(ctx._h).decode()


def chain(ctx, rows, rate=NATIVE, frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0):
    """what include/zvx.h defines zvx_spkemb_wav by, on the same batch: zvx_resample, zvx_trim_bounds, slice (and crop), zvx_melspec,
    zvx_spkemb -> (emb, begin, end, frames)"""
    if rate != NATIVE:
        out, ol = ctx.resample(rows, rate, NATIVE)
        rows = [out[b, :int(ol[b])].copy() for b in range(len(rows))]
    begin, end = ctx.trim_bounds(rows, frame, hop, top_db, keep)
    if max_samples > 0:
        end = np.minimum(end, begin + max_samples)
    mel, frames = ctx.melspec([rows[b][int(begin[b]):int(end[b])] for b in range(len(rows))])
    return ctx.spkemb(mel, frames), begin, end, frames


def reference_bounds(rows, rate, frame, hop, top_db, keep, max_samples=0):
    """from the reference alone: the windows, after asserting that no row has a frame inside the ambiguity band"""
    want = []
    for b, x in enumerate(rows):
        begin, end, worst = E.window_ref(E.at_model_rate(x, rate), frame, hop, top_db, keep, max_samples)
        assert worst > 1e3 * J.AMBIGUOUS, (b, rate, frame, hop, top_db, worst)
        want.append((begin, end))
    return want


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_embeddings_equal_the_chain_of_calls_bit_for_bit(prec):
    ctx = ctx_for("tiny", prec)
    rows = E.make_clips(0)
    res_b, res_e = set(), set()
    for frame, hop, top_db, keep in GRID:
        want = reference_bounds(rows, NATIVE, frame, hop, top_db, keep)
        emb, begin, end, frames = ctx.spkemb_wav(rows, frame=frame, hop=hop, top_db=top_db, keep=keep)
        for b in range(len(rows)):                        # every row, none skipped
            assert (int(begin[b]), int(end[b])) == want[b], (frame, hop, top_db, keep, b, begin[b], end[b], want[b])
            assert int(frames[b]) == 1 + (want[b][1] - want[b][0] + 2 * ((N_FFT - HOP) // 2) - N_FFT) // HOP
            res_b.add(want[b][0] % 4); res_e.add(want[b][1] % 4)
        c_emb, c_begin, c_end, c_frames = chain(ctx, rows, NATIVE, frame, hop, top_db, keep)
        assert np.array_equal(c_begin, begin) and np.array_equal(c_end, end) and np.array_equal(c_frames, frames)
        assert emb.shape == (len(rows), ctx.hidden) and np.array_equal(bits(emb), bits(c_emb)), (prec, frame, hop, top_db, keep,
                                                                                                  int((bits(emb) != bits(c_emb)).sum()))
        if top_db == 0.0:
            assert not begin.any() and np.array_equal(end, [len(r) for r in rows])
    assert res_b == {0, 1, 2, 3} and res_e == {0, 1, 2, 3}    # the window cut saw every source alignment
    assert (int(begin[4]), int(end[4])) == (0, len(rows[4]))   # (the short row is whole in every case)


def oracle_embeddings():
    """the float chain of tests/enroll_ref.py for the five clips, computed once"""
    if not _oracle:
        cfg, sd = model_sd()
        _oracle["v"] = [E.embed_ref(x, NATIVE, sd, cfg) for x in E.make_clips(0)]
    return _oracle["v"]


def check_embed16(e, ref, what):
    """test_gpu_parity.py's limits for the speaker encoder in 16-bit mode: cosine >= 0.9999 with the f32 reference, max |err| <= 2.5e-3"""
    e, ref = np.asarray(e, np.float64), np.asarray(ref, np.float64)
    cos = float(np.dot(e, ref) / (np.linalg.norm(e) * np.linalg.norm(ref)))
    mx = float(np.abs(e - ref).max())
    print(f"{what}: 1 - cosine {1.0 - cos:.3e}, max err {mx:.3e}")
    assert cos >= 0.9999 and mx <= 2.5e-3, f"{what}: cosine {cos:.6f}, max err {mx:.3e}"


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_embeddings_against_the_float_reference(prec):
    """the limits test_gpu_parity.py applies to ZeroVoxTTS.speaker_embed from raw audio: 5e-5 max in f32, check_embed16 in 16-bit mode"""
    ctx = ctx_for("tiny", prec)
    rows = E.make_clips(0)
    reference_bounds(rows, NATIVE, 2048, 512, 40.0, 0)
    emb, begin, end, frames = ctx.spkemb_wav(rows)
    for b, (ref, rb, re_, rf, _) in enumerate(oracle_embeddings()):
        assert (int(begin[b]), int(end[b]), int(frames[b])) == (rb, re_, rf)
        assert abs(np.linalg.norm(emb[b]) - 1.0) < 1e-4
        if prec == "f32":
            mx = float(np.abs(emb[b].astype(np.float64) - ref).max())
            print(f"clip {b} ({rf} frames): max err {mx:.3e}")
            assert mx <= 5e-5, f"clip {b}: err {mx:.3e}"
        else:
            check_embed16(emb[b], ref, f"clip {b} ({rf} frames)")


@pytest.mark.parametrize("rate", [16000, 48000])
def test_clips_at_another_rate_equal_the_chain_with_the_resampler_in_front(rate):
    ctx = ctx_for("tiny")
    rows = E.make_clips(0, rate)
    want = reference_bounds(rows, rate, 2048, 512, 40.0, 441)
    emb, begin, end, frames = ctx.spkemb_wav(rows, rate, keep=441)
    c_emb, c_begin, c_end, c_frames = chain(ctx, rows, rate, keep=441)
    assert np.array_equal(begin, c_begin) and np.array_equal(end, c_end) and np.array_equal(frames, c_frames)
    assert np.array_equal(bits(emb), bits(c_emb)), int((bits(emb) != bits(c_emb)).sum())
    n_model = [_lib.resampled_len(len(r), rate, NATIVE) for r in rows]
    for b in range(len(rows)):                            # the bounds are in samples at the model's rate
        assert (int(begin[b]), int(end[b])) == want[b] and 0 <= begin[b] < end[b] <= n_model[b]
    assert sum((int(begin[b]), int(end[b])) != (0, n_model[b]) for b in range(len(rows))) >= 4


@pytest.mark.parametrize("max_samples", [12345, 513, 1 << 20])
def test_cropped_windows_equal_the_chain_with_the_slice_cut_likewise(max_samples):
    ctx = ctx_for("tiny")
    rows = E.make_clips(0)
    want = reference_bounds(rows, NATIVE, 2048, 512, 40.0, 3, max_samples)
    emb, begin, end, frames = ctx.spkemb_wav(rows, keep=3, max_samples=max_samples)
    c_emb, c_begin, c_end, c_frames = chain(ctx, rows, keep=3, max_samples=max_samples)
    assert [(int(a), int(b)) for a, b in zip(begin, end)] == want
    assert np.array_equal(end, c_end) and np.array_equal(frames, c_frames) and np.array_equal(bits(emb), bits(c_emb))
    whole = reference_bounds(rows, NATIVE, 2048, 512, 40.0, 3)
    cut = sum(int(end[b] - begin[b]) == max_samples for b in range(len(rows)))
    assert cut == sum(e - b > max_samples for b, e in whole) and (cut >= 2, cut == 5, cut == 0)[[12345, 513, 1 << 20].index(max_samples)], cut


def test_placement_device_rows_queued_output_and_nothing_else_read_or_written():
    ctx = ctx_for("tiny")
    rows = E.make_clips(0)
    reference_bounds(rows, NATIVE, 2048, 512, 40.0, 441)
    x, n = padded(rows, odd=True)                          # odd Nmax: the rows start at every alignment
    B, Nmax = x.shape
    H = ctx.hidden
    prm = params(keep=441)
    want = np.empty((B, H), np.float32)
    rc, wb, we, wf = raw(ctx, x, n, Nmax, NATIVE, prm, want)
    assert rc == 0, err(ctx)
    xin = ctx.dev_alloc(x.nbytes + 16)
    dout = ctx.dev_alloc((B * H + 16) * 4)
    try:
        ctx.dev_from_host(xin + 4, x)                     # ... and the device copy sits one float off a 16-byte boundary
        got = np.empty((B, H), np.float32)
        rc, begin, end, frames = raw(ctx, xin + 4, n, Nmax, NATIVE, prm, got, _lib.ZVX_DEVICE_IN, extra=2)
        assert rc == 0, err(ctx)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(begin[:B], wb) and np.array_equal(end[:B], we) and np.array_equal(frames[:B], wf)
        assert np.all(begin[B:] == -7) and np.all(end[B:] == -7) and np.all(frames[B:] == -7)      # nothing beyond index B - 1
        # device in, device out, queued: sentinels on both sides of the B x hidden floats
        ctx.dev_from_host(dout, np.full(B * H + 16, SENTINEL32, np.uint32))
        rc, begin, end, frames = raw(ctx, xin + 4, n, Nmax, NATIVE, prm, dout + 32, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC)
        assert rc == 0, err(ctx)
        ctx.sync()
        buf = ctx.dev_to_host(dout, (B * H + 16,), np.uint32)
        assert np.all(buf[:8] == SENTINEL32) and np.all(buf[8 + B * H:] == SENTINEL32)
        assert np.array_equal(buf[8:8 + B * H].reshape(B, H), bits(want)) and np.array_equal(begin, wb)
        # samples at and beyond nsamples[b] are never read
        xn = x.copy()
        for b in range(B):
            xn[b, n[b]:] = np.nan
        ctx.dev_from_host(xin + 4, xn)
        for src, fl in ((xn, 0), (xin + 4, _lib.ZVX_DEVICE_IN)):
            got = np.empty((B, H), np.float32)
            rc = raw(ctx, src, n, Nmax, NATIVE, prm, got, fl)[0]
            assert rc == 0 and np.array_equal(bits(got), bits(want)), fl
        # the binding's device form, and the stage slot
        ctx.dev_from_host(xin + 4, x)
        ctx.set_int("profile", 1)
        try:
            b2, e2, f2 = ctx.spkemb_wav_device(xin + 4, n, Nmax, dout, keep=441)
            assert ctx.stage_times()["spkemb"] > 0
        finally:
            ctx.set_int("profile", 0)
        assert np.array_equal(b2, wb) and np.array_equal(e2, we) and np.array_equal(f2, wf)
        assert np.array_equal(bits(ctx.dev_to_host(dout, (B, H), np.float32)), bits(want))
    finally:
        ctx.dev_free(xin)
        ctx.dev_free(dout)


def test_errors_leave_the_context_usable():
    ctx = ctx_for("tiny")
    rows = E.make_clips(0)
    reference_bounds(rows, NATIVE, 2048, 512, 40.0, 0)
    x, n = padded(rows)
    B, Nmax = x.shape
    H = ctx.hidden
    prm = params()
    want = np.empty((B, H), np.float32)
    assert raw(ctx, x, n, Nmax, NATIVE, prm, want)[0] == 0, err(ctx)
    inv = _lib.ZVX_E_INVALID
    out = np.full((B, H), SENTINEL32, np.uint32)

    def invalid(*a, **kw):
        rc = raw(ctx, *a, **kw)[0]
        return rc == inv and len(err(ctx)) > 0 and np.all(out == SENTINEL32)

    # validation: nothing is queued, ZVX_E_INVALID with a message each
    assert ctx._lib.zvx_spkemb_wav(None, vp(x), vp(n), B, Nmax, NATIVE, C.byref(prm), vp(out), None, None, None, 0) == inv
    assert invalid(None, n, Nmax, NATIVE, prm, out)
    assert invalid(x, None, Nmax, NATIVE, prm, out, B=B)
    assert invalid(x, n, Nmax, NATIVE, None, out)
    assert raw(ctx, x, n, Nmax, NATIVE, prm, None)[0] == inv and err(ctx)
    assert invalid(x, n, Nmax, NATIVE, prm, out, B=0) and invalid(x, n, Nmax, NATIVE, prm, out, B=-1)
    assert invalid(x, n, 0, NATIVE, prm, out)
    assert invalid(x, np.array([n[0], -1, n[2], n[3], n[4]], np.int32), Nmax, NATIVE, prm, out)
    assert invalid(x, np.array([n[0], Nmax + 1, n[2], n[3], n[4]], np.int32), Nmax, NATIVE, prm, out)
    for p in (params(frame=1, hop=1), params(hop=0), params(frame=512, hop=513), params(keep=-1), params(top_db=float("nan")),
              params(top_db=float("inf")), params(max_samples=-1)):
        assert invalid(x, n, Nmax, NATIVE, p, out), (p.frame, p.hop, p.top_db, p.keep, p.max_samples)
    assert invalid(x, n, Nmax, NATIVE, prm, out, flags=_lib.ZVX_NO_SYNC)                      # ZVX_NO_SYNC without ZVX_DEVICE_OUT
    for fl in (4, 16, 32, 64, 128):
        assert invalid(x, n, Nmax, NATIVE, prm, out, flags=fl), fl
    assert invalid(x, n, Nmax, 3999, prm, out) and invalid(x, n, Nmax, 192001, prm, out)      # the rate checks of zvx_resample
    rc = raw(ctx, x, n, Nmax, 22051, prm, out)[0]                                             # L = 22050, M = 22051: no bank for it
    assert rc == _lib.ZVX_E_UNSUPPORTED and np.all(out == SENTINEL32)

    # after the wait: a window of fewer than 2 hop samples.  Row 1 carries only a click: [quiet 1500, 100 loud, quiet 1400]
    rng = np.random.default_rng(3)
    click = (E.QUIET * rng.standard_normal(3000)).astype(np.float32)
    click[1500:1600] += (0.3 * rng.standard_normal(100)).astype(np.float32)
    bad_rows = [rows[3], click, rows[1]]
    xb, nb = padded(bad_rows)
    short = params(frame=128, hop=64, top_db=25.0)
    wantb = reference_bounds(bad_rows, NATIVE, 128, 64, 25.0, 0)
    assert 0 < wantb[1][1] - wantb[1][0] < MIN_WINDOW and all(e - b >= MIN_WINDOW for b, e in (wantb[0], wantb[2]))
    for what, p, rws, bnds in (("trimmed", short, (xb, nb), wantb),
                               ("cropped", params(max_samples=300), (x, n), reference_bounds(rows, NATIVE, 2048, 512, 40.0, 0, 300)),
                               ("too short", params(top_db=0.0), padded([rows[0], rows[4][:400]]), [(0, len(rows[0])), (0, 400)])):
        xs, ns = rws
        outb = np.full((len(ns), H), SENTINEL32, np.uint32)
        rc, begin, end, frames = raw(ctx, xs, ns, xs.shape[1], NATIVE, p, outb)
        msg = err(ctx)
        first = next(b for b, (bg, en) in enumerate(bnds) if en - bg < MIN_WINDOW)
        assert rc == inv and f"row {first} " in msg and str(bnds[first][0]) in msg and str(bnds[first][1]) in msg and str(MIN_WINDOW) in msg, (what, msg)
        assert np.all(outb == SENTINEL32), what                                                # nothing is written to out
        assert [(int(a), int(b)) for a, b in zip(begin, end)] == bnds, what                    # begin / end / frames are still filled
        assert [int(f) for f in frames] == [max(0, 1 + (e - b + 2 * 384 - N_FFT) // HOP) if e - b + 2 * 384 >= N_FFT else 0 for b, e in bnds], what
        again = np.empty((B, H), np.float32)                                                   # the next valid call on the same context
        assert raw(ctx, x, n, Nmax, NATIVE, prm, again)[0] == 0 and np.array_equal(bits(again), bits(want)), what


def _post_calls_reject(ctx, bit):
    """zvx_join, zvx_loudness, zvx_normalize, zvx_true_peak and zvx_limit answer flag `bit` with ZVX_E_INVALID"""
    x = (0.1 * np.random.default_rng(0).standard_normal((2, 9000))).astype(np.float32)
    n = np.array([9000, 8000], np.int32)
    out, L = np.zeros_like(x), _lib
    jp, lp, mp = L.JoinParams(2048, 512, 40.0, 0, 0), L.LoudnessParams(-23.0, 0.891, 20.0, 0), L.LimitParams(0.891, 5.0, 4)
    ol = C.c_int64(0)
    lib, h = ctx._lib, ctx._h
    return [lib.zvx_join(h, vp(x), vp(n), 2, 9000, None, C.byref(jp), vp(out), 18000, C.byref(ol), None, None, None, bit),
            lib.zvx_loudness(h, vp(x), vp(n), 2, 9000, NATIVE, None, None, bit),
            lib.zvx_normalize(h, vp(x), vp(n), 2, 9000, NATIVE, C.byref(lp), vp(out), 9000, None, None, None, bit),
            lib.zvx_true_peak(h, vp(x), vp(n), 2, 9000, NATIVE, 4, vp(np.zeros(2, np.float32)), bit),
            lib.zvx_limit(h, vp(x), vp(n), 2, 9000, NATIVE, C.byref(mp), vp(out), 9000, None, None, bit)]


def test_device_embedding_into_synthesis_equals_the_host_embedding():
    ctx = ctx_for("tiny")
    B, T, H, hop = 2, 12, ctx.hidden, ctx.hop
    ph, pu, Tl, _, dur = synthetic.batch(B, T, 5, "uniform")
    clips = [E.make_clips(0)[1], E.make_clips(0)[3]]
    reference_bounds(clips, NATIVE, 2048, 512, 40.0, 0)
    x, n = padded(clips)
    cap = 400                                             # frames per utterance the predicted lengths may reach (about 6 per phoneme)
    stride = cap * hop
    xin, emb_d, wav_d = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(B * H * 4), ctx.dev_alloc(B * stride * 4)
    try:
        ctx.dev_from_host(xin, x)
        for duration in (dur, None):                      # forced: both calls only queue; predicted: the synthesis waits once for its lengths
            kw = dict(duration=duration, want_mel=False, Lmax_cap=cap, wav_device_ptr=wav_d, wav_stride=stride, no_sync=True)
            ctx.dev_from_host(wav_d, np.zeros(B * stride, np.float32))
            ctx.dev_from_host(emb_d, np.zeros(B * H, np.float32))
            ctx.spkemb_wav_device(xin, n, x.shape[1], emb_d, no_sync=True)
            r_dev = ctx.synthesize(ph, pu, Tl, emb_d, **kw)                                  # at once: no sync in between
            ctx.sync()
            wav_dev = ctx.dev_to_host(wav_d, (B, stride), np.float32)
            emb = ctx.dev_to_host(emb_d, (B, H), np.float32)
            assert np.array_equal(bits(emb), bits(ctx.spkemb_wav(clips)[0]))
            ctx.dev_from_host(wav_d, np.zeros(B * stride, np.float32))
            r_host = ctx.synthesize(ph, pu, Tl, emb, **kw)                                   # the same floats from the host
            ctx.sync()
            wav_host = ctx.dev_to_host(wav_d, (B, stride), np.float32)
            assert np.array_equal(r_dev["mel_len"], r_host["mel_len"]) and int(r_host["mel_len"].min()) >= 2
            assert wav_host.any() and np.array_equal(bits(wav_dev), bits(wav_host)), ("forced" if duration is not None else "predicted")
            # a call that waits for its own rows (one stream) takes the device embedding too
            one = ctx.synthesize(ph, pu, Tl, emb_d, duration=duration, want_mel=False, Lmax_cap=cap)
            ml = int(r_host["mel_len"].max()) * hop
            assert np.array_equal(bits(one["wav"][:, :ml]), bits(wav_host[:, :ml]))
        # every other entry point treats bit 64 as before: the vocoder ignores it, the post-processing calls refuse it
        mel = (0.5 * np.random.default_rng(1).standard_normal((2, 20, ctx.n_mels))).astype(np.float32)
        P = np.array([20, 17], np.int32)
        w0, w64 = np.zeros((2, 20 * hop), np.float32), np.zeros((2, 20 * hop), np.float32)
        assert ctx._lib.zvx_vocode_mel(ctx._h, vp(mel), vp(P), 2, 20, vp(w0), 20 * hop, 0) == 0
        assert ctx._lib.zvx_vocode_mel(ctx._h, vp(mel), vp(P), 2, 20, vp(w64), 20 * hop, _lib.ZVX_DEVICE_SPK) == 0
        assert np.array_equal(bits(w0), bits(w64))
        assert _post_calls_reject(ctx, _lib.ZVX_DEVICE_SPK) == [_lib.ZVX_E_INVALID] * 5
    finally:
        for p in (xin, emb_d, wav_d):
            ctx.dev_free(p)


def test_speaker_embed_batch_agrees_with_speaker_embed_per_clip():
    from zerovox_amd.mels import trim_silence
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="f32")
    try:
        ctx = synth.model.ctx
        at16 = E.make_clips(0, 16000)
        wavs = E.make_clips(0)
        rates = [NATIVE, 16000, NATIVE, 16000, NATIVE]
        wavs = [at16[i] if rates[i] == 16000 else wavs[i] for i in range(5)]
        for w, r in zip(wavs, rates):
            reference_bounds([w], r, 2048, 512, 40.0, 0)
        batch = synth.speaker_embed_batch(wavs, rates)
        assert batch.shape == (5, 1, ctx.hidden) and batch.dtype == np.float32
        for i, (w, r) in enumerate(zip(wavs, rates)):
            one = synth.speaker_embed(w, r)
            mx = float(np.abs(batch[i, 0].astype(np.float64) - one[0, 0]).max())
            print(f"clip {i} at {r} Hz: batch against speaker_embed {mx:.3e}")
            assert mx <= 5e-5, (i, mx)
            # speaker_embed itself is what it was: the chain of the calls it has always been made of
            y = w if r == NATIVE else ctx.resample([w], r, NATIVE)[0][0]
            mel, frames = ctx.melspec([trim_silence(y, top_db=40)])
            assert np.array_equal(bits(one[0, 0]), bits(ctx.spkemb(mel[:, :int(frames[0])], frames)[0])), i
        same = synth.speaker_embed_batch(wavs[::2])                                       # one rate, none given
        assert np.array_equal(bits(same), bits(batch[::2]))
    finally:
        synth.model.close()
