"""Loudness normalisation on the MI355X: zvx_loudness / zvx_normalize against tests/loudness_ref.py (scipy.signal.lfilter in float64, gates
in the power domain; never the library), queued device input, and the loudness keywords of ZeroVoxTTS.tts / tts_long end to end.
include/zvx.h defines the integrated loudness to within 1e-7 LU outside an ambiguity band of 1e-3 LU around either gate: a double
recurrence differs from the reference by its summation order and by at most 1e-12 dB of warm-up truncation, an f32 filter state by about
4e-6 dB, so the bound separates the two by more than a factor of ten on each side.  Every test first asserts, from the reference alone,
that no block of its rows -- nor of the rows pooled -- lies within 0.01 LU of a gate."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import join_ref as J
import loudness_ref as R
from stream_util import _ragged_case, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
RATES = (8000, 16000, 22050, 48000)
LUFS_TOL = 1e-7
MARGIN = 0.01                                              # ten times the ambiguity band
# (target, peak_ceiling, max_gain_db): by the reference the per-row gains of every seed end bounded by the ceiling (set 0: the probe row's
# 1.5 spike), by max_gain_db (set 1) and by neither; the common gain by max_gain_db (set 1), by the ceiling (set 3) and by neither
SETS = [(-23.0, 0.891, 20.0), (-3.0, 0.0, 5.0), (-14.0, 2.0, 40.0), (-6.0, 0.891, 20.0)]
_ctx, _ref = {}, {}


def ctx_for(voc, prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def case(seed, fs):
    """(rows, x [B][odd Nmax] with the sentinel behind every row, n, the reference's measurement), computed once and left unchanged"""
    key = (seed, fs)
    if key not in _ref:
        rows = J.make_rows(seed) + R.extra_rows(fs)
        n = np.array([len(r) for r in rows], np.int32)
        nmax = int(n.max())
        x = np.full((len(rows), nmax + (nmax % 2 == 0)), SENTINEL32, np.uint32).view(np.float32)   # nothing behind a row's end may be read
        for b, r in enumerate(rows):
            x[b, :n[b]] = r
        m = R.measure(rows, fs)
        for a in (x, n):
            a.setflags(write=False)
        _ref[key] = (rows, x, n, m)
    return _ref[key]


def assert_unambiguous(m, what):
    assert np.all(m["margin"] > MARGIN), (what, m["margin"])
    assert m["margin_common"] > MARGIN, (what, m["margin_common"])


def raw_loudness(ctx, x, n, Nmax, rate, flags=0, B=None):
    B = len(n) if B is None else B
    lufs, peak = np.full(max(B, 1), 7.0, np.float64), np.full(max(B, 1), -7.0, np.float32)
    rc = ctx._lib.zvx_loudness(ctx._h, vp(x), vp(n), B, Nmax, rate, vp(lufs), vp(peak), flags)
    return rc, lufs, peak


def params(target=-23.0, ceiling=0.891, max_gain_db=20.0, mode=0):
    return _lib.LoudnessParams(target, ceiling, max_gain_db, mode)


def raw_normalize(ctx, x, n, Nmax, rate, prm, out, stride, flags=0, B=None, results=True):
    B = len(n) if B is None else B
    lufs, peak, gain = np.full(max(B, 1), 7.0, np.float64), np.full(max(B, 1), -7.0, np.float32), np.full(max(B, 1), -7.0, np.float32)
    rc = ctx._lib.zvx_normalize(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if prm is not None else None, vp(out), stride,
                                vp(lufs) if results else None, vp(peak) if results else None, vp(gain) if results else None, flags)
    return rc, lufs, peak, gain


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("seed", range(8))
def test_measurement_matches_the_float64_reference(seed):
    ctx = ctx_for("tiny")
    removed_abs = removed_rel = 0
    worst = 0.0
    for fs in RATES:
        rows, x, n, m = case(seed, fs)
        assert_unambiguous(m, (seed, fs))
        removed_abs += sum(r[0] for r in m["removed"]); removed_rel += sum(r[1] for r in m["removed"])
        B, Nmax = x.shape
        assert Nmax % 2 == 1
        xin = ctx.dev_alloc(x.nbytes + 16)
        try:
            ctx.dev_from_host(xin + 4, x)                 # the device copy sits one float off a 16-byte boundary
            rc, lufs, peak = raw_loudness(ctx, x, n, Nmax, fs)
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
            rc, lufs_d, peak_d = raw_loudness(ctx, xin + 4, n, Nmax, fs, _lib.ZVX_DEVICE_IN)
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        finally:
            ctx.dev_free(xin)
        assert np.array_equal(lufs.view(np.uint64), lufs_d.view(np.uint64)) and same_bits(peak, peak_d), (seed, fs, "host in / device in")
        assert same_bits(peak, m["peak"]), (seed, fs, peak, m["peak"])
        for b in range(B):                                # every row, none skipped
            if m["lufs"][b] == -np.inf:
                assert lufs[b] == -np.inf, (seed, fs, b, len(rows[b]), lufs[b])
            else:
                dev = abs(lufs[b] - m["lufs"][b])
                worst = max(worst, dev)
                assert dev <= LUFS_TOL, (seed, fs, b, len(rows[b]), lufs[b], m["lufs"][b], dev)
        l2, p2 = ctx.loudness(rows, rate=fs)             # the binding's list form pads with zeros: the same numbers
        assert np.array_equal(l2.view(np.uint64), lufs.view(np.uint64)) and same_bits(p2, peak)
    print(f"seed {seed}: largest |lufs - reference| {worst:.3e} LU; blocks removed by the absolute / relative gate {removed_abs} / {removed_rel}")
    assert removed_abs > 0 and removed_rel > 0           # both gates do remove blocks in these rows


def check_normalize(ctx, rows, x, n, m, fs, xin, st, common, what):
    """one parameter set: host f32 out of place, device PCM16 out of place, device f32 in place; gains, every output bit, the sentinels"""
    B, Nmax = x.shape
    prm = params(*st, mode=_lib.ZVX_LOUD_COMMON if common else _lib.ZVX_LOUD_PER_ROW)
    want, limits = R.gains(m, *st, common=common)
    stride = Nmax + 6
    out = np.full((B + 1, stride), SENTINEL32, np.uint32)                         # one row more than the call owns
    rc, lufs, peak, gain = raw_normalize(ctx, x, n, Nmax, fs, prm, out, stride)
    assert rc == 0, (what, ctx._lib.zvx_last_error(ctx._h))
    assert within_one_ulp(gain, want), (what, gain, want)
    if common:
        assert len(set(gain.view(np.uint32).tolist())) == 1
    assert same_bits(peak, m["peak"])
    fin = np.isfinite(m["lufs"])
    assert np.array_equal(np.isneginf(lufs), ~fin) and np.all(np.abs(lufs[fin] - m["lufs"][fin]) <= LUFS_TOL), what
    for b in range(B):
        prod = x[b, :n[b]] * gain[b]                                              # ONE f32 multiply by the gain the call reported
        assert np.array_equal(out[b, :n[b]], prod.view(np.uint32)), (what, b, "host f32")
        assert np.all(out[b, n[b]:] == SENTINEL32), (what, b, "written behind nsamples[b]")
    assert np.all(out[B] == SENTINEL32), (what, "written behind the last row")
    # device in (offset pointer) -> device out, PCM16, another stride, an output pointer one sample off an 8-byte boundary
    dout = ctx.dev_alloc((B + 1) * stride * 4 + 16)
    try:
        ctx.dev_from_host(dout, np.full((B + 1) * stride * 2 + 8, SENTINEL16, np.int16))
        rc, lufs_p, peak_p, gain_p = raw_normalize(ctx, xin, n, Nmax, fs, prm, dout + 2, stride, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_PCM16)
        assert rc == 0, (what, ctx._lib.zvx_last_error(ctx._h))
        assert same_bits(gain_p, gain) and np.array_equal(lufs_p.view(np.uint64), lufs.view(np.uint64)) and same_bits(peak_p, peak)
        flat = ctx.dev_to_host(dout, ((B + 1) * stride + 8,), np.int16)
        assert flat[0] == SENTINEL16
        pcm = flat[1:1 + (B + 1) * stride].reshape(B + 1, stride)
        for b in range(B):
            assert np.array_equal(pcm[b, :n[b]], R.pcm16(x[b, :n[b]] * gain[b])), (what, b, "device pcm16")
            assert np.all(pcm[b, n[b]:] == SENTINEL16), (what, b, "pcm16 written behind nsamples[b]")
        assert np.all(pcm[B] == SENTINEL16)
        # in place on the device rows equals out of place
        work = ctx.dev_alloc(x.nbytes + 16)
        try:
            ctx.dev_from_host(work + 4, x)
            rc, lufs_i, peak_i, gain_i = raw_normalize(ctx, work + 4, n, Nmax, fs, prm, work + 4, Nmax, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT)
            assert rc == 0, (what, ctx._lib.zvx_last_error(ctx._h))
            got = ctx.dev_to_host(work + 4, (B, Nmax), np.uint32)
        finally:
            ctx.dev_free(work)
        assert same_bits(gain_i, gain)
        for b in range(B):
            assert np.array_equal(got[b, :n[b]], out[b, :n[b]]), (what, b, "in place")
            assert np.all(got[b, n[b]:] == SENTINEL32), (what, b, "in place: written behind nsamples[b]")
    finally:
        ctx.dev_free(dout)
    return limits


@pytest.mark.parametrize("seed", range(8))
def test_normalised_rows_are_the_product_with_the_reported_gain(seed):
    ctx = ctx_for("tiny")
    kinds_row, kinds_common = set(), set()
    for i, fs in enumerate(RATES):
        rows, x, n, m = case(seed, fs)
        assert_unambiguous(m, (seed, fs))
        xin = ctx.dev_alloc(x.nbytes + 16)
        try:
            ctx.dev_from_host(xin + 4, x)
            for k in (0, 1):                              # two of the four parameter sets per rate: every set at two rates per seed
                st = SETS[(seed + i + 2 * k) % 4]
                kinds_row |= set(check_normalize(ctx, rows, x, n, m, fs, xin + 4, st, False, (seed, fs, st, "per row")))
                kinds_common |= set(check_normalize(ctx, rows, x, n, m, fs, xin + 4, st, True, (seed, fs, st, "common")))
        finally:
            ctx.dev_free(xin)
    assert kinds_row == {None, "max_gain", "ceiling"} and kinds_common == {None, "max_gain", "ceiling"}, (kinds_row, kinds_common)
    rows, x, n, m = case(seed, 22050)                     # the binding's list form
    out, lufs, peak, gain = ctx.normalize(rows, -23.0, rate=22050)
    assert within_one_ulp(gain, R.gains(m, -23.0)[0]) and all(same_bits(out[b, :n[b]], x[b, :n[b]] * gain[b]) for b in range(len(rows)))
    assert all(not out[b, n[b]:].any() for b in range(len(rows)))


def test_queued_synthesis_feeds_the_normaliser_in_stream_order():
    ctx = ctx_for("tiny")
    hop, fs = ctx.hop, ctx.get_int("sampling_rate")
    cs = _ragged_case(4, 24, 43)
    host = ctx.synthesize(*cs, None, want_mel=False)
    ml = host["mel_len"]
    rows = [host["wav"][b, :int(ml[b]) * hop] for b in range(4)]
    stride = int(ml.max()) * hop + 13
    dptr = ctx.dev_alloc(4 * stride * 4)
    try:
        for common in (False, True):
            want, lufs_w, peak_w, gain_w = ctx.normalize(rows, -20.0, common=common)      # normalising the fetched rows
            ctx.dev_from_host(dptr, np.full((4, stride), SENTINEL32, np.uint32))         # nothing of an earlier round is left to be read
            ctx.synthesize(*cs, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True, native_rate=True)
            lufs, peak, gain = ctx.normalize_device(dptr, ml * hop, stride, -20.0, common=common)       # at once: no sync in between
            got = ctx.dev_to_host(dptr, (4, stride), np.float32)
            assert same_bits(gain, gain_w) and same_bits(peak, peak_w) and np.array_equal(lufs.view(np.uint64), lufs_w.view(np.uint64)), common
            for b in range(4):
                assert same_bits(got[b, :len(rows[b])], want[b, :len(rows[b])]), (common, b)
            # the queued form: nothing comes back, the rows are the same after a sync
            ctx.synthesize(*cs, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True, native_rate=True)
            assert ctx.normalize_device(dptr, ml * hop, stride, -20.0, common=common, no_sync=True) is None
            ctx.sync()
            assert same_bits(ctx.dev_to_host(dptr, (4, stride), np.float32), got), common
    finally:
        ctx.dev_free(dptr)


def test_loudness_errors_leave_the_context_usable():
    ctx = ctx_for("tiny")
    fs = 16000
    rows, x, n, m = case(2, fs)
    B, Nmax = x.shape
    inv = _lib.ZVX_E_INVALID
    out = np.zeros((B, Nmax), np.float32)
    prm = params()
    lib, h = ctx._lib, ctx._h
    nan, inf = float("nan"), float("inf")

    def norm(x_=x, n_=n, B_=None, Nmax_=Nmax, rate=fs, prm_=prm, out_=out, stride=Nmax, flags=0):
        return raw_normalize(ctx, x_, n_, Nmax_, rate, prm_, out_, stride, flags, B=B_)[0]

    def meas(x_=x, n_=n, B_=None, Nmax_=Nmax, rate=fs, flags=0):
        return raw_loudness(ctx, x_, n_, Nmax_, rate, flags, B=B_)[0]

    neg, big = n.copy(), n.copy()
    neg[1], big[1] = -1, Nmax + 1
    assert lib.zvx_loudness(None, vp(x), vp(n), B, Nmax, fs, None, None, 0) == inv
    assert lib.zvx_normalize(None, vp(x), vp(n), B, Nmax, fs, C.byref(prm), vp(out), Nmax, None, None, None, 0) == inv
    assert meas(x_=None) == inv and norm(x_=None) == inv
    assert meas(n_=None, B_=B) == inv and norm(n_=None, B_=B) == inv
    assert norm(prm_=None) == inv and norm(out_=None) == inv
    assert meas(B_=0) == inv and norm(B_=0) == inv and meas(B_=-1) == inv
    assert meas(Nmax_=0) == inv and norm(Nmax_=0) == inv
    assert meas(n_=neg) == inv and norm(n_=neg) == inv and meas(n_=big) == inv and norm(n_=big) == inv
    for rate in (3999, 192001, 0, -16000):
        assert meas(rate=rate) == inv and norm(rate=rate) == inv, rate
    assert norm(stride=Nmax - 1) == inv
    assert meas(flags=64) == inv and norm(flags=64) == inv and norm(flags=_lib.ZVX_HOST_ASYNC) == inv
    assert meas(flags=_lib.ZVX_DEVICE_OUT) == inv and meas(flags=_lib.ZVX_PCM16) == inv      # zvx_loudness knows ZVX_DEVICE_IN only
    assert norm(flags=_lib.ZVX_NO_SYNC) == inv
    xf = np.array(x)                                       # a writable copy for the in-place forms
    assert norm(x_=xf, out_=xf, flags=_lib.ZVX_PCM16) == inv
    # in place: the stride is Nmax, and both pointers lie on the same side
    for kw in (dict(stride=Nmax + 2), dict(flags=_lib.ZVX_DEVICE_IN), dict(flags=_lib.ZVX_DEVICE_OUT)):
        assert norm(x_=xf, out_=xf, **kw) == inv and b"zvx_normalize" in lib.zvx_last_error(h), kw
    for t in (nan, inf, -inf, -70.5, 0.5):
        assert norm(prm_=params(target=t)) == inv, t
    for g in (nan, inf, -0.5):
        assert norm(prm_=params(max_gain_db=g)) == inv, g
    assert norm(prm_=params(ceiling=nan)) == inv
    for mode in (2, -1):
        assert norm(prm_=params(mode=mode)) == inv, mode
    assert b"mode" in lib.zvx_last_error(h)
    # the limits of the valid ranges are accepted, and the context still works
    assert norm(prm_=params(target=-70.0, max_gain_db=0.0, ceiling=-1.0)) == 0 and norm(prm_=params(target=0.0, ceiling=inf)) == 0
    assert meas(rate=4000) == 0 and meas(rate=192000) == 0
    rc, lufs, peak = raw_loudness(ctx, x, n, Nmax, fs)
    assert rc == 0 and same_bits(peak, m["peak"])
    rc, _, _, gain = raw_normalize(ctx, xf, n, Nmax, fs, prm, xf, Nmax)                  # in place on host rows
    assert rc == 0 and within_one_ulp(gain, R.gains(m, -23.0)[0])
    for b in range(B):
        assert same_bits(xf[b, :n[b]], x[b, :n[b]] * gain[b]) and np.all(xf.view(np.uint32)[b, n[b]:] == SENTINEL32), b


def test_loudness_accounting_and_nothing_else_moved():
    ctx = ctx_for("tiny")
    cs = _ragged_case(3, 20, 41)
    before = ctx.synthesize(*cs, None, want_mel=False)
    rows, x, n, m = case(1, 22050)
    total = float(n.astype(np.int64).sum())
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.loudness(rows, rate=22050)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.loudness"]["launches"] == 1 and tags["post.loudness"]["bytes"] == 4.0 * total        # one timed group per call
        ms_measure = tags["post.loudness"]["ms"]
        ctx.reset_stats()
        ctx.normalize(rows, -23.0, rate=22050)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.loudness"]["launches"] == 1 and tags["post.loudness"]["bytes"] == 12.0 * total
        ctx.reset_stats()
        ctx.normalize(rows, -23.0, rate=22050, pcm16=True, common=True)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.loudness"]["launches"] == 1 and tags["post.loudness"]["bytes"] == 10.0 * total
        assert "post.join" not in tags and ms_measure > 0
        assert set(ctx.stage_times()) == set(_lib.STAGES) and _lib.ZVX_T_COUNT == 8
        print(f"post.loudness on {len(rows)} rows / {int(total)} samples at 22050 Hz: measure {ms_measure:.3f} ms, measure + pcm16 apply {tags['post.loudness']['ms']:.3f} ms")
    finally:
        ctx.set_int("profile", 0)
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert same_bits(after["wav"], before["wav"]) and np.array_equal(after["mel_len"], before["mel_len"])


THREE = "The quick brown fox jumps over the lazy dog; does it, really? Pack my box with five dozen liquor jugs"


def test_tts_and_tts_long_with_a_loudness_target():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    fs, target = 22050, -23.0
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    kw = dict(trim_db=0.0, fade_ms=0, pauses={".": 0, ";": 0, ",": 0, " ": 0})
    plain, seg0 = synth.tts_long(THREE, spk, **kw)
    assert len(seg0) == 3 and all("gain" not in s and "lufs" not in s for s in seg0)
    rows = [plain[s["start"]:s["start"] + s["samples"]] for s in seg0]
    m = R.measure(rows, fs)
    assert_unambiguous(m, "tts_long rows")
    ceiling = float(10.0 ** (-1.0 / 20.0))
    # "sentence": every segment is the un-normalised one times its own gain
    wav, seg = synth.tts_long(THREE, spk, loudness=target, loudness_mode="sentence", **kw)
    want, limits = R.gains(m, target, ceiling, 20.0)
    assert [(s["start"], s["samples"]) for s in seg] == [(s["start"], s["samples"]) for s in seg0]
    for i, s in enumerate(seg):
        g = np.float32(s["gain"])
        assert float(g) == s["gain"] and within_one_ulp([g], [want[i]]), (i, s["gain"], want[i])
        assert same_bits(wav[s["start"]:s["start"] + s["samples"]], rows[i] * g), i
        assert abs(s["lufs"] - m["lufs"][i]) <= LUFS_TOL, (i, s["lufs"], m["lufs"][i])
        reached = m["lufs"][i] + 20.0 * np.log10(float(g))
        print(f"sentence {i}: {m['lufs'][i]:.3f} LUFS, peak {m['peak'][i]:.3f}, gain {float(g):.5f} -> {reached:.5f} LUFS ({limits[i] or 'no bound'})")
        if limits[i] is None:
            assert abs(reached - target) <= 1e-4, (i, reached)
    # "paragraph" (the default): one gain, the pooled reference's
    wav_p, seg_p = synth.tts_long(THREE, spk, loudness=target, **kw)
    want_p = R.gains(m, target, ceiling, 20.0, common=True)[0]
    gp = np.float32(seg_p[0]["gain"])
    assert all(s["gain"] == seg_p[0]["gain"] for s in seg_p) and within_one_ulp([gp], [want_p[0]]), (gp, want_p[0])
    assert same_bits(wav_p, plain * gp)
    assert all(abs(s["lufs"] - m["lufs"][i]) <= LUFS_TOL for i, s in enumerate(seg_p))
    # tts: the same utterance times the reported gain; the plain call is untouched by the feature
    one, ph, length = synth.tts(seg0[0]["text"], spk)
    loud, ph2, length2 = synth.tts(seg0[0]["text"], spk, loudness=target)
    info = synth.last_loudness
    assert length2 == length and np.array_equal(ph, ph2) and loud.dtype == np.float32
    assert same_bits(loud, one * np.float32(info["gain"]))
    m1 = R.measure([one], fs)
    assert abs(info["lufs"] - m1["lufs"][0]) <= LUFS_TOL and np.float32(info["peak"]) == m1["peak"][0]
    assert within_one_ulp([info["gain"]], [R.gains(m1, target, ceiling, 20.0)[0][0]])
    again = synth.tts(seg0[0]["text"], spk)[0]
    assert same_bits(again, one)
    with pytest.raises(ValueError):
        synth.tts_stream(seg0[0]["text"], spk, loudness=target)
    with pytest.raises(ValueError):
        synth.tts_long(THREE, spk, loudness=target, loudness_mode="word")
    synth.model.close()
