"""True-peak metering and the look-ahead limiter on the MI355X: zvx_true_peak / zvx_limit against tests/limit_ref.py (float64 NumPy, never
the library), the exact properties of include/zvx.h on the device's own output, every form of the call, queued device input, errors,
accounting, and the limiter keywords of ZeroVoxTTS.tts / tts_long end to end.
The bound.  An oversampled point differs from the reference's by at most resample_ref.bound (T = 21 taps).  The envelope is a maximum of
such points and of exact |x|, so it moves by at most the largest bound among them; the depth 1 - c / e is 1 / c-Lipschitz in e; hold,
smoothing (weights that sum to 1) and the min are 1-Lipschitz in the sup norm; the rounding toward zero can fall on either side of an
f32 boundary (one ulp of a gain <= 1: 2^-23) and the product rounds once more (2^-24 of a value <= |x|).  Hence, for every sample,
|out - ref| <= |x[i]| (E[i] / c + 2^-22) with E[i] the largest bound of any point within 2 W samples; for os = 1 that is 2 ulp."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import join_ref as J
import limit_ref as L
import loudness_ref as R
import resample_ref as RS
from stream_util import _ragged_case, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
CEILING = 0.891
C32 = np.float32(CEILING)
RATES = (8000, 22050, 48000)
TILE = _lib.LIMIT_TILE                                     # both kernels cut a row into tiles of this many samples
CASES = [(os_, W) for os_ in (1, 4) for W in (1, 22, 110, 4096)]
_ctx, _rows, _ref = {}, {}, {}


def ctx_for(voc, prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def spike_rows(rng):
    """one spike of 2.0 over noise at 1e-3: at sample 0, at n - 1, and at t - 1, t, t + 1 for every tile edge t inside the row"""
    n = 3 * TILE + 100
    at = [0, n - 1] + [t + k for t in range(TILE, n, TILE) for k in (-1, 0, 1)]
    rows = []
    for a in at:
        x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        x[a] = 2.0 if a % 2 else -2.0
        rows.append(x)
    return rows


def make_case(seed, W):
    """(rows, x [B][odd Nmax] with the sentinel behind every row, n), computed once per (seed, W) and left unchanged"""
    key = (seed, W)
    if key not in _rows:
        rng = np.random.default_rng(1000 + seed)
        rows = L.scaled_rows(J.make_rows(seed))
        rows += [(rng.standard_normal(k) * 0.7).astype(np.float32) for k in (0, 1, 2, W, W + 1, 2 * W, 2 * W + 1)]
        rows.append((rng.standard_normal(2500) * 0.1).clip(-0.8, 0.8).astype(np.float32))     # entirely under the ceiling
        rows.append(np.full(3000, 1.0, np.float32))                                           # DC
        rows += spike_rows(rng)
        n = np.array([len(r) for r in rows], np.int32)
        nmax = int(n.max())
        x = np.full((len(rows), nmax + (nmax % 2 == 0)), SENTINEL32, np.uint32).view(np.float32)   # nothing behind a row's end may be read
        for b, r in enumerate(rows):
            x[b, :n[b]] = r
        for a in (x, n):
            a.setflags(write=False)
        _rows[key] = (rows, x, n)
    return _rows[key]


def reference(seed, W, os_):
    key = (seed, W, os_)
    if key not in _ref:
        rows = make_case(seed, W)[0]
        _ref[key] = [L.limit(r, CEILING, W, os_) for r in rows]
    return _ref[key]


def raw_true_peak(ctx, x, n, Nmax, rate, os_, flags=0, B=None, out=True):
    B = len(n) if B is None else B
    tp = np.full(max(B, 1), -7.0, np.float32)
    return ctx._lib.zvx_true_peak(ctx._h, vp(x), vp(n), B, Nmax, rate, os_, vp(tp) if out else None, flags), tp


def params(ceiling=CEILING, window_ms=5.0, oversample=4):
    return _lib.LimitParams(ceiling, window_ms, oversample)


def raw_limit(ctx, x, n, Nmax, rate, prm, out, stride, flags=0, B=None, results=True):
    B = len(n) if B is None else B
    peak, gmin = np.full(max(B, 1), -7.0, np.float32), np.full(max(B, 1), -7.0, np.float32)
    rc = ctx._lib.zvx_limit(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if prm is not None else None, vp(out), stride,
                            vp(peak) if results else None, vp(gmin) if results else None, flags)
    return rc, peak, gmin


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def ms_for(rate, W):
    ms = W * 1000.0 / rate
    assert L.window(rate, ms) == W, (rate, W, ms)
    return ms


def check_row(x, got, r, W, what):
    """one row of the device's output against the reference and against the exact properties; returns its largest error / bound"""
    n = len(x)
    if n == 0:
        return 0.0
    c = float(C32)
    err = np.abs(got.astype(np.float64) - r["out"].astype(np.float64))
    bound = np.abs(x.astype(np.float64)) * (r["E"] / c + 2.0 ** -22)
    worst = float(np.max(err - bound))
    assert worst <= 0.0, (what, int(np.argmax(err - bound)), float(err.max()), worst)          # every sample
    assert np.all(np.abs(got) <= C32), (what, float(np.abs(got).max()))                      # (a): exactly
    near = L.running_max((r["e"] >= c * (1.0 - 1e-5)).astype(np.float64), 2 * W) > 0
    keep = (r["g"] == 1.0) & ~near
    assert np.array_equal(got.view(np.uint32)[keep], x.view(np.uint32)[keep]), (what, "(b)")
    return float(np.max(err / np.maximum(bound, 1e-300)))


def implied_min_gain(x, got):
    ok = np.abs(x) > 1e-20
    return float(np.min(got[ok].astype(np.float64) / x[ok].astype(np.float64))) if ok.any() else 1.0


@pytest.mark.parametrize("seed", range(3))
def test_true_peak_matches_the_reference_and_the_resampler(seed):
    ctx = ctx_for("tiny")
    rows, x, n = make_case(seed, 22)
    B, Nmax = x.shape
    assert Nmax % 2 == 1
    xin = ctx.dev_alloc(x.nbytes + 16)
    try:
        ctx.dev_from_host(xin + 4, x)                     # the device copy sits one float off a 16-byte boundary
        for os_ in (1, 4, 8):
            rc, tp = raw_true_peak(ctx, x, n, Nmax, 22050, os_)
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
            rc, tp_d = raw_true_peak(ctx, xin + 4, n, Nmax, 22050, os_, _lib.ZVX_DEVICE_IN)
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
            assert same_bits(tp, tp_d), (os_, "host in / device in")
            rc, tp_r = raw_true_peak(ctx, x, n, Nmax, 192000, os_)                   # the rate does not enter
            assert rc == 0 and same_bits(tp, tp_r)
            peak = np.array([np.max(np.abs(r)) if len(r) else 0.0 for r in rows], np.float32)
            worst = 0.0
            for b, r in enumerate(rows):                  # every row
                want, bd = L.true_peak(r, os_)
                assert abs(float(tp[b]) - want) <= bd, (seed, os_, b, len(r), tp[b], want, bd)
                worst = max(worst, abs(float(tp[b]) - want) / bd if bd > 0 else 0.0)
            if os_ == 1:
                assert same_bits(tp, peak)
            else:                                         # the existing entry point's oversampled rows: the same bits
                y, ylen = ctx.resample(rows, 22050, os_ * 22050)
                assert np.array_equal(ylen, os_ * n)
                via = np.array([max(peak[b], np.max(np.abs(y[b, :ylen[b]])) if ylen[b] else 0.0) for b in range(B)], np.float32)
                assert same_bits(tp, via), (seed, os_, tp, via)
            assert same_bits(ctx.true_peak(rows, os_, rate=22050), tp)               # the binding's list form pads with zeros
            print(f"seed {seed} os {os_}: largest |tpeak - reference| / bound {worst:.3f}")
    finally:
        ctx.dev_free(xin)


@pytest.mark.parametrize("os_,W", CASES)
def test_limiter_matches_the_reference_in_every_form(os_, W):
    ctx = ctx_for("tiny")
    seed = CASES.index((os_, W))
    rows, x, n = make_case(seed, W)
    ref = reference(seed, W, os_)
    B, Nmax = x.shape
    stride = Nmax + 6
    first = None
    for rate in RATES:
        prm = params(CEILING, ms_for(rate, W), os_)
        out = np.full((B + 1, stride), SENTINEL32, np.uint32)                         # one row more than the call owns
        rc, peak, gmin = raw_limit(ctx, x, n, Nmax, rate, prm, out, stride)
        assert rc == 0, (rate, ctx._lib.zvx_last_error(ctx._h))
        if first is None:
            first = (out, peak, gmin)
        else:                                             # the rate enters through W alone
            assert np.array_equal(out, first[0]) and same_bits(peak, first[1]) and same_bits(gmin, first[2]), rate
    out, peak, gmin = first
    worst = 0.0
    for b in range(B):
        got = out[b, :n[b]].view(np.float32)
        assert np.all(out[b, n[b]:] == SENTINEL32), (b, "written behind nsamples[b]")
        worst = max(worst, check_row(x[b, :n[b]], got, ref[b], W, (os_, W, b, int(n[b]))))
        want_tp, bd = L.true_peak(rows[b], os_)
        assert abs(float(peak[b]) - want_tp) <= bd, (b, peak[b], want_tp, bd)
        if n[b]:
            assert abs(float(gmin[b]) - implied_min_gain(x[b, :n[b]], got)) <= float(np.spacing(gmin[b])), (b, gmin[b])
            assert abs(float(gmin[b]) - float(ref[b]["g32"].min())) <= float(ref[b]["E"].max()) / float(C32) + 2.0 ** -22, (b, gmin[b])
        else:
            assert gmin[b] == 1.0 and peak[b] == 0.0
    assert np.all(out[B] == SENTINEL32), "written behind the last row"
    under = len(J.make_rows(0)) + 7
    assert same_bits(out[under, :n[under]], x[under, :n[under]]) and gmin[under] == 1.0   # a row under the ceiling: bit for bit
    assert any(g < 1.0 for g in gmin)
    print(f"os {os_} W {W}: largest |out - reference| / bound {worst:.3f}")
    # device in (offset pointer) -> device out, PCM16, another stride, an output pointer one sample off an 8-byte boundary
    rate = RATES[1]
    prm = params(CEILING, ms_for(rate, W), os_)
    xin = ctx.dev_alloc(x.nbytes + 16)
    dout = ctx.dev_alloc((B + 1) * stride * 4 + 16)
    try:
        ctx.dev_from_host(xin + 4, x)
        ctx.dev_from_host(dout, np.full((B + 1) * stride * 2 + 8, SENTINEL16, np.int16))
        rc, peak_p, gmin_p = raw_limit(ctx, xin + 4, n, Nmax, rate, prm, dout + 2, stride, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_PCM16)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        assert same_bits(peak_p, peak) and same_bits(gmin_p, gmin)
        flat = ctx.dev_to_host(dout, ((B + 1) * stride + 8,), np.int16)
        assert flat[0] == SENTINEL16
        pcm = flat[1:1 + (B + 1) * stride].reshape(B + 1, stride)
        for b in range(B):
            assert np.array_equal(pcm[b, :n[b]], RS.pcm16(out[b, :n[b]].view(np.float32))), (b, "device pcm16")
            assert np.all(pcm[b, n[b]:] == SENTINEL16), (b, "pcm16 written behind nsamples[b]")
        assert np.all(pcm[B] == SENTINEL16)
        # in place on the device rows equals out of place
        rc, peak_i, gmin_i = raw_limit(ctx, xin + 4, n, Nmax, rate, prm, xin + 4, Nmax, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        got = ctx.dev_to_host(xin + 4, (B, Nmax), np.uint32)
        assert same_bits(peak_i, peak) and same_bits(gmin_i, gmin)
        for b in range(B):
            assert np.array_equal(got[b, :n[b]], out[b, :n[b]]), (b, "in place")
            assert np.all(got[b, n[b]:] == SENTINEL32), (b, "in place: written behind nsamples[b]")
    finally:
        ctx.dev_free(dout)
        ctx.dev_free(xin)
    o2, p2, g2 = ctx.limit(rows, CEILING, ms_for(rate, W), os_, rate=rate)             # the binding's list form
    assert same_bits(p2, peak) and same_bits(g2, gmin)
    assert all(same_bits(o2[b, :n[b]], out[b, :n[b]]) and not o2[b, n[b]:].any() for b in range(B))


def test_a_non_finite_row_leaves_the_others_alone():
    ctx = ctx_for("tiny")
    rng = np.random.default_rng(5)
    rows = [(rng.standard_normal(5000) * 0.6).astype(np.float32) for _ in range(3)]
    bad = [r.copy() for r in rows]
    bad[1][[0, 1234, 2048, 4999]] = [np.nan, np.inf, -np.inf, np.nan]
    for os_ in (1, 4):
        clean, pc, gc = ctx.limit(rows, CEILING, 1.0, os_, rate=22050)
        got, pg, gg = ctx.limit(bad, CEILING, 1.0, os_, rate=22050)                    # succeeds; row 1 is unspecified
        for b in (0, 2):
            assert same_bits(got[b], clean[b]) and same_bits(pg[b], pc[b]) and same_bits(gg[b], gc[b]), (os_, b)
        tc, tb = ctx.true_peak(rows, os_, rate=22050), ctx.true_peak(bad, os_, rate=22050)
        assert same_bits(tc[[0, 2]], tb[[0, 2]])
    again = ctx.limit(rows, CEILING, 1.0, 4, rate=22050)[0]
    assert same_bits(again, clean)


def test_queued_synthesis_and_normalise_feed_the_limiter_in_stream_order():
    ctx = ctx_for("tiny")
    hop = ctx.hop
    cs = _ragged_case(4, 24, 43)
    host = ctx.synthesize(*cs, None, want_mel=False)
    ml = host["mel_len"]
    rows = [host["wav"][b, :int(ml[b]) * hop] for b in range(4)]
    longest = int(ml.max()) * hop
    stride = longest + 13
    normed = ctx.normalize(rows, -12.0, peak_ceiling=0.0, max_gain_db=40.0)[0]        # the fetched rows, normalised with no peak ceiling
    nrows = [normed[b, :len(rows[b])] for b in range(4)]
    want, peak_w, gmin_w = ctx.limit(nrows, CEILING, 2.0)                              # ... and limited
    assert any(g < 1.0 for g in gmin_w), gmin_w                                        # the limiter does act on these rows
    dptr = ctx.dev_alloc(4 * stride * 4)
    try:
        ctx.dev_from_host(dptr, np.full((4, stride), SENTINEL32, np.uint32))
        ctx.synthesize(*cs, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True, native_rate=True)
        assert ctx.normalize_device(dptr, ml * hop, stride, -12.0, peak_ceiling=0.0, max_gain_db=40.0, no_sync=True) is None
        peak, gmin = ctx.limit_device(dptr, ml * hop, stride, CEILING, window_ms=2.0)  # at once: no sync in between
        got = ctx.dev_to_host(dptr, (4, stride), np.float32)
        assert same_bits(peak, peak_w) and same_bits(gmin, gmin_w)
        for b in range(4):
            assert same_bits(got[b, :len(rows[b])], want[b, :len(rows[b])]), b
            tail = got.view(np.uint32)[b, len(rows[b]):]       # the synthesis call's zeros up to the longest row, then what was there
            assert not tail[:longest - len(rows[b])].any() and np.all(tail[longest - len(rows[b]):] == SENTINEL32), b
        # the fully queued form: nothing comes back, the rows are the same after a sync
        ctx.synthesize(*cs, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True, native_rate=True)
        assert ctx.normalize_device(dptr, ml * hop, stride, -12.0, peak_ceiling=0.0, max_gain_db=40.0, no_sync=True) is None
        assert ctx.limit_device(dptr, ml * hop, stride, CEILING, window_ms=2.0, no_sync=True) is None
        ctx.sync()
        assert same_bits(ctx.dev_to_host(dptr, (4, stride), np.float32), got)
    finally:
        ctx.dev_free(dptr)


def test_limiter_errors_leave_the_context_usable():
    ctx = ctx_for("tiny")
    cs = _ragged_case(2, 16, 7)
    before = ctx.synthesize(*cs, None, want_mel=False)
    fs = 22050
    rng = np.random.default_rng(2)
    rows = [(rng.standard_normal(k) * 0.7).astype(np.float32) for k in (3001, 1500, 0, 2048)]
    n = np.array([len(r) for r in rows], np.int32)
    B, Nmax = len(rows), 3001
    x = np.full((B, Nmax), SENTINEL32, np.uint32).view(np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    inv, uns = _lib.ZVX_E_INVALID, _lib.ZVX_E_UNSUPPORTED
    out = np.zeros((B, Nmax), np.float32)
    prm = params()
    lib, h = ctx._lib, ctx._h
    nan, inf = float("nan"), float("inf")

    def lim(x_=x, n_=n, B_=None, Nmax_=Nmax, rate=fs, prm_=prm, out_=out, stride=Nmax, flags=0):
        return raw_limit(ctx, x_, n_, Nmax_, rate, prm_, out_, stride, flags, B=B_)[0]

    def tpk(x_=x, n_=n, B_=None, Nmax_=Nmax, rate=fs, os_=4, flags=0, out_=True):
        return raw_true_peak(ctx, x_, n_, Nmax_, rate, os_, flags, B=B_, out=out_)[0]

    neg, big = n.copy(), n.copy()
    neg[1], big[1] = -1, Nmax + 1
    assert lib.zvx_true_peak(None, vp(x), vp(n), B, Nmax, fs, 4, vp(out), 0) == inv
    assert lib.zvx_limit(None, vp(x), vp(n), B, Nmax, fs, C.byref(prm), vp(out), Nmax, None, None, 0) == inv
    assert tpk(x_=None) == inv and lim(x_=None) == inv
    assert tpk(n_=None, B_=B) == inv and lim(n_=None, B_=B) == inv
    assert lim(prm_=None) == inv and lim(out_=None) == inv and tpk(out_=False) == inv
    assert tpk(B_=0) == inv and lim(B_=0) == inv and tpk(B_=-1) == inv and lim(B_=-1) == inv
    assert tpk(Nmax_=0) == inv and lim(Nmax_=0) == inv
    assert tpk(n_=neg) == inv and lim(n_=neg) == inv and tpk(n_=big) == inv and lim(n_=big) == inv
    assert lim(stride=Nmax - 1) == inv
    for rate in (3999, 192001, 0, -16000):
        assert tpk(rate=rate) == inv and lim(rate=rate) == inv, rate
    assert tpk(flags=64) == inv and lim(flags=64) == inv and lim(flags=_lib.ZVX_HOST_ASYNC) == inv and lim(flags=_lib.ZVX_NATIVE_RATE) == inv
    assert tpk(flags=_lib.ZVX_DEVICE_OUT) == inv and tpk(flags=_lib.ZVX_PCM16) == inv      # zvx_true_peak knows ZVX_DEVICE_IN only
    assert lim(flags=_lib.ZVX_NO_SYNC) == inv
    xf = np.array(x)                                       # a writable copy for the in-place forms
    assert lim(x_=xf, out_=xf, flags=_lib.ZVX_PCM16) == inv
    # in place: the stride is Nmax, and both pointers lie on the same side
    for kw in (dict(stride=Nmax + 2), dict(flags=_lib.ZVX_DEVICE_IN), dict(flags=_lib.ZVX_DEVICE_OUT)):
        assert lim(x_=xf, out_=xf, **kw) == inv and b"zvx_limit" in lib.zvx_last_error(h), kw
    for c in (nan, inf, -inf, 0.0, -0.5, 8.5):
        assert lim(prm_=params(ceiling=c)) == inv, c
    for ms in (nan, inf, -inf, 0.0, -1.0):
        assert lim(prm_=params(window_ms=ms)) == inv, ms
    for os_ in (0, 3, 16, -1):
        assert lim(prm_=params(oversample=os_)) == inv and tpk(os_=os_) == inv, os_
    assert b"oversample" in lib.zvx_last_error(h)
    assert lim(prm_=params(window_ms=4097 * 1000.0 / fs)) == uns
    big_n = np.zeros(65536, np.int32)
    assert lim(n_=big_n, x_=np.zeros((65536, 1), np.float32), Nmax_=1, out_=np.zeros((65536, 1), np.float32), stride=1) == uns
    assert tpk(n_=big_n, x_=np.zeros((65536, 1), np.float32), Nmax_=1, out_=True) == uns
    # the limits of the valid ranges are accepted, and the context still works
    assert lim(prm_=params(window_ms=ms_for(fs, 4096))) == 0 and lim(prm_=params(ceiling=8.0)) == 0
    assert lim(rate=4000) == 0 and lim(rate=192000, prm_=params(window_ms=1.0)) == 0 and tpk(rate=4000) == 0 and tpk(rate=192000) == 0
    rc, _, gmin = raw_limit(ctx, xf, n, Nmax, fs, params(window_ms=1.0), xf, Nmax)       # in place on host rows
    assert rc == 0
    for b in range(B):
        r = L.limit(rows[b], CEILING, 22, 4)
        check_row(x[b, :n[b]], xf[b, :n[b]], r, 22, ("in place on the host", b))
        assert np.all(xf.view(np.uint32)[b, n[b]:] == SENTINEL32), b
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert same_bits(after["wav"], before["wav"]) and np.array_equal(after["mel_len"], before["mel_len"])


def test_limiter_accounting_and_nothing_else_moved():
    ctx = ctx_for("tiny")
    cs = _ragged_case(3, 20, 41)
    before = ctx.synthesize(*cs, None, want_mel=False)
    rows = make_case(1, 22)[0]
    total = float(sum(len(r) for r in rows))
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.true_peak(rows, 4, rate=22050)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.limit"]["launches"] == 1 and tags["post.limit"]["bytes"] == 4.0 * total        # one timed group per call
        ms_peak = tags["post.limit"]["ms"]
        ctx.reset_stats()
        ctx.limit(rows, CEILING, 5.0, 4, rate=22050)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.limit"]["launches"] == 1 and tags["post.limit"]["bytes"] == 8.0 * total
        ms_limit = tags["post.limit"]["ms"]
        ctx.reset_stats()
        ctx.limit(rows, CEILING, 5.0, 1, pcm16=True, rate=22050)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.limit"]["launches"] == 1 and tags["post.limit"]["bytes"] == 6.0 * total
        assert "post.loudness" not in tags and "post.join" not in tags and ms_peak > 0 and ms_limit > 0
        assert set(ctx.stage_times()) == set(_lib.STAGES) and _lib.ZVX_T_COUNT == 8
        print(f"post.limit on {len(rows)} rows / {int(total)} samples at 22050 Hz: true peak {ms_peak:.3f} ms, limiter (W 110, os 4) {ms_limit:.3f} ms")
    finally:
        ctx.set_int("profile", 0)
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert same_bits(after["wav"], before["wav"]) and np.array_equal(after["mel_len"], before["mel_len"])


THREE = "The quick brown fox jumps over the lazy dog; does it, really? Pack my box with five dozen liquor jugs"


def test_tts_and_tts_long_with_the_limiter():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    fs, target, W = 22050, -16.0, 110
    ceiling = float(10.0 ** (-1.0 / 20.0))
    c32 = np.float32(ceiling)
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    kw = dict(trim_db=0.0, fade_ms=0, pauses={".": 0, ";": 0, ",": 0, " ": 0})

    def check(x, got, what, c=ceiling):
        r = L.limit(x, c, W, 4)
        err = np.abs(got.astype(np.float64) - r["out"].astype(np.float64))
        bound = np.abs(x.astype(np.float64)) * (r["E"] / float(np.float32(c)) + 2.0 ** -22)
        assert np.all(err <= bound), (what, float(np.max(err - bound)))
        assert np.all(np.abs(got) <= np.float32(c)), what
        return r

    plain, seg0 = synth.tts_long(THREE, spk, **kw)
    assert len(seg0) == 3 and all("min_gain" not in s for s in seg0)
    rows = [plain[s["start"]:s["start"] + s["samples"]] for s in seg0]
    m = R.measure(rows, fs)
    # tts_long: the paragraph's gain without a peak ceiling, then every row limited on its own
    wav, seg = synth.tts_long(THREE, spk, loudness=target, limiter=True, **kw)
    assert [(s["start"], s["samples"]) for s in seg] == [(s["start"], s["samples"]) for s in seg0]
    want = R.gains(m, target, 0.0, 20.0, common=True)[0]
    for i, s in enumerate(seg):
        g = np.float32(s["gain"])
        assert within_one_ulp([g], [want[i]]), (i, s["gain"], want[i])
        r = check(rows[i] * g, wav[s["start"]:s["start"] + s["samples"]], ("tts_long", i))
        assert abs(s["min_gain"] - float(r["g32"].min())) <= float(r["E"].max()) / float(c32) + 2.0 ** -22, (i, s["min_gain"])
        print(f"sentence {i}: gain {float(g):.4f}, peak after the gain {float(np.abs(rows[i] * g).max()):.4f}, limiter's smallest gain {s['min_gain']:.4f}")
    # limiter alone: no loudness keys, the rows limited as they are
    wav_l, seg_l = synth.tts_long(THREE, spk, limiter=True, peak_db=-20.0, **kw)
    assert all("gain" not in s and "min_gain" in s for s in seg_l)
    for i, s in enumerate(seg_l):                         # (at -20 dBFS the limiter does act)
        check(rows[i], wav_l[s["start"]:s["start"] + s["samples"]], ("tts_long, limiter alone", i), 10.0 ** (-20.0 / 20.0))
        assert s["min_gain"] < 1.0, (i, s["min_gain"])
    # tts: gain without a peak ceiling, limiter behind it; the plain call and limiter=False are untouched by the feature
    one, ph, length = synth.tts(seg0[0]["text"], spk)
    loud, ph2, length2 = synth.tts(seg0[0]["text"], spk, loudness=target, limiter=True)
    info, lim = synth.last_loudness, synth.last_limit
    assert length2 == length and np.array_equal(ph, ph2) and loud.dtype == np.float32
    m1 = R.measure([one], fs)
    assert within_one_ulp([info["gain"]], [R.gains(m1, target, 0.0, 20.0)[0][0]])
    r = check(one * np.float32(info["gain"]), loud, "tts")
    assert set(lim) == {"peak_in", "min_gain"} and abs(lim["min_gain"] - float(r["g32"].min())) <= float(r["E"].max()) / float(c32) + 2.0 ** -22
    reached = R.measure([loud], fs)["lufs"][0]
    print(f"tts: {m1['lufs'][0]:.3f} LUFS, gain {info['gain']:.4f}, envelope peak {lim['peak_in']:.4f}, smallest gain {lim['min_gain']:.4f} -> {reached:.3f} LUFS")
    hot = synth.tts(seg0[0]["text"], spk, loudness=-8.0, limiter=True)[0]              # a target the peaks do not allow: the limiter acts
    assert within_one_ulp([synth.last_loudness["gain"]], [R.gains(m1, -8.0, 0.0, 20.0)[0][0]]) and synth.last_limit["min_gain"] < 1.0
    check(one * np.float32(synth.last_loudness["gain"]), hot, "tts at -8 LUFS")
    print(f"tts at -8 LUFS: gain {synth.last_loudness['gain']:.4f}, smallest gain {synth.last_limit['min_gain']:.4f} -> {R.measure([hot], fs)['lufs'][0]:.3f} LUFS")
    off = synth.tts(seg0[0]["text"], spk, loudness=target, limiter=False)[0]
    g_off = np.float32(synth.last_loudness["gain"])
    assert within_one_ulp([g_off], [R.gains(m1, target, ceiling, 20.0)[0][0]]) and same_bits(off, one * g_off)
    assert same_bits(synth.tts(seg0[0]["text"], spk)[0], one)
    only = synth.tts(seg0[0]["text"], spk, limiter=True, peak_db=-20.0)[0]             # limiter without loudness just limits
    assert np.all(np.abs(only) <= np.float32(10.0 ** (-20.0 / 20.0))) and len(only) == len(one)
    # under an output rate the conversion follows the limiter: the delivered sample peak is a figure, not a promise
    synth.output_rate = 48000
    try:
        up = synth.tts(seg0[0]["text"], spk, loudness=target, limiter=True)[0]
        assert len(up) == _lib.resampled_len(len(one), fs, 48000)
        print(f"output_rate 48000: delivered sample peak {float(np.abs(up).max()):.5f} against the ceiling {ceiling:.5f} "
              f"({20.0 * np.log10(max(float(np.abs(up).max()), 1e-30) / ceiling):+.4f} dB)")
    finally:
        synth.output_rate = None
    with pytest.raises(ValueError):
        synth.tts_stream(seg0[0]["text"], spk, limiter=True)
    synth.model.close()
