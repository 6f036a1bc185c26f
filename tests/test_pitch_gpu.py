"""The pitch report on the MI355X: zvx_pitch against tests/pitch_ref.py (the float64 restatement of include/zvx.h's block; never the
library) at the smallest shapes that exercise the kernel's cuts -- fewer lags than lanes (tau_max = 100), two, four and eight lags per lane
(368, 800, 1600, 2048), runs of G frames that do not divide F, frames whose window runs past either end of the row, rows without a frame --,
the independence of rows, a row with a NaN, the refusals, the accounting, and ZeroVoxTTS.pitch_report / tts(..., pitch_report=True).
Every parity test first asserts, from the reference alone, that none of its frames is AMBIGUOUS."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pitch_ref as R
from stream_util import _ragged_case, err, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

# The largest relative deviation of f0 and aper from the float64 reference over the rows of test_parity_on_the_ragged_batch, measured on an
# MI355X, and the bound held: four times that, not less than one f32 ulp.  Measured: 0 -- every f0 and aper of these rows, and of the rows
# of test_lag_tilings, has the bits of the reference's (both round the same doubles, up to the summation order, once to f32).
MEASURED = 0.0
TOL = max(4.0 * MEASURED, 6e-8)
SENTINEL = np.float32(-12345.0)
_ctx, _ref = {}, {}


def ctx_for(voc="tiny", prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def pad_rows(rows, extra=1):
    """-> (x [B][Nmax] padded with a large value nothing may read, n)"""
    n = np.array([len(r) for r in rows], np.int32)
    x = np.full((len(rows), int(n.max()) + extra), 1e30, np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def case8k():
    """the ragged 8 kHz batch (names, rows, x, n, the reference's tracks), computed once, left unchanged"""
    if "8k" not in _ref:
        rows, _ = R.rows_8k()
        names = list(rows)
        x, n = pad_rows([rows[k] for k in names])
        ref = [R.track(rows[k], **R.P8K) for k in names]
        for a in (x, n):
            a.setflags(write=False)
        _ref["8k"] = (names, [rows[k] for k in names], x, n, ref)
    return _ref["8k"]


def params(rate, fmin=60.0, fmax=500.0, threshold=0.15, gate_db=-60.0, window=None, hop=None):
    tmin, tmax, W, c = R.geometry(rate, fmin, fmax, window)
    return _lib.PitchParams(fmin, fmax, threshold, gate_db, W, max(1, rate // 100) if hop is None else hop)


def raw(ctx, x, n, Nmax, rate, prm, flags=0, f0=None, aper=None, stride=0, frames=None, B=None, want_stats=True, want_params=True):
    import ctypes as C
    B = len(n) if B is None else B
    stats = np.full((max(B, 1), _lib.ZVX_PS_COUNT), 7.0, np.float64)
    rc = ctx._lib.zvx_pitch(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if want_params else None, vp(f0), vp(aper), stride, vp(frames),
                            vp(stats) if want_stats else None, flags)
    return rc, stats


def curves_call(ctx, x, n, rate, prm, flags=0, Nmax=None, extra=3):
    """the call with both curves in sentinel-filled arrays -> (stats, f0, aper, frames)"""
    B = len(n)
    Nmax = x.shape[1] if Nmax is None else Nmax
    stride = max(1, Nmax // prm.hop) + extra
    f0, ap = np.full((B, stride), SENTINEL, np.float32), np.full((B, stride), SENTINEL, np.float32)
    fr = np.full(B, -1, np.int32)
    rc, stats = raw(ctx, x, n, Nmax, rate, prm, flags=flags, f0=f0, aper=ap, stride=stride, frames=fr)
    assert rc == 0, err(ctx)
    return stats, f0, ap, fr


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rel_dev(got, want):
    """the largest relative deviation of f32 values from the reference's (where the reference is 0 the value has to be 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0.0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if (~zero).any() else 0.0


def assert_parity(what, stats, f0, ap, fr, n, refs, hop):
    """frames exact, decisions equal, curves within TOL, nothing written past F, the statistics those of the device's own track"""
    worst = 0.0
    for b, r in enumerate(refs):
        assert r["ambiguous"] == [], (what, b, r["ambiguous"])              # from the reference alone
        F = int(n[b]) // hop
        assert fr[b] == F == r["frames"] and stats[b, _lib.ZVX_PS_FRAMES] == F, (what, b)
        assert np.all(f0[b, F:] == SENTINEL) and np.all(ap[b, F:] == SENTINEL), (what, b)
        assert np.array_equal(f0[b, :F] > 0, r["f0"] > 0), (what, b, np.flatnonzero((f0[b, :F] > 0) != (r["f0"] > 0)))
        df, da = rel_dev(f0[b, :F], r["f0"]), rel_dev(ap[b, :F], r["aper"])
        print(f"{what} row {b}: {F} frames, {int((r['f0'] > 0).sum())} voiced, relative deviation f0 {df:.3e} aper {da:.3e}")
        worst = max(worst, df, da)
        s = R.stats(f0[b, :F])                               # of the DEVICE's track
        assert stats[b, _lib.ZVX_PS_VOICED] == s["voiced"] == int((r["f0"] > 0).sum()), (what, b)
        assert (stats[b, _lib.ZVX_PS_MEDIAN], stats[b, _lib.ZVX_PS_LOW], stats[b, _lib.ZVX_PS_HIGH]) == (s["median"], s["low"], s["high"]), (what, b)
        assert abs(stats[b, _lib.ZVX_PS_MEAN] - s["mean"]) <= 1e-12 * abs(s["mean"]), (what, b, stats[b, _lib.ZVX_PS_MEAN], s["mean"])
    print(f"{what}: worst relative deviation from the float64 reference {worst:.3e} (held: {TOL:.1e})")
    assert worst <= TOL, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------ 1. against the reference
def test_parity_on_the_ragged_batch():
    """every 8 kHz row of tests/test_pitch.py in ONE ragged batch -- the three harmonic rows, the strong second harmonic, noise, silence,
    the row under the gate and the glide (lengths 2400 and 4000), then a row of 79 samples (F = 0) and an empty one: ten rows --;
    tau_max = 100: fewer lags than lanes.  Measured on an MI355X: see MEASURED."""
    ctx = ctx_for()
    names, rows, x, n, refs = case8k()
    assert sorted(set(n.tolist())) == [0, 79, 2400, 4000] and len(names) >= 8
    prm = params(**R.P8K)
    stats, f0, ap, fr = curves_call(ctx, x, n, 8000, prm)
    worst = assert_parity("8 kHz batch", stats, f0, ap, fr, n, refs, 80)
    assert worst <= 1e-5                                     # beyond that a sum is wrong, not a tolerance too tight
    # the binding: the same bits, each row's own frames
    res = ctx.pitch(rows, rate=8000, fmin=80.0, fmax=400.0, window=200, hop=80)
    for b in range(len(rows)):
        assert np.array_equal(u32(res["f0"][b]), u32(f0[b, :fr[b]])) and np.array_equal(u32(res["aper"][b]), u32(ap[b, :fr[b]])), b
    assert np.array_equal(res["frames"], fr) and all(np.array_equal(u64(res[k]), u64(stats[:, i])) for i, k in enumerate(_lib.PITCH_STATS_KEYS) if i)


# ------------------------------------------------------------------------------------------------ 2. lag tilings
TILINGS = {
    # name: (rate, keywords, the row) -- lags per lane, frames per workgroup G and frames F
    "two lags per lane": (22050, dict(hop=256), lambda: R.harmonic(120.0, 11025, 22050)),                       # tau_max 368, W 736; G 8, F 43
    "four lags per lane": (48000, dict(), lambda: R.harmonic(120.0, 4800, 48000)),                              # tau_max 800, W 1600; G 8, F 10
    "eight lags per lane": (48000, dict(fmin=30.0, hop=672), lambda: R.harmonic(90.0, 7200, 48000)),            # tau_max 1600, W 3200; G 3, F 10
    "the caps": (48000, dict(fmin=23.4375, window=4096, hop=2400), lambda: R.harmonic(70.0, 9600, 48000)),     # tau_max 2048, W 4096; G 1, F 4
}


@pytest.mark.parametrize("name", list(TILINGS))
def test_lag_tilings(name):
    ctx = ctx_for()
    rate, kw, make = TILINGS[name]
    row = make()
    prm = params(rate, **kw)
    ref = R.track(row, rate, window=prm.window, hop=prm.hop, **{k: v for k, v in kw.items() if k in ("fmin", "fmax")})
    assert (ref["f0"] > 0).any()
    F = ref["frames"]
    tmin, tmax, W, c = R.geometry(rate, prm.fmin, prm.fmax, prm.window)
    assert (F - 1) * prm.hop - c + W + tmax > len(row) and -c < 0           # the last frame's window runs past n, the first one's starts before 0
    x, n = pad_rows([row], extra=5)
    stats, f0, ap, fr = curves_call(ctx, x, n, rate, prm)
    assert_parity(name, stats, f0, ap, fr, n, [ref], prm.hop)


# ------------------------------------------------------------------------------------------------ 3. independence
def test_rows_are_independent_and_curves_touch_nothing_else():
    ctx = ctx_for()
    names, rows, x, n, refs = case8k()
    B, Nmax = x.shape
    prm = params(**R.P8K)
    stats, f0, ap, fr = curves_call(ctx, x, n, 8000, prm)
    # no curves, one curve: the same figures, and an array not asked for is not written
    rc, st0 = raw(ctx, x, n, Nmax, 8000, prm, stride=-5)                    # no curve: the stride is not looked at
    assert rc == 0 and np.array_equal(u64(st0), u64(stats))
    only = np.full_like(f0, SENTINEL)
    rc, st1 = raw(ctx, x, n, Nmax, 8000, prm, f0=only, stride=only.shape[1])
    assert rc == 0 and np.array_equal(u64(st1), u64(stats)) and np.array_equal(u32(only), u32(f0))
    res = ctx.pitch(x, rate=8000, fmin=80.0, fmax=400.0, window=200, hop=80, lengths=n, curves=False)
    assert "f0" not in res and all(np.array_equal(u64(res[k]), u64(stats[:, i])) for i, k in enumerate(_lib.PITCH_STATS_KEYS) if i)
    # every row alone, and alone under another Nmax
    for b in range(B):
        F = fr[b]
        s1, f1, a1, r1 = curves_call(ctx, np.ascontiguousarray(x[b:b + 1]), n[b:b + 1], 8000, prm)
        assert r1[0] == F and np.array_equal(u64(s1[0]), u64(stats[b])), names[b]
        assert np.array_equal(u32(f1[0, :F]), u32(f0[b, :F])) and np.array_equal(u32(a1[0, :F]), u32(ap[b, :F])), names[b]
        wide = np.full((1, Nmax + 4099), 1e30, np.float32)
        wide[0, :n[b]] = x[b, :n[b]]
        s1, f1, a1, r1 = curves_call(ctx, wide, n[b:b + 1], 8000, prm)
        assert np.array_equal(u64(s1[0]), u64(stats[b])) and np.array_equal(u32(f1[0, :F]), u32(f0[b, :F])) and np.array_equal(u32(a1[0, :F]), u32(ap[b, :F]))
        assert np.all(f1[0, F:] == SENTINEL) and np.all(a1[0, F:] == SENTINEL)
    # device input, one float off a 16-byte boundary
    xin = ctx.dev_alloc(x.nbytes + 16)
    try:
        ctx.dev_from_host(xin + 4, x)
        sd, fd, ad, rd = curves_call(ctx, xin + 4, n, 8000, prm, flags=_lib.ZVX_DEVICE_IN, Nmax=Nmax)
        assert np.array_equal(u64(sd), u64(stats)) and np.array_equal(u32(fd), u32(f0)) and np.array_equal(u32(ad), u32(ap)) and np.array_equal(rd, fr)
        res = ctx.pitch_device(xin + 4, n, Nmax, rate=8000, fmin=80.0, fmax=400.0, window=200, hop=80)
        assert all(np.array_equal(u32(res["f0"][b]), u32(f0[b, :fr[b]])) for b in range(B))
    finally:
        ctx.dev_free(xin)


# ------------------------------------------------------------------------------------------------ 4. a row with a NaN
def test_a_row_with_a_nan_leaves_the_others_alone():
    ctx = ctx_for()
    names, rows, x, n, refs = case8k()
    prm = params(**R.P8K)
    stats, f0, ap, fr = curves_call(ctx, x, n, 8000, prm)
    bad = x.copy()
    b_nan = names.index("h155")
    bad[b_nan, 1000] = np.nan
    bad[b_nan, 1700] = np.inf
    s2, f2, a2, r2 = curves_call(ctx, bad, n, 8000, prm)
    assert np.array_equal(r2, fr)
    for b in range(len(names)):
        if b != b_nan:
            assert np.array_equal(u64(s2[b]), u64(stats[b])) and np.array_equal(u32(f2[b]), u32(f0[b])) and np.array_equal(u32(a2[b]), u32(ap[b])), names[b]
    assert np.all(np.isfinite(f2[b_nan, :fr[b_nan]])) and s2[b_nan, _lib.ZVX_PS_FRAMES] == fr[b_nan]       # unspecified, but nothing faults and f0 stays a number


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_errors_name_their_argument_and_leave_the_context_usable():
    ctx = ctx_for()
    names, rows, x, n, refs = case8k()
    B, Nmax = x.shape
    good_p = params(**R.P8K)
    rc, good = raw(ctx, x, n, Nmax, 8000, good_p)
    assert rc == 0, err(ctx)
    need = max(1, Nmax // 80)
    curve = np.full((B, need), SENTINEL, np.float32)
    bad_len, neg_len = n.copy(), n.copy()
    bad_len[1], neg_len[2] = Nmax + 1, -1
    P = _lib.PitchParams
    nan, inf = float("nan"), float("inf")
    INV = _lib.ZVX_E_INVALID
    calls = [
        ("NULL in", b"NULL pointer", lambda: raw(ctx, None, n, Nmax, 8000, good_p)),
        ("NULL nsamples", b"NULL pointer", lambda: raw(ctx, x, None, Nmax, 8000, good_p, B=B)),
        ("B = 0", b"B = 0", lambda: raw(ctx, x, n, Nmax, 8000, good_p, B=0)),
        ("Nmax = 0", b"Nmax = 0", lambda: raw(ctx, x, n, 0, 8000, good_p)),
        ("a length over Nmax", b"nsamples[1]", lambda: raw(ctx, x, bad_len, Nmax, 8000, good_p)),
        ("a negative length", b"nsamples[2]", lambda: raw(ctx, x, neg_len, Nmax, 8000, good_p)),
        ("rate 3999", b"rate 3999", lambda: raw(ctx, x, n, Nmax, 3999, good_p)),
        ("rate 192001", b"rate 192001", lambda: raw(ctx, x, n, Nmax, 192001, good_p)),
        ("ZVX_DEVICE_OUT", b"flag", lambda: raw(ctx, x, n, Nmax, 8000, good_p, flags=_lib.ZVX_DEVICE_OUT)),
        ("ZVX_PCM16", b"flag", lambda: raw(ctx, x, n, Nmax, 8000, good_p, flags=_lib.ZVX_PCM16)),
        ("an unknown flag", b"flag", lambda: raw(ctx, x, n, Nmax, 8000, good_p, flags=1 << 20)),
        ("NULL params", b"params", lambda: raw(ctx, x, n, Nmax, 8000, good_p, want_params=False)),
        ("NULL stats", b"stats", lambda: raw(ctx, x, n, Nmax, 8000, good_p, want_stats=False)),
        ("fmin NaN", b"fmin", lambda: raw(ctx, x, n, Nmax, 8000, P(nan, 400.0, 0.15, -60.0, 200, 80))),
        ("fmin 0", b"fmin", lambda: raw(ctx, x, n, Nmax, 8000, P(0.0, 400.0, 0.15, -60.0, 200, 80))),
        ("fmax inf", b"fmax", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, inf, 0.15, -60.0, 200, 80))),
        ("fmax <= fmin", b"fmax", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 80.0, 0.15, -60.0, 200, 80))),
        ("threshold 0", b"threshold", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.0, -60.0, 200, 80))),
        ("threshold over 1", b"threshold", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 1.001, -60.0, 200, 80))),
        ("threshold NaN", b"threshold", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, nan, -60.0, 200, 80))),
        ("gate_db positive", b"gate_db", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.15, 0.5, 200, 80))),
        ("gate_db -inf", b"gate_db", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.15, -inf, 200, 80))),
        ("tau_max < tau_min + 2", b"tau_max", lambda: raw(ctx, x, n, Nmax, 8000, P(399.0, 400.0, 0.15, -60.0, 200, 80))),
        ("window 1", b"window", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.15, -60.0, 1, 80))),
        ("hop 0", b"hop", lambda: raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.15, -60.0, 200, 0))),
        ("f_stride too small, f0", b"f_stride", lambda: raw(ctx, x, n, Nmax, 8000, good_p, f0=curve, stride=need - 1)),
        ("f_stride too small, aper", b"f_stride", lambda: raw(ctx, x, n, Nmax, 8000, good_p, aper=curve, stride=need - 1)),
        ("f_stride negative", b"f_stride", lambda: raw(ctx, x, n, Nmax, 8000, good_p, f0=curve, aper=curve, stride=-1)),
    ]
    for what, word, call in calls:
        rc, st = call()
        assert rc == INV and word in err(ctx), (what, rc, err(ctx))
        assert np.all(st == 7.0) and np.all(curve == SENTINEL), what         # nothing was written
    # the caps: one past each is refused, the caps themselves run (test_lag_tilings, "the caps")
    UNS = _lib.ZVX_E_UNSUPPORTED
    assert (_lib.PITCH_MAX_WINDOW, _lib.PITCH_MAX_TAU, _lib.PITCH_MAX_FRAMES) == (4096, 2048, 65536)
    rc, st = raw(ctx, x, n, Nmax, 8000, P(80.0, 400.0, 0.15, -60.0, 4097, 80))
    assert rc == UNS and b"window 4097" in err(ctx) and np.all(st == 7.0), (rc, err(ctx))
    rc, st = raw(ctx, x, n, Nmax, 48000, P(23.43, 500.0, 0.15, -60.0, 4096, 480))       # ceil(48000 / 23.43) = 2049
    assert rc == UNS and b"tau_max 2049" in err(ctx) and np.all(st == 7.0), (rc, err(ctx))
    long_n = _lib.PITCH_MAX_FRAMES + 1                       # 65537 frames of one sample (refused before anything is read)
    zeros = np.zeros((1, long_n), np.float32)
    rc, st = raw(ctx, zeros, np.array([long_n], np.int32), long_n, 8000, P(80.0, 400.0, 0.15, -60.0, 200, 1))
    assert rc == UNS and b"65536" in err(ctx) and np.all(st == 7.0), (rc, err(ctx))
    with pytest.raises(_lib.ZvxError) as e:
        ctx.pitch(zeros, rate=8000, lengths=[long_n], hop=1)
    assert e.value.code == UNS
    rc, st = raw(ctx, x, np.zeros(65536, np.int32), Nmax, 8000, good_p, B=65536)       # more than 65535 rows
    assert rc == UNS and b"65536 rows" in err(ctx), (rc, err(ctx))
    rc, again = raw(ctx, x, n, Nmax, 8000, good_p)
    assert rc == 0 and np.array_equal(u64(again), u64(good))


# ------------------------------------------------------------------------------------------------ 6. accounting
def test_accounting_and_nothing_else_moved():
    ctx = ctx_for()
    cs = _ragged_case(3, 20, 41)
    before = ctx.synthesize(*cs, None, want_mel=False)
    names, rows, x, n, refs = case8k()
    total = float(n.astype(np.int64).sum())
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.pitch(rows, rate=8000, fmin=80.0, fmax=400.0, window=200, hop=80)
        tags = {t["name"]: t for t in ctx.tag_stats() if t["launches"]}
        assert set(tags) == {"post.pitch"}, sorted(tags)                      # no other tag moved
        assert tags["post.pitch"]["launches"] == 1 and tags["post.pitch"]["bytes"] == 4.0 * total and tags["post.pitch"]["ms"] > 0
        ctx.pitch(rows, rate=8000, curves=False)
        assert {t["name"]: t for t in ctx.tag_stats()}["post.pitch"]["launches"] == 2
        print(f"post.pitch on {len(rows)} rows / {int(total)} samples at 8000 Hz: {tags['post.pitch']['ms']:.3f} ms")
    finally:
        ctx.set_int("profile", 0)
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert np.array_equal(after["wav"].view(np.uint32), before["wav"].view(np.uint32)) and np.array_equal(after["mel_len"], before["mel_len"])


# ------------------------------------------------------------------------------------------------ 7. through the model
def test_pitch_report_through_the_model():
    from zerovox_amd.pitch import PitchReport, cents
    from zerovox_amd.report import LoudnessReport
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    fs = synth.output_rate
    assert synth.last_pitch_report is None
    rep = synth.pitch_report(R.harmonic(120.0, fs // 2, fs))
    assert isinstance(rep, PitchReport) and synth.last_pitch_report is rep
    hop = synth.model.ctx.hop
    print(f"pitch report of a 120 Hz row at {fs} Hz: {rep}")
    assert rep.frames == (fs // 2) // hop == len(rep.f0) == len(rep.aper)    # the model's hop: a frame is a mel frame
    assert abs(cents(rep.median_hz, 120.0)) <= 2.0 and rep.voiced_fraction > 0.9
    assert rep.low_hz <= rep.median_hz <= rep.high_hz and rep.range_semitones >= 0.0
    as16 = synth.pitch_report((R.harmonic(120.0, fs // 2, fs, scale=0.5) * 32760.0).astype(np.int16))       # int16 PCM is read as what it encodes
    assert abs(cents(as16.median_hz, 120.0)) <= 2.0
    other = synth.pitch_report(R.harmonic(100.0, 2400, 8000), 8000, fmin=80.0, fmax=400.0, window=200, hop=80)
    ref = R.track(R.harmonic(100.0, 2400, 8000), **R.P8K)
    assert other.frames == 30 and np.array_equal(other.f0 > 0, ref["f0"] > 0)
    # tts: the keyword measures the delivered waveform and changes nothing else
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    text = "The quick brown fox jumps over the lazy dog"
    synth._last_pitch_report = None
    before = synth.tts(text, spk)[0]
    assert synth.last_pitch_report is None                   # nothing is measured unless asked for
    wav, _, length = synth.tts(text, spk, pitch_report=True)
    got = synth.last_pitch_report
    assert isinstance(got, PitchReport) and got.frames == len(wav) // hop == length
    assert np.array_equal(wav.view(np.uint32), before.view(np.uint32))
    assert got == synth.pitch_report(wav) and np.array_equal(u32(got.f0), u32(synth.last_pitch_report.f0))
    after = synth.tts(text, spk)[0]
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    # an empty dict of keywords asks for the defaults, through tts as through tts_ex; a request with nothing to measure leaves no old report
    synth._last_pitch_report = None
    synth.tts(text, spk, pitch_report={})
    assert synth.last_pitch_report == got
    synth._last_pitch_report = None
    synth.tts_ex(text, spk, pitch_report={})
    assert synth.last_pitch_report == got
    synth.tts("", spk, pitch_report=True)
    assert synth.last_pitch_report is None
    # the loudness report stays what it is, with and without the new keyword
    synth.tts(text, spk, report=True)
    loud = synth.last_report
    assert isinstance(loud, LoudnessReport)
    both = synth.tts(text, spk, report=True, pitch_report=dict(fmin=80.0, fmax=400.0))[0]
    assert synth.last_report == loud and np.array_equal(both.view(np.uint32), before.view(np.uint32))
    assert synth.last_pitch_report.frames == got.frames
    # tts_long measures the joined waveform
    plain, seg0 = synth.tts_long(text + ". Pack my box with five dozen liquor jugs.", spk)
    joined, seg = synth.tts_long(text + ". Pack my box with five dozen liquor jugs.", spk, pitch_report=True)
    assert np.array_equal(joined.view(np.uint32), plain.view(np.uint32)) and synth.last_pitch_report.frames == len(joined) // hop
