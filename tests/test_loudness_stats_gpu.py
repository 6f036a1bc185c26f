"""The programme loudness report on the MI355X: zvx_loudness_stats against tests/loudness_stats_ref.py (scipy.signal.lfilter in float64 with
carried state, gates in the power domain; never the library) at the smallest shapes at which its two kernels can still go wrong -- more
short-term windows than one workgroup of the selection holds (371, 971), none (U = 29), exactly one (U = 30), an empty row --, the bits it
shares with zvx_loudness, ties, the independence of rows, the refusals, the accounting, and tts_long(..., report=True) end to end.
include/zvx.h defines every figure to within 1e-7 LU outside an ambiguity band of 1e-3 LU around either gate; every parity test first
asserts, from the reference alone, that no window of its rows lies within 0.01 LU of a gate."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import loudness_ref as R
import loudness_stats_ref as S
from stream_util import _ragged_case, err, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

TOL = 1e-7
MARGIN = 0.01                                              # ten times the ambiguity band (tests/test_loudness_gpu.py)
SENTINEL = -12345.0
_ctx, _ref = {}, {}


def ctx_for(voc="tiny", prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def burst_row(seed, n, fs):
    """noise in bursts of 0.3 .. 1.2 s at levels between -55 and -10 dBFS: windows on either side of the relative gate"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    at = 0
    while at < n:
        k = int(rng.uniform(0.3, 1.2) * fs)
        x[at:at + k] *= 10.0 ** (rng.uniform(-55.0, -10.0) / 20.0)
        at += k
    return x.astype(np.float32)


# seeds for which, by the reference alone, every row keeps MARGIN to every gate (checked on the CPU)
BURST_SEEDS = {8000: (0, 1, 3, 2, 0, 7), 22050: (0, 1, 3, 2, 4, 6)}
BURST_SECONDS = (3.0, 3.15, 4.7, 6.33, 9.1, 12.9)


def rows_for(name):
    if name == "sines":
        fs = 4000
        h = R.unit_len(fs)
        rows = [S.sine_segments(fs, S.TECH3342[1][0]), S.sine_segments(fs, S.TECH3342[4][0]), burst_row(100, 29 * h + 7, fs),
                burst_row(101, 30 * h, fs), np.zeros(0, np.float32)]
        assert [len(r) // h for r in rows] == [400, 1000, 29, 30, 0]
        return fs, rows
    fs = int(name)
    return fs, [burst_row(s, int(sec * fs) + 3 * i, fs) for i, (s, sec) in enumerate(zip(BURST_SEEDS[fs], BURST_SECONDS))]


def case(name):
    """(fs, rows, x [B][Nmax] padded with a large value nothing may read, n, the reference's measurement), computed once, left unchanged"""
    if name not in _ref:
        fs, rows = rows_for(name)
        n = np.array([len(r) for r in rows], np.int32)
        x = np.full((len(rows), int(n.max()) + 1), 1e30, np.float32)
        for b, r in enumerate(rows):
            x[b, :n[b]] = r
        m = S.measure(rows, fs)
        for a in (x, n):
            a.setflags(write=False)
        _ref[name] = (fs, rows, x, n, m)
    return _ref[name]


def raw_stats(ctx, x, n, Nmax, rate, flags=0, mom=None, sht=None, stride=0, B=None, want_stats=True):
    B = len(n) if B is None else B
    stats = np.full((max(B, 1), _lib.ZVX_LS_COUNT), 7.0, np.float64)
    rc = ctx._lib.zvx_loudness_stats(ctx._h, vp(x), vp(n), B, Nmax, rate, vp(stats) if want_stats else None, vp(mom), vp(sht), stride, flags)
    return rc, stats


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def close(got, want):
    """within TOL, infinities equal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    inf = ~np.isfinite(want)
    return bool(np.array_equal(got[inf], want[inf]) and np.all(np.abs(got[~inf] - want[~inf]) <= TOL))


def assert_parity(res, m, rows, what):
    assert np.all(m["margin"] >= MARGIN) and np.all(m["int_margin"] >= MARGIN), (what, m["margin"], m["int_margin"])      # from the reference alone
    worst = 0.0
    for b in range(len(rows)):                              # every row, none exempted
        for k in S.KEYS:
            print(f"{what} row {b} ({len(rows[b])} samples) {k}: device {res[k][b]!r} reference {m[k][b]!r}")
            assert close(res[k][b], m[k][b]), (what, b, k, res[k][b], m[k][b])
            if np.isfinite(m[k][b]):
                worst = max(worst, abs(res[k][b] - m[k][b]))
        assert res["short_gated"][b] == m["short_gated"][b], (what, b)
        assert np.float32(res["peak"][b]) == np.float32(m["peak"][b]) and res["peak"][b] == float(np.float32(res["peak"][b])), (what, b)
        for k in ("momentary", "short_term"):
            assert close(res[k][b], m[k][b]), (what, b, k, len(res[k][b]), len(m[k][b]))
            assert res["max_" + k][b] == (res[k][b].max() if len(res[k][b]) else -np.inf), (what, b, k)      # the maximum is the curve's
    print(f"{what}: worst deviation from the float64 reference {worst:.3e} LU over {len(rows)} rows")


def test_parity_on_the_tech_3342_rows_and_the_short_rows():
    ctx = ctx_for()
    fs, rows, x, n, m = case("sines")
    assert [len(c) for c in m["short_term"]] == [371, 971, 0, 1, 0]      # the selection spans 2 and 4 workgroups; none; one window
    res = ctx.loudness_stats(rows, rate=fs, curves=True)
    assert_parity(res, m, rows, "4000 Hz")
    assert abs(res["lra"][0] - 10.0) < 5e-3 and abs(res["lra"][1] - 15.0) < 5e-3 and list(res["short_gated"][:2]) == [371.0, 627.0]
    assert res["lra"][3] == 0.0 and res["lra_low"][3] == res["lra_high"][3] and res["short_gated"][3] == 1.0
    assert close(res["lra_low"][3], res["max_short_term"][3])
    assert res["max_short_term"][2] == -np.inf and np.isfinite(res["max_momentary"][2]) and res["lra"][2] == 0.0
    assert [res[k][4] for k in S.KEYS] == [-np.inf, -np.inf, -np.inf, 0.0, -np.inf, -np.inf, 0.0, 0.0]


@pytest.mark.parametrize("fs", (8000, 22050))
def test_parity_on_ragged_noise_bursts(fs):
    ctx = ctx_for()
    fs, rows, x, n, m = case(str(fs))
    assert len({len(r) // R.unit_len(fs) for r in rows}) == len(rows) and min(len(c) for c in m["short_term"]) == 1
    assert np.any(m["short_gated"] < [len(c) for c in m["short_term"]])          # the relative gate removes windows somewhere
    res = ctx.loudness_stats(rows, rate=fs, curves=True)
    assert_parity(res, m, rows, f"{fs} Hz")


@pytest.mark.parametrize("name", ("sines", "8000", "22050"))
def test_integrated_and_peak_are_zvx_loudness_bits(name):
    ctx = ctx_for()
    fs, rows, x, n, m = case(name)
    lufs, peak = ctx.loudness(x, rate=fs, lengths=n)
    res = ctx.loudness_stats(x, rate=fs, lengths=n)
    assert np.array_equal(u64(res["integrated"]), u64(lufs)), (res["integrated"], lufs)
    assert np.array_equal(u64(res["peak"]), u64(peak.astype(np.float64)))


def test_ties_break_by_index():
    ctx = ctx_for()
    fs = 4000
    h = R.unit_len(fs)
    period = (np.random.default_rng(7).standard_normal(h) * 0.1).astype(np.float32)
    row = np.tile(period, 90)                                # U = 90, W = 61: every unit from q = 2 on walks identical samples
    m = S.measure([row], fs)
    res = ctx.loudness_stats([row], rate=fs, curves=True)
    s = res["short_term"][0]
    assert len(s) == 61 and len(np.unique(u64(s[2:]))) == 1                      # bit-identical windows: 59-fold ties at both ranks
    assert res["short_gated"][0] == 61.0 and res["lra"][0] == 0.0 and res["lra_low"][0] == res["lra_high"][0] and close(res["lra_low"][0], s[2])
    for k in S.KEYS:
        assert close(res[k][0], m[k][0]), (k, res[k][0], m[k][0])


def test_rows_are_independent_and_curves_touch_nothing_else():
    ctx = ctx_for()
    fs, rows, x, n, m = case("8000")
    B, Nmax = x.shape
    h = R.unit_len(fs)
    stride = Nmax // h - 3 + 5
    mom, sht = np.full((B, stride), SENTINEL), np.full((B, stride), SENTINEL)
    rc, stats = raw_stats(ctx, x, n, Nmax, fs, mom=mom, sht=sht, stride=stride)
    assert rc == 0, err(ctx)
    for b in range(B):
        U = n[b] // h
        assert np.all(mom[b, :U - 3] != SENTINEL) and np.all(mom[b, U - 3:] == SENTINEL), b      # nothing beyond U - 3 / U - 29
        assert np.all(sht[b, :U - 29] != SENTINEL) and np.all(sht[b, U - 29:] == SENTINEL), b
    # one curve alone, none: the same figures, and an array not asked for is not written
    mom2 = np.full((B, stride), SENTINEL)
    rc, st2 = raw_stats(ctx, x, n, Nmax, fs, mom=mom2, stride=stride)
    assert rc == 0 and np.array_equal(u64(st2), u64(stats)) and np.array_equal(u64(mom2), u64(mom))
    sht2 = np.full((B, stride), SENTINEL)
    rc, st2 = raw_stats(ctx, x, n, Nmax, fs, sht=sht2, stride=stride)
    assert rc == 0 and np.array_equal(u64(st2), u64(stats)) and np.array_equal(u64(sht2), u64(sht))
    rc, st0 = raw_stats(ctx, x, n, Nmax, fs, stride=-5)      # no curve: the stride is not looked at
    assert rc == 0 and np.array_equal(u64(st0), u64(stats))
    # every row alone, and alone under another Nmax
    for b in range(B):
        rc, one = raw_stats(ctx, np.ascontiguousarray(x[b:b + 1]), n[b:b + 1], Nmax, fs)
        assert rc == 0 and np.array_equal(u64(one[0]), u64(stats[b])), b
        wide = np.full((1, Nmax + 4099), 1e30, np.float32)
        wide[0, :n[b]] = x[b, :n[b]]
        m1, s1 = np.full((1, (Nmax + 4099) // h), SENTINEL), np.full((1, (Nmax + 4099) // h), SENTINEL)
        rc, one = raw_stats(ctx, wide, n[b:b + 1], Nmax + 4099, fs, mom=m1, sht=s1, stride=m1.shape[1])
        assert rc == 0 and np.array_equal(u64(one[0]), u64(stats[b])), b
        U = n[b] // h
        assert np.array_equal(u64(m1[0, :U - 3]), u64(mom[b, :U - 3])) and np.array_equal(u64(s1[0, :U - 29]), u64(sht[b, :U - 29])), b
    # device input, one float off a 16-byte boundary
    xin = ctx.dev_alloc(x.nbytes + 16)
    try:
        ctx.dev_from_host(xin + 4, x)
        md, sd = np.full((B, stride), SENTINEL), np.full((B, stride), SENTINEL)
        rc, dev = raw_stats(ctx, xin + 4, n, Nmax, fs, flags=_lib.ZVX_DEVICE_IN, mom=md, sht=sd, stride=stride)
        assert rc == 0, err(ctx)
        assert np.array_equal(u64(dev), u64(stats)) and np.array_equal(u64(md), u64(mom)) and np.array_equal(u64(sd), u64(sht))
        res = ctx.loudness_stats_device(xin + 4, n, Nmax, rate=fs)
        assert all(np.array_equal(u64(res[k]), u64(stats[:, i])) for i, k in enumerate(_lib.LOUDNESS_STATS_KEYS))
    finally:
        ctx.dev_free(xin)


def test_errors_leave_the_context_usable():
    ctx = ctx_for()
    fs, rows, x, n, m = case("8000")
    B, Nmax = x.shape
    h = R.unit_len(fs)
    rc, good = raw_stats(ctx, x, n, Nmax, fs)
    assert rc == 0, err(ctx)
    need = max(1, Nmax // h - 3)
    curve = np.full((B, need), SENTINEL)
    bad_len, neg_len = n.copy(), n.copy()
    bad_len[1], neg_len[2] = Nmax + 1, -1
    INV = _lib.ZVX_E_INVALID
    calls = [
        ("NULL in", lambda: raw_stats(ctx, None, n, Nmax, fs)),
        ("NULL nsamples", lambda: raw_stats(ctx, x, None, Nmax, fs, B=B)),
        ("B = 0", lambda: raw_stats(ctx, x, n, Nmax, fs, B=0)),
        ("Nmax = 0", lambda: raw_stats(ctx, x, n, 0, fs)),
        ("a length over Nmax", lambda: raw_stats(ctx, x, bad_len, Nmax, fs)),
        ("a negative length", lambda: raw_stats(ctx, x, neg_len, Nmax, fs)),
        ("rate 3999", lambda: raw_stats(ctx, x, n, Nmax, 3999)),
        ("rate 192001", lambda: raw_stats(ctx, x, n, Nmax, 192001)),
        ("NULL stats", lambda: raw_stats(ctx, x, n, Nmax, fs, want_stats=False)),
        ("stride too small, momentary", lambda: raw_stats(ctx, x, n, Nmax, fs, mom=curve, stride=need - 1)),
        ("stride too small, short-term", lambda: raw_stats(ctx, x, n, Nmax, fs, sht=curve, stride=need - 1)),
        ("stride negative", lambda: raw_stats(ctx, x, n, Nmax, fs, mom=curve, sht=curve, stride=-1)),
        ("ZVX_DEVICE_OUT", lambda: raw_stats(ctx, x, n, Nmax, fs, flags=_lib.ZVX_DEVICE_OUT)),
        ("ZVX_NO_SYNC", lambda: raw_stats(ctx, x, n, Nmax, fs, flags=_lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC)),
        ("ZVX_PCM16", lambda: raw_stats(ctx, x, n, Nmax, fs, flags=_lib.ZVX_PCM16)),
        ("an unknown flag", lambda: raw_stats(ctx, x, n, Nmax, fs, flags=1 << 20)),
    ]
    for what, call in calls:
        rc, st = call()
        assert rc == INV, (what, rc, err(ctx))
        assert np.all(st == 7.0) and np.all(curve == SENTINEL), what         # nothing was written
    # the cap: a row of 65537 units (zeros the allocator never touches: the call is refused before anything is read)
    long_n = (_lib.LOUDNESS_STATS_MAX_UNITS + 1) * 400
    zeros = np.zeros((1, long_n), np.float32)
    rc, st = raw_stats(ctx, zeros, np.array([long_n], np.int32), long_n, 4000)
    assert rc == _lib.ZVX_E_UNSUPPORTED and b"65536" in err(ctx) and np.all(st == 7.0), (rc, err(ctx))
    with pytest.raises(_lib.ZvxError) as e:
        ctx.loudness_stats(zeros, rate=4000, lengths=[long_n])
    assert e.value.code == _lib.ZVX_E_UNSUPPORTED
    rc, st = raw_stats(ctx, x, np.zeros(65536, np.int32), Nmax, fs, B=65536, want_stats=True)      # more than 65535 rows
    assert rc == _lib.ZVX_E_UNSUPPORTED, (rc, err(ctx))
    rc, again = raw_stats(ctx, x, n, Nmax, fs)
    assert rc == 0 and np.array_equal(u64(again), u64(good))
    res = ctx.loudness_stats(rows, rate=fs)
    assert all(close(res[k], m[k]) for k in S.KEYS)


def test_accounting_and_nothing_else_moved():
    ctx = ctx_for()
    cs = _ragged_case(3, 20, 41)
    before = ctx.synthesize(*cs, None, want_mel=False)
    fs, rows, x, n, m = case("22050")
    total = float(n.astype(np.int64).sum())
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.loudness_stats(rows, rate=fs, curves=True)
        tags = {t["name"]: t for t in ctx.tag_stats() if t["launches"]}
        assert set(tags) == {"post.loudness"}, sorted(tags)                   # no other tag moved
        assert tags["post.loudness"]["launches"] == 1 and tags["post.loudness"]["bytes"] == 4.0 * total and tags["post.loudness"]["ms"] > 0
        ms_stats = tags["post.loudness"]["ms"]
        ctx.reset_stats()
        ctx.loudness(rows, rate=fs)
        ms_loud = {t["name"]: t for t in ctx.tag_stats()}["post.loudness"]["ms"]
        print(f"post.loudness on {len(rows)} rows / {int(total)} samples at {fs} Hz: zvx_loudness_stats {ms_stats:.3f} ms, zvx_loudness {ms_loud:.3f} ms")
    finally:
        ctx.set_int("profile", 0)
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert np.array_equal(after["wav"].view(np.uint32), before["wav"].view(np.uint32)) and np.array_equal(after["mel_len"], before["mel_len"])


THREE = "The quick brown fox jumps over the lazy dog; does it, really? Pack my box with five dozen liquor jugs"


def test_tts_long_and_tts_report_what_they_deliver():
    """last_loudness / the segments' lufs describe the rows BEFORE the gain; the report describes the finished waveform, so its integrated
    figure is held against zvx_loudness of that very waveform (the same buffer: bit for bit) and against the float64 reference."""
    from zerovox_amd.report import LoudnessReport
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    fs, target = 22050, -23.0
    ctx = synth.model.ctx
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    assert synth.last_report is None
    plain, seg0 = synth.tts_long(THREE, spk, loudness=target)
    assert synth.last_report is None                         # nothing is measured unless asked for
    wav, seg = synth.tts_long(THREE, spk, loudness=target, report=True)
    rep = synth.last_report
    assert isinstance(rep, LoudnessReport)
    assert wav.dtype == np.float32 and np.array_equal(wav.view(np.uint32), plain.view(np.uint32))       # the waveform bits are unchanged
    assert [(s["start"], s["samples"], s["gain"]) for s in seg] == [(s["start"], s["samples"], s["gain"]) for s in seg0]
    lufs, peak = ctx.loudness([wav], rate=fs)
    m = S.measure([wav], fs)
    print(f"tts_long report: {rep}; zvx_loudness of the waveform {lufs[0]!r}; reference {m['integrated'][0]!r}, margins {m['margin'][0]:.3f} / {m['int_margin'][0]:.3f} LU")
    assert m["margin"][0] >= MARGIN and m["int_margin"][0] >= MARGIN
    assert abs(rep.integrated - lufs[0]) <= TOL and rep.integrated == lufs[0]
    for k, v in (("integrated", rep.integrated), ("max_momentary", rep.max_momentary), ("max_short_term", rep.max_short_term), ("lra", rep.lra),
                 ("lra_low", rep.lra_low), ("lra_high", rep.lra_high)):
        assert close(v, m[k][0]), (k, v, m[k][0])
    assert rep.short_gated == int(m["short_gated"][0]) and rep.sample_peak_db == 20.0 * math.log10(float(peak[0]))
    assert rep.true_peak_db == 20.0 * math.log10(float(ctx.true_peak([wav], rate=fs)[0])) and rep.true_peak_db >= rep.sample_peak_db
    assert rep == synth.loudness_report(wav) and synth.last_report == rep                                   # the host form: the same figures
    # an output rate: the converted waveform is what is measured
    synth.output_rate = 16000
    conv, _ = synth.tts_long(THREE, spk, loudness=target, report=True)
    assert abs(synth.last_report.integrated - ctx.loudness([conv], rate=16000)[0][0]) <= TOL
    synth.output_rate = fs
    # tts: the report of the finished row, on the device buffer behind the gain and the limiter, and on the plain path's host row
    text = seg0[0]["text"]
    one = synth.tts(text, spk, loudness=target, limiter=True)[0]
    two = synth.tts(text, spk, loudness=target, limiter=True, report=True)[0]
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))
    assert synth.last_report.integrated == ctx.loudness([two], rate=fs)[0][0]
    raw = synth.tts(text, spk, report=True)[0]
    assert synth.last_report.integrated == ctx.loudness([raw], rate=fs)[0][0]
    assert np.array_equal(raw.view(np.uint32), synth.tts(text, spk)[0].view(np.uint32))
    synth.model.close()
