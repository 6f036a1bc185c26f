"""The leveler on the MI355X (include/zvx.h: zvx_level, zvx_level_ex, zvx_level_rows) against the float64 restatement tests/level_ref.py, and
its window forms against the whole-signal call bit for bit.  Small shapes: 4000 Hz (h = 400) with a window of 3 units and one unit of
look-ahead -- RL = 1999, RR = 799 --, and 22050 Hz with the defaults (h = 2205, not a multiple of 4; S = 30).

The bound against the reference is derived, not measured: u agrees with the sequential recurrence to 1e-7 LU (include/zvx.h, zvx_loudness),
which is 1.2e-8 in a gain; then g is rounded once to f32 and the product once, 2^-24 each: |out - x g| <= (1.2e-8 + 2^-23) |x g| < 2^-22 |x g|."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import level_ref as LV
import resample_ref as RS
from stream_util import err, same_bits, vp
from zerovox_amd import _lib, leveler

import test_stream_limit_gpu as TSL                          # ctx_for: the context the other post-processing tests share

S32, S16 = np.uint32(0xDEADBEEF), np.int16(0x5A5B)
RATE, H = 4000, 400
TARGET, WINDOW_MS, LOOKAHEAD_MS = -16.0, 300.0, 100.0
RL, RR = 1999, 799
KW = dict(target=TARGET, max_gain_db=20.0, window_ms=WINDOW_MS, lookahead_ms=LOOKAHEAD_MS)
LENGTHS = (0, 1, 399, 400, 401, 1600, 2923, 8007)
BOUND = 2.0 ** -22
INV, UNS = _lib.ZVX_E_INVALID, _lib.ZVX_E_UNSUPPORTED
_c = {}


def params(**over):
    kw = dict(KW, **over)
    return _lib.LevelParams(kw["target"], kw["max_gain_db"], kw["window_ms"], kw["lookahead_ms"])


def rows4k():
    """the eight rows at 4000 Hz and their references, computed once and left unchanged"""
    if "rows" not in _c:
        assert leveler.reach(RATE, WINDOW_MS, LOOKAHEAD_MS) == (RL, RR)
        rows = []
        for i, n in enumerate(LENGTHS):
            rng = np.random.default_rng(500 + i)
            levels = [[0.1, 0.004, 0.3, 0.03], [0.2, 0.01, 0.05]][i % 2]
            x = LV.bursts(rng, n, RATE, levels, zero_units=6 if n == 8007 else 0, zero_at=7)
            x.setflags(write=False)
            rows.append(x)
        _c["rows"] = rows
        _c["ref"] = [LV.level(x, RATE, **KW) for x in rows]
    return _c["rows"], _c["ref"]


def whole(ctx):
    """zvx_level on the eight rows: (out [B][Nmax], gain_lo, gain_hi), once"""
    if "whole" not in _c:
        rows, _ = rows4k()
        _c["whole"] = ctx.level(rows, rate=RATE, **KW)
        for a in _c["whole"]:
            a.setflags(write=False)
    return _c["whole"]


def raw(ctx, name, x, n, Nmax, prm, out, stride, tail, flags=0, B=None, rate=RATE, results=True):
    """zvx_level / zvx_level_ex / zvx_level_rows with the arguments as given -> (rc, gain_lo, gain_hi)"""
    B = len(n) if B is None else B
    lo, hi = np.full(max(B, 1), -7.0, np.float32), np.full(max(B, 1), -7.0, np.float32)
    rc = getattr(ctx._lib, name)(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if prm is not None else None, vp(out), stride,
                                 vp(lo) if results else None, vp(hi) if results else None, flags, *tail)
    return rc, lo, hi


def windows_array(wins, reserved=None):
    a = (_lib.RowWindow * len(wins))()
    for b, (o, begin, cnt, last) in enumerate(wins):
        a[b] = _lib.RowWindow(int(o), int(begin), int(cnt), int(last), 0 if reserved is None else reserved.get(b, 0))
    return a


def ulp_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def check_against_ref(got, lo, hi, x, ref, what):
    e = np.abs(got.astype(np.float64) - ref["exact"])
    tol = BOUND * np.abs(ref["exact"])
    worst = float(np.max(e / np.maximum(np.abs(ref["exact"]), 1e-300))) if len(x) else 0.0
    print(f"{what}: n = {len(x)}, max |out - ref| / |ref| = {worst:.3e} (bound {BOUND:.3e}), gain in [{lo}, {hi}]")
    assert np.all(e <= tol), (what, int(np.argmax(e - tol)))
    if len(x):
        assert ulp_apart(lo, ref["g32"].min()) <= 1 and ulp_apart(hi, ref["g32"].max()) <= 1, (what, lo, hi, ref["g32"].min(), ref["g32"].max())
    else:
        assert lo == 1.0 and hi == 1.0


# ------------------------------------------------------------------------------------------------ 1, 2: the reference, and what is exact
def test_rows_against_the_float64_reference():
    ctx = TSL.ctx_for()
    rows, refs = rows4k()
    for x in rows:
        assert LV.ambiguous(x, RATE) == []                   # no unit near the gate: the reference decides every one
    out, lo, hi = whole(ctx)
    assert out.shape == (len(rows), 8007)
    for b, (x, ref) in enumerate(zip(rows, refs)):
        n = len(x)
        check_against_ref(out[b, :n], lo[b], hi[b], x, ref, f"4000 Hz row {b}")
        assert not out[b, n:].any(), b
    # exact: rows without a whole unit, and the samples of the long row whose two nodes are 1 (a window of exact zeros under both)
    for b in (0, 1, 2):
        assert same_bits(out[b, :LENGTHS[b]], rows[b]) and lo[b] == 1.0 and hi[b] == 1.0, b
    p = LV.units(rows[7], RATE)
    G = LV.gains(p, 3, TARGET)
    assert np.all(p[9:13] == 0.0) and G[11] == 1.0 and G[12] == 1.0
    assert same_bits(out[7, 11 * H:12 * H], rows[7][11 * H:12 * H])
    assert np.any(G == 10.0) and np.any(G < 10.0) and hi[7] == np.float32(10.0) and lo[7] < 10.0
    for b in (3, 4, 5, 6, 7):
        assert not same_bits(out[b, :LENGTHS[b]], rows[b]), (b, "the leveler acts")
    # x = 1 on the same rows' lengths is not the same gain curve (the gain follows the signal), so gain_lo / gain_hi are checked against
    # the reference above; a constant row has ONE gain where every G is the bound
    quiet = np.full(1600, 2e-3, np.float32)
    quiet[::2] *= -1
    o2, l2, h2 = ctx.level([quiet], rate=RATE, **KW)
    assert l2[0] == h2[0] == np.float32(10.0) and same_bits(o2[0], quiet * np.float32(10.0))


@pytest.mark.parametrize("n", [40 * 2205 + 17, 3 * 2205 - 1])
def test_the_model_rate_with_the_defaults(n):
    ctx = TSL.ctx_for()
    rng = np.random.default_rng(n)
    x = LV.bursts(rng, n, 22050, [0.1, 0.004, 0.3, 0.03])
    assert LV.ambiguous(x, 22050) == []
    ref = LV.level(x, 22050, TARGET)
    out, lo, hi = ctx.level([x], TARGET, rate=22050)
    check_against_ref(out[0], lo[0], hi[0], x, ref, "22050 Hz")
    assert lo[0] < hi[0]


# ------------------------------------------------------------------------------------------------ 3: windows
def stream_pieces(ctx, x, sizes, pcm16, rate=RATE, kw=KW):
    calls = []

    def fn(samples, o, begin, cnt, last):
        out, lo, hi = ctx.level_window([samples], in_origin=o, out_begin=begin, out_count=cnt, last=last, pcm16=pcm16, rate=rate, **kw)
        calls.append((o, begin, cnt, last, lo[0], hi[0]))
        return out[0].copy()
    chunks, at, i = [], 0, 0
    while at < len(x):
        chunks.append(x[at:at + sizes[i % len(sizes)]])
        at += len(chunks[-1])
        i += 1
    planner = leveler.LevelPlanner(*leveler.reach(rate, kw["window_ms"], kw["lookahead_ms"]))
    pieces = []
    hist = np.zeros(0, np.float32)
    for cur, last in [(c, False) for c in chunks] + [(np.zeros(0, np.float32), True)]:
        hist = np.concatenate([hist, cur])
        o, begin, cnt, keep = planner.push(len(cur), last)
        if cnt > 0:
            pieces.append(fn(hist, o, begin, cnt, last))
        hist = hist[keep - o:]
    return pieces, calls


@pytest.mark.parametrize("cut,b,pcm16", [("400", 7, False), ("400", 7, True), ("random", 7, False), ("random", 6, True), ("1", 6, False), ("1", 6, True)])
def test_windows_concatenate_to_the_whole_call(cut, b, pcm16):
    ctx = TSL.ctx_for()
    rows, _ = rows4k()
    out, lo, hi = whole(ctx)
    x = rows[b]
    want = out[b, :len(x)]
    sizes = {"400": [400], "1": [1], "random": [int(v) for v in np.random.default_rng(11).integers(1, 1300, 50)]}[cut]
    pieces, calls = stream_pieces(ctx, x, sizes, pcm16)
    got = np.concatenate(pieces)
    if pcm16:
        assert got.dtype == np.int16 and np.array_equal(got, RS.pcm16(want)), (cut, b)
    else:
        assert same_bits(got, want), (cut, b)
    assert same_bits(min(c[4] for c in calls), lo[b]) and same_bits(max(c[5] for c in calls), hi[b])
    assert len(calls) >= 3 and any(c[0] % 4 for c in calls) and any(c[0] % H for c in calls)      # origins off every alignment and off the unit grid
    print(f"cut {cut}, row {b}, pcm16 {pcm16}: {len(calls)} windows")


def test_windows_at_the_model_rate():
    """h = 2205: no multiple of 4, so the unit spans start at every alignment"""
    ctx = TSL.ctx_for()
    n = 40 * 2205 + 17
    x = LV.bursts(np.random.default_rng(n), n, 22050, [0.1, 0.004, 0.3, 0.03])
    kw = dict(KW, window_ms=3000.0)
    want = ctx.level([x], rate=22050, **kw)[0][0]
    pieces, calls = stream_pieces(ctx, x, [4096, 5000, 777], False, rate=22050, kw=kw)
    assert same_bits(np.concatenate(pieces), want)
    assert any(c[0] > 0 for c in calls)


# ------------------------------------------------------------------------------------------------ 4: a window per row
def rows_case():
    """8 rows at 8 positions of 8 signals: (signals, [(signal, window, samples)])"""
    if "case" not in _c:
        sig = [LV.bursts(np.random.default_rng(700 + i), 9000 + 37 * i, RATE, [0.1, 0.004, 0.3, 0.03][i % 4:] + [0.05]) for i in range(8)]
        big = ((1 << 32) // H + 13) * H                        # a multiple of h beyond 2^32: the grid phase of the small origin
        rows = [(0, (0, 0, 3000, 0), 3000 + RR),                                        # starts its signal, not last
                (1, (1203, 1203 + RL, -1, 1), len(sig[1]) - 1203),                      # last, to the end
                (2, (0, 0, -1, 1), len(sig[2])),                                        # the whole signal
                (3, (2000, 2000 + RL + 5, 0, 0), 2500),                                 # an empty range
                (4, (0, 0, -1, 1), 0),                                                  # n == 0 (as a signal of its own)
                (5, (801, 801 + RL, 4097, 0), RL + 4097 + RR),                          # interior, exactly RL / RR of support, more than one tile
                (6, (1600, 1600 + RL + 3, 1, 0), RL + 3 + 1 + RR),                      # one sample
                (7, (4000, 4000 + RL + 401, 1777, 1), len(sig[7]) - 4000)]              # last, but not to the end
        out = []
        for g, w, k in rows:
            s = np.ascontiguousarray(sig[g][w[0]:w[0] + k]) if k else np.zeros(0, np.float32)
            assert len(s) == k
            c = w[2] if w[2] >= 0 else w[0] + k - w[1]
            assert LV.supported(RL, RR, w[0], k, w[1], c, w[3]), w
            s.setflags(write=False)
            out.append((g, w, s))
        _c["case"] = (sig, out, big)
    return _c["case"]


def pack_rows(samples):
    n = np.array([len(s) for s in samples], np.int32)
    nmax = max(int(n.max()), 1)
    x = np.full((len(samples), nmax + (nmax % 2 == 0)), S32, np.uint32).view(np.float32)     # the sentinel behind every row
    for b, s in enumerate(samples):
        x[b, :n[b]] = s
    return x, n


def counts(wins, n):
    return [cnt if cnt >= 0 else max(0, o + int(k) - begin) for (o, begin, cnt, last), k in zip(wins, n)]


def alone(ctx, s, w, prm, pcm16=False):
    """the one-row zvx_level_ex call with the row's window -> (its emitted samples, gain_lo, gain_hi)"""
    k = max(len(s), 1)
    xin = np.zeros(k, np.float32)
    xin[:len(s)] = s
    cnt = counts([w], [len(s)])[0]
    out = np.full((1, max(k, cnt) + 3), S16 if pcm16 else S32, np.int16 if pcm16 else np.uint32)
    rc, lo, hi = raw(ctx, "zvx_level_ex", xin, np.array([len(s)], np.int32), k, prm, out, out.shape[1], [int(v) for v in w], _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, (w, err(ctx))
    assert np.all(out[0, cnt:] == (S16 if pcm16 else S32))
    return out[0, :cnt].copy(), lo[0], hi[0]


def level_rows(ctx, samples, wins, prm, pcm16=False):
    x, n = pack_rows(samples)
    B, stride = len(n), x.shape[1] + 3
    out = np.full((B + 1, stride), S16 if pcm16 else S32, np.int16 if pcm16 else np.uint32)    # one row more than the call owns
    rc, lo, hi = raw(ctx, "zvx_level_rows", x, n, x.shape[1], prm, out, stride, [windows_array(wins)], _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, err(ctx)
    assert np.all(out[B] == (S16 if pcm16 else S32))
    return out, lo, hi, counts(wins, n)


@pytest.mark.parametrize("pcm16", [False, True])
def test_rows_equal_the_one_row_calls(pcm16):
    ctx = TSL.ctx_for()
    sig, rows, _ = rows_case()
    samples, wins = [r[2] for r in rows], [r[1] for r in rows]
    prm = params()
    out, lo, hi, cnts = level_rows(ctx, samples, wins, prm, pcm16)
    assert cnts[3] == 0 and cnts[4] == 0 and cnts[5] == 4097
    s_ = S16 if pcm16 else S32
    for b, (g, w, s) in enumerate(rows):
        cnt = cnts[b]
        assert np.all(out[b, cnt:] == s_), (b, "written beyond cnt_b")
        a, alo, ahi = alone(ctx, s, w, prm, pcm16)
        assert np.array_equal(out[b, :cnt], a), (pcm16, b, w)
        assert same_bits(lo[b], alo) and same_bits(hi[b], ahi), (b, lo[b], alo, hi[b], ahi)
        if cnt == 0:
            assert lo[b] == 1.0 and hi[b] == 1.0
    if not pcm16:                                            # and the whole-signal call, through the reference's bound and bit for bit
        for b in (1, 5, 7):
            g, w, s = rows[b]
            full = ctx.level([sig[g]], rate=RATE, **KW)[0][0]
            assert same_bits(out[b, :cnts[b]].view(np.float32), full[w[1]:w[1] + cnts[b]]), b
        g, w, s = rows[5]
        ref = LV.level_window(s, *w, RATE, **KW)
        check_against_ref(out[5, :cnts[5]].view(np.float32), lo[5], hi[5], s[w[1] - w[0]:w[1] - w[0] + cnts[5]], ref, "rows: row 5")


def test_rows_are_independent_and_origins_may_be_large():
    ctx = TSL.ctx_for()
    sig, rows, big = rows_case()
    samples, wins = [r[2] for r in rows], [r[1] for r in rows]
    prm = params()
    a, alo, ahi, cnts = level_rows(ctx, samples, wins, prm)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    b_, blo, bhi, _ = level_rows(ctx, [samples[i] for i in perm], [wins[i] for i in perm], prm)
    for j, i in enumerate(perm):
        assert np.array_equal(a[i, :cnts[i]], b_[j, :cnts[i]]) and same_bits(alo[i], blo[j]) and same_bits(ahi[i], bhi[j]), (i, j)
    # a neighbour's samples change: the row's bits do not
    other = [s.copy() for s in samples]
    other[6] = other[6] * np.float32(0.25)
    other[2] = other[2][::-1].copy()
    c_, _, _, _ = level_rows(ctx, other, wins, prm)
    for i in (0, 1, 5, 7):
        assert np.array_equal(a[i, :cnts[i]], c_[i, :cnts[i]]), i
    assert not np.array_equal(a[6, :cnts[6]], c_[6, :cnts[6]])
    # in_origin beyond 2^32, shifted by a multiple of h: the same window, the same bits
    sel = [5, 6, 0]
    shifted = [(wins[5][0] + big, wins[5][1] + big, wins[5][2], 0), (wins[6][0] + big, wins[6][1] + big, wins[6][2], 0), wins[0]]
    assert shifted[0][0] > 1 << 32 and big % H == 0
    d_, dlo, dhi, dc = level_rows(ctx, [samples[i] for i in sel], shifted, prm)
    for j, i in enumerate(sel):
        assert dc[j] == cnts[i] and np.array_equal(d_[j, :dc[j]], a[i, :cnts[i]]), i
        assert same_bits(dlo[j], alo[i]) and same_bits(dhi[j], ahi[i])


# ------------------------------------------------------------------------------------------------ 5: in place, on the device
def test_in_place_and_the_device_forms():
    ctx = TSL.ctx_for()
    sig, rows, _ = rows_case()
    prm = params()
    # in place on the host: out_begin == in_origin on every row
    ins = [rows[0][2], rows[2][2], sig[3][:2500]]
    iw = [(0, 0, 3000, 0), (0, 0, -1, 1), (0, 0, 0, 0)]
    want, wlo, whi, cnts = level_rows(ctx, ins, iw, prm)
    x, n = pack_rows(ins)
    xi = x.copy()
    rc, lo, hi = raw(ctx, "zvx_level_rows", xi, n, x.shape[1], prm, xi, x.shape[1], [windows_array(iw)])
    assert rc == 0, err(ctx)
    assert same_bits(lo, wlo) and same_bits(hi, whi)
    for b, cnt in enumerate(cnts):
        assert np.array_equal(xi[b, :cnt].view(np.uint32), want[b, :cnt]), b
        assert np.array_equal(xi[b, cnt:].view(np.uint32), x[b, cnt:].view(np.uint32)), (b, "touched outside [0, cnt_b)")
    xw = x.copy()                                            # zvx_level itself, in place
    nn = np.array([3000 + RR, len(ins[1]), 2500], np.int32)
    ref_out, rlo, rhi = ctx.level(x, rate=RATE, lengths=nn, **KW)
    rc, lo, hi = raw(ctx, "zvx_level", xw, nn, x.shape[1], prm, xw, x.shape[1], [])
    assert rc == 0 and same_bits(lo, rlo) and same_bits(hi, rhi)
    for b in range(3):
        assert same_bits(xw[b, :nn[b]], ref_out[b, :nn[b]]), b
    # one interior window through every form of the call
    g, w, s = rows[5]
    k, cnt = len(s), w[2]
    nn = np.array([k], np.int32)
    stride = k + 3
    ref = np.full((1, stride), S32, np.uint32)
    rc, lo, hi = raw(ctx, "zvx_level_ex", s, nn, k, prm, ref, stride, w)
    assert rc == 0 and lo[0] < hi[0]
    din = ctx.dev_alloc(k * 4 + 16)
    dout = ctx.dev_alloc(2 * stride * 4 + 16)
    try:
        ctx.dev_from_host(din + 4, s)                        # the device rows sit one float off a 16-byte boundary
        out = np.full((2, stride), S32, np.uint32)
        rc, l1, h1 = raw(ctx, "zvx_level_ex", din + 4, nn, k, prm, out, stride, w, _lib.ZVX_DEVICE_IN)
        assert rc == 0, err(ctx)
        assert np.array_equal(out[0], ref[0]) and np.all(out[1] == S32) and same_bits(l1, lo) and same_bits(h1, hi)
        for shift in (4, 8, 12, 0):                          # a device output at every alignment
            ctx.dev_from_host(dout, np.full(2 * stride + 4, S32, np.uint32))
            rc, l2, h2 = raw(ctx, "zvx_level_ex", s, nn, k, prm, dout + shift, stride, w, _lib.ZVX_DEVICE_OUT)
            assert rc == 0, err(ctx)
            flat = ctx.dev_to_host(dout, (2 * stride + 4,), np.uint32)
            a = shift // 4
            assert np.all(flat[:a] == S32) and np.array_equal(flat[a:a + stride], ref[0]) and np.all(flat[a + stride:] == S32), shift
            assert same_bits(l2, lo) and same_bits(h2, hi)
        ctx.dev_from_host(dout, np.full(2 * stride + 4, S32, np.uint32))
        rc, _, _ = raw(ctx, "zvx_level_ex", din + 4, nn, k, prm, dout + 4, stride, w, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC, results=False)
        assert rc == 0, err(ctx)
        ctx.sync()
        flat = ctx.dev_to_host(dout, (2 * stride + 4,), np.uint32)
        assert flat[0] == S32 and np.array_equal(flat[1:1 + stride], ref[0]) and np.all(flat[1 + stride:] == S32)
        want16 = RS.pcm16(ref[0, :cnt].view(np.float32))
        ctx.dev_from_host(dout, np.full(2 * stride + 8, S16, np.int16))
        rc, _, _ = raw(ctx, "zvx_level_ex", din + 4, nn, k, prm, dout + 2, stride, w, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_PCM16)
        assert rc == 0, err(ctx)
        flat16 = ctx.dev_to_host(dout, (2 * stride + 8,), np.int16)
        assert flat16[0] == S16 and np.array_equal(flat16[1:1 + cnt], want16) and np.all(flat16[1 + cnt:] == S16)
    finally:
        ctx.dev_free(dout)
        ctx.dev_free(din)


# ------------------------------------------------------------------------------------------------ 6: validation
def test_refusals_name_the_row_and_leave_the_context_usable():
    ctx = TSL.ctx_for()
    sig, rows, _ = rows_case()
    sel = [0, 5, 2]
    samples, good = [rows[i][2] for i in sel], [rows[i][1] for i in sel]
    x, n = pack_rows(samples)
    Nmax = stride = x.shape[1]
    prm = params()

    def call(w=good, reserved=None, prm_=prm, x_=x, n_=n, out_=None, stride_=stride, flags=0, B_=None, Nmax_=Nmax, rate=RATE, win=True):
        out = np.full((3, stride), S32, np.uint32) if out_ is None else out_
        tail = [windows_array(w, reserved) if win else None]
        rc = raw(ctx, "zvx_level_rows", x_, n_, Nmax_, prm_, out, stride_, tail, flags, B=B_, rate=rate)[0]
        return rc, out, (err(ctx) or b"").decode()
    rc, want, _ = call()
    assert rc == 0
    o, begin, cnt, _ = good[1]
    k = int(n[1])
    bad = {
        "left": (dict(w=[good[0], (o + 1, begin, cnt, 0), good[2]]), "RL = %d" % RL),
        "right": (dict(w=[good[0], (o, begin, cnt + 1, 0), good[2]]), "RR = %d" % RR),
        "reserved": (dict(reserved={1: 1}), "row 1"),
        "count": (dict(w=[good[0], (o, begin, -1, 0), good[2]]), "row 1"),
        "outside": (dict(w=[good[0], (o, o - 1, 10, 1), good[2]]), "row 1"),
        "last": (dict(w=[good[0], (o, begin, cnt, 2), good[2]]), "row 1"),
        "negative": (dict(w=[good[0], (-1, begin, cnt, 0), good[2]]), "row 1"),
    }
    for name, (kw, text) in bad.items():
        rc, out, msg = call(**kw)
        assert rc == INV and "row 1" in msg and text in msg and "zvx_level_rows" in msg, (name, rc, msg)
        if name in ("left", "right"):
            assert "1 more sample" in msg, msg
        assert np.all(out == S32), (name, "something was written")
        rc, again, _ = call()                                # the context still serves
        assert rc == 0 and np.array_equal(again, want), name
    xf = x.copy()
    rc, _, msg = call(w=[(0, 0, 100, 0), (0, 5, 100, 0), (0, 0, -1, 1)], x_=xf, out_=xf)
    assert rc == INV and "row 1" in msg and "in place" in msg and np.array_equal(xf.view(np.uint32), x.view(np.uint32))
    assert call(stride_=100)[0] == INV and call(win=False)[0] == INV and "win is NULL" in err(ctx).decode()
    # the parameters
    nan, inf = float("nan"), float("inf")
    for over in (dict(target=0.5), dict(target=-70.5), dict(target=nan), dict(target=-inf), dict(max_gain_db=-0.1), dict(max_gain_db=nan),
                 dict(max_gain_db=inf), dict(window_ms=-1.0), dict(window_ms=nan), dict(window_ms=inf), dict(lookahead_ms=-1.0), dict(lookahead_ms=nan),
                 dict(lookahead_ms=inf), dict(window_ms=100.0, lookahead_ms=200.0), dict(window_ms=0.0, lookahead_ms=151.0)):
        rc, out, msg = call(prm_=params(**over))
        assert rc == INV and np.all(out == S32), (over, rc, msg)
    assert call(prm_=params(window_ms=60049.0))[0] == INV    # S = 600 is supported: what refuses this call is the support of its rows
    assert "RL" in err(ctx).decode()
    assert call(prm_=params(window_ms=60051.0))[0] == UNS and call(prm_=params(window_ms=1e30))[0] == UNS
    assert call(prm_=params(window_ms=0.0, lookahead_ms=100.0), w=[(0, 0, 100, 0)] * 3)[0] == 0       # S = 1, a = 1
    # the checks of the rows-call contract
    assert call(prm_=None)[0] == INV and call(x_=None)[0] == INV and call(n_=None, B_=3)[0] == INV
    assert call(B_=0)[0] == INV and call(Nmax_=0)[0] == INV and call(rate=3999)[0] == INV and call(rate=192001)[0] == INV
    assert call(n_=np.array([n[0], -1, n[2]], np.int32))[0] == INV and call(n_=np.array([n[0], Nmax + 1, n[2]], np.int32))[0] == INV
    for flags in (64, _lib.ZVX_HOST_ASYNC, _lib.ZVX_NATIVE_RATE, _lib.ZVX_NO_SYNC, 128, 1 << 20):
        assert call(flags=flags)[0] == INV, flags
    lib = ctx._lib
    assert lib.zvx_level(ctx._h, vp(x), vp(n), 3, Nmax, RATE, C.byref(prm), None, Nmax, None, None, 0) == INV and b"out is NULL" in err(ctx)
    assert lib.zvx_level(ctx._h, vp(x), vp(n), 3, Nmax, RATE, C.byref(prm), vp(want), Nmax - 1, None, None, 0) == INV
    assert lib.zvx_level(ctx._h, vp(xf), vp(n), 3, Nmax, RATE, C.byref(prm), vp(xf), Nmax, None, None, _lib.ZVX_PCM16) == INV
    assert lib.zvx_level(ctx._h, vp(x), vp(n), 65536, Nmax, RATE, C.byref(prm), vp(want), Nmax, None, None, 0) == UNS      # (refused before a length is read)
    rc, again, _ = call()
    assert rc == 0 and np.array_equal(again, want)


def test_accounting():
    ctx = TSL.ctx_for()
    sig, rows, _ = rows_case()
    samples, wins = [r[2] for r in rows], [r[1] for r in rows]
    x, n = pack_rows(samples)
    total, emitted = float(n.sum()), float(sum(counts(wins, n)))
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.level_rows(samples, wins, rate=RATE, **KW)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert [t for t in tags if t != "post.level" and tags[t]["launches"]] == [] and tags["post.level"]["launches"] == 1, tags
        assert tags["post.level"]["bytes"] == 4.0 * total + 4.0 * emitted and tags["post.level"]["ms"] > 0
        ctx.reset_stats()
        ctx.level_rows(samples, wins, rate=RATE, pcm16=True, **KW)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert tags["post.level"]["launches"] == 1 and tags["post.level"]["bytes"] == 4.0 * total + 2.0 * emitted
    finally:
        ctx.set_int("profile", 0)


# ------------------------------------------------------------------------------------------------ 7: through the model
TEXT = "The quick brown fox jumps over the lazy dog"


def test_through_the_model():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    try:
        model, ctx = synth.model, synth.model.ctx
        lvl = dict(target=-16.0, window_ms=500.0, lookahead_ms=100.0)      # RR = 4409; a window shorter than the stream
        mel = np.random.default_rng(5).standard_normal((120, 80)).astype(np.float32)
        plain = np.concatenate(list(model.vocode_stream(mel, chunk_frames=16)))
        pieces = list(model.vocode_stream(mel, chunk_frames=16, level=lvl))
        got = np.concatenate(pieces)
        want, lo, hi = ctx.level([plain], **lvl)
        assert len(pieces) >= 2 and got.dtype == np.float32 and same_bits(got, want[0])
        assert not same_bits(got, plain) and lo[0] < hi[0], (lo, hi)
        assert len(pieces[0]) == 2 * 16 * ctx.hop - 4409       # RR behind: the first chunk (4096 samples) does not reach it, the second does
        assert same_bits(np.concatenate(list(model.vocode_stream(mel, chunk_frames=16, chunks_per_call=3, level=lvl))), want[0])
        # the chain: denoise, level, limit; the conversion last
        dn, lim = dict(strength=0.5, floor=0.0), dict(ceiling=10 ** (-20 / 20), window_ms=5.0, oversample=4)
        chain = np.concatenate(list(model.vocode_stream(mel, chunk_frames=16, denoise=dn, level=lvl, limiter=lim)))
        step = ctx.denoise([plain], model.denoise_bias, **dn)
        step = ctx.level([step[0]], **lvl)[0]
        step = ctx.limit([step[0]], **lim)[0][0]
        assert same_bits(chain, step)
        ctx.set_int("out_rate", 48000)
        try:
            up = np.concatenate(list(model.vocode_stream(mel, chunk_frames=16, level=lvl)))
        finally:
            ctx.set_int("out_rate", 0)
        conv, conv_len = ctx.resample([want[0]], 22050, 48000)
        assert same_bits(up, conv[0, :conv_len[0]])
        with pytest.raises(ValueError):
            list(model.vocode_stream(mel, chunk_frames=16, level=lvl, resident=True))
        # tts_stream: a plain stream is bit-equal before and after a levelled one
        spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
        before = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16)))
        levelled = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, level_lufs=-16)))
        after = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16)))
        assert same_bits(before, after) and len(levelled) == len(before)
        assert same_bits(levelled, ctx.level([before], -16.0)[0][0])
    finally:
        synth.model.close()


# ------------------------------------------------------------------------------------------------ a last window whose nodes are clamped
@pytest.mark.parametrize("lookahead_ms,out_begin", [(100.0, 20 * H + 3), (200.0, 19 * H + 5)])
def test_a_last_window_that_begins_in_the_clamped_region(lookahead_ms, out_begin):
    """the outputs begin in the signal's last a units (or its tail): the first node is clamped to unit U - 1, whose window lies to the left of
    what RL covers.  With the oldest unit's warm-up in the window the bits are zvx_level's; one sample short the call is refused."""
    ctx = TSL.ctx_for()
    rows, _ = rows4k()
    x = rows[7]
    N = len(x)
    kw = dict(KW, lookahead_ms=lookahead_ms)
    h, S, a, rl, rr = LV.geometry(RATE, WINDOW_MS, lookahead_ms)
    U = N // h
    assert N == 20 * H + 7 and out_begin // h + a - 1 > U - 1
    o_max = (U - 1 - S + 1 - 2) * h
    assert o_max < out_begin - rl                            # RL alone would admit a later origin
    assert LV.supported(rl, rr, o_max, N - o_max, out_begin, N - out_begin, True, (h, S, a))
    assert not LV.supported(rl, rr, o_max + 1, N - o_max - 1, out_begin, N - out_begin, True, (h, S, a))
    want = ctx.level([x], rate=RATE, **kw)[0][0]
    prm = params(lookahead_ms=lookahead_ms)
    cnt = N - out_begin
    other = rows[6]                                          # a whole signal beside it: the refusal names row 1
    for o, good in ((o_max, True), (o_max + 1, False), (o_max - 3, True)):
        xs, n = pack_rows([other, x[o:]])
        wins = [(0, 0, -1, 1), (o, out_begin, -1, 1)]
        out = np.full((3, xs.shape[1]), S32, np.uint32)
        rc, lo, hi = raw(ctx, "zvx_level_rows", xs, n, xs.shape[1], prm, out, xs.shape[1], [windows_array(wins)])
        if good:
            assert rc == 0, err(ctx)
            assert same_bits(out[1, :cnt].view(np.float32), want[out_begin:]) and np.all(out[1, cnt:] == S32), o
        else:
            msg = err(ctx).decode()
            assert rc == INV and "row 1" in msg and "clamped" in msg and "1 more sample" in msg, (rc, msg)
            assert np.all(out == S32), "something was written"
    o1, l1, h1 = ctx.level_window([x[o_max:]], in_origin=o_max, out_begin=out_begin, rate=RATE, **kw)      # the one-window form
    assert same_bits(o1[0], want[out_begin:])
    with pytest.raises(_lib.ZvxError):
        ctx.level_window([x[o_max + 1:]], in_origin=o_max + 1, out_begin=out_begin, rate=RATE, **kw)
