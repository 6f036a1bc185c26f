"""The rate conversion with a window per row on the GPU (include/zvx.h: zvx_resample_rows) and the batched conversions of
zvx_stream_next_many.  The reference for a row's bits is always zvx_resample_ex on that row ALONE with the row's window; since the one-row
call shares the kernel body, the f32 rows are also held against tests/resample_ref.py (float64) within resample_ref.bound, the bound
tests/test_resample_gpu.py uses.  For the many-streams part the reference is the same session stepped alone with zvx_stream_next."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resample_ref as R
from stream_util import err, same_bits, vp
from zerovox_amd import _lib

import test_resample_gpu as TR                               # ctx_for, raw_resample, check_float
import test_rows_windows_gpu as TRW                          # windows_array, open_session
import test_stream_many_gpu as TSM                           # Env, DN_KW, LIM_KW

S32, S16 = np.uint32(0xDEADBEEF), np.int16(0x5A5B)
INV, BUF, UNS = _lib.ZVX_E_INVALID, _lib.ZVX_E_BUFFER, _lib.ZVX_E_UNSUPPORTED
PAIRS = [(22050, 48000),       # up-conversion: the strided lane layout
         (22050, 8000),        # down-conversion: vector stores
         (22050, 44100),       # L = 2
         (16000, 22050),       # L = 441, the largest bank: a smaller tile
         (22050, 22050)]       # a copy
FAR = 2 ** 33 + 5
_cases = {}


def ceil_div(a, b):
    return -(-a // b)


def case(rate_in, rate_out):
    """the rows of one call -> (samples, windows (in_origin, out_begin, out_count, last), counts), made once per rate pair and read-only"""
    key = (rate_in, rate_out)
    if key in _cases:
        return _cases[key]
    L, M = R.pair(rate_in, rate_out)
    rng = np.random.default_rng(17)
    sig = [rng.uniform(-1, 1, 3000).astype(np.float32) for _ in range(10)]
    first = lambda k: ceil_div(k * L, M)                     # the first output at or behind input position k
    n_long = ceil_div(2200 * M, L)                           # more than 2 x 1024 outputs: several tiles of 1024
    rows = [
        (sig[0], (0, 0, -1, 1)),                                               # the whole signal
        (sig[1], (0, 0, 700, 0)),                                              # a head window
        (sig[2][401:1601], (401, first(401) + 20, 300, 0)),                    # interior windows: in_origin = 1, 2, 3 mod 4
        (sig[3][802:2002], (802, first(802) + 3, 257, 1)),
        (sig[4][1203:], (1203, first(1203) + 11, -1, 0)),                      # ... the last one to the end of its signal
        (sig[5][:1500], (FAR, first(FAR) + 7, 600, 0)),                        # beyond 2^32
        (sig[6][:900], (100, 50, 0, 0)),                                       # emits nothing
        (sig[7][:0], (40, 10, -1, 0)),                                         # holds nothing: zeros to the end of its (empty) signal
        (rng.uniform(-1, 1, n_long).astype(np.float32), (0, 0, -1, 0)),        # several tiles ...
        (sig[8][:400], (0, 5, 3, 0)),                                          # ... beside a row of 3 outputs
    ]
    samples = [s for s, _ in rows]
    wins = [w for _, w in rows]
    cnt = [c if c >= 0 else max(0, ceil_div((o + len(s)) * L, M) - begin) for s, (o, begin, c, _) in rows]
    assert cnt[8] > 2048 and cnt[9] == 3 and cnt[6] == 0 and cnt[7] == ceil_div(40 * L, M) - 10 and [w[0] % 4 for w in wins[2:5]] == [1, 2, 3]
    for s in samples:
        s.setflags(write=False)
    _cases[key] = (samples, wins, cnt)
    return _cases[key]


def pack_rows(samples, stride=None):
    """rows of different lengths -> (x [B][stride] with the sentinel behind every row, n); the stride is no multiple of 4"""
    n = np.array([len(s) for s in samples], np.int32)
    nmax = max(int(n.max()), 1)
    stride = stride or nmax + (1, 0, 3, 2)[nmax % 4]         # = 1 mod 4
    x = np.full((len(samples), stride), S32, np.uint32).view(np.float32)
    for b, s in enumerate(samples):
        x[b, :n[b]] = s
    return x, n


def out_rows(B, stride, pcm16):
    return np.full((B + 1, stride), S16, np.int16) if pcm16 else np.full((B + 1, stride), S32, np.uint32)      # one row more than the call owns


def raw_rows(ctx, x, n, rate_in, rate_out, out, stride, win, flags=0, out_len=None, B=None, Nmax=None):
    """the C call itself: x / out are ndarrays (host) or integer device pointers"""
    return ctx._lib.zvx_resample_rows(ctx._h, vp(x), vp(n), len(n) if B is None else B, (x.shape[1] if hasattr(x, "shape") else Nmax) if Nmax is None else Nmax,
                                      rate_in, rate_out, vp(out), stride, vp(out_len), flags, win)


def alone(ctx, s, w, rate_in, rate_out, pcm16=False):
    """zvx_resample_ex on the row alone -> its emitted samples (uint32 / int16 bits)"""
    o, begin, c, _ = w
    L, M = R.pair(rate_in, rate_out)
    cnt = c if c >= 0 else max(0, ceil_div((o + len(s)) * L, M) - begin)
    x = np.zeros((1, max(len(s), 1)), np.float32)
    x[0, :len(s)] = s
    out = out_rows(0, max(cnt, 1) + 5, pcm16)
    ol = np.zeros(1, np.int32)
    rc = TR.raw_resample(ctx, x, np.array([len(s)], np.int32), rate_in, rate_out, out, out.shape[1], _lib.ZVX_PCM16 if pcm16 else 0, ol, ex=(o, begin, c))
    assert rc == 0, err(ctx)
    assert ol[0] == cnt
    return out[0, :cnt].copy()


def rows_host(ctx, samples, wins, rate_in, rate_out, cnt, pcm16=False):
    """one zvx_resample_rows call on host rows -> the whole output block [B + 1][stride] (sentinels where nothing was written)"""
    x, n = pack_rows(samples)
    stride = max(max(cnt), 1) + 37
    out = out_rows(len(samples), stride, pcm16)
    ol = np.full(len(samples), -7, np.int32)
    rc = raw_rows(ctx, x, n, rate_in, rate_out, out, stride, TRW.windows_array(wins), _lib.ZVX_PCM16 if pcm16 else 0, ol)
    assert rc == 0, err(ctx)
    assert list(ol) == list(cnt), (list(ol), cnt)
    return out


def check_block(out, want, cnt, what):
    sentinel = S16 if out.dtype == np.int16 else S32
    for b, c in enumerate(cnt):
        assert np.array_equal(out[b, :c], want[b]), (what, b, "differs from the one-row call")
        assert np.all(out[b, c:] == sentinel), (what, b, "touched outside [0, cnt_b)")
    assert np.all(out[len(cnt)] == sentinel), (what, "the row behind the call's rows")


# ------------------------------------------------------------------------------------------------ rows equal the one-row calls
def test_the_reference_takes_an_origin_beyond_2_to_the_32():
    """no GPU work: resample_ref.resample_window at in_origin 2^33 + 5 is, bit for bit in float64, what it gives M q samples earlier with
    the outputs L q earlier (n M - k L is the same number): the reference needs no shifted origin for the far row"""
    for rate_in, rate_out in PAIRS:
        samples, wins, cnt = case(rate_in, rate_out)
        L, M = R.pair(rate_in, rate_out)
        o, begin, c, _ = wins[5]
        q = (FAR - 5) // M - 3
        far = R.resample_window(samples[5], rate_in, rate_out, o, begin, c)
        near = R.resample_window(samples[5], rate_in, rate_out, o - M * q, begin - L * q, c)
        assert 0 <= o - M * q < 4 * M + 6 and far.shape == (600,) and np.array_equal(far, near) and np.abs(far).max() > 0.1


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_rows_equal_the_one_row_calls(rate_in, rate_out):
    ctx = TR.ctx_for("tiny")
    samples, wins, cnt = case(rate_in, rate_out)
    B = len(samples)
    want = {p: [alone(ctx, s, w, rate_in, rate_out, p) for s, w in zip(samples, wins)] for p in (False, True)}
    # ---- the one-row call shares the kernel body: the f32 rows against the float64 reference
    for b, (s, (o, begin, c, _)) in enumerate(zip(samples, wins)):
        ref, A = R.resample_window(s, rate_in, rate_out, o, begin, c, want_mag=True)
        assert ref.shape == (cnt[b],)
        e, lim = np.abs(want[False][b].view(np.float32).astype(np.float64) - ref), R.bound(rate_in, rate_out, A)
        print(f"{rate_in} -> {rate_out} row {b}: {cnt[b]} samples, worst fraction of the bound {float((e / np.maximum(lim, 1e-300)).max()) if cnt[b] else 0.0:.3f}")
        assert np.all(e <= lim), b
        assert np.array_equal(want[True][b], R.pcm16(want[False][b].view(np.float32))), b
    assert np.abs(want[False][5].view(np.float32)).max() > 0.1               # the far row is not silence
    # ---- host rows
    f32 = rows_host(ctx, samples, wins, rate_in, rate_out, cnt)
    check_block(f32, want[False], cnt, "host f32")
    check_block(rows_host(ctx, samples, wins, rate_in, rate_out, cnt, pcm16=True), want[True], cnt, "host pcm16")
    # ---- device rows: both pointers off a 16-byte boundary, strides that are no multiple of 4
    x, n = pack_rows(samples)
    stride = max(cnt) + 37
    stride += (1, 0, 3, 2)[stride % 4]
    assert x.shape[1] % 4 == 1 and stride % 4 == 1
    win = TRW.windows_array(wins)
    xin, dout = ctx.dev_alloc(x.nbytes + 16), ctx.dev_alloc((B + 1) * stride * 4 + 16)
    try:
        ctx.dev_from_host(xin + 4, x)
        for pcm16, off in ((False, 4), (True, 2)):
            fill = out_rows(B, stride, pcm16)
            ctx.dev_from_host(dout + off, fill)
            ol = np.zeros(B, np.int32)
            fl = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | (_lib.ZVX_PCM16 if pcm16 else 0)
            assert raw_rows(ctx, xin + 4, n, rate_in, rate_out, dout + off, stride, win, fl, ol, Nmax=x.shape[1]) == 0, err(ctx)
            assert list(ol) == cnt
            check_block(ctx.dev_to_host(dout + off, fill.shape, fill.dtype), want[pcm16], cnt, f"device pcm16={pcm16}")
        # queued: ZVX_NO_SYNC, out_len NULL, then the context's own wait
        ctx.dev_from_host(dout + 4, out_rows(B, stride, False))
        fl = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC
        assert raw_rows(ctx, xin + 4, n, rate_in, rate_out, dout + 4, stride, win, fl, None, Nmax=x.shape[1]) == 0, err(ctx)
        ctx.sync()
        check_block(ctx.dev_to_host(dout + 4, (B + 1, stride), np.uint32), want[False], cnt, "device, queued")
    finally:
        ctx.dev_free(xin); ctx.dev_free(dout)


def test_windows_tile_the_whole_signal_call():
    """windows that tile a signal, each a row of ONE call: the whole-signal call's bits"""
    ctx = TR.ctx_for("tiny")
    from zerovox_amd.resample import rate_pair
    for rate_in, rate_out in ((22050, 48000), (22050, 8000)):
        x = np.random.default_rng(12).uniform(-1, 1, 9000).astype(np.float32)
        whole, wl = ctx.resample([x], rate_in, rate_out)
        whole = whole[0, :wl[0]]
        L, M, half = rate_pair(rate_in, rate_out)
        W = len(whole)
        cuts = [0, 1, 777, W // 3, W // 3 + 1, (5 * W) // 7, W - 5, W]
        rows, wins = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            k_lo = max(0, ceil_div(lo * M - half, L))        # the samples under the filter of outputs [lo, hi)
            k_hi = min(len(x), ((hi - 1) * M + half) // L + 1)
            rows.append(x[k_lo:k_hi]); wins.append((k_lo, lo, hi - lo if hi < W else -1))
        got, ol = ctx.resample_rows(rows, rate_in, rate_out, wins)
        assert list(ol) == [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert same_bits(np.concatenate(got), whole), (rate_in, rate_out)


# ------------------------------------------------------------------------------------------------ rows do not see each other
@pytest.mark.parametrize("rate_in,rate_out", [(22050, 48000), (22050, 8000)])
def test_rows_are_independent(rate_in, rate_out):
    ctx = TR.ctx_for("tiny")
    samples, wins, cnt = case(rate_in, rate_out)
    B = len(samples)
    base = rows_host(ctx, samples, wins, rate_in, rate_out, cnt)

    def sub(order, wins_=None):
        w = [(wins_ or wins)[i] for i in order]
        s = [samples[i] for i in order]
        L, M = R.pair(rate_in, rate_out)
        c = [k if k >= 0 else max(0, ceil_div((o + len(v)) * L, M) - begin) for v, (o, begin, k, _) in zip(s, w)]
        return rows_host(ctx, s, w, rate_in, rate_out, c), c
    # permuted
    perm = [5, 2, 7, 9, 0, 3, 8, 6, 1, 4]
    got, c = sub(perm)
    for j, i in enumerate(perm):
        assert c[j] == cnt[i] and np.array_equal(got[j, :c[j]], base[i, :cnt[i]]), (i, j)
    # rows dropped: without the long row the grid changes, the bits do not.  (The tiles per workgroup do NOT change here: about 30 tiles in
    # the whole call, tpb = min(8, tiles * B / 2048) is 1 on both sides; test_several_tiles_per_workgroup below is the one that runs tpb >= 2)
    keep = [9, 2, 5, 0]
    got, c = sub(keep)
    for j, i in enumerate(keep):
        assert np.array_equal(got[j, :c[j]], base[i, :cnt[i]]), (i, j)
    got, c = sub([4])
    assert np.array_equal(got[0, :c[0]], base[4, :cnt[4]])
    # the other rows' windows changed: rows 2 and 5 keep theirs
    other = [(o + 4, begin + 9, 100 if k != 0 else 33, last) for (o, begin, k, last) in wins]
    other[2], other[5] = wins[2], wins[5]
    got, c = sub(range(B), other)
    for i in (2, 5):
        assert np.array_equal(got[i, :c[i]], base[i, :cnt[i]]), i
    assert not np.array_equal(got[3, :100], base[3, :100])                   # (the changed windows did change something)
    # the Python layer: the same bits, f32 and int16
    rows, ol = ctx.resample_rows(samples, rate_in, rate_out, [w[:3] for w in wins])
    assert list(ol) == cnt
    for b in range(B):
        assert rows[b].dtype == np.float32 and np.array_equal(rows[b].view(np.uint32), base[b, :cnt[b]]), b
    pcm, _ = ctx.resample_rows(samples, rate_in, rate_out, wins, pcm16=True)
    for b in range(B):
        assert pcm[b].dtype == np.int16 and np.array_equal(pcm[b], R.pcm16(base[b, :cnt[b]].view(np.float32))), b


# ------------------------------------------------------------------------------------------------ several tiles per workgroup
OUT_LONG = 65536                                             # outputs of the longest row: 64 tiles of 1024
_ktest = []


def geometry(rate_in, rate_out, B, out_max):
    """What the library decides for such a call, by the shim's dry run (nothing is launched), held to the rule restated in kernel_ref."""
    import kernel_ref as K
    if not _ktest:
        _ktest.append(K.load_ktest())
    g = K.resample_geometry(_ktest[0], rate_in, rate_out, B, out_max)
    L, M = R.pair(rate_in, rate_out)
    assert (g["L"], g["M"]) == (L, M) and g["T"] == (R.taps_per_output(rate_in, rate_out) if L != M else 1) and g["fits"]
    want = K.resample_geometry_ref(L, M, g["T"], g["pitch"], B, out_max)
    assert {k: g[k] for k in want} == want, (g, want)
    return g


def ragged_rows(rate_in, rate_out, B, tile, tpb):
    """B rows for a call whose workgroups take tpb tiles of `tile` outputs each -> (samples, cnt for the rows call, natural counts).  Row 0 is
    the longest (it alone sizes the grid), row 1 ends inside a workgroup's second tile, row 2 exactly on a tpb * tile boundary, row 3 is a
    single sample, row 4 puts one output into the next workgroup, row 5 ends in a workgroup's last tile; the rest are short, every 16th
    up to three workgroups long."""
    L, M = R.pair(rate_in, rate_out)
    span = tpb * tile
    rng = np.random.default_rng(23)
    want = [None, tile + 300, span, None, span + 1, 2 * span + (tpb - 1) * tile + 5]
    want += [int(rng.integers(1, 3 * span if b % 16 == 0 else 2 * tile)) for b in range(len(want), B)]
    n = [ceil_div(c * M, L) if c is not None else 0 for c in want]
    n[0], n[3] = OUT_LONG * M // L, 1
    samples = [rng.uniform(-1, 1, k).astype(np.float32) for k in n]
    nat = [ceil_div(k * L, M) for k in n]
    cnt = [want[b] if b in (2, 4, 5) else nat[b] for b in range(B)]            # (the rows call cuts rows 2, 4, 5 to the count they are here for)
    assert all(c <= v for c, v in zip(cnt, nat)) and max(nat) == nat[0] and ceil_div(nat[0], tile) == OUT_LONG // tile
    assert tile < cnt[1] < 2 * tile and cnt[2] == span and len(samples[3]) == 1 and cnt[4] == span + 1
    for s in samples:
        s.setflags(write=False)
    return samples, cnt, nat


@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("rate_in,rate_out", [(22050, 48000), (48000, 22050)])
def test_several_tiles_per_workgroup(rate_in, rate_out, B):
    """k_resample_poly's loop over the tiles of a workgroup (tpb = min(8, tiles * B / 2048) >= 2 needs tiles * B >= 4096): 64 / 256 ragged rows
    of up to 65536 outputs, 22050 -> 48000 (the strided up-conversion layout) and 48000 -> 22050 (vector stores), f32 and int16.  Every
    row is bit-equal to the same row converted alone (64 tiles x 1 row: tpb = 1), in the rows call (nothing outside [0, cnt_b) written)
    and in the one-window call (zeros up to the longest row); two rows are held to the float64 reference."""
    ctx = TR.ctx_for("tiny")
    g = geometry(rate_in, rate_out, B, OUT_LONG)
    tile, tpb = g["tile"], g["tpb"]
    assert tile == 1024 and tpb >= 2 and (B != 256 or tpb == 8), g
    assert geometry(rate_in, rate_out, 1, OUT_LONG)["tpb"] == 1             # the reference call of every row
    samples, cnt, nat = ragged_rows(rate_in, rate_out, B, tile, tpb)
    assert geometry(rate_in, rate_out, B, max(nat))["tpb"] == tpb and geometry(rate_in, rate_out, B, max(cnt))["tpb"] == tpb
    print(f"SPEC resample_tpb_{rate_in}_{rate_out}_B{B} tile {tile} tpb {tpb} xcap {g['xcap']} lds {g['lds']} tiles/workgroup {tpb}")
    wins = [(0, 0, c, 0) for c in cnt]
    x, n = TR.padded(samples)
    for pcm16 in (False, True):
        want = [alone(ctx, s, w, rate_in, rate_out, pcm16) for s, w in zip(samples, wins)]
        if not pcm16:
            for b in (0, 1):
                ref, A = R.resample_window(samples[b], rate_in, rate_out, 0, 0, cnt[b], want_mag=True)
                e, lim = np.abs(want[b].view(np.float32).astype(np.float64) - ref), R.bound(rate_in, rate_out, A)
                print(f"SPEC resample_tpb_{rate_in}_{rate_out}_B{B} row {b} worst err/bound {float((e / np.maximum(lim, 1e-300)).max()):.3f}")
                assert np.all(e <= lim), b
        # the rows call: a window per row, nothing behind a row's own count
        check_block(rows_host(ctx, samples, wins, rate_in, rate_out, cnt, pcm16=pcm16), want, cnt, f"rows call pcm16={pcm16}")
        # the one-window call: every row to the end of its signal, zeros from there to the longest row
        stride = max(nat) + 37
        out = out_rows(B - 1, stride, pcm16)
        ol = np.zeros(B, np.int32)
        assert TR.raw_resample(ctx, x, n, rate_in, rate_out, out, stride, _lib.ZVX_PCM16 if pcm16 else 0, ol) == 0, err(ctx)
        assert list(ol) == nat
        for b in range(B):
            whole = want[b] if nat[b] == cnt[b] else alone(ctx, samples[b], (0, 0, -1, 0), rate_in, rate_out, pcm16)
            assert np.array_equal(out[b, :nat[b]], whole), (b, "one-window call differs from the row alone")
            assert not out[b, nat[b]:max(nat)].any(), (b, "no zeros behind the row")
            assert np.all(out[b, max(nat):] == (S16 if pcm16 else S32)), (b, "written past the longest row")


@pytest.mark.parametrize("rate_in,rate_out", [(192000, 8000), (192000, 6000)])
def test_decimation_past_22_to_1_halves_the_tile(rate_in, rate_out):
    """M / L = 24 and 32: the input span of 1024 outputs no longer fits beside the bank, the launcher halves the tile; at 32 : 1 the LDS
    passes 64 KiB (the opt-in path).  A row of three tiles and a few samples against the float64 reference."""
    ctx = TR.ctx_for("tiny")
    L, M = R.pair(rate_in, rate_out)
    n_out = 3 * 512 + 77
    g = geometry(rate_in, rate_out, 1, n_out)
    assert g["tile"] == 512 and g["tpb"] == 1 and (g["lds"] > 64 * 1024) == (M == 32) and g["lds"] <= 96 * 1024, g
    print(f"SPEC resample_decimate_{rate_in}_{rate_out} tile {g['tile']} tpb {g['tpb']} xcap {g['xcap']} lds {g['lds']}")
    s = np.random.default_rng(29).uniform(-1, 1, n_out * M - 5).astype(np.float32)
    got = alone(ctx, s, (0, 0, -1, 0), rate_in, rate_out)
    assert len(got) == n_out
    TR.check_float(got.view(np.float32), s, rate_in, rate_out, f"SPEC resample_decimate_{rate_in}_{rate_out}")
    assert np.array_equal(alone(ctx, s, (0, 0, -1, 0), rate_in, rate_out, True), R.pcm16(got.view(np.float32)))


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_row_and_leave_the_context_usable():
    """every refusal of include/zvx.h but one: no rate pair the bank is built for (max(L, M) <= 640: at most 74 KiB of bank) exceeds a
    workgroup's LDS, so that ZVX_E_UNSUPPORTED cannot be reached through the call, here as in zvx_resample_ex"""
    ctx = TR.ctx_for("tiny")
    ri, ro = 22050, 48000
    samples, wins, cnt = case(ri, ro)
    sel = [1, 3, 9]
    s3, good, c3 = [samples[i] for i in sel], [wins[i] for i in sel], [cnt[i] for i in sel]
    x, n = pack_rows(s3)
    stride = max(c3) + 11
    want = rows_host(ctx, s3, good, ri, ro, c3)

    def call(w=good, reserved=None, rates=(ri, ro), n_=n, flags=0, stride_=stride, x_=x, out_=True, win_=True, B=None):
        out = out_rows(3, stride, False)
        rc = raw_rows(ctx, x_, n_, rates[0], rates[1], out if out_ else None, stride_, TRW.windows_array(w, reserved) if win_ else None, flags, None,
                      B=B, Nmax=x.shape[1])
        return rc, out, (err(ctx) or b"").decode()

    def still_serves(name):
        out = rows_host(ctx, s3, good, ri, ro, c3)
        assert np.array_equal(out, want), name
    o, begin, c, last = good[1]
    bad = {
        "win NULL": (dict(win_=False), INV, "win is NULL"),
        "reserved": (dict(reserved={2: 1}), INV, "row 2"),
        "last 2": (dict(w=[good[0], (o, begin, c, 2), good[2]]), INV, "row 1"),
        "last -1": (dict(w=[(0, 0, 700, -1), good[1], good[2]]), INV, "row 0"),
        "in_origin < 0": (dict(w=[good[0], (-1, begin, c, 0), good[2]]), INV, "row 1"),
        "out_begin < 0": (dict(w=[good[0], good[1], (0, -5, 3, 0)]), INV, "row 2"),
        "out_count < -1": (dict(w=[good[0], (o, begin, -2, 0), good[2]]), INV, "row 1"),
        "in_origin > 2^40": (dict(w=[good[0], (2 ** 40 + 1, begin, c, 0), good[2]]), INV, "row 1"),
        "out_begin > 2^40": (dict(w=[good[0], good[1], (0, 2 ** 40 + 1, 3, 0)]), INV, "row 2"),
        "out_count > INT32_MAX": (dict(w=[(0, 0, 2 ** 31, 0), good[1], good[2]]), INV, "row 0"),
        "more than INT32_MAX outputs": (dict(w=[good[0], (2 ** 40, 0, -1, 0), good[2]]), INV, "row 1"),
        "out_stride": (dict(stride_=max(c3) - 1), BUF, "out_stride"),
        "rate_in": (dict(rates=(3999, ro)), INV, "3999"),
        "rate_out": (dict(rates=(ri, 192001)), INV, "192001"),
        "rate pair": (dict(rates=(ri, 22051)), UNS, "22051"),
        "nsamples": (dict(n_=np.array([n[0], x.shape[1] + 1, n[2]], np.int32)), INV, "nsamples[1]"),
        "nsamples < 0": (dict(n_=np.array([n[0], n[1], -1], np.int32)), INV, "nsamples[2]"),
        "no sync on the host": (dict(flags=_lib.ZVX_NO_SYNC), INV, "ZVX_NO_SYNC"),
        "unknown flag": (dict(flags=64), INV, "unknown flag"),
        "out NULL": (dict(out_=False), INV, "out is NULL"),
        "B": (dict(B=0), INV, "B = 0"),
    }
    for name, (kw, code, word) in bad.items():
        rc, out, msg = call(**kw)
        assert rc == code and word in msg, (name, rc, msg)
        assert "zvx_resample_rows" in msg or name.startswith("rate"), (name, msg)      # (the rate checks are the context's, shared by every caller)
        assert np.all(out == S32), (name, "something was written")
        still_serves(name)
    rc, out, msg = call(x_=None)
    assert rc == INV and "zvx_resample_rows" in msg and np.all(out == S32)
    assert ctx._lib.zvx_resample_rows(ctx._h, vp(x), None, 3, x.shape[1], ri, ro, vp(out), stride, None, 0, TRW.windows_array(good)) == INV
    still_serves("NULL arrays")
    # out_stride exactly the longest cnt_b serves
    rc, out, _ = call(stride_=max(c3))
    assert rc == 0
    flat = out.reshape(-1)
    for b in range(3):
        assert np.array_equal(flat[b * max(c3):b * max(c3) + c3[b]], want[b, :c3[b]]), b


# ------------------------------------------------------------------------------------------------ many streams
TAGS = ("voc.resample", "post.denoise", "post.limit", "post.stream")


def tags_of(ctx):
    ctx.sync()
    t = {t["name"]: t for t in ctx.tag_stats()}
    return {k: ((t[k]["launches"], t[k]["bytes"]) if k in t else (0, 0.0)) for k in TAGS}


@pytest.fixture(scope="module")
def env():
    e = TSM.Env("bf16")
    yield e
    e.model.close()


def stepped_alone(env, spec):
    """the session stepped alone with zvx_stream_next under profile 2 -> [(piece, tags of the step), ...]"""
    s, out = TRW.open_session(env, *spec), []
    while not s.done:
        env.ctx.sync()
        env.ctx.reset_stats()
        piece = s.next_piece().copy()
        out.append((piece, tags_of(env.ctx)))
    s.close()
    return out


def test_many_streams_convert_one_group_per_rate(env):
    ctx = env.ctx
    lim2 = dict(TSM.LIM_KW, window_ms=2.0)
    # (frames, chunk_frames, chunks_per_call, denoiser, limiter, captured output rate)
    specs = [(70, 16, 2, TSM.DN_KW, TSM.LIM_KW, 48000),      # three stages
             (33, 7, 2, None, None, 8000),                   # the conversion alone, another rate, ragged last group
             (70, 16, 1, TSM.DN_KW, None, 0),                # no conversion
             (40, 16, 3, None, lim2, 48000),                 # the first session's rate behind another chain
             (70, 16, 3, None, None, 8000)]
    rates = [sp[5] for sp in specs]
    ctx.set_int("profile", 2)
    try:
        single = [stepped_alone(env, sp) for sp in specs]
        live = [(i, TRW.open_session(env, *sp)) for i, sp in enumerate(specs)]
        at = [0] * len(specs)
        steps, seen = 0, set()
        while live:
            ctx.sync()
            ctx.reset_stats()
            pieces = ctx.stream_next_many([s for _, s in live])
            many = tags_of(ctx)
            emitting = [i for i, _ in live if single[i][at[i]][1]["voc.resample"][0]]
            want = {rates[i] for i in emitting}
            print(steps, many["voc.resample"], emitting, sorted(want))
            assert all(single[i][at[i]][1]["voc.resample"][0] == 1 and rates[i] for i in emitting)
            assert many["voc.resample"][0] == len(want), (steps, many, emitting)           # ONE timed group per rate, not one per session
            assert many["voc.resample"][1] == sum(single[i][at[i]][1]["voc.resample"][1] for i, _ in live), steps
            seen.add((len(emitting), len(want)))
            for (i, s), p in zip(live, pieces):
                ref = single[i][at[i]][0]
                assert len(p) == len(ref) and same_bits(p, ref), (steps, i, at[i], len(p), len(ref))
                at[i] += 1
                assert s.done == (at[i] == len(single[i])), (i, at[i])
            for _, s in live:
                if s.done:
                    s.close()
            live = [(i, s) for i, s in live if not s.done]
            steps += 1
            assert steps < 50
        assert at == [len(v) for v in single]
        assert (4, 2) in seen, seen                          # a step in which four sessions converted through two groups
        assert all(any(len(p) for p, _ in single[i]) for i in range(len(specs)))
    finally:
        ctx.set_int("profile", 0)
