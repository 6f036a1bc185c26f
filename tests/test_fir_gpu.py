"""The equaliser's FIR filter on the MI355X: zvx_fir / zvx_fir_ex / zvx_fir_rows against tests/fir_ref.py (float64 NumPy, never the library),
BIT FOR BIT -- the contract fixes the accumulator (double, from +0.0), the order (ascending k) and the one rounding, and the product of two
f32 values is exact in double, so there is no tolerance anywhere in this file.  Every comparison asserts first, on the REFERENCE, that no
output has 0 < |y| < 2^-126 (the one thing the contract leaves open), so nothing is masked.
Shapes: the smallest at which a tile edge, a halo or a 32-bit index can go wrong -- rows of 1, 700, T - 1, T, T + 1 and 2 T + 1 samples (T =
zvx_get_int("fir_tile")), filters of 1 .. 4096 taps with the delay at both ends and in the middle, windows at 2^33."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fir_ref as F
from stream_util import same_bits, vp
from zerovox_amd import _lib, config as zcfg, equaliser as E, pack, weights as zw
from zerovox_amd.stream import stream_windows

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
DEV = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT
_state, _ref = {}, {}


def ctx():
    """a tiny synthetic context (reduced model, tiny vocoder), as tests/test_denoise_gpu.py builds it"""
    if "ctx" not in _state:
        cfg = zcfg.reduced_modelcfg("styletts")
        h = zcfg.hifigan_config("tiny")
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
        _state["ctx"] = _lib.Context(man, blob, 0)
    return _state["ctx"]


def tile():
    T = ctx().get_int("fir_tile")
    assert T > 0 and T % 4 == 0
    return T


def signal(n, seed):
    rng = np.random.default_rng(4242 + seed)
    i = np.arange(n)
    x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 37.3 * i / 1024 + 0.4) + 0.2 * np.sin(2 * np.pi * 120.0 * i / 1024 + 1.1)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def taps(K, seed=0):
    h = (np.random.default_rng(900 + K + seed).standard_normal(K) / np.sqrt(K)).astype(np.float32)
    h.setflags(write=False)
    return h


def batch():
    """(rows, x [B][odd Nmax] with the sentinel behind every row, n), computed once and left unchanged"""
    if "batch" not in _state:
        T = tile()
        lengths = (1, 700, T - 1, T, T + 1, 2 * T + 1)
        rows = [signal(k, b) for b, k in enumerate(lengths)]
        n = np.array(lengths, np.int32)
        nmax = int(n.max())
        x = np.full((len(rows), nmax + (nmax % 2 == 0)), SENTINEL32, np.uint32).view(np.float32)       # nothing behind a row's end may be read
        for b, r in enumerate(rows):
            x[b, :n[b]] = r
        for a in (x, n):
            a.setflags(write=False)
        _state["batch"] = (rows, x, n)
    return _state["batch"]


def reference(K, D, seed=0):
    """fir_ref on every row of the batch, once per (K, D); the precondition of a bit comparison is asserted here"""
    key = (K, D, seed)
    if key not in _ref:
        rows = batch()[0]
        _ref[key] = [F.fir(r, taps(K, seed), D) for r in rows]
        assert all(F.no_subnormal(y) for y in _ref[key]), key
    return _ref[key]


def sentinel_rows(B, stride, pcm16=False):
    return np.full((B, stride), SENTINEL16, np.int16) if pcm16 else np.full((B, stride), SENTINEL32, np.uint32).view(np.float32)


def untouched(out, cnt):
    """everything behind a row's emitted samples still holds the sentinel"""
    s = SENTINEL16 if out.dtype == np.int16 else SENTINEL32
    v = out if out.dtype == np.int16 else out.view(np.uint32)
    return all(np.all(v[b, cnt[b]:] == s) for b in range(len(cnt)))


def raw(c, x, n, Nmax, h, K, D, out, stride, flags=0, B=None, window=None, windows=None):
    B = len(n) if B is None else B
    head = (c._h, vp(x), vp(n), B, Nmax, vp(h), K, D, vp(out), stride, flags)
    if windows is not None:
        return c._lib.zvx_fir_rows(*head, windows)
    if window is not None:
        return c._lib.zvx_fir_ex(*head, *window)
    return c._lib.zvx_fir(*head)


def run(c, x, n, h, D, pcm16=False, stride=None, window=None, windows=None):
    """zvx_fir / _ex / _rows on host rows into a sentinel-filled buffer -> out [B][stride]"""
    B, Nmax = x.shape
    stride = Nmax + 3 if stride is None else stride
    out = sentinel_rows(B, stride, pcm16)
    rc = raw(c, x, n, Nmax, h, len(h), D, out, stride, _lib.ZVX_PCM16 if pcm16 else 0, window=window, windows=windows)
    assert rc == 0, c._lib.zvx_last_error(c._h)
    return out


def row_windows(ws):
    win = (_lib.RowWindow * len(ws))()
    for b, (o, bg, cnt, last) in enumerate(ws):
        win[b] = _lib.RowWindow(int(o), int(bg), int(cnt), 1 if last else 0, 0)
    return win


@pytest.mark.parametrize("K", [1, 2, 63, 64, 255, 1023, 4096])
def test_bits_of_the_float64_reference(K):
    c = ctx()
    rows, x, n = batch()
    for D in sorted({0, (K - 1) // 2, K - 1}):
        out = run(c, x, n, taps(K), D)
        assert untouched(out, n), (K, D)
        for b, ref in enumerate(reference(K, D)):
            assert same_bits(out[b, :n[b]], ref), (K, D, b, int(n[b]))


def test_corners_and_row_independence():
    c = ctx()
    rows, x, n = batch()
    B, Nmax = x.shape
    # K = 1, h = {1}, D = 0: x's values, -0.0 becomes +0.0
    xz = np.array(x)
    xz[1, 5] = np.float32(-0.0)
    out = run(c, xz, n, np.ones(1, np.float32), 0)
    assert untouched(out, n) and out.view(np.uint32)[1, 5] == 0
    for b in range(B):
        assert np.array_equal(out[b, :n[b]], xz[b, :n[b]]) and not np.signbit(out[b, :n[b]][xz[b, :n[b]] == 0]).any(), b
        keep = np.ones(n[b], bool)
        if b == 1:
            keep[5] = False
        assert same_bits(out[b, :n[b]][keep], xz[b, :n[b]][keep]), b
    # all-zero taps: +0.0 everywhere
    out = run(c, x, n, np.zeros(63, np.float32), 31)
    assert untouched(out, n) and all(not out.view(np.uint32)[b, :n[b]].any() for b in range(B))
    # n == 0 writes nothing, and the neighbours are what they are alone
    K, D = 255, 127
    n0 = np.array(n)
    n0[[0, 3]] = 0
    out0 = run(c, x, n0, taps(K), D)
    assert untouched(out0, n0)
    ref = reference(K, D)
    for b in (1, 2, 4, 5):
        assert same_bits(out0[b, :n[b]], ref[b]), b
    # a row alone, under another Nmax and another stride, against the same row in the batch
    for b in (1, 4):
        one = np.full((1, int(n[b]) + 8), SENTINEL32, np.uint32).view(np.float32)
        one[0, :n[b]] = rows[b]
        alone = run(c, one, n[b:b + 1], taps(K), D, stride=one.shape[1] + 11)
        assert untouched(alone, n[b:b + 1]) and same_bits(alone[0, :n[b]], ref[b]), b


def pieces_of(N, size):
    return [(b, min(b + size, N)) for b in range(0, N, size)]


def support(N, b, e, RL, RR):
    """the window with exactly the reach around outputs [b, e) of an N-sample signal -> (in_origin, end, last)"""
    o, end = max(0, b - RL), min(N, e + RR)
    return o, end, end == N


@pytest.mark.parametrize("K,D", [(255, 127), (255, 0), (64, 63)])
def test_windows_concatenate_to_the_whole_call(K, D):
    c = ctx()
    rows, x, n = batch()
    T = tile()
    sig, want = rows[5], reference(K, D)[5]
    N = len(sig)
    assert N == 2 * T + 1
    RL, RR = E.reach(K, D)
    h = taps(K)
    for size in (1, 257, T):
        got = []
        for b, e in pieces_of(N, size):
            o, end, last = support(N, b, e, RL, RR)
            w = np.ascontiguousarray(sig[o:end][None, :])
            out = run(c, w, np.array([end - o], np.int32), h, D, stride=max(w.shape[1], e - b) + 2, window=(o, b, e - b, int(last)))
            assert untouched(out, [e - b]), (size, b)
            got.append(out[0, :e - b])
        assert same_bits(np.concatenate(got), want), (K, D, size)
    # out_count -1 with last: to the end of the signal
    o = max(0, T - RL)
    out = run(c, np.ascontiguousarray(sig[o:][None, :]), np.array([N - o], np.int32), h, D, stride=N, window=(o, T, -1, 1))
    assert untouched(out, [N - T]) and same_bits(out[0, :N - T], want[T:])


def test_windows_far_beyond_32_bits_and_the_support_condition():
    c = ctx()
    rows, x, n = batch()
    K, D = 255, 100
    RL, RR = E.reach(K, D)
    h = taps(K)
    sig = rows[5]
    cnt = 700
    w = np.ascontiguousarray(sig[:RL + cnt + RR][None, :])          # a window in the middle of some long signal: not first, not last
    nw = np.array([w.shape[1]], np.int32)
    small = run(c, w, nw, h, D, window=(1000, 1000 + RL, cnt, 0))
    far = run(c, w, nw, h, D, window=(2 ** 33 + 5, 2 ** 33 + 5 + RL, cnt, 0))
    want = F.fir_window(w[0], h, D, 1000, 1000 + RL, cnt, False)
    assert F.no_subnormal(want)
    assert untouched(small, [cnt]) and untouched(far, [cnt])
    assert same_bits(small[0, :cnt], want) and same_bits(far[0, :cnt], want)
    # one sample short on either side: refused, the message names the row and the side
    out = sentinel_rows(2, w.shape[1])
    two, n2 = np.ascontiguousarray(np.repeat(w, 2, axis=0)), np.repeat(nw, 2)
    win = row_windows([(1000, 1000 + RL, cnt, 0), (1000, 1000 + RL - 1, cnt, 0)])
    assert raw(c, two, n2, w.shape[1], h, K, D, out, w.shape[1], windows=win) == _lib.ZVX_E_INVALID
    msg = c._lib.zvx_last_error(c._h)
    assert b"row 1" in msg and b"RL" in msg and b"in front" in msg, msg
    win = row_windows([(1000, 1000 + RL, cnt, 0), (1000, 1000 + RL + 1, cnt, 0)])
    assert raw(c, two, n2, w.shape[1], h, K, D, out, w.shape[1], windows=win) == _lib.ZVX_E_INVALID
    msg = c._lib.zvx_last_error(c._h)
    assert b"row 1" in msg and b"RR" in msg and b"behind" in msg, msg
    assert raw(c, w, nw, w.shape[1], h, K, D, out, w.shape[1], window=(1000, 1000 + RL - 1, cnt, 0)) == _lib.ZVX_E_INVALID
    assert raw(c, w, nw, w.shape[1], h, K, D, out, w.shape[1], window=(1000, 1000 + RL + 1, cnt, 0)) == _lib.ZVX_E_INVALID
    assert untouched(out, [0, 0])                                    # nothing was written by any of them
    # at the signal's own ends no support is needed
    first = run(c, w, nw, h, D, window=(0, 0, cnt, 0))
    assert same_bits(first[0, :cnt], F.fir_window(w[0], h, D, 0, 0, cnt, False))
    tail = run(c, w, nw, h, D, window=(1000, 1000 + RL, -1, 1))
    assert same_bits(tail[0, :cnt + RR], F.fir_window(w[0], h, D, 1000, 1000 + RL, -1, True)) and untouched(tail, [cnt + RR])


def test_rows_call_equals_the_window_call_on_each_row():
    c = ctx()
    T = tile()
    K, D = 255, 127
    RL, RR = E.reach(K, D)
    h = taps(K)
    N = 2 * T + 1
    sigs = [signal(N, 50 + b) for b in range(8)]
    spans = [(0, 1), (0, 300), (5, T + 5), (T - 1, T + 1), (T, 2 * T), (700, 700), (N - 1, N), (3, N)]      # (begin, end) of the outputs; one empty
    ws, wins = [], []
    for sig, (b, e) in zip(sigs, spans):
        o, end, last = support(N, b, e, RL, RR)
        ws.append(sig[o:end])
        wins.append((o, b, e - b, last))
    n = np.array([len(w) for w in ws], np.int32)
    Nmax = int(n.max()) + 1
    x = np.full((8, Nmax), SENTINEL32, np.uint32).view(np.float32)
    for b, w in enumerate(ws):
        x[b, :n[b]] = w
    cnt = [e - b for b, e in spans]
    together = run(c, x, n, h, D, stride=Nmax + 2, windows=row_windows(wins))
    assert untouched(together, cnt)                                  # nothing outside [0, cnt_b), and the empty range writes nothing
    for b in range(8):
        alone = run(c, np.ascontiguousarray(x[b:b + 1]), n[b:b + 1], h, D, window=(wins[b][0], wins[b][1], wins[b][2], int(wins[b][3])))
        want = F.fir(sigs[b], h, D)[spans[b][0]:spans[b][1]]
        assert F.no_subnormal(want)
        assert same_bits(together[b, :cnt[b]], alone[0, :cnt[b]]) and same_bits(together[b, :cnt[b]], want), b
    got = c.fir_rows(ws, h, wins)                                    # and the binding
    assert all(same_bits(got[b], together[b, :cnt[b]]) for b in range(8))


def test_every_form_of_the_call():
    c = ctx()
    rows, x, n = batch()
    B, Nmax = x.shape
    K, D = 255, 127
    h = taps(K)
    ref = reference(K, D)
    d_in, d_out = c.dev_alloc(x.nbytes), c.dev_alloc(x.nbytes)
    try:
        for flags in (0, _lib.ZVX_DEVICE_IN, _lib.ZVX_DEVICE_OUT, DEV):
            c.dev_from_host(d_in, x)
            c.dev_from_host(d_out, sentinel_rows(B, Nmax))
            host_out = sentinel_rows(B, Nmax)
            src = d_in if flags & _lib.ZVX_DEVICE_IN else x
            dst = d_out if flags & _lib.ZVX_DEVICE_OUT else host_out
            assert raw(c, src, n, Nmax, h, K, D, dst, Nmax, flags) == 0, c._lib.zvx_last_error(c._h)
            got = c.dev_to_host(d_out, (B, Nmax), np.float32) if flags & _lib.ZVX_DEVICE_OUT else host_out
            assert untouched(got, n) and all(same_bits(got[b, :n[b]], ref[b]) for b in range(B)), flags
        # in place on device rows equals out of place; queued (no_sync), then zvx_sync
        c.dev_from_host(d_in, x)
        assert raw(c, d_in, n, Nmax, h, K, D, d_in, Nmax, DEV | _lib.ZVX_NO_SYNC) == 0, c._lib.zvx_last_error(c._h)
        c.sync()
        got = c.dev_to_host(d_in, (B, Nmax), np.float32)
        assert all(same_bits(got[b, :n[b]], ref[b]) for b in range(B))
        assert all(same_bits(got[b, n[b]:], x[b, n[b]:]) for b in range(B))          # what lies behind a row is still the input's
        # the binding's in-place form, and a second filter queued behind the first: stream order is the fence
        c.dev_from_host(d_in, x)
        assert c.fir_device(d_in, n, Nmax, h, no_sync=True) is None
        h2 = taps(63)
        c.fir_device(d_in, n, Nmax, h2, 0, no_sync=True)
        got = c.dev_to_host(d_in, (B, Nmax), np.float32)
        for b in range(B):
            want = F.fir(ref[b], h2, 0)
            assert F.no_subnormal(want) and same_bits(got[b, :n[b]], want), b
        # in place on host rows
        xf = np.array(x)
        assert raw(c, xf, n, Nmax, h, K, D, xf, Nmax) == 0
        assert all(same_bits(xf[b, :n[b]], ref[b]) and same_bits(xf[b, n[b]:], x[b, n[b]:]) for b in range(B))
    finally:
        c.dev_free(d_in)
        c.dev_free(d_out)
    # ZVX_PCM16 against the reference's int16; some samples leave [-1, 1]: the rule clamps
    loud = (4.0 * np.asarray(h)).astype(np.float32)
    i16 = run(c, x, n, loud, D, pcm16=True)
    assert untouched(i16, n)
    clipped = 0
    for b in range(B):
        y = F.fir(rows[b], loud, D)
        assert F.no_subnormal(y) and np.array_equal(i16[b, :n[b]], F.pcm16(y)), b
        clipped += int(np.sum(np.abs(y) > 1.0))
    assert clipped > 0
    assert same_bits(c.fir(rows, h)[1, :n[1]], ref[1]) and np.array_equal(c.fir(rows, loud, pcm16=True)[5, :n[5]], F.pcm16(F.fir(rows[5], loud, D)))


def test_a_host_planned_stream_equals_the_whole_row():
    c = ctx()
    K, D = 255, 127
    h = taps(K)
    chunk = 16 * c.hop
    x = signal(3 * chunk + 777, 99)
    whole = c.fir([x], h)[0, :len(x)]
    want = F.fir(x, h, D)
    assert F.no_subnormal(want) and same_bits(whole, want)
    chunks = [x[i:i + chunk] for i in range(0, len(x), chunk)]
    pieces = list(stream_windows(chunks, E.FirPlanner(K, D), lambda s, o, b, cnt, last: c.fir_window(
        [s], h, D, in_origin=o, out_begin=b, out_count=cnt, last=last)[0].copy()))
    assert len(pieces) == len(chunks) + 1 and len(pieces[0]) == chunk - D            # the stream runs RR = D samples behind its input
    assert same_bits(np.concatenate(pieces), whole)


def test_errors_leave_the_context_usable():
    c = ctx()
    rows, x, n = batch()
    B, Nmax = x.shape
    K, D = 63, 31
    h = taps(K)
    inv, uns = _lib.ZVX_E_INVALID, _lib.ZVX_E_UNSUPPORTED
    out = np.zeros((B, Nmax), np.float32)
    good = run(c, x, n, h, D, stride=Nmax)
    nan, inf = float("nan"), float("inf")

    def refused(code, x_=x, n_=n, B_=None, Nmax_=Nmax, h_=h, K_=K, D_=D, out_=out, stride=Nmax, flags=0, says=None, **kw):
        """the call is refused with `code`, and a valid call on the same context then gives the bits it gave before"""
        assert raw(c, x_, n_, Nmax_, h_, K_, D_, out_, stride, flags, B=B_, **kw) == code
        if says is not None:
            msg = c._lib.zvx_last_error(c._h)
            assert all(s in msg for s in says), msg
        assert same_bits(run(c, x, n, h, D, stride=Nmax), good)

    assert c._lib.zvx_fir(None, vp(x), vp(n), B, Nmax, vp(h), K, D, vp(out), Nmax, 0) == inv
    # the rows-call checks of zvx_limit
    refused(inv, x_=None)
    refused(inv, n_=None, B_=B)
    refused(inv, out_=None)
    for bad in (0, -1):
        refused(inv, B_=bad)
    refused(inv, Nmax_=0)
    neg, big = n.copy(), n.copy()
    neg[1], big[1] = -1, Nmax + 1
    refused(inv, n_=neg)
    refused(inv, n_=big)
    refused(inv, stride=Nmax - 1)
    for flags in (64, _lib.ZVX_HOST_ASYNC, _lib.ZVX_NATIVE_RATE, _lib.ZVX_NO_SYNC):
        refused(inv, flags=flags)
    xf = np.array(x)
    refused(inv, x_=xf, out_=xf, flags=_lib.ZVX_PCM16)
    for kw in (dict(stride=Nmax + 2), dict(flags=_lib.ZVX_DEVICE_IN), dict(flags=_lib.ZVX_DEVICE_OUT)):
        refused(inv, x_=xf, out_=xf, **kw)
    assert same_bits(xf, x)                                          # nothing was written by any of them
    z = np.zeros((65536, 1), np.float32)
    refused(uns, x_=z, n_=np.zeros(65536, np.int32), Nmax_=1, out_=np.zeros((65536, 1), np.float32), stride=1)
    # the filter
    refused(inv, h_=None, says=[b"taps"])
    for k in (0, -1):
        refused(inv, K_=k, says=[b"ntaps"])
    long = np.zeros(_lib.ZVX_FIR_MAX_TAPS + 1, np.float32)
    refused(uns, h_=long, K_=len(long), D_=0, says=[b"4096"])
    for d in (-1, K):
        refused(inv, D_=d, says=[b"delay"])
    for k, v in ((0, nan), (7, inf), (K - 1, -inf)):
        bad = np.array(h)
        bad[k] = v
        refused(inv, h_=bad, says=[b"taps[%d]" % k])
    # the windows
    for w in ((-1, 0, 5, 0), (0, -1, 5, 0), (0, 0, -2, 1), (0, 0, 5, 2), (0, 0, -1, 0), (5, 0, 5, 1), (0, 0, Nmax + 1, 1)):
        refused(inv, window=w)
    n100 = np.full(B, 100, np.int32)
    refused(inv, n_=n100, window=(10, 10 + K - 1 - D - 1, 5, 1), says=[b"row 0", b"RL"])
    refused(inv, n_=n100, window=(0, 0, 100 - D + 1, 0), says=[b"row 0", b"RR"])
    refused(inv, x_=xf, out_=xf, n_=n100, window=(0, 1, 5, 1), says=[b"in place"])
    win = row_windows([(0, 0, -1, 1)] * B)
    win[2].reserved = 1
    refused(inv, windows=win, says=[b"row 2", b"reserved"])
    assert c._lib.zvx_fir_rows(c._h, vp(x), vp(n), B, Nmax, vp(h), K, D, vp(out), Nmax, 0, None) == inv
    # the limits of the valid ranges are accepted
    full = taps(_lib.ZVX_FIR_MAX_TAPS)
    for d in (0, _lib.ZVX_FIR_MAX_TAPS - 1):
        assert raw(c, x, n, Nmax, full, len(full), d, out, Nmax) == 0
    assert same_bits(run(c, x, n, h, D, stride=Nmax), good)


THREE = "The quick brown fox jumps over the lazy dog; does it, really? Pack my box with five dozen liquor jugs"


def test_tts_and_tts_long_with_the_equaliser():
    from zerovox_amd.longform import peak_ceiling
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    c = synth.model.ctx
    rate = c.get_int("sampling_rate")
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    text = "The quick brown fox jumps over the lazy dog"
    eq = E.params("presence", rate)
    h, D = eq["taps"], eq["delay"]
    c.set_int("profile", 2)
    try:
        c.reset_stats()
        plain, ph, length = synth.tts(text, spk, eq=None)
        assert "post.fir" not in {t["name"] for t in c.tag_stats()}          # without the keyword nothing of the equaliser runs
        c.reset_stats()
        shaped, ph2, length2 = synth.tts(text, spk, eq="presence")
        tags = {t["name"]: t for t in c.tag_stats()}
        assert tags["post.fir"]["launches"] == 1 and tags["post.fir"]["bytes"] == 8.0 * len(plain) and tags["post.fir"]["ms"] > 0
        assert tags["post.fir"]["flops"] == 2.0 * len(h) * len(plain)
    finally:
        c.set_int("profile", 0)
    assert length2 == length and np.array_equal(ph, ph2) and shaped.dtype == np.float32 and len(shaped) == len(plain)
    want = F.fir(plain, h, D)
    assert F.no_subnormal(want) and same_bits(shaped, want)
    print(f"tts: eq='presence' moves the row by up to {float(np.abs(shaped - plain).max()):.3e} (peak {float(np.abs(plain).max()):.3f})")
    assert float(np.abs(shaped - plain).max()) > 0
    assert same_bits(synth.tts(text, spk)[0], plain)
    # the chain: denoise, equalise, normalise
    chain = synth.tts(text, spk, denoise=0.5, eq="presence", loudness=-23.0)[0]
    step = c.denoise([plain], synth.denoise_bias, 0.5)[0, :len(plain)]
    step = c.fir([step], h, D)[0, :len(plain)]
    step = c.normalize([step], -23.0, peak_ceiling=peak_ceiling(-1.0))[0][0, :len(plain)]
    assert same_bits(chain, step)
    # tts_long: the same layout whenever nothing is trimmed; every sentence is its own row filtered
    kw = dict(trim_db=0.0, fade_ms=0, pauses={".": 0, ";": 0, ",": 0, " ": 0})
    wav0, seg0 = synth.tts_long(THREE, spk, **kw)
    wav1, seg1 = synth.tts_long(THREE, spk, eq="presence", **kw)
    assert len(seg0) == 3 and [(s["start"], s["samples"], s["mel_len"], s["trim"]) for s in seg1] == [(s["start"], s["samples"], s["mel_len"], s["trim"]) for s in seg0]
    assert len(wav1) == len(wav0)
    for i, s in enumerate(seg1):
        want = F.fir(wav0[s["start"]:s["start"] + s["samples"]], h, D)
        assert F.no_subnormal(want) and same_bits(wav1[s["start"]:s["start"] + s["samples"]], want), i
    # ... and with the gain and the limiter behind it: the call without eq, rebuilt through post_chain_device with the REFERENCE filter
    # at the sentence rows -- the equaliser runs before both, so the level and the peak are those of the equalised rows
    from zerovox_amd.longform import LOUDNESS_MODES, limit_keywords
    wav2, seg2 = synth.tts_long(THREE, spk, eq="presence", loudness=-23.0, limiter=True, peak_db=-20.0, **kw)
    assert [(s["start"], s["samples"]) for s in seg2] == [(s["start"], s["samples"]) for s in seg0]
    lengths = np.array([s["samples"] for s in seg0], np.int32)
    stride = int(lengths.max()) + 5
    rows = np.zeros((3, stride), np.float32)
    for i, s in enumerate(seg0):
        rows[i, :lengths[i]] = F.fir(wav0[s["start"]:s["start"] + s["samples"]], h, D)
    buf = c.dev_alloc(rows.nbytes)
    try:
        c.dev_from_host(buf, rows)
        loud, lim = synth.model.post_chain_device(buf, lengths, stride, loudness=dict(target=-23.0, peak_ceiling=0.0, common=LOUDNESS_MODES["paragraph"]),
                                                  limiter=limit_keywords(True, 5.0, -20.0), rate=rate)
        rebuilt = c.dev_to_host(buf, rows.shape, np.float32)
    finally:
        c.dev_free(buf)
    for i, s in enumerate(seg2):
        assert same_bits(wav2[s["start"]:s["start"] + s["samples"]], rebuilt[i, :lengths[i]]), i
        assert s["gain"] == float(loud[2][i]) and s["min_gain"] == float(lim[1][i]), i
    assert float(min(lim[1])) < 1.0                                  # the limiter did act on the equalised rows
    with pytest.raises(ValueError):
        synth.tts(text, spk, eq="loud")
