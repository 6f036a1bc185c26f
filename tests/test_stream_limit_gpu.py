"""The windowed limiter on the MI355X: zvx_limit_ex against zvx_limit on the whole rows, bit for bit -- pieces cut at the kernels' tile
edges, windows with exactly R = 2 W + H samples of support and origins off every alignment --, every form of the call, the identity
with zvx_limit, errors, accounting, and ZeroVoxTTS.tts_stream(peak_db=...) end to end.  The whole-row limiter itself is checked against
the float64 reference in tests/test_limiter_gpu.py; here the reference is that call's own output and every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import join_ref as J
import limit_ref as L
import resample_ref as RS
from stream_util import _ragged_case, same_bits, vp, window_of
from zerovox_amd import _lib, config as zcfg, limiter as LM, pack, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
CEILING = 0.891
RATE = 22050
TILE = _lib.LIMIT_TILE
CASES = [(1, 1), (4, 1), (4, 22), (8, 110), (4, 4096)]      # (os, W)
_ctx, _rows, _whole = {}, {}, {}


def ctx_for(voc="tiny", prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def params(W, os_, ceiling=CEILING):
    ms = W * 1000.0 / RATE
    assert L.window(RATE, ms) == W == LM.window_samples(RATE, ms), (W, ms)
    return _lib.LimitParams(ceiling, ms, os_)


def raw_ex(ctx, x, n, Nmax, prm, out, stride, win, flags=0, B=None, results=True, rate=RATE):
    """zvx_limit_ex; win = (in_origin, out_begin, out_count, last) -> (rc, peak_in, min_gain)"""
    B = len(n) if B is None else B
    peak, gmin = np.full(max(B, 1), -7.0, np.float32), np.full(max(B, 1), -7.0, np.float32)
    rc = ctx._lib.zvx_limit_ex(ctx._h, vp(x), vp(n), B, Nmax, rate, C.byref(prm) if prm is not None else None, vp(out), stride,
                               vp(peak) if results else None, vp(gmin) if results else None, flags, *[int(v) for v in win])
    return rc, peak, gmin


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


def make_rows(seed):
    """speech-like rows of join_ref.make_rows (2047 .. 22050 samples, and the all-loud one) at a peak of 1.6, a row under the ceiling, DC,
    the spike rows; computed once per seed and left unchanged"""
    if seed not in _rows:
        rng = np.random.default_rng(2000 + seed)
        src = J.make_rows(seed)
        rows = L.scaled_rows(src[:4] + [src[-1]])
        rows.append((rng.standard_normal(2500) * 0.1).clip(-0.8, 0.8).astype(np.float32))     # entirely under the ceiling
        rows.append(np.full(3000, 1.0, np.float32))                                           # DC
        rows += spike_rows(rng)
        for r in rows:
            r.setflags(write=False)
        _rows[seed] = rows
    return _rows[seed]


UNDER = 5                                                    # index of the row under the ceiling


def whole(ctx, seed, os_, W):
    """zvx_limit on the whole rows: (out [B][Nmax], peak_in, min_gain), once per case"""
    key = (seed, os_, W)
    if key not in _whole:
        rows = make_rows(seed)
        out, peak, gmin = ctx.limit(rows, CEILING, params(W, os_).window_ms, os_, rate=RATE)
        for a in (out, peak, gmin):
            a.setflags(write=False)
        _whole[key] = (out, peak, gmin)
    return _whole[key]


def cuts_for(n, R):
    """piece boundaries at the tile edge and one sample to either side of it, then two more whose windows start at an origin = 1 mod 4"""
    extra = [c for c in (R + 4 * ((TILE + 300) // 4) + 1, R + 4 * ((2 * TILE + 77) // 4) + 1) if c > TILE + 1]
    return [0] + [c for c in [TILE - 1, TILE, TILE + 1] + sorted(extra) if c < n] + [n]


@pytest.mark.parametrize("os_,W", CASES)
def test_windows_concatenate_to_the_whole_call(os_, W):
    ctx = ctx_for()
    seed = CASES.index((os_, W))
    rows = make_rows(seed)
    want, peak_w, gmin_w = whole(ctx, seed, os_, W)
    R = LM.reach(W, os_)
    assert R == 2 * W + (_lib.LIMIT_ENV_REACH if os_ > 1 else 0)
    prm = params(W, os_)
    origins, calls = set(), 0
    for b, x in enumerate(rows):
        n = len(x)
        if W == 4096 and n < 20000 and b not in (0, UNDER):
            continue                                         # (R = 8203 covers these rows whole; one short row and the quiet one stay in)
        edges = cuts_for(n, R)
        peaks, gmins = [], []
        for begin, end in zip(edges[:-1], edges[1:]):
            o, w_end, last = window_of(n, begin, end, R)
            origins.add(o)
            xin = np.ascontiguousarray(x[o:w_end])
            k, cnt = len(xin), end - begin
            stride = k + 5
            out = np.full((2, stride), SENTINEL32, np.uint32)                         # one row more than the call owns
            rc, peak, gmin = raw_ex(ctx, xin, np.array([k], np.int32), k, prm, out, stride, (o, begin, cnt, last))
            assert rc == 0, (b, begin, end, ctx._lib.zvx_last_error(ctx._h))
            calls += 1
            assert np.array_equal(out[0, :cnt], want[b, begin:end].view(np.uint32)), (os_, W, b, n, begin, end, o, last)
            assert np.all(out[0, cnt:] == SENTINEL32) and np.all(out[1] == SENTINEL32), (b, begin, "written outside the emitted range")
            peaks.append(peak[0]); gmins.append(gmin[0])
        assert same_bits(np.max(peaks), peak_w[b]) and same_bits(np.min(gmins), gmin_w[b]), (b, peaks, peak_w[b], gmins, gmin_w[b])
    assert any(o % 4 == 1 for o in origins) and sum(o % 2 for o in origins) >= 2, sorted(origins)      # odd, and no multiple of 4
    assert same_bits(want[UNDER, :len(rows[UNDER])], rows[UNDER]) and any(g < 1.0 for g in gmin_w)
    print(f"os {os_} W {W}: R {R}, {calls} windows, origins {sorted(origins)[:8]} ...")


@pytest.mark.parametrize("os_,W", CASES)
def test_a_ragged_batch_to_the_end_of_every_row(os_, W):
    ctx = ctx_for()
    seed = CASES.index((os_, W))
    rows = make_rows(seed)
    want, peak_w, gmin_w = whole(ctx, seed, os_, W)
    R = LM.reach(W, os_)
    o = 101
    begin = o + R
    held = [r[o:] for r in rows]
    n = np.array([len(r) for r in held], np.int32)
    B, Nmax = len(rows), int(n.max()) + 1                    # the sentinel behind every row: nothing there may be read
    x = np.full((B, Nmax), SENTINEL32, np.uint32).view(np.float32)
    for b, r in enumerate(held):
        x[b, :n[b]] = r
    stride = Nmax + 3
    out = np.full((B + 1, stride), SENTINEL32, np.uint32)
    rc, peak, gmin = raw_ex(ctx, x, n, Nmax, params(W, os_), out, stride, (o, begin, -1, 1))
    assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
    emitted = 0
    for b, r in enumerate(rows):
        cnt = max(0, len(r) - begin)
        emitted += cnt
        assert np.array_equal(out[b, :cnt], want[b, begin:len(r)].view(np.uint32)), (b, cnt)
        assert np.all(out[b, cnt:] == SENTINEL32), (b, "written behind cnt_b")
        if cnt == 0:
            assert peak[b] == 0.0 and gmin[b] == 1.0, (b, peak[b], gmin[b])
        else:                                                # over the emitted range only: never beyond the whole row's values
            assert 0.0 < peak[b] <= peak_w[b] and gmin_w[b] <= gmin[b] <= 1.0, (b, peak[b], peak_w[b], gmin[b], gmin_w[b])
    assert np.all(out[B] == SENTINEL32) and emitted > 0
    # the binding's list form: the same window
    o2, p2, g2 = ctx.limit_window(held, CEILING, params(W, os_).window_ms, os_, in_origin=o, out_begin=begin, rate=RATE)
    assert same_bits(p2, peak) and same_bits(g2, gmin) and o2.shape == (B, max(0, max(len(r) for r in rows) - begin))
    for b, r in enumerate(rows):
        cnt = max(0, len(r) - begin)
        assert same_bits(o2[b, :cnt], want[b, begin:len(r)]) and not o2[b, cnt:].any(), b


def test_every_form_of_the_call():
    ctx = ctx_for()
    os_, W = 4, 22
    seed = CASES.index((os_, W))
    rows = make_rows(seed)
    want = whole(ctx, seed, os_, W)[0]
    R = LM.reach(W, os_)
    prm = params(W, os_)
    b, begin, end = 4, TILE + 2, 3 * TILE + 19               # the all-loud row (the limiter acts); outputs over more than two tiles
    o, w_end, last = window_of(len(rows[b]), begin, end, R)
    assert o % 2 == 1 and last == 0
    xin = np.ascontiguousarray(rows[b][o:w_end])
    k, cnt = len(xin), end - begin
    nn = np.array([k], np.int32)
    win = (o, begin, cnt, last)
    stride = k + 3
    ref = np.full((1, stride), SENTINEL32, np.uint32)
    rc, peak, gmin = raw_ex(ctx, xin, nn, k, prm, ref, stride, win)
    assert rc == 0 and np.array_equal(ref[0, :cnt], want[b, begin:end].view(np.uint32)) and gmin[0] < 1.0
    din = ctx.dev_alloc(k * 4 + 16)
    dout = ctx.dev_alloc(2 * stride * 4 + 16)
    try:
        ctx.dev_from_host(din + 4, xin)                      # the device rows sit one float off a 16-byte boundary
        # device in -> host out
        out = np.full((2, stride), SENTINEL32, np.uint32)
        rc, p1, g1 = raw_ex(ctx, din + 4, nn, k, prm, out, stride, win, _lib.ZVX_DEVICE_IN)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        assert np.array_equal(out[0], ref[0]) and np.all(out[1] == SENTINEL32) and same_bits(p1, peak) and same_bits(g1, gmin)
        # host in -> device out, at a pointer one float off
        ctx.dev_from_host(dout, np.full(2 * stride + 4, SENTINEL32, np.uint32))
        rc, p2, g2 = raw_ex(ctx, xin, nn, k, prm, dout + 4, stride, win, _lib.ZVX_DEVICE_OUT)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        flat = ctx.dev_to_host(dout, (2 * stride + 4,), np.uint32)
        assert flat[0] == SENTINEL32 and np.array_equal(flat[1:1 + stride], ref[0]) and np.all(flat[1 + stride:] == SENTINEL32)
        assert same_bits(p2, peak) and same_bits(g2, gmin)
        # the queued form: device in, device out, nothing comes back before the sync
        ctx.dev_from_host(dout, np.full(2 * stride + 4, SENTINEL32, np.uint32))
        rc, p3, g3 = raw_ex(ctx, din + 4, nn, k, prm, dout + 4, stride, win, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC, results=False)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        ctx.sync()
        assert np.array_equal(ctx.dev_to_host(dout, (2 * stride + 4,), np.uint32), flat)
        # ZVX_PCM16, on the host and on the device (an int16 pointer one sample off a 4-byte boundary)
        pcm = np.full((2, stride), SENTINEL16, np.int16)
        rc, p4, g4 = raw_ex(ctx, xin, nn, k, prm, pcm, stride, win, _lib.ZVX_PCM16)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        want16 = RS.pcm16(want[b, begin:end])
        assert np.array_equal(pcm[0, :cnt], want16) and np.all(pcm[0, cnt:] == SENTINEL16) and np.all(pcm[1] == SENTINEL16)
        assert same_bits(p4, peak) and same_bits(g4, gmin)
        ctx.dev_from_host(dout, np.full(2 * stride + 8, SENTINEL16, np.int16))
        rc, _, _ = raw_ex(ctx, din + 4, nn, k, prm, dout + 2, stride, win, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_PCM16)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        flat16 = ctx.dev_to_host(dout, (2 * stride + 8,), np.int16)
        assert flat16[0] == SENTINEL16 and np.array_equal(flat16[1:1 + cnt], want16) and np.all(flat16[1 + cnt:] == SENTINEL16)
    finally:
        ctx.dev_free(dout)
        ctx.dev_free(din)
    # an empty range: nothing is written, 0 and 1 come back
    out = np.full((1, stride), SENTINEL32, np.uint32)
    rc, p5, g5 = raw_ex(ctx, xin, nn, k, prm, out, stride, (o, begin, 0, 0))
    assert rc == 0 and np.all(out == SENTINEL32) and p5[0] == 0.0 and g5[0] == 1.0


@pytest.mark.parametrize("os_,W", CASES)
def test_origin_zero_to_the_end_is_zvx_limit(os_, W):
    ctx = ctx_for()
    seed = CASES.index((os_, W))
    rows = make_rows(seed)
    want, peak_w, gmin_w = whole(ctx, seed, os_, W)
    n = np.array([len(r) for r in rows], np.int32)
    B, Nmax = want.shape
    x = np.full((B, Nmax), SENTINEL32, np.uint32).view(np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    stride = Nmax + 6
    out = np.full((B + 1, stride), SENTINEL32, np.uint32)
    rc, peak, gmin = raw_ex(ctx, x, n, Nmax, params(W, os_), out, stride, (0, 0, -1, 1))
    assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
    assert same_bits(peak, peak_w) and same_bits(gmin, gmin_w)
    for b in range(B):
        assert np.array_equal(out[b, :n[b]], want[b, :n[b]].view(np.uint32)), b
        assert np.all(out[b, n[b]:] == SENTINEL32), b
    assert np.all(out[B] == SENTINEL32)
    o2, p2, g2 = ctx.limit_window(rows, CEILING, params(W, os_).window_ms, os_, rate=RATE)      # the binding's defaults are that call
    assert same_bits(o2, want) and same_bits(p2, peak_w) and same_bits(g2, gmin_w)


def test_window_errors_leave_the_context_usable():
    ctx = ctx_for()
    cs = _ragged_case(2, 16, 7)
    before = ctx.synthesize(*cs, None, want_mel=False)
    os_, W = 4, 22
    R = LM.reach(W, os_)
    prm = params(W, os_)
    rng = np.random.default_rng(3)
    k = 1500
    x = (rng.standard_normal((2, k)) * 0.7).astype(np.float32)
    n = np.array([k, k], np.int32)
    out = np.zeros((2, k), np.float32)
    inv = _lib.ZVX_E_INVALID
    lib, h = ctx._lib, ctx._h
    o = 1001

    def ex(win, x_=x, n_=n, out_=out, stride=k, flags=0, prm_=prm, B_=None, Nmax_=k, rate=RATE):
        return raw_ex(ctx, x_, n_, Nmax_, prm_, out_, stride, win, flags, B=B_, rate=rate)[0]

    good = (o, o + R, k - 2 * R, 0)                          # exactly R on either side
    assert ex(good) == 0, lib.zvx_last_error(h)
    # the window's own parameters
    assert ex((-1, o + R, 10, 0)) == inv and ex((0, -1, 10, 0)) == inv
    assert ex((o, o + R, -2, 1)) == inv
    assert ex((o, o + R, -1, 0)) == inv and b"last" in lib.zvx_last_error(h)
    assert ex((o, o + R, 10, 2)) == inv and ex((o, o + R, 10, -1)) == inv
    # outputs outside the window's samples
    assert ex((o, o - 1, 10, 1)) == inv and ex((o, o + R, k - R + 1, 1)) == inv
    # support short by exactly one sample, on the left and on the right; exactly R is accepted
    assert ex((o, o + R - 1, 10, 0)) == inv
    msg = lib.zvx_last_error(h)
    assert b"row 0" in msg and b"R = %d" % R in msg and b"1 more" in msg, msg
    assert ex((o, o + R, k - 2 * R + 1, 0)) == inv
    msg = lib.zvx_last_error(h)
    assert b"row 0" in msg and b"R = %d" % R in msg and b"1 more" in msg, msg
    assert ex((o, o + R, k - 2 * R + 1, 1)) == 0 and ex((0, R - 1, 10, 0)) == 0 and ex((0, 0, k - R, 0)) == 0      # the signal's own ends need none
    assert ex((0, 0, k - R + 1, 0)) == inv
    short = np.array([k, k - 1], np.int32)                   # per row: row 1 ends one sample early
    assert ex(good, n_=short) == inv and b"row 1" in lib.zvx_last_error(h)
    # the stride, in place
    assert ex(good, stride=k - 2 * R - 1) == inv and ex(good, stride=k - 1) == inv
    xf = np.array(x)
    assert ex(good, x_=xf, out_=xf) == inv and b"in place" in lib.zvx_last_error(h)
    assert np.array_equal(xf, x)
    assert ex((o, o, k, 1), x_=xf, out_=xf, flags=_lib.ZVX_PCM16) == inv and ex((o, o, k, 1), x_=xf, out_=xf, stride=k + 2) == inv
    assert ex((0, 0, -1, 1), x_=xf, out_=xf) == 0            # out_begin == in_origin: zvx_limit's in-place form
    want = ctx.limit(x, CEILING, prm.window_ms, os_, rate=RATE, lengths=n)[0]
    assert same_bits(xf, want)
    # every check of zvx_limit still stands
    assert lib.zvx_limit_ex(None, vp(x), vp(n), 2, k, RATE, C.byref(prm), vp(out), k, None, None, 0, 0, 0, -1, 1) == inv
    assert ex(good, x_=None) == inv and ex(good, n_=None, B_=2) == inv and ex(good, prm_=None) == inv and ex(good, out_=None) == inv
    assert ex(good, B_=0) == inv and ex(good, Nmax_=0) == inv and ex(good, rate=3999) == inv
    for flags in (64, _lib.ZVX_HOST_ASYNC, _lib.ZVX_NATIVE_RATE, _lib.ZVX_NO_SYNC, 128, 256, 1 << 20):
        assert ex(good, flags=flags) == inv, flags
    assert ex(good, prm_=_lib.LimitParams(CEILING, prm.window_ms, 3)) == inv and ex(good, prm_=_lib.LimitParams(0.0, prm.window_ms, 4)) == inv
    assert ex(good, prm_=_lib.LimitParams(CEILING, 4097 * 1000.0 / RATE, 4)) == _lib.ZVX_E_UNSUPPORTED
    assert ex(good) == 0
    after = ctx.synthesize(*cs, None, want_mel=False)
    assert same_bits(after["wav"], before["wav"]) and np.array_equal(after["mel_len"], before["mel_len"])


def test_window_accounting():
    ctx = ctx_for()
    os_, W = 4, 22
    R = LM.reach(W, os_)
    rows = make_rows(2)[:5]
    o = 7
    held = [r[o:] for r in rows]
    total = float(sum(len(r) for r in held))
    begin = o + R
    emitted = float(sum(max(0, len(r) + o - begin) for r in held))
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.limit_window(held, CEILING, params(W, os_).window_ms, os_, in_origin=o, out_begin=begin, rate=RATE)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert [t for t in tags if t != "post.limit" and tags[t]["launches"]] == [] and tags["post.limit"]["launches"] == 1, tags
        assert tags["post.limit"]["bytes"] == 4.0 * total + 4.0 * emitted and tags["post.limit"]["ms"] > 0
        ctx.reset_stats()
        ctx.limit_window([held[3]], CEILING, params(W, os_).window_ms, os_, in_origin=o, out_begin=begin, out_count=1000, last=False, pcm16=True, rate=RATE)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert [t for t in tags if t != "post.limit" and tags[t]["launches"]] == [] and tags["post.limit"]["launches"] == 1, tags
        assert tags["post.limit"]["bytes"] == 4.0 * len(held[3]) + 2.0 * 1000
    finally:
        ctx.set_int("profile", 0)


TEXT = "The quick brown fox jumps over the lazy dog"


def test_tts_stream_under_a_ceiling():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    try:
        ctx = synth.model.ctx
        spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
        ceiling = 10 ** (-20 / 20)
        plain = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16)))
        pieces = list(synth.tts_stream(TEXT, spk, chunk_frames=16, peak_db=-20.0))
        got = np.concatenate(pieces)
        want = ctx.limit([plain], ceiling, 5.0, 4)[0][0]
        assert len(pieces) >= 2 and got.dtype == np.float32
        assert same_bits(got, want)
        assert not same_bits(got, plain)                     # at -20 dBFS the limiter acts on this model
        assert np.all(np.abs(got) <= np.float32(ceiling))    # exactly
        # the stream runs R samples behind the vocoder: the first piece is R short of a chunk, the last piece brings the rest
        R = LM.reach(LM.window_samples(22050, 5.0), 4)
        assert R == 231 and len(pieces[0]) == 16 * ctx.hop - R
        assert same_bits(np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, chunks_per_call=3, peak_db=-20.0))), want)
        assert same_bits(np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16))), plain)      # the unlimited stream is as it was
        synth.output_rate = 48000
        try:
            up = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, peak_db=-20.0)))
            conv, conv_len = ctx.resample([want], 22050, 48000)
            assert same_bits(up, conv[0, :conv_len[0]])
        finally:
            synth.output_rate = None
        with pytest.raises(ValueError):
            synth.tts_stream(TEXT, spk, limiter=True)
    finally:
        synth.model.close()
