"""The windowed denoiser on the MI355X: zvx_denoise_ex against zvx_denoise on the whole rows, bit for bit -- pieces cut around the hop and
the frame length so that the first frame of a window takes every slot of a workgroup, windows with exactly R = n_fft - 1 samples of
support, origins beyond 2^32 --, the identity with zvx_denoise, what is written, errors, accounting, and
ZeroVoxTTS.tts_stream(denoise_strength=...) end to end.  The whole-row denoiser itself is checked against the float64 reference in
tests/test_denoise_gpu.py; here the reference is that call's own output and every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import denoise_ref as D
import denoise_window_ref as DW
from stream_util import err, same_bits, supported, vp, window_of
from zerovox_amd import _lib, config as zcfg, denoiser as DN, pack, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
STRENGTH = 0.5
MAIN = (1024, 256, 1024)
MAIN_LENGTHS = (3149, 2304, 1668)
INV = _lib.ZVX_E_INVALID
_ctx, _batch, _whole = {}, {}, {}


def ctx_for(n_fft=1024, hop=256, win_length=None):
    """a tiny synthetic context (reduced model, tiny vocoder) with the given STFT parameters, as tests/test_denoise_gpu.py builds it"""
    key = (n_fft, hop, win_length or n_fft)
    if key not in _ctx:
        cfg = zcfg.reduced_modelcfg("styletts")
        cfg["audio"].update(fft_size=n_fft, hop_size=hop, win_length=win_length or n_fft)
        h = zcfg.hifigan_config("tiny")
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def signal(rng, n, n_fft):
    i = np.arange(n)
    x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 37.3 * i / n_fft + 0.4) + 0.2 * np.sin(2 * np.pi * 120.0 * i / n_fft + 1.1)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def batch(geom, lengths):
    """(rows, bias): speech-like rows with |x| <= 1 and a bias of the size of their median magnitude; computed once, left unchanged"""
    key = (geom, tuple(lengths))
    if key not in _batch:
        n_fft, hop, wl = geom
        rng = np.random.default_rng(77 + n_fft)
        rows = [signal(rng, k, n_fft) for k in lengths]
        med = np.median(np.concatenate([np.abs(D.analysis(r, n_fft, hop, wl)).ravel() for r in rows]))
        bias = (med * rng.uniform(0.5, 1.5, n_fft // 2 + 1)).astype(np.float32)
        for a in rows + [bias]:
            a.setflags(write=False)
        _batch[key] = (rows, bias)
    return _batch[key]


def whole(geom, lengths, floor, pcm16=False):
    """zvx_denoise on the whole rows in one batch: out [B][Nmax], once per case"""
    key = (geom, tuple(lengths), floor, pcm16)
    if key not in _whole:
        rows, bias = batch(geom, lengths)
        _whole[key] = ctx_for(*geom).denoise(rows, bias, STRENGTH, floor, pcm16=pcm16)
        _whole[key].setflags(write=False)
    return _whole[key]


def raw_ex(ctx, x, n, Nmax, bias, prm, out, stride, win, flags=0, B=None):
    """zvx_denoise_ex; win = (in_origin, out_begin, out_count, last) -> rc"""
    B = len(n) if B is None else B
    return ctx._lib.zvx_denoise_ex(ctx._h, vp(x), vp(n), B, Nmax, vp(bias), C.byref(prm) if prm is not None else None, vp(out), stride, flags,
                                   *[int(v) for v in win])


def first_frame(begin, n_fft, hop):
    """the first frame that covers sample `begin`, on the signal's grid"""
    p = begin + (n_fft - hop) // 2
    return 0 if p < n_fft else (p - n_fft) // hop + 1


def pieces_equal_whole(geom, lengths, floor):
    """every row cut at the issue's boundaries, each piece from the window with exactly R samples of support -> the first frames seen"""
    n_fft, hop, wl = geom
    ctx = ctx_for(*geom)
    rows, bias = batch(geom, lengths)
    want = whole(geom, lengths, floor)
    R = DN.reach(n_fft)
    prm = _lib.DenoiseParams(STRENGTH, floor)
    firsts, lasts = set(), 0
    for b, x in enumerate(rows):
        n = len(x)
        assert not same_bits(want[b, :n], x)                                          # the denoiser acts
        edges = [c for c in DW.cuts(n, n_fft, hop) if c < n] + [n]                    # 0, 1, hop - 1, hop, hop + 1, n_fft, n_fft + 1, n / 2 + 1, n - 1; n
        for begin, end in zip(edges[:-1], edges[1:]):
            o, w_end, last = window_of(n, begin, end, R)
            xin = np.ascontiguousarray(x[o:w_end])
            k, cnt = len(xin), end - begin
            assert supported(R, o, k, begin, cnt, last)
            stride = k + 5
            out = np.full((2, stride), SENTINEL32, np.uint32)                         # one row more than the call owns
            rc = raw_ex(ctx, xin, np.array([k], np.int32), k, bias, prm, out, stride, (o, begin, cnt, last))
            assert rc == 0, (b, begin, end, err(ctx))
            assert np.array_equal(out[0, :cnt], want[b, begin:end].view(np.uint32)), (geom, floor, b, n, begin, end, o, last)
            assert np.all(out[0, cnt:] == SENTINEL32) and np.all(out[1] == SENTINEL32), (b, begin, "written outside the emitted range")
            firsts.add(first_frame(begin, n_fft, hop))
            lasts += last
    assert lasts >= len(rows)
    return firsts


@pytest.mark.parametrize("floor", [0.0, 0.1])
def test_windows_concatenate_to_the_whole_call(floor):
    firsts = pieces_equal_whole(MAIN, MAIN_LENGTHS, floor)
    assert {f % 4 for f in firsts} == {0, 1, 2, 3}, sorted(firsts)                    # every slot of a workgroup of 4 frames


@pytest.mark.parametrize("geom", [(256, 256, 128), (2048, 256, 2048), (4096, 256, 4096)])
def test_windows_at_other_transform_sizes(geom):
    """256 / 256 with a window of 128: pad 0, no overlap, 16 frames per workgroup; 2048: the radix-2 pass, 2 per workgroup; 4096: one"""
    n_fft = geom[0]
    firsts = pieces_equal_whole(geom, (3 * n_fft + 77, 2 * n_fft + 131), 0.1)
    assert len(firsts) >= 3, sorted(firsts)


def interior(geom=MAIN, b=0, o=301, extra=700):
    """an interior window of row b with exactly R on either side: (ctx, xin, n, bias, R, good window, the whole call's bits of its range)"""
    n_fft = geom[0]
    rows, bias = batch(geom, MAIN_LENGTHS)
    R = DN.reach(n_fft)
    k = 2 * R + extra
    xin = np.ascontiguousarray(rows[b][o:o + k])
    assert len(xin) == k
    return ctx_for(*geom), xin, np.array([k], np.int32), bias, R, (o, o + R, extra, 0), whole(geom, MAIN_LENGTHS, 0.1)[b, o + R:o + R + extra]


def test_one_sample_short_of_support_on_either_side():
    ctx, xin, n, bias, R, good, want = interior()
    k, (o, begin, cnt, _) = len(xin), good
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    out = np.zeros((1, k), np.float32)
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, good) == 0, err(ctx)
    assert same_bits(out[0, :cnt], want)
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, (o, begin - 1, cnt, 0)) == INV
    msg = err(ctx)
    assert b"row 0" in msg and b"R = %d" % R in msg and b"1 more" in msg and b"in front" in msg, msg
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, (o, begin, cnt + 1, 0)) == INV
    msg = err(ctx)
    assert b"row 0" in msg and b"R = %d" % R in msg and b"1 more" in msg and b"behind" in msg, msg
    two = np.stack([xin, xin])                                # per row: row 1 ends one sample early
    assert raw_ex(ctx, two, np.array([k, k - 1], np.int32), k, bias, prm, np.zeros((2, k), np.float32), k, good) == INV and b"row 1" in err(ctx)
    again = np.zeros((1, k), np.float32)
    assert raw_ex(ctx, xin, n, k, bias, prm, again, k, good) == 0 and same_bits(again, out)


def test_origin_zero_to_the_end_is_zvx_denoise():
    ctx = ctx_for(*MAIN)
    rows, bias = batch(MAIN, MAIN_LENGTHS)
    want, want16 = whole(MAIN, MAIN_LENGTHS, 0.1), whole(MAIN, MAIN_LENGTHS, 0.1, pcm16=True)
    n = np.array(MAIN_LENGTHS, np.int32)
    B, Nmax = want.shape
    x = np.full((B, Nmax), SENTINEL32, np.uint32).view(np.float32)                    # nothing behind a row's end may be read
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    ident = (0, 0, -1, 1)
    stride = Nmax + 6
    out = np.full((B + 1, stride), SENTINEL32, np.uint32)
    assert raw_ex(ctx, x, n, Nmax, bias, prm, out, stride, ident) == 0, err(ctx)
    pcm = np.full((B + 1, stride), SENTINEL16, np.int16)
    assert raw_ex(ctx, x, n, Nmax, bias, prm, pcm, stride, ident, _lib.ZVX_PCM16) == 0, err(ctx)
    for b in range(B):
        assert np.array_equal(out[b, :n[b]], want[b, :n[b]].view(np.uint32)) and np.all(out[b, n[b]:] == SENTINEL32), b
        assert np.array_equal(pcm[b, :n[b]], want16[b, :n[b]]) and np.all(pcm[b, n[b]:] == SENTINEL16), b
    assert np.all(out[B] == SENTINEL32) and np.all(pcm[B] == SENTINEL16)
    assert same_bits(ctx.denoise_window(rows, bias, STRENGTH, 0.1), want)             # the binding's defaults are that call
    # device in and out, then in place on the device (out_begin == in_origin), then in place on the host
    din, dout = ctx.dev_alloc(B * Nmax * 4 + 16), ctx.dev_alloc(B * Nmax * 4 + 16)
    try:
        ctx.dev_from_host(din, x)
        ctx.dev_from_host(dout, np.full((B, Nmax), SENTINEL32, np.uint32))
        dev = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT
        assert raw_ex(ctx, din, n, Nmax, bias, prm, dout, Nmax, ident, dev) == 0, err(ctx)
        got = ctx.dev_to_host(dout, (B, Nmax), np.uint32)
        assert raw_ex(ctx, din, n, Nmax, bias, prm, din, Nmax, ident, dev | _lib.ZVX_NO_SYNC) == 0, err(ctx)
        ctx.sync()
        inplace = ctx.dev_to_host(din, (B, Nmax), np.uint32)
        for b in range(B):
            assert np.array_equal(got[b, :n[b]], want[b, :n[b]].view(np.uint32)) and np.all(got[b, n[b]:] == SENTINEL32), b
            assert np.array_equal(inplace[b, :n[b]], want[b, :n[b]].view(np.uint32)) and np.all(inplace[b, n[b]:] == SENTINEL32), b
    finally:
        ctx.dev_free(dout)
        ctx.dev_free(din)
    xf = np.array(x)
    assert raw_ex(ctx, xf, n, Nmax, bias, prm, xf, Nmax, ident) == 0, err(ctx)
    for b in range(B):
        assert np.array_equal(xf.view(np.uint32)[b, :n[b]], want[b, :n[b]].view(np.uint32)) and np.all(xf.view(np.uint32)[b, n[b]:] == SENTINEL32), b


def test_nothing_else_is_written_by_a_ragged_window():
    ctx = ctx_for(*MAIN)
    rows, bias = batch(MAIN, MAIN_LENGTHS)
    want, want16 = whole(MAIN, MAIN_LENGTHS, 0.1), whole(MAIN, MAIN_LENGTHS, 0.1, pcm16=True)
    R = DN.reach(MAIN[0])
    o = 101
    begin = o + R
    held = [r[o:] for r in rows]
    n = np.array([len(r) for r in held], np.int32)
    B, Nmax = len(rows), int(n.max()) + 1
    x = np.full((B, Nmax), SENTINEL32, np.uint32).view(np.float32)
    for b, r in enumerate(held):
        x[b, :n[b]] = r
    stride = Nmax + 3
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    out = np.full((B + 1, stride), SENTINEL32, np.uint32)
    pcm = np.full((B + 1, stride), SENTINEL16, np.int16)
    assert raw_ex(ctx, x, n, Nmax, bias, prm, out, stride, (o, begin, -1, 1)) == 0, err(ctx)
    assert raw_ex(ctx, x, n, Nmax, bias, prm, pcm, stride, (o, begin, -1, 1), _lib.ZVX_PCM16) == 0, err(ctx)
    for b, r in enumerate(rows):
        cnt = len(r) - begin
        assert cnt > 0
        assert np.array_equal(out[b, :cnt], want[b, begin:len(r)].view(np.uint32)) and np.all(out[b, cnt:] == SENTINEL32), (b, cnt)
        assert np.array_equal(pcm[b, :cnt], want16[b, begin:len(r)]) and np.all(pcm[b, cnt:] == SENTINEL16), (b, cnt)
    assert np.all(out[B] == SENTINEL32) and np.all(pcm[B] == SENTINEL16)
    # a fixed count for every row (the shorter rows have no R samples behind it: their signals end in the window); device out at a pointer one
    # float off a 16-byte boundary
    cnt = 300
    dout = ctx.dev_alloc((B * stride + 8) * 4)
    try:
        ctx.dev_from_host(dout, np.full(B * stride + 8, SENTINEL32, np.uint32))
        assert raw_ex(ctx, x, n, Nmax, bias, prm, dout + 4, stride, (o, begin + 7, cnt, 1), _lib.ZVX_DEVICE_OUT) == 0, err(ctx)
        flat = ctx.dev_to_host(dout, (B * stride + 8,), np.uint32)
        assert flat[0] == SENTINEL32 and np.all(flat[1 + B * stride:] == SENTINEL32)
        got = flat[1:1 + B * stride].reshape(B, stride)
        for b in range(B):
            assert np.array_equal(got[b, :cnt], want[b, begin + 7:begin + 7 + cnt].view(np.uint32)) and np.all(got[b, cnt:] == SENTINEL32), b
    finally:
        ctx.dev_free(dout)
    o2 = ctx.denoise_window(held, bias, STRENGTH, 0.1, in_origin=o, out_begin=begin)      # the binding's list form: the same window
    assert o2.shape == (B, max(len(r) for r in rows) - begin)
    for b, r in enumerate(rows):
        assert same_bits(o2[b, :len(r) - begin], want[b, begin:len(r)]) and not o2[b, len(r) - begin:].any(), b


def test_origins_beyond_two_to_the_32():
    ctx, xin, n, bias, R, good, want = interior(o=301)
    k, (o, begin, cnt, _) = len(xin), good
    hop = MAIN[1]
    far = hop * 2 ** 24
    assert far == 2 ** 32 and (o + far) % hop == o % hop
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    near_out, far_out = np.full((1, k), SENTINEL32, np.uint32), np.full((1, k), SENTINEL32, np.uint32)
    assert raw_ex(ctx, xin, n, k, bias, prm, near_out, k, good) == 0, err(ctx)
    assert raw_ex(ctx, xin, n, k, bias, prm, far_out, k, (o + far, begin + far, cnt, 0)) == 0, err(ctx)
    assert np.array_equal(near_out[0, :cnt], want.view(np.uint32)) and np.array_equal(far_out, near_out)
    # the signal ends in the window: the frame count and the right mirror come from N = in_origin + n
    near_out[:] = SENTINEL32
    far_out[:] = SENTINEL32
    assert raw_ex(ctx, xin, n, k, bias, prm, near_out, k, (o, begin, -1, 1)) == 0, err(ctx)
    assert raw_ex(ctx, xin, n, k, bias, prm, far_out, k, (o + far, begin + far, -1, 1)) == 0, err(ctx)
    assert np.all(near_out[0, k - R:] == SENTINEL32) and not np.any(near_out[0, :k - R] == SENTINEL32)
    assert np.array_equal(far_out, near_out)
    # ... and is the whole call's tail where the signal is the row itself
    rows, _ = batch(MAIN, MAIN_LENGTHS)
    tail = np.ascontiguousarray(rows[0][o:])
    got = ctx.denoise_window([tail], bias, STRENGTH, 0.1, in_origin=o, out_begin=begin)
    assert same_bits(got[0], whole(MAIN, MAIN_LENGTHS, 0.1)[0, begin:len(rows[0])])
    far_got = ctx.denoise_window([tail], bias, STRENGTH, 0.1, in_origin=o + far, out_begin=begin + far)
    assert same_bits(far_got, got)


def test_copy_empty_range_and_a_non_finite_row():
    ctx, xin, n, bias, R, good, want = interior()
    k, (o, begin, cnt, _) = len(xin), good
    out = np.full((1, k), SENTINEL32, np.uint32)
    assert raw_ex(ctx, xin, n, k, bias, _lib.DenoiseParams(0.0, 0.1), out, k, good) == 0, err(ctx)      # strength 0: the emitted range's input bits
    assert np.array_equal(out[0, :cnt], xin[R:R + cnt].view(np.uint32)) and np.all(out[0, cnt:] == SENTINEL32)
    out[:] = SENTINEL32
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, (o, begin, 0, 0)) == 0, err(ctx)                   # an empty range writes nothing
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, (o, o + k, -1, 1)) == 0, err(ctx)
    assert np.all(out == SENTINEL32)
    two = np.stack([xin, xin])
    two[0, R + 5] = np.nan
    two[0, R + 400] = np.inf
    out2 = np.full((2, k), SENTINEL32, np.uint32)
    assert raw_ex(ctx, two, np.array([k, k], np.int32), k, bias, prm, out2, k, good) == 0, err(ctx)
    assert np.array_equal(out2[1, :cnt], want.view(np.uint32)) and np.all(out2[:, cnt:] == SENTINEL32)
    assert raw_ex(ctx, xin, n, k, bias, prm, out, k, good) == 0 and np.array_equal(out[0, :cnt], want.view(np.uint32))


def test_window_errors_leave_the_context_usable():
    ctx, xin, n1, bias, R, good, want = interior()
    k, (o, begin, cnt, _) = len(xin), good
    mel = np.random.default_rng(5).standard_normal((1, 40, ctx.get_int("n_mels"))).astype(np.float32)
    before = ctx.vocode_mel(mel, np.array([40], np.int32), native_rate=True)
    x = np.stack([xin, xin])
    n = np.array([k, k], np.int32)
    out = np.zeros((2, k), np.float32)
    prm = _lib.DenoiseParams(STRENGTH, 0.1)
    lib, h = ctx._lib, ctx._h

    def ex(win, x_=x, n_=n, out_=out, stride=k, flags=0, prm_=prm, bias_=bias, B_=None, Nmax_=k):
        return raw_ex(ctx, x_, n_, Nmax_, bias_, prm_, out_, stride, win, flags, B=B_)

    assert ex(good) == 0, err(ctx)
    assert same_bits(out[0, :cnt], want) and same_bits(out[1, :cnt], want)
    # the window's own parameters, one case per item of include/zvx.h
    assert ex((-1, begin, 10, 0)) == INV and ex((0, -1, 10, 0)) == INV
    assert ex((o, begin, -2, 1)) == INV
    assert ex((o, begin, -1, 0)) == INV and b"last" in err(ctx)
    assert ex((o, begin, 10, 2)) == INV and ex((o, begin, 10, -1)) == INV
    assert ex(good, stride=cnt - 1) == INV and ex(good, stride=k - 1) == INV
    xf = np.array(x)
    assert ex(good, x_=xf, out_=xf) == INV and b"in place" in err(ctx)
    assert np.array_equal(xf, x)
    assert ex((o, o, k, 1), x_=xf, out_=xf, flags=_lib.ZVX_PCM16) == INV and ex((o, o, k, 1), x_=xf, out_=xf, stride=k + 2) == INV
    # outputs outside the window's samples; the signal's own ends need no support
    assert ex((o, o - 1, 10, 1)) == INV and ex((o, begin, k - R + 1, 1)) == INV
    assert ex((o, begin, cnt + 1, 1)) == 0 and ex((0, R - 1, 10, 0)) == 0 and ex((0, 0, k - R, 0)) == 0
    assert ex((0, 0, k - R + 1, 0)) == INV
    # zvx_melspec's length conditions hold for the whole signal: checked on N_b with last
    short = np.array([300, 300], np.int32)
    assert ex((0, 0, -1, 1), n_=short) == INV and b"row 0" in err(ctx) and b"at least" in err(ctx)
    assert ex((5000, 5000 + R, -1, 1), n_=short) == 0        # N_b = 5300 is long enough; nothing is emitted
    # every check of zvx_denoise still stands
    assert lib.zvx_denoise_ex(None, vp(x), vp(n), 2, k, vp(bias), C.byref(prm), vp(out), k, 0, 0, 0, -1, 1) == INV
    assert ex(good, x_=None) == INV and ex(good, n_=None, B_=2) == INV and ex(good, prm_=None) == INV and ex(good, out_=None) == INV
    assert ex(good, bias_=None) == INV and ex(good, B_=0) == INV and ex(good, Nmax_=0) == INV
    assert ex(good, n_=np.array([k, k + 1], np.int32)) == INV and ex(good, n_=np.array([k, -1], np.int32)) == INV
    for flags in (64, _lib.ZVX_HOST_ASYNC, _lib.ZVX_NATIVE_RATE, _lib.ZVX_NO_SYNC, 128, 256, 1 << 20):
        assert ex(good, flags=flags) == INV, flags
    for bad in (_lib.DenoiseParams(-0.5, 0.1), _lib.DenoiseParams(float("nan"), 0.1), _lib.DenoiseParams(float("inf"), 0.1),
                _lib.DenoiseParams(STRENGTH, -0.1), _lib.DenoiseParams(STRENGTH, 1.5)):
        assert ex(good, prm_=bad) == INV, (bad.strength, bad.floor)
    nb = np.array(bias)
    nb[7] = -1.0
    assert ex(good, bias_=nb) == INV
    nb[7] = np.nan
    assert ex(good, bias_=nb) == INV
    out[:] = 0
    assert ex(good) == 0 and same_bits(out[0, :cnt], want) and same_bits(out[1, :cnt], want)
    assert same_bits(ctx.vocode_mel(mel, np.array([40], np.int32), native_rate=True), before)


def test_window_accounting():
    ctx = ctx_for(*MAIN)
    rows, bias = batch(MAIN, MAIN_LENGTHS)
    R = DN.reach(MAIN[0])
    o = 7
    held = [r[o:] for r in rows]
    total = float(sum(len(r) for r in held))
    begin = o + R
    emitted = float(sum(max(0, len(r) + o - begin) for r in held))
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.denoise_window(held, bias, STRENGTH, 0.1, in_origin=o, out_begin=begin)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert [t for t in tags if t != "post.denoise" and tags[t]["launches"]] == [] and tags["post.denoise"]["launches"] == 1, tags
        assert tags["post.denoise"]["bytes"] == 4.0 * total + 4.0 * emitted and tags["post.denoise"]["ms"] > 0
        ctx.reset_stats()
        ctx.denoise_window([held[0]], bias, STRENGTH, 0.1, in_origin=o, out_begin=begin, out_count=500, last=False, pcm16=True)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        assert [t for t in tags if t != "post.denoise" and tags[t]["launches"]] == [] and tags["post.denoise"]["launches"] == 1, tags
        assert tags["post.denoise"]["bytes"] == 4.0 * len(held[0]) + 2.0 * 500
    finally:
        ctx.set_int("profile", 0)


TEXT = "The quick brown fox jumps over the lazy dog"


def test_tts_stream_denoised():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    try:
        model, ctx = synth.model, synth.model.ctx
        spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
        R = DN.reach(ctx.get_int("fft_size"))
        assert R == 1023
        plain_pieces = list(synth.tts_stream(TEXT, spk, chunk_frames=16))
        plain = np.concatenate(plain_pieces)
        assert model._denoise_bias is None                   # nothing of the denoiser exists before the keyword is used
        pieces = list(synth.tts_stream(TEXT, spk, chunk_frames=16, denoise_strength=0.5))
        assert model._denoise_bias is not None
        bias = model.denoise_bias
        got = np.concatenate(pieces)
        want = ctx.denoise([plain], bias, 0.5)[0]
        assert len(pieces) >= 2 and got.dtype == np.float32
        assert same_bits(got, want) and not same_bits(got, plain)
        # the stream runs R samples behind the vocoder: no piece but the last comes earlier
        assert len(pieces) == len(plain_pieces) + 1
        received, emitted = np.cumsum([len(p) for p in plain_pieces]), np.cumsum([len(p) for p in pieces])
        assert all(emitted[j] == received[j] - R for j in range(len(plain_pieces))) and emitted[-1] == received[-1]
        assert same_bits(np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, chunks_per_call=3, denoise_strength=0.5))), want)
        # with a ceiling as well: limit(denoise(stream))
        limited = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, denoise_strength=0.5, peak_db=-20.0)))
        want_lim = ctx.limit([want], 10 ** (-20 / 20), 5.0, 4)[0][0]
        assert same_bits(limited, want_lim) and not same_bits(limited, want)
        assert same_bits(np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16))), plain)      # the plain stream is as it was
        synth.output_rate = 48000
        try:
            up = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, denoise_strength=0.5)))
            conv, conv_len = ctx.resample([want], 22050, 48000)
            assert same_bits(up, conv[0, :conv_len[0]])
        finally:
            synth.output_rate = None
        with pytest.raises(ValueError, match="denoise"):
            synth.tts_stream(TEXT, spk, denoise=0.01)
    finally:
        synth.model.close()
