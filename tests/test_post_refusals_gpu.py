"""Which rule refuses a post-processing call that breaks TWO rules at once (include/zvx.h; the order of the checks in csrc/host_post.hip and csrc/zvx.hip).
The entry points share their checks and the call path behind them, so the order in which the checks run is part of what a caller sees:
for every pair below the status, the entry point's name at the head of the message and the rule the message names are asserted, and that
the refused call wrote no output sample and issued no launch.  Every call here is answered on the host; no kernel runs.
The STFT is the small one of tests/test_stream_denoise_gpu.py (n_fft 256, hop 256, window 128): a row that is not empty needs 256 samples."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from stream_util import vp
from zerovox_amd import _lib

import test_stream_denoise_gpu as TSD                        # ctx_for: the tiny generator with a given STFT

GEOM = (256, 256, 128)
B, NMAX = 2, 2 * GEOM[0]
INV, BUF = _lib.ZVX_E_INVALID, _lib.ZVX_E_BUFFER
BAD_FLAG = 1 << 20
SENTINEL = np.uint32(0xDEADBEEF)
NO_SUPPORT = (100, 100, 10, 0)                               # outputs from the window's first sample on, inside the signal: no reach in front
IN_PLACE_OFFSET = (0, 7, 10, 0)                              # out_begin != in_origin
LIMIT, LEVEL = _lib.LimitParams(0.8, 5.0, 4), _lib.LevelParams(-23.0, 20.0, 400.0, 100.0)
DENOISE, MARK = _lib.DenoiseParams(0.5, 0.1), _lib.WatermarkParams(0x1234, 1.0, 250.0, 8000.0, 8, 4, 64, 0)


def rows(lengths=(NMAX, NMAX)):
    rng = np.random.default_rng(5)
    x = (0.5 * rng.standard_normal((B, NMAX))).astype(np.float32)
    return x, np.array(lengths, np.int32)


def filled(shape=(B, NMAX), dtype=np.float32):
    return np.full(shape, SENTINEL, np.uint32).view(dtype)


def windows(*wins):
    return (_lib.RowWindow * len(wins))(*[_lib.RowWindow(o, begin, cnt, last, 0) for o, begin, cnt, last in wins])


def refused(ctx, call, outputs, status, name, rule):
    """`call` is refused with `status`, by a message of `name` that names `rule`; the outputs keep their bits and nothing was launched"""
    before = [o.copy() for o in outputs]
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        rc = call()
        msg = ctx._lib.zvx_last_error(ctx._h).decode()
        ctx.sync()
        launches = sum(t["launches"] for t in ctx.tag_stats())
    finally:
        ctx.set_int("profile", 0)
    assert rc == status, (rc, msg)
    assert msg.startswith(name + ":"), msg
    assert rule in msg, msg
    for o, k in zip(outputs, before):
        assert np.array_equal(o.view(np.uint8), k.view(np.uint8)), msg
    assert launches == 0, (msg, launches)


def test_limit_ex():
    ctx = TSD.ctx_for(*GEOM)
    lib, h, rate = ctx._lib, ctx._h, ctx.get_int("sampling_rate")
    x, n = rows()
    out, peak, gmin = filled(), filled((B,)), filled((B,))

    def call(prm=LIMIT, o=out, stride=NMAX, flags=0, win=(0, 0, -1, 1), xin=x):
        return lambda: lib.zvx_limit_ex(h, vp(xin), vp(n), B, NMAX, rate, C.byref(prm), vp(o), stride, vp(peak), vp(gmin), flags, *win)
    keep = [out, peak, gmin]
    refused(ctx, call(o=None, flags=BAD_FLAG), keep, INV, "zvx_limit_ex", "unknown flag")
    refused(ctx, call(prm=_lib.LimitParams(-1.0, 5.0, 4), win=NO_SUPPORT), keep, INV, "zvx_limit_ex", "ceiling")
    refused(ctx, call(prm=_lib.LimitParams(0.8, 5.0, 3), win=NO_SUPPORT), keep, INV, "zvx_limit_ex", "oversample")
    xio = x.copy()
    refused(ctx, call(o=xio, xin=xio, stride=NMAX - 1, win=IN_PLACE_OFFSET), keep + [xio], INV, "zvx_limit_ex", "smaller than Nmax")
    refused(ctx, call(o=xio, xin=xio, flags=_lib.ZVX_PCM16, win=IN_PLACE_OFFSET), keep + [xio], INV, "zvx_limit_ex", "ZVX_PCM16 cannot run in place")
    assert np.array_equal(xio, x)


def test_level_rows():
    ctx = TSD.ctx_for(*GEOM)
    lib, h, rate = ctx._lib, ctx._h, ctx.get_int("sampling_rate")
    x, n = rows()
    out, lo, hi = filled(), filled((B,)), filled((B,))

    def call(prm=LEVEL, o=out, stride=NMAX, flags=0, win=windows((0, 0, -1, 1), (0, 0, -1, 1)), xin=x):
        return lambda: lib.zvx_level_rows(h, vp(xin), vp(n), B, NMAX, rate, C.byref(prm), vp(o), stride, vp(lo), vp(hi), flags, win)
    keep = [out, lo, hi]
    refused(ctx, call(o=None, flags=BAD_FLAG), keep, INV, "zvx_level_rows", "unknown flag")
    refused(ctx, call(prm=_lib.LevelParams(5.0, 20.0, 400.0, 100.0), win=windows((0, 0, -1, 1), NO_SUPPORT)), keep, INV, "zvx_level_rows", "target_lufs")
    refused(ctx, call(flags=_lib.ZVX_NO_SYNC, win=None), keep, INV, "zvx_level_rows", "ZVX_NO_SYNC needs ZVX_DEVICE_OUT")
    xio = x.copy()
    refused(ctx, call(o=xio, xin=xio, stride=NMAX - 1, win=windows((0, 0, -1, 1), IN_PLACE_OFFSET)), keep + [xio], INV, "zvx_level_rows",
            "smaller than Nmax")
    assert np.array_equal(xio, x)


def test_denoise_rows():
    ctx = TSD.ctx_for(*GEOM)
    lib, h = ctx._lib, ctx._h
    x, n = rows()
    bias = np.full(GEOM[0] // 2 + 1, 0.01, np.float32)
    out = filled()
    whole = windows((0, 0, -1, 1), (0, 0, -1, 1))

    def call(prm=DENOISE, o=out, stride=NMAX, flags=0, win=whole, xin=x, k=n):
        return lambda: lib.zvx_denoise_rows(h, vp(xin), vp(k), B, NMAX, vp(bias), C.byref(prm), vp(o), stride, flags, win)
    refused(ctx, call(o=None, flags=BAD_FLAG), [out], INV, "zvx_denoise_rows", "unknown flag")
    refused(ctx, call(prm=_lib.DenoiseParams(-1.0, 0.1), win=windows((0, 0, -1, 1), NO_SUPPORT)), [out], INV, "zvx_denoise_rows", "strength")
    xio = x.copy()
    refused(ctx, call(o=xio, xin=xio, stride=NMAX - 1, win=windows((0, 0, -1, 1), IN_PLACE_OFFSET)), [out, xio], INV, "zvx_denoise_rows", "smaller than Nmax")
    short = np.array([100, NMAX], np.int32)                  # row 0 is below the STFT's minimum, row 1's window is bad
    refused(ctx, call(k=short, win=windows((0, 0, -1, 1), (0, 0, -1, 2))), [out], INV, "zvx_denoise_rows", "row 1: last is 2")
    refused(ctx, call(k=short, win=windows((0, 0, -1, 1), NO_SUPPORT)), [out], INV, "zvx_denoise_rows", "in front of the window")
    refused(ctx, call(k=short), [out], INV, "zvx_denoise_rows", "row 0 has 100 samples")


def test_watermark_ex():
    ctx = TSD.ctx_for(*GEOM)
    lib, h = ctx._lib, ctx._h
    x, n = rows()
    out = filled()

    def call(prm=MARK, o=out, stride=NMAX, flags=0, win=(0, 0, -1, 1), xin=x, k=n):
        return lambda: lib.zvx_watermark_ex(h, vp(xin), vp(k), B, NMAX, C.byref(prm), vp(o), stride, flags, *win)
    refused(ctx, call(o=None, flags=BAD_FLAG), [out], INV, "zvx_watermark_ex", "unknown flag")
    refused(ctx, call(prm=_lib.WatermarkParams(0x1234, 1.0, 250.0, 8000.0, 8, 0, 64, 0), win=NO_SUPPORT), [out], INV, "zvx_watermark_ex", "band_bins")
    xio = x.copy()
    refused(ctx, call(o=xio, xin=xio, stride=NMAX - 1, win=IN_PLACE_OFFSET), [out, xio], INV, "zvx_watermark_ex", "smaller than Nmax")
    refused(ctx, call(o=xio, xin=xio, win=IN_PLACE_OFFSET), [out, xio], INV, "zvx_watermark_ex", "in place needs out_begin == in_origin")
    short = np.array([100, NMAX], np.int32)
    refused(ctx, call(k=short, win=(0, 0, -2, 1)), [out], INV, "zvx_watermark_ex", "out_count -2")
    refused(ctx, call(k=short), [out], INV, "zvx_watermark_ex", "row 0 has 100 samples")


def test_resample_rows():
    """its own order: out and the windows are looked at before the rates, the rates before the lengths, the stride last (ZVX_E_BUFFER)"""
    ctx = TSD.ctx_for(*GEOM)
    lib, h = ctx._lib, ctx._h
    x, n = rows()
    out, out_len = filled(), np.full(B, -7, np.int32)
    whole = windows((0, 0, -1, 0), (0, 0, -1, 0))

    def call(o=out, stride=NMAX, flags=0, win=whole, rates=(22050, 16000), k=n):
        return lambda: lib.zvx_resample_rows(h, vp(x), vp(k), B, NMAX, rates[0], rates[1], vp(o), stride, vp(out_len), flags, win)
    keep = [out, out_len]
    refused(ctx, call(o=None, flags=BAD_FLAG), keep, INV, "zvx_resample_rows", "out is NULL")
    refused(ctx, call(flags=BAD_FLAG, win=None), keep, INV, "zvx_resample_rows", "unknown flag")
    refused(ctx, call(win=windows((0, 0, -1, 0), (0, 0, -1, 2)), rates=(100, 16000)), keep, INV, "zvx_resample_rows", "row 1: last is 2")
    long = np.array([NMAX, NMAX + 1], np.int32)
    refused(ctx, call(stride=8, k=long), keep, INV, "zvx_resample_rows", "nsamples[1]")
    refused(ctx, call(stride=8), keep, BUF, "zvx_resample_rows", "out_stride 8")


def test_watermark_detect():
    ctx = TSD.ctx_for(*GEOM)
    lib, h = ctx._lib, ctx._h
    x, n = rows()
    score, off, win = filled((B,)), filled((B,), np.int32), filled((B,), np.int32)
    ws, wo = filled((B, 1)), filled((B, 1), np.int32)
    keep = [score, off, win, ws, wo]

    def call(prm=MARK, wf=0, s=score, nwmax=1, flags=0, k=n):
        return lambda: lib.zvx_watermark_detect(h, vp(x), vp(k), B, NMAX, C.byref(prm), wf, vp(s), vp(off), vp(win), vp(ws), vp(wo), nwmax, flags)
    refused(ctx, call(s=None, flags=BAD_FLAG), keep, INV, "zvx_watermark_detect", "unknown flag")
    refused(ctx, call(flags=_lib.ZVX_DEVICE_OUT, s=None), keep, INV, "zvx_watermark_detect", "unknown flag")
    refused(ctx, call(prm=_lib.WatermarkParams(0x1234, 1.0, 250.0, 8000.0, 8, 0, 64, 0), wf=1), keep, INV, "zvx_watermark_detect", "band_bins")
    refused(ctx, call(s=None, wf=1), keep, INV, "zvx_watermark_detect", "is NULL")
    assert ctx.get_int("fft_size") == GEOM[0] and ctx.hop == GEOM[1]      # rows of 512 samples: 2 frames, one window of 2 frames
    refused(ctx, call(k=np.array([100, NMAX], np.int32), nwmax=-1), keep, INV, "zvx_watermark_detect", "NWmax -1")
    # the length rule and the window count are looked at row by row: the first row that breaks either decides
    refused(ctx, call(k=np.array([100, NMAX], np.int32), nwmax=0, wf=2), keep, INV, "zvx_watermark_detect", "row 0 has 100 samples")
    refused(ctx, call(k=np.array([NMAX, 100], np.int32), nwmax=0, wf=2), keep, BUF, "zvx_watermark_detect", "row 0 has 1 windows")


def test_watermark_identify():
    ctx = TSD.ctx_for(*GEOM)
    lib, h = ctx._lib, ctx._h
    x, n = rows()
    K = 3
    keys = np.array([1, 2, 3], np.uint64)
    score, off, win, best = filled((B, K)), filled((B, K), np.int32), filled((B, K), np.int32), filled((B,), np.int32)
    keep = [score, off, win, best]
    short = np.array([100, NMAX], np.int32)

    def call(prm=MARK, ks=keys, nk=K, wf=0, flags=0, k=n):
        return lambda: lib.zvx_watermark_identify(h, vp(x), vp(k), B, NMAX, C.byref(prm), vp(ks), nk, wf, vp(score), vp(off), vp(win), vp(best), flags)
    refused(ctx, call(ks=None, flags=BAD_FLAG), keep, INV, "zvx_watermark_identify", "unknown flag")
    refused(ctx, call(prm=_lib.WatermarkParams(0x1234, 1.0, 250.0, 8000.0, 8, 0, 64, 0), nk=0), keep, INV, "zvx_watermark_identify", "band_bins")
    refused(ctx, call(ks=None, nk=0), keep, INV, "zvx_watermark_identify", "keys is NULL")
    refused(ctx, call(nk=0, wf=1), keep, INV, "zvx_watermark_identify", "K 0")
    refused(ctx, call(wf=1, k=short), keep, INV, "zvx_watermark_identify", "window_frames 1")
    many = np.arange(70000, dtype=np.uint64)                 # more keys than a call takes (ZVX_E_UNSUPPORTED), behind the length rule
    refused(ctx, call(ks=many, nk=len(many), k=short), keep, INV, "zvx_watermark_identify", "row 0 has 100 samples")
