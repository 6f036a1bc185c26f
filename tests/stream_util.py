"""What the tests of the windowed steps (zvx_limit_ex, zvx_denoise_ex) share: the support condition of include/zvx.h restated for a reach R,
the window with exactly R of support and chunking; and the small helpers of raw library calls that the other GPU tests use as well."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


def cut(x, sizes):
    """x in chunks of the given sizes (cycled), the last one as short as it comes"""
    out, at, i = [], 0, 0
    while at < len(x):
        out.append(x[at:at + sizes[i % len(sizes)]])
        at += len(out[-1])
        i += 1
    return out


def supported(R, in_origin, n_in, out_begin, cnt, last):
    """the support condition of include/zvx.h, restated for the reach R (zvx_limit_ex: 2 W + H, H = 11 where the envelope is oversampled;
    zvx_denoise_ex: n_fft - 1)"""
    if cnt <= 0:
        return True
    inside = in_origin <= out_begin and out_begin + cnt <= in_origin + n_in
    left = in_origin == 0 or out_begin - R >= in_origin
    right = bool(last) or out_begin + cnt - 1 + R <= in_origin + n_in - 1
    return inside and left and right


def window_of(n, begin, end, R):
    """the window with EXACTLY R samples of support around outputs [begin, end) of an n-sample signal: (in_origin, samples end, last)"""
    o = max(0, begin - R)
    return (o, end + R, 0) if end + R <= n else (o, n, 1)


def vp(a):
    if a is None:
        return None
    return C.c_void_p(int(a)) if isinstance(a, (int, np.integer)) else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def err(ctx):
    return ctx._lib.zvx_last_error(ctx._h)


def _ragged_case(B, T, seed):
    from zerovox_amd import synthetic
    ph, pu, Tl, spk, dur = synthetic.batch(B, T, seed, "uniform")
    Tl = np.array([T] + [max(1, T - 3 * b - 1) for b in range(1, B)], np.int32)
    for b in range(B):
        ph[b, Tl[b]:] = 0; pu[b, Tl[b]:] = 0; dur[b, Tl[b]:] = 0
    return ph, pu, Tl, spk, dur
