"""Float64 NumPy restatement of zvx_fir (include/zvx.h), never the library.

    y[i] = sum over k = 0 .. K-1 of h[k] * x[i + D - k],  x zero outside the signal,

with a double accumulator from +0.0, the terms added in ASCENDING k (vectorised over i: every output sees its own terms in that order), one
rounding to float32.  The product of two float32 values is exact in double, so NumPy's multiply-then-add gives the bits of a fused
multiply-add and the result is a function of the order alone: the device's output is compared bit for bit, with no tolerance."""
import numpy as np


def _padded(x, left, right):
    """x as float64 with `left` zeros in front and `right` behind"""
    x = np.asarray(x, np.float32)
    p = np.zeros(left + len(x) + right, np.float64)
    p[left:left + len(x)] = x
    return p


def _sum(p, first, count, h):
    """acc[e] = sum_k h[k] * p[first + e - k] for e < count, ascending k, from +0.0"""
    acc = np.zeros(count, np.float64)
    for k in range(len(h)):
        acc += h[k] * p[first - k:first - k + count]
    return acc


def fir64(x, h, D):
    """the accumulators of zvx_fir on one row before their one rounding -> float64 [len(x)]"""
    x = np.asarray(x, np.float32)
    h64 = np.asarray(h, np.float32).astype(np.float64)
    K = len(h64)
    assert K >= 1 and 0 <= D <= K - 1
    p = _padded(x, K - 1, K - 1)
    # p[K - 1 + j] = x[j]; output i reads x[i + D - k] = p[K - 1 + i + D - k]
    return _sum(p, K - 1 + D, len(x), h64)


def fir(x, h, D):
    """zvx_fir on one row -> float32 [len(x)]"""
    return fir64(x, h, D).astype(np.float32)


def count(n, in_origin, out_begin, out_count):
    return int(out_count) if out_count >= 0 else max(0, int(in_origin) + int(n) - int(out_begin))


def supported(n, K, D, in_origin, out_begin, out_count, last):
    """the support condition of zvx_fir_ex for one row: reach K - 1 - D to the left, D to the right"""
    cnt = count(n, in_origin, out_begin, out_count)
    if cnt <= 0:
        return True
    end_in, end_out = in_origin + n, out_begin + cnt
    if in_origin > out_begin or end_out > end_in:
        return False
    if in_origin != 0 and out_begin - (K - 1 - D) < in_origin:
        return False
    return bool(last) or end_out - 1 + D <= end_in - 1


def fir_window(x, h, D, in_origin, out_begin, out_count=-1, last=True):
    """zvx_fir_ex on one row: x holds samples [in_origin, in_origin + len(x)) of its signal; what lies outside the window is read as zero,
    which the support condition makes the signal's own zeros -> the outputs [out_begin, out_begin + cnt) as float32"""
    x = np.asarray(x, np.float32)
    h64 = np.asarray(h, np.float32).astype(np.float64)
    K = len(h64)
    assert supported(len(x), K, D, in_origin, out_begin, out_count, last), (len(x), K, D, in_origin, out_begin, out_count, last)
    cnt = count(len(x), in_origin, out_begin, out_count)
    p = _padded(x, K - 1, K - 1)
    return _sum(p, K - 1 + int(out_begin - in_origin) + D, cnt, h64).astype(np.float32)


def pcm16(v):
    """the resampler's rule: (int16) trunc(clamp(v * 32760, -32768, 32767)) on f32 samples"""
    v = np.asarray(v, np.float32) * np.float32(32760.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


def no_subnormal(y):
    """the precondition of a bit comparison: no output with 0 < |y| < 2^-126 (the device may flush those)"""
    a = np.abs(np.asarray(y, np.float32))
    return not np.any((a > 0) & (a < np.float32(2.0 ** -126)))
