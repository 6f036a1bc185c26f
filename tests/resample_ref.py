"""Float64 NumPy reference of the library's sample-rate conversion (include/zvx.h, zvx_resample): the filter design, the
direct-form sum and, per output, the magnitude sum A[n] = sum_k |h[n M - k L]| |x[k]| that the tests' error bound scales with.
Independent of the library: nothing here imports zerovox_amd."""
from math import gcd

import numpy as np

BETA = 5.0
ZEROS = 10


def pair(rate_in, rate_out):
    g = gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def design(rate_in, rate_out):
    """-> (L, M, half, h) with h[m + half], m = -half .. half, in float64."""
    L, M = pair(rate_in, rate_out)
    mx = max(L, M)
    half = ZEROS * mx
    m = np.arange(-half, half + 1, dtype=np.float64)
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (m / half) ** 2))) / np.i0(BETA)
    fc = 1.0 / mx
    h = fc * np.sinc(fc * m) * w
    h = h / h.sum() * L
    return L, M, half, h


def taps_per_output(rate_in, rate_out):
    """T = ceil(N / L): the most taps one output sample has."""
    L, M = pair(rate_in, rate_out)
    N = 2 * ZEROS * max(L, M) + 1
    return -(-N // L)


def out_len(n, rate_in, rate_out):
    L, M = pair(rate_in, rate_out)
    return -(-(int(n) * L) // M)


def resample_window(x, rate_in, rate_out, in_origin=0, out_begin=0, out_count=-1, want_mag=False):
    """x holds samples [in_origin, in_origin + len(x)) of a signal that is zero elsewhere -> outputs [out_begin, out_begin + out_count)
    (out_count -1: to ceil((in_origin + len(x)) L / M)) as float64; with want_mag also A[n]."""
    x = np.asarray(x, np.float64)
    if int(rate_in) == int(rate_out):
        L = M = 1
        half, h = 0, np.ones(1)
    else:
        L, M, half, h = design(rate_in, rate_out)
    if out_count < 0:
        out_count = max(0, -(-((in_origin + len(x)) * L) // M) - out_begin)
    T = -(-(2 * half + 1) // L)
    n = np.arange(out_begin, out_begin + out_count, dtype=np.int64)
    nM = n * M
    ks = -(-(nM - half) // L)                                  # first input sample under the filter
    k = ks[:, None] + np.arange(T, dtype=np.int64)[None, :]
    m = nM[:, None] - k * L
    kk = k - in_origin
    ok = (np.abs(m) <= half) & (kk >= 0) & (kk < len(x))
    hh = np.where(ok, h[np.clip(m + half, 0, 2 * half)], 0.0)
    xx = np.where(ok, x[np.clip(kk, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    y = (hh * xx).sum(axis=1)
    if want_mag:
        return y, (np.abs(hh) * np.abs(xx)).sum(axis=1)
    return y


def resample_ref(x, rate_in, rate_out, want_mag=False):
    """the whole-signal conversion: ceil(len(x) L / M) samples (float64)"""
    return resample_window(x, rate_in, rate_out, 0, 0, -1, want_mag)


def bound(rate_in, rate_out, A):
    """|got - ref| <= (T + 2) 2^-24 A[n] for an f32 implementation: T - 1 additions, one rounding per product, one for each tap's f32
    rounding, one spare for second-order terms; any summation order and any use of FMA stays inside it."""
    return (taps_per_output(rate_in, rate_out) + 2) * 2.0 ** -24 * np.asarray(A, np.float64)


def pcm16(f):
    """(int16) trunc(clamp(f * 32760, -32768, 32767)) on f32 rows, in f32 like the library"""
    v = np.asarray(f, np.float32) * np.float32(32760.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
