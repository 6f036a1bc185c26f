"""Float64 NumPy reference of the library's true-peak meter and look-ahead limiter, written from include/zvx.h (zvx_true_peak, zvx_limit):
the oversampled signal, the envelope, depth, hold, smoothing and gain, and per sample the radius E[i] that the GPU tests' error bound
scales with.  Independent of the library: nothing here imports zerovox_amd.  The filter and its f32 error bound are resample_ref's."""
import numpy as np

import resample_ref as RS

TAPS = 21                                                    # taps per oversampled point, whatever os


def window(rate, window_ms):
    """W = max(1, rint(rate * window_ms / 1000)) with window_ms the f32 the parameter struct carries"""
    return max(1, int(np.rint(float(rate) * float(np.float32(window_ms)) / 1000.0)))


def weights(W):
    """w[k + W], k = -W .. W: the raised cosine over 2 W + 1 samples, divided by its own sum"""
    k = np.arange(-W, W + 1, dtype=np.float64)
    w = (1.0 + np.cos(np.pi * k / (W + 1))) / (2.0 * (W + 1))
    return w / w.sum()


def oversample(x, os):
    """-> (y [os n], A [os n]) in float64: y[m] = sum_k h[m - k os] x[k] with h = resample_ref.design(1, os), x = 0 outside the row, and the
    magnitude sum A[m] = sum_k |h| |x| of resample_ref.bound.  Phase by phase: y[os q + p] = sum_j h[os j + p] x[q - j]."""
    x = np.asarray(x, np.float64)
    n = len(x)
    L, M, half, h = RS.design(1, os)
    assert (L, M, half) == (os, 1, 10 * os) and RS.taps_per_output(1, os) == TAPS
    y, A = np.zeros(os * n), np.zeros(os * n)
    if n == 0:
        return y, A
    j = np.arange(-10, 11)
    for p in range(os):
        m = os * j + p
        hp = np.where(np.abs(m) <= half, h[np.clip(m + half, 0, 2 * half)], 0.0)
        y[p::os] = np.convolve(x, hp)[10:10 + n]
        A[p::os] = np.convolve(np.abs(x), np.abs(hp))[10:10 + n]
    return y, A


def running_max(v, W):
    """out[i] = max of v[j] over |j - i| <= W, 0 <= j < len(v) (v >= 0)"""
    v = np.asarray(v, np.float64)
    n = len(v)
    if n == 0:
        return v.copy()
    m = np.concatenate([np.zeros(W), v, np.zeros(W + 1)])    # m[a] = v[a - W]
    P = 1
    while 2 * P <= 2 * W + 1:                                # m[a] = max over [a, a + 2 P)
        m = np.maximum(m, np.concatenate([m[P:], np.zeros(P)]))
        P *= 2
    a = np.arange(n)
    return np.maximum(m[a], m[a + 2 * W + 1 - P])


def envelope(x, os):
    """-> (e [n] float64, be [n]): e[i] = max(|x[i]|, |y[m]| for os (i - 1) < m < os (i + 1), 0 <= m < os n); be[i] = the largest
    resample_ref.bound of those oversampled points (0 for os = 1)."""
    ax = np.abs(np.asarray(x, np.float64))
    n = len(ax)
    if os == 1 or n == 0:
        return ax, np.zeros(n)
    y, A = oversample(x, os)
    bd = RS.bound(1, os, A)
    ay = np.abs(y).reshape(n, os)
    bd = bd.reshape(n, os)
    own, own_b = ay.max(axis=1), bd.max(axis=1)              # points os i .. os i + os - 1
    between, between_b = ay[:, 1:].max(axis=1), bd[:, 1:].max(axis=1)     # strictly between i and i + 1: they also count for i + 1
    prev, prev_b = np.concatenate([[0.0], between[:-1]]), np.concatenate([[0.0], between_b[:-1]])
    return np.maximum(ax, np.maximum(own, prev)), np.maximum(own_b, prev_b)


def toward_zero_f32(g):
    g = np.asarray(g, np.float64)
    f = g.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(g)
    return np.where(over, np.nextafter(f, np.float32(0.0)), f).astype(np.float32)


def limit(x, ceiling, W, os):
    """-> dict(out f32 [n], g f64, g32 f32, e f64, d f64, E f64): E[i] = the largest bound of any oversampled point that feeds e[j],
    |j - i| <= 2 W."""
    x32 = np.asarray(x, np.float32)
    n = len(x32)
    c = float(np.float32(ceiling))
    e, be = envelope(x32, os)
    if n == 0:
        z = np.zeros(0)
        return dict(out=np.zeros(0, np.float32), g=z, g32=np.zeros(0, np.float32), e=z, d=z, E=z)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(e > c, 1.0 - c / np.where(e > c, e, 1.0), 0.0)
    r = 1.0 - d
    D = running_max(d, W)
    Dp = np.concatenate([np.full(W, D[0]), D, np.full(W, D[-1])])          # D[clamp(i + k, 0, n - 1)]
    s = 1.0 - np.convolve(Dp, weights(W), mode="valid")
    g = np.minimum(s, r)
    g32 = toward_zero_f32(g)
    return dict(out=x32 * g32, g=g, g32=g32, e=e, d=d, E=running_max(be, 2 * W))


def true_peak(x, os):
    """-> (max(max |x|, max |y|) in float64, the largest bound of any oversampled point); (0, 0) for an empty row"""
    e, be = envelope(np.asarray(x, np.float32), os)
    return (float(e.max()), float(be.max())) if len(e) else (0.0, 0.0)


def over_db(peak, ceiling):
    """how far a peak lies over the ceiling, in dB (negative: under it)"""
    return 20.0 * np.log10(max(float(peak), 1e-300) / float(np.float32(ceiling)))


def scaled_rows(rows, peak=1.6):
    """every row scaled to a sample peak of `peak` (an all-zero row stays)"""
    out = []
    for r in rows:
        m = float(np.max(np.abs(r))) if len(r) else 0.0
        out.append((np.asarray(r, np.float64) * (peak / m)).astype(np.float32) if m > 0 else np.asarray(r, np.float32))
    return out
