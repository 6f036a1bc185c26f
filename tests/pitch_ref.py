"""The float64 restatement of include/zvx.h's zvx_pitch block (YIN on a frame grid): the sequential double sums, the list of AMBIGUOUS frames
per row and the nearest-rank statistics.  NumPy only; shared by tests/test_pitch.py (the definition against the truth) and
tests/test_pitch_gpu.py (the device against the definition), which also take their signals from here."""
import math

import numpy as np

REL = 1e-9                                                   # the ambiguity band of the header block


def geometry(rate, fmin, fmax, window=None):
    """-> (tau_min, tau_max, W, c): the lags formed in double from the f32 parameters, as the C side forms them"""
    tmin = max(2, int(math.floor(float(rate) / float(np.float32(fmax)))))
    tmax = int(math.ceil(float(rate) / float(np.float32(fmin))))
    W = 2 * tmax if window is None else int(window)
    return tmin, tmax, W, (W + tmax) // 2


def _near(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


def frame(v, W, tmin, tmax, fs, threshold, gate):
    """one frame from its W + tau_max samples (float64) -> (f0 Hz or 0.0, aper, ambiguous, d')"""
    P = float(np.sum(v[:W] ** 2)) / W
    # d[tau] = sum_j (v[j] - v[j + tau])^2: a [W][tau_max] table of differences reduced along j, row after row (sequential in j)
    idx = np.arange(W)[:, None] + np.arange(1, tmax + 1)[None, :]
    d = np.empty(tmax + 1)
    d[0] = 0.0
    d[1:] = ((v[:W, None] - v[idx]) ** 2).sum(axis=0)
    c = np.cumsum(d[1:])
    dn = np.ones(tmax + 1)
    pos = c > 0.0
    dn[1:][pos] = d[1:][pos] * np.arange(1, tmax + 1)[pos] / c[pos]
    rng = dn[tmin:tmax + 1]
    amb = _near(P, gate) or bool(np.any(np.abs(rng - threshold) <= REL * np.maximum(np.abs(rng), threshold)))
    below = np.flatnonzero(rng < threshold)
    if below.size == 0 or not P > gate:
        return 0.0, float(rng.min()), amb, dn
    T = tmin + int(below[0])
    while T + 1 <= tmax:
        amb = amb or _near(dn[T + 1], dn[T])
        if not dn[T + 1] < dn[T]:
            break
        T += 1
    delta = 0.0
    if T - 1 >= 1 and T + 1 <= tmax:
        a, b, e = dn[T - 1], dn[T], dn[T + 1]
        den = a - 2.0 * b + e
        if den > 0.0 and abs((a - e) / (2.0 * den)) <= 1.0:
            delta = (a - e) / (2.0 * den)
    return fs / (T + delta), float(dn[T]), amb, dn


def track(x, rate, fmin=60.0, fmax=500.0, threshold=0.15, gate_db=-60.0, window=None, hop=None):
    """one row (its f32 samples) -> dict(f0 float32 [F], aper float32 [F], frames, ambiguous: the list of ambiguous frame indices,
    f0_64 / aper_64: the same before the rounding to f32)"""
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1)
    n = x.size
    tmin, tmax, W, c = geometry(rate, fmin, fmax, window)
    H = max(1, int(rate) // 100) if hop is None else int(hop)
    F = n // H
    thr, gate = float(np.float32(threshold)), 10.0 ** (float(np.float32(gate_db)) / 10.0)
    f0, ap, amb = np.zeros(F), np.zeros(F), []
    for f in range(F):
        s = f * H - c
        v = np.zeros(W + tmax)
        lo, hi = max(s, 0), min(s + W + tmax, n)
        if hi > lo:
            v[lo - s:hi - s] = x[lo:hi]
        f0[f], ap[f], a, _ = frame(v, W, tmin, tmax, float(rate), thr, gate)
        if a:
            amb.append(f)
    return dict(f0=f0.astype(np.float32), aper=ap.astype(np.float32), f0_64=f0, aper_64=ap, frames=F, ambiguous=amb)


def stats(f0):
    """the statistics of one f32 track -> dict(frames, voiced, median, low, high, mean), nearest rank with integer divisions"""
    f0 = np.asarray(f0, np.float32)
    k = np.sort(f0[f0 > 0].astype(np.float64), kind="stable")
    nv = int(k.size)
    if nv == 0:
        return dict(frames=int(f0.size), voiced=0, median=0.0, low=0.0, high=0.0, mean=0.0)
    return dict(frames=int(f0.size), voiced=nv, median=float(k[((nv - 1) * 50 + 50) // 100]), low=float(k[((nv - 1) * 5 + 50) // 100]),
                high=float(k[((nv - 1) * 95 + 50) // 100]), mean=float(k.sum() / nv))


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / np.asarray(ref, np.float64))


# ---- the signals of the tests (float32 rows)
def harmonic(f0, n, rate, amps=(1.0, 0.5, 0.25), scale=1.0):
    """sum_k amps[k - 1] sin(2 pi k f0 t), k = 1 .. len(amps)"""
    t = np.arange(n, dtype=np.float64) / rate
    return (scale * sum(a * np.sin(2.0 * np.pi * (k + 1) * f0 * t) for k, a in enumerate(amps))).astype(np.float32)


def glide(f_from, f_to, n, rate, amps=(1.0, 0.5, 0.25)):
    """a linear glide of the fundamental over the n samples -> (row, the instantaneous fundamental per sample)"""
    t = np.arange(n, dtype=np.float64) / rate
    T = n / rate
    phase = 2.0 * np.pi * (f_from * t + (f_to - f_from) * t * t / (2.0 * T))
    return sum(a * np.sin((k + 1) * phase) for k, a in enumerate(amps)).astype(np.float32), f_from + (f_to - f_from) * t / T


def noise(n, level=0.1, seed=0):
    return (level * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


P8K = dict(rate=8000, fmin=80.0, fmax=400.0, window=200, hop=80)           # the parameters of the 8 kHz cases


def rows_8k():
    """the 8 kHz rows of the tests by name, in the order of the ragged GPU batch"""
    g, inst = glide(100.0, 200.0, 4000, 8000)
    return dict(h100=harmonic(100.0, 2400, 8000), h155=harmonic(155.3, 2400, 8000), h220=harmonic(220.0, 2400, 8000),
                strong2=harmonic(130.0, 2400, 8000, amps=(1.0, 2.5)), noise=noise(2400), silence=np.zeros(2400, np.float32),
                quiet=harmonic(100.0, 2400, 8000, scale=3e-4), glide=g,
                short=harmonic(100.0, 79, 8000), empty=np.zeros(0, np.float32)), inst
