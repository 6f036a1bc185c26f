"""float64 / NumPy / SciPy reference of zvx_loudness_stats as include/zvx.h states it, on top of tests/loudness_ref.py: the K-weighting runs
as ONE scipy.signal.lfilter pass per stage over the whole row (carried state: the sequential recurrence), every gate is decided in the
power domain.  Imports nothing from zerovox_amd."""
import numpy as np
from scipy.signal import lfilter

from loudness_ref import ABS_GATE, _lu, coefficients, gated, unit_len

ST_UNITS = 30                    # 100 ms units of a short-term window (3 s)
KEYS = ("integrated", "max_momentary", "max_short_term", "lra", "lra_low", "lra_high", "short_gated", "peak")


def lufs(p):
    """-0.691 + 10 log10 p, -inf where p == 0 (scalars or arrays)"""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(p > 0, -0.691 + 10.0 * np.log10(np.where(p > 0, p, 1.0)), -np.inf)


def unit_powers(x, fs):
    """u[q], q < U = n // h: the sum of the squares of the K-weighted samples of unit q"""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = unit_len(fs)
    U = len(x) // h
    if U == 0:
        return np.zeros(0, np.float64)
    s1, s2 = coefficients(fs)
    y = lfilter(*s2, lfilter(*s1, x))
    return (y[:U * h].reshape(U, h) ** 2).sum(axis=1)


def windows(u, count, h):
    """the mean power of every run of `count` units, summed in ascending index"""
    W = len(u) - count + 1
    if W <= 0:
        return np.zeros(0, np.float64)
    acc = u[:W].copy()
    for k in range(1, count):
        acc = acc + u[k:k + W]
    return acc / (count * h)


def rank_indices(n_g):
    """EBU Tech 3342's nearest ranks round((n - 1) p / 100) for p = 10 and 95, in integers -> (lo, hi)"""
    return ((n_g - 1) * 10 + 50) // 100, ((n_g - 1) * 95 + 50) // 100


def lra_gate(s):
    """both LRA gates over the short-term powers s -> (the gated powers sorted ascending, margin: the smallest distance in LU of any window
    to either gate, inf where nothing is compared)"""
    if len(s) == 0:
        return np.zeros(0, np.float64), np.inf
    margin = float(np.min(_lu(s, ABS_GATE)))
    g = s[s > ABS_GATE]
    if len(g) == 0:
        return g, margin
    thr = 0.01 * g.mean()
    margin = min(margin, float(np.min(_lu(g, thr))))
    return np.sort(g[g > thr]), margin


def measure_row(x, fs):
    """one row -> dict: KEYS as floats, momentary / short_term (the LUFS curves), margin, and int_margin, the integrated measurement's own
    gate margin (loudness_ref.gated)"""
    x32 = np.asarray(x, np.float32)
    h = unit_len(fs)
    u = unit_powers(x32, fs)
    z = ((u[:-3] + u[1:-2]) + u[2:-1]) + u[3:] if len(u) >= 4 else np.zeros(0, np.float64)
    z = z / (4 * h)
    s = windows(u, ST_UNITS, h)
    M, S = lufs(z), lufs(s)
    k, margin = lra_gate(s)
    L, int_margin, _, _ = gated(z)
    r = dict(integrated=float(L), max_momentary=float(M.max()) if len(M) else -np.inf, max_short_term=float(S.max()) if len(S) else -np.inf,
             short_gated=float(len(k)), peak=float(np.abs(x32).max()) if len(x32) else 0.0, momentary=M, short_term=S, margin=margin,
             int_margin=int_margin)
    if len(k):
        lo, hi = rank_indices(len(k))
        r.update(lra=float(10.0 * np.log10(k[hi] / k[lo])), lra_low=float(lufs(k[lo])), lra_high=float(lufs(k[hi])))
    else:
        r.update(lra=0.0, lra_low=-np.inf, lra_high=-np.inf)
    return r


def measure(rows, fs):
    """-> dict: KEYS as [B] float64 arrays, momentary / short_term as lists of curves, margin / int_margin [B]"""
    per = [measure_row(r, fs) for r in rows]
    out = {k: np.array([p[k] for p in per], np.float64) for k in KEYS + ("margin", "int_margin")}
    out["momentary"], out["short_term"] = [p["momentary"] for p in per], [p["short_term"] for p in per]
    return out


def sine_segments(fs, segments, f=1000.0):
    """EBU Tech 3342's test signals: consecutive segments (seconds, dBFS peak level) of one continuous sine -> float32"""
    n = [int(round(sec * fs)) for sec, _ in segments]
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for k, (_, db) in zip(n, segments)])
    t = np.arange(amp.size, dtype=np.float64) / fs
    return (amp * np.sin(2.0 * np.pi * f * t)).astype(np.float32)


# EBU Tech 3342, minimum requirements: (segments, the LRA it asks for within +- 1 LU)
TECH3342 = {
    1: ([(20, -20.0), (20, -30.0)], 10.0),
    2: ([(20, -20.0), (20, -15.0)], 5.0),
    3: ([(20, -40.0), (20, -20.0)], 20.0),
    4: ([(20, -50.0), (20, -35.0), (20, -20.0), (20, -35.0), (20, -50.0)], 15.0),
}
