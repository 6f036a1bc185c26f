"""float64 / NumPy / SciPy restatement of zvx_level and zvx_level_ex as include/zvx.h states them: sequential, without fma, every unit's
recurrence from zero state over its own 3 h samples (scipy.signal.lfilter in double, the coefficients of tests/loudness_ref.py).  The
windowed form reads its samples through a recorder, so that a test can see how far an output reaches.  Imports nothing from zerovox_amd."""
import numpy as np
from scipy.signal import lfilter

import loudness_ref as LR

GATE = LR.ABS_GATE                           # 10^((-70 + 0.691) / 10)
AMBIGUOUS_REL = 2.3e-4                       # a unit whose p lies within this (relative) of the gate may be decided either way
DEFAULTS = dict(max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0)


def unit_len(rate):
    return (int(rate) + 5) // 10


def geometry(rate, window_ms, lookahead_ms):
    """-> (h, S, a, RL, RR) with the parameters as the f32 the struct carries"""
    h = unit_len(rate)
    S = max(1, int(np.rint(float(np.float32(window_ms)) / 100.0)))
    a = int(np.rint(float(np.float32(lookahead_ms)) / 100.0))
    assert 0 <= a <= S, (a, S)
    return h, S, a, (S + 3 - a) * h - 1, (a + 1) * h - 1


class Window:
    """samples [in_origin, in_origin + len) of a signal that is zero in front of sample 0; `read` records the positions asked for"""

    def __init__(self, samples, in_origin=0):
        self.x = np.asarray(samples, np.float32).astype(np.float64)
        self.origin = int(in_origin)
        self.lo, self.hi = None, None        # the smallest and the largest position >= 0 read so far

    def read(self, begin, end):
        """positions [begin, end) as float64; positions < 0 are zeros and are not recorded; anything else outside the window is an error"""
        out = np.zeros(end - begin, np.float64)
        b = max(begin, 0)
        if b < end:
            assert self.origin <= b and end <= self.origin + len(self.x), ("read outside the window", begin, end, self.origin, len(self.x))
            out[b - begin:] = self.x[b - self.origin:end - self.origin]
            self.lo = b if self.lo is None else min(self.lo, b)
            self.hi = end - 1 if self.hi is None else max(self.hi, end - 1)
        return out


def unit_power(win, q, rate):
    """p[q] = u[q] / h: the recurrence from zero state over samples [(q - 2) h, (q + 1) h), the squares of the last h summed"""
    h = unit_len(rate)
    s1, s2 = LR.coefficients(rate)
    y = lfilter(*s2, lfilter(*s1, win.read((q - 2) * h, (q + 1) * h)))
    return float(np.cumsum(y[2 * h:] ** 2)[-1]) / h         # (cumsum adds one term after the other: the sequential sum)


def units(x, rate):
    """p[0 .. U) of a whole signal"""
    w = Window(x)
    return np.array([unit_power(w, q, rate) for q in range(len(w.x) // unit_len(rate))], np.float64)


def ambiguous(x, rate):
    """the units whose p lies within AMBIGUOUS_REL of the gate"""
    p = units(x, rate)
    return [int(q) for q in np.nonzero(np.abs(p / GATE - 1.0) <= AMBIGUOUS_REL)[0]]


def unit_gain(p_of, q, S, target, max_gain_db):
    """G[q] from p_of(k), k in [max(0, q - S + 1), q] ascending"""
    s, cnt = 0.0, 0
    for k in range(max(0, q - S + 1), q + 1):
        p = p_of(k)
        if p > GATE:
            s += p
            cnt += 1
    if cnt == 0:
        return 1.0
    L = -0.691 + 10.0 * np.log10(s / cnt)
    return float(min(10.0 ** ((target - L) / 20.0), 10.0 ** (max_gain_db / 20.0)))


def gains(p, S, target, max_gain_db=20.0):
    """G[0 .. U) from the unit powers p"""
    target, max_gain_db = float(np.float32(target)), float(np.float32(max_gain_db))
    return np.array([unit_gain(lambda k: p[k], q, S, target, max_gain_db) for q in range(len(p))], np.float64)


def supported(RL, RR, in_origin, n_in, out_begin, cnt, last, geom=None):
    """the support condition of include/zvx.h for the reaches RL / RR; geom = (h, S, a) adds its clamped left rule: a last window that
    begins inside its signal must hold the warm-up of the oldest unit under its first node, which the clamp to U - 1 may have moved left"""
    if cnt <= 0:
        return True
    inside = in_origin <= out_begin and out_begin + cnt <= in_origin + n_in
    left = in_origin == 0 or out_begin - RL >= in_origin
    right = bool(last) or out_begin + cnt - 1 + RR <= in_origin + n_in - 1
    if geom is not None and last and in_origin > 0:
        h, S, a = geom
        U = (in_origin + n_in) // h
        if U > 0:
            kf = max(0, min(out_begin // h + a - 1, U - 1) - S + 1)
            left = left and (kf - 2) * h >= in_origin
    return inside and left and right


def level_window(samples, in_origin, out_begin, out_count, last, rate, target, max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0,
                 record=None, check=True):
    """outputs [out_begin, out_begin + out_count) (out_count -1 with last: to the end) of the leveler on the signal of which `samples` are
    [in_origin, in_origin + len) -> dict(out float32, exact float64 = x * g before any rounding to f32, g32 float32).  Asserts the
    support condition (check=False: only the window's own reader guards, which raises where a read leaves the window).  record: a dict that
    receives lo / hi, the smallest and largest signal position read."""
    h, S, a, RL, RR = geometry(rate, window_ms, lookahead_ms)
    target, max_gain_db = float(np.float32(target)), float(np.float32(max_gain_db))
    win = Window(samples, in_origin)
    n_in = len(win.x)
    cnt = out_count if out_count >= 0 else max(0, in_origin + n_in - out_begin)
    assert out_count >= 0 or last
    assert not check or supported(RL, RR, in_origin, n_in, out_begin, cnt, last, (h, S, a)), (in_origin, n_in, out_begin, cnt, last, RL, RR)
    U = (in_origin + n_in) // h if last else None
    pc, gc = {}, {}

    def p_of(k):
        if k not in pc:
            pc[k] = unit_power(win, k, rate)
        return pc[k]

    def node(j):
        if U == 0:
            return 1.0
        m = max(j + a - 1, 0)
        if U is not None:
            m = min(m, U - 1)
        if m not in gc:
            gc[m] = unit_gain(p_of, m, S, target, max_gain_db)
        return gc[m]

    exact, g32 = np.zeros(cnt, np.float64), np.zeros(cnt, np.float32)
    xs = win.read(out_begin, out_begin + cnt) if cnt else np.zeros(0)
    for e in range(cnt):
        i = out_begin + e
        q = i // h
        t0, t1 = node(q), node(q + 1)
        g = t0 + (t1 - t0) * (float(i - q * h) / float(h))
        exact[e] = xs[e] * g
        g32[e] = np.float32(g)
    if record is not None:
        record["lo"], record["hi"] = win.lo, win.hi
    return dict(out=xs.astype(np.float32) * g32, exact=exact, g32=g32)


def level(x, rate, target, max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0):
    """the whole-signal call"""
    return level_window(x, 0, 0, -1, True, rate, target, max_gain_db, window_ms, lookahead_ms)


def bursts(rng, n, rate, levels, zero_units=0, zero_at=None):
    """a speech-like row of n samples: noise bursts of the given rms levels, one per stretch of 2 .. 4 units, raised-cosine edges, exact
    zeros between them; zero_units > 0 forces an all-zero stretch of that many units from unit zero_at on"""
    h = unit_len(rate)
    x = np.zeros(n, np.float64)
    at, i = 0, 0
    while at < n:
        ln = int(rng.integers(2 * h, 4 * h))
        gap = int(rng.integers(h // 8, h // 2))
        seg = min(ln, n - at)
        env = np.ones(seg)
        ramp = min(seg // 2, h // 4)
        if ramp:
            r = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
            env[:ramp] = r
            env[seg - ramp:] = r[::-1]
        x[at:at + seg] = rng.standard_normal(seg) * env * levels[i % len(levels)]
        at += seg + gap
        i += 1
    if zero_units:
        x[zero_at * h:(zero_at + zero_units) * h] = 0.0
    return np.clip(x, -1.0, 1.0).astype(np.float32)
