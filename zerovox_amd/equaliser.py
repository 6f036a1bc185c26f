"""Equaliser: linear-phase FIR taps for zvx_fir (include/zvx.h) from bells, shelves and band edges, and the planner of its stream windows.

Pure NumPy, importable without the library.  The library only filters; what is filtered WITH is designed here, in float64:

  1. a target magnitude in dB over frequency: peaking bands ``(f_hz, gain_db, width_octaves)`` as Gaussian bells over log-frequency
     (width_octaves is the full width at half the gain in dB), shelves ``(f_hz, gain_db)`` that reach half their gain at f_hz
     (gain_db / (1 + (f / f_hz)^2) for the low shelf, its mirror for the high shelf), and Butterworth-MAGNITUDE high- and low-pass slopes
     ``hz`` or ``(hz, order)`` (order 4 by default), floored at -120 dB;
  2. the target is sampled on a dense grid (GRID points up to rate / 2) and brought to the time domain by an inverse real DFT with zero
     phase; the result is even about sample 0;
  3. ONE half of it, samples 0 .. (K - 1) / 2, is cut out, multiplied by one half of a Kaiser window (beta KAISER_BETA) and mirrored: the
     taps are symmetric bit for bit by construction (an irfft result is not: at K = 1023 its two halves differ in the last bit);
  4. the taps are rounded once to float32.  delay = (K - 1) / 2: the filtered signal is time-aligned with its input.

No spec at all -- and any spec whose target is 0 dB everywhere -- gives the exact unit impulse.

What a K-tap filter can and cannot do: it resolves nothing much below about 2 * rate / K (86 Hz at 22.05 kHz and K = 511).  Bells and
shelves wider than that are realised closely; the transition of a steep high-pass near that limit is not, by several dB: deviation_db
says how far the realised response of the float32 taps is from the target, and MEASURED_DEVIATION_DB holds it for every preset (NumPy on
a CPU, no device involved).  Nothing here is a claim of audible merit: the presets are plausible curves, not tuned on a real voice.
"""
from __future__ import annotations

import numpy as np

from .leveler import LevelPlanner
from .stream import stream_windows

MAX_TAPS = 4096                               # ZVX_FIR_MAX_TAPS
GRID = 1 << 15                                # points of the inverse real DFT (GRID / 2 + 1 frequencies up to rate / 2)
KAISER_BETA = 8.0
FLOOR_DB = -120.0                             # the slopes' floor: a magnitude of exactly 0 has no dB
DEFAULT_TAPS = 511

PRESETS = {
    "flat": {},
    "presence": dict(bands=((3000.0, 4.0, 1.5),)),                            # a lift around 3 kHz for a dull voice
    "warm": dict(low_shelf=(250.0, 3.0), high_shelf=(6000.0, -3.0)),          # tames a bright vocoder
    "rumble": dict(highpass_hz=80.0),                                         # takes the rumble off
    "telephone": dict(highpass_hz=300.0, lowpass_hz=3400.0),                  # the 300-3400 Hz telephone band
}

# deviation_db(lo_hz=0) of every preset at 22.05 kHz, measured with NumPy on a CPU: the largest |realised - target| in dB over the
# frequencies where the target is >= -20 dB.  The bell is realised to a few thousandths of a dB and the shelves to a few hundredths; the
# high-pass presets are not: their transition lies at or below the filter's resolution (rumble: several dB between 45 and 80 Hz, and
# 0.012 dB above 200 Hz at K = 511).  tests/test_fir.py asserts 1.5 x these.
MEASURED_DEVIATION_DB = {
    511: {"flat": 0.0, "presence": 3.054e-3, "warm": 6.358e-2, "rumble": 7.344, "telephone": 1.968},
    1023: {"flat": 0.0, "presence": 7.651e-4, "warm": 1.663e-2, "rumble": 4.161, "telephone": 0.5567},
}


def reach(ntaps, delay=None):
    """(RL, RR) = (K - 1 - D, D): how far back and how far ahead an output sample of zvx_fir depends on its input"""
    K = int(ntaps)
    D = (K - 1) // 2 if delay is None else int(delay)
    if K < 1 or not 0 <= D <= K - 1:
        raise ValueError(f"equaliser: {K} taps with a delay of {D} (K >= 1, 0 <= delay <= K - 1)")
    return K - 1 - D, D


class FirPlanner(LevelPlanner):
    """Plans the zvx_fir_ex windows of one stream, with stream.ReachPlanner's protocol: ``push(n_new, last)`` -> ``(in_origin, out_begin,
    out_count, keep_from)``.  A non-last push emits up to received - RR, the last one everything; the history before next_out - RL is
    dropped, so an equalised stream runs RR = delay samples behind its input.  window_fn is Context.fir_window on one row."""

    def __init__(self, ntaps, delay=None):
        super().__init__(*reach(ntaps, delay))


stream_fir = stream_windows                   # stream_fir(chunks, FirPlanner(K, D), window_fn)


def _pair(v, what, n=2):
    try:
        t = tuple(float(x) for x in v)
    except TypeError:
        raise ValueError(f"equaliser: {what} must be a sequence of {n} numbers, not {v!r}") from None
    if len(t) != n or not all(np.isfinite(t)):
        raise ValueError(f"equaliser: {what} must be {n} finite numbers, not {v!r}")
    return t


def _slope(v, what):
    """hz or (hz, order) -> (hz, order)"""
    if isinstance(v, (int, float, np.integer, np.floating)):
        v = (v, 4)
    hz, order = _pair(v, what)
    if order < 1 or order != int(order) or order > 16:
        raise ValueError(f"equaliser: {what}: order {order} must be an integer in 1 .. 16")
    return hz, float(int(order))


def _spec(rate, bands, low_shelf, high_shelf, highpass_hz, lowpass_hz):
    """the design keywords checked and as one hashable tuple"""
    nyq = rate / 2.0

    def inside(f, what):
        if not 0.0 < f < nyq:
            raise ValueError(f"equaliser: {what}: {f} Hz lies outside (0, {nyq}) at {rate} Hz")
        return f
    bs = []
    for b in bands or ():
        f, g, w = _pair(b, "a band (f_hz, gain_db, width_octaves)", 3)
        if not w > 0.0:
            raise ValueError(f"equaliser: a band's width of {w} octaves must be positive")
        bs.append((inside(f, "a band"), g, w))
    lo = hi = hp = lp = None
    if low_shelf is not None:
        lo = _pair(low_shelf, "low_shelf (f_hz, gain_db)")
        inside(lo[0], "low_shelf")
    if high_shelf is not None:
        hi = _pair(high_shelf, "high_shelf (f_hz, gain_db)")
        inside(hi[0], "high_shelf")
    if highpass_hz is not None:
        hp = _slope(highpass_hz, "highpass_hz")
        inside(hp[0], "highpass_hz")
    if lowpass_hz is not None:
        lp = _slope(lowpass_hz, "lowpass_hz")
        inside(lp[0], "lowpass_hz")
    if hp is not None and lp is not None and not hp[0] < lp[0]:
        raise ValueError(f"equaliser: highpass_hz {hp[0]} must lie below lowpass_hz {lp[0]}")
    return (tuple(bs), lo, hi, hp, lp)


def target_db(freqs, spec):
    """the target magnitude in dB at `freqs` (Hz, >= 0), float64"""
    f = np.asarray(freqs, np.float64)
    bands, lo, hi, hp, lp = spec
    db = np.zeros_like(f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for f0, g, w in bands:
            sigma = w / (2.0 * np.sqrt(2.0 * np.log(2.0)))
            d = np.where(f > 0.0, np.log2(np.where(f > 0.0, f, 1.0) / f0), -np.inf)
            db = db + g * np.exp(-0.5 * (d / sigma) ** 2)
        if lo is not None:
            db = db + lo[1] / (1.0 + (f / lo[0]) ** 2)
        if hi is not None:
            r2 = (f / hi[0]) ** 2
            db = db + hi[1] * r2 / (1.0 + r2)
        if hp is not None:
            s = np.where(f > 0.0, -10.0 * np.log10(1.0 + (hp[0] / np.where(f > 0.0, f, 1.0)) ** (2.0 * hp[1])), -np.inf)
            db = db + np.maximum(s, FLOOR_DB)
        if lp is not None:
            db = db + np.maximum(-10.0 * np.log10(1.0 + (f / lp[0]) ** (2.0 * lp[1])), FLOOR_DB)
    return np.maximum(db, FLOOR_DB)


class Equaliser:
    """taps float32 [K], delay, rate and the spec they were designed from (None: taps of the caller's own)"""
    __slots__ = ("taps", "delay", "rate", "spec")

    def __init__(self, taps, delay, rate, spec=None):
        taps = np.ascontiguousarray(taps, np.float32)
        check_taps(taps, delay)
        taps.setflags(write=False)
        self.taps, self.delay, self.rate, self.spec = taps, int(delay), int(rate), spec

    def response_db(self, freqs):
        """the realised magnitude response of the float32 taps at `freqs` (Hz) in dB, evaluated in double (-inf where it is zero)"""
        f = np.asarray(freqs, np.float64).reshape(-1)
        K = len(self.taps)
        h = self.taps.astype(np.float64)
        out = np.empty(len(f))
        linear_phase = K % 2 == 1 and self.delay == (K - 1) // 2 and np.array_equal(self.taps, self.taps[::-1])
        for i in range(0, len(f), 256):                      # (bounded memory: 256 x K phases at a time)
            w = 2.0 * np.pi * f[i:i + 256] / float(self.rate)
            if linear_phase:                                 # the zero-phase sum h[c] + 2 sum_m h[c + m] cos(w m): a unit impulse is exactly 1
                c = self.delay
                out[i:i + 256] = np.abs(h[c] + 2.0 * (np.cos(np.outer(w, np.arange(1, c + 1, dtype=np.float64))) @ h[c + 1:]))
            else:
                ph = -np.outer(w, np.arange(K, dtype=np.float64))
                out[i:i + 256] = np.abs((np.cos(ph) + 1j * np.sin(ph)) @ h)
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(out)

    def deviation_db(self, lo_hz=0.0, points=2048):
        """the largest |realised - target| in dB over `points` frequencies in [lo_hz, rate / 2] where the target is >= -20 dB"""
        if self.spec is None:
            raise ValueError("equaliser: taps of the caller's own have no target")
        f = np.linspace(float(lo_hz), self.rate / 2.0, int(points))
        t = target_db(f, self.spec)
        m = t >= -20.0
        if not m.any():
            return 0.0
        return float(np.max(np.abs(self.response_db(f[m]) - t[m])))

    def params(self):
        """the Context.fir / fir_device keywords"""
        return dict(taps=self.taps, delay=self.delay)


def check_taps(taps, delay):
    """what zvx_fir checks of its filter, without a device"""
    taps = np.asarray(taps)
    if taps.ndim != 1 or not 1 <= taps.shape[0] <= MAX_TAPS:
        raise ValueError(f"equaliser: taps must be a 1-D array of 1 .. {MAX_TAPS} values, not of shape {taps.shape}")
    if not np.all(np.isfinite(taps)):
        raise ValueError("equaliser: a tap is not finite")
    if int(delay) != delay or not 0 <= int(delay) <= taps.shape[0] - 1:
        raise ValueError(f"equaliser: delay {delay} outside [0, {taps.shape[0] - 1}]")


def _bessel_i0(x):
    x = np.asarray(x, np.float64)
    s, t = np.ones_like(x), np.ones_like(x)
    for k in range(1, 64):
        t = t * (x / (2.0 * k)) ** 2
        s = s + t
    return s


def design(rate, taps=DEFAULT_TAPS, bands=(), low_shelf=None, high_shelf=None, highpass_hz=None, lowpass_hz=None):
    """-> Equaliser(taps float32 [K], delay (K - 1) / 2, rate, spec); K = `taps` must be odd (a linear-phase filter with a whole-sample
    delay) and at most MAX_TAPS.  The method and its limits: the module docstring."""
    rate, K = int(rate), int(taps)
    if not 4000 <= rate <= 192000:
        raise ValueError(f"equaliser: rate {rate} outside [4000, 192000]")
    if K != taps or K < 1 or K > MAX_TAPS or K % 2 == 0:
        raise ValueError(f"equaliser: {taps} taps: an odd number in 1 .. {MAX_TAPS - 1} is needed")
    spec = _spec(rate, bands, low_shelf, high_shelf, highpass_hz, lowpass_hz)
    c = (K - 1) // 2
    f = np.arange(GRID // 2 + 1, dtype=np.float64) * (rate / float(GRID))
    db = target_db(f, spec)
    h = np.zeros(K, np.float64)
    if not db.any():                                         # 0 dB everywhere: the exact unit impulse
        h[c] = 1.0
    else:
        half = np.fft.irfft(10.0 ** (db / 20.0), GRID)[:c + 1]
        m = np.arange(c + 1, dtype=np.float64)
        win = _bessel_i0(KAISER_BETA * np.sqrt(np.maximum(0.0, 1.0 - (m / (c + 1.0)) ** 2))) / _bessel_i0(KAISER_BETA)
        half = half * win
        h[c:] = half
        h[:c] = half[:0:-1]                                  # the mirror: symmetric bit for bit
    return Equaliser(h.astype(np.float32), c, rate, spec)


_cache = {}


def _freeze(v):
    if isinstance(v, dict):
        return tuple(sorted((k, _freeze(x)) for k, x in v.items()))
    if isinstance(v, (list, tuple, np.ndarray)):
        return tuple(_freeze(x) for x in v)
    return v


def params(eq, rate):
    """The ``eq`` keyword of ZeroVoxTTS.tts / tts_long as Context.fir_device keywords (taps, delay), or None: eq is None, a preset name
    (PRESETS), a dict of ``design`` keywords, an Equaliser designed for `rate`, or (taps, delay) of the caller's own.  Checked without a
    device (ValueError); designs are cached per (spec, rate)."""
    if eq is None:
        return None
    rate = int(rate)
    if isinstance(eq, Equaliser):
        if eq.rate != rate:
            raise ValueError(f"equaliser: designed for {eq.rate} Hz, the model runs at {rate} Hz")
        return eq.params()
    if isinstance(eq, str):
        if eq not in PRESETS:
            raise ValueError(f"equaliser: {eq!r} is none of the presets {sorted(PRESETS)}")
        kw = PRESETS[eq]
    elif isinstance(eq, dict):
        kw = eq
    elif isinstance(eq, (tuple, list)) and len(eq) == 2:
        taps, delay = eq
        try:
            return Equaliser(np.asarray(taps, np.float64), delay, rate).params()
        except TypeError:
            raise ValueError(f"equaliser: (taps, delay) needs an array and an integer, not {eq!r}") from None
    else:
        raise ValueError(f"equaliser: eq must be None, a preset name, a dict of design keywords, an Equaliser or (taps, delay), not {type(eq).__name__}")
    try:
        key = (_freeze(kw), rate)
        hash(key)
    except TypeError:
        raise ValueError(f"equaliser: design keywords {kw!r} are not plain numbers and sequences") from None
    if key not in _cache:
        try:
            _cache[key] = design(rate, **kw)
        except TypeError as e:
            raise ValueError(f"equaliser: {e}") from None
    return _cache[key].params()
