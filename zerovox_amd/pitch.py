"""What pitch was delivered: the F0 track of a waveform on a frame grid and its statistics.  The track is measured on the device
(include/zvx.h: zvx_pitch, YIN; Context.pitch, ZeroVoxTTS.pitch_report); this module holds the geometry of that definition, the report and
the reduction of a frame track to the per-phoneme pitch the model's pitch predictor was trained on.  Pure Python: importable without the
library."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np


def tau_min(rate, fmax):
    """the smallest lag searched: max(2, floor(rate / fmax)), formed in double as the C side does (fmax as the f32 it is passed as)"""
    return max(2, int(math.floor(float(rate) / float(np.float32(fmax)))))


def tau_max(rate, fmin):
    """the largest lag: ceil(rate / fmin)"""
    return int(math.ceil(float(rate) / float(np.float32(fmin))))


def frames(n, hop):
    """frames of a row of n samples: n // hop (frame f is centred on sample f * hop)"""
    return int(n) // int(hop)


def default_window(rate, fmin):
    """Context.pitch's default window: two periods of fmin"""
    return 2 * tau_max(rate, fmin)


def default_hop(rate, model_rate=None, model_hop=None):
    """Context.pitch's default hop: the model's where the rate is the model's (a frame is then a mel frame), otherwise 10 ms"""
    if model_rate is not None and model_hop and int(rate) == int(model_rate):
        return int(model_hop)
    return max(1, int(rate) // 100)


def cents(f, ref):
    """1200 log2(f / ref)"""
    return 1200.0 * math.log2(float(f) / float(ref))


@dataclass(frozen=True)
class PitchReport:
    median_hz: float          # nearest-rank median of the voiced frames' f0 (0 without one)
    low_hz: float             # their 5th percentile
    high_hz: float            # their 95th percentile
    mean_hz: float            # their mean
    range_semitones: float    # 12 log2(high / low); 0 without voiced frames
    voiced_fraction: float    # voiced / frames (0 without frames)
    frames: int
    f0: object = field(default=None, compare=False, repr=False)      # the track the figures were taken from (Hz, 0 = unvoiced), where kept
    aper: object = field(default=None, compare=False, repr=False)    # d' at each frame's pick

    @classmethod
    def from_stats(cls, stats, row=0):
        """row `row` of Context.pitch's dict (with its curves where it has them)"""
        lo, hi = float(stats["low"][row]), float(stats["high"][row])
        n, nv = int(stats["frames"][row]), int(stats["voiced"][row])
        return cls(median_hz=float(stats["median"][row]), low_hz=lo, high_hz=hi, mean_hz=float(stats["mean"][row]),
                   range_semitones=12.0 * math.log2(hi / lo) if nv > 0 and lo > 0.0 else 0.0,
                   voiced_fraction=nv / n if n > 0 else 0.0, frames=n,
                   f0=stats["f0"][row] if "f0" in stats else None, aper=stats["aper"][row] if "aper" in stats else None)

    def as_dict(self):
        """the figures (not the track)"""
        return {k: getattr(self, k) for k in ("median_hz", "low_hz", "high_hz", "mean_hz", "range_semitones", "voiced_fraction", "frames")}

    def __str__(self):
        return (f"median {self.median_hz:.1f} Hz, range {self.low_hz:.1f} .. {self.high_hz:.1f} Hz ({self.range_semitones:.2f} semitones), "
                f"mean {self.mean_hz:.1f} Hz, voiced {100.0 * self.voiced_fraction:.1f} % of {self.frames} frames")


PITCH_KEYWORDS = ("fmin", "fmax", "threshold", "gate_db", "window", "hop")


def check_keywords(kw):
    """the keywords of a pitch measurement (Context.pitch's: fmin, fmax, threshold, gate_db, window, hop) checked the way zvx_pitch checks
    its parameters -> the dict; ValueError names the keyword"""
    kw = dict(kw)
    unknown = sorted(set(kw) - set(PITCH_KEYWORDS))
    if unknown:
        raise ValueError(f"pitch_report: unknown keyword {unknown[0]!r} (one of {', '.join(PITCH_KEYWORDS)})")
    fmin, fmax = float(kw.get("fmin", 60.0)), float(kw.get("fmax", 500.0))
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0.0 < fmin < fmax):
        raise ValueError(f"pitch_report: fmin {fmin} / fmax {fmax} must be finite with 0 < fmin < fmax")
    thr, gate = float(kw.get("threshold", 0.15)), float(kw.get("gate_db", -60.0))
    if not (math.isfinite(thr) and 0.0 < thr <= 1.0):
        raise ValueError(f"pitch_report: threshold {thr} must lie in (0, 1]")
    if not (math.isfinite(gate) and gate <= 0.0):
        raise ValueError(f"pitch_report: gate_db {gate} must be finite and not positive")
    if kw.get("window") is not None and int(kw["window"]) < 2:
        raise ValueError(f"pitch_report: window {kw['window']} must be at least 2")
    if kw.get("hop") is not None and int(kw["hop"]) < 1:
        raise ValueError(f"pitch_report: hop {kw['hop']} must be at least 1")
    return kw


def fill_unvoiced(f0):
    """a frame track (Hz, 0 = unvoiced) -> float64 with every unvoiced frame filled by linear interpolation between its voiced neighbours,
    the first / last voiced value held in front of / behind them; all zeros where nothing is voiced"""
    f0 = np.asarray(f0, np.float64).reshape(-1)
    idx = np.flatnonzero(f0 > 0.0)
    if idx.size == 0:
        return np.zeros_like(f0)
    return np.interp(np.arange(f0.size), idx, f0[idx])       # (np.interp holds the end values outside [idx[0], idx[-1]])


def per_phoneme(f0, durations):
    """The per-phoneme pitch of a frame track: unvoiced frames filled (fill_unvoiced), then the mean over each phoneme's frames -- phoneme
    i owns the durations[i] frames behind those of its predecessors.  A phoneme of duration 0 takes the value at its first frame; frames
    past the end of the track read its last value; the result is all zeros where nothing is voiced (or the track is empty).
    -> float64 [len(durations)], in Hz."""
    d = np.asarray(durations, np.int64).reshape(-1)
    if (d < 0).any():
        raise ValueError("per_phoneme: a duration is negative")
    filled = fill_unvoiced(f0)
    out = np.zeros(d.size, np.float64)
    if filled.size == 0 or not filled.any():
        return out
    last = filled.size - 1
    pos = 0
    for i, n in enumerate(d):
        at = np.minimum(np.arange(pos, pos + max(int(n), 1)), last)
        out[i] = filled[at].mean()
        pos += int(n)
    return out
