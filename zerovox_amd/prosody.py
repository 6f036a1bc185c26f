"""Prosody control (include/zvx.h, zvx_prosody): speaking rate, pitch and energy of a batch, as the C struct takes them.

``Prosody.create(B, Tmax, speed=..., pitch_shift=..., ...)`` validates and expands the controls to the call's [B] / [B, Tmax] layout
and returns None when every control is neutral (the library then runs its uncontrolled path).  ``Prosody(B, Tmax, ...)`` keeps
whatever it is given, a neutral block included.

Accepted forms: shifts and ranges are scalars or [B]; targets (NaN = the prediction) are scalars, [B] or [B, T <= Tmax]; ``speed``
(speaking-rate factor, q = rint(65536 / speed)) and ``dur_scale_q16`` are scalars, [B] or [B, T <= Tmax].  Every value is checked
here, before any library call, with the limits the library enforces: ranges in [0, 4], targets NaN or in [0, 1], speed in
[1/16, 16] (q in [4096, 1048576]).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

Q_ONE = 65536
Q_MIN, Q_MAX = 4096, 1048576


class ProsodyStruct(C.Structure):
    _fields_ = [("pitch_shift", C.c_void_p), ("pitch_range", C.c_void_p), ("energy_shift", C.c_void_p), ("energy_range", C.c_void_p),
                ("pitch_target", C.c_void_p), ("energy_target", C.c_void_p), ("dur_scale_q16", C.c_void_p)]


def _per_utt(name, v, B, lo=None, hi=None):
    if v is None:
        return None
    a = np.asarray(v, np.float64)
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,):
        raise ValueError(f"prosody {name}: expected a scalar or shape ({B},), got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"prosody {name}: values must be finite")
    if lo is not None and (a.min() < lo or a.max() > hi):
        raise ValueError(f"prosody {name}: values must lie in [{lo}, {hi}]")
    return np.ascontiguousarray(a, np.float32)


def _per_phone(name, v, B, Tmax, fill, dtype):
    """scalar | [B] | [B, T <= Tmax] -> [B, Tmax] (columns past T take `fill`)"""
    if v is None:
        return None
    a = np.asarray(v)
    out = np.full((B, Tmax), fill, dtype)
    if a.ndim == 0:
        out[:] = a
    elif a.shape == (B,):
        out[:] = a[:, None]
    elif a.ndim == 2 and a.shape[0] == B and a.shape[1] <= Tmax:
        out[:, :a.shape[1]] = a
    else:
        raise ValueError(f"prosody {name}: expected a scalar, shape ({B},) or ({B}, T <= {Tmax}), got {a.shape}")
    return out


class Prosody:
    """One call's control block, expanded to [B] / [B, Tmax].  ``struct()`` is the zvx_prosody the _ex entry points take; the arrays
    it points to live as long as this object."""

    def __init__(self, B, Tmax, pitch_shift=None, pitch_range=None, energy_shift=None, energy_range=None,
                 pitch_target=None, energy_target=None, dur_scale_q16=None, speed=None):
        self.B, self.Tmax = int(B), int(Tmax)
        self.pitch_shift = _per_utt("pitch_shift", pitch_shift, B)
        self.pitch_range = _per_utt("pitch_range", pitch_range, B, 0.0, 4.0)
        self.energy_shift = _per_utt("energy_shift", energy_shift, B)
        self.energy_range = _per_utt("energy_range", energy_range, B, 0.0, 4.0)
        self.pitch_target = self._target("pitch_target", pitch_target)
        self.energy_target = self._target("energy_target", energy_target)
        if speed is not None and dur_scale_q16 is not None:
            raise ValueError("prosody: give speed or dur_scale_q16, not both")
        if speed is not None:
            s = _per_phone("speed", np.asarray(speed, np.float64), B, Tmax, 1.0, np.float64)
            if not np.all(np.isfinite(s)) or s.min() < 1 / 16 or s.max() > 16:
                raise ValueError("prosody speed: values must lie in [1/16, 16]")
            dur_scale_q16 = np.rint(Q_ONE / s).astype(np.int64)
        q = _per_phone("dur_scale_q16", dur_scale_q16, B, Tmax, Q_ONE, np.int64)
        if q is not None and (q.min() < Q_MIN or q.max() > Q_MAX):
            raise ValueError(f"prosody dur_scale_q16: values must lie in [{Q_MIN}, {Q_MAX}] (speed 1/16 ... 16)")
        self.dur_scale_q16 = None if q is None else np.ascontiguousarray(q, np.int32)

    def _target(self, name, v):
        a = _per_phone(name, None if v is None else np.asarray(v, np.float64), self.B, self.Tmax, np.nan, np.float64)
        if a is None:
            return None
        ok = np.isnan(a) | ((a >= 0) & (a <= 1))
        if not ok.all():
            raise ValueError(f"prosody {name}: values must be NaN or lie in [0, 1]")
        return np.ascontiguousarray(a, np.float32)

    @classmethod
    def create(cls, B, Tmax, speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0,
               pitch_target=None, energy_target=None, dur_scale_q16=None):
        """Validated, expanded block -- or None when every control is neutral."""
        p = cls(B, Tmax, pitch_shift, pitch_range, energy_shift, energy_range, pitch_target, energy_target,
                dur_scale_q16, None if dur_scale_q16 is not None else speed)
        if p.pitch_shift is not None and not p.pitch_shift.any():
            p.pitch_shift = None
        if p.energy_shift is not None and not p.energy_shift.any():
            p.energy_shift = None
        if p.pitch_range is not None and np.all(p.pitch_range == 1):
            p.pitch_range = None
        if p.energy_range is not None and np.all(p.energy_range == 1):
            p.energy_range = None
        if p.pitch_target is not None and np.isnan(p.pitch_target).all():
            p.pitch_target = None
        if p.energy_target is not None and np.isnan(p.energy_target).all():
            p.energy_target = None
        if p.dur_scale_q16 is not None and np.all(p.dur_scale_q16 == Q_ONE):
            p.dur_scale_q16 = None
        return None if p.is_neutral() else p

    def is_neutral(self):
        return all(getattr(self, f) is None for f, _ in ProsodyStruct._fields_)

    def struct(self):
        def ptr(a):
            return None if a is None else a.ctypes.data
        return ProsodyStruct(*(ptr(getattr(self, f)) for f, _ in ProsodyStruct._fields_))

    def check_shape(self, B, Tmax):
        if (self.B, self.Tmax) != (int(B), int(Tmax)):
            raise ValueError(f"prosody block is for [{self.B}, {self.Tmax}], the call is [{B}, {Tmax}]")

    def scaled_lengths(self, duration, T):
        """mel lengths of forced durations [B, Tmax] under this block's duration factors (the library's Q16 rule)."""
        return scaled_lengths(duration, T, self.dur_scale_q16)


def resolve(prosody, B, Tmax):
    """None | Prosody | dict of Prosody.create keywords -> Prosody or None, for a call of shape [B, Tmax]."""
    if prosody is None:
        return None
    if isinstance(prosody, dict):
        return Prosody.create(B, Tmax, **prosody)
    if isinstance(prosody, Prosody):
        prosody.check_shape(B, Tmax)
        return prosody
    raise TypeError(f"prosody: expected None, a dict or a Prosody, got {type(prosody).__name__}")


def q16_cumulative(d, q):
    """The library's duration rule for one utterance: d [T] integer durations, q [T] Q16 factors ->
    (d' [T], C [T], mel_len) with P_t = sum_{u<=t} d_u q_u, C_t = (P_t + 2^15) >> 16, d'_t = C_t - C_{t-1}."""
    d = np.minimum(np.maximum(np.asarray(d, np.int64), 0), 65536)
    P = np.cumsum(d * np.asarray(q, np.int64))
    Cs = (P + 32768) >> 16
    dp = np.diff(np.concatenate([[0], Cs]))
    return dp, Cs, int(Cs[-1]) if len(Cs) else 0


def scaled_lengths(duration, T, q):
    duration = np.asarray(duration)
    out = np.zeros(len(T), np.int64)
    for b, n in enumerate(np.asarray(T)):
        d = duration[b, :n]
        out[b] = q16_cumulative(d, q[b, :n])[2] if q is not None else int(np.minimum(np.maximum(d.astype(np.int64), 0), 65536).sum())
    return out
