"""What was delivered: the programme loudness figures a delivery specification asks for together (EBU R128 / Tech 3342 and the platform
variants) -- integrated loudness, loudness range, maximum momentary and short-term loudness, sample peak and true peak.  The figures are
measured on the device (include/zvx.h: zvx_loudness_stats, zvx_true_peak; ZeroVoxTTS.loudness_report); this module only holds and
judges them.  Pure Python: importable without the library."""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass


def _db(linear):
    """20 log10 of a linear peak (-inf for silence)"""
    return 20.0 * math.log10(linear) if linear > 0.0 else -math.inf


@dataclass(frozen=True)
class LoudnessReport:
    integrated: float        # LUFS (BS.1770-4, both gates); -inf where nothing passes the absolute gate
    lra: float               # loudness range in LU (EBU Tech 3342): lra_high - lra_low
    lra_low: float           # LUFS: the 10th percentile of the gated short-term windows (-inf without one)
    lra_high: float          # LUFS: their 95th percentile
    max_momentary: float     # LUFS: the loudest 400 ms block (-inf where the waveform is shorter than one)
    max_short_term: float    # LUFS: the loudest 3 s window (-inf where the waveform is shorter than one)
    sample_peak_db: float    # dBFS
    true_peak_db: float      # dBTP (4x oversampled)
    short_gated: int         # the number of short-term windows the loudness range was taken over

    @classmethod
    def from_stats(cls, stats, true_peak, row=0):
        """row `row` of Context.loudness_stats' dict and the linear true peak of the same row (Context.true_peak)"""
        return cls(integrated=float(stats["integrated"][row]), lra=float(stats["lra"][row]), lra_low=float(stats["lra_low"][row]),
                   lra_high=float(stats["lra_high"][row]), max_momentary=float(stats["max_momentary"][row]),
                   max_short_term=float(stats["max_short_term"][row]), sample_peak_db=_db(float(stats["peak"][row])),
                   true_peak_db=_db(float(true_peak)), short_gated=int(stats["short_gated"][row]))

    def meets(self, target, tolerance=0.5, max_true_peak_db=-1.0, max_lra=None):
        """does the programme meet a delivery specification: integrated loudness within `tolerance` LU of `target` LUFS (R128: -23 +- 0.5),
        true peak at most max_true_peak_db dBTP (None: not looked at), loudness range at most max_lra LU (None: not looked at).  A programme
        without a measurable loudness meets nothing."""
        if not math.isfinite(self.integrated) or abs(self.integrated - float(target)) > float(tolerance):
            return False
        if max_true_peak_db is not None and self.true_peak_db > float(max_true_peak_db):
            return False
        return max_lra is None or self.lra <= float(max_lra)

    def as_dict(self):
        return asdict(self)

    def __str__(self):
        return (f"integrated {self.integrated:.2f} LUFS, LRA {self.lra:.2f} LU ({self.lra_low:.2f} .. {self.lra_high:.2f} LUFS over "
                f"{self.short_gated} windows), max momentary {self.max_momentary:.2f} LUFS, max short-term {self.max_short_term:.2f} LUFS, "
                f"sample peak {self.sample_peak_db:.2f} dBFS, true peak {self.true_peak_db:.2f} dBTP")
