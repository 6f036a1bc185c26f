"""Alignment of two utterances: what Context.align measured, and the rhythm arithmetic that turns it into forced durations.

The alignment is a DTW path between DCT cepstra of the model's own log-mel (include/zvx.h, zvx_align_wav).  Its mcd_db is the distortion
between those cepstra (c0 left out) averaged over the path's cells: figures from SPTK / WORLD mel-cepstral analysis are not comparable
with it, and no perceptual claim is made.  Pure NumPy; nothing here touches the device."""
from dataclasses import dataclass

import numpy as np


@dataclass
class Alignment:
    """One pair of utterances, a against b, in mel frames."""
    cost: float            # the accumulated distance along the path
    mcd_db: float          # (10 / ln 10) sqrt(2) cost / len(path)
    frames_a: int
    frames_b: int
    path: np.ndarray       # [L][2] int32: cells (i, j) from (0, 0) to (frames_a - 1, frames_b - 1)
    a2b: np.ndarray        # [frames_a][2] int32: the first and last frame of b matched to each frame of a

    def meets(self, max_mcd_db):
        """mcd_db <= max_mcd_db, the caller's number: there is no built-in threshold."""
        return bool(self.mcd_db <= float(max_mcd_db))

    @classmethod
    def from_result(cls, res, b=0):
        """row b of what Context.align returns"""
        return cls(float(res["cost"][b]), float(res["mcd_db"][b]), int(res["frames_a"][b]), int(res["frames_b"][b]),
                   np.array(res["path"][b], np.int32), np.array(res["a2b"][b], np.int32))


def durations_from(alignment, durations, min_frames=1):
    """The durations of a first pass (per phoneme, in mel frames, their sum = alignment.frames_a) carried over to the timing of b:
    with c_p the cumulative durations, the new boundaries are e_0 = 0, e_p = a2b[c_p][0] for 0 < p < P and e_P = frames_b; a forward pass
    gives every phoneme that had a duration >= 1 at least min_frames (e_{p+1} = max(e_{p+1}, e_p + min_frames)), a backward pass restores
    e_P = frames_b under the same constraint.  Phonemes of duration 0 stay 0; the total is exactly frames_b.  ValueError where frames_b is
    too small for that, or where the durations do not add up to frames_a."""
    d = np.asarray(durations, np.int64).reshape(-1)
    fa, fb, m = int(alignment.frames_a), int(alignment.frames_b), int(min_frames)
    if np.any(d < 0) or int(d.sum()) != fa:
        raise ValueError(f"durations sum to {int(d.sum())}, the alignment has {fa} frames of a")
    if m < 0:
        raise ValueError(f"min_frames {m} is negative")
    P = len(d)
    a2b = np.asarray(alignment.a2b, np.int64).reshape(-1, 2)
    if a2b.shape[0] != fa:
        raise ValueError(f"a2b has {a2b.shape[0]} rows, the alignment {fa} frames of a")
    need = np.where(d >= 1, m, 0)
    if int(need.sum()) > fb:
        raise ValueError(f"{int((d >= 1).sum())} phonemes of at least {m} frames do not fit the {fb} frames of b")
    c = np.concatenate([[0], np.cumsum(d)])
    e = np.zeros(P + 1, np.int64)
    for p in range(1, P):
        e[p] = a2b[c[p], 0] if c[p] < fa else fb
    e[P] = fb
    for p in range(P):                                   # forward: at least `need`, and no phoneme of duration 0 grows
        e[p + 1] = e[p] if d[p] == 0 else max(e[p + 1], e[p] + need[p])
    e[P] = fb
    for p in range(P - 1, -1, -1):                       # backward: e_P = frames_b again
        e[p] = e[p + 1] if d[p] == 0 else min(e[p], e[p + 1] - need[p])
    out = np.diff(e)
    assert e[0] == 0 and int(out.sum()) == fb and np.all(out >= need) and np.all(out[d == 0] == 0)
    return out.astype(np.int32)
