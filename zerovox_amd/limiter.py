"""Streaming side of the look-ahead limiter (include/zvx.h: zvx_limit_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The limiter has finite support and no recurrence: output ``i`` depends on the input
samples within ``R = 2 W + H`` of it -- the envelope reads ``H = 11`` samples to either side where it is oversampled (none at
``oversample`` 1), hold and smoothing reach ``W`` each -- and on the signal's true ends where those lie within ``R``.  The two rules
of a stream with that reach, and the loop that drives it, are zerovox_amd.stream's; a limited stream runs ``R`` samples behind its input.
"""
from __future__ import annotations

import numpy as np

from .stream import ReachPlanner, stream_windows

ENV_REACH = 11                                # e[j] reads x[j - 11 .. j + 11] (csrc/zvx_kernels.h, LIMIT_ENV_REACH)


def window_samples(rate, window_ms):
    """W = max(1, rint(rate * window_ms / 1000)) in double, with window_ms the f32 the parameter struct carries (include/zvx.h)"""
    return max(1, int(np.rint(float(rate) * float(np.float32(window_ms)) / 1000.0)))


def reach(W, oversample):
    """R = 2 W + H: how far to either side an output sample of the limiter depends on its input"""
    return 2 * int(W) + (ENV_REACH if int(oversample) > 1 else 0)


class LimitPlanner(ReachPlanner):
    """Plans the zvx_limit_ex windows of one stream: a ReachPlanner of reach(W, oversample); window_fn is Context.limit_window on one row."""

    def __init__(self, W, oversample):
        super().__init__(reach(W, oversample))
        self.W, self.oversample = int(W), int(oversample)


stream_limit = stream_windows                 # stream_limit(chunks, LimitPlanner(W, oversample), window_fn)
