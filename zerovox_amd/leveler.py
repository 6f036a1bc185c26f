"""Streaming side of the leveler (include/zvx.h: zvx_level_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The leveler is a short-term AGC, not R128 normalisation: the gain of a sample is
interpolated between two unit nodes, each the gated loudness of ``S`` units of 100 ms ending ``a`` units ahead.  It has finite support and
no state that crosses a unit, but its reach is not the same on both sides: ``RL = (S + 3 - a) h - 1`` samples back (the oldest unit of the
window and its two units of filter warm-up) and ``RR = (a + 1) h - 1`` samples ahead.  A levelled stream runs ``RR`` samples behind its
input and keeps ``RL`` samples of history; the loop that drives it is zerovox_amd.stream's.
"""
from __future__ import annotations

import numpy as np

from .stream import stream_windows

MAX_UNITS = 600                               # the longest window, in units (csrc/zvx_kernels.h, LEVEL_MAX_S)


def units(rate):
    """h = (rate + 5) / 10: the samples of a 100 ms unit (integer division, as zvx_loudness)"""
    return (int(rate) + 5) // 10


def window_units(window_ms):
    """S = max(1, rint(window_ms / 100)) in double, with window_ms the f32 the parameter struct carries (include/zvx.h)"""
    return max(1, int(np.rint(float(np.float32(window_ms)) / 100.0)))


def lookahead_units(lookahead_ms):
    """a = rint(lookahead_ms / 100), likewise"""
    return int(np.rint(float(np.float32(lookahead_ms)) / 100.0))


def reach(rate, window_ms, lookahead_ms):
    """(RL, RR): how far back and how far ahead an output sample of the leveler depends on its input"""
    h, S, a = units(rate), window_units(window_ms), lookahead_units(lookahead_ms)
    if not 0 <= a <= S:
        raise ValueError(f"leveler: a look-ahead of {a} units needs 0 <= a <= S = {S}")
    return (S + 3 - a) * h - 1, (a + 1) * h - 1


class LevelPlanner:
    """Plans the zvx_level_ex windows of one stream, with stream.ReachPlanner's protocol for a reach of RL to the left and RR to the right:
    ``push(n_new, last)`` -> ``(in_origin, out_begin, out_count, keep_from)``.  A non-last push emits up to received - RR, the last one
    everything; the history before next_out - RL is dropped.  window_fn is Context.level_window on one row."""

    def __init__(self, RL, RR):
        self.RL, self.RR = int(RL), int(RR)
        self.received = 0                     # input samples received so far
        self.next_out = 0                     # the next output sample to emit
        self.origin = 0                       # index of the first retained input sample

    def push(self, n_new, last=False):
        self.received += int(n_new)
        end = self.received if last else max(self.next_out, self.received - self.RR)
        in_origin, out_begin = self.origin, self.next_out
        self.next_out = end
        self.origin = max(self.origin, min(end - self.RL, self.received))
        return in_origin, out_begin, end - out_begin, self.origin


stream_level = stream_windows                 # stream_level(chunks, LevelPlanner(*reach(rate, window_ms, lookahead_ms)), window_fn)
