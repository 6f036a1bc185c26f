"""The streamed post-processing steps (limiter, denoiser, sample-rate conversion) share one way of cutting a stream into windows:
which outputs are final, what history to keep, and the loop that drives a planner over the chunks.

Pure Python, importable without the library.  Each step has finite support and no recurrence: output ``i`` depends on the input
samples within some reach of it, and on the signal's true ends where those lie within that reach.  For a fixed reach ``R``:

* finality: with ``received`` input samples in hand, output ``i`` is final once ``i + R <= received - 1`` (everything on the last push);
* history: the next output ``next_out`` needs no sample before ``next_out - R``: the history before it can go.

A stream processed in these windows is bit-identical to one whole-signal call, because every sum of a sample runs over the same
values in the same order wherever the window was cut.  The price is delay: the processed stream runs ``R`` samples behind its input.
limiter.py and denoiser.py say what their ``R`` is; resample.py states the same two rules for its rational reach and has a planner
of its own, driven by the same loop.
"""
from __future__ import annotations

import numpy as np


class ReachPlanner:
    """Plans the windows of one stream for a step of fixed reach ``R``.  ``push(n_new, last)`` takes the count of newly received
    input samples and returns ``(in_origin, out_begin, out_count, keep_from)``: call the step on the retained samples
    ``[in_origin, received)`` for outputs ``[out_begin, out_begin + out_count)`` (nothing to do when ``out_count`` is 0) with that
    ``last``, then drop the history before ``keep_from``.  A push may bring no samples: ``push(0, True)`` ends a stream whose end
    was not known earlier."""

    def __init__(self, R):
        self.R = int(R)
        self.received = 0                     # input samples received so far
        self.next_out = 0                     # the next output sample to emit
        self.origin = 0                       # index of the first retained input sample

    def push(self, n_new, last=False):
        self.received += int(n_new)
        end = self.received if last else max(self.next_out, self.received - self.R)
        in_origin, out_begin = self.origin, self.next_out
        self.next_out = end
        self.origin = max(self.origin, min(end - self.R, self.received))
        return in_origin, out_begin, end - out_begin, self.origin


def stream_windows(chunks, planner, window_fn):
    """chunks: an iterable of 1-D float32 pieces of one signal -> yields its processed pieces, which concatenate to the whole-signal
    call bit for bit.  ``window_fn(samples, in_origin, out_begin, out_count, last)`` is the step over a window (one row of a
    Context.*_window call); a piece is yielded as soon as the planner calls its samples final, and the rest when ``chunks`` ends
    -- no chunk is held back to learn whether it was the last."""
    hist = np.zeros(0, np.float32)

    def step(n_new, last):
        nonlocal hist
        in_origin, out_begin, out_count, keep_from = planner.push(n_new, last)
        piece = window_fn(hist, in_origin, out_begin, out_count, last) if out_count > 0 else None
        hist = hist[keep_from - in_origin:]
        return piece

    for cur in chunks:
        cur = np.asarray(cur, np.float32)
        hist = np.concatenate([hist, cur])
        piece = step(len(cur), False)
        if piece is not None:
            yield piece
    piece = step(0, True)
    if piece is not None:
        yield piece
