"""Streaming side of the look-ahead limiter (include/zvx.h: zvx_limit_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The limiter has finite support and no recurrence: output ``i`` depends on the input
samples within ``R = 2 W + H`` of it -- the envelope reads ``H = 11`` samples to either side where it is oversampled (none at
``oversample`` 1), hold and smoothing reach ``W`` each -- and on the signal's true ends where those lie within ``R``:

* with ``received`` input samples in hand, output ``i`` is final once ``i + R <= received - 1`` (everything on the last push);
* the next output ``next_out`` needs no sample before ``next_out - R``: the history before it can go.

A stream limited in these windows is bit-identical to one whole-signal call, because every sum of a sample runs over the same
values in the same order wherever the window was cut.  The price is delay: a limited stream runs ``R`` samples behind its input.
"""
from __future__ import annotations

import numpy as np

ENV_REACH = 11                                # e[j] reads x[j - 11 .. j + 11] (csrc/zvx_kernels.h, LIMIT_ENV_REACH)


def window_samples(rate, window_ms):
    """W = max(1, rint(rate * window_ms / 1000)) in double, with window_ms the f32 the parameter struct carries (include/zvx.h)"""
    return max(1, int(np.rint(float(rate) * float(np.float32(window_ms)) / 1000.0)))


def reach(W, oversample):
    """R = 2 W + H: how far to either side an output sample of the limiter depends on its input"""
    return 2 * int(W) + (ENV_REACH if int(oversample) > 1 else 0)


class LimitPlanner:
    """Plans the zvx_limit_ex windows of one stream.  ``push(n_new, last)`` takes the count of newly received input samples and
    returns ``(in_origin, out_begin, out_count, keep_from)``: call the limiter on the retained samples ``[in_origin, received)``
    for outputs ``[out_begin, out_begin + out_count)`` (nothing to do when ``out_count`` is 0) with that ``last``, then drop the
    history before ``keep_from``.  A push may bring no samples: ``push(0, True)`` ends a stream whose end was not known earlier."""

    def __init__(self, W, oversample):
        self.W, self.oversample, self.R = int(W), int(oversample), reach(W, oversample)
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


def stream_limit(chunks, planner, window_fn):
    """chunks: an iterable of 1-D float32 pieces of one signal -> yields its limited pieces, which concatenate to the whole-signal
    limiter bit for bit.  ``window_fn(samples, in_origin, out_begin, out_count, last)`` is the limiter over a window
    (Context.limit_window on one row); a piece is yielded as soon as its samples are final, i.e. ``planner.R`` samples behind the
    input, and the rest when ``chunks`` ends -- no chunk is held back to learn whether it was the last."""
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
