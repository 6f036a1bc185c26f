"""Streaming side of the sample-rate conversion (include/zvx.h: zvx_resample_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The filter reaches ``half`` taps of the ``L``-times upsampled signal to either side
of an output, so output ``n`` needs the input samples ``k`` with ``|n M - k L| <= half``:

* with ``received`` input samples in hand, output ``n`` is final once ``n M + half <= (received - 1) L`` (everything on the last chunk);
* the next output ``n_next`` needs no sample before ``ceil((n_next M - half) / L)``: the history before it can go.

A stream converted in these windows is bit-identical to one whole-signal call, because the sum of an output runs over the same
samples in the same order wherever the window was cut.  The loop that drives the planner is zerovox_amd.stream's.
"""
from __future__ import annotations

from math import gcd

from .stream import stream_windows

ZEROS = 10                                    # half = ZEROS * max(L, M), as the library designs its filter


def rate_pair(rate_in, rate_out):
    """-> (L, M, half) of rate_in -> rate_out; equal rates are a copy: (1, 1, 0)."""
    g = gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    return L, M, (0 if L == M else ZEROS * max(L, M))


def _ceil_div(a, b):
    return -((-a) // b)


class StreamPlanner:
    """Plans the zvx_resample_ex windows of one stream.  ``push(n_new, last)`` takes the count of newly received input samples and
    returns ``(in_origin, out_begin, out_count, keep_from)``: call the resampler on the retained samples ``[in_origin, received)``
    for outputs ``[out_begin, out_begin + out_count)`` (nothing to do when ``out_count`` is 0), then drop the history before ``keep_from``."""

    def __init__(self, rate_in, rate_out):
        self.L, self.M, self.half = rate_pair(rate_in, rate_out)
        self.received = 0                     # input samples received so far
        self.n_next = 0                       # the next output sample to emit
        self.origin = 0                       # index of the first retained input sample

    def push(self, n_new, last=False):
        L, M, half = self.L, self.M, self.half
        self.received += int(n_new)
        if last:
            end = _ceil_div(self.received * L, M)
        else:
            top = (self.received - 1) * L - half
            end = top // M + 1 if top >= 0 else 0
        end = max(end, self.n_next)
        step = (self.origin, self.n_next, end - self.n_next, max(self.origin, _ceil_div(end * M - half, L)))
        self.n_next = end
        self.origin = min(step[3], self.received)
        return step[0], step[1], step[2], self.origin


def stream_resample(chunks, rate_in, rate_out, window_fn):
    """chunks: an iterable of 1-D float32 pieces of one signal at rate_in -> yields its pieces at rate_out, which concatenate to the
    whole-signal conversion bit for bit.  ``window_fn(samples, in_origin, out_begin, out_count)`` is the resampler over a window
    (Context.resample_window on one row); a piece is yielded as soon as its samples are final, and the outputs that wait for the
    signal's end come in a closing window when ``chunks`` ends (zerovox_amd.stream)."""
    return stream_windows(chunks, StreamPlanner(rate_in, rate_out), lambda x, o, b, n, last: window_fn(x, o, b, n))
