"""Streaming side of the vocoder-bias denoiser (include/zvx.h: zvx_denoise_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The denoiser has finite support and no recurrence: output ``i`` is the overlap-add of the
STFT frames that cover it, and a frame that covers ``i`` begins after ``i - n_fft`` and ends before ``i + n_fft``.  So ``i`` depends on
the input samples within ``R = n_fft - 1`` of it, and on the signal's true ends (the reflect padding) where those lie within ``R``:

* with ``received`` input samples in hand, output ``i`` is final once ``i + R <= received - 1`` (everything on the last push);
* the next output ``next_out`` needs no sample before ``next_out - R``: the history before it can go.

These are the two rules of the limiter's stream with another reach, and the planner is the limiter's.  A stream denoised in these windows
is bit-identical to one whole-signal call: the frame grid is the signal's wherever the window was cut, a frame's transform depends on its
own samples only, and the overlap-add runs over the same frames in the same order.  The price is delay -- a denoised stream runs ``R``
samples behind its input (1023 samples, 46 ms, at n_fft 1024 and 22.05 kHz) -- and work: every window transforms again the up to
``2 n_fft / hop`` frames that reach into its history.
"""
from __future__ import annotations

from .limiter import LimitPlanner, stream_limit


def reach(n_fft):
    """R = n_fft - 1: how far to either side an output sample of the denoiser depends on its input"""
    return int(n_fft) - 1


class DenoisePlanner(LimitPlanner):
    """Plans the zvx_denoise_ex windows of one stream.  ``push(n_new, last)`` takes the count of newly received input samples and
    returns ``(in_origin, out_begin, out_count, keep_from)``: call the denoiser on the retained samples ``[in_origin, received)`` for
    outputs ``[out_begin, out_begin + out_count)`` (nothing to do when ``out_count`` is 0) with that ``last``, then drop the history
    before ``keep_from``.  ``push(0, True)`` ends a stream whose end was not known earlier."""

    def __init__(self, n_fft):
        self.n_fft, self.R = int(n_fft), reach(n_fft)
        self.received = 0                     # input samples received so far
        self.next_out = 0                     # the next output sample to emit
        self.origin = 0                       # index of the first retained input sample


def stream_denoise(chunks, planner, window_fn):
    """chunks: an iterable of 1-D float32 pieces of one signal -> yields its denoised pieces, which concatenate to the whole-signal
    denoiser bit for bit.  ``window_fn(samples, in_origin, out_begin, out_count, last)`` is the denoiser over a window
    (Context.denoise_window on one row); a piece is yielded as soon as its samples are final, i.e. ``planner.R`` samples behind the
    input, and the rest when ``chunks`` ends -- no chunk is held back to learn whether it was the last."""
    return stream_limit(chunks, planner, window_fn)
