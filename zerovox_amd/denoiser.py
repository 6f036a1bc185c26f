"""Streaming side of the vocoder-bias denoiser (include/zvx.h: zvx_denoise_ex): which outputs are final, what history to keep.

Pure Python, importable without the library.  The denoiser has finite support and no recurrence: output ``i`` is the overlap-add of the
STFT frames that cover it, and a frame that covers ``i`` begins after ``i - n_fft`` and ends before ``i + n_fft``.  So ``i`` depends on
the input samples within ``R = n_fft - 1`` of it, and on the signal's true ends (the reflect padding) where those lie within ``R``.  The
two rules of a stream with that reach, and the loop that drives it, are zerovox_amd.stream's.  A stream denoised in these windows is
bit-identical to one whole-signal call: the frame grid is the signal's wherever the window was cut, a frame's transform depends on its
own samples only, and the overlap-add runs over the same frames in the same order.  The price is delay -- a denoised stream runs ``R``
samples behind its input (1023 samples, 46 ms, at n_fft 1024 and 22.05 kHz) -- and work: every window transforms again the up to
``2 n_fft / hop`` frames that reach into its history.
"""
from __future__ import annotations

from .stream import ReachPlanner, stream_windows


def reach(n_fft):
    """R = n_fft - 1: how far to either side an output sample of the denoiser depends on its input"""
    return int(n_fft) - 1


class DenoisePlanner(ReachPlanner):
    """Plans the zvx_denoise_ex windows of one stream: a ReachPlanner of reach(n_fft); window_fn is Context.denoise_window on one row."""

    def __init__(self, n_fft):
        super().__init__(reach(n_fft))
        self.n_fft = int(n_fft)


stream_denoise = stream_windows               # stream_denoise(chunks, DenoisePlanner(n_fft), window_fn)
