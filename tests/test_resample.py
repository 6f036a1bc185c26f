"""Sample-rate conversion, the parts that need no GPU: the tests' float64 reference against scipy, the length rule, the stream
planner (driven with the reference in place of the device) and the exported names."""
import os
import re

import numpy as np
import pytest

import resample_ref as R
from zerovox_amd import _lib
from zerovox_amd.resample import StreamPlanner, rate_pair, stream_resample

PAIRS = [(22050, 48000), (22050, 44100), (22050, 24000), (22050, 16000), (22050, 8000),
         (16000, 22050), (24000, 22050), (44100, 22050), (48000, 22050), (22050, 32000), (32000, 22050)]


def _signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return [rng.uniform(-1, 1, n), np.sin(2 * np.pi * 0.0137 * t) * 0.8]


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_reference_matches_scipy_resample_poly(rate_in, rate_out):
    """pins tests/resample_ref.py to an implementation the project did not write"""
    sig = pytest.importorskip("scipy.signal")
    L, M = R.pair(rate_in, rate_out)
    for n in (1, 2, 255, 3001):
        for i, x in enumerate(_signals(n, 17 * n + rate_out)):
            want = sig.resample_poly(x, L, M)
            got = R.resample_ref(x, rate_in, rate_out)
            assert len(got) == len(want) == R.out_len(n, rate_in, rate_out), (n, i, len(got), len(want))
            d = np.abs(got - want).max()
            assert d <= 1e-12, (rate_in, rate_out, n, i, d)


def test_resampled_len_is_the_integer_ceiling():
    from fractions import Fraction
    from math import ceil
    for rate_in, rate_out in PAIRS + [(22050, 22050), (8000, 192000), (192000, 4000)]:
        for n in (0, 1, 2, 3, 255, 256, 22050, 66151, 2 ** 31 - 1, 2 ** 31 - 441, 2 ** 31 - 2):
            want = ceil(Fraction(n * rate_out, rate_in))
            assert _lib.resampled_len(n, rate_in, rate_out) == want, (n, rate_in, rate_out)
            assert R.out_len(n, rate_in, rate_out) == want
    assert _lib.resampled_len(229376, 22050, 48000) == 499322
    assert _lib.resampled_len(0, 22050, 8000) == 0


@pytest.mark.parametrize("rate_out", [48000, 16000, 8000, 22050])
@pytest.mark.parametrize("chunk_frames", [1, 7, 64])
def test_stream_planner_pieces_concatenate_to_the_whole_signal(rate_out, chunk_frames):
    rate_in, hop = 22050, 256
    n = 157 * hop + 93                                        # not a multiple of any chunk size (157 is prime; + a ragged tail)
    x = np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)
    whole = R.resample_ref(x, rate_in, rate_out)
    L, M, half = rate_pair(rate_in, rate_out)
    step = chunk_frames * hop
    chunks = [x[i:i + step] for i in range(0, n, step)]
    assert len(chunks[-1]) != step

    emitted, kept = [], []

    class Feed:
        """the chunks as an iterator that counts what the driver has taken from it"""
        def __init__(self):
            self.it, self.nexts, self.received, self.done = iter(chunks), 0, 0, False

        def __iter__(self):
            return self

        def __next__(self):
            self.nexts += 1
            try:
                c = next(self.it)
            except StopIteration:
                self.done = True
                raise
            self.received += len(c)
            return c

    feed = Feed()

    def window(samples, in_origin, out_begin, out_count):
        assert not emitted or out_begin == emitted[-1][0] + emitted[-1][1], "an output is skipped or emitted twice"
        if not feed.done:                                     # every piece but the closing one: final by the samples received so far
            assert (out_begin + out_count - 1) * M + half <= (feed.received - 1) * L, (out_begin, out_count, feed.received)
        emitted.append((out_begin, out_count))
        kept.append(len(samples))
        return R.resample_window(samples, rate_in, rate_out, in_origin, out_begin, out_count)

    stream = stream_resample(feed, rate_in, rate_out, window)
    pieces = [next(stream)]
    assert len(chunks) > 2 and feed.nexts == 1 and feed.received == len(chunks[0])      # no chunk is held back for the next one
    pieces += list(stream)
    assert feed.done and feed.nexts == len(chunks) + 1
    got = np.concatenate(pieces)
    assert emitted[0][0] == 0 and sum(c for _, c in emitted) == len(whole) == R.out_len(n, rate_in, rate_out)
    assert got.shape == whole.shape and np.array_equal(got, whole)
    assert max(kept) <= 2 * half / L + 2 + step, (max(kept), 2 * half / L + 2 + step)


def test_stream_planner_finality_rule():
    """an output is released only when every sample under its filter has arrived, and no later than that"""
    for rate_out in (48000, 8000):
        L, M, half = rate_pair(22050, rate_out)
        plan = StreamPlanner(22050, rate_out)
        for n_new in (300, 1, 256, 4000):
            _, begin, count, keep = plan.push(n_new)
            end = begin + count
            if end > 0:
                assert (end - 1) * M + half <= (plan.received - 1) * L
            assert end * M + half > (plan.received - 1) * L
            assert keep <= max(0, -(-(end * M - half) // L))
        _, begin, count, _ = plan.push(5, last=True)
        assert begin + count == _lib.resampled_len(plan.received, 22050, rate_out)
    assert rate_pair(22050, 22050) == (1, 1, 0)


def test_header_binding_and_library_carry_the_new_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "zvx.h")).read()
    for name in ("zvx_resample", "zvx_resample_ex"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    assert re.search(r"ZVX_NATIVE_RATE\s*=\s*32\b", hdr) and _lib.ZVX_NATIVE_RATE == 32
    assert re.search(r"ZVX_T_RESAMPLE\s*=\s*6\b", hdr) and _lib.ZVX_T_RESAMPLE == 6
    assert re.search(r"ZVX_T_COUNT\s*=\s*8\b", hdr) and _lib.ZVX_T_COUNT == 8
    assert _lib.STAGES == ("encoder", "variance", "lenreg", "decoder", "vocoder", "spkemb")
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        h = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(h, "zvx_resample") and hasattr(h, "zvx_resample_ex")
