"""Keyed audio watermark (include/zvx.h: zvx_watermark, zvx_watermark_ex, zvx_watermark_rows, zvx_watermark_detect, zvx_watermark_identify):
defaults, the sign table, per-request keys from one secret (derive_key), the results of a detection and of an identification among many
keys, and the streaming side -- which outputs are final, what history to keep.

Pure Python, importable without the library.  The mark is a multiplicative spread-spectrum pattern on the denoiser's STFT frame grid: bands
of ``band_bins`` bins between ``lo_hz`` and ``hi_hz`` are scaled up or down by ``depth_db`` in blocks of ``block_frames`` frames, by a
keyed +1 / -1 table that repeats every ``period_blocks`` blocks.  The detector correlates band log-energy contrasts with that table over
every hop-granular offset.  The embedder has the denoiser's support: output ``i`` depends on the input within ``R = n_fft - 1`` of it, so
a stream marked in these windows is bit-identical to one whole-signal call and runs ``R`` samples behind its input.

What is measured: the arithmetic against a float64 restatement, and detection on synthetic voiced signals (tests/test_watermark.py).  Not
measured, and not claimed: inaudibility on a real checkpoint, robustness against lossy codecs, time-stretching or deliberate removal.  Short
clips cut to the telephone band are not reliably detectable.
"""
from __future__ import annotations

from collections import namedtuple

from .stream import ReachPlanner, stream_windows

M64 = (1 << 64) - 1
EMBED_DEFAULTS = dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64)
WINDOW_FRAMES = 256
# The default decision threshold on the detector's score.  Measured with the float64 restatement at the defaults above, depth 1 dB, on the
# seeded synthetic voiced signals of tests/test_watermark.py (1.5 s and 3 s at 22.05 kHz): the largest null score over 256 wrong keys, the
# unmarked signals and all 512 offsets is 4.75; the smallest score with the right key (aligned, or cut by 5000 samples) is 7.10.  The threshold lies
# between them, nearer the null side.
THRESHOLD = 5.5

WatermarkResult = namedtuple("WatermarkResult", "score offset window detected threshold windows")
WatermarkResult.__doc__ = """score: the best window's largest z; offset: the smallest offset (in frames, modulo period_blocks * block_frames)
that attains it; window: that window's index; detected: score >= threshold; windows: [(score, offset)] of every window"""


def mix64(z):
    """the splitmix64 finaliser"""
    z = (int(z) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sign_table(key, period_blocks, bands):
    """[period_blocks][bands] of +1 / -1: sign(c, j) = +1 where bit 63 of mix64(key ^ (c << 32 | j)) is set"""
    key = int(key) & M64
    return [[1 if mix64(key ^ ((c << 32) | j)) >> 63 else -1 for j in range(int(bands))] for c in range(int(period_blocks))]


def derive_key(master, ident):
    """A per-customer or per-request key from one secret: ``mix64(master ^ mix64(h))``, all in 64-bit arithmetic, where

    * ``master`` is an int in [0, 2^64);
    * for an int ``ident`` in [0, 2^64), ``h = ident``;
    * for a bytes-like ``ident``, ``h`` folds it 8 bytes at a time: ``h = len(ident)``; then for each chunk, in order,
      ``h = mix64(h ^ w)``, ``w`` the chunk as a little-endian integer (the last chunk may be shorter: its missing high bytes are 0).

    To find who asked for a clip later, derive the keys of the candidates again and hand them to ``identify_watermark``.  ValueError for
    anything else (a bool, a str, a number out of range)."""
    if not isinstance(master, int) or isinstance(master, bool) or not 0 <= master <= M64:
        raise ValueError(f"derive_key: master must be an int in [0, 2^64), not {master!r}")
    if isinstance(ident, (bytes, bytearray, memoryview)):
        data = bytes(ident)
        h = len(data) & M64
        for i in range(0, len(data), 8):
            h = mix64(h ^ int.from_bytes(data[i:i + 8], "little"))
    elif isinstance(ident, int) and not isinstance(ident, bool):
        if not 0 <= ident <= M64:
            raise ValueError(f"derive_key: an int ident must lie in [0, 2^64), not {ident!r}")
        h = ident
    else:
        raise ValueError(f"derive_key: ident must be an int or bytes, not {ident!r}")
    return mix64(master ^ mix64(h))


IdentifyResult = namedtuple("IdentifyResult", "best key score offset window margin detected threshold scores")
IdentifyResult.__doc__ = """best: the index of the candidate key with the row's largest score (the smallest such index), key: that key;
score, offset, window: what the detector gives with it; margin: score minus the second-best candidate's score (score itself with one
candidate); detected: score >= threshold; scores: every candidate's score [K].  The largest score among WRONG keys grows with the number
of keys tried: THRESHOLD was measured over 256 wrong keys and nothing beyond, so with many more candidates look at the margin too."""


def identify_result(keys, scores, offsets, windows, best=None, threshold=None):
    """one row's IdentifyResult from the per-key results [K] (best None: the smallest index of the largest score)"""
    scores = [float(v) for v in scores]
    if best is None:
        best = max(range(len(scores)), key=lambda k: (scores[k], -k))
    thr = THRESHOLD if threshold is None else float(threshold)
    second = max((v for k, v in enumerate(scores) if k != best), default=0.0)
    return IdentifyResult(int(best), int(keys[best]), scores[best], int(offsets[best]), int(windows[best]), scores[best] - second,
                          bool(scores[best] >= thr), thr, scores)


def params(watermark, **overrides):
    """the ``watermark=`` keyword (None, an int key, or a dict with ``key`` and any of the embedder's parameters) as a dict of the
    embedder's parameters with ``key``, or None; checked without a device"""
    if watermark is None:
        return None
    if isinstance(watermark, bool):
        raise ValueError(f"watermark must be None, an int key or a dict with 'key', not {watermark!r}")
    if isinstance(watermark, int):
        watermark = {"key": watermark}
    if not isinstance(watermark, dict) or "key" not in watermark:
        raise ValueError(f"watermark must be None, an int key or a dict with 'key', not {watermark!r}")
    p = {**EMBED_DEFAULTS, **watermark, **overrides}
    unknown = set(p) - set(EMBED_DEFAULTS) - {"key"}
    if unknown:
        raise ValueError(f"watermark: unknown parameters {sorted(unknown)}")
    check(p)
    return p


def check(p):
    """the library's checks of the parameters that need no model (ValueError)"""
    import math
    if not isinstance(p["key"], int) or isinstance(p["key"], bool) or not 0 <= p["key"] <= M64:
        raise ValueError(f"watermark: key must be an int in [0, 2^64), not {p['key']!r}")
    d = float(p["depth_db"])
    if not math.isfinite(d) or d < 0 or d > 6:
        raise ValueError(f"watermark: depth_db must be finite and lie in [0, 6], not {p['depth_db']!r}")
    lo, hi = float(p["lo_hz"]), float(p["hi_hz"])
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo < 0 or not lo < hi:
        raise ValueError(f"watermark: band {lo} .. {hi} Hz needs finite 0 <= lo_hz < hi_hz")
    if int(p["block_frames"]) < 1:
        raise ValueError(f"watermark: block_frames {p['block_frames']} must be at least 1")
    if int(p["band_bins"]) < 1:
        raise ValueError(f"watermark: band_bins {p['band_bins']} must be at least 1")
    if not 1 <= int(p["period_blocks"]) <= 256:
        raise ValueError(f"watermark: period_blocks {p['period_blocks']} outside [1, 256]")


def reach(n_fft):
    """R = n_fft - 1: the denoiser's reach -- the embedder runs on its frame grid"""
    return int(n_fft) - 1


class WatermarkPlanner(ReachPlanner):
    """Plans the zvx_watermark_ex windows of one stream: a ReachPlanner of reach(n_fft); window_fn is Context.watermark_window on one row."""

    def __init__(self, n_fft):
        super().__init__(reach(n_fft))
        self.n_fft = int(n_fft)


stream_watermark = stream_windows             # stream_watermark(chunks, WatermarkPlanner(n_fft), window_fn)
