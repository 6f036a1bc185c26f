"""float64 / NumPy reference of zvx_trim_bounds and zvx_join as include/zvx.h states them.  Imports nothing from zerovox_amd."""
import numpy as np

AMBIGUOUS = 1e-9                 # a frame whose p / (pmax k) lies within this of 1 may be decided either way (include/zvx.h)


def frame_powers(x, frame, hop):
    """p[f]: sum of squares of frame f, accumulated in double, with frame // 2 zeros on both sides of the row"""
    x = np.asarray(x, np.float32).astype(np.float64)
    pad = frame // 2
    xp = np.concatenate([np.zeros(pad), x, np.zeros(pad)])
    nf = 1 + (len(xp) - frame) // hop
    # (summed frame by frame, no prefix sums: their cancellation would cost the digits the ambiguity band needs)
    return np.array([np.sum(xp[f * hop:f * hop + frame] ** 2) for f in range(nf)], np.float64)


def bounds_ref(x, frame=2048, hop=512, top_db=40.0, keep=0):
    """-> (begin, end, worst): the samples [begin, end) zvx_join keeps of the row, and how close any frame comes to the threshold:
    the minimum over frames of |p / (pmax k) - 1| (inf where nothing is compared); below AMBIGUOUS the row has an ambiguous frame."""
    x = np.asarray(x, np.float32)
    n = len(x)
    top_db = float(np.float32(top_db))
    if top_db <= 0 or n < frame:
        return 0, n, np.inf
    p = frame_powers(x, frame, hop)
    pmax = float(p.max())
    if pmax < 1e-20 * frame:
        return 0, n, np.inf
    k = 10.0 ** (-top_db / 10.0)
    thr = pmax * k
    worst = float(np.min(np.abs(p / thr - 1.0)))
    audio = np.flatnonzero(p > thr)
    if audio.size == 0:
        return 0, 0, worst
    first, last = int(audio[0]), int(audio[-1])
    return max(0, first * hop - keep), min(n, (last + 1) * hop + keep), worst


def pcm16(v):
    """(int16) trunc(clamp(v * 32760, -32768, 32767)) with the product in f32"""
    v = np.asarray(v, np.float32) * np.float32(32760.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


def segment_ref(x, begin, end, fade):
    """x[begin:end] with the linear ramp over F = min(fade, m // 2) samples at both ends, one f32 division and one f32 multiply"""
    seg = np.asarray(x, np.float32)[begin:end].copy()
    m = len(seg)
    F = min(int(fade), m // 2)
    if F > 0:
        i = np.arange(F, dtype=np.int64)
        g = (2 * i + 1).astype(np.float32) / np.float32(2 * F)
        seg[:F] = seg[:F] * g
        seg[m - F:] = seg[m - F:] * g[::-1]
    return seg


def join_ref(rows, gaps=None, frame=2048, hop=512, top_db=40.0, keep=0, fade=0, as_pcm16=False):
    """-> (out, seg_pos int64 [B], seg_begin [B], seg_len [B]); out is float32, or int16 by the PCM16 rule"""
    B = len(rows)
    gaps = [0] * B if gaps is None else [int(g) for g in gaps]
    parts, pos, begins, lens, at = [], [], [], [], 0
    for b, x in enumerate(rows):
        begin, end, _ = bounds_ref(x, frame, hop, top_db, keep)
        seg = segment_ref(x, begin, end, fade)
        pos.append(at); begins.append(begin); lens.append(len(seg))
        parts += [seg, np.zeros(gaps[b], np.float32)]
        at += len(seg) + gaps[b]
    out = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return (pcm16(out) if as_pcm16 else out), np.array(pos, np.int64), np.array(begins, np.int32), np.array(lens, np.int32)


def make_rows(seed):
    """The rows of the bounds / join tests: Gaussian noise at 1e-4 with, from 5000 samples up, 1 + n // 30000 bursts of Gaussian noise at
    0.2 under a 400-sample linear attack and release, plus one all-zero and one all-loud row of 9000 samples."""
    rng = np.random.default_rng(seed)
    rows = []
    for n in (2047, 2048, 5000, 22050, 66151, 131089):
        x = rng.standard_normal(n) * 1e-4
        if n >= 5000:
            for _ in range(1 + n // 30000):
                ln = int(rng.integers(1200, max(1201, n // 3)))
                at = int(rng.integers(0, n - ln))
                env = np.minimum(1.0, np.minimum(np.arange(ln) + 1, ln - np.arange(ln)) / 400.0)
                x[at:at + ln] += rng.standard_normal(ln) * 0.2 * env
        rows.append(x.astype(np.float32))
    rows.append(np.zeros(9000, np.float32))
    rows.append((rng.standard_normal(9000) * 0.2).astype(np.float32))
    return rows
