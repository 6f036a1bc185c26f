"""Float64 NumPy restatement of the keyed audio watermark and its detector as include/zvx.h defines them (zvx_watermark, zvx_watermark_ex,
zvx_watermark_detect), on top of denoise_ref's framing, window and overlap-add: bands, the keyed sign pattern, the per-band gain, the
windowed form with checked reads, and the detector written out offset by offset from the definition (no folding).  The reference project
has no watermark; nothing here is taken from it."""
import math

import numpy as np

import denoise_ref as D
from denoise_window_ref import frame_range, reach  # noqa: F401  (reach: n_fft - 1, the denoiser's)
from stream_util import supported

M64 = (1 << 64) - 1
DEFAULTS = dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64)


def mix64(z):
    """the splitmix64 finaliser on Python ints"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def bands(lo_hz, hi_hz, band_bins, n_fft, rate):
    """-> (k_lo, J): band j is bins [k_lo + j KB, k_lo + (j + 1) KB)"""
    lo, hi = float(np.float32(lo_hz)), float(np.float32(hi_hz))              # the C struct carries f32
    k_lo = math.ceil(lo * n_fft / rate)
    J = math.floor((min(hi * n_fft / rate, n_fft / 2) - k_lo) / band_bins)
    return int(k_lo), int(J)


def sign_table(key, P, J):
    """[P][J] of +1 / -1"""
    key = int(key) & M64
    return np.array([[1 if mix64(key ^ ((c << 32) | j)) >> 63 else -1 for j in range(J)] for c in range(P)], np.int64)


def gains(depth_db):
    """(g_up, g_dn): computed in double, rounded once to f32"""
    d = float(np.float32(depth_db))
    return float(np.float32(10.0 ** (d / 20.0))), float(np.float32(10.0 ** (-d / 20.0)))


def bin_gain(key, f, depth_db, lo_hz, hi_hz, block_frames, band_bins, period_blocks, n_fft, rate):
    """[nf] float64: the gain of every bin of the SIGNAL's frame f (1 outside the bands)"""
    k_lo, J = bands(lo_hz, hi_hz, band_bins, n_fft, rate)
    assert J >= 3, J
    g_up, g_dn = gains(depth_db)
    c = (int(f) // block_frames) % period_blocks
    key = int(key) & M64
    G = np.ones(n_fft // 2 + 1)
    for j in range(J):
        s = mix64(key ^ ((c << 32) | j)) >> 63
        G[k_lo + j * band_bins:k_lo + (j + 1) * band_bins] = g_up if s else g_dn
    return G


def embed(x, key, depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64, n_fft=1024, hop=256,
          win_length=1024, rate=22050):
    """one whole row -> the marked row, float64 (depth 0 or an empty row: the row itself)"""
    x = np.asarray(x, np.float64)
    if depth_db == 0 or len(x) == 0:
        return x.copy()
    return embed_window(x, key, 0, 0, -1, True, depth_db, lo_hz, hi_hz, block_frames, band_bins, period_blocks, n_fft, hop, win_length, rate)


def embed_window(samples, key, in_origin, out_begin, out_count, last, depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4,
                 period_blocks=64, n_fft=1024, hop=256, win_length=1024, rate=22050):
    """samples: [in_origin, in_origin + len) of the signal -> the outputs [out_begin, out_begin + cnt) of embed on the whole signal,
    float64; every read of the window is checked (an index outside it is an AssertionError)"""
    x = np.asarray(samples, np.float64)
    k = len(x)
    assert in_origin >= 0 and out_begin >= 0 and out_count >= -1 and (out_count >= 0 or last)
    cnt = out_count if out_count >= 0 else max(0, in_origin + k - out_begin)
    if cnt == 0:
        return np.zeros(0)
    assert supported(reach(n_fft), in_origin, k, out_begin, cnt, last), (in_origin, k, out_begin, cnt, last)
    a = out_begin - in_origin
    if depth_db == 0:
        return x[a:a + cnt].copy()
    pad = (n_fft - hop) // 2
    N = in_origin + k if last else None
    if last:
        assert N >= D.min_samples(n_fft, hop), N
    F = None if N is None else 1 + (N + 2 * pad - n_fft) // hop
    f_lo, f_hi = frame_range(out_begin, cnt, n_fft, hop, F)
    w = D.window(n_fft, win_length)
    w2 = w ** 2
    yw = {}
    for f in range(f_lo, f_hi + 1):
        s = f * hop - pad + np.arange(n_fft)
        if in_origin == 0:
            s = np.where(s < 0, -s, s)
        if last:
            s = np.where(s >= N, 2 * (N - 1) - s, s)
        j = s - in_origin
        assert j.min() >= 0 and j.max() < k, ("a read outside the window", f, int(j.min()), int(j.max()), k)
        X = np.fft.rfft(x[j] * w)
        Xg = X * bin_gain(key, f, depth_db, lo_hz, hi_hz, block_frames, band_bins, period_blocks, n_fft, rate)
        Xg[0] = Xg[0].real
        Xg[-1] = Xg[-1].real
        yw[f] = np.fft.irfft(Xg, n=n_fft) * w
    thr = D.den_threshold(n_fft, hop, win_length)
    p = out_begin + pad + np.arange(cnt)
    num, den = np.zeros(cnt), np.zeros(cnt)
    for f in range(f_lo, f_hi + 1):                          # ascending f
        t = p - f * hop
        hit = (t >= 0) & (t < n_fft)
        num[hit] += yw[f][t[hit]]
        den[hit] += w2[t[hit]]
    covered = den >= thr
    out = x[a:a + cnt].copy()
    out[covered] = num[covered] / den[covered]
    return out


def band_contrast(x, lo_hz=250.0, hi_hz=8000.0, band_bins=4, n_fft=1024, hop=256, win_length=1024, rate=22050):
    """-> D [F][J - 2] float64 (column j - 1 is band j), J"""
    k_lo, J = bands(lo_hz, hi_hz, band_bins, n_fft, rate)
    assert J >= 3, J
    X = D.analysis(x, n_fft, hop, win_length)
    Pw = X.real ** 2 + X.imag ** 2
    L = np.log2(np.maximum(Pw[:, k_lo:k_lo + J * band_bins], 1e-6))
    LB = L.reshape(L.shape[0], J, band_bins).sum(axis=2)
    return LB[:, 1:-1] - 0.5 * (LB[:, :-2] + LB[:, 2:]), J


def windows(F, window_frames):
    """the windows [fa, fb) of a row of F frames"""
    if F <= 0:
        return []
    if window_frames <= 0 or F <= window_frames:
        return [(0, F)]
    H = window_frames // 2
    nw = 1 + -(-(F - window_frames) // H)
    return [(w * H, min(w * H + window_frames, F)) for w in range(nw)]


def window_scores(Dm, sg, fa, fb, TB, P):
    """z(o) for every offset o in [0, P TB) of the window [fa, fb), straight from the definition (no folding): sg [P][J] -> [P TB]
    float64, or a stack of tables [K][P][J] -> [K][P TB] (the E of an offset do not depend on the key)"""
    sg = np.asarray(sg)
    S = sg[..., 1:-1].astype(np.float64).reshape(-1, P, Dm.shape[1])
    z = np.zeros((S.shape[0], P * TB))
    cs = np.vstack([np.zeros((1, Dm.shape[1])), np.cumsum(Dm[fa:fb], axis=0)])      # cs[i] = sum of the window's first i frames
    for o in range(P * TB):
        first, lastb = (fa + o) // TB, (fb - 1 + o) // TB
        edges = np.clip(np.arange(first, lastb + 2) * TB - o, fa, fb) - fa               # block m holds frames [m TB - o, (m + 1) TB - o)
        E = cs[edges[1:]] - cs[edges[:-1]]
        den = float((E * E).sum())
        if den > 0:
            rows = np.arange(first, lastb + 1) % P
            z[:, o] = np.einsum("kbj,bj->k", S[:, rows, :], E) / math.sqrt(den)
    return z[0] if sg.ndim == 2 else z


def detect(x, key, window_frames=256, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64, n_fft=1024, hop=256,
           win_length=1024, rate=22050, depth_db=None, full=False):
    """one row -> (score, offset, window, [(score, offset) per window]); full: the per-window z arrays instead of the list's pairs"""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return 0.0, 0, 0, []
    Dm, J = band_contrast(x, lo_hz, hi_hz, band_bins, n_fft, hop, win_length, rate)
    sg = sign_table(key, period_blocks, J)
    per, zs = [], []
    for fa, fb in windows(Dm.shape[0], window_frames):
        z = window_scores(Dm, sg, fa, fb, block_frames, period_blocks)
        o = int(np.argmax(z))                                # the smallest o that attains the largest z
        per.append((float(z[o]), o))
        zs.append(z)
    best = max(range(len(per)), key=lambda w: (per[w][0], -w))
    return per[best][0], per[best][1], best, (zs if full else per)


def null_scores(x, keys, window_frames=256, **kw):
    """the largest z over all offsets and windows for each key, sharing one analysis -> [len(keys)]"""
    kw = {**dict(lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64, n_fft=1024, hop=256, win_length=1024, rate=22050), **kw}
    Dm, J = band_contrast(x, kw["lo_hz"], kw["hi_hz"], kw["band_bins"], kw["n_fft"], kw["hop"], kw["win_length"], kw["rate"])
    S = np.stack([sign_table(key, kw["period_blocks"], J) for key in keys])
    z = [window_scores(Dm, S, fa, fb, kw["block_frames"], kw["period_blocks"]).max(axis=1) for fa, fb in windows(Dm.shape[0], window_frames)]
    return np.max(np.stack(z), axis=0)


def voiced_signal(seconds, seed, rate=22050):
    """a seeded synthetic voiced signal with pauses: a harmonic source with a wandering F0 through three moving formant resonances, plus
    breath noise, in syllables of 120 .. 350 ms with pauses of 40 .. 250 ms between them -> [n] float32, |x| <= 0.9"""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * rate))
    t = np.arange(n) / rate
    f0 = 120.0 + 25.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6)) + 10.0 * np.sin(2 * np.pi * 2.3 * t + rng.uniform(0, 6))
    phase = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(n)
    form = [(600.0 + 250.0 * np.sin(2 * np.pi * 1.1 * t + 1.0), 90.0), (1500.0 + 500.0 * np.sin(2 * np.pi * 0.8 * t + 2.0), 120.0),
            (2800.0 + 400.0 * np.sin(2 * np.pi * 0.5 * t), 200.0), (4200.0 + 0.0 * t, 400.0), (6500.0 + 0.0 * t, 800.0)]
    for h in range(1, 70):
        fh = h * f0
        amp = np.zeros(n)
        for i, (fc, bw) in enumerate(form):
            amp += (0.6 ** i) / (1.0 + ((fh - fc) / bw) ** 2)
        x += np.where(fh < 0.45 * rate, amp, 0.0) * np.sin(h * phase + rng.uniform(0, 6)) / h ** 0.3
    x += 0.02 * rng.standard_normal(n) * (1.0 + np.sin(2 * np.pi * 3.0 * t))
    env = np.zeros(n)
    pos = int(rng.uniform(0.0, 0.05) * rate)
    while pos < n:
        syl = int(rng.uniform(0.12, 0.35) * rate)
        e = np.hanning(2 * int(0.02 * rate))
        seg = np.ones(syl)
        k = min(len(e) // 2, syl // 2)
        seg[:k] = e[:k]; seg[-k:] = e[-k:]
        end = min(n, pos + syl)
        env[pos:end] = seg[:end - pos] * rng.uniform(0.5, 1.0)
        pos = end + int(rng.uniform(0.04, 0.25) * rate)
    x = x * env + 1e-4 * rng.standard_normal(n)
    return (0.9 * x / np.max(np.abs(x))).astype(np.float32)
