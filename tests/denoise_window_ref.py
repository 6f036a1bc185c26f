"""Float64 NumPy restatement of the WINDOWED vocoder-bias denoiser as include/zvx.h defines it (zvx_denoise_ex), on top of denoise_ref: the
frame grid of the whole signal laid over a window that holds samples [in_origin, in_origin + len) of it, the mirrors only where the signal's
own ends are in the window, the frames that cover an emitted sample and no others, the overlap-add in ascending f.  Every read of the
window is checked: an index outside it is an AssertionError, so a result proves that the support condition sufficed.  The reference
project has no denoiser; nothing here is taken from it."""
import numpy as np

import denoise_ref as D
from stream_util import supported


def reach(n_fft):
    return n_fft - 1


def cuts(n, n_fft, hop):
    """the piece boundaries of the issue: 0, 1, hop - 1, hop, hop + 1, n_fft, n_fft + 1, n / 2 + 1, n - 1, n (those inside the row)"""
    return sorted({c for c in (0, 1, hop - 1, hop, hop + 1, n_fft, n_fft + 1, n // 2 + 1, n - 1, n) if 0 <= c <= n})


def frame_range(out_begin, cnt, n_fft, hop, F):
    """frames [f_lo, f_hi] that cover an emitted sample: f hop <= p < f hop + n_fft for a padded position p = i + pad of the range (F: the
    signal's frame count, None where the signal continues)"""
    pad = (n_fft - hop) // 2
    p0, p1 = out_begin + pad, out_begin + cnt - 1 + pad
    f_lo = 0 if p0 < n_fft else (p0 - n_fft) // hop + 1
    f_hi = p1 // hop if F is None else min(F - 1, p1 // hop)
    return f_lo, f_hi


def denoise_window(samples, bias, strength, floor, in_origin, out_begin, out_count, last, n_fft=1024, hop=256, win_length=1024, reads=None):
    """samples: [in_origin, in_origin + len) of the signal -> the outputs [out_begin, out_begin + cnt) of denoise_ref.denoise on the whole
    signal, float64; cnt = out_count, or to the signal's end with -1 (needs last).  reads: a list that receives (lowest, highest) window
    index read."""
    x = np.asarray(samples, np.float64)
    k = len(x)
    assert in_origin >= 0 and out_begin >= 0 and out_count >= -1 and (out_count >= 0 or last)
    cnt = out_count if out_count >= 0 else max(0, in_origin + k - out_begin)
    if cnt == 0:
        return np.zeros(0)
    assert supported(reach(n_fft), in_origin, k, out_begin, cnt, last), (in_origin, k, out_begin, cnt, last)
    a = out_begin - in_origin
    if strength == 0:
        return x[a:a + cnt].copy()
    pad = (n_fft - hop) // 2
    N = in_origin + k if last else None                      # the signal's length, where it is known
    if last:
        assert N >= D.min_samples(n_fft, hop), N
    F = None if N is None else 1 + (N + 2 * pad - n_fft) // hop
    f_lo, f_hi = frame_range(out_begin, cnt, n_fft, hop, F)
    w = D.window(n_fft, win_length)
    w2 = w ** 2
    lo_read, hi_read = k, -1
    yw = {}
    for f in range(f_lo, f_hi + 1):
        s = f * hop - pad + np.arange(n_fft)                 # absolute sample indices of the frame
        if in_origin == 0:
            s = np.where(s < 0, -s, s)                       # the reflect at sample 0: only in a window that starts there
        if last:
            s = np.where(s >= N, 2 * (N - 1) - s, s)         # the reflect at N - 1: only in the last window
        j = s - in_origin
        assert j.min() >= 0 and j.max() < k, ("a read outside the window", f, int(j.min()), int(j.max()), k)
        lo_read, hi_read = min(lo_read, int(j.min())), max(hi_read, int(j.max()))
        X = np.fft.rfft(x[j] * w)
        m = np.abs(X)
        sb = float(strength) * np.asarray(bias, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.where(m > 0, np.maximum(float(floor), 1.0 - sb / np.where(m > 0, m, 1.0)), float(floor))
        Xg = G * X
        Xg[0] = Xg[0].real
        Xg[-1] = Xg[-1].real
        yw[f] = np.fft.irfft(Xg, n=n_fft) * w
    if reads is not None:
        reads.append((lo_read, hi_read))
    thr = D.den_threshold(n_fft, hop, win_length)
    p = out_begin + pad + np.arange(cnt)                     # padded positions of the emitted samples
    num, den = np.zeros(cnt), np.zeros(cnt)
    for f in range(f_lo, f_hi + 1):                          # ascending f: the order is part of the contract
        t = p - f * hop
        hit = (t >= 0) & (t < n_fft)                         # f hop <= p < f hop + n_fft; f <= F - 1 by frame_range
        num[hit] += yw[f][t[hit]]
        den[hit] += w2[t[hit]]
    covered = den >= thr
    out = x[a:a + cnt].copy()
    out[covered] = num[covered] / den[covered]
    return out
