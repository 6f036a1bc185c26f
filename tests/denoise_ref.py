"""Float64 NumPy restatement of the vocoder-bias denoiser as include/zvx.h defines it (zvx_denoise, zvx_denoise_bias): framing, analysis, gain,
synthesis and overlap-add written out from the definition, with plain DFT matrices where the sizes allow and numpy.fft otherwise.  The
reference project has no denoiser; nothing here is taken from it."""
import numpy as np


def window(n_fft, win_length):
    """the periodic Hann of win_length centred in n_fft, float64 (mels.stft_basis's window)"""
    w = np.hanning(win_length + 1)[:-1].astype(np.float64)
    lp = (n_fft - win_length) // 2
    return np.pad(w, (lp, n_fft - win_length - lp))


def geometry(n, n_fft, hop):
    """-> (pad, F): the reflect padding and the frame count of a row of n samples (zvx_melspec's)"""
    pad = (n_fft - hop) // 2
    return pad, 1 + (n + 2 * pad - n_fft) // hop


def min_samples(n_fft, hop):
    pad = (n_fft - hop) // 2
    return max(pad + 1, n_fft - 2 * pad)


def frames(x, n_fft, hop):
    """-> [F][n_fft] float64: frame f = xp[f hop .. f hop + n_fft), xp the reflect-padded row"""
    x = np.asarray(x, np.float64)
    pad, F = geometry(len(x), n_fft, hop)
    xp = np.pad(x, (pad, pad), mode="reflect")
    idx = np.arange(n_fft)[None, :] + hop * np.arange(F)[:, None]
    return xp[idx]


def analysis(x, n_fft, hop, win_length):
    """-> X [F][nf] complex128"""
    return np.fft.rfft(frames(x, n_fft, hop) * window(n_fft, win_length)[None, :], axis=1)


def den_threshold(n_fft, hop, win_length):
    """1e-3 * max_t sum_j w[t + j hop]^2"""
    w2 = window(n_fft, win_length) ** 2
    return 1e-3 * max(w2[t::hop].sum() for t in range(hop))


def overlap_add(yw, x, n_fft, hop, win_length):
    """yw [F][n_fft] = w[t] y_f[t] -> (out [n], covered [n] bool): num / den where den >= the threshold, x elsewhere; sums in ascending f"""
    x = np.asarray(x, np.float64)
    n = len(x)
    pad, F = geometry(n, n_fft, hop)
    w2 = window(n_fft, win_length) ** 2
    num, den = np.zeros(n + 2 * pad), np.zeros(n + 2 * pad)
    for f in range(F):
        num[f * hop:f * hop + n_fft] += yw[f]
        den[f * hop:f * hop + n_fft] += w2
    num, den = num[pad:pad + n], den[pad:pad + n]
    covered = den >= den_threshold(n_fft, hop, win_length)
    out = x.copy()
    out[covered] = num[covered] / den[covered]
    return out, covered


def amplification(n, n_fft, hop, win_length):
    """[n] float64: sum_f w / sum_f w^2 over the frames that cover a sample (0 where none does) -- the factor by which an error of the
    synthesised frames y_f reaches the output; 4 / 3 in the interior of a Hann at hop = n_fft / 4"""
    pad, F = geometry(n, n_fft, hop)
    w = window(n_fft, win_length)
    s1, s2 = np.zeros(n + 2 * pad), np.zeros(n + 2 * pad)
    for f in range(F):
        s1[f * hop:f * hop + n_fft] += w
        s2[f * hop:f * hop + n_fft] += w * w
    s1, s2 = s1[pad:pad + n], s2[pad:pad + n]
    return np.where(s2 >= den_threshold(n_fft, hop, win_length), s1 / np.where(s2 > 0, s2, 1.0), 0.0)


def denoise(x, bias, strength, floor=0.0, n_fft=1024, hop=256, win_length=1024, with_cover=False):
    """one row -> the denoised row, float64 (strength == 0: the row itself)"""
    x = np.asarray(x, np.float64)
    if strength == 0 or len(x) == 0:
        return (x.copy(), np.ones(len(x), bool)) if with_cover else x.copy()
    w = window(n_fft, win_length)
    X = analysis(x, n_fft, hop, win_length)
    m = np.abs(X)
    sb = float(strength) * np.asarray(bias, np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(m > 0, np.maximum(float(floor), 1.0 - sb / np.where(m > 0, m, 1.0)), float(floor))
    Xg = G * X
    Xg[:, 0] = Xg[:, 0].real                                 # the imaginary parts of DC and Nyquist are ignored
    Xg[:, -1] = Xg[:, -1].real
    y = np.fft.irfft(Xg, n=n_fft, axis=1)                    # (1 / n_fft) sum_k c_k Re(X' e^(+2 pi i k t / n_fft))
    out, covered = overlap_add(y * w[None, :], x, n_fft, hop, win_length)
    return (out, covered) if with_cover else out


def bias_of(wav, n_fft=1024, hop=256, win_length=1024):
    """the mean over all frames of |X[f][k]| -> [nf] float64"""
    return np.abs(analysis(wav, n_fft, hop, win_length)).mean(axis=0)


def pcm16(v):
    """the resampler's rule: (int16) trunc(clamp(v * 32760, -32768, 32767)) on f32 samples"""
    v = np.asarray(v, np.float32) * np.float32(32760.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
