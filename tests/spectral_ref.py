"""References, bounds and case tables of the spectral family: dn_fft (csrc/spectral_fft.h), k_denoise_frames / k_denoise_ola (spectral.hip),
k_watermark_frames / k_wm_bands / k_wm_search (watermark.hip).  No device, no library: tests/test_spectral_reference.py holds everything
here to its mutations on the host, tests/test_spectral_gpu.py runs the kernels against it.

(a) float64 references: numpy.fft for the FFT probe, watermark_ref.band_contrast / window_scores for the detector's two launches,
    denoise_ref.denoise and watermark_ref.embed / detect for the C-ABI cases.
(b) float32 restatements of the frame pipeline (window, forward transform, gain, inverse, 1 / n_fft, window, overlap-add in ascending
    frames, the division): ORDERINGS = a radix-2 FFT written out on complex64 (fft_r2) and scipy.fft on complex64.  Two valid f32
    orderings of the same mathematics: their distance from float64 is the noise scale, their distance from each other what a margin has
    to cover.  fft_r4 states the KERNEL's ordering (radix 4, a radix-2 pass first for odd log2 n); it carries the mutations and is no
    part of any bound.
(c) dense data (dense_margin): the restatements run over SEEDS data seeds x the orderings.  rms: E_kernel <= E_ref (1 + m), E_ref the
    larger of the orderings' mean rms error against float64, m = 3 x (max - min) / mean of the 16 values.  Largest element: 2 x the
    largest element error among the 16 runs.  Nothing is measured on a device.
(d) every FFT case (ct_cap): ||err||_2 <= L eta / (1 - L eta) sqrt(N) ||x||_2 per frame, L = log2 N, eta = mu + gamma_4 (sqrt 2 + mu),
    mu the twiddle table's own error.  Loose by about sqrt N; it catches O(1) errors and is the only bound of the structured inputs.
(e) k_wm_search on exact data (search_case): D holds small integers times a power of two, every f32 partial sum of e and t exact
    (ops_ref.exact_sum per column); num and den are then exact in double and z = v / sqrt(dd) is two correctly rounded operations.
    Score: the reference's f32 value or a neighbour (one f32 ulp leaves room for 2 ulp of double in the device's sqrt and division).
    Offset: exactly the reference's; ties are exact ties of identical (v, dd) pairs and land on the smallest offset.
(f) k_wm_bands by interval (bands_tolerance): delta = (c)'s largest-element bound on the case's spectrum; every band sum lies between
    sum log2(max((|X| - delta)+^2, 1e-6)) and sum log2(max((|X| + delta)^2, 1e-6)), widened by the power's three roundings, K_ULP["log"]
    ulp per call and the f32 sum's 2 n u sum|terms|; D's tolerance is the three bands' widths combined.  A frame whose windowed input is
    all zero transforms to exact zeros: every power sits at the clamp, every band sum is the same f32 value s, D = s - 0.5 (s + s) = 0."""
import functools
import math

import numpy as np
import scipy.fft

import denoise_ref as D
import watermark_ref as W
from kernel_ref import U
from ops_ref import K_ULP, exact_sum, ulp32

POINTS = 4096                       # DENOISE_POINTS
WM_TABLE = 12288
SEEDS = 8
F32, C64 = np.float32, np.complex64


# ------------------------------------------------------------------------------------------------------------------------------
# the FFT: twiddles, two f32 orderings, the kernel's ordering with its mutations
# ------------------------------------------------------------------------------------------------------------------------------
def twiddles(N):
    """[N][2] float32 (cos, -sin)(2 pi m / N): dn_tables's design, float64 rounded once"""
    ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(F32)


def twiddle_error(N):
    """mu: the largest distance of a table entry from the exact root of unity"""
    ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    t = twiddles(N).astype(np.float64)
    return float(np.max(np.hypot(t[:, 0] - np.cos(ang), t[:, 1] + np.sin(ang))))


def _tw(N):
    t = twiddles(N)
    return (t[:, 0] + 1j * t[:, 1].astype(C64)).astype(C64)


def _c(re, im):
    out = np.empty(re.shape, C64)
    out.real, out.imag = re, im
    return out


def fft_r2(x, inverse=False):
    """[frames][N] complex64 -> the unnormalised DFT (inverse: conjugate kernel), radix 2 decimation in time, Stockham order, on the f32 table"""
    x = np.asarray(x, C64)
    N = x.shape[-1]
    tw = np.conj(_tw(N)) if inverse else _tw(N)
    half = N // 2
    j = np.arange(half)
    p = 1
    while p < N:
        k = j & (p - 1)
        a, b = x[..., j], x[..., j + half]
        if p > 1:
            b = b * tw[k * (N // (2 * p))]
        y = np.empty_like(x)
        o = ((j - k) << 1) + k
        y[..., o], y[..., o + p] = a + b, a - b
        x = y
        p <<= 1
    return x


def fft_scipy(x, inverse=False):
    x = np.asarray(x, C64)
    y = scipy.fft.ifft(x, axis=-1, norm="forward") if inverse else scipy.fft.fft(x, axis=-1)
    assert y.dtype == C64
    return y


FFT_MUTATIONS = ["inverse_twiddle_not_conjugated", "twiddle_stride_x2", "radix2_pass_dropped", "minus_i_t3_wrong_sign"]


def fft_r4(x, inverse=False, mut=None):
    """dn_fft as spectral_fft.h writes it, on complex64 in NumPy: a radix-2 pass first where log2 N is odd, then radix-4 passes with
    sub-transform size p: inputs x[j + r N / 4] times twid[r k N / (4 p)], outputs y[4 (j - k) + k + r p]"""
    x = np.asarray(x, C64)
    N = x.shape[-1]
    log2n = N.bit_length() - 1
    tw = _tw(N)
    if inverse and mut != "inverse_twiddle_not_conjugated":
        tw = np.conj(tw)
    p = 1
    if log2n & 1 and mut != "radix2_pass_dropped":
        half = N // 2
        a, b = x[..., :half], x[..., half:]
        y = np.empty_like(x)
        y[..., 0::2], y[..., 1::2] = a + b, a - b
        x, p = y, 2
    quarter = N // 4
    j = np.arange(quarter)
    while 4 * p <= N:
        k = j & (p - 1)
        v = [x[..., j + r * quarter] for r in range(4)]
        if p > 1:
            step = N // (4 * p) * (2 if mut == "twiddle_stride_x2" else 1)
            for r in range(1, 4):
                v[r] = v[r] * tw[(r * k * step) % N]
        t0, t1, t2, t3 = v[0] + v[2], v[0] - v[2], v[1] + v[3], v[1] - v[3]
        plus_i = inverse != (mut == "minus_i_t3_wrong_sign")
        q = _c(-t3.imag, t3.real) if plus_i else _c(t3.imag, -t3.real)
        y = np.empty_like(x)
        o = ((j - k) << 2) + k
        y[..., o], y[..., o + p], y[..., o + 2 * p], y[..., o + 3 * p] = t0 + t2, t1 + q, t0 - t2, t1 - q
        x = y
        p <<= 2
    return x


ORDERINGS = [("radix2", fft_r2), ("scipy", fft_scipy)]


def fft64(x, inverse=False):
    x = np.asarray(x, np.complex128)
    return np.fft.ifft(x, axis=-1) * x.shape[-1] if inverse else np.fft.fft(x, axis=-1)


def ct_cap(x, N):
    """(d) per frame of x [frames][N]: the cap on ||kernel - float64||_2"""
    L = N.bit_length() - 1
    g4 = 4 * U / (1 - 4 * U)
    eta = twiddle_error(N) + g4 * (math.sqrt(2.0) + twiddle_error(N))
    return L * eta / (1 - L * eta) * math.sqrt(N) * np.linalg.norm(np.asarray(x, np.complex128), axis=-1)


def round_trip_cap(x, X):
    """the cap on ||inverse(X) / N - x||_2 per frame, X the forward transform as computed: the forward error (at most ct_cap(x)) goes
    through the inverse, whose norm is sqrt N, and the inverse adds its own cap on the spectrum it was given"""
    N = x.shape[-1]
    return (math.sqrt(N) * ct_cap(x, N) + ct_cap(X, N)) / N


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the bound rule of dense data
# ------------------------------------------------------------------------------------------------------------------------------
def _rms(e):
    e = np.abs(np.asarray(e))
    return float(np.sqrt(np.mean(e * e))) if e.size else 0.0


class Margin:
    """E_ref, m and the largest-element limit of one dense case; errs: the 16 (rms, largest element) pairs they come from"""

    def __init__(self, errs):
        self.errs = errs
        per = {}
        for name, rms, _ in errs:
            per.setdefault(name, []).append(rms)
        allr = [r for _, r, _ in errs]
        mean = sum(allr) / len(allr)
        self.e_ref = max(sum(v) / len(v) for v in per.values())
        self.spread = (max(allr) - min(allr)) / mean if mean > 0 else 0.0
        self.m = 3.0 * self.spread
        self.rms_limit = self.e_ref * (1.0 + self.m)
        self.max_limit = 2.0 * max(e for _, _, e in errs)

    def line(self, name):
        lo, hi = min(r for _, r, _ in self.errs), max(r for _, r, _ in self.errs)
        return (f"MARGIN {name}: E_ref {self.e_ref:.3e} (16 runs {lo:.3e} .. {hi:.3e}), m {self.m:.3f}, rms limit {self.rms_limit:.3e}, "
                f"largest-element limit {self.max_limit:.3e}")


def dense_margin(run, seeds=SEEDS):
    """run(seed, fft) -> the error array of one f32 restatement against the float64 reference of the same data (already divided by
    whatever per-element scale the case applies) -> Margin over seeds x ORDERINGS"""
    errs = []
    for s in range(seeds):
        for name, fft in ORDERINGS:
            e = np.abs(run(s, fft))
            errs.append((name, _rms(e), float(e.max()) if e.size else 0.0))
    return Margin(errs)


# ------------------------------------------------------------------------------------------------------------------------------
# the FFT probe's cases
# ------------------------------------------------------------------------------------------------------------------------------
PROBE_LOG2N = list(range(2, 13))


def probe_dense(log2n, seed):
    """[POINTS >> log2n][N] complex64: every frame dense, frames of different scale"""
    N = 1 << log2n
    rng = np.random.default_rng(1000 * log2n + seed)
    fr = POINTS // N
    x = rng.standard_normal((fr, N)) + 1j * rng.standard_normal((fr, N))
    return (x * (0.25 + np.arange(fr)[:, None] % 4)).astype(C64)


@functools.lru_cache(maxsize=None)
def probe_margin(log2n, inverse):
    def run(seed, fft):
        x = probe_dense(log2n, seed)
        return fft(x, inverse) - fft64(x, inverse)
    return dense_margin(run)


def probe_structured(log2n):
    """{name: ([frames][N] complex64, exact expectation or None)}: one launch's frames all hold the same structured input at different
    scales (powers of two: the exact expectations scale with them)"""
    N = 1 << log2n
    fr = POINTS // N
    sc = (2.0 ** (np.arange(fr) % 5 - 2))[:, None]
    t = np.arange(N)
    out = {}
    imp0 = np.zeros((fr, N)); imp0[:, 0] = 1.0
    out["impulse0"] = ((imp0 * sc).astype(C64), (np.ones((fr, N)) * sc).astype(C64))
    const = np.ones((fr, N)) * sc
    dc = np.zeros((fr, N)); dc[:, 0] = N
    out["constant"] = (const.astype(C64), (dc * sc).astype(C64))
    imp1 = np.zeros((fr, N)); imp1[:, 1] = 1.0
    out["impulse1"] = ((imp1 * sc).astype(C64), None)
    out["alternating"] = ((np.where(t % 2, -1.0, 1.0)[None, :] * sc).astype(C64), None)
    kb = max(1, N // 8 + 1) % N
    out["tone"] = ((np.exp(2j * np.pi * kb * t / N)[None, :] * sc).astype(C64), None)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the frame pipeline in float32
# ------------------------------------------------------------------------------------------------------------------------------
def signal(seed, n, n_fft):
    """the denoiser tests' signal: noise and two tones, |x| <= 1, float32"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 37.3 * i / n_fft + 0.4) + 0.2 * np.sin(2 * np.pi * 120.0 * i / n_fft + 1.1)
    return np.clip(x, -1.0, 1.0).astype(F32)


def frames32(x, n_fft, hop, wl):
    """-> [F][n_fft] float32: win[t] * x[reflect(f hop - pad + t)] as the frames kernels load it"""
    x = np.asarray(x, F32)
    pad, F = D.geometry(len(x), n_fft, hop)
    s = np.arange(n_fft)[None, :] + hop * np.arange(F)[:, None] - pad
    s = np.where(s < 0, -s, s)
    s = np.where(s >= len(x), 2 * (len(x) - 1) - s, s)
    s = np.clip(s, 0, len(x) - 1)
    return D.window(n_fft, wl).astype(F32)[None, :] * x[s]


PIPE_MUTATIONS = ["conjugate_mirror_missing", "dc_nyquist_imag_kept", "inv_n_missing"]
# Equivalent by construction: the pipeline reads the REAL plane of the inverse transform only, and an imaginary part b at DC (Nyquist)
# of an otherwise conjugate-symmetric spectrum adds i b / N (i b (-1)^t / N) to the output, which is purely imaginary; for real frames b
# is zero besides.  The kernels' `im = 0` there cannot be observed through any entry point; test_spectral_reference states this.
EQUIVALENT = {"dc_nyquist_imag_kept"}


def pipeline32(x, n_fft, hop, wl, gain, fft, mut=None):
    """one whole row in f32: gain(Xh [F][nf] complex64) -> G [F][nf] float32 -> the output row, float32"""
    x = np.asarray(x, F32)
    n, nf = len(x), n_fft // 2 + 1
    pad, F = D.geometry(n, n_fft, hop)
    w32 = D.window(n_fft, wl).astype(F32)
    X = fft(frames32(x, n_fft, hop, wl).astype(C64), False)
    Xh = X[:, :nf]
    G = np.asarray(gain(Xh), F32)
    Y = _c(Xh.real * G, Xh.imag * G)
    if mut != "dc_nyquist_imag_kept":
        Y.imag[:, 0] = 0
        Y.imag[:, nf - 1] = 0
    full = X.copy()
    full[:, :nf] = Y
    if mut != "conjugate_mirror_missing":
        full[:, nf:] = np.conj(Y[:, nf - 2:0:-1])
    y = fft(full, True).real.astype(F32)
    if mut != "inv_n_missing":
        y = y * F32(1.0 / n_fft)
    yw = w32[None, :] * y
    w2 = D.window(n_fft, wl) ** 2                            # the device's win2: double
    num, den = np.zeros(n + 2 * pad + n_fft, F32), np.zeros(n + 2 * pad + n_fft)
    for f in range(F):                                       # ascending f, f32 adds
        num[f * hop:f * hop + n_fft] += yw[f]
        den[f * hop:f * hop + n_fft] += w2
    num, den = num[pad:pad + n], den[pad:pad + n]
    cov = den >= D.den_threshold(n_fft, hop, wl)
    out = x.copy()
    out[cov] = num[cov] / den[cov].astype(F32)
    return out


def denoise_gain(bias, strength, floor):
    bias, s, fl = np.asarray(bias, F32), F32(strength), F32(floor)

    def gain(Xh):
        m = np.sqrt(Xh.real * Xh.real + Xh.imag * Xh.imag)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(m > 0, np.maximum(fl, F32(1.0) - s * bias[None, :] / m), fl).astype(F32)
    return gain


EMBED_MUTATIONS = ["k_lo_off_by_one", "band_edge_off_by_one", "gain_of_the_neighbouring_block", "g_up_g_dn_swapped"]


def embed_gain(key, p, n_fft, rate, mut=None, f_first=0):
    """the keyed gain table of frames f_first .. as k_watermark_frames forms it (p: depth_db, lo_hz, hi_hz, block_frames, band_bins,
    period_blocks)"""
    k_lo, J = W.bands(p["lo_hz"], p["hi_hz"], p["band_bins"], n_fft, rate)
    g_up, g_dn = W.gains(p["depth_db"])
    if mut == "g_up_g_dn_swapped":
        g_up, g_dn = g_dn, g_up
    sg = W.sign_table(key, p["period_blocks"], J)
    KB, TB, P = p["band_bins"], p["block_frames"], p["period_blocks"]
    lo = k_lo + (1 if mut == "k_lo_off_by_one" else 0)
    hi = k_lo + J * KB + (1 if mut == "band_edge_off_by_one" else 0)

    def gain(Xh):
        G = np.ones(Xh.shape, F32)
        ks = np.arange(lo, min(hi, Xh.shape[1]))
        j = np.minimum((ks - lo) // KB, J - 1)
        for f in range(Xh.shape[0]):
            c = ((f_first + f) // TB + (1 if mut == "gain_of_the_neighbouring_block" else 0)) % P
            G[f, ks] = np.where(sg[c, j] > 0, g_up, g_dn)
        return G
    return gain


def ola_scale(n, n_fft, hop, wl):
    """what test_parity_at_other_transform_sizes scales its limit by: a sample under fewer or smaller windows than the interior of a Hann
    at hop = n_fft / 4 sees the frames' round-off behind its own factor sum w / sum w^2"""
    return np.maximum(1.0, D.amplification(int(n), n_fft, hop, wl) / (4.0 / 3.0))


def row_lengths(n_fft, hop):
    return (D.min_samples(n_fft, hop), n_fft + 1, 4 * n_fft + 77)


WM_SMALL = dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=2, band_bins=2, period_blocks=2)
WM_DEFAULT = dict(W.DEFAULTS)
KEY = 0xC0FFEE1234567
RATE = 22050
GEOMETRIES = [(512, 256, 512), (2048, 256, 2048), (4096, 256, 4096), (256, 256, 128)]     # the C-ABI watermark cases
DENOISE_GEOMETRIES = [(4096, 256, 4096), (64, 16, 64)]


def case_rows(n_fft, hop, seed):
    """the rows of a C-ABI case for a data seed (seed 0: what the device runs)"""
    return [signal(7000 + 31 * n_fft + 1000 * seed + b, k, n_fft) for b, k in enumerate(row_lengths(n_fft, hop))]


def embed_margin_of(rows_of_seed, p, n_fft, hop, wl, rate=RATE, key=KEY):
    """(c) for an embed case: rows_of_seed(seed) -> rows; the error is divided by ola_scale, so the limit applies as limit x ola_scale"""
    def run(seed, fft):
        errs = []
        for r in rows_of_seed(seed):
            ref = W.embed(r, key, n_fft=n_fft, hop=hop, win_length=wl, rate=rate, **p)
            got = pipeline32(r, n_fft, hop, wl, embed_gain(key, p, n_fft, rate), fft)
            errs.append((got.astype(np.float64) - ref) / ola_scale(len(r), n_fft, hop, wl))
        return np.concatenate(errs)
    return dense_margin(run)


WM_MAX_BANDS = 512


def wm_params(n_fft, small):
    """the parameter set of a C-ABI case: the defaults, or blocks and periods of 2 with bands of 2 bins (3 at 4096 points, where 2 would
    give 719 bands and the entry points take 512)"""
    p = dict(WM_SMALL, band_bins=2 if n_fft <= 2048 else 3) if small else dict(WM_DEFAULT)
    assert 3 <= W.bands(p["lo_hz"], p["hi_hz"], p["band_bins"], n_fft, RATE)[1] <= WM_MAX_BANDS
    return p


@functools.lru_cache(maxsize=None)
def embed_margin(n_fft, hop, wl, small=False):
    return embed_margin_of(lambda s: case_rows(n_fft, hop, s), wm_params(n_fft, small), n_fft, hop, wl)


def denoise_bias_for(rows, n_fft, hop, wl, seed):
    rng = np.random.default_rng(99 + seed)
    med = np.median(np.concatenate([np.abs(D.analysis(r, n_fft, hop, wl)).ravel() for r in rows]))
    return (med * rng.uniform(0.5, 1.5, n_fft // 2 + 1)).astype(F32)


def denoise_margin_of(data_of_seed, strength, floor, n_fft, hop, wl):
    """(c) for a denoise case: data_of_seed(seed) -> (rows, bias)"""
    def run(seed, fft):
        rows, bias = data_of_seed(seed)
        errs = []
        for r in rows:
            ref = D.denoise(r, bias, F32(strength), F32(floor), n_fft, hop, wl)
            got = pipeline32(r, n_fft, hop, wl, denoise_gain(bias, strength, floor), fft)
            errs.append((got.astype(np.float64) - ref) / ola_scale(len(r), n_fft, hop, wl))
        return np.concatenate(errs)
    return dense_margin(run)


def denoise_case_data(n_fft, hop, wl, seed):
    rows = case_rows(n_fft, hop, seed)
    return rows, denoise_bias_for(rows, n_fft, hop, wl, seed)


@functools.lru_cache(maxsize=None)
def denoise_margin(n_fft, hop, wl, strength=2.0, floor=0.1):
    return denoise_margin_of(lambda s: denoise_case_data(n_fft, hop, wl, s), strength, floor, n_fft, hop, wl)


# ------------------------------------------------------------------------------------------------------------------------------
# (f) k_wm_bands: cases, the kernel's order in f32, the interval tolerance
# ------------------------------------------------------------------------------------------------------------------------------
def _len_for(F, n_fft, hop):
    """the shortest row of F frames"""
    pad = (n_fft - hop) // 2
    return max(D.min_samples(n_fft, hop), (F - 1) * hop + n_fft - 2 * pad)


def _bc(name, n_fft, hop, k_lo, KB, J, Fs, why):
    return dict(name=name, n_fft=n_fft, hop=hop, k_lo=k_lo, KB=KB, J=J, Fs=Fs, why=why)


# Fs: frames of each row ("min": the shortest valid row; "silent": zeros, 3 frames); per = POINTS / n_fft frames per workgroup
BANDS_CASES = [
    _bc("n8_j4_nopad", 8, 8, 0, 1, 4, [513, 511, "min", "silent"], "per = 512, per J = 2048 (the whole of slb), hop = n_fft: no padding"),
    _bc("n8_j3_quarter", 8, 2, 1, 1, 3, [600, "min", "silent"], "J = 3, KB = 1, hop = n_fft / 4"),
    _bc("n256_j128", 256, 64, 0, 1, 128, [15, 16, 17, "silent"], "per J = 16 x 128 = 2048; F on both sides of 16"),
    _bc("n256_hop100", 256, 100, 5, 3, 20, [33, "min", "silent"], "a hop that divides nothing"),
    _bc("n512_nopad", 512, 512, 6, 4, 50, [7, 9, "min", "silent"], "odd log2 n; hop = n_fft; F on both sides of 8"),
    _bc("n1024_defaults", 1024, 256, 12, 4, 90, [3, 4, 5, "min", "silent"], "the shipped geometry and bands"),
    _bc("n2048_wide", 2048, 512, 1, 16, 60, [1, 2, 3, "silent"], "odd log2 n; a wide band (KB = 16); F on both sides of 2"),
    _bc("n4096_j512", 4096, 1024, 0, 4, 512, [1, 2, "silent"], "one frame per workgroup; the most bands (512), the last bin n_fft / 2 - 1"),
    _bc("n4096_hop300", 4096, 300, 2045, 1, 3, [3, "min"], "J = 3 at the top edge; a hop that divides nothing"),
]


def bands_rows(cs, seed):
    rows = []
    for i, F in enumerate(cs["Fs"]):
        if F == "silent":
            rows.append(np.zeros(_len_for(3, cs["n_fft"], cs["hop"]), F32))
        else:
            n = D.min_samples(cs["n_fft"], cs["hop"]) if F == "min" else _len_for(F, cs["n_fft"], cs["hop"]) + (i % 3)
            rows.append(signal(500 + 17 * i + 1000 * seed + cs["n_fft"], n, cs["n_fft"]))
    return rows


BANDS_MUTATIONS = ["contrast_without_half", "power_clamp_missing", "bands_k_lo_off_by_one"]


def bands32(x, cs, fft=fft_r4, mut=None):
    """k_wm_bands's order in f32 -> D [F][J - 2] float32"""
    X = fft(frames32(x, cs["n_fft"], cs["hop"], cs.get("wl", cs["n_fft"])).astype(C64), False)
    pw = X.real * X.real + X.imag * X.imag
    k_lo = cs["k_lo"] + (1 if mut == "bands_k_lo_off_by_one" else 0)
    with np.errstate(divide="ignore"):
        L = np.log2(pw if mut == "power_clamp_missing" else np.maximum(pw, F32(1e-6))).astype(F32)
    LB = np.zeros((X.shape[0], cs["J"]), F32)
    for u in range(cs["KB"]):                                # ascending bins
        LB += L[:, k_lo + u:k_lo + u + cs["J"] * cs["KB"]:cs["KB"]]
    h = F32(1.0 if mut == "contrast_without_half" else 0.5)
    with np.errstate(invalid="ignore"):
        return LB[:, 1:-1] - h * (LB[:, :-2] + LB[:, 2:])


def bands_ref(x, cs):
    """watermark_ref.band_contrast at the case's bands (rate = n_fft makes a bin one Hz)"""
    n = cs["n_fft"]
    Dm, J = W.band_contrast(x, lo_hz=float(cs["k_lo"]), hi_hz=float(cs["k_lo"] + cs["J"] * cs["KB"]), band_bins=cs["KB"], n_fft=n, hop=cs["hop"],
                            win_length=n, rate=n)
    assert J == cs["J"] and Dm.shape[1] == J - 2, (J, cs["J"])
    return Dm


@functools.lru_cache(maxsize=None)
def _bands_delta(name):
    cs = bands_case(name)

    def run(seed, fft):
        errs = []
        for r in bands_rows(cs, seed):
            fr = frames32(r, cs["n_fft"], cs["hop"], cs["n_fft"])
            errs.append(np.abs(fft(fr.astype(C64), False) - np.fft.fft(fr.astype(np.float64), axis=1)).ravel())
        return np.concatenate(errs)
    return dense_margin(run)


def bands_case(name):
    return next(c for c in BANDS_CASES if c["name"] == name)


def bands_tolerance(x, cs):
    """(f) -> (D_ref [F][J - 2], tol [F][J - 2]) for one row of the case"""
    delta = _bands_delta(cs["name"]).max_limit
    n, KB, J, k_lo = cs["n_fft"], cs["KB"], cs["J"], cs["k_lo"]
    fr = frames32(x, n, cs["hop"], n).astype(np.float64)     # the device multiplies win and x in f32: the frames ARE these values
    A = np.abs(np.fft.rfft(fr, axis=1))[:, k_lo:k_lo + J * KB]
    lg = lambda a: np.log2(np.maximum(a * a, 1e-6))          # noqa: E731
    mid, lo, hi = lg(A), lg(np.maximum(A - delta, 0.0)), lg(A + delta)
    pw_round = 3 * U / math.log(2.0) * 1.01                  # re re + im im: three roundings, relative 3 u, through log2
    term_w = np.maximum(hi - mid, mid - lo) + pw_round + K_ULP["log"] * ulp32(np.maximum(np.abs(lo), np.abs(hi)))
    absmax = np.maximum(np.abs(lo), np.abs(hi)) + term_w
    sh = (A.shape[0], J, KB)
    wband = term_w.reshape(sh).sum(axis=2) + 2 * KB * U * absmax.reshape(sh).sum(axis=2)
    LB = mid.reshape(sh).sum(axis=2)
    ref = LB[:, 1:-1] - 0.5 * (LB[:, :-2] + LB[:, 2:])
    mags = np.abs(LB) + wband
    tol = wband[:, 1:-1] + 0.5 * (wband[:, :-2] + wband[:, 2:]) + 4 * U * (mags[:, 1:-1] + mags[:, :-2] + mags[:, 2:])
    silent = ~fr.any(axis=1)                                 # exact zeros in, exact zeros out: D is exactly 0
    tol[silent] = 0.0
    assert not ref[silent].any()
    return ref, tol


# ------------------------------------------------------------------------------------------------------------------------------
# (e) k_wm_search: exact data, the definition's (v, dd), the kernel's structure with its mutations
# ------------------------------------------------------------------------------------------------------------------------------
def _sc(name, P, TB, JD, Fs, WF, why, **kw):
    JC = min(JD, WM_TABLE // P)
    return dict(name=name, P=P, TB=TB, JD=JD, J=JD + 2, Fs=Fs, WF=WF, why=why, chunks=-(-JD // JC), **kw)


SEARCH_CASES = [
    _sc("baseline", 2, 2, 4, [1, 3, 5, 13], 0, "smallest working set; F = 1, just under / over one period (4 frames), three periods + 1"),
    _sc("baseline_wf2", 2, 2, 4, [13, 2, 1, 3], 2, "WF = 2 (stride 1): rows of 12, 1, 1, 2 windows"),
    _sc("baseline_wf5", 2, 2, 4, [12, 5, 4, 13], 5, "an odd WF (stride 2): a clipped last window, WF >= F, an unclipped last window"),
    _sc("defaults", 64, 8, 88, [300, 5, 1], 0, "the shipped parameters; F below TB"),
    _sc("defaults_wf128", 64, 8, 88, [300, 128, 129], 128, "four windows, the last clipped to 108 frames; WF = F; F = WF + 1"),
    _sc("two_chunks", 256, 8, 88, [200, 7], 0, "chunked: 48 + 40 bands"),
    _sc("eleven_chunks", 256, 2, 510, [64, 3], 0, "chunked: 10 x 48 + 30 bands, J = 512"),
    _sc("uneven_slices", 100, 3, 130, [301, 299, 2], 0, "P does not divide 256 (56 idle threads, slices of 50); chunked: 122 + 8; around one period (300)"),
    _sc("uneven_wf101", 100, 3, 130, [301, 150], 101, "chunked with an odd WF: five windows, the last clipped"),
    _sc("one_part", 129, 1, 5, [130, 128, 1], 0, "P > 128: nparts = 1; TB = 1"),
    _sc("mostly_empty", 3, 5, 7, [1, 4, 14, 16, 47], 0, "P = 3: most slices empty; around one period (15)"),
    _sc("mostly_empty_wf7", 3, 5, 7, [47, 7, 10], 7, "odd WF = 7 (stride 3)"),
    _sc("p1", 1, 4, 1, [1, 3, 5, 9], 0, "P = 1 and JD = 1"),
    _sc("p1_wf2", 1, 4, 1, [9, 2], 2, "P = 1 with windows"),
    _sc("nan_row", 2, 2, 4, [13, 9, 13], 0, "row 1 holds NaN: score 0, offset 0; the others keep their bits", nan_row=1),
    _sc("zero_row", 3, 5, 7, [14, 20], 0, "row 0 is all zero: den = 0, score 0, offset 0", zero_row=0),
    _sc("tie_shifts", 4, 2, 4, [9, 16], 0, "sign rows 0 and 2 equal, 1 and 3 equal: shifts s and s + 2 tie", tie="shifts"),
    _sc("tie_phases", 4, 3, 4, [7, 11], 0, "one nonzero frame: the phases that keep it in the same block tie", tie="phases"),
    _sc("tie_chunked", 256, 2, 510, [40], 0, "all sign rows equal: every shift ties, through eleven chunks", tie="all"),
]


def search_case(name):
    return next(c for c in SEARCH_CASES if c["name"] == name)


def search_data(cs):
    """-> (rows: list of D [F][JD] float64 on the grid 2^-3, sign [P][J] int8)"""
    rng = np.random.default_rng(sum(map(ord, cs["name"])))
    P, J, JD = cs["P"], cs["J"], cs["JD"]
    sg = W.sign_table(KEY + P, P, J).astype(np.int8)
    tie = cs.get("tie")
    if tie == "shifts":
        sg[2:] = sg[:2]
    elif tie == "all":
        sg[:] = sg[0]
    rows = []
    for b, F in enumerate(cs["Fs"]):
        d = rng.integers(-8, 9, (F, JD)) / 8.0
        if tie == "phases":
            keep = d[F // 2].copy()
            d[:] = 0.0
            d[F // 2] = np.where(keep == 0, 0.5, keep)
        if cs.get("zero_row") == b:
            d[:] = 0.0
        if cs.get("nan_row") == b:
            d[F // 2, JD // 2] = np.nan
        rows.append(d)
    return rows, sg


def search_premise(rows):
    """every f32 partial sum of e and t is exact: each column of D on one grid with sum|.| below 2^24 steps (NaN rows aside)"""
    return all(exact_sum(d[:, j]) for d in rows if not np.isnan(d).any() for j in range(d.shape[1]))


def definition_v_dd(Dm, sg, fa, fb, TB, P):
    """(v [P TB], dd [P TB]) of the window [fa, fb) straight from the definition, exact in float64 on exact data"""
    S = sg[:, 1:-1].astype(np.float64)
    v, dd = np.zeros(P * TB), np.zeros(P * TB)
    f = np.arange(fa, fb)
    for o in range(P * TB):
        m = (f + o) // TB
        E = np.zeros((m[-1] - m[0] + 1, Dm.shape[1]))
        np.add.at(E, m - m[0], Dm[fa:fb])
        dd[o] = (E * E).sum()
        v[o] = (S[np.arange(m[0], m[-1] + 1) % P] * E).sum()
    return v, dd


def search_ref(cs):
    """per row, per window: (z_best float64, offset, ties) from watermark_ref.window_scores; ties: how many offsets attain z_best.  The
    premises of (e) are asserted here, on the host: the maximum is attained only by identical (v, dd) pairs and leads every other
    value by more than 64 ulp of double"""
    rows, sg = search_data(cs)
    out = []
    for d in rows:
        per = []
        for fa, fb in W.windows(d.shape[0], cs["WF"]):
            if np.isnan(d[fa:fb]).any():
                per.append((0.0, 0, 0))
                continue
            z = W.window_scores(d, sg.astype(np.int64), fa, fb, cs["TB"], cs["P"])
            v, dd = definition_v_dd(d, sg, fa, fb, cs["TB"], cs["P"])
            with np.errstate(divide="ignore", invalid="ignore"):
                z2 = np.where(dd > 0, v / np.sqrt(dd), 0.0)
            assert np.array_equal(z, z2), (cs["name"], "window_scores and the definition's (v, dd) disagree on exact data")
            o = int(np.argmax(z))
            top = z == z[o]
            assert np.all(v[top] == v[o]) and np.all(dd[top] == dd[o]), (cs["name"], "a tie of different (v, dd) pairs")
            rest = z[~top]
            assert rest.size == 0 or z[o] - rest.max() > 64 * np.spacing(abs(z[o])), (cs["name"], "a near tie")
            per.append((float(z[o]), o, int(top.sum())))
        out.append(per)
    return out


SEARCH_MUTATIONS = ["phase_off_by_one", "window_stride_rounded_up", "last_window_not_clipped", "den_from_the_folded_table",
                    "sign_row_not_wrapped", "column_against_band_without_plus_1", "tie_to_the_larger_offset", "chunk_last_band_dropped"]


def search_model(cs, mut=None):
    """k_wm_search's structure in NumPy (fold by m mod P, chunks of JC bands, shift pass, smallest offset among equals) on the case's
    data -> per row a list of (score float32, offset); e, t in f32, num, den in double"""
    rows, sg = search_data(cs)
    P, TB, JD, WF = cs["P"], cs["TB"], cs["JD"], cs["WF"]
    JC = min(JD, WM_TABLE // P)
    out = []
    for d in rows:
        F = d.shape[0]
        d32 = np.vstack([d.astype(F32), np.ones((WF + 1, JD), F32)])          # (what an unclipped window would read behind the row)
        H = ((WF + 1) // 2 if mut == "window_stride_rounded_up" else WF // 2) if WF > 0 else 0
        nw = 0 if F <= 0 else (1 if WF <= 0 or F <= WF else 1 + -(-(F - WF) // H))
        per = []
        for w in range(nw):
            fa = w * H if WF > 0 else 0
            fb = (fa + WF if mut == "last_window_not_clipped" else min(fa + WF, F)) if WF > 0 else F
            f = np.arange(fa, fb)
            zs = np.zeros((TB, P))
            for ph in range(TB):
                m = (f + ph + (1 if mut == "phase_off_by_one" else 0)) // TB
                E = np.zeros((m[-1] - m[0] + 1, JD), F32)
                np.add.at(E, m - m[0], d32[fa:fb])
                T = np.zeros((P, JD), F32)
                np.add.at(T, np.arange(m[0], m[-1] + 1) % P, E)
                den = float((T.astype(np.float64) ** 2).sum()) if mut == "den_from_the_folded_table" else float((E.astype(np.float64) ** 2).sum())
                num = np.zeros(P)
                for j0 in range(0, JD, JC):
                    jc = min(JC, JD - j0)
                    use = jc - 1 if (mut == "chunk_last_band_dropped" and JD > JC) else jc
                    col = j0 + (0 if mut == "column_against_band_without_plus_1" else 1)
                    Tc = T[:, j0:j0 + use].astype(np.float64)
                    for s in range(P):
                        r = np.arange(P) + s
                        r = np.minimum(r, P - 1) if mut == "sign_row_not_wrapped" else r % P
                        num[s] += float((sg[r, col:col + use] * Tc).sum())
                with np.errstate(invalid="ignore"):
                    zs[ph] = num / math.sqrt(den) if den > 0 else (np.nan if den != den else 0.0)
            if np.isnan(zs).any():
                per.append((F32(0.0), 0))
                continue
            o_of = np.arange(TB)[:, None] + TB * np.arange(P)[None, :]
            top = zs == zs.max()
            o = int(o_of[top].max() if mut == "tie_to_the_larger_offset" else o_of[top].min())
            per.append((F32(zs.max()), o))
        out.append(per)
    return out


def scores32(d32, sg, fa, fb, TB, P):
    """z [P TB] of the window [fa, fb) in the kernel's order on dense data: e and t in f32 (ascending frames, ascending blocks), num
    and den in double"""
    S_ = sg[:, 1:-1].astype(np.float64)
    f = np.arange(fa, fb)
    z = np.zeros(P * TB)
    for ph in range(TB):
        m = (f + ph) // TB
        E = np.zeros((m[-1] - m[0] + 1, d32.shape[1]), F32)
        np.add.at(E, m - m[0], d32[fa:fb])
        T = np.zeros((P, d32.shape[1]), F32)
        np.add.at(T, np.arange(m[0], m[-1] + 1) % P, E)
        den = float((E.astype(np.float64) ** 2).sum())
        if den > 0:
            M = S_ @ T.astype(np.float64).T                  # M[r][c] = sign row r . table row c
            c = np.arange(P)
            z[ph + TB * np.arange(P)] = np.array([M[(c + s) % P, c].sum() for s in range(P)]) / math.sqrt(den)
    return z


def detect32(x, key, p, n_fft, hop, wl, rate, wf, fft):
    """the detector's two launches in f32 on one row -> the z array of every window (float64 holding what the kernel rounds to f32)"""
    k_lo, J = W.bands(p["lo_hz"], p["hi_hz"], p["band_bins"], n_fft, rate)
    d32 = bands32(x, dict(n_fft=n_fft, hop=hop, wl=wl, k_lo=k_lo, KB=p["band_bins"], J=J), fft)
    sg = W.sign_table(key, p["period_blocks"], J)
    return [scores32(d32, sg, fa, fb, p["block_frames"], p["period_blocks"]) for fa, fb in W.windows(d32.shape[0], wf)]


def detect_margin_of(rows_of_seed, p, n_fft, hop, wl, wfs, rate=RATE, key=KEY):
    """(c) for a detector case: rows_of_seed(seed) -> the rows to detect on; the elements are the z of every offset of every window of
    every row, for each window_frames of wfs"""
    kw = {k: v for k, v in p.items() if k != "depth_db"}
    memo = {}                                                # the rows and their float64 z are the same for both orderings

    def run(seed, fft):
        if seed not in memo:
            rows = rows_of_seed(seed)
            memo[seed] = (rows, [[W.detect(r, key, window_frames=wf, n_fft=n_fft, hop=hop, win_length=wl, rate=rate, full=True, **kw)[3] for wf in wfs]
                                 for r in rows])
        errs = []
        for r, ref in zip(*memo[seed]):
            for wf, zs in zip(wfs, ref):
                errs += [a - b for a, b in zip(detect32(r, key, p, n_fft, hop, wl, rate, wf, fft), zs)]
        return np.concatenate(errs)
    return dense_margin(run)


WM_P256 = dict(W.DEFAULTS, block_frames=2, period_blocks=256)       # the chunked search behind the real band launch


def detect_rows(n_fft, hop, wl, seed, every=False):
    """the rows of the C-ABI case marked by the float64 reference and rounded to f32: the longest (4 n_fft + 77 samples), which the
    margin is taken on, or all three"""
    return [W.embed(r, KEY, n_fft=n_fft, hop=hop, win_length=wl, rate=RATE, **WM_P256).astype(F32)
            for r in case_rows(n_fft, hop, seed)[0 if every else 2:]]


def detect_wfs(n_fft, hop):
    F = D.geometry(row_lengths(n_fft, hop)[2], n_fft, hop)[1]
    return (0, max(2, F // 2))


@functools.lru_cache(maxsize=None)
def detect_margin(n_fft, hop, wl):
    return detect_margin_of(lambda s: detect_rows(n_fft, hop, wl, s), WM_P256, n_fft, hop, wl, detect_wfs(n_fft, hop))


def search_agrees(cs, got, ref=None):
    """(e) on `got` (per row a list of (score f32, offset)) -> None, or what disagrees"""
    ref = search_ref(cs) if ref is None else ref
    for b, (g, r) in enumerate(zip(got, ref)):
        if len(g) != len(r):
            return f"row {b}: {len(g)} windows, the reference has {len(r)}"
        for w, ((zs, o), (z, o_ref, _)) in enumerate(zip(g, r)):
            z32 = F32(z)
            near = (z32, np.nextafter(z32, F32(np.inf)), np.nextafter(z32, F32(-np.inf)))
            if not any(F32(zs) == q for q in near):
                return f"row {b} window {w}: score {float(zs)!r}, the reference {float(z32)!r}"
            if o != o_ref:
                return f"row {b} window {w}: offset {o}, the reference {o_ref}"
    return None
