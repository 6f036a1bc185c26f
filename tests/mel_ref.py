"""Float64 restatement of the log-mel front end (include/zvx.h, zvx_melspec) with a per-element bound, the table of STFT geometries
tests/test_mel_gpu.py runs on the device and tests/test_mel_reference.py checks on the host, and the rows of every case.

The reference is written from the header's definition, not from zerovox_amd/mels.py: reflect padding (n_fft - hop) // 2, frames
1 + (n + 2 pad - n_fft) // hop, the periodic Hann of win_length centred in n_fft, the real DFT, its magnitude, Slaney's mel basis,
log(max(., 1e-5)) (the clip is the f32 value of 1e-5, which is what a float argument of the header's call holds).  It takes the f32
signal converted to float64.  `design` builds the two constant matrices in float64, independently of the product; for the device
comparison `mel_ref` is given the f32 tensors pack_model emitted (`packed`), the kernel's own operands, so that the bound covers
arithmetic alone, and tests/test_mel_reference.py compares the two sets of matrices on the host.

The bound, per element, from the reference's own intermediates (u = 2^-24; nothing is measured on a device but K_ULP, which
tests/ops_ref.py measured once over the arguments of its own cases, profiles/ops_kernel_spec.txt):
  * each of the two GEMMs by the rule kernel_ref holds the f32 cases of the same launcher to (kernel_ref._epilogue / _store with no
    bias, alpha = out_scale = 1): an f32 sum of n terms in any order 2 n u sum|terms|, the epilogue 4 u |v|, half an ulp of f32 at
    |v| + the bound; n = n_fft for Re and Im, n = KP (the bins rounded up to 4) for the mel sum;
  * the magnitude as ops_ref's stft_mag case: |d mag| <= hypot(d re, d im), + (3 u + one sqrt of K_ULP ulps and a rounding) of the
    largest magnitude the kernel can hold, + half an ulp for the store;
  * the mel energy E = sum_f B[j][f] d mag[f] + the second GEMM's rule over the largest magnitudes the kernel can hold;
  * the log: m -> log(max(m, lo)) is Lipschitz with constant 1 / max(m_ref - E, lo) on [m_ref - E, inf), so
    |d| <= E / max(m_ref - E, lo) + K_ULP["log"] ulps of f32 at the result + half an ulp for the store (ops_ref's log_clip case).
A silent frame and an empty filter have m_ref = 0 exactly in any arithmetic (a sum of zeros), E = 0, and the device must hold
log(lo) to K_ULP["log"] ulps.  Padding rows and columns of the matrices are exact zeros and add nothing."""
import numpy as np

import kernel_ref as K
import ops_ref as R
from kernel_ref import DT_F32, U, half_ulp

LO = float(np.float32(1e-5))
LOG_LO = float(np.log(LO))
FIELDS = ("fft_size", "hop_size", "win_length", "num_mels", "sampling_rate", "fmin", "fmax")
# (fft_size, hop_size, win_length, num_mels, sampling_rate, fmin, fmax) and what the case walks
GEOMETRIES = {
    "default": (1024, 256, 1024, 80, 22050, 0, 8000),     # the shipped one
    "tiny": (64, 16, 64, 8, 22050, 0, 8000),              # fewest mels; KP = 36 is no multiple of the 16-element K step
    "no_pad": (256, 256, 128, 16, 22050, 0, 8000),        # hop = n_fft (pad 0); a centred window shorter than n_fft
    "many_mels": (512, 256, 512, 136, 22050, 0, 8000),    # more mels than the speaker encoder pools (8 x 16 taps): refused by name
    "empty_filters": (256, 64, 256, 128, 22050, 0, 8000),  # the most mels a model can have, narrower than a bin: empty filters, exact log(1e-5)
    "non_pow2": (400, 100, 400, 40, 16000, 20, 8000),     # n_fft no power of two; fmin > 0; fmax = Nyquist
    "odd_pad": (1024, 225, 900, 80, 22050, 0, 8000),      # (n_fft - hop) odd; hop % 4 != 0: frames start at 4-byte, not 16-byte boundaries
}
# a case that does not run: (the modelcfg.yaml field pack_model names, the manifest key zvx_create names, its status)
REFUSED = {"many_mels": ("num_mels", "n_mels", "UNSUPPORTED")}
RUNNING = [c for c in GEOMETRIES if c not in REFUSED]
# STFT blocks pack.check_model_config refuses: case -> (changes to the default audio block, the field named, the manifest edit that
# zvx_create refuses with the key it names, or None where the manifest carries no such key)
BAD_STFT = {
    "fft_not_mult_of_4": (dict(fft_size=1022, win_length=1022), "fft_size", ("fft_size", 1022, "fft_size")),
    "fft_below_4": (dict(fft_size=2, hop_size=1, win_length=2), "fft_size", ("fft_size", 2, "fft_size")),
    "hop_above_fft": (dict(fft_size=128, win_length=128), "hop_size", ("fft_size", 128, "hop")),
    "hop_zero": (dict(hop_size=0), "hop_size", None),
    "win_above_fft": (dict(win_length=1025), "win_length", None),
    "win_zero": (dict(win_length=0), "win_length", None),
    "fmin_negative": (dict(fmin=-1), "fmin", None),
    "fmin_at_fmax": (dict(fmin=8000), "fmin", None),
    "fmax_above_nyquist": (dict(fmax=11026), "fmax", None),
}


def geom(case):
    return dict(zip(FIELDS, GEOMETRIES[case]))


def pad_of(g):
    return (g["fft_size"] - g["hop_size"]) // 2


def frames_of(n, g):
    return 1 + (n + 2 * pad_of(g) - g["fft_size"]) // g["hop_size"]


def min_len(g):
    """the shortest legal row: a mirror on both sides (reflect padding needs pad + 1 samples) and one whole frame"""
    return max(pad_of(g) + 1, g["fft_size"] - 2 * pad_of(g))


def dims(g):
    """(nf bins, NR rows of mel.dft, KP columns of mel.basis)"""
    nf = g["fft_size"] // 2 + 1
    return nf, (2 * nf + 3) // 4 * 4, (nf + 3) // 4 * 4


# ---- the independent float64 design --------------------------------------------------------------------------------------------------
def window(g):
    """periodic Hann of win_length samples, centred in n_fft (the left gap is the smaller one)"""
    n_fft, wl = g["fft_size"], g["win_length"]
    w = np.zeros(n_fft)
    lp = (n_fft - wl) // 2
    w[lp:lp + wl] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(wl) / wl)
    return w


def slaney_hz(mel):
    mel = np.asarray(mel, np.float64)
    return np.where(mel < 15.0, mel * 200.0 / 3.0, 1000.0 * np.exp((mel - 15.0) * np.log(6.4) / 27.0))


def slaney_mel(hz):
    hz = np.asarray(hz, np.float64)
    return np.where(hz < 1000.0, hz * 3.0 / 200.0, 15.0 + np.log(np.maximum(hz, 1.0) / 1000.0) * 27.0 / np.log(6.4))


def design(g):
    """-> (dft [NR][n_fft], basis [num_mels][KP]) in float64: rows f < nf of dft are window(t) cos(2 pi f t / n_fft), rows nf + f are
    -window(t) sin(.), the angle reduced over the integers before it is scaled; basis row j is the triangle over the mel-spaced
    corners c[j] < c[j + 1] < c[j + 2] of height 2 / (c[j + 2] - c[j]) sampled at the bins k sampling_rate / n_fft.  Everything else
    (the padding rows and columns) is zero."""
    n_fft, nm, sr = g["fft_size"], g["num_mels"], g["sampling_rate"]
    nf, NR, KP = dims(g)
    ang = 2.0 * np.pi * ((np.arange(nf)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    dft = np.zeros((NR, n_fft))
    dft[:nf] = np.cos(ang) * window(g)[None, :]
    dft[nf:2 * nf] = -np.sin(ang) * window(g)[None, :]
    c = slaney_hz(np.linspace(slaney_mel(g["fmin"]), slaney_mel(g["fmax"]), nm + 2))
    hz = np.arange(nf) * (sr / n_fft)
    basis = np.zeros((nm, KP))
    for j in range(nm):
        up = (hz - c[j]) / (c[j + 1] - c[j])
        down = (c[j + 2] - hz) / (c[j + 2] - c[j + 1])
        basis[j, :nf] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (c[j + 2] - c[j])
    return dft, basis


_packed = {}


def packed(case):
    """(mel.dft [NR][n_fft], mel.basis [num_mels][KP]) as float32: the tensors pack_model emits for the case's context (the one
    test_spectral_gpu.ctx_at builds: reduced model, tiny vocoder, weights seed 0), read back out of the blob"""
    if case not in _packed:
        import test_spectral_gpu as TS
        g = geom(case)
        man, blob = TS.packed_at(g["fft_size"], g["hop_size"], g["win_length"], **{k: g[k] for k in FIELDS[3:]})
        out = {}
        for line in man.splitlines():
            p = line.split()
            if p[:1] == ["tensor"] and p[1] in ("mel.dft", "mel.basis"):
                shape = [int(d) for d in p[4:4 + int(p[3])]]
                off = int(p[4 + int(p[3])])
                out[p[1]] = blob[off:off + int(np.prod(shape))].reshape(shape)[0].copy()
        assert f"cfg fft_size {g['fft_size']}\n" in man and f"cfg hop {g['hop_size']}\n" in man
        _packed[case] = (out["mel.dft"], out["mel.basis"])
    return _packed[case]


# ---- the reference and its bound -----------------------------------------------------------------------------------------------------
def reflect(x, p):
    """numpy's 'reflect': the mirror without the edge sample"""
    x = np.asarray(x)
    return np.concatenate([x[1:p + 1][::-1], x, x[len(x) - p - 1:len(x) - 1][::-1]]) if p else x.copy()


def gemm_rule(v, mag, n):
    """kernel_ref's bound of an f32 GEMM output without bias or scales: accumulation, epilogue, the f32 store"""
    e = 2 * n * U * mag + 4 * U * np.abs(v)
    return e + half_ulp(np.abs(v) + e, DT_F32)


def mel_ref(x, g, dft=None, basis=None, mut=None):
    """One row: the f32 signal x -> (log-mel [frames][num_mels] float64, bound [frames][num_mels], mel energy [frames][num_mels]).
    dft / basis: the two matrices (default: the float64 design).  mut: one of MUTATIONS, applied to the reference."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n_fft, hop = g["fft_size"], g["hop_size"]
    nf, NR, KP = dims(g)
    if dft is None:
        dft, basis = design(g)
    dft, basis = np.asarray(dft, np.float64), np.asarray(basis, np.float64)
    if mut == "window_shift":
        dft = np.roll(dft, 1, axis=1)
    if mut == "drop_last_bin":
        basis = basis.copy()
        j = basis.shape[0] // 2
        basis[j, np.flatnonzero(basis[j])[-1]] = 0.0
    p = pad_of(g) if mut != "ceil_pad" else -((hop - n_fft) // 2)
    assert len(x) >= min_len(g), (len(x), min_len(g))
    xp = reflect(x, p)
    fr = 1 + (len(xp) - n_fft) // hop
    F = xp[np.arange(fr)[:, None] * hop + np.arange(n_fft)[None, :]]
    S, A = F @ dft.T, np.abs(F) @ np.abs(dft).T
    eS = gemm_rule(S, A, n_fft)
    re, im, ere, eim = S[:, :nf], S[:, nf:2 * nf], eS[:, :nf], eS[:, nf:2 * nf]
    m = np.hypot(re, im)
    em = np.hypot(ere, eim)
    em = em + (m + em) * (3 * U + R.rel("sqrt"))
    em = em + half_ulp(m + em, DT_F32)
    Bf = basis[:, :nf]
    M = m @ Bf.T
    E = em @ np.abs(Bf).T + gemm_rule(M, (m + em) @ np.abs(Bf).T, KP)
    E = np.where(M == 0.0, 0.0, E)                              # a sum of exact zeros is exact in any arithmetic
    v = np.log(np.maximum(M, LO))
    d = E / np.maximum(M - E, LO)
    bound = d + R.K_ULP["log"] * R.ulp32(np.abs(v) + d) + half_ulp(np.abs(v) + d, DT_F32)
    return v, bound, M


MUTATIONS = ["window_shift", "drop_last_bin", "ceil_pad"]


# ---- the rows of a case --------------------------------------------------------------------------------------------------------------
ROW_NAMES = ("shortest", "shortest+1", "boundary-1", "boundary", "boundary+1", "tone+noise", "zeros", "quiet", "at_clip")
_rows = {}


def case_rows(case):
    """The ragged batch of a case, computed once and left unchanged: the shortest legal length and one more; the lengths one below, at
    and one above a frame boundary; three dozen frames of two tones in noise; a row of zeros; noise at 1e-4 (values near the clip, or
    all under it where n_fft is small); noise scaled, by the float64 design alone, so that its median mel energy is the clip.
    -> list of float32 rows in ROW_NAMES' order"""
    if case not in _rows:
        g = geom(case)
        n_fft, hop, sr = g["fft_size"], g["hop_size"], g["sampling_rate"]
        rng = np.random.default_rng(sum(GEOMETRIES[case]))
        lo, edge = min_len(g), n_fft - 2 * pad_of(g) + 3 * hop   # edge: the first length of 4 frames
        assert edge - 1 >= lo and frames_of(edge - 1, g) == 3 and frames_of(edge, g) == 4 == frames_of(edge + 1, g)

        def sound(n, amp):
            t = np.arange(n) / sr
            return amp * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t) + 0.05 * rng.standard_normal(n))
        rows = [sound(n, 1.0) for n in (lo, lo + 1, edge - 1, edge, edge + 1, edge + 33 * hop + 7)]
        rows.append(np.zeros(edge + hop + 3))
        rows.append(1e-4 * rng.standard_normal(edge + 5 * hop + 1))
        noise = rng.standard_normal(edge + 4 * hop + 2)
        rows.append(noise * (LO / np.median(mel_ref(noise, g)[2])))             # (the energy is homogeneous in the signal)
        _rows[case] = [r.astype(np.float32) for r in rows]
    return _rows[case]


def batch(rows):
    """-> (x [B][odd Nmax] float32 with NaN behind every row's end, n [B] int32)"""
    n = np.array([len(r) for r in rows], np.int32)
    nmax = int(n.max())
    x = np.full((len(rows), nmax + (nmax % 2 == 0)), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


_refs = {}


def case_ref(case):
    """per row (value, bound, energy) against the packed operands, computed once and shared"""
    if case not in _refs:
        dft, basis = packed(case)
        _refs[case] = [mel_ref(r, geom(case), dft, basis) for r in case_rows(case)]
    return _refs[case]
