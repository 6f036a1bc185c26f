"""float64 / NumPy / SciPy reference of zvx_loudness and zvx_normalize as include/zvx.h states them: scipy.signal.lfilter in double, every
gate decided in the power domain.  Imports nothing from zerovox_amd."""
import numpy as np
from scipy.signal import lfilter

ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
AMBIGUOUS_LU = 1e-3              # a block whose z lies within this of either gate may be decided either way (include/zvx.h)


def coefficients(fs):
    """-> ((b, a) of the high shelf, (b, a) of the high pass), float64"""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs); Vh = 10.0 ** (G / 20.0); Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return (b1, a1), (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))


def unit_len(fs):
    return (int(fs) + 5) // 10


def blocks(x, fs):
    """z[j], j = 0 .. U - 4: the mean K-weighted power of the 400 ms blocks at a 100 ms step (empty where the row is shorter than one)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = unit_len(fs)
    U = len(x) // h
    if U < 4:
        return np.zeros(0, np.float64)
    s1, s2 = coefficients(fs)
    y = lfilter(*s2, lfilter(*s1, x))
    u = (y[:U * h].reshape(U, h) ** 2).sum(axis=1)
    return (u[:-3] + u[1:-2] + u[2:-1] + u[3:]) / (4 * h)


def _lu(a, b):
    with np.errstate(divide="ignore"):
        return np.abs(10.0 * np.log10(a / b))


def gated(z):
    """both gates over the blocks z -> (L, margin, n_abs_removed, n_rel_removed): L = -inf without a block above the absolute gate; margin =
    the smallest distance in LU of any block to either gate (inf where nothing is compared)"""
    if len(z) == 0:
        return -np.inf, np.inf, 0, 0
    margin = float(np.min(_lu(z, ABS_GATE)))
    g = z[z > ABS_GATE]
    if len(g) == 0:
        return -np.inf, margin, len(z), 0
    thr = 0.1 * g.mean()
    margin = min(margin, float(np.min(_lu(g, thr))))
    k = g[g > thr]
    return float(-0.691 + 10.0 * np.log10(k.mean())), margin, len(z) - len(g), len(g) - len(k)


def gain_ref(L, peak, target, peak_ceiling, max_gain_db):
    """-> (g as float64, what bounded it: None, "max_gain" or "ceiling")"""
    if not np.isfinite(L) or not peak > 0:
        return 1.0, None
    target, peak_ceiling, max_gain_db = float(np.float32(target)), float(np.float32(peak_ceiling)), float(np.float32(max_gain_db))
    g, lim = 10.0 ** ((target - L) / 20.0), None
    gmax = 10.0 ** (max_gain_db / 20.0)
    if gmax < g:
        g, lim = gmax, "max_gain"
    if peak_ceiling > 0 and float(peak) * g > peak_ceiling:
        g, lim = peak_ceiling / float(peak), "ceiling"
    return g, lim


def measure(rows, fs):
    """-> dict: lufs [B] float64, peak [B] float32, margin [B] (LU), removed [B] (abs, rel) and the pooled case: lufs_common, peak_common,
    margin_common, removed_common"""
    zs = [blocks(r, fs) for r in rows]
    per = [gated(z) for z in zs]
    peak = np.array([np.abs(np.asarray(r, np.float32)).max() if len(r) else 0.0 for r in rows], np.float32)
    pooled = gated(np.concatenate(zs) if zs else np.zeros(0))
    return dict(lufs=np.array([p[0] for p in per], np.float64), peak=peak, margin=np.array([p[1] for p in per]),
                removed=[(p[2], p[3]) for p in per], lufs_common=pooled[0], peak_common=np.float32(peak.max() if len(peak) else 0.0),
                margin_common=pooled[1], removed_common=(pooled[2], pooled[3]))


def gains(m, target, peak_ceiling=0.891, max_gain_db=20.0, common=False):
    """from measure()'s dict -> (gain [B] float32, limits [B])"""
    B = len(m["lufs"])
    if common:
        g, lim = gain_ref(m["lufs_common"], m["peak_common"], target, peak_ceiling, max_gain_db)
        return np.full(B, np.float32(g), np.float32), [lim] * B
    pairs = [gain_ref(m["lufs"][b], m["peak"][b], target, peak_ceiling, max_gain_db) for b in range(B)]
    return np.array([np.float32(p[0]) for p in pairs], np.float32), [p[1] for p in pairs]


def pcm16(v):
    """(int16) trunc(clamp(v * 32760, -32768, 32767)) with the product in f32"""
    v = np.asarray(v, np.float32) * np.float32(32760.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


def extra_rows(fs):
    """rows around the one-block threshold (4h - 1, 4h, 5h - 1, 5h samples of noise at 0.05) and the warm-up probe: 4 s of noise at -50 dBFS
    with a 0.5 DC offset over its first half and one -1.5 spike -- a truncated warm-up or lost filter state shows in every unit of the
    first half, where a recurrence restarted from zero sees a step the signal does not have.  The spike sits half a unit behind the end of
    the offset, so that the two share their blocks: spread over eight blocks instead they put the relative gate of the 22050 Hz row onto
    its noise floor (-47.06 LUFS both), which no row of a test may be (the ambiguity band of include/zvx.h)."""
    rng = np.random.default_rng(1000)
    h = unit_len(fs)
    rows = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (4 * h - 1, 4 * h, 5 * h - 1, 5 * h)]
    n = 4 * int(fs)
    x = (10.0 ** (-50.0 / 20.0) * rng.standard_normal(n)).astype(np.float32)
    x[:n // 2] += np.float32(0.5)
    x[n // 2 + h // 2] = np.float32(-1.5)
    rows.append(x)
    return rows
