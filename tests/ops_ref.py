"""Float64 restatement of the contracts of the small kernels of zerovox_amd/csrc/ops.hip (the "Small kernels" section of
zvx_kernels.h), the cases tests/test_ops_gpu.py runs through the shim entry points zvxk_<name>, and the mutations
tests/test_ops_reference.py holds the bounds to.

A case holds its buffers as raw bits.  Inputs are rounded to the type the kernel reads before the reference sees them; every input
row / column the contract masks holds NaN; every output buffer starts as the sentinel (all ones: a NaN for the float types, -1 for
the integers), in-place buffers start as their input.  ref(mut) returns, per output buffer, (ref, tol, mask) over the whole buffer:
elements inside the mask must lie within tol of ref (tol 0: the bits of ref), everything else must keep its bits, except where the
case's `may` mask says the contract leaves the value open.

Tolerances, all derived from the data of the case (u = 2^-24):
  * data movement, integers, and every result that is ONE correctly rounded IEEE operation followed by a cast (embed's add,
    bucket_embed_add's add, add_pe_cast): tol 0, bit equality;
  * element-wise f32 chains: 2^-22 x the sum of the magnitudes the chain adds, + half an ulp of the output type at |ref| + that bound;
  * an f32 sum of n terms: 2 n u sum|terms| in any order (0 where every partial sum is exact: all terms on one power-of-two grid and
    sum|terms| below 2^24 grid steps), propagated to first order through the formula the kernel executes.  The variances formed as a
    difference (colstats / instnorm_fused: a2/cnt - m1^2 about the first valid row; asp_pool: sxx/s - mu^2) carry the error of BOTH
    terms, and the root / reciprocal is bounded over the whole interval [v - e_v, v + e_v] (clamps included), not to first order;
  * a device math function: K_ULP[fn] ulp of f32 per call (measured, see below), an argument error times the derivative.
K_ULP: ROCm ships no accuracy table on the build machine, so the allowances were measured once by tools/ops_math_probe.py
(zvxk_math_probe) over exactly the arguments these cases feed each function (profiles/ops_kernel_spec.txt: worst ulp error seen;
k = twice that, at least 1)."""
import math
import zlib

import numpy as np

import kernel_ref as K
from kernel_ref import DT_F32, DT_BF16, DT_F16, U, round_to, to_bits, from_bits, half_ulp, sentinel_bits, nan_bits

I32, I16, U64 = "i32", "i16", "u64"
E1 = 2.0 ** -22
# measured on one MI355X (profiles/ops_kernel_spec.txt): worst ulp error over the cases' own arguments -> k = max(1, ceil(2 x worst)):
# expf 0.836, tanhf 1.230, logf 2.010, sqrtf 0.500, 1 / x 0.500 (the last two correctly rounded)
K_ULP = {"exp": 2, "tanh": 3, "log": 5, "sqrt": 1, "div": 1}
PROBE_FN = {"exp": 0, "tanh": 1, "log": 2, "sqrt": 3, "div": 4}
PROBE_ARGS = {k: [] for k in PROBE_FN}          # the f32 arguments the references evaluated each function at, while COLLECT is set
COLLECT = False                                 # set by tools/ops_math_probe.py, the tool that measured K_ULP
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def _np_t(dt):
    return {DT_F32: np.uint32, DT_BF16: np.uint16, DT_F16: np.uint16, I32: np.int32, I16: np.int16, U64: np.uint64}[dt]


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ulp32(x):
    return 2.0 * half_ulp(x, DT_F32)


def rel(*names):
    """Relative error of a chain of device math calls / roundings: k ulp each (an ulp is at most 2 u relative), + one rounding."""
    return sum(K_ULP[n] for n in names) * 2 * U + 2 * U


def _probe(fn, arg):
    if COLLECT:
        PROBE_ARGS[fn].append(np.asarray(arg, np.float64).astype(np.float32).ravel())


def values(bits, dt):
    if dt in (I32, I16, U64):
        return np.asarray(bits).astype(np.float64)
    return from_bits(bits, dt)


def bits_of(v, dt):
    if dt in (I32, I16, U64):
        return np.asarray(v).astype(_np_t(dt))
    v = np.asarray(v, np.float64)
    b = to_bits(np.nan_to_num(v, nan=0.0), dt)
    return np.where(np.isnan(v), nan_bits(dt), b).astype(_np_t(dt))


def store(v, err, dt):
    """(ref, tol) of the f32-class value v with error bound err after the cast to dt (kernel_ref._store's rule)."""
    ref = np.clip(v, -K.F16_MAX, K.F16_MAX) if dt == DT_F16 else v
    return ref, err + half_ulp(np.abs(ref) + err, dt)


def exact_sum(x):
    """True when every partial sum of x, in any order, is exact in f32: all terms on one power-of-two grid, sum|x| < 2^24 steps."""
    x = np.asarray(x, np.float64).ravel()
    if np.isnan(x).any():
        return False
    nz = x[x != 0]
    if not len(nz):
        return True
    m, e = np.frexp(nz)
    mi = (np.abs(m) * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64) - 53 + e      # exponent of each term's lowest set bit
    g = 2.0 ** tz.min()
    return np.abs(nz).sum() / g < 2 ** 24


def sum_err(terms, axis=None):
    t = np.asarray(terms, np.float64)
    if axis is None:
        return 0.0 if exact_sum(t) else 2 * t.size * U * np.abs(t).sum()
    return 2 * t.shape[axis] * U * np.abs(t).sum(axis)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def mlen(lens, mut, cap=None):
    """The two length mutations every ragged launcher is held to."""
    l = np.asarray(lens).copy()
    if mut == "len_plus1":
        l = l + 1
    if mut == "len_minus1":
        l = np.maximum(l - 1, 0)
    return np.minimum(l, cap) if cap is not None else l


class Case:
    def __init__(self, name, fn):
        self.name, self.fn, self.bufs, self.args, self.may, self.ref, self.info = name, fn, {}, [], {}, None, {}

    def inp(self, key, v, dt, out=False):
        self.bufs[key] = dict(bits=bits_of(np.asarray(v).ravel(), dt), dt=dt, out=out)
        return key

    def out(self, key, n, dt):
        sent = -1 if dt in (I32, I16) else (2 ** 64 - 1 if dt == U64 else sentinel_bits(dt))
        self.bufs[key] = dict(bits=np.full(n, sent).astype(_np_t(dt)) if dt != U64 else np.full(n, sent, np.uint64), dt=dt, out=True)
        return key

    def val(self, key):
        return values(self.bufs[key]["bits"], self.bufs[key]["dt"])


def full(n, ref=0.0, tol=0.0, mask=False):
    return [np.full(n, ref, np.float64), np.full(n, tol, np.float64), np.full(n, mask, bool)]


def esz(dt):
    return {DT_F32: 4, DT_BF16: 2, DT_F16: 2, I32: 4, I16: 2, U64: 8}[dt]


def nanfill(shape):
    return np.full(shape, np.nan)


def rnd(rng, shape, dt, scale=1.0, off=0.0):
    return round_to(rng.standard_normal(shape) * scale + off, dt)


# ------------------------------------------------------------------------------------------------------------------------------
# data movement and integers
# ------------------------------------------------------------------------------------------------------------------------------
def trunc16(x, dt):
    return K.trunc_to(np.clip(x, -K.F16_MAX, K.F16_MAX) if dt == DT_F16 else x, dt)


def c_cast(idt, odt, fn="cast"):
    cs = Case(f"{fn}_{K.DT_NAME[idt]}_{K.DT_NAME[odt]}", fn)
    rng = _rng(cs.name)
    x = rng.standard_normal(1000) * 10.0 ** rng.integers(-6, 5, 1000)
    x[:12] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0, -70000.0, 65520.0, -65519.9, 65504.0, 3e-8, -6e-6, 0.0]
    x = round_to(x, idt)
    n = len(x)
    cs.inp("in", x, idt); cs.out("out", n + 8, odt)
    cs.args = ["in", idt, "out", odt, n] if fn == "cast" else ["in", "out", n]

    def ref(mut=None):
        o = full(n + 8)
        o[0][:n] = trunc16(x, odt) if mut == "truncate" else round_to(x, odt)
        o[2][:int(mlen([n], mut)[0])] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_transpose16(with_len):
    cs = Case(f"transpose16_len{int(with_len)}", "transpose16")
    rng = _rng(cs.name)
    B, rows, C, ld_in, ld_out = 2, 70, 72, 80, 72
    lens = [70, 5]
    x = nanfill((B, rows, ld_in))
    for b in range(B):
        x[b, :(lens[b] if with_len else rows), :C] = rnd(rng, ((lens[b] if with_len else rows), C), DT_BF16)
    cs.inp("in", x, DT_BF16); cs.out("out", B * C * ld_out + 8, DT_BF16)
    if with_len:
        cs.inp("len", lens, I32)
    cs.args = ["in", ld_in, "out", ld_out, B, rows, C, "len" if with_len else None]

    def ref(mut=None):
        l = mlen(lens, mut, rows) if with_len else np.full(B, rows - (mut == "len_minus1"))
        o = full(B * C * ld_out + 8)
        r = np.zeros((B, C, ld_out))
        for b in range(B):
            r[b, :, :l[b]] = x[b, :l[b], :C].T
        o[0][:r.size] = r.ravel(); o[2][:r.size] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_zero_tail_cols(es):
    dt = DT_F32 if es == 4 else DT_BF16
    cs = Case(f"zero_tail_cols_es{es}", "zero_tail_cols")
    rng = _rng(cs.name)
    B, rows, cols, ld = 3, 3, 300, 304
    lens = [300, 7, 0]
    x = rnd(rng, (B, rows, ld), dt)
    cs.inp("x", x, dt, out=True); cs.inp("len", lens, I32)
    cs.args = ["x", es, ld, rows * ld, B, rows, cols, "len"]

    def ref(mut=None):
        l = mlen(lens, mut, cols)
        o = full(x.size)
        m = np.zeros(x.shape, bool)
        for b in range(B):
            m[b, :, l[b]:cols] = True
        o[2] = m.ravel()
        return {"x": o}
    cs.ref = ref
    return cs


def split_planes(v, f16):
    """[hi, lo] planes of the f32 value v as k_split3 writes them (values; lo carries its 2^11 scale in half)."""
    if not f16:
        hi = round_to(v, DT_BF16)
        return hi, round_to(f32(v - hi), DT_BF16)
    hi = round_to(v, DT_F16)
    return hi, round_to(f32(f32(v - hi) * 2048.0), DT_F16)


def c_split3(f16):
    cs = Case(f"split3_{'f16' if f16 else 'bf16'}", "split3")
    rng = _rng(cs.name)
    B, R, C, ldx = 3, 5, 24, 28
    rows = [5, 2, 0]
    pdt = DT_F16 if f16 else DT_BF16
    x = nanfill((B, R, ldx))
    for b in range(B):
        x[b, :rows[b], :C] = f32(rng.standard_normal((rows[b], C)) * 10.0 ** rng.integers(-5, 3, (rows[b], C)))
    x[0, 0, :6] = f32([65504.0, -65504.0, 70000.0, 2.0 ** -13 * 1.0003, -2.0 ** -12 * 1.00007, 1.0])
    cs.inp("x", x, DT_F32); cs.inp("rows", rows, I32); cs.out("out", B * R * 3 * C + 8, pdt)
    cs.args = ["x", ldx, "out", B, R, "rows", C, f16]

    def ref(mut=None):
        l = mlen(rows, mut, R)
        r = np.zeros((B, R, 3, C))
        for b in range(B):
            hi, lo = split_planes(x[b, :l[b], :C], f16)
            r[b, :l[b], 0], r[b, :l[b], 1], r[b, :l[b], 2] = hi, hi, (0 * lo if mut == "drop_lo" else lo)
        o = full(r.size + 8)
        o[0][:r.size] = r.ravel(); o[2][:r.size] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_split3_weights(f16):
    cs = Case(f"split3_weights_{'f16' if f16 else 'bf16'}", "split3_weights")
    rng = _rng(cs.name)
    nrows, Kk, scale = 3, 37, (2.0 ** 13 if f16 else 1.0)
    w = f32(rng.standard_normal((nrows, Kk)) * 10.0 ** rng.integers(-6, 1, (nrows, Kk)))
    w[0, :3] = [3.9, -3.99, 2.0 ** -20]
    pdt = DT_F16 if f16 else DT_BF16
    cs.inp("w", w, DT_F32); cs.out("out", nrows * 3 * Kk + 8, pdt)
    cs.args = ["w", "out", nrows, Kk, f16, float(scale)]

    def ref(mut=None):
        r = np.zeros((nrows, 3, Kk))
        if f16:
            v = f32(w * (1.0 if mut == "drop_scale" else scale))
            wh = round_to(v, DT_F16)
            r[:, 0], r[:, 1], r[:, 2] = wh, f32(v - wh).astype(np.float16).astype(np.float64), round_to(f32(v / 2048.0), DT_F16)
        else:
            hi, lo = split_planes(w, 0)
            r[:, 0], r[:, 1], r[:, 2] = hi, (0 * lo if mut == "drop_scale" else lo), hi
        o = full(r.size + 8)
        o[0][:r.size] = r.ravel(); o[2][:min(int(mlen([nrows], mut)[0]) * 3 * Kk, r.size + 8)] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_absmax(n):
    cs = Case(f"absmax_n{n}", "absmax")
    x = f32(_rng(cs.name).standard_normal(n + 4))
    if n:
        x[n - 1] = -7.25                              # the largest magnitude is negative and sits in the last element read
    x[n:] = 100.0                                     # past n: never read
    cs.inp("x", x, DT_F32); cs.out("out", 2, DT_F32)
    cs.args = ["x", n, "out"]

    def ref(mut=None):
        o = full(2)
        k = int(mlen([n], mut)[0]) if n else 0
        o[0][0] = (max(x[:k].max(), 0.0) if mut == "no_abs" else np.abs(x[:k]).max()) if k else 0.0
        o[2][0] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_embed():
    cs = Case("embed", "embed")
    rng = _rng(cs.name)
    B, Tmax, ed, pd, nph, npu = 3, 5, 24, 8, 11, 4
    T = [5, 3, 0]
    H = ed + pd
    emb, pemb, pe = rnd(rng, (nph, ed), DT_F32), rnd(rng, (npu, pd), DT_F32), rnd(rng, (Tmax, H), DT_F32)
    ph, pu = rng.integers(0, nph, (B, Tmax)), rng.integers(0, npu, (B, Tmax))
    for k, v, dt in (("ph", ph, I32), ("pu", pu, I32), ("emb", emb, DT_F32), ("pemb", pemb, DT_F32), ("pe", pe, DT_F32), ("T", T, I32)):
        cs.inp(k, v, dt)
    cs.out("out", B * Tmax * H, DT_F32)
    cs.args = ["ph", "pu", "emb", ed, "pemb", pd, "pe", "out", B, Tmax, "T"]

    def ref(mut=None):
        l = mlen(T, mut, Tmax)
        r, m = np.zeros((B, Tmax, H)), np.zeros((B, Tmax, H), bool)
        for b in range(B):
            for t in range(l[b]):
                r[b, t] = f32(np.concatenate([emb[ph[b, t]], pemb[pu[b, t]]]) + (0 if mut == "drop_pe" else pe[t]))
                m[b, t] = True
        return {"out": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


def bucket_idx(v, nb, mut=None):
    p = f32(np.nan_to_num(v, nan=0.0) * (nb - 1))
    p = np.where(np.isnan(v), 0.0, p)
    r = np.where(p >= 0, np.floor(p + 0.5), np.ceil(p - 0.5)) if mut == "half_away" else np.rint(p)
    return np.clip(r, 0, nb - 1).astype(np.int64)


def c_bucket(ctl):
    """ctl: None = the plain kernel; else a subset of {'range', 'shift', 'target'}, or 'unit' = range 1 / shift 0."""
    cs = Case("bucket_embed_add" + ("" if ctl is None else "_ctl_" + ("none" if not ctl else "_".join(sorted(ctl)))), "bucket_embed_add" + ("" if ctl is None else "_ctl"))
    rng = _rng("bucket")                              # the same data for every form: the unit form must give the plain indices
    B, Tmax, C, ldx, nb = 4, 7, 20, 24, 257
    T = [7, 5, 0, 3]
    pred = nanfill((B, Tmax))
    pred[0] = f32([0.5 / 256, 1.5 / 256, 2.5 / 256, -0.3, 1.7, np.nan, 0.4999])
    pred[1, :5] = f32([2.0 ** 24, 0.3, 0.41, 0.27, -2.0 ** 24])    # an f32 running sum loses the small terms: mean 0 instead of 0.196
    pred[3, :3] = f32([0.2, np.nan, 0.7])              # with a range the mean, and every index of the utterance, is NaN -> 0
    table = rnd(rng, (nb, C), DT_F32)
    x = nanfill((B, Tmax, ldx))
    for b in range(B):
        x[b, :T[b], :C] = rnd(rng, (T[b], C), DT_F32)
    x0 = x.copy()
    unit = ctl == {"unit"}
    if ctl is not None and (unit or "range" in ctl):
        pred[0, 5] = f32(0.9)                          # (a NaN prediction makes the utterance's mean, and with it every index, NaN -> 0)
    rg = f32([1.0] * B if unit else [1.5, 2.0, 2.0, 1.5]); sh = f32([0.0] * B if unit else [0.013, -0.2, 0.5, 0.1])
    tg = nanfill((B, Tmax)); tg[0, 1], tg[0, 5], tg[1, 0] = 0.75, 0.25, 2.5 / 256
    cs.inp("pred", pred, DT_F32); cs.inp("table", table, DT_F32); cs.inp("x", x, DT_F32, out=True); cs.out("idx", B * Tmax, I32); cs.inp("T", T, I32)
    if ctl is None:
        cs.args = ["pred", "table", nb, "x", ldx, C, "idx", B, Tmax, "T"]
    else:
        use_r, use_s, use_t = unit or "range" in ctl, unit or "shift" in ctl, "target" in ctl
        if use_r: cs.inp("range", rg, DT_F32)
        if use_s: cs.inp("shift", sh, DT_F32)
        if use_t: cs.inp("target", tg, DT_F32)
        cs.args = ["pred", "shift" if use_s else None, "range" if use_r else None, "target" if use_t else None, "table", nb, "x", ldx, C, "idx", B, Tmax, "T"]

    def ref(mut=None):
        l = mlen(T, mut, Tmax)
        xi, xm = x0.copy(), np.zeros(x0.shape, bool)
        ii, im = np.zeros((B, Tmax)), np.zeros((B, Tmax), bool)
        for b in range(B):
            if not l[b]:
                continue
            v = pred[b, :l[b]].copy()
            if ctl is not None and use_r and mut != "drop_range":
                mean = float(np.float32(math.fsum(pred[b, :l[b]]) / l[b]))      # the float64 mean rounded once (NaN if a prediction is)
                if mut == "mean_f32":                  # the mean accumulated in f32, in order
                    acc = np.float32(0.0)
                    for p_ in pred[b, :l[b]].astype(np.float32):
                        acc = np.float32(acc + p_)
                    mean = float(acc / np.float32(l[b]))
                v = f32(v + f32(f32(rg[b] - 1.0) * f32(v - mean)))
            if ctl is not None and use_s and mut != "drop_shift":
                v = f32(v + sh[b])
            if ctl is not None and use_t and mut != "no_target":
                g = tg[b, :l[b]]
                v = np.where(np.isnan(g), v, g)
            idx = bucket_idx(v, nb, mut)
            ii[b, :l[b]], im[b, :l[b]] = idx, True
            xi[b, :l[b], :C] = f32(x0[b, :l[b], :C] + table[idx])
            xm[b, :l[b], :C] = True
        return {"idx": [ii.ravel(), np.zeros(ii.size), im.ravel()], "x": [xi.ravel(), np.zeros(xi.size), xm.ravel()]}
    cs.ref = ref
    return cs


def dur_of(forced, logd):
    if forced is not None:
        return np.clip(forced, 0, 65536).astype(np.int64)
    e = np.exp(logd)
    _probe("exp", logd[~np.isnan(logd)])
    d = np.rint(f32(np.minimum(f32(e), 3e38)) - 1.0)
    return np.clip(np.where(np.isnan(logd), 0, d), 0, 65536).astype(np.int64)


def c_durations(kind, q16, big=False):
    """kind 'forced' / 'pred'.  Predicted log-durations sit at log(k + 1 + f), |f| <= 0.3: rint(exp(.) - 1) is k for any exp within the
    allowance, so the integers are exact."""
    cs = Case(f"durations{'_q16' if q16 else ''}_{kind}{'_big' if big else ''}", "durations_q16" if q16 else "durations")
    rng = _rng(cs.name)
    T = [32770] if big else [1, 63, 64, 65, 130, 0]
    B, Tmax = len(T), max(T)
    forced = logd = None
    if kind == "forced":
        forced = rng.integers(-2, 9, (B, Tmax))
        if big:
            forced[:] = 70000
        else:
            forced[4, 3], forced[4, 100] = 70000, 65536
    else:
        k = rng.integers(0, 12, (B, Tmax))
        logd = f32(np.log(k + 1 + rng.uniform(-0.3, 0.3, (B, Tmax))))
        logd[4, 0], logd[4, 1], logd[4, 2], logd[4, 70] = np.nan, -50.0, 20.0, 12.0
    src = forced if forced is not None else logd
    for b in range(B):                                 # past T[b]: never read
        src[b, T[b]:] = -7 if forced is not None else np.nan
    q = None
    if q16:
        q = rng.choice([0, 65536, 49152, 32768, 98304, 21845], (B, Tmax))
        if big:
            q[:] = 65536
        else:
            q[4, 120:124] = 2 ** 30                   # 65536-frame phonemes x 2^14: the running count passes 2^31
            if forced is not None:
                forced[4, 120:124] = 65536
            else:
                logd[4, 120:124] = 20.0
        cs.inp("q", q, I32)
    if forced is not None: cs.inp("forced", forced, I32)
    else: cs.inp("logd", logd, DT_F32)
    cs.inp("T", T, I32)
    for k_ in ("dur", "cum"):
        cs.out(k_, B * Tmax, I32)
    cs.out("mel_len", B + 2, I32)
    cs.args = ["forced" if forced is not None else None, "logd" if logd is not None else None] + (["q"] if q16 else []) + ["dur", "cum", "mel_len", B, Tmax, "T"]

    def ref(mut=None):
        l = mlen(T, mut, Tmax)
        du, cu, m = np.zeros((B, Tmax)), np.zeros((B, Tmax)), np.zeros((B, Tmax), bool)
        ml = full(B + 2)
        for b in range(B):
            n = l[b]
            d = dur_of(None if forced is None else forced[b, :n], None if logd is None else logd[b, :n])
            if mut == "no_clamp" and forced is not None:
                d = np.maximum(forced[b, :n], 0).astype(np.int64)
            if q16:
                P = np.cumsum(d * q[b, :n].astype(np.int64))
                rd = 0 if mut == "no_round" else 32768
                Cn = (P + rd) >> 16
                Cp = np.concatenate([[rd >> 16], Cn[:-1]])
                d, c = Cn - Cp, Cn
            else:
                c = np.cumsum(d)
            if mut == "wrap32":
                c = ((c + 2 ** 31) % 2 ** 32) - 2 ** 31
            du[b, :n], cu[b, :n], m[b, :n] = d, np.minimum(c, 2 ** 31 - 1), True
            ml[0][b], ml[2][b] = (min(c[-1], 2 ** 31 - 1) if n else 0), True
        return {"dur": [du.ravel(), np.zeros(du.size), m.ravel()], "cum": [cu.ravel(), np.zeros(cu.size), m.ravel()], "mel_len": ml}
    cs.ref = ref
    return cs


def c_length_regulate():
    cs = Case("length_regulate", "length_regulate")
    rng = _rng(cs.name)
    B, Tmax, C, ldx = 4, 6, 12, 16
    T = [6, 4, 0, 1]
    dur = np.array([[0, 3, 0, 2, 6, 0], [2, 0, 0, 1, 0, 0], [0] * 6, [3, 0, 0, 0, 0, 0]])
    cum = np.cumsum(dur, 1)
    mel_len = [int(cum[b, T[b] - 1]) if T[b] else 0 for b in range(B)]
    Lmax = 11
    x = nanfill((B, Tmax, ldx))
    for b in range(B):
        x[b, :T[b], :C] = rnd(rng, (T[b], C), DT_F32)
        cum[b, T[b]:] = -9
    cs.inp("x", x, DT_F32); cs.inp("cum", cum, I32); cs.inp("T", T, I32); cs.inp("mel_len", mel_len, I32); cs.out("feats", B * Lmax * C, DT_F32)
    cs.args = ["x", ldx, "cum", "T", "mel_len", "feats", B, Tmax, Lmax, C]

    def ref(mut=None):
        ml = mlen(mel_len, mut, Lmax)
        r, m = np.zeros((B, Lmax, C)), np.zeros((B, Lmax, C), bool)
        for b in range(B):
            if not T[b]:
                continue
            src = np.repeat(np.arange(T[b]), dur[b, :T[b]])
            src = np.concatenate([src, np.full(max(0, ml[b] - len(src)), T[b] - 1)])[:ml[b]]
            if mut == "src_le":
                src = np.array([int(np.searchsorted(cum[b, :T[b]], l_, side="left")) for l_ in range(ml[b])]).clip(0, T[b] - 1)
            r[b, :ml[b]], m[b, :ml[b]] = x[b, src, :C], True
        return {"feats": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


def c_add_pe_cast(ydt, with_pe, out_rows):
    cs = Case(f"add_pe_cast_{K.DT_NAME[ydt]}_pe{int(with_pe)}_rows{out_rows}", "add_pe_cast")
    rng = _rng(cs.name)
    B, Lmax, C, ldy = 3, 7, 70, 72
    L = [7, 5, 0]
    R = out_rows if out_rows > 0 else Lmax
    x = nanfill((B, Lmax, C))
    for b in range(B):
        x[b, :L[b]] = rnd(rng, (L[b], C), DT_F32, 3.0)
    pe = rnd(rng, (Lmax, C), DT_F32)
    cs.inp("x", x, DT_F32); cs.inp("pe", pe, DT_F32); cs.inp("L", L, I32); cs.out("y", B * R * ldy, ydt)
    cs.args = ["x", "pe" if with_pe else None, "y", ydt, ldy, B, Lmax, "L", C, out_rows]

    def ref(mut=None):
        l = mlen(L, mut, Lmax)
        r, m = np.zeros((B, R, ldy)), np.zeros((B, R, ldy), bool)
        for b in range(B):
            v = f32(x[b, :l[b]] + (pe[:l[b]] if with_pe and mut != "drop_pe" else 0.0))
            r[b, :l[b], :C], m[b, :l[b], :C] = (trunc16(v, ydt) if mut == "truncate" else round_to(v, ydt)), True
        return {"y": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


def c_mel_pad(mdt, vdt):
    cs = Case(f"mel_pad_{K.DT_NAME[mdt]}_{K.DT_NAME[vdt]}", "mel_pad")
    rng = _rng(cs.name)
    B, Lmax, nm, ldm, Pmax, ldv = 3, 6, 20, 24, 9, 24
    ml, P = [6, 3, 0], [9, 5, 2]
    mel = nanfill((B, Lmax, ldm))
    for b in range(B):
        mel[b, :ml[b], :nm] = rnd(rng, (ml[b], nm), mdt, 4.0)
    cs.inp("mel", mel, mdt); cs.inp("ml", ml, I32); cs.inp("P", P, I32); cs.out("v", B * Pmax * ldv, vdt)
    cs.args = ["mel", mdt, ldm, Lmax, "ml", "v", vdt, ldv, Pmax, "P", B, nm]

    def ref(mut=None):
        l = mlen(ml, mut, Lmax)
        r, m = np.zeros((B, Pmax, ldv)), np.zeros((B, Pmax, ldv), bool)
        for b in range(B):
            r[b, :l[b], :nm] = round_to(mel[b, :l[b], :nm], vdt)
            m[b, :(P[b] - (mut == "P_minus1")), :nm] = True
        return {"v": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


def c_copy_rows(sdt):
    cs = Case(f"copy_rows_f32_{K.DT_NAME[sdt]}", "copy_rows_f32")
    rng = _rng(cs.name)
    B, R, C, lds, ldd = 3, 5, 21, 24, 30
    rows = [5, 2, 0]
    s_bs, d_bs = R * lds + 8, R * ldd + 4
    src = nanfill((B, s_bs))
    for b in range(B):
        for r_ in range(rows[b]):
            src[b, r_ * lds:r_ * lds + C] = rnd(rng, C, sdt)
    cs.inp("src", src, sdt); cs.inp("rows", rows, I32); cs.out("dst", B * d_bs, DT_F32)
    cs.args = ["src", sdt, lds, s_bs, "dst", ldd, d_bs, B, R, "rows", C]

    def ref(mut=None):
        l = mlen(rows, mut, R)
        r, m = np.zeros((B, d_bs)), np.zeros((B, d_bs), bool)
        for b in range(B):
            for r_ in range(l[b]):
                r[b, r_ * ldd:r_ * ldd + C], m[b, r_ * ldd:r_ * ldd + C] = src[b, r_ * lds:r_ * lds + C], True
        return {"dst": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


def c_zero_tail_rows():
    cs = Case("zero_tail_rows", "zero_tail_rows")
    B, R, C, ldx = 3, 5, 21, 24
    rows = [5, 2, 0]
    x = rnd(_rng(cs.name), (B, R, ldx), DT_F32)
    cs.inp("x", x, DT_F32, out=True); cs.inp("rows", rows, I32)
    cs.args = ["x", ldx, B, R, "rows", C]

    def ref(mut=None):
        l = mlen(rows, mut, R)
        m = np.zeros(x.shape, bool)
        for b in range(B):
            m[b, l[b]:, :C] = True
        return {"x": [np.zeros(x.size), np.zeros(x.size), m.ravel()]}
    cs.ref = ref
    return cs


def c_count_sat16():
    cs = Case("count_sat16", "count_sat16")
    rng = _rng(cs.name)
    B, R, C, ld = 3, 6, 70, 72
    rows = [6, 3, 0]
    bs = R * ld + 8
    bits = to_bits(rng.standard_normal(B * bs), DT_F16).reshape(B, bs)
    pats = [0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7BFE, 0xFBFE]
    for b in range(B):
        for r_ in range(R):
            for i, p in enumerate(pats):
                bits[b, r_ * ld + 3 + 9 * i] = p       # inside the C columns of every row, valid or not
            bits[b, r_ * ld + C] = 0x7BFF             # a pad column
    cs.bufs["x"] = dict(bits=bits.ravel().copy(), dt=DT_F16, out=False)
    cs.bufs["count"] = dict(bits=np.array([1000, 2 ** 64 - 1], np.uint64), dt=U64, out=True)
    cs.inp("rows", rows, I32)
    cs.args = ["x", bs, ld, B, R, "rows", C, "count"]

    def ref(mut=None):
        l = mlen(rows, mut, R)
        n = 0
        for b in range(B):
            for r_ in range(l[b]):
                row = bits[b, r_ * ld:r_ * ld + C]
                n += int(((row & 0x7FFF) >= (0x7C00 if mut == "inf_only" else 0x7BFF)).sum())
        return {"count": [np.array([1000.0 + n, 0.0]), np.zeros(2), np.array([True, False])]}
    cs.ref = ref
    return cs


def c_reflect_pad():
    cs = Case("reflect_pad", "reflect_pad")
    rng = _rng(cs.name)
    B, pad, w_bs, out_cols = 3, 5, 40, 300
    n = [37, 6, 30]
    o_bs = out_cols + 4
    wav = nanfill((B, w_bs))
    for b in range(B):
        wav[b, :n[b]] = rnd(rng, n[b], DT_F32)
    cs.inp("wav", wav, DT_F32); cs.inp("n", n, I32); cs.out("out", B * o_bs, DT_F32)
    cs.args = ["wav", w_bs, "n", "out", o_bs, pad, B, out_cols]

    def ref(mut=None):
        r, m = np.zeros((B, o_bs)), np.zeros((B, o_bs), bool)
        nn = mlen(n, mut, w_bs)
        for b in range(B):
            r[b, :nn[b] + 2 * pad] = np.pad(wav[b, :nn[b]], pad, mode="symmetric" if mut == "edge_repeat" else "reflect")
            m[b, :out_cols] = True
        return {"out": [r.ravel(), np.zeros(r.size), m.ravel()]}
    cs.ref = ref
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm / SCLN
# ------------------------------------------------------------------------------------------------------------------------------
def ln_row(xr, C, mode, eps, g, be, post, mut):
    """(value, error bound) of one row in f32-class arithmetic, before the output cast."""
    xs = xr[:512] if mut == "drop_round2" else xr
    e_sum = sum_err(xs)
    mu = xs.sum() / C
    e_mu = e_sum / C + (0.0 if f32(mu) == mu else U * abs(mu))
    d = xr - mu
    e_d = e_mu + np.where(f32(d) == d, 0.0, U * np.abs(d))
    ds, es = (d[:512], e_d[:512]) if mut == "drop_round2" else (d, e_d)
    q = (ds * ds).sum()
    if mut == "uncentred":                             # the single-pass form in f32: sum x^2 - C mu^2
        q = max(float(np.sum(np.float32(xr) * np.float32(xr), dtype=np.float32)) - C * float(np.float32(mu)) ** 2, 0.0)
    e_q = (2 * np.abs(ds) * es + es * es).sum() + (0.0 if (not ds.any() and not es.any()) else (2 * C + 2) * U * q)
    m = mode ^ 1 if mut == "eps_swap" else mode
    div = C - 1 if (mode == 1) != (mut == "var_swap") else C
    if m == 0:
        inv, hi, lo = (1.0 / np.sqrt(v / div + eps) for v in (q, max(q - e_q, 0.0), q + e_q))
    else:
        inv, hi, lo = (1.0 / (np.sqrt(v / div) + eps) for v in (q, max(q - e_q, 0.0), q + e_q))
    _probe("sqrt", q / div + (eps if m == 0 else 0)); _probe("div", np.sqrt(q / div + (eps if m == 0 else 0)) + (0 if m == 0 else eps))
    e_inv = max(hi - inv, inv - lo) + inv * rel("sqrt", "div")
    p = post if (post is not None and mut != "drop_post") else 0.0
    t = d * inv * g
    y = t + be + p
    e_y = np.abs(inv * g) * e_d + np.abs(d * g) * e_inv + E1 * (np.abs(t) + np.abs(be) + np.abs(p))
    return y, e_y


LN_ROWS = [9, 5, 0]


def c_layernorm(tag, C, ldx_pad, mode, xdt, ydt, post, planes=0):
    """planes: 0 none, 1 bf16, 2 f16 (f32 output only)."""
    inplace = xdt == DT_F32 and ydt == DT_F32 and not planes
    cs = Case(f"layernorm_{tag}_m{mode}_{K.DT_NAME[xdt]}_{K.DT_NAME[ydt]}_post{int(post)}" + (f"_planes{planes}" if planes else ""), "layernorm")
    rng = _rng(cs.name)
    B, R = 3, 9
    ldx = C + ldx_pad
    ldy = ldx if inplace else C + (8 if ldx_pad == 0 else 0)
    eps = 1e-5 if mode == 0 else 1e-8
    x = nanfill((B, R, ldx))
    for b in range(B):
        for r in range(LN_ROWS[b]):
            kind = (b * 4 + r) % 9
            # kinds 6, 7: a large common offset on a power-of-two grid (100 + k 2^-6, spread ~1): every partial sum of the row is exact in f32,
            # so the bound carries no summation error of the mean and holds the CENTRED second moment; kind 8: a constant row
            v = np.ones(C) if kind == 8 else (100.0 + np.rint(rng.standard_normal(C) * 64.0) / 64.0 if kind in (6, 7) else rng.standard_normal(C))
            x[b, r, :C] = round_to(v, xdt)
    bg_bs = 2 * C + 8
    gamma, beta = rnd(rng, C, DT_F32, 0.5, 1.0), rnd(rng, C, DT_F32, 0.5)
    bg = rnd(rng, (B, bg_bs), DT_F32, 0.5, 0.5)
    pa = rnd(rng, (B, C), DT_F32)
    cs.inp("x", x, xdt, out=inplace)
    ykey = "x" if inplace else cs.out("y", B * R * ldy, ydt)
    cs.inp("rows", LN_ROWS, I32)
    if mode == 0:
        cs.inp("gamma", gamma, DT_F32); cs.inp("beta", beta, DT_F32)
    else:
        cs.inp("bg", bg, DT_F32)
    if post:
        cs.inp("post", pa, DT_F32)
    if planes:
        cs.out("planes", B * R * 3 * C + 8, DT_F16 if planes == 2 else DT_BF16)
    cs.args = ["x", xdt, ldx, ykey, ydt, ldy, B, R, "rows", C, mode, eps, "gamma" if mode == 0 else None, "beta" if mode == 0 else None,
               "bg" if mode == 1 else None, bg_bs, "post" if post else None, "planes" if planes else None, int(planes == 2)]
    cs.info = dict(B=B, R=R, C=C, ldy=ldy, planes=planes, ykey=ykey)
    if planes:                                         # the live rows' planes are held to launch_split3 of the f32 rows (test_ops_gpu)
        live = np.zeros((B, R, 3 * C), bool)
        for b in range(B):
            live[b, :LN_ROWS[b]] = True
        cs.may = {"planes": np.concatenate([live.ravel(), np.zeros(8, bool)])}

    def ref(mut=None):
        l = mlen(LN_ROWS, mut, R)
        n = B * R * ldy
        o = [x.ravel().copy(), np.zeros(n), np.zeros(n, bool)] if inplace else full(n)
        r, t, m = (a.reshape(B, R, ldy) for a in o)
        for b in range(B):
            g, be = (gamma, beta) if mode == 0 else (bg[b, C:2 * C], bg[b, :C])
            if mode == 1 and mut == "bg_swap":
                g, be = be, g
            for rr in range(l[b]):
                y, e = ln_row(x[b, rr, :C], C, mode, eps, g, be, pa[b] if post else None, mut)
                r[b, rr, :C], t[b, rr, :C] = store(y, e, ydt)
                m[b, rr, :C] = True
        res = {ykey: o}
        if planes:
            # values are held to launch_split3 of the kernel's own f32 output (test_ops_gpu); here: the zero rows past rows[b]
            po = full(B * R * 3 * C + 8)
            pm = po[2][:B * R * 3 * C].reshape(B, R, 3 * C)
            for b in range(B):
                pm[b, l[b]:] = True
            res["planes"] = po
        return res
    cs.ref = ref
    return cs


def layernorm_cases():
    cfgs = [("c8", 8, 0), ("c528", 528, 0), ("c1024", 1024, 0), ("c1032", 1032, 0), ("c20", 20, 0), ("c528pad", 528, 4)]
    pairs = [(DT_F32, DT_F32), (DT_F32, DT_BF16), (DT_F32, DT_F16), (DT_BF16, DT_BF16), (DT_F16, DT_F16)]
    out = []
    for ci, (tag, C, pad) in enumerate(cfgs):
        for mode in (0, 1):
            for pi, (xdt, ydt) in enumerate(pairs):
                out.append(c_layernorm(tag, C, pad, mode, xdt, ydt, (ci + mode + pi) % 2 == 0))
    for tag, C, pad in (cfgs[0], cfgs[1], cfgs[4]):
        for planes in (1, 2):
            out.append(c_layernorm(tag, C, pad, planes - 1, DT_F32, DT_F32, planes == 1, planes))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm family
# ------------------------------------------------------------------------------------------------------------------------------
def stats_ref(X, eps, mut=None):
    """mean, rstd of the valid rows X [L][C] and their bounds, by the shifted single pass k_colstats executes."""
    L = X.shape[0]
    sh = X[0]
    Xs = X
    if mut == "drop_last_group" and L > 1:
        Xs = X[:32 * ((L - 1) // 32)] if L > 32 else X[:L - 1]
    d = Xs - sh
    e_d = np.where(f32(d) == d, 0.0, U * np.abs(d))
    n = max(len(Xs), 1)
    a1, a2 = d.sum(0), (d * d).sum(0)
    e_a1 = 2 * n * U * np.abs(d).sum(0) + e_d.sum(0)
    e_a2 = 2 * n * U * a2 + (2 * np.abs(d) * e_d + U * d * d).sum(0)
    cnt = L - 1 if mut == "unbiased" and L > 1 else L
    m1 = a1 / L
    e_m1 = e_a1 / L + U * np.abs(m1)
    mean = sh + m1
    e_mean = e_m1 + U * np.abs(mean)
    v = a2 / cnt - m1 * m1 * (L / cnt)
    e_v = e_a2 / L + U * a2 / L + 2 * np.abs(m1) * e_m1 + e_m1 ** 2 + U * m1 * m1 + U * np.abs(v)
    if mut == "eps_outside":
        fr = lambda w: 1.0 / (np.sqrt(np.maximum(w, 0.0)) + eps)
    else:
        fr = lambda w: 1.0 / np.sqrt(np.maximum(w, 0.0) + eps)
    r = fr(v)
    _probe("sqrt", np.maximum(v, 0) + eps); _probe("div", np.sqrt(np.maximum(v, 0) + eps))
    e_r = np.maximum(fr(v - e_v) - r, r - fr(v + e_v)) + r * rel("sqrt", "div")
    return mean, e_mean + ulp32(mean), r, e_r, dict(v=v, e_v=e_v)


def apply_ref(x, m, r, gamma, beta, one_plus, act, slope, mut=None, e_m=0.0, e_r=0.0):
    g, be = 1.0, 0.0
    if gamma is not None:
        g, be = f32((1.0 if one_plus and mut != "drop_one_plus" else 0.0) + gamma), beta
    t, s = x * r * g, m * r * g
    y = t - s + be
    e = E1 * (np.abs(t) + np.abs(s) + np.abs(be)) + np.abs(r * g) * e_m + np.abs((x - m) * g) * e_r
    if act == ACT_RELU and mut != "drop_act":
        y = np.maximum(y, 0.0)
    if act == ACT_LRELU and mut != "drop_act":
        y = np.where(y >= 0, y, y * slope)
        e = e + U * np.abs(y)
    return y, e


IN_L = [1, 5, 32, 33, 127, 128, 129, 261, 0]


def c_instnorm(kind, C, xdt, ydt, affine, one_plus, act, adverse=False):
    """kind: 'stats', 'apply', 'fused'.  x [b][Lmax][ldx] (ldx > C), y a column slice (offset 8) of a buffer ldy = C + 16 wide."""
    cs = Case(f"instnorm_{kind}_c{C}_{K.DT_NAME[xdt]}" + (f"_{K.DT_NAME[ydt]}_aff{int(affine)}{int(one_plus)}_act{act}" if kind != "stats" else "")
              + ("_adverse" if adverse else ""), {"stats": "instnorm_stats", "apply": "norm_affine_act", "fused": "instnorm_fused"}[kind])
    rng = _rng(cs.name)
    Ls = [261] if adverse else IN_L
    B, Lmax = len(Ls), max(Ls)
    ldx, ldy, yoff, eps, slope = C + 8, C + 16, 8, 1e-5, 0.2
    g_bs = C + 8
    x = nanfill((B, Lmax, ldx))
    for b in range(B):
        v = rng.standard_normal((Ls[b], C)) * (0.01 if adverse else 1.0) + (1.0 if adverse else rng.standard_normal(C) * 0.5)
        if adverse and Ls[b]:
            v[0] += 100 * 0.01                        # the shift row is an outlier, 100 sigma from the mean
        x[b, :Ls[b], :C] = round_to(v, xdt)
    gamma, beta = rnd(rng, (B, g_bs), DT_F32, 0.3), rnd(rng, (B, g_bs), DT_F32, 0.3)
    mean_in, rstd_in = rnd(rng, (B, C), DT_F32, 0.5), f32(np.abs(rng.standard_normal((B, C))) + 0.5)
    cs.inp("x", x, xdt); cs.inp("L", Ls, I32)
    if kind != "apply":
        cs.out("mean", B * C, DT_F32); cs.out("rstd", B * C, DT_F32)
    else:
        cs.inp("mean", mean_in, DT_F32); cs.inp("rstd", rstd_in, DT_F32)
    if kind != "stats":
        cs.out("y", B * Lmax * ldy, ydt)
        if affine:
            cs.inp("gamma", gamma, DT_F32); cs.inp("beta", beta, DT_F32)
    ga, ba = ("gamma" if affine else None), ("beta" if affine else None)
    if kind == "stats":
        cs.args = ["x", xdt, ldx, B, Lmax, "L", C, eps, "mean", "rstd"]
    elif kind == "apply":
        cs.args = ["x", xdt, ldx, ("y", yoff), ydt, ldy, B, Lmax, "L", C, "mean", "rstd", ga, ba, g_bs, int(one_plus), act, slope]
    else:
        cs.args = ["x", xdt, ldx, ("y", yoff), ydt, ldy, B, Lmax, "L", C, eps, "mean", "rstd", ga, ba, g_bs, int(one_plus), act, slope]
    cs.info = dict(B=B, Lmax=Lmax, C=C, ldx=ldx, ldy=ldy, yoff=yoff, eps=eps, slope=slope, g_bs=g_bs, affine=affine, one_plus=one_plus, act=act,
                   xdt=xdt, ydt=ydt, adverse=adverse)
    if kind != "apply":
        zero = np.zeros((B, C), bool)
        for b in range(B):
            zero[b] = Ls[b] == 0
        cs.may = {"mean": zero.ravel(), "rstd": zero.ravel()}      # a zero-length utterance: its statistics are unspecified

    def ref(mut=None):
        l = mlen(Ls, mut, Lmax)
        res = {}
        M, R_, eM, eR, msk = (np.zeros((B, C)) for _ in range(5))
        if kind != "apply":
            for b in range(B):
                if l[b]:
                    M[b], eM[b], R_[b], eR[b], aux = stats_ref(x[b, :l[b], :C], eps, mut)
                    msk[b] = 1
                    if adverse:
                        cs.info["ratio16"] = float(np.max(eR[b] / R_[b]) / 2.0 ** -9), float(np.max(eR[b] / R_[b]) / 2.0 ** -12)
            res["mean"] = [M.ravel(), eM.ravel(), msk.ravel().astype(bool)]
            res["rstd"] = [R_.ravel(), (eR + ulp32(R_)).ravel(), msk.ravel().astype(bool)]
        else:
            M, R_ = mean_in, rstd_in
        if kind != "stats":
            o = full(B * Lmax * ldy)
            r, t, m = (a.reshape(B, Lmax, ldy) for a in o)
            for b in range(B):
                n = l[b]
                if mut == "drop_last_group" and kind == "apply" and n > 1:
                    n = n - 1                          # the last row of the four in flight
                y, e = apply_ref(x[b, :n, :C], M[b], R_[b], gamma[b, :C] if affine else None, beta[b, :C] if affine else None, one_plus, act, slope, mut,
                                 eM[b], eR[b])
                r[b, :n, yoff:yoff + C], t[b, :n, yoff:yoff + C] = store(y, e, ydt)
                m[b, :n, yoff:yoff + C] = True
            res["y"] = o
        return res
    cs.ref = ref
    return cs


def instnorm_cases():
    out = []
    acts = [(False, False, ACT_NONE), (True, True, ACT_LRELU), (True, False, ACT_RELU), (True, True, ACT_NONE)]
    for ci, C in enumerate((8, 64, 72, 136)):
        for xdt in (DT_F32, DT_BF16, DT_F16):
            out.append(c_instnorm("stats", C, xdt, xdt, False, False, 0))
        for pi, (xdt, ydt) in enumerate([(DT_BF16, DT_BF16), (DT_F16, DT_F16), (DT_F32, DT_F32), (DT_F32, DT_BF16)]):
            out.append(c_instnorm("apply", C, xdt, ydt, *acts[(ci + pi) % 4]))
        for pi, dt in enumerate((DT_BF16, DT_F16)):
            for k in range(2):
                out.append(c_instnorm("fused", C, dt, dt, *acts[(ci + pi + 2 * k) % 4]))
    for dt in (DT_BF16, DT_F16):
        out.append(c_instnorm("stats", 8, dt, dt, False, False, 0, adverse=True))
        out.append(c_instnorm("fused", 8, dt, dt, False, False, 0, adverse=True))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# softmax rows, rowdot, fc_rows, l2norm
# ------------------------------------------------------------------------------------------------------------------------------
def softmax_vals(row, mut=None):
    m = row.max()
    t = row - m
    e_t = np.where(f32(t) == t, 0.0, U * np.abs(t))
    _probe("exp", t)
    e = np.exp(t)
    rho = K_ULP["exp"] * 2 * U + e_t
    s = e.sum()
    e_s = 2 * len(row) * U * s + (rho * e).sum()
    _probe("div", s)
    p = e / s
    return p, p * (rho + e_s / s + rel("div"))


def c_softmax(pdt):
    cs = Case(f"softmax_rows_{K.DT_NAME[pdt]}", "softmax_rows")
    rng = _rng(cs.name)
    lens = [1, 7, 8, 9, 64, 65, 130]
    B, nh, Lmax = len(lens), 2, 131
    ld = 136
    sc = nanfill((B * nh, Lmax, ld))
    for b in range(B):
        for h in range(nh):
            sc[b * nh + h, :lens[b], :lens[b]] = f32(rng.standard_normal((lens[b], lens[b])) * 3.0)
        sc[b * nh, 0, lens[b] // 2] += 80.0            # exp underflows for every other key of this row
    sc = np.where(np.isnan(sc), np.nan, f32(np.nan_to_num(sc)))
    cs.inp("sc", sc, DT_F32); cs.inp("len", lens, I32); cs.out("P", B * nh * Lmax * ld, pdt)
    cs.args = ["sc", ld, "P", pdt, ld, B, nh, Lmax, "len"]

    def ref(mut=None):
        l = mlen(lens, mut, Lmax)
        o = full(B * nh * Lmax * ld)
        r, t, m = (a.reshape(B * nh, Lmax, ld) for a in o)
        for b in range(B):
            L = l[b]
            Lp = L if mut == "tail_not_zeroed" else (L + 7) & ~7
            for z in (b * nh, b * nh + 1):
                for rr in range(L):
                    p, e = softmax_vals(sc[z, rr, :L])
                    if mut == "no_max":
                        p = np.exp(sc[z, rr, :L]) / np.exp(np.minimum(sc[z, rr, :L], 80.0)).sum()
                    r[z, rr, :L], t[z, rr, :L] = store(p, e, pdt)
                    m[z, rr, :Lp] = True
        return {"P": o}
    cs.ref = ref
    return cs


def dot_ref(x, w, bias, mut=None):
    """rows of x . w + bias as an f32 sum of n products: (value, bound)."""
    n = x.shape[-1]
    if mut == "len_plus1":                             # K + 4: the next chunk of the row, which holds NaN
        x = np.concatenate([x, np.full(x.shape[:-1] + (4,), np.nan)], -1); w = np.concatenate([w, np.ones(4)])
    if mut == "drop_last_chunk":
        x = x.copy(); x[..., -4:] = 0
    s = (x * w).sum(-1) + (0.0 if mut == "drop_bias" else bias)
    mag = np.abs(x * w).sum(-1) + np.abs(bias)
    return s, (2 * n + 3) * U * mag


def c_rowdot():
    cs = Case("rowdot", "rowdot")
    rng = _rng(cs.name)
    B, Tmax, C, ldx, bias = 3, 6, 70, 72, 0.375
    T = [6, 5, 0]
    x = nanfill((B, Tmax, ldx))
    for b in range(B):
        x[b, :T[b], :C] = rnd(rng, (T[b], C), DT_F32)
    w = rnd(rng, C, DT_F32)
    cs.inp("x", x, DT_F32); cs.inp("w", w, DT_F32); cs.inp("T", T, I32); cs.out("out", B * Tmax, DT_F32)
    cs.args = ["x", ldx, "w", bias, "out", B, Tmax, "T", C]

    def ref(mut=None):
        l = mlen(T, mut, Tmax)
        o = full(B * Tmax)
        r, t, m = (a.reshape(B, Tmax) for a in o)
        for b in range(B):
            s, e = dot_ref(x[b, :l[b], :C], w, bias, mut)
            r[b, :l[b]], t[b, :l[b]] = store(s, e, DT_F32)
            m[b, :l[b]] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_fc_rows(B, Kk, with_bias=True):
    cs = Case(f"fc_rows_b{B}_k{Kk}_bias{int(with_bias)}", "fc_rows")
    rng = _rng(f"fc_rows_k{Kk}")                      # the same rows for every B of one K
    N, ldx, ldw, ldo = 7, Kk + 4, Kk + 8, 9
    x = rnd(rng, (50, ldx), DT_F32)[:B]
    x[:, Kk:] = np.nan
    w = rnd(rng, (N, ldw), DT_F32); w[:, Kk:] = np.nan
    bias = rnd(rng, N, DT_F32)
    cs.inp("x", x, DT_F32); cs.inp("w", w, DT_F32); cs.inp("bias", bias, DT_F32); cs.out("out", B * ldo, DT_F32)
    cs.args = ["x", ldx, "w", ldw, "bias" if with_bias else None, "out", ldo, B, N, Kk]
    cs.info = dict(B=B, N=N, K=Kk, ldx=ldx, ldw=ldw, ldo=ldo)

    def ref(mut=None):
        o = full(B * ldo)
        r, t, m = (a.reshape(B, ldo) for a in o)
        nb = B - 1 if mut == "len_minus1" else B
        for n in range(N):
            s, e = dot_ref(x[:nb, :Kk], w[n, :Kk], bias[n] if with_bias else 0.0, mut)
            r[:nb, n], t[:nb, n] = store(s, e, DT_F32)
            m[:nb, n] = True
        return {"out": o}
    cs.ref = ref
    return cs


def c_l2norm():
    cs = Case("l2norm_rows", "l2norm_rows")
    rng = _rng(cs.name)
    B, C = 4, 70
    x = rnd(rng, (B, C), DT_F32, 3.0)
    x[1] = 0.0
    x[2] *= 1e-3
    x = f32(x)
    cs.inp("x", x, DT_F32, out=True)
    cs.args = ["x", B, C]

    def ref(mut=None):
        o = full(B * C, mask=True)
        r, t, _ = (a.reshape(B, C) for a in o)
        Cm = int(mlen([C], mut)[0])                     # (mutated: the row norm over C -+ 1 elements of the buffer)
        flat = np.concatenate([x.ravel(), [0.0]])
        for b in range(B):
            s = (flat[b * C:b * C + Cm] ** 2).sum()
            e_s = (2 * C + 1) * U * s
            f = lambda v: 1.0 / max(np.sqrt(max(v, 0.0)), 1e-12)
            _probe("sqrt", s); _probe("div", max(np.sqrt(s), 1e-12))
            inv = f(s) if mut != "squared_norm" else 1.0 / max(s, 1e-12)
            e_inv = max(f(s - e_s) - f(s), f(s) - f(s + e_s)) + inv * rel("sqrt", "div") if s else 0.0
            r[b], t[b] = store(x[b] * inv, np.abs(x[b]) * e_inv + U * np.abs(x[b] * inv), DT_F32)
        return {"x": o}
    cs.ref = ref
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
# conv_post + tanh
# ------------------------------------------------------------------------------------------------------------------------------
def c_conv_post(xdt, kt, C, pcm16, mul2=False):
    """Utterance 1 is exact-sum data (x on k 2^-6, |k| <= 8; the weights of every case on a 2^-7 grid): its f32 accumulator is exact in any
    order, the bound is tanhf's allowance alone, and the PCM16 truncation rule is held as an exact integer on nearly all of its samples.
    mul2: out_len x 2 and in_len x 2 (the issue's output lengths include odd ones, so they run with out_mul = 1, len_mul = 2)."""
    cs = Case(f"conv_post_tanh_{K.DT_NAME[xdt]}_k{kt}_c{C}_{'pcm16' if pcm16 else 'f32'}{'_mul2' if mul2 else ''}", "conv_post_tanh")
    rng = _rng(cs.name)
    Nmax, wav_bs, ldx = 600, 608, C + 8
    nout = [600, 256, 0] if mul2 else [600, 257, 256, 3, 0]
    nin = [598, 254, 0] if mul2 else [598, 254, 252, 2, 0]
    len_mul, out_mul = 2, (2 if mul2 else 1)
    B, half, bias = len(nout), (kt - 1) // 2, 0.0625
    x = nanfill((B, Nmax, ldx))
    for b in range(B):
        v = np.rint(np.clip(rng.standard_normal((nin[b], C)) * 4.0, -8, 8)) / 64.0 if b == 1 else rng.standard_normal((nin[b], C)) * 0.5
        x[b, :nin[b], :C] = round_to(v, xdt)
        x[b, 40:60, :C] = np.where(np.isnan(x[b, 40:60, :C]), np.nan, round_to(np.abs(x[b, 40:60, :C]) * 8.0, xdt))    # |acc| large: tanh saturates
    w = np.rint((rng.standard_normal((kt, C)) * 0.15 + 0.05) * 128.0) / 128.0
    odt = I16 if pcm16 else DT_F32
    cs.inp("x", x, xdt); cs.inp("w", w, DT_F32); cs.inp("in_len", np.asarray(nin) // len_mul, I32); cs.inp("out_len", np.asarray(nout) // out_mul, I32)
    cs.out("wav", B * wav_bs, odt)
    cs.args = ["x", xdt, ldx, Nmax * ldx, "w", bias, kt, C, "wav", wav_bs, int(pcm16), B, Nmax, "in_len", len_mul, "out_len", out_mul]

    def ref(mut=None):
        no, ni = mlen(nout, mut if mut in ("len_plus1", "len_minus1") else None, Nmax), np.asarray(nin) + (mut == "nin_not_zeroed")
        o = full(B * wav_bs)
        r, t, m = (a.reshape(B, wav_bs) for a in o)
        for b in range(B):
            m[b, :Nmax] = not (mut == "tail_not_zeroed")
            n = no[b]
            if not n:
                continue
            m[b, :n] = True
            xp = np.zeros((n + kt, C))
            hi_ = min(ni[b], n + kt - 1 - half)
            xp[half:half + hi_] = x[b, :hi_, :C]
            acc, mag, prods = np.full(n, bias), np.full(n, abs(bias)), [np.array([bias])]
            for k in range(kt):
                sh = k + (1 if (mut == "shift_tap" and k == kt - 1) else 0)
                p = xp[sh:sh + n] * w[k]
                acc, mag = acc + p.sum(1), mag + np.abs(p).sum(1)
                prods.append(p.ravel())
            e_acc = 0.0 if exact_sum(np.concatenate(prods)) else (2 * kt * C + 3) * U * mag
            _probe("tanh", acc)
            v = np.tanh(acc)
            e_v = (1 - np.tanh(np.maximum(np.abs(acc) - e_acc, 0)) ** 2) * e_acc + K_ULP["tanh"] * ulp32(v)
            if not pcm16:
                r[b, :n], t[b, :n] = store(v, e_v, DT_F32)
            else:
                s = f32(v * 32760.0)
                es = e_v * 32760.0 + ulp32(s)
                ref_i = np.trunc(s)
                r[b, :n] = np.rint(s) if mut == "pcm_round" else ref_i
                t[b, :n] = np.maximum(np.abs(np.trunc(s + es) - ref_i), np.abs(np.trunc(s - es) - ref_i))
        return {"wav": o}
    cs.ref = ref
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
# speaker encoder
# ------------------------------------------------------------------------------------------------------------------------------
def c_spk_front(C0, odt):
    cs = Case(f"spk_front_c{C0}_{K.DT_NAME[odt]}", "spk_front")
    rng = _rng(cs.name)
    F, Tmax, Wout = 5, 70, 72
    lens = [70, 64, 1]
    B = len(lens)
    mels = nanfill((B, Tmax, F))
    for b in range(B):
        mels[b, :lens[b]] = rnd(rng, (lens[b], F), DT_F32, 2.0, -3.0)
    mean, rstd = rnd(rng, (B, F), DT_F32, 0.3, -3.0), f32(np.abs(rng.standard_normal((B, F))) * 0.2 + 0.5)
    w, bias = rnd(rng, (9, C0), DT_F32, 0.4), rnd(rng, C0, DT_F32, 0.2)
    bs, bt = rnd(rng, C0, DT_F32, 0.3, 1.0), rnd(rng, C0, DT_F32, 0.3)
    for k, v in (("mels", mels), ("mean", mean), ("rstd", rstd), ("w", w), ("bias", bias), ("bs", bs), ("bt", bt)):
        cs.inp(k, v, DT_F32)
    cs.inp("lens", lens, I32); cs.out("out", B * F * Wout * C0, odt)
    cs.args = ["mels", Tmax, "lens", F, "mean", "rstd", "w", "bias", "bs", "bt", C0, "out", odt, B, Wout]

    def ref(mut=None):
        l = mlen(lens, mut, Tmax)
        o = full(B * F * Wout * C0)
        r, t, m = (a.reshape(B, F, Wout, C0) for a in o)
        for b in range(B):
            T = l[b]
            if not T:
                continue
            xn = np.zeros((F + 2, T + 2))
            xn[1:F + 1, 1:T + 1] = ((mels[b, :T] - mean[b]) * rstd[b]).T
            if mut == "pad_edge":
                xn[0], xn[-1] = xn[1], xn[-2]
            e_x = 3 * U * np.abs(xn)
            a, mag, ex = np.zeros((F, T, C0)) + bias, np.zeros((F, T, C0)) + np.abs(bias), np.zeros((F, T, C0))
            for df in range(3):
                for dt_ in range(3):
                    p = xn[df:df + F, dt_:dt_ + T][:, :, None] * w[3 * df + dt_]
                    a, mag = a + p, mag + np.abs(p)
                    ex = ex + e_x[df:df + F, dt_:dt_ + T][:, :, None] * np.abs(w[3 * df + dt_])
            e_a = 22 * U * mag + ex
            y = np.maximum(a, 0) * bs + bt
            e = np.abs(bs) * e_a + E1 * (np.abs(np.maximum(a, 0) * bs) + np.abs(bt))
            r[b, :, :T], t[b, :, :T] = store(y, e, odt)
            m[b, :, :T] = True
        return {"out": o}
    cs.ref = ref
    return cs


def se_splits(H, Wmax):
    return min(max((H * Wmax + 511) // 512, 1), 64)


def c_se_pool(tag, C, H, Wmax, xdt):
    cs = Case(f"se_pool_{tag}_c{C}_h{H}_w{Wmax}_{K.DT_NAME[xdt]}", "se_pool")
    rng = _rng(cs.name)
    W = [Wmax, Wmax // 2 + 1, 1]
    B, total, S = len(W), H * Wmax, se_splits(H, Wmax)
    rpb = (total + S - 1) // S
    x = nanfill((B, H, Wmax, C))
    for b in range(B):
        x[b, :, :W[b]] = rnd(rng, (H, W[b], C), xdt, 1.0, 0.3)
    cs.inp("x", x, xdt); cs.inp("W", W, I32); cs.out("partial", B * S * C + 8, DT_F32)
    cs.args = ["x", xdt, B, H, Wmax, "W", C, "partial"]
    cs.info = dict(S=S)

    def ref(mut=None):
        l = mlen(W, mut if mut in ("len_plus1", "len_minus1") else None, Wmax)
        o = full(B * S * C + 8)
        r, t, m = (a[:B * S * C].reshape(B, S, C) for a in o)
        xf = x.reshape(B, total, C)
        col = np.arange(total) % Wmax
        for b in range(B):
            for s in range(S):
                rows = np.arange(s * rpb, min(total, (s + 1) * rpb))
                if mut == "drop_last_pass" and len(rows) > 1:
                    rows = rows[:-1]
                rows = rows[col[rows] < l[b]]
                v = xf[b, rows]
                r[b, s], t[b, s] = store(v.sum(0), 2 * max(len(rows), 1) * U * np.abs(v).sum(0), DT_F32)
                m[b, s] = True
        return {"partial": o}
    cs.ref = ref
    return cs


def c_se_fc(C, S, with_pb):
    cs = Case(f"se_fc_c{C}_s{S}_pb{int(with_pb)}", "se_fc")
    rng = _rng(cs.name)
    Cr, H, W = C // 8, 3, [20, 7, 1]
    B = len(W)
    part = rnd(rng, (B, S, C), DT_F32, 3.0, 1.0) * (np.array(W)[:, None, None] * H / S)
    part = f32(part)
    w1, b1, w2, b2 = rnd(rng, (Cr, C), DT_F32, 0.3), rnd(rng, Cr, DT_F32, 0.2), rnd(rng, (C, Cr), DT_F32, 0.5), rnd(rng, C, DT_F32, 0.3)
    pb = rnd(rng, C, DT_F32, 0.5)
    for k, v in (("partial", part), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("pb", pb)):
        cs.inp(k, v, DT_F32)
    cs.inp("W", W, I32); cs.out("scale", B * C + 8, DT_F32)
    cs.args = ["partial", S, H, "W", "w1", "b1", "w2", "b2", C, Cr, "scale", B, "pb" if with_pb else None]

    def ref(mut=None):
        o = full(B * C + 8)
        r, t, m = (a[:B * C].reshape(B, C) for a in o)
        for b in range(B):
            cnt = H * (W[b] + (mut == "len_plus1") - (mut == "len_minus1" and W[b] > 1))
            p = part[b, :S - 1] if (mut == "drop_last_partial" and S > 1) else part[b]
            mm = p.sum(0) / cnt + (pb if with_pb and mut != "drop_pool_bias" else 0.0)
            e_m = 2 * S * U * np.abs(p).sum(0) / cnt + 3 * U * np.abs(mm) + (U * np.abs(pb) if with_pb else 0)
            h = b1 + (w1 * mm).sum(1)
            e_h = (2 * C + 3) * U * (np.abs(b1) + np.abs(w1 * mm).sum(1)) + (np.abs(w1) * e_m).sum(1)
            h = np.maximum(h, 0)
            a = b2 + (w2 * h).sum(1)
            e_a = (2 * Cr + 3) * U * (np.abs(b2) + np.abs(w2 * h).sum(1)) + (np.abs(w2) * e_h).sum(1)
            _probe("exp", -a); _probe("div", 1 + np.exp(-a))
            sg = 1.0 / (1.0 + np.exp(-a))
            r[b], t[b] = store(sg, sg * (1 - sg) * (e_a + K_ULP["exp"] * 2 * U) + sg * rel("div"), DT_F32)
            m[b] = True
        return {"scale": o}
    cs.ref = ref
    return cs


def c_se_apply(C, dt):
    cs = Case(f"se_apply_c{C}_{K.DT_NAME[dt]}", "se_apply")
    rng = _rng(cs.name)
    H, Wmax = 11, 27
    W = [27, 14, 1]
    B = len(W)
    x, res = nanfill((B, H, Wmax, C)), nanfill((B, H, Wmax, C))
    for b in range(B):
        x[b, :, :W[b]], res[b, :, :W[b]] = rnd(rng, (H, W[b], C), dt), rnd(rng, (H, W[b], C), dt)
    scale = f32(rng.uniform(0.05, 0.95, (B, C)))
    cs.inp("x", x, dt); cs.inp("res", res, dt); cs.inp("scale", scale, DT_F32); cs.inp("W", W, I32); cs.out("y", x.size, dt)
    cs.args = ["x", "res", "y", dt, "scale", B, H, Wmax, "W", C]

    def ref(mut=None):
        l = mlen(W, mut, Wmax)
        o = full(x.size)
        r, t, m = (a.reshape(B, H, Wmax, C) for a in o)
        for b in range(B):
            xs = x[b, :, :l[b]] * scale[b]
            rs = 0.0 if mut == "drop_res" else res[b, :, :l[b]]
            r[b, :, :l[b]], t[b, :, :l[b]] = store(np.maximum(xs + rs, 0), E1 * (np.abs(xs) + np.abs(rs)), dt)
            m[b, :, :l[b]] = True
        return {"y": o}
    cs.ref = ref
    return cs


def asp_formulas(e, v, clamp=True):
    """weights e [T][D] (unnormalised), features v [T][D] -> mu, raw variance, sg"""
    s = e.sum(0)
    mu = (e * v).sum(0) / s
    var = (e * v * v).sum(0) / s - mu * mu
    return mu, var, np.sqrt(np.maximum(var, 1e-5) if clamp else np.maximum(var, 0.0))


def c_asp_pool(F, C, xdt, with_std):
    cs = Case(f"asp_pool_f{F}_c{C}_{K.DT_NAME[xdt]}_{'asp' if with_std else 'sap'}", "asp_pool")
    rng = _rng(cs.name)
    Wmax, W = 20, [20, 7, 1]
    B, D = len(W), F * C
    x, lg = nanfill((B, F, Wmax, C)), nanfill((B, Wmax, D))
    for b in range(B):
        x[b, :, :W[b]] = rnd(rng, (F, W[b], C), xdt)
        x[b, 1, :W[b], 3] = round_to(0.75, xdt)        # one feature column with zero weighted variance: the 1e-5 clamp
        lg[b, :W[b]] = rnd(rng, (W[b], D), DT_F32, 2.0)
    OD = (2 if with_std else 1) * D
    cs.inp("x", x, xdt); cs.inp("lg", lg, DT_F32); cs.inp("W", W, I32); cs.out("out", B * OD + 8, DT_F32)
    cs.args = ["x", xdt, "lg", B, F, Wmax, "W", C, "out", int(with_std)]

    def ref(mut=None):
        l = mlen(W, mut, Wmax)
        o = full(B * OD + 8)
        r, t, m = (a[:B * OD].reshape(B, OD) for a in o)
        for b in range(B):
            T = l[b]
            if not T:
                continue
            v = x[b, :, :T].transpose(1, 0, 2).reshape(T, D)
            a = lg[b, :T] - lg[b, :T].max(0)
            _probe("exp", a)
            e = np.exp(a)
            rho = K_ULP["exp"] * 2 * U + 2 * U * np.abs(a) + U
            s, sx, sxx = e.sum(0), (e * v).sum(0), (e * v * v).sum(0)
            e_s = 2 * T * U * s + (rho * e).sum(0)
            e_sx = 2 * T * U * np.abs(e * v).sum(0) + ((rho + U) * np.abs(e * v)).sum(0)
            e_sxx = 2 * T * U * sxx + ((rho + 2 * U) * e * v * v).sum(0)
            mu, var, sg = asp_formulas(e, v, mut != "no_clamp")
            e_mu = e_sx / s + np.abs(mu) * e_s / s + U * np.abs(mu)
            e_v = e_sxx / s + sxx / s * e_s / s + U * sxx / s + 2 * np.abs(mu) * e_mu + e_mu ** 2 + U * mu * mu + U * np.abs(var)
            f = lambda z: np.sqrt(np.maximum(z, 1e-5))
            _probe("sqrt", np.maximum(var, 1e-5))
            e_sg = np.maximum(f(var + e_v) - f(var), f(var) - f(var - e_v)) + sg * rel("sqrt")
            r[b, :D], t[b, :D] = store(mu, e_mu, DT_F32)
            m[b, :D] = True
            if with_std:
                r[b, D:], t[b, D:] = store(sg, e_sg, DT_F32)
                m[b, D:] = True
        return {"out": o}
    cs.ref = ref
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
# log-mel front end
# ------------------------------------------------------------------------------------------------------------------------------
def c_stft_mag():
    cs = Case("stft_mag", "stft_mag")
    rng = _rng(cs.name)
    B, Tmax, nf, lds_, ldm = 3, 5, 300, 604, 304
    frames = [5, 2, 0]
    spec = nanfill((B, Tmax, lds_))
    for b in range(B):
        spec[b, :frames[b], :2 * nf] = f32(rng.standard_normal((frames[b], 2 * nf)) * 10.0 ** rng.integers(-3, 3, (frames[b], 2 * nf)))
    spec[0, 0, 0] = spec[0, 0, nf] = 0.0
    cs.inp("spec", spec, DT_F32); cs.inp("frames", frames, I32); cs.out("mag", B * Tmax * ldm + 8, DT_F32)
    cs.args = ["spec", lds_, "mag", ldm, nf, B, Tmax, "frames"]

    def ref(mut=None):
        l = mlen(frames, mut, Tmax)
        o = full(B * Tmax * ldm + 8)
        r, t, m = (a[:B * Tmax * ldm].reshape(B, Tmax, ldm) for a in o)
        m[:] = True
        for b in range(B):
            re, im = spec[b, :l[b], :nf], spec[b, :l[b], nf:2 * nf]
            if mut == "im_offset":
                im = spec[b, :l[b], nf - 1:2 * nf - 1]
            p = re * re + im * im
            _probe("sqrt", p)
            v = np.sqrt(p)
            r[b, :l[b], :nf], t[b, :l[b], :nf] = store(v, v * (3 * U + rel("sqrt")), DT_F32)
        return {"mag": o}
    cs.ref = ref
    return cs


def c_log_clip():
    cs = Case("log_clip", "log_clip")
    rng = _rng(cs.name)
    B, Tmax, C, ldx, lo = 3, 5, 70, 72, 1e-5
    frames = [5, 2, 0]
    x = f32(np.abs(rng.standard_normal((B, Tmax, ldx))) * 10.0 ** rng.integers(-8, 3, (B, Tmax, ldx)))
    x[0, 0, :3] = [0.0, 1.0, 1.0 + 2.0 ** -20]
    x = f32(x)
    lo32 = float(np.float32(lo))
    cs.inp("x", x, DT_F32, out=True); cs.inp("frames", frames, I32)
    cs.args = ["x", ldx, C, lo, B, Tmax, "frames"]

    def ref(mut=None):
        l = mlen(frames, mut, Tmax)
        o = full(x.size)
        r, t, m = (a.reshape(B, Tmax, ldx) for a in o)
        m[:, :, :C] = True
        for b in range(B):
            a = np.maximum(x[b, :l[b], :C], 0.0 if mut == "no_clip" else lo32)
            _probe("log", a)
            with np.errstate(divide="ignore"):
                v = np.log(a)
            r[b, :l[b], :C], t[b, :l[b], :C] = v, K_ULP["log"] * ulp32(v) + half_ulp(v, DT_F32)
        return {"x": o}
    cs.ref = ref
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
FC_B = [1, 16, 17, 32, 33, 50]


def _build():
    cs = []
    cs += [c_cast(i, o) for i, o in ((DT_F32, DT_BF16), (DT_F32, DT_F16), (DT_BF16, DT_F32), (DT_F16, DT_F32), (DT_F16, DT_BF16), (DT_F32, DT_F32))]
    cs += [c_cast(DT_F32, DT_BF16, "f32_to_bf16")]
    cs += [c_transpose16(False), c_transpose16(True), c_zero_tail_cols(2), c_zero_tail_cols(4), c_split3(0), c_split3(1),
           c_split3_weights(0), c_split3_weights(1), c_absmax(1000), c_absmax(0), c_embed()]
    cs += layernorm_cases()
    cs += [c_softmax(dt) for dt in (DT_F32, DT_BF16, DT_F16)]
    cs += [c_rowdot(), c_bucket(None)] + [c_bucket(s) for s in ({"range"}, {"shift"}, {"target"}, set(), {"unit"}, {"range", "shift", "target"})]
    cs += [c_durations(k, q) for k in ("forced", "pred") for q in (False, True)] + [c_durations("forced", False, big=True), c_durations("forced", True, big=True)]
    cs += [c_length_regulate()] + [c_add_pe_cast(dt, pe, rows) for dt, pe, rows in ((DT_BF16, True, 0), (DT_F16, True, 9), (DT_F32, False, 9), (DT_BF16, False, 0))]
    cs += instnorm_cases()
    cs += [c_mel_pad(DT_F32, DT_BF16), c_mel_pad(DT_F32, DT_F16), c_mel_pad(DT_BF16, DT_BF16), c_copy_rows(DT_F32), c_copy_rows(DT_BF16), c_copy_rows(DT_F16)]
    cs += [c_conv_post(dt, kt, C, pcm) for dt, kt, C in ((DT_BF16, 7, 32), (DT_F16, 7, 32), (DT_BF16, 7, 16), (DT_BF16, 5, 32), (DT_F32, 7, 32)) for pcm in (0, 1)]
    cs += [c_conv_post(DT_BF16, 7, 32, 1, mul2=True), c_conv_post(DT_F32, 7, 32, 0, mul2=True)]
    cs += [c_count_sat16(), c_zero_tail_rows()]
    cs += [c_spk_front(C0, dt) for C0 in (8, 16) for dt in (DT_BF16, DT_F32)]
    pool = [("div", 32, 4, 16), ("coprime", 32, 6, 7), ("wrap", 32, 5, 24), ("long", 32, 3, 100), ("c24", 24, 4, 9), ("split", 32, 19, 27), ("c256", 256, 5, 9)]
    cs += [c_se_pool(t, C, H, Wm, dt) for t, C, H, Wm in pool for dt in (DT_BF16, DT_F32)]
    cs += [c_se_fc(C, S, (i + j) % 2 == 0) for i, C in enumerate((32, 24, 256)) for j, S in enumerate((1, 2, 5, 67))] + [c_se_fc(32, 5, False), c_se_fc(24, 2, False)]
    cs += [c_se_apply(32, DT_BF16), c_se_apply(24, DT_BF16), c_se_apply(32, DT_F32)]
    cs += [c_asp_pool(F, C, dt, ws) for F, C in ((3, 24), (5, 56)) for dt in (DT_BF16, DT_F32) for ws in (1, 0)]
    cs += [c_fc_rows(B, Kk) for Kk in (4, 256, 260) for B in FC_B] + [c_fc_rows(17, 260, False)]
    cs += [c_l2norm(), c_reflect_pad(), c_stft_mag(), c_log_clip()]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


# launcher -> the mutations of its reference that at least one of its cases must reject (tests/test_ops_reference.py)
_LEN = ["len_plus1", "len_minus1"]
MUTATIONS = {
    "cast": _LEN + ["truncate"], "f32_to_bf16": _LEN + ["truncate"], "transpose16": _LEN, "zero_tail_cols": _LEN, "split3": _LEN + ["drop_lo"],
    "split3_weights": _LEN + ["drop_scale"], "absmax": _LEN + ["no_abs"], "embed": _LEN + ["drop_pe"],
    "layernorm": _LEN + ["var_swap", "eps_swap", "bg_swap", "drop_post", "drop_round2", "uncentred"],
    "softmax_rows": _LEN + ["tail_not_zeroed", "no_max"], "rowdot": _LEN + ["drop_bias"], "bucket_embed_add": _LEN + ["half_away"],
    "bucket_embed_add_ctl": _LEN + ["half_away", "drop_shift", "no_target", "mean_f32", "drop_range"], "durations": _LEN + ["no_clamp", "wrap32"], "durations_q16": _LEN + ["no_round", "wrap32"],
    "length_regulate": _LEN + ["src_le"], "add_pe_cast": _LEN + ["drop_pe", "truncate"],
    "instnorm_stats": _LEN + ["drop_last_group", "unbiased", "eps_outside"], "norm_affine_act": _LEN + ["drop_last_group", "drop_one_plus", "drop_act"],
    "instnorm_fused": _LEN + ["drop_last_group", "unbiased", "eps_outside", "drop_one_plus", "drop_act"],
    "mel_pad": _LEN + ["P_minus1"], "copy_rows_f32": _LEN, "conv_post_tanh": _LEN + ["shift_tap", "nin_not_zeroed", "tail_not_zeroed", "pcm_round"],
    "count_sat16": _LEN + ["inf_only"], "zero_tail_rows": _LEN, "spk_front": _LEN + ["pad_edge"], "se_pool": _LEN + ["drop_last_pass"],
    "se_fc": _LEN + ["drop_pool_bias", "drop_last_partial"], "se_apply": _LEN + ["drop_res"], "asp_pool": _LEN + ["no_clamp"],
    "l2norm_rows": _LEN + ["squared_norm"], "reflect_pad": _LEN + ["edge_repeat"], "stft_mag": _LEN + ["im_offset"], "log_clip": _LEN + ["no_clip"],
    "fc_rows": _LEN + ["drop_bias", "drop_last_chunk"],
}

# launchers of the section without a case here, and why
EXCLUDED = {}
for _n in ("resample_poly", "join_powers", "join_bounds", "join_layout", "join_copy", "stream_rows", "stream_interiors", "loud_units", "loud_gates", "loud_common", "loud_apply", "limit_env", "limit_gain", "limit_reduce",
           "denoise_frames", "denoise_ola"):
    EXCLUDED["launch_" + _n] = "post-processing: compared with its own float64 reference through the C-ABI (tests/test_*_gpu.py)"
EXCLUDED["launch_window_pad"] = "enrolment: tests/test_enroll_gpu.py::test_cropped_windows_equal_the_chain_with_the_slice_cut_likewise (any offset, cropped, mirrored edges)"
# not a launcher: k_colstats' H > 1 form (a [H][Wmax] map per utterance) has no caller -- launch_instnorm_stats passes H = 1 -- so it is dead
DEAD_CODE = {"k_colstats H > 1": "no launcher passes H != 1"}


def rejected(cs, mut):
    """True when the mutated reference leaves the bound (or the written region) of the unmutated one in at least one element."""
    good, bad = cs.ref(), cs.ref(mut)
    for k, (r, t, m) in good.items():
        r2, _t2, m2 = bad[k]
        if (m != m2).any():
            return True
        with np.errstate(invalid="ignore"):
            if (~(np.abs(r2[m] - r[m]) <= t[m])).any():
                return True
    return False
