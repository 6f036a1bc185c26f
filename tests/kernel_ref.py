"""Float64 restatement of the launcher contracts of zvx_kernels.h (GemmArgs, FlashArgs, AttnF32Args), the ctypes mirror of those
structs, and the table of launcher cases that tests/test_kernels_gpu.py runs on the device and tests/test_kernel_reference.py checks
on the host.

Operands are rounded to the type the kernel reads before the reference sees them, so the only legitimate differences between a
kernel and `gemm_ref` / `attn_ref` are the fp32 accumulation order, the fp32 epilogue arithmetic and the output cast.  Every bound
is derived per element from the data:
    acc:     2 * n_terms * 2^-24 * sum |x * w|                      (fp32 accumulation, any order)
    epilogue 2^-22 * (sum of the magnitudes the epilogue adds)   (a handful of fp32 operations)
    output   + half an ulp of the output type at |ref| + the bound above (a rounding boundary may fall between kernel and reference)
Fused ResBlock kernels add the propagated term of their 16-bit intermediate (one ulp of it wherever its rounding is ambiguous
within the fp32 bound, through |W2| and the residual),
the 16-bit flash attention the term of its 16-bit probabilities.

The streaming ResBlock kernels (launch_resstream with StreamArgs, launch_narrowstage with StageArgs, launch_pairstream past one
segment) chain up to 18 convolutions through 16-bit intermediates; `chain_ref` (last section of this file) steps them in float64
with every 16-bit rounding where the kernel has it and propagates a per-element uncertainty: through |W|, through each 16-bit
rounding as Q(v + e) - Q(v - e), and through the two leaky-relus by their slope only where the sign is certain.  On exact-sum
data (every f32 partial sum exact, decided per element with exact_f32's rule) only element-wise f32 roundings remain, and the
tolerance of most elements is ZERO: the kernel must produce the reference's 16-bit value bit for bit.  That rests on one
premise -- a matrix instruction returns an exactly representable block sum exactly.  The 32 x 32 x 16 cases of GEMM_CASES have held
the kernels to it; for the 16 x 16 x 32 instruction of narrowstage nothing in the repository had measured it before
NARROW_CASES (results: profiles/stream_kernel_spec.txt).  Dense data, which sparse weights cannot replace for a misplaced weight
fragment, is checked by bit equality with the per-pair launches (resstream) or by rms against the pure float64 chain
(narrowstage, pairstream: rms_margin).
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTEST_LIB = os.path.join(ROOT, "zerovox_amd", "libzvx_ktest.so")

DT_F32, DT_BF16, DT_F16 = 0, 1, 2
DT_NAME = {DT_F32: "f32", DT_BF16: "bf16", DT_F16: "f16"}
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
MAX_TAPS = 16
U = 2.0 ** -24                     # unit roundoff of fp32
F16_MAX = 65504.0


def EPI(res, am, out):
    return res | (am << 1) | (out << 3)


EPI_DEC0, EPI_DEC1 = 16 | 8 | 0, 16 | 8 | 1
EPI_FLIP = EPI(0, 0, 1) | 32
EPI_NAMES = {EPI(0, 0, 1): "EPI(0,0,1)", EPI_FLIP: "FLIP", EPI(1, 0, 1): "EPI(1,0,1)", EPI(1, 2, 0): "EPI(1,2,0)", EPI(1, 3, 0): "EPI(1,3,0)",
             EPI(1, 1, 1): "EPI(1,1,1)", EPI_DEC0: "DEC(0)", EPI_DEC1: "DEC(1)", -1: "run-time"}


# ------------------------------------------------------------------------------------------------------------------------------
# 16-bit rounding and bit patterns
# ------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def round_to(x, dt):
    """The value the kernel reads when x is stored as dtype dt (f16 saturates to +-65504 like the kernels' stores)."""
    x = np.asarray(x, np.float64)
    if dt == DT_F32:
        return x.astype(np.float32).astype(np.float64)
    if dt == DT_BF16:
        return bf16_from_bits(bf16_bits(x.astype(np.float32)))
    return np.clip(x, -F16_MAX, F16_MAX).astype(np.float16).astype(np.float64)


def to_bits(x, dt):
    x = np.asarray(x, np.float64)
    if dt == DT_F32:
        return x.astype(np.float32).view(np.uint32)
    if dt == DT_BF16:
        return bf16_bits(x.astype(np.float32))
    return np.clip(x, -F16_MAX, F16_MAX).astype(np.float16).view(np.uint16)


def from_bits(b, dt):
    if dt == DT_F32:
        return np.asarray(b, np.uint32).view(np.float32).astype(np.float64)
    if dt == DT_BF16:
        return bf16_from_bits(b)
    return np.asarray(b, np.uint16).view(np.float16).astype(np.float64)


def half_ulp(x, dt):
    """Half a unit in the last place of dtype dt at |x| (subnormal spacing included)."""
    mant, emin = {DT_F32: (23, -126), DT_BF16: (7, -126), DT_F16: (10, -14)}[dt]
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** emin)
    return 0.5 * 2.0 ** (np.floor(np.log2(a)) - mant)


def esize(dt):
    return 4 if dt == DT_F32 else 2


def nan_bits(dt):
    return {DT_F32: 0x7FC00000, DT_BF16: 0x7FC0, DT_F16: 0x7E00}[dt]


def sentinel_bits(dt):
    return 0xFFFFFFFF if dt == DT_F32 else 0xFFFF


def bits_dtype(dt):
    return np.uint32 if dt == DT_F32 else np.uint16


# ------------------------------------------------------------------------------------------------------------------------------
# ctypes mirror of the argument structs (held to the compiled layout by test_struct_layout)
# ------------------------------------------------------------------------------------------------------------------------------
_p, _l, _i, _f = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
_taps = ctypes.c_int * MAX_TAPS


class GemmArgs(ctypes.Structure):
    _fields_ = [("X", _p), ("x_bs", _l), ("x_hs", _l), ("ldx", _i), ("W", _p), ("w_bs", _l), ("w_hs", _l), ("w_ts", _l), ("ldw", _i),
                ("Wp", _p), ("halo_l", _i), ("halo_r", _i), ("Wp2", _p), ("bias1", _p), ("dv1", _taps), ("fused", _i), ("slope1", _f),
                ("no_pairstream", _i), ("dtype", _i), ("M", _i), ("N", _i), ("K", _i), ("nbatch", _i), ("nheads", _i),
                ("in_len", _p), ("out_len", _p), ("k_len", _p), ("in_len_static", _i), ("ntaps", _i), ("du", _taps), ("dv", _taps),
                ("stride", _i), ("wout", _i), ("hin", _i), ("win", _i), ("flat_win", _i), ("flat_rows", _i), ("bflat", _i),
                ("X2", _p), ("x2_bs", _l), ("ldx2", _i), ("K2", _i), ("xcd_flat", _i), ("slab_small", _i), ("out_split3", _i),
                ("alpha", _f), ("bias", _p), ("bias_mode", _i), ("res", _p), ("r_bs", _l), ("r_hs", _l), ("ldr", _i),
                ("res_dtype", _i), ("res_mode", _i), ("res_inv_slope", _f), ("accum", _p), ("a_bs", _l), ("lda", _i),
                ("accum_mode", _i), ("accum_dtype", _i), ("out_scale", _f), ("act", _i), ("slope", _f), ("post_scale", _p),
                ("post_shift", _p), ("out", _p), ("o_bs", _l), ("o_hs", _l), ("ldo", _i), ("out_dtype", _i), ("se_part", _p),
                ("se_part_S", _p), ("ds_out", _p), ("ds_Wp", _p), ("ds_bias", _p), ("flops", ctypes.c_double)]


class FlashArgs(ctypes.Structure):
    _fields_ = [("qk", _p), ("qk_bs", _l), ("ldq", _i), ("k_off", _i), ("vt", _p), ("vt_bs", _l), ("ldv", _i), ("out", _p), ("o_bs", _l),
                ("ldo", _i), ("len", _p), ("L", _i), ("D", _i), ("nheads", _i), ("nbatch", _i), ("scale", _f), ("f16", _i), ("prof", _p)]


class AttnF32Args(ctypes.Structure):
    _fields_ = [("qkv", _p), ("bs", _l), ("ld", _i), ("q_off", _i), ("k_off", _i), ("v_off", _i), ("out", _p), ("o_bs", _l), ("ldo", _i),
                ("planes", _p), ("planes_C", _i), ("planes_f16", _i), ("len", _p), ("L", _i), ("D", _i), ("nheads", _i), ("nbatch", _i),
                ("scale", _f)]


class StreamArgs(ctypes.Structure):
    _fields_ = [("X", _p), ("x_bs", _l), ("ldx", _i), ("W1", _p * 3), ("W2", _p * 3), ("b1", _p * 3), ("b2", _p * 3), ("dil", _i * 3), ("C", _i),
                ("ntaps", _i), ("npair", _i), ("out", _p), ("o_bs", _l), ("ldo", _i), ("accum", _p), ("a_bs", _l), ("lda", _i), ("accum_mode", _i),
                ("slope1", _f), ("res_inv_slope", _f), ("out_scale", _f), ("slope", _f), ("len", _p), ("M", _i), ("nbatch", _i), ("S", _i),
                ("nseg", _i), ("dX0", _i), ("dT", _i), ("dX", _i * 3), ("flops", ctypes.c_double), ("prof", _p), ("seg_min", _i), ("f16", _i)]


class StageArgs(ctypes.Structure):
    _fields_ = [("X", _p), ("x_bs", _l), ("ldx", _i), ("W", _p), ("woff", _i * 18), ("bias", _p), ("C", _i), ("nk", _i), ("ks", _i * 3),
                ("dil", (_i * 3) * 3), ("out", _p), ("o_bs", _l), ("ldo", _i), ("slope1", _f), ("res_inv_slope", _f), ("slope", _f),
                ("len", _p), ("M", _i), ("nbatch", _i), ("f16", _i)]


class WmDetectRow(ctypes.Structure):
    _fields_ = [("x", _p), ("d", _p), ("n", _i), ("F", _i)]


class WmDetectArgs(ctypes.Structure):
    _fields_ = [("rows", _p), ("B", _i), ("n_fft", _i), ("log2n", _i), ("hop", _i), ("pad", _i), ("Fmax", _i), ("twid", _p), ("win", _p),
                ("sign", _p), ("k_lo", _i), ("KB", _i), ("J", _i), ("TB", _i), ("P", _i), ("WF", _i), ("NW", _i), ("win_score", _p),
                ("win_offset", _p)]


STRUCTS = {"GemmArgs": GemmArgs, "FlashArgs": FlashArgs, "AttnF32Args": AttnF32Args, "StreamArgs": StreamArgs, "StageArgs": StageArgs,
           "WmDetectRow": WmDetectRow, "WmDetectArgs": WmDetectArgs}


def load_ktest():
    """The test shim (built by zerovox_amd/build.py).  Loading it opens no device."""
    lib = ctypes.CDLL(KTEST_LIB)
    lib.zvxk_alloc.restype = ctypes.c_void_p
    lib.zvxk_alloc.argtypes = [ctypes.c_size_t]
    lib.zvxk_free.argtypes = [ctypes.c_void_p]
    for n in ("zvxk_h2d", "zvxk_d2h"):
        getattr(lib, n).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.zvxk_memset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    lib.zvxk_gemm.argtypes = [ctypes.POINTER(GemmArgs), ctypes.c_int]
    lib.zvxk_epi_mode.argtypes = [ctypes.POINTER(GemmArgs)]
    lib.zvxk_packed_weight_elems.restype = ctypes.c_size_t
    lib.zvxk_packed_weight_elems.argtypes = [ctypes.c_int] * 3
    lib.zvxk_pack_weights.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.zvxk_pack_pair.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.zvxk_flash.argtypes = [ctypes.POINTER(FlashArgs), ctypes.c_int]
    lib.zvxk_attn_f32.argtypes = [ctypes.POINTER(AttnF32Args), ctypes.c_int]
    lib.zvxk_resstream.argtypes = [ctypes.POINTER(StreamArgs), ctypes.c_int]
    lib.zvxk_narrowstage.argtypes = [ctypes.POINTER(StageArgs), ctypes.c_int]
    lib.zvxk_pack_narrow.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.zvxk_narrowstage_steps.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.zvxk_fft_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.zvxk_wm_bands.argtypes = [ctypes.POINTER(WmDetectArgs)]
    lib.zvxk_wm_search.argtypes = [ctypes.POINTER(WmDetectArgs)]
    lib.zvxk_variant_name.restype = ctypes.c_char_p
    lib.zvxk_sizeof.restype = ctypes.c_long
    lib.zvxk_sizeof.argtypes = [ctypes.c_char_p]
    lib.zvxk_offsetof.restype = ctypes.c_long
    lib.zvxk_offsetof.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.zvxk_field.restype = ctypes.c_char_p
    lib.zvxk_field.argtypes = [ctypes.c_int, ctypes.c_int]
    for name, sig in OPS_SIG.items():
        getattr(lib, "zvxk_" + name).argtypes = [_SIG_TYPES[ch] for ch in sig]
    return lib


# The small kernels of ops.hip (tests/ops_ref.py): zvxk_<name> takes launch_<name>'s parameters without the stream, one letter per
# parameter: p pointer, i int, f float, l long, z size_t.  Defaulted trailing parameters of a launcher follow in its own order.
_SIG_TYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "l": ctypes.c_long, "z": ctypes.c_size_t}
OPS_SIG = {
    "cast": "pipiz", "f32_to_bf16": "ppz", "transpose16": "pipiiiip", "zero_tail_cols": "pilliiip", "split3": "pipiipii",
    "split3_weights": "ppliif", "absmax": "pzp", "embed": "pppipippiip", "layernorm": "piipiiiipiifppplppi",
    "softmax_rows": "pipiiiiip", "rowdot": "pipfpiipi", "bucket_embed_add": "ppipiipiip", "bucket_embed_add_ctl": "pppppipiipiip",
    "durations": "pppppiip", "durations_q16": "ppppppiip", "length_regulate": "pippppiiii", "add_pe_cast": "pppiiiipii",
    "instnorm_stats": "piiiipifpp", "norm_affine_act": "piipiiiipippppliif", "instnorm_fused": "piipiiiipifppppliif",
    "mel_pad": "piiippiiipii", "copy_rows_f32": "piilplliipi", "conv_post_tanh": "piilpfiipliiipipi", "count_sat16": "pliiipip",
    "zero_tail_rows": "piiipi", "spk_front": "pipippppppipiii", "se_pool_splits": "ii", "se_pool": "piiiipip", "se_fc": "piipppppiipip",
    "se_apply": "pppipiiipi", "asp_pool": "pipiiipipi", "l2norm_rows": "pii", "reflect_pad": "plppliii", "stft_mag": "pipiiiip",
    "log_clip": "piifiip", "fc_rows": "pipippiiii", "math_probe": "ippi",
}


# ------------------------------------------------------------------------------------------------------------------------------
# problems: a descriptor (GemmArgs field names; pointer fields name a host array) + host arrays
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_DEFAULTS = dict(x_bs=0, x_hs=0, w_bs=0, w_hs=0, w_ts=0, fused=0, slope1=0.0, no_pairstream=0, nbatch=1, nheads=1, in_len_static=0, ntaps=1,
                     du=[0] * MAX_TAPS, dv=[0] * MAX_TAPS, dv1=[0] * MAX_TAPS, stride=1, wout=0, hin=1, win=0, bflat=0, x2_bs=0, ldx2=0, K2=0,
                     xcd_flat=1, slab_small=0, out_split3=0, alpha=1.0, bias_mode=0, r_bs=0, r_hs=0, ldr=0, res_mode=0, res_inv_slope=10.0,
                     a_bs=0, lda=0, accum_mode=0, accum_dtype=DT_F32, out_scale=1.0, act=ACT_NONE, slope=1.0, o_bs=0, o_hs=0)


class Problem:
    """One launch: `d` holds GemmArgs / FlashArgs / AttnF32Args fields; `bufs` maps a pointer field to (host values as float64 or
    raw bits, dtype, role).  role 'in' buffers are uploaded; 'out' buffers are pre-filled with the sentinel and read back."""

    def __init__(self, kind, d):
        self.kind, self.d, self.bufs = kind, d, {}
        self.sample = None              # gemm: {b: sorted output rows} compared (None: every valid row)
        self.utts = None                # gemm: the utterances the reference covers (None: all of them)
        self.raw = {}                   # output field -> the reference before the output cast (f16 saturation checks)

    def add(self, field, values, dt, role="in", bits=None):
        self.bufs[field] = dict(v=values, dt=dt, role=role, bits=bits)


def _rng(seed):
    return np.random.default_rng(seed)


def _fill_rows(buf_bits, dt, n_elems):
    return np.full(n_elems, nan_bits(dt), bits_dtype(dt))


def lens_of(d, key, nb, default):
    v = d.get(key)
    return list(v) if v is not None else [default] * nb


def row_map(d, b, rows, tap):
    """Input row (within utterance b) and validity of output rows `rows` for tap index `tap`: the GemmArgs row map."""
    in_len = lens_of(d, "in_len", d["nbatch"], d["in_len_static"])[b]
    rows = np.asarray(rows, np.int64)
    if d.get("_flat"):                                  # flattened 2-D map (launch_gemm's 9-tap path): tap offset du * win + dv
        fw, fr = d["win"], d["hin"] * d["win"]
        g = rows + d["du"][tap] * fw + d["dv"][tap]
        v = (rows % fw) + d["dv"][tap]
        ok = (g >= 0) & (g < fr) & (v >= 0) & (v < in_len)
        return g, ok
    if d["wout"] > 0:
        u, v = rows // d["wout"], rows % d["wout"]
        iu, iv = u * d["stride"] + d["du"][tap], v * d["stride"] + d["dv"][tap]
        ok = (iu >= 0) & (iu < d["hin"]) & (iv >= 0) & (iv < in_len)
        return iu * d["win"] + iv, ok
    iu, iv = d["du"][tap], rows + d["dv"][tap]
    ok = (iu >= 0) & (iu < d["hin"]) & (iv >= 0) & (iv < in_len)
    return iu * max(d["win"], 0) + iv, ok


def valid_out_rows(d, b):
    """Output rows of utterance b that the contract defines (everything else is either untouched or, where the contract says so, junk)."""
    M = d["M"]
    r = np.arange(M)
    if d.get("_flat"):
        in_len = lens_of(d, "in_len", d["nbatch"], d["in_len_static"])[b]
        return r[(r % d["win"]) < in_len]
    ol = lens_of(d, "out_len", d["nbatch"], M)[b]
    if d["wout"] > 0:
        return r[(r % d["wout"]) < ol]
    return r[r < min(ol, M)]


def grid(a):
    """The largest power of two every finite nonzero value of `a` is a multiple of (inf for none)."""
    a = np.asarray(a, np.float64)
    a = a[np.isfinite(a) & (a != 0)]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(np.abs(a))
    ints = np.round(m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((ints & -ints).astype(np.float64), e - 53)))


def exact_f32(mag, g):
    """True when every partial sum of terms that are multiples of g, bounded by mag, is exact in fp32 (|sum| <= 2^24 g):
    accumulation in any order then has no rounding error at all."""
    return mag.size == 0 or float(np.max(mag)) <= 2.0 ** 24 * g


def _conv(d, Xv, x_off, ldx, Wv, w_off, w_ts, ldw, b, rows, taps_dv, K, N, in_len_override=None, mut=None, drop_tap=None, shift_tap=None, zero_k=None):
    """sum_tap X[rowmap(r, tap)][k] W[tap][n][k], sum |.| and the grid of the products for output rows `rows` of utterance b."""
    gmin = np.inf
    acc = np.zeros((len(rows), N))
    mag = np.zeros((len(rows), N))
    dd = dict(d)
    dd["dv"] = taps_dv
    if in_len_override is not None:
        dd["in_len"] = in_len_override
    kidx = np.arange(K)
    for t in range(d["ntaps"]):
        if drop_tap == t:
            continue
        if shift_tap == t:
            dd2 = dict(dd)
            dd2["dv"] = list(taps_dv)
            dd2["dv"][t] += 1
            g, ok = row_map(dd2, b, rows, t)
        else:
            g, ok = row_map(dd, b, rows, t)
        gi = np.where(ok, g, 0)
        xg = Xv[x_off + gi[:, None] * ldx + kidx[None, :]]
        xg = np.where(ok[:, None], xg, 0.0)
        if zero_k is not None:
            xg[:, zero_k[0]:zero_k[1]] = 0.0
        wt = Wv[w_off + t * w_ts + np.arange(N)[:, None] * ldw + kidx[None, :]]
        acc += xg @ wt.T
        mag += np.abs(xg) @ np.abs(wt).T
        gmin = min(gmin, grid(xg) * grid(wt))
    return acc, mag, gmin


def gemm_ref(p, mut=None):
    """Reference of one GemmArgs launch.  Returns {field: (ref, tol, mask)} for every output buffer ('out', 'accum', 'ds_out'),
    each an array over the whole buffer (mask: elements the contract defines).  `mut` applies one of MUTATIONS to the reference."""
    d = p.d
    if d.get("fused"):
        return _fused_ref(p, mut)
    nb, nh, M, N, K = d["nbatch"], d["nheads"], d["M"], d["N"], d["K"]
    X, W = p.bufs["X"]["v"], p.bufs["W"]["v"]
    in_len = lens_of(d, "in_len", nb, d["in_len_static"])
    res = {}
    outs = {}
    for f in ("out", "accum", "ds_out"):
        if f in p.bufs:
            n = len(p.bufs[f]["bits"])
            outs[f] = [np.zeros(n), np.zeros(n), np.zeros(n, bool)]
    for b in range(nb):
        if p.utts is not None and b not in p.utts:
            continue
        rows = valid_out_rows(d, b)
        if p.sample is not None:
            rows = np.intersect1d(rows, p.sample[b])
        if len(rows) == 0:
            continue
        for h in range(nh):
            Kb = K
            if d.get("k_len") is not None:
                Kb = min(K, (d["k_len"][b] + 7) & ~7)
            il = list(in_len)
            if mut == "in_len_minus1":
                il[b] = max(0, il[b] - 1)
            zero_k = None
            if mut == "zero_last_k":
                zero_k = (max(0, Kb - 16), Kb)
            acc, mag, g = _conv(d, X, b * d["x_bs"] + h * d["x_hs"], d["ldx"], W, b * d["w_bs"] + h * d["w_hs"], d["w_ts"], d["ldw"], b, rows,
                             d["dv"], Kb, N, in_len_override=il, drop_tap=0 if mut == "drop_tap" else None,
                             shift_tap=(d["ntaps"] - 1) if mut == "shift_tap" else None, zero_k=zero_k)
            nterms = d["ntaps"] * Kb
            if d["K2"]:
                X2 = p.bufs["X2"]["v"]
                W2 = p.bufs["W2"]["v"]
                d1 = dict(d, ntaps=1, dv=[0] * MAX_TAPS, du=[0] * MAX_TAPS, in_len=il)
                a2, m2, g2 = _conv(d1, X2, b * d["x2_bs"], d["ldx2"], W2, 0, 0, d["K2"], b, rows, [0] * MAX_TAPS, d["K2"], N)
                acc += a2
                mag += m2
                g = min(g, g2)
                nterms += d["K2"]
            _epilogue(p, b, h, rows, acc, mag, nterms, outs, mut, acc_exact=exact_f32(mag, g))
    if d.get("ds_out"):
        _ds_ref(p, outs, mut)
    for f, (r, t, m) in outs.items():
        res[f] = (r, t, m)
    return res


def _epilogue(p, b, h, rows, acc, mag, nterms, outs, mut, tmag_extra=None, acc_exact=False):
    d = p.d
    N = d["N"]
    cols = np.arange(N)
    v = acc * d["alpha"]
    err = (0.0 if acc_exact else 2 * nterms * U) * mag * abs(d["alpha"])
    if tmag_extra is not None:
        err = err + tmag_extra
    epi_mag = np.abs(v)
    if d["bias_mode"] == 1 and mut != "drop_bias":
        v = v + p.bufs["bias"]["v"][None, :N]
        epi_mag = epi_mag + np.abs(p.bufs["bias"]["v"][None, :N])
    elif d["bias_mode"] == 2 and mut != "drop_bias":
        v = v + p.bufs["bias"]["v"][rows][:, None]
        epi_mag = epi_mag + np.abs(p.bufs["bias"]["v"][rows][:, None])
    if d["res_mode"]:
        R = p.bufs["res"]["v"]
        rr = R[b * d["r_bs"] + h * d["r_hs"] + rows[:, None] * d["ldr"] + cols[None, :]]
        if d["res_mode"] == 2:
            s = d["res_inv_slope"] * (0.5 if mut == "res_slope" else 1.0)
            rr = np.where(rr >= 0, rr, rr * s)
        elif mut == "res_slope":
            rr = np.where(rr >= 0, rr, rr * 0.5)
        v = v + rr
        epi_mag = epi_mag + np.abs(rr)
    if d["accum_mode"]:
        A = p.bufs["accum"]
        ai = b * d["a_bs"] + rows[:, None] * d["lda"] + cols[None, :]
        if d["accum_mode"] & 1 and mut != "skip_accum":
            av = A["v"][ai]
            v = v + av
            epi_mag = epi_mag + np.abs(av)
        err = err + 4 * U * epi_mag
        if d["accum_mode"] & 2:
            o = outs["accum"]
            adt = d["accum_dtype"]
            _store(p, "accum", o, ai, v, err, adt, mut)
    if "out" not in outs or not d.get("_has_out", True):
        return
    err = err + 4 * U * epi_mag
    v = v * d["out_scale"]
    err = err * abs(d["out_scale"])
    if d["act"] == ACT_RELU:
        v = np.maximum(v, 0)
    elif d["act"] == ACT_LRELU:
        v = np.where(v >= 0, v, v * d["slope"])
    if d.get("post_scale") is not None and "post_scale" in p.bufs:
        ps, pt = p.bufs["post_scale"]["v"][None, :N], p.bufs["post_shift"]["v"][None, :N]
        v = v * ps + pt
        err = err * np.abs(ps) + 2 * U * (np.abs(v) + np.abs(pt))
    o = outs["out"]
    odt = d["out_dtype"]
    if d["out_split3"]:
        # [hi | hi | lo] planes of the f32 result: compared after reconstruction (test side), so the reference holds v at plane 0
        oi = b * d["o_bs"] + h * d["o_hs"] + rows[:, None] * d["ldo"] + cols[None, :]
        o[0][oi] = v
        o[1][oi] = err + 2.0 ** -17 * np.abs(v) + 2.0 ** -30
        o[2][oi] = True
        return
    oi = b * d["o_bs"] + h * d["o_hs"] + rows[:, None] * d["ldo"] + cols[None, :]
    _store(p, "out", o, oi, v, err, odt, mut)


def trunc_to(x, dt):
    """x cast to 16-bit dtype dt by truncation toward zero (the 'truncate the output cast' mutation)."""
    q = round_to(x, dt)
    if dt == DT_F32:
        return q
    over = np.abs(q) > np.abs(x)
    if dt == DT_BF16:
        down = bf16_from_bits(np.where(over, bf16_bits(q.astype(np.float32)) - 1, bf16_bits(q.astype(np.float32))).astype(np.uint16))
    else:
        down = np.nextafter(q.astype(np.float16), np.float16(0)).astype(np.float64)
    return np.where(over, down, q)


def _store(p, f, o, idx, v, err, dt, mut):
    """Reference, bound and mask of output elements `idx` holding the f32-class value v (error bound err) after the cast to dt:
    |Q(v_kernel) - v| <= |Q(v_kernel) - v_kernel| + err <= half_ulp(|v| + err) + err  (f16 clamps to +-65504 first; the clamp is
    1-Lipschitz)."""
    ref = np.clip(v, -F16_MAX, F16_MAX) if dt == DT_F16 else v
    o[1][idx] = err + half_ulp(np.abs(ref) + err, dt)
    if mut == "truncate_cast":
        ref = trunc_to(ref, dt)
    o[0][idx] = ref
    o[2][idx] = True
    raw = p.raw.setdefault(f, np.zeros(len(o[0])))
    raw[idx] = v


def _ds_ref(p, outs, mut):
    """conv2d_s2's fused 1 x 1 / stride-2 shortcut: ds[r][n] = sum_k X[2u][2v][k] Wds[n][k] + ds_bias[n] as 16 bit."""
    d = p.d
    N, K = d["N"], d["K"]
    Xv, Wd, bd = p.bufs["X"]["v"], p.bufs["ds_W"]["v"], p.bufs["ds_bias"]["v"]
    o = outs["ds_out"]
    for b in range(d["nbatch"]):
        if p.utts is not None and b not in p.utts:
            continue
        rows = valid_out_rows(d, b)
        d1 = dict(d, ntaps=1, du=[0] * MAX_TAPS, dv=[0] * MAX_TAPS)
        acc, mag, g = _conv(d1, Xv, b * d["x_bs"], d["ldx"], Wd, 0, 0, K, b, rows, [0] * MAX_TAPS, K, N)
        v = acc + (0 if mut == "drop_bias" else bd[None, :N])
        err = (0.0 if exact_f32(mag, g) else 2 * K * U) * mag + 4 * U * np.abs(v)
        oi = b * d["o_bs"] + rows[:, None] * d["ldo"] + np.arange(N)[None, :]
        _store(p, "ds_out", o, oi, v, err, DT_BF16, mut)


def _fused_ref(p, mut):
    """Fused ResBlock pair.  resfuse / pairstream (fused 1): out = epi(conv2(T) + b2 + inv_lrelu(X)), T = Q16(lrelu(conv1(X) + b1, slope1));
    rb2fuse (fused 2): T = Q16(lrelu(conv1(X) + b1 + inv_lrelu(X), slope1)), out = epi(conv2(T) + b2 + inv_lrelu(T)).  T is zero
    outside [0, in_len) (conv2 zero-pads its input)."""
    d = p.d
    nb, M, C = d["nbatch"], d["M"], d["N"]
    dt = d["dtype"]
    X, W1, W2 = p.bufs["X"]["v"], p.bufs["W1"]["v"], p.bufs["W"]["v"]
    b1 = p.bufs["bias1"]["v"]
    in_len = lens_of(d, "in_len", nb, M)
    outs = {}
    for f in ("out", "accum"):
        if f in p.bufs:
            n = len(p.bufs[f]["bits"])
            outs[f] = [np.zeros(n), np.zeros(n), np.zeros(n, bool)]
    rinv = d["res_inv_slope"]
    for b in range(nb):
        if p.utts is not None and b not in p.utts:
            continue
        il = list(in_len)
        if mut == "in_len_minus1":
            il[b] = max(0, il[b] - 1)
        allr = np.arange(M)
        a1, m1, g1 = _conv(d, X, b * d["x_bs"], d["ldx"], W1, 0, C * C, C, b, allr, d["dv1"], C, C, in_len_override=il)
        t = a1 + b1[None, :C]
        tmag = m1 + np.abs(b1[None, :C])
        gt = min(g1, grid(b1[:C]))
        xr = X[b * d["x_bs"] + allr[:, None] * d["ldx"] + np.arange(C)[None, :]]
        xr = np.where((allr < il[b])[:, None], xr, 0.0)
        if d["fused"] == 2:
            xi = np.where(xr >= 0, xr, xr * rinv)
            t = t + xi
            tmag = tmag + np.abs(xi)
            gt = min(gt, grid(xi))
        # fp32 error of t: none where the data make every partial sum exact, else accumulation + epilogue additions
        e1 = 0.0 * tmag if exact_f32(m1, g1) and exact_f32(tmag, gt) else 2 * d["ntaps"] * C * U * m1 + 4 * U * tmag
        s1 = d["slope1"]
        t = np.where(t >= 0, t, t * s1)
        if np.frexp(s1)[0] != 0.5:                               # leaky-relu by a slope that is no power of two rounds once more
            e1 = e1 + U * np.abs(t)
        T = round_to(t, dt)
        # the kernel's T is Q(t_kernel) with |t_kernel - t| <= e1 (leaky-relu is 1-Lipschitz): it differs from Q(t) only where a
        # rounding boundary of the 16-bit type lies within e1 of t, and then by the gap between the two candidates
        eT = round_to(t + e1, dt) - round_to(t - e1, dt)
        inside = (allr < il[b])[:, None]
        T = np.where(inside, T, 0.0)
        eT = np.where(inside, eT, 0.0)
        rows = valid_out_rows(d, b)
        rows = rows[rows < M]
        if len(rows) == 0:
            continue
        # conv2 over T (rows of T are utterance rows; T is zero outside [0, in_len) already)
        Tflat = T.reshape(-1)
        dd = dict(d, in_len=[M] * nb, nbatch=nb)
        zero_k = (C - 16, C) if mut == "zero_last_k" else None
        acc, mag, g2 = _conv(dd, Tflat, 0, C, W2, 0, C * C, C, b, rows, d["dv"], C, C, drop_tap=0 if mut == "drop_tap" else None,
                         shift_tap=(d["ntaps"] - 1) if mut == "shift_tap" else None, zero_k=zero_k)
        if mut == "seam_halo" and il[b] > PAIR_SEG:
            # the first row of the streaming pair kernel's second segment computed as if nothing lay in front of it
            Tz = T.copy()
            Tz[:PAIR_SEG] = 0.0
            az, _, _ = _conv(dd, Tz.reshape(-1), 0, C, W2, 0, C * C, C, b, np.array([PAIR_SEG]), d["dv"], C, C)
            acc[rows == PAIR_SEG] = az
        eprop, _, _ = _conv(dd, eT.reshape(-1), 0, C, np.abs(W2), 0, C * C, C, b, rows, d["dv"], C, C)
        # residual: inverse leaky-relu of X (resfuse) or of T (rb2fuse), folded into the bias term below
        rsrc = T[rows] if d["fused"] == 2 else xr[rows]
        s = rinv * (0.5 if mut == "res_slope" else 1.0)
        rv = np.where(rsrc >= 0, rsrc, rsrc * s)
        extra = eprop + 4 * U * np.abs(rv)
        if d["fused"] == 2:
            extra = extra + eT[rows] * max(1.0, rinv)
        sub = Problem("gemm", dict(d, res_mode=0, fused=0))
        sub.bufs, sub.raw = p.bufs, p.raw
        acc = acc + rv / d["alpha"]
        exact2 = exact_f32(mag, g2)
        if d["fused"] == 1 and d["accum_mode"] and C in (32, 64):
            # KNOWN DEVIATION (resfuse_persist_kernel, variants 16 / 17): with a running sum the kernel rounds y = conv2 + b2 + x to the
            # 16-bit type before it adds the running sum and scales; the contract's epilogue keeps y in f32.  Modelled here so the
            # rest of the launch stays held to the tight bound (measured: up to 0.7 ulp of the output otherwise)
            bias2 = 0.0 if mut == "drop_bias" else p.bufs["bias"]["v"][None, :C]
            y = acc + bias2
            ey = (0.0 if exact2 else 2 * d["ntaps"] * C * U) * mag + extra + 4 * U * (np.abs(y) + np.abs(bias2))
            acc = round_to(y, dt) - bias2
            extra = round_to(y + ey, dt) - round_to(y - ey, dt)
            exact2 = True
        _epilogue(sub, b, 0, rows, acc, mag, d["ntaps"] * C, outs, mut, tmag_extra=extra, acc_exact=exact2)
    return {f: tuple(v) for f, v in outs.items()}


def attn_ref(p, mut=None):
    """softmax(Q K^T * scale, keys < len) V per (utterance, head) for query rows < len; FlashArgs (16-bit) or AttnF32Args (f32)."""
    d = p.d
    D, nh, nb = d["D"], d["nheads"], d["nbatch"]
    flash = p.kind == "flash"
    dt = (DT_F16 if d["f16"] else DT_BF16) if flash else DT_F32
    lens = list(d["_lens"])
    n = len(p.bufs["out"]["bits"])
    ref, tol, mask = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    planes = None
    if not flash and "planes" in p.bufs:
        planes = [np.zeros(len(p.bufs["planes"]["bits"])), np.zeros(len(p.bufs["planes"]["bits"])), np.zeros(len(p.bufs["planes"]["bits"]), bool)]
    scale = d["scale"]
    for b in range(nb):
        L = lens[b]
        Lk = L - 1 if mut == "len_minus1" else (L + 1 if mut == "len_plus1" else L)
        Lk = max(1, Lk)
        q = np.arange(L)
        dk = np.arange(D)
        for h in range(nh):
            if flash:
                QK = p.bufs["qk"]["v"]
                base = b * d["qk_bs"]
                Q = QK[base + q[:, None] * d["ldq"] + h * D + dk[None, :]]
                kk = np.arange(Lk)
                Kt = QK[base + kk[:, None] * d["ldq"] + d["k_off"] + h * D + dk[None, :]]
                VT = p.bufs["vt"]["v"]
                V = VT[b * d["vt_bs"] + (h * D + dk)[None, :] * d["ldv"] + kk[:, None]]
            else:
                QKV = p.bufs["qkv"]["v"]
                base = b * d["bs"]
                kk = np.arange(Lk)
                Q = QKV[base + q[:, None] * d["ld"] + d["q_off"] + h * D + dk[None, :]]
                Kt = QKV[base + kk[:, None] * d["ld"] + d["k_off"] + h * D + dk[None, :]]
                V = QKV[base + kk[:, None] * d["ld"] + d["v_off"] + h * D + dk[None, :]]
            S = (Q @ Kt.T) * scale
            ds = 2 * D * U * (np.abs(Q) @ np.abs(Kt).T) * abs(scale) + 4 * U * np.abs(S)
            m = S.max(axis=1, keepdims=True)
            E = np.exp(S - m)
            P = E / E.sum(axis=1, keepdims=True)
            O = P @ V
            PV = P @ np.abs(V)
            eps_p = (2.0 ** -8 if dt == DT_BF16 else 2.0 ** -11) if flash else 8 * U
            dsm = ds.max(axis=1, keepdims=True)
            err = (2 * eps_p + 4 * dsm + 2 * Lk * U + 2 * D * U) * (PV + np.abs(O))
            oi = b * d["o_bs"] + q[:, None] * d["ldo"] + h * D + dk[None, :]
            ref[oi] = O
            tol[oi] = err + half_ulp(np.abs(O) + err, dt)
            mask[oi] = True
            if planes is not None:
                C = d["planes_C"]
                pi = b * (d["L_rows"] * 3 * C) + q[:, None] * (3 * C) + h * D + dk[None, :]
                planes[0][pi] = O
                planes[1][pi] = err + 2 * half_ulp(np.abs(O), DT_F32) + 2.0 ** -17 * np.abs(O) + 2.0 ** -30
                planes[2][pi] = True
    res = {"out": (ref, tol, mask)}
    if planes is not None:
        res["planes"] = tuple(planes)
    return res


MUTATIONS = ["drop_tap", "shift_tap", "zero_last_k", "in_len_minus1", "res_slope", "drop_bias", "skip_accum", "truncate_cast", "seam_halo"]
PAIR_SEG = 1024                    # launch_pairstream's segment floor (rows)


def applicable_mutations(p):
    d = p.d
    m = ["drop_tap", "shift_tap", "zero_last_k", "in_len_minus1"]
    if d.get("res_mode") or d.get("fused"):
        m.append("res_slope")
    if d.get("bias_mode") or d.get("ds_out"):
        m.append("drop_bias")
    if d.get("accum_mode", 0) & 1:
        m.append("skip_accum")
    stored16 = (d.get("_has_out", True) and "out" in p.bufs and d["out_dtype"] != DT_F32) or d.get("ds_out") or \
        (d.get("accum_mode", 0) & 2 and d["accum_dtype"] != DT_F32)
    if stored16:
        m.append("truncate_cast")
    if d.get("fused") == 1 and d["N"] == 128 and max(d["in_len"]) > PAIR_SEG:
        m.append("seam_halo")
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# case construction
# ------------------------------------------------------------------------------------------------------------------------------
def taps_1d(k, dil=1):
    return [(i - (k - 1) // 2) * dil for i in range(k)]


def _pad_taps(t):
    return list(t) + [0] * (MAX_TAPS - len(t))


def _rand(rng, n, scale=1.0):
    return rng.standard_normal(n) * scale


def make_gemm(name, seed=0, *, dtype, M, N, K, nbatch=1, nheads=1, lens=None, out_lens="same", taps=(0,), du=None, stride=1, wout=0, hin=1, win=0,
              ldx=None, ldo=None, ldw=None, packed=True, bias_mode=1, act=ACT_NONE, slope=0.2, alpha=1.0, res_mode=0, res_dtype=None,
              res_inv_slope=10.0, accum_mode=0, accum_dtype=None, out_scale=1.0, post=False, out_dtype=None, has_out=True, K2=0,
              bflat=0, xcd_flat=1, slab_small=0, out_split3=0, k_len=None, flat=False, ds=False, fused=0, dil1=1, slope1=0.1,
              no_pairstream=0, row_gap=0, sample=None, x_scale=1.0, big=False, bias_scale=0.5, grid_data=None, aux_scale=1.0):
    """A GemmArgs problem in the production memory layout: X [b][rows][ldx] (rows = bflat or M + row_gap; with ldx < K the rows overlap:
    X [b][x_bs] holds (M + row_gap - 1) ldx + K elements per utterance, the frame GEMM of the log-mel front end), W [tap][N][ldw],
    out / res / accum [b][rows][ld].  Rows past in_len (and columns past K) hold NaN; output buffers are sentinel-filled by the runner."""
    rng = _rng(seed)
    # grid data (the fused pairs by default): small multiples of powers of two and sparse weights, so that every fp32 partial sum of
    # both convolutions is exact -- the kernel's 16-bit intermediate is then determined, and the bound keeps only the output cast
    grid_data = bool(fused) if grid_data is None else grid_data
    if grid_data:
        res_inv_slope, slope1 = 8.0, 0.125

    def rnd(shape, scale, kind):
        if not grid_data:
            return _rand(rng, shape, scale)
        if kind == "w":
            return rng.integers(-2, 3, shape) / 64.0 * (rng.random(shape) < 0.15)
        return rng.integers(-4, 5, shape) / (4.0 if kind == "x" else 16.0) * scale
    out_dtype = dtype if out_dtype is None else out_dtype
    res_dtype = dtype if res_dtype is None else res_dtype
    accum_dtype = dtype if accum_dtype is None else accum_dtype
    lens = [M] * nbatch if lens is None else list(lens)
    ntaps = len(taps)
    du = [0] * ntaps if du is None else list(du)
    ldx = K if ldx is None else ldx
    ldo = N if ldo is None else ldo
    ldw = K if ldw is None else ldw
    two_d = wout > 0
    if two_d:
        xrows = hin * win
    else:
        xrows = bflat if bflat else M + row_gap
    orows = bflat if bflat else M + row_gap
    d = dict(GEMM_DEFAULTS)
    d.update(name=name, dtype=dtype, M=M, N=N, K=K, nbatch=nbatch, nheads=nheads, ldx=ldx, ldw=ldw, ldo=ldo, ntaps=ntaps,
             du=_pad_taps(du), dv=_pad_taps(taps), stride=stride, wout=wout, hin=hin, win=win, bias_mode=bias_mode, act=act, slope=slope,
             alpha=alpha, res_mode=res_mode, res_dtype=res_dtype, res_inv_slope=res_inv_slope, accum_mode=accum_mode, accum_dtype=accum_dtype,
             out_scale=out_scale, out_dtype=out_dtype, bflat=bflat, xcd_flat=xcd_flat, slab_small=slab_small, out_split3=out_split3,
             in_len=lens, fused=fused, slope1=slope1, no_pairstream=no_pairstream, _flat=flat, _has_out=has_out)
    if out_lens == "same":
        d["out_len"] = None if flat else (list(lens) if not two_d else [(l + stride - 1) // stride for l in lens])
    else:
        d["out_len"] = out_lens
    if k_len is not None:
        d["k_len"] = list(k_len)
    d["x_bs"] = xrows * ldx
    overlap = ldx < K                                   # rows that overlap (frames of a signal, hop = ldx): X is a signal per utterance
    if overlap:
        assert not two_d and not bflat and ntaps == 1 and k_len is None and not K2 and not fused
        d["x_bs"] = ((xrows - 1) * ldx + K + 3 & ~3) + 4
        while d["x_bs"] % ldx == 0:                     # ... whose stride is no multiple of ldx: no row of one utterance is a row of the next
            d["x_bs"] += 4
    d["o_bs"] = orows * ldo * (3 if out_split3 else 1) if not two_d else M * ldo
    if out_split3:
        d["ldo"] = 3 * N
        d["o_bs"] = orows * 3 * N
    p = Problem("gemm", d)
    # X: valid rows random, masked rows NaN; columns past K NaN
    X = np.full((nbatch, d["x_bs"]) if overlap else (nbatch, xrows, ldx), np.nan)
    for b in range(nbatch):
        if overlap:                                     # (lens - 1) ldx + K readable elements, NaN behind the last of them
            X[b, :(lens[b] - 1) * ldx + K] = rnd((lens[b] - 1) * ldx + K, x_scale, "x")
        elif two_d:
            for u in range(hin):
                X[b, u * win:u * win + lens[b], :K] = _rand(rng, (lens[b], K), x_scale)
        else:
            X[b, :lens[b], :K] = rnd((lens[b], K), x_scale, "x")
            if k_len is not None:
                kl = k_len[b]
                X[b, :lens[b], kl:(kl + 7) & ~7] = 0.0            # read (k_len rounds up to 8) and zero by contract
                X[b, :lens[b], (kl + 7) & ~7:] = np.nan
    X = round_to(X, dtype)
    wsc = 1.0 / np.sqrt(K * ntaps + K2)
    W = round_to(rnd((ntaps, N, ldw), wsc, "w"), dtype)
    W[:, :, K:] = np.nan
    if k_len is not None:
        # W per utterance (w_bs): keys past roundup8(k_len) hold NaN, [k_len, roundup8) zero
        Wb = round_to(_rand(rng, (nbatch, N, ldw), wsc), dtype)
        for b in range(nbatch):
            kl = k_len[b]
            Wb[b, :, kl:(kl + 7) & ~7] = 0.0
            Wb[b, :, (kl + 7) & ~7:] = np.nan
        W = Wb
        d["w_bs"] = N * ldw
        d["ntaps"] = 1
    d["w_ts"] = N * ldw
    p.add("X", X.reshape(-1), dtype)
    p.add("W", W.reshape(-1), dtype)
    if packed and dtype != DT_F32:
        p.add("Wp", None, dtype, role="packed")
    if bias_mode:
        nbias = M if bias_mode == 2 else N
        bias = rnd(((nbias + 7) // 8) * 8 + 8, bias_scale, "b").astype(np.float32).astype(np.float64)
        p.add("bias", bias, DT_F32)
    if res_mode:
        R = np.full((nbatch, orows, ldo), np.nan)
        for b in range(nbatch):
            R[b, :M if two_d else min(M, orows)] = _rand(rng, (M if two_d else min(M, orows), ldo), aux_scale)
        d["ldr"], d["r_bs"] = ldo, orows * ldo
        p.add("res", round_to(R, res_dtype).reshape(-1), res_dtype)
    if accum_mode:
        A = np.full((nbatch, orows, ldo), np.nan)
        A[:, :, :] = rnd((nbatch, orows, ldo), aux_scale, "x") if accum_mode & 1 else np.nan
        d["lda"], d["a_bs"] = ldo, orows * ldo
        if accum_mode & 1:
            p.add("accum", round_to(A, accum_dtype).reshape(-1), accum_dtype, role="inout")
        else:
            p.add("accum", None, accum_dtype, role="out")
        p.bufs["accum"]["n"] = nbatch * orows * ldo
    if post:
        p.add("post_scale", round_to(rng.uniform(0.5, 1.5, N + 8), DT_F32), DT_F32)
        p.add("post_shift", round_to(_rand(rng, N + 8, 0.3), DT_F32), DT_F32)
        d["post_scale"] = True
    if has_out:
        p.add("out", None, out_dtype, role="out")
        p.bufs["out"]["n"] = nbatch * (d["o_bs"] if not two_d else M * ldo)
    if K2:
        X2 = np.full((nbatch, xrows, K2), np.nan)
        for b in range(nbatch):
            X2[b, :lens[b]] = _rand(rng, (lens[b], K2))
        d["K2"], d["ldx2"], d["x2_bs"] = K2, K2, xrows * K2
        p.add("X2", round_to(X2, dtype).reshape(-1), dtype)
        p.add("W2", round_to(_rand(rng, (1, N, K2), wsc), dtype).reshape(-1), dtype)
    if fused:
        d["dv1"] = _pad_taps(taps_1d(ntaps, dil1))
        p.add("W1", round_to(rnd((ntaps, N, K), 1.0 / np.sqrt(K * ntaps), "w"), dtype).reshape(-1), dtype)
        p.add("bias1", round_to(rnd(N + 8, 0.3 if not grid_data else bias_scale, "b"), DT_F32), DT_F32)
        # the block input lives in the activated domain: lrelu(x) with slope 1 / res_inv_slope
        Xa = X.copy()
        Xa = np.where(Xa >= 0, Xa, Xa / res_inv_slope)
        p.bufs["X"]["v"] = round_to(Xa, dtype).reshape(-1)
        d["res_mode"], d["ldr"], d["r_bs"] = 2, ldx, d["x_bs"]
        p.bufs["res"] = dict(alias="X")
    if ds:
        p.add("ds_W", round_to(_rand(rng, (1, N, K), 1.0 / np.sqrt(K)), dtype).reshape(-1), dtype)
        p.add("ds_bias", round_to(_rand(rng, N + 8, 0.3), DT_F32), DT_F32)
        p.add("ds_out", None, DT_BF16, role="out")
        p.bufs["ds_out"]["n"] = nbatch * M * ldo
        d["ds_out"] = True
    if big:
        p.big = True
    if sample is not None:
        p.sample = sample
    elif big or nbatch * M > 4096:
        p.sample = boundary_sample(d, lens)
    for f in ("out", "accum", "ds_out"):
        if f in p.bufs and p.bufs[f].get("role") in ("out", "inout"):
            dtf = p.bufs[f]["dt"]
            n = p.bufs[f]["n"]
            p.bufs[f]["bits"] = np.full(n, sentinel_bits(dtf), bits_dtype(dtf)) if p.bufs[f]["v"] is None else to_bits(p.bufs[f]["v"], dtf)
            if p.bufs[f]["v"] is not None:
                p.bufs[f]["bits"] = np.where(np.isnan(p.bufs[f]["v"]), sentinel_bits(dtf), p.bufs[f]["bits"]).astype(bits_dtype(dtf))
    return p


def make_heads(name, seed=0, *, dtype, kind, lens, nheads=2, dh=40):
    """The unfused attention products with heads, in zvx.hip's layouts plus gaps: rows between utterances, rows (or columns)
    between heads, padded leading dimensions -- every gap stays sentinel / NaN.
      kind 'qk': scores[b][h][q][k] = alpha Q[b][q][h dh:] . K[b][k][h dh:]   (x_hs = w_hs = dh columns, f32 output, o_hs rows)
      kind 'pv': O[b][q][h (dh + 8):] = P[b][h][q][:] . V^T[b][h][:][:]         (k_len = len, o_hs = dh + 8 columns)"""
    rng = _rng(seed)
    B, Lmax = len(lens), max(lens)
    Lp = ((Lmax + 7) & ~7) + 8
    d = dict(GEMM_DEFAULTS)
    d.update(name=name, dtype=dtype, nbatch=B, nheads=nheads, M=Lmax, in_len=list(lens), out_len=list(lens), xcd_flat=1, bias_mode=0,
             res_dtype=dtype, out_dtype=dtype, _has_out=True)
    p = Problem("gemm", d)
    if kind == "qk":
        Ls, ldq = Lmax + 3, nheads * dh + 8
        Q = np.full((B, Ls, ldq), np.nan)
        Kb = np.full((B, Ls, ldq), np.nan)
        for b, l in enumerate(lens):
            Q[b, :l, :nheads * dh] = _rand(rng, (l, nheads * dh))
            Kb[b, :Lmax, :nheads * dh] = _rand(rng, (Lmax, nheads * dh))     # every key row < N is read (scores past len are masked later)
        hrows = Lmax + 2
        d.update(N=Lmax, K=dh, alpha=float(np.float32(1 / np.sqrt(dh))), ldx=ldq, x_bs=Ls * ldq, x_hs=dh, ldw=ldq, w_bs=Ls * ldq, w_hs=dh,
                 ldo=Lp, o_hs=hrows * Lp, o_bs=nheads * hrows * Lp + 3 * Lp, out_dtype=DT_F32)
        p.add("X", round_to(Q, dtype).reshape(-1), dtype)
        p.add("W", round_to(Kb, dtype).reshape(-1), dtype)
        n_out = B * d["o_bs"]
    else:
        hrows, vrows = Lmax + 2, dh + 2
        P = np.full((B, nheads, hrows, Lp), np.nan)
        VT = np.full((B, nheads, vrows, Lp), np.nan)
        for b, l in enumerate(lens):
            l8 = (l + 7) & ~7
            P[b, :, :l, :l] = rng.random((nheads, l, l)) / l
            P[b, :, :l, l:l8] = 0.0                       # read (k_len rounds up to 8) and zero by contract
            VT[b, :, :dh, :l] = _rand(rng, (nheads, dh, l))
            VT[b, :, :dh, l:l8] = 0.0
        ldo = nheads * (dh + 8)
        d.update(N=dh, K=Lp, k_len=list(lens), ldx=Lp, x_hs=hrows * Lp, x_bs=nheads * hrows * Lp, ldw=Lp, w_hs=vrows * Lp,
                 w_bs=nheads * vrows * Lp, ldo=ldo, o_hs=dh + 8, o_bs=(Lmax + 3) * ldo)
        p.add("X", round_to(P, dtype).reshape(-1), dtype)
        p.add("W", round_to(VT, dtype).reshape(-1), dtype)
        n_out = B * d["o_bs"]
    odt = d["out_dtype"]
    p.add("out", None, odt, role="out")
    p.bufs["out"]["n"] = n_out
    p.bufs["out"]["bits"] = np.full(n_out, sentinel_bits(odt), bits_dtype(odt))
    return p


def boundary_sample(d, lens, extra=24):
    """Output rows compared on a large launch: every 32-row block edge (the smallest tile height) and every utterance's first and
    last valid rows, plus a fixed random spread."""
    M = d["M"]
    rng = _rng(1234)
    s = {}
    for b, l in enumerate(lens):
        r = set()
        for e in range(0, M + 1, 32):
            r.update((e - 1, e))
        r.update((0, 1, l - 2, l - 1, l, M - 1))
        r.update(rng.integers(0, M, extra).tolist())
        s[b] = np.array(sorted(x for x in r if 0 <= x < M), np.int64)
    return s


def make_attn(name, seed=0, *, flash=True, f16=False, B=1, nheads=1, lens=(8,), L=None, ldq_pad=0, ldv_pad=0, ldo_pad=0, k_off_extra=0,
              planes=False, planes_f16=False):
    rng = _rng(seed)
    D = 264
    lens = list(lens)
    L = max(lens) if L is None else L
    H = nheads * D
    d = dict(name=name, D=D, nheads=nheads, nbatch=B, L=L, scale=float(np.float32(1.0 / np.sqrt(D))), _lens=lens)
    if flash:
        dt = DT_F16 if f16 else DT_BF16
        k_off = H + k_off_extra
        ldq = k_off + H + ldq_pad
        ldv = ((L + 7) & ~7) + ldv_pad
        ldo = H + ldo_pad
        d.update(ldq=ldq, k_off=k_off, qk_bs=L * ldq, ldv=ldv, vt_bs=H * ldv, ldo=ldo, o_bs=L * ldo, f16=int(f16), prof=0)
        QK = np.full((B, L, ldq), np.nan)
        VT = np.full((B, H, ldv), np.nan)
        for b, l in enumerate(lens):
            QK[b, :l, :H] = _rand(rng, (l, H), 1.5)
            QK[b, :l, k_off:k_off + H] = _rand(rng, (l, H), 1.5)
            VT[b, :, :l] = _rand(rng, (H, l))
            VT[b, :, l:] = 1000.0              # keys past len meet exactly-zero probabilities: finite junk must not leak
        p = Problem("flash", d)
        p.add("qk", round_to(QK, dt).reshape(-1), dt)
        p.add("vt", round_to(VT, dt).reshape(-1), dt)
        p.add("out", None, dt, role="out")
        p.bufs["out"]["n"] = B * L * ldo
    else:
        ld = 3 * H + ldq_pad
        q_off, k_off, v_off = 0, H + k_off_extra, 2 * H + k_off_extra
        ld = max(ld, v_off + H)
        ld = (ld + 3) & ~3
        ldo = H + ldo_pad
        d.update(ld=ld, q_off=q_off, k_off=k_off, v_off=v_off, bs=L * ld, ldo=ldo, o_bs=L * ldo, planes_C=H if planes else 0,
                 planes_f16=int(planes_f16), L_rows=L)
        Q = np.full((B, L, ld), np.nan)
        for b, l in enumerate(lens):
            Q[b, :l, :] = _rand(rng, (l, ld), 1.5)
        p = Problem("attn_f32", d)
        p.add("qkv", round_to(Q, DT_F32).reshape(-1), DT_F32)
        p.add("out", None, DT_F32, role="out")
        p.bufs["out"]["n"] = B * L * ldo
        if planes:
            p.add("planes", None, DT_F16 if planes_f16 else DT_BF16, role="out")
            p.bufs["planes"]["n"] = B * L * 3 * H
    for f in ("out", "planes"):
        if f in p.bufs:
            dtf = p.bufs[f]["dt"]
            p.bufs[f]["bits"] = np.full(p.bufs[f]["n"], sentinel_bits(dtf), bits_dtype(dtf))
    return p


# ------------------------------------------------------------------------------------------------------------------------------
# the case table: (name, make_gemm keyword arguments, expected variant id, expected compile-time epilogue or None)
# Shapes start from the production call sites of zvx.hip (encoder GEMMs, attention P.V, decoder convolutions, the vocoder's
# ConvTranspose / ResBlock launches, the speaker encoder) and move each along the edges its launcher decides on.
# ------------------------------------------------------------------------------------------------------------------------------
BF, H16, F32 = DT_BF16, DT_F16, DT_F32
RAG3 = [300, 1, 257]               # ragged batch with a length-1 utterance


def pair_seam_kw(dt, k, dil, am):
    kw = dict(dtype=dt, M=1100, N=128, K=128, nbatch=3, lens=[1100, 1025, 1], taps=taps_1d(k), dil1=dil, fused=1, no_pairstream=2)
    if am:
        kw.update(accum_mode=am, accum_dtype=dt)
    if am in (0, 1):
        kw.update(act=ACT_LRELU, slope=0.1, out_scale=1 / 3 if am else 1.0)
    else:
        kw.update(has_out=False)
    return kw


def _gemm_table():
    T = []

    def add(name, vid, epi=None, **kw):
        T.append((name, kw, vid, epi))

    # ---- gathered-row GEMM (no packed weights): 64 x 64 tiles for small launches, the three big tilings past 512 tiles ----
    for dt, vid in ((BF, 18), (H16, 18), (F32, 19)):
        n = DT_NAME[dt]
        add(f"small_linear_{n}", vid, dtype=dt, M=100, N=72, K=40, nbatch=3, lens=[100, 1, 65], packed=False, act=ACT_RELU, row_gap=5)
        # attention products with two heads, head strides and gaps between heads and utterances (zvx.hip's unfused path)
        T.append((f"qk_heads_{n}", dict(kind="qk", dtype=dt, lens=[70, 1, 33]), vid, None))
        T.append((f"pv_heads_klen_{n}", dict(kind="pv", dtype=dt, lens=[70, 1, 33]), 4 if dt == F32 else 1, None))   # (N = 40 < 64: no 64 x 64 tile)
        add(f"small_conv5_alpha_rowbias_{n}", vid, dtype=dt, M=70, N=64, K=24, nbatch=2, lens=[70, 33], taps=taps_1d(5, 2), packed=False,
            alpha=0.37, bias_mode=2, act=ACT_LRELU, slope=0.1)
        add(f"small_res_raw_post_{n}", vid, dtype=dt, M=65, N=68, K=32, nbatch=2, lens=[65, 1], taps=(-1, 0, 1), packed=False, res_mode=1,
            post=True, act=ACT_RELU, out_scale=0.5, row_gap=7)
        add(f"small_res_inv_accum3_{n}", vid, dtype=dt, M=96, N=64, K=16, nbatch=2, lens=[96, 31], taps=(-1, 0, 1), packed=False, res_mode=2,
            accum_mode=3, accum_dtype=F32, out_scale=0.25, act=ACT_LRELU, slope=0.1)
        add(f"small_accum1_{n}", vid, dtype=dt, M=64, N=64, K=16, nbatch=1, packed=False, accum_mode=1, accum_dtype=BF if dt != F32 else F32)
        add(f"small_accum2_f16store_{n}", vid, dtype=dt, M=64, N=64, K=16, nbatch=2, lens=[64, 2], packed=False, accum_mode=2, accum_dtype=H16, has_out=False)
        add(f"small_n70_spill_{n}", vid, dtype=dt, M=40, N=70, K=16, nbatch=1, packed=False, bias_mode=0, ldo=72)
        add(f"stride2_2d_{n}", vid, dtype=dt, M=4 * 9, N=64, K=16, nbatch=2, lens=[17, 5], taps=[t % 3 - 1 for t in range(9)],
            du=[t // 3 - 1 for t in range(9)], stride=2, wout=9, hin=8, win=18, packed=False, post=True, bias_mode=0, act=ACT_RELU)
        # attention P.V with per-utterance k_len, one head: K = Lp, keys past roundup8(len) NaN
        add(f"pv_klen_heads_{n}", vid, dtype=dt, M=40, N=64, K=48, nbatch=3, nheads=1, lens=[40, 1, 13], k_len=[40, 1, 13], packed=False, bias_mode=0)
    # the frame GEMM of the log-mel front end (mel_from_padded): rows that overlap (ldx = hop < K = n_fft), an utterance stride that is no
    # multiple of ldx, a length-1 utterance, N no multiple of 32, no bias -- on the 64 x 64 tile, and past 512 tiles on the 128 x 128 one,
    # there with row starts at 4-byte, not 16-byte boundaries (ldx = 18: a hop that is no multiple of 4)
    add("frames_overlap_f32", 19, dtype=F32, M=100, N=68, K=64, ldx=16, ldo=68, nbatch=3, lens=[100, 1, 65], packed=False, bias_mode=0)
    add("frames_overlap_big_f32", 3, dtype=F32, M=22000, N=68, K=64, ldx=18, ldo=68, nbatch=3, lens=[22000, 1, 21900], packed=False, bias_mode=0,
        big=True)
    big = [("gemm128x128", 0, 3, dict(M=1024, N=128, K=64, nbatch=64)), ("gemm256x64", 1, 4, dict(M=2048, N=64, K=32, nbatch=64)),
           ("gemm256x32", 2, 5, dict(M=2048, N=32, K=32, nbatch=64))]
    for nm, v16, v32, kw in big:
        lens = [kw["M"] - (i * 37) % kw["M"] for i in range(kw["nbatch"])]
        lens[1] = 1
        for dt in (BF, H16, F32):
            add(f"{nm}_{DT_NAME[dt]}", v32 if dt == F32 else v16, dtype=dt, lens=lens, packed=False, act=ACT_LRELU, slope=0.2, big=True, **kw)

    # ---- conv-slab: 256 x 128 register-ring tile (N = 128, M > 128) with every compile-time epilogue ----
    base = dict(M=300, N=128, K=128, nbatch=2, lens=[300, 1], taps=(-1, 0, 1))
    for dt in (BF, H16):
        n = DT_NAME[dt]
        other = H16 if dt == BF else BF
        add(f"slab256_epi001_{n}", 7, EPI(0, 0, 1), dtype=dt, act=ACT_LRELU, slope=0.1, **base)
        add(f"slab256_flip_{n}_to_{DT_NAME[other]}", 7, EPI_FLIP, dtype=dt, out_dtype=other, act=ACT_LRELU, slope=0.1, **base)
        add(f"slab256_epi101_{n}", 7, EPI(1, 0, 1), dtype=dt, res_mode=2, act=ACT_LRELU, slope=0.1, **base)
        add(f"slab256_epi120_{n}", 7, EPI(1, 2, 0), dtype=dt, res_mode=2, accum_mode=2, has_out=False, **base)
        add(f"slab256_epi130_{n}", 7, EPI(1, 3, 0), dtype=dt, res_mode=2, accum_mode=3, has_out=False, **base)
        add(f"slab256_epi111_{n}", 7, EPI(1, 1, 1), dtype=dt, res_mode=2, accum_mode=1, out_scale=1 / 3, act=ACT_LRELU, slope=0.1, **base)
        add(f"slab256_runtime_{n}", 7, -1, dtype=dt, alpha=0.5, post=True, act=ACT_RELU, out_dtype=F32, **base)
        add(f"slab256_partialk_{n}", 7, EPI(0, 0, 1), dtype=dt, M=260, N=128, K=80, nbatch=2, lens=[1, 260], taps=taps_1d(7, 3), act=ACT_LRELU, slope=0.1)
        add(f"slab256_halo64_{n}", 7, -1, dtype=dt, M=300, N=128, K=64, nbatch=1, taps=(-32, 0, 32), bias_mode=0)
        add(f"slab256_halo72_v3_{n}", 7, EPI(1, 1, 1), dtype=dt, M=400, N=128, K=128, nbatch=2, lens=[400, 1], taps=taps_1d(7, 12), res_mode=2,
            accum_mode=1, out_scale=1 / 3, act=ACT_LRELU, slope=0.1)
        add(f"slab256_k2_shortcut_{n}", 7, -1, dtype=dt, M=300, N=128, K=128, K2=48, nbatch=2, lens=[300, 1], taps=(-1, 0, 1), alpha=0.7071, bias_mode=1)
        add(f"slab256_split3_{n}", 7, -1, dtype=dt, M=200, N=128, K=64, nbatch=2, lens=[200, 150], taps=taps_1d(9), out_dtype=F32, out_split3=1 if dt == BF else 2,
            act=ACT_RELU)
    add("slab256_dec0_f16", 7, EPI_DEC0, dtype=H16, out_scale=0.7071, bias_mode=1, **base)
    add("slab256_dec1_f16", 7, EPI_DEC1, dtype=H16, res_mode=1, out_scale=0.7071, bias_mode=0, **base)
    # half epilogues drive the accumulator past 65504: the stores clamp, never Inf
    add("slab256_f16_saturate", 7, EPI(0, 0, 1), dtype=H16, act=ACT_NONE, x_scale=3e4, bias_scale=2000.0, **base)
    add("slab256_dec0_f16_saturate", 7, EPI_DEC0, dtype=H16, out_scale=2.0, bias_mode=0, x_scale=3e4, **base)
    add("small_f16_saturate", 18, None, dtype=H16, M=64, N=64, K=64, packed=False, x_scale=3e4, bias_scale=2000.0)
    # ---- batch-flattened decoder convolutions (bflat) on the 128 x 128 tile with its compile-time epilogues ----
    fb = dict(M=257, N=128, K=64, nbatch=2, lens=[257, 1], taps=(-1, 0, 1), bflat=272)
    for dt in (BF, H16):
        n = DT_NAME[dt]
        add(f"slab128_bflat_epi001_{n}", 22, EPI(0, 0, 1), dtype=dt, act=ACT_LRELU, slope=0.2, **fb)
        add(f"slab128_bflat_runtime_{n}", 22, -1, dtype=dt, act=ACT_RELU, post=True, **fb)
    add("slab128_bflat_dec0_f16", 22, EPI_DEC0, dtype=H16, out_scale=0.7071, **fb)
    add("slab128_bflat_dec1_f16", 22, EPI_DEC1, dtype=H16, res_mode=1, out_scale=0.7071, bias_mode=0, **fb)
    # ---- 128 x 128 / 64 x 128 tiles of short utterances (phoneme encoder: M <= 128), encoder split-3 GEMM ----
    for dt in (BF, H16):
        n = DT_NAME[dt]
        add(f"enc_short_{n}", 22, None, dtype=dt, M=100, N=256, K=192, nbatch=3, lens=[100, 1, 64], act=ACT_RELU, xcd_flat=0)
        add(f"enc_split3_{n}", 22, None, dtype=dt, M=120, N=256, K=3 * 64, nbatch=2, lens=[120, 7], taps=taps_1d(9), out_dtype=F32,
            out_split3=1 if dt == BF else 2, act=ACT_RELU)
        add(f"single_small_rows_{n}", 22, None, dtype=dt, M=300, N=256, K=64, nbatch=1, slab_small=1, act=ACT_RELU)
        add(f"single_32ch_{n}", 9, None, dtype=dt, M=60, N=192, K=64, nbatch=1, lens=[60], slab_small=2, bias_mode=1)
        add(f"slab256x64_{n}", 8, None, dtype=dt, M=200, N=64, K=128, nbatch=2, lens=[200, 1], taps=(-1, 0, 1), act=ACT_LRELU, slope=0.1)
        add(f"slab256x32_{n}", 9, None, dtype=dt, M=200, N=32, K=64, nbatch=2, lens=[1, 200], taps=(-2, 0, 2), res_mode=1)
        # the ConvTranspose in front of a vocoder stage: polyphase taps, 128 x 256 tile when 256 x 128 would need another round
        add(f"slab128x256_{n}", 6, None, dtype=dt, M=384, N=512, K=64, nbatch=65, lens=[384 - (i * 13) % 380 for i in range(65)], taps=(0,),
            act=ACT_LRELU, slope=0.1, big=True)
    # ---- register-weight convolutions C = 32 / 64 (vocoder ResBlock convs, V3's dilation-12 taps: 72 halo rows) ----
    for dt in (BF, H16):
        n = DT_NAME[dt]
        for C, vid in ((32, 14), (64, 15)):
            add(f"convreg_c{C}_k3_{n}", vid, None, dtype=dt, M=700, N=C, K=C, nbatch=2, lens=[700, 1], taps=taps_1d(3, 5), res_mode=2, accum_mode=3,
                accum_dtype=dt, out_scale=0.5, act=ACT_LRELU, slope=0.1)
            add(f"convreg_c{C}_k11_{n}", vid, None, dtype=dt, M=300, N=C, K=C, nbatch=1, taps=taps_1d(11), act=ACT_LRELU, slope=0.1)
            add(f"convreg_c{C}_k7_halo72_{n}", vid, None, dtype=dt, M=500, N=C, K=C, nbatch=2, lens=[3, 500], taps=taps_1d(7, 12), res_mode=2, act=ACT_LRELU, slope=0.1)
    # ---- fused ResBlock pairs ----
    for dt in (BF, H16):
        n = DT_NAME[dt]
        for C, vid in ((32, 16), (64, 17)):
            add(f"resfuse_c{C}_k3_{n}", vid, None, dtype=dt, M=600, N=C, K=C, nbatch=2, lens=[600, 1], taps=taps_1d(3), dil1=5, fused=1, act=ACT_LRELU, slope=0.1)
            add(f"resfuse_c{C}_k7_accum_{n}", vid, None, dtype=dt, M=300, N=C, K=C, nbatch=2, lens=[17, 300], taps=taps_1d(7), dil1=3, fused=1,
                accum_mode=3, accum_dtype=dt, out_scale=1 / 3)
        add(f"resfuse_c64_k11_{n}", 17, None, dtype=dt, M=300, N=64, K=64, nbatch=1, taps=taps_1d(11), dil1=1, fused=1)
        add(f"pairstream_c128_{n}", 23, None, dtype=dt, M=700, N=128, K=128, nbatch=2, lens=[700, 1], taps=taps_1d(3), dil1=3, fused=1,
            no_pairstream=2, act=ACT_LRELU, slope=0.1)
        # the streaming pair kernel past one segment: M = 1100 is two 1024-row segments, 1025 puts the seam one row before an utterance's
        # end; every k with every dilation of ResBlock1, the four accumulator modes dealt over them so that each runs in both types
        for i, (k, dil) in enumerate((k, dil) for k in (3, 7, 11) for dil in (1, 3, 5)):
            am = (i + (2 if dt == H16 else 0)) % 4
            add(f"pairstream_seam_k{k}_d{dil}_am{am}_{n}", 23, None, **pair_seam_kw(dt, k, dil, am))
        for C, vid in ((32, 30), (64, 31)):
            add(f"rb2fuse_c{C}_k3_{n}", vid, None, dtype=dt, M=500, N=C, K=C, nbatch=2, lens=[500, 1], taps=taps_1d(3, 3), dil1=1, fused=2, act=ACT_LRELU, slope=0.1)
        add(f"rb2fuse_c32_k7_accum_{n}", 30, None, dtype=dt, M=400, N=32, K=32, nbatch=1, taps=taps_1d(7, 12), dil1=3, fused=2, accum_mode=3, accum_dtype=dt)
    # ---- speaker encoder: 3 x 3 maps (flattened), persistent C = 32 / 64, stride-2 level transitions ----
    k33 = dict(taps=[t % 3 - 1 for t in range(9)], du=[t // 3 - 1 for t in range(9)])
    add("spk_flat_c32_convreg", 14, None, dtype=BF, M=6 * 41, N=32, K=32, nbatch=2, lens=[40, 1], wout=41, hin=6, win=41, flat=True, bias_mode=1, **k33)
    add("spk_flat_c64_convreg", 15, None, dtype=BF, M=5 * 30, N=64, K=64, nbatch=2, lens=[29, 7], wout=30, hin=5, win=30, flat=True, bias_mode=1, **k33)
    add("spk_flat_c128_slab128", 22, None, dtype=BF, M=3 * 40, N=128, K=128, nbatch=2, lens=[39, 1], wout=40, hin=3, win=40, flat=True, bias_mode=1, **k33)
    add("spk_flat_c128_slab256", 7, None, dtype=BF, M=4 * 35, N=128, K=128, nbatch=2, lens=[34, 1], wout=35, hin=4, win=35, flat=True, bias_mode=1, **k33)
    add("spk_persist_c32", 26, None, dtype=BF, M=5 * 70, N=32, K=32, nbatch=2, lens=[69, 1], wout=70, hin=5, win=70, flat=True, bias_mode=0, post=True, act=ACT_RELU, **k33)
    add("spk_persist_c64", 27, None, dtype=BF, M=4 * 66, N=64, K=64, nbatch=2, lens=[65, 30], wout=66, hin=4, win=66, flat=True, bias_mode=1, **k33)
    add("spk_s2_ds_c32", 28, None, dtype=BF, M=4 * 21, N=64, K=32, nbatch=2, lens=[40, 3], wout=21, hin=8, win=41, stride=2, bias_mode=0, post=True,
        act=ACT_RELU, ds=True, **k33)
    add("spk_s2_c64", 29, None, dtype=BF, M=3 * 16, N=128, K=64, nbatch=2, lens=[30, 1], wout=16, hin=6, win=31, stride=2, bias_mode=0, post=True,
        act=ACT_RELU, **k33)
    # ---- every halo limit: 64 (slab), just past it (65), the 96 rows of the k = 7 register / 160-row-slab kernels, the 160 rows of the
    #      flattened 3 x 3 map on the 256 x 128 tile ----
    h65 = (-33, -20, -10, 0, 10, 20, 32)
    for dt in (BF, H16):
        n = DT_NAME[dt]
        for C, vid in ((32, 14), (64, 15)):
            add(f"convreg_c{C}_halo96_{n}", vid, None, dtype=dt, M=400, N=C, K=C, nbatch=2, lens=[400, 2], taps=taps_1d(7, 16), res_mode=2, act=ACT_LRELU, slope=0.1)
            add(f"convreg_c{C}_halo65_{n}", vid, None, dtype=dt, M=300, N=C, K=C, nbatch=2, lens=[1, 300], taps=h65, bias_mode=1)
        for nm, tp in (("halo96", taps_1d(7, 16)), ("halo65", h65)):
            add(f"slab256_{nm}_{n}", 7, EPI(1, 1, 1), dtype=dt, M=400, N=128, K=128, nbatch=2, lens=[400, 1], taps=tp, res_mode=2, accum_mode=1,
                out_scale=1 / 3, act=ACT_LRELU, slope=0.1)
    add("spk_flat_c128_halo160", 7, None, dtype=BF, M=3 * 79, N=128, K=128, nbatch=2, lens=[78, 5], wout=79, hin=3, win=79, flat=True, bias_mode=1,
        **k33)
    # ---- the other forms of variant 22 and of the fused pair dispatch ----
    for dt in (BF, H16):
        n = DT_NAME[dt]
        add(f"single_rows128_{n}", 22, None, dtype=dt, M=300, N=1024, K=64, nbatch=5, lens=[300, 1, 257, 128, 129], slab_small=1, act=ACT_RELU)
        add(f"enc_short_m50_{n}", 22, None, dtype=dt, M=50, N=256, K=64, nbatch=3, lens=[50, 1, 33], act=ACT_RELU)
        add(f"resfuse_c32_no_pairstream_{n}", 16, None, dtype=dt, M=300, N=32, K=32, nbatch=2, lens=[300, 9], taps=taps_1d(3), dil1=3, fused=1,
            no_pairstream=1)
    add("slab256_runtime_f16out", 7, -1, dtype=H16, alpha=0.5, post=True, act=ACT_RELU, **base)
    # ---- half stores past 65504, one case per half epilogue / kernel: the stores clamp to +-65504, never Inf ----
    by_name = {e[0]: e for e in T}
    for nm in ("slab256_epi101_f16", "slab256_epi120_f16", "slab256_epi130_f16", "slab256_epi111_f16", "slab256_flip_bf16_to_f16",
               "slab256_runtime_f16out", "slab256_dec1_f16", "slab128_bflat_epi001_f16", "slab128_bflat_runtime_f16", "slab128_bflat_dec0_f16",
               "slab128_bflat_dec1_f16", "slab256x64_f16", "slab256x32_f16", "enc_short_f16", "single_32ch_f16", "convreg_c32_k3_f16",
               "convreg_c64_k3_f16", "convreg_c64_halo96_f16", "resfuse_c32_k3_f16", "resfuse_c64_k7_accum_f16", "resfuse_c64_k11_f16",
               "pairstream_c128_f16", "rb2fuse_c32_k3_f16", "rb2fuse_c64_k3_f16", "rb2fuse_c32_k7_accum_f16", "pv_klen_heads_f16"):
        _, kw, vid, epi = by_name[nm]
        if kw.get("fused"):
            kw = dict(kw, x_scale=2.0 ** 12, bias_scale=2.0 ** 18, aux_scale=2.0 ** 14)   # grid data: biases past the range saturate T and the output
        else:
            kw = dict(kw, x_scale=2e4, bias_scale=1e5) if "flip" in nm else dict(kw, x_scale=1e5, bias_scale=3e4, aux_scale=3e4)      # biases / residuals / running sums of the same size: the
                                                                           # cast, the slope and the accumulator add stay visible
        T.append((nm + "_saturate", kw, vid, epi))
    return T


GEMM_CASES = _gemm_table()
# variant ids no case of the table reaches, each with its reason
# (20 / 21 and 24 / 25 -- launch_resstream, launch_narrowstage -- take their own argument structs: RESSTREAM_CASES / NARROW_CASES below)
EXCLUDED_VARIANTS = {10: "placeholder entry (unused)", 11: "retired (resfuse c8)", 12: "retired (resfuse c16)", 13: "retired (resfuse c128)"}


def _attn_table():
    T = []
    for f16 in (False, True):
        n = "f16" if f16 else "bf16"
        T.append((f"flash_L1_{n}", dict(flash=True, f16=f16, B=1, nheads=1, lens=[1])))
        T.append((f"flash_L2_{n}", dict(flash=True, f16=f16, B=1, nheads=2, lens=[2])))
        T.append((f"flash_tiles_ragged_{n}", dict(flash=True, f16=f16, B=3, nheads=2, lens=[129, 1, 64], ldq_pad=8, ldv_pad=8, ldo_pad=4, k_off_extra=8)))
        T.append((f"flash_tile_edges_{n}", dict(flash=True, f16=f16, B=3, nheads=1, lens=[127, 65, 63])))
        T.append((f"flash_896_{n}", dict(flash=True, f16=f16, B=3, nheads=2, lens=[896, 1, 300])))
    for planes, pf16 in ((False, False), (True, False), (True, True)):
        nm = "planes_f16" if pf16 else ("planes_bf16" if planes else "noplanes")
        T.append((f"attnf32_ragged_{nm}", dict(flash=False, B=3, nheads=2, lens=[129, 1, 33], planes=planes, planes_f16=pf16, ldq_pad=4, k_off_extra=4)))
    T.append(("attnf32_L2", dict(flash=False, B=1, nheads=1, lens=[2])))
    T.append(("attnf32_tile_edges", dict(flash=False, B=3, nheads=1, lens=[31, 32, 255])))
    return T


ATTN_CASES = _attn_table()


def build_case(entry, seed=0):
    name, kw = entry[0], entry[1]
    if "flash" in kw:
        return make_attn(name, seed, **kw)
    if "kind" in kw:
        return make_heads(name, seed, **kw)
    return make_gemm(name, seed, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# running a problem on the device (tests/test_kernels_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def alloc(self, nbytes):
        p = self.lib.zvxk_alloc(max(16, nbytes))
        assert p, "device allocation failed"
        self.ptrs.append(p)
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        assert self.lib.zvxk_h2d(p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def download(self, p, n, dtype):
        out = np.empty(n, dtype)
        assert self.lib.zvxk_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.zvxk_free(p)
        self.ptrs = []


def _bits_of(buf):
    if buf.get("bits") is not None:
        return buf["bits"]
    v = buf["v"]
    dt = buf["dt"]
    bits = to_bits(np.nan_to_num(v, nan=0.0), dt)
    return np.where(np.isnan(v), nan_bits(dt), bits).astype(bits_dtype(dt))


def gemm_struct(p, dev):
    """ctypes GemmArgs of problem p with its buffers on the device (dev=None: host-only descriptor with null pointers, for dry runs)."""
    d = p.d
    a = GemmArgs()
    for k in ("x_bs", "x_hs", "ldx", "w_bs", "w_hs", "w_ts", "ldw", "fused", "slope1", "no_pairstream", "dtype", "M", "N", "K", "nbatch", "nheads",
              "in_len_static", "ntaps", "stride", "wout", "hin", "win", "bflat", "x2_bs", "ldx2", "K2", "xcd_flat", "slab_small", "out_split3",
              "alpha", "bias_mode", "r_bs", "r_hs", "ldr", "res_dtype", "res_mode", "res_inv_slope", "a_bs", "lda", "accum_mode", "accum_dtype",
              "out_scale", "act", "slope", "o_bs", "o_hs", "ldo", "out_dtype"):
        setattr(a, k, d[k])
    for k in ("du", "dv", "dv1"):
        getattr(a, k)[:] = d[k]
    ptr = {}
    fake = 0x100000
    for f, buf in p.bufs.items():
        if "alias" in buf:
            continue
        if dev is None:
            ptr[f] = fake
            fake += 0x100000
            continue
        if buf["role"] == "packed":
            continue
        ptr[f] = dev.upload(_bits_of(buf))
    if "res" in p.bufs and "alias" in p.bufs["res"]:
        ptr["res"] = ptr["X"]
    for f in ("X", "W", "bias", "res", "accum", "out", "X2", "bias1", "post_scale", "post_shift", "ds_out", "ds_bias"):
        if f in ptr:
            setattr(a, {"ds_bias": "ds_bias"}.get(f, f), ptr[f])
    if "post_scale" in ptr:
        a.post_shift = ptr["post_shift"]
    if "Wp" in p.bufs or d.get("fused") or d.get("ds_out"):
        if dev is None:
            a.Wp = fake
            a.Wp2 = fake + 0x100000 if d.get("fused") else None
            a.ds_Wp = fake + 0x200000 if d.get("ds_out") else None
        else:
            lib = dev.lib
            def pack(wptr, ntaps, N, K):
                out = dev.alloc(lib.zvxk_packed_weight_elems(ntaps, N, K) * 2)
                assert lib.zvxk_pack_weights(wptr, ntaps, N, K, out) == 0
                return out
            if d.get("fused"):
                a.Wp = pack(ptr["W"], d["ntaps"], d["N"], d["K"])
                a.Wp2 = pack(ptr["W1"], d["ntaps"], d["N"], d["K"])
            elif d["K2"]:
                pa, pb = pack(ptr["W"], d["ntaps"], d["N"], d["K"]), pack(ptr["W2"], 1, d["N"], d["K2"])
                a.Wp = dev.alloc((lib.zvxk_packed_weight_elems(d["ntaps"], d["N"], d["K"]) + lib.zvxk_packed_weight_elems(1, d["N"], d["K2"])) * 2)
                assert lib.zvxk_pack_pair(pa, d["ntaps"], d["K"], pb, 1, d["K2"], d["N"], a.Wp) == 0
            else:
                a.Wp = pack(ptr["W"], d["ntaps"], d["N"], d["K"])
            if d.get("ds_out"):
                a.ds_Wp = pack(ptr["ds_W"], 1, d["N"], d["K"])
    ints = {}
    for f in ("in_len", "out_len", "k_len"):
        if f == "out_len" and d.get("fused") and d.get(f) is not None and list(d[f]) == list(d["in_len"]):
            ints[f] = ints["in_len"]                         # the fused pairs take the one length array for both (as the vocoder passes it)
            setattr(a, f, ints[f])
            continue
        if d.get(f) is not None:
            arr = np.asarray(d[f], np.int32)
            ints[f] = dev.upload(arr) if dev is not None else fake + 0x300000 + len(ints) * 0x1000
            setattr(a, f, ints[f])
    return a, ptr


def attn_struct(p, dev):
    d = p.d
    flash = p.kind == "flash"
    a = FlashArgs() if flash else AttnF32Args()
    skip = {"name", "_lens", "L_rows"}
    for k, v in d.items():
        if k not in skip and not isinstance(v, list):
            setattr(a, k, v)
    ptr = {}
    for f, buf in p.bufs.items():
        ptr[f] = dev.upload(_bits_of(buf)) if dev is not None else 0x100000 * (len(ptr) + 1)
        setattr(a, f, ptr[f])
    lens = np.asarray(d["_lens"], np.int32)
    a.len = dev.upload(lens) if dev is not None else 0x900000
    return a, ptr


# ------------------------------------------------------------------------------------------------------------------------------
# chained ResBlock kernels: launch_resstream (StreamArgs), launch_narrowstage (StageArgs), launch_pairstream past one segment
#
# chain_ref steps a ResBlock1 pair in float64 with the 16-bit roundings where the kernels put them (rs_role's epilogue_block /
# store_phase, NsKernel::conv / tile, ps_role's epilogue_out):
#     T = Q16(lrelu(conv_d(x) + b1, slope1));  y = conv_1(T) + b2 + inv_lrelu(x);  next x = Q16(lrelu(y, slope1))
# every stream zero outside [0, len).  What closes the chain differs per kernel:
#     resstream    no running sum: out = Q16(lrelu(y, slope)).  With one -- KNOWN DEVIATION, the same as variants 16 / 17 in _fused_ref --
#                  y is packed to 16 bits BEFORE xs is added: s = Q16(y) (+ xs); xs' = Q16(s); out = Q16(lrelu(s * out_scale, slope))
#     pairstream   s = y (+ xs) in f32; xs' = Q16(s); out = Q16(lrelu(s * out_scale, slope))
#     narrowstage  the sum over the ResBlocks stays in f32: out = Q16(lrelu(sum_j y_j * f32(1 / nk), slope)), one rounding
# Every value carries a per-element uncertainty e (the kernel's f32 value lies within e of the reference's): a 16-bit rounding
# turns it into Q(v + e) - Q(v - e) -- zero unless a rounding boundary lies within e of v --, a convolution spreads it through |W|,
# and the two leaky-relus scale it by their slope only on the side where the sign is certain (x - e < 0 for inv_lrelu's x
# res_inv_slope, v + e < 0 for lrelu's x slope): without the signs the bound grows 10x per pair.  The accumulation term
# 2 n U sum|x w| (n = nonzero weights of the output channel + the bias) is dropped per ELEMENT where every partial sum is exact in
# f32 -- all terms multiples of g, sum of magnitudes <= 2^24 g (exact_f32, per element).  The exact-sum cases are built so that
# this holds almost everywhere; what is left are the element-wise f32 roundings (bias and residual adds, x slope, x res_inv_slope,
# x 1 / nk: U each).  The compared value is Q16(v), the tolerance max(Q(v + e) - Q(v), Q(v) - Q(v - e)): ZERO -- bit equality --
# for every element with no rounding boundary within e.
# PREMISE: a matrix instruction whose block sum is exactly representable returns it exactly.  The 32 x 32 x 16 cases of the
# table above have held the kernels to this on hardware; for the 16 x 16 x 32 instruction of narrowstage it is what NARROW_CASES
# measures.
# ------------------------------------------------------------------------------------------------------------------------------
SLOPE01 = float(np.float32(0.1))                  # the kernels multiply by the f32 nearest to 0.1 / to 1 / 3
THIRD = float(np.float32(1.0 / 3.0))


def egrid(a):
    """Per element: the largest power of two the value is a multiple of (inf for zero)."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(np.abs(a))
    ints = np.round(m * 2.0 ** 53).astype(np.int64)
    low = (ints & -ints).astype(np.float64)
    return np.where(a == 0, np.inf, np.ldexp(np.where(a == 0, 1.0, low), e - 53))


def _cconv(x, W, dil, shift_last=False):
    """y[b][r][n] = sum_t sum_c x[b][r + (t - h) dil][c] W[t][n][c]; rows outside [0, M) are zero."""
    k, M = W.shape[0], x.shape[1]
    h = (k - 1) // 2
    y = np.zeros(x.shape[:2] + (W.shape[1],))
    for t in range(k):
        o = (t - h) * dil + (1 if shift_last and t == k - 1 else 0)
        lo, hi = max(0, -o), min(M, M - o)
        if hi > lo:
            y[:, lo:hi] += x[:, lo + o:hi + o] @ W[t].T
    return y


def _conv_grid(gx, W, dil):
    """Per output element, the grid of the products that reach it (None for dense weights: never exact)."""
    k, N, C = W.shape
    nz = np.argwhere(W != 0)
    if len(nz) > 8 * N:
        return None
    M, h = gx.shape[1], (k - 1) // 2
    gw = egrid(W)
    g = np.full(gx.shape[:2] + (N,), np.inf)
    for t, n, c in nz:
        o = (t - h) * dil
        lo, hi = max(0, -o), min(M, M - o)
        if hi > lo:
            g[:, lo:hi, n] = np.minimum(g[:, lo:hi, n], gx[:, lo + o:hi + o, c] * gw[t, n, c])
    return g


def _conv_e(x, ex, W, b, dil, bound, shift_last=False):
    """conv(x) + b with its uncertainty: ex through |W|, plus the accumulation (and bias add) term where the sums are not exact."""
    v = _cconv(x, W, dil, shift_last) + b
    if not bound:
        return v, 0.0, 0.0
    mag = _cconv(np.abs(x), np.abs(W), dil) + np.abs(b)
    e = _cconv(ex, np.abs(W), dil)
    g = _conv_grid(egrid(x), W, dil)
    nn = 2.0 * (np.count_nonzero(W, axis=(0, 2)) + 1) * U
    if g is None:
        e = e + nn * mag
    else:
        e = e + np.where(mag <= 2.0 ** 24 * np.minimum(g, egrid(b)), 0.0, nn * mag)
    return v, e, mag


def _lrelu_e(v, e, slope):
    """max(v, v * slope), 0 < slope <= 1: the uncertainty shrinks by the slope only where v + e < 0; the product rounds once."""
    if slope == 1.0:
        return v, e
    out = np.where(v >= 0, v, v * slope)
    return out, np.where(v + e < 0, e * slope, e) + np.where(v - e < 0, U * (np.abs(out) + e), 0.0)


def _inv_lrelu_e(x, ex, rinv):
    """min(x, x * rinv), rinv >= 1: the uncertainty grows by rinv only where x - ex < 0."""
    out = np.where(x >= 0, x, x * rinv)
    neg = x - ex < 0
    return out, np.where(neg, ex * rinv, ex) + np.where(neg, U * np.abs(out), 0.0)


def _q_e(v, e, dt, q):
    if not q:
        return v, e
    return round_to(v, dt), round_to(v + e, dt) - round_to(v - e, dt)


def chain_pair(x, ex, inside, pr, dt, slope1, rinv, q=True, bound=True, mut=None):
    """One pair on streams x [b][M][C] (zero outside `inside`): y = conv_1(T) + b2 + inv_lrelu(x) in f64, and its uncertainty.
    pr: dict(W1, b1, W2, b2 [k][C][C] / [C], dil)."""
    mut = mut or ()
    W1, b1, W2, b2 = pr["W1"], pr["b1"], pr["W2"], pr["b2"]
    if "drop_weight" in mut:
        W1 = W1.copy()
        W1[tuple(np.argwhere(W1 != 0)[len(np.argwhere(W1 != 0)) // 2])] = 0.0
    if "swap_taps" in mut:
        W1 = W1.copy()
        W1[[0, 1]] = W1[[1, 0]]
    if "drop_bias" in mut:
        b2 = np.zeros_like(b2)
    t, e1, _ = _conv_e(x, ex, W1, b1, pr["dil"], bound)
    t, e1 = _lrelu_e(t, e1, slope1)
    T, eT = _q_e(t, e1, dt, q and "no_round_T" not in mut)
    T, eT = np.where(inside, T, 0.0), np.where(inside, eT, 0.0)
    a2, e2, m2 = _conv_e(T, eT, W2, b2, 1, bound, shift_last="shift_tap" in mut)
    if "seam" in mut:
        # the first row of a segment / tile computed as if nothing lay in front of it
        s0 = mut["seam"]
        Tz = T.copy()
        Tz[:, :s0] = 0.0
        a2[:, s0] = (_cconv(Tz, W2, 1) + b2)[:, s0]
    r, er = _inv_lrelu_e(x, ex, rinv * (0.5 if "res_slope" in mut else 1.0))
    y = a2 + r
    return y, e2 + er + (U * (m2 + np.abs(r)) if bound else 0.0)


class ChainCase:
    """A resstream / narrowstage / pairstream problem: X [b][M][C] (rows past lens NaN), blocks = list of ResBlocks, each a list of
    pairs dict(W1, b1, W2, b2, dil, k); epilogue parameters am / has_out / out_scale / slope; xs [b][M][C] for am & 1."""

    def __init__(self, **kw):
        self.nan_utts = ()
        self.__dict__.update(kw)

    def fields(self):
        f = []
        if self.kind == "narrowstage" or self.has_out:
            f.append("out")
        if self.kind != "narrowstage" and self.am & 2:
            f.append("accum")
        return f


def chain_ref(cs, q=True, bound=True, mut=None):
    """{field: (ref, tol, mask)} [b][M][C] of a ChainCase.  q=False: no 16-bit rounding anywhere (the pure float64 chain; tol is
    meaningless).  mut: dict of mutations of the reference (tests/test_kernel_reference.py)."""
    mut = dict(mut or {})
    nb, M, C = cs.X.shape
    dt = cs.dt
    lens = np.asarray(cs.lens)
    if "len_minus1" in mut:
        lens = np.maximum(lens - 1, 0)
    inside = (np.arange(M)[None, :, None] < lens[:, None, None])
    x0 = np.where(inside, np.nan_to_num(cs.X), 0.0)
    z = np.zeros_like(x0)
    pmut = {k: v for k, v in mut.items() if k in ("drop_weight", "swap_taps", "drop_bias", "no_round_T", "shift_tap", "seam", "res_slope")}
    at = mut.get("at", None)                                     # (block, pair) the pair-level mutations apply to; default: the last pair of the last block

    def run_block(j, blk):
        x, ex = x0, z
        for t, pr in enumerate(blk):
            here = (j, t) == (at if at is not None else (len(cs.blocks) - 1, len(blk) - 1))
            m = dict(pmut) if here else ({"res_slope": 1} if "res_slope" in pmut else None)
            y, ey = chain_pair(x, ex, inside, pr, dt, cs.slope1, cs.rinv, q, bound, m)
            if t + 1 < len(blk):
                v, e = _lrelu_e(y, ey, cs.slope1)
                x, ex = _q_e(v, e, dt, q)
                x, ex = np.where(inside, x, 0.0), np.where(inside, ex, 0.0)
        return y, ey

    res = {}

    def put(f, v, e):
        ref = round_to(v, dt) if q else v
        tol = np.maximum(round_to(v + e, dt) - ref, ref - round_to(v - e, dt)) if q and bound else np.zeros_like(v)
        mask = inside & np.ones((1, 1, C), bool)
        for b in cs.nan_utts:
            mask[b] = False
        res[f] = (ref, tol, mask)

    if cs.kind == "narrowstage":
        blocks = cs.blocks[:-1] if "mean_nk_minus1" in mut else cs.blocks
        S, eS = 0.0, 0.0
        for j, blk in enumerate(blocks):
            y, ey = run_block(j, blk)
            S = S + y
            eS = eS + ey + U * np.abs(S)
        inv = float(np.float32(1.0) / np.float32(len(blocks)))
        v = S * inv
        v, e = _lrelu_e(v, eS * inv + U * np.abs(v), cs.slope)
        put("out", v, e)
        return res
    y, ey = run_block(0, cs.blocks[0])
    if cs.am == 0:
        v, e = _lrelu_e(y, ey, cs.slope)
        put("out", v, e)
        return res
    s, es = _q_e(y, ey, dt, q) if cs.kind == "resstream" else (y, ey)
    if cs.am & 1 and "skip_xs" not in mut:
        s = s + np.nan_to_num(cs.xs)
        es = es + U * np.abs(s)
    if cs.am & 2:
        put("accum", s, es)
    if cs.has_out:
        v = s * cs.out_scale
        v, e = _lrelu_e(v, es * abs(cs.out_scale) + (U * np.abs(v) if cs.out_scale != 1.0 else 0.0), cs.slope)
        put("out", v, e)
    return res


def exact_share(ref):
    """Fraction of the compared elements whose tolerance is exactly zero."""
    n = sum(int(m.sum()) for _, _, m in ref.values())
    return sum(int((t[m] == 0).sum()) for _, t, m in ref.values()) / max(n, 1)


def _sparse_w(rng, k, C):
    """4 nonzeros +-2^-j (j = 1..3) per output channel; over the 4 C of them every tap index and every input channel occurs."""
    W = np.zeros((k, C, C))
    pk, pc = rng.permutation(k), rng.permutation(C)
    for n in range(C):
        for i in range(4):
            s = 4 * n + i
            W[pk[s % k], n, pc[s % C]] = rng.choice([-1.0, 1.0]) * 2.0 ** -int(rng.integers(1, 4))
    return W


def make_chain(name, seed=0, *, kind, dt, C, blocks, M, lens, data="exact", am=0, has_out=True, out_scale=1.0, slope=SLOPE01, ld_pad=0,
               nan_utts=(), data_seed=0):
    """blocks: [(k, dilations)] -- one entry for resstream (its pairs), nk entries for narrowstage (three pairs each).  Weights and
    biases are drawn from `seed`, inputs and running sum from (`seed`, `data_seed`)."""
    rng = _rng([seed, data_seed, 11])
    rngw = _rng([seed, 7])
    nb = len(lens)
    exact = data == "exact"

    def act_in(shape):
        v = np.round(8 * rng.standard_normal(shape)) / 8 if exact else rng.standard_normal(shape)
        return round_to(np.where(v >= 0, v, v * SLOPE01), dt)
    X = np.full((nb, M, C), np.nan)
    for b, l in enumerate(lens):
        if b not in nan_utts:
            X[b, :l] = act_in((l, C))
    blks = []
    for k, dils in blocks:
        prs = []
        for d in dils:
            pr = dict(k=k, dil=d)
            for w, bn in (("W1", "b1"), ("W2", "b2")):
                pr[w] = _sparse_w(rngw, k, C) if exact else round_to(rngw.standard_normal((k, C, C)) / np.sqrt(k * C), dt)
                pr[bn] = rngw.integers(-16, 17, C) / 64.0 if exact else round_to(0.3 * rngw.standard_normal(C), DT_F32)
            prs.append(pr)
        blks.append(prs)
    xs = None
    if am & 1:
        xs = np.full((nb, M, C), np.nan)
        for b, l in enumerate(lens):
            xs[b, :l] = round_to(np.round(8 * rng.standard_normal((l, C))) / 8 if exact else rng.standard_normal((l, C)), dt)
    return ChainCase(name=name, kind=kind, dt=dt, C=C, M=M, lens=list(lens), X=X, blocks=blks, am=am, has_out=has_out, out_scale=out_scale,
                     slope=slope, slope1=SLOPE01, rinv=10.0, xs=xs, ld=C + ld_pad, data=data, nan_utts=tuple(nan_utts))


def chain_of_gemm(p, data_seed=0):
    """The ChainCase of a fused-pair GemmArgs problem (the dense pairstream cases: their rms criterion runs on chain_ref).
    data_seed > 0: the same weights under another draw of the input and the running sum."""
    cs = _chain_of_gemm(p)
    if data_seed:
        rng = _rng([data_seed, 13])
        inside = ~np.isnan(cs.X)
        v = round_to(rng.standard_normal(cs.X.shape), cs.dt)
        cs.X = np.where(inside, round_to(np.where(v >= 0, v, v / cs.rinv), cs.dt), np.nan)
        if cs.xs is not None:
            cs.xs = np.where(inside, round_to(rng.standard_normal(cs.X.shape), cs.dt), np.nan)
    return cs


def _chain_of_gemm(p):
    d = p.d
    nb, M, C, k = d["nbatch"], d["M"], d["N"], d["ntaps"]
    pr = dict(k=k, dil=d["dv1"][1] - d["dv1"][0], W1=p.bufs["W1"]["v"].reshape(k, C, C), b1=p.bufs["bias1"]["v"][:C],
              W2=p.bufs["W"]["v"].reshape(k, C, d["ldw"])[:, :, :C], b2=p.bufs["bias"]["v"][:C])
    am = d["accum_mode"]
    xs = p.bufs["accum"]["v"].reshape(nb, -1, d["lda"])[:, :M, :C] if am & 1 else None
    return ChainCase(name=d["name"], kind="pairstream", dt=d["dtype"], C=C, M=M, lens=list(d["in_len"]), blocks=[[pr]],
                     X=p.bufs["X"]["v"].reshape(nb, -1, d["ldx"])[:, :M, :C], am=am, has_out=d["_has_out"],
                     out_scale=float(np.float32(d["out_scale"])), slope=float(np.float32(d["slope"])) if d["act"] == ACT_LRELU else 1.0,
                     slope1=float(np.float32(d["slope1"])), rinv=d["res_inv_slope"], xs=xs, ld=d["ldo"], data="dense")


# ---- the rms criterion of the dense cases ----
RMS_SEEDS = 8


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


def rms_vs_pure(values, pure, mask):
    return _rms((values - pure)[mask])


def rms_margin(build, seeds=RMS_SEEDS):
    """E_r = rms(chain_ref's rounded values - the pure float64 chain) per output field for `seeds` data seeds of build(seed) (the
    weights stay: E_r scales with the chain's gain, which is the weights', not the data's), and the
    margin m = 3 x (max - min) / mean of E_r over the seeds: what the reference's own error varies by from one draw of the data to
    the next, from the reference alone.  Returns {field: (E_r of seed 0, spread, m)}."""
    er = {}
    for s in range(seeds):
        cs = build(s)
        a, b = chain_ref(cs, q=True, bound=False), chain_ref(cs, q=False, bound=False)
        for f in a:
            er.setdefault(f, []).append(rms_vs_pure(a[f][0], b[f][0], a[f][2]))
    out = {}
    for f, v in er.items():
        spread = (max(v) - min(v)) / (sum(v) / len(v))
        out[f] = (v[0], spread, 3.0 * spread)
    return out


def dense_builder(entry):
    """data seed -> ChainCase of a dense NARROW_CASES / PAIR_DENSE_CASES entry (seed 0: the case the device runs)."""
    if "kind" in entry[1]:
        return lambda seed: make_chain(entry[0], 0, data_seed=seed, **entry[1])
    p = build_case(entry)
    return lambda seed: chain_of_gemm(p, seed)


# ---- tables ----
RS_FORMS = [(32, 3, (1, 3, 5)), (32, 7, (1, 3, 5)), (32, 11, (1, 3, 5)), (64, 3, (1, 3, 5)), (64, 7, (1, 3)), (64, 7, (5,)), (64, 11, (1, 3)),
            (64, 11, (5,))]                                      # the eight RS_TRY forms of launch_resstream
RS_LENS = [600, 257, 1]                                          # S = 256: three segments; 257 is one row into a segment


def _rs_epi(am):
    return dict(am=am, has_out=am < 2, out_scale=THIRD if am == 1 else 1.0)


def _resstream_table():
    T = []
    for i, (C, k, dils) in enumerate(RS_FORMS):
        for di, dt in enumerate((DT_BF16, DT_F16)):
            for am in (0, 1 + (i + di) % 3):                     # am 0 on every form; 1 / 2 / 3 dealt so that each runs at both C in both types
                for data in ("exact", "dense"):
                    nm = f"resstream_c{C}_k{k}_np{len(dils)}_am{am}_{data}_{DT_NAME[dt]}"
                    T.append((nm, dict(kind="resstream", dt=dt, C=C, blocks=[(k, dils)], M=600, lens=RS_LENS, data=data,
                                       ld_pad=8 if dt == DT_F16 else 0, **_rs_epi(am)), 20 if C == 32 else 21))
    # a length that is exactly one segment
    T.append(("resstream_c32_k3_len256_exact_bf16", dict(kind="resstream", dt=DT_BF16, C=32, blocks=[(3, (1, 3, 5))], M=600, lens=[256, 600], **_rs_epi(3)), 20))
    T.append(("resstream_c64_k7_len256_exact_f16", dict(kind="resstream", dt=DT_F16, C=64, blocks=[(7, (1, 3))], M=600, lens=[256, 600], **_rs_epi(0)), 21))
    return T


NS_R = {16: 384, 8: 512}                                         # rows per tile (launch_narrowstage)
NS_WGPC = {16: 1, 8: 2}                                          # workgroups per CU
NS_KS = [(3, 7, 11), (5,), (11, 3), (7, 5, 3)]


def ns_lens(C):
    R = NS_R[C]
    return [2 * R + 80, 2 * R + 79, R, R + 1, 57, 1]             # 2 R + 80: the first interior tile (m0 + R + NS_HB + NS_GUARD <= len), by equality


def _narrow_table():
    T = []
    for C in (16, 8):
        for dt in (DT_BF16, DT_F16):
            for ks in NS_KS:
                for data in ("exact", "dense"):
                    nm = f"narrowstage_c{C}_k{'_'.join(map(str, ks))}_{data}_{DT_NAME[dt]}"
                    T.append((nm, dict(kind="narrowstage", dt=dt, C=C, blocks=[(k, (1, 3, 5)) for k in ks], M=3 * NS_R[C] + 40, lens=ns_lens(C),
                                       data=data), 24 if C == 16 else 25))
    return T


def narrow_reuse_kw(C, ncu):
    """More one-tile utterances than workgroups, so that a workgroup takes a second tile; two utterances hold NaN: the one a second
    tile follows in its workgroup, and a second tile."""
    n = ncu * NS_WGPC[C] + 8
    lens = [1 + (i * 29) % 48 for i in range(n)]
    return dict(kind="narrowstage", dt=DT_BF16 if C == 16 else DT_F16, C=C, blocks=[(k, (1, 3, 5)) for k in (3, 7, 11)], M=48, lens=lens,
                nan_utts=(5, n - 6))


def _pair_dense_table():
    T = []
    for dt in (DT_BF16, DT_F16):
        for i, (k, dil) in enumerate((k, dil) for k in (3, 7, 11) for dil in (1, 3, 5)):
            am = (i + (2 if dt == DT_F16 else 0)) % 4
            T.append((f"pairstream_seam_k{k}_d{dil}_am{am}_dense_{DT_NAME[dt]}", dict(pair_seam_kw(dt, k, dil, am), grid_data=False), 23, None))
    return T


RESSTREAM_CASES = _resstream_table()
NARROW_CASES = _narrow_table()
PAIR_DENSE_CASES = _pair_dense_table()


def build_chain(entry, seed=0):
    return make_chain(entry[0], seed, **entry[1])


# ---- descriptors and launches ----
def _fake(i):
    return 0x100000 * (i + 1)


def _bits_nan(v, dt):
    return np.where(np.isnan(v), nan_bits(dt), to_bits(np.nan_to_num(v), dt)).astype(bits_dtype(dt))


def _out_buffers(cs, dev, fields):
    """Output / running-sum buffers [b][M][ld] as bits: sentinel everywhere, xs in the valid rows of an accumulated running sum."""
    nb, M, C = cs.X.shape
    before, ptr = {}, {}
    for f in fields:
        bits = np.full((nb, M, cs.ld), sentinel_bits(cs.dt), bits_dtype(cs.dt))
        if f == "accum" and cs.am & 1:
            xb = to_bits(np.nan_to_num(cs.xs), cs.dt)
            bits[:, :, :C] = np.where(np.isnan(cs.xs), bits[:, :, :C], xb)
        before[f] = bits.reshape(-1)
        ptr[f] = dev.upload(before[f]) if dev is not None else _fake(20 + len(ptr))
    return before, ptr


def stream_struct(cs, dev):
    """StreamArgs of a resstream ChainCase (dev=None: fake pointers for dry runs).  Returns (args, {field: device pointer}, {field: bits before})."""
    nb, M, C = cs.X.shape
    a = StreamArgs()
    a.x_bs, a.ldx, a.C, a.ntaps, a.npair = M * C, C, C, cs.blocks[0][0]["k"], len(cs.blocks[0])
    a.o_bs = a.a_bs = M * cs.ld
    a.ldo = a.lda = cs.ld
    a.accum_mode, a.slope1, a.res_inv_slope, a.out_scale, a.slope = cs.am, cs.slope1, cs.rinv, cs.out_scale, cs.slope
    a.M, a.nbatch, a.seg_min, a.f16 = M, nb, 0, int(cs.dt == DT_F16)
    a.X = dev.upload(_bits_nan(cs.X, cs.dt)) if dev is not None else _fake(0)
    a.len = dev.upload(np.asarray(cs.lens, np.int32)) if dev is not None else _fake(1)
    for t, pr in enumerate(cs.blocks[0]):
        a.dil[t] = pr["dil"]
        for q, (w, bn) in enumerate((("W1", "b1"), ("W2", "b2"))):
            if dev is None:
                wp, bp = _fake(2 + 4 * t + 2 * q), _fake(3 + 4 * t + 2 * q)
            else:
                k = pr["k"]
                raw = dev.upload(to_bits(pr[w], cs.dt))
                wp = dev.alloc(dev.lib.zvxk_packed_weight_elems(k, C, C) * 2)
                assert dev.lib.zvxk_pack_weights(raw, k, C, C, wp) == 0
                bp = dev.upload(np.concatenate([pr[bn], np.zeros(8)]).astype(np.float32))
                pr["_" + w], pr["_" + bn] = wp, bp               # (also the operands of the per-pair launches of the bit-equality check)
            getattr(a, w)[t] = wp
            getattr(a, bn)[t] = bp
    fields = (["out"] if cs.has_out else []) + (["accum"] if cs.am else [])
    before, ptr = _out_buffers(cs, dev, fields)
    a.out, a.accum = ptr.get("out"), ptr.get("accum")
    return a, ptr, before


def resfuse_chain(cs, dev, a):
    """The same chain as len(pairs) launch_resfuse launches (no_pairstream = 1, variants 16 / 17) on the operands stream_struct put on
    the device: {field: bits} of fresh output buffers."""
    nb, M, C = cs.X.shape
    lib = dev.lib
    before, ptr = _out_buffers(cs, dev, (["out"] if cs.has_out else []) + (["accum"] if cs.am else []))
    cur, ld = a.X, C
    prs = cs.blocks[0]
    for t, pr in enumerate(prs):
        last = t + 1 == len(prs)
        g = GemmArgs()
        k = pr["k"]
        g.X, g.x_bs, g.ldx, g.ldw, g.w_ts = cur, M * ld, ld, C, C * C
        g.Wp, g.Wp2, g.bias, g.bias1 = pr["_W2"], pr["_W1"], pr["_b2"], pr["_b1"]
        g.dv1[:] = _pad_taps(taps_1d(k, pr["dil"]))
        g.dv[:] = _pad_taps(taps_1d(k))
        g.fused, g.slope1, g.no_pairstream, g.dtype = 1, cs.slope1, 1, cs.dt
        g.M, g.N, g.K, g.nbatch, g.nheads, g.ntaps, g.stride, g.hin, g.xcd_flat = M, C, C, nb, 1, k, 1, 1, 1
        g.in_len = g.out_len = a.len
        g.alpha, g.bias_mode, g.out_scale = 1.0, 1, 1.0
        g.res, g.r_bs, g.ldr, g.res_dtype, g.res_mode, g.res_inv_slope = cur, M * ld, ld, cs.dt, 2, cs.rinv
        g.accum_dtype = g.out_dtype = cs.dt
        if not last:
            nxt = dev.upload(np.full(nb * M * C, sentinel_bits(cs.dt), bits_dtype(cs.dt)))
            g.out, g.o_bs, g.ldo, g.act, g.slope = nxt, M * C, C, ACT_LRELU, cs.slope1
        else:
            g.o_bs = g.a_bs = M * cs.ld
            g.ldo = g.lda = cs.ld
            g.out, g.accum, g.accum_mode = ptr.get("out"), ptr.get("accum"), cs.am
            g.out_scale = cs.out_scale
            g.act, g.slope = (ACT_LRELU, cs.slope) if cs.has_out and cs.slope != 1.0 else (ACT_NONE, 1.0)
        vid = lib.zvxk_gemm(g, 0)
        assert vid > -1000, f"{cs.name}: per-pair launch {t}: HIP error {-vid - 1000}"
        assert vid == (16 if C == 32 else 17), f"{cs.name}: per-pair launch {t} returned {vid}"
        if not last:
            cur, ld = g.out, C
    n = nb * M * cs.ld
    return {f: dev.download(ptr[f], n, bits_dtype(cs.dt)) for f in ptr}


def stage_struct(cs, dev):
    """StageArgs of a narrowstage ChainCase: the fragments of convolution 6 j + 2 t + {0: conv1, 1: conv2} at woff, biases in that order."""
    nb, M, C = cs.X.shape
    a = StageArgs()
    a.x_bs = a.o_bs = M * C
    a.ldx = a.ldo = a.C = C
    a.nk, a.slope1, a.res_inv_slope, a.slope, a.M, a.nbatch, a.f16 = len(cs.blocks), cs.slope1, cs.rinv, cs.slope, M, nb, int(cs.dt == DT_F16)
    steps = lambda k: (k + 32 // C - 1) // (32 // C)             # narrowstage_steps (held to the shim's by test_kernels_gpu)
    nfrag, bias = 0, []
    for j, blk in enumerate(cs.blocks):
        a.ks[j] = blk[0]["k"]
        for t, pr in enumerate(blk):
            a.dil[j][t] = pr["dil"]
            for q, (w, bn) in enumerate((("W1", "b1"), ("W2", "b2"))):
                a.woff[6 * j + 2 * t + q] = nfrag
                nfrag += steps(pr["k"])
                bias.append(pr[bn])
    before, ptr = _out_buffers(cs, dev, ["out"])
    a.out = ptr["out"]
    if dev is None:
        a.X, a.W, a.bias, a.len = _fake(0), _fake(1), _fake(2), _fake(3)
        return a, ptr, before
    lib = dev.lib
    a.X = dev.upload(_bits_nan(cs.X, cs.dt))
    a.len = dev.upload(np.asarray(cs.lens, np.int32))
    a.bias = dev.upload(np.concatenate(bias).astype(np.float32))
    a.W = dev.alloc(nfrag * 1024)
    for j, blk in enumerate(cs.blocks):
        for t, pr in enumerate(blk):
            for q, w in enumerate(("W1", "W2")):
                assert lib.zvxk_narrowstage_steps(C, pr["k"]) == steps(pr["k"])
                raw = dev.upload(to_bits(pr[w], cs.dt))
                assert lib.zvxk_pack_narrow(raw, pr["k"], C, a.W + a.woff[6 * j + 2 * t + q] * 1024) == 0
    return a, ptr, before


# ------------------------------------------------------------------------------------------------------------------------------
# persistent kernels past a workgroup's first tile (tests/test_persistent_tiles_gpu.py, checked on the host by
# tests/test_kernel_reference.py)
#
# Every kernel that sizes its grid to the chip walks several tiles or segments per workgroup at production shapes and exactly one
# in the tables above.  The cases below are built at run time from the CU count so that every workgroup takes at least
# PERSIST_TRIPS[kernel] units; the grid rule of each launcher is restated here (*_grid) and the walk of its kernel (strided_walk,
# dealt_walk), and the number of trips is asserted on the host before anything is launched.
#
# What the shipped geometry allows.  resfuse_persist, narrowstage, conv2d_persist and conv2d_s2 tile every utterance over the common
# M, so a case mixes utterances of one and of several tiles.  launch_resstream and launch_pairstream choose the segment length
# S >= M nbatch / nwg: nsegs = nbatch ceil(M / S) < nbatch + nwg, so three segments per workgroup need nbatch > 2 nwg, hence S > 2 M
# and ONE segment per utterance -- with these two launchers "several trips" and "several segments per utterance" exclude each
# other, and no utterance can be exactly one segment long.  Their cases here are many one-segment utterances; the seam inside an
# utterance stays with RESSTREAM_CASES / the pairstream_seam cases.
# ------------------------------------------------------------------------------------------------------------------------------
PERSIST_TRIPS = {"resfuse": 5, "conv2d_persist": 3, "conv2d_s2": 3, "narrowstage": 3, "resstream": 3, "pairstream": 3}
RS_R = {(32, 3, 3): 64, (32, 7, 3): 64, (32, 11, 3): 64, (64, 3, 3): 32, (64, 7, 2): 32, (64, 7, 1): 64, (64, 11, 2): 32, (64, 11, 1): 64}
PS_R = 128


def _cdiv(a, b):
    return -(-a // b)


def resfuse_grid(C, k, M, nbatch, ncu):
    """launch_resfuse_persist_c: tiles of BMO = BM1 - (k - 1) output rows, one workgroup per CU."""
    bm1 = 64 if (C == 64 and k == 11) else (256 if C == 32 else 128)
    rows = bm1 - (k - 1)
    per = _cdiv(M, rows)
    return dict(G=min(per * nbatch, ncu), per=per, rows=rows)


def narrow_grid(C, M, nbatch, ncu):
    per = _cdiv(M, NS_R[C])
    return dict(G=min(per * nbatch, ncu * NS_WGPC[C]), per=per, rows=NS_R[C])


def resstream_grid(C, k, npair, M, nbatch, ncu, seg_min=0):
    """launch_rs: about one segment per CU, never shorter than 256 rows (seg_min = 0), whole row blocks."""
    R = RS_R[(C, k, npair)]
    S = _cdiv(M * nbatch, ncu)
    if S < 2048:
        S = 2048 if seg_min < 0 else max(S, seg_min if seg_min > 0 else 256)
    S = _cdiv(S, R) * R
    per = _cdiv(M, S)
    return dict(G=min(per * nbatch, ncu), per=per, rows=S)


def pairstream_grid(M, nbatch, ncu):
    S = _cdiv(max(_cdiv(M * nbatch, ncu), 1024), PS_R) * PS_R
    per = _cdiv(M, S)
    return dict(G=min(per * nbatch, ncu), per=per, rows=S)


def conv2d_grid(kind, C, M, nbatch, ncu):
    """launch_conv2d_persist (C = 32: two workgroups per CU) / launch_conv2d_s2_variant: a multiple of 8 workgroups."""
    bm = {("persist", 32): 384, ("persist", 64): 256, ("s2", 32): 256, ("s2", 64): 128}[(kind, C)]
    wgpc = 2 if (kind, C) == ("persist", 32) else 1
    per = _cdiv(M, bm)
    G = max((wgpc * ncu) & ~7, 8)
    if per * nbatch < G:
        G = (per * nbatch + 7) & ~7
    return dict(G=G, per=per, rows=bm)


def strided_walk(g, nbatch, lens):
    """resfuse_persist / narrowstage / resstream / pairstream: workgroup w takes units w, w + G, ...; unit t is tile (segment) t % per of
    utterance t // per and is run when its first row lies inside the utterance.  -> per workgroup the (utterance, tile) it runs, in order."""
    lens = np.asarray(lens)
    out = []
    for w in range(g["G"]):
        t = np.arange(w, g["per"] * nbatch, g["G"])
        b, j = t // g["per"], t % g["per"]
        ok = j * g["rows"] < lens[b]
        out.append(list(zip(b[ok].tolist(), j[ok].tolist())))
    return out


def dealt_walk(g, nbatch):
    """conv2d_persist / conv2d_s2 (tile_of): rounds of G tiles, a round dealt in contiguous runs per XCD (workgroup = 8 slot + xcd); every
    tile is run whatever the utterance's width."""
    G, ntiles = g["G"], g["per"] * nbatch
    out = [[] for _ in range(G)]
    for base in range(0, ntiles, G):
        n = min(ntiles - base, G)
        per = (n + 7) >> 3
        for w in range(G):
            t = (w & 7) * per + (w >> 3)
            if (w >> 3) < per and t < n:
                out[w].append(divmod(base + t, g["per"]))
    return out


def walk_plan(walk, nbatch, long_utts, want_nan=True):
    """From a walk: the least number of units a workgroup runs; which (long?, long?) successions occur inside a workgroup; two utterances
    to fill with NaN (one that another utterance follows in its workgroup, one that is itself a later unit -- both short, with
    neighbours that are not the other one); and the utterances a sampled float64 comparison must cover: every long one, whatever
    follows a long one or comes next to a NaN one in a workgroup, and a spread of the rest."""
    long_utts = set(long_utts)
    trips = min(len(w) for w in walk)
    follow, before, patterns = {}, {}, set()
    for w in walk:
        for (b0, _), (b1, _) in zip(w, w[1:]):
            if b0 != b1:
                follow.setdefault(b0, set()).add(b1)
                before.setdefault(b1, set()).add(b0)
                patterns.add((b0 in long_utts, b1 in long_utts))
    nan = ()
    if want_nan:
        short = [b for b in range(nbatch) if b not in long_utts]
        first = next(b for b in short if follow.get(b))
        later = next(b for b in reversed(short) if before.get(b) and b != first and first not in before[b] | follow.get(b, set())
                     and not (follow.get(b, set()) | before[b]) & (follow[first] | before.get(first, set())))
        nan = (first, later)
    sample = set(long_utts) | set(range(0, nbatch, max(1, nbatch // 24)))
    for b in list(long_utts) + list(nan):
        sample |= follow.get(b, set()) | before.get(b, set())
    return dict(trips=trips, patterns=patterns, nan=nan, sample=sorted(sample - set(nan)))


def _short_lens(n, hi=48):
    return [1 + (i * 29) % hi for i in range(n)]


def _coprime_per(G, lo=3):
    from math import gcd
    per = lo
    while gcd(G, per) != 1:
        per += 1
    return per


def _place_long(lens, G, per, rows, M):
    """A few utterances of two or three units among the short ones, so that a workgroup runs long-then-long (A's first unit, then B's),
    long-then-short and short-then-long; one utterance of exactly one unit.  Returns the long ones."""
    A = 10
    B, j = divmod(per * A + G, per)
    assert B > A + 4 and B + 4 < len(lens)
    lens[A] = min(M, 2 * rows + 1)                           # three units (two where M ends earlier)
    lens[B] = min(M, j * rows + 33)                          # long enough for the unit that follows A's first one in its workgroup
    lens[A + 2] = rows + 1                                   # two units, the second of one row
    lens[B + 2] = min(M, 2 * rows + 17)
    lens[A + 4] = rows                                       # exactly one unit
    D = A + len(lens) // 2                                   # a long one met on a later trip: short-then-long
    lens[D] = rows + 9
    long_utts = [b for b in (A, B, A + 2, B + 2, D) if lens[b] > rows]
    if j == 0:                                               # B's first unit follows: B is long by its length alone
        lens[B] = min(M, rows + 33)
        long_utts = sorted(set(long_utts) | {B})
    return long_utts


def resfuse_persist_cases(ncu):
    """[(name, make_gemm keywords, variant id, meta)]: launch_resfuse_persist_c with at least 5 tiles per workgroup, both length paths
    (LDS table for nbatch <= 128, scalar loads above), both 16-bit types, the four accumulator modes dealt over them."""
    T = []

    def epi(am, dt):
        kw = dict(accum_mode=am, accum_dtype=dt) if am else {}
        if am in (0, 1):
            kw.update(act=ACT_LRELU, slope=0.1, out_scale=1 / 3 if am else 1.0)
        else:
            kw.update(has_out=False)
        return kw
    # ---- nbatch = 128, utterances of many tiles (C = 32, k = 3): lengths from the LDS table
    C, k = 32, 3
    rows = resfuse_grid(C, k, 1, 1, ncu)["rows"]
    per = _cdiv(5 * ncu, 128) + 1
    while True:
        M = per * rows
        lens = [M - (i * 37) % rows for i in range(128)]
        for i, l in ((3, rows), (7, 1), (20, 2 * rows + 1), (21, 48), (64, rows + 1), (65, 17), (100, 3 * rows), (101, 5), (127, 30)):
            lens[i] = l
        g = resfuse_grid(C, k, M, 128, ncu)
        long_utts = [b for b, l in enumerate(lens) if l > rows]
        plan = walk_plan(strided_walk(g, 128, lens), 128, long_utts)
        if plan["trips"] >= PERSIST_TRIPS["resfuse"] and g["G"] % per:
            break
        per += 1
    for am in range(4):
        dt = DT_BF16 if am % 2 == 0 else DT_F16
        T.append((f"resfuse_persist_table_c32_k3_am{am}_{DT_NAME[dt]}",
                  dict(dtype=dt, M=M, N=C, K=C, nbatch=128, lens=lens, taps=taps_1d(k), dil1=5, fused=1, **epi(am, dt)), 16, dict(plan, grid=g, long=long_utts)))
    # ---- nbatch > 128, mostly one-tile utterances: lengths through scalar loads.  The tile count per utterance is coprime to the grid, so
    #      that every workgroup meets first tiles; tiles past a short utterance's end are the ones the walk skips
    for C, k, dil, ams in ((32, 3, 3, (0, 1, 2, 3)), (64, 7, 1, (1, 2)), (64, 11, 1, (3, 0))):
        rows = resfuse_grid(C, k, 1, 1, ncu)["rows"]
        per = _coprime_per(ncu)
        M = (per - 1) * rows + 40
        nbatch = 5 * ncu + 9
        while True:
            lens = _short_lens(nbatch)
            g = resfuse_grid(C, k, M, nbatch, ncu)
            long_utts = _place_long(lens, g["G"], per, rows, M)
            plan = walk_plan(strided_walk(g, nbatch, lens), nbatch, long_utts)
            if plan["trips"] >= PERSIST_TRIPS["resfuse"]:
                break
            nbatch += ncu // 4
        for i, am in enumerate(ams):
            dt = DT_F16 if (am + (C == 32)) % 2 == 0 else DT_BF16
            T.append((f"resfuse_persist_sload_c{C}_k{k}_am{am}_{DT_NAME[dt]}",
                      dict(dtype=dt, M=M, N=C, K=C, nbatch=nbatch, lens=lens, taps=taps_1d(k), dil1=dil, fused=1, **epi(am, dt)), 16 if C == 32 else 17,
                      dict(plan, grid=g, long=long_utts)))
    return T


def pairstream_persist_cases(ncu):
    """launch_pairstream with at least 3 segments per workgroup: 3 nwg + 7 one-segment utterances (see the section comment)."""
    T = []
    nbatch, M = 3 * ncu + 7, 48
    lens = _short_lens(nbatch)
    lens[10], lens[11] = M, M - 1
    g = pairstream_grid(M, nbatch, ncu)
    assert pairstream_grid(M, 1, ncu)["rows"] == g["rows"]                    # the alone launch cuts the same segments
    plan = walk_plan(strided_walk(g, nbatch, lens), nbatch, [])
    for i, (k, dil) in enumerate(((3, 1), (7, 3), (11, 5))):
        for dt in (DT_BF16, DT_F16):
            am = (i + (2 if dt == DT_F16 else 0)) % 4
            kw = dict(pair_seam_kw(dt, k, dil, am), M=M, nbatch=nbatch, lens=lens)
            T.append((f"pairstream_persist_k{k}_d{dil}_am{am}_{DT_NAME[dt]}", kw, 23, dict(plan, grid=g, long=[])))
    return T


K33 = dict(taps=[t % 3 - 1 for t in range(9)], du=[t // 3 - 1 for t in range(9)])


def conv2d_persist_cases(ncu):
    """conv2d_persist (both epilogue forms, C = 32 / 64, the fused SE pool) and conv2d_s2 (with and without the fused shortcut) with at
    least 3 tiles per workgroup and a short last round: maps of two tiles each, mostly 1 to 5 columns wide, a few as wide as the map."""
    T = []

    def add(name, vid, kind, C, hin, win, pool=False, **kw):
        two_d = kind == "s2"
        wout = (win - 1) // 2 + 1 if two_d else win
        M = ((hin - 1) // 2 + 1) * wout if two_d else hin * win
        g1 = conv2d_grid(kind, C, M, 1 << 20, ncu)
        nbatch = _cdiv(3 * g1["G"] + 5, g1["per"])
        g = conv2d_grid(kind, C, M, nbatch, ncu)
        assert g["per"] == 2 and g["G"] == g1["G"]
        lens = [1 + (i * 7) % 5 for i in range(nbatch)]
        A = 10
        B = (2 * A + g["G"]) // 2
        wide = [A, B, A + 3, B + 3, A + nbatch // 2]          # (the last one is met on a later trip: narrow-then-wide)
        for b in wide:
            lens[b] = win - 1
        lens[A + 3] = win - 2
        plan = walk_plan(dealt_walk(g, nbatch), nbatch, wide)
        kw = dict(dtype=DT_BF16, M=M, N=2 * C if two_d else C, K=C, nbatch=nbatch, lens=lens, wout=wout, hin=hin, win=win, **K33, **kw)
        T.append((name, kw, vid, dict(plan, grid=g, long=wide, pool=pool, kind=kind)))
    add("conv2d_persist_c32_relu_bn", 26, "persist", 32, 6, 66, flat=True, bias_mode=0, post=True, act=ACT_RELU)
    add("conv2d_persist_c32_bias", 26, "persist", 32, 6, 66, flat=True, bias_mode=1)
    add("conv2d_persist_c32_bias_pool", 26, "persist", 32, 6, 66, pool=True, flat=True, bias_mode=1)
    add("conv2d_persist_c64_relu_bn", 27, "persist", 64, 4, 66, flat=True, bias_mode=0, post=True, act=ACT_RELU)
    add("conv2d_persist_c64_bias", 27, "persist", 64, 4, 66, flat=True, bias_mode=1)
    add("conv2d_s2_ds_c32", 28, "s2", 32, 26, 41, stride=2, bias_mode=0, post=True, act=ACT_RELU, ds=True)
    add("conv2d_s2_c64", 29, "s2", 64, 18, 31, stride=2, bias_mode=0, post=True, act=ACT_RELU)
    return T


def gemm_persist_cases(ncu):
    return resfuse_persist_cases(ncu) + pairstream_persist_cases(ncu) + conv2d_persist_cases(ncu)


def build_persist_gemm(entry):
    """The Problem of a *_persist_cases entry: the NaN utterances hold NaN in every row, the reference covers meta['sample']."""
    name, kw, vid, meta = entry
    p = make_gemm(name, 0, **kw)
    d = p.d
    X = p.bufs["X"]["v"].reshape(d["nbatch"], -1)
    for b in meta["nan"]:
        X[b] = np.nan
    p.utts = set(meta["sample"])                             # whole utterances are sampled, every valid row of each
    p.sample = None
    p.nan_utts = tuple(meta["nan"])
    return p


def pool_ref(p, b):
    """conv2d_persist's fused squeeze-excite pool for utterance b: partial[s][n] = the sum over the valid positions (row < M, column < width)
    of rows [96 s, 96 s + 96) of the f32 convolution results BEFORE the bias, s < 4 ntm (C = 32: four waves of 96 rows per 384-row tile),
    and its bound: the accumulation bound of every summand plus an f32 sum of up to 96 of them in any order."""
    d = p.d
    rows = valid_out_rows(d, b)
    acc, mag, g = _conv(d, p.bufs["X"]["v"], b * d["x_bs"], d["ldx"], p.bufs["W"]["v"], 0, d["w_ts"], d["ldw"], b, rows, d["dv"], d["K"], d["N"])
    S = 4 * _cdiv(d["M"], 384)
    ref, tol = np.zeros((S, d["N"])), np.zeros((S, d["N"]))
    eacc = 0.0 if exact_f32(mag, g) else 2 * d["ntaps"] * d["K"] * U
    for s in range(S):
        m = (rows >= 96 * s) & (rows < 96 * s + 96)
        ref[s] = acc[m].sum(axis=0)
        tol[s] = eacc * mag[m].sum(axis=0) + 2 * 96 * U * np.abs(acc[m]).sum(axis=0)
    return ref, tol


def chain_persist_cases(ncu):
    """[(name, make_chain keywords, variant id, meta)] for launch_narrowstage (utterances of one to three tiles over a tile count coprime
    to the grid) and launch_resstream (one-segment utterances, every form of the launcher), at least 3 units per workgroup."""
    T = []
    for C, dt in ((16, DT_BF16), (16, DT_F16), (8, DT_F16), (8, DT_BF16)):
        R = NS_R[C]
        G = ncu * NS_WGPC[C]
        per = _coprime_per(G)
        M = (per - 1) * R + 90
        nbatch = 3 * G + 9
        while True:
            lens = _short_lens(nbatch)
            g = narrow_grid(C, M, nbatch, ncu)
            long_utts = _place_long(lens, g["G"], per, R, M)
            plan = walk_plan(strided_walk(g, nbatch, lens), nbatch, long_utts)
            if plan["trips"] >= PERSIST_TRIPS["narrowstage"]:
                break
            nbatch += G // 4
        T.append((f"narrowstage_persist_c{C}_{DT_NAME[dt]}", dict(kind="narrowstage", dt=dt, C=C, blocks=[(k, (1, 3, 5)) for k in (3, 7, 11)], M=M,
                                                                 lens=lens, nan_utts=plan["nan"]), 24 if C == 16 else 25, dict(plan, grid=g, long=long_utts)))
    nbatch, M = 3 * ncu + 7, 64
    lens = _short_lens(nbatch)
    lens[10], lens[11] = M, M - 1
    for i, (C, k, dils) in enumerate(RS_FORMS):
        dt = DT_BF16 if i % 2 == 0 else DT_F16
        am = (i + (2 if i >= 4 else 0)) % 4
        g = resstream_grid(C, k, len(dils), M, nbatch, ncu)
        assert resstream_grid(C, k, len(dils), M, 1, ncu)["rows"] == g["rows"]     # the alone launch cuts the same segments
        plan = walk_plan(strided_walk(g, nbatch, lens), nbatch, [])
        T.append((f"resstream_persist_c{C}_k{k}_np{len(dils)}_am{am}_{DT_NAME[dt]}",
                  dict(kind="resstream", dt=dt, C=C, blocks=[(k, dils)], M=M, lens=lens, nan_utts=plan["nan"], ld_pad=8 if dt == DT_F16 else 0, **_rs_epi(am)),
                  20 if C == 32 else 21, dict(plan, grid=g, long=[])))
    return T


def sub_chain(cs, utts):
    """The ChainCase of utterances `utts` alone, cropped to their longest (utterances do not see each other)."""
    utts = list(utts)
    Ms = max(cs.lens[b] for b in utts)
    kw = dict(cs.__dict__)
    kw.update(X=cs.X[utts, :Ms], lens=[cs.lens[b] for b in utts], xs=None if cs.xs is None else cs.xs[utts, :Ms], nan_utts=(), M=Ms)
    return ChainCase(**kw)


# ---- the resampler's launch geometry (launch_resample_poly / resample_geometry_of) ----
def resample_geometry(lib, rate_in, rate_out, B, out_max):
    """The shim's dry run: dict(L, M, T, pitch, tile, tpb, xcap, lds, fits)."""
    lib.zvxk_resample_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.POINTER(ctypes.c_int)]
    g = (ctypes.c_int * 8)()
    ok = lib.zvxk_resample_geometry(rate_in, rate_out, B, out_max, g)
    d = dict(zip(("L", "M", "T", "pitch", "tile", "tpb", "xcap", "lds"), (int(v) for v in g)))
    d["fits"] = bool(ok)
    return d


def resample_geometry_ref(L, M, T, pitch, B, out_max):
    """The rule restated: the bank [L][pitch] (padded to 4 floats) and one tile's input span share at most 96 KiB; the tile halves from
    1024 until they do; tpb = min(8, max(1, tiles B / 2048))."""
    nbank = (L * pitch + 3) & ~3
    cap = lambda t: ((t - 1) * M // L + T + 12) & ~3
    tile = 1024
    while tile > 4 and (nbank + cap(tile)) * 4 > 96 * 1024:
        tile >>= 1
    tiles = _cdiv(out_max, tile)
    return dict(tile=tile, tpb=min(8, max(1, tiles * B // 2048)), xcap=cap(tile), lds=(nbank + cap(tile)) * 4)
