"""A float64 restatement of the voice matching contract (include/zvx.h: zvx_spk_score, zvx_spk_topk).  It never calls the library.

    score(b, k) = dot(q_b, e_k) / max(|q_b| |e_k|, FLT_MIN);   a score that is not finite is -2
    topk: per query the `top` largest scores, by descending score and by ascending index among equal scores

The bound tol(dim) = (2 dim + 8) 2^-24 on |f32 result - float64 result|, for round-to-nearest f32 accumulation in ANY order and
|score| <= 1, with u = 2^-24:
  * the dot product: each of the dim products and each of the dim additions is rounded once; relative to sum |q_i e_i| <= |q| |e| the
    accumulated error of a sum of dim terms is below dim u (first order), so it moves the score by at most dim u;
  * the two sums of squares have the same bound dim u each, relative to themselves; the square root halves a relative error, so each norm
    is off by at most dim u / 2, and the two together move the score by at most dim u;
  * a few u cover what is rounded once per score: the two square roots, the product of the norms (or the scaling of the query by one
    of them, which is one rounding per element but relative, so u on the dot product), the division and a reciprocal of 1 ulp: 8 u."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)                   # 2^-126
NOT_FINITE = -2.0


def tol(dim):
    return (2 * int(dim) + 8) * 2.0 ** -24


def scores(q, lib):
    """q [B][dim], lib [K][dim] (any float type; read as the float32 values they hold) -> float64 [B][K]"""
    q = np.asarray(q, np.float32).astype(np.float64)
    lib = np.asarray(lib, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        dot = np.einsum("bd,kd->bk", q, lib)
        # a product with a NaN or inf factor is not finite even where einsum's order would let another term dominate
        bad = (~np.isfinite(q).all(axis=1))[:, None] | (~np.isfinite(lib).all(axis=1))[None, :]
        nq = np.sqrt((q * q).sum(axis=1))
        ne = np.sqrt((lib * lib).sum(axis=1))
        s = dot / np.maximum(nq[:, None] * ne[None, :], FLT_MIN)
    s = np.where(bad | ~np.isfinite(s), NOT_FINITE, s)
    return s


def topk(s, top):
    """s [B][K] -> (score [B][top], index [B][top] int32): descending score, ascending index among equal scores"""
    s = np.asarray(s)
    B, K = s.shape
    assert 1 <= top <= K
    idx = np.empty((B, top), np.int32)
    for b in range(B):
        order = np.lexsort((np.arange(K), -s[b].astype(np.float64)))       # last key first: by -score, then by index
        idx[b] = order[:top]
    return np.take_along_axis(s, idx.astype(np.int64), axis=1), idx


def min_gap(s, top):
    """the smallest gap among each query's best top + 1 float64 scores, over all queries: where it exceeds 2 tol, a result within tol
    selects the same rows in the same order"""
    s = np.asarray(s, np.float64)
    best = -np.sort(-s, axis=1)[:, :top + 1]
    return float(np.min(best[:, :-1] - best[:, 1:]))
