"""Float64 restatement of include/zvx.h's alignment block (zvx_dtw, zvx_align_wav).  It never calls the library.

The recurrence has one addition per cell, so there is no order freedom beyond the local distance: sweeping the anti-diagonals with NumPy
gives the values a cell-by-cell loop gives."""
import math

import numpy as np

AMBIGUITY = 1e-9


def local_distance(a, b):
    """d[i][j] = sqrt(sum_k (a[i][k] - b[j][k])^2) in float64, the sum over k in ascending order"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if b.ndim == 1:
        b = b[:, None]
    acc = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for k in range(a.shape[1]):
        df = a[:, k][:, None] - b[:, k][None, :]
        acc += df * df
    return np.sqrt(acc)


def accumulate(d):
    """C of the recurrence over a local-distance matrix, swept along the anti-diagonals; a missing neighbour is +inf"""
    Ta, Tb = d.shape
    C = np.full((Ta + 1, Tb + 1), np.inf)                # C[i + 1][j + 1] = C(i, j); row 0 and column 0 are the missing neighbours
    C[1, 1] = d[0, 0]
    for s in range(1, Ta + Tb - 1):
        i = np.arange(max(0, s - (Tb - 1)), min(s, Ta - 1) + 1)
        j = s - i
        C[i + 1, j + 1] = d[i, j] + np.minimum(np.minimum(C[i, j], C[i, j + 1]), C[i + 1, j])
    return C[1:, 1:]


def backtrack(C):
    """-> (path [L][2] forward, ambiguous: the on-path cells whose decision has its two smallest candidates within a relative AMBIGUITY)"""
    i, j = C.shape[0] - 1, C.shape[1] - 1
    cells, ambiguous = [(i, j)], []
    while i or j:
        cand = [C[i - 1, j - 1] if i and j else np.inf, C[i - 1, j] if i else np.inf, C[i, j - 1] if j else np.inf]
        k = int(np.argmin(cand))                         # (the first of equal minima: diagonal, then (i-1, j), then (i, j-1))
        lo, nxt = sorted(cand)[:2]
        if np.isfinite(nxt) and abs(nxt - lo) <= AMBIGUITY * max(abs(lo), abs(nxt)):
            ambiguous.append((i, j))
        if k != 2:
            i -= 1
        if k != 1:
            j -= 1
        cells.append((i, j))
    return np.array(cells[::-1], np.int32), ambiguous


def a2b_of(path, Ta):
    out = np.zeros((Ta, 2), np.int32)
    out[:, 0] = np.iinfo(np.int32).max
    out[:, 1] = -1
    for i, j in np.asarray(path):
        out[i, 0] = min(out[i, 0], j)
        out[i, 1] = max(out[i, 1], j)
    return out


def dtw(a, b):
    """-> dict(cost, path, a2b, ambiguous) of one pair"""
    C = accumulate(local_distance(a, b))
    path, ambiguous = backtrack(C)
    return {"cost": float(C[-1, -1]), "path": path, "a2b": a2b_of(path, C.shape[0]), "ambiguous": ambiguous}


def valid_path(path, Ta, Tb):
    """starts at (0, 0), ends at (Ta-1, Tb-1), every step is one of (1, 1), (1, 0), (0, 1)"""
    p = np.asarray(path, np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or len(p) == 0 or tuple(p[0]) != (0, 0) or tuple(p[-1]) != (Ta - 1, Tb - 1):
        return False
    st = np.diff(p, axis=0)
    return bool(np.all((st >= 0) & (st <= 1)) and np.all(st.sum(axis=1) >= 1))


def path_cost(a, b, path):
    """the sum of d over the cells of any valid path, accumulated in path order as the recurrence does"""
    d = local_distance(a, b)
    total = None
    for i, j in np.asarray(path):
        total = d[i, j] if total is None else d[i, j] + total
    return float(total)


def brute_force(d):
    """the smallest cost over ALL monotone paths of a small matrix, by enumeration -> (cost, the set of optimal paths)"""
    Ta, Tb = d.shape
    best, arg = np.inf, []

    def walk(i, j, cells):
        nonlocal best, arg
        if (i, j) == (Ta - 1, Tb - 1):
            c = d[0, 0]
            for (u, v) in cells[1:]:
                c = d[u, v] + c
            if c < best:
                best, arg = c, [list(cells)]
            elif c == best:
                arg.append(list(cells))
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Ta and j + dj < Tb:
                walk(i + di, j + dj, cells + [(i + di, j + dj)])

    walk(0, 0, [(0, 0)])
    return float(best), arg


def cost_bound(Ta, Tb, dim, cost_ref):
    """the derived bound of the header: 2 (Ta + Tb + dim) 2^-53 cost_ref"""
    return 2.0 * (Ta + Tb + dim) * 2.0 ** -53 * abs(cost_ref)


def cepstra(logmel, n_cep):
    """c[t][k-1] = sqrt(2 / M) sum_m L[t][m] cos(pi k (m + 1/2) / M), k = 1 .. n_cep, in float64 (not rounded to f32)"""
    L = np.asarray(logmel, np.float64)
    M = L.shape[-1]
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    table = np.cos(np.pi * k * (m + 0.5) / M)
    return math.sqrt(2.0 / M) * (L @ table.T)


def mcd_db(cost, path_len):
    return (10.0 / math.log(10.0)) * math.sqrt(2.0) * float(cost) / float(path_len)


# ---- the seeded cases of tests/test_align_gpu.py; tests/test_align.py asserts on the CPU that none holds an ambiguous on-path decision ----
SHAPES = [(1, 1, 1), (1, 5, 3), (5, 1, 3), (2, 2, 1),
          (63, 65, 13), (64, 64, 13), (65, 63, 13),
          (255, 300, 13), (256, 257, 13), (257, 40, 32),
          (1025, 7, 2), (7, 1025, 2)]
RAGGED = [(65, 63, 13), (255, 300, 13), (64, 64, 13)]   # one batch of three of them inside a larger Tamax / Tbmax, NaN in the padding
BIG = (4096, 4096, 13)


def case(Ta, Tb, dim, seed=0):
    """seeded Gaussian f32 features of one pair"""
    rng = np.random.default_rng([Ta, Tb, dim, seed])
    return rng.standard_normal((Ta, dim)).astype(np.float32), rng.standard_normal((Tb, dim)).astype(np.float32)


def integer_case(Ta=40, Tb=50, seed=0):
    """dim 1, values 0 .. 3: full of exact ties, every distance a small integer"""
    rng = np.random.default_rng([Ta, Tb, seed, 7])
    return rng.integers(0, 4, (Ta, 1)).astype(np.float32), rng.integers(0, 4, (Tb, 1)).astype(np.float32)
