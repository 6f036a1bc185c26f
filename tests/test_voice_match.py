"""Voice matching without a GPU: the surface (header, bindings, exports, keywords), the float64 reference of tests/voice_ref.py against
torch in float64 and against mutations of itself, and the host logic of voices.VoiceLibrary over a fake context."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import voice_ref as V
from zerovox_amd import _lib, voices
from zerovox_amd.synthesize import ZeroVoxTTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN = np.float32(np.finfo(np.float32).tiny)


# ---- surface --------------------------------------------------------------------------------------------------------------
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zvx.h")).read(), flags=re.S)


def declared_args(name):
    m = re.search(r"zvx_status\s+" + name + r"\s*\(([^)]*)\)", header_code())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def ctype_of(arg):
    if "*" in arg:
        return C.c_void_p
    t = arg.rsplit(" ", 1)[0]
    return {"int": C.c_int, "int64_t": C.c_int64}[t]


@pytest.mark.parametrize("name", ["zvx_spk_score", "zvx_spk_topk"])
def test_header_declaration_matches_the_binding(name):
    lib = _lib.load()
    args = declared_args(name)
    assert [ctype_of(a) for a in args] == list(getattr(lib, name).argtypes), args
    assert name in _lib.EXPORTS
    assert getattr(lib, name) is not None


def test_header_constants_and_argument_order():
    hdr = open(os.path.join(ROOT, "include", "zvx.h")).read()
    assert re.search(r"#define\s+ZVX_SPK_TOP_MAX\s+32\b", hdr)
    assert _lib.ZVX_SPK_TOP_MAX == voices.TOP_MAX == 32
    assert [a.split()[-1].lstrip("*") for a in declared_args("zvx_spk_score")] == ["ctx", "query", "B", "lib", "K", "dim", "score", "flags"]
    assert [a.split()[-1].lstrip("*") for a in declared_args("zvx_spk_topk")] == ["ctx", "query", "B", "lib", "K", "dim", "top", "score", "index",
                                                                                 "flags"]
    kh = open(os.path.join(ROOT, "zerovox_amd", "csrc", "voicematch_kernels.h")).read()
    assert int(re.search(r"constexpr int SPK_SLAB = (\d+);", kh).group(1)) == voices.SLAB_ROWS
    assert int(re.search(r"constexpr int SPK_DIM_MAX = (\d+);", kh).group(1)) == voices.DIM_MAX
    # the launchers are declared in the unit's own header, not where tests/test_ops_reference.py scans
    assert "launch_spk_match" not in open(os.path.join(ROOT, "zerovox_amd", "csrc", "zvx_kernels.h")).read()


@pytest.mark.parametrize("fn", ["tts", "tts_ex", "tts_long"])
def test_voice_report_keyword_defaults_to_off(fn):
    p = inspect.signature(getattr(ZeroVoxTTS, fn)).parameters["voice_report"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert ZeroVoxTTS._voice_keywords(False) is None and ZeroVoxTTS._voice_keywords(True) == {}
    assert ZeroVoxTTS._voice_keywords({"top_db": 30.0}) == {"top_db": 30.0}
    with pytest.raises(ValueError, match="threshold"):
        ZeroVoxTTS._voice_keywords({"threshold": 0.5})      # there is none
    with pytest.raises(ValueError):
        ZeroVoxTTS._voice_keywords(0.5)
    sig = inspect.signature(ZeroVoxTTS.voice_report).parameters
    assert "min_similarity" not in sig and "threshold" not in sig
    assert voices.VoiceReport(0.5, 10, 0, 100).meets(0.5) and not voices.VoiceReport(0.5, 10, 0, 100).meets(0.51)


# ---- the reference --------------------------------------------------------------------------------------------------------
def ragged_cases():
    """(q, lib): ragged sizes, sides that are not normalised, tied rows, zero rows, tiny and huge rows"""
    out = []
    for seed, (B, K, dim) in enumerate([(1, 1, 4), (3, 7, 8), (2, 33, 36), (5, 65, 264), (4, 19, 528)]):
        rng = np.random.default_rng(100 + seed)
        q = rng.standard_normal((B, dim)).astype(np.float32) * np.float32(3.0)
        lib = (rng.standard_normal((K, dim)) * rng.uniform(0.1, 10.0, (K, 1))).astype(np.float32)
        if K >= 7:
            lib[5] = lib[1]                                  # a tie, bit for bit
            lib[3] = 0.0
            lib[2] *= np.float32(1e-20)
            lib[4] *= np.float32(1e18)
        out.append((q, lib))
    return out


def test_reference_against_torch_in_float64():
    for q, lib in ragged_cases():
        s = V.scores(q, lib)
        tq, tl = torch.from_numpy(q.astype(np.float64)), torch.from_numpy(lib.astype(np.float64))
        want = torch.nn.functional.cosine_similarity(tq[:, None, :], tl[None, :, :], dim=2, eps=0.0).numpy()
        zero = ~lib.any(axis=1)
        assert np.all(s[:, zero] == 0.0)                     # (torch gives NaN there: the FLT_MIN clamp is the contract's)
        assert np.max(np.abs(s[:, ~zero] - want[:, ~zero])) <= 1e-12
        for top in (1, min(5, lib.shape[0])):
            ts, ti = torch.topk(torch.from_numpy(s), top, dim=1)
            rs, ri = V.topk(s, top)
            assert np.max(np.abs(rs - ts.numpy())) <= 1e-12  # (the values; torch's order among ties is not defined)
            assert np.array_equal(rs, np.take_along_axis(s, ri.astype(np.int64), axis=1))
            for b in range(s.shape[0]):
                assert all(rs[b, i] > rs[b, i + 1] or (rs[b, i] == rs[b, i + 1] and ri[b, i] < ri[b, i + 1]) for i in range(top - 1))


def test_reference_clamp_and_not_finite_rule():
    q = np.array([[1e-30, 0, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4], [np.nan, 0, 0, 0]], np.float32)
    lib = np.array([[1e-30, 0, 0, 0], [1, 0, 0, 0], [np.inf, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    s = V.scores(q, lib)
    f = lambda v: float(np.float32(v))
    assert s[0, 0] == pytest.approx(f(1e-30) * f(1e-30) / V.FLT_MIN, rel=1e-12)    # |q| |e| < FLT_MIN: the clamp divides
    assert s[0, 1] == pytest.approx(1.0, rel=1e-12)
    assert np.all(s[1, [0, 1, 3]] == 0.0) and np.all(s[:, 3][:3] == 0.0)           # a zero row on either side scores 0
    assert np.all(s[:, 2] == -2.0) and np.all(s[3] == -2.0)                        # inf / NaN in the inputs


def mutated_scores(q, lib, what):
    q64, l64 = q.astype(np.float64), lib.astype(np.float64)
    nq, ne = np.sqrt((q64 * q64).sum(1)), np.sqrt((l64 * l64).sum(1))
    with np.errstate(all="ignore"):
        if what == "drop_last":
            dot = q64[:, :-1] @ l64[:, :-1].T
            return dot / np.maximum(nq[:, None] * ne[None, :], V.FLT_MIN)
        if what == "lib_not_normalised":
            return (q64 @ l64.T) / np.maximum(nq[:, None], V.FLT_MIN)
        if what == "clamp_zero":
            return np.nan_to_num((q64 @ l64.T) / np.maximum(nq[:, None] * ne[None, :], 0.0), nan=0.0, posinf=0.0, neginf=0.0)
    raise KeyError(what)


def mutated_topk(s, top, what):
    rs, ri = V.topk(s, top)
    if what == "ties_to_higher_index":
        K = s.shape[1]
        ri = np.stack([np.lexsort((-np.arange(K), -s[b]))[:top] for b in range(s.shape[0])]).astype(np.int32)
    elif what == "unsorted":
        ri = np.sort(ri, axis=1)                             # the right set, in index order
    return np.take_along_axis(s, ri.astype(np.int64), axis=1), ri


@pytest.mark.parametrize("what", ["drop_last", "lib_not_normalised", "clamp_zero"])
def test_score_mutations_leave_the_tolerance(what):
    cases = ragged_cases()
    tiny = np.array([[1e-25, 2e-25, 0, 0]], np.float32)      # |q| |e| below FLT_MIN: only the clamp tells
    cases.append((tiny, tiny.copy()))
    worst = 0.0
    for q, lib in cases:
        worst = max(worst, float(np.max(np.abs(mutated_scores(q, lib, what) - V.scores(q, lib)) / V.tol(q.shape[1]))))
    assert worst > 1.0, (what, worst)


@pytest.mark.parametrize("what", ["ties_to_higher_index", "unsorted"])
def test_topk_mutations_are_seen(what):
    seen = False
    for q, lib in ragged_cases():
        s = V.scores(q, lib)
        top = min(5, lib.shape[0])
        rs, ri = V.topk(s, top)
        ms, mi = mutated_topk(s, top, what)
        seen |= not np.array_equal(ri, mi) or bool(np.max(np.abs(rs - ms)) > V.tol(q.shape[1]))
    assert seen, what


def test_min_gap_and_tol():
    assert V.tol(528) == (2 * 528 + 8) * 2.0 ** -24
    s = np.array([[0.9, 0.1, 0.5, 0.45], [0.0, 0.3, 0.2, -2.0]])
    assert V.min_gap(s, 2) == pytest.approx(0.05)
    assert V.min_gap(s, 1) == pytest.approx(0.1)


# ---- VoiceLibrary over a fake context ---------------------------------------------------------------------------------------
class FakeCtx:
    """device memory as host byte arrays at made-up addresses; the searches are the reference's"""
    hidden = 8

    def __init__(self):
        self.mem, self.next, self.copies, self._h = {}, 0x10000, [], 1

    def _at(self, ptr, nbytes):
        for base, a in self.mem.items():
            if base <= ptr and ptr + nbytes <= base + a.size:
                return a[ptr - base:ptr - base + nbytes]
        raise AssertionError(f"[{ptr:#x}, +{nbytes}) is in no allocation")

    def dev_alloc(self, nbytes):
        p = self.next
        self.mem[p] = np.zeros(nbytes, np.uint8)
        self.next += (nbytes + 0xfff) & ~0xfff
        return p

    def dev_free(self, ptr):
        del self.mem[ptr]

    def dev_from_host(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._at(ptr, arr.nbytes)[:] = arr.view(np.uint8).reshape(-1)

    def dev_copy(self, dst, src, nbytes):
        self.copies.append((dst, src, nbytes))
        self._at(dst, nbytes)[:] = self._at(src, nbytes).copy()

    def dev_to_host(self, ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self._at(ptr, n).copy().view(dtype).reshape(shape)

    def spk_score(self, q, lib_ptr, K, dim=None):
        return V.scores(q, self.dev_to_host(lib_ptr, (K, dim), np.float32)).astype(np.float32)

    def spk_topk(self, q, lib_ptr, K, top=5, dim=None):
        return V.topk(self.spk_score(q, lib_ptr, K, dim), top)


def embeddings(n, dim=8, seed=0):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def test_library_add_grow_remove():
    ctx = FakeCtx()
    lib = voices.VoiceLibrary(ctx, capacity=2)
    e = embeddings(5)
    assert lib.dim == 8 and len(lib) == 0 and lib.embeddings().shape == (0, 8)
    assert lib.add(["a", "b"], e[:2]) == [0, 1] and lib.capacity == 2 and not ctx.copies
    first = lib.ptr
    assert lib.add(["c", "d", "e"], e[2:, None, :]) == [2, 3, 4]              # [n][1][dim] too
    assert lib.capacity == 8 and lib.ptr != first and first not in ctx.mem    # doubled until it fits, the old buffer freed
    assert ctx.copies == [(lib.ptr, first, 2 * 8 * 4)]                        # one device-to-device copy of the rows in use
    assert lib.names == ["a", "b", "c", "d", "e"] and np.array_equal(lib.embeddings(), e)
    lib.remove("b")                                                           # the last row moves into the hole
    assert lib.names == ["a", "e", "c", "d"] and np.array_equal(lib.embeddings(), e[[0, 4, 2, 3]])
    lib.remove("d")                                                           # the last row itself: nothing moves
    assert lib.names == ["a", "e", "c"] and len(ctx.copies) == 2
    got = lib.match(e[[4, 2]], top=2)
    assert [m[0].name for m in got] == ["e", "c"] and [m[0].index for m in got] == [1, 2]
    assert all(abs(m[0].score - 1.0) < 1e-6 and m[0].score >= m[1].score for m in got)
    assert lib.add(["b"], e[1]) == [3]                                        # one [dim] row; a removed name may come back
    hits = lib.screen(e[1], 0.999)
    assert [[m.name for m in h] for h in hits] == [["b"]]
    lib.close()
    assert not ctx.mem


def test_library_save_load_round_trip(tmp_path):
    ctx = FakeCtx()
    lib = voices.VoiceLibrary(ctx, dim=12, capacity=4)
    e = embeddings(3, 12, seed=3)
    lib.add(["anna", "björn", "c d"], e)
    path = str(tmp_path / "voices.npz")
    lib.save(path)
    assert os.path.exists(path)                                               # exactly the path given, no suffix added
    back = voices.VoiceLibrary.load(FakeCtx(), path)
    assert back.names == lib.names and back.dim == 12
    assert np.array_equal(back.embeddings().view(np.uint32), e.view(np.uint32))


def test_library_value_errors():
    ctx = FakeCtx()
    for dim in (0, 2, 6, 2052):
        with pytest.raises(ValueError, match="dim"):
            voices.VoiceLibrary(ctx, dim=dim)
    with pytest.raises(ValueError, match="capacity"):
        voices.VoiceLibrary(ctx, capacity=0)
    lib = voices.VoiceLibrary(ctx)
    e = embeddings(3)
    lib.add(["a", "b"], e[:2])
    before = (lib.names, lib.embeddings().copy())
    with pytest.raises(ValueError, match="already"):
        lib.add(["c", "a"], e[:2])
    with pytest.raises(ValueError, match="already"):
        lib.add(["c", "c"], e[:2])
    with pytest.raises(ValueError, match=r"\[n\]\[8\]"):
        lib.add(["c"], np.zeros((1, 12), np.float32))
    with pytest.raises(ValueError, match="names"):
        lib.add(["c"], e[:2])
    with pytest.raises(ValueError, match="not in the library"):
        lib.remove("zz")
    for top in (0, 3, 33):
        with pytest.raises(ValueError, match="top"):
            lib.match(e[:1], top=top)
    with pytest.raises(ValueError, match="queries"):
        lib.match(np.zeros((1, 4), np.float32), top=1)
    with pytest.raises(ValueError, match="names"):
        lib.enroll(["x", "y"], [np.zeros(10, np.float32)])
    assert lib.names == before[0] and np.array_equal(lib.embeddings(), before[1])   # a refused call changes nothing
