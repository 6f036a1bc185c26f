"""Alignment without a GPU (include/zvx.h: zvx_dtw, zvx_align_wav): the surface (header, bindings, exports), the float64 restatement
tests/align_ref.py against a brute-force enumeration of all monotone paths, the rhythm arithmetic of align.durations_from on hand-made
alignments, the keyword checks of ZeroVoxTTS without a model, and -- from the reference alone -- that none of the seeded cases of
tests/test_align_gpu.py holds an ambiguous decision on its path, so that the path comparison on the device leaves no case out."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import align_ref as R
from zerovox_amd import _lib
from zerovox_amd import align as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decl(code, name):
    m = re.search(r"zvx_status\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
    assert m, f"{name} not declared"
    return " ".join(m.group(1).split()).replace(" ,", ",").replace("( ", "(")


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_both_calls_both_structs_and_the_enum():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert _decl(code, "zvx_dtw") == ("zvx_ctx* ctx, const float* a, const int32_t* Ta, int Tamax, const float* b, const int32_t* Tb, int Tbmax, "
                                      "int B, int dim, const zvx_dtw_params* params, double* cost, int32_t* path_len, int32_t* path, "
                                      "int64_t path_stride, int32_t* a2b, int flags")
    assert _decl(code, "zvx_align_wav") == ("zvx_ctx* ctx, const float* wav_a, const int32_t* n_a, int Nmax_a, const float* wav_b, const int32_t* n_b, "
                                            "int Nmax_b, int B, const zvx_align_params* params, double* stats, int32_t* path, int64_t path_stride, "
                                            "int32_t* a2b, int64_t a2b_stride, float* cep_a, float* cep_b, int64_t cep_stride, int flags")
    m = re.search(r"typedef struct zvx_dtw_params\s*\{([^}]*)\}\s*zvx_dtw_params;", code)
    assert m and " ".join(m.group(1).split()) == "int32_t reserved[4];"
    m = re.search(r"typedef struct zvx_align_params\s*\{([^}]*)\}\s*zvx_align_params;", code)
    assert m and " ".join(m.group(1).split()) == "int32_t n_cep; int32_t reserved[3];"
    m = re.search(r"enum\s*\{\s*(ZVX_AL_FRAMES_A[^}]*)\}", code)
    assert m and " ".join(m.group(1).split()) == "ZVX_AL_FRAMES_A = 0, ZVX_AL_FRAMES_B, ZVX_AL_PATH_LEN, ZVX_AL_COST, ZVX_AL_MCD_DB, ZVX_AL_COUNT = 5"
    for text in ("C(0, 0) = d(0, 0)", "AMBIGUOUS", "relative 1e-9", "(Ta + Tb + dim) 2^-53", "2 (Ta + Tb + dim) 2^-53 cost_ref", '"post.align"',
                 "diagonal-major", "48 KiB", "dim > 32", "above 4096", "B > 65535", "2^30", "Sakoe-Chiba", "soft-DTW",
                 "(10 / ln 10) sqrt(2) COST / PATH_LEN", "SPTK / WORLD", "no perceptual", "c0 is left out", "one\n *      f32 ulp"):
        assert text in h, text


def test_binding_exports_and_python_entry_points():
    assert "zvx_dtw" in _lib.EXPORTS and "zvx_align_wav" in _lib.EXPORTS
    assert (_lib.ZVX_AL_FRAMES_A, _lib.ZVX_AL_FRAMES_B, _lib.ZVX_AL_PATH_LEN, _lib.ZVX_AL_COST, _lib.ZVX_AL_MCD_DB, _lib.ZVX_AL_COUNT) == tuple(range(6))
    assert C.sizeof(_lib.DtwParams) == 16 and C.sizeof(_lib.AlignParams) == 16
    assert _lib.AlignParams._fields_[0] == ("n_cep", C.c_int32)
    lib = _lib.load()
    vp = C.c_void_p
    assert lib.zvx_dtw.argtypes == [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(_lib.DtwParams), vp, vp, vp, C.c_int64, vp, C.c_int]
    assert lib.zvx_align_wav.argtypes == [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(_lib.AlignParams), vp, vp, C.c_int64, vp, C.c_int64,
                                          vp, vp, C.c_int64, C.c_int]
    p = inspect.signature(_lib.Context.dtw).parameters
    assert list(p) == ["self", "a", "b", "lengths_a", "lengths_b", "path"] and [p[k].default for k in list(p)[3:]] == [None, None, True]
    p = inspect.signature(_lib.Context.align).parameters
    assert list(p) == ["self", "rows_a", "rows_b", "n_cep", "lengths_a", "lengths_b", "cepstra"]
    assert [p[k].default for k in list(p)[3:]] == [13, None, None, False]
    assert hasattr(_lib.Context, "dtw_device")
    assert (_lib.DTW_MAX_FRAMES, _lib.DTW_MAX_DIM) == (4096, 32)


def test_library_exports_the_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    lib.zvx_dtw.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64, vp, C.c_int]
    lib.zvx_align_wav.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, C.c_int]
    assert lib.zvx_dtw(None, None, None, 0, None, None, 0, 0, 0, None, None, None, None, 0, None, 0) == _lib.ZVX_E_INVALID          # a NULL context
    assert lib.zvx_align_wav(None, None, None, 0, None, None, 0, 0, None, None, None, 0, None, 0, None, None, 0, 0) == _lib.ZVX_E_INVALID


def test_feature_rows_of_the_binding():
    x, T = _lib.Context._feature_rows([np.ones((3, 2)), np.zeros((5, 2))], None)
    assert x.shape == (2, 5, 2) and x.dtype == np.float32 and T.tolist() == [3, 5] and x[0, 3:].sum() == 0
    x, T = _lib.Context._feature_rows([np.arange(4.0)], None)               # a 1-D row is [T][1]
    assert x.shape == (1, 4, 1)
    with pytest.raises(ValueError):
        _lib.Context._feature_rows([np.ones((3, 2)), np.zeros((5, 3))], None)
    x, T = _lib.Context._feature_rows(np.zeros((2, 7, 3)), [7, 2])
    assert x.shape == (2, 7, 3) and T.tolist() == [7, 2]


# ------------------------------------------------------------------------------------------------ the reference against brute force
@pytest.mark.parametrize("Ta", [1, 2, 3, 4, 5])
def test_reference_finds_the_optimum_of_all_monotone_paths(Ta):
    for Tb in range(1, 6):
        for seed in range(3):
            a, b = R.case(Ta, Tb, 2, seed)
            r = R.dtw(a, b)
            best, arg = R.brute_force(R.local_distance(a, b))
            assert r["cost"] == best, (Ta, Tb, seed)         # one addition per cell in path order: the same doubles
            assert R.valid_path(r["path"], Ta, Tb) and R.path_cost(a, b, r["path"]) == best
            assert [tuple(c) for c in r["path"]] in arg
            assert np.array_equal(r["a2b"], R.a2b_of(r["path"], Ta)) and (r["a2b"][:, 0] <= r["a2b"][:, 1]).all()
        ai, bi = R.integer_case(Ta, Tb, Ta * 7 + Tb)         # exact ties: the reference takes the diagonal, then (i-1, j), then (i, j-1)
        r = R.dtw(ai, bi)
        best, arg = R.brute_force(R.local_distance(ai, bi))
        assert r["cost"] == best and [tuple(c) for c in r["path"]] in arg


def test_reference_tie_order_and_ambiguity():
    a = np.zeros((3, 1), np.float32)
    r = R.dtw(a, a)
    assert r["cost"] == 0.0 and r["path"].tolist() == [[0, 0], [1, 1], [2, 2]]
    assert r["ambiguous"] == [(2, 2), (1, 1)]                # all three candidates are 0: the decision is a tie, the diagonal is taken
    r = R.dtw(np.zeros((1, 1)), np.zeros((3, 1)))
    assert r["path"].tolist() == [[0, 0], [0, 1], [0, 2]] and r["ambiguous"] == [] and r["a2b"].tolist() == [[0, 2]]
    assert R.cost_bound(4096, 4096, 13, 1.0) < 2e-12
    assert math.isclose(R.mcd_db(13.0, 10), 10.0 / math.log(10.0) * math.sqrt(2.0) * 1.3)
    c = R.cepstra(np.ones((2, 80)), 13)                      # a flat log-mel has no cepstrum beyond c0
    assert c.shape == (2, 13) and np.abs(c).max() < 1e-13


def test_the_gpu_cases_hold_no_ambiguous_decision():
    """every seeded case of tests/test_align_gpu.py, the 4096 x 4096 pair included: from the reference alone"""
    for Ta, Tb, dim in R.SHAPES + R.RAGGED + [R.BIG]:
        r = R.dtw(*R.case(Ta, Tb, dim))
        assert r["ambiguous"] == [], (Ta, Tb, dim, r["ambiguous"][:3])
        assert R.valid_path(r["path"], Ta, Tb)
    ai, bi = R.integer_case()
    r = R.dtw(ai, bi)
    assert r["ambiguous"] and r["cost"] == round(r["cost"])  # the integer case IS full of ties, and its optimum is an integer


# ------------------------------------------------------------------------------------------------ Alignment, durations_from
def _alignment(path, fa, fb):
    path = np.array(path, np.int32)
    return A.Alignment(cost=1.0, mcd_db=2.0, frames_a=fa, frames_b=fb, path=path, a2b=R.a2b_of(path, fa))


def test_alignment_meets_takes_the_callers_number():
    al = _alignment([(i, i) for i in range(4)], 4, 4)
    assert al.meets(2.0) and al.meets(2.5) and not al.meets(1.99)
    assert "max_mcd_db" in inspect.signature(A.Alignment.meets).parameters
    assert inspect.signature(A.Alignment.meets).parameters["max_mcd_db"].default is inspect.Parameter.empty
    res = dict(cost=[3.0], mcd_db=[1.5], frames_a=[2], frames_b=[3], path=[np.array([[0, 0], [1, 1], [1, 2]])], a2b=[np.array([[0, 0], [1, 2]])])
    al = A.Alignment.from_result(res)
    assert (al.cost, al.mcd_db, al.frames_a, al.frames_b) == (3.0, 1.5, 2, 3) and al.path.dtype == np.int32 and al.a2b.tolist() == [[0, 0], [1, 2]]


def test_durations_from_identity_and_stretch():
    d = [3, 0, 2, 5, 1]
    diag = _alignment([(i, i) for i in range(11)], 11, 11)
    assert A.durations_from(diag, d).tolist() == d
    twice = _alignment([(i // 2, i) for i in range(22)], 11, 22)
    out = A.durations_from(twice, d)
    assert out.tolist() == [6, 0, 4, 10, 2] and out.sum() == 22 and out.dtype == np.int32
    half = _alignment([(i, i // 2) for i in range(12)], 12, 6)
    assert A.durations_from(half, [4, 4, 4]).tolist() == [2, 2, 2]


def test_durations_from_zero_durations_min_frames_and_total():
    # a's frames 0 .. 5 all sit on b's frame 0, the rest of b belongs to a's last frame: the boundaries collapse to 0
    path = [(i, 0) for i in range(6)] + [(5, j) for j in range(1, 10)]
    al = _alignment(path, 6, 10)
    assert A.durations_from(al, [2, 0, 2, 2]).tolist() == [1, 0, 1, 8]       # the forward pass gives 1 frame each; zeros stay zero
    assert A.durations_from(al, [2, 0, 2, 2], min_frames=3).tolist() == [3, 0, 3, 4]
    assert A.durations_from(al, [2, 0, 2, 2], min_frames=0).tolist() == [0, 0, 0, 10]
    # the other way round: everything but a's first frame sits on b's last frame; the backward pass makes room
    path = [(0, j) for j in range(10)] + [(i, 9) for i in range(1, 6)]
    al = _alignment(path, 6, 10)
    assert A.durations_from(al, [2, 0, 2, 2]).tolist() == [8, 0, 1, 1]
    assert A.durations_from(al, [2, 0, 2, 2], min_frames=3).tolist() == [4, 0, 3, 3]
    for m in (0, 1, 2, 3):
        out = A.durations_from(al, [2, 0, 2, 2], min_frames=m)
        assert out.sum() == 10 and out[1] == 0 and (out[[0, 2, 3]] >= m).all()
    rng = np.random.default_rng(5)
    for _ in range(20):                                      # seeded alignments: the total is frames_b, zeros stay, every other has min_frames
        a, b = R.case(int(rng.integers(8, 30)), int(rng.integers(8, 30)), 2, int(rng.integers(100)))
        r = R.dtw(a, b)
        al = A.Alignment(r["cost"], 0.0, len(a), len(b), r["path"], r["a2b"])
        d = rng.multinomial(len(a), np.ones(6) / 6)
        out = A.durations_from(al, d)
        assert out.sum() == len(b) and (out[d == 0] == 0).all() and (out[d > 0] >= 1).all()


def test_durations_from_refuses_what_does_not_fit():
    al = _alignment([(i, min(i, 2)) for i in range(6)], 6, 3)
    with pytest.raises(ValueError, match="do not fit"):
        A.durations_from(al, [2, 1, 1, 2])                   # four phonemes of at least one frame in three frames
    assert A.durations_from(al, [2, 2, 2]).tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="do not fit"):
        A.durations_from(al, [2, 2, 2], min_frames=2)
    with pytest.raises(ValueError, match="sum to"):
        A.durations_from(al, [2, 2, 1])


# ------------------------------------------------------------------------------------------------ ZeroVoxTTS without a model
def test_rhythm_keywords_default_to_off_and_refuse_speed():
    from zerovox_amd.synthesize import ZeroVoxTTS
    p = inspect.signature(ZeroVoxTTS.tts).parameters
    assert p["rhythm_from"].default is None and p["rhythm_rate"].default is None and p["rhythm_from"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (ZeroVoxTTS.tts_long, ZeroVoxTTS.tts_stream, ZeroVoxTTS.tts_ex):
        assert "rhythm_from" not in inspect.signature(fn).parameters
    p = inspect.signature(ZeroVoxTTS.fidelity_report).parameters
    assert list(p)[:4] == ["self", "wav", "ref_wav", "sampling_rate"] and p["sampling_rate"].default is None
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                   # no model: whatever touches it raises AttributeError, not ValueError
    assert synth.last_alignment is None
    with pytest.raises(ValueError, match="rhythm_from.*speed"):
        synth.tts("hello there", None, rhythm_from=np.zeros(8000, np.float32), speed=1.1)
    with pytest.raises(AttributeError):
        synth.tts("hello there", None, rhythm_from=np.zeros(8000, np.float32))
