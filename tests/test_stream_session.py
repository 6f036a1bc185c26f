"""Stream sessions (include/zvx.h: zvx_stream_open / zvx_stream_next), no GPU needed: the C++ planners of csrc/stream_plan.h against
the Python planners they restate, and the surface (header, bindings, exports)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from zerovox_amd import _lib, resample as RSM, stream as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "stream_plan_main.cpp")
REACHES = [0, 1, 231, 1023, 4095]
RATES = [(22050, 48000), (22050, 8000), (22050, 22050)]
BIG = 2 ** 32 + 5
FUNCS = ("zvx_stream_open", "zvx_stream_next", "zvx_stream_info", "zvx_stream_close")


def push_patterns(R, seed):
    """the push patterns of tests/test_stream.py: all ones, fixed 64, random, one big push"""
    rng = np.random.default_rng(seed)
    return [[1] * (2 * R + 52), [64] * 80, [int(v) for v in rng.integers(1, 3 * R + 5, 60)], [5 * R + 5]]


def sequences(R, seed):
    """every pattern closed by push(0, last) and with its last push flagged last, then both again behind a first push of 2^32 + 5"""
    out = []
    for sizes in push_patterns(R, seed):
        for lead in ([], [BIG]):
            out.append([(n, False) for n in lead + sizes] + [(0, True)])
            out.append([(n, False) for n in lead + sizes[:-1]] + [(sizes[-1], True)])
    return out


@pytest.fixture(scope="module")
def planner_exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan") / "stream_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", MAIN, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def run_planner(exe, head, seqs, make):
    """feeds every sequence to a fresh C++ planner (`head` starts one) and to make() -> asserts the steps equal line by line"""
    text, want = [], []
    for seq in seqs:
        text.append(head)
        p = make()
        for n, last in seq:
            text.append(f"push {n} {int(last)}")
            want.append(" ".join(str(int(v)) for v in p.push(n, last)))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (head, i, g, w)


@pytest.mark.parametrize("R", REACHES)
def test_reach_planner_equals_the_python_planner(planner_exe, R):
    run_planner(planner_exe, f"reach {R}", sequences(R, R), lambda: S.ReachPlanner(R))


@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_resample_planner_equals_the_python_planner(planner_exe, rate_in, rate_out):
    half = RSM.rate_pair(rate_in, rate_out)[2]
    run_planner(planner_exe, f"rate {rate_in} {rate_out}", sequences(half // 8, rate_out), lambda: RSM.StreamPlanner(rate_in, rate_out))


@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_history_and_piece_bounds_of_the_conversion(rate_in, rate_out):
    """what zvx_stream_open sizes the conversion's buffers and max_piece from: at most 2 half / L + 2 retained samples, and a push of n
    samples emits at most ceil((n + ceil(half / L) + 1) L / M) outputs"""
    L, M, half = RSM.rate_pair(rate_in, rate_out)
    reach = -(-half // L) + 1 if half else 0
    for seq in sequences(half // 8, 7):
        p = RSM.StreamPlanner(rate_in, rate_out)
        for n, last in seq:
            _, _, count, keep = p.push(n, last)
            assert p.received - keep <= 2 * half // L + 2
            assert count <= -(-(n + reach) * L // M)


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


def test_header_declares_the_session():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"typedef\s+struct\s+zvx_stream\s+zvx_stream\s*;", code)
    m = re.search(r"typedef struct zvx_stream_params \{(.*?)\} zvx_stream_params;", code, flags=re.S)
    assert m, "zvx_stream_params not declared"
    fields = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
    assert fields == ["int32_t chunk_frames", "int32_t chunks_per_call", "int32_t halo", "const zvx_denoise_params* denoise",
                      "const float* denoise_bias", "const zvx_limit_params* limit"], fields
    decl = {n: " ".join(re.search(r"zvx_status\s+%s\s*\(([^;]*)\)\s*;" % n, code).group(1).split()) for n in FUNCS}
    assert decl["zvx_stream_open"] == "zvx_ctx* ctx, const float* mel, int frames, const zvx_stream_params* params, int flags, zvx_stream** out"
    assert decl["zvx_stream_next"] == "zvx_stream* s, void* out, int64_t capacity, int64_t* n_out, int32_t* done, int flags"
    assert decl["zvx_stream_info"] == "const zvx_stream* s, int64_t* info, int n_info"
    assert decl["zvx_stream_close"] == "zvx_stream* s"
    assert '"voc.stream"' in h and "bit for bit the concatenation of ZeroVox.vocode_stream" in h and "NOTHING consumed" in h


def test_bindings_and_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    for name in FUNCS:
        assert name in _lib.EXPORTS, name
    assert [f[0] for f in _lib.StreamParams._fields_] == ["chunk_frames", "chunks_per_call", "halo", "denoise", "denoise_bias", "limit"]
    assert C.sizeof(_lib.StreamParams) == 40
    p = inspect.signature(_lib.Context.stream_open).parameters
    assert p["mel"].default is None and p["frames"].default == 0 and p["chunk_frames"].default is inspect.Parameter.empty
    assert p["chunks_per_call"].default == 1 and p["halo"].default == 16 == ZeroVox.STREAM_HALO
    assert all(p[k].default is None for k in ("denoise", "bias", "limit"))
    assert inspect.signature(ZeroVox.vocode_stream).parameters["resident"].default is False
    assert inspect.signature(ZeroVoxTTS.tts_stream).parameters["resident"].default is False
    for name in ("info", "close", "__iter__", "next_piece", "next_device"):
        assert hasattr(_lib.Stream, name), name


def test_library_exports_the_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in FUNCS:
        assert hasattr(lib, name), name
    # a NULL context or session is refused before anything else is looked at
    lib.zvx_stream_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.zvx_stream_next.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    lib.zvx_stream_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.zvx_stream_close.argtypes = [C.c_void_p]
    assert lib.zvx_stream_open(None, None, 0, None, 0, None) == _lib.ZVX_E_INVALID
    assert lib.zvx_stream_next(None, None, 0, None, None, 0) == _lib.ZVX_E_INVALID
    assert lib.zvx_stream_info(None, None, 0) == _lib.ZVX_E_INVALID
    assert lib.zvx_stream_close(None) == _lib.ZVX_E_INVALID
