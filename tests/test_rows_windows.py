"""Per-row windows (include/zvx.h: zvx_denoise_rows, zvx_limit_rows), no GPU needed: the surface (header, bindings, exports), the refusals
that need no context, and partition_classes of csrc/stream_plan.h -- how zvx_stream_next_many batches one kind of post stage over its
sessions -- against a Python restatement."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "stream_classes_main.cpp")


def header_code():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    return h, re.sub(r"/\*.*?\*/", "", h, flags=re.S)


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_both_calls_and_the_struct():
    h, code = header_code()
    m = re.search(r"typedef\s+struct\s+zvx_row_window\s*\{([^}]*)\}\s*zvx_row_window\s*;", code)
    assert m, "zvx_row_window not declared"
    assert " ".join(m.group(1).split()) == "int64_t in_origin, out_begin, out_count; int32_t last; int32_t reserved;"
    m = re.search(r"zvx_status\s+zvx_denoise_rows\s*\(([^;]*)\)\s*;", code)
    assert m, "zvx_denoise_rows not declared"
    assert " ".join(m.group(1).split()) == ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias, "
                                            "const zvx_denoise_params* params, void* out, int64_t out_stride, int flags, const zvx_row_window* win")
    m = re.search(r"zvx_status\s+zvx_limit_rows\s*\(([^;]*)\)\s*;", code)
    assert m, "zvx_limit_rows not declared"
    assert " ".join(m.group(1).split()) == ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, "
                                            "const zvx_limit_params* params, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags, "
                                            "const zvx_row_window* win")
    # the _ex calls keep their signatures
    assert re.search(r"zvx_denoise_ex\s*\([^;]*int64_t in_origin, int64_t out_begin, int64_t out_count, int last\)\s*;", code)
    assert re.search(r"zvx_limit_ex\s*\([^;]*int64_t in_origin, int64_t out_begin, int64_t out_count, int last\)\s*;", code)
    assert "reserved != 0" in h and '"post.stream"' in h and "zvx_resample_ex has another window contract" in h


def test_bindings_and_exports():
    assert "zvx_denoise_rows" in _lib.EXPORTS and "zvx_limit_rows" in _lib.EXPORTS
    assert C.sizeof(_lib.RowWindow) == 32
    assert [f[0] for f in _lib.RowWindow._fields_] == ["in_origin", "out_begin", "out_count", "last", "reserved"]
    lib = _lib.load()
    assert lib.zvx_denoise_rows.argtypes == lib.zvx_denoise.argtypes + [C.POINTER(_lib.RowWindow)]
    assert lib.zvx_limit_rows.argtypes == lib.zvx_limit.argtypes + [C.POINTER(_lib.RowWindow)]
    p = inspect.signature(_lib.Context.denoise_rows).parameters
    assert list(p) == ["self", "rows", "bias", "strength", "windows", "floor", "pcm16", "lengths"]
    assert (p["floor"].default, p["pcm16"].default, p["lengths"].default) == (0.0, False, None)
    p = inspect.signature(_lib.Context.limit_rows).parameters
    assert list(p)[:6] == ["self", "rows", "ceiling", "windows", "window_ms", "oversample"]
    assert (p["window_ms"].default, p["oversample"].default) == (5.0, 4)


def test_library_exports_the_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    assert hasattr(lib, "zvx_denoise_rows") and hasattr(lib, "zvx_limit_rows")
    lib.zvx_denoise_rows.argtypes = [vp] * 3 + [C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int, vp]
    lib.zvx_limit_rows.argtypes = [vp] * 3 + [C.c_int] * 3 + [vp, vp, C.c_int64, vp, vp, C.c_int, vp]
    assert lib.zvx_denoise_rows(None, None, None, 0, 0, None, None, None, 0, 0, None) == _lib.ZVX_E_INVALID      # a NULL context
    assert lib.zvx_limit_rows(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None) == _lib.ZVX_E_INVALID


def test_row_windows_helper():
    n = np.array([100, 50, 0], np.int32)
    win, out, cnt = _lib.Context._row_windows([(0, 0, -1, True), (1 << 33, (1 << 33) + 7, 20, False), (5, 5, 0, False)], n, 100, False)
    assert list(cnt) == [100, 20, 0] and out.shape == (3, 100) and out.dtype == np.float32
    assert (win[1].in_origin, win[1].out_begin, win[1].out_count, win[1].last, win[1].reserved) == (1 << 33, (1 << 33) + 7, 20, 0, 0)
    assert win[0].last == 1 and win[0].out_count == -1
    with pytest.raises(ValueError):
        _lib.Context._row_windows([(0, 0, -1, True)], n, 100, False)


# ------------------------------------------------------------------------------------------------ the partition
def build(tmp, name, sanitize):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp / name)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san + [MAIN, "-o", exe], check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def classes_exe(tmp_path_factory):
    """the stand-alone program, under the host compiler's address and undefined-behaviour sanitizers"""
    return build(tmp_path_factory.mktemp("classes"), "stream_classes_main", True)


def python_partition(cls):
    """groups in the order of their first member, members in call order; negative: no stage"""
    groups = {}
    for i, c in enumerate(cls):
        if c >= 0:
            groups.setdefault(c, []).append(i)                # (dicts keep insertion order: the first member's)
    return list(groups.values())


def cases():
    rng = np.random.default_rng(5)
    out = [[], [0], [-1], [-1] * 5,
           [3] * 8,                                            # all sessions equal
           list(range(8)), [7, 5, 3, 1, 0, 2, 4, 6],           # all different
           [0, 1, 0, 1, 2, 0, 2, 1],                           # interleaved classes
           [-1, 4, -1, 4, 9, -1, 9, -7],                       # sessions without a stage
           [0] * 64, list(range(64)), [i % 3 for i in range(64)], [(-1 if i % 5 == 0 else i % 4) for i in range(64)]]      # 64 sessions
    for _ in range(60):
        n = int(rng.integers(1, 65))
        out.append([int(v) for v in rng.integers(-2, int(rng.integers(1, 9)), n)])
    return out


def test_partition_equals_the_python_restatement(classes_exe):
    cs = cases()
    text = "".join("%d %s\n" % (len(c), " ".join(map(str, c))) for c in cs)
    r = subprocess.run([classes_exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    at = 0
    for c in cs:
        want = python_partition(c)
        assert lines[at] == "groups %d %d" % (len(want), sum(map(len, want))), (c, lines[at])
        got = [[int(v) for v in ln.split()] for ln in lines[at + 1:at + 1 + len(want)]]
        assert got == want, (c, got, want)
        at += 1 + len(want)
    assert at == len(lines)
    # the properties the batched stages rest on: every session with a stage exactly once, one class per group, first members ascending
    for c in cs:
        g = python_partition(c)
        assert sorted(i for m in g for i in m) == [i for i, v in enumerate(c) if v >= 0]
        assert all(len({c[i] for i in m}) == 1 and m == sorted(m) for m in g) and [m[0] for m in g] == sorted(m[0] for m in g)
