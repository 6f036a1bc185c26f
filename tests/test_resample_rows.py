"""The rate conversion with a window per row (include/zvx.h: zvx_resample_rows), no GPU needed: the surface -- header, built library,
bindings -- and the refusal that needs no context."""
import ctypes as C
import inspect
import os
import re

from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_code():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    return h, re.sub(r"/\*.*?\*/", "", h, flags=re.S)


def test_header_declares_the_call():
    h, code = header_code()
    m = re.search(r"zvx_status\s+zvx_resample_rows\s*\(([^;]*)\)\s*;", code)
    assert m, "zvx_resample_rows not declared"
    assert " ".join(m.group(1).split()) == ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out, "
                                            "int64_t out_stride, int32_t* out_len, int flags, const zvx_row_window* win")
    assert code.index("} zvx_row_window;") < m.start()       # the struct is declared in front of its user
    # zvx_resample_ex keeps its signature
    assert re.search(r"zvx_resample_ex\s*\([^;]*int flags, int64_t in_origin, int64_t out_begin, int64_t out_count\)\s*;", code)
    # what the header has to say about the call, and no longer says about the streams
    for phrase in ("NO zero fill", "has no meaning here", "ZVX_E_BUFFER: out_stride smaller than the longest cnt_b", '"voc.resample"'):
        assert phrase in h, phrase
    assert "stays one call per session" not in h and "it has no rows form" not in h


def test_library_exports_the_entry_point():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_resample_rows")
    vp = C.c_void_p
    lib.zvx_resample_rows.argtypes = [vp] * 3 + [C.c_int] * 4 + [vp, C.c_int64, vp, C.c_int, vp]
    assert lib.zvx_resample_rows(None, None, None, 0, 0, 0, 0, None, 0, None, 0, None) == _lib.ZVX_E_INVALID      # a NULL context


def test_bindings_and_exports():
    assert "zvx_resample_rows" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.zvx_resample_rows.argtypes == lib.zvx_resample.argtypes + [C.POINTER(_lib.RowWindow)]
    p = inspect.signature(_lib.Context.resample_rows).parameters
    assert list(p) == ["self", "rows", "rate_in", "rate_out", "windows", "pcm16", "lengths"]
    assert (p["pcm16"].default, p["lengths"].default) == (False, None)
