"""The windowed limiter, the parts that need no GPU: zerovox_amd.limiter's planner against the float64 reference of tests/limit_ref.py
(a stream limited window by window concatenates to the whole-row result: equal f32 bits, equal f64 gains), the support condition of
include/zvx.h restated on every planned window, and the surface of the feature (header, exports, constants,
keywords, refusals)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import limit_ref as L
from stream_util import ROOT, cut, header, supported
from zerovox_amd import _lib, limiter as LM

CEILING = 0.891
CONFIGS = [(1, 1), (5, 1), (22, 4), (110, 4), (40, 8), (110, 2)]          # (W, os)
_rows, _ref = {}, {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def row(n):
    """uniform noise, quieter over one stretch, loud at both ends, scaled to a peak of 1.6: the limiter acts on most of it"""
    if n not in _rows:
        rng = np.random.default_rng(n)
        x = rng.uniform(-1.0, 1.0, n)
        x[n // 3:n // 2] *= 0.5
        x[0], x[-1] = 0.9, -0.8
        _rows[n] = L.scaled_rows([x.astype(np.float32)])[0]
        _rows[n].setflags(write=False)
    return _rows[n]


def whole(n, W, os_):
    key = (n, W, os_)
    if key not in _ref:
        _ref[key] = L.limit(row(n), CEILING, W, os_)
    return _ref[key]


def run_stream(x, W, os_, sizes):
    """-> (out f32, g f64, windows): x streamed in chunks through stream_limit, every window limited by the float64 reference"""
    gains, windows = [], []

    def window_fn(samples, in_origin, out_begin, out_count, last):
        windows.append((in_origin, len(samples), out_begin, out_count, last))
        r = L.limit(samples, CEILING, W, os_)
        a = out_begin - in_origin
        gains.append(r["g"][a:a + out_count])
        return r["out"][a:a + out_count]

    pieces = list(LM.stream_limit(cut(x, sizes), LM.LimitPlanner(W, os_), window_fn))
    return (np.concatenate(pieces) if pieces else np.zeros(0, np.float32)), (np.concatenate(gains) if gains else np.zeros(0)), windows


def chunkings(n, R, seed):
    rng = np.random.default_rng(seed)
    return {"fixed 256": [256], "fixed 700": [700], "one chunk": [n], "shorter than R": [max(1, R // 3)],
            "random": [int(v) for v in rng.integers(1, 900, 64)]}


@pytest.mark.parametrize("W,os_", CONFIGS)
def test_stream_concatenates_to_the_whole_row(W, os_):
    R = LM.reach(W, os_)
    assert R == 2 * W + (11 if os_ > 1 else 0)
    acted = 0
    for n in (300, 2500, 6000):
        ref = whole(n, W, os_)
        acted += int(np.count_nonzero(ref["g"] < 1.0))
        for name, sizes in chunkings(n, R, 7 * W + os_).items():
            if name == "shorter than R" and n > 2500:
                continue                                     # (many small windows: the two shorter rows carry this case)
            out, g, windows = run_stream(row(n), W, os_, sizes)
            assert len(out) == n and np.array_equal(bits(out), bits(ref["out"])), (n, name)
            assert np.array_equal(g, ref["g"]), (n, name)
            for (o, k, b, c, last) in windows:
                assert supported(R, o, k, b, c, last), (n, name, o, k, b, c, last)
    assert acted > 4400, acted                                # the limiter acts on most samples of these rows


@pytest.mark.parametrize("W,os_", [(1, 1), (5, 1), (22, 4)])
def test_one_sample_chunks(W, os_):
    n = 300
    ref = whole(n, W, os_)
    out, g, windows = run_stream(row(n), W, os_, [1])
    assert np.array_equal(bits(out), bits(ref["out"])) and np.array_equal(g, ref["g"])
    R = LM.reach(W, os_)
    assert all(supported(R, *w) for w in windows)
    assert max(k for (_, k, _, _, _) in windows) <= 1 + 2 * R


def test_a_window_one_sample_short_is_not_supported_and_may_differ():
    """the restated condition is tight: R is the reach, R - 1 is not (the reference on a window cut one sample early differs)"""
    W, os_, n = 22, 4, 2500
    R = LM.reach(W, os_)
    ref, x = whole(n, W, os_), row(n)
    assert supported(R, 501, 1200, 501 + R, 100, False) and not supported(R, 501, 1200, 500 + R, 100, False)
    assert supported(R, 501, 1200, 900, 1200 - 399 - R, False) and not supported(R, 501, 1200, 900, 1201 - 399 - R, False)
    assert supported(R, 0, 700, 0, 700 - R, False) and supported(R, 900, n - 900, 900 + R, n - 900 - R, True)
    differs = 0
    for begin in range(300, 1500, 7):                        # emit ONE sample whose support is short by one on the left
        o = begin - (R - 1)
        r = L.limit(x[o:begin + R + 1], CEILING, W, os_)
        differs += int(r["g"][begin - o] != ref["g"][begin])
        ok = L.limit(x[o - 1:begin + R + 1], CEILING, W, os_)
        assert ok["g"][begin - o + 1] == ref["g"][begin] and bits(ok["out"])[begin - o + 1] == bits(ref["out"])[begin]
    print(f"{differs} of {len(range(300, 1500, 7))} samples differ when the window is one sample short")


def test_window_rule():
    for rate, ms in ((22050, 5.0), (22050, 1.0), (8000, 0.01), (48000, 4096 / 48.0), (44100, 2.5), (22050, 0.1)):
        assert LM.window_samples(rate, ms) == L.window(rate, ms), (rate, ms)
    assert LM.window_samples(22050, 5.0) == 110 and LM.reach(110, 4) == 231 and LM.reach(110, 1) == 220 and LM.reach(1, 2) == 13


def test_header_and_constants():
    h = header()
    assert re.search(r"zvx_status\s+zvx_limit_ex\s*\(", h)
    decl = re.search(r"zvx_status\s+zvx_limit_ex\s*\(([^;]*)\)\s*;", h).group(1)
    assert re.search(r"int64_t\s+in_origin\s*,\s*int64_t\s+out_begin\s*,\s*int64_t\s+out_count\s*,\s*int\s+last\s*$", decl.strip())
    assert "R = 2 W + H" in h and "H = 11" in h and "in ascending k" in h and "a double sum in any order" not in h
    with open(os.path.join(ROOT, "zerovox_amd", "csrc", "zvx_kernels.h")) as f:
        k = f.read()
    assert int(re.search(r"constexpr int LIMIT_ENV_REACH = (\d+);", k).group(1)) == _lib.LIMIT_ENV_REACH == LM.ENV_REACH == 11


def test_library_exports_the_entry_point():
    assert "zvx_limit_ex" in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_limit_ex")
    lib.zvx_limit_ex.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
                                 + [C.c_int64] * 3 + [C.c_int])
    assert lib.zvx_limit_ex(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, 0, 0, -1, 1) == _lib.ZVX_E_INVALID


def test_bindings_and_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    p = inspect.signature(_lib.Context.limit_window).parameters
    assert p["ceiling"].default is inspect.Parameter.empty and p["window_ms"].default == 5.0 and p["oversample"].default == 4
    assert p["in_origin"].default == 0 and p["out_begin"].default == 0 and p["out_count"].default == -1 and p["last"].default is True
    assert p["pcm16"].default is False and p["rate"].default is None and p["lengths"].default is None
    p = inspect.signature(ZeroVoxTTS.tts_stream).parameters
    assert p["peak_db"].default is None and p["limiter_ms"].default == 5.0 and p["limiter"].default is False and p["loudness"].default is None
    assert inspect.signature(ZeroVox.vocode_stream).parameters["limiter"].default is None
    assert "not built" not in ZeroVoxTTS.tts_stream.__doc__


def test_refusals_come_before_the_model_is_touched():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)
    with pytest.raises(ValueError, match="peak_db"):
        synth.tts_stream("hello there", None, limiter=True)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            synth.tts_stream("hello there", None, peak_db=bad)
    with pytest.raises(ValueError):
        synth.tts_stream("hello there", None, loudness=-16.0, peak_db=-1.0)
