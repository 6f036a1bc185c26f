"""The windowed denoiser, the parts that need no GPU: the float64 windowed restatement (tests/denoise_window_ref.py) against
denoise_ref.denoise of the whole row, bit for bit, over every geometry and cut; a stream driven by zerovox_amd.denoiser through that
reference (the support condition of include/zvx.h restated on every planned window); and the surface of the feature (header, exports, keywords, refusals)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import denoise_ref as D
import denoise_window_ref as DW
from stream_util import cut, header, supported, window_of
from zerovox_amd import _lib, denoiser as DN

GEOMETRIES = [(1024, 256, 1024), (512, 256, 512), (256, 256, 128), (2048, 256, 2048), (64, 16, 64)]      # (n_fft, hop, win_length)
STRENGTH, FLOOR = 0.5, 0.1
_rows, _whole = {}, {}


def lengths(n_fft, hop):
    """three row lengths: one sample above the minimum, one off every multiple, one of several frames"""
    return (D.min_samples(n_fft, hop) + 1, 2 * n_fft + 77, 3 * n_fft + hop + 13)


def row(n, n_fft):
    key = (n, n_fft)
    if key not in _rows:
        rng = np.random.default_rng(n + n_fft)
        i = np.arange(n)
        x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 37.3 * i / n_fft + 0.4) + 0.2 * np.sin(2 * np.pi * 11.0 * i / n_fft + 1.1)
        _rows[key] = np.clip(x, -1.0, 1.0).astype(np.float32)
        _rows[key].setflags(write=False)
    return _rows[key]


def bias_for(n_fft, hop, wl):
    """a bias of the size of the rows' median magnitude, so that many bins clamp and many do not"""
    key = ("bias", n_fft, hop, wl)
    if key not in _rows:
        rng = np.random.default_rng(n_fft)
        med = np.median(np.abs(D.analysis(row(lengths(n_fft, hop)[2], n_fft), n_fft, hop, wl)))
        _rows[key] = (med * rng.uniform(0.5, 1.5, n_fft // 2 + 1)).astype(np.float32)
    return _rows[key]


def whole(n, n_fft, hop, wl):
    key = (n, n_fft, hop, wl)
    if key not in _whole:
        _whole[key] = D.denoise(row(n, n_fft), bias_for(n_fft, hop, wl), STRENGTH, FLOOR, n_fft, hop, wl)
        _whole[key].setflags(write=False)
    return _whole[key]


def same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n_fft,hop,wl", GEOMETRIES)
def test_windows_with_exactly_R_of_support_reproduce_the_whole_row(n_fft, hop, wl):
    R = DW.reach(n_fft)
    bias = bias_for(n_fft, hop, wl)
    pieces = moved = 0
    for n in lengths(n_fft, hop):
        x, want = row(n, n_fft), whole(n, n_fft, hop, wl)
        moved += int(np.count_nonzero(want != x))
        edges = DW.cuts(n, n_fft, hop)
        for begin, end in zip(edges[:-1], edges[1:]):
            o, w_end, last = window_of(n, begin, end, R)
            reads = []
            got = DW.denoise_window(x[o:w_end], bias, STRENGTH, FLOOR, o, begin, end - begin, last, n_fft, hop, wl, reads=reads)
            assert same_f64(got, want[begin:end]), (n, begin, end, o, w_end, last, int(np.count_nonzero(got != want[begin:end])))
            assert 0 <= reads[0][0] and reads[0][1] < w_end - o                       # (the restatement asserts it on every frame as well)
            pieces += 1
        # out_count -1: to the end of the signal, from the last cut
        o, w_end, last = window_of(n, edges[-2], n, R)
        assert last == 1 and same_f64(DW.denoise_window(x[o:], bias, STRENGTH, FLOOR, o, edges[-2], -1, 1, n_fft, hop, wl), want[edges[-2]:])
    assert pieces >= 15 and moved > 0, (pieces, moved)                 # (hop == n_fft: some of the cuts coincide)


def test_one_sample_short_of_support_is_refused_by_the_restatement():
    n_fft, hop, wl = 1024, 256, 1024
    R, n = DW.reach(n_fft), 3 * 1024 + 77
    x, bias = row(n, n_fft), bias_for(n_fft, hop, wl)
    assert supported(R, 100, 2 * R + 10, 100 + R, 10, 0) and not supported(R, 100, 2 * R + 10, 99 + R, 10, 0)
    assert not supported(R, 100, 2 * R + 10, 100 + R, 11, 0) and supported(R, 100, 2 * R + 10, 100 + R, 11, 1)
    assert supported(R, 0, R + 10, 0, 10, 0) and not supported(R, 0, R + 10, 0, 11, 0)
    with pytest.raises(AssertionError):
        DW.denoise_window(x[100:100 + 2 * R + 10], bias, STRENGTH, FLOOR, 100, 99 + R, 10, 0)
    # the condition is tight on the grid: an output at a frame's last sample reads R samples back, one at its first sample R ahead
    pad = (n_fft - hop) // 2
    i = 4 * hop - pad + n_fft - 1                            # the last sample of frame 4
    reads = []
    DW.denoise_window(x[i - R:i + R + 1], bias, STRENGTH, FLOOR, i - R, i, 1, 0, reads=reads)
    assert reads[0][0] == 0
    i = 6 * hop - pad                                        # the first sample of frame 6
    reads = []
    DW.denoise_window(x[i - R:i + R + 1], bias, STRENGTH, FLOOR, i - R, i, 1, 0, reads=reads)
    assert reads[0][1] == 2 * R


@pytest.mark.parametrize("n_fft,hop,wl", GEOMETRIES)
def test_stream_concatenates_to_the_whole_row(n_fft, hop, wl):
    R = DN.reach(n_fft)
    assert R == n_fft - 1 == DW.reach(n_fft)
    bias = bias_for(n_fft, hop, wl)
    rng = np.random.default_rng(n_fft + hop)
    for n in lengths(n_fft, hop):
        x, want = row(n, n_fft), whole(n, n_fft, hop, wl)
        chunkings = {"hop": [hop], "one chunk": [n], "shorter than R": [max(1, R // 3)], "random": [int(v) for v in rng.integers(1, 2 * n_fft, 64)],
                     "random small": [int(v) for v in rng.integers(1, hop + 2, 64)]}
        for name, sizes in chunkings.items():
            windows = []

            def window_fn(samples, in_origin, out_begin, out_count, last):
                windows.append((in_origin, len(samples), out_begin, out_count, last))
                return DW.denoise_window(samples, bias, STRENGTH, FLOOR, in_origin, out_begin, out_count, last, n_fft, hop, wl)

            pieces = list(DN.stream_denoise(cut(x, sizes), DN.DenoisePlanner(n_fft), window_fn))
            got = np.concatenate(pieces)
            assert same_f64(got, want), (n, name, len(got))
            assert all(supported(R, *w) for w in windows), (n, name)
            assert max(k for (_, k, _, _, _) in windows) <= max(sizes) + 2 * R


def test_limiter_module_is_untouched_by_the_shared_planner():
    from zerovox_amd import limiter as LM, stream
    assert issubclass(DN.DenoisePlanner, stream.ReachPlanner) and issubclass(LM.LimitPlanner, stream.ReachPlanner)
    assert not issubclass(DN.DenoisePlanner, LM.LimitPlanner)
    assert LM.LimitPlanner(110, 4).R == 231 and LM.reach(110, 4) == 231
    assert DN.reach(1024) == 1023


def test_header_declares_the_entry_point():
    h = header()
    decl = re.search(r"zvx_status\s+zvx_denoise_ex\s*\(([^;]*)\)\s*;", h).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["zvx_ctx* ctx", "const float* in", "const int32_t* nsamples", "int B", "int Nmax", "const float* bias",
                    "const zvx_denoise_params* params", "void* out", "int64_t out_stride", "int flags",
                    "int64_t in_origin", "int64_t out_begin", "int64_t out_count", "int last"], args
    assert "R = n_fft - 1" in h and "zvx_denoise is zvx_denoise_ex(..., 0, 0, -1, 1)" in h and "ascending f" in h
    assert "same double table" in h and "its own n_fft samples only" in h


def test_library_exports_the_entry_point():
    assert "zvx_denoise_ex" in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_denoise_ex")
    lib.zvx_denoise_ex.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_int64] * 3 + [C.c_int]
    assert lib.zvx_denoise_ex(None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, -1, 1) == _lib.ZVX_E_INVALID


def test_bindings_and_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    p = inspect.signature(_lib.Context.denoise_window).parameters
    assert list(p)[1:] == ["rows", "bias", "strength", "floor", "in_origin", "out_begin", "out_count", "last", "pcm16", "lengths"]
    assert p["strength"].default is inspect.Parameter.empty and p["floor"].default == 0.0
    assert p["in_origin"].default == 0 and p["out_begin"].default == 0 and p["out_count"].default == -1 and p["last"].default is True
    assert p["pcm16"].default is False and p["lengths"].default is None
    p = inspect.signature(ZeroVoxTTS.tts_stream).parameters
    assert p["denoise_strength"].default is None and p["denoise"].default is None
    assert inspect.signature(ZeroVox.vocode_stream).parameters["denoise"].default is None
    doc = ZeroVoxTTS.tts_stream.__doc__
    assert "not denoised either" not in doc and "no windowed form" not in doc and "denoise_strength" in doc


def test_refusals_come_before_the_model_is_touched():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                   # no model: whatever touches it raises AttributeError, not ValueError
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            synth.tts_stream("hello there", None, denoise_strength=bad)
    with pytest.raises(ValueError, match="denoise") as e:
        synth.tts_stream("hello there", None, denoise=0.01)
    assert "denoise_strength" in str(e.value)                # the old keyword's message points to the new one
    with pytest.raises(ValueError):
        synth.tts_stream("hello there", None, denoise_strength=0.01, loudness=-16)
