"""Loudness normalisation, the parts that need no GPU: the float64 reference of tests/loudness_ref.py against the published BS.1770-4
figures, and the surface of the feature (header, exports, bindings, keywords)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loudness_ref as R
from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


def test_reference_coefficients_are_the_bs1770_table_at_48k():
    (b1, a1), (b2, a2) = R.coefficients(48000)
    got = [b1[0], b1[1], b1[2], a1[1], a1[2], a2[1], a2[2]]
    want = [1.53512486, -2.69169619, 1.19839281, -1.69065929, 0.73248077, -1.99004745, 0.99007225]
    assert a1[0] == 1.0 and a2[0] == 1.0 and list(b2) == [1.0, -2.0, 1.0]
    assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-8, got


def test_reference_reads_a_full_scale_997_hz_sine_at_minus_3_01():
    fs = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * fs) / fs).astype(np.float32)
    m = R.measure([x], fs)
    assert abs(m["lufs"][0] - (-3.01)) <= 0.01, m["lufs"][0]
    assert m["removed"][0] == (0, 0) and abs(m["lufs_common"] - m["lufs"][0]) < 1e-12


def test_reference_gates_and_gain_rules():
    fs = 16000
    h = R.unit_len(fs)
    assert h == 1600 and R.unit_len(22050) == 2205 and R.unit_len(44100) == 4410 and R.unit_len(11025) == 1103
    rng = np.random.default_rng(3)
    loud, quiet = rng.standard_normal(8 * h) * 0.1, rng.standard_normal(8 * h) * 1e-3
    m = R.measure([np.concatenate([loud, quiet]).astype(np.float32), np.zeros(9 * h, np.float32), loud[:4 * h - 1].astype(np.float32)], fs)
    assert m["removed"][0][1] > 0 and np.isfinite(m["lufs"][0])               # the quiet half falls to the relative gate
    assert m["lufs"][1] == -np.inf and m["removed"][1] == (6, 0)              # silence: every block under the absolute gate
    assert m["lufs"][2] == -np.inf and m["margin"][2] == np.inf               # shorter than one block: nothing measured
    assert R.gain_ref(-np.inf, 0.5, -23, 0.891, 20) == (1.0, None) and R.gain_ref(-20.0, 0.0, -23, 0.891, 20) == (1.0, None)
    assert R.gain_ref(-43.0, 0.001, -23.0, 0.891, 12.0) == (10.0 ** (12.0 / 20.0), "max_gain")
    g, lim = R.gain_ref(-20.0, 0.5, -10.0, 0.891, 20.0)
    assert lim == "ceiling" and g == float(np.float32(0.891)) / 0.5
    g, lim = R.gain_ref(-20.0, 0.5, -23.0, 0.0, 20.0)
    assert lim is None and abs(g - 10.0 ** (-3.0 / 20.0)) < 1e-15


def test_header_declares_the_loudness_interface():
    h = header()
    assert re.search(r"zvx_status\s+zvx_loudness\s*\(", h) and re.search(r"zvx_status\s+zvx_normalize\s*\(", h)
    assert re.search(r"typedef\s+struct\s+zvx_loudness_params\s*\{[^}]*target_lufs[^}]*peak_ceiling[^}]*max_gain_db[^}]*mode[^}]*\}\s*zvx_loudness_params\s*;", h)
    assert re.search(r"ZVX_LOUD_PER_ROW\s*=\s*0\s*,\s*ZVX_LOUD_COMMON\s*=\s*1", h)
    assert '"post.loudness"' in h
    assert (_lib.ZVX_LOUD_PER_ROW, _lib.ZVX_LOUD_COMMON) == (0, 1)
    assert [f[0] for f in _lib.LoudnessParams._fields_] == ["target_lufs", "peak_ceiling", "max_gain_db", "mode"] and C.sizeof(_lib.LoudnessParams) == 16


def test_library_exports_both_entry_points():
    assert "zvx_loudness" in _lib.EXPORTS and "zvx_normalize" in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("zvx_loudness", "zvx_normalize"):
        assert hasattr(lib, name), name
    # NULL context: refused before anything else is looked at
    assert lib.zvx_loudness(None, None, None, 0, 0, 0, None, None, 0) == _lib.ZVX_E_INVALID


def test_no_new_stage_slot():
    assert re.search(r"ZVX_T_COUNT\s*=\s*8\b", header()) and _lib.ZVX_T_COUNT == 8
    assert _lib.STAGES == ("encoder", "variance", "lenreg", "decoder", "vocoder", "spkemb")


def test_bindings_and_keywords_are_there():
    import inspect
    from zerovox_amd.synthesize import ZeroVoxTTS
    for name in ("loudness", "normalize", "normalize_device"):
        assert callable(getattr(_lib.Context, name))
    p = inspect.signature(_lib.Context.normalize).parameters
    assert p["peak_ceiling"].default == 0.891 and p["max_gain_db"].default == 20.0 and p["common"].default is False and p["rate"].default is None
    for fn in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long):
        p = inspect.signature(fn).parameters
        assert p["loudness"].default is None and p["peak_db"].default == -1.0, fn
    assert inspect.signature(ZeroVoxTTS.tts_long).parameters["loudness_mode"].default == "paragraph"


def test_a_stream_cannot_be_normalised():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                  # the refusal comes before anything of the model is touched
    with pytest.raises(ValueError):
        synth.tts_stream("hello there", None, loudness=-23)
    from zerovox_amd.longform import synthesize_long
    with pytest.raises(ValueError):
        synthesize_long(None, "hello there", None, loudness=-23, loudness_mode="word")
