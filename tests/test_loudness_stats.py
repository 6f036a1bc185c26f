"""The programme loudness report without a GPU (include/zvx.h: zvx_loudness_stats): the surface (header, binding, exports, the Python entry
points and their defaults), the float64 restatement tests/loudness_stats_ref.py against the minimum-requirement signals of EBU Tech 3342
(the loudness range each asks for, within Tech 3342's own +- 1 LU), the nearest-rank indices, the short and silent rows, and
report.LoudnessReport.meets."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import loudness_ref as R
import loudness_stats_ref as S
from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_code():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    return h, re.sub(r"/\*.*?\*/", "", h, flags=re.S)


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_the_call_and_the_enum():
    h, code = header_code()
    m = re.search(r"zvx_status\s+zvx_loudness_stats\s*\(([^;]*)\)\s*;", code)
    assert m, "zvx_loudness_stats not declared"
    assert " ".join(m.group(1).split()) == ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, double* stats, "
                                            "double* momentary, double* short_term, int64_t curve_stride, int flags")
    m = re.search(r"enum\s*\{\s*(ZVX_LS_INTEGRATED[^}]*)\}", code)
    assert m, "the ZVX_LS_ enum is not declared"
    assert " ".join(m.group(1).split()) == ("ZVX_LS_INTEGRATED = 0, ZVX_LS_MOMENTARY_MAX, ZVX_LS_SHORT_MAX, ZVX_LS_LRA, ZVX_LS_LRA_LOW, "
                                            "ZVX_LS_LRA_HIGH, ZVX_LS_SHORT_GATED, ZVX_LS_PEAK, ZVX_LS_COUNT = 8")
    # the new block stands behind zvx_normalize and points back; zvx_loudness's own block stays as it was
    assert h.index("zvx_status zvx_normalize(") < h.index("Programme loudness report") < h.index("zvx_status zvx_loudness_stats(")
    assert h.index("zvx_status zvx_loudness_stats(") < h.index("zvx_status zvx_true_peak(")
    assert "Not here: momentary /" in h
    for text in ('"not here" for that call', "((n_g - 1) * 10 + 50) / 100", "((n_g - 1) * 95 + 50) / 100", "s[j] > 0.01 Gamma", "65536 units",
                 "curve_stride >= max(1, Nmax / h - 3)", '"post.loudness"', "relative 2.3e-4"):
        assert text in h, text


def test_binding_exports_and_python_entry_points():
    assert "zvx_loudness_stats" in _lib.EXPORTS
    assert (_lib.ZVX_LS_INTEGRATED, _lib.ZVX_LS_MOMENTARY_MAX, _lib.ZVX_LS_SHORT_MAX, _lib.ZVX_LS_LRA, _lib.ZVX_LS_LRA_LOW, _lib.ZVX_LS_LRA_HIGH,
            _lib.ZVX_LS_SHORT_GATED, _lib.ZVX_LS_PEAK, _lib.ZVX_LS_COUNT) == tuple(range(9))
    assert _lib.LOUDNESS_STATS_KEYS == S.KEYS and len(S.KEYS) == _lib.ZVX_LS_COUNT
    lib = _lib.load()
    vp = C.c_void_p
    assert lib.zvx_loudness_stats.argtypes == [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int]
    p = inspect.signature(_lib.Context.loudness_stats).parameters
    assert list(p) == ["self", "rows", "rate", "lengths", "curves"]
    assert (p["rate"].default, p["lengths"].default, p["curves"].default) == (None, None, False)
    p = inspect.signature(_lib.Context.loudness_stats_device).parameters
    assert list(p)[:5] == ["self", "ptr", "lengths", "Nmax", "rate"] and p["rate"].default is None
    assert all(q.default is not inspect.Parameter.empty for q in list(p.values())[4:])


def test_library_exports_the_entry_point():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_loudness_stats")
    vp = C.c_void_p
    lib.zvx_loudness_stats.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int]
    assert lib.zvx_loudness_stats(None, None, None, 0, 0, 0, None, None, None, 0, 0) == _lib.ZVX_E_INVALID          # a NULL context


def test_report_keywords_default_to_off():
    from zerovox_amd.longform import synthesize_long
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    for fn in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long, synthesize_long, ZeroVox.inference_ex):
        p = inspect.signature(fn).parameters
        assert p["report"].default is False, fn
    assert "report" not in inspect.signature(ZeroVoxTTS.tts_stream).parameters
    p = inspect.signature(ZeroVoxTTS.loudness_report).parameters
    assert list(p) == ["self", "wav", "sampling_rate"] and p["sampling_rate"].default is None
    assert isinstance(ZeroVoxTTS.last_report, property)


def test_demo_and_the_long_form_bench_take_report():
    for path in (os.path.join(ROOT, "zerovox_amd", "demo.py"), os.path.join(ROOT, "tools", "longform_bench.py")):
        with open(path) as f:
            assert '"--report"' in f.read(), path


def test_report_module_imports_without_the_library():
    code = ("import sys, zerovox_amd.report as r; assert 'zerovox_amd._lib' not in sys.modules and 'numpy' not in sys.modules; "
            "print(sorted(f for f in r.LoudnessReport.__dataclass_fields__))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == str(sorted(["integrated", "lra", "lra_low", "lra_high", "max_momentary", "max_short_term", "sample_peak_db",
                                             "true_peak_db", "short_gated"])).split()


# ------------------------------------------------------------------------------------------------ the reference and EBU Tech 3342
# what a float64 restatement of the contract gives on the four signals at every rate: LRA to the third decimal, n_g, and the gate margin
TECH3342_EXPECT = {1: (10.0, 371, 12.6), 2: (5.0, 371, 16.8), 3: (20.0, 371, 2.97), 4: (15.0, 627, 0.356)}


@pytest.mark.parametrize("fs", (8000, 22050, 48000))
@pytest.mark.parametrize("case", sorted(S.TECH3342))
def test_reference_meets_tech_3342(case, fs):
    segments, want = S.TECH3342[case]
    r = S.measure_row(S.sine_segments(fs, segments), fs)
    W = int(sum(sec for sec, _ in segments)) * 10 - 29
    print(f"Tech 3342 case {case} at {fs} Hz: LRA {r['lra']:.4f} LU ({r['lra_low']:.3f} .. {r['lra_high']:.3f} LUFS), n_g {int(r['short_gated'])} of "
          f"{len(r['short_term'])}, margin {r['margin']:.3f} LU")
    assert abs(r["lra"] - want) <= 1.0, (case, fs, r["lra"])                           # Tech 3342's own tolerance
    lra, n_g, margin = TECH3342_EXPECT[case]
    assert len(r["short_term"]) == W and len(r["momentary"]) == W + 26
    assert abs(r["lra"] - lra) < 5e-3 and int(r["short_gated"]) == n_g, (case, fs, r["lra"], r["short_gated"])
    assert abs(r["margin"] - margin) <= 0.05 * margin + 0.01, (case, fs, r["margin"])
    assert abs(r["lra"] - (r["lra_high"] - r["lra_low"])) < 1e-9
    # a 1 kHz sine at -20 dBFS reads -23.0 LUFS (K-weighting is 0.691 dB up at 1 kHz at 48 kHz; the shelf redesigned for another rate is a
    # few hundredths of a dB off that there): the loudest window of every case
    top = max(db for _, db in segments)
    assert abs(r["max_short_term"] - (top - 3.01)) < 0.1 and abs(r["max_momentary"] - (top - 3.01)) < 0.1


@pytest.mark.parametrize("fs", (4000, 8000))
def test_reference_on_the_shortened_case_1(fs):
    r = S.measure_row(S.sine_segments(fs, [(8, -20.0), (8, -30.0)]), fs)
    assert abs(r["lra"] - 10.0) < 5e-3 and r["margin"] > 1.0, (fs, r["lra"], r["margin"])
    assert len(r["short_term"]) == 131 and int(r["short_gated"]) == 131


def test_nearest_rank_indices():
    assert [S.rank_indices(n) for n in (1, 2, 3, 10, 11, 12, 101, 371, 627)] == \
        [(0, 0), (0, 1), (0, 2), (1, 9), (1, 10), (1, 10), (10, 95), (37, 352), (63, 595)]
    for n in range(1, 400):                                  # round((n - 1) p / 100) with halves up, in exact arithmetic
        lo, hi = S.rank_indices(n)
        assert lo == math.floor(Fraction((n - 1) * 10, 100) + Fraction(1, 2)) and hi == math.floor(Fraction((n - 1) * 95, 100) + Fraction(1, 2)), n
        assert 0 <= lo <= hi < n
    # hand-made lists: the powers are picked at those ranks of the ascending sort
    for powers in ([3e-3], [5e-3, 2e-3], [1e-3 * (1 + k) for k in (4, 0, 3, 1, 2, 9, 7, 8, 6, 5, 10)]):
        s = np.array(powers)
        k, _ = S.lra_gate(s)
        assert np.array_equal(k, np.sort(s))                 # (all within 20 LU of their mean and far above the absolute gate)
        lo, hi = S.rank_indices(len(k))
        assert (lo, hi) == {1: (0, 0), 2: (0, 1), 11: (1, 10)}[len(s)]
        assert (k[lo], k[hi]) == {1: (3e-3, 3e-3), 2: (2e-3, 5e-3), 11: (1e-3 * 2, 1e-3 * 11)}[len(s)]


def _noise(n, amp=0.05, seed=0):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def test_reference_edge_cases():
    fs = 4000
    h = R.unit_len(fs)
    r = S.measure_row(_noise(4 * h - 1), fs)                 # U < 4: no block, no window; the peak still counts every sample
    assert r["integrated"] == r["max_momentary"] == r["max_short_term"] == r["lra_low"] == r["lra_high"] == -np.inf
    assert r["lra"] == 0.0 and r["short_gated"] == 0.0 and r["peak"] > 0 and len(r["momentary"]) == len(r["short_term"]) == 0
    r = S.measure_row(_noise(29 * h + h - 1), fs)            # 4 <= U < 30: blocks, no window
    assert np.isfinite(r["integrated"]) and np.isfinite(r["max_momentary"]) and len(r["momentary"]) == 26
    assert r["max_short_term"] == r["lra_low"] == r["lra_high"] == -np.inf and r["lra"] == 0.0 and r["short_gated"] == 0.0
    assert len(r["short_term"]) == 0 and r["margin"] == np.inf
    r = S.measure_row(_noise(30 * h), fs)                    # exactly one window: both ranks are it
    assert len(r["short_term"]) == 1 and r["short_gated"] == 1.0 and r["lra"] == 0.0 and r["lra_low"] == r["lra_high"] == r["max_short_term"]
    r = S.measure_row(np.zeros(40 * h, np.float32), fs)      # all silent: every power is 0
    assert r["integrated"] == r["max_momentary"] == r["max_short_term"] == -np.inf and r["peak"] == 0.0
    assert np.all(r["momentary"] == -np.inf) and np.all(r["short_term"] == -np.inf) and len(r["short_term"]) == 11
    assert r["lra"] == 0.0 and r["short_gated"] == 0.0 and r["lra_low"] == -np.inf
    r = S.measure_row(_noise(40 * h, amp=10.0 ** (-80.0 / 20.0)), fs)      # under the absolute gate: measured, never gated in
    assert r["integrated"] == -np.inf and np.isfinite(r["max_momentary"]) and r["max_momentary"] < -70.0 and r["max_short_term"] < -70.0
    assert r["lra"] == 0.0 and r["short_gated"] == 0.0 and r["lra_low"] == r["lra_high"] == -np.inf and r["margin"] > 1.0
    r = S.measure_row(np.zeros(0, np.float32), fs)           # n == 0
    assert r["integrated"] == -np.inf and r["peak"] == 0.0 and r["lra"] == 0.0 and r["short_gated"] == 0.0
    m = S.measure([_noise(35 * h), np.zeros(0, np.float32)], fs)
    assert all(m[k].shape == (2,) for k in S.KEYS) and len(m["momentary"]) == 2
    # the integrated figure and the blocks are loudness_ref's
    x = _noise(50 * h, seed=3)
    assert S.measure_row(x, fs)["integrated"] == R.measure([x], fs)["lufs"][0]
    assert np.allclose(S.measure_row(x, fs)["momentary"], S.lufs(R.blocks(x, fs)), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ LoudnessReport
def test_loudness_report_meets():
    from zerovox_amd.report import LoudnessReport
    stats = {k: np.array([v]) for k, v in dict(integrated=-23.2, max_momentary=-18.0, max_short_term=-20.0, lra=7.5, lra_low=-28.0,
                                               lra_high=-20.5, short_gated=120.0, peak=0.5).items()}
    rep = LoudnessReport.from_stats(stats, np.float32(0.708))
    assert rep.integrated == -23.2 and rep.lra == 7.5 and rep.short_gated == 120 and isinstance(rep.short_gated, int)
    assert abs(rep.sample_peak_db - 20.0 * math.log10(0.5)) < 1e-12 and abs(rep.true_peak_db - 20.0 * math.log10(float(np.float32(0.708)))) < 1e-12
    assert rep.meets(-23.0) and rep.meets(-23) and not rep.meets(-23.0, tolerance=0.1) and not rep.meets(-16.0)
    assert not rep.meets(-23.0, max_true_peak_db=-3.5) and rep.meets(-23.0, max_true_peak_db=-2.9) and rep.meets(-23.0, max_true_peak_db=None)
    assert rep.meets(-23.0, max_lra=8.0) and not rep.meets(-23.0, max_lra=7.0)
    p = inspect.signature(LoudnessReport.meets).parameters
    assert list(p) == ["self", "target", "tolerance", "max_true_peak_db", "max_lra"]
    assert (p["tolerance"].default, p["max_true_peak_db"].default, p["max_lra"].default) == (0.5, -1.0, None)
    over = LoudnessReport.from_stats(stats, 0.95)            # -0.45 dBTP: over the default -1 dBTP
    assert not over.meets(-23.0) and over.meets(-23.0, max_true_peak_db=0.0)
    silent = LoudnessReport.from_stats({k: np.array([v]) for k, v in dict(integrated=-np.inf, max_momentary=-np.inf, max_short_term=-np.inf, lra=0.0,
                                                                         lra_low=-np.inf, lra_high=-np.inf, short_gated=0.0, peak=0.0).items()}, 0.0)
    assert silent.sample_peak_db == -math.inf and silent.true_peak_db == -math.inf and not silent.meets(-23.0, tolerance=1e9)
    assert set(rep.as_dict()) == set(LoudnessReport.__dataclass_fields__) and "LUFS" in str(rep)
