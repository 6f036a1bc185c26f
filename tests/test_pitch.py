"""The pitch report without a GPU (include/zvx.h: zvx_pitch): the surface (header, binding, exports, the Python entry points and their
defaults), the float64 restatement tests/pitch_ref.py against the truth of synthetic rows (the bounds are those of the NumPy prototype of
the definition: measured figures next to each), pitch.PitchReport and pitch.per_phoneme on hand-made tracks, and the keyword checks of
ZeroVoxTTS without a model."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import pitch_ref as R
from zerovox_amd import _lib
from zerovox_amd import pitch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_the_call_the_struct_and_the_enum():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"zvx_status\s+zvx_pitch\s*\(([^;]*)\)\s*;", code)
    assert m, "zvx_pitch not declared"
    # (the declaration carries comments between a name and its comma: the blank they leave is not part of it)
    assert " ".join(m.group(1).split()).replace(" ,", ",") == ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, "
                                            "const zvx_pitch_params* params, float* f0, float* aper, int64_t f_stride, int32_t* frames, "
                                            "double* stats, int flags")
    m = re.search(r"typedef struct zvx_pitch_params\s*\{([^}]*)\}\s*zvx_pitch_params;", code)
    assert m and " ".join(m.group(1).split()) == "float fmin, fmax; float threshold; float gate_db; int32_t window; int32_t hop;"
    m = re.search(r"enum\s*\{\s*(ZVX_PS_FRAMES[^}]*)\}", code)
    assert m and " ".join(m.group(1).split()) == "ZVX_PS_FRAMES = 0, ZVX_PS_VOICED, ZVX_PS_MEDIAN, ZVX_PS_LOW, ZVX_PS_HIGH, ZVX_PS_MEAN, ZVX_PS_COUNT = 6"
    assert h.index("zvx_status zvx_loudness_stats(") < h.index("Pitch report:") < h.index("zvx_status zvx_pitch(") < h.index("zvx_status zvx_true_peak(")
    for text in ("tau_min = max(2, floor(fs / fmax))", "tau_max = ceil(fs / fmin)", "c = (W + tau_max) / 2", "F = n / H", "AMBIGUOUS", "relative 1e-9",
                 "((n_v - 1) * 50 + 50) / 100", "((n_v - 1) * 5 + 50) / 100", "((n_v - 1) * 95 + 50) / 100", "f_stride < max(1, Nmax / hop)",
                 "tau_max < tau_min + 2", '"post.pitch"', "window > 4096 or tau_max > 2048", "65536 frames", "pYIN", "a windowed or streaming form",
                 "speaker-similarity"):
        assert text in h, text


def test_binding_exports_and_python_entry_points():
    assert "zvx_pitch" in _lib.EXPORTS
    assert (_lib.ZVX_PS_FRAMES, _lib.ZVX_PS_VOICED, _lib.ZVX_PS_MEDIAN, _lib.ZVX_PS_LOW, _lib.ZVX_PS_HIGH, _lib.ZVX_PS_MEAN, _lib.ZVX_PS_COUNT) == tuple(range(7))
    assert _lib.PITCH_STATS_KEYS == ("frames", "voiced", "median", "low", "high", "mean") and len(_lib.PITCH_STATS_KEYS) == _lib.ZVX_PS_COUNT
    assert C.sizeof(_lib.PitchParams) == 24
    assert [(n, t) for n, t in _lib.PitchParams._fields_] == [("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float), ("gate_db", C.c_float),
                                                              ("window", C.c_int32), ("hop", C.c_int32)]
    lib = _lib.load()
    vp = C.c_void_p
    assert lib.zvx_pitch.argtypes == [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(_lib.PitchParams), vp, vp, C.c_int64, vp, vp, C.c_int]
    p = inspect.signature(_lib.Context.pitch).parameters
    assert list(p) == ["self", "rows", "rate", "fmin", "fmax", "threshold", "gate_db", "window", "hop", "lengths", "curves"]
    assert [p[k].default for k in list(p)[2:]] == [None, 60.0, 500.0, 0.15, -60.0, None, None, None, True]
    # the caps admit the defaults at every rate from 8 to 48 kHz (and say where they end)
    for rate in (8000, 16000, 22050, 24000, 32000, 44100, 48000):
        assert P.tau_max(rate, 60.0) <= _lib.PITCH_MAX_TAU and P.default_window(rate, 60.0) <= _lib.PITCH_MAX_WINDOW
    assert (P.tau_max(48000, 60.0), P.default_window(48000, 60.0)) == (800, 1600)


def test_library_exports_the_entry_point():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_pitch")
    vp = C.c_void_p
    lib.zvx_pitch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int]
    assert lib.zvx_pitch(None, None, None, 0, 0, 0, None, None, None, 0, None, None, 0) == _lib.ZVX_E_INVALID       # a NULL context


def test_keywords_default_to_off_and_are_checked_without_a_model():
    from zerovox_amd.synthesize import ZeroVoxTTS
    for fn in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long):
        p = inspect.signature(fn).parameters
        assert p["pitch_report"].default is False and p["pitch_report"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["report"].default is False                       # the loudness report's keyword stays what it was
    p = inspect.signature(ZeroVoxTTS.pitch_report).parameters
    assert list(p)[:3] == ["self", "wav", "sampling_rate"] and p["sampling_rate"].default is None
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                   # no model: whatever touches it raises AttributeError, not ValueError
    assert synth.last_pitch_report is None
    assert ZeroVoxTTS._pitch_keywords(False) is None and ZeroVoxTTS._pitch_keywords(None) is None and ZeroVoxTTS._pitch_keywords(True) == {}
    assert ZeroVoxTTS._pitch_keywords(dict(fmin=80.0, fmax=400.0)) == dict(fmin=80.0, fmax=400.0)
    wav = np.zeros(800, np.float32)
    for bad, name in ((dict(fmin=500.0, fmax=60.0), "fmin"), (dict(fmin=float("nan")), "fmin"), (dict(fmax=float("inf")), "fmax"), (dict(fmin=0.0), "fmin"),
                      (dict(threshold=0.0), "threshold"), (dict(threshold=1.5), "threshold"), (dict(gate_db=3.0), "gate_db"),
                      (dict(gate_db=float("-inf")), "gate_db"), (dict(window=1), "window"), (dict(hop=0), "hop"), (dict(smoothing=1), "smoothing")):
        with pytest.raises(ValueError, match=name):
            synth.pitch_report(wav, 8000, **bad)
        with pytest.raises(ValueError, match=name):
            synth.tts("hello there", None, pitch_report=bad)
        with pytest.raises(ValueError, match=name):
            synth.tts_long("hello there. and again.", None, pitch_report=bad)
    with pytest.raises(ValueError, match="pitch_report"):
        synth.tts("hello there", None, pitch_report="yes")
    with pytest.raises(AttributeError):
        synth.pitch_report(wav, 8000)                        # good keywords: it goes on to the model it does not have


# ------------------------------------------------------------------------------------------------ the reference against the truth
@pytest.fixture(scope="module")
def ref8k():
    rows, inst = R.rows_8k()
    return rows, inst, {k: R.track(x, **R.P8K) for k, x in rows.items()}


def test_geometry_helpers():
    assert (P.tau_min(8000, 400.0), P.tau_max(8000, 80.0)) == (20, 100) == R.geometry(8000, 80.0, 400.0, 200)[:2]
    assert (P.tau_min(22050, 500.0), P.tau_max(22050, 60.0)) == (44, 368)
    assert P.tau_min(4000, 3000.0) == 2                      # never below 2
    assert (P.frames(2400, 80), P.frames(79, 80), P.frames(0, 80)) == (30, 0, 0)
    assert (P.default_hop(22050, 22050, 256), P.default_hop(8000, 22050, 256), P.default_hop(48000), P.default_hop(50)) == (256, 80, 480, 1)
    assert R.geometry(48000, 60.0, 500.0) == (96, 800, 1600, 1200)


@pytest.mark.parametrize("name, truth, hold", [("h100", 100.0, 2.0), ("h155", 155.3, 2.0), ("h220", 220.0, 2.0), ("strong2", 130.0, 0.1)])
def test_harmonic_rows_read_their_fundamental(ref8k, name, truth, hold):
    """measured with this restatement: 0.13, 0.15, 0.65 cents for the three harmonic rows (hold 2), 0.084 for the row whose second harmonic
    is 2.5 times its fundamental (hold 0.1)"""
    r = ref8k[2][name]
    F = r["frames"]
    assert F == 30 and r["ambiguous"] == []
    inner = r["f0_64"][3:F - 3]
    assert (inner > 0).all()
    worst = float(np.abs(R.cents(inner, truth)).max())
    print(f"{name}: worst {worst:.4f} cents over frames 3 .. {F - 4}")
    assert worst <= hold


def test_noise_silence_and_a_row_under_the_gate_are_unvoiced(ref8k):
    """measured: the smallest d' of the noise row is 0.73 (this generator and seed)"""
    res = ref8k[2]
    for name in ("noise", "silence", "quiet"):
        r = res[name]
        assert r["frames"] == 30 and r["ambiguous"] == [] and not (r["f0"] > 0).any(), name
    print("noise: smallest d'", float(res["noise"]["aper"].min()))
    assert res["noise"]["aper"].min() > 0.5
    assert (res["silence"]["aper"] == 1.0).all()              # c[tau] == 0 everywhere: d' = 1
    # the quiet row is the 100 Hz row times 3e-4: periodic (d' dips under the threshold), only its power keeps it unvoiced
    assert res["quiet"]["aper"].min() < 0.15
    assert (res["short"]["frames"], res["empty"]["frames"]) == (0, 0)        # n < H: no frame


def test_a_glide_is_followed(ref8k):
    """measured: 48 of 50 frames voiced (the first two are half padding), at most 10.3 cents from the instantaneous fundamental (hold 15)"""
    _, inst, res = ref8k
    r = res["glide"]
    assert r["frames"] == 50 and r["ambiguous"] == []
    v = r["f0"] > 0
    assert int(v.sum()) == 48
    worst = float(np.abs(R.cents(r["f0_64"][v], inst[np.arange(50) * 80][v])).max())
    print(f"glide: worst {worst:.3f} cents")
    assert worst <= 15.0


def test_model_rate_row():
    """measured: 0.031 cents (hold 0.05)"""
    r = R.track(R.harmonic(120.0, 11025, 22050), rate=22050, fmin=60.0, fmax=500.0, window=1024, hop=256)
    F = r["frames"]
    assert F == 43 and r["ambiguous"] == []
    worst = float(np.abs(R.cents(r["f0_64"][3:F - 3], 120.0)).max())
    print(f"22050 Hz: worst {worst:.4f} cents")
    assert worst <= 0.05


def test_nearest_rank_statistics():
    f0 = np.array([0, 100, 0, 300, 200, 0, 400, 500], np.float32)
    assert R.stats(f0) == dict(frames=8, voiced=5, median=300.0, low=100.0, high=500.0, mean=300.0)
    assert R.stats(np.zeros(4, np.float32)) == dict(frames=4, voiced=0, median=0.0, low=0.0, high=0.0, mean=0.0)
    k = np.arange(1, 102, dtype=np.float32)                  # 101 voiced frames: ranks 50, 5, 95
    assert [R.stats(k)[q] for q in ("median", "low", "high")] == [51.0, 6.0, 96.0]
    assert R.stats(np.array([7.0], np.float32)) == dict(frames=1, voiced=1, median=7.0, low=7.0, high=7.0, mean=7.0)


# ------------------------------------------------------------------------------------------------ PitchReport, per_phoneme
def test_pitch_report_from_stats():
    stats = dict(frames=np.array([40, 10]), voiced=np.array([30.0, 0.0]), median=np.array([120.0, 0.0]), low=np.array([100.0, 0.0]),
                 high=np.array([200.0, 0.0]), mean=np.array([130.0, 0.0]), f0=[np.ones(40, np.float32), np.zeros(10, np.float32)],
                 aper=[np.zeros(40, np.float32), np.ones(10, np.float32)])
    rep = P.PitchReport.from_stats(stats)
    assert (rep.median_hz, rep.low_hz, rep.high_hz, rep.mean_hz, rep.frames) == (120.0, 100.0, 200.0, 130.0, 40)
    assert rep.range_semitones == pytest.approx(12.0) and rep.voiced_fraction == 0.75
    assert rep.f0 is stats["f0"][0] and rep.aper is stats["aper"][0]
    assert rep.as_dict() == dict(median_hz=120.0, low_hz=100.0, high_hz=200.0, mean_hz=130.0, range_semitones=rep.range_semitones, voiced_fraction=0.75,
                                 frames=40)
    s = str(rep)
    assert "median 120.0 Hz" in s and "12.00 semitones" in s and "75.0 %" in s and "40 frames" in s
    none = P.PitchReport.from_stats(stats, row=1)
    assert (none.median_hz, none.range_semitones, none.voiced_fraction, none.frames) == (0.0, 0.0, 0.0, 10)
    del stats["f0"], stats["aper"]
    assert P.PitchReport.from_stats(stats).f0 is None
    empty = P.PitchReport.from_stats(dict(frames=[0], voiced=[0], median=[0.0], low=[0.0], high=[0.0], mean=[0.0]))
    assert empty.voiced_fraction == 0.0 and empty.range_semitones == 0.0
    assert P.cents(200.0, 100.0) == pytest.approx(1200.0)


def test_per_phoneme():
    #            0    1      2      3    4      5    6    7
    f0 = [0.0, 0.0, 100.0, 0.0, 200.0, 0.0, 0.0, 0.0]
    filled = P.fill_unvoiced(f0)
    assert filled.tolist() == [100.0, 100.0, 100.0, 150.0, 200.0, 200.0, 200.0, 200.0]       # gaps at both ends are held, the inner one interpolated
    out = P.per_phoneme(f0, [2, 0, 3, 1, 0, 4, 2])
    # frames [0, 2) | first frame 2 | [2, 5) | [5, 6) | first frame 6 | [6, 10): 6, 7, then the last value twice | past the end
    assert out.tolist() == [100.0, 100.0, 150.0, 200.0, 200.0, 200.0, 200.0]
    assert P.per_phoneme([0.0, 110.0, 130.0], [1, 2]).tolist() == [110.0, 120.0]
    assert P.per_phoneme([0.0, 0.0, 0.0], [1, 2, 0]).tolist() == [0.0, 0.0, 0.0]             # nothing voiced
    assert P.per_phoneme([], [1, 2]).tolist() == [0.0, 0.0] and P.per_phoneme([100.0], []).size == 0
    assert P.per_phoneme(np.array([100.0, 0.0, 300.0], np.float32), [3]).tolist() == [200.0]
    with pytest.raises(ValueError):
        P.per_phoneme([100.0], [-1])
    assert math.isclose(P.per_phoneme([100.0, 200.0], [0, 0, 5])[2], (100.0 + 4 * 200.0) / 5)
