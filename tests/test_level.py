"""The leveler without a GPU (include/zvx.h: zvx_level, zvx_level_ex, zvx_level_rows): the surface (header, bindings, exports, the stream
keywords), the planner of zerovox_amd/leveler.py driven over the float64 restatement tests/level_ref.py -- a stream's pieces concatenate to
the whole-signal call exactly and every window meets the support condition --, the tightness of the two reaches, and the exact corners."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import level_ref as LV
from zerovox_amd import _lib, leveler
from zerovox_amd.stream import stream_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, WINDOW_MS, LOOKAHEAD_MS, TARGET = 4000, 300.0, 100.0, -16.0      # h = 400, S = 3, a = 1
KW = dict(rate=RATE, target=TARGET, max_gain_db=20.0, window_ms=WINDOW_MS, lookahead_ms=LOOKAHEAD_MS)
_cache = {}


def header_code():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        h = f.read()
    return h, re.sub(r"/\*.*?\*/", "", h, flags=re.S)


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_the_three_calls_and_the_struct():
    h, code = header_code()
    m = re.search(r"typedef\s+struct\s+zvx_level_params\s*\{([^}]*)\}\s*zvx_level_params\s*;", code)
    assert m, "zvx_level_params not declared"
    assert " ".join(m.group(1).split()) == "float target_lufs; float max_gain_db; float window_ms; float lookahead_ms;"
    base = ("zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* params, void* out, "
            "int64_t out_stride, float* gain_lo, float* gain_hi, int flags")
    for name, tail in (("zvx_level", ""), ("zvx_level_ex", ", int64_t in_origin, int64_t out_begin, int64_t out_count, int last"),
                       ("zvx_level_rows", ", const zvx_row_window* win")):
        m = re.search(r"zvx_status\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name + " not declared"
        assert " ".join(m.group(1).split()) == base + tail, name
    for text in ("RL = (S + 3 - a) h - 1", "RR = (a + 1) h - 1", "zvx_level is zvx_level_ex(..., 0, 0, -1, 1)", '"post.level"',
                 "the absolute gate of BS.1770 applied per 100 ms unit", "part of the contract, not an", "relative gating",
                 "a level stage inside zvx_stream_open"):
        assert text in h, text
    # the paragraphs this block refers to stay as they were
    assert "Not here: momentary /" in h and "a streamed loudness gain (it is not known before the last chunk)" in h


def test_bindings_and_exports():
    for name in ("zvx_level", "zvx_level_ex", "zvx_level_rows"):
        assert name in _lib.EXPORTS, name
    assert C.sizeof(_lib.LevelParams) == 16
    assert [f[0] for f in _lib.LevelParams._fields_] == ["target_lufs", "max_gain_db", "window_ms", "lookahead_ms"]
    lib = _lib.load()
    assert lib.zvx_level.argtypes[6] == C.POINTER(_lib.LevelParams) and len(lib.zvx_level.argtypes) == 12
    assert lib.zvx_level_ex.argtypes == lib.zvx_level.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    assert lib.zvx_level_rows.argtypes == lib.zvx_level.argtypes + [C.POINTER(_lib.RowWindow)]
    p = inspect.signature(_lib.Context.level).parameters
    assert list(p)[:6] == ["self", "rows", "target", "max_gain_db", "window_ms", "lookahead_ms"]
    assert (p["max_gain_db"].default, p["window_ms"].default, p["lookahead_ms"].default, p["pcm16"].default, p["lengths"].default) == \
        (20.0, 3000.0, 100.0, False, None)
    p = inspect.signature(_lib.Context.level_window).parameters
    assert (p["in_origin"].default, p["out_begin"].default, p["out_count"].default, p["last"].default) == (0, 0, -1, True)
    assert list(inspect.signature(_lib.Context.level_rows).parameters)[:4] == ["self", "rows", "windows", "target"]


def test_library_exports_the_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    base = [vp] * 3 + [C.c_int] * 3 + [vp, vp, C.c_int64, vp, vp, C.c_int]
    for name in ("zvx_level", "zvx_level_ex", "zvx_level_rows"):
        assert hasattr(lib, name), name
    lib.zvx_level.argtypes = base
    lib.zvx_level_ex.argtypes = base + [C.c_int64] * 3 + [C.c_int]
    lib.zvx_level_rows.argtypes = base + [vp]
    assert lib.zvx_level(None, None, None, 0, 0, 0, None, None, 0, None, None, 0) == _lib.ZVX_E_INVALID          # a NULL context
    assert lib.zvx_level_ex(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, 0, 0, -1, 1) == _lib.ZVX_E_INVALID
    assert lib.zvx_level_rows(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None) == _lib.ZVX_E_INVALID


def test_stream_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    p = inspect.signature(ZeroVoxTTS.tts_stream).parameters
    assert (p["level_lufs"].default, p["level_window_ms"].default, p["level_lookahead_ms"].default) == (None, 3000.0, 100.0)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("level_lufs", "level_window_ms", "level_lookahead_ms"))
    assert inspect.signature(ZeroVox.vocode_stream).parameters["level"].default is None
    assert "level" not in inspect.signature(ZeroVoxTTS.tts).parameters           # the whole-utterance answer stays loudness=
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                   # no model: whatever touches it raises AttributeError, not ValueError
    with pytest.raises(ValueError, match="level_lufs"):
        synth.tts_stream("hello there", None, loudness=-16)
    with pytest.raises(ValueError, match="no level stage yet"):
        synth.tts_stream("hello there", None, level_lufs=-16, resident=True)
    with pytest.raises(ValueError, match="no level stage yet"):
        synth.tts_stream_many(["hello there"], None, level_lufs=-16)
    for bad in (dict(level_lufs=1.0), dict(level_lufs=float("nan")), dict(level_lufs=-71.0), dict(level_lufs=-16, level_window_ms=-1.0),
                dict(level_lufs=-16, level_lookahead_ms=float("inf")), dict(level_lufs=-16, level_window_ms=100.0, level_lookahead_ms=200.0),
                dict(level_lufs=-16, level_window_ms=60100.0)):
        with pytest.raises(ValueError):
            synth.tts_stream("hello there", None, **bad)
    assert ZeroVoxTTS._level(None, 3000.0, 100.0) is None
    assert ZeroVoxTTS._level(-16, 3000.0, 100.0) == dict(target=-16.0, window_ms=3000.0, lookahead_ms=100.0)


# ------------------------------------------------------------------------------------------------ geometry and planner
def test_geometry():
    assert leveler.units(4000) == 400 and leveler.units(22050) == 2205 and leveler.units(44100) == 4410
    assert leveler.window_units(3000.0) == 30 and leveler.window_units(0.0) == 1 and leveler.window_units(49.0) == 1 and leveler.window_units(300.0) == 3
    assert leveler.reach(4000, 300.0, 100.0) == (1999, 799)
    assert leveler.reach(22050, 3000.0, 100.0) == (32 * 2205 - 1, 4409)
    assert leveler.reach(22050, 3000.0, 0.0) == (33 * 2205 - 1, 2204)
    assert LV.geometry(RATE, WINDOW_MS, LOOKAHEAD_MS) == (400, 3, 1, 1999, 799)
    with pytest.raises(ValueError):
        leveler.reach(4000, 100.0, 200.0)
    p = leveler.LevelPlanner(1999, 799)
    assert p.push(500) == (0, 0, 0, 0)                       # fewer than RR samples: nothing is final
    assert p.push(500) == (0, 0, 201, 0)                     # 1000 received: outputs [0, 201)
    assert p.push(3000) == (0, 201, 3000, 1202)              # emits up to 4000 - 799 = 3201; history before 3201 - 1999 goes
    assert p.push(0, True) == (1202, 3201, 799, 2001)


def signal():
    """a speech-like row with bursts at levels from far below the gate's reach to loud, and a zero stretch longer than S + 2 units"""
    if "sig" not in _cache:
        x = LV.bursts(np.random.default_rng(41), 5 * 400 + 123, RATE, [0.1, 0.004, 0.3, 0.03])
        y = LV.bursts(np.random.default_rng(42), 13 * 400 + 57, RATE, [0.2, 0.01, 0.05], zero_units=6, zero_at=4)
        for a in (x, y):
            a.setflags(write=False)
        _cache["sig"] = (x, y)
        _cache["whole"] = tuple(LV.level(s, **KW) for s in (x, y))
    return _cache["sig"], _cache["whole"]


def run_stream(x, sizes):
    """the reference leveler driven by LevelPlanner over x cut into chunks of `sizes` -> (pieces, windows)"""
    windows = []

    def fn(samples, in_origin, out_begin, out_count, last):
        windows.append((in_origin, len(samples), out_begin, out_count, last))
        return LV.level_window(samples, in_origin, out_begin, out_count, last, **KW)["out"]
    chunks, at, i = [], 0, 0
    while at < len(x):
        chunks.append(x[at:at + sizes[i % len(sizes)]])
        at += len(chunks[-1])
        i += 1
    planner = leveler.LevelPlanner(*leveler.reach(RATE, WINDOW_MS, LOOKAHEAD_MS))
    return list(leveler.stream_level(chunks, planner, fn)), windows


def test_stream_level_is_the_shared_loop():
    assert leveler.stream_level is stream_windows
    p = inspect.signature(leveler.LevelPlanner.push).parameters
    assert list(p) == ["self", "n_new", "last"] and p["last"].default is False


@pytest.mark.parametrize("name", ["one sample", "h", "one chunk", "below RR", "random"])
def test_a_streams_pieces_concatenate_to_the_whole_call(name):
    (x, y), (wx, wy) = signal()
    RL, RR = leveler.reach(RATE, WINDOW_MS, LOOKAHEAD_MS)
    sig, want = (x, wx) if name == "one sample" else (y, wy)             # (one window per sample: the shorter row)
    rng = np.random.default_rng(7)
    sizes = {"one sample": [1], "h": [400], "one chunk": [len(sig)], "below RR": [RR - 1, 13, RR // 2],
             "random": [int(v) for v in rng.integers(1, 1500, 40)]}[name]
    pieces, windows = run_stream(sig, sizes)
    got = np.concatenate(pieces)
    assert got.dtype == np.float32 and len(got) == len(sig)
    assert np.array_equal(got.view(np.uint32), want["out"].view(np.uint32)), name
    for o, n_in, begin, cnt, last in windows:                # (level_window asserts it as well)
        assert LV.supported(RL, RR, o, n_in, begin, cnt, last), (o, n_in, begin, cnt, last)
    assert windows[-1][4] and not any(w[4] for w in windows[:-1])
    if name != "one chunk":
        assert len(windows) >= 3
        assert max(w[1] for w in windows[1:]) <= RL + RR + max(sizes) + 1      # the history stays bounded
    if name in ("h", "random"):
        assert any(w[0] > 0 and w[0] % 400 for w in windows), "no window starts off the unit grid"


def test_the_leveler_acts_and_rests():
    (x, y), (wx, wy) = signal()
    h = 400
    p = LV.units(y, RATE)
    G = LV.gains(p, 3, TARGET)
    assert np.all(p[6:10] == 0.0) and G[8] == 1.0 and G[9] == 1.0        # a window of exact zeros: cnt == 0
    assert np.any(G == 10.0) and np.any((G > 1.0) & (G < 10.0)) and np.any(G < 1.0)      # max_gain_db, in between, and attenuation
    # nodes 8 / 9 are G[8] / G[9] (a = 1): the samples of unit 8 keep the bits of x
    assert np.array_equal(wy["out"][8 * h:9 * h].view(np.uint32), y[8 * h:9 * h].view(np.uint32))
    assert not np.array_equal(wy["out"].view(np.uint32), y.view(np.uint32))
    assert LV.ambiguous(x, RATE) == [] and LV.ambiguous(y, RATE) == []


# ------------------------------------------------------------------------------------------------ the reaches are tight
def test_the_reaches_are_tight():
    (x, y), _ = signal()
    h, S, a, RL, RR = LV.geometry(RATE, WINDOW_MS, LOOKAHEAD_MS)
    q = 8
    rec = {}
    i = q * h                                                # the first sample of a unit: its second node's unit ends RR ahead
    LV.level_window(y[i - RL:i + RR + 1], i - RL, i, 1, False, record=rec, **KW)
    assert rec["hi"] == i + RR and rec["lo"] > i - RL
    i = q * h + h - 1                                        # the last sample of a unit: its first node's oldest unit starts RL back
    LV.level_window(y[i - RL:i + RR + 1], i - RL, i, 1, False, record=rec, **KW)
    assert rec["lo"] == i - RL and rec["hi"] < i + RR
    for i, cut in ((q * h, "right"), (q * h + h - 1, "left")):           # one sample less on that side: the read leaves the window
        o, end = (i - RL, i + RR) if cut == "right" else (i - RL + 1, i + RR + 1)
        with pytest.raises(AssertionError):
            LV.level_window(y[o:end], o, i, 1, False, **KW)


# ------------------------------------------------------------------------------------------------ corners
def test_corners():
    rng = np.random.default_rng(3)
    short = (rng.standard_normal(399) * 0.2).astype(np.float32)          # U == 0: every node is 1
    r = LV.level(short, **KW)
    assert np.array_equal(r["out"].view(np.uint32), short.view(np.uint32)) and np.all(r["g32"] == 1.0)
    assert len(LV.level(np.zeros(0, np.float32), **KW)["out"]) == 0
    zeros = np.zeros(1700, np.float32)
    zeros[5] = -0.0
    r = LV.level(zeros, **KW)
    assert np.array_equal(r["out"].view(np.uint32), zeros.view(np.uint32))
    quiet = (rng.standard_normal(2923) * 2e-3).astype(np.float32)        # above the gate, 44 dB below the target: every G is the bound
    assert np.all(LV.units(quiet, RATE) > LV.GATE)
    r = LV.level(quiet, **KW)
    assert np.all(r["g32"] == np.float32(10.0))
    assert np.array_equal(r["out"].view(np.uint32), (quiet * np.float32(10.0)).view(np.uint32))


# ------------------------------------------------------------------------------------------------ a last window whose nodes are clamped
@pytest.mark.parametrize("lookahead_ms,out_begin", [(100.0, 20 * 400 + 3), (200.0, 19 * 400 + 5), (200.0, 20 * 400), (300.0, 18 * 400 + 1)])
def test_a_last_window_that_begins_in_the_clamped_region(lookahead_ms, out_begin):
    """where the outputs of a last window begin in the signal's last a units (or its tail) the clamp to U - 1 moves the first node's window
    to the left of what RL covers: the support condition's clamped left rule asks for exactly the samples the reference then reads"""
    kw = dict(KW, lookahead_ms=lookahead_ms)
    h, S, a, RL, RR = LV.geometry(RATE, WINDOW_MS, lookahead_ms)
    N = 20 * h + 7
    x = LV.bursts(np.random.default_rng(77), N, RATE, [0.1, 0.004, 0.3, 0.03])
    want = LV.level(x, **kw)["out"]
    U = N // h
    assert out_begin // h + a - 1 > U - 1                    # the first node is clamped
    kf = min(out_begin // h + a - 1, U - 1) - S + 1
    o_max = (kf - 2) * h                                     # the oldest unit's warm-up starts here
    assert 0 < o_max < out_begin - RL, "the plain left condition alone would admit a later origin"
    ok = lambda o: LV.supported(RL, RR, o, N - o, out_begin, N - out_begin, True, (h, S, a))
    assert ok(o_max) and not ok(o_max + 1) and ok(0)
    assert LV.supported(RL, RR, o_max + 1, N - o_max - 1, out_begin, N - out_begin, True)          # (RL / RR alone do not see it)
    rec = {}
    got = LV.level_window(x[o_max:], o_max, out_begin, -1, True, record=rec, **kw)["out"]
    assert rec["lo"] == o_max and np.array_equal(got.view(np.uint32), want[out_begin:].view(np.uint32))
    with pytest.raises(AssertionError, match="read outside the window"):
        LV.level_window(x[o_max + 1:], o_max + 1, out_begin, -1, True, check=False, **kw)
    # the rule never refuses what RL admits where the clamp does not act, and every admitted window reads inside itself
    rng = np.random.default_rng(5)
    for _ in range(60):
        begin = int(rng.integers(RL + 1, N))
        o = int(rng.integers(1, begin - RL + 1))
        if begin // h + a - 1 <= U - 1:
            assert ok_at(o, begin, N, RL, RR, (h, S, a))
        if ok_at(o, begin, N, RL, RR, (h, S, a)):
            LV.level_window(x[o:], o, begin, min(3, N - begin), True, check=False, **kw)


def ok_at(o, begin, N, RL, RR, geom):
    return LV.supported(RL, RR, o, N - o, begin, min(3, N - begin), True, geom)
