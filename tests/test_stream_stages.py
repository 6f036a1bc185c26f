"""The level and watermark stages of a stream session (include/zvx.h: zvx_stream_open_ex), no GPU needed: zvx_plan::LevelPlanner and the
five-stage chain of csrc/stream_plan.h against the Python planners they restate, what zvx_stream_open_ex sizes the leveler's buffers
from, and the surface (header, bindings, keywords, the batcher's forwarding)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from zerovox_amd import _lib, leveler, resample as RSM, stream as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "stream_stages_main.cpp")
BIG = 2 ** 32 + 5
# (h, S, a): the smallest and the largest reach the session tests and the defaults use, at 4 kHz, 22.05 kHz and a unit of 7 samples
GEOMS = [(7, 1, 0), (7, 2, 1), (7, 30, 1), (400, 1, 0), (400, 3, 3), (2205, 2, 1), (2205, 30, 1)]


def reaches(h, S_, a):
    return (S_ + 3 - a) * h - 1, (a + 1) * h - 1


def sequences(scale, seed):
    """random pushes with zeros among them, fixed small ones, one big push; each closed by push(0, last) and with its last push flagged
    last while it brings samples (what a session does); then both again behind a first push of 2^32 + 5"""
    rng = np.random.default_rng(seed)
    rand = [int(v) for v in rng.integers(0, 3 * scale + 5, 60)]
    for i in rng.integers(0, 59, 12):
        rand[int(i)] = 0
    rand[-1] = max(rand[-1], 1)
    pats = [rand, [1] * 40 + [scale] * 6, [64] * 80, [5 * scale + 5], [0, 0, 3]]
    out = []
    for sizes in pats:
        for lead in ([], [BIG]):
            out.append([(n, False) for n in lead + sizes] + [(0, True)])
            out.append([(n, False) for n in lead + sizes[:-1]] + [(sizes[-1], True)])
    return out


@pytest.fixture(scope="module")
def stages_exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("stages") / "stream_stages_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", MAIN, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def run_exe(exe, text, want):
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


@pytest.mark.parametrize("h,S_,a", GEOMS)
def test_level_planner_equals_the_python_planner(stages_exe, h, S_, a):
    RL, RR = reaches(h, S_, a)
    assert h != 2205 or (RL, RR) == leveler.reach(22050, 100.0 * S_, 100.0 * a)
    text, want = [], []
    for seq in sequences(RL // 4 + 1, RL):
        text.append(f"level {RL} {RR}")
        p = leveler.LevelPlanner(RL, RR)
        for n, last in seq:
            text.append(f"push {n} {int(last)}")
            want.append(" ".join(str(int(v)) for v in p.push(n, last)))
    run_exe(stages_exe, text, want)


def chain_push(planners, n, last):
    """one step of a session's chain: every stage is pushed with what the stage before it emitted, all with the same `last`"""
    steps = []
    for p in planners:
        steps.append(p.push(n, last))
        n = steps[-1][2]
    return steps


@pytest.mark.parametrize("rate_out", [22050, 48000, 8000])
def test_five_stage_chain_equals_the_chained_python_planners(stages_exe, rate_out):
    """reach (denoiser), level, reach (watermark), reach (limiter), rate conversion"""
    RL, RR = leveler.reach(22050, 200.0, 100.0)
    head = f"chain 1023 {RL} {RR} 1023 231 22050 {rate_out}"
    text, want = [], []
    for seq in sequences(4096, rate_out):
        text.append(head)
        ps = [S.ReachPlanner(1023), leveler.LevelPlanner(RL, RR), S.ReachPlanner(1023), S.ReachPlanner(231), RSM.StreamPlanner(22050, rate_out)]
        for n, last in seq:
            text.append(f"push {n} {int(last)}")
            want += [" ".join(str(int(v)) for v in st) for st in chain_push(ps, n, last)]
    run_exe(stages_exe, text, want)


@pytest.mark.parametrize("h,S_,a", GEOMS)
def test_what_the_session_sizes_and_assumes_of_the_leveler(h, S_, a):
    """zvx_stream_open_ex: the stage retains at most RL + RR samples between two calls and a push of n samples emits at most n + RR.
    stream_plan_step: a last push that brings samples (in_origin > 0) never has its first node under the clamp to unit U - 1 --
    out_begin / h + a - 1 <= U - 1 -- so the reach RL alone is the stage's left support."""
    RL, RR = reaches(h, S_, a)
    for seq in sequences(RL // 4 + 1, 3 * h + a):
        p = leveler.LevelPlanner(RL, RR)
        for n, last in seq:
            in_origin, out_begin, count, keep = p.push(n, last)
            assert count <= n + RR
            if not last:
                assert p.received - keep <= RL + RR
            elif count > 0 and in_origin > 0:
                U = p.received // h
                assert out_begin // h + a - 1 <= U - 1
                assert out_begin - RL >= in_origin
                first = max(0, out_begin // h + a - 1 - S_ + 1)
                assert (first - 2) * h >= in_origin


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


def test_header_declares_the_stages():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"typedef struct zvx_stream_stages \{(.*?)\} zvx_stream_stages;", code, flags=re.S)
    assert m, "zvx_stream_stages not declared"
    fields = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
    assert fields == ["const zvx_level_params* level", "const struct zvx_watermark_params* watermark", "int64_t reserved[2]"], fields
    decl = " ".join(re.search(r"zvx_status\s+zvx_stream_open_ex\s*\(([^;]*)\)\s*;", code).group(1).split())
    assert decl == ("zvx_ctx* ctx, const float* mel, int frames, const zvx_stream_params* params, const zvx_stream_stages* more, "
                    "int flags, zvx_stream** out")
    # zvx_stream_params is ABI: byte for byte what it was
    m = re.search(r"typedef struct zvx_stream_params \{(.*?)\} zvx_stream_params;", code, flags=re.S)
    assert [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()] == [
        "int32_t chunk_frames", "int32_t chunks_per_call", "int32_t halo", "const zvx_denoise_params* denoise", "const float* denoise_bias",
        "const zvx_limit_params* limit"]
    assert "resample(limit(watermark(level(denoise(plain)))))" in h
    assert "has no watermark stage" not in h and "a change of its own on top of" not in h          # the "Not here" sentences are gone


def test_bindings_and_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    assert "zvx_stream_open_ex" in _lib.EXPORTS
    assert [f[0] for f in _lib.StreamStages._fields_] == ["level", "watermark", "reserved"]
    assert C.sizeof(_lib.StreamStages) == 32 and C.sizeof(_lib.StreamParams) == 40
    p = inspect.signature(_lib.Context.stream_open).parameters
    assert p["level"].default is None and p["watermark"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("level", "watermark"))
    p = inspect.signature(ZeroVox.vocode_stream_sessions).parameters
    assert p["level"].default is None and p["watermark"].default is None
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("self", "mels"))
    p = inspect.signature(ZeroVoxTTS.tts_stream_sessions).parameters
    assert (p["level_lufs"].default, p["level_window_ms"].default, p["level_lookahead_ms"].default, p["watermark"].default) == (None, 3000.0, 100.0, None)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("self", "texts", "spkembs"))


def test_library_exports_the_entry_point():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_stream_open_ex")
    lib.zvx_stream_open_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.zvx_stream_open_ex(None, None, 0, None, None, 0, None) == _lib.ZVX_E_INVALID          # a NULL context


def test_tts_stream_sessions_checks_its_arguments_without_a_model():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                   # no model: whatever touches it raises AttributeError, not ValueError
    texts = ["hello there", "good morning"]
    for bad in (dict(level_lufs=1.0), dict(level_lufs=float("nan")), dict(level_lufs=-71.0), dict(level_lufs=-16, level_window_ms=-1.0),
                dict(level_lufs=-16, level_window_ms=100.0, level_lookahead_ms=200.0), dict(watermark=True), dict(watermark=-1),
                dict(watermark=2 ** 64), dict(watermark=dict(depth_db=1.0)), dict(watermark=dict(key=1, depth_db=7.0)),
                dict(watermark=[1, dict(key=2, period_blocks=300)]), dict(watermark=[1]), dict(watermark=[1, 2, 3]),
                dict(loudness=-16), dict(limiter=True), dict(denoise=0.5)):
        with pytest.raises(ValueError):
            synth.tts_stream_sessions(texts, None, **bad)
    with pytest.raises(ValueError, match="1 watermarks for 2 texts"):
        synth.tts_stream_sessions(texts, None, watermark=[5])
    # good arguments: a generator that has not touched the model yet
    g = synth.tts_stream_sessions(texts, None, level_lufs=-16.0, watermark=[7, dict(key=8, depth_db=2.0)], peak_db=-1.0, denoise_strength=0.5)
    assert inspect.isgenerator(g)
    # tts_stream_many keeps its refusals and is otherwise tts_stream_sessions
    with pytest.raises(ValueError, match="no level stage yet"):
        synth.tts_stream_many(texts, None, level_lufs=-16)
    with pytest.raises(ValueError, match="no watermark stage yet"):
        synth.tts_stream_many(texts, None, watermark=7)
    assert inspect.isgenerator(synth.tts_stream_many(texts, None))


# ------------------------------------------------------------------------------------------------ StreamBatcher forwards the stages
class FakeStream:
    def __init__(self, chunks, cpc):
        self.left, self.cpc, self.done, self.closed = chunks, cpc, False, False

    def close(self):
        self.closed = True


class FakeContext:
    """what StreamBatcher needs of a context: stream_open and stream_next_many; it records the keywords every session was opened with"""

    def __init__(self):
        self.opened, self.streams = [], []

    def stream_open(self, mel, frames=0, *, chunk_frames, chunks_per_call=1, **kw):
        s = FakeStream(-(-len(mel) // chunk_frames), chunks_per_call)
        self.streams.append(s)
        self.opened.append(kw)
        return s

    def stream_next_many(self, streams, capacities=None):
        out = []
        for s in streams:
            r = min(s.cpc, s.left)
            s.left -= r
            s.done = s.left == 0
            out.append(np.zeros(0, np.float32))              # (a stage still filling its reach: nothing to yield)
        return out


def test_batcher_forwards_level_and_watermark():
    from zerovox_amd import watermark as WM
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx)
    lvl = dict(target=-23.0, window_ms=200.0, lookahead_ms=100.0)
    marks = [WM.params(WM.derive_key(99, i)) for i in range(2)]
    ids = [b.open(np.zeros((5, 80), np.float32), chunk_frames=2, level=lvl, watermark=m) for m in marks]
    ids.append(b.open(np.zeros((3, 80), np.float32), chunk_frames=2))
    assert ctx.opened[0] == dict(level=lvl, watermark=marks[0]) and ctx.opened[1] == dict(level=lvl, watermark=marks[1])
    assert ctx.opened[2] == {} and marks[0]["key"] != marks[1]["key"]
    while len(b):
        b.step()
    assert all(s.closed for s in ctx.streams)


def test_vocode_stream_sessions_hands_every_session_its_own_watermark():
    """ZeroVox.vocode_stream_sessions: one params dict for all, a sequence with one per mel (None: unmarked), a wrong length refused"""
    from zerovox_amd import model as M, serve, watermark as WM

    class Model:
        _session_stages = staticmethod(M.ZeroVox._session_stages)
        denoise_bias = None

        def __init__(self):
            self._ctx = FakeContext()

    mels = [np.zeros((4, 80), np.float32)] * 3
    marks = [WM.params(1), None, WM.params(3)]
    m = Model()
    assert list(M.ZeroVox.vocode_stream_sessions(m, mels, chunk_frames=2, level=dict(target=-20.0), watermark=marks)) == []
    assert m._ctx.opened == [dict(denoise=None, bias=None, limit=None, halo=M.ZeroVox.STREAM_HALO, level=dict(target=-20.0), **(
        {} if w is None else dict(watermark=w))) for w in marks]
    m = Model()
    list(M.ZeroVox.vocode_stream_sessions(m, mels, chunk_frames=2, watermark=marks[0]))
    assert [o.get("watermark") for o in m._ctx.opened] == [marks[0]] * 3 and not any("level" in o for o in m._ctx.opened)
    m = Model()
    list(M.ZeroVox.vocode_stream_sessions(m, mels, chunk_frames=2))
    assert not any("level" in o or "watermark" in o for o in m._ctx.opened)
    m = Model()
    m.vocode_stream_sessions = lambda *a, **k: M.ZeroVox.vocode_stream_sessions(m, *a, **k)
    list(M.ZeroVox.vocode_stream_many(m, mels, chunk_frames=2))       # vocode_stream_many is a call of it
    assert len(m._ctx.opened) == 3 and not any("level" in o or "watermark" in o for o in m._ctx.opened)
    with pytest.raises(ValueError, match="2 watermarks for 3 mels"):
        list(M.ZeroVox.vocode_stream_sessions(Model(), mels, chunk_frames=2, watermark=marks[:2]))
    assert serve.MAX_SESSIONS == 64
