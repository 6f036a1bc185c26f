"""Many stream sessions per call (include/zvx.h: zvx_stream_next_many), no GPU needed: the surface (header, bindings, exports), the
scheduling of serve.StreamBatcher against a stand-in context, and the group arithmetic of csrc/stream_plan.h against the rows
ZeroVox._vocode_stream_native builds."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "stream_group_main.cpp")
NAME = "zvx_stream_next_many"


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_the_call():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"zvx_status\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert m, "zvx_stream_next_many not declared"
    assert " ".join(m.group(1).split()) == ("zvx_stream* const* sessions, int n, void* const* out, const int64_t* capacity, "
                                            "int64_t* n_out, int32_t* done, int flags")
    assert re.search(r"enum\s*\{\s*ZVX_STREAM_MANY_MAX_SESSIONS\s*=\s*64\s*,\s*ZVX_STREAM_MANY_MAX_ROWS\s*=\s*256\s*\}\s*;", code)
    assert "several utterances per session" in h and "NO session has consumed anything" in h
    with open(os.path.join(ROOT, "zerovox_amd", "csrc", "zvx_kernels.h")) as f:
        k = f.read()
    assert re.search(r"STREAM_MANY_MAX_SESSIONS\s*=\s*64\b", k) and re.search(r"STREAM_MANY_MAX_ROWS\s*=\s*256\b", k)


def test_bindings_and_keywords():
    from zerovox_amd import serve
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    assert NAME in _lib.EXPORTS
    assert (_lib.ZVX_STREAM_MANY_MAX_SESSIONS, _lib.ZVX_STREAM_MANY_MAX_ROWS) == (64, 256) == (serve.MAX_SESSIONS, serve.MAX_ROWS)
    vp = C.c_void_p
    assert _lib.load().zvx_stream_next_many.argtypes == [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                         C.POINTER(C.c_int32), C.c_int]
    p = inspect.signature(_lib.Context.stream_next_many).parameters
    assert list(p) == ["self", "streams", "capacities"] and p["capacities"].default is None
    p = inspect.signature(_lib.Context.stream_next_many_device).parameters
    assert list(p) == ["self", "streams", "ptrs", "capacities", "no_sync"] and p["no_sync"].default is False
    p = inspect.signature(serve.StreamBatcher.__init__).parameters
    assert list(p) == ["self", "ctx", "max_rows"] and p["max_rows"].default == 256
    for name in ("open", "step", "close", "__len__"):
        assert hasattr(serve.StreamBatcher, name), name
    p = inspect.signature(ZeroVox.vocode_stream_many).parameters
    assert list(p) == ["self", "mels", "chunk_frames", "halo", "chunks_per_call", "limiter", "denoise"]
    assert (p["chunk_frames"].default, p["halo"].default, p["chunks_per_call"].default) == (64, ZeroVox.STREAM_HALO, 1)
    assert p["limiter"].default is None and p["denoise"].default is None
    many, one = inspect.signature(ZeroVoxTTS.tts_stream_many).parameters, inspect.signature(ZeroVoxTTS.tts_stream).parameters
    assert list(many)[:3] == ["self", "texts", "spkembs"]
    for k, v in one.items():                                 # every stream keyword of tts_stream, with its default
        if k not in ("self", "text", "spkemb", "resident"):
            assert k in many and many[k].default == v.default and many[k].kind == v.kind, k


def test_library_exports_the_entry_point():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME)
    f = lib.zvx_stream_next_many
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    # NULL sessions, n < 1 and an array without any session are refused before anything is touched
    assert f(None, 1, None, None, None, None, 0) == _lib.ZVX_E_INVALID
    none = (C.c_void_p * 3)()
    n_out, done, cap = (C.c_int64 * 3)(-5, -5, -5), (C.c_int32 * 3)(7, 7, 7), (C.c_int64 * 3)()
    assert f(none, 0, None, cap, n_out, done, 0) == _lib.ZVX_E_INVALID
    assert f(none, -1, None, cap, n_out, done, 0) == _lib.ZVX_E_INVALID
    assert f(none, 3, None, cap, n_out, done, 0) == _lib.ZVX_E_INVALID
    assert list(n_out) == [-5] * 3 and list(done) == [7] * 3


# ------------------------------------------------------------------------------------------------ StreamBatcher's scheduling
class FakeStream:
    def __init__(self, chunks, cpc, log):
        self.left, self.cpc, self.done, self.closed, self.log = chunks, cpc, False, False, log

    def close(self):
        self.closed = True


class FakeContext:
    """what StreamBatcher needs of a context: stream_open and stream_next_many.  A piece is [session number, first chunk, rows]."""

    def __init__(self):
        self.calls, self.streams = [], []

    def stream_open(self, mel, frames=0, *, chunk_frames, chunks_per_call=1, **kw):
        s = FakeStream(-(-len(mel) // chunk_frames), chunks_per_call, [])
        s.number = len(self.streams)
        self.streams.append(s)
        return s

    def stream_next_many(self, streams, capacities=None):
        assert streams and len(streams) <= 64 and len(set(map(id, streams))) == len(streams)
        assert not any(s.done or s.closed for s in streams)
        rows = [min(s.cpc, s.left) for s in streams]
        self.calls.append([(s.number, r) for s, r in zip(streams, rows)])
        out = []
        for s, r in zip(streams, rows):
            s.left -= r
            s.done = s.left == 0
            out.append(np.full(r, s.number, np.float32))
        return out


def run_batcher(b, ctx, joins=()):
    """steps until empty; joins: {step number: [(frames, cpc), ...]} opened before that step -> per id the concatenated pieces, step log"""
    got, steps, k = {}, [], 0
    while len(b) or any(j >= k for j in dict(joins)):
        for frames, cpc in dict(joins).get(k, []):
            b.open(np.zeros((frames, 80), np.float32), chunk_frames=1, chunks_per_call=cpc)
        r = b.step()
        steps.append([i for i, _, _ in r])
        for i, piece, done in r:
            got.setdefault(i, []).append(piece)
            assert done == (i not in b._open)
        k += 1
        assert k < 1000
    return {i: np.concatenate(v) for i, v in got.items()}, steps


def test_batcher_steps_everything_that_fits():
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx)
    ids = [b.open(np.zeros((f, 80), np.float32), chunk_frames=1, chunks_per_call=c) for f, c in ((5, 2), (1, 3), (4, 1))]
    assert ids == [0, 1, 2] and len(b) == 3
    got, steps = run_batcher(b, ctx)
    assert steps == [[0, 1, 2], [0, 2], [0, 2], [2]]                 # one call per step, done sessions dropped
    assert ctx.calls == [[(0, 2), (1, 1), (2, 1)], [(0, 2), (2, 1)], [(0, 1), (2, 1)], [(2, 1)]]
    assert [len(got[i]) for i in ids] == [5, 1, 4] and len(b) == 0
    assert all(s.closed for s in ctx.streams)
    assert b.step() == []


def test_batcher_serves_the_longest_wait_first_and_nobody_starves():
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx, max_rows=4)
    for _ in range(5):                                               # five sessions of 6 chunks, 2 rows per group: two fit a step
        b.open(np.zeros((6, 80), np.float32), chunk_frames=1, chunks_per_call=2)
    got, steps = run_batcher(b, ctx)
    assert all(sum(r for _, r in call) <= 4 for call in ctx.calls)
    # by wait, ties by opening order: after [1, 2] session 3 has waited two steps, 0 and 4 one each
    assert steps[:5] == [[0, 1], [2, 3], [4, 0], [1, 2], [3, 0]]
    last_seen = {}
    for k, st in enumerate(steps):                                   # nobody waits more than ceil(5 / 2) steps between two turns
        for i in st:
            assert k - last_seen.get(i, -1) <= 3, (i, k, steps)
            last_seen[i] = k
    assert all(len(got[i]) == 6 and (got[i] == i).all() for i in range(5))


def test_batcher_skips_what_does_not_fit_but_not_forever():
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx, max_rows=3)
    b.open(np.zeros((4, 80), np.float32), chunk_frames=1, chunks_per_call=2)     # 0: 2 rows
    b.open(np.zeros((6, 80), np.float32), chunk_frames=1, chunks_per_call=3)     # 1: 3 rows, only fits alone
    b.open(np.zeros((2, 80), np.float32), chunk_frames=1, chunks_per_call=1)     # 2: 1 row
    got, steps = run_batcher(b, ctx)
    assert steps[0] == [0, 2] and steps[1] == [1]                    # 1 waited one step, then goes first
    assert [len(got[i]) for i in range(3)] == [4, 6, 2]
    with pytest.raises(ValueError):
        b.open(np.zeros((9, 80), np.float32), chunk_frames=1, chunks_per_call=4)
    with pytest.raises(ValueError):
        StreamBatcher(ctx, max_rows=257)


def test_batcher_caps_the_sessions_of_a_step():
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx)
    for _ in range(70):
        b.open(np.zeros((2, 80), np.float32), chunk_frames=1)
    _, steps = run_batcher(b, ctx)
    assert steps[0] == list(range(64)) and steps[1] == list(range(64, 70)) + list(range(58))
    assert max(len(c) for c in ctx.calls) == 64


def test_batcher_takes_sessions_opened_between_steps_and_closes_on_request():
    from zerovox_amd.serve import StreamBatcher
    ctx = FakeContext()
    b = StreamBatcher(ctx)
    b.open(np.zeros((4, 80), np.float32), chunk_frames=1)
    got, steps = run_batcher(b, ctx, joins={2: [(2, 1)], 7: [(1, 1)]})
    assert steps == [[0], [0], [0, 1], [0, 1], [], [], [], [2]]
    assert [len(got[i]) for i in range(3)] == [4, 2, 1]
    i = b.open(np.zeros((4, 80), np.float32), chunk_frames=1)
    b.step()
    b.close(i)
    assert len(b) == 0 and ctx.streams[i].closed and b.step() == []
    with pytest.raises(KeyError):
        b.close(i)


# ------------------------------------------------------------------------------------------------ the group arithmetic
@pytest.fixture(scope="module")
def group_exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("group") / "stream_group_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", MAIN, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def python_rows(frames, chunk, halo, cpc, hop):
    """the groups ZeroVox._vocode_stream_native builds, read off its own vocoder calls: a mel whose frame f holds f tells a row's first
    frame, a waveform whose sample j holds j tells where the kept interior began -> the lines stream_group_main prints"""
    from zerovox_amd.model import ZeroVox
    calls = []

    def vocode_mel(batch, P, native_rate=False):
        assert batch.shape[:2] == (len(P), int(P.max()))
        for i, p in enumerate(P):
            assert (batch[i, p:] == 0).all() and (batch[i, :p, 0] == batch[i, 0, 0] + np.arange(p)).all()
        calls.append((batch[:, 0, 0].astype(np.int64), P.astype(np.int64)))
        return np.tile(np.arange(int(P.max()) * hop, dtype=np.float32), (len(P), 1))

    me = types.SimpleNamespace(_hop_length=hop, _ctx=types.SimpleNamespace(vocode_mel=vocode_mel))
    mel = np.repeat(np.arange(frames, dtype=np.float32)[:, None], 2, axis=1)
    pieces = list(ZeroVox._vocode_stream_native(me, mel, chunk, halo, cpc, True))
    lines, at, first = [], 0, 0
    for lo, P in calls:
        rows, pos = [], 0
        for i in range(len(P)):
            piece = pieces[at + i]
            rows.append((int(lo[i]), int(P[i]), int(piece[0]), len(piece), pos))
            assert (piece == piece[0] + np.arange(len(piece))).all()
            pos += len(piece)
        at += len(P)
        last = int(at == len(pieces))
        lines.append(f"group {first} {len(P)} {last} {int(P.max())} {max(r[3] for r in rows)} {pos}")
        lines += [" ".join(map(str, r)) for r in rows]
        first += len(P)
    assert at == len(pieces)
    return lines


def test_group_arithmetic_equals_the_python_rows(group_exe):
    rng = np.random.default_rng(11)
    cases = [(70, 16, 16, 3, 256), (10, 16, 16, 3, 256), (2, 1, 0, 2, 256), (33, 7, 16, 2, 256), (70, 16, 16, 1, 256),   # the GPU test's sessions
             (5, 9, 0, 1, 8), (9, 2, 5, 4, 3), (64, 64, 16, 64, 1), (1000, 1, 1000, 64, 2)]
    for _ in range(150):
        frames = int(rng.integers(2, 200))
        chunk = int(rng.integers(1, 2 * frames if rng.random() < 0.3 else 24))          # frames < chunk among them
        halo = int(rng.choice([0, 0, 1, int(rng.integers(0, 3 * chunk + 2)), 16]))    # halo = 0 and halo > chunk among them
        cases.append((frames, chunk, halo, int(rng.integers(1, 9)), int(rng.choice([1, 4, 256]))))
    assert any(f < c for f, c, _, _, _ in cases) and any(h > c for _, c, h, _, _ in cases) and any(h == 0 for _, _, h, _, _ in cases)
    want = []
    for case in cases:
        want += python_rows(*case)
    text = "".join("%d %d %d %d %d\n" % case for case in cases)
    r = subprocess.run([group_exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
