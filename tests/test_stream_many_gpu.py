"""Many stream sessions per call on the GPU (include/zvx.h: zvx_stream_next_many).  The reference for a session is always an identically
opened session stepped ALONE with zvx_stream_next: every piece of a session stepped together with others must have the same length and
the same bits, `done` must flip at the same call and zvx_stream_info must agree after every step.  One tiny synthetic model serves every
test; the references are computed once per session shape and kept read-only."""
import ctypes as C

import numpy as np
import pytest

from stream_util import err, same_bits
from zerovox_amd import _lib

pytestmark = pytest.mark.gpu

DN_KW = dict(strength=0.5, floor=0.0)
LIM_KW = dict(ceiling=10 ** (-20 / 20), window_ms=5.0, oversample=4)
CHAINS = {"plain": (None, None, 0), "denoise": (DN_KW, None, 0), "limit": (None, LIM_KW, 0), "both": (DN_KW, LIM_KW, 0),
          "both-48000": (DN_KW, LIM_KW, 48000)}
# name: (frames, chunk_frames, halo, chunks_per_call, chain)
SPECS = {
    "A": (70, 16, 16, 3, "both-48000"),      # groups of 3 + 2 rows; three stages; misaligned stage destinations (history of 2 * 1023 samples)
    "B": (10, 16, 16, 3, "plain"),           # one chunk: done in its first step, while the others go on
    "C": (2, 1, 0, 2, "plain"),              # 1-frame rows beside 48-frame rows: zero padding to the longest row
    "D": (33, 7, 16, 2, "denoise"),          # halo larger than the chunk; ragged last group
    "E": (70, 16, 16, 1, "limit"),           # joins the loop after two steps
    "F": (40, 16, 16, 2, "both"),            # the session stepped alone between two steps of the others
}


class Env:
    def __init__(self, precision):
        from zerovox_amd.synthesize import ZeroVoxTTS
        _, self.synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision=precision)
        self.model, self.ctx = self.synth.model, self.synth.model.ctx
        self.mel = np.random.default_rng(5).standard_normal((70, 80)).astype(np.float32)
        self.bias = self.model.denoise_bias
        self._ref = {}

    def open(self, spec, ctx=None, chain=None):
        frames, chunk, halo, cpc, ch = SPECS[spec] if isinstance(spec, str) else spec
        dn, lim, rate = CHAINS[chain or ch]
        ctx = ctx or self.ctx
        ctx.set_int("out_rate", rate)
        try:
            return ctx.stream_open(self.mel[:frames], chunk_frames=chunk, chunks_per_call=cpc, halo=halo, denoise=dn,
                                   bias=self.bias if dn else None, limit=lim)
        finally:
            ctx.set_int("out_rate", 0)                       # the session has captured its rate

    def ref(self, spec, chain=None):
        """the session stepped alone with zvx_stream_next -> [(piece, done, info), ...], computed once"""
        key = (spec, chain)
        if key not in self._ref:
            s, out = self.open(spec, chain=chain), []
            while not s.done:
                piece = s.next_piece().copy()
                piece.setflags(write=False)
                out.append((piece, s.done, s.info()))
            s.close()
            self._ref[key] = out
        return self._ref[key]


@pytest.fixture(scope="module")
def env():
    e = Env("bf16")
    yield e
    e.model.close()


def check_step(env, live, got, pieces, chain=None):
    """one step's pieces against the references: live = [(name, stream)], got[name] = pieces so far -> the sessions still running"""
    rest = []
    for (name, s), piece in zip(live, pieces):
        want, done, info = env.ref(name, chain)[len(got[name])]
        assert len(piece) == len(want) and same_bits(piece, want), (name, len(got[name]), len(piece), len(want))
        assert s.done == done and s.info() == info, (name, len(got[name]))
        got[name].append(piece.copy())
        if s.done:
            s.close()
        else:
            rest.append((name, s))
    return rest


def run_together(env, names, join=None, order=None, chain=None, between=None):
    """steps the sessions `names` together until each is done, finished ones dropped; join = (step, name) lets a session in later"""
    live = [(n, env.open(n, chain=chain)) for n in names]
    got = {n: [] for n in names}
    k = 0
    while live or (join and k <= join[0]):
        if join and k == join[0]:
            live.append((join[1], env.open(join[1], chain=chain)))
            got[join[1]] = []
        if order:
            live = order(live)
        pieces = env.ctx.stream_next_many([s for _, s in live])
        live = check_step(env, live, got, pieces, chain)
        if between:
            between()
        k += 1
        assert k < 50
    for n, v in got.items():
        assert len(v) == len(env.ref(n, chain)), n
    return got


def test_same_pieces(env):
    got = run_together(env, ["A", "B", "C", "D"], join=(2, "E"))
    assert len(got["B"]) == 1 and len(got["A"]) == 2 and len(got["C"]) == 1 and len(got["D"]) == 3 and len(got["E"]) == 5
    total = sum(len(p) for p in got["A"])
    assert total == _lib.resampled_len(70 * env.ctx.hop, env.ctx.get_int("sampling_rate"), 48000)
    assert not same_bits(np.concatenate(got["E"]), np.concatenate([p for p, _, _ in env.ref("E", "plain")]))     # the stages do run


def test_order_and_company_do_not_matter(env):
    run_together(env, ["A", "B", "C", "D"], join=(2, "E"), order=lambda live: live[::-1])
    run_together(env, ["A"])                                 # n = 1
    run_together(env, ["C", "A"])


def test_together_equals_the_host_planned_stream(env):
    """The reference of this file, the session stepped alone, runs the same stepping code as the sessions stepped together; this test
    anchors a together-run on the independent path: the host-planned Python stream (three Python planners, the window calls)."""
    names = ["A", "D"]
    live = [(n, env.open(n)) for n in names]
    got = {n: [] for n in names}
    while live:
        pieces = env.ctx.stream_next_many([s for _, s in live])
        for (n, s), piece in zip(live, pieces):
            got[n].append(piece.copy())
            if s.done:
                s.close()
        live = [(n, s) for n, s in live if not s.done]
        assert sum(len(v) for v in got.values()) < 50
    for n in names:
        frames, chunk, halo, cpc, chain = SPECS[n]
        dn, lim, rate = CHAINS[chain]
        env.ctx.set_int("out_rate", rate)
        try:
            want = np.concatenate(list(env.model.vocode_stream(env.mel[:frames], chunk_frames=chunk, halo=halo, chunks_per_call=cpc, limiter=lim,
                                                               denoise=dn, resident=False)))
        finally:
            env.ctx.set_int("out_rate", 0)
        have = np.concatenate(got[n])
        assert len(have) == len(want) and same_bits(have, want), (n, len(have), len(want))


def test_all_or_nothing_capacity(env):
    names = ["A", "D", "E"]
    live = [(n, env.open(n)) for n in names]
    got = {n: [] for n in names}
    tried = 0
    while live:
        sizes = [len(env.ref(n)[len(got[n])][0]) for n, _ in live]
        short = next((i for i in range(len(live) - 1, -1, -1) if sizes[i] > 0), None)
        if short is not None and tried < 2:                  # the last session of the call that carries samples gets one sample too few
            tried += 1
            caps = list(sizes)
            caps[short] -= 1
            before = [s.info() for _, s in live]
            with pytest.raises(_lib.ZvxError) as e:
                env.ctx.stream_next_many([s for _, s in live], caps)
            assert e.value.code == _lib.ZVX_E_BUFFER and e.value.n_out == sizes
            assert f"capacity[{short}]" in str(e.value) and str(sizes[short]) in str(e.value) and str(sizes[short] - 1) in str(e.value)
            assert [s.info() for _, s in live] == before and not any(s.done for _, s in live)
        pieces = env.ctx.stream_next_many([s for _, s in live], sizes)
        live = check_step(env, live, got, pieces)
    assert tried == 2


def voc_tags(ctx):
    ctx.sync()
    return {t["name"]: t for t in ctx.tag_stats() if t["launches"] and t["name"].startswith("voc.")}


def test_one_vocoder_run_two_gathers(env):
    ctx, names = env.ctx, ["A", "B", "D"]
    ctx.set_int("profile", 2)
    try:
        single = {}
        for n in names:
            s = env.open(n)
            ctx.sync()
            ctx.reset_stats()
            s.next_piece()
            single[n] = voc_tags(ctx)
            s.close()
            assert single[n]["voc.stream"]["launches"] == 2
        live = [env.open(n) for n in names]
        ctx.sync()
        ctx.reset_stats()
        pieces = ctx.stream_next_many(live)
        many = voc_tags(ctx)
        for s in live:
            s.close()
    finally:
        ctx.set_int("profile", 0)
    print({k: (v["launches"], v["bytes"]) for k, v in many.items()}, {n: {k: v["launches"] for k, v in t.items()} for n, t in single.items()})
    assert [len(p) for p in pieces] == [len(env.ref(n)[0][0]) for n in names]
    assert many["voc.stream"]["launches"] == 2
    assert many["voc.stream"]["bytes"] == sum(single[n]["voc.stream"]["bytes"] for n in names) > 0
    assert "voc.pre" in many and set(many) == set(single["A"])
    for tag, t in many.items():                              # one run of the vocoder: every stage launches what one zvx_stream_next launches
        if tag != "voc.stream":
            assert t["launches"] == single["A"][tag]["launches"], tag


def test_device_output_queues(env):
    ctx, names = env.ctx, ["A", "C", "E"]
    live = [(n, env.open(n)) for n in names]
    total = {n: s.info()["total"] for n, s in live}
    bufs = {n: ctx.dev_alloc(total[n] * 4 + 64) for n in names}
    at, sizes = {n: 0 for n in names}, {n: [] for n in names}
    try:
        while live:
            k = ctx.stream_next_many_device([s for _, s in live], [bufs[n] + at[n] * 4 for n, _ in live], [total[n] - at[n] for n, _ in live],
                                            no_sync=True)
            for (n, _), v in zip(live, k):
                sizes[n].append(v)
                at[n] += v
            live = [(n, s) for n, s in live if not s.done]
        ctx.sync()
        got = {n: ctx.dev_to_host(bufs[n], (total[n],), np.float32) for n in names}
    finally:
        for b in bufs.values():
            ctx.dev_free(b)
    for n in names:
        assert sizes[n] == [len(p) for p, _, _ in env.ref(n)] and at[n] == total[n]
        assert same_bits(got[n], np.concatenate([p for p, _, _ in env.ref(n)])), n


def test_other_calls_in_between(env):
    other_mel = np.random.default_rng(9).standard_normal((2, 33, 80)).astype(np.float32)
    f, got_f = env.open("F"), []

    def between():
        env.ctx.vocode_mel(other_mel, np.array([33, 20], np.int32))
        if not f.done:
            got_f.append(f.next_piece().copy())

    run_together(env, ["A", "D", "E"], between=between)
    assert f.done and len(got_f) == len(env.ref("F")) and all(same_bits(p, w) for p, (w, _, _) in zip(got_f, env.ref("F")))


def test_f32_mode():
    e = Env("f32")
    try:
        got = run_together(e, ["A", "B", "C"], chain="plain")
        assert sum(len(p) for p in got["A"]) == 70 * e.ctx.hop
    finally:
        e.model.close()


def raw(ctx, handles, outs, caps, flags=0, n=None, null=()):
    """zvx_stream_next_many on raw arrays -> (status, n_out, done); null: names of the arrays passed as NULL"""
    k = len(handles)
    hs, out, cap = (C.c_void_p * max(k, 1))(*handles), (C.c_void_p * max(k, 1))(*outs), (C.c_int64 * max(k, 1))(*caps)
    n_out, done = (C.c_int64 * max(k, 1))(*([-1] * k)), (C.c_int32 * max(k, 1))()
    arg = dict(sessions=hs, out=out, capacity=cap, n_out=n_out, done=done)
    a = {key: (None if key in null else v) for key, v in arg.items()}
    rc = ctx._lib.zvx_stream_next_many(a["sessions"], k if n is None else n, a["out"], a["capacity"], a["n_out"], a["done"], flags)
    return rc, list(n_out[:k]), list(done[:k])


def test_errors_consume_nothing(env):
    ctx = env.ctx
    ctx2 = _lib.Context(env.model._packed[0], env.model._packed[1], env.model._device)
    foreign = env.open("B", ctx=ctx2)
    finished = env.open("B")
    finished.next_piece()
    assert finished.done
    tiny = [env.open((2, 1, 0, 1, "plain")) for _ in range(65)]
    wide = [env.open((64, 1, 0, 64, "plain")) for _ in range(5)]
    buf = np.empty(1 << 16, np.float32)
    p, cap = buf.ctypes.data, len(buf)
    I, S, U = _lib.ZVX_E_INVALID, _lib.ZVX_E_STATE, _lib.ZVX_E_UNSUPPORTED
    cases = [   # (status, words of the message, the call on the pair (a, b))
        (I, None, lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], null=("sessions",))),
        (I, b"capacity", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], null=("capacity",))),
        (I, b"n_out", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], null=("n_out",))),
        (I, b"done", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], null=("done",))),
        (I, None, lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], n=0)),
        (I, None, lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], n=-3)),
        (I, b"sessions[1] is NULL", lambda a, b: raw(ctx, [a._h, None, b._h], [p, p, p], [cap] * 3)),
        (I, b"same session", lambda a, b: raw(ctx, [a._h, b._h, a._h], [p, p, p], [cap] * 3)),
        (I, b"another context", lambda a, b: raw(ctx, [a._h, foreign._h, b._h], [p, p, p], [cap] * 3)),
        (I, b"negative", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, -1])),
        (I, b"out is NULL", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], null=("out",))),
        (I, b"out[1] is NULL", lambda a, b: raw(ctx, [a._h, b._h], [p, None], [cap, cap])),
        (I, b"unknown flag", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], flags=128)),
        (I, b"ZVX_NO_SYNC", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], flags=_lib.ZVX_NO_SYNC)),
        (S, b"sessions[1] is done", lambda a, b: raw(ctx, [a._h, finished._h, b._h], [p, p, p], [cap] * 3)),
        (U, b"ZVX_PCM16", lambda a, b: raw(ctx, [a._h, b._h], [p, p], [cap, cap], flags=_lib.ZVX_PCM16)),
        (U, b"65 sessions", lambda a, b: raw(ctx, [s._h for s in tiny], [p] * 65, [cap] * 65)),
        (U, b"320 rows", lambda a, b: raw(ctx, [s._h for s in wide], [p] * 5, [cap] * 5)),
    ]
    try:
        for status, words, call in cases:
            live = [("E", env.open("E")), ("D", env.open("D"))]
            got = {"E": [], "D": []}
            live = check_step(env, live, got, ctx.stream_next_many([s for _, s in live]))       # the error strikes sessions under way
            before = [s.info() for _, s in live]
            rc, _, _ = call(live[0][1], live[1][1])
            assert rc == status, (status, words, rc, err(ctx))
            assert words is None or words in err(ctx), (words, err(ctx))
            assert [s.info() for _, s in live] == before
            while live:
                live = check_step(env, live, got, ctx.stream_next_many([s for _, s in live]))
            assert len(got["E"]) == len(env.ref("E")) and len(got["D"]) == len(env.ref("D"))
        assert all(s.info()["emitted"] == 0 and not s.done for s in tiny + wide)
        # 64 sessions and 256 rows are still served: the caps are the first counts refused
        pieces = ctx.stream_next_many(tiny[:64])
        assert all(len(x) == ctx.hop for x in pieces) and same_bits(pieces[0], pieces[63])
        pieces = ctx.stream_next_many(wide[:4])
        assert all(len(x) == 64 * ctx.hop and s.done for x, s in zip(pieces, wide[:4])) and same_bits(pieces[0], pieces[3])
    finally:
        for s in tiny + wide + [foreign, finished]:
            s.close()
        ctx2.close()


def test_python_layers(env):
    from zerovox_amd.serve import StreamBatcher
    model, synth, ctx = env.model, env.synth, env.ctx
    # ---- vocode_stream_many: per index the concatenation of vocode_stream(resident=True)
    mels = [env.mel[:70], env.mel[:10], env.mel[5:38]]
    kw = dict(chunk_frames=16, chunks_per_call=2, limiter=LIM_KW, denoise=DN_KW)
    got = {}
    for i, piece in model.vocode_stream_many(mels, **kw):
        assert len(piece) and piece.dtype == np.float32
        got.setdefault(i, []).append(piece.copy())
    for i, m in enumerate(mels):
        assert same_bits(np.concatenate(got[i]), np.concatenate(list(model.vocode_stream(m, resident=True, **kw)))), i
    # ---- tts_stream_many: the front end as one batch, the sessions on its mels
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    texts = ["The quick brown fox jumps over the lazy dog", "Hello there", "   "]
    got = {}
    for i, piece in synth.tts_stream_many(texts, spk, chunk_frames=16, denoise_strength=0.5, peak_db=-20):
        got.setdefault(i, []).append(piece.copy())
    assert sorted(got) == [0, 1] and sorted(synth.last_stream_mels) == [0, 1]
    lim, den = synth._limiter(True, 5.0, -20), synth._denoise(0.5)
    for i in (0, 1):
        want = np.concatenate(list(model.vocode_stream(synth.last_stream_mels[i], chunk_frames=16, limiter=lim, denoise=den, resident=True)))
        assert same_bits(np.concatenate(got[i]), want), i
    # ---- StreamBatcher under a row budget that forces two rounds per step: A brings 3 rows, D 2, E 1, B 1
    b = StreamBatcher(ctx, max_rows=4)
    ids, got, steps = {}, {}, 0
    for n in ("A", "D", "E", "B"):
        frames, chunk, halo, cpc, chain = SPECS[n]
        dn, lim, rate = CHAINS[chain]
        ctx.set_int("out_rate", rate)
        try:
            ids[b.open(env.mel[:frames], chunk_frames=chunk, chunks_per_call=cpc, halo=halo, denoise=dn, bias=env.bias if dn else None, limit=lim)] = n
        finally:
            ctx.set_int("out_rate", 0)
    first = b.step()
    assert [ids[i] for i, _, _ in first] == ["A", "E"]               # A's 3 rows and the next that still fits; D and B wait
    for i, piece, done in first:
        got.setdefault(ids[i], []).append(piece.copy())
    while len(b):
        for i, piece, done in b.step():
            got.setdefault(ids[i], []).append(piece.copy())
        steps += 1
        assert steps < 50
    for n in ("A", "D", "E", "B"):
        assert same_bits(np.concatenate(got[n]), np.concatenate([p for p, _, _ in env.ref(n)])), n
