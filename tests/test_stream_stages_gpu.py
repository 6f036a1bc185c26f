"""The level and watermark stages of a stream session on the GPU (include/zvx.h: zvx_stream_open_ex): the resident stream against the
host-planned one and against the whole-signal chain bit for bit, the piece sizes against the chained planners, zvx_stream_next_many with
keys and level parameters shared across sessions, the NULL forms, the errors and the model's entry points.  One tiny synthetic model
serves every test; references are computed once and cached.

Geometry: 150 frames of 256 samples in chunks of 16 frames (4096 samples a call); the leveler with a window of 200 ms and 100 ms of
look-ahead at 22.05 kHz has S = 2, a = 1, RL = 4 h - 1 = 8819, RR = 2 h - 1 = 4409, so its history is dropped several times before the
last group.  Target and input are those of tests/test_level_gpu.py's stream (-16 LUFS on the vocoder's output of a standard-normal mel):
the gain is not 1, which test_the_reference_is_levelled asserts of the host-planned reference alone."""
import ctypes as C

import numpy as np
import pytest

from stream_util import err, same_bits
from zerovox_amd import _lib, denoiser as DN, leveler, limiter as LM, resample as RSM, watermark as WM

pytestmark = pytest.mark.gpu

TEXTS = ["The quick brown fox jumps over the lazy dog", "Pack my box with five dozen liquor jugs"]
FRAMES, CHUNK = 150, 16                                  # 9 full chunks and one of 6 frames; with 3 chunks per call: groups of 3, 3, 3, 1
DN_KW = dict(strength=0.5, floor=0.0)
LIM_KW = dict(ceiling=10 ** (-20 / 20), window_ms=5.0, oversample=4)
LVL_KW = dict(target=-16.0, max_gain_db=20.0, window_ms=200.0, lookahead_ms=100.0)
KEYS = [WM.derive_key(0xC0FFEE1234567, i) for i in range(3)]
WM_KW = WM.params(KEYS[0])
# chain -> (denoise, level, watermark, limit, out_rate)
CHAINS = {"plain": (None, None, None, None, 0), "level": (None, LVL_KW, None, None, 0), "watermark": (None, None, WM_KW, None, 0),
          "level+watermark": (None, LVL_KW, WM_KW, None, 0), "old": (DN_KW, None, None, LIM_KW, 0), "all": (DN_KW, LVL_KW, WM_KW, LIM_KW, 0),
          "old-48000": (DN_KW, None, None, LIM_KW, 48000), "all-48000": (DN_KW, LVL_KW, WM_KW, LIM_KW, 48000),
          "old-8000": (DN_KW, None, None, LIM_KW, 8000), "all-8000": (DN_KW, LVL_KW, WM_KW, LIM_KW, 8000),
          "level+limit-48000": (None, LVL_KW, None, LIM_KW, 48000)}
# the chain without the new stages
WITHOUT = {"level": "plain", "watermark": "plain", "level+watermark": "plain", "all": "old", "all-48000": "old-48000", "all-8000": "old-8000"}


class Env:
    def __init__(self):
        from zerovox_amd.synthesize import ZeroVoxTTS
        _, self.synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
        self.model, self.ctx = self.synth.model, self.synth.model.ctx
        self.mel = np.random.default_rng(5).standard_normal((FRAMES, 80)).astype(np.float32)
        self.bias = self.model.denoise_bias
        self.native = self.ctx.get_int("sampling_rate")
        self._host = {}

    def open(self, chain, cpc=1, mel=None, chunk=CHUNK, key=None, **kw):
        """a session of the chain through Context.stream_open (zvx_stream_open_ex where the chain has a new stage)"""
        dn, lvl, wm, lim, rate = CHAINS[chain]
        if wm is not None and key is not None:
            wm = dict(wm, key=key)
        self.ctx.set_int("out_rate", rate)
        try:
            return self.ctx.stream_open(self.mel if mel is None else mel, chunk_frames=chunk, chunks_per_call=cpc, denoise=dn,
                                        bias=self.bias if dn else None, limit=lim, level=lvl, watermark=wm, **kw)
        finally:
            self.ctx.set_int("out_rate", 0)                  # the session has captured its rate

    def host(self, chain, cpc, frames=FRAMES):
        """the host-planned stream's concatenation (ZeroVox.vocode_stream), computed once per case"""
        k = (chain, cpc, frames)
        if k not in self._host:
            dn, lvl, wm, lim, rate = CHAINS[chain]
            self.ctx.set_int("out_rate", rate)
            try:
                self._host[k] = np.concatenate(list(self.model.vocode_stream(self.mel[:frames], chunk_frames=CHUNK, chunks_per_call=cpc,
                                                                             limiter=lim, denoise=dn, level=lvl, watermark=wm)))
            finally:
                self.ctx.set_int("out_rate", 0)
            self._host[k].setflags(write=False)
        return self._host[k]

    def chained(self, chain, plain):
        """resample(limit(watermark(level(denoise(plain))))) by the whole-signal calls, every absent step dropped"""
        dn, lvl, wm, lim, rate = CHAINS[chain]
        x = plain
        if dn:
            x = self.ctx.denoise([x], self.bias, **dn)[0]
        if lvl:
            x = self.ctx.level([x], **lvl)[0][0]
        if wm:
            x = self.ctx.watermark([x], **wm)[0]
        if lim:
            x = self.ctx.limit([x], **lim)[0][0]
        if rate:
            y, n = self.ctx.resample([x], self.native, rate)
            x = y[0, :n[0]]
        return x

    def planners(self, chain):
        dn, lvl, wm, lim, rate = CHAINS[chain]
        fft = self.ctx.get_int("fft_size")
        return ([DN.DenoisePlanner(fft)] if dn else []) + \
               ([leveler.LevelPlanner(*leveler.reach(self.native, lvl["window_ms"], lvl["lookahead_ms"]))] if lvl else []) + \
               ([WM.WatermarkPlanner(fft)] if wm else []) + \
               ([LM.LimitPlanner(LM.window_samples(self.native, lim["window_ms"]), lim["oversample"])] if lim else []) + \
               ([RSM.StreamPlanner(self.native, rate)] if rate else [])

    def planned(self, chain, counts):
        """per push of the chained Python planners, the last push flagged last: the chain's output count, and every stage's"""
        plans = self.planners(chain)
        out, stages = [], []
        for j, n in enumerate(counts):
            row = []
            for p in plans:
                n = p.push(n, j == len(counts) - 1)[2]
                row.append(n)
            out.append(n)
            stages.append(row)
        return out, stages


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.model.close()


def all_pieces(s):
    """every zvx_stream_next of a session, empty pieces included"""
    out = []
    while not s.done:
        out.append(s.next_piece().copy())
    return out


def counts_of(frames, cpc, hop, chunk=CHUNK):
    """the new native samples of every group"""
    per = [min(chunk, frames - s) * hop for s in range(0, frames, chunk)]
    return [sum(per[g:g + cpc]) for g in range(0, len(per), cpc)]


def test_the_reference_is_levelled(env):
    """the host-planned reference alone: the leveler's gain is not 1 here, and the mark changes the samples"""
    plain, lv = env.host("plain", 1), env.host("level", 1)
    _, lo, hi = env.ctx.level([plain], **LVL_KW)
    print("gain", lo, hi, "peak", np.abs(plain).max(), np.abs(lv).max())
    assert len(lv) == len(plain) == FRAMES * env.ctx.hop and not same_bits(lv, plain)
    nz = plain != 0
    assert nz.any() and np.abs(lv[nz] / plain[nz] - 1.0).max() > 0.05                  # a gain that is not 1
    assert not same_bits(env.host("watermark", 1), plain)
    assert leveler.reach(env.native, 200.0, 100.0) == (4 * 2205 - 1, 2 * 2205 - 1)


@pytest.mark.parametrize("cpc", [1, 3])
@pytest.mark.parametrize("chain", list(WITHOUT))
def test_resident_stream_equals_the_host_planned_stream(env, chain, cpc):
    want = env.host(chain, cpc)
    pieces = list(env.open(chain, cpc))
    got = np.concatenate(pieces)
    assert got.dtype == np.float32 and len(pieces) >= 2 and all(len(p) for p in pieces)
    assert same_bits(got, want)
    assert same_bits(got, env.chained(chain, env.host("plain", cpc)))
    assert not same_bits(got, env.host(WITHOUT[chain], cpc))
    if chain == "level+watermark":
        assert not same_bits(got, env.host("level", cpc)) and not same_bits(got, env.host("watermark", cpc))


def test_a_single_chunk(env):
    frames = 10                                              # below chunk_frames: one chunk, one group, the FIRST push is flagged last
    for chain in ("level+watermark", "all-48000"):
        got = np.concatenate(list(env.open(chain, 3, mel=env.mel[:frames])))
        assert same_bits(got, env.host(chain, 3, frames))
        assert same_bits(got, env.chained(chain, env.host("plain", 3, frames)))
    s = env.open("all-48000", 3, mel=env.mel[:frames])
    piece = s.next_piece()
    assert s.done and len(piece) == s.info()["total"] == _lib.resampled_len(frames * env.ctx.hop, env.native, 48000)


def test_piece_sizes_follow_the_chained_planners(env):
    hop, fft = env.ctx.hop, env.ctx.get_int("fft_size")
    RL, RR = leveler.reach(env.native, 200.0, 100.0)
    for chain, cpc in (("level", 1), ("watermark", 1), ("all", 1), ("all-48000", 1), ("all-8000", 3), ("level+watermark", 3)):
        want, _ = env.planned(chain, counts_of(FRAMES, cpc, hop))
        s = env.open(chain, cpc)
        info = s.info()
        rate = CHAINS[chain][4] or env.native
        assert info["rate"] == rate and info["emitted"] == 0 and info["total"] == _lib.resampled_len(FRAMES * hop, env.native, rate)
        pieces = all_pieces(s)
        print(chain, cpc, [len(p) for p in pieces], info)
        assert [len(p) for p in pieces] == want
        assert max(len(p) for p in pieces) <= info["max_piece"]
        assert s.info()["emitted"] == sum(want) == info["total"]
        assert same_bits(np.concatenate(pieces), env.host(chain, cpc))
        dn, lvl, wm, lim, _ = CHAINS[chain]
        L, M, half = RSM.rate_pair(env.native, rate)
        delay = (fft - 1 if dn else 0) + (RR if lvl else 0) + (fft - 1 if wm else 0) + \
                (LM.reach(LM.window_samples(env.native, 5.0), 4) if lim else 0) + (-(-half // L) + 1 if half else 0)
        assert info["delay"] == delay and info["max_piece"] == -(-(cpc * CHUNK * hop + delay) * L // M) + 1
        s.close()
    # one chunk of 4096 samples behind a leveler that runs 4409 late: the first call hands out nothing
    assert env.planned("level", counts_of(FRAMES, 1, hop))[0][:2] == [0, 2 * CHUNK * hop - RR]


# the five sessions of one zvx_stream_next_many: A, B, C differ in their watermark key alone; D and E share their level parameters
# (with A .. C as well: the leveler's class is its parameters and the native rate)
MANY = [("all", 1, 0), ("all", 1, 1), ("all", 1, 2), ("level", 3, None), ("level+limit-48000", 2, None)]


def test_many_sessions_equal_their_own_runs_and_share_their_groups(env):
    ctx, hop = env.ctx, env.ctx.hop
    key = lambda k: None if k is None else KEYS[k]
    refs = [all_pieces(env.open(chain, cpc, key=key(k))) for chain, cpc, k in MANY]
    assert not same_bits(np.concatenate(refs[0]), np.concatenate(refs[1])) and not same_bits(np.concatenate(refs[1]), np.concatenate(refs[2]))
    assert same_bits(np.concatenate(refs[0]), env.host("all", 1))                      # KEYS[0] is the reference's key
    # the steps at which the keyed sessions' watermark stage emits, and any leveler does (stage 2 / 1 of "all", stage 0 of the others)
    wm_runs = [row[2] > 0 for row in env.planned("all", counts_of(FRAMES, 1, hop))[1]]
    lvl_runs = [[row[1 if chain == "all" else 0] > 0 for row in env.planned(chain, counts_of(FRAMES, cpc, hop))[1]] for chain, cpc, _ in MANY]
    live = [env.open(chain, cpc, key=key(k)) for chain, cpc, k in MANY]
    got = [[] for _ in MANY]
    ctx.set_int("profile", 2)
    try:
        step, marks, levels, drops = 0, 0, 0, 0
        while any(not s.done for s in live):
            idx = [i for i, s in enumerate(live) if not s.done]
            ctx.sync()
            ctx.reset_stats()
            pieces = ctx.stream_next_many([live[i] for i in idx])
            ctx.sync()
            tags = {t["name"]: t["launches"] for t in ctx.tag_stats()}
            for i, p in zip(idx, pieces):
                got[i].append(p.copy())
            # ONE "post.watermark" group for the three keys, ONE "post.level" group for every leveler of the call, ONE launch of drops
            assert tags.get("post.watermark", 0) == (1 if step < len(wm_runs) and wm_runs[step] else 0), (step, tags)
            assert tags.get("post.level", 0) == (1 if any(step < len(r) and r[step] for r in lvl_runs) else 0), (step, tags)
            assert tags.get("post.stream", 0) <= 1 and tags.get("voc.stream", 0) == 2, (step, tags)
            marks += tags.get("post.watermark", 0); levels += tags.get("post.level", 0); drops += tags.get("post.stream", 0)
            step += 1
        print("steps", step, "watermark groups", marks, "level groups", levels, "drop launches", drops)
        assert step == 10 and marks >= 5 and levels >= 5 and drops >= 5
    finally:
        ctx.set_int("profile", 0)
        for s in live:
            s.close()
    for i, (g, r) in enumerate(zip(got, refs)):
        assert len(g) == len(r) and all(same_bits(a, b) for a, b in zip(g, r)), i


def raw_open_ex(env, more, rate=48000):
    """zvx_stream_open_ex called directly on the denoise + limit chain -> Stream"""
    ctx = env.ctx
    dn, lm = _lib.DenoiseParams(DN_KW["strength"], DN_KW["floor"]), _lib.LimitParams(LIM_KW["ceiling"], LIM_KW["window_ms"], LIM_KW["oversample"])
    bias = np.ascontiguousarray(env.bias, np.float32)
    prm = _lib.StreamParams(CHUNK, 3, 16, C.pointer(dn), bias.ctypes.data, C.pointer(lm))
    h = C.c_void_p()
    ctx.set_int("out_rate", rate)
    try:
        rc = ctx._lib.zvx_stream_open_ex(ctx._h, _lib._ptr(env.mel), FRAMES, C.byref(prm), None if more is None else C.byref(more), 0, C.byref(h))
    finally:
        ctx.set_int("out_rate", 0)
    return rc, (_lib.Stream(ctx, h, [dn, lm, bias]) if rc == _lib.ZVX_OK else None)


def test_without_stages_it_is_zvx_stream_open(env):
    ref = all_pieces(env.open("old-48000", 3))
    want_info = env.open("old-48000", 3).info()
    for more in (None, _lib.StreamStages()):
        rc, s = raw_open_ex(env, more)
        assert rc == _lib.ZVX_OK and s.info() == want_info
        got = all_pieces(s)
        assert [len(p) for p in got] == [len(p) for p in ref] and all(same_bits(a, b) for a, b in zip(got, ref))


def short_stream(env):
    """a successful stream: the context is still usable"""
    got = np.concatenate(list(env.ctx.stream_open(env.mel[:20], chunk_frames=CHUNK)))
    assert len(got) == 20 * env.ctx.hop


def test_errors_at_open_leave_the_context_usable(env):
    """(too few samples for the watermark: with n_fft 1024 and a hop of 256 the STFT needs 385 samples, which two frames already are, so
    the one length below it is a single frame -- refused, like every other length a session cannot take, before anything is allocated)"""
    ctx, mel = env.ctx, env.mel
    nan = float("nan")
    invalid = [
        dict(mel=mel, level=dict(target=-16.0, window_ms=100.0, lookahead_ms=200.0)),       # a > S
        dict(mel=mel, level=dict(target=nan)),
        dict(mel=mel, level=dict(target=-16.0, max_gain_db=-1.0)),
        dict(mel=mel, watermark=dict(WM_KW, depth_db=7.0)),
        dict(mel=mel, watermark=dict(WM_KW, period_blocks=300)),
        dict(mel=mel, watermark=dict(WM_KW, lo_hz=9000.0)),
        dict(mel=mel[:1], watermark=WM_KW),
        dict(mel=mel, level=LVL_KW, watermark=dict(WM_KW, depth_db=nan)),
    ]
    for kw in invalid:
        with pytest.raises(_lib.ZvxError) as e:
            ctx.stream_open(chunk_frames=CHUNK, **kw)
        assert e.value.code == _lib.ZVX_E_INVALID, kw
        short_stream(env)
    with pytest.raises(_lib.ZvxError) as e:
        ctx.stream_open(mel, chunk_frames=CHUNK, level=dict(target=-16.0, window_ms=60100.0))
    assert e.value.code == _lib.ZVX_E_UNSUPPORTED
    short_stream(env)
    for word in (0, 1):
        more = _lib.StreamStages()
        more.reserved[word] = 1
        rc, _ = raw_open_ex(env, more)
        assert rc == _lib.ZVX_E_INVALID and b"reserved" in err(ctx)
        short_stream(env)
    # ... and a good session right after them
    assert same_bits(np.concatenate(list(env.open("level+watermark", 3))), env.host("level+watermark", 3))


def test_through_the_model(env):
    model, synth = env.model, env.synth
    # vocode_stream(resident=True, watermark=) and vocode_stream_sessions(level=) against their host-planned equals
    got = np.concatenate(list(model.vocode_stream(env.mel, chunk_frames=CHUNK, chunks_per_call=3, watermark=WM_KW, resident=True)))
    assert same_bits(got, env.host("watermark", 3))
    got = [p for i, p in model.vocode_stream_sessions([env.mel], chunk_frames=CHUNK, level=LVL_KW) if i == 0]
    assert same_bits(np.concatenate(got), env.host("level", 1))
    # tts_stream_sessions: two texts, a key each, the leveler for both
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    kw = dict(level_lufs=-16.0, level_window_ms=200.0, level_lookahead_ms=100.0)
    got = {}
    for i, piece in synth.tts_stream_sessions(TEXTS, spk, chunk_frames=CHUNK, watermark=[KEYS[0], KEYS[1]], **kw):
        got.setdefault(i, []).append(piece)
    assert sorted(got) == [0, 1]
    mels = dict(synth.last_stream_mels)
    lvl = synth._level(-16.0, 200.0, 100.0)
    for i in (0, 1):
        want = np.concatenate(list(model.vocode_stream(mels[i], chunk_frames=CHUNK, level=lvl, watermark=WM.params(KEYS[i]))))
        assert same_bits(np.concatenate(got[i]), want), i
        other = np.concatenate(list(model.vocode_stream(mels[i], chunk_frames=CHUNK, level=lvl, watermark=WM.params(KEYS[1 - i]))))
        assert not same_bits(want, other)
    # tts_stream_many is tts_stream_sessions without the stages
    plain = {}
    for i, piece in synth.tts_stream_many(TEXTS, spk, chunk_frames=CHUNK):
        plain.setdefault(i, []).append(piece)
    for i in (0, 1):
        assert same_bits(np.concatenate(plain[i]), np.concatenate(list(model.vocode_stream(synth.last_stream_mels[i], chunk_frames=CHUNK))))
