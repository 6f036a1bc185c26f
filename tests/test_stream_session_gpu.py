"""Stream sessions on the GPU (include/zvx.h: zvx_stream_open / zvx_stream_next): the resident stream against the host-planned one bit for
bit, the piece sizes against the chained planners, ZVX_E_BUFFER, independence from other calls on the context, the mel=None form, device
output, the errors and the accounting.  One tiny synthetic model serves every test; references are computed once and cached."""
import ctypes as C

import numpy as np
import pytest

from stream_util import err, same_bits
from zerovox_amd import _lib, denoiser as DN, limiter as LM, resample as RSM

pytestmark = pytest.mark.gpu

TEXT = "The quick brown fox jumps over the lazy dog"
FRAMES, CHUNK = 70, 16                                   # 4 full chunks and one of 6 frames; with 3 chunks per call: groups of 3 + 2
DN_KW = dict(strength=0.5, floor=0.0)
LIM_KW = dict(ceiling=10 ** (-20 / 20), window_ms=5.0, oversample=4)
CHAINS = {"plain": (None, None, 0), "denoise": (DN_KW, None, 0), "limit": (None, LIM_KW, 0), "both": (DN_KW, LIM_KW, 0),
          "both-48000": (DN_KW, LIM_KW, 48000), "both-8000": (DN_KW, LIM_KW, 8000)}


class Env:
    def __init__(self):
        from zerovox_amd.synthesize import ZeroVoxTTS
        _, self.synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
        self.model, self.ctx = self.synth.model, self.synth.model.ctx
        self.mel = np.random.default_rng(5).standard_normal((FRAMES, 80)).astype(np.float32)
        self.bias = self.model.denoise_bias
        self.native = self.ctx.get_int("sampling_rate")
        self._host = {}

    def stream(self, chain, cpc, frames=FRAMES, chunk=CHUNK, resident=False):
        dn, lim, rate = CHAINS[chain]
        self.ctx.set_int("out_rate", rate)
        try:
            return list(self.model.vocode_stream(self.mel[:frames], chunk_frames=chunk, chunks_per_call=cpc, limiter=lim, denoise=dn, resident=resident))
        finally:
            self.ctx.set_int("out_rate", 0)

    def host(self, chain, cpc, frames=FRAMES):
        """the host-planned stream's concatenation, computed once per case"""
        key = (chain, cpc, frames)
        if key not in self._host:
            self._host[key] = np.concatenate(self.stream(chain, cpc, frames))
            self._host[key].setflags(write=False)
        return self._host[key]

    def chained(self, chain, plain):
        """resample(limit(denoise(plain))) by the whole-signal calls, every absent step dropped"""
        dn, lim, rate = CHAINS[chain]
        x = plain
        if dn:
            x = self.ctx.denoise([x], self.bias, **dn)[0]
        if lim:
            x = self.ctx.limit([x], **lim)[0][0]
        if rate:
            y, n = self.ctx.resample([x], self.native, rate)
            x = y[0, :n[0]]
        return x

    def open(self, chain, cpc=1, mel=None, chunk=CHUNK, **kw):
        dn, lim, rate = CHAINS[chain]
        self.ctx.set_int("out_rate", rate)
        try:
            return self.ctx.stream_open(self.mel if mel is None else mel, chunk_frames=chunk, chunks_per_call=cpc, denoise=dn,
                                        bias=self.bias if dn else None, limit=lim, **kw)
        finally:
            self.ctx.set_int("out_rate", 0)                  # the session has captured its rate

    def planned(self, chain, counts):
        """cumulative outputs after every push of the chained Python planners, the last push flagged last"""
        dn, lim, rate = CHAINS[chain]
        plans = ([DN.DenoisePlanner(self.ctx.get_int("fft_size"))] if dn else []) + \
                ([LM.LimitPlanner(LM.window_samples(self.native, lim["window_ms"]), lim["oversample"])] if lim else []) + \
                ([RSM.StreamPlanner(self.native, rate)] if rate else [])
        out = []
        for j, n in enumerate(counts):
            for p in plans:
                n = p.push(n, j == len(counts) - 1)[2]
            out.append(n)
        return out


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


@pytest.mark.parametrize("cpc", [1, 3])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_resident_stream_equals_the_host_planned_stream(env, chain, cpc):
    want = env.host(chain, cpc)
    pieces = env.stream(chain, cpc, resident=True)
    got = np.concatenate(pieces)
    assert got.dtype == np.float32 and all(len(p) for p in pieces)
    assert same_bits(got, want)
    plain = env.host("plain", cpc)
    assert same_bits(got, env.chained(chain, plain))
    assert chain == "plain" or not same_bits(got, plain)


def test_a_single_chunk(env):
    frames = 10                                              # below chunk_frames: one chunk, one group, one call flagged last
    for chain in ("plain", "both-48000"):
        got = np.concatenate(env.stream(chain, 3, frames=frames, resident=True))
        assert same_bits(got, env.host(chain, 3, frames))
        assert same_bits(got, env.chained(chain, env.host("plain", 3, frames)))
    s = env.open("both-48000", 3, mel=env.mel[:frames])
    piece = s.next_piece()
    assert s.done and len(piece) == s.info()["total"] == _lib.resampled_len(frames * env.ctx.hop, env.native, 48000)


def test_piece_sizes_follow_the_chained_planners(env):
    hop = env.ctx.hop
    for chain, chunk in (("both-48000", CHUNK), ("both-8000", CHUNK), ("plain", CHUNK), ("both", 2), ("denoise", 2)):
        counts = [min(chunk, FRAMES - s) * hop for s in range(0, FRAMES, chunk)]
        want = env.planned(chain, counts)
        s = env.open(chain, 1, chunk=chunk)
        info = s.info()
        rate = CHAINS[chain][2] or env.native
        assert info["rate"] == rate and info["emitted"] == 0 and info["total"] == _lib.resampled_len(FRAMES * hop, env.native, rate)
        pieces = all_pieces(s)
        print(chain, chunk, [len(p) for p in pieces][:8], info)
        assert [len(p) for p in pieces] == want
        assert max(len(p) for p in pieces) <= info["max_piece"]
        assert s.info()["emitted"] == sum(want) == info["total"]
        assert same_bits(np.concatenate(pieces), env.host(chain, 1))
        if chunk == 2:
            # 512 samples per call behind a denoiser that runs 1023 samples late (and a limiter 231 more): the first calls hand out nothing
            lead = 2 if chain == "both" else 1
            assert want[:lead] == [0] * lead and want[lead] > 0
        s.close()
    dn, lim = env.ctx.get_int("fft_size") - 1, LM.reach(LM.window_samples(env.native, 5.0), 4)
    s = env.open("both-48000", 3)
    L, M, half = RSM.rate_pair(env.native, 48000)
    delay = dn + lim + -(-half // L) + 1
    assert s.info()["delay"] == delay and s.info()["max_piece"] == -(-(3 * CHUNK * hop + delay) * L // M) + 1
    s.close()
    s = env.open("plain", 3)
    assert s.info()["delay"] == 0 and s.info()["max_piece"] == 3 * CHUNK * hop + 1
    s.close()


def test_a_small_buffer_consumes_nothing(env):
    ref = all_pieces(env.open("both-48000", 1))
    s = env.open("both-48000", 1)
    got = []
    tried = 0
    while not s.done:
        n = len(ref[len(got)])
        if n > 0 and tried < 2:                              # the first two pieces that carry samples
            tried += 1
            small = np.full(n, -7.0, np.float32)
            with pytest.raises(_lib.ZvxError) as e:
                s._next(_lib._ptr(small), n - 1, 0)
            assert e.value.code == _lib.ZVX_E_BUFFER and e.value.n_out == n
            assert str(n) in str(e.value) and str(n - 1) in str(e.value)
            assert (small == -7.0).all() and not s.done and s.info()["emitted"] == sum(len(p) for p in got)
        got.append(s.next_piece(capacity=n).copy())
    assert tried == 2 and len(got) == len(ref) and all(same_bits(a, b) for a, b in zip(got, ref))


def test_sessions_do_not_depend_on_what_else_the_context_runs(env):
    ref_a, ref_b = all_pieces(env.open("both-48000", 1)), all_pieces(env.open("limit", 3))
    a, b = env.open("both-48000", 1), env.open("limit", 3)
    other_mel = np.random.default_rng(9).standard_normal((2, 33, 80)).astype(np.float32)
    other_row = (0.7 * np.random.default_rng(10).standard_normal(3000)).astype(np.float32)
    got_a, got_b = [], []
    while not (a.done and b.done):
        if not a.done:
            got_a.append(a.next_piece().copy())
        env.ctx.vocode_mel(other_mel, np.array([33, 20], np.int32))
        if not b.done:
            got_b.append(b.next_piece().copy())
        env.ctx.limit([other_row], 0.3, 2.0, 2)
    assert len(got_a) == len(ref_a) and all(same_bits(x, y) for x, y in zip(got_a, ref_a))
    assert len(got_b) == len(ref_b) and all(same_bits(x, y) for x, y in zip(got_b, ref_b))


def test_tts_stream_resident_takes_the_contexts_mel(env):
    synth = env.synth
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    kw = dict(chunk_frames=16, denoise_strength=0.5, peak_db=-20)
    want = np.concatenate(list(synth.tts_stream(TEXT, spk, **kw)))
    got = np.concatenate(list(synth.tts_stream(TEXT, spk, resident=True, **kw)))
    assert same_bits(got, want)
    plain = np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16, resident=True)))
    assert same_bits(plain, np.concatenate(list(synth.tts_stream(TEXT, spk, chunk_frames=16)))) and not same_bits(got, plain)


def test_device_output_queues(env):
    ctx = env.ctx
    ref = all_pieces(env.open("both-48000", 3))
    s = env.open("both-48000", 3)
    info = s.info()
    buf = ctx.dev_alloc(info["total"] * 4 + 64)
    try:
        at, sizes = 0, []
        while not s.done:
            n = s.next_device(buf + at * 4, info["total"] - at, no_sync=True)
            sizes.append(n)
            at += n
        ctx.sync()
        got = ctx.dev_to_host(buf, (info["total"],), np.float32)
    finally:
        ctx.dev_free(buf)
    assert sizes == [len(p) for p in ref] and at == info["total"] and same_bits(got, np.concatenate(ref))
    with pytest.raises(_lib.ZvxError) as e:                  # ZVX_NO_SYNC is for device output only
        env.open("plain")._next(None, 0, _lib.ZVX_NO_SYNC)
    assert e.value.code == _lib.ZVX_E_INVALID


def short_stream(env):
    """a successful stream: the context is still usable"""
    mel = env.mel[:20]
    got = np.concatenate(list(env.ctx.stream_open(mel, chunk_frames=CHUNK)))
    assert len(got) == 20 * env.ctx.hop


def test_errors_leave_the_context_usable(env):
    ctx, mel, bias = env.ctx, env.mel, env.bias
    bad_bias = bias.copy()
    bad_bias[3] = -1.0
    invalid = [
        dict(mel=mel[:1], chunk_frames=16),
        dict(mel=mel, chunk_frames=0),
        dict(mel=mel, chunk_frames=16, chunks_per_call=0),
        dict(mel=mel, chunk_frames=16, chunks_per_call=65),
        dict(mel=mel, chunk_frames=16, halo=-1),
        dict(mel=mel, chunk_frames=16, denoise=DN_KW),
        dict(mel=mel, chunk_frames=16, bias=bias),
        dict(mel=mel, chunk_frames=16, denoise=dict(strength=-1.0), bias=bias),
        dict(mel=mel, chunk_frames=16, denoise=dict(strength=float("nan")), bias=bias),
        dict(mel=mel, chunk_frames=16, denoise=dict(strength=0.5, floor=2.0), bias=bias),
        dict(mel=mel, chunk_frames=16, denoise=DN_KW, bias=bad_bias),
        dict(mel=mel, chunk_frames=16, limit=dict(ceiling=0.0)),
        dict(mel=mel, chunk_frames=16, limit=dict(ceiling=0.5, window_ms=0.0)),
        dict(mel=mel, chunk_frames=16, limit=dict(ceiling=0.5, oversample=3)),
        dict(mel=mel, chunk_frames=16, flags=128),
        dict(mel=None, frames=5, chunk_frames=16),
    ]
    for kw in invalid:
        with pytest.raises(_lib.ZvxError) as e:
            ctx.stream_open(**kw)
        assert e.value.code == _lib.ZVX_E_INVALID, kw
        short_stream(env)
    lib, h = ctx._lib, C.c_void_p()
    prm = _lib.StreamParams(16, 1, 16, None, None, None)
    assert lib.zvx_stream_open(ctx._h, _lib._ptr(mel), FRAMES, None, 0, C.byref(h)) == _lib.ZVX_E_INVALID and b"params" in err(ctx)
    assert lib.zvx_stream_open(ctx._h, _lib._ptr(mel), FRAMES, C.byref(prm), 0, None) == _lib.ZVX_E_INVALID
    assert lib.zvx_stream_open(None, _lib._ptr(mel), FRAMES, C.byref(prm), 0, C.byref(h)) == _lib.ZVX_E_INVALID
    short_stream(env)
    for kw in (dict(mel=mel, chunk_frames=16, flags=_lib.ZVX_PCM16), dict(mel=mel, chunk_frames=16, limit=dict(ceiling=0.5, window_ms=1000.0))):
        with pytest.raises(_lib.ZvxError) as e:
            ctx.stream_open(**kw)
        assert e.value.code == _lib.ZVX_E_UNSUPPORTED, kw
        short_stream(env)
    with pytest.raises(_lib.ZvxError) as e:                  # a session's vocoder call has voided the context's mel
        ctx.stream_open(None, chunk_frames=16)
    assert e.value.code == _lib.ZVX_E_STATE
    short_stream(env)
    s = ctx.stream_open(mel[:20], chunk_frames=16, chunks_per_call=2)
    assert len(s.next_piece()) == 20 * ctx.hop and s.done
    with pytest.raises(_lib.ZvxError) as e:
        s.next_piece()
    assert e.value.code == _lib.ZVX_E_STATE and b"done" in err(ctx)
    with pytest.raises(_lib.ZvxError) as e:
        env.open("plain")._next(None, 0, _lib.ZVX_PCM16)
    assert e.value.code == _lib.ZVX_E_UNSUPPORTED
    short_stream(env)


def test_accounting(env):
    ctx = env.ctx
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        wav = ctx.vocode_mel(env.mel[None, :40], np.array([40], np.int32))
        ctx.limit(ctx.denoise([wav[0]], env.bias, 0.5), **LIM_KW)
        ctx.sync()
        tags = {t["name"]: t for t in ctx.tag_stats() if t["launches"]}
        assert "voc.stream" not in tags and "post.denoise" in tags and "post.limit" in tags
        ctx.reset_stats()
        calls = len(all_pieces(env.open("both", 3)))
        ctx.sync()
        tags = {t["name"]: t for t in ctx.tag_stats() if t["launches"]}
        assert calls == 2 and tags["voc.stream"]["launches"] == 2 * calls and tags["voc.stream"]["bytes"] > 0
        assert "post.denoise" in tags and "post.limit" in tags and "voc.post" in tags
    finally:
        ctx.set_int("profile", 0)


def test_history_drops_are_one_launch_per_call(env):
    """zvx_stream_next drops the history of all its stages in ONE launch over a table ("post.stream"), and the drops do happen"""
    ctx = env.ctx
    s = env.open("both-48000", 3)
    ctx.set_int("profile", 2)
    try:
        calls, drops = 0, 0
        while not s.done:
            ctx.sync()
            ctx.reset_stats()
            s.next_piece()
            ctx.sync()
            tags = {t["name"]: t["launches"] for t in ctx.tag_stats()}
            assert tags.get("post.stream", 0) <= 1 and tags.get("voc.stream", 0) == 2, (calls, tags)
            drops += tags.get("post.stream", 0)
            calls += 1
        assert calls == 2 and drops >= 1
    finally:
        ctx.set_int("profile", 0)
        s.close()
