"""Voice matching on the MI355X: zvx_spk_score and zvx_spk_topk against the float64 restatement of tests/voice_ref.py (never the
library), the position contract bit for bit, top-k as the exact selection over the score matrix, the refusals, voices.VoiceLibrary on the
device and ZeroVoxTTS.voice_report / tts(..., voice_report=True)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import enroll_ref as E
import voice_ref as V
from stream_util import vp
from zerovox_amd import _lib, voices

import test_enroll_gpu as TE                                 # ctx_for: the medium front end with the tiny vocoder

SENTINEL = np.uint32(0xDEADBEEF)
DIN, DOUT, NOSYNC = _lib.ZVX_DEVICE_IN, _lib.ZVX_DEVICE_OUT, _lib.ZVX_NO_SYNC
DIMS = (4, 8, 36, 264, 528, 2048)
BS, KS = (1, 3, 65), (1, 2, 63, 64, 65, 257, 1000)
PAD = 8                                                      # sentinel words behind every output


def ctx():
    return TE.ctx_for("tiny")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inputs(dim, seed=0):
    """65 queries and 1000 library rows, neither side normalised.  Library: row 1 zero, 5 scaled by 1e-20, 6 by 1e+18, 7 with a NaN, 8 with
    an inf.  Queries: 1 zero, 5 scaled by 1e-20, 6 by 1e+18."""
    rng = np.random.default_rng(1000 * dim + seed)
    q = (rng.standard_normal((65, dim)) * rng.uniform(0.2, 5.0, (65, 1))).astype(np.float32)
    lib = (rng.standard_normal((1000, dim)) * rng.uniform(0.2, 5.0, (1000, 1))).astype(np.float32)
    lib[10:20] = q[:10] * np.float32(0.7) + np.float32(0.05) * lib[10:20]      # some rows close to some queries
    lib[1] = 0.0
    lib[5] *= np.float32(1e-20)
    lib[6] *= np.float32(1e18)
    lib[7, dim // 2] = np.nan
    lib[8, dim - 1] = np.inf
    q[1] = 0.0
    q[5] *= np.float32(1e-20)
    q[6] *= np.float32(1e18)
    return q, lib


class Dev:
    """device copies of host arrays, freed at the end of the test"""

    def __init__(self, c):
        self.c, self.ptrs = c, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.c.dev_alloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.c.dev_from_host(p, a)
        return p

    def close(self):
        for p in self.ptrs:
            self.c.dev_free(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = Dev(ctx())
    yield d
    d.close()


def score_call(c, d, q, lib_ptr, K, dim, dev_in=False, dev_out=False):
    """the C call with sentinel words behind the output -> score [B][K] float32"""
    B = q.shape[0]
    flags = (DIN if dev_in else 0) | (DOUT if dev_out else 0)
    qa = d.put(q) if dev_in else np.ascontiguousarray(q)
    host = np.full(B * K + PAD, SENTINEL, np.uint32)
    out = d.put(host) if dev_out else host
    rc = c._lib.zvx_spk_score(c._h, vp(qa), B, vp(lib_ptr), K, dim, vp(out), flags)
    assert rc == 0, c._lib.zvx_last_error(c._h).decode()
    if dev_out:
        host = c.dev_to_host(out, (B * K + PAD,), np.uint32)
    assert np.all(host[B * K:] == SENTINEL)
    return host[:B * K].view(np.float32).reshape(B, K)


def topk_call(c, d, q, lib_ptr, K, dim, top, dev_in=False, dev_out=False):
    B = q.shape[0]
    flags = (DIN if dev_in else 0) | (DOUT if dev_out else 0)
    qa = d.put(q) if dev_in else np.ascontiguousarray(q)
    hs, hi = np.full(B * top + PAD, SENTINEL, np.uint32), np.full(B * top + PAD, SENTINEL, np.uint32)
    os_, oi = (d.put(hs), d.put(hi)) if dev_out else (hs, hi)
    rc = c._lib.zvx_spk_topk(c._h, vp(qa), B, vp(lib_ptr), K, dim, top, vp(os_), vp(oi), flags)
    assert rc == 0, c._lib.zvx_last_error(c._h).decode()
    if dev_out:
        hs, hi = c.dev_to_host(os_, hs.shape, np.uint32), c.dev_to_host(oi, hi.shape, np.uint32)
    assert np.all(hs[B * top:] == SENTINEL) and np.all(hi[B * top:] == SENTINEL)
    return hs[:B * top].view(np.float32).reshape(B, top), hi[:B * top].view(np.int32).reshape(B, top)


# ---- 1. scores against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_scores_against_float64(dim, dev):
    c = ctx()
    q, lib = inputs(dim)
    lib_ptr = dev.put(lib)
    ref = V.scores(q, lib)
    assert np.all(ref[:, 7] == -2.0) and np.all(ref[:, 8] == -2.0) and np.all(ref[1, [0, 2, 3]] == 0.0) and np.all(ref[[0, 2], 1] == 0.0)
    worst, n = 0.0, 0
    for B in BS:
        for K in KS:
            # host and device queries, host and device outputs: the four forms go round the cases; every form meets every B
            form = n % 4
            n += 1
            got = score_call(c, dev, q[:B], lib_ptr, K, dim, dev_in=bool(form & 1), dev_out=bool(form & 2))
            err = np.abs(got.astype(np.float64) - ref[:B, :K])
            worst = max(worst, float(err.max()))
            assert err.max() <= V.tol(dim), (dim, B, K, form, float(err.max()), V.tol(dim), np.unravel_index(err.argmax(), err.shape))
            assert np.all(got[ref[:B, :K] == -2.0] == np.float32(-2.0))
            assert np.all(got[ref[:B, :K] == 0.0] == 0.0)
    print(f"zvx_spk_score dim {dim}: largest |f32 - f64| {worst:.3e} = {worst / 2.0 ** -24:.2f} u (bound {2 * dim + 8} u)")


# ---- 2. the position contract, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (8, 528))
def test_position_contract(dim, dev):
    c = ctx()
    q, lib = inputs(dim, seed=1)
    K = 1000
    lib_ptr = dev.put(lib)
    whole = score_call(c, dev, q, lib_ptr, K, dim)
    perm = np.random.default_rng(7).permutation(K)
    permuted = score_call(c, dev, q, dev.put(lib[perm]), K, dim, dev_in=True, dev_out=True)
    assert np.array_equal(bits(permuted), bits(whole[:, perm]))              # a permuted library gives the permuted bits
    for Kp in (1, 63, 65, 513):
        assert np.array_equal(bits(score_call(c, dev, q, lib_ptr, Kp, dim)), bits(whole[:, :Kp]))
    for b in (0, 1, 5, 6, 17, 63, 64):                                       # 64: the one query of the second group
        one = score_call(c, dev, q[b:b + 1], lib_ptr, K, dim)
        assert np.array_equal(bits(one), bits(whole[b:b + 1])), b
    few = score_call(c, dev, q[60:63], lib_ptr, 257, dim, dev_in=True)
    assert np.array_equal(bits(few), bits(whole[60:63, :257]))


# ---- 3. top-k is the selection ------------------------------------------------------------------------------------------------
def slab_case():
    """dim 8, three slabs of the first launch and a ragged tail; one vector sits bit for bit on both sides of every slab boundary and
    at rows 0 and K - 1, and is query 0"""
    S = voices.SLAB_ROWS
    K, dim = 3 * S + 37, 8
    rng = np.random.default_rng(11)
    lib = rng.standard_normal((K, dim)).astype(np.float32)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    dup = [0, S - 1, S, 2 * S - 1, 2 * S, 3 * S - 1, 3 * S, K - 1]
    lib[dup] = q[0] * np.float32(1.5)
    lib[[S - 2, S + 1]] = q[2] * np.float32(0.5)             # a second tie, across a boundary, for another query
    return q, lib, dup


@pytest.mark.parametrize("top", (1, 2, 5, 32))
def test_topk_is_the_selection_over_the_score_matrix(top, dev):
    c = ctx()
    q, lib, dup = slab_case()
    K, dim = lib.shape
    lib_ptr = dev.put(lib)
    matrix = score_call(c, dev, q, lib_ptr, K, dim)
    assert len(set(bits(matrix[0, dup]).tolist())) == 1                      # the duplicates tie bit for bit
    want_s, want_i = V.topk(matrix, top)
    assert want_i[0].tolist() == dup[:top] if top <= len(dup) else want_i[0, :len(dup)].tolist() == dup   # the tie rule decides
    for form in range(4):
        got_s, got_i = topk_call(c, dev, q, lib_ptr, K, dim, top, dev_in=bool(form & 1), dev_out=bool(form & 2))
        assert np.array_equal(got_i, want_i), (top, form)
        assert np.array_equal(bits(got_s), bits(want_s)), (top, form)
    # ragged sizes round one slab and the 64-query group, special rows included
    q2, lib2 = inputs(36, seed=2)
    p2 = dev.put(lib2)
    for B, K2 in ((65, 1000), (3, 65), (1, max(top, 2)), (65, 513)):
        if top > K2:
            continue
        m2 = score_call(c, dev, q2[:B], p2, K2, 36)
        ws, wi = V.topk(m2, top)
        gs, gi = topk_call(c, dev, q2[:B], p2, K2, 36, top)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), (top, B, K2)


SEPARATED_SEED = 3


def test_topk_indices_equal_the_float64_reference(dev):
    c = ctx()
    dim, K, B, top = 36, 1000, 5, 5
    rng = np.random.default_rng(SEPARATED_SEED)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    lib = rng.standard_normal((K, dim)).astype(np.float32)
    ref = V.scores(q, lib)
    assert V.min_gap(ref, top) > 2.0 * V.tol(dim)            # on the reference alone: every query, none left out
    want_s, want_i = V.topk(ref, top)
    got_s, got_i = topk_call(c, dev, q, dev.put(lib), K, dim, top)
    assert np.array_equal(got_i, want_i)
    assert np.max(np.abs(got_s.astype(np.float64) - want_s)) <= V.tol(dim)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def refused(c, call, outputs, name, rule):
    before = [o.copy() for o in outputs]
    c.set_int("profile", 2)
    try:
        c.reset_stats()
        rc = call()
        msg = c._lib.zvx_last_error(c._h).decode()
        c.sync()
        launches = sum(t["launches"] for t in c.tag_stats())
    finally:
        c.set_int("profile", 0)
    assert rc == _lib.ZVX_E_INVALID, (rc, msg)
    assert msg.startswith(name + ":"), msg
    assert rule in msg, msg
    for o, k in zip(outputs, before):
        assert np.array_equal(bits(o), bits(k)), msg
    assert launches == 0, (msg, launches)


def test_refusals(dev):
    c = ctx()
    dim, K, B = 8, 40, 2
    q, lib = inputs(dim)
    q, lib = q[:B], lib[:K]
    lib_ptr = dev.put(lib)
    s = np.full((B, K), SENTINEL, np.uint32).view(np.float32)
    ts, ti = np.full((B, 5), SENTINEL, np.uint32).view(np.float32), np.full((B, 5), SENTINEL, np.uint32).view(np.int32)
    L = c._lib

    def score(qa=q, Bv=B, lp=lib_ptr, Kv=K, dv=dim, out=s, flags=0):
        return lambda: L.zvx_spk_score(c._h, vp(qa), Bv, vp(lp), Kv, dv, vp(out), flags)

    def topk(qa=q, Bv=B, lp=lib_ptr, Kv=K, dv=dim, top=5, out=ts, idx=ti, flags=0):
        return lambda: L.zvx_spk_topk(c._h, vp(qa), Bv, vp(lp), Kv, dv, top, vp(out), vp(idx), flags)
    keep = [s, ts, ti]
    for fn, call in (("zvx_spk_score", score), ("zvx_spk_topk", topk)):
        refused(c, call(qa=None), keep, fn, "query is NULL")
        refused(c, call(lp=None), keep, fn, "lib is NULL")
        refused(c, call(out=None), keep, fn, "score is NULL")
        refused(c, call(Bv=0), keep, fn, "B = 0")
        refused(c, call(Bv=-1), keep, fn, "B = -1")
        refused(c, call(Kv=0), keep, fn, "K = 0")
        refused(c, call(Kv=-5), keep, fn, "K = -5")
        for bad in (0, 2, 6, 2052, -4):
            refused(c, call(dv=bad), keep, fn, f"dim {bad}")
        refused(c, call(flags=1 << 20), keep, fn, "unknown flag")
        refused(c, call(flags=NOSYNC), keep, fn, "ZVX_NO_SYNC needs ZVX_DEVICE_OUT")
    refused(c, topk(idx=None), keep, "zvx_spk_topk", "index is NULL")
    for bad in (0, -1, 33, K + 1):
        refused(c, topk(top=bad, Kv=K if bad != K + 1 else 20), keep, "zvx_spk_topk", "top")
    refused(c, topk(top=21, Kv=20), keep, "zvx_spk_topk", "top")
    # the context is still usable
    assert score()() == 0 and topk()() == 0
    ref = V.scores(q, lib)
    assert np.max(np.abs(s.astype(np.float64) - ref)) <= V.tol(dim)
    ws, wi = V.topk(s, 5)
    assert np.array_equal(ti, wi) and np.array_equal(bits(ts), bits(ws))


def test_launches_carry_the_tag(dev):
    c = ctx()
    q, lib = inputs(8)
    lib_ptr = dev.put(lib)
    c.set_int("profile", 2)
    try:
        c.reset_stats()
        c.spk_topk(q[:3], lib_ptr, 1000, 5, 8)
        c.spk_score(q[:3], lib_ptr, 1000, 8)
        c.sync()
        tags = {t["name"]: t["launches"] for t in c.tag_stats() if t["launches"]}
    finally:
        c.set_int("profile", 0)
    assert tags == {"spk.match": 2}, tags


# ---- 5. VoiceLibrary on the device --------------------------------------------------------------------------------------------
def test_voice_library_on_the_device(tmp_path):
    c = ctx()
    clips = E.make_clips(0)
    names = [f"voice{i}" for i in range(len(clips))]
    emb, begin, end, frames = c.spkemb_wav(clips)
    lib = voices.VoiceLibrary(c, capacity=2)                 # grows twice under the two enrolments
    try:
        rows, b2, e2, f2 = lib.enroll(names[:2], clips[:2])
        rows += lib.enroll(names[2:], clips[2:])[0]
        assert rows == list(range(len(clips))) and lib.names == names and lib.capacity >= len(clips)
        assert np.array_equal(b2, begin[:2]) and np.array_equal(e2, end[:2]) and np.array_equal(f2, frames[:2])
        solo = np.concatenate([c.spkemb_wav(clips[:2])[0], c.spkemb_wav(clips[2:])[0]])
        assert np.array_equal(bits(lib.embeddings()), bits(solo))            # the bits spkemb_wav returns for the same batches
        tol = V.tol(c.hidden)
        got = lib.match(solo, top=2)
        for i, m in enumerate(got):
            assert m[0].name == names[i] and m[0].index == i and abs(m[0].score - 1.0) <= tol, (i, m)
        assert [h[0].name for h in lib.screen(solo, 1.0 - 2 * tol)] == names
        lib.remove(names[1])
        assert lib.names == [names[0], names[4], names[2], names[3]]
        assert np.array_equal(bits(lib.embeddings()), bits(solo[[0, 4, 2, 3]]))
        again = lib.match(solo[1], top=len(lib))
        assert names[1] not in [m.name for m in again[0]] and len(again[0]) == 4
        path = str(tmp_path / "voices.npz")
        lib.save(path)
        back = voices.VoiceLibrary.load(c, path)
        try:
            assert back.names == lib.names and np.array_equal(bits(back.embeddings()), bits(lib.embeddings()))
            assert [m[0].name for m in back.match(solo[[4, 0]], top=1)] == [names[4], names[0]]
        finally:
            back.close()
    finally:
        lib.close()


# ---- 6. the voice report ------------------------------------------------------------------------------------------------------
def cosine64(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(a @ b / max(np.sqrt(a @ a) * np.sqrt(b @ b), V.FLT_MIN))


def test_voice_report():
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    c = synth.model.ctx
    tol = V.tol(c.hidden)
    clip = E.make_clips(0)[0]
    spk = np.random.default_rng(5).standard_normal((1, 1, c.hidden)).astype(np.float32)
    assert synth.last_voice_report is None
    emb, begin, end, frames = c.spkemb_wav([clip])
    rep = synth.voice_report(clip, spk, sampling_rate=c.get_int("sampling_rate"))
    assert isinstance(rep, voices.VoiceReport) and synth.last_voice_report is rep
    assert (rep.begin, rep.end, rep.frames) == (int(begin[0]), int(end[0]), int(frames[0]))
    assert abs(rep.similarity - cosine64(emb[0], spk)) <= tol, (rep.similarity, cosine64(emb[0], spk))
    same = synth.voice_report(clip, emb, sampling_rate=c.get_int("sampling_rate"))
    assert abs(same.similarity - 1.0) <= tol and same.meets(1.0 - tol) and not same.meets(1.0 + 2 * tol)
    pcm = np.round(clip * 32760.0).astype(np.int16)          # int16 PCM is read as the samples it encodes
    as_float = synth.voice_report(pcm.astype(np.float32) / np.float32(32760.0), spk, sampling_rate=c.get_int("sampling_rate"))
    last = synth.voice_report(pcm, spk, sampling_rate=c.get_int("sampling_rate"))
    assert last == as_float
    print(f"voice report of a reference clip against a random embedding: {rep}; against its own: {same}")
    text = "the quick brown fox jumps over the lazy dog"
    before = synth.tts(text, spk)[0]
    assert synth.last_voice_report is last                   # without the keyword it keeps its value
    wav, _, length = synth.tts(text, spk, voice_report=True)
    got = synth.last_voice_report
    assert np.array_equal(wav.view(np.uint32), before.view(np.uint32))
    assert isinstance(got, voices.VoiceReport) and got is not last and got == synth.voice_report(wav, spk)
    w_emb = c.spkemb_wav([wav], rate=synth.output_rate, max_samples=30 * c.get_int("sampling_rate"))[0]
    assert abs(got.similarity - cosine64(w_emb[0], spk)) <= tol
    synth.tts(text, spk)
    assert synth.last_voice_report == got
    synth.tts("", spk, voice_report=True)                    # asked for, nothing to measure
    assert synth.last_voice_report is None
    plain, _ = synth.tts_long(text + ". Pack my box with five dozen liquor jugs.", spk)
    joined, seg = synth.tts_long(text + ". Pack my box with five dozen liquor jugs.", spk, voice_report=dict(top_db=30.0))
    assert np.array_equal(joined.view(np.uint32), plain.view(np.uint32)) and isinstance(synth.last_voice_report, voices.VoiceReport)
    assert synth.last_voice_report == synth.voice_report(joined, spk, top_db=30.0)
