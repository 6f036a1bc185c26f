"""Alignment on the MI355X: zvx_dtw against tests/align_ref.py (the float64 restatement of include/zvx.h's block; never the library) at the
smallest shapes that exercise the kernel's cuts -- single cells and single rows, the wave edge (63 .. 65 rows), 255 .. 257 rows and dim at
its limit (32), a band of 1024 rows and a second one (1025), a ragged batch
inside a larger padding that holds NaN, and one pair at the size limit --, ties, the independence of pairs, device input, every refusal,
zvx_align_wav against zvx_melspec, the float64 DCT and zvx_dtw, and tts(rhythm_from=...) on the tiny synthetic model.  tests/test_align.py asserts on the CPU, from the reference
alone, that none of the seeded cases holds an ambiguous decision on its path: the path comparison here leaves no case out."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import align_ref as R
import pitch_ref as PR
from stream_util import err, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

SENT_I, SENT_D = np.int32(-777), -12345.0
_ctx, _ref = {}, {}


def ctx_for(voc="tiny", prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def ref_of(Ta, Tb, dim):
    """the seeded pair and its reference, computed once, left unchanged"""
    key = (Ta, Tb, dim)
    if key not in _ref:
        a, b = R.case(Ta, Tb, dim)
        for x in (a, b):
            x.setflags(write=False)
        _ref[key] = (a, b, R.dtw(a, b))
    return _ref[key]


def padded(rows, Tmax, fill=np.nan):
    dim = rows[0].shape[1]
    x = np.full((len(rows), Tmax, dim), fill, np.float32)
    for p, r in enumerate(rows):
        x[p, :len(r)] = r
    return x


def raw(ctx, a, Ta, Tamax, b, Tb, Tbmax, B, dim, flags=0, want_path=True, want_a2b=True, stride=None, prm=None, cost=True, plen=True):
    """zvx_dtw straight through ctypes with sentinel-filled outputs -> (rc, cost, path_len, path, a2b)"""
    Ta_, Tb_ = (None if Ta is None else np.ascontiguousarray(Ta, np.int32)), (None if Tb is None else np.ascontiguousarray(Tb, np.int32))
    nb = max(B, 1)
    if stride is None:
        stride = int(max(np.asarray(Ta_, np.int64) + Tb_)) - 1 + 3
    co, pl = np.full(nb, SENT_D, np.float64), np.full(nb, SENT_I, np.int32)
    path = np.full((nb, max(stride, 1), 2), SENT_I, np.int32)
    a2b = np.full((nb, max(Tamax, 1), 2), SENT_I, np.int32)
    rc = ctx._lib.zvx_dtw(ctx._h, vp(a), vp(Ta_), Tamax, vp(b), vp(Tb_), Tbmax, B, dim, prm, vp(co) if cost else None, vp(pl) if plen else None,
                          vp(path) if want_path else None, stride, vp(a2b) if want_a2b else None, flags)
    return rc, co, pl, path, a2b


def check_pair(what, Ta, Tb, dim, ref, cost, plen, path, a2b):
    """the cost within the derived bound, the path cell for cell the reference's, a2b consistent with it, nothing written past either"""
    assert ref["ambiguous"] == [], what                      # from the reference alone (also asserted on the CPU)
    L = len(ref["path"])
    dev = abs(cost - ref["cost"]) / ref["cost"] if ref["cost"] else abs(cost)
    print(f"{what}: cost {cost!r} ref {ref['cost']!r} relative deviation {dev:.3e} (bound {2.0 * (Ta + Tb + dim) * 2.0 ** -53:.3e}), path {plen} cells")
    assert abs(cost - ref["cost"]) <= R.cost_bound(Ta, Tb, dim, ref["cost"]), (what, cost, ref["cost"])
    assert plen == L, (what, plen, L)
    assert np.array_equal(path[:L], ref["path"]), (what, np.flatnonzero((path[:L] != ref["path"]).any(axis=1))[:5])
    assert np.all(path[L:] == SENT_I), what
    assert np.array_equal(a2b[:Ta], R.a2b_of(path[:L], Ta)) and np.array_equal(a2b[:Ta], ref["a2b"]), what
    assert np.all(a2b[Ta:] == SENT_I), what
    return dev


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("Ta, Tb, dim", R.SHAPES)
def test_single_pairs(Ta, Tb, dim):
    ctx = ctx_for()
    a, b, ref = ref_of(Ta, Tb, dim)
    rc, co, pl, path, a2b = raw(ctx, a, [Ta], Ta, b, [Tb], Tb, 1, dim)
    assert rc == 0, err(ctx)
    check_pair(f"{Ta} x {Tb} x {dim}", Ta, Tb, dim, ref, co[0], pl[0], path[0], a2b[0])
    res = ctx.dtw([a], [b])                                  # the binding gives the same
    assert res["cost"][0] == co[0] and np.array_equal(res["path"][0], ref["path"]) and np.array_equal(res["a2b"][0], ref["a2b"])
    assert "path" not in ctx.dtw([a], [b], path=False)


def ragged():
    cases = [ref_of(*s) for s in R.RAGGED]
    Ta, Tb = [len(c[0]) for c in cases], [len(c[1]) for c in cases]
    Tamax, Tbmax = max(Ta) + 9, max(Tb) + 21
    return cases, Ta, Tb, Tamax, Tbmax, padded([c[0] for c in cases], Tamax), padded([c[1] for c in cases], Tbmax)


def test_ragged_batch_with_nan_in_the_padding_and_independence():
    ctx = ctx_for()
    cases, Ta, Tb, Tamax, Tbmax, xa, xb = ragged()
    dim = xa.shape[2]
    rc, co, pl, path, a2b = raw(ctx, xa, Ta, Tamax, xb, Tb, Tbmax, len(cases), dim)
    assert rc == 0, err(ctx)
    for p, (a, b, ref) in enumerate(cases):
        check_pair(f"ragged pair {p}", Ta[p], Tb[p], dim, ref, co[p], pl[p], path[p], a2b[p])
        rc1, co1, pl1, path1, a2b1 = raw(ctx, a, [Ta[p]], Ta[p], b, [Tb[p]], Tb[p], 1, dim)      # alone: the same bits
        assert rc1 == 0 and co1.view(np.uint64)[0] == co.view(np.uint64)[p] and pl1[0] == pl[p]
        assert np.array_equal(path1[0, :pl[p]], path[p, :pl[p]]) and np.array_equal(a2b1[0, :Ta[p]], a2b[p, :Ta[p]])
    # a pair with NaN among its own rows: the call succeeds, the others keep their bits, its path is still a monotone path
    bad = xa.copy()
    bad[1, 7, 3] = np.nan
    rc2, co2, pl2, path2, _ = raw(ctx, bad, Ta, Tamax, xb, Tb, Tbmax, len(cases), dim)
    assert rc2 == 0, err(ctx)
    for p in (0, 2):
        assert co2.view(np.uint64)[p] == co.view(np.uint64)[p] and np.array_equal(path2[p], path[p])
    assert 1 <= pl2[1] <= Ta[1] + Tb[1] - 1 and R.valid_path(path2[1, :pl2[1]], Ta[1], Tb[1])


def test_the_size_limit_once():
    ctx = ctx_for()
    Ta, Tb, dim = R.BIG
    a, b = R.case(Ta, Tb, dim)
    ref = R.dtw(a, b)
    rc, co, pl, path, a2b = raw(ctx, a, [Ta], Ta, b, [Tb], Tb, 1, dim)
    assert rc == 0, err(ctx)
    check_pair("4096 x 4096 x 13", Ta, Tb, dim, ref, co[0], pl[0], path[0], a2b[0])


# ------------------------------------------------------------------------------------------------ 2. ties
def test_a_sequence_against_itself_is_the_diagonal_at_cost_zero():
    ctx = ctx_for()
    a, _ = R.case(300, 1, 13, seed=3)                        # distinct frames
    res = ctx.dtw([a], [a])
    assert res["cost"][0] == 0.0 and res["path_len"][0] == 300
    assert np.array_equal(res["path"][0], np.stack([np.arange(300)] * 2, axis=1)) and np.array_equal(res["a2b"][0], res["path"][0])


def test_integer_features_exact_ties_and_the_square_root():
    ctx = ctx_for()
    a, b = R.integer_case()
    ref = R.dtw(a, b)
    assert ref["ambiguous"] and ref["cost"] == round(ref["cost"])
    res = ctx.dtw([a], [b])
    path = res["path"][0]
    assert R.valid_path(path, len(a), len(b)) and len(path) == res["path_len"][0]
    assert res["cost"][0] == ref["cost"]                     # small integers: every sum is exact, so d must be the exact integer
    assert R.path_cost(a, b, path) == ref["cost"]
    assert np.array_equal(res["a2b"][0], R.a2b_of(path, len(a)))
    # d on perfect squares, one cell each: sqrt((x - 0)^2) = x for integers up to 2^24, and 3-4-5 / 8-15-17 triangles at dim 2
    xs = np.array([1, 2, 3, 5, 7, 255, 4097, 65535, 1 << 20, (1 << 24) - 1], np.float32)
    one = ctx.dtw([np.array([[x]], np.float32) for x in xs], [np.zeros((1, 1), np.float32)] * len(xs))
    assert np.array_equal(one["cost"], xs.astype(np.float64))
    tri = ctx.dtw([np.array([[3, 4]], np.float32), np.array([[8, 15]], np.float32)], [np.zeros((1, 2), np.float32)] * 2)
    assert tri["cost"].tolist() == [5.0, 17.0]


# ------------------------------------------------------------------------------------------------ 3. device input
def test_device_input_gives_the_same_bits():
    ctx = ctx_for()
    cases, Ta, Tb, Tamax, Tbmax, xa, xb = ragged()
    host = ctx.dtw(xa, xb, lengths_a=Ta, lengths_b=Tb)
    buf = ctx.dev_alloc(xa.nbytes + xb.nbytes + 512)
    try:
        pb = buf + ((xa.nbytes + 255) & ~255)
        ctx.dev_from_host(buf, xa)
        ctx.dev_from_host(pb, xb)
        dev = ctx.dtw_device(buf, Ta, Tamax, pb, Tb, Tbmax, xa.shape[2])
    finally:
        ctx.dev_free(buf)
    assert np.array_equal(dev["cost"].view(np.uint64), host["cost"].view(np.uint64)) and np.array_equal(dev["path_len"], host["path_len"])
    for p in range(len(cases)):
        assert np.array_equal(dev["path"][p], host["path"][p]) and np.array_equal(dev["a2b"][p], host["a2b"][p])


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_outputs_and_the_context_alone():
    ctx = ctx_for()
    a, b, ref = ref_of(5, 1, 3)
    INV, UNS = _lib.ZVX_E_INVALID, _lib.ZVX_E_UNSUPPORTED
    ok = dict(a=a, Ta=[5], Tamax=5, b=b, Tb=[1], Tbmax=1, B=1, dim=3)

    def refused(code, word, **kw):
        args = dict(ok, **kw)
        extra = {k: args.pop(k) for k in ("flags", "stride", "prm", "cost", "plen") if k in args}
        rc, co, pl, path, a2b = raw(ctx, **args, **extra)
        msg = err(ctx).decode() if isinstance(err(ctx), bytes) else str(err(ctx))
        assert rc == code, (kw.keys(), rc, msg)
        assert word in msg, (word, msg)
        assert np.all(co == SENT_D) and np.all(pl == SENT_I) and np.all(path == SENT_I) and np.all(a2b == SENT_I), kw.keys()

    assert ctx._lib.zvx_dtw(None, vp(a), vp(np.array([5], np.int32)), 5, vp(b), vp(np.array([1], np.int32)), 1, 1, 3, None, None, None, None, 0, None,
                            0) == INV
    refused(INV, "NULL", a=None)
    refused(INV, "NULL", b=None)
    refused(INV, "NULL", Ta=None, stride=8)
    refused(INV, "NULL", Tb=None, stride=8)
    refused(INV, "NULL", cost=False)
    refused(INV, "NULL", plen=False)
    refused(INV, "B = 0", B=0)
    refused(INV, "B = -1", B=-1)
    refused(INV, "dim = 0", dim=0)
    refused(INV, "pair 0", Ta=[0])
    refused(INV, "pair 0", Ta=[6])
    refused(INV, "pair 0", Tb=[0])
    refused(INV, "pair 0", Tb=[2])
    refused(INV, "path_stride", stride=4)                    # 5 + 1 - 1 cells are possible
    refused(INV, "flag", flags=_lib.ZVX_DEVICE_OUT)
    refused(INV, "flag", flags=_lib.ZVX_DEVICE_IN | _lib.ZVX_NO_SYNC)
    prm = _lib.DtwParams()
    prm.reserved[2] = 1
    refused(INV, "reserved", prm=C.byref(prm))
    # the second pair of a batch is named
    two_a, two_b = np.zeros((2, 5, 3), np.float32), np.zeros((2, 4, 3), np.float32)
    refused(INV, "pair 1", a=two_a, b=two_b, Ta=[5, 6], Tb=[4, 4], Tbmax=4, B=2)
    # ZVX_E_UNSUPPORTED
    refused(UNS, "dim = 33", a=np.zeros((1, 5, 33), np.float32), b=np.zeros((1, 1, 33), np.float32), dim=33)
    refused(UNS, "pair 0", a=np.zeros((1, 4097, 1), np.float32), Ta=[4097], Tamax=4097, b=np.zeros((1, 1, 1), np.float32), dim=1)
    refused(UNS, "pair 0", a=np.zeros((1, 1, 1), np.float32), Ta=[1], Tamax=1, b=np.zeros((1, 4097, 1), np.float32), Tb=[4097], Tbmax=4097, dim=1)
    many = 65536
    refused(UNS, "65535", a=np.zeros((many, 1, 1), np.float32), Ta=np.ones(many, np.int32), Tamax=1, b=np.zeros((many, 1, 1), np.float32),
            Tb=np.ones(many, np.int32), Tbmax=1, B=many, dim=1)
    refused(UNS, "2^30", a=np.zeros((65, 4096, 1), np.float32), Ta=np.full(65, 4096, np.int32), Tamax=4096, b=np.zeros((65, 4096, 1), np.float32),
            Tb=np.full(65, 4096, np.int32), Tbmax=4096, B=65, dim=1)
    # zero reserved fields are accepted, and the context is usable
    rc, co, pl, path, a2b = raw(ctx, prm=C.byref(_lib.DtwParams()), **ok)
    assert rc == 0, err(ctx)
    check_pair("after the refusals", 5, 1, 3, ref, co[0], pl[0], path[0], a2b[0])


def test_accounting():
    ctx = ctx_for()
    cases, Ta, Tb, Tamax, Tbmax, xa, xb = ragged()
    dim = xa.shape[2]
    want = float(sum((ta + tb) * dim * 4 + ta * tb for ta, tb in zip(Ta, Tb)))
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.dtw(xa, xb, lengths_a=Ta, lengths_b=Tb)
        tags = {t["name"]: t for t in ctx.tag_stats() if t["launches"]}
        assert set(tags) == {"post.align", "post.align.forward", "post.align.backtrack"}, sorted(tags)
        assert tags["post.align"]["launches"] == 1 and tags["post.align"]["bytes"] == want and tags["post.align"]["ms"] > 0
        print(f"post.align on the ragged batch: {tags['post.align']['ms']:.3f} ms (forward {tags['post.align.forward']['ms']:.3f}, backtrack "
              f"{tags['post.align.backtrack']['ms']:.3f})")
    finally:
        ctx.set_int("profile", 0)


# ------------------------------------------------------------------------------------------------ 5. zvx_align_wav
def test_align_wav_is_melspec_the_dct_and_dtw():
    ctx = ctx_for()
    fs = ctx.get_int("sampling_rate")
    n0 = int(0.4 * fs)
    # a glide and a time-stretched copy of it (the same trajectory over 1.5 times the samples), and the other way round
    g0, g1 = PR.glide(100.0, 200.0, n0, fs)[0] * 0.3, PR.glide(100.0, 200.0, n0 * 3 // 2, fs)[0] * 0.3
    rows_a, rows_b = [g0, g1], [g1, g0]
    res = ctx.align(rows_a, rows_b, n_cep=13, cepstra=True)
    mel_a, fr_a = ctx.melspec(rows_a)
    mel_b, fr_b = ctx.melspec(rows_b)
    assert np.array_equal(res["frames_a"], fr_a) and np.array_equal(res["frames_b"], fr_b) and fr_a.min() >= 30
    worst = 0.0
    for side, mel, fr in (("cep_a", mel_a, fr_a), ("cep_b", mel_b, fr_b)):
        for p in range(2):
            got = res[side][p]
            want = R.cepstra(mel[p, :fr[p]], 13)             # the float64 DCT of zvx_melspec's own log-mel of that row
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert got.shape == want.shape
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / ulp)))
    print(f"cepstra: worst deviation from the float64 DCT {worst:.3f} f32 ulp")
    assert worst <= 1.0
    again = ctx.dtw(res["cep_a"], res["cep_b"])              # zvx_dtw on the returned cepstra: the same bits
    assert np.array_equal(again["cost"].view(np.uint64), res["cost"].view(np.uint64)) and np.array_equal(again["path_len"], res["path_len"])
    for p in range(2):
        assert np.array_equal(again["path"][p], res["path"][p]) and np.array_equal(again["a2b"][p], res["a2b"][p])
        assert res["mcd_db"][p] == R.mcd_db(res["cost"][p], res["path_len"][p])
        assert R.valid_path(res["path"][p], fr_a[p], fr_b[p])
    # the log-mel chain inside is zvx_melspec's: n_cep = n_mels - 1 cepstra of a row are the DCT of exactly that log-mel
    full = ctx.align([g0], [g1], n_cep=min(32, ctx.n_mels - 1), cepstra=True)
    want = R.cepstra(mel_a[0, :fr_a[0]], min(32, ctx.n_mels - 1))
    assert np.all(np.abs(full["cep_a"][0].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
    # a signal against itself: distortion 0 along the diagonal
    same = ctx.align([g1], [g1])
    F = int(same["frames_a"][0])
    assert same["mcd_db"][0] == 0.0 and same["cost"][0] == 0.0 and np.array_equal(same["path"][0], np.stack([np.arange(F)] * 2, axis=1))
    # refusals name the side and the row, and n_cep has its range
    for kw, word in ((dict(rows_a=[g0, g0[:10]], rows_b=rows_b), "side a, row 1"), (dict(rows_a=rows_a, rows_b=[g0[:10], g0]), "side b, row 0")):
        with pytest.raises(_lib.ZvxError, match=word):
            ctx.align(**kw)
    for bad in (0, 33, ctx.n_mels):
        with pytest.raises(_lib.ZvxError, match="n_cep"):
            ctx.align(rows_a, rows_b, n_cep=bad)
    assert ctx.align([g1], [g1])["mcd_db"][0] == 0.0


# ------------------------------------------------------------------------------------------------ 6. through the model
def test_rhythm_copy_through_the_model():
    from zerovox_amd.align import Alignment
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    ctx, hop = synth.model.ctx, synth.model.ctx.hop
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    text = "The quick brown fox jumps over the lazy dog"
    assert synth.last_alignment is None
    before, phoneme, length = synth.tts(text, spk)           # the plain call, before any rhythm_from call in the process
    assert synth.last_alignment is None
    first = np.rint(ctx.fetch("duration", (1, phoneme.shape[1]))[0]).astype(np.int32)
    assert first.sum() == length and len(before) == length * hop
    w = synth.tts_ex(text, spk, duration=[int(v) for v in 2 * first])[0]     # the same text at half the speed
    assert len(w) == 2 * length * hop
    begin, end = ctx.trim_bounds([w], top_db=40.0)
    clip = w[int(begin[0]):int(end[0])]
    frames_b = int(ctx.melspec([clip])[1][0])                # the mel frames of the trimmed clip: asserted, not assumed
    print(f"first pass {length} frames, recording {2 * length} frames, trimmed to samples [{int(begin[0])}, {int(end[0])}): {frames_b} frames")
    assert frames_b >= length
    wav, ph2, len2 = synth.tts(text, spk, rhythm_from=w)
    al = synth.last_alignment
    assert isinstance(al, Alignment) and al.frames_a == length and al.frames_b == frames_b
    assert len2 == frames_b and len(wav) == frames_b * hop and np.array_equal(ph2, phoneme)
    assert R.valid_path(al.path, al.frames_a, al.frames_b) and np.array_equal(al.a2b, R.a2b_of(al.path, al.frames_a))
    second = np.rint(ctx.fetch("duration", (1, phoneme.shape[1]))[0]).astype(np.int32)
    assert second.sum() == frames_b and np.all(second[first == 0] == 0) and np.all(second[first > 0] >= 1)
    # fidelity_report: the delivered waveform against the recording, and against itself
    rep = synth.fidelity_report(wav, w)
    assert synth.last_alignment is rep and rep.frames_b == frames_b and rep.frames_a == frames_b and np.isfinite(rep.mcd_db) and rep.mcd_db >= 0.0
    print(f"rhythm copy against the recording: {rep.mcd_db:.3f} dB over {len(rep.path)} cells; first pass against it: {al.mcd_db:.3f} dB")
    assert rep.meets(rep.mcd_db) and not rep.meets(rep.mcd_db - 1e-6) if rep.mcd_db > 0 else rep.meets(0.0)
    # the plain call keeps its bits
    after = synth.tts(text, spk)[0]
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    with pytest.raises(ValueError, match="rhythm_from"):
        synth.tts(text, spk, rhythm_from=w, speed=1.1)
