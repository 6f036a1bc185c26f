"""Host-side checks of the float64 kernel reference (tests/kernel_ref.py) that tests/test_kernels_gpu.py holds the kernels to:
  * the ctypes mirror of GemmArgs / FlashArgs / AttnF32Args has the compiled layout (read from the shim without opening a device);
  * gemm_ref / attn_ref agree with an independent formulation (torch.nn.functional on the CPU) for each row-map kind;
  * the references discriminate: every mutation of the reference (a dropped or shifted tap, a lost K chunk, an off-by-one length,
    the wrong residual slope, a dropped bias, a skipped accumulator add) leaves the bound of every case it applies to;
  * the chained reference of the streaming ResBlock kernels (chain_ref): equal to torch's HiFi-GAN ResBlock1 / stage with the
    roundings off, at least 30 % of every exact-sum case held to bit equality, and every mutation of it outside the bound (the
    dense cases' rms criterion rejects two swapped taps)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as K


def _needs_lib():
    if not os.path.exists(K.KTEST_LIB):
        pytest.fail(f"{K.KTEST_LIB} is missing: run zerovox_amd.build first")


def test_struct_layout():
    """Every field of the three argument structs sits where the compiled shim says, and the sizes agree."""
    _needs_lib()
    lib = K.load_ktest()
    seen = set()
    for i in range(lib.zvxk_num_fields()):
        st, name = lib.zvxk_field(i, 0).decode(), lib.zvxk_field(i, 1).decode()
        cls = K.STRUCTS[st]
        assert getattr(cls, name).offset == lib.zvxk_offsetof(st.encode(), name.encode()), (st, name)
        seen.add((st, name))
    for st, cls in K.STRUCTS.items():
        assert ctypes.sizeof(cls) == lib.zvxk_sizeof(st.encode()), st
        for f, _t in cls._fields_:
            assert (st, f) in seen, f"{st}.{f} is mirrored in Python but not reported by the shim"


def _ref_out(p):
    r, t, m = K.gemm_ref(p)["out"]
    return r, m


def test_ref_conv1d_dilated_vs_torch():
    """1-D taps with dilation, ragged lengths (zero padding past in_len): F.conv1d per utterance."""
    p = K.make_gemm("t", 1, dtype=K.DT_F32, M=50, N=24, K=16, nbatch=2, lens=[50, 9], taps=K.taps_1d(5, 3), packed=False, bias_mode=0)
    r, m = _ref_out(p)
    d = p.d
    X = p.bufs["X"]["v"].reshape(2, -1, d["ldx"])
    W = p.bufs["W"]["v"].reshape(5, d["N"], d["ldw"])
    w = torch.tensor(W[:, :, :16]).permute(1, 2, 0)                 # [N][K][tap]
    for b, l in enumerate([50, 9]):
        x = torch.tensor(np.nan_to_num(X[b, :l, :16])).T[None]
        y = F.conv1d(x, w, padding=6, dilation=3)[0].T.numpy()
        got = r[b * d["o_bs"]:b * d["o_bs"] + l * d["ldo"]].reshape(l, d["ldo"])[:, :24]
        np.testing.assert_allclose(got, y, rtol=1e-12, atol=1e-12)


def test_ref_conv_transpose_polyphase_vs_torch():
    """Polyphase ConvTranspose1d (stride 4, kernel 8, padding 2) as one 1-tap-per-weight-column launch per output phase."""
    rng = np.random.default_rng(3)
    Cin, Cout, k, s, pad, L = 16, 8, 8, 4, 2, 12
    x = rng.standard_normal((Cin, L))
    w = rng.standard_normal((Cin, Cout, k))
    y = F.conv_transpose1d(torch.tensor(x)[None], torch.tensor(w), stride=s, padding=pad)[0].numpy()   # [Cout][(L-1)s - 2p + k]
    Lout = y.shape[1]
    for ph in range(s):
        r0, q = (ph + pad) % s, (ph + pad) // s
        ms = list(range(r0, k, s))
        taps = [q - j for j in range(len(ms))]
        T = (Lout - ph + s - 1) // s
        p = K.make_gemm("ct", 0, dtype=K.DT_F32, M=T, N=Cout, K=Cin, lens=[L], out_lens=[T], taps=taps, packed=False, bias_mode=0)
        Xv = np.full(len(p.bufs["X"]["v"]), np.nan)
        Xv[:L * Cin] = x.T.reshape(-1)
        p.bufs["X"]["v"] = Xv
        p.bufs["W"]["v"] = np.stack([w[:, :, m].T for m in ms]).reshape(-1)
        r, msk = _ref_out(p)
        got = r[:T * Cout].reshape(T, Cout)
        np.testing.assert_allclose(got, y[:, ph::s].T, rtol=1e-12, atol=1e-12)


def test_ref_conv2d_stride2_and_flat_vs_torch():
    """2-D taps with stride 2 (ResNet level transition) and the flattened stride-1 map: F.conv2d with padding 1."""
    for stride, flat in ((2, False), (1, True)):
        hin, win, C, N, lens = 6, 11, 8, 16, [10, 3]
        wout = (win - 1) // stride + 1
        hout = (hin - 1) // stride + 1
        p = K.make_gemm("c2", 2, dtype=K.DT_F32, M=hout * wout, N=N, K=C, nbatch=2, lens=lens, taps=[t % 3 - 1 for t in range(9)],
                        du=[t // 3 - 1 for t in range(9)], stride=stride, wout=wout, hin=hin, win=win, flat=flat, packed=False, bias_mode=0)
        r, m = _ref_out(p)
        d = p.d
        X = p.bufs["X"]["v"].reshape(2, hin, win, C)
        W = p.bufs["W"]["v"].reshape(9, N, C)
        w = torch.tensor(W.reshape(3, 3, N, C)).permute(2, 3, 0, 1)
        for b, l in enumerate(lens):
            x = torch.tensor(np.nan_to_num(X[b, :, :l])).permute(2, 0, 1)[None]
            y = F.conv2d(x, w, padding=1, stride=stride)[0].permute(1, 2, 0).numpy()       # [hout][wo][N]
            got = r[b * d["o_bs"]:b * d["o_bs"] + hout * wout * d["ldo"]].reshape(hout, wout, d["ldo"])[:, :, :N]
            wv = (l + stride - 1) // stride
            np.testing.assert_allclose(got[:, :wv], y[:, :wv], rtol=1e-12, atol=1e-12)


def test_ref_linear_heads_klen_vs_torch():
    """Batched product with per-utterance k_len (attention P.V): F.linear over the first k_len columns."""
    p = K.make_gemm("pv", 4, dtype=K.DT_F32, M=20, N=12, K=24, nbatch=3, lens=[20, 1, 13], k_len=[20, 1, 13], packed=False, bias_mode=0, alpha=0.5)
    r, m = _ref_out(p)
    d = p.d
    X = p.bufs["X"]["v"].reshape(3, -1, d["ldx"])
    W = p.bufs["W"]["v"].reshape(3, d["N"], d["ldw"])
    for b, l in enumerate([20, 1, 13]):
        y = 0.5 * F.linear(torch.tensor(X[b, :l, :l]), torch.tensor(W[b, :, :l])).numpy()
        got = r[b * d["o_bs"]:b * d["o_bs"] + l * d["ldo"]].reshape(l, d["ldo"])[:, :12]
        np.testing.assert_allclose(got, y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("flash", [True, False])
def test_attn_ref_vs_torch(flash):
    """Masked softmax attention (keys < len, 1 / sqrt(D)) per utterance and head: torch softmax in float64."""
    p = K.make_attn("a", 5, flash=flash, B=2, nheads=2, lens=[9, 1])
    r, t, m = K.attn_ref(p)["out"]
    d = p.d
    D = 264
    for b, l in enumerate([9, 1]):
        for h in range(2):
            if flash:
                QK = p.bufs["qk"]["v"].reshape(2, d["L"], d["ldq"])
                Q, Kt = QK[b, :l, h * D:(h + 1) * D], QK[b, :l, d["k_off"] + h * D:d["k_off"] + (h + 1) * D]
                V = p.bufs["vt"]["v"].reshape(2, -1, d["ldv"])[b, h * D:(h + 1) * D, :l].T
            else:
                A = p.bufs["qkv"]["v"].reshape(2, d["L"], d["ld"])
                Q, Kt, V = (A[b, :l, o + h * D:o + (h + 1) * D] for o in (d["q_off"], d["k_off"], d["v_off"]))
            s = torch.tensor(Q) @ torch.tensor(Kt).T * d["scale"]          # (1 / sqrt(D) as the f32 the launcher gets)
            y = (torch.softmax(s, dim=1) @ torch.tensor(V)).numpy()
            got = r[b * d["o_bs"]:b * d["o_bs"] + l * d["ldo"]].reshape(l, d["ldo"])[:, h * D:(h + 1) * D]
            np.testing.assert_allclose(got, y, rtol=1e-10, atol=1e-12)


def _exceeds(ref, tol, mask, mut):
    diff = np.abs(mut[mask] - ref[mask])
    return bool(np.any(~(diff <= tol[mask])))


@pytest.mark.parametrize("entry", K.GEMM_CASES, ids=[e[0] for e in K.GEMM_CASES])
def test_mutations_leave_bound(entry):
    """Each applicable mutation of the reference exceeds the case's own bound on the case's own data somewhere: a kernel wrong in
    that way would fail test_kernels_gpu."""
    p = K.build_case(entry)
    true = K.gemm_ref(p)
    weak = []
    for mut in K.applicable_mutations(p):
        got = K.gemm_ref(p, mut)
        if not any(_exceeds(true[f][0], true[f][1], true[f][2], got[f][0]) for f in true if true[f][2].any()):
            weak.append(mut)
    assert not weak, f"{entry[0]}: mutations within the bound: {weak}"


@pytest.mark.parametrize("entry", K.ATTN_CASES, ids=[e[0] for e in K.ATTN_CASES])
def test_attention_mutations_leave_bound(entry):
    """One key fewer and a 2 % wrong softmax scale leave the attention bound (wherever an utterance has two or more keys: over a
    single key the softmax is 1 whatever the scores)."""
    p = K.build_case(entry)
    r, t, m = K.attn_ref(p)["out"]
    if max(p.d["_lens"]) > 1:
        assert _exceeds(r, t, m, K.attn_ref(p, "len_minus1")["out"][0])
        p.d["scale"] *= 1.02
        assert _exceeds(r, t, m, K.attn_ref(p)["out"][0])


# ------------------------------------------------------------------------------------------------------------------------------
# the chained reference of launch_resstream / launch_narrowstage / launch_pairstream
# ------------------------------------------------------------------------------------------------------------------------------
def _torch_resblock(x, blk, slope, L):
    """hifigan.py's ResBlock1 on one utterance x [C][L] (float64): x += conv_1(lrelu(conv_d(lrelu(x)))) per pair."""
    for pr in blk:
        k, d = pr["k"], pr["dil"]
        w1, w2 = (torch.tensor(pr[w]).permute(1, 2, 0) for w in ("W1", "W2"))
        t = F.conv1d(F.leaky_relu(x, slope)[None], w1, torch.tensor(pr["b1"]), padding=d * (k - 1) // 2, dilation=d)[0]
        x = x + F.conv1d(F.leaky_relu(t, slope)[None], w2, torch.tensor(pr["b2"]), padding=(k - 1) // 2)[0]
    return x


@pytest.mark.parametrize("kind", ["resstream", "narrowstage", "pairstream"])
def test_chain_ref_without_roundings_vs_torch(kind):
    """slope 1 / 8 against res_inv_slope 8, so that inv_lrelu undoes lrelu exactly as HiFi-GAN's raw residual has it."""
    slope = 0.125
    if kind == "narrowstage":
        cs = K.make_chain("t", 3, kind=kind, dt=K.DT_BF16, C=8, blocks=[(3, (1, 3, 5)), (11, (1, 3, 5))], M=90, lens=[90, 31, 1], data="dense", slope=0.25)
    else:
        cs = K.make_chain("t", 4, kind=kind, dt=K.DT_F16, C=16, blocks=[(7, (1, 3, 5) if kind == "resstream" else (3,))], M=70, lens=[70, 9], data="dense",
                          am=3, has_out=False)
    cs.slope1, cs.rinv = slope, 1 / slope
    ref = K.chain_ref(cs, q=False)
    f = "out" if kind == "narrowstage" else "accum"
    for b, l in enumerate(cs.lens):
        xa = torch.tensor(cs.X[b, :l].T)
        x = torch.where(xa >= 0, xa, xa / slope)
        ys = [_torch_resblock(x, blk, slope, l) for blk in cs.blocks]
        if kind == "narrowstage":
            y = F.leaky_relu(sum(ys) / len(ys), cs.slope)
        else:
            y = ys[0] + torch.tensor(cs.xs[b, :l].T)
        np.testing.assert_allclose(ref[f][0][b, :l], y.T.numpy(), rtol=1e-12, atol=1e-12)
        assert ref[f][2][b, :l].all() and not ref[f][2][b, l:].any()


def _chain_exact_entries():
    E = [e for e in K.RESSTREAM_CASES + K.NARROW_CASES if e[1].get("data", "exact") == "exact"]
    return E + [(f"narrowstage_c{C}_tile_reuse", K.narrow_reuse_kw(C, 256), 24 if C == 16 else 25) for C in (16, 8)]


def _chain_mutations(cs):
    nk, last = len(cs.blocks), len(cs.blocks[-1]) - 1
    muts = [dict(drop_weight=1, at=(j, t)) for j in range(nk) for t in range(len(cs.blocks[j]))]
    muts += [dict(shift_tap=1), dict(len_minus1=1), dict(res_slope=1), dict(drop_bias=1), dict(no_round_T=1)]
    if cs.kind != "narrowstage" and cs.am & 1:
        muts.append(dict(skip_xs=1))
    if cs.kind == "narrowstage" and nk > 1:
        muts.append(dict(mean_nk_minus1=1))
    seam = 256 if cs.kind == "resstream" else K.NS_R[cs.C]
    if max(cs.lens) > seam:
        muts.append(dict(seam=seam))
    return muts


@pytest.mark.parametrize("entry", _chain_exact_entries(), ids=[e[0] for e in _chain_exact_entries()])
def test_chain_exact_share_and_mutations(entry):
    """From the reference alone: at least 30 % of the compared elements of an exact-sum case have tolerance zero (the kernel must
    match the reference's 16-bit value bit for bit there), and every mutation of the reference leaves the bound somewhere."""
    cs = K.build_chain(entry)
    true = K.chain_ref(cs)
    share = K.exact_share(true)
    assert share >= 0.30, f"{entry[0]}: exact share {share:.3f}"
    weak = []
    for mut in _chain_mutations(cs):
        got = K.chain_ref(cs, bound=False, mut=mut)
        if not any(_exceeds(true[f][0], true[f][1], true[f][2], got[f][0]) for f in true):
            weak.append(mut)
    assert not weak, f"{entry[0]}: mutations within the bound: {weak}"


# ------------------------------------------------------------------------------------------------------------------------------
# the persistent-tile cases (tests/test_persistent_tiles_gpu.py) on the host
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", [64, 256, 304])
def test_persistent_case_builders_make_the_trips_they_claim(ncu):
    """For every CU count the builders give every workgroup at least PERSIST_TRIPS units -- recounted here from the restated grid rule and
    walk, independently of the builder's own search --, the long-then-short, short-then-long and long-then-long successions wherever a
    case has long utterances, an utterance of exactly one unit and units the walk skips, both length paths of resfuse_persist, and NaN
    utterances whose neighbours in a workgroup are compared against float64."""
    entries = K.gemm_persist_cases(ncu) + K.chain_persist_cases(ncu)
    assert [e[0] for e in entries] == [e[0] for e in K.gemm_persist_cases(256) + K.chain_persist_cases(256)]      # the test ids hold on any device
    seen = set()
    for name, kw, vid, meta in entries:
        kernel = next(k for k in K.PERSIST_TRIPS if name.startswith(k))
        seen.add(kernel)
        lens, g, M = kw["lens"], meta["grid"], kw["M"]
        nb = len(lens)
        if kernel.startswith("conv2d"):
            assert g == K.conv2d_grid(meta["kind"], kw["K"], M, nb, ncu)
            walk = K.dealt_walk(g, nb)
            assert sorted(t for w in walk for t in w) == [(b, j) for b in range(nb) for j in range(g["per"])]      # every tile once
            assert len(walk[-1]) == 3 and len(walk[0]) == 4                                                        # a short last round
        else:
            want = dict(resfuse=lambda: K.resfuse_grid(kw["N"], len(kw["taps"]), M, nb, ncu), pairstream=lambda: K.pairstream_grid(M, nb, ncu),
                        narrowstage=lambda: K.narrow_grid(kw["C"], M, nb, ncu),
                        resstream=lambda: K.resstream_grid(kw["C"], kw["blocks"][0][0], len(kw["blocks"][0][1]), M, nb, ncu))[kernel]()
            assert g == want and g["G"] == ncu * (K.NS_WGPC[kw["C"]] if kernel == "narrowstage" else 1)
            walk = K.strided_walk(g, nb, lens)
            run = sorted(t for w in walk for t in w)
            assert run == [(b, j) for b in range(nb) for j in range(g["per"]) if j * g["rows"] < lens[b]]
            if g["per"] > 1:
                assert len(run) < nb * g["per"] and g["rows"] in lens                      # units the walk skips; an utterance of exactly one unit
        assert min(len(w) for w in walk) == meta["trips"] >= K.PERSIST_TRIPS[kernel], name
        if meta["long"]:
            assert {(True, False), (False, True), (True, True)} <= meta["patterns"], name
        first, later = meta["nan"]
        pos = {b: (w, i) for w in walk for i, (b, j) in enumerate(w) if b in meta["nan"]}
        w, i = pos[first]
        assert i + 1 < len(w) and w[i + 1][0] in meta["sample"], name                    # another utterance follows the first NaN one ...
        w, i = pos[later]
        assert i >= 1 and w[i - 1][0] in meta["sample"], name                            # ... and the second is itself a later unit
        assert set(meta["long"]) <= set(meta["sample"]) and not set(meta["nan"]) & set(meta["sample"])
        for w in walk:
            for (b0, _), (b1, _) in zip(w, w[1:]):
                assert b0 not in meta["long"] or b1 in meta["sample"] or b1 in meta["nan"], name
        if name.startswith("resfuse_persist_table"):
            assert nb <= 128 and min(lens[b] for b in meta["long"]) > g["rows"] and len(meta["long"]) > 100
        if name.startswith("resfuse_persist_sload"):
            assert nb > 128
    assert seen == set(K.PERSIST_TRIPS)
    # the accumulator modes and both 16-bit types per kernel family
    for fam in ("resfuse_persist_table", "resfuse_persist_sload", "pairstream_persist", "resstream_persist"):
        names = [e[0] for e in entries if e[0].startswith(fam)]
        assert {n.split("_am")[1][0] for n in names} == set("0123"), fam
        assert {n.rsplit("_", 1)[1] for n in names} == {"bf16", "f16"}, fam


def test_resample_geometry_rule_matches_the_launcher():
    """kernel_ref.resample_geometry_ref restates launch_resample_poly's decision (tile, tiles per workgroup, staged span, LDS bytes); the
    shim's dry run reports what the launcher decides.  Equal over the rate pairs of the resampler tests and over batch and row sizes on
    both sides of every threshold: tpb = 1 .. 8, tile 1024 / 512 / 256, LDS on both sides of 64 KiB."""
    _needs_lib()
    lib = K.load_ktest()
    seen_tpb, seen_tile, seen_big = set(), set(), set()
    for ri, ro in [(22050, 48000), (48000, 22050), (22050, 8000), (16000, 22050), (22050, 22050), (22050, 44100), (192000, 8000), (192000, 6000),
                   (192000, 4000), (4000, 192000)]:
        for B in (1, 2, 5, 64, 192, 256, 1000):
            for out_max in (1, 1023, 1024, 1025, 4096, 65536, 65537, 1 << 20):
                g = K.resample_geometry(lib, ri, ro, B, out_max)
                want = K.resample_geometry_ref(g["L"], g["M"], g["T"], g["pitch"], B, out_max)
                assert g["fits"] and {k: g[k] for k in want} == want, (ri, ro, B, out_max, g, want)
                assert g["T"] + 1 <= g["pitch"] <= g["T"] + 8
                seen_tpb.add(g["tpb"]); seen_tile.add(g["tile"]); seen_big.add(g["lds"] > 64 * 1024)
    assert seen_tpb == set(range(1, 9)) and {1024, 512, 256} <= seen_tile and seen_big == {False, True}


def _dense_rms_entries():
    return [e for e in K.NARROW_CASES if e[1]["data"] == "dense"] + K.PAIR_DENSE_CASES


@pytest.mark.parametrize("entry", _dense_rms_entries(), ids=[e[0] for e in _dense_rms_entries()])
def test_dense_rms_criterion_rejects_swapped_taps(entry):
    """E <= E_r (1 + m) against the pure float64 chain: two swapped taps of one convolution (which sparse weights cannot see as a
    misplaced fragment) exceed it, and m stays a margin, not a licence (below 1: the criterion never allows twice the reference's
    own error)."""
    build = K.dense_builder(entry)
    cs = build(0)
    pure = K.chain_ref(cs, q=False, bound=False)
    mutated = K.chain_ref(cs, bound=False, mut=dict(swap_taps=1, at=(0, 0)))
    for f, (er, spread, m) in K.rms_margin(build).items():
        assert m < 1.0, f"{entry[0]}.{f}: margin {m:.3f}"
        em = K.rms_vs_pure(mutated[f][0], pure[f][0], pure[f][2])
        assert em > er * (1 + m), f"{entry[0]}.{f}: swapped taps give rms {em:.3g}, within {er:.3g} x (1 + {m:.3f})"
