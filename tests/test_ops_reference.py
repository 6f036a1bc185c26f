"""Host-side checks of tests/ops_ref.py, the float64 references tests/test_ops_gpu.py holds the small kernels of ops.hip to:
  * the shim exports every zvxk_<launcher> entry the cases call, with the registered argument types;
  * each reference agrees to 1e-12 with an independent formulation in torch float64 on its ragged cases;
  * the references discriminate: every mutation of ops_ref.MUTATIONS leaves the bound -- computed from the unmutated reference
    alone -- of at least one element of at least one case of its launcher, so no tolerance is loose enough to hide that fault;
  * coverage: every launch_* declared in the ops.hip section of zvx_kernels.h has a case or a reasoned entry in ops_ref.EXCLUDED."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as K
import ops_ref as R

TOL = dict(rtol=1e-12, atol=1e-12)


def _ref(name, key):
    cs = R.case(name)
    with np.errstate(all="ignore"):
        r, _t, m = cs.ref()[key]
    return cs, r, m


def test_shim_exports_every_entry():
    if not os.path.exists(K.KTEST_LIB):
        pytest.fail(f"{K.KTEST_LIB} is missing: run zerovox_amd.build first")
    lib = K.load_ktest()                               # registers the argtypes: a missing symbol raises here
    for c in R.cases():
        f = getattr(lib, "zvxk_" + c.fn)
        assert len(f.argtypes) == len(c.args), f"{c.name}: {len(c.args)} arguments for zvxk_{c.fn}{K.OPS_SIG[c.fn]}"
        for a, ch in zip(c.args, K.OPS_SIG[c.fn]):
            assert (ch == "p") == (a is None or isinstance(a, (str, tuple))), f"{c.name}: argument {a!r} against '{ch}'"
    assert lib.zvxk_se_pool_splits(19, 27) == R.se_splits(19, 27) == 2


@pytest.mark.parametrize("name", ["layernorm_c20_m0_f32_bf16_post0", "layernorm_c528_m0_f32_f32_post0", "layernorm_c8_m0_f32_f32_post1"])
def test_layernorm_vs_torch(name):
    cs, r, m = _ref(name, R.case(name).info["ykey"])
    i = cs.info
    B, Rr, C = i["B"], i["R"], i["C"]
    x = cs.val("x").reshape(B, Rr, -1)[:, :, :C]
    r = r.reshape(B, Rr, i["ldy"])[:, :, :C]
    for b, n in enumerate(R.LN_ROWS):
        y = F.layer_norm(torch.tensor(x[b, :n]), (C,), torch.tensor(cs.val("gamma")), torch.tensor(cs.val("beta")), eps=1e-5).numpy()
        if "post" in cs.bufs:
            y = y + cs.val("post").reshape(B, C)[b]
        np.testing.assert_allclose(r[b, :n], y, **TOL)
    assert m.sum() == sum(R.LN_ROWS) * C


def test_scln_vs_hand_written():
    """SCLN (fs2.py:76-90): unbiased std, / (sigma + eps), beta = first half of the style row, gamma = second half."""
    cs, r, m = _ref("layernorm_c528_m1_f32_bf16_post0", "y")
    i = cs.info
    B, Rr, C = i["B"], i["R"], i["C"]
    x = torch.tensor(cs.val("x").reshape(B, Rr, -1)[:, :, :C])
    bg = torch.tensor(cs.val("bg").reshape(B, -1))
    r = r.reshape(B, Rr, i["ldy"])[:, :, :C]
    for b, n in enumerate(R.LN_ROWS):
        if not n:
            continue
        xb = x[b, :n]
        y = bg[b, C:2 * C] * (xb - xb.mean(-1, keepdim=True)) / (xb.std(-1, unbiased=True, keepdim=True) + 1e-8) + bg[b, :C]
        np.testing.assert_allclose(r[b, :n], y.numpy(), **TOL)


def test_instnorm_vs_torch():
    name = "instnorm_fused_c72_bf16_bf16_aff00_act0"
    cs = R.case(name)
    with np.errstate(all="ignore"):
        ref = cs.ref()
    i = cs.info
    B, Lmax, C = i["B"], i["Lmax"], i["C"]
    x = cs.val("x").reshape(B, Lmax, i["ldx"])[:, :, :C]
    y = ref["y"][0].reshape(B, Lmax, i["ldy"])[:, :, i["yoff"]:i["yoff"] + C]
    for b, n in enumerate(R.IN_L):
        if n < 2:
            continue
        xb = torch.tensor(x[b, :n]).T[None]
        np.testing.assert_allclose(y[b, :n], F.instance_norm(xb, eps=1e-5)[0].T.numpy(), **TOL)
        np.testing.assert_allclose(ref["mean"][0].reshape(B, C)[b], xb[0].mean(1).numpy(), **TOL)
        np.testing.assert_allclose(ref["rstd"][0].reshape(B, C)[b], 1 / np.sqrt(xb[0].var(1, unbiased=False).numpy() + 1e-5), **TOL)


def test_norm_affine_act_vs_torch():
    name = next(c.name for c in R.cases() if c.fn == "norm_affine_act" and c.info["affine"] and c.info["one_plus"] and c.info["act"] == R.ACT_LRELU)
    cs, r, m = _ref(name, "y")
    i = cs.info
    B, Lmax, C = i["B"], i["Lmax"], i["C"]
    x = cs.val("x").reshape(B, Lmax, i["ldx"])[:, :, :C]
    g, be = (cs.val(k).reshape(B, i["g_bs"])[:, :C] for k in ("gamma", "beta"))
    mean, rstd = cs.val("mean").reshape(B, C), cs.val("rstd").reshape(B, C)
    r = r.reshape(B, Lmax, i["ldy"])[:, :, i["yoff"]:i["yoff"] + C]
    for b, n in enumerate(R.IN_L):
        g1 = (np.float32(1.0) + g[b].astype(np.float32)).astype(np.float64)
        y = F.leaky_relu(torch.tensor((x[b, :n] - mean[b]) * rstd[b] * g1 + be[b]), i["slope"]).numpy()
        np.testing.assert_allclose(r[b, :n], y, **TOL)


def test_softmax_vs_torch():
    cs, r, m = _ref("softmax_rows_f32", "P")
    sc = cs.val("sc").reshape(14, 131, 136)
    r = r.reshape(14, 131, 136)
    for z in range(14):
        L = [1, 7, 8, 9, 64, 65, 130][z // 2]
        np.testing.assert_allclose(r[z, :L, :L], torch.softmax(torch.tensor(sc[z, :L, :L]), -1).numpy(), **TOL)
        assert not r[z, :L, L:].any()


def test_conv_post_vs_torch():
    cs, r, m = _ref("conv_post_tanh_f32_k7_c32_f32", "wav")
    x = cs.val("x").reshape(5, 600, 40)[:, :, :32]
    w = torch.tensor(cs.val("w").reshape(7, 32)).T[None]          # [1][C][k]
    r = r.reshape(5, 608)
    for b, (no, ni) in enumerate(zip([600, 257, 256, 3, 0], [598, 254, 252, 2, 0])):
        if not no:
            continue
        xin = np.zeros((no, 32))
        xin[:ni] = x[b, :ni]
        y = torch.tanh(F.conv1d(torch.tensor(xin).T[None], w, bias=torch.tensor([0.0625], dtype=torch.float64), padding=3))[0, 0].numpy()
        np.testing.assert_allclose(r[b, :no], y, **TOL)
        assert not r[b, no:].any()


def test_spk_front_vs_torch():
    cs, r, m = _ref("spk_front_c16_f32", "out")
    B, F_, T_, Wout, C0 = 3, 5, 70, 72, 16
    mels, mean, rstd = cs.val("mels").reshape(B, T_, F_), cs.val("mean").reshape(B, F_), cs.val("rstd").reshape(B, F_)
    w = torch.tensor(cs.val("w").reshape(3, 3, C0)).permute(2, 0, 1)[:, None]       # [C0][1][df][dt]
    r = r.reshape(B, F_, Wout, C0)
    for b, n in enumerate([70, 64, 1]):
        img = torch.tensor(((mels[b, :n] - mean[b]) * rstd[b]).T)[None, None]        # [1][1][F][T]
        y = F.relu(F.conv2d(img, w, torch.tensor(cs.val("bias")), padding=1))[0]
        y = y * torch.tensor(cs.val("bs"))[:, None, None] + torch.tensor(cs.val("bt"))[:, None, None]
        np.testing.assert_allclose(r[b, :, :n], y.permute(1, 2, 0).numpy(), **TOL)


def test_se_vs_torch():
    """Pool: the partial sums add up to the masked sum of the map.  MLP: mean (+ pool bias) -> linear -> relu -> linear -> sigmoid."""
    cs, r, m = _ref("se_pool_split_c32_h19_w27_f32", "partial")
    x = np.nan_to_num(cs.val("x").reshape(3, 19, 27, 32))
    np.testing.assert_allclose(r[:3 * 2 * 32].reshape(3, 2, 32).sum(1), x.sum((1, 2)), **TOL)
    cs, r, m = _ref("se_fc_c32_s5_pb1", "scale")
    p = torch.tensor(cs.val("partial").reshape(3, 5, 32))
    for b, Wb in enumerate([20, 7, 1]):
        mean = p[b].sum(0) / (3 * Wb) + torch.tensor(cs.val("pb"))
        h = F.relu(F.linear(mean, torch.tensor(cs.val("w1").reshape(4, 32)), torch.tensor(cs.val("b1"))))
        y = torch.sigmoid(F.linear(h, torch.tensor(cs.val("w2").reshape(32, 4)), torch.tensor(cs.val("b2"))))
        np.testing.assert_allclose(r[b * 32:(b + 1) * 32], y.numpy(), **TOL)


def test_asp_vs_torch():
    cs, r, m = _ref("asp_pool_f3_c24_f32_asp", "out")
    B, F_, Wmax, C = 3, 3, 20, 24
    D = F_ * C
    x, lg = cs.val("x").reshape(B, F_, Wmax, C), cs.val("lg").reshape(B, Wmax, D)
    for b, T in enumerate([20, 7, 1]):
        v = torch.tensor(x[b, :, :T]).permute(1, 0, 2).reshape(T, D)
        w = torch.softmax(torch.tensor(lg[b, :T]), 0)
        mu = (w * v).sum(0)
        sg = torch.sqrt(((w * v * v).sum(0) - mu * mu).clamp(min=1e-5))
        np.testing.assert_allclose(r[b * 2 * D:b * 2 * D + D], mu.numpy(), **TOL)
        np.testing.assert_allclose(r[b * 2 * D + D:(b + 1) * 2 * D], sg.numpy(), **TOL)
        assert sg[C + 3] == np.sqrt(1e-5)                          # the constant column sits on the clamp


def test_length_regulate_vs_torch():
    cs, r, m = _ref("length_regulate", "feats")
    x = cs.val("x").reshape(4, 6, 16)[:, :, :12]
    cum = cs.val("cum").reshape(4, 6).astype(np.int64)
    r = r.reshape(4, 11, 12)
    for b, T in enumerate([6, 4, 0, 1]):
        if not T:
            assert not m.reshape(4, 11, 12)[b].any()
            continue
        dur = np.diff(np.concatenate([[0], cum[b, :T]]))
        y = torch.repeat_interleave(torch.tensor(x[b, :T]), torch.tensor(dur), 0).numpy()
        assert np.array_equal(r[b, :len(y)], y) and m.reshape(4, 11, 12)[b, :len(y)].all() and not m.reshape(4, 11, 12)[b, len(y):].any()


def test_durations_vs_integer_cumsum():
    cs = R.case("durations_forced")
    ref = cs.ref()
    T = [1, 63, 64, 65, 130, 0]
    f = torch.tensor(cs.val("forced").reshape(6, 130).astype(np.int64))
    for b, n in enumerate(T):
        d = f[b, :n].clamp(0, 65536)
        assert np.array_equal(ref["dur"][0].reshape(6, 130)[b, :n], d.numpy()) and np.array_equal(ref["cum"][0].reshape(6, 130)[b, :n], torch.cumsum(d, 0).numpy())
        assert ref["mel_len"][0][b] == int(d.sum())
    cs = R.case("durations_q16_forced")
    ref = cs.ref()
    f, q = cs.val("forced").reshape(6, 130), cs.val("q").reshape(6, 130)
    for b, n in enumerate(T):
        P, prev = 0, 0
        for t in range(n):                                          # exact integers: Python's own
            P += min(max(int(f[b, t]), 0), 65536) * int(q[b, t])
            c = (P + 32768) >> 16
            assert ref["dur"][0].reshape(6, 130)[b, t] == c - prev and ref["cum"][0].reshape(6, 130)[b, t] == min(c, 2 ** 31 - 1)
            prev = c
        assert ref["mel_len"][0][b] == min(prev, 2 ** 31 - 1)
    big = R.case("durations_forced_big").ref()
    assert big["cum"][0].max() == 2 ** 31 - 1 and big["mel_len"][0][0] == 2 ** 31 - 1 and big["cum"][0][32766] == 32767 * 65536


_PAIRS = [(fn, mut) for fn, muts in R.MUTATIONS.items() for mut in muts]


@pytest.mark.parametrize("fn,mut", _PAIRS, ids=[f"{f}-{m}" for f, m in _PAIRS])
def test_mutation_leaves_the_bound(fn, mut):
    with np.errstate(all="ignore"):
        assert any(R.rejected(c, mut) for c in R.cases() if c.fn == fn), f"{fn}: no case rejects the mutation '{mut}': a case or a bound is too loose"


def test_every_launcher_has_mutations_and_cases():
    fns = {c.fn for c in R.cases()}
    assert fns == set(R.MUTATIONS), fns ^ set(R.MUTATIONS)
    for needed in ("len_plus1", "len_minus1", "drop_last_group", "unbiased", "eps_outside", "var_swap", "eps_swap", "bg_swap", "drop_one_plus", "drop_post",
                   "drop_round2", "tail_not_zeroed", "shift_tap", "nin_not_zeroed", "drop_pool_bias", "no_clamp", "no_round", "half_away", "uncentred",
                   "mean_f32", "drop_range", "pcm_round"):
        assert any(needed in v for v in R.MUTATIONS.values()), needed
    for fn, muts in R.MUTATIONS.items():
        assert "len_plus1" in muts and "len_minus1" in muts, f"{fn}: a length off by one in either direction"


def test_every_launcher_of_the_section_is_covered():
    src = open(os.path.join(K.ROOT, "zerovox_amd", "csrc", "zvx_kernels.h")).read()
    sec = src[src.index("Small kernels (ops.hip)"):]
    declared = set(re.findall(r"^\s*(?:void|bool|int)\s+(launch_\w+)\s*\(", sec, re.M))
    assert len(declared) > 50, declared
    covered = {"launch_" + c.fn for c in R.cases()}
    assert not covered & set(R.EXCLUDED), covered & set(R.EXCLUDED)
    missing = declared - covered - set(R.EXCLUDED)
    assert not missing, f"launchers without a case in tests/ops_ref.py or a reason in EXCLUDED: {sorted(missing)}"
    stale = (covered | set(R.EXCLUDED)) - declared
    assert not stale, f"not declared in the section any more: {sorted(stale)}"
