"""Host checks of tests/mel_ref.py, the float64 reference tests/test_mel_gpu.py holds zvx_melspec to (no GPU): the reference against the
two other statements of get_mel_from_wav at every geometry, the packed matrices against the independent float64 design, the
preconditions of the device cases from the reference alone, the mutations the bound must tell apart, and pack_model's refusals."""
import copy

import numpy as np
import pytest

import mel_ref as MR
from oracle import mel_oracle as O
from zerovox_amd import config as zcfg, mels as P, pack

# worst |difference| of the log-mel over every row of every geometry, measured here (x 4 is the asserted limit, the margin of the two
# shape sweeps): reference - product 7.69e-06 (many_mels), reference - oracle 7.19e-07 (odd_pad), product - oracle 7.63e-06 (many_mels)
WORST = {"ref-product": 7.69e-06, "ref-oracle": 7.19e-07, "product-oracle": 7.63e-06}


def _args(g):
    return tuple(g[k] for k in ("sampling_rate", "fft_size", "hop_size", "win_length", "num_mels", "fmin", "fmax"))


@pytest.mark.parametrize("case", list(MR.GEOMETRIES))
def test_three_statements_agree(case):
    """mel_ref (float64 throughout, from the header), zerovox_amd.mels.get_mel_from_wav (f32 window, f32 magnitudes and basis) and
    oracle/mel_oracle.get_mel_from_wav (per-frame float64 FFT, f32 magnitudes and basis) agree to the float32 rounding of a float64
    pipeline on every row of the case, the refused geometry included (the host statements take any).  Measured (absolute, on the
    log-mel; the worst over the seven geometries, each at the geometry named): reference - product 7.69e-06 (many_mels), reference -
    oracle 7.19e-07 (odd_pad), product - oracle 7.63e-06 (many_mels); per geometry the three figures are printed.  Limit: 4 x these."""
    g = MR.geom(case)
    w = dict.fromkeys(WORST, 0.0)
    for r in MR.case_rows(case):
        v, _, _ = MR.mel_ref(r, g)
        a = P.get_mel_from_wav(r, *_args(g))[0].T.astype(np.float64)
        b = O.get_mel_from_wav(r, *_args(g))[0].T.astype(np.float64)
        assert v.shape == a.shape == b.shape == (MR.frames_of(len(r), g), g["num_mels"])
        for k, d in (("ref-product", v - a), ("ref-oracle", v - b), ("product-oracle", a - b)):
            w[k] = max(w[k], float(np.abs(d).max()))
    print(f"SPEC mel {case} host statements: " + ", ".join(f"{k} {x:.3g}" for k, x in w.items()))
    for k, x in w.items():
        assert x <= 4 * WORST[k], (case, k, x)


@pytest.mark.parametrize("case", MR.RUNNING)
def test_packed_matrices_equal_the_design(case):
    """mel.dft and mel.basis as pack_model emits them against the independent float64 design rounded to f32.  Measured: mel.basis is
    equal at every geometry, value for value.  mel.dft differs in 1 to 8 % of its elements: where cos / sin vanish (the product scales
    the angle before it reduces it and holds up to 1e-13 where the design holds 0 or 1e-16), by at most 2e-6 f32 ulp of the row's
    peak; and with win_length = 900, where the two window formulas round apart, by one ulp of a small element, 0.031 ulp of the peak.
    The peak is that of the row's envelope, the window: the sine rows of DC and Nyquist vanish altogether, and a peak of their own
    would be rounding junk.  Structural zeros -- the columns where the window is zero, the padding rows of mel.dft, everything
    outside a triangle and the padding columns of mel.basis -- are exact."""
    g = MR.geom(case)
    nf, NR, KP = MR.dims(g)
    dft, basis = MR.packed(case)
    d64, b64 = MR.design(g)
    assert dft.shape == d64.shape == (NR, g["fft_size"]) and basis.shape == b64.shape == (g["num_mels"], KP)
    assert dft.dtype == basis.dtype == np.float32
    assert np.array_equal(basis, b64.astype(np.float32))                           # (as values: the product holds -0.0 at bin 0 of filter 0)
    assert not basis[:, nf:].any() and not dft[2 * nf:].any() and not dft[:, MR.window(g) == 0].any()
    live = d64[:2 * nf]
    ulp = 2 * MR.half_ulp(MR.window(g).max(), MR.DT_F32)
    off = dft[:2 * nf] != live.astype(np.float32)
    dist = float((np.abs(dft[:2 * nf].astype(np.float64) - live.astype(np.float32)) / ulp).max())
    print(f"SPEC mel {case} packed: mel.basis equal; mel.dft {int(off.sum())} of {off.size} elements not bit-equal, "
          f"worst distance {dist:.3g} f32 ulp of the row's peak")
    assert dist <= 1.0, dist


def test_case_preconditions():
    """What the device cases rest on, from the reference alone.  The issue's 136-mel geometry has NO empty filter (its narrowest filter
    sums to 2.0e-3: a triangle 44 Hz wide always holds one of the 43 Hz bins) and more mels than a model may have; empty_filters (128
    mels over the 86 Hz bins of n_fft = 256) has 26, so its device run reaches the clip through a filter."""
    _, b136 = MR.design(MR.geom("many_mels"))
    assert (b136.sum(axis=1) > 1e-3).all() and MR.geom("many_mels")["num_mels"] > 8 * pack.MAX_TAPS
    for case in MR.RUNNING:
        g = MR.geom(case)
        nf, _, KP = MR.dims(g)
        rows, ref = MR.case_rows(case), MR.case_ref(case)
        n = [len(r) for r in rows]
        lo = MR.min_len(g)
        assert n[0] == lo and n[1] == lo + 1 and [MR.frames_of(k, g) for k in n[2:5]] == [3, 4, 4] and MR.frames_of(n[5], g) >= 36
        assert MR.frames_of(lo, g) >= 1 and (lo - 1 < MR.pad_of(g) + 1 or MR.frames_of(lo - 1, g) < 1)
        empty = ~MR.packed(case)[1].any(axis=1)
        assert empty.sum() == (26 if case == "empty_filters" else 0), (case, int(empty.sum()))
        zeros, quiet, clip = (ref[MR.ROW_NAMES.index(k)] for k in ("zeros", "quiet", "at_clip"))
        assert not zeros[2].any() and np.all(zeros[0] == MR.LOG_LO)                      # the silent row clips everywhere, exactly
        for v, bd, M in ref:
            assert np.all(v[:, empty] == MR.LOG_LO) and np.all(bd[M == 0] <= (MR.R.K_ULP["log"] + 0.5) * MR.R.ulp32(MR.LOG_LO))
        assert (quiet[2] < 10 * MR.LO).mean() > 0.05                                     # near the clip or under it (tiny: all under)
        assert 0.3 < (clip[2] < MR.LO).mean() < 0.7 and clip[2].max() < 100 * MR.LO      # on both sides of the clip, near it
        rel = np.concatenate([(bd / np.abs(v)).ravel() for v, bd, _ in ref])
        ab = np.concatenate([bd.ravel() for _, bd, _ in ref])
        print(f"SPEC mel {case} bound: {len(rel)} elements; bound / |ref| largest {rel.max():.3g}, median {np.median(rel):.3g}; "
              f"bound largest {ab.max():.3g}, median {np.median(ab):.3g}")
        assert np.isfinite(ab).all() and (ab > 0).all()


@pytest.mark.parametrize("mut", MR.MUTATIONS)
def test_bound_tells_the_mutations_apart(mut):
    """A front end that shifts the window by one sample, loses the last bin of one filter, or rounds the padding up leaves the bound of
    the reference somewhere in every geometry it changes (rounding the padding up changes only odd_pad, where n_fft - hop is odd)."""
    for case in MR.RUNNING:
        g = MR.geom(case)
        if mut == "ceil_pad" and (g["fft_size"] - g["hop_size"]) % 2 == 0:
            continue
        dft, basis = MR.packed(case)
        out = 0
        for r, (v, bd, _) in zip(MR.case_rows(case), MR.case_ref(case)):
            if mut == "ceil_pad" and len(r) < MR.pad_of(g) + 2:
                continue                                                                  # (shorter than the longer mirror)
            w = MR.mel_ref(r, g, dft, basis, mut=mut)[0]
            k = min(len(v), len(w))
            out += int((np.abs(w[:k] - v[:k]) > bd[:k]).sum()) + abs(len(v) - len(w))
        assert out > 0, (case, mut)


def _cfg(changes):
    cfg = zcfg.reduced_modelcfg("styletts")
    cfg["audio"].update(changes)
    return cfg


@pytest.mark.parametrize("bad", list(MR.BAD_STFT))
def test_check_model_config_names_the_stft_field(bad):
    changes, field, _ = MR.BAD_STFT[bad]
    with pytest.raises(ValueError, match=field + " = "):
        pack.check_model_config(_cfg(changes), "bf16", 80)


def test_pack_model_refuses_and_accepts_by_geometry():
    """pack_model itself: the 136-mel geometry and an STFT block with hop_size > fft_size are refused by name before anything is packed;
    the shipped configs and every running geometry pass (test_packed_matrices_equal_the_design packs those)."""
    import test_spectral_gpu as TS
    g = MR.geom("many_mels")
    with pytest.raises(ValueError, match=MR.REFUSED["many_mels"][0] + " = 136"):
        TS.packed_at(g["fft_size"], g["hop_size"], g["win_length"], **{k: g[k] for k in MR.FIELDS[3:]})
    with pytest.raises(ValueError, match="hop_size = 256"):
        TS.packed_at(128, 256, 128)
    with pytest.raises(ValueError, match="win_length = 512"):
        TS.packed_at(256, 256, 512)
    for kind in ("styletts", "fastspeech2"):
        pack.check_stft_config(zcfg.medium_modelcfg(kind)["audio"])
        pack.check_stft_config(zcfg.reduced_modelcfg(kind)["audio"])
    for case in MR.RUNNING:
        pack.check_stft_config(copy.deepcopy(MR.geom(case)))
