"""Generator shapes outside the named configurations (config._HIFIGAN) against the oracle: the routing layer of zvx.hip
(voc_domains, voc_upsample, voc_narrow_stage, voc_resblock, stage_close) turns ANY config.json into launches, and every branch of it
is walked here by one entry of generator_ref.SWEEP.

CPU part: the oracle against an independent float64 generator at every shape of the table; the packed polyphase taps against
conv_transpose1d; the refusals of pack_model.
GPU part (-m gpu): per case either parity with the oracle or a refusal at pack_model AND at zvx_create that names the field --
a silently wrong waveform is the one outcome that fails.
  f32 context   the deciding check: every row of a ragged batch against its own batch-1 oracle call at check_f32's 2e-4 x max(1, max|ref|)
  16-bit        finite; check_wav's "vocoder alone" limits, unchanged; bit-equal with every fusion switched off; an utterance alone ==
                inside the batch, bit for bit; the launch counts per kernel variant pinned in generator_ref.LAUNCHES
ZVX_SWEEP_LOG=<file>: every comparison appends what it measured (profiles/generator_shape_sweep.txt is such a file).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import generator_ref as G
from oracle import zvx_oracle as O                      # checker only
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

CASES = list(G.SWEEP)
RUNNING = [c for c in CASES if G.runs(c, "f32")]
REFUSED = [(c, p) for c in CASES for p in ("f32", "bf16") if not G.runs(c, p)]
SEED = 3                                                # of the generator's weights

# max|oracle - ref| / max|ref| per stage tensor and for the waveform: the oracle's own f32 arithmetic.  Measured over the table
# (weights seed 3, the first row of each case's batch): 4.9e-7 .. 1.09e-6, worst c4_tail's last stage.  Asserted at 4 x the worst --
# a wrong tap, padding or scale is O(1).
ORACLE_REL = 4 * 1.09e-6

_cache = {}


def _log(case, what, *vals):
    line = f"{case} | {what} | " + " ".join(v if isinstance(v, str) else f"{v:.3e}" for v in vals)
    print(line)
    path = os.environ.get("ZVX_SWEEP_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _gen(case):
    """(h, state dict, folded state dict) of a case: computed once, shared, never modified"""
    if ("gen", case) not in _cache:
        h = G.SWEEP[case]["h"]
        hsd = zw.hifigan_state_dict(h, SEED)
        _cache["gen", case] = (h, hsd, zw.folded(hsd))
    return _cache["gen", case]


def _oracle_rows(case, seed=0):
    """the ragged batch of a case and, per row, its own batch-1 oracle call (wav, stages)"""
    if ("rows", case, seed) not in _cache:
        h, hsd, _ = _gen(case)
        mel, P = G.batch_mel(case, seed)
        _cache["rows", case, seed] = (mel, P, [O.hifigan_generator(mel[b, :P[b]].T, hsd, h, return_stages=True) for b in range(len(P))])
    return _cache["rows", case, seed]


def _packed(case, prec, h=None):
    """pack_model of the reduced TTS model (a few MB) with the case's generator; h: another generator config with the case's hop"""
    hop = G.SWEEP[case]["hop"]
    cfg = zcfg.reduced_modelcfg("styletts")
    cfg["audio"]["hop_size"] = hop
    if "tts" not in _cache:
        _cache["tts"] = zw.tts_state_dict(cfg, 0)
    if h is None:
        h, hsd, _ = _gen(case)
    else:
        hsd = zw.hifigan_state_dict(h, SEED)
    return pack.pack_model(cfg, _cache["tts"], h, hsd, prec)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_oracle_agrees_with_the_float64_generator(case):
    """Every entry of the table -- the refused ones too: the reference accepts them, and `odd_k_minus_u` yields T u + 1 rows per
    stage in both -- stage by stage and for the waveform."""
    h, _, fsd = _gen(case)
    mel, P, rows = _oracle_rows(case)
    wav, stages = rows[0]
    rwav, rstages = G.generator_ref(mel[0, :P[0]].T, fsd, h)
    assert wav.shape == rwav.shape and len(stages) == len(rstages) == len(h["upsample_rates"])
    if (h["upsample_kernel_sizes"][0] - h["upsample_rates"][0]) % 2 == 0:
        assert wav.shape == (int(P[0]) * G.SWEEP[case]["hop"],)
    errs = []
    for a, b in list(zip(stages, rstages)) + [(wav, rwav)]:
        assert a.shape == b.shape
        errs.append(float(np.abs(a - b).max() / np.abs(b).max()))
    _log(case, "oracle vs f64 ref, max|err|/max|ref| per stage, wav", *errs)
    assert max(errs) <= ORACLE_REL, errs


@pytest.mark.parametrize("case", RUNNING)
def test_packed_polyphase_taps_equal_conv_transpose1d(case):
    """The 3-tap weights pack_model emits (voc.up{i}_w, and _wlo / _whi where present), evaluated in float64 as
    out[t u + ph] = sum_tap poly[tap] . x[t + dv], against conv_transpose1d on the folded weights -- every row, so the first and the
    last u outputs (where a tap reads past either end) included."""
    h, _, fsd = _gen(case)
    man, blob = _packed(case, "f32")
    rng = np.random.default_rng(17)
    cin = h["upsample_initial_channel"]
    forms = set()
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = rng.standard_normal((5, cin))
        ref = F.conv_transpose1d(torch.as_tensor(x.T)[None], torch.as_tensor(fsd[f"ups.{i}.weight"].astype(np.float64)),
                                 torch.as_tensor(fsd[f"ups.{i}.bias"].astype(np.float64)), stride=u, padding=(k - u) // 2)[0].numpy().T
        got = G.polyphase_upsample(x, man, blob, i, u)
        for form, y in got.items():
            assert y.shape == ref.shape == (5 * u, cin // 2)
            err = float(np.abs(y - ref).max())
            assert err <= 1e-12, (case, i, u, k, form, err)
            forms.add(form)
        assert ("lohi" in got) == (k == 2 * u and u % 2 == 0 and cin >= 256)
        cin //= 2
    if case == "one_block":
        assert forms == {"w", "lohi"}
    if case == "odd_rates":
        assert forms == {"w"}


@pytest.mark.parametrize("case,prec", REFUSED)
def test_pack_model_refuses_by_naming_the_field(case, prec):
    field = G.SWEEP[case]["refused"][prec][0]
    with pytest.raises(ValueError, match=field):
        _packed(case, prec)


def test_pack_model_refuses_other_malformed_generators():
    ok = G.SWEEP["rb2_one"]["h"]
    for field, change in (("upsample_rates", {"upsample_rates": [8, 8, 2]}), ("upsample_kernel_sizes", {"upsample_kernel_sizes": [16, 16]}),
                          ("upsample_kernel_sizes", {"upsample_kernel_sizes": [16, 6, 8]}), ("upsample_initial_channel", {"upsample_initial_channel": 36}),
                          ("resblock_kernel_sizes", {"resblock_kernel_sizes": [4]}), ("resblock_kernel_sizes", {"resblock_kernel_sizes": [17]}),
                          ("resblock_dilation_sizes", {"resblock_dilation_sizes": [[1], [2]]}), ("resblock_dilation_sizes", {"resblock_dilation_sizes": [[]]})):
        with pytest.raises(ValueError, match=field):
            pack.check_generator_config({**ok, **change}, 256, "bf16")
    pack.check_generator_config(ok, 256, "bf16")
    for name in ("v1", "v2", "v3", "tiny", "tiny2", "tiny3"):
        for prec in ("bf16", "f32"):
            pack.check_generator_config(zcfg.hifigan_config(name), 256, prec)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------
def _dev(fn, *a, **kw):
    """A HIP error ends the session: nothing more is started on a device that faulted.  (A machine without a device: the GPU cases skip.)"""
    try:
        return fn(*a, **kw)
    except _lib.ZvxError as e:
        if e.code == _lib.ZVX_E_HIP and "no HIP device available" in str(e):
            pytest.skip("no GPU")
        if e.code == _lib.ZVX_E_HIP:
            pytest.exit(f"HIP error: {e}", returncode=3)
        raise


def _variants(ctx, fn):
    from test_gpu_parity import _variants_of
    return {k: n for k, n in _dev(_variants_of, ctx, fn).items() if n}


def _check_refused_at_create(case, prec):
    """zvx_create on a manifest written by hand (pack_model refuses the config): the packed manifest of the nearest shape the device
    runs with the offending cfg line replaced.  The refusal names the key, and the process goes on working."""
    e = G.SWEEP[case]
    key = e["refused"][prec][1]
    if key == "voc_ksizes":
        near = {**e["h"], "upsample_kernel_sizes": [2 * u for u in e["h"]["upsample_rates"]]}
        man, blob = _packed(case, prec, near)
        bad = man.replace("cfg voc_ksizes " + ",".join(str(k) for k in near["upsample_kernel_sizes"]),
                          "cfg voc_ksizes " + ",".join(str(k) for k in e["h"]["upsample_kernel_sizes"]))
    else:
        man, blob = _packed(case, "f32")
        bad = man.replace("cfg precision f32", "cfg precision " + prec)
    assert bad != man
    with pytest.raises(_lib.ZvxError) as ei:
        _dev(_lib.Context, bad, blob, 0)
    _log(case, f"zvx_create refusal [{prec}]", str(ei.value))
    assert ei.value.code in (_lib.ZVX_E_UNSUPPORTED, _lib.ZVX_E_MANIFEST) and key in str(ei.value), str(ei.value)
    ctx = _dev(_lib.Context, man, blob, 0)                    # the library is still usable
    try:
        wav = _dev(ctx.vocode_mel, np.ones((1, 2, 80), np.float32), np.array([2], np.int32))
        assert wav.shape == (1, 2 * e["hop"]) and np.isfinite(wav).all() and wav.any()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_generator_shape_in_f32_equals_the_oracle_or_is_refused(case):
    """The deciding check.  Each row of the ragged batch [pmax, 1, pmax // 2] (mel rows behind an utterance's end hold NaN) against its own
    batch-1 oracle call; the waveform is P x hop samples and zero behind P[b] x hop (include/zvx.h); row 1 alone == row 1 in the batch."""
    from test_gpu_parity import check_f32, stats
    if not G.runs(case, "f32"):
        with pytest.raises(ValueError):
            _packed(case, "f32")
        return _check_refused_at_create(case, "f32")
    hop = G.SWEEP[case]["hop"]
    mel, P, rows = _oracle_rows(case)
    man, blob = _packed(case, "f32")
    ctx = _dev(_lib.Context, man, blob, 0)
    try:
        v = _variants(ctx, lambda: ctx.vocode_mel(mel, P))
        _log(case, "launches [f32]", repr(dict(sorted(v.items()))))
        wav = _dev(ctx.vocode_mel, mel, P)
        assert wav.shape == (len(P), int(P.max()) * hop) and wav.dtype == np.float32
        for b in range(len(P)):
            n = int(P[b]) * hop
            ref = rows[b][0]
            assert ref.shape == (n,)
            mx, rms, _, bm = stats(wav[b, :n], ref)
            _log(case, f"f32 row {b} (P {int(P[b])}): max err, rms err, max|ref|", mx, rms, bm)
        for b in range(len(P)):
            n = int(P[b]) * hop
            check_f32(wav[b, :n], rows[b][0], f"{case} row {b}")
            assert not wav[b, n:].any(), f"{case} row {b}: samples behind P x hop"
        alone = _dev(ctx.vocode_mel, mel[1:2, :1], P[1:2])
        assert np.array_equal(alone[0, :hop], wav[1, :hop])
        assert v == G.LAUNCHES[case]["f32"], v
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_generator_shape_in_16_bit_stays_in_its_limits_and_bit_equal_without_fusions(case):
    """The 16-bit context of every case (the f32 comparison above is the correctness check; these limits guard regressions):
      * every sample finite, each row within check_wav's "vocoder alone" limits of its arithmetic, unchanged: 2e-3 / 4e-4 for a generator
        all in IEEE half, 5e-3 / 9e-4 where a 128-channel ResBlock1 stage runs in bf16 (voc_domains; `mixed` in the table), as for V1;
      * bit-equal with zvx_set_int resstream 0, rb2fuse 0, pairstream 0 -- the three fusions that claim it (resstream == per-pair
        resfuse, rb2fuse == per-convolution, pairstream == two conv-slab launches) -- and, where a 128-channel ResBlock1 stage exists,
        with pairstream 3 (the pair kernel whatever the job size).  narrowstage.hip makes no such claim and stays on in every run;
      * row 1 (one frame) alone == inside the batch, bit for bit;
      * the launch counts per kernel variant equal generator_ref.LAUNCHES, and the variants the table rules out are absent.
    c4_tail (a 4-channel last stage) is refused in the 16-bit precision, so there is no bf16-generator limit to measure."""
    from test_gpu_parity import check_wav, stats
    e = G.SWEEP[case]
    if not G.runs(case, "bf16"):
        with pytest.raises(ValueError):
            _packed(case, "bf16")
        return _check_refused_at_create(case, "bf16")
    hop = e["hop"]
    mel, P, rows = _oracle_rows(case)
    man, blob = _packed(case, "bf16")
    ctx = _dev(_lib.Context, man, blob, 0)
    try:
        v = _variants(ctx, lambda: ctx.vocode_mel(mel, P))
        _log(case, "launches [bf16]", repr(dict(sorted(v.items()))))
        wav = _dev(ctx.vocode_mel, mel, P)
        assert wav.shape == (len(P), int(P.max()) * hop)
        assert np.isfinite(wav).all()
        for b in range(len(P)):
            n = int(P[b]) * hop
            mx, rms, _, bm = stats(wav[b, :n], rows[b][0])
            _log(case, f"16-bit row {b} (P {int(P[b])}): max err, rms err, max|ref|", mx, rms, bm)
        for b in range(len(P)):
            n = int(P[b]) * hop
            check_wav(wav[b, :n], rows[b][0], "bf16", f"{case} row {b}", e2e=False, voc="v1" if e.get("mixed") else case)
            assert not wav[b, n:].any(), f"{case} row {b}: samples behind P x hop"
        # fusions off / forced
        for k, val in (("resstream", 0), ("rb2fuse", 0), ("pairstream", 0)):
            ctx.set_int(k, val)
        voff = _variants(ctx, lambda: ctx.vocode_mel(mel, P))
        _log(case, "launches [bf16, fusions off]", repr(dict(sorted(voff.items()))))
        off = _dev(ctx.vocode_mel, mel, P)
        assert not [n for n in voff if n.startswith(("resstream_", "rb2fuse_", "pairstream_"))], voff
        assert np.array_equal(off, wav), (case, float(np.abs(off - wav).max()))
        for k, val in (("resstream", 1), ("rb2fuse", 1), ("pairstream", 3 if e.get("mixed") else 1)):
            ctx.set_int(k, val)
        if e.get("mixed"):
            vforce = _variants(ctx, lambda: ctx.vocode_mel(mel, P))
            _log(case, "launches [bf16, pairstream 3]", repr(dict(sorted(vforce.items()))))
            forced = _dev(ctx.vocode_mel, mel, P)
            assert [n for n in vforce if n.startswith("pairstream_")], vforce
            assert np.array_equal(forced, wav), (case, float(np.abs(forced - wav).max()))
            ctx.set_int("pairstream", 1)
        alone = _dev(ctx.vocode_mel, mel[1:2, :1], P[1:2])
        assert np.array_equal(alone[0, :hop], wav[1, :hop])
        # routing
        for prefix in e.get("absent", ()):
            assert not [n for n in v if n.startswith(prefix)], (prefix, v)
        assert v == G.LAUNCHES[case]["bf16"], v
    finally:
        ctx.close()
