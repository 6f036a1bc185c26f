"""Front-end shapes outside the two named configurations (config.medium_modelcfg, config.reduced_modelcfg) against the oracle: the
routing layer of zvx.hip (read_config, fft_block, variance_predictor, run_encode, decoder_fs2, decoder_styletts, spkemb_from_mels) turns
ANY modelcfg into launches, and every branch of it is walked here by one entry of frontend_ref.SWEEP.

CPU part: the oracle against the fixtures the reference itself produced at every shape of the table (tests/golden/sweep_<case>.npz); the
oracle's discrete decisions sit off their rounding boundaries; the refusals of pack_model.
GPU part (-m gpu): per case either parity with the oracle or a refusal at pack_model AND at zvx_create that names the field -- a silently
wrong tensor and "launch_gemm rejected shape" are the outcomes that fail.
  f32 context   the deciding check: every row of a ragged batch against its own batch-1 oracle call at check_f32's 2e-4 x max(1, max|ref|),
                mel_len exact, predicted durations / bucket ids exact off the rounding boundaries, three ragged speaker embeddings
  16-bit        finite; check_mel / check_embed16 / check_f32 (encoder side), unchanged; poison_pads; every front-end fusion switched off
                relates to the default as the pairwise tests of test_gpu_parity.py state; the kernel families of frontend_ref.ROUTING and
                the launch counts of frontend_ref.LAUNCHES
ZVX_SWEEP_LOG=<file>: every comparison appends what it measured (profiles/frontend_shape_sweep.txt is such a file).

Oracle against the reference's fixtures, max|oracle - golden| / max(1, max|golden|) per tensor, measured over the table (weights seed 0):
worst 2.785e-06 (mel of h128_sty_mels64); speaker embedding worst 1.192e-07.  Asserted at 4 x the worst -- the generator sweep's margin: a
wrong tap, padding or head split is O(1), f32 summation order is what remains (profiles/frontend_shape_sweep.txt).
"""
import hashlib
import os

import numpy as np
import pytest

import frontend_ref as FR
from oracle import zvx_oracle as O                      # checker only
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = list(FR.SWEEP)
RUNNING = [c for c in CASES if FR.runs(c, "f32")]
REFUSED = [(c, p) for c in CASES for p in ("f32", "bf16") if not FR.runs(c, p)]
FIXTURES = [c for c in CASES if FR.has_fixture(c)]
SEED = 0                                                # of the weights (the fixtures' weight_seed)

ORACLE_REL = 4 * 2.785e-06                              # see the header

_cache = {}


def _log(case, what, *vals):
    line = f"{case} | {what} | " + " ".join(v if isinstance(v, str) else f"{v:.3e}" for v in vals)
    print(line)
    path = os.environ.get("ZVX_SWEEP_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _model(case):
    """(modelcfg, tts state dict, generator config, generator state dict) of a case: computed once, shared, never modified"""
    if ("model", case) not in _cache:
        cfg = FR.modelcfg(case)
        h = zcfg.hifigan_config(FR.VOC)
        _cache["model", case] = (cfg, zw.tts_state_dict(cfg, SEED), h, zw.hifigan_state_dict(h, SEED, FR.voc_mels(case)))
    return _cache["model", case]


def _packed(case, prec):
    cfg, sd, h, hsd = _model(case)
    return pack.pack_model(cfg, sd, h, hsd, prec)


def _oracle_rows(case):
    """per row of the case's ragged batch its own batch-1 oracle calls: forced durations (encoder, variance adaptor, mel), predicted
    durations (the discrete decisions) and the speaker embedding of the row's reference mel"""
    if ("rows", case) not in _cache:
        cfg, sd, _, _ = _model(case)
        x = FR.inputs(case)
        rows = []
        for b, T in enumerate(x["T"]):
            ph, pu, spk = x["phoneme"][b, :T], x["puncts"][b, :T], x["spk"][b]
            forced = O.fs2_encoder(ph, pu, spk, sd, cfg, duration=x["duration"][b, :T])
            forced["mel"] = O.mel_decoder(forced["features"], spk, sd, cfg)
            pred = O.fs2_encoder(ph, pu, spk, sd, cfg)
            emb = O.resnet_se34v2(x["ref_mels"][b, :x["ref_lens"][b]], sd, cfg)
            rows.append(dict(forced=forced, pred=pred, embed=emb))
        _cache["rows", case] = (x, rows)
    return _cache["rows", case]


def _safe(pred, n_bins):
    """_durations_and_buckets' margins (test_gpu_parity.py) with n_bins - 1 in place of 255: a rounding boundary closer than 1e-3 would
    make the discrete outcome legitimately ambiguous in fp32"""
    safe_p = np.abs((pred["pitch"] * (n_bins - 1)) % 1 - 0.5) > 1e-3
    safe_e = np.abs((pred["energy"] * (n_bins - 1)) % 1 - 0.5) > 1e-3
    safe_d = np.abs((np.exp(pred["log_duration"]) - 1) % 1 - 0.5) > 1e-3
    return safe_p, safe_e, safe_d


# ------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIXTURES)
def test_oracle_agrees_with_the_reference_fixture(case):
    """Every entry of the table the reference can run -- the refused ones too -- on row 0 of the case's batch and its 97-frame reference
    mel: the fixture's inputs are the seeded ones, and every captured tensor agrees to f32 summation order."""
    g = np.load(os.path.join(GOLDEN, "sweep_" + case + ".npz"))
    x, rows = _oracle_rows(case)
    T = int(x["T"][0])
    assert np.array_equal(g["phoneme"], x["phoneme"][0, :T]) and np.array_equal(g["puncts"], x["puncts"][0, :T])
    assert np.array_equal(g["duration"], x["duration"][0, :T]) and np.array_equal(g["spk"], x["spk"][0]) and int(g["seed"]) == SEED
    ref_mel = np.ascontiguousarray(x["ref_mels"][0, :x["ref_lens"][0]])
    assert hashlib.sha256(ref_mel.tobytes()).hexdigest() == str(g["ref_mel_sha256"])
    o = rows[0]["forced"]
    assert int(g["mel_len"]) == o["mel_len"] == int(np.maximum(x["duration"][0, :T], 0).sum()) < 60
    got = dict(encoder_raw=o["encoder_out"] - x["spk"][0][None], features=o["features"], pitch=o["pitch"], energy=o["energy"],
               log_duration=o["log_duration"], mel=o["mel"].T, embed=rows[0]["embed"])
    errs = {}
    for k, a in got.items():
        assert a.shape == g[k].shape, (k, a.shape, g[k].shape)
        errs[k] = float(np.abs(a.astype(np.float64) - g[k]).max() / max(1.0, float(np.abs(g[k]).max())))
    _log(case, "oracle vs reference, max|err|/max(1,max|ref|): " + " ".join(errs), *errs.values())
    assert max(errs.values()) <= ORACLE_REL, errs


@pytest.mark.parametrize("case", RUNNING)
def test_oracle_discrete_decisions_sit_off_their_rounding_boundaries(case):
    """The predicted-duration call of the GPU part compares bucket ids and durations on the `safe` positions only; asserted from the oracle
    alone, so that a later change of inputs cannot hollow that check out: at least 0.8 of every row's phonemes are safe for each decision
    (the one-phoneme row: its only one)."""
    cfg, _, _, _ = _model(case)
    x, rows = _oracle_rows(case)
    nb = cfg["model"]["encoder"]["ve_n_bins"]
    for b, r in enumerate(rows):
        shares = [float(s.mean()) for s in _safe(r["pred"], nb)]
        _log(case, f"row {b}: safe share pitch, energy, duration; predicted mel_len", *shares, float(r["pred"]["mel_len"]))
        assert min(shares) >= 0.8, (case, b, shares)
        assert 0 < r["pred"]["mel_len"] < 400


@pytest.mark.parametrize("case,prec", REFUSED)
def test_pack_model_refuses_by_naming_the_field(case, prec):
    field = FR.SWEEP[case]["refused"][prec][0]
    with pytest.raises(ValueError, match=field):
        _packed(case, prec)


@pytest.mark.parametrize("case", RUNNING)
def test_pack_model_packs_every_running_case(case):
    for prec in ("f32", "bf16"):
        if FR.runs(case, prec):
            man, blob = _packed(case, prec)
            assert f"cfg hidden {FR.hidden(case)}\n" in man and 1 << 18 < blob.nbytes < 64 << 20, (case, prec, blob.nbytes)


def test_check_model_config_refuses_other_malformed_front_ends():
    ok = zcfg.reduced_modelcfg("fastspeech2")
    for kind in ("styletts", "fastspeech2"):
        for prec in ("bf16", "f32"):
            pack.check_model_config(zcfg.medium_modelcfg(kind), prec, 80)
            pack.check_model_config(zcfg.reduced_modelcfg(kind), prec, 80)

    def changed(path, value):
        import copy
        cfg = copy.deepcopy(ok)
        d = cfg
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
        return cfg

    for field, path, value in (("n_head", ("model", "decoder", "n_head"), 3), ("fs2_head", ("model", "encoder", "fs2_head"), 0),
                               ("n_head", ("model", "decoder", "n_head"), 8),                      # depth 4
                               ("conv_kernel_size", ("model", "decoder", "conv_kernel_size"), [9, 2]),
                               ("conv_kernel_size", ("model", "decoder", "conv_kernel_size"), [9]),
                               ("vp_filter_size", ("model", "encoder", "vp_filter_size"), 0), ("ve_n_bins", ("model", "encoder", "ve_n_bins"), 1),
                               ("num_mels", ("audio", "num_mels"), 136), ("num_filters", ("model", "resnet", "num_filters"), [8, 8, 16, 20]),
                               ("num_filters", ("model", "resnet", "num_filters"), [8, 8, 16, 264]), ("num_filters", ("model", "resnet", "num_filters"), [8, 8, 16]),
                               ("layers", ("model", "resnet", "layers"), [1, 1, 0, 1])):
        with pytest.raises(ValueError, match=field):
            pack.check_model_config(changed(path, value), "bf16", 80)
    with pytest.raises(ValueError, match="conv_pre"):
        pack.check_model_config(ok, "bf16", 40)
    pack.check_model_config(changed(("model", "decoder", "conv_filter_size"), 68), "f32", 80)


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


def _manifest_value(cfg, key):
    """the value pack_model writes for a cfg key of the manifest"""
    m = cfg["model"]
    v = {"hidden": m["emb_dim"] + m["punct_emb_dim"], "enc_heads": m["encoder"]["fs2_head"], "ffn_k": m["decoder"]["conv_kernel_size"],
         "vp_dim": m["encoder"]["vp_filter_size"], "vp_k": m["encoder"]["vp_kernel_size"], "ffn_dim": m["decoder"]["conv_filter_size"],
         "n_mels": cfg["audio"]["num_mels"]}[key]
    return ",".join(str(int(k)) for k in v) if isinstance(v, (list, tuple)) else str(int(v))


def _check_refused_at_create(case, prec):
    """zvx_create on a manifest written by hand (pack_model refuses the config): the packed manifest of the reduced model -- the table's
    neighbour on every axis -- with the offending cfg line replaced.  The refusal names the key, and the process goes on working."""
    field, key, status = FR.SWEEP[case]["refused"][prec]
    near = zcfg.reduced_modelcfg(FR.SWEEP[case]["kind"])
    h = zcfg.hifigan_config(FR.VOC)
    man, blob = pack.pack_model(near, zw.tts_state_dict(near, SEED), h, zw.hifigan_state_dict(h, SEED), prec)
    old, new = f"cfg {key} {_manifest_value(near, key)}\n", f"cfg {key} {_manifest_value(FR.modelcfg(case), key)}\n"
    assert man.count(old) == 1 and old != new
    bad = man.replace(old, new)
    B, T, H = 1, 4, near["model"]["emb_dim"] + near["model"]["punct_emb_dim"]
    ids, spk = np.ones((B, T), np.int32), np.full((B, H), H ** -0.5, np.float32)
    if status == "ENCODE":                                                      # zvx_create takes it, the first zvx_encode refuses, before any launch
        ctx = _dev(_lib.Context, bad, blob, 0)
        try:
            with pytest.raises(_lib.ZvxError) as ei:
                _dev(ctx.encode, ids, ids, np.array([T], np.int32), spk, ids)
            assert ei.value.code == _lib.ZVX_E_UNSUPPORTED and field in str(ei.value), str(ei.value)
        finally:
            ctx.close()
    else:
        with pytest.raises(_lib.ZvxError) as ei:
            _dev(_lib.Context, bad, blob, 0)
        assert ei.value.code == getattr(_lib, "ZVX_E_" + status) and key in str(ei.value), str(ei.value)
    _log(case, f"refusal [{prec}]", str(ei.value))
    ctx = _dev(_lib.Context, man, blob, 0)                                      # the library is still usable
    try:
        mel_len, logd, _, _ = _dev(ctx.encode, ids, ids, np.array([T], np.int32), spk, ids)
        assert int(mel_len[0]) == T and np.isfinite(logd).all()
    finally:
        ctx.close()


def _front_end(ctx, x, forced=True):
    """encode (forced or predicted durations) + decode of the case's ragged batch -> dict of what the context hands back"""
    B, Tmax = x["phoneme"].shape
    H = x["spk"].shape[1]
    mel_len, logd, pitch, energy = _dev(ctx.encode, x["phoneme"], x["puncts"], x["T"], x["spk"], x["duration"] if forced else None)
    Lmax = int(mel_len.max())
    out = dict(mel_len=mel_len, log_duration=logd, pitch=pitch, energy=energy, Lmax=Lmax,
               encoder_out=_dev(ctx.fetch, "encoder_out", (B, Tmax, H)).copy(), features=_dev(ctx.fetch, "features", (B, Lmax, H)).copy())
    if not forced:
        for k, name in (("pitch_idx", "pitch_idx"), ("energy_idx", "energy_idx"), ("duration", "duration")):
            out[k] = _dev(ctx.fetch, name, (B, Tmax)).copy()
    out["mel"] = _dev(ctx.decode, B, Lmax).copy()
    return out


def _valid(out, x, key):
    """the rows of a per-utterance tensor that hold an utterance's own values, concatenated over the batch"""
    n = out["mel_len"] if key in ("mel", "features") else x["T"]
    return np.concatenate([np.asarray(out[key][b, :n[b]]).reshape(int(n[b]), -1) for b in range(len(n))])


def _check_routing(case, prec, v, vspk):
    r = FR.ROUTING[case]
    for prefix in r.get("present", {}).get(prec, ()):
        assert [n for n in v if n.startswith(prefix)], (case, prec, "missing", prefix, v)
    for prefix in r.get("absent", {}).get(prec, ()):
        assert not [n for n in v if n.startswith(prefix)], (case, prec, "unexpected", prefix, v)
    assert v == FR.LAUNCHES[case][prec]["front"], (case, prec, v)
    assert vspk == FR.LAUNCHES[case][prec]["spk"], (case, prec, vspk)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_frontend_shape_in_f32_equals_the_oracle_or_is_refused(case):
    """The deciding check.  Each row of the ragged batch T = (13, 1, 7) against its own batch-1 oracle call: mel_len exact; encoder output,
    features, pitch, energy, log-duration and mel at check_f32's 2e-4 x max(1, max|ref|); rows behind an utterance's end read zero; the
    speaker embeddings of three ragged reference mels (NaN behind a clip's end) at the same; with predicted durations the bucket ids,
    durations and mel_len on the safe positions, as _durations_and_buckets compares them."""
    from test_gpu_parity import check_f32, stats
    if not FR.runs(case, "f32"):
        with pytest.raises(ValueError):
            _packed(case, "f32")
        return _check_refused_at_create(case, "f32")
    cfg, _, _, _ = _model(case)
    x, rows = _oracle_rows(case)
    man, blob = _packed(case, "f32")
    ctx = _dev(_lib.Context, man, blob, 0)
    try:
        v = _variants(ctx, lambda: _front_end(ctx, x))
        _log(case, "launches [f32]", repr(dict(sorted(v.items()))))
        out = _front_end(ctx, x)
        keys = ("encoder_out", "features", "pitch", "energy", "log_duration", "mel")
        for b, r in enumerate(rows):
            o, T = r["forced"], int(x["T"][b])
            ml = o["mel_len"]
            assert int(out["mel_len"][b]) == ml, (case, b, out["mel_len"][b], ml)
            ref = dict(o, mel=o["mel"])
            got = {k: out[k][b, :(ml if k in ("features", "mel") else T)] for k in keys}
            figs = [stats(got[k], ref[k])[0] / max(1.0, stats(got[k], ref[k])[3]) for k in keys]
            _log(case, f"f32 row {b} (T {T}, L {ml}) max err / max(1, max|ref|): " + " ".join(keys), *figs)
        for b, r in enumerate(rows):
            o, T = r["forced"], int(x["T"][b])
            ml = o["mel_len"]
            for k in keys:
                n = ml if k in ("features", "mel") else T
                check_f32(out[k][b, :n], o[k], f"{case} row {b} {k}")
            assert not out["mel"][b, ml:].any() and not out["log_duration"][b, T:].any(), f"{case} row {b}: values behind the utterance's end"
        vspk = _variants(ctx, lambda: ctx.spkemb(x["ref_mels"], x["ref_lens"]))
        _log(case, "speaker encoder launches [f32]", repr(dict(sorted(vspk.items()))))
        emb = _dev(ctx.spkemb, x["ref_mels"], x["ref_lens"])
        for b, r in enumerate(rows):
            _log(case, f"f32 embedding {b} ({int(x['ref_lens'][b])} frames): max err, |norm - 1|", stats(emb[b], r["embed"])[0], abs(float(np.linalg.norm(emb[b])) - 1.0))
        for b, r in enumerate(rows):
            check_f32(emb[b], r["embed"], f"{case} embedding {b}")
        # predicted durations: the discrete decisions
        pr = _front_end(ctx, x, forced=False)
        nb = cfg["model"]["encoder"]["ve_n_bins"]
        for b, r in enumerate(rows):
            o, T = r["pred"], int(x["T"][b])
            safe_p, safe_e, safe_d = _safe(o, nb)
            safe_e = safe_e & (pr["pitch_idx"][b, :T] == o["pitch_idx"])              # energy sees the pitch-embedded input
            assert np.array_equal(pr["pitch_idx"][b, :T][safe_p], o["pitch_idx"][safe_p]), (case, b)
            assert np.array_equal(pr["energy_idx"][b, :T][safe_e], o["energy_idx"][safe_e]), (case, b)
            assert np.array_equal(pr["duration"][b, :T][safe_d], o["duration"][safe_d]), (case, b)
            if safe_d.all() and safe_p.all() and safe_e.all():
                assert int(pr["mel_len"][b]) == o["mel_len"], (case, b)
            if safe_d.all() and safe_p.all() and safe_e.all() and T > 1:             # (one phoneme over several frames: nothing to be exact against, frontend_ref.inputs)
                check_f32(pr["mel"][b, :o["mel_len"]], O.mel_decoder(o["features"], x["spk"][b], _model(case)[1], cfg), f"{case} row {b} mel, predicted durations")
        _check_routing(case, "f32", v, vspk)
    finally:
        ctx.close()


def _check_mel16(case, got, ref, what, dec16):
    """check_mel, unchanged: its kind "bf16" for a decoder that computes in bf16 (no case of the table needed a limit of its own)"""
    from test_gpu_parity import check_mel
    check_mel(got, ref, "bf16", what, "bf16" if dec16 == "bf16" else FR.SWEEP[case]["kind"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_frontend_shape_in_16_bit_stays_in_its_limits_and_relates_to_its_switches(case):
    """The 16-bit context of every case (the f32 comparison above is the correctness check; these limits guard regressions), every row
    against its own batch-1 oracle call:
      * every value finite; mel within check_mel, unchanged -- its kind "bf16" where the table says the decoder computes in bf16 (an FS2
        decoder off head depth 264); the encoder-side tensors within check_f32, as test_e2e_against_reference_golden holds them in both
        modes; mel_len exact; embeddings within check_embed16;
      * zvx_set_int("poison_pads", 1) leaves the mel unchanged to the bit (test_decoder_padding_rows_never_reach_a_result);
      * switched off, each front-end fusion relates to the default as its pairwise test in test_gpu_parity.py states: attn_f32 0 within
        2e-4 x max(1, max|.|) on the encoder output; enc_split 0 (exact-f32 encoder) within check_f32 of the oracle; flash 0 and dec_f16 0
        within check_mel's kind "bf16" of the oracle (the FS2 decoder, for which check_mel states it), flash 0 within 2e-2 + 4e-2 of the default; dec_flat 0 and slab_small 0 bit-equal;
        dec_sc_fuse 0 within 1.5e-2; speaker encoder: spk_pool_fuse 0 within 1.5e-3, slab_small 2 | 32 within 1e-6 of that, spk_s2_fuse 0
        within 1.5e-3;
      * the kernel families of frontend_ref.ROUTING, the launch counts of frontend_ref.LAUNCHES, and the launches dec_sc_fuse saves."""
    from test_gpu_parity import check_embed16, check_f32, stats
    e = FR.SWEEP[case]
    if not FR.runs(case, "bf16"):
        with pytest.raises(ValueError):
            _packed(case, "bf16")
        return _check_refused_at_create(case, "bf16")
    x, rows = _oracle_rows(case)
    man, blob = _packed(case, "bf16")
    ctx = _dev(_lib.Context, man, blob, 0)
    sty = e["kind"] == "styletts"
    try:
        v = _variants(ctx, lambda: _front_end(ctx, x))
        _log(case, "launches [bf16]", repr(dict(sorted(v.items()))))
        out = _front_end(ctx, x)
        enc_keys = ("encoder_out", "features", "pitch", "energy", "log_duration")
        for k in enc_keys + ("mel",):
            assert np.isfinite(out[k]).all(), (case, k)
        for b, r in enumerate(rows):
            o, T = r["forced"], int(x["T"][b])
            ml = o["mel_len"]
            assert int(out["mel_len"][b]) == ml
            figs = [stats(out[k][b, :(ml if k == "features" else T)], o[k])[0] for k in enc_keys]
            mx, rms, ref_rms, _ = stats(out["mel"][b, :ml], o["mel"])
            _log(case, f"16-bit row {b} (T {T}, L {ml}) max err: " + " ".join(enc_keys) + "; mel max err, rms err, ref rms, rms share", *figs, mx, rms, ref_rms, rms / ref_rms)
        for b, r in enumerate(rows):
            o, T = r["forced"], int(x["T"][b])
            ml = o["mel_len"]
            for k in enc_keys:
                check_f32(out[k][b, :(ml if k == "features" else T)], o[k], f"{case} row {b} {k}")
            _check_mel16(case, out["mel"][b, :ml], o["mel"], f"{case} row {b} mel", e["dec16"])
            assert not out["mel"][b, ml:].any()
        # padding rows never reach a result
        try:
            ctx.set_int("poison_pads", 1)
            p1 = _front_end(ctx, x); p2 = _front_end(ctx, x)
        finally:
            ctx.set_int("poison_pads", 0)
        assert np.isfinite(_valid(p1, x, "mel")).all(), f"{case}: NaN reached an utterance"
        assert np.array_equal(_valid(p1, x, "mel"), _valid(out, x, "mel")) and np.array_equal(_valid(p2, x, "mel"), _valid(out, x, "mel")), f"{case}: mel depends on padding rows"
        # the fusions, switched off one at a time
        def off(key, value, restore):
            try:
                ctx.set_int(key, value)
                voff = _variants(ctx, lambda: _front_end(ctx, x))
                return _front_end(ctx, x), voff
            finally:
                ctx.set_int(key, restore)

        a0, va = off("attn_f32", 0, 1)
        d = float(np.abs(_valid(a0, x, "encoder_out") - _valid(out, x, "encoder_out")).max())
        _log(case, "16-bit attn_f32 0 vs default, encoder output: max diff", d)
        assert not [n for n in va if n.startswith("attention_f32")] and d <= 2e-4 * max(1.0, float(np.abs(_valid(out, x, "encoder_out")).max())), (case, d)
        s0, _ = off("enc_split", 0, 2)
        for b, r in enumerate(rows):
            check_f32(s0["encoder_out"][b, :x["T"][b]], r["forced"]["encoder_out"], f"{case} row {b} encoder_out, enc_split 0")
        for key in ("dec_flat", "slab_small"):
            z, _ = off(key, 0, {"dec_flat": 1, "slab_small": 2}[key])
            assert np.array_equal(_valid(z, x, "mel"), _valid(out, x, "mel")), (case, key, float(np.abs(_valid(z, x, "mel") - _valid(out, x, "mel")).max()))
        h0, vh = off("dec_f16", 0, 1)
        assert not [n for n in vh if n.startswith("flash_attention_f16")], vh
        assert np.isfinite(_valid(h0, x, "mel")).all()
        for b, r in enumerate(rows):
            mx, rms, ref_rms, _ = stats(h0["mel"][b, :r["forced"]["mel_len"]], r["forced"]["mel"])
            _log(case, f"16-bit dec_f16 0 row {b}: mel max err, rms err, ref rms", mx, rms, ref_rms)
            if not sty:                                  # (check_mel states its bf16 limits for the FS2 decoder; StyleTTS in bf16 is its 7e-2 floor, why it runs in half)
                _check_mel16(case, h0["mel"][b, :r["forced"]["mel_len"]], r["forced"]["mel"], f"{case} row {b} mel, dec_f16 0", "bf16")
        if not sty:
            f0, vf = off("flash", 0, 1)
            assert not [n for n in vf if n.startswith("flash_attention")], vf
            for b, r in enumerate(rows):
                _check_mel16(case, f0["mel"][b, :r["forced"]["mel_len"]], r["forced"]["mel"], f"{case} row {b} mel, flash 0", "bf16")
            d = float(np.abs(_valid(f0, x, "mel") - _valid(out, x, "mel")).max())
            _log(case, "16-bit flash 0 vs default, mel: max diff", d)
            assert d <= 2e-2 + 4e-2, (case, d)
        else:
            c0, vc = off("dec_sc_fuse", 0, 1)
            d = float(np.abs(_valid(c0, x, "mel") - _valid(out, x, "mel")).max())
            saved = sum(vc.values()) - sum(v.values())
            _log(case, "16-bit dec_sc_fuse 0 vs default, mel: max diff; launches saved by the fusion", d, float(saved))
            assert d <= 1.5e-2, (case, d)
            assert saved == FR.ROUTING[case]["sc_fused"], (case, saved, v, vc)
        # speaker encoder
        vspk = _variants(ctx, lambda: ctx.spkemb(x["ref_mels"], x["ref_lens"]))
        _log(case, "speaker encoder launches [bf16]", repr(dict(sorted(vspk.items()))))
        emb = _dev(ctx.spkemb, x["ref_mels"], x["ref_lens"])
        assert np.isfinite(emb).all()
        for b, r in enumerate(rows):
            cos = float(np.dot(emb[b], r["embed"]) / (np.linalg.norm(emb[b]) * np.linalg.norm(r["embed"])))
            _log(case, f"16-bit embedding {b} ({int(x['ref_lens'][b])} frames): 1 - cosine, max err", 1.0 - cos, stats(emb[b], r["embed"])[0])
        for b, r in enumerate(rows):
            check_embed16(emb[b], r["embed"], f"{case} embedding {b}")
        try:
            ctx.set_int("spk_pool_fuse", 0); e_pass = _dev(ctx.spkemb, x["ref_mels"], x["ref_lens"])
            ctx.set_int("slab_small", 2 | 32); e_old = _dev(ctx.spkemb, x["ref_mels"], x["ref_lens"])
            ctx.set_int("slab_small", 2); ctx.set_int("spk_s2_fuse", 0); e_s2 = _dev(ctx.spkemb, x["ref_mels"], x["ref_lens"])
        finally:
            ctx.set_int("spk_pool_fuse", 1); ctx.set_int("slab_small", 2); ctx.set_int("spk_s2_fuse", 1)
        d1, d2, d3 = float(np.abs(emb - e_pass).max()), float(np.abs(e_pass - e_old).max()), float(np.abs(e_s2 - e_pass).max())
        _log(case, "16-bit embeddings: fused pool vs pool pass, persistent vs per-tile kernels, fused level transition vs two launches", d1, d2, d3)
        assert d1 <= 1.5e-3 and d2 <= 1e-6 and d3 <= 1.5e-3, (case, d1, d2, d3)
        _check_routing(case, "bf16", v, vspk)
    finally:
        ctx.close()
