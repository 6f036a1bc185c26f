"""Prosody control (include/zvx.h, zvx_prosody): speaking rate, pitch and energy through the C-ABI, _lib.Context, ZeroVox and ZeroVoxTTS.

The controlled variance adaptor is restated here from the oracle's own primitives (O.variance_predictor, O.bucketize,
O.length_regulate) with the header's semantics; the CPU tests pin that restatement, the Q16 duration rule and the Prosody value type,
the GPU tests (-m gpu) hold the HIP kernels to them.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import zvx_oracle as O                      # checker only
from zerovox_amd import _lib, config as zcfg, pack, synthetic, weights as zw
from zerovox_amd.prosody import Prosody, ProsodyStruct, q16_cumulative

VA = "_phoneme_encoder._variance_adaptor"
MARGIN = 1e-3                                            # rounding-ambiguity margin of test_predicted_durations_and_buckets_exact
_sd, _ctx = {}, {}


def tts_sd(kind):
    if kind not in _sd:
        cfg = zcfg.medium_modelcfg(kind)
        _sd[kind] = (cfg, zw.tts_state_dict(cfg, 0))
    return _sd[kind]


def voc_sd(name):
    if name not in _sd:
        h = zcfg.hifigan_config(name)
        _sd[name] = (h, zw.hifigan_state_dict(h, 0))
    return _sd[name]


def ctx_for(kind, voc, prec):
    key = (kind, voc, prec)
    if key not in _ctx:
        if len(_ctx) >= 3:
            _ctx.pop(next(iter(_ctx))).close()
        cfg, sd = tts_sd(kind)
        h, hsd = voc_sd(voc)
        man, blob = pack.pack_model(cfg, sd, h, hsd, prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


# ---------------------------------------------------------------------------------------------------------------- restated adaptor
def control(v, shift=None, rng=None, target=None):
    """header semantics on one utterance's predictions v [T] f32: every op a separately rounded f32 op (numpy does not contract)"""
    v = np.asarray(v, np.float32)
    if rng is not None:
        m = np.float32(v.astype(np.float64).sum() / len(v))
        v = v + (np.float32(rng) - np.float32(1)) * (v - m)
    if shift is not None:
        v = v + np.float32(shift)
    if target is not None:
        t = np.asarray(target, np.float32)
        v = np.where(np.isnan(t), v, t).astype(np.float32)
    return v


def _bucket(v, nb, hint):
    """O.bucketize; at a position within MARGIN of a rounding boundary the device's bucket (hint) is taken as the outcome"""
    idx = O.bucketize(v, nb)
    amb = np.abs((v.astype(np.float64) * (nb - 1)) % 1 - 0.5) <= MARGIN
    if hint is not None:
        idx = np.where(amb, np.asarray(hint, np.int64), idx)
    return idx, amb


def adaptor(x, sd, cfg, pshift=None, prange=None, ptarget=None, eshift=None, erange=None, etarget=None, q=None, duration=None,
            pidx_hint=None, eidx_hint=None):
    """VarianceAdaptor.forward (fs2.py:652-693) with the zvx_prosody controls of include/zvx.h; x [T][H] = encoder output + style"""
    nb = cfg["model"]["encoder"]["ve_n_bins"]
    log_d = O.variance_predictor(x, sd, VA + ".duration_predictor")
    pitch = O.variance_predictor(x, sd, VA + ".pitch_predictor")
    pv = control(pitch, pshift, prange, ptarget)
    pidx, pamb = _bucket(pv, nb, pidx_hint)
    x = x + sd[VA + ".pitch_embedding.weight"][pidx]
    energy = O.variance_predictor(x, sd, VA + ".energy_predictor")       # reads the CONTROLLED pitch embedding
    ev = control(energy, eshift, erange, etarget)
    eidx, eamb = _bucket(ev, nb, eidx_hint)
    x = x + sd[VA + ".energy_embedding.weight"][eidx]
    if duration is None:
        duration = np.maximum(np.rint(np.exp(log_d) - log_d.dtype.type(1)), 0)
    d = np.asarray(duration).astype(np.int64)
    if q is not None:
        d = q16_cumulative(d, q)[0]
    feats = O.length_regulate(x, d)
    return dict(features=feats, pitch=pitch, energy=energy, log_duration=log_d, mel_len=feats.shape[0], duration=d,
                pitch_idx=pidx, energy_idx=eidx, pitch_amb=pamb, energy_amb=eamb)


def enc_x(ph, pu, spk, sd, cfg):
    return O.encoder(ph, pu, sd, cfg) + np.asarray(spk, np.float32).reshape(1, -1)


# ---------------------------------------------------------------------------------------------------------------- CPU tests
def test_restated_adaptor_with_neutral_controls_is_the_oracle():
    cfg, sd = tts_sd("styletts")
    ph, pu, T, spk, _ = synthetic.batch(2, 20, 70, None)
    for b in range(2):
        ref = O.fs2_encoder(ph[b], pu[b], spk[b], sd, cfg)
        x = enc_x(ph[b], pu[b], spk[b], sd, cfg)
        got = adaptor(x, sd, cfg, pshift=0.0, prange=1.0, ptarget=np.full(20, np.nan), eshift=0.0, erange=1.0,
                      etarget=np.full(20, np.nan), q=np.full(20, 65536))
        for k in ("features", "pitch", "energy", "log_duration", "pitch_idx", "energy_idx", "duration"):
            assert np.array_equal(got[k], ref[k]), k
        assert got["mel_len"] == ref["mel_len"]


def test_q16_rule_hand_worked_cases():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 12, 37)
    L = int(d.sum())
    dp, Cs, ml = q16_cumulative(d, np.full(37, 65536))
    assert np.array_equal(dp, d) and ml == L and np.array_equal(Cs, np.cumsum(d))
    dp, Cs, ml = q16_cumulative(d, np.full(37, 32768))                   # speed 2
    assert ml == (L + 1) // 2
    for q in (np.full(37, 81920), rng.integers(4096, 1048577, 37), np.full(37, 4096)):
        dp, Cs, ml = q16_cumulative(d, q)
        assert dp.sum() == Cs[-1] == ml and (dp >= 0).all()
        assert abs(ml - float((d * q).sum()) / 65536) <= 0.5              # the total is exact to half a frame
    # a slowed short phoneme is not lost to per-phoneme rounding: three 1-frame phonemes at 1.5x -> 4.5 -> 5 frames (not 3 x 2 = 6 or 3)
    assert q16_cumulative([1, 1, 1], [98304] * 3)[2] == 5


def test_prosody_neutral_is_none_and_expands():
    assert Prosody.create(3, 8) is None
    assert Prosody.create(3, 8, speed=1.0, pitch_shift=0.0, pitch_range=np.ones(3), energy_target=np.full((3, 5), np.nan)) is None
    p = Prosody.create(3, 8, speed=2.0, pitch_shift=0.1)
    assert p.pitch_shift.shape == (3,) and np.allclose(p.pitch_shift, 0.1) and p.pitch_range is None
    assert p.dur_scale_q16.shape == (3, 8) and (p.dur_scale_q16 == 32768).all()
    p = Prosody.create(3, 8, speed=[0.5, 1.0, 1.25], pitch_range=[1.0, 0.5, 2.0])
    assert list(p.dur_scale_q16[:, 0]) == [131072, 65536, 52429] and p.pitch_range.dtype == np.float32
    t = np.full((3, 5), 0.25, np.float32)
    t[1, 2] = np.nan
    p = Prosody.create(3, 8, pitch_target=t, speed=np.full((3, 5), 0.8))
    assert p.pitch_target.shape == (3, 8) and np.isnan(p.pitch_target[:, 5:]).all() and np.isnan(p.pitch_target[1, 2])
    assert (p.dur_scale_q16[:, :5] == 81920).all() and (p.dur_scale_q16[:, 5:] == 65536).all()
    s = p.struct()
    assert s.pitch_target == p.pitch_target.ctypes.data and not s.pitch_shift
    # an explicitly neutral block is kept by the constructor (it reaches the C side)
    n = Prosody(3, 8, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0, pitch_target=np.nan,
                energy_target=np.nan, dur_scale_q16=65536)
    assert not n.is_neutral() and all(getattr(n.struct(), f) for f, _ in ProsodyStruct._fields_)


@pytest.mark.parametrize("kw", [dict(pitch_shift=np.nan), dict(energy_shift=[0.0, np.inf]), dict(pitch_range=4.5), dict(energy_range=-0.1),
                                dict(speed=20.0), dict(speed=[1.0, 1 / 17]), dict(pitch_target=1.5), dict(dur_scale_q16=4095),
                                dict(pitch_shift=[0.1, 0.2, 0.3])])
def test_prosody_rejects_bad_values_before_any_library_call(kw, monkeypatch):
    def no_lib():
        raise AssertionError("library touched")
    monkeypatch.setattr(_lib, "load", no_lib)
    with pytest.raises(ValueError):
        Prosody.create(2, 6, **kw)


# ---------------------------------------------------------------------------------------------------------------- GPU tests
PRECS = ["f32", "bf16"]


def _neutral_struct(B, Tmax):
    keep = dict(ps=np.zeros(B, np.float32), pr=np.ones(B, np.float32), es=np.zeros(B, np.float32), er=np.ones(B, np.float32),
                pt=np.full((B, Tmax), np.nan, np.float32), et=np.full((B, Tmax), np.nan, np.float32), q=np.full((B, Tmax), 65536, np.int32))
    s = ProsodyStruct(*(keep[k].ctypes.data for k in ("ps", "pr", "es", "er", "pt", "et", "q")))
    return s, keep


def _raw_synth(ctx, ph, pu, T, spk, dur, Lmax, pros):
    """zvx_synthesize(_ex) straight through ctypes: (wav, mel, mel_len, log_duration)"""
    B, Tmax = ph.shape
    wav = np.zeros((B, Lmax * ctx.hop), np.float32)
    mel = np.zeros((B, Lmax, ctx.n_mels), np.float32)
    ml = np.zeros(B, np.int32)
    logd = np.zeros((B, Tmax), np.float32)
    p = _lib._ptr
    args = (ctx._h, p(ph), p(pu), p(dur), p(T), B, Tmax, p(spk), None, Lmax, p(wav), wav.shape[1], p(ml), p(mel), Lmax, p(logd), 0)
    lib = ctx._lib
    ctx._chk(lib.zvx_synthesize(*args) if pros is None else lib.zvx_synthesize_ex(*args, C.byref(pros)))
    return wav, mel, ml, logd


def _taps(ctx, B, Tmax):
    return {w: ctx.fetch(w, (B, Tmax)) for w in ("pitch_idx", "energy_idx", "duration", "pitch", "energy", "log_duration")}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("forced", [False, True])
def test_neutral_block_is_bit_identical(prec, forced):
    ctx = ctx_for("styletts", "tiny", prec)
    ph, pu, T, spk, dur = synthetic.batch(3, 20, 70, "uniform" if forced else None)
    T[1] = 13
    s, _keep = _neutral_struct(3, 20)
    a = _raw_synth(ctx, ph, pu, T, spk, dur, 2000, None)
    ta = _taps(ctx, 3, 20)
    enc_a = ctx.fetch("encoder_out", (3, 20, ctx.hidden))
    b = _raw_synth(ctx, ph, pu, T, spk, dur, 2000, s)
    tb = _taps(ctx, 3, 20)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    assert np.array_equal(enc_a, ctx.fetch("encoder_out", (3, 20, ctx.hidden)))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("forced", [False, True])
def test_speed_is_exact(prec, forced):
    ctx = ctx_for("styletts", "tiny", prec)
    ph, pu, T, spk, dur = synthetic.batch(3, 20, 70, "uniform" if forced else None)
    T[2] = 15
    cap = 4000
    base = ctx.synthesize(ph, pu, T, spk, dur, Lmax_cap=cap)
    d0 = ctx.fetch("duration", (3, 20)).astype(np.int64)
    rng = np.random.default_rng(5)
    cases = [dict(speed=s) for s in (0.5, 0.8, 1.25, 2.0)] + [dict(dur_scale_q16=rng.integers(20000, 150000, (3, 20)))]
    for kw in cases:
        p = Prosody.create(3, 20, **kw)
        out = ctx.synthesize(ph, pu, T, spk, dur, Lmax_cap=cap, prosody=p)
        dtap = ctx.fetch("duration", (3, 20)).astype(np.int64)
        exp_d = np.zeros((3, 20), np.int64)
        for b in range(3):
            dp, _, ml = q16_cumulative(d0[b, :T[b]], p.dur_scale_q16[b, :T[b]])
            exp_d[b, :T[b]] = dp
            assert int(out["mel_len"][b]) == ml, (kw, b)
        assert np.array_equal(dtap, exp_d), kw
        ref = ctx.synthesize(ph, pu, T, spk, exp_d.astype(np.int32))
        L = int(out["mel_len"].max())
        assert np.array_equal(out["mel"][:, :L], ref["mel"][:, :L]), kw
        assert np.array_equal(out["wav"][:, :L * ctx.hop], ref["wav"][:, :L * ctx.hop]), kw
    assert np.array_equal(base["mel_len"], ctx.synthesize(ph, pu, T, spk, dur, Lmax_cap=cap)["mel_len"])


def _check_close(a, b, prec, what, mel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mx, bm = float(np.abs(a - b).max()), float(np.abs(b).max())
    if prec == "f32":
        assert mx <= 2e-4 * max(1.0, bm), f"{what}: {mx:.3e}"
        return
    rms, ref_rms = float(np.sqrt(np.mean((a - b) ** 2))), float(np.sqrt(np.mean(b ** 2)))
    lim_mx, lim_rms = (2e-2, 0.004 * ref_rms) if mel else (4e-3, 8e-4)   # test_gpu_parity check_mel / check_wav (all-half generator)
    assert mx <= lim_mx and rms <= lim_rms, f"{what}: max {mx:.3e} rms {rms:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_pitch_and_energy_controls_against_the_oracle(prec):
    ctx = ctx_for("styletts", "tiny", prec)
    cfg, sd = tts_sd("styletts")
    ph, pu, T, spk, _ = synthetic.batch(3, 20, 70, None)
    ctl = dict(pitch_shift=[0.05, -0.1, 0.2], pitch_range=[1.5, 0.0, 0.7], energy_shift=[-0.03, 0.08, 0.0], energy_range=[0.5, 2.0, 1.3])
    ctx.encode(ph, pu, T, spk, prosody=ctl)
    tp = _taps(ctx, 3, 20)
    for b in range(3):
        x = enc_x(ph[b], pu[b], spk[b], sd, cfg)
        r = adaptor(x, sd, cfg, pshift=ctl["pitch_shift"][b], prange=ctl["pitch_range"][b], eshift=ctl["energy_shift"][b],
                    erange=ctl["energy_range"][b])
        assert np.array_equal(tp["pitch_idx"][b][~r["pitch_amb"]], r["pitch_idx"][~r["pitch_amb"]])
        safe_e = ~r["energy_amb"] & (tp["pitch_idx"][b] == r["pitch_idx"])
        assert safe_e.mean() >= 0.8
        assert np.array_equal(tp["energy_idx"][b][safe_e], r["energy_idx"][safe_e])
        assert np.abs(tp["pitch"][b] - r["pitch"]).max() <= 2e-4 * max(1, np.abs(r["pitch"]).max())   # outputs stay the raw predictions
    # end to end on the FS2 decoder, forced durations: mel and waveform against the restated adaptor + the oracle's decoder / vocoder
    ctx = ctx_for("fastspeech2", "tiny", prec)
    cfg, sd = tts_sd("fastspeech2")
    h, hsd = voc_sd("tiny")
    ph, pu, T, spk, dur = synthetic.batch(2, 16, 3, "uniform")
    ctl = dict(pitch_shift=[0.1, -0.05], pitch_range=[1.8, 0.3], energy_shift=[0.05, 0.0], energy_range=[1.0, 2.5])
    out = ctx.synthesize(ph, pu, T, spk, dur, prosody=ctl)
    tp = _taps(ctx, 2, 16)
    for b in range(2):
        x = enc_x(ph[b], pu[b], spk[b], sd, cfg)
        r = adaptor(x, sd, cfg, pshift=ctl["pitch_shift"][b], prange=ctl["pitch_range"][b], eshift=ctl["energy_shift"][b],
                    erange=ctl["energy_range"][b], duration=dur[b], pidx_hint=tp["pitch_idx"][b], eidx_hint=tp["energy_idx"][b])
        assert np.array_equal(tp["pitch_idx"][b], r["pitch_idx"]) and np.array_equal(tp["energy_idx"][b], r["energy_idx"])
        ml = r["mel_len"]
        assert int(out["mel_len"][b]) == ml
        mel = O.mel_decoder(r["features"], spk[b], sd, cfg)
        wav = O.hifigan_generator(mel.T, hsd, h)
        _check_close(out["mel"][b, :ml], mel, prec, "mel", True)
        _check_close(out["wav"][b, :ml * 256], wav[:ml * 256], prec, "wav", False)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_targets_at_bucket_centres_reproduce_and_moved_targets_drive_energy(prec):
    ctx = ctx_for("styletts", "tiny", prec)
    cfg, sd = tts_sd("styletts")
    nb = cfg["model"]["encoder"]["ve_n_bins"]
    ph, pu, T, spk, _ = synthetic.batch(3, 20, 70, None)
    T[0] = 11
    cap = 1200
    base = ctx.synthesize(ph, pu, T, spk, None, Lmax_cap=cap)
    tb = _taps(ctx, 3, 20)
    tgt = dict(pitch_target=(tb["pitch_idx"] / np.float32(nb - 1)).astype(np.float32),
               energy_target=(tb["energy_idx"] / np.float32(nb - 1)).astype(np.float32))
    for kw in (dict(pitch_target=tgt["pitch_target"]), tgt):
        out = ctx.synthesize(ph, pu, T, spk, None, Lmax_cap=cap, prosody=kw)
        for k in ("wav", "mel", "mel_len", "log_duration"):
            assert np.array_equal(out[k], base[k]), k
        t2 = _taps(ctx, 3, 20)
        for k in tb:
            assert np.array_equal(t2[k], tb[k]), k
    # pitch targets that move buckets: the energy prediction follows the controlled pitch embedding
    moved = np.clip(tb["pitch_idx"] + 40, 0, nb - 1) / np.float32(nb - 1)
    moved[:, ::3] = np.nan                                               # every third phoneme keeps its prediction
    ctx.encode(ph, pu, T, spk, prosody=dict(pitch_target=moved.astype(np.float32)))
    tm = _taps(ctx, 3, 20)
    assert not np.array_equal(tm["energy"], tb["energy"])
    for b in range(3):
        n = T[b]
        x = enc_x(ph[b, :n], pu[b, :n], spk[b], sd, cfg)
        r = adaptor(x, sd, cfg, ptarget=moved[b, :n], pidx_hint=tm["pitch_idx"][b, :n])
        assert np.array_equal(tm["pitch_idx"][b, :n][~r["pitch_amb"]], r["pitch_idx"][~r["pitch_amb"]])
        assert np.abs(tm["energy"][b, :n] - r["energy"]).max() <= 2e-4 * max(1, np.abs(r["energy"]).max())
        safe = ~r["energy_amb"]
        assert np.array_equal(tm["energy_idx"][b, :n][safe], r["energy_idx"][safe])


def _ragged_controls():
    rng = np.random.default_rng(11)
    pt = np.full((4, 24), np.nan, np.float32)
    pt[2, 3:9] = np.linspace(0.2, 0.9, 6)
    return dict(pitch_shift=[0.0, 0.1, -0.2, 0.05], pitch_range=[1.0, 2.0, 0.5, 0.0], energy_shift=[0.1, 0.0, -0.05, 0.0],
                energy_range=[0.8, 1.0, 1.5, 3.0], pitch_target=pt, dur_scale_q16=rng.integers(20000, 150000, (4, 24)))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ragged_batch_rows_equal_batch1_calls(prec):
    ctx = ctx_for("styletts", "tiny", prec)
    ph, pu, T, spk, _ = synthetic.batch(4, 24, 40, None)
    T[:] = [24, 9, 17, 5]
    ctl = _ragged_controls()
    cap = 4000
    p = Prosody.create(4, 24, **ctl)
    out = ctx.synthesize(ph, pu, T, spk, None, Lmax_cap=cap, prosody=p)
    tp = _taps(ctx, 4, 24)
    for b in range(4):
        one = dict(pitch_shift=ctl["pitch_shift"][b], pitch_range=ctl["pitch_range"][b], energy_shift=ctl["energy_shift"][b],
                   energy_range=ctl["energy_range"][b], pitch_target=ctl["pitch_target"][b:b + 1], dur_scale_q16=ctl["dur_scale_q16"][b:b + 1])
        o1 = ctx.synthesize(ph[b:b + 1], pu[b:b + 1], T[b:b + 1], spk[b:b + 1], None, Lmax_cap=cap, prosody=one)
        t1 = _taps(ctx, 1, 24)
        ml = int(out["mel_len"][b])
        assert int(o1["mel_len"][0]) == ml
        assert np.array_equal(out["mel"][b, :ml], o1["mel"][0, :ml])
        assert np.array_equal(out["wav"][b, :ml * ctx.hop], o1["wav"][0, :ml * ctx.hop])
        for k in tp:
            assert np.array_equal(tp[k][b], t1[k][0]), (b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_queued_paths_with_controls(prec):
    ctx = ctx_for("styletts", "tiny", prec)
    ph, pu, T, spk, dur = synthetic.batch(3, 20, 70, "uniform")
    ctl = dict(pitch_shift=[0.1, 0.0, -0.1], pitch_range=[1.5, 1.0, 0.5], dur_scale_q16=np.full((3, 20), 52429))
    p = Prosody.create(3, 20, **ctl)
    ref = ctx.synthesize(ph, pu, T, spk, dur, prosody=p)
    lens = p.scaled_lengths(dur, T)
    assert np.array_equal(ref["mel_len"], lens)
    Lmax = int(lens.max())
    n = Lmax * ctx.hop
    wptr = ctx.dev_alloc(3 * n * 4)
    try:
        q = ctx.synthesize(ph, pu, T, spk, dur, want_mel=False, wav_device_ptr=wptr, wav_stride=n, no_sync=True, prosody=p)
        assert np.array_equal(q["mel_len"], lens)                         # filled on the host, before the GPU has finished
        ctx.sync()
        assert np.array_equal(ctx.dev_to_host(wptr, (3, n), np.float32), ref["wav"][:, :n])
    finally:
        ctx.dev_free(wptr)
    a = ctx.synthesize(ph, pu, T, spk, dur, want_mel=False, host_async=True, prosody=p)
    assert np.array_equal(a["mel_len"], lens)
    rows = ctx.wait_host(a["slot"])
    assert np.array_equal(rows, ref["wav"][:, :rows.shape[1]]) and rows.shape[1] == n


@pytest.mark.gpu
def test_invalid_controls_and_overlong_slowdown():
    ctx = ctx_for("styletts", "tiny", "bf16")
    ph, pu, T, spk, dur = synthetic.batch(2, 12, 3, "uniform")
    bad = [dict(pitch_shift=np.array([np.nan, 0], np.float32)), dict(energy_range=np.array([1.0, 4.5], np.float32)),
           dict(pitch_target=np.full((2, 12), 1.2, np.float32)), dict(dur_scale_q16=np.full((2, 12), 2_000_000, np.int32))]
    for kw in bad:
        keep = {k: np.ascontiguousarray(v) for k, v in kw.items()}
        s = ProsodyStruct(**{k: v.ctypes.data for k, v in keep.items()})
        with pytest.raises(_lib.ZvxError) as e:
            _raw_synth(ctx, ph, pu, T, spk, dur, 200, s)
        assert e.value.code == _lib.ZVX_E_INVALID, kw
    # the next valid call equals one on a fresh context
    got = ctx.synthesize(ph, pu, T, spk, dur, prosody=dict(speed=1.25, pitch_shift=0.1))
    cfg, sd = tts_sd("styletts")
    h, hsd = voc_sd("tiny")
    fresh = _lib.Context(*pack.pack_model(cfg, sd, h, hsd, "bf16"), 0)
    try:
        want = fresh.synthesize(ph, pu, T, spk, dur, prosody=dict(speed=1.25, pitch_shift=0.1))
    finally:
        fresh.close()
    for k in ("wav", "mel", "mel_len", "log_duration"):
        assert np.array_equal(got[k], want[k]), k
    L0 = int(ctx.encode(ph, pu, T, spk)[0].max())
    assert ctx.synthesize(ph, pu, T, spk, None, Lmax_cap=L0 + 1)["mel_len"].max() == L0
    with pytest.raises(_lib.ZvxError) as e:
        ctx.synthesize(ph, pu, T, spk, None, Lmax_cap=L0 + 1, prosody=dict(speed=1 / 16))
    assert e.value.code == _lib.ZVX_E_BUFFER


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_host_api_keywords(prec):
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision=prec)
    rng = np.random.default_rng(2)
    spk = rng.standard_normal(528).astype(np.float32)
    spk /= np.linalg.norm(spk)
    text = "hello world, this is a test of the speaking rate."
    synth.model._min_mel_len = 2                                         # no vocoder padding: tts and tts_stream see the same frames
    w0, p0, l0, m0 = synth.tts_ex(text, spk[None, None])
    synth.model._min_mel_len = 2
    w1, p1, l1, m1 = synth.tts_ex(text, spk[None, None], speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0)
    assert l0 == l1 and np.array_equal(w0, w1) and np.array_equal(m0, m1)
    synth.model._min_mel_len = 2
    _, _, l2, _ = synth.tts_ex(text, spk[None, None], speed=2.0)
    assert l2 == (l0 + 1) // 2
    synth.model._min_mel_len = 2
    w3, _, l3 = synth.tts(text, spk[None, None], speed=0.8, pitch_range=1.4)
    assert l3 > l0
    got = np.concatenate(list(synth.tts_stream(text, spk[None, None], chunk_frames=40, speed=0.8, pitch_range=1.4)))
    assert got.shape == w3.shape
    if prec == "bf16":
        assert np.array_equal(got, w3)
    else:
        assert np.abs(got - w3).max() <= 1e-5
    assert synth.tts_ex("", spk[None, None], speed=2.0)[2] == 0           # the empty-text sentinel is unchanged


@pytest.mark.gpu
def test_launch_sequence_lists_new_kernels_only_with_controls():
    ctx = ctx_for("styletts", "tiny", "bf16")
    ph, pu, T, spk, dur = synthetic.batch(2, 16, 3, "uniform")
    new = {"bucket_embed_add_ctl", "durations_q16"}
    ctx.set_int("profile", 2)
    try:
        ctx.reset_stats()
        ctx.synthesize(ph, pu, T, spk, dur)
        names0 = {k["name"] for k in ctx.kernel_stats()}
        tags0 = {t["name"]: t["launches"] for t in ctx.tag_stats()}
        assert not names0 & new
        ctx.reset_stats()
        ctx.synthesize(ph, pu, T, spk, dur, prosody=dict(speed=1.5, pitch_shift=0.1, energy_range=0.5))
        ks = {k["name"]: k["launches"] for k in ctx.kernel_stats()}
        tags1 = {t["name"]: t["launches"] for t in ctx.tag_stats()}
        assert ks.get("bucket_embed_add_ctl") == 2 and ks.get("durations_q16") == 1
        assert tags1["variance"] == tags0["variance"] + 2 and tags1["lenreg"] == tags0["lenreg"] + 1
        ctx.reset_stats()
        ctx.synthesize(ph, pu, T, spk, dur)
        assert not {k["name"] for k in ctx.kernel_stats()} & new
    finally:
        ctx.set_int("profile", 0)
