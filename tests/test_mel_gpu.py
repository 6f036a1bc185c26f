"""Spec-level tests of the log-mel front end on the MI355X (zvx_melspec; mel_from_padded in csrc/zvx.hip, the analysis zvx_spkemb_wav runs
inside enrolment) against the float64 reference of tests/mel_ref.py at every STFT geometry of its table.  Every bound is derived there
from the reference's own intermediates; nothing is tuned against the kernels.  Per geometry one ragged batch (mel_ref.case_rows) with
NaN behind every row's end and an odd Nmax, behind a longer call on the same context: frames exact, every element of every row within
its bound, silent frames and empty filters at log(1e-5), rows past a row's frames all-zero bits at both a tight and a loose Tmax, each
row alone bit-equal to itself in the batch, the sentinel behind `mel` untouched.  A geometry the device does not run is refused by name
at pack_model and at zvx_create.  Each case prints `SPEC mel <case> worst err/bound ...` (profiles/mel_frontend_spec.txt).  A HIP error
ends the session."""

import numpy as np
import pytest

import mel_ref as MR
import test_spectral_gpu as TS
from zerovox_amd import _lib, config as zcfg

pytestmark = pytest.mark.gpu

SENT = np.uint32(0xFFFFFFFF)
GUARD = 16
_AUDIO0 = zcfg.reduced_modelcfg("styletts")["audio"]


def ctx_of(case):
    """ctx_at's context of the case's geometry: one per geometry, cached there (the shipped geometry is the denoiser tests' context)"""
    g = MR.geom(case)
    audio = {k: g[k] for k in MR.FIELDS[3:] if g[k] != _AUDIO0[k]}
    ctx = _dev(TS.ctx_at, g["fft_size"], g["hop_size"], g["win_length"], **audio)
    assert ctx.get_int("fft_size") == g["fft_size"] and ctx.hop == g["hop_size"] and ctx.n_mels == g["num_mels"]
    assert ctx.get_int("sampling_rate") == g["sampling_rate"]
    return ctx


def _dev(fn, *a, **kw):
    """A HIP error ends the session: nothing more is started on a device that faulted."""
    try:
        return fn(*a, **kw)
    except _lib.ZvxError as e:
        if e.code == _lib.ZVX_E_HIP:
            pytest.exit(f"HIP error: {e}", returncode=3)
        raise


def melspec(ctx, x, n, Tmax):
    """the raw call on x [B][Nmax] (NaN behind the rows) -> (status, mel bits [B * Tmax * n_mels + GUARD] that started as the sentinel,
    frames [B] that started as -7)"""
    B, Nmax = x.shape
    assert x.dtype == np.float32 and x.flags.c_contiguous and n.dtype == np.int32
    mel = np.full(B * Tmax * ctx.n_mels + GUARD, SENT, np.uint32)
    frames = np.full(B, -7, np.int32)
    rc = ctx._lib.zvx_melspec(ctx._h, _lib._ptr(x), _lib._ptr(n), B, Nmax, _lib._ptr(mel), Tmax, _lib._ptr(frames))
    if rc == _lib.ZVX_E_HIP:
        pytest.exit(f"HIP error: {ctx._lib.zvx_last_error(ctx._h).decode()}", returncode=3)
    return rc, mel, frames


def err(ctx):
    return ctx._lib.zvx_last_error(ctx._h).decode()


@pytest.mark.parametrize("case", MR.RUNNING)
def test_melspec_at_geometry(case):
    g = MR.geom(case)
    nm, hop = g["num_mels"], g["hop_size"]
    ctx = ctx_of(case)
    rows, ref = MR.case_rows(case), MR.case_ref(case)
    x, n = MR.batch(rows)
    B = len(rows)
    want = np.array([MR.frames_of(k, g) for k in n], np.int32)
    Tf = int(want.max())
    # a longer and wider call first: the rows handed back below must not carry its work buffers
    big = np.ones((B + 1, int(n.max()) + 5 * hop), np.float32)
    rc, _, _ = melspec(ctx, big, np.full(B + 1, big.shape[1], np.int32), MR.frames_of(big.shape[1], g))
    assert rc == 0, err(ctx)
    kept = None
    for Tmax in (Tf, Tf + 3):
        rc, bits, frames = melspec(ctx, x, n, Tmax)
        assert rc == 0, err(ctx)
        assert np.array_equal(frames, want), (frames, want)
        assert np.all(bits[B * Tmax * nm:] == SENT)                                       # the sentinel behind mel
        mel = bits[:B * Tmax * nm].reshape(B, Tmax, nm)
        for b in range(B):
            assert not mel[b, want[b]:].any(), (case, Tmax, b)                            # rows past the frames: all-zero bits
        if kept is None:
            kept = mel
        else:
            assert all(np.array_equal(kept[b, :want[b]], mel[b, :want[b]]) for b in range(B))   # Tmax changes no bit
    worst, at, clip_ulp, n_clip = 0.0, (0, 0, 0), 0.0, 0    # worst err/bound over the elements with energy; the exact-zero ones in ulps
    lim = MR.R.K_ULP["log"] * MR.R.ulp32(MR.LOG_LO)
    for b, (v, bd, M) in enumerate(ref):
        got = kept[b, :want[b]].view(np.float32).astype(np.float64)
        assert got.shape == v.shape
        with np.errstate(invalid="ignore"):
            e = np.abs(got - v)
            bad = ~(e <= bd)                                                              # (a NaN is out of bound)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{case} row {b} ({MR.ROW_NAMES[b]}): {int(bad.sum())} of {bad.size} elements out of bound; [frame, mel] = {i}: "
                                 f"got {got[i]!r} ref {v[i]!r} bound {bd[i]:.3g}")
        assert np.all(np.abs(got[M == 0] - MR.LOG_LO) <= lim), (case, b)                  # silent frames, empty filters: log(1e-5)
        if (M == 0).any():
            clip_ulp, n_clip = max(clip_ulp, float(np.abs(got[M == 0] - MR.LOG_LO).max() / MR.R.ulp32(MR.LOG_LO))), n_clip + int((M == 0).sum())
        r = np.where(M == 0, 0.0, e / bd)
        if r.max() > worst:
            worst, at = float(r.max()), (b,) + tuple(int(k) for k in np.unravel_index(np.argmax(r), r.shape))
    zeros = kept[MR.ROW_NAMES.index("zeros"), :want[MR.ROW_NAMES.index("zeros")]].view(np.float32)
    assert np.all(np.abs(zeros.astype(np.float64) - MR.LOG_LO) <= lim) and len(np.unique(zeros.view(np.uint32))) == 1
    # every row alone: the bits it has in the batch
    for b in range(B):
        xb = np.full((1, n[b] + (n[b] % 2 == 0)), np.nan, np.float32)
        xb[0, :n[b]] = rows[b]
        rc, bits, frames = melspec(ctx, xb, n[b:b + 1], int(want[b]))
        assert rc == 0 and frames[0] == want[b], err(ctx)
        assert np.array_equal(bits[:want[b] * nm].reshape(want[b], nm), kept[b, :want[b]]), (case, b, MR.ROW_NAMES[b])
        assert np.all(bits[want[b] * nm:] == SENT)
    empty = int((~MR.packed(case)[1].any(axis=1)).sum())
    print(f"SPEC mel {case} {MR.GEOMETRIES[case]}: frames {want.tolist()}, {sum(r[0].size for r in ref)} elements, {empty} empty filters: "
          f"worst err/bound {worst:.4f} at [row, frame, mel] = {list(at)} ({MR.ROW_NAMES[at[0]]}); {n_clip} elements of exactly zero "
          f"energy within {clip_ulp:.2f} ulp of log(1e-5) (limit {MR.R.K_ULP['log']})")


@pytest.mark.parametrize("case", MR.RUNNING)
def test_melspec_refusals_at_geometry(case):
    """A row one sample below the shortest legal length: ZVX_E_INVALID; Tmax one short of the longest row's frames: ZVX_E_BUFFER (the
    statuses include/zvx.h names).  The message names the row, nothing is written, and the context serves the next call."""
    g = MR.geom(case)
    ctx = ctx_of(case)
    rows = [MR.case_rows(case)[MR.ROW_NAMES.index(k)] for k in ("boundary", "tone+noise", "shortest")]
    x, n = MR.batch(rows)
    want = np.array([MR.frames_of(k, g) for k in n], np.int32)
    Tf = int(want.max())
    rc, good, _ = melspec(ctx, x, n, Tf)
    assert rc == 0, err(ctx)

    def refused(n_, Tmax, status, row):
        rc, bits, frames = melspec(ctx, x, n_, Tmax)
        assert rc == status, (rc, err(ctx))
        assert f"utterance {row} " in err(ctx), err(ctx)
        assert np.all(bits == SENT) and np.all(frames == -7)
    short = n.copy()
    short[2] = MR.min_len(g) - 1
    refused(short, Tf, _lib.ZVX_E_INVALID, 2)
    refused(n, Tf - 1, _lib.ZVX_E_BUFFER, 1)
    over = n.copy()
    over[0] = x.shape[1] + 1
    refused(over, Tf, _lib.ZVX_E_INVALID, 0)
    rc, again, frames = melspec(ctx, x, n, Tf)
    assert rc == 0 and np.array_equal(again, good) and np.array_equal(frames, want)


def _refused_at_create(key, value, named, status="UNSUPPORTED"):
    """zvx_create on a manifest written by hand: the packed manifest of the shipped geometry with one cfg line replaced.  The refusal
    names the key, and the library goes on working."""
    man, blob = TS.packed_at(1024, 256, 1024)
    old = f"cfg {key} {dict(fft_size=1024, n_mels=80)[key]}\n"
    assert man.count(old) == 1
    with pytest.raises(_lib.ZvxError) as ei:
        _dev(_lib.Context, man.replace(old, f"cfg {key} {value}\n"), blob, 0)
    assert ei.value.code == getattr(_lib, "ZVX_E_" + status) and named in str(ei.value), str(ei.value)
    print(f"SPEC mel refusal at zvx_create [{key} {value}]: {ei.value}")
    ctx = _dev(_lib.Context, man, blob, 0)
    try:
        mel, frames = _dev(ctx.melspec, [np.zeros(1024, np.float32)])
        assert frames[0] == 4 and mel.shape == (1, 4, 80)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", list(MR.REFUSED))
def test_refused_geometry(case):
    """A geometry of the table the device does not run: pack_model names the field (tests/test_mel_reference.py holds that on the host
    too), zvx_create the manifest's key."""
    field, key, status = MR.REFUSED[case]
    g = MR.geom(case)
    with pytest.raises(ValueError, match=field):
        TS.packed_at(g["fft_size"], g["hop_size"], g["win_length"], **{k: g[k] for k in MR.FIELDS[3:]})
    _refused_at_create(key, g["num_mels"], key, status)


@pytest.mark.parametrize("bad", [k for k, v in MR.BAD_STFT.items() if v[2]])
def test_bad_stft_refused_at_create(bad):
    """The STFT blocks pack.check_model_config refuses (tests/test_mel_reference.py), as far as the manifest carries them: fft_size
    and the hop.  win_length, fmin and fmax are no manifest keys; they reach the device only inside mel.dft and mel.basis."""
    key, value, named = MR.BAD_STFT[bad][2]
    _refused_at_create(key, value, named)
