"""Spec-level tests of the spectral family on the MI355X against tests/spectral_ref.py (its docstring states every bound; none is measured
on a device): dn_fft alone through zvxk_fft_probe at every size it accepts, k_wm_search on exact data through zvxk_wm_search (chunked
table, uneven slices, windows, ties), k_wm_bands by interval through zvxk_wm_bands, and the C-ABI (zvx_watermark, zvx_watermark_detect,
zvx_denoise) at the transform sizes the other suites leave out.  Each case prints `SPEC <case> ...`, the share of its bound the kernel
used (profiles/spectral_kernel_spec.txt).  A HIP error after a launch ends the session (_ran)."""
import ctypes

import numpy as np
import pytest

import denoise_ref as D
import kernel_ref as K
import spectral_ref as S
import watermark_ref as W

pytestmark = pytest.mark.gpu

SENT = np.uint32(0xFFFFFFFF)
F32, C64 = np.float32, np.complex64


@pytest.fixture(scope="module")
def lib():
    return K.load_ktest()


def _ran(rc, what):
    """A HIP error after a launch (the shim's -(1000 + code)) ends the session: nothing more is started on a device that faulted."""
    if rc <= -1000:
        pytest.exit(f"{what}: HIP error {-rc - 1000}", returncode=3)
    return rc


# ---- the FFT probe ------------------------------------------------------------------------------------------------------------------
def _probe(lib, x, inverse):
    """[frames][N] complex64 -> dn_fft of one launch, [frames][N] complex64 (the planes' bits as the device left them)"""
    fr, N = x.shape
    assert fr * N == S.POINTS
    dev = K.Device(lib)
    try:
        re, im = dev.upload(np.ascontiguousarray(x.real.ravel())), dev.upload(np.ascontiguousarray(x.imag.ravel()))
        tw = dev.upload(S.twiddles(N).ravel())
        assert _ran(lib.zvxk_fft_probe(re, im, tw, N.bit_length() - 1, int(inverse)), f"fft_probe N = {N}") == 0
        out = np.empty((fr, N), C64)
        out.real, out.imag = dev.download(re, S.POINTS, F32).reshape(fr, N), dev.download(im, S.POINTS, F32).reshape(fr, N)
        return out
    finally:
        dev.free()


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log2n", S.PROBE_LOG2N)
def test_fft_probe_dense(lib, log2n, inverse):
    N = 1 << log2n
    x = S.probe_dense(log2n, 0)
    mg = S.probe_margin(log2n, inverse)
    got = _probe(lib, x, inverse)
    e = got.astype(np.complex128) - S.fft64(x, inverse)
    rms, worst = S._rms(e), float(np.abs(e).max())
    cap_share = float(np.max(np.linalg.norm(e, axis=-1) / S.ct_cap(x, N)))
    print(f"SPEC fft_probe log2n {log2n} {'inverse' if inverse else 'forward'}: E_k / E_ref {rms / mg.e_ref:.3f} against 1 + m = {1 + mg.m:.3f}; "
          f"worst element / limit {worst / mg.max_limit:.3f}; norm / cap {cap_share:.4f}")
    assert rms <= mg.rms_limit, (rms, mg.rms_limit)
    assert worst <= mg.max_limit, (worst, mg.max_limit)
    assert cap_share <= 1.0


@pytest.mark.parametrize("log2n", S.PROBE_LOG2N)
def test_fft_probe_structured_round_trip_and_frame_independence(lib, log2n):
    N = 1 << log2n
    worst = 0.0
    for name, (x, exact) in S.probe_structured(log2n).items():
        for inverse in (False, True):
            y = _probe(lib, x, inverse)
            if exact is not None:                            # an impulse at t = 0: all ones; a constant: N at DC, zeros elsewhere -- exactly
                assert np.array_equal(y, exact), (name, inverse)
            share = float(np.max(np.linalg.norm(y - S.fft64(x, inverse), axis=-1) / S.ct_cap(x, N)))
            worst = max(worst, share)
            assert share <= 1.0, (name, inverse, share)
    x = S.probe_dense(log2n, 0)
    X = _probe(lib, x, False)
    back = _probe(lib, X, True) * F32(1.0 / N)
    rt = float(np.max(np.linalg.norm(back - x, axis=-1) / S.round_trip_cap(x, X)))
    assert rt <= 1.0, rt
    if x.shape[0] > 1:                                       # one frame of NaN leaves the bits of the others unchanged
        bad = x.copy()
        bad[1] = np.nan
        Y = _probe(lib, bad, False)
        keep = np.arange(x.shape[0]) != 1
        assert np.array_equal(Y[keep].view(np.uint32), X[keep].view(np.uint32)) and np.isnan(Y[1]).all()
    print(f"SPEC fft_probe log2n {log2n} structured: worst norm / cap {worst:.4f}; round trip / cap {rt:.4f}")


# ---- k_wm_search on exact data ------------------------------------------------------------------------------------------------------
def _search(lib, cs, rows, sg):
    """-> (per row a list of (score f32, offset) for the row's windows, the raw [B][NW] result bits)"""
    B = len(rows)
    nws = [len(W.windows(d.shape[0], cs["WF"])) for d in rows]
    NW = max(max(nws), 1) + 1                                # one column more than any row has windows: it keeps the sentinel
    dev = K.Device(lib)
    try:
        tab = (K.WmDetectRow * B)()
        for b, d in enumerate(rows):
            tab[b].x, tab[b].d, tab[b].n, tab[b].F = None, dev.upload(d.astype(F32).ravel()), 0, d.shape[0]
        tab_d = dev.alloc(ctypes.sizeof(tab))
        assert lib.zvxk_h2d(tab_d, ctypes.addressof(tab), ctypes.sizeof(tab)) == 0
        a = K.WmDetectArgs()
        a.rows, a.B, a.Fmax = tab_d, B, max(d.shape[0] for d in rows)
        a.sign = dev.upload(sg.astype(np.int8).ravel())
        a.J, a.TB, a.P, a.WF, a.NW = cs["J"], cs["TB"], cs["P"], cs["WF"], NW
        a.win_score, a.win_offset = dev.upload(np.full(B * NW, SENT, np.uint32)), dev.upload(np.full(B * NW, SENT, np.uint32))
        assert _ran(lib.zvxk_wm_search(ctypes.byref(a)), f"wm_search {cs['name']}") == 0
        sc = dev.download(a.win_score, B * NW, np.uint32).reshape(B, NW)
        of = dev.download(a.win_offset, B * NW, np.uint32).reshape(B, NW)
    finally:
        dev.free()
    for b in range(B):                                       # entries at or past a row's window count keep the sentinel
        assert np.all(sc[b, nws[b]:] == SENT) and np.all(of[b, nws[b]:] == SENT), (cs["name"], b)
    return [[(sc[b, w:w + 1].view(F32)[0], int(of[b, w])) for w in range(nws[b])] for b in range(B)], (sc, of)


@pytest.mark.parametrize("name", [c["name"] for c in S.SEARCH_CASES])
def test_wm_search_exact(lib, name):
    cs = S.search_case(name)
    rows, sg = S.search_data(cs)
    assert S.search_premise(rows)                            # a case that is not exact-sum data fails here, on the host
    ref = S.search_ref(cs)
    got, bits = _search(lib, cs, rows, sg)
    why = S.search_agrees(cs, got, ref)
    exact = sum(F32(z) == s for g, r in zip(got, ref) for (s, _), (z, _, _) in zip(g, r))
    total = sum(len(r) for r in ref)
    print(f"SPEC wm_search {name}: (P, TB, JD) = ({cs['P']}, {cs['TB']}, {cs['JD']}), chunks {cs['chunks']}, {total} windows: "
          f"{exact} scores are the reference's f32 value, {total - exact} its neighbour; every offset the reference's")
    assert why is None, why
    if "nan_row" in cs:                                      # the NaN row: score 0, offset 0; the others keep their bits
        b = cs["nan_row"]
        assert got[b] == [(F32(0.0), 0)]
        clean = [np.nan_to_num(d, nan=0.0) for d in rows]
        _, bits2 = _search(lib, cs, clean, sg)
        keep = np.arange(len(rows)) != b
        assert np.array_equal(bits[0][keep], bits2[0][keep]) and np.array_equal(bits[1][keep], bits2[1][keep])
    if "zero_row" in cs:
        assert got[cs["zero_row"]] == [(F32(0.0), 0)]


# ---- k_wm_bands by interval ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in S.BANDS_CASES])
def test_wm_bands_interval(lib, name):
    cs = S.bands_case(name)
    rows = S.bands_rows(cs, 0)
    n_fft, hop, JD = cs["n_fft"], cs["hop"], cs["J"] - 2
    B, GUARD = len(rows), 16
    Fs = [D.geometry(len(r), n_fft, hop)[1] for r in rows]
    dev = K.Device(lib)
    try:
        tab = (K.WmDetectRow * B)()
        dptr = []
        for b, r in enumerate(rows):
            xb = np.concatenate([r, np.full(GUARD, np.nan, F32)])                         # input past the row's end holds NaN
            dptr.append(dev.upload(np.full(Fs[b] * JD + GUARD, SENT, np.uint32)))
            tab[b].x, tab[b].d, tab[b].n, tab[b].F = dev.upload(xb), dptr[b], len(r), Fs[b]
        tab_d = dev.alloc(ctypes.sizeof(tab))
        assert lib.zvxk_h2d(tab_d, ctypes.addressof(tab), ctypes.sizeof(tab)) == 0
        a = K.WmDetectArgs()
        a.rows, a.B, a.Fmax = tab_d, B, max(Fs)
        a.n_fft, a.log2n, a.hop, a.pad = n_fft, n_fft.bit_length() - 1, hop, (n_fft - hop) // 2
        a.twid, a.win = dev.upload(S.twiddles(n_fft).ravel()), dev.upload(D.window(n_fft, n_fft).astype(F32))
        a.k_lo, a.KB, a.J = cs["k_lo"], cs["KB"], cs["J"]
        assert _ran(lib.zvxk_wm_bands(ctypes.byref(a)), f"wm_bands {name}") == 0
        got = [dev.download(dptr[b], Fs[b] * JD + GUARD, np.uint32) for b in range(B)]
    finally:
        dev.free()
    worst = 0.0
    for b, r in enumerate(rows):
        assert np.all(got[b][Fs[b] * JD:] == SENT), (name, b)                             # nothing behind the row's D
        ref, tol = S.bands_tolerance(r, cs)
        val = got[b][:Fs[b] * JD].view(F32).astype(np.float64).reshape(Fs[b], JD)
        with np.errstate(invalid="ignore"):
            e = np.abs(val - ref)
            assert np.all(e <= tol), (name, b, float(np.nanmax(e / np.maximum(tol, 1e-300))))
        silent = tol == 0
        assert not val[silent].any()                                                      # a silent frame: D is exactly 0
        if (~silent).any():
            worst = max(worst, float(np.max(e[~silent] / tol[~silent])))
    print(f"SPEC wm_bands {name}: n_fft {n_fft} hop {hop} k_lo {cs['k_lo']} KB {cs['KB']} J {cs['J']}, frames {Fs}: worst err / tol {worst:.3f}")


# ---- the C-ABI at the other transform sizes -----------------------------------------------------------------------------------------
_ctx = {}


def packed_at(n_fft, hop, wl, **audio):
    """(manifest, blob) of ctx_at's model, on the host: the reduced model config with this STFT (audio: further fields of its audio
    block -- num_mels, sampling_rate, fmin, fmax), the tiny vocoder (a hop other than its 256 gets two stages with that product; its
    conv_pre takes num_mels channels), weights seed 0"""
    from zerovox_amd import config as zcfg, pack, weights as zw
    cfg = zcfg.reduced_modelcfg("styletts")
    cfg["audio"].update(fft_size=n_fft, hop_size=hop, win_length=wl, **audio)
    h = zcfg.hifigan_config("tiny")
    if hop != 256:
        u = int(round(hop ** 0.5))
        assert u * u == hop
        k = 2 * u if u % 2 == 0 else 3 * u                   # (k - u must be even, k at most 3 u: pack.check_generator_config)
        h.update(upsample_rates=[u, u], upsample_kernel_sizes=[k, k], upsample_initial_channel=32)
    return pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0, cfg["audio"]["num_mels"]), "bf16")


def ctx_at(n_fft, hop, wl, **audio):
    """the denoiser tests' tiny synthetic context; a hop other than the tiny vocoder's 256, or other fields of the audio block, get
    packed_at's model"""
    from zerovox_amd import _lib
    if hop == 256 and not audio:
        import test_denoise_gpu as TD
        return TD.ctx_for(n_fft, hop, wl)
    key = (n_fft, hop, wl) + tuple(sorted(audio.items()))
    if key not in _ctx:
        _ctx[key] = _lib.Context(*packed_at(n_fft, hop, wl, **audio), 0)
    return _ctx[key]


def _held(name, out, refs, lens, geom, mg):
    """rule (c) on a C-ABI case: the rows' errors divided by ola_scale, rms and largest element"""
    e = np.concatenate([(out[b, :n].astype(np.float64) - refs[b]) / S.ola_scale(n, *geom) for b, n in enumerate(lens)])
    rms, worst = S._rms(e), float(np.abs(e).max())
    print(f"SPEC {name}: E_k / E_ref {rms / mg.e_ref:.3f} against 1 + m = {1 + mg.m:.3f}; worst element / limit {worst / mg.max_limit:.3f} "
          f"(limit {mg.max_limit:.3e})")
    assert rms <= mg.rms_limit, (name, rms, mg.rms_limit)
    assert worst <= mg.max_limit, (name, worst, mg.max_limit)


@pytest.mark.parametrize("small", [False, True], ids=["default", "small"])
@pytest.mark.parametrize("geom", S.GEOMETRIES, ids=lambda g: "%d_%d_%d" % g)
def test_embed_at_other_transform_sizes(geom, small):
    import test_watermark_gpu as TW
    n_fft, hop, wl = geom
    ctx = ctx_at(*geom)
    assert ctx.get_int("fft_size") == n_fft and ctx.hop == hop and ctx.get_int("sampling_rate") == S.RATE
    p = S.wm_params(n_fft, small)
    rows = S.case_rows(n_fft, hop, 0)
    x, n = TW.padded(rows)
    out = TW.run(ctx, x, n, p, key=S.KEY)
    refs = [W.embed(r, S.KEY, n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, **p) for r in rows]
    assert max(float(np.max(np.abs(r - x0))) for r, x0 in zip(refs, rows)) > 1e-3                  # the mark acts
    _held(f"embed {geom} {'small' if small else 'default'}", out, refs, n, geom, S.embed_margin(n_fft, hop, wl, small))


def lead_rule(got_windows, zs, limit, what):
    """test_detector_scores_against_the_reference's rule with the case's own bound: every window's score within `limit` of the
    reference's largest z; the offset within one frame of the reference's wherever its best leads every z more than a frame away by
    more than the bound, and equal to it where no other z comes that close -> the largest |score - ref|"""
    assert len(got_windows) == len(zs), what
    worst = 0.0
    for w, z in enumerate(zs):
        s, off = got_windows[w]
        o, T = int(np.argmax(z)), len(z)
        e = abs(s - float(z[o]))
        worst = max(worst, e)
        assert e <= limit, (what, w, e, limit)
        q = np.arange(T)
        away = np.minimum((q - o) % T, (o - q) % T) > 1
        lead = float(z[o] - z[away].max()) if away.any() else np.inf
        if lead > limit:
            assert min((off - o) % T, (o - off) % T) <= 1, (what, w, off, o)
            if np.sum(z >= z[o] - limit) == 1:
                assert off == o, (what, w, off, o)
    return worst


@pytest.mark.parametrize("geom", S.GEOMETRIES, ids=lambda g: "%d_%d_%d" % g)
def test_detect_at_other_transform_sizes(geom):
    """zvx_watermark_detect with period_blocks = 256 on rows marked by the float64 reference (the embedder is held above): the real band
    launch feeds the search, chunked wherever the geometry has more than 50 bands"""
    n_fft, hop, wl = geom
    ctx = ctx_at(*geom)
    p = S.WM_P256
    kw = {k: v for k, v in p.items() if k != "depth_db"}
    J = W.bands(p["lo_hz"], p["hi_hz"], p["band_bins"], n_fft, S.RATE)[1]
    chunks = -(-(J - 2) // min(J - 2, S.WM_TABLE // p["period_blocks"]))
    rows = S.detect_rows(n_fft, hop, wl, 0, every=True)     # min_samples, n_fft + 1 and 4 n_fft + 77 samples
    limit = S.detect_margin(n_fft, hop, wl).max_limit
    worst = 0.0
    for wf in S.detect_wfs(n_fft, hop):
        got = ctx.watermark_detect(rows, S.KEY, window_frames=wf, **kw)
        for b, r in enumerate(rows):
            score, off, win, zs = W.detect(r, S.KEY, window_frames=wf, n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, full=True, **kw)
            worst = max(worst, lead_rule(got[b].windows, zs, limit, (geom, wf, b)))
            assert abs(got[b].score - score) <= limit
            tops = sorted(float(z.max()) for z in zs)
            if len(tops) < 2 or tops[-1] - tops[-2] > limit:
                assert got[b].window == win, (geom, wf, b)
    print(f"SPEC detect {geom} period_blocks 256: J {J}, search chunks {chunks}, window_frames {S.detect_wfs(n_fft, hop)}: worst |score - ref| / limit "
          f"{worst / limit:.3f} (limit {limit:.3e})")
    assert geom != (4096, 256, 4096) or chunks > 1


@pytest.mark.parametrize("geom", S.DENOISE_GEOMETRIES, ids=lambda g: "%d_%d_%d" % g)
def test_denoise_at_other_transform_sizes(geom):
    import test_denoise_gpu as TD
    n_fft, hop, wl = geom
    ctx = ctx_at(*geom)
    assert ctx.get_int("fft_size") == n_fft and ctx.hop == hop
    rows, bias = S.denoise_case_data(n_fft, hop, wl, 0)
    n = np.array([len(r) for r in rows], np.int32)
    nmax = int(n.max())
    x = np.full((len(rows), nmax + (nmax % 2 == 0)), TD.SENTINEL32, np.uint32).view(F32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    out = TD.run(ctx, x, n, bias, 2.0, 0.1)
    assert TD.untouched(out, n)
    refs = [D.denoise(r, bias, F32(2.0), F32(0.1), n_fft, hop, wl) for r in rows]
    assert max(float(np.max(np.abs(r - x0))) for r, x0 in zip(refs, rows)) > 0.05                  # the case does subtract
    _held(f"denoise {geom}", out, refs, n, geom, S.denoise_margin(n_fft, hop, wl))
