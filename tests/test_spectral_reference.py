"""Host-side checks of tests/spectral_ref.py: the references and bounds that tests/test_spectral_gpu.py holds dn_fft, the denoiser and the
watermark kernels to would reject a kernel that is subtly wrong.  Each mutation is applied to a restatement of the KERNEL's own
structure (fft_r4, pipeline32, bands32, search_model: no device), and must leave the unmutated reference's bound in at least one case of
the tables the device runs; the unmutated restatement must stay inside every bound.  The margins of rule (c) are computed and printed
here for every dense case; a device run reads nothing that these functions did not produce from the references."""
import contextlib

import numpy as np
import pytest

import denoise_ref as D
import spectral_ref as S
import watermark_ref as W
from denoise_window_ref import frame_range, reach


def _unrejected(mutations, rejected):
    left = [m for m in mutations if m not in rejected]
    assert not left, f"no case rejects: {left}"


# ---- the FFT ----------------------------------------------------------------------------------------------------------------------
def _probe_verdict(log2n, inverse, got, x):
    """None, or which of (c) / (d) the transform `got` of the dense probe input x leaves"""
    mg = S.probe_margin(log2n, inverse)
    e = got.astype(np.complex128) - S.fft64(x, inverse)
    if not S._rms(e) <= mg.rms_limit:
        return "rms"
    if not float(np.abs(e).max()) <= mg.max_limit:
        return "largest element"
    if not np.all(np.linalg.norm(e, axis=-1) <= S.ct_cap(x, 1 << log2n)):
        return "cap"
    return None


def test_fft_margins_and_the_kernels_ordering():
    for log2n in S.PROBE_LOG2N:
        for inverse in (False, True):
            mg = S.probe_margin(log2n, inverse)
            print(mg.line(f"fft log2n {log2n} {'inverse' if inverse else 'forward'}"))
            assert 0 < mg.m < 1.0                            # the two orderings differ, by less than their own size
            x = S.probe_dense(log2n, 0)
            assert _probe_verdict(log2n, inverse, S.fft_r4(x, inverse), x) is None, (log2n, inverse)


def test_fft_structured_inputs_on_the_kernels_ordering():
    """what the device test asserts of dn_fft holds for its restatement: the exact expectations bit for bit, the rest under the cap"""
    for log2n in S.PROBE_LOG2N:
        N = 1 << log2n
        for name, (x, exact) in S.probe_structured(log2n).items():
            for inverse in (False, True):
                y = S.fft_r4(x, inverse)
                if exact is not None:
                    assert np.array_equal(y, exact), (log2n, name, inverse)
                assert np.all(np.linalg.norm(y - S.fft64(x, inverse), axis=-1) <= S.ct_cap(x, N)), (log2n, name, inverse)
        x = S.probe_dense(log2n, 0)
        X = S.fft_r4(x, False)
        back = S.fft_r4(X, True) * np.float32(1.0 / N)
        assert np.all(np.linalg.norm(back - x, axis=-1) <= S.round_trip_cap(x, X)), log2n


def test_fft_mutations_are_rejected():
    rejected = {}
    for mut in S.FFT_MUTATIONS:
        for log2n in S.PROBE_LOG2N:
            for inverse in (False, True):
                x = S.probe_dense(log2n, 0)
                why = _probe_verdict(log2n, inverse, S.fft_r4(x, inverse, mut), x)
                if why:
                    rejected.setdefault(mut, []).append((log2n, inverse, why))
    for mut, cases in rejected.items():
        print(f"MUTATION {mut}: rejected by {len(cases)} of {2 * len(S.PROBE_LOG2N)} probe cases, first {cases[0]}")
    _unrejected(S.FFT_MUTATIONS, rejected)
    # the structured inputs reject them under the cap alone
    for mut in S.FFT_MUTATIONS:
        hit = False
        for log2n in (5, 6):
            for name, (x, _) in S.probe_structured(log2n).items():
                for inverse in (False, True):
                    e = np.linalg.norm(S.fft_r4(x, inverse, mut) - S.fft64(x, inverse), axis=-1)
                    hit = hit or bool(np.any(e > S.ct_cap(x, 1 << log2n)))
        assert hit, mut


# ---- k_wm_search --------------------------------------------------------------------------------------------------------------------
def test_search_cases_premises_and_ties():
    chunked = 0
    for cs in S.SEARCH_CASES:
        rows, sg = S.search_data(cs)
        assert S.search_premise(rows), (cs["name"], "not exact-sum data")
        assert set(np.unique(sg)) <= {-1, 1} and sg.shape == (cs["P"], cs["J"])
        ref = S.search_ref(cs)                               # asserts: ties are identical (v, dd) pairs, no near tie
        ties = [t for r in ref for _, _, t in r]
        print(f"SEARCH {cs['name']}: (P, TB, JD) = ({cs['P']}, {cs['TB']}, {cs['JD']}), F {cs['Fs']}, WF {cs['WF']}, "
              f"{'chunks: ' + str(cs['chunks']) if cs['chunks'] > 1 else 'one chunk'}, offsets attaining the maximum per window {ties}")
        chunked += cs["chunks"] > 1
        if cs.get("tie"):
            assert all(t >= 2 for t in ties), (cs["name"], ties)         # the constructed ties are ties in the float64 reference
        assert S.search_agrees(cs, S.search_model(cs), ref) is None, cs["name"]
    assert chunked >= 3
    assert S.search_case("two_chunks")["chunks"] == 2 and S.search_case("eleven_chunks")["chunks"] == 11 and S.search_case("uneven_slices")["chunks"] == 2


def test_search_mutations_are_rejected():
    rejected = {}
    for cs in S.SEARCH_CASES:
        ref = S.search_ref(cs)
        for mut in S.SEARCH_MUTATIONS:
            why = S.search_agrees(cs, S.search_model(cs, mut), ref)
            if why:
                rejected.setdefault(mut, []).append(cs["name"])
    for mut, cases in rejected.items():
        print(f"MUTATION {mut}: rejected by {cases}")
    _unrejected(S.SEARCH_MUTATIONS, rejected)
    assert all(S.search_case(n)["chunks"] > 1 for n in rejected["chunk_last_band_dropped"])


# ---- k_wm_bands ---------------------------------------------------------------------------------------------------------------------
def _bands_verdict(cs, mut=None):
    worst = 0.0
    for b, r in enumerate(S.bands_rows(cs, 0)):
        ref, tol = S.bands_tolerance(r, cs)
        got = S.bands32(r, cs, mut=mut).astype(np.float64)
        with np.errstate(invalid="ignore"):
            e = np.abs(got - ref)
            if not np.all(e <= tol):
                return f"row {b}", worst
        if (tol > 0).any():
            worst = max(worst, float(np.max(e[tol > 0] / tol[tol > 0])))
    return None, worst


def test_bands_tolerance_and_mutations():
    rejected = {}
    for cs in S.BANDS_CASES:
        per = S.POINTS // cs["n_fft"]
        assert per * cs["J"] <= S.POINTS // 2 and cs["k_lo"] + cs["J"] * cs["KB"] <= cs["n_fft"] // 2
        mg = S._bands_delta(cs["name"])
        why, worst = _bands_verdict(cs)
        print(mg.line(f"bands {cs['name']} spectrum") + f"; the kernel's ordering uses {worst:.3f} of D's tolerance")
        assert why is None, (cs["name"], why)
        for mut in S.BANDS_MUTATIONS:
            if _bands_verdict(cs, mut)[0]:
                rejected.setdefault(mut, []).append(cs["name"])
    for mut, cases in rejected.items():
        print(f"MUTATION {mut}: rejected by {cases}")
    _unrejected(S.BANDS_MUTATIONS, rejected)


# ---- the frame pipeline behind the C-ABI --------------------------------------------------------------------------------------------
def _embed_verdict(geom, small, mut=None, kind=None):
    n_fft, hop, wl = geom
    mg = S.embed_margin(n_fft, hop, wl, small)
    p = S.wm_params(n_fft, small)
    errs = []
    for r in S.case_rows(n_fft, hop, 0):
        ref = W.embed(r, S.KEY, n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, **p)
        got = S.pipeline32(r, n_fft, hop, wl, S.embed_gain(S.KEY, p, n_fft, S.RATE, mut if kind == "gain" else None), S.fft_r4,
                           mut if kind == "pipe" else None)
        errs.append((got - ref) / S.ola_scale(len(r), n_fft, hop, wl))
    e = np.concatenate(errs)
    return (S._rms(e) > mg.rms_limit or float(np.abs(e).max()) > mg.max_limit), S._rms(e) / mg.rms_limit, float(np.abs(e).max()) / mg.max_limit


def test_pipeline_margins_and_mutations():
    rejected = {}
    for geom in S.GEOMETRIES:
        for small in (False, True):
            mg = S.embed_margin(*geom, small)
            bad, r, m = _embed_verdict(geom, small)
            print(mg.line(f"embed {geom} {'small' if small else 'default'}") + f"; the kernel's ordering: rms {r:.3f}, largest element {m:.3f} of the limit")
            assert not bad, (geom, small, r, m)
            for mut in S.PIPE_MUTATIONS + S.EMBED_MUTATIONS:
                if _embed_verdict(geom, small, mut, "pipe" if mut in S.PIPE_MUTATIONS else "gain")[0]:
                    rejected.setdefault(mut, []).append((geom, small))
    for geom in S.DENOISE_GEOMETRIES:
        mg = S.denoise_margin(*geom)
        rows, bias = S.denoise_case_data(*geom, 0)
        worst = {}
        for mut in [None] + S.PIPE_MUTATIONS:
            e = np.concatenate([(S.pipeline32(r, *geom, S.denoise_gain(bias, 2.0, 0.1), S.fft_r4, mut) - D.denoise(r, bias, np.float32(2.0), np.float32(0.1), *geom))
                                / S.ola_scale(len(r), *geom) for r in rows])
            worst[mut] = (S._rms(e) / mg.rms_limit, float(np.abs(e).max()) / mg.max_limit)
            if mut and max(worst[mut]) > 1:
                rejected.setdefault(mut, []).append((geom, "denoise"))
        print(mg.line(f"denoise {geom}") + f"; the kernel's ordering: rms {worst[None][0]:.3f}, largest element {worst[None][1]:.3f} of the limit")
        assert max(worst[None]) <= 1, (geom, worst[None])
    for mut, cases in rejected.items():
        print(f"MUTATION {mut}: rejected by {len(cases)} cases, first {cases[0]}")
    # dc_nyquist_imag_kept cannot be observed (spectral_ref.EQUIVALENT): it changes the result by rounding alone
    assert S.EQUIVALENT == {"dc_nyquist_imag_kept"} and "dc_nyquist_imag_kept" not in rejected
    _unrejected([m for m in S.PIPE_MUTATIONS + S.EMBED_MUTATIONS if m not in S.EQUIVALENT], rejected)


@pytest.mark.parametrize("geom", S.GEOMETRIES, ids=lambda g: "%d_%d_%d" % g)
def test_detector_margins(geom):
    """rule (c) on the z of every offset of every window; the kernel's ordering stays inside it"""
    n_fft, hop, wl = geom
    mg = S.detect_margin(n_fft, hop, wl)
    p = S.WM_P256
    kw = {k: v for k, v in p.items() if k != "depth_db"}
    worst = 0.0
    for r in S.detect_rows(n_fft, hop, wl, 0):
        for wf in S.detect_wfs(n_fft, hop):
            zs = W.detect(r, S.KEY, window_frames=wf, n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, full=True, **kw)[3]
            worst = max([worst] + [float(np.abs(a - b).max()) for a, b in zip(S.detect32(r, S.KEY, p, n_fft, hop, wl, S.RATE, wf, S.fft_r4), zs)])
    print(mg.line(f"detect {geom} period_blocks 256") + f"; the kernel's ordering: largest element {worst / mg.max_limit:.3f} of the limit")
    assert worst <= mg.max_limit


def test_frame_index_without_f_first_is_rejected():
    """a window that begins late in the signal: the gain of frame f follows the SIGNAL's frame index; counted from the window's first
    frame it is the gain of another block, and the result leaves the case's largest-element limit"""
    n_fft, hop, wl = S.GEOMETRIES[0]
    p = S.WM_SMALL
    x = S.case_rows(n_fft, hop, 0)[2]
    whole = W.embed(x, S.KEY, n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, **p)
    o = 4 * hop + 5
    begin, cnt = o + reach(n_fft), len(x) - o - reach(n_fft)
    F = D.geometry(len(x), n_fft, hop)[1]
    f_lo = frame_range(begin, cnt, n_fft, hop, F)[0]
    assert f_lo % (p["block_frames"] * p["period_blocks"]) != 0, f_lo

    @contextlib.contextmanager
    def shifted(by):
        real = W.bin_gain
        W.bin_gain = lambda key, f, *a: real(key, f - by, *a)
        try:
            yield
        finally:
            W.bin_gain = real
    kw = dict(n_fft=n_fft, hop=hop, win_length=wl, rate=S.RATE, **p)
    got = W.embed_window(x[o:], S.KEY, o, begin, cnt, True, **kw)
    assert np.max(np.abs(got - whole[begin:])) < 1e-12
    with shifted(f_lo):
        mutated = W.embed_window(x[o:], S.KEY, o, begin, cnt, True, **kw)
    limit = S.embed_margin(n_fft, hop, wl, True).max_limit
    assert np.max(np.abs(mutated - whole[begin:]) / S.ola_scale(len(x), n_fft, hop, wl)[begin:]) > limit


@pytest.mark.parametrize("n_fft", [256, 4096])
def test_restatements_are_float32_and_independent(n_fft):
    x = S.probe_dense(n_fft.bit_length() - 1, 1)
    a, b = S.fft_r2(x), S.fft_scipy(x)
    assert a.dtype == b.dtype == np.complex64 and not np.array_equal(a, b)
    assert S._rms(a - b) < 4 * S.probe_margin(n_fft.bit_length() - 1, False).e_ref
