"""Spec-level tests of the conv-GEMM launcher (launch_gemm / launch_resfuse / launch_rb2fuse) and the two fused attention kernels
against the float64 reference of tests/kernel_ref.py, driven through the test shim libzvx_ktest.so with hand-built descriptors.

Per element, |kernel - ref| <= bound, with the bound of kernel_ref (fp32 accumulation 2 n 2^-24 sum|x w|, epilogue 2^-22 sum of
magnitudes, + half an ulp of the output type at |ref| plus the bound itself; fused kernels add one ulp of their 16-bit intermediate
propagated through |W2| and the residual; flash adds 2^-8 (bf16) / 2^-11 (f16) relative for its 16-bit probabilities).
Output / accumulator / shortcut buffers start as a sentinel bit pattern that every element the contract does not write must keep;
input rows, keys and columns the contract masks hold NaN.

The streaming ResBlock kernels -- launch_resstream (StreamArgs), launch_narrowstage (StageArgs) and launch_pairstream past one
segment -- are held to kernel_ref.chain_ref, a float64 chain with the 16-bit roundings where the kernels put them:
  * exact-sum data (sparse power-of-two weights, inputs on a grid: every f32 partial sum exact, per element): the kernel must equal
    the reference's 16-bit value BIT FOR BIT wherever no rounding boundary lies within the propagated element-wise f32 roundings
    (at least 30 % of every case, asserted on the host; measured shares in profiles/stream_kernel_spec.txt), and lie within the
    propagated bound elsewhere.  Premise: a matrix instruction returns an exactly representable block sum exactly -- established
    for 32 x 32 x 16 by the conv-GEMM cases, and what the narrowstage cases measure for 16 x 16 x 32;
  * dense data: resstream bit-equal to the same chain as per-pair launch_resfuse launches (variants 16 / 17, spec-tested above);
    narrowstage and pairstream by rms against the PURE float64 chain: E_kernel <= E_reference (1 + m), m = 3 x the relative
    spread of E_reference over 8 data seeds (kernel_ref.rms_margin)."""
import numpy as np
import pytest

import kernel_ref as K

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def lib():
    return K.load_ktest()


def _effective_epi(p, vid, mode):
    """Which epilogue instantiation the launch ran.  launch_convslab (gemm.hip) hands gemm_epi_mode_of's mode to exactly two
    launch sites: the 256 x 128 tile of a 1-D launch (its tile switch and the 160-row-halo form, which only takes EPI(1,1,1)), and
    the 128 x 128 tile of a batch-flattened decoder launch (bflat hint, no slab_small), which has EPI(0,0,1) and DEC(0/1) only.
    Every other site -- the flattened 3 x 3 maps, the small-row, short-utterance and 64 x 128 forms of id 22 -- instantiates the
    run-time epilogue."""
    d = p.d
    if vid == 7 and not d.get("_flat"):
        return mode
    if vid == 22 and d["bflat"] and not d["slab_small"] and mode in (K.EPI(0, 0, 1), K.EPI_DEC0, K.EPI_DEC1):
        return mode
    return -1


def _check_buffer(name, got_bits, dt, ref, tol, mask, before_bits, may_write, split3=None):
    """Valid elements within their bound (no NaN / Inf), untouched elements bit-equal to what the buffer held before."""
    got = K.from_bits(got_bits, dt)
    if split3 is not None:
        ldo, N, pdt = split3
        idx = np.nonzero(mask)[0]
        row, col = idx // ldo, idx % ldo
        base = row * ldo + col
        hi = K.from_bits(got_bits[base], pdt)
        lo = K.from_bits(got_bits[base + 2 * N], pdt)
        assert np.array_equal(got_bits[base], got_bits[base + N]), f"{name}: the two hi planes differ"
        val = hi + lo / (2048.0 if pdt == K.DT_F16 else 1.0)
        err = np.abs(val - ref[idx])
        bad = ~(err <= tol[idx])
        assert not bad.any(), f"{name}: {bad.sum()} split-plane elements out of bound, worst err {np.nanmax(err):.3g} vs tol {tol[idx][np.argmax(err)]:.3g}"
        written = np.zeros(len(got_bits), bool)
        written[base] = written[base + N] = written[base + 2 * N] = True
        ok = written | may_write
        untouched = got_bits[~ok] == before_bits[~ok]
        assert untouched.all(), f"{name}: {(~untouched).sum()} elements outside the valid region were written"
        return float(np.max(err / np.maximum(tol[idx], 1e-300))) if len(idx) else 0.0
    err = np.abs(got[mask] - ref[mask])
    bad = ~(err <= tol[mask])
    if bad.any():
        i = np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf), -1))
        gi = np.nonzero(mask)[0][i]
        raise AssertionError(f"{name}: {bad.sum()}/{mask.sum()} elements out of bound; element {gi}: got {got[gi]!r} ref {ref[gi]!r} tol {tol[gi]:.3g}")
    keep = ~(mask | may_write)
    untouched = got_bits[keep] == before_bits[keep]
    if not untouched.all():
        gi = np.nonzero(keep)[0][np.argmin(untouched)]
        raise AssertionError(f"{name}: {(~untouched).sum()} elements outside the contract's region were written (first at {gi})")
    return float(np.max(err / np.maximum(tol[mask], 1e-300))) if mask.any() else 0.0


def _may_write(p, f):
    """Elements outside the compared region that the contract allows a launch to write (bflat / flattened maps: every row; the
    round-up-to-4 / 8 column spill; the rows a sampled comparison skips)."""
    d = p.d
    n = len(p.bufs[f]["bits"])
    mw = np.zeros(n, bool)
    ld = d["lda"] if f == "accum" else d["ldo"]
    bs = d["a_bs"] if f == "accum" else d["o_bs"]
    N = d["N"] * (3 if d["out_split3"] and f == "out" else 1)
    spill = (N + 7) & ~7 if "Wp" in p.bufs or d.get("fused") else (N + 3) & ~3
    rows_per_b = bs // ld if ld else 0
    for b in range(d["nbatch"]):
        for h in range(d["nheads"]):
            off = b * bs + h * (d["o_hs"] if f != "accum" else 0)
            if d["bflat"] or d.get("_flat") or (d["wout"] > 0 and d["stride"] == 2 and "Wp" in p.bufs):
                # batch-flattened launches, flattened maps and the stride-2 level transitions write every row of the map
                rows = np.arange(min(rows_per_b, d["M"]) if rows_per_b else d["M"])
            else:
                rows = K.valid_out_rows(d, b)                  # (2-D: only the columns < out_len of every map row)
            c = np.arange(spill)
            ix = off + rows[:, None] * ld + c[None, :]
            mw[ix[ix < n]] = True
    return mw


@pytest.mark.parametrize("entry", K.GEMM_CASES, ids=[e[0] for e in K.GEMM_CASES])
def test_gemm_case(lib, entry):
    name, kw, vid, epi = entry
    p = K.build_case(entry)
    a, _ = K.gemm_struct(p, None)
    dry = lib.zvxk_gemm(a, 1)
    assert dry == vid, f"{name}: the launcher picks variant {dry} ({lib.zvxk_variant_name(dry) if dry >= 0 else 'refused'}), the case expects {vid}"
    mode = lib.zvxk_epi_mode(a)
    if epi is not None:
        assert _effective_epi(p, vid, mode) == epi, f"{name}: epilogue {K.EPI_NAMES.get(mode, mode)}, expected {K.EPI_NAMES[epi]}"
    dev = K.Device(lib)
    try:
        a, ptr = K.gemm_struct(p, dev)
        got = lib.zvxk_gemm(a, 0)
        assert got == vid, f"{name}: launch returned {got}"
        ref = K.gemm_ref(p)
        worst, saturated = {}, 0
        for f, (r, t, m) in ref.items():
            buf = p.bufs[f]
            bits = dev.download(ptr[f], len(buf["bits"]), K.bits_dtype(buf["dt"]))
            split3 = (p.d["ldo"], p.d["N"], K.DT_F16 if p.d["out_split3"] == 2 else K.DT_BF16) if f == "out" and p.d["out_split3"] else None
            if split3:
                bits = dev.download(ptr[f], len(buf["bits"]) * 2, np.uint16)
                before = np.full(len(bits), 0xFFFF, np.uint16)
                worst[f] = _check_buffer(f"{name}.{f}", bits, split3[2], r, t, m, before, _may_write_split(p, len(bits)), split3)
                continue
            before = buf["bits"]
            worst[f] = _check_buffer(f"{name}.{f}", bits, buf["dt"], r, t, m, before, _may_write(p, f))
            if buf["dt"] == K.DT_F16 and f in p.raw:
                # half stores: never Inf; where the f32 result lies past 65520 (+ its bound) the store holds exactly +-65504
                # (pack_f16x2_sat, or a plain convert under MODE.FP16_OVFL)
                vals = K.from_bits(bits[m], K.DT_F16)
                assert not np.isinf(vals).any(), f"{name}.{f}: Inf stored"
                over = np.abs(p.raw[f][m]) >= 65520.0 + t[m]
                assert np.array_equal(vals[over], np.sign(p.raw[f][m][over]) * K.F16_MAX), f"{name}.{f}: a store past the range is not +-65504"
                saturated += int(over.sum())
        if "saturate" in name:
            assert saturated > 0, f"{name}: no half store was driven past 65504"
        print(f"{name}: variant {vid} {lib.zvxk_variant_name(vid).decode()} epi {K.EPI_NAMES.get(_effective_epi(p, vid, mode))} worst err/bound " +
              ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    finally:
        dev.free()


def _may_write_split(p, n16):
    """Split-plane outputs: rows of 3 N 16-bit elements, ldo = 3 N, stored 8-wide per plane."""
    d = p.d
    mw = np.zeros(n16, bool)
    for b in range(d["nbatch"]):
        rows = np.arange(d["M"]) if (d["bflat"] or p.sample is not None) else K.valid_out_rows(d, b)
        ix = b * d["o_bs"] + rows[:, None] * d["ldo"] + np.arange(3 * d["N"])[None, :]
        mw[ix[ix < n16]] = True
    return mw


@pytest.mark.parametrize("entry", K.ATTN_CASES, ids=[e[0] for e in K.ATTN_CASES])
def test_attention_case(lib, entry):
    name = entry[0]
    p = K.build_case(entry)
    fn = lib.zvxk_flash if p.kind == "flash" else lib.zvxk_attn_f32
    a, _ = K.attn_struct(p, None)
    assert fn(a, 1) == 1, f"{name}: the launcher declines the shape"
    dev = K.Device(lib)
    try:
        a, ptr = K.attn_struct(p, dev)
        assert fn(a, 0) == 1, f"{name}: launch failed"
        ref = K.attn_ref(p)
        d = p.d
        for f, (r, t, m) in ref.items():
            buf = p.bufs[f]
            bits = dev.download(ptr[f], len(buf["bits"]), K.bits_dtype(buf["dt"]))
            mw = np.zeros(len(bits), bool)
            if f == "out" and p.kind != "flash":
                # exact-f32 kernel: query rows of the utterance's last 32-row tile past len are written as zeros
                for b, l in enumerate(d["_lens"]):
                    hi = min(d["L"], (l + 31) // 32 * 32)
                    rows = np.arange(l, hi)
                    ix = b * d["o_bs"] + rows[:, None] * d["ldo"] + np.arange(d["nheads"] * d["D"])[None, :]
                    mw[ix.reshape(-1)] = True
                    assert np.all(K.from_bits(bits[ix.reshape(-1)], K.DT_F32)[bits[ix.reshape(-1)] != 0xFFFFFFFF] == 0.0)
            if f == "planes":
                C = d["planes_C"]
                for b, l in enumerate(d["_lens"]):
                    rows = np.arange(0, min(d["L"], (l + 31) // 32 * 32))
                    ix = b * d["L_rows"] * 3 * C + rows[:, None] * 3 * C + np.arange(3 * C)[None, :]
                    mw[ix.reshape(-1)] = True
                pdt = K.DT_F16 if d["planes_f16"] else K.DT_BF16
                _check_buffer(f"{name}.planes", bits, pdt, r, t, m, buf["bits"], mw, split3=(3 * C, C, pdt))
                continue
            w = _check_buffer(f"{name}.{f}", bits, buf["dt"], r, t, m, buf["bits"], mw)
            print(f"{name}: worst err/bound {w:.3f}")
    finally:
        dev.free()


# ------------------------------------------------------------------------------------------------------------------------------
# streaming ResBlock kernels against the chained reference
# ------------------------------------------------------------------------------------------------------------------------------
def _ran(rc, what):
    """A HIP error after a launch (the shim's -(1000 + code)) ends the session: nothing more is started on a device that faulted."""
    if rc <= -1000:
        pytest.exit(f"{what}: HIP error {-rc - 1000}", returncode=3)
    return rc


def _check_chain(cs, got, ref, before):
    """got / before: {field: bits of the [b][M][ld] buffer}.  Compared elements within their tolerance (zero: bit equality with the
    reference's 16-bit value), everything else -- rows at or past len, pad columns, a running sum that is only read -- as it was; the
    valid rows of an utterance with NaN input may hold anything.  Returns (worst err / tol over tol > 0, zero-tolerance share)."""
    nb, M, C = cs.X.shape
    worst = 0.0
    for f in before:
        g = got[f].reshape(nb, M, cs.ld)
        keep = np.ones((nb, M, cs.ld), bool)
        if f in ref:
            r, t, m = ref[f]
            keep[:, :, :C] = ~m
            for b in cs.nan_utts:
                keep[b, :cs.lens[b], :C] = False
            vals = K.from_bits(g[:, :, :C], cs.dt)
            err = np.abs(vals[m] - r[m])
            bad = ~(err <= t[m])
            if bad.any():
                i = np.argwhere(m)[np.argmax(bad)]
                raise AssertionError(f"{cs.name}.{f}: {bad.sum()}/{m.sum()} elements out of tolerance ({(bad & (t[m] == 0)).sum()} of them at tolerance zero); "
                                     f"[b, row, ch] = {i.tolist()}: got {vals[tuple(i)]!r} ref {r[tuple(i)]!r} tol {t[tuple(i)]:.3g}")
            pos = t[m] > 0
            if pos.any():
                worst = max(worst, float(np.max(err[pos] / t[m][pos])))
        same = g[keep] == before[f].reshape(nb, M, cs.ld)[keep]
        assert same.all(), f"{cs.name}.{f}: {(~same).sum()} elements outside the contract's region were written"
    return worst, K.exact_share(ref)


def _rms_check(name, build, cs, got, spec):
    """E_k <= E_r (1 + m) per output field against the pure float64 chain (m from the reference alone: K.rms_margin)."""
    nb, M, C = cs.X.shape
    pure = K.chain_ref(cs, q=False, bound=False)
    for f, (er, spread, m) in K.rms_margin(build).items():
        vals = K.from_bits(got[f].reshape(nb, M, cs.ld)[:, :, :C], cs.dt)
        mask = pure[f][2]
        assert np.isfinite(vals[mask]).all(), f"{name}.{f}: non-finite values"
        ek = K.rms_vs_pure(vals, pure[f][0], mask)
        spec.append(f"{f}: E_r {er:.4g} spread {spread:.4f} m {m:.4f} E_k/E_r {ek / er:.4f}")
        print(f"SPEC {name} " + spec[-1])
        assert ek <= er * (1 + m), f"{name}.{f}: rms against the pure float64 chain {ek:.4g} > {er:.4g} x (1 + {m:.4f})"


@pytest.mark.parametrize("entry", K.RESSTREAM_CASES, ids=[e[0] for e in K.RESSTREAM_CASES])
def test_resstream_case(lib, entry):
    """launch_resstream with hand-built StreamArgs.  exact-sum data: chain_ref's bound (bit equality at tolerance zero); dense data:
    bit equality with the same chain run pair by pair on launch_resfuse, as resstream.hip's header claims."""
    name, kw, vid = entry
    cs = K.build_chain(entry)
    a, _, _ = K.stream_struct(cs, None)
    assert lib.zvxk_resstream(a, 1) == vid, f"{name}: dry run"
    dev = K.Device(lib)
    try:
        a, ptr, before = K.stream_struct(cs, dev)
        assert _ran(lib.zvxk_resstream(a, 0), name) == vid, f"{name}: launch"
        n = len(next(iter(before.values())))
        got = {f: dev.download(ptr[f], n, K.bits_dtype(cs.dt)) for f in ptr}
        if cs.data == "exact":
            worst, share = _check_chain(cs, got, K.chain_ref(cs), before)
            print(f"SPEC {name} worst err/bound {worst:.3f} exact share {share:.3f}")
        else:
            pairwise = K.resfuse_chain(cs, dev, a)
            for f in got:
                diff = got[f] != pairwise[f]
                assert not diff.any(), f"{name}.{f}: {diff.sum()} elements differ from the per-pair launches (first at {np.argmax(diff)})"
            nb, M, C = cs.X.shape
            for f in got:                                          # rows past len and pad columns keep the sentinel (an accumulated running sum: xs)
                g, b0 = got[f].reshape(nb, M, cs.ld), before[f].reshape(nb, M, cs.ld)
                written = np.zeros((nb, M, cs.ld), bool)
                if not (f == "accum" and cs.am == 1):
                    for b, l in enumerate(cs.lens):
                        written[b, :l, :C] = True
                assert (g[~written] == b0[~written]).all(), f"{name}.{f}: elements outside the contract's region were written"
                assert np.isfinite(K.from_bits(g[written], cs.dt)).all(), f"{name}.{f}: non-finite values"
            print(f"SPEC {name} bit-equal to {len(cs.blocks[0])} per-pair launches")
    finally:
        dev.free()


@pytest.mark.parametrize("entry", K.NARROW_CASES, ids=[e[0] for e in K.NARROW_CASES])
def test_narrowstage_case(lib, entry):
    """launch_narrowstage with hand-built StageArgs (16 x 16 x 32 MFMA: the exact-sum premise is measured here; measured exact
    shares and worst err / bound per case in profiles/stream_kernel_spec.txt)."""
    name, kw, vid = entry
    cs = K.build_chain(entry)
    a, _, _ = K.stage_struct(cs, None)
    assert lib.zvxk_narrowstage(a, 1) == 1, f"{name}: dry run"
    dev = K.Device(lib)
    try:
        a, ptr, before = K.stage_struct(cs, dev)
        assert _ran(lib.zvxk_narrowstage(a, 0), name) == 1, f"{name}: launch"
        got = {"out": dev.download(ptr["out"], len(before["out"]), K.bits_dtype(cs.dt))}
        if cs.data == "exact":
            worst, share = _check_chain(cs, got, K.chain_ref(cs), before)
            print(f"SPEC {name} worst err/bound {worst:.3f} exact share {share:.3f}")
        else:
            nb, M, C = cs.X.shape
            g = got["out"].reshape(nb, M, C)
            for b, l in enumerate(cs.lens):
                assert (g[b, l:] == K.sentinel_bits(cs.dt)).all(), f"{name}: rows past len written"
            _rms_check(name, K.dense_builder(entry), cs, got, [])
    finally:
        dev.free()


@pytest.mark.parametrize("C", [16, 8])
def test_narrowstage_tile_reuse(lib, C):
    """More one-tile utterances than workgroups: a persistent workgroup takes a second tile.  Two utterances hold NaN input (one
    whose workgroup goes on to a second tile, and a second tile); every other utterance meets its bound."""
    entry = (f"narrowstage_c{C}_tile_reuse", K.narrow_reuse_kw(C, lib.zvxk_num_cus()), 24 if C == 16 else 25)
    cs = K.build_chain(entry)
    dev = K.Device(lib)
    try:
        a, ptr, before = K.stage_struct(cs, dev)
        assert _ran(lib.zvxk_narrowstage(a, 0), entry[0]) == 1
        got = {"out": dev.download(ptr["out"], len(before["out"]), K.bits_dtype(cs.dt))}
        worst, share = _check_chain(cs, got, K.chain_ref(cs), before)
        print(f"SPEC {entry[0]} ({len(cs.lens)} utterances) worst err/bound {worst:.3f} exact share {share:.3f}")
    finally:
        dev.free()


@pytest.mark.parametrize("entry", K.PAIR_DENSE_CASES, ids=[e[0] for e in K.PAIR_DENSE_CASES])
def test_pairstream_dense_case(lib, entry):
    """launch_pairstream across a segment seam on dense data: rms against the pure float64 chain, rows past len untouched."""
    name, kw, vid, _ = entry
    p = K.build_case(entry)
    a, _ = K.gemm_struct(p, None)
    assert lib.zvxk_gemm(a, 1) == vid, f"{name}: dry run"
    dev = K.Device(lib)
    try:
        a, ptr = K.gemm_struct(p, dev)
        assert _ran(lib.zvxk_gemm(a, 0), name) == vid, f"{name}: launch"
        cs = K.chain_of_gemm(p)
        nb, M, C = cs.X.shape
        got = {}
        for f in cs.fields():
            buf = p.bufs[f]
            bits = dev.download(ptr[f], len(buf["bits"]), K.bits_dtype(buf["dt"]))
            g, b0 = bits.reshape(nb, M, cs.ld), buf["bits"].reshape(nb, M, cs.ld)
            for b, l in enumerate(cs.lens):
                assert (g[b, l:] == b0[b, l:]).all(), f"{name}.{f}: rows past len written"
            got[f] = bits
        if cs.am == 1:
            buf = p.bufs["accum"]
            assert (dev.download(ptr["accum"], len(buf["bits"]), K.bits_dtype(buf["dt"])) == buf["bits"]).all(), f"{name}: a running sum that is only read changed"
        _rms_check(name, K.dense_builder(entry), cs, got, [])
    finally:
        dev.free()


def test_stream_launcher_refusals(lib):
    """Descriptors launch_resstream / launch_narrowstage must refuse, by dry run only."""
    cs = K.build_chain(K.RESSTREAM_CASES[0])
    a, _, _ = K.stream_struct(cs, None)
    assert lib.zvxk_resstream(a, 1) == 20

    def probe(**kw):
        b = K.StreamArgs.from_buffer_copy(a)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(b, k)[:] = v
            else:
                setattr(b, k, v)
        return lib.zvxk_resstream(b, 1)

    assert probe(ldx=40) == -1                                         # the DMA image assumes dense rows
    assert probe(dil=(1, 3, 4)) == -1                                  # the dilations are template constants
    assert probe(npair=4) == -1
    assert probe(accum=0x900000, accum_mode=2) == -1                   # an output beside a running sum that is only written
    assert probe(out=None, accum=0x900000, accum_mode=1) == -1         # nothing to write
    assert probe(out=None, accum=0x900000, accum_mode=3) == 20
    ns = K.build_chain(K.NARROW_CASES[0])
    s, _, _ = K.stage_struct(ns, None)
    assert lib.zvxk_narrowstage(s, 1) == 1

    def nprobe(f):
        b = K.StageArgs.from_buffer_copy(s)
        f(b)
        return lib.zvxk_narrowstage(b, 1)

    def set_dil(b):
        b.dil[0][1] = 2

    def set_k(b):
        b.ks[1] = 9
    assert nprobe(set_dil) == 0 and nprobe(set_k) == 0
    assert nprobe(lambda b: setattr(b, "ldo", 24)) == 0
    assert nprobe(lambda b: setattr(b, "nk", 4)) == 0


def test_launcher_refusals(lib):
    """Descriptors the launchers must refuse, probed with dry runs only (nothing is launched)."""
    base = K.build_case(next(e for e in K.GEMM_CASES if e[0] == "slab256_epi001_bf16"))
    a, _ = K.gemm_struct(base, None)

    def probe(**kw):
        b = K.GemmArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return lib.zvxk_gemm(b, 1)

    assert probe(N=0) < 0 and probe(M=0) < 0 and probe(nbatch=0) < 0
    assert probe(ntaps=0) == -2 and probe(ntaps=K.MAX_TAPS + 1) == -2
    assert probe(out_split3=1) == -2                                   # split planes need an f32 output
    assert probe(N=126, ldo=126) == -2                                 # N % 4 with a per-n bias
    assert probe(K2=48, X2=None) == -5 and probe(K2=40, X2=0x1000, ldx2=40) == -5
    far = K.GemmArgs.from_buffer_copy(a)
    far.dv[0], far.dv[2] = -100, 100                                   # 200 halo rows: more than any tile stages
    assert lib.zvxk_gemm(far, 1) == 18                                 # ... so even with packed weights the 64 x 64 gathered-row kernel runs it
    far.Wp = None
    assert lib.zvxk_gemm(far, 1) == 18
    ds = K.GemmArgs.from_buffer_copy(a)
    ds.ds_out = 0x1000
    assert lib.zvxk_gemm(ds, 1) == -7                                  # the fused level transition asked for an uncovered shape
    # accumulate into an IEEE-half running sum on the 256 x 128 tile's run-time epilogue: refused (-6)
    acc = K.GemmArgs.from_buffer_copy(a)
    acc.accum, acc.accum_mode, acc.accum_dtype, acc.lda, acc.alpha = 0x2000, 1, K.DT_F16, 128, 0.5
    assert lib.zvxk_gemm(acc, 1) == -6
    # fused pairs: f32, N != K, uncovered tap counts
    fz = K.build_case(next(e for e in K.GEMM_CASES if e[0] == "resfuse_c32_k3_bf16"))
    f, _ = K.gemm_struct(fz, None)
    for kw in (dict(dtype=K.DT_F32), dict(K=64), dict(ntaps=5)):
        g = K.GemmArgs.from_buffer_copy(f)
        for k, v in kw.items():
            setattr(g, k, v)
        assert lib.zvxk_gemm(g, 1) == -1, kw
    g = K.GemmArgs.from_buffer_copy(f)
    g.fused = 2
    g.ntaps = 11
    assert lib.zvxk_gemm(g, 1) == -1
    # C = 128 pairs exist only as the streaming pair kernel: no_pairstream = 1 (the bit-equality reference) leaves nothing to run
    ps = K.build_case(next(e for e in K.GEMM_CASES if e[0] == "pairstream_c128_bf16"))
    g, _ = K.gemm_struct(ps, None)
    g.no_pairstream = 1
    assert lib.zvxk_gemm(g, 1) == -1
    # attention: D other than 264, misaligned strides
    fa = K.build_case(K.ATTN_CASES[0])
    x, _ = K.attn_struct(fa, None)
    for kw in (dict(D=128), dict(L=0), dict(ldq=x.ldq + 4), dict(ldv=x.ldv + 4), dict(k_off=x.k_off + 4)):
        y = K.FlashArgs.from_buffer_copy(x)
        for k, v in kw.items():
            setattr(y, k, v)
        assert lib.zvxk_flash(y, 1) == 0, kw
    fb = K.build_case(next(e for e in K.ATTN_CASES if e[0].startswith("attnf32")))
    x, _ = K.attn_struct(fb, None)
    for kw in (dict(D=256), dict(L=0), dict(ld=x.ld + 2), dict(k_off=x.k_off + 2)):
        y = K.AttnF32Args.from_buffer_copy(x)
        for k, v in kw.items():
            setattr(y, k, v)
        assert lib.zvxk_attn_f32(y, 1) == 0, kw


def test_coverage(lib):
    """Every variant of kVariants is reached by a case of the tables (GEMM_CASES; RESSTREAM_CASES / NARROW_CASES for the launchers
    with their own argument structs) in every dtype it has a form for (bar the listed exclusions),
    and every compile-time epilogue of the 256 x 128 / 128 x 128 conv-slab tiles in every dtype it is compiled for.  Derived from
    dry runs of the whole table (nothing is launched), so it holds under any selection or order; test_gemm_case checks that each
    launch returns the id its dry run names."""
    nv = lib.zvxk_num_variants()
    names = {i: lib.zvxk_variant_name(i).decode() for i in range(nv)}
    expected = set()
    for i, n in names.items():
        if i in K.EXCLUDED_VARIANTS:
            continue
        dts = ("f32",) if n.startswith("gemm_f32") else (("bf16",) if n.startswith("conv2d_") else ("bf16", "f16"))
        expected |= {(i, dt) for dt in dts}
    reached, epis = set(), set()
    for entry in K.GEMM_CASES:
        p = K.build_case(entry)
        a, _ = K.gemm_struct(p, None)
        vid = lib.zvxk_gemm(a, 1)
        assert vid == entry[2], f"{entry[0]}: dry run picks {vid}, the case expects {entry[2]}"
        dt = K.DT_NAME[p.d["dtype"]]
        reached.add((vid, dt))
        if vid in (7, 22):
            e = _effective_epi(p, vid, lib.zvxk_epi_mode(a))
            epis.add((vid, K.EPI_NAMES[e], dt + (("->" + K.DT_NAME[p.d["out_dtype"]]) if e == K.EPI_FLIP else "")))
    # the streaming kernels with their own argument structs: dry runs of their tables
    for entry in K.RESSTREAM_CASES:
        cs = K.build_chain(entry)
        vid = lib.zvxk_resstream(K.stream_struct(cs, None)[0], 1)
        assert vid == entry[2], f"{entry[0]}: dry run picks {vid}, the case expects {entry[2]}"
        reached.add((vid, K.DT_NAME[cs.dt]))
    for entry in K.NARROW_CASES:
        cs = K.build_chain(entry)
        assert lib.zvxk_narrowstage(K.stage_struct(cs, None)[0], 1) == 1, f"{entry[0]}: the launcher declines the case"
        reached.add((entry[2], K.DT_NAME[cs.dt]))                      # launch_narrowstage has one kernel per C: 24 (C = 16), 25 (C = 8)
    print("reached (variant, dtype):", sorted(reached))
    print("excluded:", {i: f"{names[i]}: {why}" for i, why in K.EXCLUDED_VARIANTS.items()})
    print("reached (tile, epilogue, dtype):", sorted(epis))
    assert expected <= reached, f"variants without a case: {sorted(expected - reached)}"
    assert reached <= expected, f"cases reaching an excluded or unknown variant: {sorted(reached - expected)}"
    want_epi = set()
    for dt in ("bf16", "f16"):
        for e in ("EPI(0,0,1)", "EPI(1,0,1)", "EPI(1,2,0)", "EPI(1,3,0)", "EPI(1,1,1)", "run-time"):
            want_epi.add((7, e, dt))
        want_epi.add((22, "EPI(0,0,1)", dt))
        want_epi.add((22, "run-time", dt))
    want_epi |= {(7, "FLIP", "bf16->f16"), (7, "FLIP", "f16->bf16"), (7, "DEC(0)", "f16"), (7, "DEC(1)", "f16"), (22, "DEC(0)", "f16"), (22, "DEC(1)", "f16")}
    assert want_epi <= epis, f"epilogues not reached: {sorted(want_epi - epis)}"
