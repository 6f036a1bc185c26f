"""The persistent kernels past a workgroup's first tile.  Every kernel that sizes its grid to the chip -- resfuse_persist (variants
16 / 17), conv2d_persist (26 / 27, with the fused squeeze-excite pool), conv2d_s2 (28 / 29), narrowstage (24 / 25), resstream
(20 / 21), pairstream (23) -- walks several tiles or segments per workgroup at production shapes and one in the small cases of
tests/test_kernels_gpu.py.  The cases here are built from the device's CU count (kernel_ref.*_persist_cases) so that every workgroup
takes at least kernel_ref.PERSIST_TRIPS units; the count is asserted on the host, from the launcher's restated grid rule, before the launch.

Per case, on ONE batched launch:
  1. sampled utterances (every long one, whatever follows a long or a NaN one in a workgroup, a spread of the rest) within the
     unchanged bound of kernel_ref.gemm_ref / chain_ref against float64; nothing outside the contract's region is written;
  2. EVERY utterance bit-equal to the same utterance launched alone (same M, same segment length: only the grid differs) -- an
     utterance's bits depend neither on its batch nor on which workgroup ran it after what;
  3. two utterances hold NaN in every row (one that another utterance follows in its workgroup, one that is itself a later unit):
     every valid element of every other utterance is finite.
Each case prints `SPEC <case> worst err/bound ... trips/workgroup ...` (one run: profiles/persistent_tile_spec.txt)."""
import ctypes

import numpy as np
import pytest

import kernel_ref as K
import test_kernels_gpu as TK                                # _check_buffer, _may_write, _check_chain, _ran

pytestmark = pytest.mark.gpu

_NCU = 256                                                   # the case NAMES are those of a 256-CU table; the shapes follow the device


@pytest.fixture(scope="module")
def lib():
    return K.load_ktest()


def _entry(table, name, ncu):
    return next(e for e in table(ncu) if e[0] == name)


def _assert_trips(entry, kernel):
    meta = entry[3]
    assert meta["trips"] >= K.PERSIST_TRIPS[kernel], f"{entry[0]}: a workgroup runs {meta['trips']} units"
    if meta["long"]:
        assert {(True, False), (False, True), (True, True)} <= meta["patterns"], f"{entry[0]}: successions {sorted(meta['patterns'])}"
    assert len(meta["nan"]) == 2


def _kernel_of(name):
    return next(k for k in ("resfuse", "pairstream", "conv2d_persist", "conv2d_s2", "narrowstage", "resstream") if name.startswith(k))


# ------------------------------------------------------------------------------------------------------------------------------
# GemmArgs launches: resfuse_persist, pairstream, conv2d_persist, conv2d_s2
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_NAMES = [e[0] for e in K.gemm_persist_cases(_NCU)]


@pytest.mark.parametrize("name", GEMM_NAMES)
def test_gemm_persistent_case(lib, name):
    entry = _entry(K.gemm_persist_cases, name, lib.zvxk_num_cus())
    _, kw, vid, meta = entry
    _assert_trips(entry, _kernel_of(name))
    p = K.build_persist_gemm(entry)
    d = p.d
    nb, es = d["nbatch"], K.esize(d["dtype"])
    a, _ = K.gemm_struct(p, None)
    assert lib.zvxk_gemm(a, 1) == vid, f"{name}: dry run"
    outs = [f for f in ("out", "accum", "ds_out") if f in p.bufs and p.bufs[f].get("role") in ("out", "inout")]
    stride = {"out": d["o_bs"], "ds_out": d["o_bs"], "accum": d["a_bs"]}
    dev = K.Device(lib)
    try:
        a, ptr = K.gemm_struct(p, dev)
        ptr2 = {f: dev.upload(p.bufs[f]["bits"]) for f in outs}                # the alone launches write into buffers of their own
        S, part, part2, nS = ctypes.c_int(0), None, None, 0
        if meta.get("pool"):
            nS = 4 * meta["grid"]["per"] * d["N"]                                 # [b][4 ntm][C] f32 partial sums
            fill = np.full(nb * nS, 0x7FC00000, np.uint32)
            part, part2 = dev.upload(fill), dev.upload(fill)
            a.se_part, a.se_part_S = part, ctypes.addressof(S)
        assert TK._ran(lib.zvxk_gemm(a, 0), name) == vid, f"{name}: launch"
        got = {f: dev.download(ptr[f], len(p.bufs[f]["bits"]), K.bits_dtype(p.bufs[f]["dt"])) for f in outs}
        # ---- 1. the sampled utterances against float64, the sentinel everywhere outside the contract's region
        ref = K.gemm_ref(p)
        worst = {}
        for f, (r, t, m) in ref.items():
            buf = p.bufs[f]
            worst[f] = TK._check_buffer(f"{name}.{f}", got[f], buf["dt"], r, t, m, buf["bits"], TK._may_write(p, f))
        if d["accum_mode"] == 1:
            assert np.array_equal(got["accum"], p.bufs["accum"]["bits"]), f"{name}: a running sum that is only read changed"
        if meta.get("pool"):
            assert S.value == 4 * meta["grid"]["per"], f"{name}: the launcher reports {S.value} partials per utterance"
            pg = dev.download(part, nb * nS, np.float32).reshape(nb, -1, d["N"]).astype(np.float64)
            w = 0.0
            for b in meta["sample"]:
                r, t = K.pool_ref(p, b)
                e = np.abs(pg[b] - r)
                assert (e <= t).all(), f"{name}: pool partials of utterance {b}: worst err / bound {float((e / np.maximum(t, 1e-300)).max()):.3f}"
                w = max(w, float((e / np.maximum(t, 1e-300)).max()))
            worst["se_part"] = w
        # ---- 3. NaN stays inside its utterance
        for f in outs:
            vals = K.from_bits(got[f], p.bufs[f]["dt"])
            ld = d["lda"] if f == "accum" else d["ldo"]
            for b in range(nb):
                if b in p.nan_utts:
                    continue
                ix = b * stride[f] + K.valid_out_rows(d, b)[:, None] * ld + np.arange(d["N"])[None, :]
                assert np.isfinite(vals[ix]).all(), f"{name}.{f}: utterance {b} holds a non-finite value"
        if meta.get("pool"):
            ok = [b for b in range(nb) if b not in p.nan_utts]
            assert np.isfinite(pg[ok]).all(), f"{name}: non-finite pool partials outside the NaN utterances"
        # ---- 2. every utterance alone: the same bits
        for b in range(nb):
            if b in p.nan_utts:
                continue
            g = K.GemmArgs.from_buffer_copy(a)
            g.nbatch = 1
            g.X = a.X + b * d["x_bs"] * es
            if a.res:
                g.res = a.res + b * d["r_bs"] * K.esize(d["res_dtype"])
            g.in_len = a.in_len + 4 * b
            if a.out_len:
                g.out_len = a.out_len + 4 * b
            for f in outs:
                setattr(g, f, ptr2[f] + b * stride[f] * K.esize(p.bufs[f]["dt"]))
            if part:
                g.se_part = part2 + b * nS * 4
            assert TK._ran(lib.zvxk_gemm(g, 0), f"{name} utterance {b} alone") == vid
        for f in outs:
            one = dev.download(ptr2[f], len(p.bufs[f]["bits"]), K.bits_dtype(p.bufs[f]["dt"])).reshape(nb, -1)
            diff = (one != got[f].reshape(nb, -1)).any(axis=1)
            diff[list(p.nan_utts)] = False
            assert not diff.any(), f"{name}.{f}: utterances {np.nonzero(diff)[0][:8].tolist()} differ from their launch alone ({int(diff.sum())} in all)"
        if part:
            one = dev.download(part2, nb * nS, np.uint32).reshape(nb, -1)
            diff = (one != dev.download(part, nb * nS, np.uint32).reshape(nb, -1)).any(axis=1)
            diff[list(p.nan_utts)] = False
            assert not diff.any(), f"{name}: pool partials of utterances {np.nonzero(diff)[0][:8].tolist()} differ from their launch alone"
        print(f"SPEC {name} variant {vid} worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
              f" trips/workgroup {meta['trips']} ({nb} utterances of {meta['grid']['per']} tiles on {meta['grid']['G']} workgroups, {len(meta['sample'])} against float64, all bit-equal alone)")
    finally:
        dev.free()


# ------------------------------------------------------------------------------------------------------------------------------
# StageArgs / StreamArgs launches: narrowstage, resstream
# ------------------------------------------------------------------------------------------------------------------------------
CHAIN_NAMES = [e[0] for e in K.chain_persist_cases(_NCU)]


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_persistent_case(lib, name):
    entry = _entry(K.chain_persist_cases, name, lib.zvxk_num_cus())
    _, kw, vid, meta = entry
    narrow = name.startswith("narrowstage")
    _assert_trips(entry, _kernel_of(name))
    cs = K.build_chain(entry)
    nb, M, C = cs.X.shape
    mk, fn, Args = (K.stage_struct, lib.zvxk_narrowstage, K.StageArgs) if narrow else (K.stream_struct, lib.zvxk_resstream, K.StreamArgs)
    want_rc = 1 if narrow else vid
    assert fn(mk(cs, None)[0], 1) == want_rc, f"{name}: dry run"
    dev = K.Device(lib)
    try:
        a, ptr, before = mk(cs, dev)
        ptr2 = {f: dev.upload(before[f]) for f in ptr}
        assert TK._ran(fn(a, 0), name) == want_rc, f"{name}: launch"
        dtb = K.bits_dtype(cs.dt)
        got = {f: dev.download(ptr[f], nb * M * cs.ld, dtb) for f in ptr}
        inside = np.arange(M)[None, :, None] < np.asarray(cs.lens)[:, None, None]
        valid = inside & (np.arange(cs.ld) < C)[None, None, :]
        clean = np.ones(nb, bool)
        clean[list(cs.nan_utts)] = False
        for f in got:
            g3, b3 = got[f].reshape(nb, M, cs.ld), before[f].reshape(nb, M, cs.ld)
            # rows at or past len and pad columns as they were (a running sum that is only read: everywhere)
            keep = ~valid if not (f == "accum" and cs.am == 1) else np.ones_like(valid)
            assert (g3[keep] == b3[keep]).all(), f"{name}.{f}: elements outside the contract's region were written"
            # 3. NaN stays inside its utterance
            assert np.isfinite(K.from_bits(g3[valid & clean[:, None, None]], cs.dt)).all(), f"{name}.{f}: non-finite values outside the NaN utterances"
        # ---- 1. the sampled utterances against the float64 chain
        utts = meta["sample"]
        sub = K.sub_chain(cs, utts)
        Ms = sub.X.shape[1]
        sel = lambda x: np.ascontiguousarray(x.reshape(nb, M, cs.ld)[utts, :Ms]).reshape(-1)
        worst, share = TK._check_chain(sub, {f: sel(got[f]) for f in got}, K.chain_ref(sub), {f: sel(before[f]) for f in got})
        # ---- 2. every utterance alone: the same bits
        for b in range(nb):
            if b in cs.nan_utts:
                continue
            g = Args.from_buffer_copy(a)
            g.nbatch = 1
            g.X = a.X + b * a.x_bs * 2
            g.len = a.len + 4 * b
            g.out = ptr2["out"] + b * a.o_bs * 2 if "out" in ptr2 else None
            if "accum" in ptr2:
                g.accum = ptr2["accum"] + b * a.a_bs * 2
            assert TK._ran(fn(g, 0), f"{name} utterance {b} alone") == want_rc
        for f in got:
            one = dev.download(ptr2[f], nb * M * cs.ld, dtb).reshape(nb, -1)
            diff = (one != got[f].reshape(nb, -1)).any(axis=1) & clean
            assert not diff.any(), f"{name}.{f}: utterances {np.nonzero(diff)[0][:8].tolist()} differ from their launch alone ({int(diff.sum())} in all)"
        print(f"SPEC {name} worst err/bound {worst:.3f} exact share {share:.3f} trips/workgroup {meta['trips']} "
              f"({nb} utterances of {meta['grid']['per']} units on {meta['grid']['G']} workgroups, {len(utts)} against float64, all bit-equal alone)")
    finally:
        dev.free()
