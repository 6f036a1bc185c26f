"""Spec-level tests of the small kernels of zerovox_amd/csrc/ops.hip against the float64 references of tests/ops_ref.py, driven
through the shim entry points zvxk_<launcher> of libzvx_ktest.so with hand-built arguments.

Per element of every output buffer: inside the contract's written region |kernel - ref| <= tol (tol 0: the reference's bits --
data movement, integers, the zeros the contract writes, single correctly rounded operations), outside it the bits the buffer held
before (the sentinel).  Masked input rows and columns hold NaN, so a read past a length shows as a NaN inside the region.  The
tolerances come from ops_ref alone (its docstring); each case prints `SPEC <case> worst err/bound ...`, the share of its bound the
kernel used (profiles/ops_kernel_spec.txt).  Three bit-equality claims of ops.hip are held as such: LayerNorm's split planes =
launch_split3 of its own f32 output, launch_instnorm_fused = launch_instnorm_stats + launch_norm_affine_act, k_fc_rows4 = k_fc_rows."""
import numpy as np
import pytest

import kernel_ref as K
import ops_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return K.load_ktest()


def _ran(rc, what):
    """A HIP error after a launch (the shim's -(1000 + code)) ends the session: nothing more is started on a device that faulted."""
    if rc <= -1000:
        pytest.exit(f"{what}: HIP error {-rc - 1000}", returncode=3)
    return rc


def _launch(lib, dev, fn, bufs, args, what):
    """Upload bufs {key: {bits, dt, out}}, call zvxk_<fn>, return ({key: device pointer}, {key: bits of every `out` buffer})."""
    ptr = {k: dev.upload(b["bits"]) for k, b in bufs.items()}
    call = []
    for a in args:
        if isinstance(a, str):
            call.append(ptr[a])
        elif isinstance(a, tuple):
            call.append(ptr[a[0]] + a[1] * R.esz(bufs[a[0]]["dt"]))
        else:
            call.append(a if a is None or isinstance(a, float) else int(a))
    assert _ran(getattr(lib, "zvxk_" + fn)(*call), what) == 0, f"{what}: launch"
    return ptr, {k: dev.download(ptr[k], len(b["bits"]), b["bits"].dtype) for k, b in bufs.items() if b["out"]}


def _run(lib, cs):
    dev = K.Device(lib)
    try:
        return _launch(lib, dev, cs.fn, cs.bufs, cs.args, cs.name)[1]
    finally:
        dev.free()


def _check(cs, got):
    """Every output buffer against (ref, tol, mask); returns the largest err / tol over the elements with a tolerance."""
    worst = 0.0
    ref = cs.ref()
    assert set(ref) == set(got), f"{cs.name}: the reference covers {sorted(ref)}, the case writes {sorted(got)}"
    for k, (r, t, m) in ref.items():
        b, g = cs.bufs[k], got[k]
        val = R.values(g, b["dt"])
        with np.errstate(invalid="ignore"):
            err = np.abs(val - r)
            bad = m & ~(err <= t)
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError(f"{cs.name}.{k}: {bad.sum()}/{m.sum()} elements out of bound; element {i}: got {val[i]!r} ref {r[i]!r} tol {t[i]:.3g}")
        if b["dt"] in (K.DT_F32, K.DT_BF16, K.DT_F16):
            ex = m & (t == 0)
            same = g[ex] == R.bits_of(r[ex], b["dt"])
            assert same.all(), f"{cs.name}.{k}: {(~same).sum()} elements differ in bits from an exact reference (first at {np.nonzero(ex)[0][np.argmin(same)]})"
        keep = ~m & ~cs.may.get(k, np.zeros(len(m), bool))
        same = g[keep] == b["bits"][keep]
        assert same.all(), f"{cs.name}.{k}: {(~same).sum()} elements outside the contract's region were written (first at {np.nonzero(keep)[0][np.argmin(same)]})"
        loose = m & (t > 0)
        if loose.any():
            worst = max(worst, float(np.max(err[loose] / t[loose])))
    return worst


_PLAIN = [c.name for c in R.cases()]


@pytest.mark.parametrize("name", _PLAIN)
def test_ops_case(lib, name):
    cs = R.case(name)
    got = _run(lib, cs)
    worst = _check(cs, got)
    extra = ""
    if "ratio16" in cs.info:
        extra = f" rstd bound / 16-bit half-ulp: {cs.info['ratio16'][0]:.1f} (bf16) {cs.info['ratio16'][1]:.1f} (f16)"
    print(f"SPEC {name} worst err/bound {worst:.3f}{extra}")


@pytest.mark.parametrize("name", [c.name for c in R.cases() if c.fn == "layernorm" and c.info["planes"]])
def test_layernorm_planes_equal_split3_of_the_f32_rows(lib, name):
    """The [hi | hi | lo] planes k_layernorm emits are "what k_split3 would write": launch_split3 on the kernel's own f32 output."""
    cs = R.case(name)
    i = cs.info
    got = _run(lib, cs)
    pdt = cs.bufs["planes"]["dt"]
    n = i["B"] * i["R"] * 3 * i["C"]
    y = got[i["ykey"]].copy()
    bufs = dict(x=dict(bits=y, dt=K.DT_F32, out=False), rows=cs.bufs["rows"], out=dict(bits=cs.bufs["planes"]["bits"].copy(), dt=pdt, out=True))
    dev = K.Device(lib)
    try:
        _, sp = _launch(lib, dev, "split3", bufs, ["x", i["ldy"], "out", i["B"], i["R"], "rows", i["C"], int(i["planes"] == 2)], name + ".split3")
    finally:
        dev.free()
    assert np.array_equal(got["planes"][:n], sp["out"][:n]), f"{name}: {(got['planes'][:n] != sp['out'][:n]).sum()} plane elements differ from launch_split3"
    assert np.array_equal(got["planes"][n:], cs.bufs["planes"]["bits"][n:])
    print(f"SPEC {name} planes bit-equal to launch_split3 of the f32 rows")


@pytest.mark.parametrize("name", [c.name for c in R.cases() if c.fn == "instnorm_fused"])
def test_instnorm_fused_equals_stats_plus_apply(lib, name):
    """launch_instnorm_fused is "bit-identical to k_colstats + k_norm_affine_act": mean, rstd and y of the same data."""
    cs = R.case(name)
    i = cs.info
    fused = _run(lib, cs)
    dev = K.Device(lib)
    try:
        ptr, st = _launch(lib, dev, "instnorm_stats", {k: cs.bufs[k] for k in ("x", "L", "mean", "rstd")},
                          ["x", i["xdt"], i["ldx"], i["B"], i["Lmax"], "L", i["C"], i["eps"], "mean", "rstd"], name + ".stats")
        bufs = {k: v for k, v in cs.bufs.items() if k not in ("mean", "rstd")}
        for k in ("mean", "rstd"):
            bufs[k] = dict(bits=st[k], dt=K.DT_F32, out=False)
        ga, ba = ("gamma" if i["affine"] else None), ("beta" if i["affine"] else None)
        _, ap = _launch(lib, dev, "norm_affine_act", bufs, ["x", i["xdt"], i["ldx"], ("y", i["yoff"]), i["ydt"], i["ldy"], i["B"], i["Lmax"], "L", i["C"],
                                                            "mean", "rstd", ga, ba, i["g_bs"], int(i["one_plus"]), i["act"], i["slope"]], name + ".apply")
    finally:
        dev.free()
    live = ~cs.may["mean"]                             # (a zero-length utterance's statistics are unspecified)
    for k in ("mean", "rstd"):
        assert np.array_equal(fused[k][live], st[k][live]), f"{name}: {k} differs from launch_instnorm_stats in {(fused[k][live] != st[k][live]).sum()} elements"
    assert np.array_equal(fused["y"], ap["y"]), f"{name}: y differs from the two-kernel path in {(fused['y'] != ap['y']).sum()} elements"
    print(f"SPEC {name} bit-equal to launch_instnorm_stats + launch_norm_affine_act")


@pytest.mark.parametrize("Kk", [4, 256, 260])
def test_fc_rows4_equals_fc_rows(lib, Kk):
    """B = 33 runs k_fc_rows4, "bit-identical to k_fc_rows": the same rows as two launches of <= 32 rows on the one-column kernel."""
    cs = R.case(f"fc_rows_b33_k{Kk}_bias1")
    i = cs.info
    whole = _run(lib, cs)["out"]
    parts = []
    for lo, hi in ((0, 32), (32, 33)):
        bufs = dict(cs.bufs)
        bufs["x"] = dict(bits=cs.bufs["x"]["bits"][lo * i["ldx"]:hi * i["ldx"]].copy(), dt=K.DT_F32, out=False)
        bufs["out"] = dict(bits=cs.bufs["out"]["bits"][lo * i["ldo"]:hi * i["ldo"]].copy(), dt=K.DT_F32, out=True)
        dev = K.Device(lib)
        try:
            parts.append(_launch(lib, dev, "fc_rows", bufs, ["x", i["ldx"], "w", i["ldw"], "bias", "out", i["ldo"], hi - lo, i["N"], Kk], cs.name)[1]["out"])
        finally:
            dev.free()
    assert np.array_equal(whole, np.concatenate(parts)), f"K = {Kk}: {(whole != np.concatenate(parts)).sum()} elements differ"
    print(f"SPEC fc_rows_b33_k{Kk} bit-equal to launches of 32 + 1 rows on k_fc_rows")


def test_bucket_ctl_unit_equals_the_plain_kernel(lib):
    """range = 1, shift = 0 gives the plain kernel's indices and rows bit for bit (include/zvx.h)."""
    a, b = _run(lib, R.case("bucket_embed_add")), _run(lib, R.case("bucket_embed_add_ctl_unit"))
    keep_i, keep_x = np.ones(len(a["idx"]), bool), np.ones(len(a["x"]), bool)
    keep_i[5], keep_x[5 * 24:6 * 24] = False, False    # the plain case's NaN prediction: a finite one in the forms that take a mean
    keep_i[3 * 7:], keep_x[3 * 7 * 24:] = False, False  # utterance 3 holds a NaN: under a range its mean is NaN and every index 0 (zvx_kernels.h)
    assert np.array_equal(a["idx"][keep_i], b["idx"][keep_i]) and np.array_equal(a["x"][keep_x], b["x"][keep_x])
    print("SPEC bucket_embed_add_ctl_unit bit-equal to bucket_embed_add")
