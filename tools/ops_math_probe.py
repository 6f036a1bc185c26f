"""Measure the device's expf / tanhf / logf / sqrtf / reciprocal against float64 over exactly the arguments the cases of
tests/ops_ref.py feed them (zvxk_math_probe of the test shim: a kernel of its own, no code under test), in ulp of f32 at the true
value.  Prints the MATH lines of profiles/ops_kernel_spec.txt; k = max(1, ceil(2 x worst)) is what ops_ref.K_ULP holds.
Needs a GPU and the built shim:  python tools/ops_math_probe.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import kernel_ref as K      # noqa: E402
import ops_ref as R         # noqa: E402

TRUE = {"exp": np.exp, "tanh": np.tanh, "log": np.log, "sqrt": np.sqrt, "div": lambda x: 1.0 / x}


def main():
    R.COLLECT = True
    with np.errstate(all="ignore"):
        for c in R.cases():
            c.ref()
    R.COLLECT = False
    lib = K.load_ktest()
    dev = K.Device(lib)
    try:
        for fn, code in R.PROBE_FN.items():
            a = np.unique(np.concatenate(R.PROBE_ARGS[fn]).astype(np.float32))
            a = a[np.isfinite(a)]
            if fn in ("log", "div"):
                a = a[a > 0]
            pin, pout = dev.upload(a), dev.alloc(a.nbytes)
            rc = lib.zvxk_math_probe(code, pin, pout, len(a))
            if rc:
                print(f"MATH {fn}: HIP error {rc}")
                return 3
            got = dev.download(pout, len(a), np.float32).astype(np.float64)
            with np.errstate(all="ignore"):
                true = TRUE[fn](a.astype(np.float64))
            ok = np.isfinite(true) & (np.abs(true) > 2.0 ** -126) & (np.abs(true) < 3e38)       # results that are normal f32 numbers
            err = np.abs(got[ok] - true[ok]) / R.ulp32(true[ok])
            i = int(np.argmax(err))
            print(f"MATH {fn}: {int(ok.sum())} unique arguments, worst {err[i]:.3f} ulp at {float(a[ok][i])!r} -> k = {max(1, int(np.ceil(2 * err[i])))}", flush=True)
    finally:
        dev.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
