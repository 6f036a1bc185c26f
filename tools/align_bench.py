"""Alignment, milliseconds: the launch-group time of zvx_dtw ("post.align" in zvx_tag_stats, hipEvent-timed, with its two launches under
"post.align.forward" / "post.align.backtrack") on device rows of seeded Gaussian features, dim 13 -- 1 pair of 256 x 256 frames, 32 pairs of
512 x 512, 32 pairs of 1024 x 1024 and 1 pair of 4096 x 4096 -- and of zvx_align_wav on 32 pairs of 6 s of noise-like audio (host rows: wall
time includes their upload).  Cells per second = sum Ta Tb / group time.  There is no earlier path to compare with.  Median of --reps calls
after --warmup; StyleTTS decoder + HiFi-GAN V1 bf16, synthetic weights (the model only gives the front end its geometry).

    python tools/align_bench.py [--reps 5] [--warmup 2] [--out profiles/align_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zerovox_amd.synthesize import ZeroVoxTTS                # noqa: E402

DIM = 13
SHAPES = [(1, 256), (32, 512), (32, 1024), (1, 4096)]
TAGS = ("post.align", "post.align.forward", "post.align.backtrack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:v1", infer_device="cuda:0", precision="bf16")
    ctx = synth.model.ctx
    rate = ctx.get_int("sampling_rate")

    def group_ms(call):
        """median launch-group times (one per tag of TAGS) and wall time of `call` in ms"""
        group, wall = [], []
        ctx.set_int("profile", 2)
        try:
            for _ in range(args.warmup + args.reps):
                ctx.reset_stats()
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                tags = {t["name"]: t for t in ctx.tag_stats()}
                group.append([tags[k]["ms"] for k in TAGS])
        finally:
            ctx.set_int("profile", 0)
        return np.median(np.array(group[args.warmup:]), axis=0), float(np.median(wall[args.warmup:]))

    lines = [f"Alignment (zvx_dtw, zvx_align_wav; tools/align_bench.py): seeded Gaussian features, dim {DIM}, rows on the device.",
             f"group = hipEvent time of the launch group (\"post.align\"; forward / backtrack: its two launches), wall = host wall time of the call "
             f"with the path and a2b to the host; median of {args.reps} after {args.warmup} warm-ups.  No earlier path exists to compare with.", ""]
    rng = np.random.default_rng(0)
    for B, T in SHAPES:
        xa, xb = rng.standard_normal((B, T, DIM)).astype(np.float32), rng.standard_normal((B, T, DIM)).astype(np.float32)
        lens = np.full(B, T, np.int32)
        buf = ctx.dev_alloc(2 * xa.nbytes)
        try:
            ctx.dev_from_host(buf, xa)
            ctx.dev_from_host(buf + xa.nbytes, xb)
            res = ctx.dtw_device(buf, lens, T, buf + xa.nbytes, lens, T, DIM)
            (g, f, k), w = group_ms(lambda: ctx.dtw_device(buf, lens, T, buf + xa.nbytes, lens, T, DIM))
        finally:
            ctx.sync()
            ctx.dev_free(buf)
        cells = float(B) * T * T
        out = [f"{B} pair(s) of {T} x {T} frames ({cells:.3g} cells, mean path {float(np.mean(res['path_len'])):.0f} cells):",
               f"  zvx_dtw: group {g:.3f} ms (forward {f:.3f}, backtrack {k:.3f}), wall {w:.3f} ms; {cells / g / 1e6:.2f} G cells/s", ""]
        print("\n".join(out), flush=True)
        lines += out
    B, n = 32, 6 * rate
    wa, wb = (0.1 * rng.standard_normal((B, n))).astype(np.float32), (0.1 * rng.standard_normal((B, n))).astype(np.float32)
    lens = np.full(B, n, np.int32)
    res = ctx.align(wa, wb, lengths_a=lens, lengths_b=lens)
    (g, f, k), w = group_ms(lambda: ctx.align(wa, wb, lengths_a=lens, lengths_b=lens))
    cells = float(np.sum(res["frames_a"].astype(np.int64) * res["frames_b"]))
    out = [f"zvx_align_wav: {B} pairs of 6 s at {rate} Hz ({int(res['frames_a'][0])} x {int(res['frames_b'][0])} frames each, host rows):",
           f"  alignment group {g:.3f} ms (forward {f:.3f}, backtrack {k:.3f}; {cells / g / 1e6:.2f} G cells/s), wall of the whole call with upload, "
           f"front end and cepstra {w:.3f} ms", ""]
    print("\n".join(out), flush=True)
    lines += out
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
