"""Voice matching, milliseconds: zvx_spk_topk and zvx_spk_score against a library of K embeddings at the medium model's width, next to what
a user would write today with torch on the same device, and the untouched paths next to the parent commit's -- all in ONE visit of one
GPU (16-bit mode, synthetic weights):

    (a) K = 10^4 / 10^5 / 10^6 library rows of dim = hidden, B = 1 / 16 / 64 queries, top = 5; queries, library and results on the device.
        Per shape: the launch group of zvx_spk_topk and of zvx_spk_score (device events around the launches: stage tag "spk.match" of
        zvx_tag_stats) and the host wall clock around a call that waits; `torch.topk(q @ lib.T, 5)` on a PRE-NORMALISED library of the
        same shape (the favourable baseline: no norms at search time), timed by device events; and the floor K dim 4 bytes / 6.3 TB/s,
        the copy bandwidth measured on this GPU (MI355X_MICROARCH.md).  Each kernel is given as a multiple of the floor and of the torch
        baseline.  torch brings a HIP runtime of its own, which does not find the device in a process where the library's runtime has
        opened it, so the baseline runs in a child process of the same visit on the same GPU, on Gaussian rows of its own.
    (b) with --parent DIR, a built checkout of the parent commit: plain tts_long of the paragraph of tools/denoise_bench.py and
        bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline, in child processes, in the order parent, this, parent, this.

Medians of --reps runs after --warmup untimed ones.

    python tools/voice_bench.py [--reps 7] [--warmup 3] [--parent DIR] [--out profiles/voice_match.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from denoise_bench import box, load  # noqa: E402
from watermark_bench import BENCH, run_bench  # noqa: E402

COPY_BYTES_PER_S = 6.3e12
KS, BS, TOP = (10 ** 4, 10 ** 5, 10 ** 6), (1, 16, 64), 5
DIM = 528                                                     # the medium model's hidden width (asserted against the context)


def median_events(torch, fn, reps, warmup):
    ms = []
    for _ in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[warmup:]))


def median_call(ctx, fn, reps, warmup):
    """-> (event-timed ms of the "spk.match" launch group, host wall ms around the waiting call)"""
    wall = []
    for _ in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    ev = []
    ctx.set_int("profile", 2)
    try:
        for _ in range(reps):
            ctx.reset_stats()
            fn()
            ev.append({t["name"]: t for t in ctx.tag_stats()}["spk.match"]["ms"])
    finally:
        ctx.set_int("profile", 0)
    return float(np.median(ev)), float(np.median(wall[warmup:]))


def torch_child(reps, warmup):
    """the torch baseline in a process of its own: {"K,B": ms} of torch.topk(q @ lib.T, TOP) on a pre-normalised library, device events"""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {"dim": DIM}
    for K in KS:
        lib_n = torch.nn.functional.normalize(torch.randn((K, DIM), generator=g, device=dev, dtype=torch.float32), dim=1)
        for B in BS:
            q_n = torch.nn.functional.normalize(torch.randn((B, DIM), generator=g, device=dev, dtype=torch.float32), dim=1)
            out[f"{K},{B}"] = median_events(torch, lambda: torch.topk(q_n @ lib_n.T, TOP), reps, warmup)
        del lib_n
        torch.cuda.empty_cache()
    print(json.dumps(out))


def shapes(synth, reps, warmup, base):
    ctx = synth.model.ctx
    dim = ctx.hidden
    assert dim == DIM, (dim, DIM)
    rng = np.random.default_rng(0)
    lines = []
    for K in KS:
        lib = ctx.dev_alloc(K * dim * 4)
        part = 100000                                         # (the host side is generated and sent in parts)
        for k0 in range(0, K, part):
            n = min(part, K - k0)
            ctx.dev_from_host(lib + k0 * dim * 4, (rng.standard_normal((n, dim)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32))
        floor_ms = K * dim * 4 / COPY_BYTES_PER_S * 1e3
        for B in BS:
            q = ctx.dev_alloc(B * dim * 4)
            ctx.dev_from_host(q, rng.standard_normal((B, dim)).astype(np.float32))
            ts, ti, sc = ctx.dev_alloc(B * TOP * 4), ctx.dev_alloc(B * TOP * 4), ctx.dev_alloc(B * K * 4)
            topk = lambda: ctx.spk_topk_device(q, B, lib, K, ts, ti, TOP, dim)       # noqa: E731
            score = lambda: ctx.spk_score_device(q, B, lib, K, sc, dim)              # noqa: E731
            k_ev, k_wall = median_call(ctx, topk, reps, warmup)
            s_ev, s_wall = median_call(ctx, score, reps, warmup)
            # the two calls agree with each other on the device's own matrix (the tests hold them to the float64 reference)
            same = bool(np.array_equal(ctx.dev_to_host(ti, (B,  TOP), np.int32)[:, 0], ctx.dev_to_host(sc, (B, K), np.float32).argmax(axis=1)))
            t_ms = base.get(f"{K},{B}")
            vs = (lambda v: f"{v / t_ms:.2f}x torch") if t_ms else (lambda v: "torch not measured")
            lines.append(f"(a) K = {K:>7d}, B = {B:>2d}, dim {dim}: floor {floor_ms:.4f} ms; zvx_spk_topk {k_ev:.4f} ms [{k_wall:.3f} wall] = "
                         f"{k_ev / floor_ms:.2f}x floor, {vs(k_ev)}; zvx_spk_score {s_ev:.4f} ms [{s_wall:.3f} wall] = "
                         f"{s_ev / floor_ms:.2f}x floor, {vs(s_ev)}; torch.topk(q @ lib.T, {TOP}) "
                         + (f"{t_ms:.4f} ms = {t_ms / floor_ms:.2f}x floor" if t_ms else "not measured") + f"; top-1 of the two calls equal: {same}")
            print(lines[-1], flush=True)
            for p in (q, ts, ti, sc):
                ctx.dev_free(p)
        ctx.dev_free(lib)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its tts_long and bench.py are the baseline")
    ap.add_argument("--out", default=None)
    ap.add_argument("--torch-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.dirname(HERE)
    if args.torch_child:
        torch_child(args.reps, args.warmup)
        return

    def long_child(root):
        p = subprocess.run([sys.executable, os.path.join(root, "tools", "watermark_bench.py"), "--long-child", "--reps", "5", "--warmup", "2"],
                           capture_output=True, text=True, cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=600)
        if p.returncode:
            raise SystemExit(f"tts_long in {root} failed:\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])["plain"]

    lines = [f"Voice matching (tools/voice_bench.py): {box()}, 16-bit mode.",
             f"median of {args.reps} runs after {args.warmup} warm-ups; kernels: device events around the launch group (stage tag spk.match), in brackets "
             f"the host wall clock around the call and its wait; torch: device events.  floor = K dim 4 bytes / 6.3 TB/s."]
    passes = []
    if args.parent:                                           # parent, this, parent, this: child processes, one at a time
        parent = os.path.abspath(args.parent)
        for name, root in (("parent", parent), ("this", here), ("parent", parent), ("this", here)):
            passes.append((name, long_child(root), run_bench(root)))
            print(passes[-1], flush=True)
    # torch carries a HIP runtime of its own; that one and the library's do not both find the device in one process, so the baseline runs
    # in a child process of this visit, before this process opens the device
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                       capture_output=True, text=True, timeout=900)
    base = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else {}
    if not base:
        lines.append("torch baseline NOT measured: " + (p.stderr.strip().splitlines() or ["no output"])[-1][:200])
    synth, _ = load(here)
    lines += shapes(synth, args.reps, args.warmup, base)
    if passes:
        lines.append("(b) the untouched paths, child processes in the order run: plain tts_long of 32 sentences of 1024 frames (tools/watermark_bench.py "
                     "--long-child); bench.py " + " ".join(BENCH))
        for name, long_ms, (step_ms, value) in passes:
            lines.append(f"    {name:6s}: tts_long {long_ms:.2f} ms; bench.py " + (f"{step_ms:.3f} ms per step, " if step_ms is not None else "")
                         + f"{value:.0f} samples/s")

        def spread(v):
            return 100.0 * (max(v) - min(v)) / min(v)
        for label, pick in (("tts_long ms", lambda p: p[1]), ("bench.py samples/s", lambda p: p[2][1])):
            par, this = [pick(p) for p in passes if p[0] == "parent"], [pick(p) for p in passes if p[0] == "this"]
            lines.append(f"    {label}: parent passes differ by {spread(par):.2f} %, this tree's by {spread(this):.2f} %; means: this / parent = "
                         f"{np.mean(this) / np.mean(par):.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
