"""The equaliser's FIR filter (zvx_fir), milliseconds, all in ONE visit of one GPU (16-bit mode, synthetic weights):

    (a) 32 rows x 1024 frames, device rows, out of place, at K = 63 / 255 / 511 / 1023 / 4095 taps;
    (b) one row of 10 s at K = 511;
    (c) 64 rows of one 16-frame piece each (with their support) at K = 511: ONE zvx_fir_rows call against 64 zvx_fir_ex calls;
    (d) (a) at K = 511 in place (Context.fir_device: the filter into the work buffer and the copy back) against out of place;
    (e) ZeroVoxTTS.tts_long of a paragraph of 32 sentences of 1024 frames with and without eq="presence";
    (f) torch.nn.functional.conv1d on the same device rows in float32 and in float64, in a child process (torch brings a HIP runtime of
        its own), device events;
    (g) with --parent DIR, a built checkout of the parent commit: plain tts_long there (a child process) and `bench.py --gpus 1` in both
        trees, two passes each, alternating -- the paths this change must not touch.

"group" is the event time of the call's timed launch group (tag "post.fir" of zvx_tag_stats), "wall" the host clock around a call that
waits; medians of --reps runs after --warmup untimed ones.  Next to each group time stands the double-precision FMA rate it amounts to
(K FMAs per emitted sample); the only other double-rate figure the project has is zvx_pitch's 4.3e12 subtract-plus-FMA pairs per second
(profiles/pitch_bench.txt).

    python tools/fir_bench.py [--reps 5] [--warmup 2] [--parent DIR] [--out profiles/fir_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROWS, FRAMES = 32, 1024
TAPS = (63, 255, 511, 1023, 4095)
PIECES, PIECE_FRAMES = 64, 16
SENTENCE = "The quick brown fox jumps over the lazy dog while five wizards pack my box with dozen liquor jugs."
PITCH_PAIRS_PER_S = 4.3e12


def box():
    try:
        out = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=20).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l and ("Instinct" in l or "MI3" in l)]
        return f"{len(names)} x {names[0]}" if names else "unknown GPU"
    except Exception:
        return "unknown GPU"


def paragraph(synth):
    ph, _ = synth.text2phonemeids(SENTENCE)
    T = len(ph)
    dur = [FRAMES // T + (1 if i < FRAMES % T else 0) for i in range(T)]
    return " ".join([SENTENCE] * ROWS), [dur] * ROWS


def time_long(synth, spk, reps, warmup, variants):
    """median wall-clock ms of tts_long per variant (a dict name -> keywords); the variants alternate within a repetition"""
    text, durs = paragraph(synth)
    kw = dict(durations=durs, max_batch=ROWS, max_frames=FRAMES, trim_db=0.0, fade_ms=0)
    ms = {k: [] for k in variants}
    for r in range(warmup + reps):
        for name, extra in variants.items():
            t0 = time.perf_counter()
            wav, seg = synth.tts_long(text, spk, **kw, **extra)
            dt = (time.perf_counter() - t0) * 1e3
            assert len(seg) == ROWS and all(s["mel_len"] == FRAMES for s in seg)
            if r >= warmup:
                ms[name].append(dt)
    return {k: float(np.median(v)) for k, v in ms.items()}


def load(root):
    sys.path.insert(0, root)
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    return synth, spk


def taps_of(K):
    return (np.random.default_rng(K).standard_normal(K) / np.sqrt(K)).astype(np.float32)


def measure(ctx, call, reps, warmup):
    """-> (median group ms from the post.fir tag, median wall ms, launches per call) of call(), which waits for its result"""
    wall = []
    for r in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.set_int("profile", 2)
    group, launches = [], 0
    try:
        for r in range(reps):
            ctx.reset_stats()
            call()
            ctx.sync()
            tag = {t["name"]: t for t in ctx.tag_stats()}["post.fir"]
            group.append(tag["ms"])
            launches = tag["launches"]
    finally:
        ctx.set_int("profile", 0)
    return float(np.median(group)), float(np.median(wall[warmup:])), launches


def torch_child(reps, warmup, n):
    """conv1d on ROWS rows of n samples at every K of TAPS, float32 and float64: {"K,dtype": ms}, device events"""
    import torch
    dev = torch.device("cuda:0")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for dt, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        x = (0.3 * torch.randn((ROWS, 1, n), generator=g, device=dev, dtype=torch.float32)).to(dt)
        for K in TAPS:
            w = torch.randn((1, 1, K), generator=g, device=dev, dtype=torch.float32).to(dt)
            ms = []
            for r in range(warmup + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.nn.functional.conv1d(x, w, padding=(K - 1) // 2)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            print(json.dumps({f"{K},{name}": float(np.median(ms[warmup:]))}), flush=True)


def bench_py(tree, steps, warmup):
    """one pass of bench.py --gpus 1 in `tree` -> ms per step"""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True,
                       cwd=tree, env=dict(os.environ, PYTHONPATH=tree), timeout=900)
    if p.returncode:
        raise SystemExit(f"bench.py in {tree} failed:\n{p.stderr[-2000:]}")
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return float(res["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the baseline of the untouched paths")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--torch-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--torch-timeout", type=int, default=240, help="seconds the torch baseline may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.torch_child:
        torch_child(args.reps, args.warmup, args.torch_child)
        return
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synth, spk = load(os.getcwd() if args.baseline_child else here)
    if args.baseline_child:                                   # (runs inside the parent's tree: no eq keyword there)
        print(json.dumps(time_long(synth, spk, args.reps, args.warmup, {"plain": {}})))
        return
    from zerovox_amd import _lib, equaliser
    ctx = synth.model.ctx
    lib, h_ = ctx._lib, ctx._h
    hop, rate = ctx.hop, ctx.get_int("sampling_rate")
    n = FRAMES * hop
    DEV = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT
    lines = [f"Equaliser FIR (zvx_fir; tools/fir_bench.py): {box()}, 16-bit mode, one process; tile {ctx.get_int('fir_tile')} samples per workgroup.",
             f"group = event time of the launch group (post.fir), wall = host clock around a call that waits; medians of {args.reps} after {args.warmup} warm-ups.",
             f"GFMA/s = K double-precision FMAs per emitted sample over the group time; zvx_pitch reaches {PITCH_PAIRS_PER_S:.1e} subtract-plus-FMA pairs/s (profiles/pitch_bench.txt).", ""]
    print("\n".join(lines), flush=True)

    def add(line):                                            # (every figure is shown as it is taken)
        lines.append(line)
        print(line, flush=True)
    vp = lambda p: C.c_void_p(int(p))

    def fir_call(src, dst, lengths, Nmax, h, stride):
        nn = np.ascontiguousarray(lengths, np.int32)
        K = len(h)
        def call():
            rc = lib.zvx_fir(h_, vp(src), nn.ctypes.data_as(C.c_void_p), len(nn), Nmax, h.ctypes.data_as(C.c_void_p), K, (K - 1) // 2, vp(dst), stride, DEV)
            assert rc == 0, lib.zvx_last_error(h_)
        return call

    rng = np.random.default_rng(1)
    x = (0.3 * rng.standard_normal((ROWS, n))).astype(np.float32)
    lengths = np.full(ROWS, n, np.int32)
    src, dst = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(x.nbytes)
    own = {}
    try:
        ctx.dev_from_host(src, x)
        add(f"(a) {ROWS} rows x {FRAMES} frames ({n} samples per row, {ROWS * n / rate:.1f} s of audio), device rows, out of place:")
        for K in TAPS:
            g, w, l = measure(ctx, fir_call(src, dst, lengths, n, taps_of(K), n), args.reps, args.warmup)
            own[K] = g
            add(f"    K = {K:4d}: group {g:.4f} ms, wall {w:.4f} ms, {K * ROWS * n / g / 1e6:.0f} GFMA/s, {8.0 * ROWS * n / g / 1e6:.0f} GB/s algorithmic")
        n10 = 10 * rate
        g, w, l = measure(ctx, fir_call(src, dst, [n10], n10, taps_of(511), n10), args.reps, args.warmup)
        add(f"(b) one row of 10 s ({n10} samples), K = 511: group {g:.4f} ms, wall {w:.4f} ms, {511 * n10 / g / 1e6:.0f} GFMA/s")
        # (c) 64 pieces of 16 frames with 255 samples of support on either side, in the middle of their signals
        K, piece = 511, PIECE_FRAMES * hop
        h = taps_of(K)
        RL, RR = equaliser.reach(K)
        wlen = RL + piece + RR
        nn = np.full(PIECES, wlen, np.int32)
        win = (_lib.RowWindow * PIECES)(*[_lib.RowWindow(100000, 100000 + RL, piece, 0, 0) for _ in range(PIECES)])
        def rows_call():
            rc = lib.zvx_fir_rows(h_, vp(src), nn.ctypes.data_as(C.c_void_p), PIECES, wlen, h.ctypes.data_as(C.c_void_p), K, RR, vp(dst), wlen, DEV, win)
            assert rc == 0, lib.zvx_last_error(h_)
        n1 = nn[:1].copy()
        def ex_calls():
            for b in range(PIECES):
                rc = lib.zvx_fir_ex(h_, vp(src + b * wlen * 4), n1.ctypes.data_as(C.c_void_p), 1, wlen, h.ctypes.data_as(C.c_void_p), K, RR,
                                    vp(dst + b * wlen * 4), wlen, DEV, 100000, 100000 + RL, piece, 0)
                assert rc == 0, lib.zvx_last_error(h_)
        g1, w1, l1 = measure(ctx, rows_call, args.reps, args.warmup)
        g2, w2, l2 = measure(ctx, ex_calls, args.reps, args.warmup)
        add(f"(c) {PIECES} rows of one {PIECE_FRAMES}-frame piece each ({piece} samples + {RL} / {RR} of support), K = {K}: ONE zvx_fir_rows call: group {g1:.4f} ms "
                     f"({l1} group), wall {w1:.4f} ms; {PIECES} zvx_fir_ex calls: groups {g2:.4f} ms ({l2} groups), wall {w2:.4f} ms")
        h = taps_of(511)
        gi, wi, li = measure(ctx, lambda: ctx.fir_device(src, lengths, n, h), args.reps, args.warmup)
        add(f"(d) (a) at K = 511 in place (filter into the work buffer, copy back): group {gi:.4f} ms, wall {wi:.4f} ms; out of place: group {own[511]:.4f} ms")
    finally:
        ctx.sync()
        ctx.dev_free(src)
        ctx.dev_free(dst)
    res = time_long(synth, spk, args.reps, args.warmup, {"plain": {}, "eq": {"eq": "presence"}})
    add(f"(e) tts_long, {ROWS} sentences of {FRAMES} frames, no equaliser: {res['plain']:.2f} ms; with eq='presence' (K = {equaliser.DEFAULT_TAPS}): {res['eq']:.2f} ms "
                 f"({res['eq'] - res['plain']:+.2f} ms)")
    tool = os.path.abspath(__file__)
    try:                                                      # (a figure per line: what a run that is cut short has measured still counts)
        p = subprocess.run([sys.executable, tool, "--torch-child", str(n), "--reps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=args.torch_timeout)
        got, why = p.stdout, (p.stderr.strip().splitlines() or ["no output"])[-1][:200] if p.returncode else ""
    except subprocess.TimeoutExpired as e:
        got = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        why = f"the child was stopped after {args.torch_timeout} s"
    t = {}
    for l in got.splitlines():
        if l.startswith("{"):
            t.update(json.loads(l))
    if "device" in t:
        add(f"    (the device, as torch names it: {t['device']})")
    add(f"(f) torch.nn.functional.conv1d on the same {ROWS} x {n} device rows (a child process, device events, median of 3), against (a):" + (f" [{why}]" if why else ""))
    for K in TAPS:
        vs = lambda v: f"{v:.4f} ms (zvx_fir takes {own[K] / v:.2f}x of it)" if v is not None else "not measured"
        add(f"    K = {K:4d}: float32 {vs(t.get(f'{K},f32'))}, float64 {vs(t.get(f'{K},f64'))}; zvx_fir {own[K]:.4f} ms")
    if args.parent:
        parent = os.path.abspath(args.parent)
        def fresh_long(tree):                                 # plain tts_long in a fresh process of its own, the same for both trees
            p = subprocess.run([sys.executable, tool, "--baseline-child", "--reps", str(args.reps), "--warmup", str(args.warmup)], capture_output=True, text=True,
                               cwd=tree, env=dict(os.environ, PYTHONPATH=tree), timeout=600)
            if p.returncode:
                raise SystemExit(f"the baseline run in {tree} failed:\n{p.stderr[-2000:]}")
            return json.loads(p.stdout.strip().splitlines()[-1])["plain"]
        longs = [(name, fresh_long(tree)) for _ in range(2) for name, tree in (("the parent", parent), ("this tree", here))]
        add(f"(g) the paths this change does not touch, this tree against the parent commit (its own build), every run a fresh child process, same visit:")
        add("    plain tts_long, ms, two passes each, alternating: " + "; ".join(f"{name} {v:.2f}" for name, v in longs) +
            f" (in THIS process, behind the measurements above and with their work buffers alive: {res['plain']:.2f} ms)")
        del synth
        passes = [(name, bench_py(tree, args.bench_steps, 5)) for _ in range(2) for name, tree in (("this tree", here), ("the parent", parent))]
        add("    bench.py --gpus 1 --steps %d --warmup 5, ms per step, two passes each, alternating: " % args.bench_steps +
                     "; ".join(f"{name} {v:.2f}" for name, v in passes))
    else:
        add("(g) the parent commit's figures: not run (no --parent checkout given)")
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
