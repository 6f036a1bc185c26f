"""The keyed watermark and its detector, milliseconds, next to zvx_denoise on the same rows; and the untouched paths next to the parent
commit's, all in ONE visit of one GPU (16-bit mode, synthetic weights):

    (a) zvx_denoise (strength 0.01), zvx_watermark (the defaults, depth 1 dB) and zvx_watermark_detect (window_frames 256) on 32 device rows
        of 1024 mel frames (262 144 samples each at hop 256), and on ONE row of 10 s; embed and denoise in place;
    (b) ZeroVoxTTS.tts_long of a paragraph of 32 sentences, every sentence forced to 1024 frames: plain, and with watermark=KEY;
    (c) bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline as a child process;
    (d) with --parent DIR, a built checkout of the parent commit: (b) plain and (c) run there in child processes, in the order parent, this,
        parent, this -- the spread between the two passes of one tree is what a difference between the trees is read against.

    (e) with --identify K [K ...]: ONE zvx_watermark_identify call over K candidate keys against K zvx_watermark_detect calls, in this process,
        on the two shapes of (a); the event-timed launches of the identify call (stage tag "post.wmidentify") stand in brackets;
    (f) with --identify: ONE zvx_watermark_rows call over 64 rows with 64 keys against 64 zvx_watermark_ex calls of one row -- the shape of
        tools/rows_bench.py: each row at a position of its own, one 16-frame piece behind the history the stage keeps, device rows, every
        call queued (ZVX_NO_SYNC) and one wait at the end.

Each figure of (a), (b), (e) and (f) is the median of --reps timed runs after --warmup untimed ones (wall clock around calls that wait for
their result).

    python tools/watermark_bench.py [--reps 5] [--warmup 2] [--parent DIR] [--identify 16 256 1024] [--out profiles/watermark_identify.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from denoise_bench import FRAMES, ROWS, box, load, time_long  # noqa: E402

KEY = 0x5EEDC0FFEE
BENCH = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]


def timed(ctx, fn, reps, warmup):
    ms = []
    for _ in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[warmup:]))


def tagged(ctx, fn, tag):
    ctx.set_int("profile", 2)
    ctx.reset_stats()
    fn()
    t = {t["name"]: t for t in ctx.tag_stats()}[tag]
    ctx.set_int("profile", 0)
    return t["ms"]


def calls(synth, rows, n, reps, warmup):
    """-> {name: (wall ms, event-timed ms)} of the three calls on `rows` device rows of n samples"""
    ctx = synth.model.ctx
    rng = np.random.default_rng(1)
    x = (0.3 * rng.standard_normal((rows, n))).astype(np.float32)
    bias = synth.denoise_bias
    lengths = np.full(rows, n, np.int32)
    buf = ctx.dev_alloc(x.nbytes)
    try:
        ctx.dev_from_host(buf, x)
        fns = {"zvx_denoise": (lambda: ctx.denoise_device(buf, lengths, n, bias, 0.01), "post.denoise"),
               "zvx_watermark": (lambda: ctx.watermark_device(buf, lengths, n, KEY), "post.watermark"),
               "zvx_watermark_detect": (lambda: ctx.watermark_detect(None, KEY, lengths=lengths, device_ptr=buf, Nmax=n), "post.wmdetect")}
        return {k: (timed(ctx, f, reps, warmup), tagged(ctx, f, tag)) for k, (f, tag) in fns.items()}
    finally:
        ctx.sync()
        ctx.dev_free(buf)


def identify_lines(synth, counts, reps, warmup):
    """(e): one identify call over K keys against K detect calls, on 32 rows x 1024 frames and on one row of 10 s"""
    ctx = synth.model.ctx
    hop, rate = ctx.hop, ctx.get_int("sampling_rate")
    rng = np.random.default_rng(2)
    out = []
    for rows, n, what in ((1, 10 * rate, "one row of 10 s"), (ROWS, FRAMES * hop, f"{ROWS} rows x {FRAMES} frames")):
        x = (0.3 * rng.standard_normal((rows, n))).astype(np.float32)
        lengths = np.full(rows, n, np.int32)
        buf = ctx.dev_alloc(x.nbytes)
        try:
            ctx.dev_from_host(buf, x)
            for K in counts:
                keys = [int(k) for k in rng.integers(0, 1 << 63, K)]
                one = lambda: ctx.watermark_identify(None, keys, lengths=lengths, device_ptr=buf, Nmax=n)      # noqa: E731
                def many():
                    for k in keys:
                        ctx.watermark_detect(None, k, lengths=lengths, device_ptr=buf, Nmax=n)
                a, b = one(), [ctx.watermark_detect(None, k, lengths=lengths, device_ptr=buf, Nmax=n) for k in keys[:4]]
                same = all(a[r].scores[k] == b[k][r].score for r in range(rows) for k in range(min(K, 4)))
                t_one, t_many = timed(ctx, one, reps, warmup), timed(ctx, many, max(1, reps // 2) if K >= 256 else reps, 1 if K >= 256 else warmup)
                out.append(f"(e) {what}, K = {K}: one zvx_watermark_identify {t_one:.3f} ms [{tagged(ctx, one, 'post.wmidentify'):.3f}]; {K} zvx_watermark_detect "
                           f"calls {t_many:.3f} ms; calls / identify = {t_many / t_one:.1f}x; {1e3 * t_one / K:.1f} us per key; first scores equal: {same}")
        finally:
            ctx.sync()
            ctx.dev_free(buf)
    return out


def rows_line(synth, reps, warmup, B=64):
    """(f): one zvx_watermark_rows call of B rows and B keys against B zvx_watermark_ex calls (the shape of tools/rows_bench.py)"""
    import ctypes as C
    from zerovox_amd import _lib
    ctx = synth.model.ctx
    lib, vp = ctx._lib, C.c_void_p
    R, NEW = ctx.get_int("fft_size") - 1, 16 * ctx.hop
    n = 2 * R + NEW
    x = (np.random.default_rng(1).standard_normal((B, n)) * 0.4).astype(np.float32)
    xd, od = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(x.nbytes)
    flags = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC
    try:
        ctx.dev_from_host(xd, x)
        lens = np.full(B, n, np.int32)
        keys = np.array([KEY + 977 * b for b in range(B)], np.uint64)
        win = (_lib.RowWindow * B)(*[_lib.RowWindow(1000 * b + 7, 1000 * b + 7 + R, NEW, 0, 0) for b in range(B)])
        prms = [_lib.Context._watermark_params(int(k)) for k in keys]

        def a():
            for b in range(B):
                rc = lib.zvx_watermark_ex(ctx._h, vp(xd + 4 * n * b), lens[b:b + 1].ctypes.data_as(vp), 1, n, C.byref(prms[b]), vp(od + 4 * n * b), n, flags,
                                          win[b].in_origin, win[b].out_begin, win[b].out_count, 0)
                assert rc == 0, lib.zvx_last_error(ctx._h)
            ctx.sync()

        def b_():
            rc = lib.zvx_watermark_rows(ctx._h, vp(xd), lens.ctypes.data_as(vp), B, n, C.byref(prms[0]), keys.ctypes.data_as(vp), vp(od), n, flags, win)
            assert rc == 0, lib.zvx_last_error(ctx._h)
            ctx.sync()
        got = []
        for f in (a, b_):
            f()
            got.append(ctx.dev_to_host(od, (B, n), np.uint32)[:, :NEW].copy())
            ctx.dev_from_host(od, np.zeros((B, n), np.float32))
        ta, tb = timed(ctx, a, reps, warmup), timed(ctx, b_, reps, warmup)
        return (f"(f) {B} rows with {B} keys, one 16-frame piece each ({n} samples a row, {NEW} emitted), device rows, queued calls and one wait: {B} "
                f"zvx_watermark_ex calls {ta:.3f} ms; one zvx_watermark_rows call {tb:.3f} ms; calls / rows call = {ta / tb:.1f}x; same bits: "
                f"{bool(np.array_equal(got[0], got[1]))}")
    finally:
        ctx.sync()
        ctx.dev_free(xd)
        ctx.dev_free(od)


def run_bench(root):
    """bench.py in `root` as a child process -> ms per step"""
    p = subprocess.run([sys.executable, "bench.py"] + BENCH, capture_output=True, text=True, cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=900)
    if p.returncode:
        raise SystemExit(f"bench.py in {root} failed:\n{p.stderr[-2000:]}")
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return j.get("ms_per_step", None), j["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its tts_long and bench.py are the baseline")
    ap.add_argument("--long-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--identify", type=int, nargs="+", default=None, metavar="K",
                    help="also time one zvx_watermark_identify call over K keys against K zvx_watermark_detect calls, and the rows call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if args.long_child:                                       # plain tts_long in the tree of the current directory (no watermark keyword needed)
        synth, spk = load(os.getcwd())
        print(json.dumps(time_long(synth, spk, args.reps, args.warmup, {"plain": {}})))
        return

    def long_child(root):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--long-child", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                           capture_output=True, text=True, cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=600)
        if p.returncode:
            raise SystemExit(f"tts_long in {root} failed:\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])["plain"]

    lines = [f"Keyed watermark and detector (tools/watermark_bench.py): {box()}, 16-bit mode.",
             f"median of {args.reps} runs after {args.warmup} warm-ups, wall-clock ms around calls that wait for their result; in brackets the event-timed launches."]
    passes = []
    if args.parent:                                           # parent, this, parent, this: child processes, one at a time
        parent = os.path.abspath(args.parent)
        for name, root in (("parent", parent), ("this", here), ("parent", parent), ("this", here)):
            passes.append((name, long_child(root), run_bench(root)))
    else:
        passes.append(("this", long_child(here), run_bench(here)))
    synth, spk = load(here)
    ctx = synth.model.ctx
    hop, rate = ctx.hop, ctx.get_int("sampling_rate")
    for rows, n, what in ((ROWS, FRAMES * hop, f"{ROWS} rows x {FRAMES} frames ({ROWS * FRAMES * hop / rate:.1f} s of audio)"), (1, 10 * rate, "one row of 10 s")):
        r = calls(synth, rows, n, args.reps, args.warmup)
        lines.append(f"(a) {what}: " + "; ".join(f"{k} {w:.3f} ms [{e:.3f}]" for k, (w, e) in r.items())
                     + f"; embed / denoise {r['zvx_watermark'][0] / r['zvx_denoise'][0]:.2f}x")
    if args.identify:
        lines += identify_lines(synth, args.identify, args.reps, args.warmup)
        lines.append(rows_line(synth, args.reps, args.warmup))
    res = time_long(synth, spk, args.reps, args.warmup, {"plain": {}, "watermark": {"watermark": KEY}})
    lines.append(f"(b) tts_long, {ROWS} sentences of {FRAMES} frames, in this process: plain {res['plain']:.2f} ms; with watermark=KEY {res['watermark']:.2f} ms "
                 f"({res['watermark'] - res['plain']:+.2f} ms)")
    lines.append("(c, d) the untouched paths, child processes in the order run: plain tts_long of the same paragraph; bench.py " + " ".join(BENCH))
    for name, long_ms, (step_ms, value) in passes:
        lines.append(f"    {name:6s}: tts_long {long_ms:.2f} ms; bench.py " + (f"{step_ms:.3f} ms per step, " if step_ms is not None else "") + f"{value:.0f} samples/s")
    if args.parent:
        def spread(v):
            return 100.0 * (max(v) - min(v)) / min(v)
        for label, pick in (("tts_long ms", lambda p: p[1]), ("bench.py samples/s", lambda p: p[2][1])):
            par, this = [pick(p) for p in passes if p[0] == "parent"], [pick(p) for p in passes if p[0] == "this"]
            lines.append(f"    {label}: parent passes differ by {spread(par):.2f} %, this tree's by {spread(this):.2f} %; means: this / parent = "
                         f"{np.mean(this) / np.mean(par):.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
