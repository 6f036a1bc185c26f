"""The vocoder-bias denoiser, milliseconds: 32 rows of 1024 mel frames (262 144 samples each at hop 256), all in ONE process on one GPU
(16-bit mode, synthetic weights):

    (a) zvx_denoise alone, in place on device rows (Context.denoise_device; the two launches and nothing else), strength 0.01;
    (b) ZeroVoxTTS.tts_long of a paragraph of 32 sentences, every sentence forced to 1024 frames, without the denoiser;
    (c) the same paragraph with denoise=0.01;
    (d) with --parent DIR, a built checkout of the parent commit: (b) run there in a child process -- the baseline the default path of
        this tree must not be slower than.

Each figure is the median of --reps timed runs after --warmup untimed ones (wall clock around calls that wait for their result); (b)
and (c) alternate within a repetition so that drift of the box lands on both alike.

    python tools/denoise_bench.py [--reps 5] [--warmup 2] [--parent DIR] [--out profiles/denoise_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROWS, FRAMES = 32, 1024
SENTENCE = "The quick brown fox jumps over the lazy dog while five wizards pack my box with dozen liquor jugs."


def box():
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=20).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l and "AMD Instinct" in l]
        return f"{len(names)} x {names[0]}" if names else "unknown GPU"
    except Exception:
        return "unknown GPU"


def paragraph(synth):
    """-> (text of ROWS sentences, one list of per-phoneme frame counts per sentence summing to FRAMES)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its tts_long of the same paragraph is the baseline")
    ap.add_argument("--baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    # the package of this tree; the baseline child runs this file inside the parent's checkout and takes the package found there
    synth, spk = load(os.getcwd() if args.baseline_child else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if args.baseline_child:                                   # (runs inside the parent's tree: no denoise keyword there)
        print(json.dumps(time_long(synth, spk, args.reps, args.warmup, {"plain": {}})))
        return
    ctx = synth.model.ctx
    hop = ctx.hop
    n = FRAMES * hop
    lines = [f"Vocoder-bias denoiser, {ROWS} rows x {FRAMES} frames ({n} samples per row, hop {hop}) (tools/denoise_bench.py): {box()}, 16-bit mode, one process.",
             f"median of {args.reps} runs after {args.warmup} warm-ups, wall-clock ms around calls that wait for their result."]
    # (a) the denoiser alone, in place on device rows
    rng = np.random.default_rng(1)
    x = (0.3 * rng.standard_normal((ROWS, n))).astype(np.float32)
    bias = synth.denoise_bias
    lengths = np.full(ROWS, n, np.int32)
    buf = ctx.dev_alloc(x.nbytes)
    try:
        ctx.dev_from_host(buf, x)
        alone = []
        for r in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.denoise_device(buf, lengths, n, bias, 0.01)
            alone.append((time.perf_counter() - t0) * 1e3)
        alone = float(np.median(alone[args.warmup:]))
        ctx.set_int("profile", 2)
        ctx.reset_stats()
        ctx.denoise_device(buf, lengths, n, bias, 0.01)
        tag = {t["name"]: t for t in ctx.tag_stats()}["post.denoise"]
        ctx.set_int("profile", 0)
    finally:
        ctx.sync()
        ctx.dev_free(buf)
    audio_s = ROWS * n / float(ctx.get_int("sampling_rate"))
    lines.append(f"(a) zvx_denoise alone, strength 0.01, in place on the device: {alone:.3f} ms per call ({audio_s:.1f} s of audio; event-timed launches "
                 f"{tag['ms']:.3f} ms, {tag['bytes'] / tag['ms'] / 1e6:.0f} GB/s algorithmic, {tag['flops'] / tag['ms'] / 1e9:.2f} TFLOP/s of FFT)")
    res = time_long(synth, spk, args.reps, args.warmup, {"plain": {}, "denoise": {"denoise": 0.01}})
    lines.append(f"(b) tts_long, {ROWS} sentences of {FRAMES} frames, no denoiser: {res['plain']:.2f} ms")
    lines.append(f"(c) the same with denoise=0.01: {res['denoise']:.2f} ms ({res['denoise'] - res['plain']:+.2f} ms)")
    if args.parent:
        tool = os.path.abspath(__file__)
        env = dict(os.environ, PYTHONPATH=os.path.abspath(args.parent))
        p = subprocess.run([sys.executable, tool, "--baseline-child", "--reps", str(args.reps), "--warmup", str(args.warmup)], capture_output=True, text=True,
                           cwd=os.path.abspath(args.parent), env=env, timeout=600)
        if p.returncode:
            raise SystemExit(f"the baseline run in {args.parent} failed:\n{p.stderr[-2000:]}")
        base = json.loads(p.stdout.strip().splitlines()[-1])["plain"]
        lines.append(f"(d) the parent commit, the same paragraph, no denoiser (its own build, a child process): {base:.2f} ms; this tree's default path (b) "
                     f"against it: {res['plain'] - base:+.2f} ms")
    else:
        lines.append("(d) the parent commit's time for the same paragraph: not run (no --parent checkout given)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
