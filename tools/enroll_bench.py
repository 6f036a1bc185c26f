"""Speaker enrolment from raw audio, clips per second: 3 s reference clips at 22 050 Hz and at 16 000 Hz, B = 32 and B = 250, all in ONE
process on one GPU (16-bit mode, synthetic weights):

    (a) a loop of ZeroVoxTTS.speaker_embed per clip: resample on the device, trim on the host, zvx_melspec, zvx_spkemb, one clip at a time;
    (b) one ZeroVoxTTS.speaker_embed_batch: zvx_spkemb_wav, the audio never leaves the device;
    (c) ctx.spkemb on the precomputed mels of the same windows: the speaker encoder alone, the floor.

Each figure is the median of --reps timed runs after --warmup untimed ones (wall clock around calls that wait for their result); the
three alternate within a repetition so that drift of the box lands on all of them alike.

    python tools/enroll_bench.py [--reps 5] [--warmup 2] [--seconds 3.0] [--out profiles/enroll_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd.synthesize import ZeroVoxTTS


def make_clips(B, rate, seconds, seed):
    """voiced tones with 0.2 s of near-silence at both ends: the trimmer has something to cut"""
    rng = np.random.default_rng(seed)
    n, q = int(round(seconds * rate)), int(round(0.2 * rate))
    t = np.arange(n - 2 * q) / float(rate)
    clips = []
    for b in range(B):
        f0 = 100.0 + 150.0 * rng.random()
        body = 0.25 * np.sin(2 * np.pi * f0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(len(t))
        clips.append(np.concatenate([1e-4 * rng.standard_normal(q), body, 1e-4 * rng.standard_normal(q)]).astype(np.float32))
    return clips


def box():
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=20).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l and "AMD Instinct" in l]
        return f"{len(names)} x {names[0]}" if names else "unknown GPU"
    except Exception:
        return "unknown GPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--batches", default="32,250")
    ap.add_argument("--rates", default="22050,16000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:tiny", infer_device="cuda:0", precision="bf16")
    ctx = synth.model.ctx
    lines = [f"Speaker enrolment from raw {args.seconds:g} s clips, clips per second (tools/enroll_bench.py): {box()}, 16-bit mode, one process.",
             f"median of {args.reps} runs after {args.warmup} warm-ups; (a) speaker_embed per clip, (b) one speaker_embed_batch (zvx_spkemb_wav), "
             f"(c) ctx.spkemb on precomputed mels", ""]
    for rate in (int(r) for r in args.rates.split(",")):
        for B in (int(b) for b in args.batches.split(",")):
            clips = make_clips(B, rate, args.seconds, seed=B + rate)
            emb, begin, end, frames = ctx.spkemb_wav(clips, rate)
            mels = np.zeros((B, int(frames.max()), ctx.n_mels), np.float32)
            mels[:] = np.random.default_rng(0).standard_normal(mels.shape).astype(np.float32)
            runs = {"a": lambda: [synth.speaker_embed(w, rate) for w in clips],
                    "b": lambda: synth.speaker_embed_batch(clips, rate),
                    "c": lambda: ctx.spkemb(mels, frames)}
            sec = {k: [] for k in runs}
            for i in range(args.warmup + args.reps):
                for k, f in runs.items():
                    t0 = time.perf_counter()
                    f()
                    if i >= args.warmup:
                        sec[k].append(time.perf_counter() - t0)
            a, b, c = (B / float(np.median(sec[k])) for k in "abc")
            worst = float(np.abs(np.stack([synth.speaker_embed(w, rate)[0, 0] for w in clips[:4]]) - emb[:4]).max())
            lines.append(f"{rate:>6} Hz  B = {B:>3}  ({int(frames.min())}-{int(frames.max())} frames per clip):  (a) {a:9.1f}   (b) {b:9.1f}   (c) {c:9.1f} clips/s"
                         f"   (b) / (a) = {b / a:5.1f} x   (b) / (c) = {b / c:5.2f}   max |a - b| over 4 clips {worst:.1e}")
            print(lines[-1], flush=True)
    synth.model.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
