"""The pitch report, milliseconds: the launch-group time of zvx_pitch ("post.pitch" in zvx_tag_stats, hipEvent-timed) at the shapes the other
post-processing tools use -- 32 rows of 1024 mel frames, and the joined waveform of paragraphs of 8, 32 and 128 sentences of 64 phonemes as
ONE row -- with zvx_loudness_stats ("post.loudness") on the same device rows next to it as a yardstick.  Defaults of Context.pitch: 60 ..
500 Hz, window two periods of 60 Hz, the model's hop.  A row of more than 65536 frames is refused by the call (ZVX_E_UNSUPPORTED); such a
row is said so and timed at twice the hop instead.  Median of --reps calls after --warmup; StyleTTS decoder + HiFi-GAN V1 bf16, synthetic
weights.

    python tools/pitch_bench.py [--reps 5] [--warmup 3] [--out profiles/pitch_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zerovox_amd import _lib, pitch as zp                    # noqa: E402
from zerovox_amd.synthesize import ZeroVoxTTS                # noqa: E402

ROWS, FRAMES = 32, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:v1", infer_device="cuda:0", precision="bf16")
    ctx = synth.model.ctx
    rate, hop = ctx.get_int("sampling_rate"), ctx.hop
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((258, 80)).astype(np.float32))
    tmax = zp.tau_max(rate, 60.0)
    W = zp.default_window(rate, 60.0)

    def sentence(i):
        """64 phones, whatever the normaliser does to the words (tools/longform_bench.py's)"""
        words, s = ["lorem", "ipsum", "dolor", "sit", "amet", "consetetur", "sadipscing", "elitr", "sed", "diam", "nonumy"], ""
        k = i
        while len(synth.text2phonemeids(s)[0]) < 64:
            s += ("" if not s else " ") + words[k % len(words)]
            k += 1
        while len(synth.text2phonemeids(s)[0]) > 64:
            s = s[:-1]
        return s.strip() + "."

    def group_ms(call, tag):
        """median launch-group and wall time of `call` in ms"""
        group, wall = [], []
        ctx.set_int("profile", 2)
        try:
            for _ in range(args.warmup + args.reps):
                ctx.reset_stats()
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                group.append({t["name"]: t for t in ctx.tag_stats()}[tag]["ms"])
        finally:
            ctx.set_int("profile", 0)
        return float(np.median(group[args.warmup:])), float(np.median(wall[args.warmup:]))

    def measure(what, x, lens):
        """x [B][Nmax] f32 on the host -> the lines of one shape"""
        B, Nmax = x.shape
        buf = ctx.dev_alloc(x.nbytes)
        try:
            ctx.dev_from_host(buf, x)
            h, note = hop, ""
            if int(lens.max()) // h > _lib.PITCH_MAX_FRAMES:
                try:
                    ctx.pitch_device(buf, lens, Nmax, rate=rate, curves=False)
                    raise SystemExit("a row of more than 65536 frames was not refused")
                except _lib.ZvxError as e:
                    assert e.code == _lib.ZVX_E_UNSUPPORTED
                h = 2 * hop
                note = f" (at hop {hop} the longest row has {int(lens.max()) // hop} frames: refused, ZVX_E_UNSUPPORTED; timed at hop {h})"
            res = ctx.pitch_device(buf, lens, Nmax, rate=rate, hop=h, curves=False)
            frames = int(res["frames"].sum())
            pg, pw = group_ms(lambda: ctx.pitch_device(buf, lens, Nmax, rate=rate, hop=h, curves=False), "post.pitch")
            cg, cw = group_ms(lambda: ctx.pitch_device(buf, lens, Nmax, rate=rate, hop=h, curves=True), "post.pitch")
            lg, lw = group_ms(lambda: ctx.loudness_stats_device(buf, lens, Nmax, rate=rate), "post.loudness")
        finally:
            ctx.sync()
            ctx.dev_free(buf)
        pairs = float(frames) * W * tmax
        return [f"{what}: {B} row(s), {int(lens.astype(np.int64).sum()) / rate:.2f} s of audio, {frames} frames{note}",
                f"  zvx_pitch: group {pg:.4f} ms, wall {pw:.4f} ms ({pairs / pg / 1e9:.2f} T lag-sample pairs/s, each one double subtraction and one double FMA: 2 instructions, 3 flops; "
                f"{int(res['voiced'].sum())} voiced frames); with both curves to the host: group {cg:.4f} ms, wall {cw:.4f} ms",
                f"  zvx_loudness_stats on the same rows: group {lg:.4f} ms, wall {lw:.4f} ms", ""]

    lines = [f"Pitch report (zvx_pitch) at {rate} Hz, 60 .. 500 Hz, window {W}, tau_max {tmax}, hop {hop} (tools/pitch_bench.py): StyleTTS decoder + "
             f"HiFi-GAN V1 bf16, synthetic weights.",
             f"Rows on the device; group = hipEvent time of the launch group (\"post.pitch\" / \"post.loudness\"), wall = host wall time of the call; "
             f"median of {args.reps} after {args.warmup} warm-ups.", ""]
    n = FRAMES * hop
    t = np.arange(n, dtype=np.float64) / rate
    rng = np.random.default_rng(1)
    x = np.stack([(0.2 * (np.sin(2 * np.pi * f * t) + 0.5 * np.sin(4 * np.pi * f * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
                  for f in np.linspace(90.0, 300.0, ROWS)])
    lines += measure(f"{ROWS} rows x {FRAMES} frames (harmonic rows, 90 .. 300 Hz, with noise)", x, np.full(ROWS, n, np.int32))
    print("\n".join(lines), flush=True)
    for N in (8, 32, 128):
        wav, _ = synth.tts_long(" ".join(sentence(i) for i in range(N)), spk)
        out = measure(f"{N} sentences joined", np.ascontiguousarray(wav[None, :], np.float32), np.array([len(wav)], np.int32))
        print("\n".join(out), flush=True)
        lines += out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
