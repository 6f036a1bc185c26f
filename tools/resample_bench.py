"""Cost of the output-rate stage at the headline shape (32 utterances x 128 phonemes, HiFi-GAN V1, queued device-output calls as in
bench.py): the step time with out_rate 0 and with 48000 / 16000 / 8000, f32 and int16 rows, all in ONE process on one GPU, the
settings alternating over several passes so that each one's run-to-run spread is visible next to the differences; then the stage's
own hipEvent time (profile 1, a pass of its own: events on the stream are not free) and its algorithmic bytes per second against the
achievable HBM rate.

    python tools/resample_bench.py [--steps 60] [--passes 4] [--batch 32] [--phonemes 128] [--vocoder v1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd import _lib, config as zcfg, pack, synthetic, weights as zw

HBM_ACHIEVABLE = 6.3e12                                  # bytes/s a streaming kernel reaches on an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--vocoder", default="v1")
    ap.add_argument("--rates", default="0,48000,16000,8000")
    args = ap.parse_args()

    cfg = zcfg.medium_modelcfg("styletts")
    h = zcfg.hifigan_config(args.vocoder)
    man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
    ctx = _lib.Context(man, blob, 0)
    ctx.comm_init(None, 0, 1)                            # as bench.py: the context owns its four streams
    B, T, hop, native = args.batch, args.phonemes, ctx.hop, ctx.get_int("sampling_rate")
    ph, pu, Tlen, spk, dur = synthetic.batch(B, T, first_utt=0, dur_mode="const7")
    L = int(dur[0].sum())
    pad_to = np.full(B, max(689, L), np.int32)
    rates = [int(r) for r in args.rates.split(",")]
    nmax = max(_lib.resampled_len(L * hop, native, r or native) for r in rates)
    bufs = [ctx.dev_alloc(B * nmax * 4) for _ in range(2)]
    settings = [(r, p) for r in rates for p in (False, True)]

    def run(rate, pcm, steps):
        ctx.set_int("out_rate", rate)
        n = ctx.out_samples(L * hop)
        for i in range(steps):
            ctx.synthesize(ph, pu, Tlen, spk, dur, pad_to, want_mel=False, wav_device_ptr=bufs[i & 1], wav_stride=n, no_sync=True, pcm16=pcm)
        ctx.sync()

    for rate, pcm in settings:
        run(rate, pcm, args.warmup)
    ms = {s: [] for s in settings}
    for _ in range(args.passes):                         # the settings alternate: drift of the box lands on all of them alike
        for s in settings:
            t0 = time.perf_counter()
            run(s[0], s[1], args.steps)
            ms[s].append((time.perf_counter() - t0) * 1e3 / args.steps)
    # the stage's own time and bytes, in passes of their own
    stage = {}
    for s in settings:
        if not s[0]:
            continue
        ctx.set_int("profile", 1)
        ev = []
        for _ in range(10):
            run(s[0], s[1], 1)
            ev.append(ctx.resample_ms())
        ctx.set_int("profile", 2); ctx.reset_stats()
        run(s[0], s[1], 1)
        tag = {t["name"]: t for t in ctx.tag_stats()}["voc.resample"]
        ctx.set_int("profile", 0)
        stage[s] = (float(np.median(ev)), float(min(ev)), tag["bytes"] / tag["launches"])
    ctx.set_int("out_rate", 0)

    base = {p: float(np.median(ms[(0, p)])) for p in (False, True)} if 0 in rates else {}
    print(f"headline shape: {B} x {T} phonemes, {L} frames = {L * hop} native samples per row, vocoder {args.vocoder}; {args.passes} passes x {args.steps} steps")
    print(f"{'out_rate':>8} {'rows':>5} {'step ms (median)':>17} {'min':>8} {'max':>8} {'vs off':>8} {'stage ms':>9} {'(min)':>8} {'MB/launch':>10} {'TB/s':>6} {'of HBM':>7}")
    out = []
    for s in settings:
        v = ms[s]
        med = float(np.median(v))
        d = f"{med - base[s[1]]:+8.3f}" if base and s[0] else f"{'':>8}"
        line = f"{s[0]:>8} {'pcm16' if s[1] else 'f32':>5} {med:17.3f} {min(v):8.3f} {max(v):8.3f} {d}"
        rec = {"out_rate": s[0], "pcm16": s[1], "step_ms": v}
        if s in stage:
            e, emin, by = stage[s]
            line += f" {e:9.4f} {emin:8.4f} {by / 1e6:10.2f} {by / (e * 1e-3) / 1e12:6.2f} {by / (e * 1e-3) / HBM_ACHIEVABLE:7.1%}"
            rec.update(stage_ms=e, stage_ms_min=emin, stage_bytes=by)
        print(line)
        out.append(rec)
    print(json.dumps({"resample_bench": out}))


if __name__ == "__main__":
    main()
