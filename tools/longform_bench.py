"""Long-form synthesis against the loop a caller writes without it: paragraphs of 8, 32 and 128 sentences of 64 phonemes each,
StyleTTS decoder + HiFi-GAN V1, bf16, synthetic weights.
   python tools/longform_bench.py [out.json] [--loudness [LUFS]]
Per paragraph, host wall time (median of 20 after 3 warm-ups, same process, same device) of
  (a) one tts() per sentence, mels.trim_silence and np.concatenate on the host -- what the API offered before tts_long, and
  (b) tts_long (batched synthesis into one device buffer, zvx_join on the device, one copy out),
then from one profiled call of (b): the post.join stage time, its algorithmic bytes (zvx_tag_stats) as a fraction of the 8 TB/s HBM
rate, and the vocoder stage time of the same call (the last batch's, where the paragraph needs several).  The ratio (b) / (a) and the
HBM fraction are reported, not gated; the one condition -- post.join below the vocoder's stage time at 32 sentences -- fails the run.
--loudness [LUFS] (default -23): also (c) tts_long(..., loudness=LUFS), timed right after (b) in the same process, the "post.loudness"
launch group of one profiled call of (c), and zvx_normalize alone, in place on 32 x 229 376 device samples (both modes)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd.longform import PAUSES_MS, split_sentences
from zerovox_amd.mels import trim_silence
from zerovox_amd.synthesize import ZeroVoxTTS

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--loudness", type=float, nargs="?", const=-23.0, default=None, metavar="LUFS")
args = ap.parse_args()
HBM_BYTES_PER_S = 8e12
_, synth = ZeroVoxTTS.load_model("synthetic:styletts", "synthetic:v1", infer_device="cuda:0", precision="bf16")
ctx = synth.model.ctx
spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((258, 80)).astype(np.float32))
rate = ctx.get_int("sampling_rate")


def sentence(i):
    """64 phones, whatever the normaliser does to the words"""
    words, s = ["lorem", "ipsum", "dolor", "sit", "amet", "consetetur", "sadipscing", "elitr", "sed", "diam", "nonumy"], ""
    k = i
    while len(synth.text2phonemeids(s)[0]) < 64:
        s += ("" if not s else " ") + words[k % len(words)]
        k += 1
    while len(synth.text2phonemeids(s)[0]) > 64:
        s = s[:-1]
    return s.strip() + "."


def loop(sents):
    """(a): the caller's loop"""
    parts = []
    for i, s in enumerate(sents):
        wav = trim_silence(synth.tts(s, spk)[0], top_db=40)
        parts.append(wav)
        if i + 1 < len(sents):
            parts.append(np.zeros(int(round(PAUSES_MS["."] * rate / 1000.0)), np.float32))
    return np.concatenate(parts)


def median_ms(f, n=20, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


res = {"workload": "paragraphs of N sentences x 64 phonemes, StyleTTS decoder + HiFi-GAN V1 bf16, synthetic weights, predicted durations, "
                   "host waveform out; ms = host wall time, median of 20 after 3 warm-ups", "paragraphs": []}
ok = True
for N in (8, 32, 128):
    sents = [sentence(i) for i in range(N)]
    text = " ".join(sents)
    assert [s for s, _ in split_sentences(text)] == sents
    a = median_ms(lambda: loop(sents))
    b = median_ms(lambda: synth.tts_long(text, spk))
    wav, seg = synth.tts_long(text, spk)
    ctx.set_int("profile", 2); ctx.reset_stats()
    synth.tts_long(text, spk)
    tag = {t["name"]: t for t in ctx.tag_stats()}["post.join"]
    join_ms, voc_ms = ctx.join_ms(), ctx.stage_times()["vocoder"]
    ctx.set_int("profile", 0)
    row = {"sentences": N, "audio_s": round(len(wav) / rate, 2), "loop_tts_trim_concat_ms": round(a, 3), "tts_long_ms": round(b, 3),
           "ratio_b_over_a": round(b / a, 4), "post_join_ms": round(join_ms, 4), "post_join_launch_group_ms": round(tag["ms"], 4),
           "post_join_bytes": tag["bytes"], "post_join_frac_of_8TBps": round(tag["bytes"] / (tag["ms"] * 1e-3) / HBM_BYTES_PER_S, 4),
           "vocoder_ms_last_batch": round(voc_ms, 4), "batches": (N + 31) // 32}
    if args.loudness is not None:
        c = median_ms(lambda: synth.tts_long(text, spk, loudness=args.loudness))
        ctx.set_int("profile", 2); ctx.reset_stats()
        synth.tts_long(text, spk, loudness=args.loudness)
        lt = {t["name"]: t for t in ctx.tag_stats()}["post.loudness"]
        ctx.set_int("profile", 0)
        row.update({"tts_long_loudness_ms": round(c, 3), "loudness_over_plain": round(c / b - 1.0, 4), "post_loudness_launch_group_ms": round(lt["ms"], 4),
                    "post_loudness_bytes": lt["bytes"], "post_loudness_frac_of_plain_tts_long": round(lt["ms"] / b, 4)})
    if N == 32:
        row["post_join_below_vocoder"] = bool(join_ms < voc_ms)
        ok = ok and row["post_join_below_vocoder"]
    res["paragraphs"].append(row)
    print(row, flush=True)
if args.loudness is not None:
    B, n = 32, 229376
    x = (np.random.default_rng(1).standard_normal((B, n)) * 0.05).astype(np.float32)
    buf = ctx.dev_alloc(x.nbytes)
    try:
        alone = {"rows": B, "samples_per_row": n, "rate": rate}
        for common in (False, True):
            ts = []
            ctx.set_int("profile", 2)
            for i in range(8):                            # every call normalises fresh rows; the first three warm up
                ctx.dev_from_host(buf, x)
                ctx.reset_stats()
                ctx.normalize_device(buf, np.full(B, n, np.int32), n, args.loudness, common=common)
                ts.append({t["name"]: t for t in ctx.tag_stats()}["post.loudness"]["ms"])
            ctx.set_int("profile", 0)
            alone["post_loudness_ms_common" if common else "post_loudness_ms_per_row"] = round(float(np.median(ts[3:])), 4)
        res["zvx_normalize_alone"] = alone
        print(alone, flush=True)
    finally:
        ctx.dev_free(buf)
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
sys.exit(0 if ok else 1)
