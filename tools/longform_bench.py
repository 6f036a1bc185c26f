"""Long-form synthesis against the loop a caller writes without it: paragraphs of 8, 32 and 128 sentences of 64 phonemes each,
StyleTTS decoder + HiFi-GAN V1, bf16, synthetic weights.
   python tools/longform_bench.py [out.json] [--loudness [LUFS]]
   python tools/longform_bench.py --limit [out.txt]
   python tools/longform_bench.py --report [out.txt]
Per paragraph, host wall time (median of 20 after 3 warm-ups, same process, same device) of
  (a) one tts() per sentence, mels.trim_silence and np.concatenate on the host -- what the API offered before tts_long, and
  (b) tts_long (batched synthesis into one device buffer, zvx_join on the device, one copy out),
then from one profiled call of (b): the post.join stage time, its algorithmic bytes (zvx_tag_stats) as a fraction of the 8 TB/s HBM
rate, and the vocoder stage time of the same call (the last batch's, where the paragraph needs several).  The ratio (b) / (a) and the
HBM fraction are reported, not gated; the one condition -- post.join below the vocoder's stage time at 32 sentences -- fails the run.
--loudness [LUFS] (default -23): also (c) tts_long(..., loudness=LUFS), timed right after (b) in the same process, the "post.loudness"
launch group of one profiled call of (c), and zvx_normalize alone, in place on 32 x 229 376 device samples (both modes).
--limit [out.txt]: ONLY the limiter, no paragraph is synthesised: the "post.limit" launch group of zvx_limit in place on 32 x 229 376
device samples at 22050 Hz, W = 110 (5 ms), os = 4 and os = 1, on Gaussian rows of sigma 0.3 (a sample over the 0.891 ceiling in nearly
every tile) and of sigma 0.05 (none: every tile takes the copy path); beside it the apply pass of zvx_normalize on the same rows -- the
"post.loudness" group of zvx_normalize minus that of zvx_loudness, the same bytes read and written once -- and the float64 NumPy
reference of tests/limit_ref.py on the same rows on this host.  Medians of 5 after 3 warm-ups; written as text (default
profiles/limiter_bench.txt).
--report [out.txt]: ONLY the programme loudness report: per paragraph the host wall time of tts_long(text, spk) and of the same call with
report=True, plain and under loudness=-23 (medians of 10 after 3 warm-ups, same process); then, on the joined waveform as ONE device row,
the "post.loudness" launch group and the host wall time of zvx_loudness_stats beside those of zvx_loudness, the yardstick that makes the
first two of its four launches, and of zvx_true_peak, the report's other call (medians of 5 after 3 warm-ups).  Written as text (default
profiles/loudness_stats.txt)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd.longform import PAUSES_MS, split_sentences
from zerovox_amd.mels import trim_silence
from zerovox_amd.synthesize import ZeroVoxTTS

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--loudness", type=float, nargs="?", const=-23.0, default=None, metavar="LUFS")
ap.add_argument("--limit", action="store_true")
ap.add_argument("--report", action="store_true")
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


def limiter_bench(out_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import limit_ref
    B, n, ceiling, ms = 32, 229376, 0.891, 5.0
    W = limit_ref.window(rate, ms)
    lens = np.full(B, n, np.int32)
    lines = [f"zvx_limit in place on {B} rows x {n} device samples, {rate} Hz, ceiling {ceiling}, W = {W} ({ms} ms); hipEvent time of the launch group,",
             "median of 5 calls after 3 warm-ups; every call starts from fresh rows.  apply pass = post.loudness(zvx_normalize) - post.loudness(zvx_loudness).", ""]
    buf = ctx.dev_alloc(B * n * 4)
    try:
        for name, sigma in (("dense (sigma 0.3)", 0.3), ("quiet (sigma 0.05)", 0.05)):
            x = (np.random.default_rng(1).standard_normal((B, n)) * sigma).astype(np.float32)

            def group(tag, call):
                ts = []
                ctx.set_int("profile", 2)
                for _ in range(8):
                    ctx.dev_from_host(buf, x)
                    ctx.reset_stats()
                    call()
                    ts.append({t["name"]: t for t in ctx.tag_stats()}[tag]["ms"])
                ctx.set_int("profile", 0)
                return float(np.median(ts[3:]))

            norm = group("post.loudness", lambda: ctx.normalize_device(buf, lens, n, -23.0, rate=rate))
            meas = group("post.loudness", lambda: ctx._chk(ctx._lib.zvx_loudness(ctx._h, buf, lens.ctypes.data, B, n, rate, None, None, _DEVICE_IN)))
            apply_ms = norm - meas
            lines.append(f"{name}: zvx_normalize {norm:.4f} ms, zvx_loudness {meas:.4f} ms -> apply pass {apply_ms:.4f} ms")
            for os_ in (4, 1):
                t = group("post.limit", lambda: ctx.limit_device(buf, lens, n, ceiling, window_ms=ms, oversample=os_, rate=rate))
                lines.append(f"{name}: post.limit os = {os_}: {t:.4f} ms = {t / apply_ms:.2f} x the apply pass "
                             f"({8.0 * B * n / (t * 1e-3) / HBM_BYTES_PER_S:.3f} of 8 TB/s by its 8 bytes per sample)")
            t0 = time.perf_counter()
            for b in range(B):
                limit_ref.limit(x[b], ceiling, W, 4)
            t4 = time.perf_counter() - t0
            t0 = time.perf_counter()
            for b in range(B):
                limit_ref.limit(x[b], ceiling, W, 1)
            t1 = time.perf_counter() - t0
            lines.append(f"{name}: NumPy reference on this host, all rows: os = 4 {t4 * 1e3:.0f} ms, os = 1 {t1 * 1e3:.0f} ms")
            lines.append("")
    finally:
        ctx.dev_free(buf)
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text)


def median_ms(f, n=20, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


if args.limit:
    from zerovox_amd._lib import ZVX_DEVICE_IN as _DEVICE_IN
    limiter_bench(args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "limiter_bench.txt"))
    sys.exit(0)


def report_bench(out_path):
    lines = [f"Programme loudness report (zvx_loudness_stats + zvx_true_peak) on paragraphs of N sentences x 64 phonemes, StyleTTS decoder + HiFi-GAN V1 bf16,",
             f"synthetic weights, {rate} Hz.  tts_long: host wall time, median of 10 after 3 warm-ups.  Calls alone: the joined waveform as ONE device row,",
             "median of 5 after 3 warm-ups; group = hipEvent time of the \"post.loudness\" launch group, wall = host wall time of the call.", ""]
    for N in (8, 32, 128):
        sents = [sentence(i) for i in range(N)]
        text = " ".join(sents)
        plain = median_ms(lambda: synth.tts_long(text, spk), n=10)
        rep = median_ms(lambda: synth.tts_long(text, spk, report=True), n=10)
        loud = median_ms(lambda: synth.tts_long(text, spk, loudness=-23.0), n=10)
        loud_rep = median_ms(lambda: synth.tts_long(text, spk, loudness=-23.0, report=True), n=10)
        wav, _ = synth.tts_long(text, spk, loudness=-23.0, report=True)
        r = synth.last_report
        n = len(wav)
        lens = np.array([n], np.int32)
        buf = ctx.dev_alloc(n * 4)
        try:
            ctx.dev_from_host(buf, wav)

            def alone(call, tag):
                group, wall = [], []
                ctx.set_int("profile", 2)
                for _ in range(8):
                    ctx.reset_stats()
                    t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
                    group.append({t["name"]: t for t in ctx.tag_stats()}[tag]["ms"])
                ctx.set_int("profile", 0)
                return float(np.median(group[3:])), float(np.median(wall[3:]))

            st = alone(lambda: ctx.loudness_stats_device(buf, lens, n, rate=rate), "post.loudness")
            ld = alone(lambda: ctx._chk(ctx._lib.zvx_loudness(ctx._h, buf, lens.ctypes.data, 1, n, rate, None, None, _DEVICE_IN)), "post.loudness")
            tp = alone(lambda: ctx.true_peak_device(buf, lens, n, rate=rate), "post.limit")
        finally:
            ctx.dev_free(buf)
        lines += [f"{N} sentences, {n / rate:.2f} s of audio, {n // ((rate + 5) // 10) - 29} short-term windows: {r}",
                  f"  tts_long {plain:.3f} ms, with report {rep:.3f} ms ({(rep / plain - 1.0) * 100.0:+.2f} %); under loudness=-23 {loud:.3f} ms, "
                  f"with report {loud_rep:.3f} ms ({(loud_rep / loud - 1.0) * 100.0:+.2f} %)",
                  f"  zvx_loudness_stats: group {st[0]:.4f} ms, wall {st[1]:.4f} ms; zvx_loudness: group {ld[0]:.4f} ms, wall {ld[1]:.4f} ms; "
                  f"zvx_true_peak (4x): group {tp[0]:.4f} ms, wall {tp[1]:.4f} ms", ""]
        print("\n".join(lines[-4:]), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))


if args.report:
    from zerovox_amd._lib import ZVX_DEVICE_IN as _DEVICE_IN
    report_bench(args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loudness_stats.txt"))
    sys.exit(0)
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
