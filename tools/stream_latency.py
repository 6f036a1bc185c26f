"""First-audio latency of the chunked vocoder: one 896-frame mel, HiFi-GAN V1, batch 1.
   python tools/stream_latency.py [out.json]   -> per chunk size: time to the first waveform chunk, time for all chunks, and
   the whole-utterance call for comparison (host mel in, host waveform out: the PCIe copies are inside every figure).
   python tools/stream_latency.py --peak-db DB [--limiter-ms MS] [out.json]   -> the same stream WITH and WITHOUT the windowed limiter
   (zvx_limit_ex at DB dBFS, 4x oversampled envelope), in this one process: first audio, all chunks and the median time between two
   pieces for both, and the samples the limited stream runs behind (limiter.reach).
   python tools/stream_latency.py --denoise S [--peak-db DB] [out.json]   -> the same stream WITH and WITHOUT the windowed denoiser
   (zvx_denoise_ex at strength S with the model's own bias), in this one process: first piece, all pieces, the median piece gap, the
   samples the denoised stream runs behind (denoiser.reach) and whether the pieces equal zvx_denoise of the whole stream bit for bit;
   with --peak-db as well also the combined chain, limit(denoise(stream)).
   python tools/stream_latency.py --resident [--denoise S] [--peak-db DB] [out.json]   -> next to every chain above, in the same process,
   the figures of the same stream run by a stream session of the library (zvx_stream_open; vocode_stream(resident=True)): first piece,
   all pieces, the median piece gap, and whether its concatenation equals the host-planned one bit for bit.
   python tools/stream_latency.py --level LUFS [--denoise S --peak-db DB] [out.json]   -> the same stream WITH and WITHOUT the windowed leveler
   (zvx_level_ex towards LUFS, 3000 ms window, 100 ms look-ahead): first piece, all pieces, the median piece gap, the samples the levelled
   stream runs behind (leveler.reach: RR) and whether the pieces equal zvx_level of the whole stream bit for bit; with --denoise and
   --peak-db as well also the whole chain, limit(level(denoise(stream))).  With --resident the levelled chains are also run by a session
   with a level stage (zvx_stream_open_ex).
   python tools/stream_latency.py --watermark KEY [--level LUFS] [--resident] [out.json]   -> the same stream marked with KEY window by window
   (zvx_watermark_ex, the embedder's defaults), behind the leveler where --level is given: first piece, all pieces, the median piece gap and
   whether the pieces equal the whole-signal calls bit for bit; with --resident also the session with those stages.
   --chunks 16,64 restricts the chunk sizes (default: 16,32,64,128,256)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd import config as zcfg, weights as zw
from zerovox_amd.model import ZeroVox

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", help="write the result as JSON here")
ap.add_argument("--peak-db", type=float, default=None, metavar="DB", help="also time the stream limited at this ceiling (dBFS)")
ap.add_argument("--limiter-ms", type=float, default=5.0, metavar="MS")
ap.add_argument("--denoise", type=float, default=None, metavar="S", help="also time the stream denoised at this strength")
ap.add_argument("--resident", action="store_true", help="also time every chain run by a stream session of the library")
ap.add_argument("--level", type=float, default=None, metavar="LUFS", help="also time the stream levelled towards this short-term loudness")
ap.add_argument("--watermark", type=lambda v: int(v, 0), default=None, metavar="KEY", help="also time the stream marked with this key (behind the leveler with --level)")
ap.add_argument("--chunks", default="16,32,64,128,256", help="the chunk sizes to time, in frames")
args = ap.parse_args()

cfg = zcfg.medium_modelcfg("styletts"); sd = zw.tts_state_dict(cfg, 0)
h = zcfg.hifigan_config("v1"); hsd = zw.hifigan_state_dict(h, 0)
model = ZeroVox(cfg, sd, h, hsd, "cuda:0", "bf16")
ctx = model.ctx
STREAM_HALO = ZeroVox.STREAM_HALO
rng = np.random.default_rng(3)
L = 896
mel = rng.standard_normal((L, 80)).astype(np.float32)
whole = ctx.vocode_mel(mel[None], np.array([L], np.int32))[0]


def best(f, n=20):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def piece_gap(make_stream, n=5):
    """median time between two successive pieces of a stream, ms, over n runs (the first piece, which carries the start-up, is not counted)"""
    gaps = []
    for _ in range(n):
        ts = [time.perf_counter()]
        for _ in make_stream():
            ts.append(time.perf_counter())
        gaps += list(np.diff(ts)[1:])
    return float(np.median(gaps)) * 1e3 if gaps else 0.0


def resident(cf, host_planned, limiter=None, denoise=None, level=None, watermark=None):
    """the figures of one chain run by a stream session, and whether it hands out the host-planned stream's bits"""
    def make():
        return iter(ctx.stream_open(mel, chunk_frames=cf, halo=STREAM_HALO, denoise=denoise, bias=model.denoise_bias if denoise else None,
                                    limit=limiter, **ZeroVox._session_stages(level, watermark)))
    got = np.concatenate(list(make()))
    return {"first_piece_ms": round(best(lambda: next(iter(make()))), 3), "all_pieces_ms": round(best(lambda: list(make()), n=5), 3),
            "piece_gap_ms": round(piece_gap(make), 3),
            "bit_equal_to_host_planned": bool(got.shape == host_planned.shape and np.array_equal(got.view(np.uint32), host_planned.view(np.uint32)))}


res = {"workload": f"one {L}-frame mel ({L * 256 / 22050:.2f} s of audio), HiFi-GAN V1 bf16, batch 1, halo {STREAM_HALO} frames per side",
       "whole_utterance_ms": best(lambda: ctx.vocode_mel(mel[None], np.array([L], np.int32))), "chunks": []}
for cf in [int(v) for v in args.chunks.split(",")]:
    got = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf)))
    first = best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf))))
    total = best(lambda: list(model.vocode_stream(mel, chunk_frames=cf)), n=5)
    res["chunks"].append({"chunk_frames": cf, "chunk_audio_ms": round(cf * 256 / 22.05, 1), "first_chunk_ms": round(first, 3), "all_chunks_ms": round(total, 3),
                          "bit_equal_to_whole": bool(np.array_equal(got, whole)), "max_abs_diff": float(np.abs(got - whole).max())})
    if args.resident:
        res["chunks"][-1]["piece_gap_ms"] = round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf)), 3)
        res["chunks"][-1]["resident"] = resident(cf, got)
    if args.peak_db is not None:
        from zerovox_amd.limiter import reach, window_samples
        from zerovox_amd.longform import limit_keywords
        lim = limit_keywords(True, args.limiter_ms, args.peak_db)
        native = ctx.get_int("sampling_rate")
        limited = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, limiter=lim)))
        want = ctx.limit([whole], rate=native, **lim)[0][0]
        res["chunks"][-1].update({
            "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf)), 3),
            "limited": {"peak_db": args.peak_db, "limiter_ms": args.limiter_ms,
                        "delay_samples": reach(window_samples(native, args.limiter_ms), lim["oversample"]),
                        "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, limiter=lim)))), 3),
                        "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, limiter=lim)), n=5), 3),
                        "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, limiter=lim)), 3),
                        "bit_equal_to_whole_limit": bool(np.array_equal(limited, want)),
                        "samples_changed": int(np.count_nonzero(limited != got))}})
        if args.resident:
            res["chunks"][-1]["limited"]["resident"] = resident(cf, limited, limiter=lim)
    if args.denoise is not None:
        from zerovox_amd.denoiser import reach as denoise_reach
        den = dict(strength=float(args.denoise), floor=0.0)
        bias = model.denoise_bias                            # (first use runs the vocoder: outside every timed region)
        R = denoise_reach(ctx.get_int("fft_size"))
        denoised = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, denoise=den)))
        want = ctx.denoise([whole], bias, **den)[0]
        if "piece_gap_ms" not in res["chunks"][-1]:
            res["chunks"][-1]["piece_gap_ms"] = round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf)), 3)
        res["chunks"][-1]["denoised"] = {
            "strength": args.denoise, "delay_samples": R,
            "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, denoise=den)))), 3),
            "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, denoise=den)), n=5), 3),
            "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, denoise=den)), 3),
            "bit_equal_to_whole_denoise": bool(np.array_equal(denoised.view(np.uint32), want.view(np.uint32))),
            "samples_changed": int(np.count_nonzero(denoised != got))}
        if args.resident:
            res["chunks"][-1]["denoised"]["resident"] = resident(cf, denoised, denoise=den)
        if args.peak_db is not None:
            both = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, denoise=den, limiter=lim)))
            want_both = ctx.limit([want], rate=native, **lim)[0][0]
            res["chunks"][-1]["denoised_limited"] = {
                "delay_samples": R + reach(window_samples(native, args.limiter_ms), lim["oversample"]),
                "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, denoise=den, limiter=lim)))), 3),
                "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, denoise=den, limiter=lim)), n=5), 3),
                "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, denoise=den, limiter=lim)), 3),
                "bit_equal_to_whole_limit_of_denoise": bool(np.array_equal(both.view(np.uint32), want_both.view(np.uint32)))}
            if args.resident:
                res["chunks"][-1]["denoised_limited"]["resident"] = resident(cf, both, denoise=den, limiter=lim)
    if args.level is not None:
        from zerovox_amd.leveler import reach as level_reach
        lvl = dict(target=float(args.level), window_ms=3000.0, lookahead_ms=100.0)
        native = ctx.get_int("sampling_rate")
        levelled = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, level=lvl)))
        want_lvl = ctx.level([whole], rate=native, **lvl)[0][0]
        if "piece_gap_ms" not in res["chunks"][-1]:
            res["chunks"][-1]["piece_gap_ms"] = round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf)), 3)
        res["chunks"][-1]["levelled"] = {
            "level_lufs": args.level, "delay_samples": level_reach(native, lvl["window_ms"], lvl["lookahead_ms"])[1],
            "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, level=lvl)))), 3),
            "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, level=lvl)), n=5), 3),
            "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, level=lvl)), 3),
            "bit_equal_to_whole_level": bool(np.array_equal(levelled.view(np.uint32), want_lvl.view(np.uint32)))}
        if args.resident:
            res["chunks"][-1]["levelled"]["resident"] = resident(cf, levelled, level=lvl)
        if args.denoise is not None and args.peak_db is not None:
            chain = dict(denoise=den, level=lvl, limiter=lim)
            all3 = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, **chain)))
            want3 = ctx.limit([ctx.level([want], rate=native, **lvl)[0][0]], rate=native, **lim)[0][0]
            res["chunks"][-1]["denoised_levelled_limited"] = {
                "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, **chain)))), 3),
                "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, **chain)), n=5), 3),
                "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, **chain)), 3),
                "bit_equal_to_limit_of_level_of_denoise": bool(np.array_equal(all3.view(np.uint32), want3.view(np.uint32)))}
            if args.resident:
                res["chunks"][-1]["denoised_levelled_limited"]["resident"] = resident(cf, all3, denoise=den, level=lvl, limiter=lim)
    if args.watermark is not None:
        from zerovox_amd import watermark as WM
        wm = WM.params(args.watermark)
        lvl_w = dict(target=float(args.level), window_ms=3000.0, lookahead_ms=100.0) if args.level is not None else None
        chain = dict(watermark=wm, **({} if lvl_w is None else dict(level=lvl_w)))
        marked = np.concatenate(list(model.vocode_stream(mel, chunk_frames=cf, **chain)))
        before = whole if lvl_w is None else ctx.level([whole], rate=ctx.get_int("sampling_rate"), **lvl_w)[0][0]
        want_wm = ctx.watermark([before], **wm)[0]
        if "piece_gap_ms" not in res["chunks"][-1]:
            res["chunks"][-1]["piece_gap_ms"] = round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf)), 3)
        name = "marked" if lvl_w is None else "levelled_marked"
        res["chunks"][-1][name] = {
            "first_piece_ms": round(best(lambda: next(iter(model.vocode_stream(mel, chunk_frames=cf, **chain)))), 3),
            "all_pieces_ms": round(best(lambda: list(model.vocode_stream(mel, chunk_frames=cf, **chain)), n=5), 3),
            "piece_gap_ms": round(piece_gap(lambda: model.vocode_stream(mel, chunk_frames=cf, **chain)), 3),
            "bit_equal_to_whole_calls": bool(np.array_equal(marked.view(np.uint32), want_wm.view(np.uint32)))}
        if args.resident:
            res["chunks"][-1][name]["resident"] = resident(cf, marked, **chain)
    print(res["chunks"][-1], flush=True)
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
