"""What stepping many stream sessions in one call buys (include/zvx.h: zvx_stream_next_many): N listeners, HiFi-GAN V1 bf16, one 896-frame
mel each, 16-frame chunks, chunks_per_call 1, in one process on one GPU.  A development aid; nothing on the product path imports it.
   python tools/stream_many_bench.py [--denoise S] [--peak-db DB] [--level LUFS] [--watermark KEY] [--out-rate HZ] [--sessions 1,4,16,64] [--no-many] [out.json]
Per chain (the plain chain; with --denoise / --peak-db also denoiser + limiter; with --level and / or --watermark also that chain with the
leveler (3000 ms window, 100 ms look-ahead) and the watermark between them, session i marked with derive_key(KEY, i)) and per N, the median time of one ROUND -- every session
advanced by one piece, host pieces, the call's own wait inside --
   (a) by N zvx_stream_next calls, one after the other,
   (b) by one zvx_stream_next_many,
(one stepping path in the library: (a) is N steps of one session each, (b) one step of N sessions -- the comparison is between N small
batches with N waits and one large batch with one wait, not between two implementations), the two alternating pass by pass over the same mels, the ratio (a) / (b), whether both hand out the same bits, and for (b) the split of a
round between the vocoder stage (zvx_stage_times, profile 1, in passes of their own) and the rest.  The first round of a pass (start-up)
and the last (the stages flush) are not counted.  --no-many times (a) alone: it uses only entry points that exist without the call, so it
runs on a tree that lacks it.  --out-rate HZ opens every session under that output rate (zvx_set_int "out_rate" around the opens), so each
chain ends in the rate conversion; the rows then also carry, from one pass of (b) under profile 2, the time per round of the post
stages' launch groups by tag and the "voc.resample" groups per round."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd import _lib, config as zcfg, weights as zw
from zerovox_amd.model import ZeroVox

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", help="write the result as JSON here")
ap.add_argument("--denoise", type=float, default=None, metavar="S", help="also time the chain denoiser + limiter: the denoiser's strength")
ap.add_argument("--peak-db", type=float, default=None, metavar="DB", help="... and the limiter's ceiling (dBFS); both or neither")
ap.add_argument("--level", type=float, default=None, metavar="LUFS", help="also time the chain with a level stage towards this loudness (zvx_stream_open_ex)")
ap.add_argument("--watermark", type=lambda v: int(v, 0), default=None, metavar="KEY", help="... and / or a watermark stage, session i keyed derive_key(KEY, i)")
ap.add_argument("--out-rate", type=int, default=0, metavar="HZ", help="open the sessions under this output rate (0: the model's own)")
ap.add_argument("--sessions", default="1,4,16,64")
ap.add_argument("--passes", type=int, default=3, help="passes per mode and N (a pass streams every mel to its end)")
ap.add_argument("--no-many", action="store_true", help="mode (a) only")
args = ap.parse_args()
if (args.denoise is None) != (args.peak_db is None):
    ap.error("--denoise and --peak-db go together")

cfg = zcfg.medium_modelcfg("styletts"); sd = zw.tts_state_dict(cfg, 0)
h = zcfg.hifigan_config("v1"); hsd = zw.hifigan_state_dict(h, 0)
model = ZeroVox(cfg, sd, h, hsd, "cuda:0", "bf16")
ctx = model.ctx
L, CHUNK = 896, 16
NS = [int(v) for v in args.sessions.split(",")]
rng = np.random.default_rng(3)
mels = rng.standard_normal((max(NS), L, 80)).astype(np.float32)
chains = {"plain": {}}
if args.denoise is not None:
    from zerovox_amd.longform import limit_keywords
    chains["denoise+limit"] = dict(denoise=dict(strength=float(args.denoise), floor=0.0), bias=model.denoise_bias, limit=limit_keywords(True, 5.0, args.peak_db))
if args.level is not None or args.watermark is not None:
    from zerovox_amd import watermark as WM
    more = {}
    if args.level is not None:
        more["level"] = dict(target=float(args.level), window_ms=3000.0, lookahead_ms=100.0)
    if args.watermark is not None:
        more["watermark"] = lambda i: WM.params(WM.derive_key(args.watermark, i))             # (per session: session_kw below)
    name = "+".join((["denoise"] if args.denoise is not None else []) + sorted(more) + (["limit"] if args.denoise is not None else []))
    chains[name] = dict(chains.get("denoise+limit", {}), **more)


def session_kw(kw, i):
    """the keywords session i is opened with: a callable value is that session's own"""
    return {k: (v(i) if callable(v) else v) for k, v in kw.items()}


def run_pass(N, kw, many, profile=False):
    """streams N mels to their ends -> (round times [s], vocoder stage ms per round or None, the concatenated pieces per session)"""
    ctx.set_int("out_rate", args.out_rate)                   # captured by the sessions as they open
    try:
        streams = [ctx.stream_open(mels[i], chunk_frames=CHUNK, chunks_per_call=1, **session_kw(kw, i)) for i in range(N)]
    finally:
        ctx.set_int("out_rate", 0)
    cap = max(s.info()["max_piece"] for s in streams)
    bufs = [np.empty(cap, np.float32) for _ in range(N)]
    ptrs = [_lib._ptr(b) for b in bufs]
    got = [[] for _ in range(N)]
    ctx.sync()
    rounds, voc = [], []
    while not streams[0].done:
        t0 = time.perf_counter()
        if many:
            n = ctx._stream_next_many(streams, [b.ctypes.data for b in bufs], [cap] * N, 0)
        else:
            n = [s._next(p, cap, 0)[0] for s, p in zip(streams, ptrs)]
        rounds.append(time.perf_counter() - t0)
        if profile:
            voc.append(ctx.stage_times()["vocoder"])
        for i in range(N):
            got[i].append(bufs[i][:n[i]].copy())
    assert all(s.done for s in streams)
    for s in streams:
        s.close()
    return rounds[1:-1], (voc[1:-1] if profile else None), [np.concatenate(g) for g in got]


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


TAGS = ("voc.resample", "post.denoise", "post.level", "post.watermark", "post.limit", "post.stream")


def tag_split(N, kw):
    """one pass of (b) under profile 2 -> ({tag: ms per round}, "voc.resample" launch groups per round), over all rounds of the pass"""
    ctx.set_int("profile", 2)
    try:
        ctx.sync()
        ctx.reset_stats()
        rounds = len(run_pass(N, kw, True)[0]) + 2
        ctx.sync()
        t = {v["name"]: v for v in ctx.tag_stats()}
    finally:
        ctx.set_int("profile", 0)
    return ({k: round(t[k]["ms"] / rounds, 4) for k in TAGS if k in t},
            round(t["voc.resample"]["launches"] / rounds, 2) if "voc.resample" in t else 0.0)


res = {"workload": f"N sessions, one {L}-frame mel each, HiFi-GAN V1 bf16, {CHUNK}-frame chunks, chunks_per_call 1, halo {ZeroVox.STREAM_HALO}, "
                   f"output rate {args.out_rate or 'native'}; "
                   f"median ms per round of {L // CHUNK - 2} rounds x {args.passes} passes", "rows": []}
for name, kw in chains.items():
    for N in NS:
        run_pass(N, kw, False)                               # warm-up: every shape both modes use
        if not args.no_many:
            run_pass(N, kw, True)
        ta, tb, ref, equal = [], [], None, True
        for _ in range(args.passes):                         # the two modes alternate
            r, _, got = run_pass(N, kw, False)
            ta += r
            ref = ref or got
            if not args.no_many:
                r, _, got = run_pass(N, kw, True)
                tb += r
                equal = equal and same(got, ref)
        row = {"chain": name, "N": N, "a_next_ms": round(float(np.median(ta)) * 1e3, 3)}
        if not args.no_many:
            ctx.set_int("profile", 1)
            try:
                r, v, _ = run_pass(N, kw, True, profile=True)
            finally:
                ctx.set_int("profile", 0)
            row.update({"b_next_many_ms": round(float(np.median(tb)) * 1e3, 3), "a_over_b": round(float(np.median(ta) / np.median(tb)), 2),
                        "same_bits": bool(equal), "b_profiled_round_ms": round(float(np.median(r)) * 1e3, 3),
                        "b_vocoder_stage_ms": round(float(np.median(v)), 3),
                        "b_rest_ms": round(float(np.median(r)) * 1e3 - float(np.median(v)), 3)})
            if args.out_rate:
                row["b_tag_ms_per_round"], row["b_resample_groups_per_round"] = tag_split(N, kw)
        res["rows"].append(row)
        print(row, flush=True)
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
