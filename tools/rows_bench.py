"""What a window per row buys on its own (include/zvx.h: zvx_denoise_rows, zvx_limit_rows, zvx_resample_rows, zvx_level_rows): 64 signals, each
at a position of its own, one 16-frame piece of each -- 4096 new samples behind the history its stage keeps -- through the denoiser, through
the limiter, through the rate conversion (to 48000 and to 8000 Hz) and through the leveler
   (a) by 64 zvx_denoise_ex / zvx_limit_ex / zvx_resample_ex / zvx_level_ex calls of one row,
   (b) by one zvx_denoise_rows / zvx_limit_rows / zvx_resample_rows / zvx_level_rows call of 64 rows,
device rows in and out, everything queued (ZVX_NO_SYNC) and one wait at the end, the two alternating.  A development aid; nothing on the
product path imports it.
   python tools/rows_bench.py [--rows 64] [--reps 30] [--stages denoise,limit,resample,level] [out.json]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zerovox_amd import _lib, config as zcfg, leveler, weights as zw
from zerovox_amd.model import ZeroVox

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", help="write the result as JSON here")
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--stages", default="denoise,limit,resample,level", help="which lines to run, comma-separated")
args = ap.parse_args()

cfg = zcfg.medium_modelcfg("styletts"); h = zcfg.hifigan_config("v1")
model = ZeroVox(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "cuda:0", "bf16")
ctx, lib = model.ctx, model.ctx._lib
B, NEW, RATE = args.rows, 16 * ctx.hop, ctx.get_int("sampling_rate")
n_fft = ctx.get_int("fft_size")
bias = np.ascontiguousarray(model.denoise_bias, np.float32)
dn = _lib.DenoiseParams(0.01, 0.0)
lim = _lib.LimitParams(10 ** (-1 / 20), 5.0, 4)
lvl = _lib.LevelParams(-16.0, 20.0, 3000.0, 100.0)
W = max(1, int(np.rint(RATE * 5.0 / 1000.0)))
F = _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC
vp = C.c_void_p


def bench(name, R, one, rows, ratio=None):
    """rows of 2 R history + NEW samples, row b at in_origin 1000 b + 7: its outputs [in_origin + R, in_origin + R + NEW); with ratio = (L, M)
    the outputs are counted at the output rate: NEW L / M of them from the first one at or behind input position in_origin + R"""
    n = 2 * R + NEW
    x = (np.random.default_rng(1).standard_normal((B, n)) * 0.4).astype(np.float32)
    xd, od = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(x.nbytes * (3 if ratio else 1))
    ctx.dev_from_host(xd, x)
    lens = np.full(B, n, np.int32)
    if ratio:
        Lr, Mr = ratio
        win = (_lib.RowWindow * B)(*[_lib.RowWindow(1000 * b + 7, -(-(1000 * b + 7 + R) * Lr // Mr), NEW * Lr // Mr, 0, 0) for b in range(B)])
        return bench_resample(name, n, x, xd, od, lens, win, one, rows)
    win = (_lib.RowWindow * B)(*[_lib.RowWindow(1000 * b + 7, 1000 * b + 7 + R, NEW, 0, 0) for b in range(B)])

    def a():
        for b in range(B):
            rc = one(vp(xd + 4 * n * b), lens[b:b + 1], n, vp(od + 4 * n * b), win[b])
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        ctx.sync()

    def b_():
        rc = rows(vp(xd), lens, n, vp(od), win)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        ctx.sync()
    got = []
    for f in (a, b_):
        f()
        got.append(ctx.dev_to_host(od, (B, n), np.uint32)[:, :NEW].copy())
        ctx.dev_from_host(od, np.zeros((B, n), np.float32))
    ta, tb = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); a(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b_(); tb.append(time.perf_counter() - t0)
    ctx.dev_free(xd); ctx.dev_free(od)
    row = {"stage": name, "rows": B, "samples_per_row": n, "emitted_per_row": NEW, "a_ex_calls_ms": round(float(np.median(ta)) * 1e3, 3),
           "b_rows_call_ms": round(float(np.median(tb)) * 1e3, 3), "a_over_b": round(float(np.median(ta) / np.median(tb)), 2),
           "same_bits": bool(np.array_equal(got[0], got[1]))}
    print(row, flush=True)
    return row


def bench_resample(name, n, x, xd, od, lens, win, one, rows):
    """the same two loops over output rows of 3 n samples (the counts are at the output rate)"""
    cnt = int(win[0].out_count)
    assert cnt <= 3 * n

    def a():
        for b in range(B):
            rc = one(vp(xd + 4 * n * b), lens[b:b + 1], n, vp(od + 12 * n * b), win[b])
            assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        ctx.sync()

    def b_():
        rc = rows(vp(xd), lens, n, vp(od), win)
        assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
        ctx.sync()
    got = []
    for f in (a, b_):
        f()
        got.append(ctx.dev_to_host(od, (B, 3 * n), np.uint32)[:, :cnt].copy())
        ctx.dev_from_host(od, np.zeros((B, 3 * n), np.float32))
    ta, tb = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); a(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b_(); tb.append(time.perf_counter() - t0)
    ctx.dev_free(xd); ctx.dev_free(od)
    row = {"stage": name, "rows": B, "samples_per_row": n, "emitted_per_row": cnt, "a_ex_calls_ms": round(float(np.median(ta)) * 1e3, 3),
           "b_rows_call_ms": round(float(np.median(tb)) * 1e3, 3), "a_over_b": round(float(np.median(ta) / np.median(tb)), 2),
           "same_bits": bool(np.array_equal(got[0], got[1]) and got[1].any())}
    print(row, flush=True)
    return row


def resample_line(rate_out):
    from zerovox_amd.resample import rate_pair
    Lr, Mr, half = rate_pair(RATE, rate_out)
    return bench(f"resample {RATE} -> {rate_out}", half // Lr + 1,
                 lambda x, l, n, o, w: lib.zvx_resample_ex(ctx._h, x, _lib._ptr(l), 1, n, RATE, rate_out, o, 3 * n, None, F, w.in_origin, w.out_begin, w.out_count),
                 lambda x, l, n, o, w: lib.zvx_resample_rows(ctx._h, x, _lib._ptr(l), B, n, RATE, rate_out, o, 3 * n, None, F, w), ratio=(Lr, Mr))


LINES = {
    "denoise": lambda: [bench("denoise", n_fft - 1,
          lambda x, l, n, o, w: lib.zvx_denoise_ex(ctx._h, x, _lib._ptr(l), 1, n, _lib._ptr(bias), C.byref(dn), o, n, F, w.in_origin, w.out_begin, w.out_count, 0),
          lambda x, l, n, o, w: lib.zvx_denoise_rows(ctx._h, x, _lib._ptr(l), B, n, _lib._ptr(bias), C.byref(dn), o, n, F, w))],
    "limit": lambda: [bench("limit", 2 * W + _lib.LIMIT_ENV_REACH,
          lambda x, l, n, o, w: lib.zvx_limit_ex(ctx._h, x, _lib._ptr(l), 1, n, RATE, C.byref(lim), o, n, None, None, F, w.in_origin, w.out_begin, w.out_count, 0),
          lambda x, l, n, o, w: lib.zvx_limit_rows(ctx._h, x, _lib._ptr(l), B, n, RATE, C.byref(lim), o, n, None, None, F, w))],
    "resample": lambda: [resample_line(48000), resample_line(8000)],
    # the leveler's reach is asymmetric: rows carry RL on both sides (RR < RL), 3 s of history for 186 ms of new samples
    "level": lambda: [bench("level", leveler.reach(RATE, 3000.0, 100.0)[0],
          lambda x, l, n, o, w: lib.zvx_level_ex(ctx._h, x, _lib._ptr(l), 1, n, RATE, C.byref(lvl), o, n, None, None, F, w.in_origin, w.out_begin, w.out_count, 0),
          lambda x, l, n, o, w: lib.zvx_level_rows(ctx._h, x, _lib._ptr(l), B, n, RATE, C.byref(lvl), o, n, None, None, F, w))]}
res = {"workload": f"{B} rows, one 16-frame piece each, device rows, queued calls and one wait; median of {args.reps}",
       "rows": [row for name in args.stages.split(",") for row in LINES[name.strip()]()]}
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
