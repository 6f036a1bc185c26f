"""Per-row windows on the MI355X (include/zvx.h: zvx_denoise_rows, zvx_limit_rows, and the batched post stages of zvx_stream_next_many).
The reference of a row is the one-row _ex call with that row's window -- every comparison with it is exact -- and, for the arithmetic, the
float64 restatements tests/denoise_window_ref.py and tests/limit_ref.py under the bounds tests/test_denoise_gpu.py and
tests/test_limiter_gpu.py already hold.  A session stepped with others is compared with the same session stepped alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import denoise_ref as D
import denoise_window_ref as DW
import limit_ref as L
from stream_util import err, same_bits, supported, vp
from zerovox_amd import _lib, config as zcfg, denoiser as DN, limiter as LM, pack, weights as zw

import test_denoise_gpu as TD                                # LIMIT: the bound against the float64 denoiser
import test_stream_denoise_gpu as TSD                        # ctx_for, signal, raw_ex, first_frame
import test_stream_limit_gpu as TSL                          # ctx_for, params, raw_ex
import test_stream_many_gpu as TSM                           # Env

S32, S16 = TSD.SENTINEL32, TSD.SENTINEL16
INV = _lib.ZVX_E_INVALID
STRENGTH, FLOOR = 0.5, 0.1
RATE, CEILING, TILE = TSL.RATE, TSL.CEILING, _lib.LIMIT_TILE
_dn, _lim, _ctx = {}, {}, {}


def windows_array(wins, reserved=None):
    a = (_lib.RowWindow * len(wins))()
    for b, (o, begin, cnt, last) in enumerate(wins):
        a[b] = _lib.RowWindow(int(o), int(begin), int(cnt), int(last), 0 if reserved is None else reserved.get(b, 0))
    return a


def pack_rows(samples, dtype=np.float32):
    """rows of different lengths -> (x [B][odd Nmax] with the sentinel behind every row, n)"""
    n = np.array([len(s) for s in samples], np.int32)
    nmax = max(int(n.max()), 1)
    x = np.full((len(samples), nmax + (nmax % 2 == 0)), S32, np.uint32).view(np.float32)
    for b, s in enumerate(samples):
        x[b, :n[b]] = s
    return x, n


def counts(wins, n):
    return [cnt if cnt >= 0 else max(0, o + int(k) - begin) for (o, begin, cnt, last), k in zip(wins, n)]


def out_rows(B, stride, pcm16):
    return np.full((B + 1, stride), S16, np.int16) if pcm16 else np.full((B + 1, stride), S32, np.uint32)      # one row more than the call owns


def kept(out, b, cnt):
    s = S16 if out.dtype == np.int16 else S32
    return bool(np.all(out[b, cnt:] == s))


# ------------------------------------------------------------------------------------------------ the denoiser
def dn_case(geom):
    """8 rows that differ in every per-row quantity -> (samples, windows, bias); signals of 2000 .. 4000 samples bounded by 1"""
    if geom not in _dn:
        n_fft, hop, wl = geom
        R = DN.reach(n_fft)
        rng = np.random.default_rng(300 + n_fft)

        def begin_for(o, residue):
            """the first output at or behind o + R (0 for o = 0) whose first needed frame is `residue` mod 4"""
            b = o + R if o else 0
            while TSD.first_frame(b, n_fft, hop) % 4 != residue:
                b += 1
            return b

        sig = lambda k: TSD.signal(rng, k, n_fft)
        big = (1 << 33) + 77
        rows = []                                            # (samples, (in_origin, out_begin, out_count, last))
        rows.append((sig(3000), (0, 0, 3000 - R, 0)))                                  # in_origin == 0, not last
        b1 = begin_for(700, 1)
        rows.append((sig(2800), (700, b1, -1, 1)))                                     # last, in_origin > 0 (the signal has 3500 samples)
        rows.append((sig(2500), (0, 0, -1, 1)))                                        # the whole signal
        rows.append((sig(2100), (500, 500 + R + 77, 0, 0)))                            # cnt == 0
        rows.append((sig(0), (0, 0, -1, 1)))                                           # n == 0
        b5 = begin_for(big, 3)
        rows.append((sig(3100), (big, b5, 900, 0)))                                    # in_origin beyond 2^33
        b6 = begin_for(1000, 2)
        rows.append((sig(3000), (1000, b6, 900, 0)))                                   # interior
        b7 = begin_for(2000 + hop, 0)
        rows.append((sig(3999), (2000, b7, 3999 - R - (b7 - 2000), 0)))                # interior, a first frame that is 0 mod 4 and not 0
        samples, wins = [r[0] for r in rows], [r[1] for r in rows]
        for s, (o, begin, cnt, last) in zip(samples, wins):
            c = cnt if cnt >= 0 else max(0, o + len(s) - begin)
            assert supported(R, o, len(s), begin, c, last), (o, begin, cnt, last, len(s))
        firsts = [TSD.first_frame(w[1], n_fft, hop) for s, w in zip(samples, wins) if len(s) and w[2] != 0]
        assert {f % 4 for f in firsts} == {0, 1, 2, 3}, firsts
        assert TSD.first_frame(b7, n_fft, hop) > 0
        med = np.median(np.concatenate([np.abs(D.analysis(s, n_fft, hop, wl)).ravel() for s in samples if len(s)]))
        bias = (med * rng.uniform(0.5, 1.5, n_fft // 2 + 1)).astype(np.float32)
        for a in samples + [bias]:
            a.setflags(write=False)
        _dn[geom] = (samples, wins, bias)
    return _dn[geom]


def dn_ctx(geom):
    """TSD.ctx_for; a hop other than the tiny vocoder's 256 takes a vocoder of two x8 stages, so that prod(upsample_rates) is the hop"""
    if geom[1] == 256:
        return TSD.ctx_for(*geom)
    if geom not in _ctx:
        assert geom[1] == 64
        cfg = zcfg.reduced_modelcfg("styletts")
        cfg["audio"].update(fft_size=geom[0], hop_size=geom[1], win_length=geom[2])
        h = dict(zcfg.hifigan_config("tiny"), upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16])
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
        _ctx[geom] = _lib.Context(man, blob, 0)
    return _ctx[geom]


def raw_dn_rows(ctx, x, n, bias, prm, out, stride, win, flags=0):
    return ctx._lib.zvx_denoise_rows(ctx._h, vp(x), vp(n), len(n), x.shape[1], vp(bias), C.byref(prm), vp(out), stride, flags, win)


def dn_alone(ctx, s, w, bias, prm, pcm16=False):
    """the one-row zvx_denoise_ex call with the row's window -> its emitted samples"""
    k = max(len(s), 1)
    xin = np.zeros(k, np.float32)
    xin[:len(s)] = s
    cnt = counts([w], [len(s)])[0]
    out = out_rows(1, max(k, cnt) + 3, pcm16)
    rc = TSD.raw_ex(ctx, xin, np.array([len(s)], np.int32), k, bias, prm, out, out.shape[1], w, _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, (w, err(ctx))
    return out[0, :cnt].copy()


@pytest.mark.parametrize("geom", [(1024, 256, 1024), (256, 64, 256)])
def test_denoiser_rows_equal_the_one_row_calls(geom):
    """256 / 64: a workgroup holds 16 frames"""
    n_fft, hop, wl = geom
    ctx = dn_ctx(geom)
    assert ctx.get_int("fft_size") == n_fft and ctx.hop == hop
    samples, wins, bias = dn_case(geom)
    x, n = pack_rows(samples)
    B = len(n)
    cnts = counts(wins, n)
    prm = _lib.DenoiseParams(STRENGTH, FLOOR)
    stride = x.shape[1] + 3
    out = out_rows(B, stride, False)
    rc = raw_dn_rows(ctx, x, n, bias, prm, out, stride, windows_array(wins))
    assert rc == 0, err(ctx)
    assert np.all(out[B] == S32)
    worst = 0.0
    for b in range(B):
        cnt = cnts[b]
        assert kept(out, b, cnt), (b, "written beyond cnt_b")
        alone = dn_alone(ctx, samples[b], wins[b], bias, prm)
        assert np.array_equal(out[b, :cnt], alone), (geom, b, wins[b])
        if cnt:
            ref = DW.denoise_window(samples[b], bias, np.float32(STRENGTH), np.float32(FLOOR), *wins[b], n_fft=n_fft, hop=hop, win_length=wl)
            e = float(np.max(np.abs(out[b, :cnt].view(np.float32).astype(np.float64) - ref)))
            print(f"{geom} row {b} window {wins[b]}: {cnt} samples, max |out - ref| = {e:.3e} (limit {TD.LIMIT:.3e})")
            worst = max(worst, e)
            a = wins[b][1] - wins[b][0]
            assert not np.array_equal(out[b, :cnt], samples[b][a:a + cnt].view(np.uint32)), (b, "the denoiser acts")
    assert worst <= TD.LIMIT, worst                          # (measured at 1024 / 256; a 256-point transform has one pass fewer, not more error)
    # int16: the same bits as the one-row call, nothing behind
    out16 = out_rows(B, stride, True)
    assert raw_dn_rows(ctx, x, n, bias, prm, out16, stride, windows_array(wins), _lib.ZVX_PCM16) == 0, err(ctx)
    for b in range(B):
        assert kept(out16, b, cnts[b]) and np.array_equal(out16[b, :cnts[b]], dn_alone(ctx, samples[b], wins[b], bias, prm, True)), b
    # strength 0: a copy of each emitted range
    out0 = out_rows(B, stride, False)
    assert raw_dn_rows(ctx, x, n, bias, _lib.DenoiseParams(0.0, FLOOR), out0, stride, windows_array(wins)) == 0, err(ctx)
    for b in range(B):
        a = wins[b][1] - wins[b][0]
        assert kept(out0, b, cnts[b]) and np.array_equal(out0[b, :cnts[b]], samples[b][a:a + cnts[b]].view(np.uint32)), b


# ------------------------------------------------------------------------------------------------ the limiter
W_MAIN = 110


def lim_case():
    """(signals, rows): rows = (signal number, (in_origin, out_begin, out_count, last), samples); W = 110, R = 231 with os 4"""
    if not _lim:
        rng = np.random.default_rng(808)
        R = LM.reach(W_MAIN, 4)
        loud = lambda k: L.scaled_rows([(rng.standard_normal(k) * np.hanning(k) ** 0.25).astype(np.float32)])[0]
        sig = [loud(4000), loud(3000), (rng.standard_normal(2500) * 0.1).clip(-0.8, 0.8).astype(np.float32), loud(3500), loud(4500)]
        rows = [(0, (300, 300 + R + 70, 1500, 0), 2100)]                                  # off = 301: no multiple of the tile
        rows += [(1, (0, 0, c, 0), c + R + 5) for c in (TILE - 1, TILE, TILE + 1)]        # in_origin == 0; cnt around the tile
        rows.append((2, (0, 0, -1, 1), 2500))                                             # wholly under the ceiling
        rows.append((3, (1500, 1500 + R + 13, -1, 1), 2000))                              # a last row
        rows.append((4, (1024, 1024 + TILE, 1100, 0), TILE + 1100 + R))                   # interior, off a multiple of the tile
        rows.append((0, (1000, 1000 + R, 0, 0), 900))                                     # an empty range
        out = []
        for g, w, k in rows:
            s = np.ascontiguousarray(sig[g][w[0]:w[0] + k])
            assert len(s) == k and (not w[3] or w[0] + k == len(sig[g]))
            c = w[2] if w[2] >= 0 else w[0] + k - w[1]
            assert supported(R, w[0], k, w[1], c, w[3]), w
            s.setflags(write=False)
            out.append((g, w, s))
        assert (out[0][1][1] - out[0][1][0]) % TILE and float(np.abs(sig[2]).max()) < CEILING < float(np.abs(sig[0]).max())
        _lim["case"] = (sig, out)
        _lim["ref"] = {}
    return _lim["case"]


def lim_ref(g, os_):
    sig, _ = lim_case()
    if (g, os_) not in _lim["ref"]:
        _lim["ref"][(g, os_)] = L.limit(sig[g], CEILING, W_MAIN, os_)
    return _lim["ref"][(g, os_)]


def raw_lim_rows(ctx, x, n, prm, out, stride, win, flags=0):
    B = len(n)
    peak, gmin = np.full(B, -7.0, np.float32), np.full(B, -7.0, np.float32)
    rc = ctx._lib.zvx_limit_rows(ctx._h, vp(x), vp(n), B, x.shape[1], RATE, C.byref(prm), vp(out), stride, vp(peak), vp(gmin), flags, win)
    return rc, peak, gmin


def lim_alone(ctx, s, w, prm, pcm16=False):
    cnt = counts([w], [len(s)])[0]
    out = out_rows(1, max(len(s), cnt) + 3, pcm16)
    rc, peak, gmin = TSL.raw_ex(ctx, s, np.array([len(s)], np.int32), len(s), prm, out, out.shape[1], w, _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, (w, err(ctx))
    return out[0, :cnt].copy(), peak[0], gmin[0]


@pytest.mark.parametrize("os_,pcm16", [(4, False), (1, False), (4, True)])
def test_limiter_rows_equal_the_one_row_calls(os_, pcm16):
    ctx = TSL.ctx_for()
    sig, rows = lim_case()
    samples, wins = [r[2] for r in rows], [r[1] for r in rows]
    x, n = pack_rows(samples)
    B = len(n)
    cnts = counts(wins, n)
    assert cnts[1:4] == [TILE - 1, TILE, TILE + 1] and cnts[-1] == 0
    prm = TSL.params(W_MAIN, os_)
    stride = x.shape[1] + 3
    out = out_rows(B, stride, pcm16)
    rc, peak, gmin = raw_lim_rows(ctx, x, n, prm, out, stride, windows_array(wins), _lib.ZVX_PCM16 if pcm16 else 0)
    assert rc == 0, err(ctx)
    s_ = S16 if pcm16 else S32
    assert np.all(out[B] == s_)
    c = float(np.float32(CEILING))
    for b, (g, w, s) in enumerate(rows):
        cnt = cnts[b]
        assert kept(out, b, cnt), (b, "written beyond cnt_b")
        alone, pk, gm = lim_alone(ctx, s, w, prm, pcm16)
        assert np.array_equal(out[b, :cnt], alone), (os_, pcm16, b, w)
        assert same_bits(peak[b], pk) and same_bits(gmin[b], gm), (b, peak[b], pk, gmin[b], gm)
        if cnt == 0:
            assert peak[b] == 0.0 and gmin[b] == 1.0
        if cnt and not pcm16:
            r = lim_ref(g, os_)
            sl = slice(w[1], w[1] + cnt)
            xs = sig[g][sl].astype(np.float64)
            got = out[b, :cnt].view(np.float32)
            e = np.abs(got.astype(np.float64) - r["out"][sl].astype(np.float64))
            bound = np.abs(xs) * (r["E"][sl] / c + 2.0 ** -22)          # tests/test_limiter_gpu.py, check_row
            print(f"os {os_} row {b} window {w}: max err {e.max():.3e}, max err - bound {float(np.max(e - bound)):.3e}")
            assert float(np.max(e - bound)) <= 0.0, (b, int(np.argmax(e - bound)))
            assert np.all(np.abs(got) <= np.float32(CEILING))
            assert abs(float(gmin[b]) - float(r["g32"][sl].min())) <= float(r["E"][sl].max()) / c + 2.0 ** -22, (b, gmin[b])
    if not pcm16:
        assert gmin[4] == 1.0 and np.array_equal(out[4, :cnts[4]], samples[4].view(np.uint32))      # under the ceiling: a copy, beside rows that are not
        assert gmin[0] < 1.0 and gmin[5] < 1.0


# ------------------------------------------------------------------------------------------------ rows do not see each other
def test_rows_are_independent_and_in_place():
    geom = TSD.MAIN
    ctx = TSD.ctx_for(*geom)
    samples, wins, bias = dn_case(geom)
    prm = _lib.DenoiseParams(STRENGTH, FLOOR)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]

    def dn(order):
        x, n = pack_rows([samples[i] for i in order])
        out = out_rows(len(order), x.shape[1], False)
        assert raw_dn_rows(ctx, x, n, bias, prm, out, x.shape[1], windows_array([wins[i] for i in order])) == 0, err(ctx)
        return out
    a, b = dn(range(8)), dn(perm)
    for j, i in enumerate(perm):
        assert np.array_equal(a[i], b[j]), (i, j)            # (the rows have one width: the sentinels behind cnt_b compare too)
    lctx = TSL.ctx_for()
    _, rows = lim_case()
    lprm = TSL.params(W_MAIN, 4)

    def lim(order):
        x, n = pack_rows([rows[i][2] for i in order])
        out = out_rows(len(order), x.shape[1], False)
        rc, peak, gmin = raw_lim_rows(lctx, x, n, lprm, out, x.shape[1], windows_array([rows[i][1] for i in order]))
        assert rc == 0, err(lctx)
        return out, peak, gmin
    (a, pa, ga), (b, pb, gb) = lim(range(8)), lim(perm)
    for j, i in enumerate(perm):
        assert np.array_equal(a[i], b[j]) and same_bits(pa[i], pb[j]) and same_bits(ga[i], gb[j]), (i, j)
    # a subset of the rows: the same bits again
    (c3, p3, g3) = lim([6, 0])
    assert np.array_equal(c3[0, :1100], a[6, :1100]) and np.array_equal(c3[1, :1500], a[0, :1500])
    # in place, out_begin == in_origin on every row (so every window starts its signal)
    R = DN.reach(geom[0])
    ins = [samples[0], samples[2], samples[7], samples[5]]
    iw = [(0, 0, len(ins[0]) - R, 0), (0, 0, -1, 1), (0, 0, 0, 0), (0, 0, 1000, 0)]
    x, n = pack_rows(ins)
    want = out_rows(4, x.shape[1], False)
    assert raw_dn_rows(ctx, x, n, bias, prm, want, x.shape[1], windows_array(iw)) == 0, err(ctx)
    xi = x.copy()
    assert raw_dn_rows(ctx, xi, n, bias, prm, xi, x.shape[1], windows_array(iw)) == 0, err(ctx)
    for b_, cnt in enumerate(counts(iw, n)):
        assert np.array_equal(xi[b_, :cnt].view(np.uint32), want[b_, :cnt]), b_
        assert np.array_equal(xi[b_, cnt:].view(np.uint32), x[b_, cnt:].view(np.uint32)), (b_, "touched outside [0, cnt_b)")
    lins = [rows[1][2], rows[4][2], rows[2][2]]
    lw = [(0, 0, TILE - 1, 0), (0, 0, -1, 1), (0, 0, TILE, 0)]
    x, n = pack_rows(lins)
    want = out_rows(3, x.shape[1], False)
    rc, pw, gw = raw_lim_rows(lctx, x, n, lprm, want, x.shape[1], windows_array(lw))
    assert rc == 0, err(lctx)
    xi = x.copy()
    rc, pi_, gi = raw_lim_rows(lctx, xi, n, lprm, xi, x.shape[1], windows_array(lw))
    assert rc == 0, err(lctx)
    assert same_bits(pw, pi_) and same_bits(gw, gi)
    for b_, cnt in enumerate(counts(lw, n)):
        assert np.array_equal(xi[b_, :cnt].view(np.uint32), want[b_, :cnt]), b_
        assert np.array_equal(xi[b_, cnt:].view(np.uint32), x[b_, cnt:].view(np.uint32)), (b_, "touched outside [0, cnt_b)")


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_row_and_leave_the_context_usable():
    geom = TSD.MAIN
    ctx = TSD.ctx_for(*geom)
    samples, wins, bias = dn_case(geom)
    prm = _lib.DenoiseParams(STRENGTH, FLOOR)
    R = DN.reach(geom[0])
    sel = [0, 6, 2]                                          # in_origin 0 / interior / whole
    x, n = pack_rows([samples[i] for i in sel])
    good = [wins[i] for i in sel]
    stride = x.shape[1]

    def call(w, reserved=None, inplace=False):
        out = x.copy() if inplace else out_rows(3, stride, False)
        rc = raw_dn_rows(ctx, out if inplace else x, n, bias, prm, out, stride, windows_array(w, reserved))
        return rc, out, (err(ctx) or b"").decode()
    rc, want, _ = call(good)
    assert rc == 0
    o, begin, cnt, _ = good[1]
    k = int(n[1])
    bad = {
        "left": ([good[0], (o, o + R - 1, cnt, 0), good[2]], None, False, "row 1"),
        "right": ([good[0], (o, begin, o + k - R - begin + 1, 0), good[2]], None, False, "row 1"),
        "reserved": (good, {2: 1}, False, "row 2"),
        "count": ([good[0], (o, begin, -1, 0), good[2]], None, False, "row 1"),
        "in place": ([(0, 0, 100, 0), (0, 5, 100, 0), (0, 0, -1, 1)], None, True, "row 1"),
    }
    for name, (w, reserved, inplace, row) in bad.items():
        rc, out, msg = call(w, reserved, inplace)
        assert rc == INV and row in msg and "zvx_denoise_rows" in msg, (name, rc, msg)
        if name in ("left", "right"):
            assert "reach R = %d" % R in msg and "1 more sample" in msg, msg
        if inplace:
            assert np.array_equal(out.view(np.uint32), x.view(np.uint32)), name
        else:
            assert np.all(out == S32), (name, "something was written")
        rc, again, _ = call(good)                            # the context still serves
        assert rc == 0 and np.array_equal(again, want), name
    # the limiter's form of the same refusals
    lctx = TSL.ctx_for()
    _, rows = lim_case()
    lprm = TSL.params(W_MAIN, 4)
    RL = LM.reach(W_MAIN, 4)
    lsel = [1, 0, 4]
    lx, ln = pack_rows([rows[i][2] for i in lsel])
    lgood = [rows[i][1] for i in lsel]

    def lcall(w, reserved=None, inplace=False):
        out = lx.copy() if inplace else out_rows(3, lx.shape[1], False)
        rc, peak, gmin = raw_lim_rows(lctx, out if inplace else lx, ln, lprm, out, lx.shape[1], windows_array(w, reserved))
        return rc, out, (err(lctx) or b"").decode()
    rc, lwant, _ = lcall(lgood)
    assert rc == 0
    o, begin, cnt, _ = lgood[1]
    k = int(ln[1])
    lbad = {
        "left": ([lgood[0], (o, o + RL - 1, cnt, 0), lgood[2]], None, False, "row 1"),
        "right": ([lgood[0], (o, begin, o + k - RL - begin + 1, 0), lgood[2]], None, False, "row 1"),
        "reserved": (lgood, {0: -3}, False, "row 0"),
        "count": ([lgood[0], (o, begin, -1, 0), lgood[2]], None, False, "row 1"),
        "in place": ([(0, 0, 100, 0), (0, 0, 100, 0), (0, 1, -1, 1)], None, True, "row 2"),
    }
    for name, (w, reserved, inplace, row) in lbad.items():
        rc, out, msg = lcall(w, reserved, inplace)
        assert rc == INV and row in msg and "zvx_limit_rows" in msg, (name, rc, msg)
        rc, again, _ = lcall(lgood)
        assert rc == 0 and np.array_equal(again, lwant), name
    win = windows_array(lgood)
    assert raw_lim_rows(lctx, lx, ln, lprm, out_rows(3, 100, False), 100, win)[0] == INV      # out_stride below the longest cnt_b (and Nmax)
    assert lctx._lib.zvx_limit_rows(lctx._h, vp(lx), vp(ln), 3, lx.shape[1], RATE, C.byref(lprm), vp(lwant), lx.shape[1], None, None, 0, None) == INV
    assert "win is NULL" in err(lctx).decode()


# ------------------------------------------------------------------------------------------------ many streams
POST = ("post.denoise", "post.limit", "post.stream")


def post_tags(ctx):
    ctx.sync()
    t = {t["name"]: t for t in ctx.tag_stats()}
    return {k: ((t[k]["launches"], t[k]["bytes"]) if k in t else (0, 0.0)) for k in POST}


@pytest.fixture(scope="module")
def env():
    e = TSM.Env("bf16")
    yield e
    e.model.close()


def open_session(env, frames, chunk, cpc, dn=None, lim=None, rate=0):
    ctx = env.ctx
    ctx.set_int("out_rate", rate)
    try:
        return ctx.stream_open(env.mel[:frames], chunk_frames=chunk, chunks_per_call=cpc, halo=16, denoise=dn, bias=env.bias if dn else None, limit=lim)
    finally:
        ctx.set_int("out_rate", 0)


def alone(env, spec):
    """the session stepped alone with zvx_stream_next under profile 2 -> [(piece, tags of the step), ...]"""
    s, out = open_session(env, *spec), []
    while not s.done:
        env.ctx.sync()
        env.ctx.reset_stats()
        piece = s.next_piece().copy()
        out.append((piece, post_tags(env.ctx)))
    s.close()
    return out


def test_many_streams_run_one_group_per_stage(env):
    ctx = env.ctx
    spec = (70, 16, 2, TSM.DN_KW, TSM.LIM_KW, 0)
    ctx.set_int("profile", 2)
    try:
        single = alone(env, spec)
        # (a single step is the n = 1 case of the one stepping path: its history drops are ONE "post.stream" launch too)
        assert all(t["post.denoise"][0] == 1 and t["post.limit"][0] == 1 and t["post.stream"][0] <= 1 for _, t in single), [t for _, t in single]
        assert sum(t["post.stream"][0] for _, t in single) >= 1
        live = [open_session(env, *spec) for _ in range(4)]
        for k, (want, tags) in enumerate(single):
            ctx.sync()
            ctx.reset_stats()
            pieces = ctx.stream_next_many(live)
            many = post_tags(ctx)
            print(k, many, tags)
            assert many["post.denoise"][0] == 1 and many["post.limit"][0] == 1, (k, many)          # ONE timed group per stage and step, not four
            assert many["post.denoise"][1] == 4 * tags["post.denoise"][1] > 0 and many["post.limit"][1] == 4 * tags["post.limit"][1] > 0, (k, many, tags)
            assert many["post.stream"][0] == tags["post.stream"][0] <= 1 and many["post.stream"][1] == 4 * tags["post.stream"][1], (k, many, tags)
            for p in pieces:
                assert len(p) == len(want) and same_bits(p, want), k
        assert all(s.done for s in live)
        for s in live:
            s.close()
    finally:
        ctx.set_int("profile", 0)


def test_many_streams_with_mixed_parameters(env):
    ctx = env.ctx
    lim2 = dict(TSM.LIM_KW, window_ms=2.0)
    dn2 = dict(strength=0.25, floor=0.0)
    specs = [(70, 16, 3, TSM.DN_KW, TSM.LIM_KW, 0),          # denoiser class a, limiter class a
             (33, 7, 2, TSM.DN_KW, lim2, 0),                 # a, b: the 2 ms window
             (70, 16, 1, dn2, None, 0),                      # b, no limiter
             (40, 16, 2, dn2, TSM.LIM_KW, 48000),            # b, a, and a rate conversion
             (70, 16, 2, TSM.DN_KW, TSM.LIM_KW, 0)]          # a, a
    dn_cls, lim_cls = [0, 0, 1, 1, 0], [0, 1, None, 0, 0]
    ctx.set_int("profile", 2)
    try:
        single = [alone(env, sp) for sp in specs]
        live = [(i, open_session(env, *sp)) for i, sp in enumerate(specs)]
        at = [0] * len(specs)
        steps = 0
        while live:
            ctx.sync()
            ctx.reset_stats()
            pieces = ctx.stream_next_many([s for _, s in live])
            many = post_tags(ctx)
            want_dn = {dn_cls[i] for i, _ in live if single[i][at[i]][1]["post.denoise"][0]}
            want_lim = {lim_cls[i] for i, _ in live if single[i][at[i]][1]["post.limit"][0]}
            print(steps, many, sorted(want_dn), sorted(want_lim))
            assert many["post.denoise"][0] == len(want_dn) and many["post.limit"][0] == len(want_lim), (steps, many)
            assert many["post.denoise"][1] == sum(single[i][at[i]][1]["post.denoise"][1] for i, _ in live), steps
            assert many["post.limit"][1] == sum(single[i][at[i]][1]["post.limit"][1] for i, _ in live), steps
            assert many["post.stream"][0] <= 1
            for (i, s), p in zip(live, pieces):
                want = single[i][at[i]][0]
                assert len(p) == len(want) and same_bits(p, want), (steps, i, at[i], len(p), len(want))
                at[i] += 1
                assert s.done == (at[i] == len(single[i])), (i, at[i])
            for _, s in live:
                if s.done:
                    s.close()
            live = [(i, s) for i, s in live if not s.done]
            steps += 1
            assert steps < 50
        assert at == [len(v) for v in single]
        assert any(len(p) for p, _ in single[3]) and steps >= 5
    finally:
        ctx.set_int("profile", 0)
