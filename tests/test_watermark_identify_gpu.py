"""Per-request watermark keys on the MI355X: zvx_watermark_identify against K zvx_watermark_detect calls and zvx_watermark_rows against
zvx_watermark_ex on each row alone, both bit for bit; the device-built sign tables through those equalities (the single-key calls read a
table built on the host, which tests/test_watermark.py holds to watermark.sign_table); identification among 64 keys end to end; and the
table of refusals.  Nothing here has a tolerance: every comparison is of bit patterns, or of decisions the float64 reference made with
margins of more than 1 in the score (tests/test_watermark_identify.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import denoise_ref as D
import watermark_ref as W
from stream_util import err, same_bits, vp
from test_watermark_identify import CUT, KEYS, check_identification, clean_rows, device_sign_rule, key_of_row
from zerovox_amd import _lib, config as zcfg, pack, watermark as WM, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
N_FFT, HOP, RATE = 1024, 256, 22050
PAD = (N_FFT - HOP) // 2
KEY = 0xC0FFEE1234567
DEFAULT = dict(WM.EMBED_DEFAULTS)
INV, UNSUP = 1, 6
KC = 8                                                       # keys per workgroup of the search (watermark_kernels.h, WM_KEYS)
_ctx, _sig = {}, {}


def ctx_for():
    if "c" not in _ctx:
        cfg = zcfg.reduced_modelcfg("styletts")
        cfg["audio"].update(fft_size=N_FFT, hop_size=HOP, win_length=N_FFT)
        h = zcfg.hifigan_config("tiny")
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), "bf16")
        _ctx["c"] = _lib.Context(man, blob, 0)
        assert _ctx["c"].get_int("fft_size") == N_FFT and _ctx["c"].hop == HOP and _ctx["c"].get_int("sampling_rate") == RATE
    return _ctx["c"]


def prm_of(p, key=KEY):
    return _lib.WatermarkParams(key, p["depth_db"], p["lo_hz"], p["hi_hz"], p["block_frames"], p["band_bins"], p["period_blocks"], 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- zvx_watermark_identify against K zvx_watermark_detect calls -----------------------------------------------------------------------
# 19 keys: not a multiple of the 8 a workgroup serves, three key chunks; keys 4 and 17 repeat keys 0 and 9
CAND = [W.mix64(0xABCD + 977 * k) for k in range(19)]
CAND[4], CAND[17] = CAND[0], CAND[9]
assert len(CAND) % KC != 0 and len(CAND) > 2 * KC
PARAM_SETS = {
    "defaults": DEFAULT,
    "P1": {**DEFAULT, "period_blocks": 1},
    "P3": {**DEFAULT, "period_blocks": 3},
    "P100": {**DEFAULT, "period_blocks": 100},               # two slices of the table's rows share the workgroup
    # 510 columns: 11 band runs of 48.  Two phases, not the default eight: a workgroup's time grows with P J block_frames whatever the window
    "P256_J512": {**DEFAULT, "period_blocks": 256, "band_bins": 1, "lo_hz": 0.0, "hi_hz": 11025.0, "block_frames": 2},
    "TB1": {**DEFAULT, "block_frames": 1},
    "narrow": {**DEFAULT, "hi_hz": 4000.0},                  # a narrower band than the rows were marked with
}


def identify_rows():
    """three ragged rows of 0.4 .. 1.2 s, the middle one empty; the first carries CAND[2]'s mark, the last CAND[11]'s (on the device)"""
    if "id" not in _sig:
        ctx = ctx_for()
        a, b = W.voiced_signal(0.4, 31), W.voiced_signal(1.2, 32)
        ya, yb = ctx.watermark([a], CAND[2])[0], ctx.watermark([b], CAND[11])[0]
        n = np.array([len(a), 0, len(b)], np.int32)
        x = np.full((3, len(b) + 1), SENTINEL32, np.uint32).view(np.float32)            # nothing behind a row's end may be read
        x[0, :n[0]], x[2, :n[2]] = ya[:n[0]], yb[:n[2]]
        x.setflags(write=False)
        _sig["id"] = (x, n)
    return _sig["id"]


def raw_detect(ctx, xp, n, Nmax, p, key, wf, flags=0):
    B = len(n)
    sc, of, wi = np.full(B, np.nan, np.float32), np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    prm = prm_of(p, key)
    rc = ctx._lib.zvx_watermark_detect(ctx._h, xp, vp(n), B, Nmax, C.byref(prm), wf, vp(sc), vp(of), vp(wi), None, None, 0, flags)
    assert rc == 0, err(ctx)
    return sc, of, wi


def raw_identify(ctx, xp, n, Nmax, p, keys, wf, flags=0, K=None, outs=None, prm=None):
    B = len(n)
    K = len(keys) if K is None else K
    ka = None if keys is None else np.array(keys, np.uint64)
    if outs is None:
        outs = [np.full((B, max(K, 1)), np.nan, np.float32), np.full((B, max(K, 1)), -7, np.int32), np.full((B, max(K, 1)), -7, np.int32),
                np.full(B, -7, np.int32)]
    prm = prm_of(p, 0xBAD) if prm is None else prm             # params->key is not read
    rc = ctx._lib.zvx_watermark_identify(ctx._h, xp, vp(n), B, Nmax, None if prm is False else C.byref(prm), vp(ka), K, wf, *[vp(o) for o in outs], flags)
    return rc, outs


@pytest.mark.parametrize("wf", [0, 2, 64, 200])             # 64: a clipped last window; 200: larger than every row
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_identify_equals_k_detect_calls_bit_for_bit(name, wf):
    """K = 1, 3 and 19 (three key chunks, the last one of 3 keys; two duplicates) on host rows, K = 3 on device rows as well"""
    ctx = ctx_for()
    p = PARAM_SETS[name]
    x, n = identify_rows()
    Nmax = x.shape[1]
    F = [D.geometry(int(k), N_FFT, HOP)[1] if k else 0 for k in n]
    assert F[2] == 103 and F[0] < 64                          # 64: three windows on the long row, the last one clipped; the short row: one
    single = [raw_detect(ctx, vp(x), n, Nmax, p, key, wf) for key in CAND]
    dev = ctx.dev_alloc(x.nbytes)
    try:
        ctx.dev_from_host(dev, x)
        for K, xp, flags in ((1, vp(x), 0), (3, vp(x), 0), (3, vp(dev), _lib.ZVX_DEVICE_IN), (len(CAND), vp(x), 0)):
            rc, (sc, of, wi, best) = raw_identify(ctx, xp, n, Nmax, p, CAND[:K], wf, flags)
            assert rc == 0, (name, wf, K, err(ctx))
            for k in range(K):
                assert np.array_equal(bits(sc[:, k]), bits(single[k][0])), (name, wf, K, k, sc[:, k], single[k][0])
                assert np.array_equal(of[:, k], single[k][1]) and np.array_equal(wi[:, k], single[k][2]), (name, wf, K, k)
            assert np.all(sc[1] == 0.0) and np.all(of[1] == 0) and np.all(wi[1] == 0) and best[1] == 0      # the empty row
            for b in range(3):
                assert best[b] == int(np.argmax(sc[b])), (name, wf, K, b)               # argmax: the first of equals
        # duplicate keys: the same bits
        assert np.array_equal(bits(sc[:, 4]), bits(sc[:, 0])) and np.array_equal(bits(sc[:, 17]), bits(sc[:, 9]))
    finally:
        ctx.dev_free(dev)


def test_the_wrapper_agrees_with_watermark_detect():
    ctx = ctx_for()
    x, n = identify_rows()
    kw = {k: v for k, v in DEFAULT.items() if k != "depth_db"}
    res = ctx.watermark_identify(x, CAND, lengths=n, window_frames=64, **kw)
    one = ctx.watermark_detect(x, CAND[11], lengths=n, window_frames=64, **kw)
    assert [r.scores[11] for r in res] == [o.score for o in one]
    print(f"marked rows: best {[(r.best, round(r.score, 2), round(r.margin, 2)) for r in res]}")
    assert res[2].best == 11 and res[2].key == CAND[11] and res[2].detected and res[2].margin > 2.0
    assert (res[2].offset, res[2].window) == (one[2].offset, one[2].window) and len(res[2].scores) == len(CAND)


def test_the_smallest_index_wins_among_equal_scores():
    ctx = ctx_for()
    x, n = identify_rows()
    keys = [CAND[11], CAND[3], CAND[11], CAND[11]]
    rc, (sc, of, wi, best) = raw_identify(ctx, vp(x), n, x.shape[1], DEFAULT, keys, 64)
    assert rc == 0, err(ctx)
    assert best[2] == 0 and bits(sc[2, 0]) == bits(sc[2, 2]) == bits(sc[2, 3]) and sc[2, 0] > sc[2, 1]
    rc, (sc, of, wi, best) = raw_identify(ctx, vp(x), n, x.shape[1], DEFAULT, keys[1:], 64)
    assert rc == 0 and best[2] == 1


# ---- zvx_watermark_rows against zvx_watermark_ex on each row alone ----------------------------------------------------------------------
SMALL = dict(depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=2, band_bins=2, period_blocks=2)
R = WM.reach(N_FFT)


def rows_case():
    """4 rows at 4 stream positions, 3 distinct keys (rows 0 and 3 share one): from the start; from the middle; to the end (last); and a
    row that emits nothing -> (rows, windows, keys)"""
    if "rows" not in _sig:
        rng = np.random.default_rng(99)
        sig = [np.clip(0.4 * rng.standard_normal(k), -1, 1).astype(np.float32) for k in (6007, 9001, 5003, 4000)]
        rows = [sig[0][:3000 + R], sig[1][2500 - R:5100 + R], sig[2][1800 - R:], sig[3][700:700 + 2 * R + 300]]
        windows = [(0, 0, 3000, 0), (2500 - R, 2500, 2600, 0), (1800 - R, 1800, -1, 1), (700, 700 + R, 0, 0)]
        keys = [KEYS[1], KEYS[2], KEYS[3], KEYS[1]]
        _sig["rows"] = ([np.ascontiguousarray(r) for r in rows], windows, keys)
    return _sig["rows"]


def raw_rows(ctx, x, n, Nmax, prm, keys, out, stride, win, flags=0):
    wa = (_lib.RowWindow * len(win))(*[_lib.RowWindow(int(w[0]), int(w[1]), int(w[2]), int(w[3]), 0) for w in win]) if win is not None else None
    ka = None if keys is None else np.array(keys, np.uint64)
    return ctx._lib.zvx_watermark_rows(ctx._h, vp(x), vp(n), len(n), Nmax, C.byref(prm) if prm is not None else None, vp(ka), vp(out), stride, flags, wa)


def alone(ctx, row, window, p, key, pcm16=False):
    """zvx_watermark_ex on one row"""
    return ctx.watermark_window([row], key, in_origin=window[0], out_begin=window[1], out_count=window[2], last=bool(window[3]), pcm16=pcm16, **p)[0]


def padded(rows):
    n = np.array([len(r) for r in rows], np.int32)
    x = np.full((len(rows), int(n.max()) + 1), SENTINEL32, np.uint32).view(np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


@pytest.mark.parametrize("name", ["small", "default"])
def test_rows_call_equals_the_single_row_calls_bit_for_bit(name):
    ctx = ctx_for()
    p = SMALL if name == "small" else DEFAULT
    rows, windows, keys = rows_case()
    x, n = padded(rows)
    Nmax = x.shape[1]
    want = [alone(ctx, rows[b], windows[b], p, keys[b]) for b in range(4)]
    cnt = [len(w) for w in want]
    assert cnt == [3000, 2600, len(rows[2]) - R, 0]
    stride = Nmax + 3
    out = np.full((4, stride), SENTINEL32, np.uint32)
    assert raw_rows(ctx, x, n, Nmax, prm_of(p, 0xBAD), keys, out, stride, windows) == 0, err(ctx)
    for b in range(4):
        assert np.array_equal(out[b, :cnt[b]], bits(want[b])), (name, b)
        assert np.all(out[b, cnt[b]:] == SENTINEL32), (name, b)                          # nothing outside [0, cnt_b) is written
    # the device's tables are the Python side's: rows 0 and 3 share a key and a table; another key on row 1 alone moves row 1 alone
    assert not same_bits(alone(ctx, rows[1], windows[1], p, keys[0]), want[1])
    other = np.full((4, stride), SENTINEL32, np.uint32)
    assert raw_rows(ctx, x, n, Nmax, prm_of(p), [keys[0], keys[0], keys[2], keys[1]], other, stride, windows) == 0, err(ctx)
    assert np.array_equal(other[0], out[0]) and np.array_equal(other[2], out[2]) and not np.array_equal(other[1], out[1])
    assert np.array_equal(other[1, :cnt[1]], bits(alone(ctx, rows[1], windows[1], p, keys[0])))
    # keys == NULL: params->key for every row
    null = np.full((4, stride), SENTINEL32, np.uint32)
    assert raw_rows(ctx, x, n, Nmax, prm_of(p, keys[2]), None, null, stride, windows) == 0, err(ctx)
    for b in range(4):
        assert np.array_equal(null[b, :cnt[b]], bits(alone(ctx, rows[b], windows[b], p, keys[2]))) and np.all(null[b, cnt[b]:] == SENTINEL32), b
    # the wrapper, and PCM16 (not in place)
    via = ctx.watermark_rows(rows, keys, windows, **p)
    assert all(same_bits(via[b], want[b]) for b in range(4))
    pcm = ctx.watermark_rows(rows, keys, windows, pcm16=True, **p)
    assert all(np.array_equal(pcm[b], alone(ctx, rows[b], windows[b], p, keys[b], pcm16=True)) and pcm[b].dtype == np.int16 for b in range(4))
    assert all(np.array_equal(pcm[b], D.pcm16(want[b])) for b in range(3))
    # depth 0: a copy of each row's outputs, whatever the keys
    zero = ctx.watermark_rows(rows, keys, windows, **{**p, "depth_db": 0.0})
    assert all(same_bits(zero[b], rows[b][windows[b][1] - windows[b][0]:][:cnt[b]]) for b in range(4))


def test_rows_call_in_place_and_whole_rows():
    """in place needs out_begin == in_origin: whole rows (windows None in the wrapper) with a key each, against zvx_watermark per row"""
    ctx = ctx_for()
    rows = [r for r in clean_rows()[:1]] + [W.voiced_signal(0.4, 33), W.voiced_signal(0.7, 34)]
    keys = [KEYS[7], KEYS[8], KEYS[7]]
    want = [ctx.watermark([r], k)[0] for r, k in zip(rows, keys)]
    x, n = padded(rows)
    win = [(0, 0, -1, 1)] * 3
    assert raw_rows(ctx, x, n, x.shape[1], prm_of(DEFAULT, 0), keys, x, x.shape[1], win) == 0, err(ctx)
    for b in range(3):
        assert same_bits(x[b, :n[b]], want[b][:n[b]]) and np.all(x.view(np.uint32)[b, n[b]:] == SENTINEL32), b
    via = ctx.watermark_rows(rows, keys)
    assert all(same_bits(via[b], want[b][:n[b]]) for b in range(3))
    y = np.zeros_like(x)                                      # PCM16 in place is refused, as zvx_denoise_rows refuses it
    assert raw_rows(ctx, y, n, x.shape[1], prm_of(DEFAULT, 0), keys, y, x.shape[1], win, flags=_lib.ZVX_PCM16) == INV


def test_device_sign_tables_equal_the_python_tables():
    """k_wm_signs through the calls that use it: a one-row zvx_watermark_rows with key k (device table) equals zvx_watermark_ex with key
    k (host table) bit for bit, and a different table would not: flipping ONE sign of the Python table changes the float64 reference by
    far more than an f32 ulp.  Keys 0 and 2^64 - 1 are the hash's corners."""
    ctx = ctx_for()
    row = np.ascontiguousarray(clean_rows()[0][:8000])
    for p in (SMALL, DEFAULT, {**DEFAULT, "period_blocks": 3, "band_bins": 1, "lo_hz": 0.0, "hi_hz": 11025.0}):
        keys = [0, (1 << 64) - 1, KEY]
        got = ctx.watermark_rows([row] * 3, keys, **p)
        for b, key in enumerate(keys):
            assert same_bits(got[b], ctx.watermark([row], key, **p)[0][:len(row)]), (p, key)
        assert not same_bits(got[0], got[1]) and not same_bits(got[0], got[2])
        J = W.bands(p["lo_hz"], p["hi_hz"], p["band_bins"], N_FFT, RATE)[1]
        assert np.array_equal(device_sign_rule(keys, p["period_blocks"], J)[2], np.array(WM.sign_table(KEY, p["period_blocks"], J)))
    # identify reads the same device tables: a key's score is the host-table detector's (the bit-equality test above), here on the corners
    x, n = identify_rows()
    for key in (0, (1 << 64) - 1):
        rc, (sc, of, wi, best) = raw_identify(ctx, vp(x), n, x.shape[1], DEFAULT, [key], 0)
        assert rc == 0 and np.array_equal(bits(sc[:, 0]), bits(raw_detect(ctx, vp(x), n, x.shape[1], DEFAULT, key, 0)[0]))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_mark_four_rows_with_four_keys_and_identify_among_64():
    ctx = ctx_for()
    clean = clean_rows()
    marked = ctx.watermark_rows(clean, [KEYS[key_of_row(b)] for b in range(4)])
    assert all(len(m) == len(c) and not same_bits(m, c) for m, c in zip(marked, clean))
    rm = ctx.watermark_identify(marked, KEYS)
    rc_ = ctx.watermark_identify(clean, KEYS)
    cut = ctx.watermark_identify([m[CUT:] for m in marked], KEYS)
    check_identification([r.scores for r in rm], [r.scores for r in rc_], [cut[b].scores[key_of_row(b)] for b in range(4)])
    for b in range(4):
        assert rm[b].best == key_of_row(b) and rm[b].detected and rm[b].offset == 0 and not rc_[b].detected
        assert cut[b].best == key_of_row(b) and cut[b].offset in (19, 20)               # 5000 / 256 = 19.5 frames


# ---- validation -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    ctx = ctx_for()
    x, n = identify_rows()
    Nmax = x.shape[1]
    xp = vp(x)
    rc, want = raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64)
    assert rc == 0, err(ctx)

    def still_fine():
        rc2, got = raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64)
        assert rc2 == 0 and all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)), err(ctx)

    fresh = lambda: [np.zeros((3, 3), np.float32), np.zeros((3, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros(3, np.int32)]      # noqa: E731
    cases = [("keys NULL", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, None, 64, K=3)[0], INV)]
    for i, what in enumerate(("score", "offset", "window", "best")):
        outs = fresh()
        outs[i] = None
        cases.append((what + " NULL", lambda o=outs: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, outs=o)[0], INV))
    cases += [
        ("K 0", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, K=0)[0], INV),
        ("K -1", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, K=-1)[0], INV),
        ("window_frames 1", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 1)[0], INV),
        ("window_frames -1", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], -1)[0], INV),
        ("params NULL", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, prm=False)[0], INV),
        ("flags", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, flags=_lib.ZVX_PCM16)[0], INV),
        ("no sync", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, flags=_lib.ZVX_NO_SYNC)[0], INV),
        ("in NULL", lambda: raw_identify(ctx, None, n, Nmax, DEFAULT, CAND[:3], 64)[0], INV),
        ("a short row", lambda: raw_identify(ctx, xp, np.array([n[0], 300, n[2]], np.int32), Nmax, DEFAULT, CAND[:3], 64)[0], INV),
        ("a row longer than Nmax", lambda: raw_identify(ctx, xp, np.array([n[0], 0, Nmax + 1], np.int32), Nmax, DEFAULT, CAND[:3], 64)[0], INV),
    ]
    for kw in (dict(depth_db=6.5), dict(lo_hz=-1.0), dict(lo_hz=8000.0), dict(hi_hz=float("inf")), dict(block_frames=0), dict(band_bins=0),
               dict(period_blocks=0), dict(period_blocks=257), dict(lo_hz=1000.0, hi_hz=1100.0)):
        cases.append((str(kw), lambda kw=kw: raw_identify(ctx, xp, n, Nmax, {**DEFAULT, **kw}, CAND[:3], 64)[0], INV))
    res = _lib.WatermarkParams(0, 1.0, 250.0, 8000.0, 8, 4, 64, 1)
    cases.append(("reserved", lambda: raw_identify(ctx, xp, n, Nmax, DEFAULT, CAND[:3], 64, prm=res)[0], INV))
    # the cap: K P J signs in the tables, 2^26 at most -- refused before the K-sized arrays are looked at (one key stands for all)
    wide = {**DEFAULT, "period_blocks": 256, "band_bins": 1, "lo_hz": 0.0, "hi_hz": 11025.0}      # P J = 256 x 512 = 2^17
    for p, K in ((wide, 513), (DEFAULT, (1 << 26) // (64 * 89) + 1), ({**DEFAULT, "period_blocks": 1}, (1 << 16) + 1)):
        cases.append((f"K = {K}", lambda p=p, K=K: raw_identify(ctx, xp, n, Nmax, p, CAND[:1], 64, K=K, outs=fresh())[0], UNSUP))
    for what, call, code in cases:
        assert call() == code, (what, err(ctx))
        if code == UNSUP and what != f"K = {(1 << 16) + 1}":
            assert b"K P J" in err(ctx) and b"signs in the tables" in err(ctx), err(ctx)
        still_fine()
    # zvx_watermark_rows: zvx_watermark_ex's checks and zvx_denoise_rows' on win
    rows, windows, keys = rows_case()
    xr, nr = padded(rows)
    out = np.zeros((4, xr.shape[1]), np.float32)
    ok = lambda **kw: raw_rows(ctx, kw.get("x", xr), kw.get("n", nr), xr.shape[1], kw.get("prm", prm_of(SMALL)), keys, kw.get("out", out),  # noqa: E731
                               kw.get("stride", xr.shape[1]), kw.get("win", windows), kw.get("flags", 0))
    assert ok() == 0, err(ctx)
    want_rows = out.copy()
    bad_win = lambda b, w: [w if i == b else v for i, v in enumerate(windows)]      # noqa: E731
    rcases = [("win NULL", dict(win=None)), ("params NULL", dict(prm=None)), ("out NULL", dict(out=None)), ("flags", dict(flags=1 << 20)),
              ("depth", dict(prm=prm_of({**SMALL, "depth_db": 7.0}))), ("period", dict(prm=prm_of({**SMALL, "period_blocks": 257}))),
              ("stride", dict(stride=2999)),
              ("support in front", dict(win=bad_win(1, (2500 - R, 2499, 2600, 0)))), ("support behind", dict(win=bad_win(1, (2500 - R, 2500, 2601, 0)))),
              ("negative origin", dict(win=bad_win(0, (-1, 0, 3000, 0)))), ("count -1 without last", dict(win=bad_win(2, (1800 - R, 1800, -1, 0)))),
              ("last 2", dict(win=bad_win(2, (1800 - R, 1800, -1, 2)))),
              ("in place off origin", dict(out=xr.copy(), x=None))]
    for what, kw in rcases:
        if what == "in place off origin":
            buf = xr.copy()
            rc = raw_rows(ctx, buf, nr, xr.shape[1], prm_of(SMALL), keys, buf, xr.shape[1], windows)
            assert rc == INV and b"row 1" in err(ctx) and b"in place" in err(ctx), (what, err(ctx))
        else:
            assert ok(**kw) == INV, (what, err(ctx))
            if "support" in what:
                assert b"row 1" in err(ctx), err(ctx)
        out[:] = 0
        assert ok() == 0 and np.array_equal(out.view(np.uint32), want_rows.view(np.uint32)), (what, err(ctx))
    still_fine()
