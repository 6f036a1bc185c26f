"""Long-form synthesis on the MI355X: zvx_trim_bounds / zvx_join against tests/join_ref.py (float64 decisions, f32 ramp; never the
library), queued device input, and ZeroVoxTTS.tts_long end to end.  Bounds and the joined row are demanded EXACTLY: include/zvx.h
defines both to the bit outside an ambiguity band of 1e-9 around the trim threshold, and every test first asserts, from the
reference alone, that its rows have no frame inside that band."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import join_ref as J
from stream_util import _ragged_case, vp
from zerovox_amd import _lib, config as zcfg, pack, weights as zw

SENTINEL32 = np.uint32(0xDEADBEEF)
SENTINEL16 = np.int16(0x5A5B)
FRAMES = [(2048, 512), (1024, 256), (400, 160)]
TOP_DB = [25, 40, 60]
GAPS = [0, 1, 37, 4410, 0, 3, 22050, 5]
_ctx = {}


def ctx_for(voc, prec="bf16"):
    key = (voc, prec)
    if key not in _ctx:
        cfg = zcfg.medium_modelcfg("styletts")
        h = zcfg.hifigan_config(voc)
        man, blob = pack.pack_model(cfg, zw.tts_state_dict(cfg, 0), h, zw.hifigan_state_dict(h, 0), prec)
        _ctx[key] = _lib.Context(man, blob, 0)
    return _ctx[key]


def padded(rows, odd=False):
    n = np.array([len(r) for r in rows], np.int32)
    nmax = max(int(n.max()), 1)
    x = np.zeros((len(rows), nmax + (odd and nmax % 2 == 0)), np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def params(frame=2048, hop=512, top_db=40.0, keep=0, fade=0):
    return _lib.JoinParams(frame, hop, top_db, keep, fade)


def raw_bounds(ctx, x, n, Nmax, prm, flags=0):
    B = len(n)
    begin, end = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    rc = ctx._lib.zvx_trim_bounds(ctx._h, vp(x), vp(n), B, Nmax, C.byref(prm), vp(begin), vp(end), flags)
    return rc, begin, end


def raw_join(ctx, x, n, Nmax, gaps, prm, out, cap, flags=0, B=None):
    """the C call itself: x / out are ndarrays (host) or integer device pointers -> (rc, out_len, seg_pos, seg_begin, seg_len)"""
    B = len(n) if B is None else B
    out_len = C.c_int64(-1)
    pos, begin, ln = np.full(max(B, 1), -7, np.int64), np.full(max(B, 1), -7, np.int32), np.full(max(B, 1), -7, np.int32)
    rc = ctx._lib.zvx_join(ctx._h, vp(x), vp(n), B, Nmax, vp(gaps), C.byref(prm) if prm is not None else None, vp(out), cap,
                           C.byref(out_len), vp(pos), vp(begin), vp(ln), flags)
    return rc, int(out_len.value), pos, begin, ln


def assert_unambiguous(rows, frame, hop, top_db):
    """from the reference alone: no frame of any row within the band in which include/zvx.h allows either decision"""
    for b, x in enumerate(rows):
        worst = J.bounds_ref(x, frame, hop, top_db)[2]
        assert worst > 1e3 * J.AMBIGUOUS, (b, len(x), frame, hop, top_db, worst)


@pytest.mark.parametrize("seed", range(8))
def test_bounds_are_exact(seed):
    ctx = ctx_for("tiny")
    rows = J.make_rows(seed)
    x, n = padded(rows, odd=True)                          # odd Nmax: rows start at every alignment
    B, Nmax = x.shape
    xin = ctx.dev_alloc(x.nbytes + 16)
    try:
        ctx.dev_from_host(xin + 4, x)                     # ... and the device copy sits one float off a 16-byte boundary
        trimmed = 0
        for frame, hop in FRAMES:
            for top_db in TOP_DB:
                assert_unambiguous(rows, frame, hop, top_db)
                for keep in (0, 441):
                    want = [J.bounds_ref(r, frame, hop, top_db, keep)[:2] for r in rows]
                    prm = params(frame, hop, top_db, keep)
                    rc, begin, end = raw_bounds(ctx, x, n, Nmax, prm)
                    assert rc == 0, ctx._lib.zvx_last_error(ctx._h)
                    rc2, begin_d, end_d = raw_bounds(ctx, xin + 4, n, Nmax, prm, _lib.ZVX_DEVICE_IN)
                    assert rc2 == 0, ctx._lib.zvx_last_error(ctx._h)
                    for b in range(B):                    # every row, none skipped
                        assert (int(begin[b]), int(end[b])) == want[b], (frame, hop, top_db, keep, b, len(rows[b]), begin[b], end[b], want[b])
                        assert (int(begin_d[b]), int(end_d[b])) == want[b], ("device in", frame, hop, top_db, keep, b)
                    if (frame, hop, top_db, keep) == (2048, 512, 40, 0):
                        trimmed = sum(w != (0, len(r)) for w, r in zip(want, rows))
        assert trimmed >= 3, trimmed
        b1, e1 = ctx.trim_bounds(rows, top_db=40.0)      # the binding's list form
        assert [(int(a), int(b)) for a, b in zip(b1, e1)] == [J.bounds_ref(r)[:2] for r in rows]
        b0, e0 = ctx.trim_bounds(rows, top_db=0.0)       # trimming off: every row whole
        assert not b0.any() and np.array_equal(e0, n)
    finally:
        ctx.dev_free(xin)


def check_join(ctx, rows, x, n, xin, gaps, kw, pcm, what):
    """one parameter set through host in / device in x host out / device out; every output bit, the layout and the sentinels"""
    B, Nmax = x.shape
    ref, rpos, rbegin, rlen = J.join_ref(rows, gaps, as_pcm16=pcm, **kw)
    total = len(ref)
    cap = total + 37 + (total % 2 == 0)                   # an odd capacity
    sent, dt = (SENTINEL16, np.int16) if pcm else (SENTINEL32, np.uint32)
    prm = params(kw["frame"], kw["hop"], kw["top_db"], kw["keep"], kw["fade"])
    g = np.asarray(gaps, np.int32)
    fl = _lib.ZVX_PCM16 if pcm else 0
    dout = ctx.dev_alloc((cap + 64) * 4)
    try:
        for dev_in in (False, True):
            for dev_out in (False, True):
                tag = (what, "device in" if dev_in else "host in", "device out" if dev_out else "host out", "pcm16" if pcm else "f32")
                buf = np.full(cap + 64, sent, dt)
                if dev_out:
                    ctx.dev_from_host(dout, buf)
                rc, out_len, pos, begin, ln = raw_join(ctx, xin if dev_in else x, n, Nmax, g, prm, dout if dev_out else buf, cap,
                                                       fl | (_lib.ZVX_DEVICE_IN if dev_in else 0) | (_lib.ZVX_DEVICE_OUT if dev_out else 0))
                assert rc == 0, (tag, ctx._lib.zvx_last_error(ctx._h))
                if dev_out:
                    buf = ctx.dev_to_host(dout, (cap + 64,), dt)
                assert out_len == total, (tag, out_len, total)
                assert np.array_equal(pos, rpos) and np.array_equal(begin, rbegin) and np.array_equal(ln, rlen), tag
                got = buf[:total]
                if pcm:
                    assert np.array_equal(got, ref), (tag, int((got != ref).sum()))
                else:
                    assert np.array_equal(got, ref.view(np.uint32)), (tag, int((got != ref.view(np.uint32)).sum()))
                assert np.all(buf[total:] == sent), (tag, "written behind out_len or behind the capacity")
    finally:
        ctx.dev_free(dout)
    return total


@pytest.mark.parametrize("seed", range(8))
def test_joined_row_is_bit_exact(seed):
    ctx = ctx_for("tiny")
    rows = J.make_rows(seed)
    x, n = padded(rows, odd=True)                          # odd Nmax
    frame, hop = FRAMES[seed % 3]
    top_db = TOP_DB[(seed // 3) % 3]
    assert_unambiguous(rows, frame, hop, top_db)
    gaps = GAPS[seed % 4:] + GAPS[:seed % 4]
    xin = ctx.dev_alloc(x.nbytes + 16)
    try:
        ctx.dev_from_host(xin + 4, x)                     # input pointer offset by one float
        for fade in (0, 1, 110, 5000):                    # 5000: longer than half of the short rows
            for keep in (0, 441):
                kw = dict(frame=frame, hop=hop, top_db=top_db, keep=keep, fade=fade)
                pcm = (fade in (1, 5000)) == (keep == 0)  # both sample formats see every fade and every keep over the seeds' parameter sets
                check_join(ctx, rows, x, n, xin + 4, gaps, kw, pcm, f"seed {seed} fade {fade} keep {keep}")
                if seed == 0:
                    check_join(ctx, rows, x, n, xin + 4, gaps, kw, not pcm, f"seed {seed} fade {fade} keep {keep}")
        kw = dict(frame=frame, hop=hop, top_db=0.0, keep=0, fade=110)
        check_join(ctx, rows, x, n, xin + 4, gaps, kw, False, "trimming off")
        # the binding: host rows as a list, no gaps
        wav, pos, begin, ln = ctx.join(rows, frame=frame, hop=hop, top_db=top_db, keep=441, fade=110)
        ref, rpos, rbegin, rlen = J.join_ref(rows, None, frame, hop, top_db, 441, 110)
        assert np.array_equal(wav.view(np.uint32), ref.view(np.uint32)) and np.array_equal(pos, rpos) and np.array_equal(ln, rlen)
    finally:
        ctx.dev_free(xin)


def test_many_segments_and_empty_ones():
    """more segments than one scan chunk (256) and than the LDS position table (2047), empty segments and zero gaps among them"""
    ctx = ctx_for("tiny")
    rng = np.random.default_rng(5)
    for B in (300, 2500):
        lens = rng.integers(0, 90, B)
        lens[rng.integers(0, B, B // 5)] = 0
        rows = [rng.uniform(-1, 1, int(v)).astype(np.float32) for v in lens]
        gaps = rng.integers(0, 3, B).astype(np.int32)
        x, n = padded(rows, odd=True)
        for pcm in (False, True):
            kw = dict(frame=64, hop=16, top_db=0.0, keep=0, fade=7)
            wav, pos, begin, ln = ctx.join(rows, gaps, pcm16=pcm, **kw)
            ref, rpos, rbegin, rlen = J.join_ref(rows, gaps, as_pcm16=pcm, **kw)
            assert np.array_equal(pos, rpos) and np.array_equal(ln, rlen) and not begin.any()
            assert wav.dtype == ref.dtype and np.array_equal(wav.view(np.uint16 if pcm else np.uint32), ref.view(np.uint16 if pcm else np.uint32)), (B, pcm)


def test_join_errors_leave_the_context_usable():
    ctx = ctx_for("tiny")
    rows = J.make_rows(2)[2:5]
    x, n = padded(rows)
    B, Nmax = x.shape
    gaps = np.array([5, 0, 9], np.int32)
    ref = J.join_ref(rows, gaps, fade=50)[0]
    total = len(ref)
    prm = params(fade=50)
    # capacity one short: ZVX_E_BUFFER, nothing written, both numbers in the message, the layout still reported
    buf = np.full(total + 8, SENTINEL32, np.uint32)
    rc, out_len, pos, _, ln = raw_join(ctx, x, n, Nmax, gaps, prm, buf, total - 1)
    assert rc == _lib.ZVX_E_BUFFER and out_len == total
    msg = ctx._lib.zvx_last_error(ctx._h).decode()
    assert str(total) in msg and str(total - 1) in msg, msg
    assert np.all(buf == SENTINEL32)
    dout = ctx.dev_alloc((total + 8) * 4)
    try:
        ctx.dev_from_host(dout, buf)
        rc = raw_join(ctx, x, n, Nmax, gaps, prm, dout, total - 1, _lib.ZVX_DEVICE_OUT)[0]
        assert rc == _lib.ZVX_E_BUFFER
        assert np.all(ctx.dev_to_host(dout, (total + 8,), np.uint32) == SENTINEL32)
    finally:
        ctx.dev_free(dout)
    rc, out_len = raw_join(ctx, x, n, Nmax, gaps, prm, buf, total)[:2]      # the exact capacity is enough, and the context still works
    assert rc == 0 and out_len == total and np.array_equal(buf[:total], ref.view(np.uint32)) and np.all(buf[total:] == SENTINEL32)
    # validation: nothing is queued, ZVX_E_INVALID each
    out = np.zeros(total, np.float32)
    inv = _lib.ZVX_E_INVALID
    bad_params = [params(frame=1, hop=1), params(hop=0), params(frame=512, hop=513), params(keep=-1), params(fade=-1),
                  params(top_db=float("nan")), params(top_db=float("inf"))]
    for p in bad_params:
        assert raw_join(ctx, x, n, Nmax, gaps, p, out, total)[0] == inv, (p.frame, p.hop, p.top_db, p.keep, p.fade)
        assert raw_bounds(ctx, x, n, Nmax, p)[0] == inv
    assert raw_join(ctx, x, n, Nmax, gaps, prm, out, total, B=0)[0] == inv
    assert raw_join(ctx, None, n, Nmax, gaps, prm, out, total)[0] == inv
    assert raw_join(ctx, x, None, Nmax, gaps, prm, out, total, B=B)[0] == inv
    assert raw_join(ctx, x, n, Nmax, gaps, None, out, total)[0] == inv
    assert raw_join(ctx, x, n, Nmax, gaps, prm, None, total)[0] == inv
    assert raw_join(ctx, x, n, Nmax, np.array([5, -1, 9], np.int32), prm, out, total)[0] == inv
    assert raw_join(ctx, x, np.array([n[0], -1, n[2]], np.int32), Nmax, gaps, prm, out, total)[0] == inv
    assert raw_join(ctx, x, np.array([n[0], Nmax + 1, n[2]], np.int32), Nmax, gaps, prm, out, total)[0] == inv
    assert raw_join(ctx, x, n, Nmax, gaps, prm, out, total, flags=_lib.ZVX_NO_SYNC)[0] == inv
    assert raw_join(ctx, x, n, Nmax, gaps, prm, out, total, flags=64)[0] == inv
    assert ctx._lib.zvx_join(ctx._h, vp(x), vp(n), B, Nmax, vp(gaps), C.byref(prm), vp(out), total, None, None, None, None, 0) == inv
    assert ctx._lib.zvx_trim_bounds(ctx._h, vp(x), vp(n), B, Nmax, C.byref(prm), None, None, 0) == inv
    assert raw_bounds(ctx, x, n, Nmax, prm, _lib.ZVX_DEVICE_OUT)[0] == inv
    assert raw_bounds(ctx, x, n, Nmax, prm, 64)[0] == inv and b"zvx_trim_bounds" in ctx._lib.zvx_last_error(ctx._h)
    rc, out_len = raw_join(ctx, x, n, Nmax, gaps, prm, buf, total)[:2]
    assert rc == 0 and np.array_equal(buf[:total], ref.view(np.uint32))


TIGHT_DB = (6.0, 1.0)      # synthetic weights make noise-like audio: a tight threshold is what makes the trimmer cut something


@pytest.mark.parametrize("voc", ["tiny", "v1"])
def test_queued_synthesis_feeds_the_join_in_stream_order(voc):
    ctx = ctx_for(voc)
    hop = ctx.hop
    case = _ragged_case(4, 24, 43)
    host = ctx.synthesize(*case, None, want_mel=False)
    ml = host["mel_len"]
    rows = [host["wav"][b, :int(ml[b]) * hop] for b in range(4)]
    gaps = [100, 0, 2205, 7]
    stride = int(ml.max()) * hop + 13
    dptr = ctx.dev_alloc(4 * stride * 4)
    try:
        for out_rate in (0, 16000):                       # native_rate takes the queued call out of the context's output rate
            ctx.set_int("out_rate", out_rate)
            for top_db in TIGHT_DB:
                ctx.dev_from_host(dptr, np.full((4, stride), SENTINEL32, np.uint32))       # nothing of an earlier round is left to be read
                kw = dict(frame=2048, hop=512, top_db=top_db, keep=100, fade=64)
                assert_unambiguous(rows, 2048, 512, top_db)
                ref, rpos, rbegin, rlen = J.join_ref(rows, gaps, **kw)
                ctx.synthesize(*case, None, want_mel=False, wav_device_ptr=dptr, wav_stride=stride, no_sync=True, native_rate=True)
                wav, pos, begin, ln = ctx.join_device(dptr, ml * hop, stride, gaps, **kw)      # at once: no sync in between
                print(f"{voc} out_rate {out_rate} top_db {top_db}: kept {[int(v) for v in ln]} of {[len(r) for r in rows]}")
                assert np.array_equal(wav.view(np.uint32), ref.view(np.uint32)), (voc, out_rate, top_db)
                assert np.array_equal(pos, rpos) and np.array_equal(begin, rbegin) and np.array_equal(ln, rlen)
    finally:
        ctx.set_int("out_rate", 0)
        ctx.dev_free(dptr)


def test_join_accounting_and_nothing_else_moved():
    ctx = ctx_for("tiny")
    case = _ragged_case(3, 20, 41)
    before = ctx.synthesize(*case, None, want_mel=False)
    rows = J.make_rows(1)
    gaps = GAPS
    ctx.set_int("profile", 2); ctx.reset_stats()
    try:
        wav, pos, begin, ln = ctx.join(rows, gaps, top_db=40.0, fade=110)
        tags = {t["name"]: t for t in ctx.tag_stats()}
        n_in = sum(len(r) for r in rows if len(r) >= 2048)
        assert tags["post.join"]["launches"] == 1        # the call's launches are timed as one group
        assert tags["post.join"]["bytes"] == 4.0 * n_in + 4.0 * int(ln.sum()) + 4.0 * len(wav)
        assert ctx.join_ms() > 0 and set(ctx.stage_times()) == set(_lib.STAGES)
    finally:
        ctx.set_int("profile", 0)
    after = ctx.synthesize(*case, None, want_mel=False)
    assert np.array_equal(after["wav"].view(np.uint32), before["wav"].view(np.uint32)) and np.array_equal(after["mel_len"], before["mel_len"])


THREE = "The quick brown fox jumps over the lazy dog; does it, really? Pack my box with five dozen liquor jugs"
FORTY = " ".join(f"Sentence number {i} of the long paragraph says hello{'!' if i % 3 == 0 else ('; and more' if i % 3 == 1 else '.')}" for i in range(40))


@pytest.mark.parametrize("voc", ["tiny", "v2"])
def test_tts_long_end_to_end(voc):
    from zerovox_amd.longform import PAUSES_MS, split_sentences
    from zerovox_amd.synthesize import ZeroVoxTTS
    _, synth = ZeroVoxTTS.load_model("synthetic:styletts", f"synthetic:{voc}", infer_device="cuda:0", precision="bf16")
    ctx, hop, native = synth.model.ctx, 256, 22050
    spk = synth.speaker_embed_from_mel(np.random.default_rng(0).standard_normal((96, 80)).astype(np.float32))
    for text, nsent in ((THREE, 3), (FORTY, None)):
        pieces = split_sentences(text)
        ids = [synth.text2phonemeids(s) for s, _ in pieces]
        N = len(pieces)
        assert N == nsent or (nsent is None and N > 32)   # the long text needs two batches
        rows, mls = [], []
        for b0 in range(0, N, 32):                        # the rows synthesize_batch returns for the same sentences
            grp = ids[b0:b0 + 32]
            T = np.array([len(p) for p, _ in grp], np.int32)
            ph, pu = np.zeros((len(grp), int(T.max())), np.int32), np.zeros((len(grp), int(T.max())), np.int32)
            for i, (p, u) in enumerate(grp):
                ph[i, :T[i]], pu[i, :T[i]] = p, u
            r = synth.model.synthesize_batch(ph, pu, T, np.repeat(np.asarray(spk, np.float32).reshape(1, -1), len(grp), axis=0), want_mel=False, Lmax_cap=2048)
            rows += [r["wav"][i, :int(r["mel_len"][i]) * hop].copy() for i in range(len(grp))]
            mls += [int(v) for v in r["mel_len"]]
        gaps = [int(round(PAUSES_MS[c] * native / 1000.0)) for _, c in pieces]
        gaps[-1] = 0
        keep, fade = int(round(20 * native / 1000.0)), int(round(5 * native / 1000.0))
        for trim_db in (0.0,) + TIGHT_DB:                 # trimming off, then thresholds that cut
            assert_unambiguous(rows, 2048, 512, trim_db)
            ref, rpos, rbegin, rlen = J.join_ref(rows, gaps, 2048, 512, trim_db, keep, fade)
            wav, seg = synth.tts_long(text, spk, trim_db=trim_db)
            assert wav.dtype == np.float32 and np.array_equal(wav.view(np.uint32), ref.view(np.uint32)), (voc, N, trim_db)
            assert [s["text"] for s in seg] == [p for p, _ in pieces]
            assert [s["start"] for s in seg] == list(rpos) and [s["samples"] for s in seg] == list(rlen) and [s["trim"] for s in seg] == list(rbegin)
            assert [s["mel_len"] for s in seg] == mls
            for s, (p, _) in zip(seg, ids):
                assert len(s["durations"]) == len(p) and int(np.sum(s["durations"])) == s["mel_len"]
            print(f"{voc}, {N} sentences, trim_db {trim_db}: mel_len {min(mls)} .. {max(mls)}, {sum(int(v) < m * hop for v, m in zip(rlen, mls))} rows cut")
        pcm, _ = synth.tts_long(text, spk, trim_db=trim_db, pcm16=True)
        assert pcm.dtype == np.int16 and np.array_equal(pcm, J.pcm16(ref))
        if N > 32:
            continue
        for rate in (48000, 16000):                       # one resample of the joined row
            synth.output_rate = rate
            try:
                got, seg_r = synth.tts_long(text, spk, trim_db=trim_db)
            finally:
                synth.output_rate = native
            want, wl = ctx.resample([ref], native, rate)
            assert np.array_equal(got.view(np.uint32), want[0, :wl[0]].view(np.uint32)), (voc, rate)
            assert [s["start"] for s in seg_r] == [_lib.resampled_len(int(p), native, rate) for p in rpos]
            assert sum(1 for s in seg_r if s["samples"] > 0) == sum(1 for v in rlen if v > 0)
        # forced durations, as tts_ex(duration=...) forces them; a prosody keyword reaches every sentence
        forced = [np.asarray(s["durations"]) + 1 for s in seg]
        wav_f, seg_f = synth.tts_long(text, spk, trim_db=0.0, durations=forced)
        assert [s["mel_len"] for s in seg_f] == [int(f.sum()) for f in forced] and all(np.array_equal(s["durations"], f) for s, f in zip(seg_f, forced))
        assert len(wav_f) == sum(int(f.sum()) * hop for f in forced) + sum(gaps)
        one, _, length = synth.tts(pieces[0][0], spk, speed=1.25)
        wav_s, seg_s = synth.tts_long(text, spk, trim_db=0.0, fade_ms=0, speed=1.25)
        assert seg_s[0]["mel_len"] == length and np.array_equal(wav_s[:length * hop].view(np.uint32), one.view(np.uint32))
    for empty in ("", "   ", "... !?"):
        wav, seg = synth.tts_long(empty, spk)
        assert seg == [] and wav.shape == (1, 1) and wav.dtype == np.float32 and wav[0, 0] == 0.0
    with pytest.raises(ValueError):
        synth.tts_long(THREE, spk, durations=[[1, 2]])
    again = synth.tts(pieces[0][0], spk)[0]               # the context is usable after the error
    assert len(again) > 0
    synth.model.close()
