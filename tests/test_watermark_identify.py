"""Per-request watermark keys without a device: derive_key against values worked out by hand from its documented rule, the device's
sign rule (k_wm_signs of watermark.hip: 64-bit integer arithmetic, one byte per (key, c, j)) restated here against the two Python tables,
the refusals of ZeroVoxTTS.identify_watermark, the bindings of the two new calls, and identification among 64 candidate keys with the
float64 restatement alone (tests/watermark_ref.py: one analysis, a stack of tables)."""
import ctypes as C
import re

import numpy as np
import pytest

import watermark_ref as W
from stream_util import header
from zerovox_amd import _lib, watermark as WM

KEY = 0xC0FFEE1234567
M64 = (1 << 64) - 1
# the candidates and the marked rows of the identification tests (tests/test_watermark_identify_gpu.py runs the same on the device)
KEYS = [W.mix64(0xC0FFEE1234567 + k) for k in range(64)]
ROWS = [(1.5, 21), (3.0, 22), (3.0, 23), (1.5, 24)]
CUT = 5000
_sig = {}


def key_of_row(b):
    return 5 + 13 * b


def clean_rows():
    if "clean" not in _sig:
        _sig["clean"] = [W.voiced_signal(sec, seed) for sec, seed in ROWS]
        for r in _sig["clean"]:
            r.setflags(write=False)
    return _sig["clean"]


def check_identification(scores_marked, scores_clean, scores_cut_right):
    """the conditions both the float64 reference and the device must meet: scores_marked / scores_clean [4][64], scores_cut_right [4]"""
    for b in range(len(ROWS)):
        res = WM.identify_result(KEYS, scores_marked[b], [0] * 64, [0] * 64)
        wrong = np.delete(np.asarray(scores_marked[b], np.float64), key_of_row(b))
        print(f"row {b}: best {res.best} score {res.score:.2f} margin {res.margin:.2f}; largest wrong {wrong.max():.2f}, "
              f"unmarked {float(np.max(scores_clean[b])):.2f}, cut by {CUT}: {float(scores_cut_right[b]):.2f}")
        assert res.best == key_of_row(b) and res.key == KEYS[key_of_row(b)] and int(np.argmax(scores_marked[b])) == key_of_row(b)
        assert res.score >= WM.THRESHOLD and res.detected
        assert wrong.max() < WM.THRESHOLD and float(np.max(scores_clean[b])) < WM.THRESHOLD
        assert res.margin > 2.0 and res.margin == res.score - wrong.max()
        assert float(scores_cut_right[b]) >= WM.THRESHOLD


def test_derive_key_against_values_computed_by_hand():
    # mix64 itself, step by step, on one value
    z = (5 + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    assert WM.mix64(5) == z == W.mix64(5)
    m = WM.mix64
    master = 0x0123456789ABCDEF
    # an int: mix64(master ^ mix64(ident))
    assert WM.derive_key(master, 5) == m(master ^ z)
    assert WM.derive_key(0, 0) == m(m(0)) and WM.derive_key(M64, M64) == m(M64 ^ m(M64))
    # bytes: h = len; h = mix64(h ^ chunk) over little-endian chunks of 8, the last one short
    assert WM.derive_key(master, b"") == m(master ^ m(0))
    assert WM.derive_key(master, b"\x01") == m(master ^ m(m(1 ^ 1)))
    ident = b"request-0001"                                     # 12 bytes: "request-" and "0001"
    w0, w1 = int.from_bytes(b"request-", "little"), int.from_bytes(b"0001", "little")
    assert w0 == 0x2D74736575716572 and w1 == 0x31303030
    assert WM.derive_key(master, ident) == m(master ^ m(m(m(12 ^ w0) ^ w1)))
    assert WM.derive_key(master, bytearray(ident)) == WM.derive_key(master, ident) == WM.derive_key(master, memoryview(ident))
    # the length is part of it: trailing zero bytes make another key; so do another master and another ident
    assert len({WM.derive_key(master, b"ab"), WM.derive_key(master, b"ab\x00"), WM.derive_key(master + 1, b"ab"), WM.derive_key(master, b"ac")}) == 4
    assert all(0 <= WM.derive_key(master, i) <= M64 for i in (0, 1, M64))
    for bad in [(-1, 1), (1 << 64, 1), (True, 1), (1.0, 1), ("1", 1), (1, -1), (1, 1 << 64), (1, True), (1, "id"), (1, 1.5), (1, None)]:
        with pytest.raises(ValueError, match="derive_key"):
            WM.derive_key(*bad)


def device_sign_rule(keys, P, J):
    """k_wm_signs restated (its byte form; the packed form holds the same signs, bit j % 32 of word j / 32 of a row): byte i of
    out[n][P][J] belongs to t = i / (P J), c = (i mod P J) / J, j = (i mod P J) mod J, and is +1 where
    bit 63 of the splitmix64 finaliser of keys[t] ^ (c << 32 | j) is set -- in wrapping uint64 arithmetic, as the kernel's"""
    keys = np.asarray(keys, np.uint64)
    i = np.arange(len(keys) * P * J, dtype=np.int64)
    t, rest = i // (P * J), i % (P * J)
    c, j = (rest // J).astype(np.uint64), (rest % J).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = keys[t] ^ ((c << np.uint64(32)) | j)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return np.where(z >> np.uint64(63), 1, -1).astype(np.int8).reshape(len(keys), P, J)


@pytest.mark.parametrize("P,J", [(1, 3), (3, 5), (64, 89), (256, 512)])
def test_the_device_sign_rule_is_the_tables_of_the_python_side(P, J):
    keys = [0, M64, KEY]
    got = device_sign_rule(keys, P, J)
    for t, key in enumerate(keys):
        assert np.array_equal(got[t], np.array(WM.sign_table(key, P, J))), (key, P, J)
        assert np.array_equal(got[t], W.sign_table(key, P, J)), (key, P, J)
    assert 0.3 < float(np.mean(got == 1)) < 0.7 or P * J < 64


def test_identify_refusals_come_before_the_model_is_touched():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                    # no model, no device: a refusal must not need either
    wav = np.zeros(22050, np.float32)
    bad = [dict(depth_db=-0.5), dict(depth_db=6.5), dict(depth_db=float("nan")), dict(lo_hz=-1.0), dict(lo_hz=9000.0), dict(hi_hz=float("inf")),
           dict(block_frames=0), dict(band_bins=0), dict(period_blocks=0), dict(period_blocks=257), dict(reserved=1)]
    for kw in bad:
        with pytest.raises(ValueError, match="watermark"):
            synth.identify_watermark(wav, [1, 2], **kw)
        with pytest.raises(ValueError, match="watermark"):     # ... as detect_watermark does
            synth.detect_watermark(wav, 1, **kw)
    for keys in ([-1], [1, 1 << 64], [True], ["key"], [1.5], [1, None]):
        with pytest.raises(ValueError, match="watermark"):
            synth.identify_watermark(wav, keys)
    with pytest.raises(ValueError, match="keys is empty"):
        synth.identify_watermark(wav, [])


def test_the_two_new_calls_are_declared_bound_and_exported():
    assert {"zvx_watermark_rows", "zvx_watermark_identify"} <= set(_lib.EXPORTS)
    h = header()
    for name in ("zvx_watermark_rows", "zvx_watermark_identify"):
        assert re.search(r"zvx_status\s+" + name + r"\s*\(", h), name
    assert '"post.wmidentify"' in h
    lib = _lib.load()
    assert len(lib.zvx_watermark_rows.argtypes) == 11 and lib.zvx_watermark_rows.argtypes[-1] == C.POINTER(_lib.RowWindow)
    assert len(lib.zvx_watermark_identify.argtypes) == 14
    # a NULL context is refused before anything else is looked at
    assert lib.zvx_watermark_rows(None, None, None, 0, 0, None, None, None, 0, 0, None) == _lib.ZVX_E_INVALID
    assert lib.zvx_watermark_identify(None, None, None, 0, 0, None, None, 0, 0, None, None, None, None, 0) == _lib.ZVX_E_INVALID


def test_identify_result_ties_and_margin():
    r = WM.identify_result([10, 11, 12], [3.0, 7.0, 7.0], [1, 2, 3], [0, 1, 0])
    assert (r.best, r.key, r.score, r.offset, r.window, r.margin, r.detected, r.threshold) == (1, 11, 7.0, 2, 1, 0.0, True, WM.THRESHOLD)
    assert r.scores == [3.0, 7.0, 7.0]
    one = WM.identify_result([10], [6.0], [4], [2], best=0, threshold=6.5)
    assert (one.best, one.margin, one.detected, one.threshold) == (0, 6.0, False, 6.5)
    none = WM.identify_result([10, 11], [0.0, 0.0], [0, 0], [0, 0])
    assert (none.best, none.score, none.margin, none.detected) == (0, 0.0, 0.0, False)


def test_identification_among_64_keys_with_the_reference():
    """four rows, each marked with its own key of the 64 candidates at the defaults: the right key wins with a margin, every wrong key and
    every unmarked row stays under the threshold, and the right key still passes on the row cut by 5000 samples"""
    clean = clean_rows()
    marked = [W.embed(r, KEYS[key_of_row(b)]) for b, r in enumerate(clean)]
    sm = [W.null_scores(m, KEYS) for m in marked]
    sc = [W.null_scores(r, KEYS) for r in clean]
    cut = [W.null_scores(m[CUT:], [KEYS[key_of_row(b)]])[0] for b, m in enumerate(marked)]
    check_identification(sm, sc, cut)
