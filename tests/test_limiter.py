"""True-peak metering and the look-ahead limiter, the parts that need no GPU: the float64 reference of tests/limit_ref.py against the
properties include/zvx.h states, the overshoot figure the header quotes, and the surface of the feature (header, exports, bindings,
keywords)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import join_ref as J
import limit_ref as L
import resample_ref as RS
from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEILING = 0.891


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("os_", [2, 4, 8])
def test_phase_by_phase_oversampling_is_the_resamplers_sum(os_):
    x = np.random.default_rng(os_).standard_normal(333).astype(np.float32)
    y, A = L.oversample(x, os_)
    want, wantA = RS.resample_ref(x, 1, os_, want_mag=True)          # (L, M) = (os, 1) whatever the rate
    assert len(y) == os_ * len(x) == len(want)
    assert np.max(np.abs(y - want)) <= 1e-14 and np.max(np.abs(A - wantA)) <= 1e-14
    assert RS.taps_per_output(1, os_) == L.TAPS == 21
    assert np.all(np.abs(y[::os_] - x) <= 1e-3 * np.max(np.abs(x)))  # phase 0 all but reproduces the samples


def test_window_rule_and_weights():
    assert L.window(22050, 5.0) == 110 and L.window(22050, 1.0) == 22 and L.window(8000, 0.01) == 1 and L.window(48000, 4096 / 48.0) == 4096
    for W in (1, 22, 110, 4096):
        w = L.weights(W)
        assert len(w) == 2 * W + 1 and abs(w.sum() - 1.0) <= 1e-15 and np.all(w > 0) and np.array_equal(w, w[::-1])
    v = np.abs(np.random.default_rng(0).standard_normal(97))
    for W in (1, 2, 3, 7, 40, 200):
        want = np.array([v[max(0, i - W):i + W + 1].max() for i in range(len(v))])
        assert np.array_equal(L.running_max(v, W), want), W


def in_reach(e, c, W):
    """True where some e[j] > c has |j - i| <= 2 W"""
    return L.running_max((np.asarray(e) > c).astype(np.float64), 2 * W) > 0


def test_reference_holds_the_ceiling_exactly_and_keeps_untouched_bits():
    c32 = np.float32(CEILING)
    rows = L.scaled_rows(J.make_rows(0))[:5] + [np.full(700, 1.0, np.float32), (J.make_rows(1)[2] * np.float32(0.5))]
    touched = kept = 0
    for os_ in (1, 4):
        for W in (1, 22, 110):
            for b, x in enumerate(rows):
                r = L.limit(x, CEILING, W, os_)
                assert np.all(np.abs(r["out"]) <= c32), (os_, W, b)                      # (a): no tolerance
                assert np.all(r["g32"].astype(np.float64) <= r["g"]) and np.all(r["g"] <= 1.0)
                far = ~in_reach(r["e"], float(c32), W)
                assert np.array_equal(bits(r["out"])[far], bits(x)[far]), (os_, W, b)    # (b)
                assert np.all(r["g32"][far] == 1.0)
                touched += int((~far).sum()); kept += int(far.sum())
    assert touched > 0 and kept > 0
    under = rows[-1]
    assert L.true_peak(under, 4)[0] < CEILING
    assert np.array_equal(bits(L.limit(under, CEILING, 110, 4)["out"]), bits(under))     # a row under the ceiling: bit for bit
    dc = L.limit(rows[-2], CEILING, 22, 1)                                               # DC at 1.0: one gain throughout
    assert np.all(dc["out"] <= c32) and np.all(dc["out"] >= c32 * np.float32(1 - 2e-7))
    empty = L.limit(np.zeros(0, np.float32), CEILING, 22, 4)
    assert len(empty["out"]) == 0 and L.true_peak(np.zeros(0, np.float32), 4) == (0.0, 0.0)


@pytest.mark.parametrize("W", [1, 5, 22])
def test_a_single_spike_gives_the_hann_plateau(W):
    n, at, h = 40 * W + 50, 17 * W + 3, 2.5
    x = np.zeros(n, np.float32)
    x[at] = h
    r = L.limit(x, CEILING, W, 1)
    c = float(np.float32(CEILING))
    depth = 1.0 - c / h
    w = L.weights(W)
    # the held depth is a box of 2 W + 1 samples around the spike; smoothed by w it is the box's overlap with the window
    j = np.arange(n) - at
    shape = np.array([w[max(-W, -W - jj) + W:min(W, W - jj) + W + 1].sum() if abs(jj) <= 2 * W else 0.0 for jj in j])
    assert np.max(np.abs(r["g"] - (1.0 - depth * shape))) <= 1e-15
    assert abs(r["g"][at] - c / h) <= 1e-15 and r["g"].argmin() == at                   # the minimum, c / h, is reached at the spike
    assert np.all(r["g"][np.abs(j) > 2 * W] == 1.0) and np.all(r["g"][np.abs(j) <= 2 * W] < 1.0)
    assert np.all(np.diff(r["g"][:at + 1]) <= 0) and np.all(np.diff(r["g"][at:]) >= 0)
    assert np.all(r["d"][j != 0] == 0) and r["out"][at] <= np.float32(CEILING) and r["out"][at] >= np.float32(CEILING) * np.float32(1 - 2e-7)


def test_header_declares_the_limiter_interface():
    h = header()
    assert re.search(r"zvx_status\s+zvx_true_peak\s*\(", h) and re.search(r"zvx_status\s+zvx_limit\s*\(", h)
    assert re.search(r"typedef\s+struct\s+zvx_limit_params\s*\{[^}]*ceiling[^}]*window_ms[^}]*oversample[^}]*\}\s*zvx_limit_params\s*;", h)
    assert '"post.limit"' in h and re.search(r"ZVX_T_COUNT\s*=\s*8\b", h) and _lib.ZVX_T_COUNT == 8
    assert "Not here: true-peak" not in h and "limiting, momentary" not in h
    assert [f[0] for f in _lib.LimitParams._fields_] == ["ceiling", "window_ms", "oversample"] and C.sizeof(_lib.LimitParams) == 12
    with open(os.path.join(ROOT, "zerovox_amd", "csrc", "zvx_kernels.h")) as f:
        k = f.read()
    assert int(re.search(r"constexpr int LIMIT_TILE = (\d+);", k).group(1)) == _lib.LIMIT_TILE
    assert int(re.search(r"constexpr int LIMIT_MAX_W = (\d+);", k).group(1)) == _lib.LIMIT_MAX_W == 4096


def test_library_exports_both_entry_points():
    assert "zvx_true_peak" in _lib.EXPORTS and "zvx_limit" in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("zvx_true_peak", "zvx_limit"):
        assert hasattr(lib, name), name
    # NULL context: refused before anything else is looked at
    assert lib.zvx_true_peak(None, None, None, 0, 0, 0, 0, None, 0) == _lib.ZVX_E_INVALID
    lib.zvx_limit.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    assert lib.zvx_limit(None, None, None, 0, 0, 0, None, None, 0, None, None, 0) == _lib.ZVX_E_INVALID


def test_bindings_and_keywords_are_there():
    from zerovox_amd.synthesize import ZeroVoxTTS
    for name in ("true_peak", "limit", "limit_device"):
        assert callable(getattr(_lib.Context, name))
    p = inspect.signature(_lib.Context.true_peak).parameters
    assert p["oversample"].default == 4 and p["rate"].default is None and p["lengths"].default is None
    p = inspect.signature(_lib.Context.limit).parameters
    assert p["window_ms"].default == 5.0 and p["oversample"].default == 4 and p["pcm16"].default is False and p["ceiling"].default is inspect.Parameter.empty
    p = inspect.signature(_lib.Context.limit_device).parameters
    assert p["no_sync"].default is False and p["window_ms"].default == 5.0 and p["oversample"].default == 4
    for fn in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long):
        p = inspect.signature(fn).parameters
        assert p["limiter"].default is False and p["limiter_ms"].default == 5.0, fn
    assert inspect.signature(ZeroVoxTTS.tts_stream).parameters["limiter"].default is False
    assert isinstance(ZeroVoxTTS.last_limit, property)


def test_a_stream_cannot_be_limited_and_the_limiter_needs_a_ceiling():
    from zerovox_amd.longform import limit_keywords, synthesize_long
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                  # the refusal comes before anything of the model is touched
    with pytest.raises(ValueError):
        synth.tts_stream("hello there", None, limiter=True)
    with pytest.raises(ValueError):
        synthesize_long(None, "hello there", None, limiter=True, peak_db=None)
    assert limit_keywords(False, 5.0, -1.0) is None
    kw = limit_keywords(True, 3.0, -1.0)
    assert kw == dict(ceiling=float(10.0 ** (-1.0 / 20.0)), window_ms=3.0, oversample=4)
    # under a limiter the loudness gain carries no peak ceiling; without one it keeps today's
    assert synth._post(-16.0, -1.0, True, 5.0) == dict(loudness=dict(target=-16.0, peak_ceiling=0.0), limiter=limit_keywords(True, 5.0, -1.0))
    assert synth._post(-16.0, -1.0, False, 5.0) == dict(loudness=dict(target=-16.0, peak_ceiling=float(10.0 ** (-1.0 / 20.0))))
    assert synth._post(None, -1.0, False, 5.0) == {} and set(synth._post(None, -1.0, True, 5.0)) == {"limiter"}


def test_true_peak_after_limiting_stays_near_the_ceiling():
    """Property (c) of the header: the reference's own limited rows, measured by the reference's 4x true peak.  Over make_rows(seed), seeds
    0-7, every row scaled to a sample peak of 1.6, c = 0.891: detection on the 4x envelope keeps the true peak within 0.01 dB of c at
    W = 22 and within 0.001 dB at W = 110; detection on sample peaks (os = 1) does not.  The worst figures are printed: the header quotes
    them."""
    worst = {22: -np.inf, 110: -np.inf, "os1": -np.inf}
    for seed in range(8):
        for x in L.scaled_rows(J.make_rows(seed)):
            for W in (22, 110):
                tp = L.true_peak(L.limit(x, CEILING, W, 4)["out"], 4)[0]
                worst[W] = max(worst[W], L.over_db(tp, CEILING))
            tp = L.true_peak(L.limit(x, CEILING, 110, 1)["out"], 4)[0]
            worst["os1"] = max(worst["os1"], L.over_db(tp, CEILING))
    print(f"true peak over the ceiling after limiting: {worst[22]:.5f} dB at W = 22, {worst[110]:.6f} dB at W = 110 (os = 4); {worst['os1']:.3f} dB with os = 1")
    assert worst[22] <= 0.01 and worst[110] <= 0.001
    assert worst["os1"] > 0.01                              # sample-peak detection leaves inter-sample peaks: why true-peak detection exists
