"""The equaliser without a device: the float64 reference of zvx_fir (tests/fir_ref.py) against itself and against numpy.convolve, the
design of zerovox_amd/equaliser.py, its eq keyword, the stream planner, and what the four Context.fir* bindings hand to the library.

deviation_db of every preset at 22.05 kHz (the largest |realised - target| in dB where the target is >= -20 dB, lo_hz = 0), measured here
with NumPy on a CPU and asserted at 1.5 x the measured value -- the margin covers other NumPy FFT builds, nothing else:

    K = 511:   flat 0   presence 3.054e-3   warm 6.358e-2   rumble 7.344   telephone 1.968
    K = 1023:  flat 0   presence 7.651e-4   warm 1.663e-2   rumble 4.161   telephone 0.5567

Bells and shelves are realised closely; the high-pass presets are not: a K-tap filter resolves nothing much below 2 * rate / K (86 Hz at
K = 511), and the -20 dB point of an 80 Hz or 300 Hz fourth-order slope lies inside that.  Above 200 Hz the rumble preset is within 0.012 dB."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fir_ref as F
from stream_util import same_bits
from test_post_bindings import FakeLib, norm_result
from zerovox_amd import _lib, equaliser as E
from zerovox_amd._lib import Context
from zerovox_amd.stream import stream_windows

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fir_bindings_expected.json")
RATE = 22050
KD = [(1, 0), (63, 31), (63, 0), (64, 63)]


def signal(n, seed=0):
    rng = np.random.default_rng(77 + seed)
    i = np.arange(n)
    x = 0.3 * rng.standard_normal(n) + 0.3 * np.sin(0.21 * i + 0.4) + 0.2 * np.sin(0.73 * i + 1.1)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def taps(K, seed=0):
    rng = np.random.default_rng(1000 + K + seed)
    return (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)


@pytest.mark.parametrize("K,D", KD + [(255, 127)])
def test_the_references_windows_tile_to_its_whole_signal_result(K, D):
    x, h = signal(1500), taps(K)
    whole = F.fir(x, h, D)
    assert whole.dtype == np.float32 and whole.shape == x.shape and F.no_subnormal(whole)
    RL, RR = K - 1 - D, D
    for piece in (1, 7, 256, 700):
        got = []
        for b in range(0, len(x), piece):
            e = min(b + piece, len(x))
            o, end = max(0, b - RL), min(len(x), e + RR)           # exactly the reach on either side, or the signal's own end
            last = end == len(x)
            got.append(F.fir_window(x[o:end], h, D, o, b, e - b, last))
        assert same_bits(np.concatenate(got), whole), (K, D, piece)
    # one sample short on either side is outside the support condition
    assert not F.supported(700, K, D, 100, 100 + RL - 1, 10, False)
    assert not F.supported(700, K, D, 0, 0, 700 - RR + 1, False)
    assert F.supported(700, K, D, 100, 100 + RL, 700 - RL - RR, False)


@pytest.mark.parametrize("K,D", KD + [(1023, 511)])
def test_the_reference_agrees_with_numpy_convolve(K, D):
    """another summation order: each double accumulator differs from numpy.convolve's by at most K * 2^-53 * sum |h| |x| over its own
    terms (K - 1 additions of exact products, each rounding at most 2^-53 of the running magnitude, which the sum of magnitudes bounds)"""
    x, h = signal(3000, 1), taps(K, 1)
    acc = F.fir64(x, h, D)
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    conv = np.convolve(x64, h64, "full")[D:D + len(x)]
    bound = K * 2.0 ** -53 * np.convolve(np.abs(x64), np.abs(h64), "full")[D:D + len(x)]
    err = np.abs(acc - conv)
    print(f"K {K} D {D}: max |ref - convolve| = {err.max():.3e}, largest share of the bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    assert same_bits(F.fir(x, h, D), acc.astype(np.float32))


def test_exact_corners_of_the_reference():
    x = signal(300)
    x[5] = np.float32(-0.0)
    y = F.fir(x, np.ones(1, np.float32), 0)
    assert y.view(np.uint32)[5] == 0 and same_bits(np.delete(y, 5), np.delete(x, 5))        # -0.0 becomes +0.0, nothing else moves
    assert not F.fir(x, np.zeros(9, np.float32), 4).view(np.uint32).any()                   # all-zero taps: +0.0 everywhere
    assert len(F.fir(x[:0], taps(9), 4)) == 0
    assert np.array_equal(F.pcm16(np.array([1.5, -1.5, 0.5, -0.00001], np.float32)), np.array([32767, -32768, 16380, 0], np.int16))


def test_design_is_symmetric_flat_is_the_unit_impulse_and_k_is_odd():
    for K in (1, 3, 511, 1023, 4095):
        for name, kw in E.PRESETS.items():
            eq = E.design(RATE, K, **kw)
            assert eq.taps.dtype == np.float32 and eq.taps.shape == (K,) and eq.delay == (K - 1) // 2 and eq.rate == RATE, (K, name)
            assert same_bits(eq.taps, eq.taps[::-1]), (K, name)
            assert np.all(np.isfinite(eq.taps)), (K, name)
        for flat in (E.design(RATE, K), E.design(RATE, K, bands=((1000.0, 0.0, 1.0),), low_shelf=(200.0, 0.0))):
            want = np.zeros(K, np.float32)
            want[(K - 1) // 2] = 1.0
            assert same_bits(flat.taps, want), K
    for bad in (0, 2, 512, 4096, 4097, -1, 3.5):
        with pytest.raises(ValueError):
            E.design(RATE, bad)
    for kw in (dict(bands=((0.0, 3.0, 1.0),)), dict(bands=((12000.0, 3.0, 1.0),)), dict(bands=((1000.0, 3.0, 0.0),)), dict(bands=((1000.0, 3.0),)),
               dict(low_shelf=(100.0,)), dict(high_shelf=(100.0, float("nan"))), dict(highpass_hz=-1.0), dict(lowpass_hz=20000.0),
               dict(highpass_hz=4000.0, lowpass_hz=3000.0), dict(highpass_hz=(100.0, 0))):
        with pytest.raises(ValueError):
            E.design(RATE, 63, **kw)
    with pytest.raises(ValueError):
        E.design(1000, 63)
    assert E.reach(511) == (255, 255) and E.reach(64, 63) == (0, 63) and E.reach(63, 0) == (62, 0) and E.reach(1, 0) == (0, 0)
    for bad in ((0, 0), (5, 5), (5, -1)):
        with pytest.raises(ValueError):
            E.reach(*bad)


@pytest.mark.parametrize("K", [511, 1023])
def test_deviation_of_every_preset(K):
    assert sorted(E.MEASURED_DEVIATION_DB[K]) == sorted(E.PRESETS)
    for name, kw in E.PRESETS.items():
        eq = E.design(RATE, K, **kw)
        dev, measured = eq.deviation_db(), E.MEASURED_DEVIATION_DB[K][name]
        print(f"K {K} {name}: deviation {dev:.6e} dB, recorded {measured:.6e} dB")
        assert dev <= 1.5 * measured, (K, name, dev, measured)
    # the response the deviation is taken from is the float32 taps' own: a presence lift is where it is asked for
    pres = E.design(RATE, K, **E.PRESETS["presence"])
    r = pres.response_db([100.0, 3000.0, 10000.0])
    assert abs(r[1] - 4.0) < 0.01 and abs(r[0]) < 0.01 and np.all(np.abs(r - E.target_db([100.0, 3000.0, 10000.0], pres.spec)) < 0.01)
    tel = E.design(RATE, K, **E.PRESETS["telephone"]).response_db([50.0, 1000.0, 8000.0])
    assert tel[0] < -20.0 and abs(tel[1]) < 0.5 and tel[2] < -25.0
    with pytest.raises(ValueError):
        E.Equaliser(pres.taps, pres.delay, RATE).deviation_db()
    # taps of the caller's own, not linear-phase: the general evaluation
    own = E.Equaliser(np.array([1.0, -1.0], np.float32), 0, RATE)
    assert abs(own.response_db([RATE / 4.0])[0] - 20.0 * np.log10(np.sqrt(2.0))) < 1e-9


def test_params_accepts_and_refuses():
    assert E.params(None, RATE) is None
    for name in E.PRESETS:
        p = E.params(name, RATE)
        assert sorted(p) == ["delay", "taps"] and p["taps"].dtype == np.float32 and p["taps"].shape == (E.DEFAULT_TAPS,) and p["delay"] == 255
        assert E.params(name, RATE)["taps"] is p["taps"]                      # cached per (spec, rate)
        assert E.params(name, 16000)["taps"] is not p["taps"]
    d = E.params(dict(taps=63, bands=[(2000.0, -3.0, 1.0)], highpass_hz=(120.0, 2)), RATE)
    assert d["taps"].shape == (63,) and d["delay"] == 31
    assert E.params(dict(taps=63, bands=((2000.0, -3.0, 1.0),), highpass_hz=(120.0, 2)), RATE)["taps"] is d["taps"]
    eq = E.design(RATE, 127, low_shelf=(300.0, 2.0))
    assert E.params(eq, RATE)["taps"] is eq.taps and E.params(eq, RATE)["delay"] == 63
    own = E.params((np.array([0.5, 0.25, 0.25]), 0), RATE)
    assert own["delay"] == 0 and own["taps"].dtype == np.float32 and np.array_equal(own["taps"], [0.5, 0.25, 0.25])
    bad = ["loud", 3, 1.5, dict(taps=64), dict(bogus=1), dict(bands=[(1.0,)]), (np.zeros(3),), (np.zeros(0), 0), (np.zeros(4097), 0),
           (np.array([1.0, np.nan]), 0), (np.array([1.0, np.inf]), 1), (np.ones(3), 3), (np.ones(3), -1), (np.ones((2, 2)), 0), (np.ones(3), 0.5),
           dict(bands=[(2000.0, object(), 1.0)])]
    for b in bad:
        with pytest.raises(ValueError):
            E.params(b, RATE)
    with pytest.raises(ValueError):
        E.params(eq, 16000)                                                    # designed for another rate
    with pytest.raises(ValueError):
        E.params("telephone", 6000)                                            # 3400 Hz does not lie below 3000 Hz


@pytest.mark.parametrize("K,D", KD)
def test_fir_planner_with_the_reference_as_window_function(K, D):
    x, h = signal(1111, 2), taps(K, 2)
    whole = F.fir(x, h, D)
    RL, RR = E.reach(K, D)
    for size in (1, 7, 256, RL + RR + 5):
        planner = E.FirPlanner(K, D)
        assert (planner.RL, planner.RR) == (RL, RR)
        seen = []

        def window_fn(samples, in_origin, out_begin, out_count, last):
            assert F.supported(len(samples), K, D, in_origin, out_begin, out_count, last)
            assert len(samples) <= size + RL + RR                            # the history is dropped: a window is never long
            seen.append((planner.received, out_begin + out_count, last))
            return F.fir_window(samples, h, D, in_origin, out_begin, out_count, last)
        chunks = [x[i:i + size] for i in range(0, len(x), size)]
        pieces = list(stream_windows(chunks, planner, window_fn))
        assert same_bits(np.concatenate(pieces), whole), (K, D, size)
        # the stream runs RR samples behind its input: a non-last push emits up to received - RR, the last one everything
        assert all(end == (rec if last else rec - RR) for rec, end, last in seen), (K, D, size)
        assert seen[-1][1] == len(x)


def cases(c):
    rows = [np.sin(0.7 * np.arange(n) + b).astype(np.float32) * 0.9 for b, n in enumerate((5, 0, 9))]
    h = np.array([0.25, 0.5, 0.25, -0.125, 0.0625], np.float32)
    per_row = [(0, 0, -1, True), (3, 4, 2, False), (2, 3, 4, True)]
    out = []
    for pcm16 in (False, True):
        t = "pcm16" if pcm16 else "f32"
        out += [
            (f"fir/{t}", lambda p=pcm16: c.fir(rows, h, pcm16=p)),
            (f"fir/delay/{t}", lambda p=pcm16: c.fir(rows, h, 0, pcm16=p)),
            (f"fir_window/whole/{t}", lambda p=pcm16: c.fir_window(rows, h, pcm16=p)),
            (f"fir_window/part/{t}", lambda p=pcm16: c.fir_window(rows, h, 4, in_origin=3, out_begin=4, out_count=2, last=False, pcm16=p)),
            (f"fir_rows/{t}", lambda p=pcm16: c.fir_rows(rows, h, per_row, pcm16=p)),
        ]
    padded = np.zeros((3, 9), np.float32)
    out.append(("fir/padded", lambda: c.fir(padded, h.astype(np.float64), 1, lengths=(5, 0, 9))))
    for no_sync in (False, True):
        out.append((f"fir_device/{'no_sync' if no_sync else 'sync'}", lambda s=no_sync: c.fir_device(0x1000, (5, 0, 9), 9, h, 2, no_sync=s)))
    return out


def test_fir_bindings_reach_the_library(monkeypatch):
    """the symbol and the arguments of the four Context.fir* forms against a fake library, pinned in tests/fir_bindings_expected.json
    (record mode: ZVX_RECORD_FIR_BINDINGS=1)"""
    lib = FakeLib()
    c = Context.__new__(Context)
    c._lib, c._h, c.hop, c.n_mels, c.hidden = lib, C.c_void_p(0x10), 16, 8, 4
    c.get_int = lambda key: {"sampling_rate": RATE, "fft_size": 64, "hop": 16}[key]
    monkeypatch.setattr(_lib, "_ptr", lambda a: a)
    try:
        got = {}
        for name, call in cases(c):
            del lib.calls[:]
            res = call()
            got[name] = {"calls": json.loads(json.dumps(lib.calls)), "returns": norm_result(res)}
    finally:
        c._h = None
    if os.environ.get("ZVX_RECORD_FIR_BINDINGS") == "1":
        with open(EXPECTED, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
    with open(EXPECTED) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name]["calls"] == want[name]["calls"], name
        assert got[name]["returns"] == want[name]["returns"], name
    # what the record says, spelled out once: the symbol of each form, taps / ntaps / delay between Nmax and out, delay None = (K - 1) // 2
    sym = {n: [cl[0] for cl in v["calls"]] for n, v in want.items()}
    assert sym["fir/f32"] == ["zvx_fir"] and sym["fir_window/part/f32"] == ["zvx_fir_ex"] and sym["fir_rows/pcm16"] == ["zvx_fir_rows"]
    assert sym["fir_device/no_sync"] == ["zvx_fir"]
    args = want["fir/f32"]["calls"][0][1]
    assert args[3:5] == [3, 9] and args[5]["dtype"] == "float32" and args[5]["shape"] == [5] and args[6:8] == [5, 2] and args[9:] == [9, 0]
    assert want["fir/delay/f32"]["calls"][0][1][7] == 0
    assert want["fir_window/part/pcm16"]["calls"][0][1][7:] == [4, want["fir_window/part/pcm16"]["calls"][0][1][8], 9, _lib.ZVX_PCM16, 3, 4, 2, 0]
    dev = want["fir_device/no_sync"]["calls"][0][1]
    assert dev[1] == dev[8] == {"void_p": 0x1000} and dev[9:] == [9, _lib.ZVX_DEVICE_IN | _lib.ZVX_DEVICE_OUT | _lib.ZVX_NO_SYNC]
    assert want["fir_device/no_sync"]["returns"] is None and set(_lib.EXPORTS) >= {"zvx_fir", "zvx_fir_ex", "zvx_fir_rows"}
