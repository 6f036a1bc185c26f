"""What the ctypes bindings of the post-processing steps hand to the library, and what they hand back, pinned call by call.

A Context is built around a FAKE library: every symbol is a function that records (symbol, arguments) and returns ZVX_OK without
writing anything.  The records and the dtypes and shapes of the returned values are compared with tests/post_bindings_expected.json,
which this module's record mode wrote (ZVX_RECORD_POST_BINDINGS=1 python -m pytest tests/test_post_bindings.py); the bindings may be
reorganised freely as long as every call still reaches the library with the same symbol and the same arguments.  No GPU, no libzvx."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from zerovox_amd import _lib
from zerovox_amd._lib import Context

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "post_bindings_expected.json")
INTS = {"sampling_rate": 22050, "fft_size": 64, "hop": 16}
LENGTHS = (5, 0, 9)
NMAX = max(LENGTHS)
DEV = 0x1000
WHOLE, PART = (0, 0, -1, True), (3, 4, 2, False)
PER_ROW = [(0, 0, -1, True), (3, 4, 2, False), (2, 3, 4, True)]
KEY = 0x0123456789ABCDEF


def norm_arg(a):
    """an argument as JSON: arrays -> dtype, shape, bytes; byref structs and ctypes arrays -> bytes; c_void_p -> value; ints as they are"""
    if a is None or isinstance(a, (bool, int, str)):
        return a
    if isinstance(a, (np.integer,)):
        return int(a)
    if isinstance(a, np.ndarray):
        return {"dtype": str(a.dtype), "shape": list(a.shape), "bytes": np.ascontiguousarray(a).tobytes().hex()}
    if isinstance(a, C.c_void_p):
        return {"void_p": a.value}
    if hasattr(a, "_obj"):                                   # ctypes.byref(struct)
        return {"byref": type(a._obj).__name__, "bytes": bytes(a._obj).hex()}
    if isinstance(a, (C.Array, C.Structure)):
        return {"ctypes": type(a).__name__, "bytes": bytes(a).hex()}
    raise TypeError(f"argument of type {type(a)}")


def norm_result(r):
    """a returned value as JSON: the dtypes and shapes of its arrays, its containers as they nest"""
    if isinstance(r, np.ndarray):
        return {"dtype": str(r.dtype), "shape": list(r.shape)}
    if isinstance(r, dict):
        return {"dict": {k: norm_result(v) for k, v in sorted(r.items())}}
    if isinstance(r, tuple) and hasattr(r, "_fields"):
        return {type(r).__name__: {k: norm_result(v) for k, v in zip(r._fields, r)}}
    if isinstance(r, (list, tuple)):
        return {type(r).__name__: [norm_result(v) for v in r]}
    if r is None or isinstance(r, (bool, int, float, str)):
        return r
    return {"type": type(r).__name__}


class FakeLib:
    """every attribute is a function that records (symbol, normalised arguments) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append([name, [norm_arg(a) for a in args]])
            return 0
        return call


def rows():
    return [np.sin(0.7 * np.arange(n) + b).astype(np.float32) * 0.9 for b, n in enumerate(LENGTHS)]


def cases(c):
    """(name, call) of every binding of the post-processing steps, in the forms the issue of the shared call path lists"""
    bias = np.linspace(0.0, 1.0, INTS["fft_size"] // 2 + 1).astype(np.float32)
    n = np.array(LENGTHS, np.int32)
    wm = dict(depth_db=1.5, lo_hz=300.0, hi_hz=7000.0, block_frames=4, band_bins=2, period_blocks=8)
    out = []
    for pcm16 in (False, True):
        t = "pcm16" if pcm16 else "f32"
        out += [
            (f"limit/{t}", lambda p=pcm16: c.limit(rows(), 0.8, window_ms=2.0, oversample=2, pcm16=p)),
            (f"limit_rows/{t}", lambda p=pcm16: c.limit_rows(rows(), 0.8, PER_ROW, pcm16=p, rate=16000)),
            (f"denoise/{t}", lambda p=pcm16: c.denoise(rows(), bias, 0.5, floor=0.1, pcm16=p)),
            (f"denoise_rows/{t}", lambda p=pcm16: c.denoise_rows(rows(), bias, 0.5, PER_ROW, pcm16=p)),
            (f"level/{t}", lambda p=pcm16: c.level(rows(), -23.0, max_gain_db=12.0, pcm16=p)),
            (f"level_rows/{t}", lambda p=pcm16: c.level_rows(rows(), PER_ROW, -23.0, window_ms=400.0, pcm16=p, rate=16000)),
            (f"watermark/{t}", lambda p=pcm16: c.watermark(rows(), KEY, pcm16=p, **wm)),
            (f"watermark_rows/keys/{t}", lambda p=pcm16: c.watermark_rows(rows(), [1, 2, 1], PER_ROW, pcm16=p, **wm)),
            (f"watermark_rows/one_key/{t}", lambda p=pcm16: c.watermark_rows(rows(), None, None, pcm16=p, key=KEY)),
            (f"resample_rows/{t}", lambda p=pcm16: c.resample_rows(rows(), 22050, 16000, PER_ROW, pcm16=p)),
            (f"resample_rows/3-tuples/{t}", lambda p=pcm16: c.resample_rows(rows(), 22050, 48000, [w[:3] for w in PER_ROW], pcm16=p)),
            (f"normalize/{t}", lambda p=pcm16: c.normalize(rows(), -23.0, peak_ceiling=0.5, common=True, pcm16=p)),
        ]
        for wn, w in (("whole", WHOLE), ("part", PART)):
            kw = dict(in_origin=w[0], out_begin=w[1], out_count=w[2], last=w[3])
            out += [
                (f"limit_window/{wn}/{t}", lambda p=pcm16, kw=kw: c.limit_window(rows(), 0.8, pcm16=p, **kw)),
                (f"denoise_window/{wn}/{t}", lambda p=pcm16, kw=kw: c.denoise_window(rows(), bias, 0.5, pcm16=p, **kw)),
                (f"level_window/{wn}/{t}", lambda p=pcm16, kw=kw: c.level_window(rows(), -23.0, pcm16=p, **kw)),
                (f"watermark_window/{wn}/{t}", lambda p=pcm16, kw=kw: c.watermark_window(rows(), KEY, pcm16=p, **kw, **wm)),
                (f"resample_window/{wn}/{t}", lambda p=pcm16, w=w: c.resample_window(rows(), 22050, 16000, w[0], w[1], w[2], pcm16=p)),
            ]
    padded = np.zeros((len(LENGTHS), NMAX), np.float32)
    for b, r in enumerate(rows()):
        padded[b, :len(r)] = r
    out.append(("limit/padded", lambda: c.limit(padded, 0.8, lengths=LENGTHS)))
    for no_sync in (False, True):
        t = "no_sync" if no_sync else "sync"
        out += [
            (f"limit_device/{t}", lambda s=no_sync: c.limit_device(DEV, LENGTHS, NMAX, 0.8, window_ms=2.0, no_sync=s)),
            (f"denoise_device/{t}", lambda s=no_sync: c.denoise_device(DEV, LENGTHS, NMAX, bias, 0.5, floor=0.1, no_sync=s)),
            (f"watermark_device/{t}", lambda s=no_sync: c.watermark_device(DEV, LENGTHS, NMAX, KEY, no_sync=s, **wm)),
            (f"normalize_device/{t}", lambda s=no_sync: c.normalize_device(DEV, LENGTHS, NMAX, -23.0, max_gain_db=6.0, no_sync=s)),
        ]
    det = {k: v for k, v in wm.items()}
    out += [
        ("loudness_stats", lambda: c.loudness_stats(rows())),
        ("loudness_stats/curves", lambda: c.loudness_stats(rows(), rate=100, curves=True)),
        ("loudness_stats_device", lambda: c.loudness_stats_device(DEV, LENGTHS, NMAX, curves=True)),
        ("pitch", lambda: c.pitch(rows())),
        ("pitch/no_curves", lambda: c.pitch(rows(), rate=16000, window=4, hop=2, curves=False)),
        ("pitch_device", lambda: c.pitch_device(DEV, LENGTHS, NMAX, fmin=80.0)),
        ("true_peak", lambda: c.true_peak(rows(), oversample=2)),
        ("true_peak_device", lambda: c.true_peak_device(DEV, LENGTHS, NMAX, rate=48000)),
        ("watermark_detect", lambda: c.watermark_detect(rows(), KEY, window_frames=0, **det)),
        ("watermark_detect/padded", lambda: c.watermark_detect(padded, KEY, lengths=n, threshold=4.0)),
        ("watermark_detect/device", lambda: c.watermark_detect(None, KEY, lengths=LENGTHS, device_ptr=DEV, Nmax=NMAX, **det)),
        ("watermark_identify", lambda: c.watermark_identify(rows(), [3, KEY, 5], window_frames=0, **det)),
        ("watermark_identify/device", lambda: c.watermark_identify(None, [3, KEY], lengths=LENGTHS, device_ptr=DEV, Nmax=NMAX, key=9)),
    ]
    return out


@pytest.fixture
def ctx(monkeypatch):
    lib = FakeLib()
    c = Context.__new__(Context)
    c._lib, c._h, c.hop, c.n_mels, c.hidden = lib, C.c_void_p(0x10), INTS["hop"], 8, 4
    c.get_int = lambda key: INTS[key]
    monkeypatch.setattr(_lib, "_ptr", lambda a: a)           # arrays reach the fake library as they are
    # (an output array made with numpy.empty would put arbitrary bytes into the record)
    monkeypatch.setattr(np, "empty", lambda shape, dtype=float, **kw: np.zeros(shape, dtype))
    yield c
    c._h = None


def run_cases(c):
    got = {}
    for name, call in cases(c):
        del c._lib.calls[:]
        res = call()
        got[name] = {"calls": json.loads(json.dumps(c._lib.calls)), "returns": norm_result(res)}
    return got


def test_post_bindings_reach_the_library_unchanged(ctx):
    got = run_cases(ctx)
    if os.environ.get("ZVX_RECORD_POST_BINDINGS") == "1":
        with open(EXPECTED, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
    with open(EXPECTED) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name]["calls"] == want[name]["calls"], name
        assert got[name]["returns"] == want[name]["returns"], name
