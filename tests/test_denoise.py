"""The vocoder-bias denoiser, the parts that need no GPU: the float64 reference of tests/denoise_ref.py against the properties include/zvx.h
states, and the surface of the feature (header, exports, bindings, keyword checks that run before a device is touched)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import denoise_ref as D
from zerovox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP = 1024, 256


def header():
    with open(os.path.join(ROOT, "include", "zvx.h")) as f:
        return f.read()


@pytest.mark.parametrize("n", [700, 1024, 5000])
def test_zero_bias_reconstructs_every_covered_sample(n):
    x = np.random.default_rng(n).uniform(-1.0, 1.0, n)
    out, covered = D.denoise(x, np.zeros(N_FFT // 2 + 1), 1.0, with_cover=True)
    assert covered.all()                                      # at 1024 / 256 the pass-through rule engages nowhere
    assert np.max(np.abs(out - x)) <= 1e-12


def test_strength_zero_is_the_row_itself():
    x = np.random.default_rng(1).uniform(-1.0, 1.0, 900)
    assert np.array_equal(D.denoise(x, np.ones(N_FFT // 2 + 1), 0.0), x)


@pytest.mark.parametrize("k,s", [(40, 0.5), (100, 30.0), (3, 200.0)])
def test_a_sine_on_a_bin_is_attenuated_by_the_predicted_gain(k, s):
    """x = A cos(2 pi k i / n_fft + phi) sits on bin k of every frame: |X[f][k]| = m = A sum(w) / 2 = A n_fft / 4, and with bias = delta_k that
    line is scaled by the predicted G = 1 - s b / m.  The Hann's two side lines (k +- 1, half the size) meet a zero bias and stay.  Taking
    (1 - G) of the centre line off a windowed frame takes (1 - G) / 2 x off it (the centre line of w x is x / 2), so the frame becomes
    (w - (1 - G) / 2) x, and the overlap-add of the interior, sum w (w - (1 - G) / 2) / sum w^2 with sum w = 2 and sum w^2 = 3 / 2 at
    hop = n_fft / 4, hands back x (1 - 2 (1 - G) / 3)."""
    n, A = 8 * N_FFT, 0.8
    x = A * np.cos(2.0 * np.pi * k * np.arange(n) / N_FFT + 0.3)
    bias = np.zeros(N_FFT // 2 + 1)
    bias[k] = 1.0
    m = A * N_FFT / 4.0
    G = 1.0 - s / m
    assert 0.0 < G < 1.0
    inner = slice(N_FFT, n - N_FFT)                           # frames that see no reflected edge
    X = D.analysis(x, N_FFT, HOP, N_FFT)[4:-4]
    assert np.max(np.abs(np.abs(X[:, k]) - m)) <= 1e-9 and np.max(np.abs(np.abs(X[:, k + 1]) - m / 2)) <= 1e-9
    out = D.denoise(x, bias, s)
    assert np.max(np.abs(out[inner] - (1.0 - 2.0 * (1.0 - G) / 3.0) * x[inner])) <= 1e-9
    # a floor above G wins
    Gf = min(1.0, G + 0.05)
    out_f = D.denoise(x, bias, s, floor=Gf)
    assert np.max(np.abs(out_f[inner] - (1.0 - 2.0 * (1.0 - Gf) / 3.0) * x[inner])) <= 1e-9


def test_huge_bias_with_floor_zero_silences_the_row():
    x = np.random.default_rng(2).uniform(-1.0, 1.0, 1500)
    out = D.denoise(x, np.full(N_FFT // 2 + 1, 1e30), 1.0)
    assert np.array_equal(out, np.zeros_like(x)) and not np.signbit(out).any()


def test_pass_through_rule_engages_when_hop_exceeds_the_padding():
    """hop > pad: n_fft 64 / hop 48 with a window of 32 centred in the frame leaves positions no window reaches -- there the input's own
    sample comes out, everywhere else the zero-bias reconstruction"""
    n_fft, hop, wl, n = 64, 48, 32, 400
    assert hop > (n_fft - hop) // 2 and n >= D.min_samples(n_fft, hop)
    x = np.random.default_rng(3).uniform(-1.0, 1.0, n)
    bias = np.full(n_fft // 2 + 1, 1e30)
    out, covered = D.denoise(x, bias, 1.0, n_fft=n_fft, hop=hop, win_length=wl, with_cover=True)
    assert 0 < covered.sum() < n
    assert np.array_equal(out[~covered], x[~covered]) and np.all(out[covered] == 0.0)
    rec = D.denoise(x, np.zeros(n_fft // 2 + 1), 1.0, n_fft=n_fft, hop=hop, win_length=wl)
    assert np.max(np.abs(rec - x)) <= 1e-12
    # the threshold is relative to the fully overlapped sum
    w2 = D.window(n_fft, wl) ** 2
    assert D.den_threshold(n_fft, hop, wl) == 1e-3 * max(w2[t::hop].sum() for t in range(hop))


def test_rows_are_framed_as_the_mel_front_end_frames_them():
    from zerovox_amd import mels
    assert np.array_equal(D.window(N_FFT, N_FFT).astype(np.float32), mels.stft_basis(N_FFT, N_FFT)[0].astype(np.float32))
    assert np.array_equal(D.window(64, 32).astype(np.float32), mels.stft_basis(64, 32)[0].astype(np.float32))
    for n in (385, 700, 1024, 5000):
        pad, F = D.geometry(n, N_FFT, HOP)
        assert pad == 384 and F == 1 + (n + 768 - 1024) // 256 and D.frames(np.zeros(n), N_FFT, HOP).shape == (F, N_FFT)
    assert D.min_samples(N_FFT, HOP) == 385


def test_bias_is_the_mean_magnitude_over_all_frames():
    x = np.random.default_rng(4).uniform(-1.0, 1.0, 88 * HOP)
    b = D.bias_of(x)
    X = D.analysis(x, N_FFT, HOP, N_FFT)
    assert X.shape == (88, N_FFT // 2 + 1) and b.shape == (N_FFT // 2 + 1,)
    assert np.allclose(b, np.abs(X).sum(axis=0) / 88.0, rtol=1e-14, atol=0) and np.all(b >= 0)


def test_pcm16_rule():
    v = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.2, -1.2, 3.05e-5], np.float32)
    assert D.pcm16(v).tolist() == [0, 16380, -16380, 32760, -32760, 32767, -32768, 0]


def test_header_declares_the_entry_points():
    h = header()
    assert re.search(r"zvx_status\s+zvx_denoise_bias\s*\(\s*zvx_ctx\*\s*\w*,\s*float\*\s*bias\s*\)\s*;", h)
    decl = re.search(r"zvx_status\s+zvx_denoise\s*\(([^;]*)\)\s*;", h).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "in", "nsamples", "B", "Nmax", "bias", "params", "out", "out_stride", "flags"]
    assert re.search(r"typedef struct zvx_denoise_params\s*\{\s*float\s+strength;[^}]*float\s+floor;[^}]*\}\s*zvx_denoise_params;", h)
    assert "post.denoise" in h and "NOT measured" in h       # the perceptual benefit is stated as unmeasured
    assert [n for n, _ in _lib.DenoiseParams._fields_] == ["strength", "floor"] and C.sizeof(_lib.DenoiseParams) == 8


def test_library_exports_the_entry_points():
    assert "zvx_denoise" in _lib.EXPORTS and "zvx_denoise_bias" in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "zvx_denoise") and hasattr(lib, "zvx_denoise_bias")
    lib.zvx_denoise.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    lib.zvx_denoise_bias.argtypes = [C.c_void_p, C.c_void_p]
    # a NULL context is refused before anything else is looked at
    assert lib.zvx_denoise(None, None, None, 0, 0, None, None, None, 0, 0) == _lib.ZVX_E_INVALID
    assert lib.zvx_denoise_bias(None, None) == _lib.ZVX_E_INVALID


def test_bindings_and_keywords():
    from zerovox_amd.model import ZeroVox
    from zerovox_amd.synthesize import ZeroVoxTTS
    p = inspect.signature(_lib.Context.denoise).parameters
    assert list(p)[1:] == ["rows", "bias", "strength", "floor", "pcm16", "lengths"] and p["floor"].default == 0.0
    p = inspect.signature(_lib.Context.denoise_device).parameters
    assert list(p)[1:] == ["ptr", "lengths", "Nmax", "bias", "strength", "floor", "no_sync"]
    assert p["floor"].kind is inspect.Parameter.KEYWORD_ONLY and p["no_sync"].default is False
    assert hasattr(_lib.Context, "denoise_bias")
    for f in (ZeroVoxTTS.tts, ZeroVoxTTS.tts_ex, ZeroVoxTTS.tts_long, ZeroVoxTTS.tts_stream, ZeroVox.inference_ex):
        assert inspect.signature(f).parameters["denoise"].default is None, f
    assert isinstance(ZeroVoxTTS.denoise_bias, property) and callable(ZeroVoxTTS.refresh_denoise_bias)


def test_refusals_come_before_the_model_is_touched():
    from zerovox_amd.synthesize import ZeroVoxTTS
    synth = ZeroVoxTTS.__new__(ZeroVoxTTS)                    # no model, no device: a refusal must not need either
    for bad in (-0.01, float("nan"), float("inf"), -float("inf")):
        for call in (synth.tts, synth.tts_ex, synth.tts_long):
            with pytest.raises(ValueError, match="denoise"):
                call("hello there", None, denoise=bad)
    with pytest.raises(ValueError, match="denoise"):
        synth.tts_stream("hello there", None, denoise=0.01)
    assert ZeroVoxTTS._denoise(None) is None and ZeroVoxTTS._denoise(0.01) == dict(strength=0.01, floor=0.0)
