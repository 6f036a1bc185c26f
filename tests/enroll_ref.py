"""Float reference of zvx_spkemb_wav as include/zvx.h composes it: resample_ref (float64 polyphase filter), join_ref.bounds_ref (float64
trim decisions), the crop, oracle.mel_oracle on the window and the oracle speaker encoder.  Imports nothing from zerovox_amd but the model
configuration and the synthetic weights the oracle runs on; it never touches the library."""
import numpy as np

import join_ref as J
import resample_ref as R
from oracle import mel_oracle as MO

NATIVE = 22050
QUIET = 1e-4


def audio_args(cfg):
    a = cfg["audio"]
    return dict(sampling_rate=a["sampling_rate"], fft_size=a["fft_size"], hop_size=a["hop_size"], win_length=a["win_length"],
                num_mels=a["num_mels"], fmin=a["fmin"], fmax=a["fmax"])


def make_clips(seed=0, rate=NATIVE):
    """Five ragged reference clips at `rate`: a voiced tone (amplitude-modulated, with 0.02 of noise) between a head and a tail of 1e-4
    noise of different lengths -- about 35 000, 12 000, 20 000 and 7 700 samples at 22 050 Hz -- and one all-voiced clip of about 1 500
    samples, shorter than the 2048-sample trim frame and so left whole by it."""
    rng = np.random.default_rng(seed)
    k = rate / float(NATIVE)
    clips = []
    for head, body, tail, f0 in ((3000, 29400, 2613, 140.0), (0, 7903, 4100, 196.0), (5000, 15011, 0, 110.0), (1700, 5142, 900, 233.0),
                                 (0, 1501, 0, 175.0)):
        head, body, tail = int(round(head * k)), int(round(body * k)), int(round(tail * k))
        t = np.arange(body) / float(rate)
        voiced = 0.25 * np.sin(2 * np.pi * f0 * t + 0.7) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(body)
        clips.append(np.concatenate([QUIET * rng.standard_normal(head), voiced, QUIET * rng.standard_normal(tail)]).astype(np.float32))
    return clips


def at_model_rate(x, rate, native=NATIVE):
    """step 1: the clip as a float32 signal at the model's rate"""
    x = np.asarray(x, np.float32)
    return x if int(rate) == int(native) else R.resample_ref(x, rate, native).astype(np.float32)


def window_ref(x, frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0):
    """steps 2 and 3 on a model-rate signal -> (begin, end, worst): the trim bounds, cut to max_samples, and bounds_ref's distance of the
    nearest frame from the trim threshold"""
    begin, end, worst = J.bounds_ref(x, frame, hop, top_db, keep)
    if max_samples > 0:
        end = min(end, begin + int(max_samples))
    return begin, end, worst


def frames_ref(m, fft_size=1024, hop_size=256):
    pad = (fft_size - hop_size) // 2
    return 1 + (int(m) + 2 * pad - fft_size) // hop_size


def window_mel(x, begin, end, sampling_rate, fft_size, hop_size, win_length, num_mels, fmin, fmax):
    """step 4 by INDEX arithmetic on the whole row, the way a device kernel has to do it: sample i of the padded window is
    x[begin + reflect(i - pad)] with the mirror about the window's own first and last sample -> log-mel [frames][num_mels] f32"""
    x = np.asarray(x, np.float32)
    m, pad = int(end) - int(begin), (fft_size - hop_size) // 2
    assert m > pad, "the reflect padding needs more samples than it adds"
    k = np.abs(np.arange(-pad, m + pad))
    k = np.where(k >= m, 2 * (m - 1) - k, k)
    xp = x[int(begin) + k]
    mag = MO.stft_magnitude(xp, fft_size, hop_size, win_length).astype(np.float32)
    mel = MO.mel_basis(sampling_rate, fft_size, num_mels, fmin, fmax).astype(np.float32) @ mag
    return np.log(np.clip(mel, 1e-5, None)).astype(np.float32).T


def embed_ref(x, rate, sd, cfg, frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0):
    """the whole chain for one clip -> (embedding [hidden] float64-accurate, begin, end, frames, worst)"""
    from oracle import zvx_oracle as O
    a = audio_args(cfg)
    y = at_model_rate(x, rate, a["sampling_rate"])
    begin, end, worst = window_ref(y, frame, hop, top_db, keep, max_samples)
    mel = window_mel(y, begin, end, **a)
    assert mel.shape[0] == frames_ref(end - begin, a["fft_size"], a["hop_size"])
    return np.asarray(O.resnet_se34v2(mel, sd, cfg)), begin, end, mel.shape[0], worst
