"""Host synthesis API: drop-in for ``zerovox.tts.synthesize.ZeroVoxTTS`` (synthesize.py:38-328).

Same method names, argument meaning, return order and sentinel/error behaviour; tensors are NumPy arrays
instead of torch tensors and all model arithmetic runs in libzvx (HIP, gfx950).
"""
from __future__ import annotations

import glob
import os
import time
import wave

import numpy as np

from . import _lib
from .mels import trim_silence
from .model import ZeroVox, load_meldec_weights, load_tts_weights
from .normalize import ZeroVoxNormalizer
from .symbols import Symbols

DEFAULT_TTS_MODEL_NAME_EN = "tts_en_zerovox2_medium_2_styledec"          # synthesize.py:34-36
DEFAULT_TTS_MODEL_NAME_DE = "tts_de_zerovox2_medium_3_styledec"
DEFAULT_REFAUDIO = "en_kevin.wav"


def _float_row(wav):
    """one waveform, float or int16 PCM (read as the samples it encodes, / 32760) -> a float32 row"""
    wav = np.asarray(wav)
    if wav.dtype == np.int16:
        wav = wav.astype(np.float32) / np.float32(32760.0)
    return np.asarray(wav, np.float32).reshape(-1)


class ZeroVoxTTS:

    @staticmethod
    def get_default_model(lang: str):
        if lang == "en":
            return os.getenv("ZEROVOX_TTS_MODEL_EN", DEFAULT_TTS_MODEL_NAME_EN)
        if lang == "de":
            return os.getenv("ZEROVOX_TTS_MODEL_DE", DEFAULT_TTS_MODEL_NAME_DE)
        return None

    def __init__(self, language, syms: Symbols, model: ZeroVox, meldec_model, hop_length, sampling_rate, n_mel_channels,
                 fft_size, win_length, mel_fmin, mel_fmax, infer_device="cuda", num_threads=-1, verbose=False):
        self._hop_length, self._infer_device, self._sampling_rate = hop_length, infer_device, sampling_rate
        self._language, self._meldec_model = language, meldec_model
        self._fft_size, self._win_length, self._num_mels = fft_size, win_length, n_mel_channels
        self._mel_fmin, self._mel_fmax, self._verbose = mel_fmin, mel_fmax, verbose
        self._model = model
        self._symbols = syms
        self._normalizer = ZeroVoxNormalizer(language)
        # num_threads: the reference sets torch's global intra-op thread count (synthesize.py:93-94);
        # there is no host compute here, the argument is accepted and ignored.

    @staticmethod
    def available_speakerrefs(refdir=None):
        """Bundled reference voices (synthesize.py:99-110).  The build ships no audio assets: lists ``refdir``."""
        if refdir is None or not os.path.isdir(refdir):
            return []
        return sorted((f for f in os.listdir(refdir) if f.endswith(".wav")), key=str.casefold)

    @staticmethod
    def _read_pcm(path):
        """a wav file (8/16/32-bit PCM) -> (float32 mono in [-1, 1), its sampling rate)"""
        with wave.open(str(path), "rb") as w:
            sr, nch, sw = w.getframerate(), w.getnchannels(), w.getsampwidth()
            raw = w.readframes(w.getnframes())
        dt = {1: np.uint8, 2: np.int16, 4: np.int32}[sw]
        a = np.frombuffer(raw, dtype=dt).astype(np.float32)
        a = (a - 128.0) / 128.0 if sw == 1 else a / float(2 ** (8 * sw - 1))
        if nch > 1:
            a = a.reshape(-1, nch).mean(axis=1)
        return a, sr

    @staticmethod
    def get_speakerref(speakerref, sampling_rate):
        """Load a reference wav (8/16/32-bit PCM) as float32 mono at ``sampling_rate`` (synthesize.py:112-121).  The reference
        goes through ``librosa.load(sr=sampling_rate)``, which resamples with soxr_hq; here a file at another rate is
        resampled with a polyphase Kaiser filter (scipy.signal.resample_poly) -- the same band-limited signal, not
        bit-identical to soxr (parity of resampled references is unpinned: librosa/soxr are not installable here)."""
        a, sr = ZeroVoxTTS._read_pcm(speakerref)
        if sr != sampling_rate:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(sr), int(sampling_rate))
            a = resample_poly(a.astype(np.float64), int(sampling_rate) // g, int(sr) // g).astype(np.float32)
        return a

    def speakerref_samples(self, path):
        """A reference wav file as float32 mono at the model's rate: read at its own rate and converted on the device (zvx_resample),
        where ``get_speakerref`` -- a static method without a context -- converts on the host."""
        a, sr = self._read_pcm(path)
        if sr != self._sampling_rate:
            a = self._model.ctx.resample([a], sr, self._sampling_rate)[0][0]
        return a

    def speaker_embed_file(self, path):
        """reference wav file -> [1, 1, hidden] speaker embedding; every step after the PCM decoding runs in libzvx"""
        return self.speaker_embed(self.speakerref_samples(path))

    def speaker_embed(self, wav: np.ndarray, sampling_rate=None):
        """wav -> [1, 1, hidden] speaker embedding (synthesize.py:123-143).  ``sampling_rate``: the rate of ``wav`` where it is not the
        model's; it is converted on the device before the trim, as librosa.load(sr=...) converts before librosa.effects.trim."""
        if sampling_rate is not None and int(sampling_rate) != int(self._sampling_rate):
            wav = self._model.ctx.resample([np.asarray(wav, np.float32)], int(sampling_rate), self._sampling_rate)[0][0]
        wav = trim_silence(wav, top_db=40)
        mel, frames = self._model.ctx.melspec([wav])                      # get_mel_from_wav on the device (zvx_melspec)
        return self._model._spkemb(mel[:, :int(frames[0])])

    def speaker_embed_batch(self, wavs, sampling_rate=None, *, top_db=40.0, max_seconds=None):
        """reference clips -> [B, 1, hidden] speaker embeddings, enrolled on the device (include/zvx.h, zvx_spkemb_wav): conversion to the
        model's rate, the silence trim of ``speaker_embed`` (top_db; <= 0: none), the log-mel front end and the speaker encoder run there
        for the whole batch, and only the embeddings come back.  ``sampling_rate``: None (the model's), one rate for all clips, or one per
        clip; the clips are grouped by rate, one call per distinct rate, and the results come back in input order.  ``max_seconds``: None,
        or the length each clip is cut to after trimming.  A clip that trims to less than two mel frames raises ZvxError, as
        ``speaker_embed`` does for it."""
        wavs = [np.asarray(w, np.float32).reshape(-1) for w in wavs]
        B = len(wavs)
        if sampling_rate is None or np.ndim(sampling_rate) == 0:
            rates = [int(self._sampling_rate if sampling_rate is None else sampling_rate)] * B
        else:
            rates = [int(r) for r in sampling_rate]
            if len(rates) != B:
                raise ValueError(f"speaker_embed_batch: {B} clips, {len(rates)} sampling rates")
        cut = 0 if max_seconds is None else max(1, int(round(float(max_seconds) * self._sampling_rate)))
        ctx = self._model.ctx
        out = np.zeros((B, 1, ctx.hidden), np.float32)
        for rate in sorted(set(rates)):
            idx = [i for i in range(B) if rates[i] == rate]
            emb = ctx.spkemb_wav([wavs[i] for i in idx], rate, top_db=top_db, max_samples=cut)[0]
            out[idx, 0, :] = emb
        return out

    def speaker_embed_files(self, paths):
        """reference wav files -> [B, 1, hidden]: ``speaker_embed_batch`` over the decoded PCM, every file at its own rate"""
        clips = [self._read_pcm(p) for p in paths]
        return self.speaker_embed_batch([a for a, _ in clips], [sr for _, sr in clips])

    def speaker_embed_from_mel(self, mel: np.ndarray):
        """[Tr, n_mels] log-mel -> [1, 1, hidden] (precomputed-mel entry used by the benchmarks)."""
        return self._model._spkemb(np.asarray(mel, np.float32)[None])

    def transcript2phonemids(self, transcript: str):
        """synthesize.py:145-190: whitespace/punctuation runs collapse to the max punct id on the previous phone."""
        phones, puncts = [], []
        punct = 0
        i, n = 0, len(transcript)
        while i < n:
            p = transcript[i]
            if p == " " or self._symbols.is_punct(p):
                while i < n and (transcript[i] == " " or self._symbols.is_punct(transcript[i])):
                    punct = max(punct, self._symbols.encode_punct(transcript[i]))
                    i += 1
                if puncts:
                    puncts[-1] = punct
                continue
            if self._symbols.is_phone(p):
                punct = 0
                phones.append(self._symbols.encode_phone(p))
                puncts.append(punct)
            i += 1
        return phones, puncts

    def text2phonemeids(self, text: str):
        transcript_uroman, _ = self._normalizer.normalize(text)
        phone_ids, punct_ids = self.transcript2phonemids(transcript_uroman)
        if self._verbose:
            print(f"Raw Text Sequence: {text}\nNormalized       : {transcript_uroman}")
            print(f"Phoneme IDs      : {phone_ids}\nPunct IDs        : {punct_ids}")
        return phone_ids, punct_ids

    @staticmethod
    def _prosody(speed, pitch_shift, pitch_range, energy_shift, energy_range):
        """the keyword scalars as Prosody.create keywords, or None when all are at their defaults (the uncontrolled call)"""
        kw = dict(speed=speed, pitch_shift=pitch_shift, pitch_range=pitch_range, energy_shift=energy_shift, energy_range=energy_range)
        return None if kw == dict(speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0) else kw

    @staticmethod
    def _loudness(loudness, peak_db):
        """the loudness keywords as Context.normalize_device keywords, or None (nothing is normalised)"""
        from .longform import peak_ceiling
        return None if loudness is None else dict(target=float(loudness), peak_ceiling=peak_ceiling(peak_db))

    @staticmethod
    def _denoise(denoise):
        """the denoise keyword as Context.denoise_device keywords, or None (nothing is denoised); checked without a device"""
        if denoise is None:
            return None
        s = float(denoise)
        if not np.isfinite(s) or s < 0:
            raise ValueError(f"denoise must be None or a finite strength >= 0, not {denoise!r}")
        return dict(strength=s, floor=0.0)

    @staticmethod
    def _limiter(limiter, limiter_ms, peak_db):
        """the limiter keywords as Context.limit_device keywords, or None (nothing is limited)"""
        from .longform import limit_keywords
        return limit_keywords(limiter, limiter_ms, peak_db)

    def tts_ex(self, text: str, spkemb, duration=None, *, speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0,
               loudness=None, peak_db=-1.0, limiter=False, limiter_ms=5.0, denoise=None, report=False, pitch_report=False, watermark=None,
               voice_report=False, eq=None):
        """-> (wav f32[N], phoneme i32[1,T], length, mel f32[n_mels, L]); empty text -> the reference's sentinel
        (synthesize.py:213-239).  Prosody (include/zvx.h, zvx_prosody): speed = speaking-rate factor (2.0: half the frames),
        pitch / energy shift (in normalised predictor units) and range (spread about the utterance mean).
        loudness: None (the default: the level the model gives), or the integrated loudness in LUFS (BS.1770 / R128) the waveform is
        brought to on the device (include/zvx.h, zvx_normalize): the vocoder's row stays there, is measured and multiplied by one gain in
        place -- at most +20 dB, and no sample above peak_db dBFS (None: no ceiling) --, an ``output_rate`` converts it afterwards (the
        ceiling applies before that conversion) and only then it comes to the host; ``last_loudness`` reports dict(lufs, peak, gain).
        limiter: with True a look-ahead limiter (include/zvx.h, zvx_limit) holds the row under peak_db dBFS on the device, its gain
        smoothed over limiter_ms on either side and driven by the 4x oversampled (true-peak) envelope.  With ``loudness`` the gain is
        then NOT bounded by the peak (only by +20 dB), so the target is reached and the limiter takes the peaks; without it the row is
        just limited.  Order: gain, limiter, output-rate conversion, copy to the host.  ``last_limit`` reports dict(peak_in, min_gain).
        denoise: None (the default: no launch, buffer or table of it exists), or the strength of the vocoder-bias denoiser (include/zvx.h,
        zvx_denoise; NVIDIA's scripts use 0.01): that multiple of ``denoise_bias`` is taken off the magnitude of every STFT bin of the
        vocoder's row, on the device, in place, directly behind the vocoder -- before the gain, the limiter and the rate conversion.
        Its audible benefit on a real checkpoint is not measured here.
        watermark: None (the default: nothing changes, bit for bit), an int key, or a dict with ``key`` and any of watermark.EMBED_DEFAULTS
        (depth_db, lo_hz, hi_hz, block_frames, band_bins, period_blocks): the keyed mark of include/zvx.h, zvx_watermark, laid on the
        vocoder's row on the device, in place, behind the denoiser and before the loudness gain and the limiter; ``detect_watermark``
        finds it again with the key.  Whether it is inaudible on a real checkpoint, and whether it survives lossy codecs,
        time-stretching or deliberate removal, is not measured.
        eq: None (the default: no launch, buffer or upload of it exists), a preset name of zerovox_amd.equaliser.PRESETS ("presence",
        "warm", "rumble", "telephone", "flat"), a dict of equaliser.design keywords (taps, bands, low_shelf, high_shelf, highpass_hz,
        lowpass_hz), an equaliser.Equaliser or (taps, delay): a linear-phase FIR designed at the model's native rate filters the vocoder's
        row on the device, in place (include/zvx.h, zvx_fir), behind the denoiser and before the mark, the loudness gain and the limiter
        -- the reported level and peak are those of the equalised signal.  How close a design comes to its target is
        ``Equaliser.deviation_db``; no claim of audible merit is made.
        report: False (the default: nothing is added to the call), or True: the finished waveform is measured as it is delivered -- at
        the output rate, behind every step above, on the device where its buffer is still there (include/zvx.h, zvx_loudness_stats and
        zvx_true_peak) -- and ``last_report`` holds the report.LoudnessReport (see ``loudness_report``).  The waveform is the same.
        pitch_report: False (the default: nothing is added to the call), True, or a dict of ``pitch_report`` keywords: the delivered
        waveform's F0 track is measured on the device (include/zvx.h, zvx_pitch) and ``last_pitch_report`` holds the pitch.PitchReport
        with its track -- what pitch_shift / pitch_range did to the audio, in Hz and semitones.  The waveform is the same.
        voice_report: False (the default: nothing is added to the call), True, or a dict of ``voice_report`` keywords (top_db,
        max_seconds): the delivered waveform is embedded again on the device and compared with ``spkemb`` (include/zvx.h, zvx_spkemb_wav
        and zvx_spk_score), and ``last_voice_report`` holds the voices.VoiceReport -- whose voice was delivered.  The waveform is the
        same.  No threshold is given: what similarity separates two speakers on a real checkpoint is not measured."""
        pkw = self._pitch_keywords(pitch_report)
        vkw = self._voice_keywords(voice_report)
        prosody = self._prosody(speed, pitch_shift, pitch_range, energy_shift, energy_range)
        dn = self._denoise(denoise)
        wm = self._watermark(watermark)
        fir = self._eq(eq)
        text = text.strip()
        t0 = time.time()
        phone_ids, punct_ids = self.text2phonemeids(text)
        if not phone_ids:
            if pkw is not None:
                self._last_pitch_report = None               # asked for, nothing to measure: not the previous call's
            if vkw is not None:
                self._last_voice_report = None
            return (np.array([[0.0]], dtype=np.float32), np.array([[0]], dtype=np.int32), 0,
                    np.array([[0.0]], dtype=np.float32))
        phoneme = np.array([phone_ids], dtype=np.int32)
        puncts = np.array([punct_ids], dtype=np.int32)
        duration = np.array([duration], dtype=np.int32) if duration is not None else None
        t1 = time.time()
        wav, length, _, mel = self._model.inference_ex({"phoneme": phoneme, "puncts": puncts, "duration": duration},
                                                       style_embed=spkemb, force_duration=duration is not None, prosody=prosody,
                                                       **self._post(loudness, peak_db, limiter, limiter_ms, dn),
                                                       **({"report": True} if report else {}), **({} if wm is None else {"watermark": wm}),
                                                       **({} if fir is None else {"eq": fir}))
        if self._verbose:
            print(f"tts timing stats: g2p={t1 - t0}s, synth={time.time() - t1}s")
        if pkw is not None:
            self.pitch_report(wav, **pkw)
        if vkw is not None:
            self.voice_report(wav, spkemb, **vkw)
        return wav, phoneme, length, mel

    def _post(self, loudness, peak_db, limiter, limiter_ms, denoise=None):
        """the inference_ex keywords of the denoise / loudness / limiter steps ({}: none of them, the plain path)"""
        lim = self._limiter(limiter, limiter_ms, peak_db)
        kw = {} if denoise is None else {"denoise": denoise}
        if loudness is not None:
            kw["loudness"] = self._loudness(loudness, None if lim else peak_db)      # under a limiter the gain has no peak ceiling
        if lim:
            kw["limiter"] = lim
        return kw

    def tts(self, text: str, spkemb, *, speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0, loudness=None,
            peak_db=-1.0, limiter=False, limiter_ms=5.0, denoise=None, report=False, pitch_report=False, watermark=None, voice_report=False,
            rhythm_from=None, rhythm_rate=None, eq=None):
        """-> (wav, phoneme, length): ``tts_ex`` without the mel.  rhythm_from: None (the default: nothing is added to the call), or a
        recording of the same text at rhythm_rate Hz (None: the model's rate) whose timing is copied: a first pass with predicted durations
        is aligned with the trimmed recording on the device (``fidelity_report``), align.durations_from turns the path into per-phoneme
        frame counts, and the second pass runs with them as forced durations -- it has exactly the mel frames of the trimmed recording.
        ``last_alignment`` holds the alignment of the first pass.  Refused together with speed != 1.0: both set durations.  Whether a
        copied rhythm sounds right on a real checkpoint is not measured."""
        duration = None
        if rhythm_from is not None:
            if speed != 1.0:
                raise ValueError(f"rhythm_from and speed={speed!r} both set durations: give one of them")
            duration = self._rhythm_durations(text, spkemb, rhythm_from, rhythm_rate, dict(pitch_shift=pitch_shift, pitch_range=pitch_range,
                                                                                          energy_shift=energy_shift, energy_range=energy_range))
        wav, phoneme, length, _ = self.tts_ex(text=text, spkemb=spkemb, duration=duration, speed=speed, pitch_shift=pitch_shift,
                                              pitch_range=pitch_range,
                                              energy_shift=energy_shift, energy_range=energy_range, loudness=loudness, peak_db=peak_db,
                                              limiter=limiter, limiter_ms=limiter_ms, denoise=denoise, report=report,
                                              pitch_report=pitch_report, watermark=watermark, voice_report=voice_report, eq=eq)
        return wav, phoneme, length

    def _rhythm_durations(self, text, spkemb, ref_wav, ref_rate, prosody):
        """the first pass of tts(rhythm_from=...): predicted durations, the alignment of its waveform with the recording, and the
        per-phoneme frame counts that follow from it (None for an empty text: nothing to align)"""
        from .align import durations_from
        wav, phoneme, length, _ = self.tts_ex(text=text, spkemb=spkemb, **prosody)
        if length == 0:
            self._last_alignment = None
            return None
        T = phoneme.shape[1]
        first = np.rint(self._model.ctx.fetch("duration", (1, T))[0]).astype(np.int64)
        al = self.fidelity_report(wav, ref_wav, sampling_rate=ref_rate, wav_rate=self.output_rate)
        if int(first.sum()) != al.frames_a:
            raise RuntimeError(f"the first pass has {int(first.sum())} frames by its durations and {al.frames_a} by its waveform")
        return [int(v) for v in durations_from(al, first)]

    def fidelity_report(self, wav, ref_wav, sampling_rate=None, *, wav_rate=None, n_cep=13):
        """How far a delivered waveform is from a recording of the same sentence: both at the model's rate (ref_wav at sampling_rate Hz and
        wav at wav_rate Hz are converted on the device where they are not), the recording trimmed as ``speaker_embed`` trims a reference
        clip (Context.trim_bounds, top_db 40), then the DTW path between the DCT cepstra of their log-mels and the distortion along it
        (include/zvx.h, zvx_align_wav) -> align.Alignment(cost, mcd_db, frames_a, frames_b, path, a2b), a = wav and b = the recording; also
        kept as ``last_alignment``.  mcd_db is the distortion of cepstra of the model's own log-mel with c0 left out: figures from SPTK /
        WORLD analysis in papers are not comparable with it, and no perceptual claim is made.  There is no default threshold:
        ``Alignment.meets(max_mcd_db)`` takes the caller's."""
        from .align import Alignment
        ctx = self._model.ctx
        rows = []
        for w, rate in ((wav, wav_rate), (ref_wav, sampling_rate)):
            w = _float_row(w)
            if rate is not None and int(rate) != int(self._sampling_rate):
                out, n = ctx.resample([w], int(rate), self._sampling_rate)
                w = np.ascontiguousarray(out[0, :int(n[0])])
            rows.append(w)
        begin, end = ctx.trim_bounds([rows[1]], top_db=40.0)
        rows[1] = np.ascontiguousarray(rows[1][int(begin[0]):int(end[0])])
        self._last_alignment = Alignment.from_result(ctx.align([rows[0]], [rows[1]], n_cep=n_cep))
        return self._last_alignment

    @property
    def last_alignment(self):
        """the align.Alignment of the last ``fidelity_report`` call or of the first pass of the last tts(rhythm_from=...) (None before)"""
        return getattr(self, "_last_alignment", None)

    def _eq(self, eq):
        """the eq keyword (None, a preset name, a dict of design keywords, an Equaliser or (taps, delay)) as Context.fir_device keywords
        at the model's native rate, or None; checked without a device"""
        if eq is None:
            return None
        from .equaliser import params
        return params(eq, self._sampling_rate)

    @staticmethod
    def _watermark(watermark):
        """the watermark keyword (None, an int key, or a dict with ``key``) as Context.watermark_device keywords, or None; checked without
        a device"""
        from .watermark import params
        return params(watermark)

    def detect_watermark(self, wav, key, sampling_rate=None, *, window_frames=None, threshold=None, **params):
        """Does this audio carry the mark of `key`?  wav: one waveform (float, or int16 PCM read as the samples it encodes) at
        sampling_rate Hz (None: the model's) -> watermark.WatermarkResult(score, offset, window, detected, threshold, windows), from
        the device (include/zvx.h, zvx_watermark_detect).  A waveform at another rate is converted to the model's first (zvx_resample)
        and hi_hz is lowered to what survived the lower of the two rates (0.45 of it).  params: the embedder's lo_hz, hi_hz,
        block_frames, band_bins, period_blocks where they were not the defaults; window_frames (default 256) and threshold (default
        watermark.THRESHOLD).  Short clips cut to the telephone band are not reliably detectable; nothing is claimed about lossy
        codecs, time-stretching or deliberate removal."""
        from . import watermark as wm
        rows, p = self._watermark_search_args(wav, sampling_rate, wm.params({"key": key, **params}), window_frames)
        return self._model.ctx.watermark_detect(rows, p.pop("key"), threshold=threshold, **p)[0]

    def _watermark_search_args(self, wav, sampling_rate, p, window_frames):
        """what detect_watermark and identify_watermark make of their arguments: the waveform as one float row at the model's rate, and the
        checked parameters p with hi_hz lowered where the rate was converted, depth_db dropped and window_frames set -> ([row], p)"""
        from . import watermark as wm
        wav = _float_row(wav)
        ctx = self._model.ctx
        native = ctx.get_int("sampling_rate")
        rate = native if sampling_rate is None else int(sampling_rate)
        if rate != native:
            out, out_len = ctx.resample([wav], rate, native)
            wav = out[0, :out_len[0]]
            p["hi_hz"] = min(p["hi_hz"], 0.45 * min(rate, native))
            wm.check(p)
        p.pop("depth_db")
        p["window_frames"] = wm.WINDOW_FRAMES if window_frames is None else int(window_frames)
        return [wav], p

    def identify_watermark(self, wav, keys, sampling_rate=None, *, window_frames=None, threshold=None, **params):
        """Which of the candidate `keys` marked this audio?  wav and sampling_rate as detect_watermark's (a waveform at another rate is
        converted first and hi_hz lowered likewise); keys: a sequence of int keys, e.g. watermark.derive_key(master, request_id) of every
        request in question -> watermark.IdentifyResult(best, key, score, offset, window, margin, detected, threshold, scores), from the
        device in one call for all keys (include/zvx.h, zvx_watermark_identify), each key's score the one detect_watermark gives.  The
        largest score among wrong keys grows with their number: the default threshold was measured over 256 wrong keys and nothing
        beyond, so with many more candidates judge by ``margin`` (best minus second best) as well.  What detect_watermark does not
        claim is not claimed here either."""
        from . import watermark as wm
        keys = list(keys)
        if not keys:
            raise ValueError("identify_watermark: keys is empty")
        p = None
        for k in keys:                                      # every key goes through the checks of the one-key call
            p = wm.params({"key": k, **params})
        rows, p = self._watermark_search_args(wav, sampling_rate, p, window_frames)
        p.pop("key")
        return self._model.ctx.watermark_identify(rows, keys, threshold=threshold, **p)[0]

    @staticmethod
    def _pitch_keywords(pitch_report):
        """the pitch_report keyword of tts / tts_ex / tts_long -> None (nothing is measured) or the checked ``pitch_report`` keywords"""
        from .pitch import check_keywords
        if pitch_report is None or pitch_report is False:
            return None
        if pitch_report is True:
            return {}
        if not isinstance(pitch_report, dict):
            raise ValueError(f"pitch_report must be False, True or a dict of pitch_report keywords, not {pitch_report!r}")
        return check_keywords(pitch_report)

    def pitch_report(self, wav, sampling_rate=None, **keywords):
        """What pitch was delivered: the F0 track of a waveform at sampling_rate Hz (None: ``output_rate``), measured on the device
        (include/zvx.h, zvx_pitch: YIN on a frame grid), and its statistics -> pitch.PitchReport: median, 5th / 95th percentile and mean
        of the voiced frames in Hz, their span in semitones, the voiced fraction; its ``f0`` / ``aper`` hold the track (Hz per frame,
        0 = unvoiced; pitch.per_phoneme turns it into per-phoneme values).  keywords: fmin (60), fmax (500), threshold (0.15), gate_db
        (-60), window (two periods of fmin), hop (the model's hop at the model's rate: a frame is then a mel frame; otherwise 10 ms).
        int16 PCM is read as the samples it encodes (/ 32760).  Also kept as ``last_pitch_report``."""
        from .pitch import PitchReport, check_keywords
        keywords = check_keywords(keywords)
        rate = self.output_rate if sampling_rate is None else int(sampling_rate)
        stats = self._model.ctx.pitch([_float_row(wav)], rate=rate, **keywords)
        self._last_pitch_report = PitchReport.from_stats(stats)
        return self._last_pitch_report

    VOICE_KEYWORDS = ("top_db", "max_seconds")

    @classmethod
    def _voice_keywords(cls, voice_report):
        """the voice_report keyword of tts / tts_ex / tts_long -> None (nothing is measured) or the checked ``voice_report`` keywords"""
        if voice_report is None or voice_report is False:
            return None
        if voice_report is True:
            return {}
        if not isinstance(voice_report, dict):
            raise ValueError(f"voice_report must be False, True or a dict of voice_report keywords, not {voice_report!r}")
        unknown = sorted(set(voice_report) - set(cls.VOICE_KEYWORDS))
        if unknown:
            raise ValueError(f"voice_report: unknown keyword {unknown[0]!r} (one of {', '.join(cls.VOICE_KEYWORDS)})")
        return dict(voice_report)

    def voice_report(self, wav, spkemb, sampling_rate=None, *, top_db=40.0, max_seconds=30.0):
        """Whose voice was delivered: the cosine similarity ("SIM") between the speaker embedding of a waveform at sampling_rate Hz (None:
        ``output_rate``) and ``spkemb`` ([hidden], [1, hidden] or [1, 1, hidden]), both on the device: the waveform is enrolled as a
        reference clip is (include/zvx.h, zvx_spkemb_wav: converted to the model's rate, trimmed at top_db, cut to max_seconds; None: no
        cut) and its embedding, which stays on the device, is scored against ``spkemb`` by zvx_spk_score
        -> voices.VoiceReport(similarity, frames, begin, end); also kept as ``last_voice_report``.  int16 PCM is read as the samples it
        encodes (/ 32760).  There is NO default threshold: ``VoiceReport.meets(min_similarity)`` takes the caller's.  What similarity
        separates two speakers depends on the checkpoint's speaker encoder and is not measured here, and no perceptual meaning is claimed
        for the figure."""
        from .voices import VoiceReport, rows_2d
        ctx = self._model.ctx
        e = rows_2d(spkemb, ctx.hidden, "spkemb")
        if e.shape[0] != 1:
            raise ValueError(f"voice_report: one embedding, not {e.shape[0]}")
        row = _float_row(wav)
        rate = self.output_rate if sampling_rate is None else int(sampling_rate)
        cut = 0 if max_seconds is None else max(1, int(round(float(max_seconds) * self._sampling_rate)))
        n = len(row)
        row_bytes, emb_bytes = (max(n, 1) * 4 + 255) & ~255, (ctx.hidden * 4 + 255) & ~255
        buf = ctx.dev_alloc(row_bytes + 2 * emb_bytes)       # the row, its embedding, the embedding asked for
        try:
            q, lib = buf + row_bytes, buf + row_bytes + emb_bytes
            if n:
                ctx.dev_from_host(buf, row)
            ctx.dev_from_host(lib, e)
            begin, end, frames = ctx.spkemb_wav_device(buf, [n], max(n, 1), q, rate, top_db=float(top_db), max_samples=cut, no_sync=True)
            score = ctx.spk_score_device(q, 1, lib, 1)
        finally:
            ctx.dev_free(buf)
        self._last_voice_report = VoiceReport(similarity=float(score[0, 0]), frames=int(frames[0]), begin=int(begin[0]), end=int(end[0]))
        return self._last_voice_report

    @property
    def last_voice_report(self):
        """the voices.VoiceReport of the last tts / tts_ex / tts_long call with voice_report or ``voice_report`` call (None before)"""
        return getattr(self, "_last_voice_report", None)

    @property
    def last_pitch_report(self):
        """the pitch.PitchReport of the last tts / tts_ex / tts_long call with pitch_report or ``pitch_report`` call (None before)"""
        return getattr(self, "_last_pitch_report", None)

    def loudness_report(self, wav, sampling_rate=None):
        """What was delivered: the programme loudness report of a waveform at sampling_rate Hz (None: ``output_rate``), measured on the
        device -- integrated loudness, loudness range (EBU Tech 3342) with its bounds, maximum momentary and short-term loudness, sample
        peak (include/zvx.h, zvx_loudness_stats) and the 4x oversampled true peak (zvx_true_peak) -> report.LoudnessReport, whose
        ``meets(target, tolerance, max_true_peak_db, max_lra)`` checks it against a delivery specification.  int16 PCM is read as the
        samples it encodes (/ 32760).  Also kept as ``last_report``."""
        return self._model.loudness_report(_float_row(wav), sampling_rate)

    @property
    def last_report(self):
        """the report.LoudnessReport of the last tts / tts_ex / tts_long call with report=True or loudness_report call (None before)"""
        return self._model.last_report

    @property
    def denoise_bias(self):
        """[fft_size / 2 + 1] float32: the bias spectrum ``denoise=`` subtracts (include/zvx.h, zvx_denoise_bias): what the vocoder emits
        for silence, computed once per context on first use.  It depends on the vocoder's arithmetic: call ``refresh_denoise_bias()``
        after a vocoder precision switch (set_int "voc_f16" / "voc_f16_stages")."""
        return self._model.denoise_bias

    def refresh_denoise_bias(self):
        """recompute ``denoise_bias`` under the context's current switches -> the new bias"""
        return self._model.refresh_denoise_bias()

    @property
    def last_limit(self):
        """dict(peak_in, min_gain) of the last tts / tts_ex call that ran the limiter (None before the first)"""
        return self._model.last_limit

    @property
    def last_loudness(self):
        """dict(lufs, peak, gain) of the last tts / tts_ex call that asked for a loudness (None before the first)"""
        return self._model.last_loudness

    def tts_stream(self, text: str, spkemb, chunk_frames=64, chunks_per_call=1, *, speed=1.0, pitch_shift=0.0, pitch_range=1.0,
                   energy_shift=0.0, energy_range=1.0, loudness=None, limiter=False, peak_db=None, limiter_ms=5.0, denoise=None,
                   denoise_strength=None, resident=False, level_lufs=None, level_window_ms=3000.0, level_lookahead_ms=100.0, watermark=None):
        """Streaming variant of ``tts`` (not in the reference): encoder + mel decoder run once, the vocoder
        runs chunk by chunk (16-frame halo), yielding float32 waveform pieces that concatenate to ``tts(text, spkemb)[0]``
        up to the reference's `_min_mel_len` zero-padding of short utterances.  A stream cannot be loudness-normalised: the gain is not
        known before the last chunk, so ``loudness`` other than None raises ValueError (use tts / tts_long).
        peak_db: None (the default: nothing is limited), or the ceiling in dBFS the stream is held under by the windowed look-ahead
        limiter (include/zvx.h, zvx_limit_ex; zerovox_amd.limiter), its gain smoothed over limiter_ms on either side and driven by the
        4x oversampled envelope.  The pieces then concatenate bit for bit to zvx_limit of the unlimited stream's own concatenation
        -- not to ``tts(limiter=True)``, which pads a short utterance first -- and run limiter.reach(W, 4) samples behind the vocoder
        (2 W + 11: 231 samples for 5 ms at 22.05 kHz); under an ``output_rate`` the conversion follows the limiter, as in ``tts``.
        That delay is why the ceiling is asked for by name: ``limiter=True`` still raises ValueError and points here.
        denoise_strength: None (the default: nothing of the denoiser is created), or the strength of the vocoder-bias denoiser (see
        tts_ex) the stream is put through window by window (include/zvx.h, zvx_denoise_ex; zerovox_amd.denoiser), directly behind the
        vocoder.  The pieces then concatenate bit for bit to zvx_denoise of the undenoised stream's own concatenation -- not to
        ``tts(denoise=...)``, which pads a short utterance first -- and run n_fft - 1 samples behind the vocoder (1023: 46 ms at 22.05
        kHz).  With ``peak_db`` as well the stream is limit(denoise(stream)) and runs n_fft - 1 + limiter.reach(W, 4) samples behind;
        an ``output_rate`` converts last.  That delay is why the strength is asked for by this name: ``denoise=...``, the
        whole-utterance keyword of tts and tts_long, still raises ValueError and points here.
        level_lufs: None (the default: the level the model gives), or the short-term loudness in LUFS the stream is steered towards by
        the windowed leveler (include/zvx.h, zvx_level_ex; zerovox_amd.leveler): a gain curve from the gated loudness of the last
        level_window_ms, looking level_lookahead_ms ahead, at most +20 dB.  It is an AGC, not the R128 normalisation of ``loudness=``.
        The pieces concatenate bit for bit to zvx_level of the stream that reaches the stage; the chain is denoise, level, limit,
        conversion, and the levelled stream runs (a + 1) h - 1 samples behind the stage's input (4409: 200 ms at 22.05 kHz with the
        defaults).  With ``resident=True`` this method still raises ValueError; sessions with a level stage are reached through
        ``tts_stream_sessions`` and ``ZeroVox.vocode_stream(resident=True, level=...)``.
        watermark: None (the default: nothing changes), an int key, or a dict with ``key`` (see tts_ex): the stream is marked window by
        window (include/zvx.h, zvx_watermark_ex; zerovox_amd.watermark).  The pieces concatenate bit for bit to zvx_watermark of the
        stream that reaches the stage; the chain is denoise, level, watermark, limit, conversion, and the marked stream runs n_fft - 1
        samples more behind.  With ``resident=True`` this method still raises ValueError; sessions with a watermark stage are reached
        through ``tts_stream_sessions`` and ``ZeroVox.vocode_stream(resident=True, watermark=...)``.
        resident: False (the default: the stream is planned on the host), or True: a stream session of the library runs it (include/zvx.h,
        zvx_stream_open; ZeroVox.vocode_stream(resident=True)) -- the decoder's mel never leaves the device and every piece costs one
        wait.  The concatenation is the same to the bit; the pieces may be cut elsewhere."""
        prosody, lim, den = self._stream_keywords(speed, pitch_shift, pitch_range, energy_shift, energy_range, loudness, limiter, peak_db,
                                                  limiter_ms, denoise, denoise_strength)
        lvl = self._level(level_lufs, level_window_ms, level_lookahead_ms)
        if lvl is not None and resident:
            raise ValueError("tts_stream: stream sessions have no level stage yet: level_lufs needs resident=False")
        wm = self._watermark(watermark)
        if wm is not None and resident:
            raise ValueError("tts_stream: stream sessions have no watermark stage yet: watermark needs resident=False")
        return self._tts_stream(text, spkemb, chunk_frames, chunks_per_call, prosody, lim, den, resident, lvl, wm)

    @staticmethod
    def _level(level_lufs, window_ms, lookahead_ms):
        """the level keywords as Context.level_window keywords, or None (nothing is levelled); checked without a device"""
        if level_lufs is None:
            return None
        from .leveler import MAX_UNITS, lookahead_units, window_units
        t, w, a = float(level_lufs), float(window_ms), float(lookahead_ms)
        if not np.isfinite(t) or not -70.0 <= t <= 0.0:
            raise ValueError(f"level_lufs must be None or lie in [-70, 0] LUFS, not {level_lufs!r}")
        if not (np.isfinite(w) and w >= 0 and np.isfinite(a) and a >= 0):
            raise ValueError(f"level_window_ms / level_lookahead_ms must be finite and not negative, not {window_ms!r} / {lookahead_ms!r}")
        if window_units(w) > MAX_UNITS or lookahead_units(a) > window_units(w):
            raise ValueError(f"level_window_ms {window_ms!r} / level_lookahead_ms {lookahead_ms!r}: at most {MAX_UNITS} units of 100 ms, and the "
                             "look-ahead no longer than the window")
        return dict(target=t, window_ms=w, lookahead_ms=a)

    def _stream_keywords(self, speed, pitch_shift, pitch_range, energy_shift, energy_range, loudness, limiter, peak_db, limiter_ms, denoise,
                         denoise_strength):
        """the checks of tts_stream's keywords -> (prosody, limiter keywords or None, denoiser keywords or None)"""
        if denoise is not None:
            raise ValueError("tts_stream does not take denoise=: pass denoise_strength=<strength> (the stream is then denoised window by window, "
                             "n_fft - 1 samples behind the vocoder); denoise= is the whole-utterance keyword of tts and tts_long")
        den = self._denoise(denoise_strength)
        if loudness is not None:
            raise ValueError("tts_stream cannot normalise loudness: the gain is unknown until the last chunk (use tts or tts_long; "
                             "level_lufs=<LUFS> levels a stream by its short-term loudness instead)")
        if limiter:
            raise ValueError("tts_stream takes its ceiling by name: pass peak_db=<dBFS> (the stream is then limited window by window, "
                             "2 W + 11 samples behind the vocoder); limiter=True is the whole-utterance switch of tts and tts_long")
        lim = None
        if peak_db is not None:
            if not np.isfinite(peak_db):
                raise ValueError(f"tts_stream: peak_db must be finite, not {peak_db}")
            lim = self._limiter(True, limiter_ms, peak_db)
        return self._prosody(speed, pitch_shift, pitch_range, energy_shift, energy_range), lim, den

    def tts_stream_many(self, texts, spkembs, chunk_frames=64, chunks_per_call=1, *, speed=1.0, pitch_shift=0.0, pitch_range=1.0,
                        energy_shift=0.0, energy_range=1.0, loudness=None, limiter=False, peak_db=None, limiter_ms=5.0, denoise=None,
                        denoise_strength=None, max_frames=2048, level_lufs=None, level_window_ms=3000.0, level_lookahead_ms=100.0, watermark=None):
        """Many texts streamed together -> yields (index, piece), non-empty float32 pieces only; the stream keywords are those of
        ``tts_stream`` and apply to every text.  spkembs: one embedding per text ([B, hidden]), or one for all.  The front end runs as ONE
        batch (``synthesize_batch(want_mel=True)``, at most max_frames mel frames per text), one stream session is opened on every mel,
        and each round steps all of them with one zvx_stream_next_many (``ZeroVox.vocode_stream_many``): the chunks of all texts ride
        through the vocoder as one batch.  The pieces of index i concatenate bit for bit to ``vocode_stream(mel_i, ..., resident=True)``
        on the mel the batch made for text i (``last_stream_mels[i]``).  A text without phonemes yields nothing.
        ``level_lufs`` and ``watermark`` are still refused here (ValueError); ``tts_stream_sessions`` is this method with both stages."""
        if level_lufs is not None or watermark is not None:
            self._stream_keywords(speed, pitch_shift, pitch_range, energy_shift, energy_range, loudness, limiter, peak_db, limiter_ms, denoise,
                                  denoise_strength)            # (the other keywords' errors come first, as they always did)
            if level_lufs is not None:
                raise ValueError("tts_stream_many: stream sessions have no level stage yet: level_lufs is tts_stream's (resident=False)")
            raise ValueError("tts_stream_many: stream sessions have no watermark stage yet: watermark is tts_stream's (resident=False)")
        return self.tts_stream_sessions(texts, spkembs, chunk_frames=chunk_frames, chunks_per_call=chunks_per_call, speed=speed,
                                        pitch_shift=pitch_shift, pitch_range=pitch_range, energy_shift=energy_shift, energy_range=energy_range,
                                        loudness=loudness, limiter=limiter, peak_db=peak_db, limiter_ms=limiter_ms, denoise=denoise,
                                        denoise_strength=denoise_strength, max_frames=max_frames)

    def tts_stream_sessions(self, texts, spkembs, *, chunk_frames=64, chunks_per_call=1, speed=1.0, pitch_shift=0.0, pitch_range=1.0,
                            energy_shift=0.0, energy_range=1.0, loudness=None, limiter=False, peak_db=None, limiter_ms=5.0, denoise=None,
                            denoise_strength=None, max_frames=2048, level_lufs=None, level_window_ms=3000.0, level_lookahead_ms=100.0,
                            watermark=None):
        """``tts_stream_many`` with every stage of a stream session (include/zvx.h, zvx_stream_open_ex): what it does and yields --
        (index, piece), non-empty float32 pieces only, one session per text, one zvx_stream_next_many per round -- and besides
        level_lufs / level_window_ms / level_lookahead_ms: the leveler of ``tts_stream``, for every text;
        watermark: None, one key or dict for every text (see tts_ex), or a sequence of them, one per text (None entries: that text
        goes out unmarked).  Sessions that differ in their key alone are marked by one launch group per round.
        The chain is denoise, level, watermark, limit, conversion; the pieces of index i concatenate bit for bit to
        ``vocode_stream(mel_i, ..., level=, watermark=)``, host-planned or resident, on ``last_stream_mels[i]``.  Every argument is
        checked before the model is touched."""
        prosody, lim, den = self._stream_keywords(speed, pitch_shift, pitch_range, energy_shift, energy_range, loudness, limiter, peak_db,
                                                  limiter_ms, denoise, denoise_strength)
        lvl = self._level(level_lufs, level_window_ms, level_lookahead_ms)
        texts = list(texts)
        if watermark is None or isinstance(watermark, (int, dict)):
            marks = [self._watermark(watermark)] * len(texts)
        else:
            marks = [self._watermark(w) for w in watermark]
            if len(marks) != len(texts):
                raise ValueError(f"tts_stream_sessions: {len(marks)} watermarks for {len(texts)} texts")
        return self._tts_stream_many(texts, spkembs, chunk_frames, chunks_per_call, prosody, lim, den, int(max_frames), lvl, marks)

    def _tts_stream_many(self, texts, spkembs, chunk_frames, chunks_per_call, prosody, limiter, denoise, max_frames, level=None, marks=None):
        ids = [self.text2phonemeids(t.strip()) for t in texts]
        keep = [i for i, (ph, _) in enumerate(ids) if ph]
        self.last_stream_mels = {}
        if not keep:
            return
        spk = np.asarray(spkembs, np.float32)
        spk = np.repeat(spk.reshape(1, -1), len(texts), axis=0) if spk.size == spk.shape[-1] else spk.reshape(len(texts), -1)
        B, Tmax = len(keep), max(len(ids[i][0]) for i in keep)
        phoneme, puncts = np.zeros((B, Tmax), np.int32), np.zeros((B, Tmax), np.int32)
        T = np.array([len(ids[i][0]) for i in keep], np.int32)
        for b, i in enumerate(keep):
            phoneme[b, :T[b]], puncts[b, :T[b]] = ids[i]
        if denoise is not None:
            self._model.denoise_bias                                 # (first use runs the vocoder: before this call's front end)
        r = self._model.synthesize_batch(phoneme, puncts, T, spk[keep], want_mel=True, Lmax_cap=max_frames, prosody=prosody)
        ml = [int(v) for v in r["mel_len"]]
        if min(ml) < 2:
            raise ValueError(f"predicted mel length {min(ml)} is too short to synthesise")
        mels = [np.ascontiguousarray(r["mel"][b, :ml[b]]) for b in range(B)]
        self.last_stream_mels = {i: mels[b] for b, i in enumerate(keep)}
        marks = [marks[i] for i in keep] if marks is not None and any(m is not None for m in marks) else None
        for b, piece in self._model.vocode_stream_sessions(mels, chunk_frames=chunk_frames, chunks_per_call=chunks_per_call, limiter=limiter,
                                                           denoise=denoise, level=level, watermark=marks):
            yield keep[b], piece

    def _tts_stream(self, text, spkemb, chunk_frames, chunks_per_call, prosody, limiter=None, denoise=None, resident=False, level=None,
                    watermark=None):
        text = text.strip()
        phone_ids, punct_ids = self.text2phonemeids(text)
        if not phone_ids:
            return
        phoneme, puncts = np.array([phone_ids], np.int32), np.array([punct_ids], np.int32)
        ctx = self._model.ctx
        if denoise is not None:
            self._model.denoise_bias                                 # (first use runs the vocoder: before this call's encoder)
        mel_len, _, _, _ = ctx.encode(phoneme, puncts, np.array([len(phone_ids)], np.int32), np.asarray(spkemb, np.float32).reshape(1, -1),
                                   prosody=prosody)
        ml = int(mel_len[0])
        if ml < 2:
            raise ValueError(f"predicted mel length {ml} is too short to synthesise")
        if resident:                                                 # no host mel: the session takes the context's with a device copy
            ctx._chk(ctx._lib.zvx_decode(ctx._h, None, 0, 0))
            yield from self._model.vocode_stream(None, chunk_frames=chunk_frames, chunks_per_call=chunks_per_call, limiter=limiter,
                                                 denoise=denoise, resident=True)
            return
        mel = ctx.decode(1, ml)[0, :ml]
        yield from self._model.vocode_stream(mel, chunk_frames=chunk_frames, chunks_per_call=chunks_per_call, limiter=limiter,
                                             denoise=denoise, level=level, **({} if watermark is None else {"watermark": watermark}))

    def tts_long(self, text: str, spkemb, *, pauses=None, trim_db=40.0, keep_ms=20, fade_ms=5, max_batch=32, max_frames=2048, pcm16=False,
                 durations=None, max_chars=200, speed=1.0, pitch_shift=0.0, pitch_range=1.0, energy_shift=0.0, energy_range=1.0,
                 loudness=None, peak_db=-1.0, loudness_mode="paragraph", limiter=False, limiter_ms=5.0, denoise=None, report=False,
                 pitch_report=False, watermark=None, voice_report=False, eq=None):
        """A paragraph -> (wav, segments): one waveform with every sentence in text order (not in the reference).  The text is split by
        longform.split_sentences; the sentences run in batches of at most max_batch, each batch ONE queued synthesize call into
        consecutive rows of one device buffer (every row is the fresh-model ``tts`` of its sentence; a sentence of more than max_frames
        mel frames is an error); then ONE zvx_join trims each row's silence (trim_db, as librosa.effects.trim's top_db; <= 0: off;
        keep_ms kept around the cut, fade_ms of linear fade at both cuts) and writes the rows with the pauses between them on the
        device; under an ``output_rate`` the joined row is converted by one zvx_resample.  pauses: ms by closing class, default
        longform.PAUSES_MS ('.' 350, ';' 250, ',' 120, ' ' 0; nothing behind the last sentence).  The prosody keywords apply to every
        sentence; durations: None or one list of per-phoneme frame counts per sentence, forced as tts_ex(duration=...) does.
        wav: float32, or int16 with pcm16.  segments: one dict per sentence -- text, start / samples (its place in wav, in output
        samples), mel_len, trim (samples cut in front, at the model's rate) and durations (the per-phoneme frame counts as
        synthesised): what subtitles or lip-sync need.  Empty or phone-less text: the reference's sentinel waveform and [].
        loudness: None, or the integrated loudness in LUFS the paragraph is brought to: ONE zvx_normalize over all rows of the device
        buffer, in place, between the synthesis calls and the join.  loudness_mode "paragraph": the sentences are measured as one
        programme and share one gain (their relative levels stay); "sentence": every sentence gets its own gain.  The gain is at most
        +20 dB and leaves no sample above peak_db dBFS (None: no ceiling).  The measurement is at the model's rate, untrimmed, before any
        output-rate conversion: the ceiling applies BEFORE resampling, whose band-limited interpolation may overshoot it -- pcm16
        still clamps what does.  Every segment dict then also carries lufs (the sentence's own measured loudness, -inf where it is
        shorter than 0.4 s or silent) and gain (the linear factor applied).
        limiter: with True ONE zvx_limit over all rows, in place, between the normalise and the join, at peak_db dBFS with a 4x
        oversampled envelope and limiter_ms of smoothing on either side; the loudness gain then has no peak ceiling (see tts_ex).
        Every segment dict then also carries min_gain (the limiter's smallest gain in that sentence; 1.0: untouched).
        denoise: None, or the strength of the vocoder-bias denoiser (see tts_ex): ONE zvx_denoise over all rows of the device buffer, in
        place, behind the synthesis calls and before the normalise.  The segments' layout is that of the same call without it whenever
        trim_db <= 0 (the trim decides on the denoised rows).
        watermark: None (the default: nothing changes), an int key, or a dict with ``key`` (see tts_ex): ONE zvx_watermark over all
        sentence rows of the device buffer, in place, between the denoise and the normalise; every sentence's pattern starts at its own
        first frame, so ``detect_watermark`` finds each sentence at its own offset through its windows.
        eq: None (the default: nothing changes), or the equaliser of tts_ex: ONE zvx_fir over all sentence rows of the device buffer, in
        place, between the denoise and the watermark; every sentence is filtered as a signal of its own (zeros beyond its ends).
        report: False (the default: nothing is added to the call), or True: the joined waveform is measured as it is delivered, at the
        output rate, and ``last_report`` holds its report.LoudnessReport (see ``loudness_report``).  A float waveform at the model's
        rate is joined into a device buffer, measured there and copied to the host afterwards -- the same bits as without the report --;
        a converted or int16 waveform is measured as it arrives.
        pitch_report: False (the default: nothing is added to the call), True, or a dict of ``pitch_report`` keywords: the joined
        waveform's F0 track is measured as delivered and ``last_pitch_report`` holds its pitch.PitchReport (see tts_ex).  The
        measurement runs behind the synthesis, and zvx_pitch takes at most 65536 frames per row: a paragraph whose joined waveform is
        longer than that at the hop (about 760 s at the model's rate and hop 256) must pass a larger one, ``pitch_report=dict(hop=512)``.
        Where it is not, the ZvxError (ZVX_E_UNSUPPORTED) is raised with the finished ``(wav, segments)`` in its ``result`` attribute,
        so that the waveform is not lost, and ``last_pitch_report`` is None.
        voice_report: False (the default: nothing is added to the call), True, or a dict of ``voice_report`` keywords: the joined waveform
        is embedded again on the device (its first max_seconds, 30 by default) and compared with ``spkemb``; ``last_voice_report``
        holds the voices.VoiceReport (see tts_ex).  No threshold is given."""
        from ._lib import ZvxError
        from .longform import synthesize_long
        pkw = self._pitch_keywords(pitch_report)
        vkw = self._voice_keywords(voice_report)
        wav, segments = synthesize_long(self, text, spkemb, pauses=pauses, trim_db=trim_db, keep_ms=keep_ms, fade_ms=fade_ms, max_batch=max_batch,
                               max_frames=max_frames, pcm16=pcm16, durations=durations, max_chars=max_chars,
                               prosody=self._prosody(speed, pitch_shift, pitch_range, energy_shift, energy_range),
                               loudness=loudness, peak_db=peak_db, loudness_mode=loudness_mode, limiter=limiter, limiter_ms=limiter_ms,
                               denoise=self._denoise(denoise), **({"report": True} if report else {}),
                               **({} if watermark is None else {"watermark": self._watermark(watermark)}),
                               **({} if eq is None else {"eq": self._eq(eq)}))
        if pkw is not None:
            self._last_pitch_report = None
        if pkw is not None and segments:
            try:
                self.pitch_report(wav, **pkw)
            except ZvxError as e:
                e.result = (wav, segments)
                raise
        if vkw is not None:
            self._last_voice_report = None
        if vkw is not None and segments:
            self.voice_report(wav, spkemb, **vkw)
        return wav, segments

    @property
    def output_rate(self):
        """sampling rate of the waveforms tts / tts_ex / tts_stream hand back (default: the model's); set it to have them converted
        on the device.  The returned ``length`` stays in mel frames; the waveform holds resampled_len(length * hop) samples."""
        return self._model.output_rate

    @output_rate.setter
    def output_rate(self, hz):
        self._model.output_rate = hz

    @property
    def normalizer(self):
        return self._normalizer

    @property
    def language(self):
        return self._normalizer.language

    @language.setter
    def language(self, value):
        if value != self._normalizer.language:
            self._normalizer = ZeroVoxNormalizer(lang=value)

    @property
    def meldec_model(self):
        return self._meldec_model

    @property
    def model(self):
        return self._model

    @classmethod
    def load_model(cls, modelpath, meldec_model, infer_device="cuda", num_threads=-1, verbose=False, precision="bf16"):
        """-> (modelcfg, synth)   (synthesize.py:285-328).  ``modelpath``: directory with modelcfg.yaml +
        weights.npz, or ``synthetic:<decoder_kind>[:seed]``; ``meldec_model``: directory with config.json +
        generator.npz, or ``synthetic:<v1|v2|v3|tiny>[:seed]``."""
        modelcfg, sd = load_tts_weights(modelpath)
        hcfg, hsd = load_meldec_weights(meldec_model, tts_modelpath=modelpath)
        model = ZeroVox(modelcfg, sd, hcfg, hsd, infer_device=infer_device, precision=precision, verbose=verbose)
        a = modelcfg["audio"]
        synth = cls(language=modelcfg["lang"][0], syms=Symbols(modelcfg["model"]["phones"], modelcfg["model"]["puncts"]),
                    model=model, meldec_model=str(meldec_model), hop_length=a["hop_size"], win_length=a["win_length"],
                    mel_fmin=a["fmin"], mel_fmax=a["fmax"], sampling_rate=a["sampling_rate"],
                    n_mel_channels=a["num_mels"], fft_size=a["fft_size"], infer_device=infer_device,
                    num_threads=num_threads, verbose=verbose)
        return modelcfg, synth


def write_wav_to_file(wav, length, filename, sample_rate, hop_length, samples=None):
    """demo.py:29-35: int16 PCM, x32760, cut to length*hop -- or to `samples` where the waveform is not at the model's rate
    (ZeroVoxTTS.output_rate: length stays in mel frames, the rows are resampled_len(length*hop) long and may overshoot [-1, 1])."""
    if samples is not None:
        pcm = np.clip(np.asarray(wav, np.float32) * np.float32(32760), -32768, 32767).astype("int16")[: int(samples)]
    else:
        pcm = (np.asarray(wav) * 32760).astype("int16")[: length * hop_length]
    with wave.open(str(filename), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())
