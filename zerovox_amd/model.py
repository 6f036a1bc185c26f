"""Model-level host mirror of the reference's ``ZeroVox`` inference API (model.py:308-351).

``ZeroVox.inference_ex`` / ``inference`` keep the reference's argument meaning and return order; the
computation happens in libzvx on an MI355X.  There is no CPU path: constructing the model without the
HIP library or a GPU raises.
"""
from __future__ import annotations

import json
import os

import numpy as np
import yaml

from . import _lib, config as zcfg, pack, weights as zw
from .denoiser import DenoisePlanner
from .leveler import LevelPlanner, reach as level_reach
from .limiter import LimitPlanner, window_samples
from .report import LoudnessReport
from .watermark import WatermarkPlanner
from .resample import stream_resample
from .stream import stream_windows

DEFAULT_MELDEC_MODEL_NAME = "zerovox-hifigan-vctk-v2-en-1"      # model.py:84


def parse_device(infer_device) -> int:
    """'cuda' | 'cuda:N' | 'hip:N' | int -> HIP device index.  'cpu' is refused: the product path is GPU-only."""
    if isinstance(infer_device, int):
        return infer_device
    s = str(infer_device)
    if s == "cpu":
        raise _lib.ZvxError(_lib.ZVX_E_UNSUPPORTED, "zerovox_amd has no CPU path; use infer_device='cuda[:N]'")
    if ":" in s:
        return int(s.split(":")[1])
    return 0


def load_tts_weights(modelpath):
    """-> (modelcfg, state_dict).  ``synthetic:<styletts|fastspeech2>[:seed]``, or a directory holding ``modelcfg.yaml``
    (synthesize.py:310-326) and either ``weights.npz`` (tools/convert_checkpoint.py output, torch-free) or the reference's
    own ``checkpoints/*.ckpt`` / ``checkpoint.pkl`` (synthesize.py:295-304; read with torch through zerovox_amd.convert)."""
    spec = str(modelpath)
    if spec.startswith("synthetic:"):
        parts = spec.split(":")
        cfg = zcfg.medium_modelcfg(parts[1])
        return cfg, zw.tts_state_dict(cfg, int(parts[2]) if len(parts) > 2 else 0)
    with open(os.path.join(spec, "modelcfg.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader)
    if os.path.exists(os.path.join(spec, "weights.npz")):
        return cfg, dict(np.load(os.path.join(spec, "weights.npz")))
    from .convert import read_tts_checkpoint          # a reference model directory as downloaded: needs torch to unpickle
    sd, _ = read_tts_checkpoint(spec)
    return cfg, sd


def load_meldec_weights(modelspec, tts_modelpath=None):
    """-> (hifigan_cfg, state_dict).  ``synthetic:<v1|v2|v3|tiny|tiny2>[:seed]`` or a directory with
    ``config.json`` (model.py:90-105) + ``generator.npz`` (converted) or the reference's ``generator.ckpt``.

    A vocoder BAKED INTO the TTS checkpoint (``_meldec.*`` keys, utils/edit_meldec_in_checkpoint.py:77-90; split off
    by tools/convert_checkpoint.py into ``<tts_modelpath>/generator.npz``) overrides the external weights, exactly as
    ``ZeroVox.load_from_checkpoint(strict=False)`` loads those keys on top of ``get_meldec()`` (synthesize.py:78-91);
    the external model then only supplies ``config.json``.  A baked-in state dict whose keys/shapes do not fit that
    config is an error, not a silent fallback."""
    spec = str(modelspec)
    if spec.startswith("synthetic:"):
        parts = spec.split(":")
        h = zcfg.hifigan_config(parts[1])
        hsd = zw.hifigan_state_dict(h, int(parts[2]) if len(parts) > 2 else 0)
    else:
        with open(os.path.join(spec, "config.json")) as f:
            h = json.load(f)
        if os.path.exists(os.path.join(spec, "generator.npz")):
            hsd = dict(np.load(os.path.join(spec, "generator.npz")))
        else:                                           # the reference's own layout: generator.ckpt next to config.json (model.py:90-111)
            from .convert import read_generator_checkpoint
            hsd = read_generator_checkpoint(os.path.join(spec, "generator.ckpt"))
    bsd = None
    if tts_modelpath is not None and not str(tts_modelpath).startswith("synthetic:"):
        baked = os.path.join(str(tts_modelpath), "generator.npz")
        if os.path.exists(baked):
            bsd = dict(np.load(baked))
        elif not os.path.exists(os.path.join(str(tts_modelpath), "weights.npz")):
            from .convert import find_tts_checkpoint, read_tts_checkpoint
            if find_tts_checkpoint(str(tts_modelpath)):
                bsd = read_tts_checkpoint(str(tts_modelpath))[1] or None
                baked = find_tts_checkpoint(str(tts_modelpath))
    if bsd:
        # The reference bakes the vocoder in AFTER remove_weight_norm() (model.py:115, 247; edit_meldec_in_checkpoint.py:77-84
        # copies meldec.state_dict()): a Lightning / edited checkpoint holds plain `.weight` tensors, generator.ckpt holds
        # weight_g / weight_v pairs.  Compare the two in the folded domain (pack._wn accepts either form).
        fb, fh = zw.folded(bsd), zw.folded(hsd)
        bad = sorted(k for k in set(fb) | set(fh) if k not in fb or k not in fh or fb[k].shape != fh[k].shape)
        if bad:
            raise ValueError(f"{baked}: baked-in vocoder does not match {spec}/config.json (first mismatching keys: {bad[:4]})")
        hsd = bsd
    return h, hsd


class ZeroVox:
    """GPU-resident model: phoneme encoder, speaker encoder, mel decoder and HiFi-GAN (model.py:206-249)."""

    def __init__(self, modelcfg, tts_sd, meldec_cfg, meldec_sd, infer_device="cuda", precision="bf16", verbose=False):
        self._modelcfg = modelcfg
        self._hop_length = modelcfg["audio"]["hop_size"]
        self._verbose = verbose
        manifest, blob = pack.pack_model(modelcfg, tts_sd, meldec_cfg, meldec_sd, precision)
        self._packed, self._device = (manifest, blob), parse_device(infer_device)
        self._ctx = _lib.Context(manifest, blob, self._device)
        self._more_ctx = []                             # further contexts of the same model (synthesize_batches; release_contexts() frees them)
        self._streaming = False                         # a synthesize_batches generator is live: self._ctx belongs to its worker threads
        self._min_mel_len = 689                         # model.py:254 -- stateful, see inference_ex
        self.last_loudness = None                       # dict(lufs, peak, gain) of the last inference_ex(..., loudness=...) call
        self.last_limit = None                          # dict(peak_in, min_gain) of the last inference_ex(..., limiter=...) call
        self.last_report = None                         # report.LoudnessReport of the last call that asked for one (report=True)
        self._denoise_bias = None                       # zvx_denoise_bias of the main context, computed on first use (denoise_bias)
        self.hidden = self._ctx.hidden

    @property
    def ctx(self):
        return self._ctx

    @property
    def output_rate(self):
        """sampling rate of every waveform the model hands back: the model's own by default; another rate is converted on the
        device as the last launch of each waveform call (zvx_set_int "out_rate")"""
        return self._ctx.get_int("out_rate") or self._ctx.get_int("sampling_rate")

    @output_rate.setter
    def output_rate(self, hz):
        if self._streaming:
            raise RuntimeError("output_rate while a synthesize_batches generator is active: its contexts are in use")
        hz = int(hz or 0)
        if hz == self._ctx.get_int("sampling_rate"):
            hz = 0
        for c in [self._ctx] + self._more_ctx:
            c.set_int("out_rate", hz)

    @property
    def denoise_bias(self):
        """[fft_size / 2 + 1] float32: the vocoder's bias spectrum (include/zvx.h, zvx_denoise_bias), computed once, on first use.  It
        runs the vocoder, so it is taken BEFORE a call's encoder, never between a decode and its vocode."""
        if self._denoise_bias is None:
            self._denoise_bias = self._ctx.denoise_bias()
        return self._denoise_bias

    def refresh_denoise_bias(self):
        """recompute the bias, e.g. after a switch that changes the vocoder's arithmetic (set_int "voc_f16") -> the new bias"""
        self._denoise_bias = None
        return self.denoise_bias

    def loudness_report(self, wav, rate=None):
        """the programme loudness report of one finished waveform on the host (zvx_loudness_stats + zvx_true_peak, 4x) at `rate` Hz (None:
        the output rate) -> report.LoudnessReport, also kept as ``last_report``"""
        rate = self.output_rate if rate is None else int(rate)
        row = [np.asarray(wav, np.float32).reshape(-1)]
        self.last_report = LoudnessReport.from_stats(self._ctx.loudness_stats(row, rate=rate), self._ctx.true_peak(row, rate=rate)[0])
        return self.last_report

    def loudness_report_device(self, ptr, n, rate):
        """likewise for n f32 samples at `ptr` on the device, behind whatever was queued on them: nothing but the figures comes to the host"""
        ctx = self._ctx
        self.last_report = LoudnessReport.from_stats(ctx.loudness_stats_device(ptr, [n], max(n, 1), rate=rate),
                                                     ctx.true_peak_device(ptr, [n], max(n, 1), rate=rate)[0])
        return self.last_report

    def post_chain_device(self, buf, lengths, stride, *, denoise=None, watermark=None, loudness=None, limiter=None, rate=None, eq=None):
        """Denoise, equalise, watermark, normalise, limit, in this order and IN PLACE over device rows [B][stride] f32 at `buf` (at `rate`
        Hz), each None or the keywords of its Context.*_device call (denoise with its bias; eq: taps and delay, equaliser.params).  The
        first three only queue, the last two wait for their figures -> (normalize_device's (lufs, peak, gain) or None, limit_device's
        (peak_in, min_gain) or None).  The equaliser runs before the mark, so that the mark is not reshaped, and before the gain and the
        limiter, so that the delivered level and peak hold for the equalised signal."""
        ctx = self._ctx
        if denoise is not None:
            ctx.denoise_device(buf, lengths, stride, no_sync=True, **denoise)
        if eq is not None:
            ctx.fir_device(buf, lengths, stride, no_sync=True, **eq)
        if watermark is not None:
            ctx.watermark_device(buf, lengths, stride, no_sync=True, **watermark)
        return (None if loudness is None else ctx.normalize_device(buf, lengths, stride, rate=rate, **loudness),
                None if limiter is None else ctx.limit_device(buf, lengths, stride, rate=rate, **limiter))

    def _spkemb(self, x):
        """ResNetSE34V2.forward: x [B, Tr, 80] -> [B, 1, hidden] (ResNetSE34V2.py:176-212)."""
        x = np.asarray(x, np.float32)
        lens = np.full(x.shape[0], x.shape[1], np.int32)
        return self._ctx.spkemb(x, lens)[:, None, :]

    def inference_ex(self, x, style_embed, normalize_before=True, force_duration=False, prosody=None, loudness=None, limiter=None,
                     denoise=None, report=False, watermark=None, eq=None):
        """model.py:308-347.  x = {"phoneme" [1,T], "puncts" [1,T], "duration" [1,T]|None}; returns
        (wav[:mel_len*hop], mel_len, log_duration [1,T], mel [n_mels, mel_len]).  Batch-1 like the reference.
        Under an output_rate the waveform holds resampled_len(mel_len*hop) samples of that rate; mel_len stays in frames.
        prosody: None, a prosody.Prosody or a dict of Prosody.create keywords (speed, pitch / energy shift and range, targets).
        loudness: None (the path above, untouched) or Context.normalize_device keywords (target, peak_ceiling, max_gain_db).
        limiter: None (likewise) or Context.limit_device keywords (ceiling, window_ms, oversample); it runs behind the loudness gain.
        denoise: None (likewise) or Context.denoise_device keywords (strength, floor): the bias denoiser, directly behind the vocoder.
        watermark: None (likewise) or watermark.params(...) (key and the embedder's parameters): the keyed mark, behind the denoiser and
        before the loudness gain and the limiter.
        eq: None (likewise) or equaliser.params(...) (taps, delay): the FIR equaliser (zvx_fir), behind the denoiser and before the mark.
        report: with True the returned waveform is measured as delivered (at the output rate, behind every step above; on the device
        where it is still there) and ``last_report`` holds its report.LoudnessReport; False (the default) adds nothing to the call."""
        if denoise is not None:
            denoise = dict(denoise, bias=self.denoise_bias)          # (first use runs the vocoder: before this call's encoder)
        phoneme = np.asarray(x["phoneme"], np.int32)
        puncts = np.asarray(x["puncts"], np.int32)
        if phoneme.ndim != 2 or phoneme.shape[0] != 1:
            raise ValueError("inference_ex is batch-1 (model.py:325); use synthesize_batch for batches")
        T = np.array([phoneme.shape[1]], np.int32)
        dur = np.asarray(x["duration"], np.int32) if (force_duration and x.get("duration") is not None) else None
        spk = np.asarray(style_embed, np.float32).reshape(1, -1)
        mel_len, logd, _, _ = self._ctx.encode(phoneme, puncts, T, spk, dur, prosody=prosody)
        ml = int(mel_len[0])
        if ml < 2:
            # the reference raises inside InstanceNorm1d / conv stacks for degenerate lengths
            raise ValueError(f"predicted mel length {ml} is too short to synthesise")
        mel = self._ctx.decode(1, ml)
        pad_to = self._min_mel_len                       # model.py:331-335: pad up, or raise the floor
        if ml > self._min_mel_len:
            self._min_mel_len = ml
        if loudness is not None or limiter is not None or denoise is not None or watermark is not None or eq is not None:
            wav = self._vocode_normalized(mel_len, pad_to, loudness, limiter, denoise, report, watermark, eq)
            return wav, ml, logd, np.ascontiguousarray(mel[0, :ml].T)
        wav = self._ctx.vocode(1, mel_len, np.array([pad_to], np.int32))
        wav = wav[0, : self._ctx.out_samples(ml * self._hop_length)]
        if report:
            self.loudness_report(wav)
        return wav, ml, logd, np.ascontiguousarray(mel[0, :ml].T)

    def _vocode_normalized(self, mel_len, pad_to, loudness, limiter=None, denoise=None, report=False, watermark=None, eq=None):
        """The vocoder writes its row on the device at the model's rate, post_chain_device runs over it in place (queued behind the vocoder:
        stream order is the fence), an output rate converts it, and only then the row comes to the host.  Every step may be absent.
        self.last_loudness reports dict(lufs, peak, gain), self.last_limit dict(peak_in, min_gain); with `report` self.last_report is the finished row's LoudnessReport, measured on the
        device buffer unless an output rate converts it (the converted row is then measured as it arrives)."""
        ctx = self._ctx
        n = int(mel_len[0]) * self._hop_length
        native = ctx.get_int("sampling_rate")
        out_rate = ctx.get_int("out_rate") or native
        buf = ctx.dev_alloc(n * 4)
        try:
            ctx.vocode_device(mel_len, np.array([pad_to], np.int32), buf, n, native_rate=True, no_sync=True)
            loud, lim = self.post_chain_device(buf, [n], n, denoise=denoise, watermark=watermark, loudness=loudness, limiter=limiter, rate=native,
                                               eq=eq)
            if loud is not None:
                self.last_loudness = dict(lufs=float(loud[0][0]), peak=float(loud[1][0]), gain=float(loud[2][0]))
            if lim is not None:
                self.last_limit = dict(peak_in=float(lim[0][0]), min_gain=float(lim[1][0]))
            if out_rate == native:
                if report:
                    self.loudness_report_device(buf, n, native)
                return ctx.dev_to_host(buf, (n,), np.float32)
            wav = ctx.resample_device(buf, n, native, out_rate)
            if report:
                self.loudness_report(wav, out_rate)
            return wav
        finally:
            try:
                ctx.sync()
            finally:
                ctx.dev_free(buf)

    def inference(self, x, style_embed, normalize_before=True):
        wav, mel_len, log_duration, _ = self.inference_ex(x=x, style_embed=style_embed, normalize_before=normalize_before)
        return wav, mel_len, log_duration

    # HiFi-GAN's receptive field in mel frames (conv_pre k7: 3; upsample stacks: ~1; ResBlock k=11 dilations 1/3/5 at 8
    # samples per frame: 60 / 8 = 7.5; later stages < 2 in total): SURVEY.md 8(f-4) quotes 9-13.  A halo of 16 frames on
    # each side makes a chunk's interior identical to the same samples of a whole-utterance pass.
    STREAM_HALO = 16

    def vocode_stream(self, mel, chunk_frames=64, halo=STREAM_HALO, chunks_per_call=1, limiter=None, denoise=None, resident=False, level=None,
                      watermark=None):
        """Chunked vocoding for first-audio latency: mel [L, n_mels] -> yields waveform chunks (np.float32) that
        concatenate to ``vocode_mel(mel)``.  Every chunk is vocoded with ``halo`` extra frames on each side and only its
        interior is kept; ``chunks_per_call`` chunks ride in one launch sequence as independent batch rows.
        Under an output rate (the context's "out_rate") the chunks are still vocoded at the native rate (ZVX_NATIVE_RATE) and the
        stream is converted window by window (zerovox_amd.resample): the pieces concatenate bit for bit to the conversion of the
        whole native stream; a piece is yielded once every sample under its filter has arrived.
        limiter: None, or the keywords longform.limit_keywords builds (ceiling, window_ms, oversample): the native-rate chunks pass
        through the windowed limiter (zerovox_amd.limiter, zvx_limit_ex) and concatenate bit for bit to zvx_limit of the whole native
        stream; the limited stream runs limiter.reach(W, oversample) samples behind the vocoder.  Limiter first, conversion second.
        denoise: None (nothing of the denoiser is created), or the keywords ZeroVoxTTS._denoise builds (strength, floor): the native-rate
        chunks pass through the windowed denoiser (zerovox_amd.denoiser, zvx_denoise_ex) with ``denoise_bias`` and concatenate bit for
        bit to zvx_denoise of the whole native stream; the denoised stream runs denoiser.reach(fft_size) = fft_size - 1 samples behind
        the vocoder.  Denoiser first, then the limiter, then the conversion -- the order of ``inference_ex``; the delays add up.
        level: None, or Context.level_window keywords (target, and optionally max_gain_db, window_ms, lookahead_ms): the native-rate
        chunks pass through the windowed leveler (zerovox_amd.leveler, zvx_level_ex) and concatenate bit for bit to zvx_level of the
        whole stream that reaches it; the levelled stream runs RR = leveler.reach(...)[1] samples behind that stage's input (4409
        samples, 200 ms, at 22.05 kHz with the defaults).  The chain is denoise, then level, then limit, then the conversion.  With
        resident=True this method still raises ValueError for level; a session with a level stage is ``vocode_stream_sessions([mel],
        level=...)`` or ``Context.stream_open(..., level=...)``.
        watermark: None, or watermark.params(...) (key and the embedder's parameters): the native-rate chunks pass through the windowed
        embedder (zerovox_amd.watermark, zvx_watermark_ex) and concatenate bit for bit to zvx_watermark of the whole stream that reaches
        it; the marked stream runs watermark.reach(fft_size) = fft_size - 1 samples behind that stage's input.  The chain is denoise,
        level, watermark, limit, conversion.
        resident: False (the default: the host-planned stream above), or True: the same keywords drive a stream session of the library
        (include/zvx.h, zvx_stream_open) -- the mel is uploaded once, the samples stay on the device between the steps and every piece
        costs one wait.  The pieces concatenate to the same bits; where they are cut may differ.  With a watermark the session is one of
        zvx_stream_open_ex, the stage planned inside the library like the others.  mel None (resident only): the mel the context holds
        after decode."""
        if resident:
            if level is not None:
                raise ValueError("vocode_stream: resident=True does not take level= (a session with a level stage is "
                                 "vocode_stream_sessions([mel], level=...); or use resident=False)")
            yield from self._vocode_stream_resident(mel, chunk_frames, halo, chunks_per_call, limiter, denoise, None, watermark)
            return
        ctx = self._ctx
        rate, native = ctx.get_int("out_rate"), ctx.get_int("sampling_rate")
        convert = rate > 0 and rate != native
        if denoise is not None:
            denoise = dict(denoise, bias=self.denoise_bias)          # (first use runs the vocoder: before this stream's first chunk)
        chunks = self._vocode_stream_native(mel, chunk_frames, halo, chunks_per_call,
                                            convert or limiter is not None or denoise is not None or level is not None or watermark is not None)
        if denoise is not None:
            chunks = stream_windows(chunks, DenoisePlanner(ctx.get_int("fft_size")), lambda x, o, b, n, last: ctx.denoise_window(
                [x], in_origin=o, out_begin=b, out_count=n, last=last, **denoise)[0].copy())
        if level is not None:
            level = dict(dict(window_ms=3000.0, lookahead_ms=100.0), **level)
            plan = LevelPlanner(*level_reach(native, level["window_ms"], level["lookahead_ms"]))
            chunks = stream_windows(chunks, plan, lambda x, o, b, n, last: ctx.level_window(
                [x], in_origin=o, out_begin=b, out_count=n, last=last, rate=native, **level)[0][0].copy())
        if watermark is not None:
            chunks = stream_windows(chunks, WatermarkPlanner(ctx.get_int("fft_size")), lambda x, o, b, n, last: ctx.watermark_window(
                [x], in_origin=o, out_begin=b, out_count=n, last=last, **watermark)[0].copy())
        if limiter is not None:
            plan = LimitPlanner(window_samples(native, limiter["window_ms"]), limiter["oversample"])
            chunks = stream_windows(chunks, plan, lambda x, o, b, n, last: ctx.limit_window(
                [x], in_origin=o, out_begin=b, out_count=n, last=last, rate=native, **limiter)[0][0].copy())
        if convert:
            chunks = stream_resample(chunks, native, rate, lambda x, o, b, n: ctx.resample_window([x], native, rate, o, b, n)[0][0].copy())
        yield from chunks

    @staticmethod
    def _session_stages(level, watermark):
        """the level / watermark keywords of a session (Context.stream_open): none where neither stage is asked for"""
        more = {}
        if level is not None:
            more["level"] = level
        if watermark is not None:
            more["watermark"] = watermark
        return more

    def _vocode_stream_resident(self, mel, chunk_frames, halo, chunks_per_call, limiter, denoise, level=None, watermark=None):
        bias = self.denoise_bias if denoise is not None else None           # (first use runs the vocoder: before the session opens)
        yield from self._ctx.stream_open(mel, chunk_frames=chunk_frames, chunks_per_call=max(1, chunks_per_call), halo=halo, denoise=denoise,
                                         bias=bias, limit=limiter, **self._session_stages(level, watermark))

    def vocode_stream_many(self, mels, chunk_frames=64, halo=STREAM_HALO, chunks_per_call=1, limiter=None, denoise=None):
        """Many utterances streamed together: mels, a list of [L_i, n_mels] arrays -> yields (index, piece) with non-empty float32 pieces
        only.  One stream session per mel (the keywords of ``vocode_stream``), all stepped by one zvx_stream_next_many per round
        (zerovox_amd.serve.StreamBatcher): the chunks of every utterance ride through the vocoder as one batch.  The pieces of index i
        concatenate bit for bit to ``vocode_stream(mels[i], ..., resident=True)``.  ``vocode_stream_sessions`` is this method with the
        level and watermark stages."""
        return self.vocode_stream_sessions(mels, chunk_frames=chunk_frames, halo=halo, chunks_per_call=chunks_per_call, limiter=limiter,
                                           denoise=denoise)

    def vocode_stream_sessions(self, mels, *, chunk_frames=64, halo=STREAM_HALO, chunks_per_call=1, limiter=None, denoise=None, level=None,
                               watermark=None):
        """``vocode_stream_many`` with every stage of a stream session (include/zvx.h, zvx_stream_open_ex): what it does and yields, and
        level: None or the ``level`` keywords of ``vocode_stream``, for every mel;
        watermark: None, one watermark.params(...) dict for every mel, or a sequence of them, one per mel (None entries: that mel goes
        out unmarked) -- sessions that differ in their key alone are marked by one launch group per round.
        The pieces of index i concatenate bit for bit to ``vocode_stream(mels[i], ..., level=, watermark=)``, resident or host-planned."""
        from .serve import StreamBatcher
        mels = list(mels)
        if watermark is None or isinstance(watermark, dict):
            marks = [watermark] * len(mels)
        else:
            marks = list(watermark)
            if len(marks) != len(mels):
                raise ValueError(f"vocode_stream_sessions: {len(marks)} watermarks for {len(mels)} mels")
        bias = self.denoise_bias if denoise is not None else None           # (first use runs the vocoder: before the sessions open)
        batcher = StreamBatcher(self._ctx)
        try:
            index = {batcher.open(np.asarray(m, np.float32), chunk_frames=chunk_frames, chunks_per_call=max(1, chunks_per_call), halo=halo,
                                  denoise=denoise, bias=bias, limit=limiter, **self._session_stages(level, marks[i])): i for i, m in enumerate(mels)}
            while len(batcher):
                for id_, piece, _ in batcher.step():
                    if len(piece):
                        yield index[id_], piece
        finally:
            batcher.close_all()

    def _vocode_stream_native(self, mel, chunk_frames, halo, chunks_per_call, native_rate):
        mel = np.asarray(mel, np.float32)
        L, hop = mel.shape[0], self._hop_length
        starts = list(range(0, L, chunk_frames))
        for g in range(0, len(starts), max(1, chunks_per_call)):
            grp = starts[g:g + max(1, chunks_per_call)]
            spans = [(max(0, s - halo), min(L, s + chunk_frames + halo)) for s in grp]
            P = np.array([hi - lo for lo, hi in spans], np.int32)
            batch = np.zeros((len(grp), int(P.max()), mel.shape[1]), np.float32)
            for i, (lo, hi) in enumerate(spans):
                batch[i, :hi - lo] = mel[lo:hi]
            wav = self._ctx.vocode_mel(batch, P, native_rate=native_rate)
            for i, s in enumerate(grp):
                lo = spans[i][0]
                n = min(chunk_frames, L - s)
                yield wav[i, (s - lo) * hop:(s - lo + n) * hop].copy()

    def synthesize_batches(self, batches, in_flight=2, want_mel=False):
        """Throughput mode for a stream of batches: `in_flight` contexts of this model (one stream and one set of work buffers
        each; the first call creates them, +~0.5 GB of weights apiece), batches alternating between them from worker threads
        (the C calls release the GIL), so that batch i + 1's encoder / decoder -- latency-paced launches -- run under batch i's
        vocoder, which holds the chip at its power limit.  Measured at 32 x 128 phonemes with the waveforms delivered to host memory
        (tools/two_contexts.py): 24.5 ms per batch sequentially, 23.5 with two in flight, 22.5 with three (device-resident outputs
        through the C-ABI: 23.4 -> 21.4 with two).  `batches` yields dicts of synthesize_batch arguments (phoneme, puncts, T, style_embed[, duration, pad_to,
        Lmax_cap, prosody]); results come back IN ORDER, each bit-identical to synthesize_batch on the same arguments."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        n = max(1, int(in_flight))
        if self._streaming:
            raise RuntimeError("a synthesize_batches generator of this model is still active: its contexts are in use "
                               "(exhaust or close() it first; a context is not re-entrant, include/zvx.h)")
        while len(self._more_ctx) < n - 1:
            self._more_ctx.append(_lib.Context(self._packed[0], self._packed[1], self._device))
            self._more_ctx[-1].set_int("out_rate", self._ctx.get_int("out_rate"))       # every context of the model delivers at its output_rate
        ctxs = [self._ctx] + self._more_ctx[:n - 1]
        self._streaming = True
        try:
            yield from self._run_batches(ctxs, batches, n, want_mel)
        finally:
            self._streaming = False

    def release_contexts(self):
        """Free the extra contexts synthesize_batches created (weights + work buffers, ~0.5 GB each); the next call re-creates them."""
        if self._streaming:
            raise RuntimeError("a synthesize_batches generator is still active")
        for c in self._more_ctx:
            c.close()
        self._more_ctx = []

    def close(self):
        """Release every context of the model (device memory, streams).  The object is unusable afterwards."""
        self.release_contexts()
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def _run_batches(self, ctxs, batches, n, want_mel):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        def run(c, kw):
            B = np.asarray(kw["phoneme"]).shape[0]
            pad_to = kw.get("pad_to")
            if pad_to is None:
                pad_to = np.full(B, 689, np.int32)
            return c.synthesize(kw["phoneme"], kw["puncts"], kw["T"], kw["style_embed"], kw.get("duration"), pad_to, want_mel, kw.get("Lmax_cap", 0),
                                prosody=kw.get("prosody"))

        with ThreadPoolExecutor(max_workers=n) as ex:
            pending = deque()
            for i, kw in enumerate(batches):
                if len(pending) >= n:                   # context i % n is the one whose batch i - n is the oldest pending
                    yield pending.popleft().result()
                pending.append(ex.submit(run, ctxs[i % n], kw))
            while pending:
                yield pending.popleft().result()

    def synthesize_batch(self, phoneme, puncts, T, style_embed, duration=None, pad_to=None, want_mel=True, Lmax_cap=0, prosody=None):
        """B independent utterances in one launch sequence; each equals a batch-1 ``inference_ex`` call with
        ``_min_mel_len == pad_to[b]`` (default: the fresh-model value 689).  Padded [B, Tmax] id arrays.  prosody: as for inference_ex,
        per utterance ([B] / [B, Tmax] controls).  style_embed: [B, hidden] floats, or an int -- a device pointer to them, e.g. what
        Context.spkemb_wav_device wrote (ZVX_DEVICE_SPK)."""
        B = np.asarray(phoneme).shape[0]
        if pad_to is None:
            pad_to = np.full(B, 689, np.int32)
        if self._streaming:
            raise RuntimeError("synthesize_batch while a synthesize_batches generator is active: the context is not re-entrant")
        return self._ctx.synthesize(phoneme, puncts, T, style_embed, duration, pad_to, want_mel, Lmax_cap, prosody=prosody)
