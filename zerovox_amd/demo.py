"""`python -m zerovox_amd.demo` -- the reference's `demo.py --iter N` benchmark loop (demo.py:99-138) on libzvx:
same RTF definition (audio seconds / synthesis seconds), same warm-up rule (iterations i <= 10 discarded), same prints.

    python -m zerovox_amd.demo --model synthetic:styletts --meldec-model synthetic:v1 --iter 30 "hello world, this is a test."

`--long`: the text (or, where the argument names a file, the file's contents) is a paragraph: ZeroVoxTTS.tts_long synthesises it
sentence by sentence in batches and joins the sentences on the device; --wav-filename receives the joined waveform.
`--loudness LUFS` (with `--peak-db DB`) brings the waveform -- with `--long` the paragraph as one programme -- to an integrated loudness on
the device (zvx_normalize).  `--limiter` (with `--limiter-ms MS`) holds it under `--peak-db` with the true-peak look-ahead limiter
(zvx_limit); the loudness gain is then no longer bounded by the peak.  `--denoise S` takes S times the vocoder's bias spectrum off the
waveform on the device, directly behind the vocoder (zvx_denoise; 0.01 is the usual strength; its audible benefit is not measured here).
`--eq NAME`: a preset of zerovox_amd.equaliser (presence, warm, rumble, telephone, flat) filters the waveform on the device, behind the denoiser
and before the mark, the loudness gain and the limiter (zvx_fir; tts and --long, not the --level stream; no claim of audible merit is made).
`--level LUFS`: the utterance is STREAMED (ZeroVoxTTS.tts_stream) and levelled window by window towards a short-term loudness on the device
(zvx_level_ex: an AGC, not the R128 normalisation of --loudness; its audible merit is not measured here); --denoise and, with --limiter,
--peak-db apply to the stream as well, and the pieces are joined for the WAV file.
`--report`: the finished waveform is measured as delivered, on the device (zvx_loudness_stats, zvx_true_peak): integrated loudness, loudness
range, maximum momentary and short-term loudness, sample and true peak are printed, and with --loudness whether it meets that target.
`--pitch-report`: the finished waveform's F0 track is measured on the device (zvx_pitch) and its median, 5th .. 95th percentile range in Hz
and semitones, mean and voiced fraction are printed: what --pitch-shift / --pitch-range did to the audio.
`--watermark KEY`: the waveform carries the keyed mark of zvx_watermark (tts, --long and the --level stream alike; KEY as 0x... or decimal).
`--detect-watermark KEY FILE`: no synthesis -- the 16-bit mono WAV file is searched for KEY's mark on the device (zvx_watermark_detect) and
the score, offset and decision are printed.  Detection is measured on synthetic signals only; short telephone-band clips are not reliably
detectable, and nothing is claimed about audibility or robustness against codecs.
`--identify-watermark KEYFILE FILE`: no synthesis -- KEYFILE holds one candidate key per line (decimal or 0x hex; blank lines and lines that
start with # are skipped), and the WAV file is searched for all of them in one call (zvx_watermark_identify): the best key, its score, the
margin over the second best and the decision are printed.  The largest wrong-key score grows with the number of keys tried.
`--voice-report`: the finished waveform is embedded again on the device and compared with the speaker embedding it was conditioned on
(zvx_spkemb_wav, zvx_spk_score); the cosine similarity is printed.  No threshold is applied: none is measured.
`--match-voice LIBRARY.npz FILE`: no synthesis -- the 16-bit mono WAV file is enrolled on the device and searched for in the library of
voices (voices.VoiceLibrary.save's .npz of names and embeddings; zvx_spk_topk); the best five are printed.
`--mcd REF.wav`: the finished waveform is aligned on the device with the 16-bit mono recording of the same sentence (zvx_align_wav) and the
mel-cepstral distortion along the DTW path is printed.  It is the distortion of DCT cepstra of the model's own log-mel, c0 left out: figures
from SPTK / WORLD analysis in papers are not comparable with it, and no perceptual claim is made.
`--rhythm-from REF.wav`: the text is said with the timing of that recording -- a first pass is aligned with it and its per-phoneme frame
counts become forced durations of the second (tts(rhythm_from=...)).  Whether that sounds right on a real checkpoint is not measured.
"""
import argparse
import os
import time

import numpy as np

from .synthesize import ZeroVoxTTS, write_wav_to_file


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("text", nargs="?", default="")
    ap.add_argument("--model", default="synthetic:styletts")
    ap.add_argument("--meldec-model", default="synthetic:v1")
    ap.add_argument("--infer-device", default="cuda")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--iter", type=int, default=1)
    ap.add_argument("--refmel-frames", type=int, default=258, help="synthetic 3 s reference mel for the speaker encoder")
    ap.add_argument("--wav-filename", default=None)
    ap.add_argument("--speed", type=float, default=1.0, help="speaking-rate factor (2.0: twice as fast)")
    ap.add_argument("--pitch-shift", type=float, default=0.0, help="added to the normalised pitch prediction")
    ap.add_argument("--pitch-range", type=float, default=1.0, help="pitch spread about the utterance mean (0: flat, 1: as predicted)")
    ap.add_argument("--energy-shift", type=float, default=0.0)
    ap.add_argument("--energy-range", type=float, default=1.0)
    ap.add_argument("--out-rate", type=int, default=0, help="output sampling rate in Hz, converted on the device (0: the model's rate)")
    ap.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                    help="integrated loudness (BS.1770 / R128) the waveform is brought to on the device, e.g. -16 or -23 (default: as the model gives it)")
    ap.add_argument("--peak-db", type=float, default=-1.0, metavar="DB", help="sample-peak ceiling of the loudness gain in dBFS")
    ap.add_argument("--limiter", action="store_true", help="limit the waveform to --peak-db on the device (true-peak detection, look-ahead)")
    ap.add_argument("--limiter-ms", type=float, default=5.0, metavar="MS", help="smoothing window of the limiter's gain on either side of a peak")
    ap.add_argument("--denoise", type=float, default=None, metavar="S",
                    help="strength of the vocoder-bias denoiser on the device, e.g. 0.01 (default: off)")
    ap.add_argument("--eq", default=None, metavar="NAME", help="equaliser preset applied on the device: presence, warm, rumble, telephone, flat (default: off)")
    ap.add_argument("--level", type=float, default=None, metavar="LUFS",
                    help="stream the utterance and level it towards this short-term loudness on the device, e.g. -16 (default: off)")
    ap.add_argument("--long", action="store_true", help="long-form: split the text (or the file it names) into sentences and join them on the device")
    ap.add_argument("--report", action="store_true", help="measure the finished waveform on the device and print its programme loudness report")
    ap.add_argument("--pitch-report", action="store_true", help="measure the finished waveform's F0 track on the device and print its pitch report")
    ap.add_argument("--watermark", type=lambda v: int(v, 0), default=None, metavar="KEY", help="mark the waveform with this key on the device (default: off)")
    ap.add_argument("--detect-watermark", nargs=2, default=None, metavar=("KEY", "FILE"),
                    help="no synthesis: search the 16-bit mono WAV FILE for KEY's mark and print the result")
    ap.add_argument("--identify-watermark", nargs=2, default=None, metavar=("KEYFILE", "FILE"),
                    help="no synthesis: search the 16-bit mono WAV FILE for the mark of every key in KEYFILE (one per line, decimal or 0x hex)")
    ap.add_argument("--voice-report", action="store_true",
                    help="embed the finished waveform again on the device and print its similarity to the speaker embedding asked for")
    ap.add_argument("--match-voice", nargs=2, default=None, metavar=("LIBRARY.npz", "FILE"),
                    help="no synthesis: enrol the 16-bit mono WAV FILE on the device and print the best five voices of the library")
    ap.add_argument("--mcd", default=None, metavar="REF.wav",
                    help="align the finished waveform with this 16-bit mono recording of the same sentence on the device and print the distortion")
    ap.add_argument("--rhythm-from", default=None, metavar="REF.wav", help="copy the timing of this 16-bit mono recording of the same text")
    args = ap.parse_args()
    if (args.mcd or args.rhythm_from) and (args.long or args.level is not None):
        ap.error("--mcd and --rhythm-from go with one plain utterance: neither with --long nor with --level")
    if args.detect_watermark is None and args.identify_watermark is None and args.match_voice is None and not args.text:
        ap.error("the text is missing")
    if args.eq is not None:
        from .equaliser import PRESETS
        if args.eq not in PRESETS:
            ap.error(f"--eq: {args.eq!r} is none of {', '.join(sorted(PRESETS))}")
        if args.level is not None:
            ap.error("--eq does not go with --level: the stream has no equaliser stage yet")
    if args.level is not None and (args.long or args.loudness is not None):
        ap.error("--level streams one utterance: it goes with neither --long nor --loudness")

    modelcfg, synth = ZeroVoxTTS.load_model(args.model, args.meldec_model, infer_device=args.infer_device, precision=args.precision)
    if args.out_rate:
        synth.output_rate = args.out_rate
    sr = synth.output_rate                                  # RTF and the WAV header follow the rate of the samples handed back
    if args.detect_watermark is not None:
        import wave
        with wave.open(args.detect_watermark[1], "rb") as f:
            if f.getnchannels() != 1 or f.getsampwidth() != 2:
                ap.error("--detect-watermark reads 16-bit mono WAV files")
            rate, pcm = f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), np.int16)
        res = synth.detect_watermark(pcm, int(args.detect_watermark[0], 0), sampling_rate=rate)
        print(f"watermark: {'DETECTED' if res.detected else 'not detected'} (score {res.score:.2f}, threshold {res.threshold:g}, offset "
              f"{res.offset} frames, window {res.window} of {len(res.windows)})")
        return
    if args.identify_watermark is not None:
        import wave
        with open(args.identify_watermark[0]) as f:
            keys = [int(line.strip(), 0) for line in f if line.strip() and not line.lstrip().startswith("#")]
        if not keys:
            ap.error("--identify-watermark: KEYFILE holds no key")
        with wave.open(args.identify_watermark[1], "rb") as f:
            if f.getnchannels() != 1 or f.getsampwidth() != 2:
                ap.error("--identify-watermark reads 16-bit mono WAV files")
            rate, pcm = f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), np.int16)
        res = synth.identify_watermark(pcm, keys, sampling_rate=rate)
        print(f"watermark: {'DETECTED' if res.detected else 'not detected'}: key {res.best} of {len(keys)} (0x{res.key:016x}), score {res.score:.2f}, "
              f"margin {res.margin:.2f} over the second best, threshold {res.threshold:g}, offset {res.offset} frames, window {res.window}")
        return
    if args.match_voice is not None:
        import wave
        from .voices import VoiceLibrary
        with wave.open(args.match_voice[1], "rb") as f:
            if f.getnchannels() != 1 or f.getsampwidth() != 2:
                ap.error("--match-voice reads 16-bit mono WAV files")
            rate, pcm = f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), np.int16)
        library = VoiceLibrary.load(synth.model.ctx, args.match_voice[0])
        query = synth.speaker_embed_batch([pcm.astype(np.float32) / np.float32(32760.0)], rate)
        for rank, m in enumerate(library.match(query, top=min(5, len(library)))[0]):
            print(f"{rank + 1}. {m.name} (row {m.index}): similarity {m.score:.4f}")
        library.close()
        return
    print("computing speaker embedding...")
    refmel = np.random.default_rng(0).standard_normal((args.refmel_frames, modelcfg["audio"]["num_mels"])).astype(np.float32)
    spkemb = synth.speaker_embed_from_mel(refmel)
    rtf, warmup = [], 10

    def print_report(rep):
        print(f"loudness report: {rep}")
        if args.loudness is not None:
            print(f"  meets {args.loudness:g} LUFS +- 0.5 LU, true peak <= {args.peak_db:g} dBTP: {rep.meets(args.loudness, max_true_peak_db=args.peak_db)}")

    def read_ref(path, flag):
        import wave
        with wave.open(path, "rb") as f:
            if f.getnchannels() != 1 or f.getsampwidth() != 2:
                ap.error(f"{flag} reads 16-bit mono WAV files")
            return f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), np.int16)
    rhythm_rate, rhythm = read_ref(args.rhythm_from, "--rhythm-from") if args.rhythm_from else (None, None)
    text = open(args.text, encoding="utf-8").read() if (args.long and os.path.isfile(args.text)) else args.text
    for i in range(args.iter):
        t0 = time.time()
        if args.long:
            wav, segments = synth.tts_long(text, spkemb, speed=args.speed, pitch_shift=args.pitch_shift, pitch_range=args.pitch_range,
                                           energy_shift=args.energy_shift, energy_range=args.energy_range, loudness=args.loudness,
                                           peak_db=args.peak_db, limiter=args.limiter, limiter_ms=args.limiter_ms, denoise=args.denoise,
                                           report=args.report, pitch_report=args.pitch_report, watermark=args.watermark,
                                           voice_report=args.voice_report, eq=args.eq)
            elapsed = time.time() - t0
            wav_len = (wav.shape[0] if segments else 0) / sr
            print(f"[{i + 1}/{args.iter}] Synth time: {elapsed:.2f} sec, {len(segments)} sentences, voice length: {wav_len:.2f} sec, rtf: {wav_len / elapsed:.2f}")
            if args.wav_filename and segments:
                write_wav_to_file(wav, length=0, filename=args.wav_filename, sample_rate=sr, hop_length=modelcfg["audio"]["hop_size"], samples=len(wav))
            if args.report and segments:
                print_report(synth.last_report)
            if args.pitch_report and segments:
                print(f"pitch report: {synth.last_pitch_report}")
            if args.voice_report and segments:
                print(f"voice report: {synth.last_voice_report}")
            if i > warmup:
                rtf.append(wav_len / elapsed)
            continue
        if args.level is not None:
            pieces = list(synth.tts_stream(args.text, spkemb, speed=args.speed, pitch_shift=args.pitch_shift, pitch_range=args.pitch_range,
                                           energy_shift=args.energy_shift, energy_range=args.energy_range, level_lufs=args.level,
                                           peak_db=args.peak_db if args.limiter else None, limiter_ms=args.limiter_ms,
                                           denoise_strength=args.denoise, watermark=args.watermark))
            wav = np.concatenate(pieces) if pieces else np.zeros(0, np.float32)
            elapsed = time.time() - t0
            wav_len = wav.shape[0] / sr
            print(f"[{i + 1}/{args.iter}] Synth time: {elapsed:.2f} sec, {len(pieces)} pieces, voice length: {wav_len:.2f} sec, rtf: {wav_len / elapsed:.2f}")
            if args.wav_filename and len(wav):
                write_wav_to_file(wav, length=0, filename=args.wav_filename, sample_rate=sr, hop_length=modelcfg["audio"]["hop_size"], samples=len(wav))
            if args.report and len(wav):                             # (a stream has no buffer left to measure: the joined pieces are)
                print_report(synth.loudness_report(wav, sr))
            if args.pitch_report and len(wav):
                print(f"pitch report: {synth.pitch_report(wav, sr)}")
            if args.voice_report and len(wav):
                print(f"voice report: {synth.voice_report(wav, spkemb, sr)}")
            if i > warmup:
                rtf.append(wav_len / elapsed)
            continue
        wav, phoneme, length = synth.tts(args.text, spkemb, speed=args.speed, pitch_shift=args.pitch_shift, pitch_range=args.pitch_range,
                                         energy_shift=args.energy_shift, energy_range=args.energy_range, loudness=args.loudness,
                                         peak_db=args.peak_db, limiter=args.limiter, limiter_ms=args.limiter_ms, denoise=args.denoise,
                                         report=args.report, pitch_report=args.pitch_report, watermark=args.watermark,
                                         voice_report=args.voice_report, rhythm_from=rhythm, rhythm_rate=rhythm_rate, eq=args.eq)
        elapsed = time.time() - t0
        wav_len = wav.shape[0] / sr
        print(f"[{i + 1}/{args.iter}] Synth time: {elapsed:.2f} sec, voice length: {wav_len:.2f} sec, rtf: {wav_len / elapsed:.2f}")
        if args.wav_filename:
            write_wav_to_file(wav, length=length, filename=args.wav_filename, sample_rate=sr, hop_length=modelcfg["audio"]["hop_size"],
                              samples=len(wav))
        if args.report and length:
            print_report(synth.last_report)
        if args.pitch_report and length:
            print(f"pitch report: {synth.last_pitch_report}")
        if args.voice_report and length:
            print(f"voice report: {synth.last_voice_report}")
        if rhythm is not None and length:
            al = synth.last_alignment
            print(f"rhythm: first pass {al.frames_a} frames against {al.frames_b} of the recording, {length} delivered")
        if args.mcd and length:
            ref_rate, ref = read_ref(args.mcd, "--mcd")
            al = synth.fidelity_report(wav, ref, sampling_rate=ref_rate, wav_rate=sr)
            print(f"fidelity: {al.mcd_db:.3f} dB between DCT cepstra of the model's log-mel (c0 left out; not comparable with SPTK / WORLD "
                  f"figures) over {len(al.path)} path cells, {al.frames_a} frames against {al.frames_b}")
        if i > warmup:
            rtf.append(wav_len / elapsed)
    if rtf:
        print("Average RTF: {:.2f}".format(np.mean(rtf)))


if __name__ == "__main__":
    main()
