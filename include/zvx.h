/*
 * zvx.h -- C-ABI of libzvx, the MI355X-native ZeroVOX synthesis path.
 *
 * The reference (gooofy/zerovox) has no FFI/plugin interface: its seam is the Python object API
 * (SURVEY.md 8b).  Each entry point below names the reference call it replaces.  A maintainer binds
 * them with ctypes; no torch types appear in any signature.
 *
 * Conventions
 *   - every function returns a zvx_status (0 = ok); zvx_last_error() returns the message of the last
 *     failure on that context (or of zvx_create when ctx is NULL);
 *   - one context per device, NOT thread-safe (like the reference object); no mutable process-wide state: every
 *     switch of zvx_set_int lives in its context, several contexts may be driven from several threads;
 *   - buffers are caller-allocated.  Host pointers by default; outputs flagged ZVX_DEVICE_OUT are
 *     device pointers on the context's device (used for the RCCL waveform gather);
 *   - batches are padded row-major: [B][Tmax] ids, [B][Lmax][80] mels, wav rows of `wav_stride` floats;
 *     every utterance is computed exactly as an independent batch-1 reference call
 *     (model.py:325-328 is batch-1 only), i.e. no statistic ever sees padding;
 *   - activations are time-major / channel-contiguous on the device ([time][channel]).
 */
#ifndef ZVX_H
#define ZVX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zvx_ctx zvx_ctx;
typedef int zvx_status;

enum {
    ZVX_OK = 0,
    ZVX_E_INVALID = 1,   /* bad argument / id out of range (reference: torch IndexError, assert) */
    ZVX_E_MANIFEST = 2,  /* manifest or weight blob malformed, tensor missing, unknown decoder kind (model.py:244) */
    ZVX_E_HIP = 3,       /* HIP runtime failure (message carries hipGetErrorString) */
    ZVX_E_STATE = 4,     /* call order violated (e.g. zvx_decode before zvx_encode) */
    ZVX_E_BUFFER = 5,    /* caller buffer too small for the produced length */
    ZVX_E_UNSUPPORTED = 6
};

enum {                   /* flags */
    ZVX_DEVICE_OUT = 1,  /* wav (and mel, if given) output pointers are device pointers */
    ZVX_NO_SYNC = 2,     /* do not hipStreamSynchronize before returning (device outputs only) */
    ZVX_DEVICE_IN = 8,   /* the bulk input (zvx_vocode_mel: mel, zvx_spkemb_ex: ref_mels) is a device pointer */
    ZVX_PCM16 = 4,       /* wav rows are int16 PCM: (int16)(sample * 32760), truncated like numpy astype (demo.py:29-35,
                            model.py:44-63); halves the bytes of the multi-GPU waveform gather.  wav_stride stays in samples */
    ZVX_HOST_ASYNC = 16, /* zvx_synthesize / zvx_vocode / zvx_vocode_mel: the waveform is delivered to HOST memory without the call waiting
                            for it (round 6) -- `wav` / `wav_stride` are ignored (wav may be NULL): the rows go to one of the context's two
                            pinned host slots on a copy stream of their own, the call returns after queueing (as with
                            ZVX_DEVICE_OUT | ZVX_NO_SYNC; no host mel / log_duration output), zvx_get_int("host_slot") names the slot
                            and zvx_wait_host(ctx, slot, ...) is where the host meets the rows.  Slots alternate (call i: slot i & 1);
                            a slot's rows stay valid until the second next ZVX_HOST_ASYNC call */
    ZVX_NATIVE_RATE = 32,/* zvx_vocode / zvx_vocode_mel / zvx_synthesize / zvx_synthesize_ex: this call ignores zvx_set_int("out_rate") and delivers
                            the generator's own samples at the model's rate (chunked streaming vocodes at the native rate and converts the
                            stream itself, zvx_resample_ex; it is also how a caller gets both) */
    ZVX_DEVICE_SPK = 64  /* zvx_synthesize / zvx_synthesize_ex only: `spk` is a device pointer on the context's device ([B][hidden] f32, e.g. the
                            ZVX_DEVICE_OUT | ZVX_NO_SYNC output of zvx_spkemb_wav / zvx_spkemb_ex queued just before).  It is copied device to device
                            into the call's speaker plane instead of travelling in the pinned input upload, behind everything issued so far on
                            the context's main stream (an event fences the front stream: no host wait); queued calls stay queued, and the
                            waveform is bit for bit that of the same floats passed from the host.  The buffer must stay alive until the call
                            has run (zvx_sync) */
};

enum {                   /* zvx_stage_times indices (milliseconds, hipEvent-timed on the ctx stream) */
    ZVX_T_ENCODER = 0, ZVX_T_VARIANCE = 1, ZVX_T_LENREG = 2, ZVX_T_DECODER = 3, ZVX_T_VOCODER = 4,
    ZVX_T_SPKEMB = 5, ZVX_T_RESAMPLE = 6,   /* the sample-rate conversion of the last waveform call (0 when that call ran none) or zvx_resample */
    ZVX_T_JOIN = 7,                         /* the launches of the last zvx_join / zvx_trim_bounds (bounds, layout, copy) */
    ZVX_T_COUNT = 8
};

/* Build a synthesis context on HIP device `device` from a text manifest + fp32 weight blob produced
 * by zerovox_amd.pack (weight-norm folded, conv weights laid out [tap][Cout][Cin]).
 * Replaces ZeroVoxTTS.__init__ / ZeroVox.load_from_checkpoint + get_meldec
 * (synthesize.py:48-97, model.py:86-118, model.py:206-249).
 * Generator shapes the device does not run are refused here (zvx_last_error(NULL) names the manifest key): ZVX_E_UNSUPPORTED for an
 * upsampling stage with an odd k - u or k > 3u (voc_ksizes / voc_rates), a last stage of fewer than 8 channels in the 16-bit precision
 * (4 in f32; voc_c0) and a ResBlock kernel of more than 16 taps (voc_rb_k); ZVX_E_MANIFEST for lists that do not fit each other.
 * Front-end shapes accepted (anything else: ZVX_E_UNSUPPORTED naming the key): `hidden` a multiple of 8; `enc_heads` / `dec_heads` dividing it
 * into head depths that are multiples of 8; both `ffn_k` odd and at most 15; `vp_dim` a multiple of 4; `ffn_dim` a multiple of 8 (4 in the f32
 * precision); `n_bins` >= 2; `n_mels` a multiple of 8 up to 128; four `rn_layers` >= 1 and four `rn_filters` that are multiples of 8 up to 256.
 * ZVX_E_MANIFEST where `n_mels` is not the input width of the tensor voc.pre_w (the generator's conv_pre).  `vp_k` other than 3 is accepted here
 * and refused by the first zvx_encode (ZVX_E_UNSUPPORTED).  A config zvx_create accepted never ends in a launcher refusing its shape. */
zvx_status zvx_create(const char* manifest, const void* weights, size_t nbytes, int device, zvx_ctx** out);
void       zvx_destroy(zvx_ctx* ctx);
const char* zvx_last_error(const zvx_ctx* ctx);
/* "precision" -> 0 bf16 / 1 f32; "hidden", "n_mels", "hop", "device" ... ; -1 if unknown.
 * "host_slot": the pinned host slot the last ZVX_HOST_ASYNC call writes (-1: none yet).
 * "f16_sat_events" (round 6): the telltale of the half mode's clamp.  Every 16-bit store of the IEEE-half kernels saturates at +-65504
 *   (below); after zvx_set_int("f16_sat_check", 1) every convolution of the vocoder and the mel decoders runs as its own launch (no
 *   LDS-resident intermediate; same arithmetic per convolution, ~3x the time: a debug mode) and every 16-bit tensor it writes is
 *   scanned for clamped values.  This key drains the context and returns how many were seen since the switch was last set: 0 means no
 *   clamp engaged on the inputs run so far -- the check to make once on a real checkpoint (the reference, fp32, has no such failure
 *   mode).
 * Every key of zvx_set_int returns its current value. */
int64_t    zvx_get_int(const zvx_ctx* ctx, const char* key);
/* "profile" 0/1/2 (0 off, 1 per-stage events, 2 + per-GEMM-launch events); "profile_only" variant id (-1 = all);
 * "shape_log" 0/1 (one stderr line per timed launch); "max_frames" hard cap on a predicted mel length (default 2^18:
 * the reference has none, fs2.py:678-681 -- a garbage log-duration must not drive an allocation -> ZVX_E_BUFFER).
 * "f16_sat_check" 0/1: the saturation audit of the half mode (see zvx_get_int "f16_sat_events"); setting it (re)zeroes the counter.
 * "out_rate" hz: the sampling rate of every waveform the context hands back (0, the default = the model's "sampling_rate": nothing changes, no
 *   extra launch or buffer).  Checked when set, against the model's rate, as zvx_resample checks a pair (ZVX_E_INVALID / ZVX_E_UNSUPPORTED,
 *   the switch keeps its value); see "Output rate" below.
 * Every other key is an A/B switch of a scheduling / tiling / arithmetic choice (INTEGRATION.md has the table and each key's values:
 * "enc_split", "attn_f32", "flash", "front_overlap", "va_overlap_maxb", "dec_f16", "dec_flat", "dec_sc_fuse", "norm_fuse_maxb", "voc_f16",
 * "voc_f16_stages", "voc_overlap_maxb", "voc_overlap_frames", "stagefuse", "rb2fuse", "resstream", "rs_seg_min", "pairstream", "slab_small",
 * "slab_flat", "spk_pool_fuse", "spk_s2_fuse", "poison_pads", "rs_prof");
 * all of them live in the context.  Unknown keys and values outside a key's set: ZVX_E_INVALID. */
zvx_status zvx_set_int(zvx_ctx* ctx, const char* key, int64_t value);

/* Speaker encoder: ref_mels [B][Tmax][80] log-mels, lens[B] frames -> out [B][hidden], L2-normalised.
 * Replaces ResNetSE34V2.forward (ResNetSE34V2.py:176-212) as called by ZeroVoxTTS.speaker_embed
 * (synthesize.py:139-141). */
zvx_status zvx_spkemb(zvx_ctx* ctx, const float* ref_mels, const int32_t* lens, int B, int Tmax, float* out);
/* same with flags: ZVX_DEVICE_IN (ref_mels on the device), ZVX_DEVICE_OUT (out on the device), ZVX_NO_SYNC */
zvx_status zvx_spkemb_ex(zvx_ctx* ctx, const float* ref_mels, const int32_t* lens, int B, int Tmax, float* out, int flags);

/* Speaker enrolment from raw audio, on the device: wav [B][Nmax] f32 with nsamples[b] valid samples at `rate` Hz -> out [B][hidden].
 * Defined as a composition of the calls of this header, run on the same batch of B rows:
 *   1. rate: rate == the model's "sampling_rate": the rows as given; otherwise row b is what zvx_resample(rate -> sampling_rate) computes
 *      for it, a signal of its own length ceil(n L / M), converted into a work buffer of the context (rate checks and ZVX_E_UNSUPPORTED as
 *      for zvx_resample).  Everything below is in samples at the model's rate.
 *   2. bounds: [begin, end) is what zvx_trim_bounds defines for (frame, hop, top_db, keep) -- its ambiguity band and its rules for rows
 *      left whole included.
 *   3. crop: max_samples > 0: end = min(end, begin + max_samples).
 *   4. mel: the m = end - begin samples of the window are a signal of their own; the mel is what zvx_melspec computes for it (the reflect
 *      padding mirrors about the window's own first and last sample and reads nothing outside [begin, end)); frames[b] = 1 + (m + 2 pad -
 *      n_fft) / hop.
 *   5. embedding: what zvx_spkemb computes on those mels with lens = frames.
 * Outside ambiguous trim frames `out` is bit for bit what zvx_resample, zvx_trim_bounds, a slice (and crop), zvx_melspec and zvx_spkemb
 * hand back for the same B rows: the same kernels in the same launch shapes; the one new launch cuts the reflect-padded windows at bounds
 * only the device knows.
 * Host traffic: the audio never goes to the host.  The call waits ONCE, for the bounds (as zvx_join waits for its layout): they give the host
 * the frame counts that validate the windows and size the GEMMs.  Everything behind that wait is queued on the main stream; with
 * ZVX_DEVICE_OUT | ZVX_NO_SYNC the call returns once it has queued.  begin / end / frames: host int32 [B], each may be NULL.
 * Flags: ZVX_DEVICE_IN (wav on the device: the rows may be the output of a synthesis call queued just before, stream order is the fence),
 *   ZVX_DEVICE_OUT (out on the device), ZVX_NO_SYNC (device out only).
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): a NULL ctx / wav / nsamples / params / out, B <= 0,
 *   Nmax <= 0, a negative length, nsamples[b] > Nmax, frame / hop / keep / top_db as for zvx_trim_bounds, max_samples < 0, unknown flags,
 *   ZVX_NO_SYNC without ZVX_DEVICE_OUT.  After the wait: a window that does not meet zvx_melspec's length conditions or has fewer than the 2
 *   frames zvx_spkemb needs is ZVX_E_INVALID (the message names the row, its bounds and the minimum); nothing is written to out, begin / end /
 *   frames are still filled, the context stays usable.
 * Accounting: stage slot ZVX_T_SPKEMB over the window cut, the front end and the encoder (the front end's launches counted as zvx_melspec's
 *   are); the conversion and the bounds as zvx_resample (ZVX_T_RESAMPLE) and zvx_trim_bounds (ZVX_T_JOIN, "post.join") count theirs.
 * Replaces ZeroVoxTTS.speaker_embed (synthesize.py:123-143) for a batch of reference clips: librosa.load(sr=...), librosa.effects.trim,
 * get_mel_from_wav and ResNetSE34V2.forward without the audio, the mel or the embedding crossing to the host in between. */
typedef struct zvx_ref_params {
    int32_t frame, hop;    /* trim analysis window and step in samples at the MODEL's rate (ZeroVoxTTS.speaker_embed: 2048 / 512) */
    float   top_db;        /* as zvx_join_params.top_db (speaker_embed: 40); <= 0: no trimming */
    int32_t keep;          /* as zvx_join_params.keep */
    int32_t max_samples;   /* > 0: the window is cut to its first max_samples samples after trimming; 0: no cut */
} zvx_ref_params;
zvx_status zvx_spkemb_wav(zvx_ctx* ctx, const float* wav, const int32_t* nsamples, int B, int Nmax, int rate,
                          const zvx_ref_params* params, float* out /* [B][hidden] */,
                          int32_t* begin, int32_t* end, int32_t* frames /* host [B], each may be NULL */, int flags);

/* Log-mel front end of reference audio: wav [B][Nmax] f32 in [-1, 1] with nsamples[b] valid samples ->
 * mel [B][Tmax][n_mels] = log(clip(mel_basis . |STFT|, 1e-5)) (reflect padding (n_fft-hop)/2, hann window, center=False)
 * and frames[b] = 1 + (nsamples[b] + 2*pad - n_fft) / hop, pad = (n_fft-hop)/2 rounded down.  The window is the periodic Hann of
 * win_length samples centred in n_fft; the mel basis is Slaney's (area-normalised triangles on the Slaney mel scale between fmin and
 * fmax).  Rows >= frames[b] are zero.  ZVX_E_INVALID if an utterance has fewer than max(pad + 1, n_fft - 2*pad) samples (a mirror on
 * both sides, one whole frame) or more than Nmax; ZVX_E_BUFFER if an utterance has more than Tmax frames.  Either message names the
 * utterance, and a refused call writes nothing.  The model's STFT: fft_size a multiple of 4, 1 <= hop_size <= fft_size,
 * 1 <= win_length <= fft_size, 0 <= fmin < fmax <= sampling_rate / 2 (pack_model and zvx_create refuse anything else by name).
 * Replaces get_mel_from_wav (mels.py:357-395) as called by ZeroVoxTTS.speaker_embed (synthesize.py:128-137). */
zvx_status zvx_melspec(zvx_ctx* ctx, const float* wav, const int32_t* nsamples, int B, int Nmax, float* mel, int Tmax,
                       int32_t* frames);

/* Phoneme encoder + variance adaptor + length regulator.  duration == NULL -> predicted durations
 * (fs2.py:678-681), else forced (force_duration=True, fs2.py:745).  Writes mel_len[B]; optional
 * log_duration / pitch / energy [B][Tmax].  The expanded features stay in the context.
 * Replaces FS2Encoder.forward (fs2.py:732-775). */
zvx_status zvx_encode(zvx_ctx* ctx, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration,
                      const int32_t* T, int B, int Tmax, const float* spk,
                      int32_t* mel_len, float* log_duration, float* pitch, float* energy);

/* Prosody control (opt-in; every pointer may be NULL = neutral).  nb = ve_n_bins, T_b = utterance b's phoneme count, p_t / e_t the
 * pitch / energy predictions, d_t today's integer duration (predicted max(rint(exp(logd)-1),0) or forced, clamped as without control).
 *   pitch:  m_b = mean of p_t over t < T_b (accumulated in f64, rounded once to f32);
 *           p'_t = (p_t + (pitch_range[b] - 1) * (p_t - m_b)) + pitch_shift[b], every operation a separately rounded f32 op (no FMA),
 *           so range 1 / shift 0 gives p_t bit for bit; pitch_target[b][t], where not NaN, replaces p'_t (the reference's train-time
 *           target path, fs2.py:631); bucket = clamp(rint(v * (nb-1)), 0, nb-1).
 *   energy: the same with energy_shift / energy_range / energy_target on e_t.  The energy predictor reads x + pitch_embedding[the
 *           CONTROLLED pitch bucket] (fs2.py:665-671): a pitch control changes the energy prediction.
 *   duration: q_t = dur_scale_q16[b][t] (65536 = unchanged; a factor of q / 65536 on the duration, i.e. speed = 65536 / q).
 *           P_t = sum_{u<=t} (int64) d_u * q_u, C_t = (P_t + 32768) >> 16, d'_t = C_t - C_{t-1}, mel_len = C_{T_b-1}: the running sum
 *           is rounded, not each phoneme, so the total is exact to half a frame.  Applies to predicted and forced durations (forced:
 *           the host computes mel_len with the same integer rule, the queued path stays free of syncs).
 *   outputs: log_duration / pitch / energy stay the RAW predictions; zvx_fetch "pitch_idx" / "energy_idx" / "duration" report the
 *           controlled values.
 *   validation (before anything is queued, ZVX_E_INVALID, the context stays usable): shifts and ranges finite, ranges in [0, 4],
 *           targets NaN or in [0, 1], q in [4096, 1048576] (factor 1/16 ... 16), over t < T_b.  A slowed utterance past Lmax_cap /
 *           max_frames is ZVX_E_BUFFER as for any predicted length. */
typedef struct zvx_prosody {
    const float*   pitch_shift;   /* [B] */
    const float*   pitch_range;   /* [B] */
    const float*   energy_shift;  /* [B] */
    const float*   energy_range;  /* [B] */
    const float*   pitch_target;  /* [B][Tmax], NaN = predicted */
    const float*   energy_target; /* [B][Tmax], NaN = predicted */
    const int32_t* dur_scale_q16; /* [B][Tmax], 65536 = 1.0 */
} zvx_prosody;

/* zvx_encode with prosody control; prosody == NULL is zvx_encode.  The control arrays are copied before the call returns. */
zvx_status zvx_encode_ex(zvx_ctx* ctx, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration,
                         const int32_t* T, int B, int Tmax, const float* spk,
                         int32_t* mel_len, float* log_duration, float* pitch, float* energy, const zvx_prosody* prosody);

/* Mel decoder on the context's features; mel_out [B][Lstride][n_mels] may be NULL; rows in [mel_len[b], max_b mel_len)
 * of utterance b are written as zeros.
 * Replaces FS2Decoder.forward (fs2.py:281-315) / StyleTTSDecoder.forward (styletts.py:181-205). */
zvx_status zvx_decode(zvx_ctx* ctx, float* mel_out, int Lstride, int flags);

/* Same on caller-supplied features [B][Lmax][hidden] (L[B] valid frames, spk [B][hidden]). */
zvx_status zvx_decode_features(zvx_ctx* ctx, const float* features, const int32_t* L, int B, int Lmax,
                               const float* spk, float* mel_out, int Lstride);

/* HiFi-GAN on the context's mel.  pad_to[B]: utterance b is vocoded on max(pad_to[b], mel_len[b]) frames,
 * rows >= mel_len zero (the reference's stateful `_min_mel_len`, model.py:331-335; NULL = no padding);
 * wav row b receives mel_len[b]*hop samples (model.py:347) followed by ZEROS up to max_b(mel_len[b])*hop -- the bytes
 * handed back never depend on earlier calls on the context; samples beyond that bound are not touched.  wav_stride
 * samples between rows; float rows, or int16 rows with ZVX_PCM16.
 * Replaces hifigan.Generator.forward (hifigan.py:114-130). */
zvx_status zvx_vocode(zvx_ctx* ctx, const int32_t* pad_to, void* wav, int64_t wav_stride, int flags);

/* Stand-alone vocoder: mel [B][Pmax][n_mels], P[B] frames -> wav rows of P[b]*hop samples.
 * Arithmetic of the 16-bit mode: weights, activations and the running sum of the generator are IEEE half on the f16 MFMA (round 5) in
 * every stage but a ResBlock1 stage of 128 channels, which computes in bf16 (round 6; zvx_set_int "voc_f16_stages": a mask of the stages
 * in half, "voc_f16" 0: the bf16 kernels of rounds 1-4 everywhere).  Every half store SATURATES at +-65504 (MODE.FP16_OVFL in the
 * kernels) -- a mel scaled far past the trained range gives a finite, clipped waveform, never Inf / NaN; whether a clamp ever engaged on
 * given weights and inputs: zvx_set_int "f16_sat_check" / zvx_get_int "f16_sat_events".
 * Non-finite input (NaN / Inf in a mel): the call succeeds and nothing faults; the samples of THAT utterance are unspecified (finite or
 * not -- the leaky-relu forms are compiled without NaN propagation guarantees); every other utterance of the batch and every later call
 * are bit for bit what they are without it.  The reference would propagate the NaN through that utterance as well. */
zvx_status zvx_vocode_mel(zvx_ctx* ctx, const float* mel, const int32_t* P, int B, int Pmax,
                          void* wav, int64_t wav_stride, int flags);

/* encode + decode + vocode.  mel_out / log_duration may be NULL.  With predicted durations the caller
 * sizes wav for Lmax_cap frames per utterance; ZVX_E_BUFFER if a prediction exceeds it.
 * Queued calls: with forced durations, ZVX_DEVICE_OUT | ZVX_NO_SYNC and mel_out == log_duration == NULL the call only
 * QUEUES work on the context's stream and returns (the host inputs are copied into pinned staging before it returns and may be
 * reused at once; mel_len is filled from the durations): successive calls keep the GPU fed whatever the host thread's timing.
 * With predicted durations the call waits once, for the predicted mel lengths.
 * Queued calls overlap (round 4): the context issues encoder / variance adaptor / mel decoder on its front stream and the vocoder on
 * its main stream; call i + 1's front end waits only for call i's vocoder to have copied the mel, so it runs UNDER that vocoder
 * (23.1 -> 21.2 ms per 32 x 128-phoneme batch on one context; bit-identical to the serial schedule; zvx_set_int "front_overlap").
 * A device mel output (mel_out with ZVX_DEVICE_OUT) is written on the front stream; zvx_sync drains every stream.
 * Replaces ZeroVox.inference_ex (model.py:308-347) over B independent utterances. */
zvx_status zvx_synthesize(zvx_ctx* ctx, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration,
                          const int32_t* T, int B, int Tmax, const float* spk, const int32_t* pad_to,
                          int Lmax_cap, void* wav, int64_t wav_stride, int32_t* mel_len,
                          float* mel_out, int Lstride, float* log_duration, int flags);
/* zvx_synthesize with prosody control (see zvx_prosody); prosody == NULL is zvx_synthesize.  Queued calls stay queued: the control
 * arrays travel in the call's one input upload (pinned staging) and may be reused as soon as the call returns. */
zvx_status zvx_synthesize_ex(zvx_ctx* ctx, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration,
                             const int32_t* T, int B, int Tmax, const float* spk, const int32_t* pad_to,
                             int Lmax_cap, void* wav, int64_t wav_stride, int32_t* mel_len,
                             float* mel_out, int Lstride, float* log_duration, int flags, const zvx_prosody* prosody);

/* Host side of ZVX_HOST_ASYNC: blocks until the waveform copy into `slot` (0 / 1) has landed, then hands out the slot's pinned rows:
 * *rows -> [*nrows][*stride] samples (f32, or int16 for a ZVX_PCM16 call), the first *valid samples of a row defined as for zvx_vocode
 * (mel_len[b]*hop samples, then zeros up to max_b).  Any out pointer may be NULL.  The memory belongs to the context (freed by
 * zvx_destroy, reused by the second next ZVX_HOST_ASYNC call).  ZVX_E_STATE if no call has used the slot.
 * Replaces the `.cpu().numpy()` hand-over of ZeroVoxTTS.tts_ex (synthesize.py:233-239) for a host that keeps calls in flight. */
zvx_status zvx_wait_host(zvx_ctx* ctx, int slot, const void** rows, int64_t* stride, int32_t* nrows, int64_t* valid);

/* Sample-rate conversion on the device: in [B][Nmax] f32 with nsamples[b] valid samples at rate_in -> row b of out: out_len[b] =
 * ceil(nsamples[b] * L / M) samples at rate_out, then zeros up to max_b out_len[b]; nothing beyond that is touched.  out_stride samples
 * between rows (ZVX_E_BUFFER if smaller than the longest row); float rows, or int16 rows with ZVX_PCM16; out_len may be NULL.
 * The filter, with g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, mx = max(L, M), half = 10 mx, fc = 1 / mx, m = -half .. half:
 *     w[m] = I0(5 sqrt(1 - (m / half)^2)) / I0(5)                 (Kaiser window, beta = 5)
 *     h[m] = fc sinc(fc m) w[m];  h /= sum(h);  h *= L             (sinc(x) = sin(pi x) / (pi x))
 *     y[n] = sum_k h[n M - k L] x[k],  x = 0 outside the given samples
 * -- what scipy.signal.resample_poly(x, L, M) computes with its defaults (stop band about -54 dB).  The taps are designed in double on the
 * host, rounded once to f32 and cached in the context per (L, M); the sum of one output runs in f32 over its ceil((2 half + 1) / L) taps in one
 * fixed order, so an output sample's bits depend on nothing but (L, M) and the samples under the filter: not on the batch, the row's
 * neighbours or the window of zvx_resample_ex.  Rates outside [4000, 192000]: ZVX_E_INVALID; mx > 640: ZVX_E_UNSUPPORTED (the message
 * names L and M; every pair between 22050 and 8000 / 11025 / 12000 / 16000 / 24000 / 32000 / 44100 / 48000 is inside).  Equal rates: a copy.
 * ZVX_PCM16: (int16) trunc(clamp(v * 32760, -32768, 32767)) -- clamped, because a band-limited interpolation of samples in [-1, 1]
 * overshoots (a full-scale 300 Hz square wave reaches 1.28 after 22050 -> 48000).
 * Flags: ZVX_DEVICE_IN (in on the device), ZVX_DEVICE_OUT, ZVX_NO_SYNC (device output only), ZVX_PCM16.  nsamples / out_len are host arrays.
 * Replaces librosa.load(sr=...) of ZeroVoxTTS.get_speakerref (synthesize.py:112-121) and any host-side conversion of a finished waveform. */
zvx_status zvx_resample(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out,
                        void* out, int64_t out_stride, int32_t* out_len, int flags);
/* The same filter over a window, so that a stream converts piece by piece and comes out bit-identical to one whole-signal call: row b
 * holds samples [in_origin, in_origin + nsamples[b]) of a signal that is zero everywhere else; outputs [out_begin, out_begin + out_count)
 * go to positions [0, out_count) of the row.  out_count = -1: to the end, ceil((in_origin + nsamples[b]) * L / M) - out_begin outputs for
 * row b, zeros up to the longest row; out_len (may be NULL) receives the per-row counts.  zvx_resample is origin 0, begin 0, count -1. */
zvx_status zvx_resample_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out,
                           void* out, int64_t out_stride, int32_t* out_len, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count);
/* Output rate: after zvx_set_int(ctx, "out_rate", hz) zvx_vocode, zvx_vocode_mel, zvx_synthesize and zvx_synthesize_ex deliver their rows at
 * hz: the generator writes f32 into a work buffer of the context and the resampler, one more launch on the main stream behind conv_post,
 * writes the caller's rows.  wav_stride, the ZVX_E_BUFFER bound and the `valid` of zvx_wait_host are then in OUTPUT samples: row b carries
 * ceil(mel_len[b] * hop * L / M) samples, then zeros up to the longest row's count; pad_to still only pads the mel.  Each utterance is
 * resampled as a signal of its own length: no filter tap sees padding or a neighbour.  Every flag keeps its meaning (ZVX_PCM16 rows
 * are clamped as above); ZVX_NATIVE_RATE takes one call out of it. */

/* Long-form output: the B padded rows of a batch, in [B][Nmax] f32 with nsamples[b] valid samples, become ONE contiguous row on the device:
 * every row trimmed of its leading and trailing silence, faded at the cuts, with gap[b] zeros behind segment b.
 *     out = segment 0, gap[0] zeros, segment 1, gap[1] zeros, ... segment B-1, gap[B-1] zeros
 * Bounds of row b (the decisions of zerovox_amd.mels.trim_silence, i.e. of librosa.effects.trim, restated so that they are decidable): with
 *   n = nsamples[b], pad = frame / 2 zeros on both sides of the n samples and nf = 1 + (n + 2 pad - frame) / hop frames, frame f covers padded
 *   samples [f hop, f hop + frame);  p[f] = the sum of the squares of its samples ACCUMULATED IN DOUBLE (each f32 sample converted to double
 *   first; any summation order), pmax = max_f p[f], k = 10^(-top_db / 10) computed once on the host in double (top_db converted to double first):
 *   frame f is audio when p[f] > pmax * k (a double compare; no log, no sqrt).  With first / last the first and last audio frame:
 *       begin = max(0, first * hop - keep),   end = min(n, (last + 1) * hop + keep).
 *   A row is left whole (begin = 0, end = n) when top_db <= 0, when n < frame, or when pmax < 1e-20 * frame (the host function's 1e-10 floor on
 *   the RMS); n = 0 gives an empty segment.  No audio frame at all (only possible where k rounds to 1): begin = end = 0, as trim_silence hands
 *   back an empty array.  A frame whose p[f] / (pmax k) lies within 1e-9 of 1 is AMBIGUOUS: either decision is then allowed (the order of
 *   the double summation is not fixed); everywhere else begin / end are defined exactly.
 * Segment b has m = end - begin samples and F = min(fade, m / 2).  Sample i of it is x[begin + i] * g(i), ONE f32 multiply, with
 *       g(i) = (float)(2 i + 1) / (float)(2 F)   for i < F        (one IEEE-correct f32 division: a linear ramp, defined to the bit)
 *       g(i) = g(m - 1 - i)                      for i >= m - F
 *   and no multiply at all -- the input's bits -- in between.
 * Layout (int64, computed on the device): pos[0] = 0, pos[b + 1] = pos[b] + m_b + gap[b]; segment b starts at pos[b]; the gaps are written as
 *   zeros: the call owns every sample in [0, out_len), the trailing gap included; *out_len = pos[B].  Samples in [out_len, out_capacity) are not
 *   touched.  out_len > out_capacity: ZVX_E_BUFFER, nothing at all is written, the message names both numbers, the layout outputs are still filled.
 *   float row, or with ZVX_PCM16 an int16 row by the resampler's rule, (int16) trunc(clamp(v * 32760, -32768, 32767)).
 *   seg_pos[b] = pos[b], seg_begin[b] = begin, seg_len[b] = m_b (host arrays, each may be NULL).
 * Syncs: the bounds, the prefix sum over the B segments and the copy all run on the context's main stream without the host in between; the call
 *   waits ONCE, for the layout (out_len, seg_pos, seg_begin, seg_len) -- a host output row arrives through pinned memory of the context under
 *   that same wait -- as zvx_synthesize waits once for predicted lengths.  With ZVX_DEVICE_IN the rows may be the ZVX_DEVICE_OUT | ZVX_NO_SYNC
 *   output of a synthesis call queued just before on the same context: stream order is the only fence needed.
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): B <= 0, Nmax <= 0, a NULL ctx / in / nsamples / params / out /
 *   out_len (zvx_trim_bounds: begin / end), frame < 2, hop < 1, hop > frame, keep < 0, fade < 0, a negative gap or length, nsamples[b] > Nmax,
 *   out_capacity < 0, unknown flags, top_db not finite.
 * Flags of zvx_join: ZVX_DEVICE_IN (in on the device), ZVX_DEVICE_OUT (out on the device), ZVX_PCM16.  nsamples and gap are host arrays.
 * Stage slot ZVX_T_JOIN, stage tag "post.join" in zvx_tag_stats: algorithmic bytes = samples read (once for the bounds where top_db > 0, once for
 *   the copy) + samples written.
 * Replaces the loop a caller of ZeroVoxTTS.tts writes around it for a paragraph: librosa.effects.trim per sentence, pauses and np.concatenate on
 * the host (the reference has no long-form entry point, synthesize.py:213-239 is one utterance). */
typedef struct zvx_join_params {
    int32_t frame, hop;   /* trim analysis window and step in samples (librosa.effects.trim's 2048 / 512 are the Python defaults) */
    float   top_db;       /* a frame is audio when its power is within top_db of the row's loudest frame; <= 0: no trimming */
    int32_t keep;         /* samples kept outside the detected bounds on either side (clamped to the row) */
    int32_t fade;         /* linear fade-in / fade-out length at every segment edge, samples; 0: none */
} zvx_join_params;

/* per row: [begin[b], end[b]) = the samples zvx_join would keep (host int32 arrays); fade is not looked at.  flags: ZVX_DEVICE_IN */
zvx_status zvx_trim_bounds(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* params,
                           int32_t* begin, int32_t* end, int flags);
/* rows in [B][Nmax] f32, nsamples[b] valid -> ONE row of *out_len samples; gap [B], >= 0, NULL = none */
zvx_status zvx_join(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap,
                    const zvx_join_params* params, void* out, int64_t out_capacity, int64_t* out_len,
                    int64_t* seg_pos, int32_t* seg_begin, int32_t* seg_len, int flags);

/* Loudness: the integrated loudness (ITU-R BS.1770-4 / EBU R128, mono) and the sample peak of every row of a batch, in [B][Nmax] f32 with
 * nsamples[b] valid samples at `rate` Hz, measured on the device; zvx_normalize also applies the gain that brings a row (or the whole batch
 * as one programme) to a target.  Nothing is normalised unless one of these two is called.  Every decision is made in the power domain, in
 * double, so that it is decidable the way the trim bounds are.
 * K-weighting, fs = rate, coefficients designed on the host in double and cached per rate:
 *   stage 1, high shelf: f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *       Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;  b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],
 *       a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0;
 *   stage 2, high pass: f0 = 38.13547087602444, Q = 0.5003270373238773;  b = [1, -2, 1], a1 = 2 (K^2 - 1) / (1 + K / Q + K^2),
 *       a2 = (1 - K / Q + K^2) / (1 + K / Q + K^2)
 *   (at 48 kHz the table of BS.1770-4: 1.53512486, -2.69169619, 1.19839281 / -1.69065929, 0.73248077 / -1.99004745, 0.99007225).
 *   Each stage is a transposed direct form II in DOUBLE on the f32 samples converted to double:  y = b0 x + s1;  s1 = b1 x - a1 y + s2;
 *   s2 = b2 x - a2 y;  stage 1 feeds stage 2; the state is zero at sample 0 of the row (the signal is zero before it).
 * Units, blocks, gates: h = (fs + 5) / 10 samples (integer: 100 ms), U = n / h whole units (a shorter tail is not measured), u[q] = the
 *   double sum of y^2 over samples [q h, (q + 1) h); block j = 0 .. U - 4 has z[j] = (u[j] + u[j + 1] + u[j + 2] + u[j + 3]) / (4 h).
 *   Absolute gate: z[j] > 10^((-70 + 0.691) / 10) (computed once on the host in double); Gamma = the mean of z over the blocks that pass it;
 *   relative gate: z[j] > 0.1 Gamma (-10 LU is exactly a factor 0.1 in power);  L = -0.691 + 10 log10(mean of z over the blocks that pass
 *   both).  No block (n < 4 h) or none above the absolute gate: L = -INFINITY.  peak = max |x[i]| over the n samples, exact.
 *   A block whose z lies within a relative 2.3e-4 (1e-3 LU) of either threshold is AMBIGUOUS: either decision is allowed there; L is otherwise
 *   defined to within 1e-7 LU of the sequential double recurrence.  (An implementation may start a unit's recurrence from zero state some
 *   way before the unit instead of carrying state, provided it stays within that figure: this one starts two units, 0.2 s, early, which
 *   leaves 1e-12 dB.)
 * Gain, in double on the device, rounded once to f32: g = 10^((target - L) / 20); g = min(g, 10^(max_gain_db / 20)); then, if peak_ceiling > 0
 *   and peak g > peak_ceiling, g = peak_ceiling / peak.  L = -INFINITY or peak = 0: g = 1.  Output sample i is x[i] * g, ONE f32 multiply;
 *   with ZVX_PCM16 the resampler's rule follows, (int16) trunc(clamp(v * 32760, -32768, 32767)).
 *   ZVX_LOUD_COMMON: both gates run over the union of all rows' blocks (blocks never span two rows), peak is the maximum over the rows, ONE g
 *   is computed and gain[b] = g for every row; lufs[b] / peak[b] still report the per-row values.
 * Syncs: measurement, gates, gain and multiply run on the context's main stream without the host in between; the call waits once, for the
 *   host outputs.  With ZVX_DEVICE_OUT | ZVX_NO_SYNC and lufs == peak == gain == NULL zvx_normalize only queues.  With ZVX_DEVICE_IN the rows
 *   may be the output of a synthesis call queued just before on the same context: stream order is the fence, as for zvx_join.
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): a NULL ctx / in / nsamples (zvx_normalize: params / out),
 *   B <= 0, Nmax <= 0, a negative length, nsamples[b] > Nmax, rate outside [4000, 192000], out_stride < Nmax, unknown flags, ZVX_NO_SYNC
 *   without ZVX_DEVICE_OUT, ZVX_PCM16 with out == in, out == in with another stride or on another side than in, target_lufs not finite or
 *   outside [-70, 0], max_gain_db not finite or negative, peak_ceiling NaN, an unknown mode.  More than 65535 rows: ZVX_E_UNSUPPORTED.
 * Stage tag "post.loudness" in zvx_tag_stats (one timed group per call; no stage slot): algorithmic bytes = 4 sum(n) for the measurement;
 *   zvx_normalize adds 4 sum(n) read and the bytes written.
 * Replaces a host-side meter and gain (pyloudnorm and the like) behind ZeroVoxTTS.tts; the reference hands its waveform back at whatever
 * level the model gives (synthesize.py:213-239).  True-peak metering and a limiter: zvx_true_peak / zvx_limit below.  Not here: momentary /
 * short-term loudness, several channels. */
enum { ZVX_LOUD_PER_ROW = 0, ZVX_LOUD_COMMON = 1 };
typedef struct zvx_loudness_params {
    float   target_lufs;   /* integrated loudness to reach, finite, in [-70, 0] */
    float   peak_ceiling;  /* linear sample-peak ceiling after the gain (0.891 = -1 dBFS); <= 0: none */
    float   max_gain_db;   /* upper bound on the gain in dB, finite, >= 0 (keeps a near-silent row from being blown up) */
    int32_t mode;          /* PER_ROW: each row its own gain; COMMON: one gain from all rows measured as one programme */
} zvx_loudness_params;

/* measure: lufs[B] (double; -INFINITY where undefined), peak[B] (float) -- host arrays, either may be NULL.  flags: ZVX_DEVICE_IN */
zvx_status zvx_loudness(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                        double* lufs, float* peak, int flags);
/* measure + gain: row b of out receives nsamples[b] samples x[i] * gain[b]; nothing else is touched.  out_stride samples between rows;
 * out == in (same stride) is allowed for float rows: in place.  lufs / peak / gain: host arrays, each may be NULL.
 * flags: ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only), ZVX_PCM16 (not in place) */
zvx_status zvx_normalize(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                         const zvx_loudness_params* params, void* out, int64_t out_stride,
                         double* lufs, float* peak, float* gain, int flags);

/* Programme loudness report: what a delivery specification (EBU R128 / Tech 3342 and the platform variants) asks for next to the integrated
 * loudness -- maximum momentary and short-term loudness and the loudness range (LRA) -- for every row of a batch, on the device, from the
 * measurement zvx_loudness makes (the block above defines K-weighting, units, blocks and the integrated gates; momentary and short-term
 * loudness, "not here" for that call, are here).  For a row of n samples, h = (rate + 5) / 10 and U = n / h:
 * Units: u[q] are exactly zvx_loudness's: the same launch, zero state two units early, the same fma chain.
 * Momentary: z[j], j = 0 .. U - 4, exactly zvx_loudness's block, (((u[j] + u[j + 1]) + u[j + 2]) + u[j + 3]) / (4 h);
 *   M[j] = -0.691 + 10 log10 z[j] in double, -INFINITY where z[j] == 0;  stats[MOMENTARY_MAX] = max_j M[j], -INFINITY where U < 4.
 * Short-term: s[j] = (u[j] + ... + u[j + 29]) / (30 h), j = 0 .. U - 30, summed in ascending index in double; S[j] is its LUFS value as for
 *   M[j];  stats[SHORT_MAX] = max_j S[j], -INFINITY where U < 30.
 * Integrated and peak: stats[INTEGRATED] and stats[PEAK] are bit for bit the lufs[b] and (double) peak[b] zvx_loudness gives on the same rows.
 * LRA (EBU Tech 3342) over the short-term windows: absolute gate s[j] > 10^((-70 + 0.691) / 10), zvx_loudness's constant; Gamma = the mean
 *   of s over the windows that pass it; relative gate s[j] > 0.01 Gamma (-20 LU is exactly a factor 0.01 in power); n_g = the number of
 *   windows that pass both, k[0 .. n_g) their powers sorted ascending;  s_lo = k[((n_g - 1) * 10 + 50) / 100] and
 *   s_hi = k[((n_g - 1) * 95 + 50) / 100], integer divisions (Tech 3342's nearest rank round((n - 1) p / 100));  LRA_LOW and LRA_HIGH are
 *   the LUFS values of s_lo and s_hi, LRA = 10 log10(s_hi / s_lo), SHORT_GATED = (double) n_g.  n_g == 0: LRA = 0, both bounds -INFINITY.
 *   A window whose s lies within a relative 2.3e-4 of either gate is AMBIGUOUS, as for zvx_loudness: either decision is allowed.
 *   Every figure and every curve entry lies within 1e-7 LU of the sequential double recurrence; INTEGRATED and PEAK are exact as above; n_g
 *   is exact wherever no window is ambiguous.
 * Curves: entries [0, U - 3) of momentary[b] and [0, U - 29) of short_term[b] are written, nothing else is touched;
 *   curve_stride >= max(1, Nmax / h - 3) doubles between rows is required when either curve is asked for.
 * Rows are independent.  n == 0 gives -INFINITY for every loudness, LRA = 0, SHORT_GATED = 0, PEAK = 0.  Non-finite input: zvx_vocode_mel's
 *   rule -- the call succeeds, that row is unspecified, every other row keeps its bits.
 * Launches: zvx_loudness's two, unchanged; one workgroup per row that forms s[j] into a work buffer of the context, writes the curves into
 *   device staging, reduces the maxima and runs both gates as fixed-order sums; and a selection without a sort: thread j counts the gated
 *   windows i with s[i] < s[j], or s[i] == s[j] and i < j, streaming s through LDS tiles, and the one thread whose count is a target rank
 *   stores its power (ties break by index: no atomics, no workgroup that waits for another).  The three logarithms of the two selected
 *   powers are taken on the host.  The call waits once, for the host outputs.
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): every check zvx_loudness makes, a NULL stats, a
 *   curve_stride that is negative or too small while a curve is asked for, any flag but ZVX_DEVICE_IN.  ZVX_E_UNSUPPORTED: more than 65535
 *   rows; a row of more than 65536 units (the selection is quadratic in the window count: the cap bounds it at about 1.8 h per row).
 * Stage tag "post.loudness" (one timed group per call): algorithmic bytes = 4 sum(n).
 * Replaces a host-side meter (pyloudnorm and the like) behind ZeroVoxTTS.tts / tts_long(..., report=True).  Not here: several channels, a
 * windowed or streaming form, target checks (zerovox_amd.report.LoudnessReport.meets does those in Python). */
enum { ZVX_LS_INTEGRATED = 0, ZVX_LS_MOMENTARY_MAX, ZVX_LS_SHORT_MAX, ZVX_LS_LRA, ZVX_LS_LRA_LOW, ZVX_LS_LRA_HIGH,
       ZVX_LS_SHORT_GATED, ZVX_LS_PEAK, ZVX_LS_COUNT = 8 };
zvx_status zvx_loudness_stats(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                              double* stats,        /* host [B][ZVX_LS_COUNT], required */
                              double* momentary,    /* host [B][curve_stride] or NULL: M[j] in LUFS */
                              double* short_term,   /* host [B][curve_stride] or NULL: S[j] in LUFS */
                              int64_t curve_stride, int flags /* ZVX_DEVICE_IN only */);

/* Pitch report: the fundamental frequency (F0) track of every row of a batch on a frame grid, and its statistics, measured on the device --
 * the meter of the prosody controls (pitch_shift, pitch_range, pitch_target act in the model's bucket units; this reads the audio they
 * made).  Rows in [B][Nmax] f32 with nsamples[b] valid samples at `rate` Hz.  The estimator is YIN (de Cheveigne and Kawahara 2002, steps
 * 1 to 5), restated so that every decision is decidable the way the gates of zvx_loudness are.
 * Setup, per row of n samples at fs = rate: tau_min = max(2, floor(fs / fmax)) and tau_max = ceil(fs / fmin), both formed on the host in
 *   double;  c = (W + tau_max) / 2 (integer division);  F = n / H frames (integer division: with H = the model's hop and a synthesised
 *   waveform of mel_len * hop samples a frame is a mel frame).
 * Per frame f < F, with s = f H - c, so that frame f is centred on sample f H:
 *   Samples: v[j] = (double) x[s + j], 0 <= j < W + tau_max; samples outside [0, n) are zero; nothing outside the row is read.
 *   Power gate: P = (sum_{j < W} v[j]^2) / W; the frame is voiced only if P > 10^(gate_db / 10) (computed once on the host in double).
 *   Difference: d[tau] = sum_{j < W} (v[j] - v[j + tau])^2, tau = 1 .. tau_max, in double, in any summation order.
 *   Normalisation: c[tau] = d[1] + ... + d[tau];  d'[tau] = d[tau] tau / c[tau] where c[tau] > 0, otherwise 1.
 *   Pick: T = the smallest tau in [tau_min, tau_max] with d'[tau] < threshold; none: the frame is unvoiced.  Otherwise descend: while
 *     T + 1 <= tau_max and d'[T + 1] < d'[T], T = T + 1.
 *   Refinement, where T - 1 >= 1 and T + 1 <= tau_max: a = d'[T - 1], b = d'[T], e = d'[T + 1], den = a - 2 b + e; if den > 0 and
 *     |(a - e) / (2 den)| <= 1 then delta = (a - e) / (2 den), otherwise (and without both neighbours) delta = 0;
 *     f0 = fs / (T + delta) in double, rounded once to f32.
 *   Outputs: f0[b][f] = that value, 0 for an unvoiced frame;  aper[b][f] = d'[T] for a voiced frame, otherwise the minimum of d' over
 *     [tau_min, tau_max], rounded to f32.
 *   A frame is AMBIGUOUS, and either decision is allowed, when P lies within a relative 1e-9 of the gate, any d'[tau] in
 *     [tau_min, tau_max] within a relative 1e-9 of the threshold, or two neighbours compared during the descent within a relative 1e-9
 *     of equality.  Every term of d is non-negative, so the summation order moves d' by about W 2^-53, far inside that band.
 *   Elsewhere f0 and aper lie within one f32 ulp (a relative 6e-8) of the sequential double sums; measured on an MI355X against
 *     tests/pitch_ref.py (tests/test_pitch_gpu.py): a largest relative deviation of 0, every f32 bit equal.
 * Statistics, in double: FRAMES = F;  VOICED = n_v, the number of voiced frames;  k[0 .. n_v) the voiced f0 sorted ascending and, nearest
 *   rank with integer divisions as for LRA, MEDIAN = k[((n_v - 1) * 50 + 50) / 100], LOW = k[((n_v - 1) * 5 + 50) / 100],
 *   HIGH = k[((n_v - 1) * 95 + 50) / 100];  MEAN = the mean of the voiced f0.  n_v == 0: all four are 0.
 * Rows are independent: a row's bits depend neither on B, nor on Nmax, nor on its neighbours.  n < H gives F = 0 and writes nothing for that
 *   row; only entries [0, F) of a curve row are written.  Non-finite input: zvx_vocode_mel's rule -- the call succeeds, that row is
 *   unspecified, every other row keeps its bits.
 * Launches: one workgroup of 256 lanes per run of G consecutive frames of a row (G <= 8, chosen from H, W and tau_max alone) stages their
 *   (G - 1) H + W + tau_max samples once in LDS as doubles; lane l owns the lags l + 1, l + 257, ..., each with its own double accumulator;
 *   d goes to LDS, an inclusive scan forms c, the first crossing is a minimum-index reduction, one lane descends and refines.  Then one
 *   workgroup per row forms n_v and the mean in a fixed order, and zvx_loudness_stats's selection without a sort (rank counts, ties broken
 *   by index) picks the three ranks.  No atomics, no workgroup that waits for another.  The call waits once, for the host outputs.
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): the checks zvx_loudness_stats makes on ctx / in /
 *   nsamples / B / Nmax / lengths / rate / flags; a NULL params or stats; fmin, fmax, threshold or gate_db not finite or outside the ranges
 *   below; tau_max < tau_min + 2; window < 2 or hop < 1; f_stride < max(1, Nmax / hop) while a curve is asked for.
 *   ZVX_E_UNSUPPORTED: more than 65535 rows; window > 4096 or tau_max > 2048 (the LDS plan: 6144 staged doubles and 8 lags per lane; the
 *   defaults of Context.pitch -- 60 .. 500 Hz, window = 2 tau_max -- fit from 4 kHz to 122 kHz: tau_max = 800, W = 1600 at 48 kHz); a row
 *   of more than 65536 frames (zvx_loudness_stats's bound, for the same quadratic selection).
 * Stage tag "post.pitch" (one timed group per call): algorithmic bytes = 4 sum(n).
 * Not here: a windowed or streaming form, octave-jump smoothing across frames (pYIN), the normalisation of Hz into pitch_target's [0, 1]
 * (zerovox_amd.pitch.per_phoneme gives the per-phoneme Hz it starts from), a speaker-similarity figure. */
typedef struct zvx_pitch_params {
    float   fmin, fmax;   /* search range in Hz, finite, 0 < fmin < fmax */
    float   threshold;    /* absolute threshold on d', in (0, 1] (0.15 is YIN's) */
    float   gate_db;      /* a frame whose mean power is not above 10^(gate_db / 10) is unvoiced; finite, <= 0 */
    int32_t window;       /* W: samples integrated per lag, >= 2 */
    int32_t hop;          /* H: samples between frames, >= 1 */
} zvx_pitch_params;
enum { ZVX_PS_FRAMES = 0, ZVX_PS_VOICED, ZVX_PS_MEDIAN, ZVX_PS_LOW, ZVX_PS_HIGH, ZVX_PS_MEAN, ZVX_PS_COUNT = 6 };
zvx_status zvx_pitch(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                     const zvx_pitch_params* params,
                     float* f0,       /* host [B][f_stride] or NULL: Hz, 0 = unvoiced */
                     float* aper,     /* host [B][f_stride] or NULL: d' at the pick */
                     int64_t f_stride, int32_t* frames /* host [B] or NULL */,
                     double* stats    /* host [B][ZVX_PS_COUNT], required */, int flags /* ZVX_DEVICE_IN only */);

/* True-peak metering and a look-ahead limiter for rows in [B][Nmax] f32 with nsamples[b] valid samples at `rate` Hz.  Rows are independent;
 * nothing sees a neighbouring row or the padding.  The algorithm has finite support and no recurrence, so it is defined to the bit where
 * the other post-processing is.  Per row of n samples:
 * Oversampled signal: y[m], m < os n, is what zvx_resample computes for (L, M) = (os, 1): the same taps (half = 10 os, 21 per output), the
 *   same f32 sum in the same order, x = 0 outside the row.  The bank depends on (L, M) only -- `rate` does not enter it, so os * rate may
 *   exceed 192000.  y is never written to memory.  os = 1 uses no filter at all.
 * Envelope (f32): e[i] = max(|x[i]|, |y[m]| for os (i - 1) < m < os (i + 1), 0 <= m < os n): an inter-sample peak between i and i + 1
 *   counts for both neighbours.  os = 1: e[i] = |x[i]|.
 * Depth, in double: d[i] = e[i] > c ? 1 - (double) c / (double) e[i] : 0;  r[i] = 1 - d[i].
 * Hold: D[i] = the maximum of d[j] over |j - i| <= W, 0 <= j < n (exact: any order).
 * Smooth: w[k] = (1 + cos(pi k / (W + 1))) / (2 (W + 1)), k = -W .. W, designed on the host in double, divided by their own sum (in exact
 *   arithmetic they sum to 1 already) and cached per W;  s[i] = 1 - sum_k w[k] D[clamp(i + k, 0, n - 1)], a double sum (one fma per term, from 0) in
 *   ascending k = -W .. W -- the order is part of the contract: it is what makes the windows of zvx_limit_ex concatenate to the bit.
 * Gain: g[i] = min(s[i], r[i]);  g32[i] = g[i] rounded toward zero to f32;  out[i] = x[i] * g32[i], ONE f32 multiply; with ZVX_PCM16 the
 *   resampler's rule follows.
 * What follows from that:
 *   (a) the ceiling holds exactly: |out[i]| <= c, no tolerance.  Every D under the sum has i in its window, so s <= r up to rounding; the
 *       min and the rounding toward zero remove the rest, and c is an f32.
 *   (b) untouched samples keep their bits: where no e[j] > c within 2 W of i every term is exactly 0, g32 = 1 and out[i] has the bits of
 *       x[i]; a row that never exceeds the ceiling passes through bit for bit.
 *   (c) the TRUE peak after limiting is not an exact guarantee: the gain is applied at the base rate, so the oversampled output only stays
 *       near c.  Measured by the float64 reference (tests/test_limiter.py: speech-like rows at a peak of 1.6, c = 0.891, os = 4): at most
 *       0.0033 dB over c with a 1 ms window (W = 22 at 22.05 kHz: 0.00321 dB) and below 1e-4 dB with 5 ms (W = 110: 0.000024 dB); with
 *       os = 1 (sample peaks only) the same rows end up to 3.0 dB over it.
 *   (d) non-finite input: the call succeeds and nothing faults; that row is unspecified, every other row is bit for bit what it is without
 *       it (zvx_vocode_mel's rule).
 *   (e) n = 0 writes nothing (peak_in = 0, min_gain = 1); n <= W is legal: the clamped index handles it.
 * zvx_true_peak: tpeak[b] = max_i e[i] = max(max_i |x[i]|, max_m |y[m]|); 0 for an empty row.
 * Launches: the envelope (a tile plus a halo of 10 / 11 samples staged in LDS) into a work buffer of the context; hold, smooth, gain and
 *   multiply over a tile plus a halo of 2 W envelope samples in LDS -- it reads the envelope, never a neighbour's x, so out == in is safe --;
 *   a reduction per row.  Lengths are read on the device, nothing syncs in between.
 * Syncs: as for zvx_normalize -- the call waits once, for the host outputs; with ZVX_DEVICE_OUT | ZVX_NO_SYNC and peak_in == min_gain == NULL
 *   zvx_limit only queues; with ZVX_DEVICE_IN the rows may be the output of a zvx_synthesize / zvx_normalize call queued just before on the
 *   same context.  (The first use of an oversampling factor or of a window W uploads its table and waits for that once.)
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): a NULL ctx / in / nsamples / params / out (zvx_true_peak:
 *   tpeak), B <= 0, Nmax <= 0, a negative length, nsamples[b] > Nmax, out_stride < Nmax, rate outside [4000, 192000], unknown flags,
 *   ZVX_NO_SYNC without ZVX_DEVICE_OUT, ZVX_PCM16 with out == in, out == in with another stride or on another side than in, a ceiling that
 *   is not finite or outside (0, 8], a window_ms that is not finite or <= 0, an oversample outside {1, 2, 4, 8}.  ZVX_E_UNSUPPORTED: more
 *   than 65535 rows, W > 4096.
 * Stage tag "post.limit" in zvx_tag_stats (one timed group per call; no stage slot): algorithmic bytes = 4 sum(n) for zvx_true_peak;
 *   4 sum(n) read plus the bytes written for zvx_limit and zvx_limit_ex (4 or, with ZVX_PCM16, 2 per emitted sample).
 * Replaces a host-side true-peak meter and limiter behind zvx_normalize, whose gain a sample-peak ceiling otherwise bounds. */
typedef struct zvx_limit_params {
    float   ceiling;     /* linear ceiling c, finite, 0 < c <= 8 (0.891 = -1 dBFS) */
    float   window_ms;   /* W = max(1, rint(rate * window_ms / 1000)), on the host in double; W > 4096: ZVX_E_UNSUPPORTED */
    int32_t oversample;  /* os: 1 = sample peaks, 2 / 4 / 8 = true-peak detection */
} zvx_limit_params;

/* tpeak[b] (host float[B]) = max(max_i |x[i]|, max_m |y[m]|), y = the os-times oversampled row.  flags: ZVX_DEVICE_IN */
zvx_status zvx_true_peak(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, int oversample,
                         float* tpeak, int flags);
/* out row b = x[i] * g32[i]; peak_in[b] = max_i e[i], min_gain[b] = min_i g32[i] (host arrays, each may be NULL).
 * flags: ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only), ZVX_PCM16 (not in place); out == in (same stride) allowed for f32 */
zvx_status zvx_limit(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                     const zvx_limit_params* params, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags);
/* The same limiter over a window, so that a stream is limited piece by piece and comes out bit-identical to one whole-signal call (as
 * zvx_resample_ex converts one).  Row b holds samples [in_origin, in_origin + nsamples[b]) of a signal x that starts at sample 0; with
 * last != 0 x ends at N_b = in_origin + nsamples[b], with last == 0 it continues past the window.  The outputs [out_begin, out_begin + cnt_b)
 * of zvx_limit on the WHOLE signal go to positions [0, cnt_b) of out row b; nothing else in out is touched.  cnt_b = out_count; with
 * out_count == -1, which needs last, cnt_b = in_origin + nsamples[b] - out_begin (to the end of the row's signal; none where that is <= 0).
 * Reach: R = 2 W + H, H = 11 for oversample > 1 and H = 0 for oversample 1: e[j] reads x[j - 11 .. j + 11], hold and smoothing reach W each.
 * Support condition, per row with cnt_b > 0 (otherwise ZVX_E_INVALID; the message names the row, R and the missing samples):
 *     in_origin <= out_begin  and  out_begin + cnt_b <= in_origin + nsamples[b];
 *     left:  in_origin == 0  or  out_begin - R >= in_origin;
 *     right: last  or  out_begin + cnt_b - 1 + R <= in_origin + nsamples[b] - 1.
 *   Under it no emitted sample sees a cut edge: the clamps at 0 and N - 1 and the zeros outside the row are then the true signal's.
 * Results: the emitted samples are bit for bit those of zvx_limit on the whole signal (f32, and int16 with ZVX_PCM16): the oversampled
 *   sums run in the fixed tap order, the hold is an exact maximum and the smoothing sum runs in ascending k whatever the window.
 *   peak_in[b] = max e[i] and min_gain[b] = min g32[i] over the EMITTED range only, so the max / min over a stream's pieces are the whole
 *   call's values; an empty range writes nothing and gives 0 and 1.
 * zvx_limit is zvx_limit_ex(..., 0, 0, -1, 1).  Validation: every check of zvx_limit (out_stride >= Nmax included), and ZVX_E_INVALID for a
 *   negative in_origin or out_begin, out_count < -1, out_count == -1 without last, last outside {0, 1}, out_stride smaller than the
 *   longest cnt_b, out == in unless out_begin == in_origin (then zvx_limit's in-place conditions apply).  Flags, syncs, the queued form,
 *   the non-finite rule and the "post.limit" tag are zvx_limit's; `last` is a parameter, not a flag bit.
 * A stream: zerovox_amd/limiter.py plans the windows -- a non-last push emits up to received - R, the last one everything, the history
 *   before next_out - R is dropped -- so a limited stream runs R samples behind its input (231 samples for 5 ms at 22.05 kHz, os 4). */
zvx_status zvx_limit_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                        const zvx_limit_params* params, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags,
                        int64_t in_origin, int64_t out_begin, int64_t out_count, int last);

/* Vocoder-bias denoiser: spectral subtraction of the vocoder's own constant hum from rows in [B][Nmax] f32 with nsamples[b] valid samples at
 * the model's rate.  The vocoder is run on a silent mel, the magnitude spectrum of what it emits is the bias, and a multiple of it is taken
 * off the magnitude of every STFT frame of real output, the phase kept (NVIDIA's WaveGlow / HiFi-GAN inference scripts: --denoising-strength).
 * Whether this is audible on a real checkpoint is NOT measured here: the arithmetic is pinned against a float64 restatement, nothing more.
 * With n_fft, hop, win_length the model's mel parameters, nf = n_fft / 2 + 1, pad = (n_fft - hop) / 2, per row of n samples:
 * Framing: exactly zvx_melspec's.  xp = the row reflect-padded by pad on both sides; F = 1 + (n + 2 pad - n_fft) / hop frames; frame f covers
 *   xp[f hop .. f hop + n_fft); w[t] = the periodic Hann of win_length centred in n_fft (the window inside mel.dft), designed in double on
 *   the host; the transforms use it rounded once to f32.
 * Analysis:  X[f][k] = sum_t w[t] xp[f hop + t] e^(-2 pi i k t / n_fft), k < nf.
 * Gain (f32): m = sqrtf(re^2 + im^2);  G = m > 0 ? fmaxf(floor, 1 - strength * bias[k] / m) : floor;  X' = G X -- spectral subtraction of
 *   strength * bias from the magnitude with the phase kept; no atan2.
 * Synthesis: y_f[t] = (1 / n_fft) sum_k c_k Re(X'[f][k] e^(+2 pi i k t / n_fft)), c_0 = c_(n_fft / 2) = 1, otherwise c_k = 2; the imaginary
 *   parts of DC and Nyquist are ignored.
 * Overlap-add, for padded position p = i + pad:  num[p] = sum_f w[p - f hop] y_f[p - f hop] (f32, from +0),  den[p] = sum_f w[p - f hop]^2
 *   (from the DOUBLE window, summed in double, rounded once to f32), both over the frames f < F that cover p in ASCENDING f -- the order is
 *   part of the contract, as in the limiter's smoothing sum.  out[i] = num / den, one f32 division, where den[p] (the double sum) >= 1e-3 *
 *   max_t sum_j w[t + j hop]^2; elsewhere out[i] = x[i], the input's bits.  At 1024 / 256 every sample is covered; the rule serves other
 *   configurations.  With ZVX_PCM16 the resampler's rule follows.
 * Exact corners: strength == 0 is a copy (the bits of x, nothing is transformed, as equal rates in zvx_resample).  Where every G under a
 *   sample is 0, out[i] == +0.0f exactly.  Rows are independent: a row's bits depend on its own samples, bias, strength and floor only, not
 *   on B, Nmax or a neighbour.  Non-finite input: zvx_vocode_mel's rule (that row unspecified, nothing faults, the others untouched).
 *   out == in (f32, same stride) is allowed: the overlap-add reads the frame buffer, and x only at its own index.  n == 0 writes nothing.
 * The error against the float64 restatement is that of an f32 FFT pair: measured at most 2.5e-7 on rows with |x| <= 1 (1024 / 256;
 *   tests/test_denoise_gpu.py holds 4x that).
 * Launches: one launch loads, windows and transforms the frames -- an FFT in LDS, several frames per workgroup, twiddles from a table
 *   designed in double, rounded once and cached in the context like the resampler's taps --, applies the gain, transforms back and stores
 *   w[t] y_f[t] into a work buffer of the context (F n_fft f32 per row, 4x the audio at 1024 / 256); no spectrum goes to memory.  A second
 *   launch is the gather-form overlap-add.  Lengths are read on the device.
 * Bias: zvx_denoise_bias runs the context's vocoder, at the native rate and under the current precision switches, on 88 all-zero mel frames
 *   (what zvx_vocode_mel hands back for them), frames the 88 hop samples as above, and bias[k] = the mean over ALL frames of |X[f][k]|,
 *   accumulated in double and rounded once to f32.  NVIDIA's script takes frame 0 alone; the mean does not hinge on one reflect-padded
 *   frame.  Recompute it after a switch that changes the vocoder's arithmetic ("voc_f16", "voc_f16_stages").  The call waits for the bias.
 * Flags, syncs, validation: the rows-call contract as zvx_limit uses it.  ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only),
 *   ZVX_PCM16 (not in place); with ZVX_DEVICE_OUT | ZVX_NO_SYNC the call only queues (the first call of a context uploads its tables and
 *   waits for that once).  bias is a HOST array [nf]; it travels through pinned staging and may be reused when the call returns.
 *   ZVX_E_INVALID, before anything is queued, the context stays usable: every check of zvx_limit on ctx / in / nsamples / out / B / Nmax /
 *   lengths / out_stride / flags / in-place use; a NULL bias or params; a strength that is not finite or negative; a floor outside [0, 1]; a
 *   bias entry that is negative or NaN; a row with 0 < n that fails zvx_melspec's length conditions (n >= pad + 1 and n + 2 pad >= n_fft:
 *   the message names the row and the minimum).  ZVX_E_UNSUPPORTED: n_fft not a power of two, below 4 or above 4096; more than 65535 rows.
 * Stage tag "post.denoise" in zvx_tag_stats (one timed group per call; no stage slot): algorithmic bytes = 4 sum(n) read plus the bytes
 *   written.  zvx_get_int("fft_size") gives n_fft.
 * Replaces a host-side torch.stft / istft round trip between the vocoder and zvx_normalize / zvx_limit. */
typedef struct zvx_denoise_params {
    float strength;   /* finite, >= 0: the multiple of the bias taken off every magnitude (0: a copy) */
    float floor;      /* in [0, 1]: the smallest gain of a bin */
} zvx_denoise_params;
/* bias: host [nf] */
zvx_status zvx_denoise_bias(zvx_ctx* ctx, float* bias);
/* out row b = the denoised nsamples[b] samples of in row b; nothing else is touched.  out_stride samples between rows.
 * flags: ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only), ZVX_PCM16 (not in place); out == in (same stride) allowed for f32 */
zvx_status zvx_denoise(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                       const zvx_denoise_params* params, void* out, int64_t out_stride, int flags);
/* The same denoiser over a window, so that a stream is denoised piece by piece and comes out bit-identical to one whole-signal call (as
 * zvx_limit_ex limits one).  Row b holds samples [in_origin, in_origin + nsamples[b]) of a signal x that starts at sample 0; with
 * last != 0 x ends at N_b = in_origin + nsamples[b], with last == 0 it continues past the window.  The outputs [out_begin, out_begin + cnt_b)
 * of zvx_denoise on the WHOLE signal go to positions [0, cnt_b) of out row b; nothing else in out is touched.  cnt_b = out_count; with
 * out_count == -1, which needs last, cnt_b = in_origin + nsamples[b] - out_begin (to the end of the row's signal; none where that is <= 0).
 * Frame grid: the whole signal's -- frame f covers padded positions [f hop, f hop + n_fft), i.e. samples [f hop - pad, f hop - pad + n_fft),
 *   whatever in_origin is.  The reflect at sample 0 exists only in a window with in_origin == 0, the reflect at N_b - 1 only with last.  F
 *   comes from N_b with last and is unbounded otherwise.
 * Reach: R = n_fft - 1: a frame that covers sample i begins after i - n_fft and ends before i + n_fft (four frames cover a sample at 1024 /
 *   256; 1023 samples to either side).
 * Support condition, per row with cnt_b > 0 (otherwise ZVX_E_INVALID; the message names the row, R and the missing samples):
 *     in_origin <= out_begin  and  out_begin + cnt_b <= in_origin + nsamples[b];
 *     left:  in_origin == 0  or  out_begin - R >= in_origin;
 *     right: last  or  out_begin + cnt_b - 1 + R <= in_origin + nsamples[b] - 1.
 *   Under it every frame that covers an emitted sample reads inside the window, or in a mirror that is the true signal's.
 * Results: the emitted samples are bit for bit those of zvx_denoise on the whole signal (f32, and int16 with ZVX_PCM16), because (1) a
 *   frame's transform depends on its own n_fft samples only, not on which slot of a workgroup it lands in; (2) the overlap-add runs over the
 *   same frames in ascending f; (3) den comes from the same double table.  (1) is kept by construction, not left to the compiler: a
 *   workgroup holds 4096 / n_fft frames and its unrolled butterfly copies serve different slots, so frame f is always given slot
 *   f mod (4096 / n_fft), the one it has in the whole call -- the work buffer is indexed from the first needed frame rounded down to a
 *   multiple of that, and the slots in front of the first needed frame stay empty.  Only the frames that cover an emitted sample are
 *   transformed.  The den < den_min rule (out = x) uses the whole signal's F, so the uncovered tail of the last window behaves as in the
 *   whole call.  strength == 0 is still a copy, of the emitted range, after the same validation.
 * zvx_denoise is zvx_denoise_ex(..., 0, 0, -1, 1).  Validation: every check of zvx_denoise (out_stride >= Nmax included), and ZVX_E_INVALID
 *   for a negative in_origin or out_begin, out_count < -1, out_count == -1 without last, last outside {0, 1}, out_stride smaller than the
 *   longest cnt_b, out == in unless out_begin == in_origin (then zvx_denoise's in-place conditions apply).  zvx_melspec's length conditions
 *   apply to the whole SIGNAL: they are checked on N_b with last; a window that is not the last needs the support condition only.  Flags,
 *   syncs, the queued form, the non-finite rule and the "post.denoise" tag are zvx_denoise's (bytes: 4 per sample read plus the bytes written
 *   per emitted sample); `last` is a parameter, not a flag bit.  No sample or frame index is formed in 32 bits from an absolute position:
 *   in_origin and out_begin may lie beyond 2^32.
 * A stream: zerovox_amd/denoiser.py plans the windows -- a non-last push emits up to received - R, the last one everything, the history
 *   before next_out - R is dropped -- so a denoised stream runs R samples behind its input (1023 samples, 46 ms, at 1024 / 22.05 kHz).  Each
 *   window transforms again the up to 2 (n_fft / hop) frames that reach into its history; no frame state is carried between calls. */
zvx_status zvx_denoise_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                          const zvx_denoise_params* params, void* out, int64_t out_stride, int flags,
                          int64_t in_origin, int64_t out_begin, int64_t out_count, int last);

/* A window per row: zvx_denoise_rows and zvx_limit_rows are zvx_denoise_ex / zvx_limit_ex with win[b] (a HOST array of B entries) in place of
 * the call's one window, for a caller that holds several signals at different positions -- B streams, each somewhere else on its signal, in
 * ONE call and one launch sequence instead of B.  Row b holds samples [in_origin, in_origin + nsamples[b]) of its signal; the outputs
 * [out_begin, out_begin + cnt_b) go to positions [0, cnt_b) of out row b.  The rows-call contract is the _ex calls': strided rows on the
 * host or on the device, the same flags, syncs and queued form; the denoiser's bias, strength and floor and the limiter's ceiling,
 * window_ms and oversample stay per CALL (the gain launch's LDS layout depends on W).
 * Contract: row b's emitted samples are bit for bit those of the _ex call on that row alone with win[b], and therefore those of the
 *   whole-signal call (f32, and int16 with ZVX_PCM16).  Independently per row: peak_in[b] / min_gain[b] cover the row's emitted range (0 and
 *   1 where it is empty); out_count == -1 needs that row's last; an empty range writes nothing; a row's bits depend neither on which other
 *   rows share the call nor on their windows; nothing outside [0, cnt_b) of an output row is touched.
 * How: the kernels read one row descriptor at their top -- input, output and work-buffer / envelope pointers, length, emitted range, and
 *   for the denoiser origin, first frame, skip, rel and the two mirrors -- and work from it alone.  EVERY call of the denoiser and the
 *   limiter -- whole-row, _ex, _rows, zvx_true_peak, zvx_denoise_bias, the streams' stages -- forms these descriptors on the host and
 *   uploads them as one row table through the context's pinned staging arena, queued like a launch: there is one way to fill a descriptor
 *   and one kernel body, so no two forms can contract a multiply-add differently.  (A table larger than what is left of the 2 MiB arena --
 *   roughly 32 k rows in one call -- goes over as a plain copy that is COMPLETE when it returns: such a call, when queued, waits once;
 *   nothing else about it changes.)  Each denoiser row's first frame is rounded down to
 *   a multiple of 4096 / n_fft on its OWN grid, so a frame keeps the slot it has in the whole call; the signal's frame count is formed in
 *   64 bits from the row's origin; the overlap-add sums in ascending f.  The limiter's envelope runs on each row's own tile grid over its
 *   window, the gain tiles start at the row's own offset, the sums keep their orders.  No index is formed in 32 bits from an absolute
 *   position: a row's in_origin may lie beyond 2^32.  Grids are sized by the longest row; workgroups past a row's extent return at once.
 * Validation, all before anything is queued (ZVX_E_INVALID, the context stays usable): every check of the _ex call, the window's checks and
 *   the support condition per row with the message naming the row; a NULL win; reserved != 0; out_stride smaller than the longest cnt_b;
 *   out == in unless every row with cnt_b > 0 has out_begin == in_origin; for the denoiser zvx_melspec's length conditions on each row whose
 *   window is last.  strength == 0 stays a copy of each emitted range.
 * Accounting: the tags stay "post.denoise" / "post.limit", one timed group per call; bytes are the sum over the rows of what the one-row _ex
 *   calls count.
 * zvx_resample_ex has another window contract (its rows are zero outside the window and it has no support condition): its rows form is
 * zvx_resample_rows below, with rules of its own. */
typedef struct zvx_row_window {
    int64_t in_origin, out_begin, out_count;   /* as the _ex calls' parameters; out_count -1: to the end of the row's signal (needs last) */
    int32_t last;                              /* 0 or 1 */
    int32_t reserved;                          /* must be 0 */
} zvx_row_window;
zvx_status zvx_denoise_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                            const zvx_denoise_params* params, void* out, int64_t out_stride, int flags, const zvx_row_window* win);
zvx_status zvx_limit_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                          const zvx_limit_params* params, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags,
                          const zvx_row_window* win);
/* The rate conversion with a window per row: zvx_resample_ex with win[b] (a HOST array of B entries) in place of the call's one window.  Row b
 * holds samples [in_origin, in_origin + nsamples[b]) of a signal that is zero everywhere else; outputs [out_begin, out_begin + cnt_b) go to
 * positions [0, cnt_b) of out row b, cnt_b = out_count, or with out_count == -1 max(0, ceil((in_origin + nsamples[b]) * L / M) - out_begin).
 * Contract: row b's emitted samples are bit for bit those of zvx_resample_ex on that row alone with win[b] (f32, and int16 with ZVX_PCM16),
 *   and therefore the whole-signal call's bits wherever the windows tile a signal; a row's bits depend neither on which rows share the call
 *   nor on their windows.
 * Unlike zvx_resample_ex: nothing outside [0, cnt_b) of an output row is touched -- there is NO zero fill up to the longest row, as in the
 *   other two rows forms; out_len[b] = cnt_b (may be NULL); `last` must be 0 or 1 and has no meaning here (the signal is zero outside the
 *   window, so out_count -1 does not need it); `reserved` must be 0.
 * Like zvx_resample_ex: the rate pair stays per CALL (the polyphase bank and the tile depend on (L, M) only); the flags, syncs and the queued
 *   form -- ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device output only), ZVX_PCM16; win and nsamples are host arrays and may be reused
 *   when the call returns; equal rates are a copy of each emitted range.
 * How: the one resampling kernel reads a row descriptor at its top -- input and output pointers, length, in_origin, out_begin, cnt and
 *   the bound up to which zeros follow (the longest row for zvx_resample / zvx_resample_ex, cnt_b here) -- and works from it alone.  EVERY
 *   rate conversion -- this call, zvx_resample, zvx_resample_ex, zvx_vocode under an output rate, zvx_spkemb_wav, the streams -- forms these
 *   descriptors on the host and uploads them as one row table through the context's pinned staging arena, queued like a launch (a table
 *   larger than what is left of the 2 MiB arena is a plain copy, complete when it returns: such a call, when queued, waits once).  One way
 *   to fill a descriptor, one body: the sum of an output keeps its single order in every call.  The 16-byte load and store paths are chosen per row
 *   from that row's own pointers and in_origin & 3 and change no bit.  No index is formed in 32 bits from an absolute position: in_origin and
 *   out_begin may lie beyond 2^32.  The grid is sized by the longest cnt_b; workgroups past a row's extent return at once.
 * Validation, all before anything is queued (the context stays usable): every check of zvx_resample_ex, its window checks per row with the
 *   message naming the row.  ZVX_E_INVALID: a NULL win, reserved != 0, last outside {0, 1}, more than INT32_MAX outputs in a row.
 *   ZVX_E_BUFFER: out_stride smaller than the longest cnt_b.  ZVX_E_UNSUPPORTED: a bank that does not fit a workgroup's LDS.
 * Accounting: tag "voc.resample", slot ZVX_T_RESAMPLE, one timed group per call; bytes are the sum over the rows of what the one-row
 *   zvx_resample_ex calls count (a row that emits nothing counts nothing). */
zvx_status zvx_resample_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out,
                             int64_t out_stride, int32_t* out_len, int flags, const zvx_row_window* win);

/* Leveler: a gain curve that follows the gated SHORT-TERM loudness of a sliding window, with a bounded look-ahead, for rows in [B][Nmax] f32
 * with nsamples[b] valid samples at `rate` Hz.  It is an automatic gain control, not R128 normalisation: the integrated gain of
 * zvx_normalize is not known before a signal ends, this curve has finite support and can therefore be applied to a stream.  Whether it is
 * pleasant to listen to on a real voice is NOT measured here: the arithmetic is pinned against a float64 restatement, nothing more.
 * Per row of n samples:
 * Units: h = (rate + 5) / 10 samples, U = n / h whole units.  u[q] is exactly zvx_loudness's: K-weighting in double with that call's
 *   coefficients; the recurrence of unit q runs from ZERO state over samples [(q - 2) h, (q + 1) h), samples in front of sample 0 are zero,
 *   and u[q] is the double sum of y^2 over the last h of them.  Here the zero-state start two units early is part of the contract, not an
 *   allowance: it makes a unit's power a function of 3 h samples and so makes the windows tile.  p[q] = u[q] / h.
 * Parameters (zvx_level_params): S = max(1, rint(window_ms / 100)) units of window and a = rint(lookahead_ms / 100) units of look-ahead,
 *   0 <= a <= S, both on the host in double.
 * Unit gain: over the units k in [max(0, q - S + 1), q], in ascending k and in double, sum = the sum of p[k] and cnt = their number over
 *   those with p[k] > 10^((-70 + 0.691) / 10) -- the absolute gate of BS.1770 applied per 100 ms unit, the constant computed once on the
 *   host.  cnt == 0: G[q] = 1.  Otherwise L = -0.691 + 10 log10(sum / cnt) and G[q] = min(10^((target_lufs - L) / 20), 10^(max_gain_db / 20)),
 *   in double.  A unit whose p lies within a relative 2.3e-4 of the gate is AMBIGUOUS, as for zvx_loudness: either decision is allowed.
 * Nodes: T[j] = G[clamp(j + a - 1, 0, U - 1)], j = 0 .. U + 1: the gain at the START of unit j is that of the window that ends a units
 *   ahead of the unit in front of it.  U == 0: every T is 1.
 * Gain: for sample i with q = i / h:  g = fma(T[q + 1] - T[q], (double)(i - q h) / (double) h, T[q]);  g32 = g rounded to nearest f32;
 *   out[i] = x[i] * g32, ONE f32 multiply; with ZVX_PCM16 the resampler's rule follows.
 * What follows from that:
 *   (a) where both nodes of a sample are 1 the output has the bits of x[i]: silence under the gate is left alone, and so is a whole row
 *       that never passes it;
 *   (b) where both nodes are equal the gain is exactly constant (the fma adds an exact 0);
 *   (c) rows are independent; n == 0 writes nothing (gain_lo = gain_hi = 1); non-finite input follows zvx_vocode_mel's rule (that row
 *       unspecified, nothing faults, the others untouched).
 * gain_lo[b] / gain_hi[b]: the minimum and maximum of g32 over the emitted range; 1 and 1 where it is empty.
 * zvx_level_ex: the same over a window, under the contract of zvx_limit_ex word for word -- row b holds samples [in_origin, in_origin +
 *   nsamples[b]) of a signal that starts at sample 0 and, with last, ends with the row; outputs [out_begin, out_begin + cnt_b) of zvx_level on
 *   the WHOLE signal go to positions [0, cnt_b) of out row b; cnt_b = out_count, or with out_count == -1 (needs last) in_origin + nsamples[b]
 *   - out_begin -- except that the reach is ASYMMETRIC: RL = (S + 3 - a) h - 1 to the left (the oldest unit of the window under the
 *   sample's first node, and its two units of warm-up), RR = (a + 1) h - 1 to the right (the unit under its second node).
 *   Support condition, per row with cnt_b > 0 (otherwise ZVX_E_INVALID; the message names the row, RL or RR and the missing samples):
 *     in_origin <= out_begin  and  out_begin + cnt_b <= in_origin + nsamples[b];
 *     left:  in_origin == 0  or  out_begin - RL >= in_origin;
 *     right: last  or  out_begin + cnt_b - 1 + RR <= in_origin + nsamples[b] - 1.
 *     left, clamped: a window with last and in_origin > 0 whose outputs begin in the signal's last a units or its tail has its first node
 *       clamped to unit U - 1, which moves that node's window out_begin / h + a - U units to the LEFT of where RL assumes it.  Such a row
 *       also needs  (kf - 2) h >= in_origin,  kf = max(0, min(out_begin / h + a - 1, U - 1) - S + 1)  the oldest unit under its first node
 *       (integer divisions, U = (in_origin + nsamples[b]) / h; no rule where U == 0).  Wherever the clamp does not act RL implies it.
 *   With last, U comes from N_b = in_origin + nsamples[b] and the clamp to U - 1 acts; without it the right condition puts every needed
 *   unit inside the window, where the clamp would not have acted: the two agree.  The unit grid is the SIGNAL's, whatever in_origin is.
 *   Results: the emitted samples are bit for bit those of zvx_level on the whole signal (f32, and int16 with ZVX_PCM16): a unit's p
 *   depends on its own 3 h samples, the gated sum runs in ascending k, and a sample's gain on its two nodes and its offset in the unit.
 *   The min / max of gain_lo / gain_hi over a stream's pieces are the whole call's values.
 * zvx_level is zvx_level_ex(..., 0, 0, -1, 1).  zvx_level_rows is zvx_level_ex with win[b] (a HOST array of B entries) in place of the call's
 *   one window, under the contract of zvx_limit_rows: row b's bits are those of the _ex call on that row alone, whatever shares the call;
 *   nothing outside [0, cnt_b) of an output row is touched; the parameters stay per call.
 * Launches: one lane per needed unit runs the 3 h-step recurrence over samples read relative to in_origin (nothing outside the row is
 *   read; staged through LDS as 16-byte groups aligned as addresses, as zvx_loudness does) and writes p into a work buffer of the context
 *   indexed from the row's first needed unit; tiles of the emitted range then form the few G they need once in LDS and multiply, 16-byte
 *   loads and stores where the row's own pointers allow (chosen per row, no bit changes); a reduction per row.  Every call forms one row
 *   descriptor per row on the host -- input, output and unit-buffer pointers, length, in_origin, emitted range, first and last needed
 *   unit, the signal's unit count where the window is last -- and uploads them as one table through the pinned staging arena: one body
 *   serves all three calls.  No index is formed in 32 bits from an absolute position: in_origin and out_begin may lie beyond 2^32.
 * Flags, syncs, in-place use, the queued form: the rows-call contract exactly as zvx_limit / zvx_limit_ex / zvx_limit_rows use it
 *   (ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC with a device output only, ZVX_PCM16 not in place; out == in for f32 rows with the same
 *   stride, on the same side, and out_begin == in_origin; the call waits once, for the host outputs; with ZVX_DEVICE_OUT | ZVX_NO_SYNC
 *   and gain_lo == gain_hi == NULL it only queues).  The apply launch reads x at a sample's own index only.
 * Validation, before anything is queued (ZVX_E_INVALID, the context stays usable): every check zvx_limit_ex / zvx_limit_rows make on ctx /
 *   in / nsamples / params / out / B / Nmax / lengths / rate / out_stride / flags / in-place use / the window's numbers / win / reserved,
 *   the support condition per row, its clamped left rule included; target_lufs not finite or outside [-70, 0]; max_gain_db not finite or negative; window_ms or
 *   lookahead_ms not finite or negative; a > S.  ZVX_E_UNSUPPORTED: S > 600, more than 65535 rows.
 * Stage tag "post.level" in zvx_tag_stats (one timed group per call; no stage slot): algorithmic bytes = 4 per sample read plus the bytes
 *   written (4 or, with ZVX_PCM16, 2 per emitted sample).
 * A stream: zerovox_amd/leveler.py plans the windows -- a non-last push emits up to received - RR, the last one everything, the history
 *   before next_out - RL is dropped -- so a levelled stream runs RR samples behind its input (4409 samples, 200 ms, at 22.05 kHz with
 *   the defaults of 3000 ms / 100 ms).  ZeroVox.vocode_stream(level=) puts it between the denoiser and the limiter.
 * Stream sessions: a level stage inside zvx_stream_open / zvx_stream_next_many is asked for through zvx_stream_open_ex (zvx_stream_stages
 *   below; zvx_stream_params is ABI and stays as it is): the session plans these same windows inside the library, and
 *   zvx_stream_next_many levels its sessions of equal parameters through one zvx_level_rows body.
 * Not here: relative gating, a lower bound on the gain, several channels. */
typedef struct zvx_level_params {
    float target_lufs;    /* short-term loudness to steer towards, finite, in [-70, 0] */
    float max_gain_db;    /* upper bound on the gain in dB, finite, >= 0 */
    float window_ms;      /* S = max(1, rint(window_ms / 100)) units, finite, >= 0; S > 600: ZVX_E_UNSUPPORTED */
    float lookahead_ms;   /* a = rint(lookahead_ms / 100) units, finite, >= 0, a <= S */
} zvx_level_params;
/* out row b = x[i] * g32[i]; gain_lo[b] / gain_hi[b] = min / max of g32 (host arrays, each may be NULL).
 * flags: ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only), ZVX_PCM16 (not in place); out == in (same stride) allowed for f32 */
zvx_status zvx_level(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                     const zvx_level_params* params, void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags);
zvx_status zvx_level_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                        const zvx_level_params* params, void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags,
                        int64_t in_origin, int64_t out_begin, int64_t out_count, int last);
zvx_status zvx_level_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, int rate,
                          const zvx_level_params* params, void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags,
                          const zvx_row_window* win);

/* Equaliser: a general FIR filter over rows [B][Nmax] f32 with nsamples[b] valid samples -- the tone-shaping stage between clean-up
 * (denoiser) and loudness (gain, limiter).  zerovox_amd/equaliser.py designs linear-phase taps from bells, shelves and band edges; the
 * library only filters.  No claim of audible merit is made: the arithmetic is pinned, nothing more.
 * Per row of N samples, K = ntaps, D = delay, h = taps (a HOST array [K], may be reused when the call returns):
 *     y[i] = sum over k = 0 .. K-1 of h[k] * x[i + D - k],   0 <= i < N,   x[j] = 0 for j < 0 and j >= N.
 *   Output row b has the input's length.  With D = (K - 1) / 2 and symmetric taps (linear phase) the output is time-aligned with the
 *   input; with D = 0 the filter is causal.  0 <= D <= K - 1.
 * Arithmetic, part of the contract: acc is a double that starts at +0.0; the terms are added in ASCENDING k, acc = acc + (double) h[k] *
 *   (double) x[i + D - k]; out = (float) acc, one rounding to nearest-even; with ZVX_PCM16 the resampler's rule follows on that float.
 *   The product of two f32 values is exact in double (24 + 24 <= 53 bits of significand, magnitude in [2^-298, 2^256)), so a fused
 *   multiply-add and a multiply followed by an add give the same bits and the result depends on the order of k alone -- which is fixed, not
 *   left to the compiler, to a split of the sum or to a matrix unit.  Zero terms change nothing (the kernel skips or adds the zeros outside
 *   the signal), and acc is never -0.0: it starts at +0, and in round-to-nearest neither +0 + (-0) nor x + (-x) gives -0.  No output is -0.0.
 * Exact corners: K = 1, h = {1}, D = 0 returns x's values (-0.0 becomes +0.0); all-zero taps give +0.0 everywhere; n == 0 writes nothing;
 *   a row's bits depend on its own samples, the taps and D only -- not on B, Nmax, strides or neighbours; non-finite input follows
 *   zvx_vocode_mel's rule (that row unspecified, nothing faults, the others untouched); results of magnitude below 2^-126 may be kept or
 *   flushed, unspecified.
 * zvx_fir_ex / zvx_fir_rows: the same over a window / a window per row, under the contract of zvx_limit_ex / zvx_denoise_ex / zvx_*_rows
 *   word for word, with an ASYMMETRIC reach as the leveler has it: RL = K - 1 - D to the left and RR = D to the right.  Support condition,
 *   per row with cnt_b > 0 (otherwise ZVX_E_INVALID; the message names the row, RL or RR and the missing samples):
 *     in_origin <= out_begin  and  out_begin + cnt_b <= in_origin + nsamples[b];
 *     left:  in_origin == 0  or  out_begin - RL >= in_origin;
 *     right: last  or  out_begin + cnt_b - 1 + RR <= in_origin + nsamples[b] - 1.
 *   The emitted samples are bit for bit those of zvx_fir on the whole signal: an output's terms are the same numbers in the same order,
 *   wherever the window sits.  zvx_fir is zvx_fir_ex(..., 0, 0, -1, 1).  Absolute positions may lie beyond 2^32: no index is formed in 32
 *   bits from one.  _rows: row b is bit for bit the _ex call on that row alone, nothing outside [0, cnt_b) of an output row is touched; the
 *   taps and D stay per CALL.
 * Flags: ZVX_DEVICE_IN, ZVX_DEVICE_OUT, ZVX_NO_SYNC (device out only), ZVX_PCM16 (not in place).  out == in is allowed for f32 rows with
 *   the same stride, on the same side and out_begin == in_origin: a FIR reads its neighbours, so the in-place call filters into a work
 *   buffer of the context and copies the emitted ranges back in the same timed group; the bits are those of the out-of-place call.  With
 *   ZVX_DEVICE_OUT | ZVX_NO_SYNC the call only queues: the taps travel through pinned staging like the denoiser's bias.
 * Validation, before anything is queued (the context stays usable): the rows-call checks of zvx_limit; ZVX_E_INVALID for NULL taps, ntaps
 *   < 1, delay outside [0, K - 1], a tap that is not finite, the window checks and the support condition per row; ZVX_E_UNSUPPORTED for
 *   ntaps > ZVX_FIR_MAX_TAPS and more than 65535 rows.
 * Launches: one row descriptor per row is formed on the host -- input, output, length, emitted range -- and uploaded as one table through
 *   the pinned staging arena, the taps likewise as doubles: one kernel body serves all three calls (csrc/fir.hip: a workgroup stages its
 *   tile's slab in LDS, each lane keeps 4 consecutive outputs in registers and slides one new sample in per tap).
 * Stage tag "post.fir" in zvx_tag_stats (one timed group per call; no stage slot): algorithmic bytes = 4 per sample read plus 4 (or, with
 *   ZVX_PCM16, 2) per emitted sample; flops = 2 K per emitted sample.
 * A stream: zerovox_amd/equaliser.py's FirPlanner plans the windows -- a non-last push emits up to received - RR, the history before
 *   next_out - RL is dropped -- so an equalised stream runs RR = D samples behind its input.
 * Not here: a stage in zvx_stream_open_ex (zvx_stream_stages stays as it is), per-row taps, IIR sections, several channels. */
#define ZVX_FIR_MAX_TAPS 4096
zvx_status zvx_fir(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay,
                   void* out, int64_t out_stride, int flags);
zvx_status zvx_fir_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay,
                      void* out, int64_t out_stride, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count, int last);
zvx_status zvx_fir_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay,
                        void* out, int64_t out_stride, int flags, const zvx_row_window* win);

/* Stream sessions: chunked vocoding of ONE utterance with the planning inside the library.  A session owns the utterance's mel on the
 * device, vocodes it group by group and runs the new samples device to device through the optional denoiser, leveler, watermark, limiter
 * and rate conversion (leveler and watermark: zvx_stream_open_ex); each zvx_stream_next hands out one finished piece with one wait.  It is
 * what ZeroVox.vocode_stream does with its Python planners and up to one host round trip per stage per piece (zerovox_amd/stream.py,
 * denoiser.py, leveler.py, watermark.py, limiter.py, resample.py), moved behind this header; the planners are restated in
 * zerovox_amd/csrc/stream_plan.h (host integer arithmetic, int64 positions).
 * Contract: the concatenation of a session's pieces is bit for bit the concatenation of ZeroVox.vocode_stream(mel, chunk_frames, halo,
 *   chunks_per_call, limiter=, denoise=, level=, watermark=) on the same context under the same "out_rate", and that equals
 *   resample(limit(watermark(level(denoise(plain))))) by the whole-signal calls, plain being the concatenation of the stream without post
 *   steps and every absent step dropped from the chain.  It follows from three things: the rows of each vocoder call are the same, in the
 *   same batch; the window contract of zvx_denoise_ex / zvx_level_ex / zvx_watermark_ex / zvx_limit_ex / zvx_resample_ex holds wherever a
 *   stream is cut; the stage order is the same.  Where the pieces are CUT may differ from the Python
 *   stream (a session flags its last group `last` instead of closing with an empty push); their concatenation does not.
 * zvx_stream_open: mel != NULL: [frames][n_mels] f32 on the host, or on the device with ZVX_DEVICE_IN, copied into a buffer of the session
 *   (a host mel may be reused when the call returns).  mel == NULL: utterance 0 of the mel the context holds after zvx_decode, taken with a
 *   device-to-device copy; frames must be 0; no mel in the context: ZVX_E_STATE; a context batch other than 1: ZVX_E_UNSUPPORTED.
 *   Captured at open: the context's "out_rate", the model's rate and hop, the denoiser's and limiter's parameters (a copy of the bias
 *   included); every table a stage needs on first use (the limiter's window, its oversampling bank, the FFT tables, the resampler's bank)
 *   is uploaded here and the context's work buffers of a step (its table, a group's mel rows, the vocoder's rows) are grown to the
 *   session's largest group, so no zvx_stream_next waits for a table of a stage or an allocation of the step's own, and a later
 *   zvx_set_int("out_rate") does not touch an open session.
 *   zvx_stream_open_ex is zvx_stream_open with two more stages, asked for through zvx_stream_stages (zvx_stream_params is ABI and stays as
 *   it is): `level` puts the leveler (zvx_level_ex's windows, RL to the left and RR to the right) behind the denoiser, `watermark` the
 *   keyed embedder (zvx_watermark_ex's windows, reach n_fft - 1) behind the leveler; watermark->key is THIS session's key.  The chain is
 *   denoise -> level -> watermark -> limit -> rate conversion, the host-planned stream's.  Both structs are copied at open; the FFT tables
 *   and the work buffers the two bodies take (the leveler's unit powers, partials and row table; the embedder's frames, row table, keys
 *   and sign tables) are grown here to the session's largest step.  more == NULL, or both pointers NULL, is zvx_stream_open: the same
 *   buffers, the same pieces, the same launches.
 *   Validation, before anything is allocated (ZVX_E_INVALID, the context stays usable): a NULL ctx / params / out, frames < 2, frames != 0
 *   with a NULL mel, chunk_frames < 1, chunks_per_call outside 1 .. 64, halo < 0, denoise without denoise_bias or the reverse, every check
 *   zvx_denoise and zvx_limit make on their own parameters and bias, frames * hop samples that fail zvx_melspec's length conditions while a
 *   denoiser is asked for, unknown flags; zvx_stream_open_ex: a reserved word that is not 0, every check zvx_level and zvx_watermark make
 *   on their own parameters (a > S, a target_lufs that is not finite, depth_db outside [0, 6], period_blocks outside [1, 256], ...),
 *   frames * hop samples that fail zvx_melspec's length conditions while a watermark is asked for.  ZVX_E_UNSUPPORTED: ZVX_PCM16, what
 *   the stages themselves call unsupported (W > 4096, n_fft, S > 600, more than 512 bands), a group of more than 2^28 samples.
 * zvx_stream_next: vocodes exactly one group -- the next chunks_per_call chunks, fewer at the end -- and pushes its samples through the
 *   stages.  Chunk s is vocoded on mel frames [max(0, s - halo), min(frames, s + chunk_frames + halo)), a row of its own in one batch of
 *   the group's rows at the native rate (the rows ZeroVox._vocode_stream_native builds), and only its chunk_frames * hop interior samples
 *   are kept.  The group's interiors, as ONE run of new samples, go through denoiser, leveler, watermark, limiter and rate conversion -- those
 *   the session has, in this order --, each under the two rules of a stream of its reach (a non-last push emits what is final, the history
 *   before next_out - R is dropped; the leveler: final up to received - RR, dropped before next_out - RL); the call that
 *   vocodes the last group pushes with `last`: everything left comes out in it and *done becomes 1.  *n_out samples, f32 at the session's
 *   output rate, are written to out; *n_out may be 0 while a stage is still filling its reach (out may then be NULL).  After *done:
 *   ZVX_E_STATE.  *n_out is known before anything is queued: capacity < *n_out is ZVX_E_BUFFER with NOTHING consumed -- *n_out is still
 *   filled, the message names both numbers, and the same call with a larger buffer succeeds and yields the same bits.
 *   Flags: ZVX_DEVICE_OUT (out on the device), ZVX_NO_SYNC (device out only: the call only queues).  Without ZVX_DEVICE_OUT the piece
 *   reaches the host through pinned memory of the session under the call's ONE wait.  Everything is queued on the context's main stream;
 *   a session creates no stream of its own.  A zvx_stream_next voids the context's intermediates as zvx_vocode_mel does.  Between two
 *   calls of a session the context may serve any other call, calls of other open sessions included: the session's bits do not depend on it.
 * Device state: per stage two buffers [history | new], sized at open from chunks_per_call * chunk_frames * hop plus the history the stage
 *   retains (2 R; RL + RR for the leveler of zvx_stream_open_ex, 2 (n_fft - 1) for its watermark; 2 half / L + 2 for the conversion) plus
 *   the reaches in front of it; a stage writes straight behind the next stage's
 *   history through the per-row form behind its _rows call (device in, device out, no sync); dropping history copies the retained tail
 *   into the stage's other buffer, never over itself -- the drops of all stages of a call are ONE launch over a table, stage tag
 *   "post.stream".  A session's device footprint is its mel, its stage buffers and the staging of a host piece; a group's gathered mel
 *   rows and the vocoder's rows are work buffers of the CONTEXT, shared by every session.  zvx_stream_next allocates nothing of the
 *   session's (the context's own work buffers grow on first use, as in every call).  New launches: the gather of the group's mel rows
 *   with halo, zero-padded to the longest row, and the gather of the rows' interiors into one run -- stage tag "voc.stream" in
 *   zvx_tag_stats, counted only when a session runs (bytes read plus bytes written); their small per-row table (and the drops') is built
 *   on the host and uploaded once per call through the context's pinned staging, queued like a launch: no host wait.  The stages'
 *   launches count as their _rows calls count them.
 *   zvx_stream_next is the n = 1 case of zvx_stream_next_many below: ONE stepping path serves both, the two differ in their argument
 *   checks and messages only.
 * zvx_stream_info fills, in order and as far as n_info reaches: the stream's total output samples, the output samples emitted so far,
 *   the output rate, the native samples the output runs behind the vocoder (the sum of the stages' reaches: n_fft - 1, the leveler's RR,
 *   n_fft - 1 again for the watermark, 2 W + H, ceil(half / L) + 1; 0 without any), and max_piece = ceil((chunks_per_call * chunk_frames * hop + delay) * L / M) + 1, an upper bound
 *   on any single *n_out, so that a caller sizes one buffer.
 * zvx_stream_close frees everything (NULL: ZVX_E_INVALID); zvx_destroy closes the context's open sessions first.  Errors of session calls
 *   are reported through zvx_last_error of the session's context.
 * Not here: ZVX_PCM16 pieces, several utterances per session (a session is one utterance; zvx_stream_next_many below steps many sessions
 *   in one call), a streamed loudness gain (it is not known before the last chunk), per-session caching of the leveler's unit powers
 *   (the stage keeps RL samples of history instead). */
typedef struct zvx_stream zvx_stream;
typedef struct zvx_stream_params {
    int32_t chunk_frames;              /* mel frames per chunk, >= 1 */
    int32_t chunks_per_call;           /* chunks vocoded per zvx_stream_next as independent batch rows, 1 .. 64 */
    int32_t halo;                      /* mel frames vocoded on either side of a chunk and dropped, >= 0 (ZeroVox.STREAM_HALO is 16) */
    const zvx_denoise_params* denoise; /* NULL: no denoiser */
    const float* denoise_bias;         /* host [n_fft / 2 + 1], copied at open; required iff denoise != NULL */
    const zvx_limit_params* limit;     /* NULL: no limiter */
} zvx_stream_params;
/* the stages zvx_stream_params has no room for (zvx_watermark_params is defined with zvx_watermark below) */
struct zvx_watermark_params;
typedef struct zvx_stream_stages {
    const zvx_level_params* level;                /* NULL: no leveler */
    const struct zvx_watermark_params* watermark; /* NULL: no watermark; params->key is THIS session's key */
    int64_t reserved[2];                          /* 0 */
} zvx_stream_stages;

zvx_status zvx_stream_open(zvx_ctx* ctx, const float* mel, int frames, const zvx_stream_params* params, int flags, zvx_stream** out);
/* zvx_stream_open is zvx_stream_open_ex(..., NULL, ...) */
zvx_status zvx_stream_open_ex(zvx_ctx* ctx, const float* mel, int frames, const zvx_stream_params* params, const zvx_stream_stages* more,
                              int flags, zvx_stream** out);
zvx_status zvx_stream_next(zvx_stream* s, void* out, int64_t capacity, int64_t* n_out, int32_t* done, int flags);
zvx_status zvx_stream_info(const zvx_stream* s, int64_t* info, int n_info);
zvx_status zvx_stream_close(zvx_stream* s);

/* Many streams in one call: continuous batching of stream sessions.  Sessions stay independent objects -- opened and closed at any time,
 * different in every parameter --; zvx_stream_next_many steps any subset of ONE context's open sessions, and the groups of all of them
 * travel through the vocoder as one batch.  A step of a single stream is a launch-bound job on one short row; n of them in one batch cost
 * one launch sequence instead of n.
 * Result: for every i, out[i], n_out[i] and done[i] are exactly what zvx_stream_next(sessions[i], out[i], capacity[i], &n_out[i],
 *   &done[i], flags) would have produced, and the session's state afterwards is the same: the same piece boundaries and the same bits,
 *   piece by piece.  A session's results do not depend on which other sessions share the call, on their order or on their parameters
 *   (chunk_frames, chunks_per_call, halo, chain, captured "out_rate", length, progress): a waveform's bits do not depend on the batch its
 *   rows travel in, which is what the rows of a chunks_per_call group already rest on.
 * One vocoder run: session i contributes min(chunks_per_call, chunks left) rows; the rows go in session order, within a session in chunk
 *   order, zero-padded to the longest row of the call, through ONE run of the vocoder at the native rate.  The rows and the vocoder's output
 *   rows are work buffers of the context (they grow on first use like every other); the call allocates nothing of a session's.
 * Two new launches per call, whatever n is, both under the stage tag "voc.stream" with the bytes the single-session gathers would count in
 *   sum: a gather builds the batch's mel rows from the sessions' resident mels, and a scatter moves every row's interior samples straight
 *   behind the history of the owning session's first stage buffer (to that session's final destination where it has no stage).  Their
 *   per-row tables (source mel pointer and frame count; source offset, count and destination pointer) and the table of the history drops
 *   are built on the host and uploaded as ONE table through the context's pinned staging, queued like a launch: no host wait.
 * Post stages: batched across the sessions through the per-row forms behind zvx_denoise_rows / zvx_limit_rows / zvx_resample_rows.  The
 *   stages run kind by kind -- all denoisers, then the levelers, the watermarks, the limiters, the rate conversions -- on the one stream; a
 *   session's chain order denoise -> level -> watermark -> limit -> resample is kept.  Within a kind the sessions whose stage has
 *   bitwise-equal parameters form one group (the bias compared by content; the leveler's class is its four parameters; the watermark's is
 *   every parameter BUT the key -- the group is one zvx_watermark_rows body with keys[] = its members' keys in call order, so 64 listeners
 *   with 64 keys cost one launch group per round; the limiter's class is W, oversampling and ceiling; the rate conversion's is the native
 *   rate and the session's captured output rate), and a group is ONE call of the per-row form: its rows are the sessions'
 *   [history | new] buffers, each with that session's own window, and each output goes straight behind the next stage's history or to the
 *   session's final destination.  Groups run in the order of their first member, rows within a group in call order, and the bias is
 *   uploaded once per group (the partition is zvx_plan::partition_classes in zerovox_amd/csrc/stream_plan.h).  Each group counts under
 *   "post.denoise" / "post.level" / "post.watermark" / "post.limit" / "voc.resample" as one timed group with the bytes its sessions' single steps count in sum.  A stage
 *   that emits nothing in this call takes no part.  The history drops of all stages of all sessions are ONE launch over a
 *   table of (source, destination, count), each retained tail into its stage's other buffer, under the stage tag "post.stream".
 *   zvx_stream_next is this same path with n = 1 (a group of one row per stage); that a row's bits do not depend on its company is the
 *   per-row contract.
 * One wait: host pieces travel through each session's pinned buffer -- all copies are queued, the call waits once, then copies out.  With
 *   ZVX_DEVICE_OUT every out[i] is a device pointer; with ZVX_DEVICE_OUT | ZVX_NO_SYNC the call only queues.  Everything runs on the
 *   context's main stream.  The context's intermediates are void afterwards, as after zvx_stream_next.
 * All or nothing: every session's piece size is planned on copies of its planners before anything is queued, and every n_out[i] is always
 *   filled.  If any capacity[i] < n_out[i] the call returns ZVX_E_BUFFER and NO session has consumed anything; the message names the first
 *   such index and both numbers, and the same call with larger buffers yields the same bits.
 * Validation, before anything is planned or queued.  ZVX_E_INVALID: a NULL sessions / capacity / n_out / done, n < 1, a NULL entry, the
 *   same session twice, sessions of different contexts, a negative capacity, a NULL out array or a NULL out[i] where n_out[i] > 0, unknown
 *   flags, ZVX_NO_SYNC without ZVX_DEVICE_OUT.  ZVX_E_STATE, with nothing consumed in any session: a session that is already done (the
 *   message names the index).  ZVX_E_UNSUPPORTED: ZVX_PCM16, n > ZVX_STREAM_MANY_MAX_SESSIONS, more than ZVX_STREAM_MANY_MAX_ROWS rows in
 *   total (the message names the count).  Errors are reported through zvx_last_error of the sessions' context (with NULL sessions, n < 1 or
 *   no session at all among the entries there is none: the status alone).
 * A HIP failure past the point where the groups are consumed ends EVERY session of the call (done), as it ends the one session of
 *   zvx_stream_next. */
enum { ZVX_STREAM_MANY_MAX_SESSIONS = 64, ZVX_STREAM_MANY_MAX_ROWS = 256 };
zvx_status zvx_stream_next_many(zvx_stream* const* sessions, int n, void* const* out, const int64_t* capacity,
                                int64_t* n_out, int32_t* done, int flags);

/* Debug/parity taps: copy an intermediate of the last call to host fp32.
 * what: "encoder_out" [B][Tmax][hidden] (after the style add), "features" [B][Lmax][hidden],
 *       "mel" [B][Lmax][n_mels], "pitch_idx"/"energy_idx"/"duration" [B][Tmax] (as float). */
zvx_status zvx_fetch(zvx_ctx* ctx, const char* what, float* out, size_t out_floats);

/* ---- multi-GPU: utterances shard across ranks with no data-path exchange; the ONE collective is the gather of the
 * finished waveform rows to one rank, issued here directly on RCCL (grouped ncclSend / ncclRecv: every peer -> root
 * transfer rides its own xGMI link).  The reference has no distributed layer; one process per GPU,
 * one context per process.  librccl.so.1 is dlopen'ed by zvx_comm_unique_id / zvx_comm_init only; it must belong to the
 * same ROCm runtime as the HIP library already in the process (do not import a framework that bundles its own ROCm AFTER
 * this library has been loaded). ---- */
#define ZVX_COMM_ID_BYTES 128
/* rank 0 creates the communicator id (ncclGetUniqueId) and ships the 128 bytes to the other ranks out of band */
zvx_status zvx_comm_unique_id(void* id_out);
zvx_status zvx_comm_init(zvx_ctx* ctx, const void* id, int rank, int world);
/* Every rank contributes `bytes` bytes at device pointer `local`; rank `root` receives them in rank order at device
 * pointer `recv` (world * bytes; ignored elsewhere).  Enqueued on the context's communication stream behind everything
 * issued so far on its compute stream, so with ZVX_NO_SYNC it overlaps the next synthesis call; a later
 * ZVX_DEVICE_OUT synthesis into `local` waits on the device for this gather to have read it.  world == 1: a copy. */
zvx_status zvx_comm_gather(zvx_ctx* ctx, const void* local, size_t bytes, void* recv, int root, int flags);
/* all ranks: returns after every rank has drained both of its streams and arrived (ncclAllReduce of one word) */
zvx_status zvx_comm_barrier(zvx_ctx* ctx);
/* *value = max over ranks (bench.py: MAX-over-ranks elapsed time) */
zvx_status zvx_comm_max_f64(zvx_ctx* ctx, double* value);
/* Collective (every rank calls it): who is in the job as the communicator itself reports it -- out[0] = world, out[1] =
 * ncclCommCount, out[2] = ncclGetVersion code, out[3] = ranks that contributed to an all-reduce SUM of ones, out[4 + r] = PCI
 * address ((domain << 16) | (bus << 8) | (device << 3) | function) of rank r's device.  n_out >= 4 + world.  bench.py puts it
 * into the N > 1 JSON line ("rccl": {...}). */
zvx_status zvx_comm_info(zvx_ctx* ctx, int64_t* out, int n_out);
void       zvx_comm_destroy(zvx_ctx* ctx);

/* Keyed audio watermark on the device, and its detector: a multiplicative spread-spectrum mark laid on the denoiser's STFT frame grid, so that
 * an operator can later ask "did this audio come from my deployment" with the key.  The embedder scales bands of bins up or down by
 * depth_db in a keyed pattern over (time block, band); the detector looks for that pattern in the band log-energies.
 * Framing, analysis, synthesis, overlap-add, den_min, the PCM16 rule and the reflect padding are zvx_denoise's, word for word: the model's
 *   n_fft / hop / window, the same tables rounded once to f32, the ascending-f sums.  Rows are at the model's rate (`rate` below is
 *   zvx_get_int("sampling_rate")).
 * Bands: k_lo = ceil(lo_hz n_fft / rate); J = floor((min(hi_hz n_fft / rate, n_fft / 2) - k_lo) / KB); band j is bins
 *   [k_lo + j KB, k_lo + (j + 1) KB), computed in double on the host.  J < 3 is ZVX_E_INVALID, J > 512 ZVX_E_UNSUPPORTED.
 * Pattern: sign(c, j) = +1 if bit 63 of mix64(key ^ ((uint64)c << 32 | j)) is set, else -1, for c in [0, P); mix64 is the splitmix64
 *   finaliser: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  The
 *   P x J table is built on the host and uploaded through the pinned staging arena.
 * Gain: frame f of the SIGNAL (absolute index) is in block c = (f / TB) mod P.  g_up = (float)10^(depth_db / 20), g_dn =
 *   (float)10^(-depth_db / 20), both computed in double on the host.  For the bins of band j: X' = g X, g = g_up or g_dn by sign(c, j); every
 *   other bin: X' = X, no multiply.  The imaginary parts of DC and Nyquist are dropped as in zvx_denoise.  depth_db == 0: a copy, the bits of
 *   x, nothing is transformed.
 * zvx_watermark_ex: the window contract, the reach R = n_fft - 1, the support condition, the validation and the flags of zvx_denoise_ex.
 *   The emitted samples are bit for bit those of the whole-signal call: a frame keeps the slot it has in the whole call (zvx_denoise_ex),
 *   and the block index comes from the absolute frame index, formed in 64 bits.  zvx_watermark is zvx_watermark_ex(..., 0, 0, -1, 1).
 * Detector (zvx_watermark_detect), whole rows only; per row:
 *   the STFT as above, Pw = re^2 + im^2; LB[f][j] = sum over the band's bins of log2(max(Pw, 1e-6));
 *   D[f][j] = LB[f][j] - (LB[f][j - 1] + LB[f][j + 1]) / 2 for 1 <= j <= J - 2 (the neighbours' mean takes the spectral envelope off);
 *   windows of window_frames frames with hop window_frames / 2, the last one clipped to the row: window w is frames
 *   [w H, min(w H + window_frames, F)), H = window_frames / 2, w < 1 + ceil((F - window_frames) / H); window_frames == 0, or a row of no
 *   more frames than that: one window, the row.  window_frames == 1 is ZVX_E_INVALID.
 *   In a window, for each offset o in [0, P TB): frame f (the ROW's index) has block (f + o) / TB; E[block][j] is the sum of D over the
 *   block's frames inside the window; z(o) = sum sign(block mod P, j) E / sqrt(sum E^2), 0 where the denominator is 0, the sums in double.
 *   Per window the largest z and the smallest o that attains it; per row the best window (the first of equals).
 *   score[b], offset[b], window[b] (HOST arrays [B]) receive them; win_score / win_offset (HOST [B][NWmax], or both NULL) every window's
 *   -- entries past a row's window count are not touched; NWmax smaller than a row's window count is ZVX_E_BUFFER.
 *   The detector's band may be narrower than the embedder's: bands are counted from k_lo, so a smaller hi_hz detects after a
 *   down-conversion (same lo_hz, KB, TB, P).  depth_db is not read.  The offset search is at hop granularity: audio cut at the front by
 *   c samples shows the offset nearest c / hop; a sample shift below a hop costs score, it does not move the grid.
 *   On the device: one launch does FFT, Pw, the band log sums and D into an F x (J - 2) f32 work buffer (no spectrum goes to memory); one
 *   launch, a workgroup per (row, window), does the search: for each of the TB phases the blocks' E are folded by block mod P into a table
 *   in LDS, a run of 12288 / P bands at a time, so that each of the P shifts is one pass over it; the denominator is formed per phase
 *   from the unfolded E.  The device's sums are f32 up to E and double from there, in the folded order -- the scores agree with the
 *   float64 restatement (tests/watermark_ref.py) to the measured bound below, not bit for bit.
 * Rest: rows are independent; n == 0 writes nothing and scores 0 (offset 0, window 0); non-finite input follows zvx_vocode_mel's rule (that
 *   row unspecified, nothing faults, the others untouched).  Flags of zvx_watermark / _ex: zvx_denoise's; zvx_watermark_detect:
 *   ZVX_DEVICE_IN only, and the call waits once for its results.
 *   ZVX_E_INVALID, before anything is queued, the context stays usable: every check of zvx_denoise(_ex) on rows, output, window and
 *   lengths; a NULL params; depth_db not finite or outside [0, 6]; lo_hz / hi_hz not finite, lo_hz < 0 or lo_hz >= hi_hz; block_frames or
 *   band_bins < 1; period_blocks outside [1, 256]; reserved != 0; J < 3; for the detector a NULL score / offset / window, a negative
 *   window_frames or 1, one of win_score / win_offset without the other, NWmax < 0.  ZVX_E_UNSUPPORTED: zvx_denoise's, and J > 512.
 * Stage tags "post.watermark", "post.wmdetect" and "post.wmidentify" in zvx_tag_stats (one timed group per call).
 * Measured (MI355X, n_fft 1024 / hop 256, rows with |x| <= 1, against tests/watermark_ref.py): embed, largest |out - ref| 2.52e-7 (the denoiser's transform pair: 2.48e-7 there);
 *   detect, largest |score - ref| 7.7e-6 on scores of 2 .. 13.5.  The tests hold 4x these.
 *   What is measured is the arithmetic, and detection on synthetic voiced signals (tests/test_watermark.py: at depth 1 dB and the defaults of
 *   zerovox_amd/watermark.py, 1.5 s and 3 s at 22.05 kHz).  Short clips cut to the telephone band are NOT reliably detectable (a float64
 *   prototype gave a score of 3.1 at 1.5 s after an 8 kHz round trip against a wrong-key null of about 2.5).
 * zvx_watermark_rows: zvx_watermark_ex with a window AND a key per row -- win[b] (HOST [B]) is row b's window, keys[b] (HOST [B]) its
 *   key; keys == NULL: params->key for every row.  Row b's emitted samples are bit for bit those of zvx_watermark_ex on that row alone with
 *   win[b] and params with key = keys[b], whatever shares the call; nothing outside [0, cnt_b) of an output row is touched.  The rows-call
 *   contract is zvx_denoise_rows' own: its flags, the queued form (ZVX_NO_SYNC; keys and win may be reused at once), in place with
 *   out_begin == in_origin per row, ZVX_PCM16 not in place.  Validation: zvx_watermark_ex's, and zvx_denoise_rows' on win.  depth_db == 0
 *   is a copy and no key is read.  The sign tables of the call's DISTINCT keys are built on the device by one small launch (the rule
 *   above in 64-bit integer arithmetic; the keys go up through the pinned staging arena) into a stack [n][P][J]; rows of equal keys share
 *   a table.  Stage tag "post.watermark".
 * zvx_watermark_identify: which of K candidate keys marked each row -- ONE analysis (the detector's first launch), one launch that builds
 *   the K sign tables on the device (packed, 32 signs to a word), and one search launch over all keys: a workgroup serves 8 keys of one (window, row), builds the folded
 *   table and the denominator of a phase once and runs the shift pass per key, every sum in the single-key kernel's order.
 *   score[b][k], offset[b][k], window[b][k] (HOST [B][K]) are bit for bit what zvx_watermark_detect writes to score[b], offset[b],
 *   window[b] with params->key = keys[k] and the same window_frames; best[b] (HOST [B]) is the smallest k that attains the row's largest
 *   score (0 for a row of n == 0, whose scores are all 0).  The best over a row's windows is taken on the host from [B][NW][K] device
 *   results.  params->key is not read (depth_db is checked as the detector checks it, not used); duplicate keys are allowed; per-window
 *   results are not returned (zvx_watermark_detect has them).  Flags: ZVX_DEVICE_IN only; the call waits once, for its results.
 *   ZVX_E_INVALID, before anything is queued: every check of zvx_watermark_detect; a NULL keys / score / offset / window / best; K < 1.
 *   ZVX_E_UNSUPPORTED: K P J > 2^26 signs (the message names the product; the tables are a work buffer of one BIT per sign, rows padded
 *   to 32-bit words, and the results one of 8 B NW K bytes), or K > 65536.  Stage tag "post.wmidentify".
 *   The LARGEST score over wrong keys grows with the number of keys tried.  The default threshold of zerovox_amd/watermark.py (5.5) was
 *   measured over 256 wrong keys; nothing is measured beyond that, and a caller who tries thousands of keys has to judge by the margin
 *   between the best and the second-best score as well.
 * Stream sessions: zvx_stream_open_ex takes these parameters, key included, as a session's watermark stage (zvx_stream_stages); sessions
 *   that differ in their key alone are marked by ONE zvx_watermark_rows body per zvx_stream_next_many.
 * Not here: robustness against lossy codecs, time-stretching
 *   or deliberate removal; whether the mark is inaudible on a real checkpoint -- none of these is measured, and nothing here claims them. */
typedef struct zvx_watermark_params {
    uint64_t key;            /* the secret */
    float    depth_db;       /* finite, 0 .. 6; 0: a copy (the bits of x, nothing transformed) */
    float    lo_hz, hi_hz;   /* marked band, 0 <= lo_hz < hi_hz; hi is clipped to rate / 2 */
    int32_t  block_frames;   /* TB >= 1: frames per time block */
    int32_t  band_bins;      /* KB >= 1: bins per band */
    int32_t  period_blocks;  /* P, 1 .. 256: the pattern repeats every P blocks */
    int32_t  reserved;       /* 0 */
} zvx_watermark_params;
zvx_status zvx_watermark(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                         void* out, int64_t out_stride, int flags);
zvx_status zvx_watermark_ex(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                            void* out, int64_t out_stride, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count, int last);
/* score, offset, window: host [B]; win_score, win_offset: host [B][NWmax] or NULL.  flags: ZVX_DEVICE_IN only */
zvx_status zvx_watermark_detect(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                                int window_frames, float* score, int32_t* offset, int32_t* window, float* win_score, int32_t* win_offset,
                                int NWmax, int flags);

/* keys: host [B] or NULL (params->key for every row); win: host [B] */
zvx_status zvx_watermark_rows(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                              const uint64_t* keys, void* out, int64_t out_stride, int flags, const zvx_row_window* win);
/* keys: host [K]; score, offset, window: host [B][K]; best: host [B].  flags: ZVX_DEVICE_IN only */
zvx_status zvx_watermark_identify(zvx_ctx* ctx, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                                  const uint64_t* keys, int K, int window_frames, float* score, int32_t* offset, int32_t* window, int32_t* best,
                                  int flags);

/* ---- voice matching: cosine scores of query embeddings against a device-resident library of embeddings, and the best of them --------
 * zvx_spk_score writes score[b][k] for every query b < B and library row k < K; zvx_spk_topk writes, per query, the `top` largest of
 *   those scores with their row indices.  The two questions they answer: whose voice was delivered (the similarity of a re-embedded
 *   waveform, zvx_spkemb_wav, to the embedding it was conditioned on: K = 1), and which enrolled voice a clip is (look-up, duplicates at
 *   enrolment, a list of voices that must not be cloned).
 * Arguments: query [B][dim] f32, on the host, or on the device with ZVX_DEVICE_IN -- for example the ZVX_DEVICE_OUT | ZVX_NO_SYNC output
 *   of zvx_spkemb_wav queued just before; stream order is the fence.  lib [K][dim] f32 is ALWAYS a device pointer on the context's device
 *   (zvx_dev_alloc / zvx_dev_from_host, or rows that zvx_spkemb_wav wrote there), aligned to 16 bytes; a library is resident by nature, so
 *   no flag says so.  The outputs follow ZVX_DEVICE_OUT; ZVX_NO_SYNC is allowed with a device output only (the call then only queues).
 *   dim is explicit, not read from the context: a multiple of 4 with 4 <= dim <= 2048.  Neither side has to be normalised (a centroid of
 *   several clips is not a unit vector).
 * Arithmetic, in f32: score(b, k) = dot(q_b, e_k) / max(|q_b| |e_k|, FLT_MIN).  A zero row on either side therefore scores 0.  A score
 *   that is not finite (NaN or inf in the inputs; also a norm that exceeds FLT_MAX) is delivered as -2.0f, by both calls.  The norms are
 *   formed with three scaled sums of squares, so rows scaled by 1e-20 or 1e+18 keep their accuracy; the query is divided by its norm
 *   before the products.  Against a float64 evaluation every score lies within (2 dim + 8) 2^-24 (tests/voice_ref.py derives the bound).
 * Position contract (the rows contract of the post-processing calls, applied here): the bits of score(b, k) depend on the values of
 *   q_b and e_k and on dim only -- not on B, K, top, the row's position in the library, or which of the two calls produced them.  The
 *   order in which the dim products are added is fixed.
 * Top-k: 1 <= top <= min(K, ZVX_SPK_TOP_MAX).  score / index [B][top], sorted by descending score and by ascending index among equal
 *   scores: exactly the selection over what zvx_spk_score would write.  Indices are int32, so K <= 2^31 - 1.  No B x K matrix is formed:
 *   the first launch keeps a sorted list per (query, slab of 512 rows), a second small launch merges the lists; no host wait in between.
 * The library is read once per group of up to 64 queries (fewer where dim or top are large: the group is staged in 160 KB of LDS; 64 at
 *   dim 528, 16 at dim 2048); larger B is looped over inside the call.
 * ZVX_E_INVALID, before anything is queued, the context stays usable and nothing is written: unknown flag bits; ZVX_NO_SYNC without
 *   ZVX_DEVICE_OUT; a NULL query / lib / score / index; B <= 0; K <= 0 or K > 2^31 - 1; a bad dim; a bad top; lib not aligned to 16
 *   bytes.  ZVX_E_UNSUPPORTED: B > 65535.  The message names the function and the argument.
 * Stage tag "spk.match" in zvx_tag_stats (one timed group per call); no ZVX_T_* slot.
 * Not here: a speaker-verification threshold.  What similarity separates two speakers depends on the checkpoint's speaker encoder and is
 *   not measured; nothing here claims a perceptual meaning for a score. */
#define ZVX_SPK_TOP_MAX 32
zvx_status zvx_spk_score(zvx_ctx* ctx, const float* query, int B, const float* lib, int64_t K, int dim, float* score /* [B][K] */, int flags);
zvx_status zvx_spk_topk(zvx_ctx* ctx, const float* query, int B, const float* lib, int64_t K, int dim, int top, float* score /* [B][top] */,
                        int32_t* index /* [B][top] */, int flags);

/* Alignment: dynamic time warping (DTW) of B independent pairs of feature sequences on the device.  Pair p uses rows a[p][0 .. Ta[p]) and
 * b[p][0 .. Tb[p]) of [B][Tamax][dim] and [B][Tbmax][dim] f32; nothing else of the padding is read.
 * Definition, per pair, with i < Ta and j < Tb:
 *   Local distance: d(i, j) = sqrt(sum_k ((double) a[i][k] - (double) b[j][k])^2) in double; the sum in any order, with or without fma.
 *   Recurrence: C(0, 0) = d(0, 0); otherwise C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)), a missing neighbour taken as
 *     +inf: one double addition per cell, so there is no order freedom beyond d.
 *   Path: backtracked from (Ta-1, Tb-1) to (0, 0) over the device's own values of C; among equal candidates the order is the diagonal,
 *     then (i-1, j), then (i, j-1).
 *   Outputs: cost = C(Ta-1, Tb-1);  path_len = L, the number of cells of the path;  path[0 .. L) = its cells (i, j) in forward order, (0, 0)
 *     first;  a2b[i] = (min j, max j) over the path's cells of row i, for i < Ta.  Entries past L and rows past Ta are not written.
 *   A backtrack decision is AMBIGUOUS, and either step is allowed there, when its two smallest candidates lie within a relative 1e-9 of
 *     each other.
 *   The result is deterministic from run to run.  Pairs are independent: a pair's bits depend neither on B, nor on Tamax / Tbmax, nor on its
 *     neighbours.
 *   Derived bounds (not measurements): every term of a path's sum is non-negative, so the accumulated rounding of any path's sum is at most
 *     (Ta + Tb + dim) 2^-53 relative, and |cost - cost_ref| <= 2 (Ta + Tb + dim) 2^-53 cost_ref against the float64 restatement
 *     (tests/align_ref.py): about 2e-12 at the size limit, far inside the ambiguity band.  Where the reference's own path holds no ambiguous
 *     decision, the device's path equals it cell for cell.  This assumes a faithfully rounded f64 sqrt; tests/test_align_gpu.py checks d on
 *     perfect squares (dim 1, integer features: d is the exact integer).
 *     Measured on an MI355X against tests/align_ref.py (tests/test_align_gpu.py, pairs from 1 x 1 to 4096 x 4096): a largest relative
 *     deviation of 0 -- every cost has the bits of the reference's, and every path is the reference's.
 *   Non-finite input: zvx_vocode_mel's rule -- the call succeeds, that pair is unspecified (its path is still a monotone path of at most
 *     Ta + Tb - 1 cells), every other pair keeps its bits.
 * Launches (zerovox_amd/csrc/align.hip).  Forward: one workgroup per pair, 64 .. 1024 lanes (the call's longest Ta rounded up to a wave; the
 *   bits do not depend on it).  The rows of a are taken in bands of that many; lane l of a band keeps row i0 + l of a in registers and
 *   the band sweeps its anti-diagonals, one barrier per step.  The left neighbour is the lane's own previous value, the up neighbour the
 *   next-lower lane's previous value through a double-buffered LDS line (between waves and inside them: no DPP form was built), the diagonal
 *   neighbour the up value read one step earlier; the last row of a band waits in an LDS edge of Tb doubles for the next band.  The b rows
 *   are read from memory two steps ahead of their cell and the distance is formed one step ahead of it, so that between two barriers only
 *   the LDS read, the minimum, the addition and the stores wait for each other.  The direction of every cell goes to a context work buffer as one byte, diagonal-major per pair
 *   (diagonal s contiguous, its offset computed analytically): Ta Tb bytes per pair.  LDS: 48 KiB per workgroup (32 KiB edge, 16 KiB line).
 *   Backtrack: one wave per pair; one lane walks the direction bytes (one dependent load per step; no LDS tile was built), the wave then
 *   turns the reversed cells round into `path` and fills a2b.  No atomics, no workgroup that waits for another.  The call waits once, for
 *   the host outputs.
 * Validation, before anything is queued (the context stays usable).  ZVX_E_INVALID: a NULL ctx / a / b / Ta / Tb / cost / path_len; B < 1;
 *   dim < 1; a Ta[p] outside [1, Tamax] or Tb[p] outside [1, Tbmax]; path given with path_stride < max_p (Ta[p] + Tb[p] - 1); a flag other
 *   than ZVX_DEVICE_IN; a non-zero reserved field.  ZVX_E_UNSUPPORTED: dim > 32; a Ta[p] or Tb[p] above 4096; B > 65535; more than 2^30
 *   cells in the call (sum_p Ta[p] Tb[p]).  The message names the pair.
 * Stage tag "post.align" (one timed group per call; its two launches also under "post.align.forward" / "post.align.backtrack"):
 *   algorithmic bytes = sum_p ((Ta + Tb) dim 4 + Ta Tb).
 * Not here: a Sakoe-Chiba band or other path constraints, subsequence / open-end DTW, soft-DTW, pairs longer than 4096 frames, a streaming
 *   form. */
typedef struct zvx_dtw_params { int32_t reserved[4]; } zvx_dtw_params;   /* all zero; NULL allowed */
zvx_status zvx_dtw(zvx_ctx* ctx,
                   const float* a, const int32_t* Ta, int Tamax,   /* [B][Tamax][dim] f32 */
                   const float* b, const int32_t* Tb, int Tbmax,   /* [B][Tbmax][dim] f32 */
                   int B, int dim, const zvx_dtw_params* params,
                   double* cost,        /* host [B], required */
                   int32_t* path_len,   /* host [B], required */
                   int32_t* path,       /* host [B][path_stride][2] (i, j), forward order, or NULL */
                   int64_t path_stride,
                   int32_t* a2b,        /* host [B][Tamax][2]: first and last j matched to frame i, or NULL */
                   int flags            /* ZVX_DEVICE_IN only: a and b are device pointers */);

/* Two batches of waveforms at the model's rate in, their alignment and a mel-cepstral distortion out; the chain stays on the device.
 *   1. The log-mel of both batches by zvx_melspec's path: a row's log-mel is bit for bit zvx_melspec's of that row.  The refusals are
 *      zvx_melspec's; the message names the side (a or b) and the row.
 *   2. Cepstra: c[t][k-1] = (float) (sqrt(2 / M) sum_m L[t][m] cos(pi k (m + 1/2) / M)), k = 1 .. n_cep, M = n_mels; the sum in double from
 *      the f32 log-mel, in any order, rounded once; c0 is left out; the cosine table is built on the host in double.  They lie within one
 *      f32 ulp of the float64 DCT of that log-mel.
 *   3. zvx_dtw's two launches on the cepstra with dim = n_cep: COST, path and a2b are bit for bit what zvx_dtw returns on them.
 * stats[p]: FRAMES_A, FRAMES_B (mel frames of the two rows), PATH_LEN, COST, and MCD_DB = (10 / ln 10) sqrt(2) COST / PATH_LEN in double
 *   (the front end's log is the natural log, so the constant is the usual one).
 * What this MCD is: the distortion between DCT cepstra of the model's own log-mel, c0 left out, averaged over the cells of the DTW path.
 *   What it is not: figures from SPTK / WORLD mel-cepstral analysis, as papers quote them, are not comparable with it, and no perceptual
 *   claim is made.
 * path [B][path_stride][2], a2b [B][a2b_stride][2], cep_a / cep_b [B][cep_stride][n_cep] are optional host outputs (cepstra rows past a
 *   row's frames are zero up to the longest row of their side).  ZVX_E_INVALID beyond the above: a NULL params or stats, n_cep outside
 *   [1, min(32, n_mels - 1)], a non-zero reserved field, a2b_stride or cep_stride smaller than the longest row they hold, a flag other than
 *   ZVX_DEVICE_IN.  ZVX_E_UNSUPPORTED: zvx_dtw's limits, on the frame counts. */
typedef struct zvx_align_params { int32_t n_cep; /* 1 .. min(32, n_mels - 1); 13 is the default of the bindings */ int32_t reserved[3]; } zvx_align_params;
enum { ZVX_AL_FRAMES_A = 0, ZVX_AL_FRAMES_B, ZVX_AL_PATH_LEN, ZVX_AL_COST, ZVX_AL_MCD_DB, ZVX_AL_COUNT = 5 };
zvx_status zvx_align_wav(zvx_ctx* ctx, const float* wav_a, const int32_t* n_a, int Nmax_a,
                         const float* wav_b, const int32_t* n_b, int Nmax_b, int B,
                         const zvx_align_params* params, double* stats /* host [B][ZVX_AL_COUNT] */,
                         int32_t* path, int64_t path_stride, int32_t* a2b /* [B][a2b_stride][2] */, int64_t a2b_stride,
                         float* cep_a, float* cep_b /* host [B][cep_stride][n_cep] or NULL */, int64_t cep_stride, int flags);

/* Device buffers for ZVX_DEVICE_OUT outputs / zvx_comm_gather without any other GPU runtime in the process. */
zvx_status zvx_dev_alloc(zvx_ctx* ctx, size_t bytes, void** out);
zvx_status zvx_dev_free(zvx_ctx* ctx, void* p);
zvx_status zvx_dev_from_host(zvx_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
zvx_status zvx_dev_to_host(zvx_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* device to device on the context's stream, behind everything queued there; the ranges must not overlap; returns when the copy is done
 * (a library of embeddings grows and closes its holes with it: zerovox_amd/voices.py) */
zvx_status zvx_dev_copy(zvx_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);

/* drains every stream of the context (compute, front end, communication) */
zvx_status zvx_sync(zvx_ctx* ctx);
zvx_status zvx_stage_times(zvx_ctx* ctx, float ms[ZVX_T_COUNT]);

/* Per-kernel-variant counters accumulated while "profile" == 2: launches, summed milliseconds,
 * algorithmic FLOPs and algorithmic bytes.  Returns the number of variants; name buffers are 64 bytes. */
typedef struct {
    char   name[64];
    int64_t launches;
    double ms;
    double flops;
    double bytes;
} zvx_kernel_stat;
int        zvx_kernel_stats(zvx_ctx* ctx, zvx_kernel_stat* out, int max_out);
/* The same counters grouped by pipeline stage ("encoder", "variance", "lenreg", "decoder", "decoder.norm", "voc.pre",
 * "voc.up1".."voc.res4", "voc.post", "voc.resample", "voc.stream", "post.join", "post.loudness", "post.limit", "post.denoise", "post.watermark", "post.wmdetect", "post.wmidentify", "post.align", "spkemb"; name = stage): every launch of the stage, including the HBM-bound helper
 * kernels, while "profile" == 2 and "profile_only" == -1.  Feeds the per-stage roofline fractions of bench.py. */
int        zvx_tag_stats(zvx_ctx* ctx, zvx_kernel_stat* out, int max_out);
zvx_status zvx_reset_stats(zvx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* ZVX_H */
