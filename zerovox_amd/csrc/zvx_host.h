// zvx_host.h -- what the host units of libzvx share (zvx.hip, host_*.hip); no kernel unit includes it.
//
// Host-side C++ only sequences kernels: every contraction is a launch_gemm() (gemm.hip), everything
// else a kernel from ops.hip.  One HIP stream per context; workspaces are grown on demand and reused.
// Reference call structure being replaced: ZeroVox.inference_ex (model.py:308-347).
//
// Everything in it is in namespace zvx::host, except zvx_ctx and zvx_stream: they are at global scope, as include/zvx.h declares them.
// What only one unit uses stays in that unit's own anonymous namespace and is not declared here.
//
// The functions that cross a unit boundary (unit that defines them: names -> units that call them):
//   zvx.hip          run_vocoder -> host_post (do_denoise_bias), host_stream
//   host_post.hip    rows contract: rows_check, flags_check, out_rows_check, rows_to_device, stage_rows -> zvx.hip (the measuring calls)
//                    resampler: rs_pair, rs_bank, model_rate, run_resample_rows -> zvx.hip, host_stream;  rs_plan, plan_rows -> zvx.hip
//                    join / trim: join_check, bounds_to_host -> zvx.hip (do_spkemb_wav)
//                    windows, limiter, leveler, denoiser, watermark: limit_win, window_count_row, limit_os_check, limit_params_check,
//                    run_limit_rows, level_params_check, level_clamped_support_check, run_level_rows, dn_geom, denoise_params_check,
//                    run_denoise_rows, run_watermark_rows -> host_stream;  loud_coef, dn_tables, watermark_params_check -> zvx.hip, host_stream;
//                    stft_len_check, wm_sign_table -> zvx.hip (watermark detection)
//                    entry functions: do_resample, do_resample_rows, do_trim_bounds, do_join, do_limit, do_level, do_denoise, do_denoise_bias,
//                    do_watermark, do_fir -> zvx.hip
//   host_stream.hip  stream_free, do_stream_open, do_stream_next, do_stream_next_many, do_stream_info -> zvx.hip (the entry points)
// and, defined here: guarded (zvx.hip, host_comm.hip), gemm_base, set_taps_1d, dn_min_samples, dn_frames, dn_fft_flops, and the structs of the
// rows and window contracts (RowsInfo, DevRows, TagScope, RowsReturn, RowsWindow, PostRow, RowsWindows, RsPlan, WindowsIn).
// So host_comm calls no other unit; host_post calls zvx.hip for the generator only; host_stream calls the generator and host_post; zvx.hip
// (measuring calls, do_vocode, the entry points) calls host_post and host_stream.
#ifndef ZVX_HOST_H
#define ZVX_HOST_H

#include "../../include/zvx.h"
#include "zvx_kernels.h"
#include "watermark_kernels.h"
#include "voicematch_kernels.h"
#include "stream_plan.h"

#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

// the communicator's handle as <rccl/rccl.h> declares it (the same typedef again): only host_comm.hip includes that header
struct ncclComm;
typedef struct ncclComm* ncclComm_t;

namespace zvx::host {

struct ZvxError : std::runtime_error {
    int code;
    ZvxError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw ZvxError(code, buf);
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) fail(ZVX_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

extern thread_local std::string g_create_error;   // (zvx.hip)

struct Tensor {
    char kind = 'p';
    std::vector<int> dims;
    size_t off = 0, numel = 0;
    void* dev = nullptr;
    int dtype = DT_F32;
    const float* host = nullptr;
    float alpha = 1.f;                       // split-plane weights in IEEE half: the planes carry w * 2^s, alpha = 2^-s (applied by the GEMM epilogue)
    int dim(int i) const { return dims.at(i); }
};

struct DevBuf { void* p = nullptr; void* base = nullptr; size_t cap = 0; };

struct GemmEvent { hipEvent_t a, b; int variant; double flops, bytes; long rows; int N, K, taps, res, fused; std::string tag, kname; };

}  // namespace zvx::host

// Deliberately at global scope in this header: zvx_ctx and zvx_stream are global (include/zvx.h) and their inline members name Tensor, fail,
// GemmArgs ... unqualified, as they did in the one file.  Only host units include this header, and each of them wants both directives.
using namespace zvx;
using namespace zvx::host;

struct zvx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream launches are being issued on (swapped to a side stream and back by the schedules below)
    hipStream_t main0 = nullptr;           // the context's main stream (what `stream` is outside those swaps)
    // multi-GPU (zvx_comm_*): communicator, its own stream, and per-buffer "the gather has read this" events
    hipStream_t comm_stream = nullptr;
    hipStream_t voc_aux[2] = {nullptr, nullptr};   // single requests: the non-final pairs of the 2nd / 3rd ResBlock of a vocoder stage run beside the 1st
    hipEvent_t voc_ev[3] = {nullptr, nullptr, nullptr};
    int voc_overlap_maxb = 1 << 20;        // zvx_set_int("voc_overlap_maxb", n): batches of at most n utterances use them (0: never; A/B)
    int voc_overlap_frames = 28672;        // zvx_set_int("voc_overlap_frames", n): ... and only below n mel frames per call (B x Pmax)
    // Front end of call i+1 under the vocoder of call i (zvx_synthesize): encoder / variance adaptor / length regulator / mel decoder are
    // issued on front_stream, the vocoder on `stream`.  The two meet in ONE buffer, "mel": the vocoder waits for ev_front_done, the
    // next call's front end waits for ev_mel_free (recorded behind the vocoder's first kernel, which copies the mel into its padded
    // input).  A host that queues calls (ZVX_DEVICE_OUT | ZVX_NO_SYNC) gets the latency-paced front end (5-28 % of the matrix roof)
    // hidden under the previous call's vocoder; a host that waits for every call sees the serial schedule.  Results are bit-identical
    // (same kernels on the same data).  zvx_set_int("front_overlap", v): 1 (default) = queued calls (ZVX_DEVICE_OUT | ZVX_NO_SYNC) take the
    // two-stream schedule, 2 = every zvx_synthesize call does (tests), 0 = everything on `stream` (A/B).
    hipStream_t front_stream = nullptr;
    hipEvent_t ev_front_done = nullptr, ev_mel_free = nullptr, ev_main_join = nullptr;
    int front_overlap = 1;
    bool mel_free_pending = false;         // ev_mel_free is recorded and the front stream has not waited for it yet
    bool front_dirty_main = true;          // front-end buffers were touched on `stream` (zvx_encode / zvx_decode ...) since the front stream last joined it
    // Asynchronous host delivery (ZVX_HOST_ASYNC; synthesize.py:233-239 hands the caller host memory): the finished waveform rows go to one
    // of two PINNED host slots on a copy stream of their own, behind an event the vocoder's last kernel records -- the copy of call i runs
    // under the front end / vocoder of call i + 1, the host thread never waits inside a synthesis call (zvx_wait_host does).
    struct HostSlot { void* p = nullptr; size_t cap = 0; hipEvent_t ready = nullptr, done = nullptr; bool pending = false; int B = 0, pcm16 = 0; long stride = 0, need = 0; };
    HostSlot host_slot[2];
    int host_next = 0, host_last = -1;
    hipStream_t copy_stream = nullptr;
    bool copy_is_comm = false;
    hipStream_t aux_stream = nullptr;      // second compute stream: the duration predictor of a small batch beside the pitch predictor
    hipEvent_t ev_aux[2] = {nullptr, nullptr};
    int va_overlap_maxb = 1 << 20;             // zvx_set_int("va_overlap_maxb", n): batches of at most n utterances overlap the two predictors (0: never; A/B)
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    hipEvent_t ev_compute = nullptr;
    std::map<const void*, hipEvent_t> gather_fence;
    std::string err;
    std::map<std::string, std::string> cfg;
    std::map<std::string, Tensor> tensors;
    std::vector<float> host_blob;
    std::map<std::string, DevBuf> bufs;
    std::map<const void*, const void*> packed;   // bf16 weight tensor -> its MFMA-fragment-order copy (conv-slab kernel)
    std::map<const void*, const void*> pair_packed;   // StyleTTS residual blocks with a 1x1 shortcut: conv2 weight tensor -> combined fragment stream [conv2 | shortcut] per channel tile
    int dt = DT_BF16;               // activation / weight dtype of the bf16-able stages
    // config
    int H = 0, emb_dim = 0, punct_dim = 0, n_phone_rows = 0, n_punct_rows = 0, max_txt_len = 0, max_mel_len = 0;
    int enc_layers = 0, enc_heads = 0, ffn_dim = 0, ffn_k0 = 0, ffn_k1 = 0, vp_dim = 0, vp_k = 0, n_bins = 0;
    int dec_layers = 0, dec_heads = 0, dec_scln = 0, n_mels = 0, hop = 0, res_dim = 0, dec_kind = 0, rn_asp = 1;
    std::vector<int> rn_layers, rn_filters, voc_rates, voc_ksizes, voc_rb_k;
    std::vector<std::vector<int>> voc_rb_d;
    int voc_resblock = 1, voc_c0 = 0;
    // per-call state
    int B = 0, Tmax = 0, Lmax = 0;
    std::vector<int> T_host, mel_len_host;
    std::vector<int> in_stage;            // host staging of a call's integer inputs (one upload)
    bool have_features = false, have_mel = false;
    // profiling
    int profile = 0;
    int profile_only = -1;                 // >= 0: per-launch events only for this kernel variant (keeps the timed region lean)
    int rs_prof = 0;                       // zvx_set_int("rs_prof", 1): per-wave cycle counters of the streaming kernels (library built with -DRS_PROFILE)
    int enc_split = 0;                     // 16-bit mode: the f32 GEMMs of the phoneme encoder run as 3-plane 16-bit GEMMs: 2 = IEEE-half planes (default: 2^-24-class, f32
                                           // results), 1 = bf16 planes (rounds 2-3: 5e-5 on the encoder output; A/B), 0 = the exact-f32 MFMA
    const void* fft_xs_ready = nullptr;     // fft.xs holds the split planes of this buffer (written by the previous FFT block's last LayerNorm)
    int norm_fuse_maxb = 1 << 20;          // zvx_set_int("norm_fuse_maxb", n): batches of at most n utterances may take the one-launch InstanceNorm of the StyleTTS decoder (0: never; A/B)
    int dec_sc_fuse = 1;                   // zvx_set_int("dec_sc_fuse", 0): the 1x1 shortcut of a StyleTTS residual block as its own launch (A/B; the fused form skips one 16-bit rounding of the conv2 result)
    int dec_flat = 1;                      // zvx_set_int("dec_flat", 0): the StyleTTS decoder's convolutions per utterance instead of batch-flattened (A/B, bit-identical)
    int voc_f16_stages = -1;               // zvx_set_int("voc_f16_stages", mask): which domains of the generator (bit 0: mel / conv_pre, bit i: upsampling stage i) compute in IEEE half when voc_f16 is on, the others in bf16; -1 (default): all but a 128-channel ResBlock1 stage
    int voc_h16_ok = -1;                   // every contraction weight of the generator has an IEEE-half copy (decided on the first vocoder call)
    int voc_f16 = 1;                       // zvx_set_int("voc_f16", 0): the vocoder's activations / weights / running sum in bf16 instead of IEEE half (A/B; round 5)
    int dec_f16 = 1;                       // zvx_set_int("dec_f16", 0): StyleTTS decoder activations / weights in bf16 instead of IEEE half (A/B)
    int use_attn_f32 = 1;                  // zvx_set_int("attn_f32", 0): the encoder's attention as V^T / score / P.V GEMMs + softmax (A/B)
    int use_flash = 1;                     // zvx_set_int("flash", 0): the decoder's attention as score GEMM + softmax + PV GEMM (A/B)
    int use_resstream = 1;                 // zvx_set_int("resstream", 0): ResBlocks of the narrow stages as per-pair launches (A/B, bit-equal)
    int rs_seg_min = 0;                    // zvx_set_int("rs_seg_min", -1): streaming ResBlock segments never shorter than 2048 rows (A/B of the single-request sizing)
    int spk_s2_fuse = 1;                   // zvx_set_int("spk_s2_fuse", 0): the level transitions as two launches of the gathered-row GEMM (A/B)
    int spk_pool_fuse = 1;                 // zvx_set_int("spk_pool_fuse", 0): the speaker encoder's SE pool as its own pass everywhere (A/B)
    int slab_small = 2, slab_flat = 1;     // zvx_set_int("slab_small" / "slab_flat", v): conv-slab tile choice for single requests / whole-grid XCD remap (A/B; per context)
    int poison_pads = 0;                   // zvx_set_int("poison_pads", 1): every work buffer of the mel decoders is filled with NaN bit patterns before a decode (tests: padding rows / stale rows must never reach a result -- ADVICE r4)
    // Saturation audit of the half mode (zvx_set_int("f16_sat_check", 1)): every 16-bit tensor of the vocoder and the mel
    // decoders goes through HBM (one launch per convolution: no LDS-resident intermediate) and is scanned for clamped values
    // (+-65504) behind the launch that wrote it; zvx_get_int("f16_sat_events") is the count since the switch was last set.  A debug mode:
    // same arithmetic per convolution, ~3x the time.
    int sat_check = 0;
    unsigned long long* sat_count_dev() { return (unsigned long long*)buf("sat.count", 64); }
    void sat_scan(const void* x, int dt, long bs, int ld, int B, int rows_max, const int* rows, int C) {
        if (sat_check && x && dt == DT_F16) launch_count_sat16(x, bs, ld, B, rows_max, rows, C, sat_count_dev(), stream);
    }
    int use_rb2fuse = 1;                   // zvx_set_int("rb2fuse", 0): every convolution of a ResBlock2 (HiFi-GAN V3 / resblock "2") as its own launch instead of one launch per block (A/B)
    int use_stagefuse = 1;                 // zvx_set_int("stagefuse", 0): narrow vocoder stages (C = 16 / 8) as per-pair launches instead of ONE launch per stage (narrowstage.hip; A/B)
    struct NsWeights { void* W = nullptr; float* bias = nullptr; int woff[18] = {0}; };
    std::map<std::string, NsWeights> ns_weights;   // narrowstage.hip fragment order, per (stage, dtype), built on first use
    int use_pairstream = 1;                // zvx_set_int("pairstream", v): C = 128 ResBlock pairs on pairstream.hip: 1 = every k (default; jobs under ~200 k rows run the bit-identical two-launch path), 3 = every k and every job size (tests), -1 / 0 = two conv-slab launches per pair (the bit-equality reference)
    int shape_log = 0;                     // zvx_set_int("shape_log", 1): one stderr line per timed launch (profile 2)
    int max_frames = 1 << 18;              // hard cap on a predicted mel length (guards the allocation, fs2.py:678-681 has none)
    // Output rate (zvx_set_int("out_rate", hz); 0 = the model's own rate): the waveform calls resample their rows on the device as
    // their last launch (do_vocode).  The polyphase banks are designed on the host in double, rounded once to f32 and kept per (L, M).
    int out_rate = 0;
    struct RsBank { int L = 0, M = 0, half = 0, T = 0, pitch = 0; const float* dev = nullptr; };
    std::map<std::pair<int, int>, RsBank> rs_banks;
    std::map<int, const double*> lim_wins;  // zvx_limit: the smoothing weights on the device, designed in double, per window W
    std::map<int, LoudCoef> loud_coefs;    // zvx_loudness / zvx_normalize: the K-weighting biquads, designed in double, per sampling rate
    // zvx_denoise / zvx_denoise_bias: twiddles, window and squared window on the device, designed in double on first use (n_fft, hop and
    // win_length are the model's: one set per context); nothing exists before the first call
    struct DnTables { int n_fft = 0, log2n = 0, win_length = 0; const float* twid = nullptr; const float* win = nullptr; const double* win2 = nullptr; double den_min = 0; };
    DnTables dn_tab;
    // zvx_join / zvx_trim_bounds / zvx_spkemb_wav / zvx_loudness / zvx_normalize / zvx_true_peak / zvx_limit: pinned host memory the
    // layout, bounds or result words (and host output rows) land in under the call's one wait
    void* join_host = nullptr;
    size_t join_host_cap = 0;
    void* join_pinned(size_t bytes) {
        if (bytes > join_host_cap) {
            if (join_host) { HIPCHK(hipStreamSynchronize(stream)); HIPCHK(hipHostFree(join_host)); join_host = nullptr; join_host_cap = 0; }
            const size_t cap = bytes + bytes / 8 + 256;
            HIPCHK(hipHostMalloc(&join_host, cap, hipHostMallocDefault));
            join_host_cap = cap;
        }
        return join_host;
    }
    hipEvent_t stage_ev[ZVX_T_COUNT][2];
    bool stage_used[ZVX_T_COUNT];
    float stage_ms[ZVX_T_COUNT];
    std::vector<GemmEvent> pending;
    std::vector<zvx_kernel_stat> stats;
    std::string tag = "other";             // stage label of the launches being issued (per-stage roofline accounting, profile 2)
    std::map<std::string, zvx_kernel_stat> tagstats;
    std::map<std::string, zvx_kernel_stat> namedstats;   // helper kernels timed under a name of their own (the prosody-control kernels)
    std::vector<hipEvent_t> event_pool;
    std::vector<zvx_stream*> streams;       // the open stream sessions (zvx_stream_open); zvx_destroy closes what is left

    // ------------------------------------------------------------------ helpers
    int cfg_int(const char* k) const {
        auto it = cfg.find(k);
        if (it == cfg.end()) fail(ZVX_E_MANIFEST, "manifest: missing cfg '%s'", k);
        return atoi(it->second.c_str());
    }
    std::vector<int> cfg_list(const char* k) const {
        auto it = cfg.find(k);
        if (it == cfg.end()) fail(ZVX_E_MANIFEST, "manifest: missing cfg '%s'", k);
        std::vector<int> v; std::stringstream ss(it->second); std::string tok;
        while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(atoi(tok.c_str()));
        return v;
    }
    const Tensor& t(const std::string& name) const {
        auto it = tensors.find(name);
        if (it == tensors.end()) fail(ZVX_E_MANIFEST, "weights: tensor '%s' missing", name.c_str());
        return it->second;
    }
    bool has(const std::string& name) const { return tensors.count(name) != 0; }
    const float* pf(const std::string& name) const { return (const float*)t(name).dev; }

    // A buffer about to be freed may still be read by work queued on ANY of the context's streams (the two-stream schedule: the front
    // end of call i + 1 regrows "mel" on the front stream while call i's launch_mel_pad is queued on the main stream) -- every stream
    // of the context is drained first; hipFree's own device-wide synchronisation is not a contract to lean on
    void drain_for_free() {
        HIPCHK(hipStreamSynchronize(stream));
        for (hipStream_t s2 : {main0, front_stream, aux_stream, voc_aux[0], voc_aux[1], comm_stream, copy_stream})
            if (s2 && s2 != stream) HIPCHK(hipStreamSynchronize(s2));
    }
    void* buf(const std::string& name, size_t bytes) {
        DevBuf& d = bufs[name];
        if (bytes > d.cap) {
            if (d.base) { drain_for_free(); HIPCHK(hipFree(d.base)); d.base = nullptr; d.p = nullptr; }
            size_t cap = bytes + bytes / 8 + 256;
            HIPCHK(hipMalloc(&d.base, cap));
            HIPCHK(hipMemsetAsync(d.base, 0, cap, stream));
            d.p = d.base;
            d.cap = cap;
        }
        return d.p;
    }
    // Several small named buffers as slices of ONE allocation, so that a call zero-fills / uploads them with one operation instead of
    // one each (a single request is paced by its launch count).  Lookups by name keep working; the slices are re-cut on every call.
    char* carve(const std::string& pool, const std::vector<std::string>& names, size_t bytes_each, size_t* stride_out) {
        const size_t stride = (bytes_each + 255) & ~(size_t)255;
        char* base = (char*)buf(pool, stride * names.size());
        for (size_t i = 0; i < names.size(); i++) {
            DevBuf& d = bufs[names[i]];
            if (d.base) { drain_for_free(); HIPCHK(hipFree(d.base)); d.base = nullptr; }
            d.p = base + i * stride; d.cap = stride;
        }
        *stride_out = stride;
        return base;
    }
    int* ibuf(const std::string& name, size_t n) { return (int*)buf(name, n * sizeof(int)); }
    float* fbuf(const std::string& name, size_t n) { return (float*)buf(name, n * sizeof(float)); }
    // Small host -> device copies go through PINNED memory owned by the context.  A copy from pageable memory makes the runtime
    // wait for the stream before it returns; from pinned memory it is queued like a launch.  With forced durations and a device
    // output (ZVX_NO_SYNC) a whole zvx_synthesize call then only QUEUES work: the host runs ahead of the GPU by a call or more and
    // a slow or preempted host thread no longer shows up as GPU idle time.  Two arenas alternate between API calls; an arena is
    // reused only after the event recorded behind its last copy has passed.
    struct Arena { char* p = nullptr; size_t cap = 0, cur = 0; hipEvent_t ev = nullptr; bool pending = false; };
    Arena arena[2];
    int arena_i = 0;
    int api_depth = 0;
    static constexpr size_t ARENA_BYTES = 2u << 20;
    void arena_begin() {
        Arena& a = arena[arena_i];
        if (a.pending) { HIPCHK(hipEventSynchronize(a.ev)); a.pending = false; }
        a.cur = 0;
    }
    void arena_end() {                      // only a call that uploaded something rotates the arenas: a gather or a query between two
        Arena& a = arena[arena_i];          // synthesis calls must not send them both to the same arena (the second would wait for the first)
        if (!a.cur || !stream) return;
        if (!a.ev) HIPCHK(hipEventCreateWithFlags(&a.ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(a.ev, stream));
        a.pending = true;
        arena_i ^= 1;
    }
    void upload(void* dst, const void* src, size_t bytes) {
        Arena& a = arena[arena_i];
        const size_t need = (bytes + 63) & ~(size_t)63;
        if (!a.p) { HIPCHK(hipHostMalloc((void**)&a.p, ARENA_BYTES, hipHostMallocDefault)); a.cap = ARENA_BYTES; }
        if (a.cur + need > a.cap) {
            // larger than what is left of the arena: a plain copy, COMPLETED before this returns (the caller's / the context's staging
            // memory may be reused right after the call; the runtime's own staging of pageable copies is not a contract to lean on)
            HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
            return;
        }
        memcpy(a.p + a.cur, src, bytes);
        HIPCHK(hipMemcpyAsync(dst, a.p + a.cur, bytes, hipMemcpyHostToDevice, stream));
        a.cur += need;
    }
    int* upload_ints(const std::string& name, const int* v, size_t n) {
        int* d = ibuf(name, n);
        upload(d, v, n * sizeof(int));
        return d;
    }
    size_t es() const { return dtype_size(dt); }

    hipEvent_t new_event() {
        hipEvent_t e;
        if (!event_pool.empty()) { e = event_pool.back(); event_pool.pop_back(); return e; }
        HIPCHK(hipEventCreate(&e));
        return e;
    }
    void stage_begin(int s) { if (profile) { HIPCHK(hipEventRecord(stage_ev[s][0], stream)); } }
    void stage_end(int s) { if (profile) { HIPCHK(hipEventRecord(stage_ev[s][1], stream)); stage_used[s] = true; } }

    // One dispatch that carries its own start / stop events (profile 2; no marker packets on the stream): arm the launchers' event pair,
    // launch, disarm on every way out (a throwing `launch` included), and queue the GemmEvent that `describe` fills in.  `vid` names the
    // variant the profile_only filter compares (asked only while that filter is set); `launch` returns the variant id that ran and throws
    // where it cannot.
    template <typename V, typename L, typename D>
    void profiled(V&& vid, L&& launch, D&& describe) {
        const bool prof = profile >= 2 && (profile_only < 0 || vid() == profile_only);
        if (!prof) { launch(); return; }
        GemmEvent ev{};
        ev.a = new_event(); ev.b = new_event();
        struct Armed { Armed(hipEvent_t a, hipEvent_t b) { profile_events(a, b); } ~Armed() { profile_events(nullptr, nullptr); } };
        ev.variant = [&] { Armed armed(ev.a, ev.b); return launch(); }();
        describe(ev);
        ev.tag = tag;
        pending.push_back(ev);
    }
    void gemm(GemmArgs& a) {
        if (a.flops <= 0) a.flops = 2.0 * (double)a.M * a.nbatch * a.nheads * (double)a.N * ((double)a.K * a.ntaps + (double)a.K2);
        if (!a.Wp && a.dtype != DT_F32) { auto it = packed.find(a.W); if (it != packed.end()) a.Wp = it->second; }
        a.slab_small = slab_small | (spk_s2_fuse ? 0 : 32); a.xcd_flat = slab_flat;      // (bit 5: no conv2d_s2_kernel -- spk_s2_fuse 0 is the gathered-row launch set for BOTH level transitions)
        profiled([&] { return gemm_variant_of(a); }, [&] {
            const int id = a.fused == 2 ? launch_rb2fuse(a, stream) : (a.fused ? launch_resfuse(a, stream) : launch_gemm(a, stream));
            if (id < 0) fail(ZVX_E_INVALID, "launch_gemm rejected shape M=%d N=%d K=%d taps=%d", a.M, a.N, a.K, a.ntaps);
            return id;
        }, [&](GemmEvent& ev) {
            ev.flops = a.flops; ev.rows = (long)a.M * a.nbatch * a.nheads; ev.N = a.N; ev.K = a.K; ev.taps = a.ntaps; ev.res = a.res_mode; ev.fused = a.fused;
            const double esz = dtype_size(a.dtype);
            // algorithmic bytes: input rows + weights + everything the epilogue reads and writes (output, residual, running sum)
            const double cells = (double)a.M * a.nbatch * a.nheads * a.N;
            ev.bytes = ((double)a.M * a.nbatch * a.nheads) * (double)(a.K + a.K2) * esz + (double)a.N * ((double)a.K * a.ntaps + a.K2) * esz * (a.fused ? 2 : 1) +
                       (a.out ? cells * dtype_size(a.out_dtype) : 0.0) + ((a.res_mode && !a.fused) ? cells * dtype_size(a.res_dtype) : 0.0) +
                       ((a.accum && (a.accum_mode & 1)) ? cells * dtype_size(a.accum_dtype) : 0.0) + ((a.accum && (a.accum_mode & 2)) ? cells * dtype_size(a.accum_dtype) : 0.0);
        });
        if (sat_check && a.nheads == 1) {                   // (audit mode: the attention products run fused, their output is scanned by fft_block)
            sat_scan(a.out, a.out_dtype, a.o_bs, a.ldo, a.nbatch, a.M, a.out_len, a.N);
            if (a.accum && (a.accum_mode & 2)) sat_scan(a.accum, a.accum_dtype, a.a_bs, a.lda, a.nbatch, a.M, a.out_len, a.N);
        }
    }
    // streaming ResBlock chain (resstream.hip); returns false (nothing launched) when the shape is not covered
    bool run_stream(StreamArgs& a) {
        const int id = launch_resstream(a, this->stream, true);
        if (id < 0) return false;
        profiled([&] { return id; }, [&] {
            const int id2 = launch_resstream(a, this->stream, false);
            if (id2 < 0) fail(ZVX_E_INVALID, "launch_resstream rejected a shape its dry run accepted (C=%d k=%d pairs=%d)", a.C, a.ntaps, a.npair);
            return id2;
        }, [&](GemmEvent& ev) {
            const double rows = (double)a.M * a.nbatch;
            ev.flops = 2.0 * 2.0 * a.npair * rows * a.C * a.C * a.ntaps; ev.rows = (long)rows; ev.N = a.C; ev.K = a.C; ev.taps = a.ntaps;
            ev.res = a.accum_mode; ev.fused = 10 + a.npair;
            ev.bytes = rows * a.C * 2.0 * (1 + (a.out ? 1 : 0) + ((a.accum && (a.accum_mode & 1)) ? 1 : 0) + ((a.accum && (a.accum_mode & 2)) ? 1 : 0));
        });
        return true;
    }
    // the HBM-bound helpers (norms, gathers, conv_post ...): event-timed as a group when every launch is being profiled
    // kname: also counted under that name in zvx_kernel_stats
    template <typename F>
    void timed(double flops, double bytes, F&& f, const char* kname = nullptr) {
        const bool prof = profile >= 2 && profile_only < 0;
        GemmEvent ev{};
        if (prof) { ev.a = new_event(); ev.b = new_event(); HIPCHK(hipEventRecord(ev.a, stream)); }
        f();
        if (prof) { HIPCHK(hipEventRecord(ev.b, stream)); ev.variant = -1; ev.flops = flops; ev.bytes = bytes; ev.tag = tag; if (kname) ev.kname = kname; pending.push_back(ev); }
    }
    void resolve_events() {
        if (stats.empty()) {
            stats.resize(gemm_num_variants());
            for (int i = 0; i < gemm_num_variants(); i++) { memset(&stats[i], 0, sizeof stats[i]); snprintf(stats[i].name, 64, "%s", gemm_variant_name(i)); }
        }
        for (auto& e : pending) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            if (shape_log && e.variant >= 0) fprintf(stderr, "launch %-24s rows=%-8ld N=%-4d K=%-4d taps=%-2d res=%d fused=%d  %8.3f ms %8.1f TF/s %8.1f GB/s(alg)\n",
                                   gemm_variant_name(e.variant), e.rows, e.N, e.K, e.taps, e.res, e.fused, ms, e.flops / ms / 1e9, e.bytes / ms / 1e6);
            else if (shape_log) fprintf(stderr, "launch %-24s [%s]  %8.3f ms %8.1f GB/s(alg)\n", "(helper)", e.tag.c_str(), ms, e.bytes / ms / 1e6);
            if (e.variant >= 0) { auto& s = stats[e.variant]; s.launches++; s.ms += ms; s.flops += e.flops; s.bytes += e.bytes; }
            auto& ts = tagstats[e.tag];
            if (!ts.name[0]) snprintf(ts.name, 64, "%s", e.tag.c_str());
            ts.launches++; ts.ms += ms; ts.flops += e.flops; ts.bytes += e.bytes;
            if (!e.kname.empty()) {
                auto& ks = namedstats[e.kname];
                if (!ks.name[0]) snprintf(ks.name, 64, "%s", e.kname.c_str());
                ks.launches++; ks.ms += ms; ks.flops += e.flops; ks.bytes += e.bytes;
            }
            event_pool.push_back(e.a); event_pool.push_back(e.b);
        }
        pending.clear();
        for (int s = 0; s < ZVX_T_COUNT; s++)
            if (stage_used[s]) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, stage_ev[s][0], stage_ev[s][1])); stage_ms[s] = ms; stage_used[s] = false; }
    }
    void sync() {
        if (front_stream) HIPCHK(hipStreamSynchronize(front_stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (comm_stream) HIPCHK(hipStreamSynchronize(comm_stream));
        if (copy_stream && !copy_is_comm) HIPCHK(hipStreamSynchronize(copy_stream));
        if (profile) resolve_events();
    }
    // error path of an API call: whatever it queued on a side stream before it threw is drained, so that the next call's main-stream
    // work cannot race with it (the joins that normally order the streams were never issued)
    void quiesce_side_streams() noexcept {
        if (front_stream) (void)hipStreamSynchronize(front_stream);
        if (aux_stream) (void)hipStreamSynchronize(aux_stream);
        for (int i = 0; i < 2; i++) if (voc_aux[i]) (void)hipStreamSynchronize(voc_aux[i]);
        front_dirty_main = true; mel_free_pending = false;
    }
    void front_setup() {                   // the front stream runs at the highest priority the device offers
        if (front_stream) return;
        int least = 0, greatest = 0;                                         // (numerically: greatest priority = the smaller value)
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&front_stream, hipStreamNonBlocking, greatest));
        HIPCHK(hipEventCreateWithFlags(&ev_front_done, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_mel_free, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_main_join, hipEventDisableTiming));
    }
};

namespace zvx::host {

// What the checks of a post step's parameters yield (level_params_check, dn_geom, watermark_params_check); a session keeps its own.
struct LevelGeom { int h, S, a; int64_t RL, RR; };          // S and a in units of h samples (100 ms)
struct DnGeom { int n_fft, log2n, hop, pad, nf; };           // the model's STFT geometry
struct WmPlan { DnGeom g; int k_lo, J; };                    // ... and the watermark's bands
}  // namespace zvx::host

// A stream session (include/zvx.h: zvx_stream_open): one utterance's mel on the device, the planners of its post stages and, per stage,
// two device buffers laid out [history | new].  A stage's output is written straight behind the next stage's history; dropping the history
// before keep_from copies the retained tail into the stage's OTHER buffer (never an overlapping copy) and swaps the two.  A group's gathered
// rows and what the vocoder makes of them are not the session's: every step, of one session or of many, takes them from the context
// ("stream.rows", "stream.wav"), which zvx_stream_open has grown to the session's largest group.
struct zvx_stream {
    zvx_ctx* c = nullptr;
    int frames = 0, chunk = 0, cpc = 0, halo = 0, hop = 0, native = 0, out_rate = 0;
    int nchunks = 0, next_chunk = 0, done = 0;
    int Pcap = 0;                          // the longest row a group can have, in mel frames
    int64_t total = 0, emitted = 0, delay = 0, max_piece = 0;
    enum { DENOISE = 0, LIMIT = 1, RESAMPLE = 2, LEVEL = 3, WATERMARK = 4, KINDS = 5 };
    struct Stage {
        int kind = DENOISE;
        zvx_plan::ReachPlanner reach;      // DENOISE, WATERMARK (n_fft - 1), LIMIT
        zvx_plan::ResamplePlanner rate;
        zvx_plan::LevelPlanner level;
        float* buf[2] = {nullptr, nullptr};
        int cur = 0;
        int64_t cap = 0, hist = 0;         // samples a buffer holds; retained samples [origin, received) at the front of buf[cur]
        zvx_plan::Step push(int64_t n, bool last) { return kind == RESAMPLE ? rate.push(n, last) : kind == LEVEL ? level.push(n, last) : reach.push(n, last); }
        int64_t received() const { return kind == RESAMPLE ? rate.received : kind == LEVEL ? level.received : reach.received; }
    };
    std::vector<Stage> stages;             // in the order they run: denoiser, leveler, watermark, limiter, rate conversion
    zvx_denoise_params dn{};
    std::vector<float> bias;
    zvx_limit_params lim{};
    int lim_W = 0;                         // the limiter's window in samples
    zvx_level_params lvl{};                // (zvx_stream_open_ex)
    LevelGeom lvl_g{};
    zvx_watermark_params wm{};             // wm.key is this session's key
    WmPlan wm_plan{};
    char* dev = nullptr;                   // ONE device allocation: the mel, the stage buffers, the host piece's staging
    float* mel = nullptr;
    float* ostage = nullptr;
    float* pinned = nullptr;               // host piece: [max_piece] f32
};

namespace zvx::host {

inline GemmArgs gemm_base(int dtype) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.dtype = dtype; a.nbatch = 1; a.nheads = 1; a.ntaps = 1; a.stride = 1; a.wout = 0; a.hin = 1; a.win = 0;
    a.alpha = 1.f; a.out_scale = 1.f; a.out_dtype = dtype; a.res_dtype = dtype;
    return a;
}
inline void set_taps_1d(GemmArgs& a, int k, int dilation) {
    a.ntaps = k;
    for (int i = 0; i < k; i++) { a.du[i] = 0; a.dv[i] = (int)((i - (k - 1) / 2) * dilation); }
}

struct RowsInfo { long n_max = 0; double n_sum = 0; };      // the longest row, and all samples of the batch

struct DevRows { const float* x; const int* len; };

// "issue the following under tag T", between the stage slot's events where one is given; the tag is restored on every way out
struct TagScope {
    zvx_ctx* c; std::string keep; int slot;
    TagScope(zvx_ctx* c_, const char* tag, int slot_ = -1) : c(c_), keep(c_->tag), slot(slot_) {
        c->tag = tag;
        if (slot >= 0) c->stage_begin(slot);
    }
    ~TagScope() { c->tag = keep; }
    void close() { if (slot >= 0) c->stage_end(slot); c->tag = keep; }
};

// What zvx_normalize / zvx_limit and their measuring forms hand back: `res_bytes` of result words (padded to 256 bytes in the pinned
// block) and, with a host output, the rows: staged on the device at a stride of their own, brought over behind the words, one wait.
struct RowsReturn {
    zvx_ctx* c; int B; size_t res_bytes, res_pad, ss; long n_max, ostage; bool want_host, host_out; char* host = nullptr; void* odev = nullptr;
    RowsReturn(zvx_ctx* c_, int B_, size_t res_bytes_, bool want_host_, bool writes_rows, long n_max_, int flags)
        : c(c_), B(B_), res_bytes(res_bytes_), res_pad((res_bytes_ + 255) & ~(size_t)255), ss((flags & ZVX_PCM16) ? 2 : 4), n_max(n_max_),
          ostage((n_max_ + 7) & ~7L), want_host(want_host_), host_out(writes_rows && !(flags & ZVX_DEVICE_OUT)) {
        if (want_host || host_out) host = (char*)c->join_pinned(res_pad + (host_out ? (size_t)B * ostage * ss : 0));
    }
    // where the launches write the rows, and at which stride: the staging buffer `name`, or the caller's device rows
    void* out_rows(const char* name, void* out, int64_t out_stride, long* bs) {
        *bs = host_out ? ostage : (long)out_stride;
        return odev = host_out ? c->buf(name, (size_t)B * ostage * ss + 16) : out;
    }
    // -> the result words on the host; nullptr where none were asked for (with ZVX_NO_SYNC the call has then only queued)
    const char* finish(const void* res_dev, void* out, int64_t out_stride, const int32_t* nsamples, int flags) {
        if (want_host) HIPCHK(hipMemcpyAsync(host, res_dev, res_bytes, hipMemcpyDeviceToHost, c->stream));
        if (host_out && n_max > 0) HIPCHK(hipMemcpyAsync(host + res_pad, odev, (size_t)B * ostage * ss, hipMemcpyDeviceToHost, c->stream));
        if (!want_host && (flags & ZVX_NO_SYNC)) return nullptr;     // device output, nothing for the host: the call only queues
        c->sync();                                                   // the call's one wait
        if (host_out)
            for (int b = 0; b < B; b++)
                if (nsamples[b] > 0) memcpy((char*)out + (size_t)b * out_stride * ss, host + res_pad + (size_t)b * ostage * ss, (size_t)nsamples[b] * ss);
        return want_host ? host : nullptr;
    }
};

// The window of the post-processing steps: a row holds samples [in_origin, in_origin + n) of its signal, the outputs
// [out_begin, out_begin + cnt) are emitted.  The whole-row calls are {0, 0, -1, 1}.  The denoiser and the limiter add a support condition
// and `last` (the signal ends with the window); the resampler's rows are zero outside the window and `last` takes no part.
struct RowsWindow { int64_t in_origin = 0, out_begin = 0, out_count = -1; int last = 1; };

// One row of a post-processing step: n samples at `in` on the device, the window they are of their signal, the emitted count, and where
// emitted sample 0 goes.  Rows of one call may lie in unrelated buffers.
struct PostRow { const float* in; void* out; int32_t n; RowsWindow w; int32_t cnt; };

// The windows of a call after its checks, per row (B entries) or ONE for every row, and per row the emitted count
struct RowsWindows {
    std::vector<RowsWindow> w; std::vector<int32_t> cnt; long cnt_max = 0;
    const RowsWindow& at(int b) const { return w[w.size() == 1 ? 0 : (size_t)b]; }
};

// Every row converted as a signal of its own length len[b] * mul, held from sample in_origin on and zero elsewhere: per row the outputs
// [out_begin, out_begin + cnt[b]) (out_count -1: to the end of the row's signal), and the longest of them.
struct RsPlan { RowsWindow w; long out_max = 0; std::vector<long> cnt; };

// The three ways a window reaches the denoiser and the limiter: none (the whole rows), ONE for the call (_ex), one per row (_rows)
struct WindowsIn { enum Form { WHOLE, ONE, PER_ROW } form = WHOLE; RowsWindow one; const zvx_row_window* rows = nullptr; };

// the least length of a non-empty row: zvx_melspec's conditions (a mirror exists on both sides, one whole frame)
inline int dn_min_samples(const DnGeom& g) { return std::max(g.pad + 1, g.n_fft - 2 * g.pad); }

inline int dn_frames(const DnGeom& g, long n) { return n > 0 ? (int)(1 + (n + 2 * g.pad - g.n_fft) / g.hop) : 0; }

inline double dn_fft_flops(const DnGeom& g, double frames, int transforms) { return transforms * frames * 5.0 * g.n_fft * g.log2n; }

// ---- zvx.hip: the generator
void run_vocoder(zvx_ctx* c, const float* mel, int ldm, int Lmel_max, const int* mel_len_host, const int* P_host, int B,
                 void* wav_dev, long wav_stride, int pcm16);

// ---- host_post.hip: rows contract, planners and parameter checks of the effects, their run_*_rows, their entry functions
RowsInfo rows_check(const char* who, const void* in, const int32_t* nsamples, int B, int Nmax, int max_rows = INT32_MAX);
void flags_check(const char* who, int flags, int allowed);
void out_rows_check(const char* who, const void* in, const void* out, int64_t out_stride, int Nmax, int flags);
const float* rows_to_device(zvx_ctx* c, const std::string& prefix, const float* in, int B, int Nmax, int flags);
DevRows stage_rows(zvx_ctx* c, const std::string& prefix, const float* in, const int32_t* nsamples, int B, int Nmax, int flags);
void rs_pair(int rate_in, int rate_out, int* L, int* M);
RsPlan rs_plan(const int* len, int mul, int B, int L, int M, long in_origin = 0, long out_begin = 0, long out_count = -1);
std::vector<PostRow> plan_rows(const RsPlan& p, const float* x, long x_bs, void* out, long out_bs, size_t ss, const int* len, int mul, int B);
const zvx_ctx::RsBank& rs_bank(zvx_ctx* c, int L, int M);
void run_resample_rows(zvx_ctx* c, const zvx_ctx::RsBank& bk, const PostRow* rows, int B, int pcm16, long zero_to = -1);
int model_rate(const zvx_ctx* c);
void do_resample(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out, int64_t out_stride,
                 int32_t* out_len, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count);
void join_check(const char* who, const void* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap, const zvx_join_params* p);
const int* bounds_to_host(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* p, int flags);
void do_trim_bounds(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* p, int32_t* begin, int32_t* end, int flags);
void do_join(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap, const zvx_join_params* p, void* out,
             int64_t out_capacity, int64_t* out_len, int64_t* seg_pos, int32_t* seg_begin, int32_t* seg_len, int flags);
const double* limit_win(zvx_ctx* c, int W);
int32_t window_count_row(const char* who, const RowsWindow& w, int32_t nsamples, int b, int64_t R, int64_t Rr = -1);
void limit_os_check(const char* who, int os);
int limit_params_check(const char* who, int rate, const zvx_limit_params* p);
const float* run_limit_rows(zvx_ctx* c, const char* who, const PostRow* rows, int B, const zvx_limit_params* p, int W, int pcm16, int measure_os = 0);
void do_limit(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_limit_params* p,
              int oversample, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags, const WindowsIn& win = {});
const LoudCoef& loud_coef(zvx_ctx* c, int rate);
LevelGeom level_params_check(const char* who, int rate, const zvx_level_params* p);
void level_clamped_support_check(const char* who, const RowsWindows& rw, const int32_t* nsamples, int B, const LevelGeom& g);
const float* run_level_rows(zvx_ctx* c, const PostRow* rows, int B, int rate, const zvx_level_params* p, const LevelGeom& g, int pcm16);
void do_level(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* p,
              void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags, const WindowsIn& win = {});
DnGeom dn_geom(const zvx_ctx* c, const char* who);
void stft_len_check(const char* who, const DnGeom& g, int b, int32_t n, const RowsWindow& w = {});
const zvx_ctx::DnTables& dn_tables(zvx_ctx* c, const DnGeom& g);
DnGeom denoise_params_check(const zvx_ctx* c, const char* who, const float* bias, const zvx_denoise_params* p);
void run_denoise_rows(zvx_ctx* c, const DnGeom& g, const PostRow* rows, int B, const float* bias, const zvx_denoise_params* p, int pcm16);
void do_denoise(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias, const zvx_denoise_params* p,
                void* out, int64_t out_stride, int flags, const WindowsIn& win = {});
WmPlan watermark_params_check(const zvx_ctx* c, const char* who, const zvx_watermark_params* p);
const signed char* wm_sign_table(zvx_ctx* c, const zvx_watermark_params* p, int J);
void run_watermark_rows(zvx_ctx* c, const WmPlan& wp, const PostRow* rows, int B, const zvx_watermark_params* p, int pcm16,
                        const uint64_t* keys = nullptr);
void do_watermark(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* p,
                  void* out, int64_t out_stride, int flags, const WindowsIn& win = {}, const uint64_t* keys = nullptr);
void do_resample_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out, int64_t out_stride,
                      int32_t* out_len, int flags, const zvx_row_window* win);
void do_denoise_bias(zvx_ctx* c, float* bias);
void do_fir(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay,
            void* out, int64_t out_stride, int flags, const WindowsIn& win = {});

// ---- host_stream.hip: stream sessions
void stream_free(zvx_stream* s);
void do_stream_open(zvx_ctx* c, const char* who, const float* mel, int frames, const zvx_stream_params* p, const zvx_stream_stages* more, int flags,
                    zvx_stream** out);
void do_stream_next(zvx_stream* s, void* out, int64_t capacity, int64_t* n_out, int32_t* done, int flags);
void do_stream_next_many(zvx_ctx* c, zvx_stream* const* ss, int n, void* const* out, const int64_t* capacity, int64_t* n_out, int32_t* done,
                         int flags);
void do_stream_info(const zvx_stream* s, int64_t* info, int n_info);

// ---- the frame of every entry point of the C-ABI (zvx.hip, host_comm.hip)
template <typename F>
zvx_status guarded(zvx_ctx* ctx, F&& f) {
    if (!ctx) return ZVX_E_INVALID;
    try {
        HIPCHK(hipSetDevice(ctx->device));
        const bool outer = ctx->api_depth++ == 0;               // (an entry point that calls another one keeps the outer call's arena)
        struct End { zvx_ctx* c; ~End() { try { if (--c->api_depth == 0) c->arena_end(); } catch (...) {} } } end{ctx};
        if (outer) ctx->arena_begin();
        f();
        return ZVX_OK;
    } catch (const ZvxError& e) {
        ctx->err = e.what();
        ctx->quiesce_side_streams();
        return e.code;
    } catch (const std::exception& e) {
        ctx->err = e.what();
        ctx->quiesce_side_streams();
        return ZVX_E_INVALID;
    }
}


}  // namespace zvx::host

#endif  // ZVX_HOST_H
