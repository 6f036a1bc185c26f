// zvx_ktest.hip -- test-only C shim over the launchers of libzvx (tests/test_kernels_gpu.py, tests/kernel_ref.py).
// Host code only (but for k_math_probe, which calls nothing of the project): it is linked from the SAME object files as
// libzvx.so (zerovox_amd/build.py), so the kernels under test are the shipped ones.  Every entry point is a plain C function with
// the zvxk_ prefix; the argument structs are mirrored in Python with ctypes, and zvxk_sizeof / zvxk_offsetof let the tests hold
// that mirror to the compiled layout.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include "../../zerovox_amd/csrc/zvx_kernels.h"
#include "../../zerovox_amd/csrc/watermark_kernels.h"
#include "../../zerovox_amd/csrc/spectral_fft.h"

using namespace zvx;

namespace {
int hip_status(hipError_t e) { return e == hipSuccess ? 0 : -(1000 + (int)e); }
int sync_status() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_status(e);
    return hip_status(hipDeviceSynchronize());
}

struct Field { const char* st; const char* name; size_t off; };
#define F_(S, f) {#S, #f, offsetof(S, f)}
const Field kFields[] = {
    F_(GemmArgs, X), F_(GemmArgs, x_bs), F_(GemmArgs, x_hs), F_(GemmArgs, ldx), F_(GemmArgs, W), F_(GemmArgs, w_bs), F_(GemmArgs, w_hs),
    F_(GemmArgs, w_ts), F_(GemmArgs, ldw), F_(GemmArgs, Wp), F_(GemmArgs, halo_l), F_(GemmArgs, halo_r), F_(GemmArgs, Wp2),
    F_(GemmArgs, bias1), F_(GemmArgs, dv1), F_(GemmArgs, fused), F_(GemmArgs, slope1), F_(GemmArgs, no_pairstream), F_(GemmArgs, dtype),
    F_(GemmArgs, M), F_(GemmArgs, N), F_(GemmArgs, K), F_(GemmArgs, nbatch), F_(GemmArgs, nheads), F_(GemmArgs, in_len),
    F_(GemmArgs, out_len), F_(GemmArgs, k_len), F_(GemmArgs, in_len_static), F_(GemmArgs, ntaps), F_(GemmArgs, du), F_(GemmArgs, dv),
    F_(GemmArgs, stride), F_(GemmArgs, wout), F_(GemmArgs, hin), F_(GemmArgs, win), F_(GemmArgs, flat_win), F_(GemmArgs, flat_rows),
    F_(GemmArgs, bflat), F_(GemmArgs, X2), F_(GemmArgs, x2_bs), F_(GemmArgs, ldx2), F_(GemmArgs, K2), F_(GemmArgs, xcd_flat),
    F_(GemmArgs, slab_small), F_(GemmArgs, out_split3), F_(GemmArgs, alpha), F_(GemmArgs, bias), F_(GemmArgs, bias_mode),
    F_(GemmArgs, res), F_(GemmArgs, r_bs), F_(GemmArgs, r_hs), F_(GemmArgs, ldr), F_(GemmArgs, res_dtype), F_(GemmArgs, res_mode),
    F_(GemmArgs, res_inv_slope), F_(GemmArgs, accum), F_(GemmArgs, a_bs), F_(GemmArgs, lda), F_(GemmArgs, accum_mode),
    F_(GemmArgs, accum_dtype), F_(GemmArgs, out_scale), F_(GemmArgs, act), F_(GemmArgs, slope), F_(GemmArgs, post_scale),
    F_(GemmArgs, post_shift), F_(GemmArgs, out), F_(GemmArgs, o_bs), F_(GemmArgs, o_hs), F_(GemmArgs, ldo), F_(GemmArgs, out_dtype),
    F_(GemmArgs, se_part), F_(GemmArgs, se_part_S), F_(GemmArgs, ds_out), F_(GemmArgs, ds_Wp), F_(GemmArgs, ds_bias), F_(GemmArgs, flops),
    F_(FlashArgs, qk), F_(FlashArgs, qk_bs), F_(FlashArgs, ldq), F_(FlashArgs, k_off), F_(FlashArgs, vt), F_(FlashArgs, vt_bs),
    F_(FlashArgs, ldv), F_(FlashArgs, out), F_(FlashArgs, o_bs), F_(FlashArgs, ldo), F_(FlashArgs, len), F_(FlashArgs, L), F_(FlashArgs, D),
    F_(FlashArgs, nheads), F_(FlashArgs, nbatch), F_(FlashArgs, scale), F_(FlashArgs, f16), F_(FlashArgs, prof),
    F_(AttnF32Args, qkv), F_(AttnF32Args, bs), F_(AttnF32Args, ld), F_(AttnF32Args, q_off), F_(AttnF32Args, k_off), F_(AttnF32Args, v_off),
    F_(AttnF32Args, out), F_(AttnF32Args, o_bs), F_(AttnF32Args, ldo), F_(AttnF32Args, planes), F_(AttnF32Args, planes_C),
    F_(AttnF32Args, planes_f16), F_(AttnF32Args, len), F_(AttnF32Args, L), F_(AttnF32Args, D), F_(AttnF32Args, nheads),
    F_(AttnF32Args, nbatch), F_(AttnF32Args, scale),
    F_(StreamArgs, X), F_(StreamArgs, x_bs), F_(StreamArgs, ldx), F_(StreamArgs, W1), F_(StreamArgs, W2), F_(StreamArgs, b1), F_(StreamArgs, b2),
    F_(StreamArgs, dil), F_(StreamArgs, C), F_(StreamArgs, ntaps), F_(StreamArgs, npair), F_(StreamArgs, out), F_(StreamArgs, o_bs),
    F_(StreamArgs, ldo), F_(StreamArgs, accum), F_(StreamArgs, a_bs), F_(StreamArgs, lda), F_(StreamArgs, accum_mode), F_(StreamArgs, slope1),
    F_(StreamArgs, res_inv_slope), F_(StreamArgs, out_scale), F_(StreamArgs, slope), F_(StreamArgs, len), F_(StreamArgs, M),
    F_(StreamArgs, nbatch), F_(StreamArgs, S), F_(StreamArgs, nseg), F_(StreamArgs, dX0), F_(StreamArgs, dT), F_(StreamArgs, dX),
    F_(StreamArgs, flops), F_(StreamArgs, prof), F_(StreamArgs, seg_min), F_(StreamArgs, f16),
    F_(StageArgs, X), F_(StageArgs, x_bs), F_(StageArgs, ldx), F_(StageArgs, W), F_(StageArgs, woff), F_(StageArgs, bias), F_(StageArgs, C),
    F_(StageArgs, nk), F_(StageArgs, ks), F_(StageArgs, dil), F_(StageArgs, out), F_(StageArgs, o_bs), F_(StageArgs, ldo), F_(StageArgs, slope1),
    F_(StageArgs, res_inv_slope), F_(StageArgs, slope), F_(StageArgs, len), F_(StageArgs, M), F_(StageArgs, nbatch), F_(StageArgs, f16),
    F_(WmDetectRow, x), F_(WmDetectRow, d), F_(WmDetectRow, n), F_(WmDetectRow, F),
    F_(WmDetectArgs, rows), F_(WmDetectArgs, B), F_(WmDetectArgs, n_fft), F_(WmDetectArgs, log2n), F_(WmDetectArgs, hop), F_(WmDetectArgs, pad),
    F_(WmDetectArgs, Fmax), F_(WmDetectArgs, twid), F_(WmDetectArgs, win), F_(WmDetectArgs, sign), F_(WmDetectArgs, k_lo), F_(WmDetectArgs, KB),
    F_(WmDetectArgs, J), F_(WmDetectArgs, TB), F_(WmDetectArgs, P), F_(WmDetectArgs, WF), F_(WmDetectArgs, NW), F_(WmDetectArgs, win_score),
    F_(WmDetectArgs, win_offset),
};
#undef F_

__global__ void k_math_probe(int fn, const float* in, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    out[i] = fn == 0 ? expf(x) : fn == 1 ? tanhf(x) : fn == 2 ? logf(x) : fn == 3 ? sqrtf(x) : 1.0f / x;
}

// dn_fft of spectral_fft.h and nothing else: DENOISE_POINTS complex points (DENOISE_POINTS >> log2n frames) into LDS at dn_at, the
// transform, the planes back.  No window, no scaling.
template <bool INV>
__global__ __launch_bounds__(DN_THREADS) void k_fft_probe(float* re, float* im, const float2* twid, int log2n) {
    __shared__ float sre[DN_PLANE], sim[DN_PLANE];
    const int tid = threadIdx.x;
    for (int i = tid; i < DENOISE_POINTS; i += DN_THREADS) { sre[dn_at(i)] = re[i]; sim[dn_at(i)] = im[i]; }
    __syncthreads();
    dn_fft<INV>(sre, sim, twid, log2n, tid);
    for (int i = tid; i < DENOISE_POINTS; i += DN_THREADS) { re[i] = sre[dn_at(i)]; im[i] = sim[dn_at(i)]; }
}
}  // namespace

extern "C" {

// ---- device memory ----
void* zvxk_alloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess ? p : nullptr; }
int zvxk_free(void* p) { return hip_status(hipFree(p)); }
int zvxk_h2d(void* dst, const void* src, size_t bytes) { return hip_status(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
int zvxk_d2h(void* dst, const void* src, size_t bytes) { return hip_status(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }
int zvxk_memset(void* dst, int value, size_t bytes) { return hip_status(hipMemset(dst, value, bytes)); }
int zvxk_sync() { return sync_status(); }

// ---- launchers ----
// variant id (>= 0) or the launcher's negative refusal; a HIP error after the launch is returned as -(1000 + code)
int zvxk_gemm(const GemmArgs* a, int dry_run) {
    if (dry_run) return gemm_variant_of(*a);
    const int id = a->fused == 2 ? launch_rb2fuse(*a, nullptr) : (a->fused ? launch_resfuse(*a, nullptr) : launch_gemm(*a, nullptr));
    const int st = sync_status();
    return st < 0 ? st : id;
}
int zvxk_epi_mode(const GemmArgs* a) { return gemm_epi_mode_of(*a); }
size_t zvxk_packed_weight_elems(int ntaps, int N, int K) { return packed_weight_elems(ntaps, N, K); }
int zvxk_pack_weights(const void* w16, int ntaps, int N, int K, void* out) {
    launch_pack_weights(w16, ntaps, N, K, out, nullptr);
    return sync_status();
}
int zvxk_pack_pair(const void* pa, int ntapsA, int KA, const void* pb, int ntapsB, int KB, int N, void* out) {
    launch_pack_pair(pa, ntapsA, KA, pb, ntapsB, KB, N, out, nullptr);
    return sync_status();
}
// 1 launched (or, dry_run, covered), 0 refused, < 0 HIP error
int zvxk_flash(const FlashArgs* a, int dry_run) {
    const bool ok = launch_flash_attention(*a, nullptr, dry_run != 0);
    if (dry_run || !ok) return ok ? 1 : 0;
    const int st = sync_status();
    return st < 0 ? st : 1;
}
int zvxk_attn_f32(const AttnF32Args* a, int dry_run) {
    const bool ok = launch_attention_f32(*a, nullptr, dry_run != 0);
    if (dry_run || !ok) return ok ? 1 : 0;
    const int st = sync_status();
    return st < 0 ? st : 1;
}
// streaming ResBlock chain (resstream.hip): variant id (20 / 21) or -1 when the launcher refuses; < -1000: HIP error
int zvxk_resstream(const StreamArgs* a, int dry_run) {
    const int id = launch_resstream(*a, nullptr, dry_run != 0);
    if (dry_run || id < 0) return id;
    const int st = sync_status();
    return st < 0 ? st : id;
}
// a whole narrow stage (narrowstage.hip): 1 launched (or, dry_run, covered), 0 refused, < 0 HIP error
int zvxk_narrowstage(const StageArgs* a, int dry_run) {
    const bool ok = launch_narrowstage(*a, nullptr, dry_run != 0);
    if (dry_run || !ok) return ok ? 1 : 0;
    const int st = sync_status();
    return st < 0 ? st : 1;
}
int zvxk_pack_narrow(const void* w16, int k, int C, void* out) {
    launch_pack_narrow(w16, k, C, out, nullptr);
    return sync_status();
}
int zvxk_narrowstage_steps(int C, int k) { return narrowstage_steps(C, k); }
int zvxk_num_cus() { return num_cus(); }
const char* zvxk_variant_name(int id) { return (id >= 0 && id < gemm_num_variants()) ? gemm_variant_name(id) : nullptr; }
int zvxk_num_variants() { return gemm_num_variants(); }

// ---- the small kernels of ops.hip (tests/test_ops_gpu.py, tests/ops_ref.py): the launcher's own parameter list without the stream ----
#define ZK_(call) do { call; return sync_status(); } while (0)
int zvxk_cast(const void* in, int in_dt, void* out, int out_dt, size_t n) { ZK_(launch_cast(in, in_dt, out, out_dt, n, nullptr)); }
int zvxk_f32_to_bf16(const float* in, bf16_t* out, size_t n) { ZK_(launch_f32_to_bf16(in, out, n, nullptr)); }
int zvxk_transpose16(const void* in, int ld_in, void* out, int ld_out, int B, int rows, int C, const int* len) { ZK_(launch_transpose16(in, ld_in, out, ld_out, B, rows, C, nullptr, len)); }
int zvxk_zero_tail_cols(void* x, int es, long ld, long bs, int B, int rows, int cols, const int* len) { ZK_(launch_zero_tail_cols(x, es, ld, bs, B, rows, cols, len, nullptr)); }
int zvxk_split3(const float* x, int ldx, void* out, int B, int rows_max, const int* rows, int C, int f16) { ZK_(launch_split3(x, ldx, out, B, rows_max, rows, C, nullptr, f16)); }
int zvxk_split3_weights(const float* w, void* out, long nrows, int K, int f16, float scale) { ZK_(launch_split3_weights(w, out, nrows, K, nullptr, f16, scale)); }
int zvxk_absmax(const float* x, size_t n, float* out) { ZK_(launch_absmax(x, n, out, nullptr)); }
int zvxk_embed(const int* ph, const int* pu, const float* emb, int ed, const float* pemb, int pd, const float* pe, float* out, int B, int Tmax, const int* T) {
    ZK_(launch_embed(ph, pu, emb, ed, pemb, pd, pe, out, B, Tmax, T, nullptr));
}
int zvxk_layernorm(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int rows_max, const int* rows, int C, int mode, float eps,
                   const float* gamma, const float* beta, const float* bg, long bg_bs, const float* post_add, void* planes, int planes_f16) {
    ZK_(launch_layernorm(x, x_dt, ldx, y, y_dt, ldy, B, rows_max, rows, C, mode, eps, gamma, beta, bg, bg_bs, post_add, nullptr, planes, planes_f16));
}
int zvxk_softmax_rows(const float* sc, int lds, void* P, int p_dt, int ldp, int nbatch, int nheads, int Lmax, const int* len) {
    ZK_(launch_softmax_rows(sc, lds, P, p_dt, ldp, nbatch, nheads, Lmax, len, nullptr));
}
int zvxk_rowdot(const float* x, int ldx, const float* w, float bias, float* out, int B, int Tmax, const int* T, int C) { ZK_(launch_rowdot(x, ldx, w, bias, out, B, Tmax, T, C, nullptr)); }
int zvxk_bucket_embed_add(const float* pred, const float* table, int nbins, float* x, int ldx, int C, int* idx, int B, int Tmax, const int* T) {
    ZK_(launch_bucket_embed_add(pred, table, nbins, x, ldx, C, idx, B, Tmax, T, nullptr));
}
int zvxk_bucket_embed_add_ctl(const float* pred, const float* shift, const float* range, const float* target, const float* table, int nbins, float* x,
                              int ldx, int C, int* idx, int B, int Tmax, const int* T) {
    ZK_(launch_bucket_embed_add_ctl(pred, shift, range, target, table, nbins, x, ldx, C, idx, B, Tmax, T, nullptr));
}
int zvxk_durations(const int* forced, const float* logd, int* dur, int* cum, int* mel_len, int B, int Tmax, const int* T) {
    ZK_(launch_durations(forced, logd, dur, cum, mel_len, B, Tmax, T, nullptr));
}
int zvxk_durations_q16(const int* forced, const float* logd, const int* q, int* dur, int* cum, int* mel_len, int B, int Tmax, const int* T) {
    ZK_(launch_durations_q16(forced, logd, q, dur, cum, mel_len, B, Tmax, T, nullptr));
}
int zvxk_length_regulate(const float* x, int ldx, const int* cum, const int* T, const int* mel_len, float* feats, int B, int Tmax, int Lmax, int C) {
    ZK_(launch_length_regulate(x, ldx, cum, T, mel_len, feats, B, Tmax, Lmax, C, nullptr));
}
int zvxk_add_pe_cast(const float* x, const float* pe, void* y, int y_dt, int ldy, int B, int Lmax, const int* L, int C, int out_rows_max) {
    ZK_(launch_add_pe_cast(x, pe, y, y_dt, ldy, B, Lmax, L, C, nullptr, out_rows_max));
}
int zvxk_instnorm_stats(const void* x, int x_dt, int ldx, int B, int Lmax, const int* L, int C, float eps, float* mean, float* rstd) {
    ZK_(launch_instnorm_stats(x, x_dt, ldx, B, Lmax, L, C, eps, mean, rstd, nullptr));
}
int zvxk_norm_affine_act(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax, const int* L, int C, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, long g_bs, int one_plus, int act, float slope) {
    ZK_(launch_norm_affine_act(x, x_dt, ldx, y, y_dt, ldy, B, Lmax, L, C, mean, rstd, gamma, beta, g_bs, one_plus, act, slope, nullptr));
}
int zvxk_instnorm_fused(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax, const int* L, int C, float eps, float* mean,
                        float* rstd, const float* gamma, const float* beta, long g_bs, int one_plus, int act, float slope) {
    ZK_(launch_instnorm_fused(x, x_dt, ldx, y, y_dt, ldy, B, Lmax, L, C, eps, mean, rstd, gamma, beta, g_bs, one_plus, act, slope, nullptr));
}
int zvxk_mel_pad(const void* mel, int m_dt, int ldm, int Lmax, const int* mel_len, void* v, int v_dt, int ldv, int Pmax, const int* P, int B, int nm) {
    ZK_(launch_mel_pad(mel, m_dt, ldm, Lmax, mel_len, v, v_dt, ldv, Pmax, P, B, nm, nullptr));
}
int zvxk_copy_rows_f32(const void* src, int s_dt, int lds, long s_bs, float* dst, long ldd, long d_bs, int B, int rows_max, const int* rows, int C) {
    ZK_(launch_copy_rows_f32(src, s_dt, lds, s_bs, dst, ldd, d_bs, B, rows_max, rows, C, nullptr));
}
int zvxk_conv_post_tanh(const void* x, int x_dt, int ldx, long x_bs, const float* w, float bias, int ktaps, int C, void* wav, long wav_bs, int pcm16,
                        int B, int Nmax, const int* in_len, int len_mul, const int* out_len, int out_mul) {
    ZK_(launch_conv_post_tanh(x, x_dt, ldx, x_bs, w, bias, ktaps, C, wav, wav_bs, pcm16, B, Nmax, in_len, len_mul, out_len, out_mul, nullptr));
}
int zvxk_count_sat16(const void* x, long bs, int ld, int B, int rows_max, const int* rows, int C, unsigned long long* count) {
    ZK_(launch_count_sat16(x, bs, ld, B, rows_max, rows, C, count, nullptr));
}
int zvxk_zero_tail_rows(float* x, int ldx, int B, int rows_max, const int* rows, int C) { ZK_(launch_zero_tail_rows(x, ldx, B, rows_max, rows, C, nullptr)); }
int zvxk_spk_front(const float* mels, int Tmax, const int* lens, int F, const float* mean, const float* rstd, const float* w, const float* bias,
                   const float* bn_scale, const float* bn_shift, int C0, void* out, int o_dt, int B, int Wout) {
    ZK_(launch_spk_front(mels, Tmax, lens, F, mean, rstd, w, bias, bn_scale, bn_shift, C0, out, o_dt, B, Wout, nullptr));
}
int zvxk_se_pool_splits(int H, int Wmax) { return se_pool_splits(H, Wmax); }
int zvxk_se_pool(const void* x, int x_dt, int B, int H, int Wmax, const int* W, int C, float* partial) { ZK_(launch_se_pool(x, x_dt, B, H, Wmax, W, C, partial, nullptr)); }
int zvxk_se_fc(const float* partial, int S, int H, const int* W, const float* w1, const float* b1, const float* w2, const float* b2, int C, int Cr,
               float* scale, int B, const float* pool_bias) {
    ZK_(launch_se_fc(partial, S, H, W, w1, b1, w2, b2, C, Cr, scale, B, nullptr, pool_bias));
}
int zvxk_se_apply(const void* x, const void* res, void* y, int dt, const float* scale, int B, int H, int Wmax, const int* W, int C) {
    ZK_(launch_se_apply(x, res, y, dt, scale, B, H, Wmax, W, C, nullptr));
}
int zvxk_asp_pool(const void* x, int x_dt, const float* logits, int B, int F, int Wmax, const int* W, int C, float* out, int with_std) {
    ZK_(launch_asp_pool(x, x_dt, logits, B, F, Wmax, W, C, out, with_std, nullptr));
}
int zvxk_l2norm_rows(float* x, int B, int C) { ZK_(launch_l2norm_rows(x, B, C, nullptr)); }
int zvxk_reflect_pad(const float* wav, long w_bs, const int* n, float* out, long o_bs, int pad, int B, int out_cols) {
    ZK_(launch_reflect_pad(wav, w_bs, n, out, o_bs, pad, B, out_cols, nullptr));
}
int zvxk_stft_mag(const float* spec, int lds_, float* mag, int ldm, int nf, int B, int Tmax, const int* frames) {
    ZK_(launch_stft_mag(spec, lds_, mag, ldm, nf, B, Tmax, frames, nullptr));
}
int zvxk_log_clip(float* x, int ldx, int C, float lo, int B, int Tmax, const int* frames) { ZK_(launch_log_clip(x, ldx, C, lo, B, Tmax, frames, nullptr)); }
int zvxk_fc_rows(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int ldo, int B, int N, int K) {
    ZK_(launch_fc_rows(x, ldx, w, ldw, bias, out, ldo, B, N, K, nullptr));
}
#undef ZK_
// The resampler's launch geometry for rate_in -> rate_out, B rows, out_max outputs in the longest row, as the library designs the bank
// (L, M by the gcd, half = 10 max(L, M), T = ceil((2 half + 1) / L), resample_bank_pitch) and as launch_resample_poly decides it; nothing
// is launched.  g[8] = {L, M, T, pitch, tile, tpb, xcap, LDS bytes}.  1: fits, 0: exceeds the LDS of a workgroup.
int zvxk_resample_geometry(int rate_in, int rate_out, int B, long out_max, int* g) {
    int x = rate_in, y = rate_out;
    while (y) { const int t = x % y; x = y; y = t; }
    ResampleArgs a{};
    a.L = rate_out / x; a.M = rate_in / x; a.B = B; a.out_max = out_max;
    if (a.L == 1 && a.M == 1) { a.half = 0; a.T = 1; a.pitch = 2; }
    else { a.half = 10 * (a.L > a.M ? a.L : a.M); a.T = (2 * a.half + 1 + a.L - 1) / a.L; a.pitch = resample_bank_pitch(a.L, a.M, a.T); }
    ResampleGeometry r;
    const bool ok = resample_geometry_of(a, &r);
    g[0] = a.L; g[1] = a.M; g[2] = a.T; g[3] = a.pitch; g[4] = r.tile; g[5] = r.tpb; g[6] = r.xcap; g[7] = (int)r.lds;
    return ok ? 1 : 0;
}
// the device's own math functions over given arguments (the per-call ulp allowances of tests/ops_ref.py were measured with it; it
// touches no code under test).  fn: 0 expf, 1 tanhf, 2 logf, 3 sqrtf, 4 1 / x
int zvxk_math_probe(int fn, const float* in, float* out, int n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, in, out, n);
    return sync_status();
}

// ---- the spectral family (tests/test_spectral_gpu.py, tests/spectral_ref.py) ----
// dn_fft alone over DENOISE_POINTS points in place; twid: n_fft (cos, -sin) pairs as dn_tables designs them; log2n in 2 .. 12
int zvxk_fft_probe(float* re, float* im, const float* twid, int log2n, int inverse) {
    if (log2n < 2 || (1 << log2n) > DENOISE_POINTS) return -1;
    if (inverse) hipLaunchKernelGGL(k_fft_probe<true>, dim3(1), dim3(DN_THREADS), 0, nullptr, re, im, (const float2*)twid, log2n);
    else hipLaunchKernelGGL(k_fft_probe<false>, dim3(1), dim3(DN_THREADS), 0, nullptr, re, im, (const float2*)twid, log2n);
    return sync_status();
}
// the detector's two launches on a hand-built row table (a->rows on the device)
int zvxk_wm_bands(const WmDetectArgs* a) { launch_wm_bands(*a, nullptr); return sync_status(); }
int zvxk_wm_search(const WmDetectArgs* a) { launch_wm_search(*a, nullptr); return sync_status(); }
int zvxk_wm_table() { return WM_TABLE; }

// ---- layout of the argument structs ----
long zvxk_sizeof(const char* name) {
    if (!strcmp(name, "GemmArgs")) return (long)sizeof(GemmArgs);
    if (!strcmp(name, "FlashArgs")) return (long)sizeof(FlashArgs);
    if (!strcmp(name, "AttnF32Args")) return (long)sizeof(AttnF32Args);
    if (!strcmp(name, "StreamArgs")) return (long)sizeof(StreamArgs);
    if (!strcmp(name, "StageArgs")) return (long)sizeof(StageArgs);
    if (!strcmp(name, "WmDetectRow")) return (long)sizeof(WmDetectRow);
    if (!strcmp(name, "WmDetectArgs")) return (long)sizeof(WmDetectArgs);
    return -1;
}
long zvxk_offsetof(const char* st, const char* field) {
    for (const Field& f : kFields)
        if (!strcmp(f.st, st) && !strcmp(f.name, field)) return (long)f.off;
    return -1;
}
int zvxk_num_fields() { return (int)(sizeof(kFields) / sizeof(kFields[0])); }
const char* zvxk_field(int i, int which) { return (i < 0 || i >= zvxk_num_fields()) ? nullptr : (which ? kFields[i].name : kFields[i].st); }

}  // extern "C"
