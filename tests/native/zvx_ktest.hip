// zvx_ktest.hip -- test-only C shim over the launchers of libzvx (tests/test_kernels_gpu.py, tests/kernel_ref.py).
// Host code only: it is linked from the SAME object files as libzvx.so (zerovox_amd/build.py), so the kernels under test are the
// shipped ones.  Every entry point is a plain C function with the zvxk_ prefix; the argument structs are mirrored in Python with
// ctypes, and zvxk_sizeof / zvxk_offsetof let the tests hold that mirror to the compiled layout.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include "../../zerovox_amd/csrc/zvx_kernels.h"

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
};
#undef F_
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

// ---- layout of the argument structs ----
long zvxk_sizeof(const char* name) {
    if (!strcmp(name, "GemmArgs")) return (long)sizeof(GemmArgs);
    if (!strcmp(name, "FlashArgs")) return (long)sizeof(FlashArgs);
    if (!strcmp(name, "AttnF32Args")) return (long)sizeof(AttnF32Args);
    if (!strcmp(name, "StreamArgs")) return (long)sizeof(StreamArgs);
    if (!strcmp(name, "StageArgs")) return (long)sizeof(StageArgs);
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
