// gemm.hip -- the MFMA kernels of the synthesis path on gfx950.  See GemmArgs in zvx_kernels.h.
//
//   gemm_kernel             generic gathered-row GEMM (this comment): f32 path, attention products, 2-D taps
//   convslab_kernel         bf16 1-D convs / linears against static weights: slab in LDS, fragment-packed weight stream
//   convreg_kernel          single square convs with C <= 64: all weight fragments in registers
//   rb2fuse_kernel          a whole ResBlock2 (two dilated convolutions + residuals), one tile per workgroup (HiFi-GAN V3)
//   resfuse_persist_kernel  fused ResBlock1 pair, persistent + wave-specialised (C = 8 .. 128)
//   epilogue / epilogue_rows / epilogue_direct   MFMA-layout, LDS-transposed row-major, and bf16-staged epilogues
//
// The generic kernel covers every contraction shape of the path: dilated Conv1d (HiFi-GAN ResBlocks,
// hifigan.py:25-86; FFN conv k=9, fs2.py:175-187; StyleTTS k=3 convs, styletts.py:28-29), polyphase
// ConvTranspose1d (hifigan.py:100-103), Linear (fs2.py:118-128), the attention products (fs2.py:49-56)
// and the ResNet Conv2d (ResNetSE34V2.py:74-76) via 2-D taps.
//
// Mapping to CDNA4: a 256-thread workgroup (4 waves) owns a BM(time) x BN(channel) output tile.  Both
// operands are K-contiguous in HBM and are staged as 64-byte K-slices (32 bf16 / 16 f32) through LDS with
// an 80-byte row pitch (conflict-free ds_read_b128 for 16 distinct rows).  Weights feed MFMA srcA and
// activations srcB, so every lane ends up holding 4 consecutive CHANNELS of one time row per accumulator
// quad: the epilogue reads/writes 8-byte (bf16) / 16-byte (f32) vectors of the time-major tensors.
//   bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulate.    f32: v_mfma_f32_32x32x2_f32 (exact f32 fma chain).
// Global loads of K-step s+1 are issued before the MFMAs of step s and written to the other LDS buffer
// afterwards (one barrier per step).  blockIdx is remapped so each XCD walks a contiguous tile range
// (all channel tiles of a time tile share that XCD's L2).
#include "mfma_util.h"
#include "zvx_kernels.h"

#include <cstring>
#include <type_traits>

// (gemm.hip is compiled as TWO translation units -- zerovox_amd/build.py: -DZVX_GEMM_PART=1 = everything but the fused ResBlock-pair kernels,
// -DZVX_GEMM_PART=2 = those kernels and launch_resfuse() -- so that a clean build takes the time of the larger half; no macro: one unit)
#ifndef ZVX_GEMM_PART
#define ZVX_GEMM_PART 0
#endif
#define ZVX_PART_MAIN (ZVX_GEMM_PART != 2)
#define ZVX_PART_RESFUSE (ZVX_GEMM_PART != 1)
#if ZVX_GEMM_PART == 2
extern thread_local bool zvx_gemm_dry_run;
#else
thread_local hipEvent_t zvx_gemm_ev_start = nullptr, zvx_gemm_ev_stop = nullptr;     // the launchers' shared event pair (zvx_kernels.h)
thread_local bool zvx_gemm_dry_run = false;     // gemm_variant_of(): walk the launcher's decisions without dispatching
#endif
#define g_dry_run zvx_gemm_dry_run

#define ZVX_LAUNCH(...) do { if (!g_dry_run) ZVX_DISPATCH(__VA_ARGS__); } while (0)

namespace zvx {


#define PITCH 80      // bytes per LDS row: 64 B of K + 16 B pad
#define KBYTES 64

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);   // round-to-nearest-even (finite inputs)
    return (unsigned short)(u >> 16);
}

template <int DT>
__device__ __forceinline__ void load4(const void* base, long idx, float v[4]) {
    if (DT == DT_F32) {
        float4 t = *(const float4*)((const float*)base + idx);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        uint2 t = *(const uint2*)((const unsigned short*)base + idx);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    }
}
__device__ __forceinline__ void load4_dyn(const void* base, int dt, long idx, float v[4]) {
    if (dt == DT_F32) load4<DT_F32>(base, idx, v);
    else if (dt == DT_F16) {
        const uint2 t = *(const uint2*)((const unsigned short*)base + idx);
        const f32x2 a = unpack_f16x2(t.x), b = unpack_f16x2(t.y);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else load4<DT_BF16>(base, idx, v);
}
__device__ __forceinline__ void store4_dyn(void* base, int dt, long idx, const float v[4]) {
    if (dt == DT_F32) {
        *(float4*)((float*)base + idx) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (dt == DT_F16) {
        uint2 t;
        t.x = pack_f16x2_sat(v[0], v[1]); t.y = pack_f16x2_sat(v[2], v[3]);
        *(uint2*)((unsigned short*)base + idx) = t;
    } else {
        uint2 t;
        t.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
        t.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
        *(uint2*)((unsigned short*)base + idx) = t;
    }
}

// ---- shared epilogue: lane holds, per 32x32 tile and accumulator quad g, 4 consecutive channels of one time row ----
template <int TM, int TN>
__device__ __forceinline__ void epilogue(const GemmArgs& a, f32x16 (&acc)[TN][TM], int b, int h, int row_base, int col_base,
                                         int out_len, bool two_d, int lane) {
    const long ooff = (long)b * a.o_bs + (long)h * a.o_hs;
    const long roff = (long)b * a.r_bs + (long)h * a.r_hs;
    const long aoff = (long)b * a.a_bs;
#pragma unroll
    for (int j = 0; j < TM; j++) {
        const int r = row_base + j * 32 + (lane & 31);
        bool rok = r < a.M;
        if (two_d) rok = rok && (r % a.wout) < out_len; else rok = rok && r < out_len;
        if (!rok) continue;
        const float brow = (a.bias_mode == 2) ? a.bias[r] : 0.f;
#pragma unroll
        for (int i = 0; i < TN; i++) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int n = col_base + i * 32 + 8 * g + 4 * (lane >> 5);
                if (n >= a.N) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = acc[i][j][4 * g + e] * a.alpha + brow;
                if (a.bias_mode == 1) {
                    const float4 bb = *(const float4*)(a.bias + n);
                    v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w;
                }
                if (a.res_mode) {
                    float rr[4];
                    load4_dyn(a.res, a.res_dtype, roff + (long)r * a.ldr + n, rr);
                    if (a.res_mode == 2) {
#pragma unroll
                        for (int e = 0; e < 4; e++) rr[e] = rr[e] >= 0.f ? rr[e] : rr[e] * a.res_inv_slope;
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] += rr[e];
                }
                if (a.accum_mode) {
                    const long ai = aoff + (long)r * a.lda + n;
                    if (a.accum_mode & 1) {
                        float t[4];
                        load4_dyn(a.accum, a.accum_dtype, ai, t);
                        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
                    }
                    if (a.accum_mode & 2) store4_dyn(a.accum, a.accum_dtype, ai, v);
                }
                if (a.out) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        float t = v[e] * a.out_scale;
                        if (a.act == ACT_RELU) t = fmaxf(t, 0.f);
                        else if (a.act == ACT_LRELU) t = t >= 0.f ? t : t * a.slope;
                        v[e] = t;
                    }
                    if (a.post_scale) {
                        const float4 ps = *(const float4*)(a.post_scale + n), pt = *(const float4*)(a.post_shift + n);
                        v[0] = v[0] * ps.x + pt.x; v[1] = v[1] * ps.y + pt.y;
                        v[2] = v[2] * ps.z + pt.z; v[3] = v[3] * ps.w + pt.w;
                    }
                    store4_dyn(a.out, a.out_dtype, ooff + (long)r * a.ldo + n, v);
                }
            }
        }
    }
}

template <int DT, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
    constexpr int ES = (DT == DT_F32) ? 4 : 2;       // element size
    constexpr int EPC = 16 / ES;                      // elements per 16-byte chunk
    constexpr int BKE = KBYTES / ES;                  // elements per K-step
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int XCH = BM * 4 / 256;                 // X chunks per thread per step
    constexpr int WCH = (BN * 4 + 255) / 256;         // W chunks per thread per step
    static_assert(WM * WN == 4, "4 waves");

    __shared__ __attribute__((aligned(16))) unsigned char lds[2][(BM + BN) * PITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave % WM, wc = wave / WM;

    // ---- tile coordinates (XCD-aware, bijective remap) ----
    const int ntn = (a.N + BN - 1) / BN;
    const int nwg = gridDim.x;
    int wg;
    {
        const int id = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    const int nt = wg % ntn, mt = wg / ntn;
    const int m0 = mt * BM, n0 = nt * BN;
    const int z = blockIdx.y, b = z / a.nheads, h = z - b * a.nheads;

    const int out_len = a.out_len ? a.out_len[b] : a.M;
    const int in_len = a.in_len ? a.in_len[b] : a.in_len_static;
    const bool two_d = a.wout > 0;
    if (!two_d && m0 >= out_len) return;
    if (m0 >= a.M) return;
    int Kb = a.K;
    if (a.k_len) { Kb = (a.k_len[b] + 7) & ~7; if (Kb > a.K) Kb = a.K; }

    const unsigned char* Xp = (const unsigned char*)a.X + ((long)b * a.x_bs + (long)h * a.x_hs) * ES;
    const unsigned char* Wp = (const unsigned char*)a.W + ((long)b * a.w_bs + (long)h * a.w_hs) * ES;

    // ---- per-thread staging roles (fixed across K-steps) ----
    int xu[XCH], xv[XCH];
    const int kc = tid & 3;                            // 16-byte chunk within the 64-byte K-slice
#pragma unroll
    for (int i = 0; i < XCH; i++) {
        const int r = m0 + (tid >> 2) + i * 64;
        if (two_d) { xu[i] = (r / a.wout) * a.stride; xv[i] = (r % a.wout) * a.stride; }
        else { xu[i] = 0; xv[i] = r; }
    }

    const int kchunks = (Kb + BKE - 1) / BKE;
    const int S = a.ntaps * kchunks;

    uint4 xreg[XCH], wreg[WCH];

    auto load_regs = [&](int s) {
        const int tap = s / kchunks;
        const int k = (s - tap * kchunks) * BKE + kc * EPC;
        const bool kok = k < Kb;
        const int du = a.du[tap], dv = a.dv[tap];
#pragma unroll
        for (int i = 0; i < XCH; i++) {
            const int iu = xu[i] + du, iv = xv[i] + dv;
            const bool ok = kok && iu >= 0 && iu < a.hin && iv >= 0 && iv < in_len;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *(const uint4*)(Xp + ((long)(iu * a.win + iv) * a.ldx + k) * ES);
            xreg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < WCH; i++) {
            const int c = tid + i * 256;
            const int n = n0 + (c >> 2);
            uint4 v = make_uint4(0, 0, 0, 0);
            if ((BN * 4 >= 256 * (i + 1) || c < BN * 4) && kok && n < a.N)
                v = *(const uint4*)(Wp + ((long)tap * a.w_ts + (long)n * a.ldw + k) * ES);
            wreg[i] = v;
        }
    };
    auto store_lds = [&](int buf) {
        unsigned char* base = lds[buf];
#pragma unroll
        for (int i = 0; i < XCH; i++)
            *(uint4*)(base + ((tid >> 2) + i * 64) * PITCH + kc * 16) = xreg[i];
#pragma unroll
        for (int i = 0; i < WCH; i++) {
            const int c = tid + i * 256;
            if (BN * 4 >= 256 * (i + 1) || c < BN * 4)
                *(uint4*)(base + (BM + (c >> 2)) * PITCH + kc * 16) = wreg[i];
        }
    };

    f32x16 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; i++)
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

    const int xrow = wr * (BM / WM) + (lane & 31);
    const int wrow = BM + wc * (BN / WN) + (lane & 31);
    const int koff = (lane >> 5) * 16;

    if (S > 0) {
        load_regs(0);
        store_lds(0);
    }
    __syncthreads();
    for (int s = 0; s < S; s++) {
        if (s + 1 < S) load_regs(s + 1);
        const unsigned char* base = lds[s & 1];
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            uint4 xf[TM], wf[TN];
#pragma unroll
            for (int j = 0; j < TM; j++) xf[j] = *(const uint4*)(base + (xrow + j * 32) * PITCH + sub * 32 + koff);
#pragma unroll
            for (int i = 0; i < TN; i++) wf[i] = *(const uint4*)(base + (wrow + i * 32) * PITCH + sub * 32 + koff);
#pragma unroll
            for (int i = 0; i < TN; i++)
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    if (DT == DT_BF16) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, wf[i]), __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
                    } else if (DT == DT_F16) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                            __builtin_bit_cast(f16x8, wf[i]), __builtin_bit_cast(f16x8, xf[j]), acc[i][j], 0, 0, 0);
                    } else {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf[i].x), __uint_as_float(xf[j].x), acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf[i].y), __uint_as_float(xf[j].y), acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf[i].z), __uint_as_float(xf[j].z), acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf[i].w), __uint_as_float(xf[j].w), acc[i][j], 0, 0, 0);
                    }
                }
        }
        if (s + 1 < S) store_lds((s + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue ----
    epilogue<TM, TN>(a, acc, b, h, m0 + wr * (BM / WM), n0 + wc * (BN / WN), out_len, two_d, lane);
}

// ---- row-major epilogue: accumulators -> per-wave LDS transpose -> every lane owns 8 consecutive channels of a row ----
// Global traffic of the epilogue (output, residual, f32 accumulator) becomes full-line: a wave instruction touches
// 8 (NW=64) or 16 (NW=32) rows x 128/64 contiguous bytes instead of 32 rows x 16 bytes.  The per-element arithmetic is kept
// to a handful of VALU ops (all mode switches are wave-uniform branches OUTSIDE the element loops; leaky-relu = max(x, s*x),
// its inverse = min(y, y/s); bf16 packing via the hardware RNE convert): with two waves per SIMD the epilogue is otherwise
// VALU-bound (measured 27k cycles per tile for the branchy per-element version vs 7k for the LDS transposes).
// (pack_bf16x2 / unpack_bf16x2 / lrelu2 / inv_lrelu2 and the IEEE-half helpers: mfma_util.h)
// run-time 16-bit dtype switch of the run-time epilogue (the kernel has NOT set MODE.FP16_OVFL there: saturating converts)
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) { return pack_f16x2_sat(lo, hi); }
__device__ __forceinline__ unsigned pack16x2(float lo, float hi, bool f16) { return f16 ? pack_f16x2_sat(lo, hi) : pack_bf16x2(lo, hi); }
__device__ __forceinline__ f32x2 unpack16x2(unsigned u, bool f16) { return f16 ? unpack_f16x2(u) : unpack_bf16x2(u); }

// Epilogue modes known at compile time (EPI >= 0) cover the HiFi-GAN convolutions: alpha = 1, per-channel bias, bf16
// output (or none), activation none / leaky-relu, bf16 residual in the activated domain, bf16 running sum.
//   bit 0: residual (res_mode 2)   bits 1-2: accum_mode   bit 3: an output is written
// EPI < 0: everything is read from GemmArgs at run time (decoder GEMMs, f32 outputs, per-row bias, ...).  A run-time
// switch costs more than its branches: hipcc merges the `s_waitcnt vmcnt` of the untaken paths' loads into every launch.
#define ZVX_EPI(res, am, out) ((res) | ((am) << 1) | ((out) << 3))
// ... and (round 5) the mel decoders' residual convolutions: alpha = 1, bias per channel or none, RAW 16-bit residual (res = 1) or none,
// result x out_scale, no activation, 16-bit output -- (conv2(t) [+ shortcut] [+ x]) / sqrt(2) of a StyleTTS residual block
#define ZVX_EPI_DEC(res) (16 | 8 | (res))
// ... and (round 6) "bias + activation -> 16 bit" with the OTHER 16-bit type on the output side: the ConvTranspose in front of a vocoder stage
// whose arithmetic differs from the previous one's (zvx_set_int "voc_f16_stages"): half in -> bf16 out or bf16 in -> half out
#define ZVX_EPI_FLIP (ZVX_EPI(0, 0, 1) | 32)
// H16 (compile-time modes only): the 16-bit tensors are IEEE half and the KERNEL has set MODE.FP16_OVFL (f16_saturate_mode): plain converts

template <int TM, int TN, int RES_LDS = 0, int EPI = -1, bool H16 = false>   // RES_LDS: residual source: 0 global memory, 1 padded LDS slab
__device__ __forceinline__ void epilogue_rows(const GemmArgs& a, f32x16 (&acc)[TN][TM], int b, int row_base, int col_base,
                                              int out_len, int lane, unsigned char* stage /* >= 32*(TN*32*4+16) bytes, this wave's */,
                                              const unsigned char* res_lds = nullptr /* RES_LDS 1: LDS row of output row `row_base` */,
                                              int res_pitch = 0) {
    constexpr int NW = TN * 32;                 // channels handled by this wave
    constexpr int EP = NW * 4 + 16;             // LDS row pitch in bytes
    constexpr int LPR = NW / 8;                 // lanes per row
    constexpr int RPP = 64 / LPR;               // rows per pass
    constexpr int NP = 32 / RPP;
    constexpr bool CT = EPI >= 0;
    constexpr bool DEC = CT && (EPI & 16) != 0;             // the decoders' residual form (ZVX_EPI_DEC)
    constexpr bool BURST = !(CT && !DEC && ((EPI >> 1) & 1));       // xs-reading modes hold more registers: store each row block at once
    const long ooff = (long)b * a.o_bs, roff = (long)b * a.r_bs, aoff = (long)b * a.a_bs;
    const int c8 = lane % LPR;
    const int n = col_base + c8 * 8;
    const bool nok = n < a.N;
    // mode words: compile-time constants or wave-uniform run-time values, read once
    const float alpha = CT ? 1.f : a.alpha, oscale = a.out_scale, rinv = a.res_inv_slope;
    const int act = DEC ? ACT_NONE : (CT ? ACT_LRELU : a.act);
    const float slope = CT ? (a.act == ACT_LRELU ? a.slope : 1.f) : a.slope;        // CT: slope 1 = no activation
    const int res_mode = RES_LDS ? 2 : (DEC ? (EPI & 1) : (CT ? ((EPI & 1) ? 2 : 0) : a.res_mode));
    const int accum_mode = DEC ? 0 : (CT ? (EPI >> 1) & 3 : a.accum_mode), bias_mode = (CT && !DEC) ? 1 : a.bias_mode;
    const bool has_out = CT ? (EPI >> 3) & 1 : a.out != nullptr, out_bf16 = CT || a.out_dtype != DT_F32, has_post = !CT && a.post_scale != nullptr;
    // (run-time epilogue: a half running sum on every shape but the 256 x 128 / 128 x 256 tiles -- those sit exactly at 256 registers,
    // even the comparison `accum_dtype != DT_F32` instead of `== DT_BF16` made them spill 24; launch_convslab refuses the combination,
    // which no shape of the path asks for)
    const bool out_f16 = CT ? H16 : a.out_dtype == DT_F16, res_f16 = (CT || RES_LDS) ? H16 : a.res_dtype == DT_F16, acc_f16 = CT ? H16 : ((TN == 1 || TM <= 2) && a.accum_dtype == DT_F16);
    const bool acc_bf16 = CT || a.accum_dtype == DT_BF16 || acc_f16, res_bf16 = CT || RES_LDS || a.res_dtype != DT_F32;     // ("bf16" here reads "16-bit")
    // 16-bit packing of a result pair: in the compile-time half modes the kernel runs with saturating converts (no clamp instructions)
#define pk2(lo, hi, f16) ((CT && H16) ? pack_f16x2_raw(lo, hi) : pack16x2(lo, hi, f16))
    f32x2 bcol[4];
#pragma unroll
    for (int e = 0; e < 4; e++) bcol[e] = (f32x2){0.f, 0.f};
    if (bias_mode == 1 && nok) {
        const float4 b0 = *(const float4*)(a.bias + n), b1 = *(const float4*)(a.bias + n + 4);
        bcol[0] = (f32x2){b0.x, b0.y}; bcol[1] = (f32x2){b0.z, b0.w}; bcol[2] = (f32x2){b1.x, b1.y}; bcol[3] = (f32x2){b1.z, b1.w};
    }
    u32x4 pk[TM][NP];                            // bf16 results, stored in one burst at the end
    // bf16 residual rows from global memory are requested one 32-row block ahead (their latency hides behind the
    // previous block's LDS transpose + arithmetic)
    const bool res_glb = !RES_LDS && res_mode && res_bf16;
    uint4 rnext[NP];
    auto res_prefetch = [&](int j) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int r = row_base + j * 32 + p * RPP + lane / LPR;
            const bool okp = r < a.M && r < out_len && nok;
            rnext[p] = *(const uint4*)((const unsigned short*)a.res + (okp ? roff + (long)r * a.ldr + n : 0));
        }
    };
    if (res_glb) res_prefetch(0);
#pragma unroll
    for (int j = 0; j < TM; j++) {
        // write this wave's 32 x NW block (MFMA layout: lane = time row, 4 consecutive channels per quad)
#pragma unroll
        for (int i = 0; i < TN; i++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *(float4*)(stage + (lane & 31) * EP + (i * 32 + 8 * g + 4 * (lane >> 5)) * 4) =
                    make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        // phase A: every load of the 32-row block in flight at once (branch-free: invalid lanes read element 0)
        f32x2 v[NP][4];
        uint4 rraw[NP];
        float4 aa0[NP], aa1[NP];
        uint4 aab[NP];
        bool ok[NP];
        if (res_glb) {
#pragma unroll
            for (int p = 0; p < NP; p++) rraw[p] = rnext[p];
            if (j + 1 < TM) res_prefetch(j + 1);
        }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int rl = p * RPP + lane / LPR;
            const int r = row_base + j * 32 + rl;
            ok[p] = r < a.M && r < out_len && nok;
            const float4 v0 = *(const float4*)(stage + rl * EP + c8 * 32), v1 = *(const float4*)(stage + rl * EP + c8 * 32 + 16);
            v[p][0] = (f32x2){v0.x, v0.y}; v[p][1] = (f32x2){v0.z, v0.w}; v[p][2] = (f32x2){v1.x, v1.y}; v[p][3] = (f32x2){v1.z, v1.w};
            if (RES_LDS == 1) rraw[p] = *(const uint4*)(res_lds + (j * 32 + rl) * res_pitch + (col_base + c8 * 8) * 2);
            if (accum_mode & 1) {
                const long ai = ok[p] ? aoff + (long)r * a.lda + n : 0;
                if (acc_bf16) aab[p] = *(const uint4*)((const unsigned short*)a.accum + ai);
                else { const float* ap = (const float*)a.accum + ai; aa0[p] = *(const float4*)ap; aa1[p] = *(const float4*)(ap + 4); }
            }
        }
        // phase B: arithmetic on float pairs (uniform branches outside the element loops)
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int r = row_base + j * 32 + p * RPP + lane / LPR;
            f32x2* t = v[p];
            if (alpha != 1.f) {
#pragma unroll
                for (int e = 0; e < 4; e++) t[e] *= alpha;
            }
            if (bias_mode == 1) {
#pragma unroll
                for (int e = 0; e < 4; e++) t[e] += bcol[e];
            } else if (bias_mode == 2) {
                const float brow = ok[p] ? a.bias[r] : 0.f;
#pragma unroll
                for (int e = 0; e < 4; e++) t[e] += brow;
            }
            if (res_mode) {
                f32x2 q[4];
                if (res_bf16) {
                    q[0] = unpack16x2(rraw[p].x, res_f16); q[1] = unpack16x2(rraw[p].y, res_f16); q[2] = unpack16x2(rraw[p].z, res_f16); q[3] = unpack16x2(rraw[p].w, res_f16);
                } else {
                    const float* rp = (const float*)a.res + (ok[p] ? roff + (long)r * a.ldr + n : 0);
                    const float4 t0 = *(const float4*)rp, t1 = *(const float4*)(rp + 4);
                    q[0] = (f32x2){t0.x, t0.y}; q[1] = (f32x2){t0.z, t0.w}; q[2] = (f32x2){t1.x, t1.y}; q[3] = (f32x2){t1.z, t1.w};
                }
                if (res_mode == 2) {            // inverse leaky-relu (1/slope > 1): x = min(y, y/slope)
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] += inv_lrelu2(q[e], rinv);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] += q[e];
                }
            }
            if (accum_mode & 1) {
                if (acc_bf16) {
                    t[0] += unpack16x2(aab[p].x, acc_f16); t[1] += unpack16x2(aab[p].y, acc_f16); t[2] += unpack16x2(aab[p].z, acc_f16); t[3] += unpack16x2(aab[p].w, acc_f16);
                } else {
                    t[0] += (f32x2){aa0[p].x, aa0[p].y}; t[1] += (f32x2){aa0[p].z, aa0[p].w};
                    t[2] += (f32x2){aa1[p].x, aa1[p].y}; t[3] += (f32x2){aa1[p].z, aa1[p].w};
                }
            }
            if ((accum_mode & 2) && ok[p]) {
                const long ai = aoff + (long)r * a.lda + n;
                if (acc_bf16) {
                    *(u32x4*)((unsigned short*)a.accum + ai) =
                        (u32x4){pk2(t[0].x, t[0].y, acc_f16), pk2(t[1].x, t[1].y, acc_f16), pk2(t[2].x, t[2].y, acc_f16), pk2(t[3].x, t[3].y, acc_f16)};
                } else {
                    float* ap = (float*)a.accum + ai;
                    *(float4*)ap = make_float4(t[0].x, t[0].y, t[1].x, t[1].y);
                    *(float4*)(ap + 4) = make_float4(t[2].x, t[2].y, t[3].x, t[3].y);
                }
            }
            if (has_out) {
                if (DEC || (CT ? accum_mode != 0 : oscale != 1.f)) {      // compile-time modes: only the xs-closing launch (and the decoders' form) scales
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] *= oscale;
                }
                if (act == ACT_LRELU) {          // 0 <= slope <= 1: leaky-relu = max(x, slope*x)
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] = lrelu2(t[e], slope);
                } else if (act == ACT_RELU) {
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] = (f32x2){fmaxf(t[e].x, 0.f), fmaxf(t[e].y, 0.f)};
                }
                if (has_post && nok) {
                    const float4 s0 = *(const float4*)(a.post_scale + n), s1 = *(const float4*)(a.post_scale + n + 4);
                    const float4 h0 = *(const float4*)(a.post_shift + n), h1 = *(const float4*)(a.post_shift + n + 4);
                    t[0] = t[0] * (f32x2){s0.x, s0.y} + (f32x2){h0.x, h0.y}; t[1] = t[1] * (f32x2){s0.z, s0.w} + (f32x2){h0.z, h0.w};
                    t[2] = t[2] * (f32x2){s1.x, s1.y} + (f32x2){h1.x, h1.y}; t[3] = t[3] * (f32x2){s1.z, s1.w} + (f32x2){h1.z, h1.w};
                }
                if (out_bf16) {
                    const u32x4 o = (u32x4){pk2(t[0].x, t[0].y, out_f16), pk2(t[1].x, t[1].y, out_f16), pk2(t[2].x, t[2].y, out_f16), pk2(t[3].x, t[3].y, out_f16)};
                    if (BURST) pk[j][p] = o;
                    else if (ok[p]) *(u32x4*)((unsigned short*)a.out + ooff + (long)r * a.ldo + n) = o;
                } else if (ok[p]) {
                    if (!CT && a.out_split3) {
                        // 16-bit split planes [hi | hi | lo] of the f32 result (ops.hip: split2 / split2h), the operand layout of the next 3-plane GEMM
                        unsigned short* op = (unsigned short*)a.out + ooff + (long)r * a.ldo + n;
                        u32x4 hv, lv;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if (a.out_split3 == 2) {                               // IEEE-half planes: lo scaled by 2^11 (ops.hip: split2h)
                                const unsigned hp = pack_f16x2(t[e].x, t[e].y);
                                const f32x2 rem = (t[e] - unpack_f16x2(hp)) * 2048.f;
                                hv[e] = hp; lv[e] = pack_f16x2(rem.x, rem.y);
                            } else {
                                const unsigned hp = pack_bf16x2(t[e].x, t[e].y);
                                const f32x2 rem = t[e] - unpack_bf16x2(hp);
                                hv[e] = hp; lv[e] = pack_bf16x2(rem.x, rem.y);
                            }
                        }
                        *(u32x4*)op = hv; *(u32x4*)(op + a.N) = hv; *(u32x4*)(op + 2 * a.N) = lv;
                    } else {
                        float* op = (float*)a.out + ooff + (long)r * a.ldo + n;
                        *(float4*)op = make_float4(t[0].x, t[0].y, t[1].x, t[1].y);
                        *(float4*)(op + 4) = make_float4(t[2].x, t[2].y, t[3].x, t[3].y);
                    }
                }
            }
        }
    }
    if (has_out && out_bf16 && BURST) {
        unsigned short* obase = (unsigned short*)a.out + ooff + n;
        const int ldo = a.ldo;
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const int r = row_base + j * 32 + p * RPP + lane / LPR;
                if (r < a.M && r < out_len && nok) *(u32x4*)(obase + (long)r * ldo) = pk[j][p];
            }
    }
#undef pk2
}

// Epilogue for "bias + activation -> bf16" with nothing to read (EPI = ZVX_EPI(0, 0, 1): conv1 of a ResBlock pair,
// polyphase ConvTranspose): the arithmetic runs in the MFMA layout, only the bf16 results cross the LDS stage (half
// the bytes of the f32 transpose) and come back as whole channel rows for 16-byte stores.
template <int TM, int TN, bool F16 = false>
__device__ __forceinline__ void epilogue_direct(const GemmArgs& a, f32x16 (&acc)[TN][TM], int b, int row_base, int col_base,
                                                int out_len, int lane, unsigned char* stage /* >= 32*(TN*64+16) bytes, this wave's */) {
    constexpr int NW = TN * 32, EP = NW * 2 + 16, LPR = NW / 8, RPP = 64 / LPR, NP = 32 / RPP;
    const float slope = a.act == ACT_LRELU ? a.slope : 1.f;
    const int h4 = 4 * (lane >> 5), c8 = lane % LPR, n = col_base + c8 * 8;
    const bool nok = n < a.N;
    float4 bb[TN][4];
#pragma unroll
    for (int i = 0; i < TN; i++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int co = col_base + i * 32 + 8 * g + h4;
            bb[i][g] = co < a.N ? *(const float4*)(a.bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    unsigned short* obase = (unsigned short*)a.out + (long)b * a.o_bs + n;
    u32x4 o[TM][NP];
#pragma unroll
    for (int j = 0; j < TM; j++) {
#pragma unroll
        for (int i = 0; i < TN; i++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x2 v01 = lrelu2((f32x2){acc[i][j][4 * g], acc[i][j][4 * g + 1]} + (f32x2){bb[i][g].x, bb[i][g].y}, slope);
                const f32x2 v23 = lrelu2((f32x2){acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]} + (f32x2){bb[i][g].z, bb[i][g].w}, slope);
                uint2 pk;
                pk.x = pack16x2(v01.x, v01.y, F16);
                pk.y = pack16x2(v23.x, v23.y, F16);
                *(uint2*)(stage + (lane & 31) * EP + (i * 32 + 8 * g + h4) * 2) = pk;
            }
#pragma unroll
        for (int p = 0; p < NP; p++) o[j][p] = *(const u32x4*)(stage + (p * RPP + lane / LPR) * EP + c8 * 16);
    }
#pragma unroll
    for (int j = 0; j < TM; j++)
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int r = row_base + j * 32 + p * RPP + lane / LPR;
            if (r < a.M && r < out_len && nok) *(u32x4*)(obase + (long)r * a.ldo) = o[j][p];
        }
}

#if ZVX_PART_MAIN
// ================================================================================================
// conv-slab kernel: bf16 1-D convolutions / linears against STATIC weights.
//
// Each workgroup owns BM time rows x BN channels.  Per 64-channel K-chunk the input slab
// (BM + halo rows) x 64 ch is staged ONCE into LDS and re-used by every tap (a tap is just a row offset
// into the slab), instead of being re-staged per tap.  Weights are pre-packed at load time into MFMA-fragment
// order ([channel tile][K-chunk][tap][k16][lane][8 bf16], 1 KiB per fragment).  Two ways of streaming them
// (template parameter R): R == 0 -- every wave fetches the fragments of its own channel tiles with coalesced
// 16-byte global loads straight into a 4-step ring of srcA registers (256x128 tiles: no barrier inside a K-chunk);
// R > 0 -- one LDS ring per workgroup filled by LDS-DMA, R-1 steps ahead, one barrier per step (other tile shapes).
// Two workgroups per CU overlap one block's refill / epilogue with the other's MFMAs.
// ================================================================================================
#define SLAB_KC 64
#define SLAB_PITCH 144      // 128 B of channels + 16 B pad: 16 consecutive rows hit 16 distinct 16-B slots

__global__ void k_pack_w(const unsigned short* w, int ntaps, int N, int K, unsigned short* out, int nkc, long total_frag_lanes) {
    // out index: ((((nt * nkc + kc) * ntaps + tap) * 4 + k16) * 64 + lane) * 8 + e
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total_frag_lanes) return;
    const int lane = idx & 63; long t = idx >> 6;
    const int k16 = t & 3; t >>= 2;
    const int tap = t % ntaps; t /= ntaps;
    const int kc = t % nkc; const int nt = t / nkc;
    const int n = nt * 32 + (lane & 31);
    const int k0 = kc * SLAB_KC + k16 * 16 + 8 * (lane >> 5);
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int k = k0 + e;
        v[e] = (n < N && k < K) ? w[((long)tap * N + n) * K + k] : (unsigned short)0;
    }
    uint4 o;
    o.x = v[0] | ((unsigned)v[1] << 16); o.y = v[2] | ((unsigned)v[3] << 16);
    o.z = v[4] | ((unsigned)v[5] << 16); o.w = v[6] | ((unsigned)v[7] << 16);
    *(uint4*)(out + idx * 8) = o;
}

size_t packed_weight_elems(int ntaps, int N, int K) {
    const int nkc = (K + SLAB_KC - 1) / SLAB_KC, nt = (N + 31) / 32;
    return (size_t)nt * nkc * ntaps * 4 * 64 * 8;
}
void launch_pack_weights(const void* w_bf16, int ntaps, int N, int K, void* out, hipStream_t s) {
    const int nkc = (K + SLAB_KC - 1) / SLAB_KC, nt = (N + 31) / 32;
    const long total = (long)nt * nkc * ntaps * 4 * 64;
    hipLaunchKernelGGL(k_pack_w, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const unsigned short*)w_bf16, ntaps, N, K,
                       (unsigned short*)out, nkc, total);
}

void launch_pack_pair(const void* packedA, int ntapsA, int KA, const void* packedB, int ntapsB, int KB, int N, void* out, hipStream_t s) {
    const size_t nt = (N + 31) / 32;
    const size_t szA = (size_t)((KA + SLAB_KC - 1) / SLAB_KC) * ntapsA * 4 * 1024, szB = (size_t)((KB + SLAB_KC - 1) / SLAB_KC) * ntapsB * 4 * 1024;
    (void)hipMemcpy2DAsync(out, szA + szB, packedA, szA, szA, nt, hipMemcpyDeviceToDevice, s);
    (void)hipMemcpy2DAsync((char*)out + szA, szA + szB, packedB, szB, szB, nt, hipMemcpyDeviceToDevice, s);
}

// F16: the operands are IEEE half (v_mfma_f32_32x32x16_f16, same rate), the StyleTTS decoder's launches; everything else is bf16
template <int BM, int BN, int WM, int WN, bool FULLK, int MINW, int R, int EPI = -1, int MAXH = 64, bool F16 = false>
__global__ __launch_bounds__(256, MINW) void convslab_kernel(const GemmArgs a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NIT = ((BM + MAXH) * 8 + 255) / 256;    // staging iterations (halo_l + halo_r <= MAXH rows)
    static_assert(WM * WN == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab[];
    if (F16 && EPI >= 0 && EPI != ZVX_EPI(0, 0, 1) && EPI != ZVX_EPI_FLIP) f16_saturate_mode();   // compile-time half epilogues convert without clamps (mfma_util.h)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: SGPR arithmetic, scalar branches
    const int wr = wave % WM, wc = wave / WM;
    const int ntn = (a.N + BN - 1) / BN;
    int wg, b;
    if (a.xcd_flat) {
        // workgroups reach the XCDs round-robin in LINEAR order (x fastest, then y): remap over the whole grid, so that each XCD walks a
        // contiguous range of (utterance, time tile, channel tile) whatever gridDim.x is modulo 8
        const int nx = gridDim.x, nwg = nx * gridDim.y, id = blockIdx.y * nx + blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
        b = w / nx; wg = w - b * nx;
    } else {
        const int nwg = gridDim.x, id = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
        b = blockIdx.y;
    }
    const int nt = wg % ntn, mt = wg / ntn;
    const int m0 = mt * BM, n0 = nt * BN;
    const bool bflat = a.bflat != 0;                      // batch-flattened launch: b == 0, a.M = all rows, lengths looked up per row
    const int out_len = bflat ? a.M : (a.out_len ? a.out_len[b] : a.M);
    const int in_len = bflat ? 0 : (a.in_len ? a.in_len[b] : a.in_len_static);
    if (m0 >= out_len || m0 >= a.M) return;
    if (bflat) {                                          // a tile that lies wholly in one utterance's padding rows: nothing to write
        const int b0 = m0 / a.bflat, t0 = m0 - b0 * a.bflat;
        if (t0 >= a.out_len[b0] && t0 + BM <= a.bflat) return;
    }

    const int HL = a.halo_l, SR = BM + a.halo_l + a.halo_r;
    const int nkc = (a.K + SLAB_KC - 1) / SLAB_KC, n16 = a.K >> 4, ntaps = a.ntaps;
    const unsigned short* Xp = (const unsigned short*)a.X + (long)b * a.x_bs;
    // second source (GemmArgs::X2; !FULLK variants): nkc2 more chunks of ONE tap (row offset 0) behind the nkc chunks of X
    const int nkc2 = (!FULLK && a.K2 > 0) ? (a.K2 + SLAB_KC - 1) / SLAB_KC : 0, n16_2 = a.K2 >> 4;
    const unsigned short* Xp2 = (const unsigned short*)a.X2 + (long)b * a.x2_bs;
    // flattened 2-D maps (MAXH > 64 instantiations): in_len is the utterance's valid WIDTH; which of this thread's slab rows are
    // valid positions of the map is the same for every K-chunk -> one bit per staging iteration.  Batch-flattened 1-D launches
    // use the same bit: row g is position g % bflat of utterance g / bflat, valid below THAT utterance's length.
    const int in_rows = ((MAXH > 64 || bflat) && a.flat_win) ? a.flat_rows : in_len;
    unsigned rowmask = 0xffffffffu;
    if (bflat) {
        rowmask = 0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int g = m0 - HL + ((tid + it * 256) >> 3);
            if (g >= 0 && g < in_rows) { const int bb = g / a.bflat; if (g - bb * a.bflat < a.in_len[bb]) rowmask |= 1u << it; }
        }
    } else if (MAXH > 64 && a.flat_win) {
        rowmask = 0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int g = m0 - HL + ((tid + it * 256) >> 3);
            if (g >= 0 && g < in_rows && (g % a.flat_win) < in_len) rowmask |= 1u << it;
        }
    }

    f32x16 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; i++)
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

    // ---- weights: ONE ring per workgroup, filled by LDS-DMA (global_load_lds, 1 KiB fragment per instruction) ----
    // The packed stream of a 32-channel tile is contiguous over (K-chunk, tap, k16): global step gs lives at
    // tile base + gs KiB.  Ring slot gs % R holds the F fragments (all channel tiles of the workgroup) of step gs;
    // wave w requests fragments [w*CNT, w*CNT+CNT) of every step, D = R-1 steps ahead of the MFMAs, so each
    // fragment is fetched once per workgroup.  Per step: this wave's counted vmcnt (its pieces of step s+1 have
    // landed) + s_barrier (so have everyone else's; and every wave is done reading slot s-1, which the next
    // request overwrites).  No VGPR staging, no fence: DMAs stay in flight across the barrier.
    // R == 0 selects the register variant: every wave streams the fragments of ITS OWN channel tiles straight into a
    // 4-step register ring with plain (saddr-form) global loads -- an LDS-DMA instruction costs the issuing wave 100-300
    // cycles, a global_load a few, and with no shared ring there is no per-step barrier.  The two waves that share a
    // channel tile fetch the same lines within a few hundred cycles of each other (L1 hits).
    constexpr bool WREG = R == 0;
    constexpr int F = BN / 32, CNT = F >= 4 ? F / 4 : 1, WD = 4, D = WREG ? WD : R - 1, WAITN = WREG ? (WD - 1) * TN : (D - 2) * CNT;
    const int nt32_total = (a.N + 31) >> 5;
    const int nsteps = a.ntaps * 4, gtotal = nkc * nsteps + nkc2 * 4;
    const uint4* wsrc[CNT];
#pragma unroll
    for (int j = 0; j < CNT; j++) {
        const int f = wave * CNT + j, t32 = (n0 >> 5) + f;
        wsrc[j] = (const uint4*)a.Wp + (long)(t32 < nt32_total ? t32 : 0) * gtotal * 64 + lane;
    }
    const int xrow0 = HL + wr * (BM / WM) + (lane & 31);
    const int koff = (lane >> 5) * 16;
    unsigned char* ring = slab + ((SR * SLAB_PITCH + 1023) & ~1023);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)slab;   // LDS byte address of the window
    const int dvreg = a.dv[lane & (ZVX_MAX_TAPS - 1)];              // lane t holds tap t's row offset (read back with v_readlane)
    const bool loader = wave * CNT < F;
    const unsigned char* wq[TN];                                    // register variant: this wave's channel tiles (wave-uniform)
#pragma unroll
    for (int i = 0; i < TN; i++) {
        const int t32 = (n0 >> 5) + wc * TN + i;
        wq[i] = (const unsigned char*)a.Wp + (long)(t32 < nt32_total ? t32 : 0) * gtotal * 1024;
    }
    // A wave whose channels all lie past N (N = 528 is 4.125 tiles of 128: two of the last tile's four waves) multiplies nothing:
    // its k16 count is zero (!FULLK variants -- every N that is not a multiple of the tile width comes with such a K here).  The
    // chip is power-limited: MFMAs on zeros are time.
    const bool wave_dead = __builtin_amdgcn_readfirstlane((int)(n0 + wc * TN * 32 >= a.N)) != 0;
    const unsigned lane16 = lane * 16;
    u32x4 wreg[WREG ? WD : 1][TN] = {};                              // 4-step ring: slot = k16 index within the tap
    auto wload = [&](int gs, int slot) {                            // slot is a literal at every call site
        const long off = (long)(gs < gtotal ? gs : gtotal - 1) * 1024;  // past the end: harmless re-loads keep vmcnt counting uniform
#pragma unroll
        for (int i = 0; i < TN; i++)
            asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(wreg[WREG ? slot : 0][i]) : "v"(lane16), "s"(wq[i] + off) : "memory");   // "+v": the ring slot keeps ONE physical register across the tap loop
    };
    auto dma = [&](int gs) {
        if (WREG || !loader) return;
        const int slot = gs & (R - 1);
        const long off = (long)(gs < gtotal ? gs : gtotal - 1) * 64;      // past the end: harmless re-loads keep vmcnt counting uniform
#pragma unroll
        for (int j = 0; j < CNT; j++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[j] + off),
                                             (__attribute__((address_space(3))) void*)(ring + (slot * F + wave * CNT + j) * 1024), 16, 0, 0);
    };
    // the first D steps are requested BEFORE the slab fill so that their L2 latency overlaps the fill's
    if (WREG) { wload(0, 0); wload(1, 1); wload(2, 2); wload(3, 3); }
    else {
#pragma unroll
        for (int s0 = 0; s0 < D; s0++) dma(s0);
    }

    for (int kc = 0; kc < nkc + nkc2; kc++) {
        const bool src2 = !FULLK && kc >= nkc;                       // wave-uniform
        const unsigned short* const Xs = src2 ? Xp2 : Xp;
        const int ldxs = src2 ? a.ldx2 : a.ldx, Ks = src2 ? a.K2 : a.K, kbase = (src2 ? kc - nkc : kc) * SLAB_KC;
        // ---- stage the slab: rows [m0-HL, m0+BM+HR) x 64 channels of chunk kc (FCH iterations of loads in flight, then their stores) ----
        {
            constexpr int FCH = NIT > 10 ? (NIT + 1) / 2 : NIT;      // wide-halo instantiations: two rounds (register budget)
#pragma unroll
            for (int h0 = 0; h0 < NIT; h0 += FCH) {
                uint4 sv[FCH];
#pragma unroll
                for (int i = 0; i < FCH; i++) {
                    const int it = h0 + i;
                    const int c = tid + it * 256;
                    const int row = c >> 3, q = c & 7;
                    const int g = m0 - HL + row, k = kbase + q * 8;
                    sv[i] = make_uint4(0, 0, 0, 0);
                    if (it < NIT && c < SR * 8 && g >= 0 && g < in_rows && k < Ks && ((rowmask >> it) & 1)) sv[i] = *(const uint4*)(Xs + (long)g * ldxs + k);
                }
                if (kc && h0 == 0) __syncthreads();   // (after the refill loads are in flight) every wave is done with chunk kc-1's slab
#pragma unroll
                for (int i = 0; i < FCH; i++) {
                    const int c = tid + (h0 + i) * 256;
                    if (h0 + i < NIT && c < SR * 8) *(uint4*)(slab + (c >> 3) * SLAB_PITCH + (c & 7) * 16) = sv[i];
                }
            }
        }
        __syncthreads();                          // (drains this wave's DMAs too: the chunk's first D steps are in the ring)
        int nk16 = 4;
        if (!FULLK) { nk16 = src2 ? n16_2 - (kc - nkc) * 4 : n16 - kc * 4; if (nk16 > 4) nk16 = 4; if (wave_dead) nk16 = 0; }
        const int ntaps_kc = src2 ? 1 : ntaps;

        // LDS reads of the main loop are inline asm: hipcc would otherwise drain every pending LDS-DMA (vmcnt(0))
        // in front of each ds_read.  Fragments of step s+1 are read while the MFMAs of step s run (sets A/B).
        uint4 xA[TM], wA[TN], xB[TM], wB[TN];
        const unsigned ring_rd = lds_base + (unsigned)(size_t)(ring - slab) + lane * 16 + wc * TN * 1024;
        const int gs0 = src2 ? nkc * nsteps + (kc - nkc) * 4 : kc * nsteps;
        auto rd = [&](uint4 (&xf)[TM], uint4 (&wf)[TN], int gs, unsigned rowoff, int kk) {
            if (!WREG) {
                const unsigned wa = ring_rd + (gs & ((WREG ? 1 : R) - 1)) * (F * 1024);
#pragma unroll
                for (int i = 0; i < TN; i++)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[i]) : "v"(wa), "n"(i * 1024));
            }
#pragma unroll
            for (int j = 0; j < TM; j++)
                asm volatile("ds_read_b128 %0, %1" : "=v"(xf[j]) : "v"(lds_base + rowoff + j * 32 * SLAB_PITCH + kk * 32));
        };
        auto mma = [&](uint4 (&xf)[TM], uint4 (&wf)[TN]) {
#pragma unroll
            for (int i = 0; i < TN; i++)
#pragma unroll
                for (int j = 0; j < TM; j++)
                    acc[i][j] = F16 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[i]), __builtin_bit_cast(f16x8, xf[j]), acc[i][j], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[i]),
                                                                       __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
        };
        auto mma_r = [&](uint4 (&xf)[TM], int slot) {
#pragma unroll
            for (int i = 0; i < TN; i++)
#pragma unroll
                for (int j = 0; j < TM; j++)
                    acc[i][j] = F16 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wreg[WREG ? slot : 0][i]), __builtin_bit_cast(f16x8, xf[j]), acc[i][j], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wreg[WREG ? slot : 0][i]),
                                                                       __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
        };
        auto rowoff_of = [&](int tap) {
            const int d = src2 ? 0 : __builtin_amdgcn_readlane(dvreg, tap < ntaps ? tap : ntaps - 1);
            return (unsigned)((xrow0 + d) * SLAB_PITCH + koff);
        };
        unsigned rowoff = rowoff_of(0);
        rd(xA, wA, gs0, rowoff, 0);
        for (int tap = 0; tap < ntaps_kc; tap++) {
            const unsigned rowoff_next = rowoff_of(tap + 1);
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const int gs = gs0 + tap * 4 + kk;
                // ring variant: this wave's pieces of step gs+1 have landed (only its requests for steps gs+2 .. gs+D-1 may stay
                // in flight) + barrier; register variant: this step's own fragments, requested 4 steps ago
                if (WREG) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(WAITN) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(WAITN) : "memory");
                dma(gs + D);
                if (kk & 1) rd(xA, wA, gs + 1, kk == 3 ? rowoff_next : rowoff, (kk + 1) & 3);
                else        rd(xB, wB, gs + 1, rowoff, kk + 1);
                // wait for THIS step's set only: the reads just issued may remain outstanding
                asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(WREG ? TM : TM + TN) : "memory");
                __builtin_amdgcn_sched_barrier(0);
                if (FULLK || kk < nk16) {
                    if (WREG) { if (kk & 1) mma_r(xB, kk); else mma_r(xA, kk); }
                    else { if (kk & 1) mma(xB, wB); else mma(xA, wA); }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (WREG) wload(gs + WD, kk);                     // the slot just consumed takes the fragments of step gs + 4
            }
            rowoff = rowoff_next;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the speculative reads of the chunk's last step
    }
    if (WREG) {
        // The ring registers stay allocated THROUGH this wait (tied operands): the last requests are still landing in them,
        // and hipcc would otherwise hand the (to it: dead) registers to the epilogue's address arithmetic first.
#pragma unroll
        for (int sl = 0; sl < (WREG ? WD : 1); sl++)
#pragma unroll
            for (int i = 0; i < TN; i++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(wreg[sl][i]) :: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // tail DMAs
    }
    __syncthreads();                             // every wave is done with the slab: its LDS becomes the transpose stage
    if (EPI == ZVX_EPI_FLIP)
        epilogue_direct<TM, TN, !F16>(a, acc, b, m0 + wr * (BM / WM), n0 + wc * (BN / WN), out_len, lane, slab + wave * (32 * (TN * 64 + 16)));
    else if (EPI == ZVX_EPI(0, 0, 1))
        epilogue_direct<TM, TN, F16>(a, acc, b, m0 + wr * (BM / WM), n0 + wc * (BN / WN), out_len, lane, slab + wave * (32 * (TN * 64 + 16)));
    else
        epilogue_rows<TM, TN, 0, EPI, (F16 && EPI >= 0)>(a, acc, b, m0 + wr * (BM / WM), n0 + wc * (BN / WN), out_len, lane, slab + wave * (32 * (TN * 32 * 4 + 16)));
}

// ================================================================================================
// conv-reg kernel: square bf16 convolutions with few channels (C = 32 / 64: HiFi-GAN stages 3-4).
// These layers are HBM-bound and their whole weight set is small, so each wave keeps the weight fragments
// of its 32 output channels for ALL taps in registers (NT*C/16 fragments, loaded once, coalesced, from the
// packed stream) and the main loop is nothing but ds_read_b128 of the LDS slab + MFMA: no weight traffic,
// no waits on global memory, no barrier between the slab fill and the epilogue.
// ================================================================================================
template <int C, int NT, int BM, int WM, int WN, int MINW, int MAXH = 64, bool F16 = false>
__global__ __launch_bounds__(256, MINW) void convreg_kernel(const GemmArgs a) {
    constexpr int TM = BM / WM / 32;
    constexpr int KS = C / 16;                           // k16 steps per tap
    constexpr int PITCH_ = C * 2 + 16;                   // LDS row pitch (80 B / 144 B: conflict-free b128 reads)
    constexpr int CPR = C / 8;                           // 16-byte chunks per row
    constexpr int NIT = ((BM + MAXH) * CPR + 255) / 256;
    constexpr int FCH = NIT > 12 ? 8 : NIT;              // staging iterations in flight at a time (register budget next to the weights)
    static_assert(WM * WN == 4 && WN * 32 == C, "wave layout");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave % WM, wc = wave / WM;
    int wg;
    {
        const int nwg = gridDim.x, id = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    const int m0 = wg * BM, b = blockIdx.y;
    const int out_len = a.out_len ? a.out_len[b] : a.M;
    const int in_len = a.in_len ? a.in_len[b] : a.in_len_static;
    if (m0 >= out_len || m0 >= a.M) return;
    const int HL = a.halo_l, SR = BM + a.halo_l + a.halo_r;
    const unsigned short* Xp = (const unsigned short*)a.X + (long)b * a.x_bs;

    // ---- all weight fragments of this wave's 32 output channels -> registers (packed stream: [nt32][tap][4 k16 slots]) ----
    uint4 w[NT][KS];
    {
        const uint4* Wq = (const uint4*)a.Wp + ((long)wc * NT * 4) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int kk = 0; kk < KS; kk++) w[t][kk] = Wq[(t * 4 + kk) * 64];
    }
    // ---- slab: rows [m0-HL, m0+BM+HR) x C channels, FCH iterations of loads in flight, then their LDS stores ----
    // (flattened 2-D maps: in_len is the valid WIDTH; a row is a position of the map iff its column g % flat_win is inside it)
    {
        const bool flat = MAXH > 64 && a.flat_win;
        const int in_rows = flat ? a.flat_rows : in_len;
#pragma unroll
        for (int h0 = 0; h0 < NIT; h0 += FCH) {
            uint4 sv[FCH];
#pragma unroll
            for (int i = 0; i < FCH; i++) {
                const int c = tid + (h0 + i) * 256;
                const int row = c / CPR, q = c % CPR;
                const int g = m0 - HL + row;
                sv[i] = make_uint4(0, 0, 0, 0);
                if (h0 + i < NIT && c < SR * CPR && g >= 0 && g < in_rows && (!flat || (g % a.flat_win) < in_len)) sv[i] = *(const uint4*)(Xp + (long)g * a.ldx + q * 8);
            }
#pragma unroll
            for (int i = 0; i < FCH; i++) {
                const int c = tid + (h0 + i) * 256;
                if (h0 + i < NIT && c < SR * CPR) *(uint4*)(slab + (c / CPR) * PITCH_ + (c % CPR) * 16) = sv[i];
            }
        }
    }
    __syncthreads();

    f32x16 acc[1][TM];
#pragma unroll
    for (int j = 0; j < TM; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
    const int xrow0 = HL + wr * (BM / WM) + (lane & 31);
    const int koff = (lane >> 5) * 16;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const unsigned char* rowp = slab + (xrow0 + a.dv[t]) * PITCH_ + koff;
#pragma unroll
        for (int kk = 0; kk < KS; kk++)
#pragma unroll
            for (int j = 0; j < TM; j++) {
                const uint4 xf = *(const uint4*)(rowp + j * 32 * PITCH_ + kk * 32);
                acc[0][j] = mfma16<F16>(w[t][kk], xf, acc[0][j]);
            }
    }
    __syncthreads();
    epilogue_rows<TM, 1>(a, acc, b, m0 + wr * (BM / WM), wc * 32, out_len, lane, slab + wave * (32 * (32 * 4 + 16)));
}

// Stores of a 32 x 32 result block from the MFMA layout (conv2d_persist_kernel / conv2d_s2_kernel): a lane holds 4 groups of 4 consecutive
// channels of one row, packed to 8 bytes each (pk[g]: channels 8 g + 4 (lane >> 5) ..+3); lanes l and l + 32 hold the two halves of each
// 16-byte piece.  v_permlane32_swap trades them (gfx950): the low lane ends up with both halves of groups 0 / 2, the high lane with
// both halves of groups 1 / 3 -> TWO 16-byte stores per lane and block instead of four 8-byte ones (C = 32: conv1 166 -> 154 us, conv2
// 208 -> 171 us per launch).  The 8-wave kernels store the 8-byte pieces directly: they have no registers for the trade (24-60 spilled).
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
__device__ __forceinline__ void store_block_mfma_layout(unsigned short* row_ptr /* channel 0 of this wave's 32, this lane's row */, const uint2 (&pk)[4], int lane, bool ok) {
#pragma unroll
    for (int pr = 0; pr < 2; pr++) {
        const u32x2_t sx = __builtin_amdgcn_permlane32_swap(pk[2 * pr].x, pk[2 * pr + 1].x, false, false);
        const u32x2_t sy = __builtin_amdgcn_permlane32_swap(pk[2 * pr].y, pk[2 * pr + 1].y, false, false);
        if (ok) *(u32x4*)(row_ptr + 8 * (2 * pr + (lane >> 5))) = (u32x4){sx.x, sy.x, sx.y, sy.y};
    }
}

// ================================================================================================
// conv2d-persist kernel (round 5): the 3 x 3 convolutions over flattened [H][W] maps with C = 32 / 64 channels (the speaker encoder's
// first two levels, ResNetSE34V2.py:74-76) as PERSISTENT workgroups.  convreg_kernel above spends a tile on serial latencies -- 72 KB of
// weight fragments per workgroup from L2, then the slab rows in two rounds of loads, then 0.8 us of matrix steps, then an epilogue
// through the LDS transpose -- with two workgroups per CU to hide them behind: 1.7 TB/s and 330 TFLOP/s at C = 32.  Here
//  * a workgroup keeps its weight fragments for ALL its tiles;
//  * the rows of its next tile are requested (branch-free raw buffer loads, out-of-range offset = masked) right after the current
//    tile's rows are committed to LDS: they are in flight under the matrix steps and the epilogue;
//  * results leave from the MFMA layout (store_block_mfma_layout above: two 16-byte stores per lane and 32 x 32 block after a
//    v_permlane32_swap of the packed halves).  The LDS transpose of epilogue_rows measured 12 k of 25 k cycles per 768-row tile
//    (cut-outs, tools/experiments/README.md);
//  * tiles are dealt round by round, in contiguous runs per XCD (a tile's halo rows are its neighbours' centre rows: same L2);
//  * MODE 0 (conv2, the block's second convolution) also leaves the squeeze-excite pool's partial sums (GemmArgs::se_part): one
//    [32-channel] partial per (tile, wave) in a fixed slot, folded by k_se_fc in a fixed order -- no pass over the output for the pool.
// C = 32: 4 waves, two workgroups per CU (246-250 registers).  C = 64 (144 registers of weights per wave): 8 waves of 64 rows, one
// workgroup per CU, so that the requests of a tile spread over twice the lanes; the epilogue constants live in LDS there.
// ================================================================================================
template <int C, int BM, int WM, int WN, int MAXH, int MODE, int WGPC, bool POOL = false>
__global__ __launch_bounds__(WM * WN * 64, WM * WN * WGPC / 4) void conv2d_persist_kernel(const GemmArgs a, const int ntm, const int ntiles) {
    constexpr int NTHR = WM * WN * 64;
    constexpr int NT = 9, TM = BM / WM / 32, KS = C / 16, PITCH_ = C * 2 + 16, CPR = C / 8, RSTEP = NTHR / CPR;
    constexpr int NIT = ((BM + MAXH) * CPR + NTHR - 1) / NTHR;
    constexpr bool EC_LDS = NTHR > 256;
    static_assert(WN * 32 == C && BM % (WM * 32) == 0, "wave layout");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave % WM, wc = wave / WM;
    const int G = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;      // G is a multiple of 8
    auto tile_of = [&](int r) {                                                 // this workgroup's tile of round r (or ntiles: none)
        const int base = r * G, n = ntiles - base < G ? ntiles - base : G;
        if (n <= 0) return ntiles;
        const int per = (n + 7) >> 3, t = xcd * per + slot;
        return (slot < per && t < n) ? base + t : ntiles;
    };
    const int HL = a.halo_l, SR = BM + a.halo_l + a.halo_r, win = a.flat_win, in_rows = a.flat_rows;

    uint4 w[NT][KS];
    {
        const uint4* Wq = (const uint4*)a.Wp + ((long)wc * NT * 4) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int kk = 0; kk < KS; kk++) w[t][kk] = Wq[(t * 4 + kk) * 64];
    }
    // epilogue constants of this lane's 16 channels (MFMA layout: 4 groups of 4 consecutive channels, 8 g + 4 (lane >> 5) + e):
    // MODE 0: + bias (conv2 with its folded BatchNorm); MODE 1: ReLU, then x scale + shift (conv1 -> ReLU -> BatchNorm)
    float* const ecl = (float*)(slab + ((SR * PITCH_ + 15) & ~15));            // EC_LDS: [C] bias / scale, [C] shift behind the slab
    float4 ec0[EC_LDS ? 1 : 4], ec1[(MODE == 1 && !EC_LDS) ? 4 : 1];
    if (EC_LDS) {
        if (tid < C) { ecl[tid] = MODE == 0 ? a.bias[tid] : a.post_scale[tid]; if (MODE == 1) ecl[C + tid] = a.post_shift[tid]; }
    } else {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int ch = wc * 32 + 8 * g + 4 * (lane >> 5);
            if (MODE == 0) ec0[g] = *(const float4*)(a.bias + ch);
            else { ec0[g] = *(const float4*)(a.post_scale + ch); ec1[g] = *(const float4*)(a.post_shift + ch); }
        }
    }
    u32x4 sv[NIT];
    const int row_t = tid / CPR, q8 = (tid % CPR) * 8;
    auto request = [&](int t) __attribute__((always_inline)) {
        const int b = t / ntm, m0 = (t - b * ntm) * BM;
        const int in_len = a.in_len[b];
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)((const unsigned short*)a.X + (long)b * a.x_bs), 0, in_rows * a.ldx * 2, 0x00020000);
        int g = m0 - HL + row_t;
        int col = (g + 2 * win) % win;                    // (HL = win + 1: g >= -2 win; the launcher guarantees win >= RSTEP)
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const bool ok = tid + it * NTHR < SR * CPR && g >= 0 && g < in_rows && col < in_len;
            sv[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (g * a.ldx + q8) * 2 : (int)0x80000000, 0, 0);
            g += RSTEP; col += RSTEP; if (col >= win) col -= win;
        }
    };
    int r = 0, t = tile_of(0);
    if (t < ntiles) request(t);
    const int xrow0 = HL + wr * (BM / WM) + (lane & 31);
    const int koff = (lane >> 5) * 16;
    constexpr bool pool = MODE == 0 && POOL;
    while (t < ntiles) {
        const int b = t / ntm, mt = t - b * ntm, m0 = mt * BM;
        // (barriers as bare s_barrier behind an LDS-only wait: __syncthreads() would also wait for the requests in flight)
        if (r) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is done with the previous tile's rows
        int ts = tid;
        asm volatile("" : "+v"(ts));                  // opaque: the per-iteration LDS addresses are recomputed per tile instead of living in NIT registers
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int c = ts + it * NTHR;
            if (c < SR * CPR) *(u32x4*)(slab + (c / CPR) * PITCH_ + (c % CPR) * 16) = sv[it];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const int tn = tile_of(++r);
        if (tn < ntiles) request(tn);

        f32x16 acc[1][TM];
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
#pragma unroll
        for (int tp = 0; tp < NT; tp++) {
            const unsigned char* rowp = slab + (xrow0 + a.dv[tp]) * PITCH_ + koff;
#pragma unroll
            for (int kk = 0; kk < KS; kk++)
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    const uint4 xf = *(const uint4*)(rowp + j * 32 * PITCH_ + kk * 32);
                    acc[0][j] = mfma16<false>(w[tp][kk], xf, acc[0][j]);
                }
        }
        {
            unsigned short* const ob = (unsigned short*)a.out + (long)b * a.o_bs + wc * 32 + (EC_LDS ? 4 * (lane >> 5) : 0);
            const int row0 = m0 + wr * (BM / WM) + (lane & 31);
            // squeeze-excite pool (MODE 0): this lane's sums over its valid rows (positions of the utterance's true width) of the
            // f32 results BEFORE the bias (k_se_fc adds it to the mean: every valid position carries it once)
            // (a block's sums are taken AFTER its stores: the running sums take over the registers of the first block's accumulators)
            float ps[16];
            int col = 0, wlen = 0;
            if (pool) { col = row0 % win; wlen = a.in_len[b]; }
#pragma unroll
            for (int j = 0; j < TM; j++) {
                const int row = row0 + j * 32;
                uint2 pk[4];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    float v0 = acc[0][j][4 * g], v1 = acc[0][j][4 * g + 1], v2 = acc[0][j][4 * g + 2], v3 = acc[0][j][4 * g + 3];
                    float4 e0, e1 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (EC_LDS) {
                        const int ch = wc * 32 + 8 * g + 4 * (lane >> 5);
                        e0 = *(const float4*)(ecl + ch); if (MODE == 1) e1 = *(const float4*)(ecl + C + ch);
                    } else { e0 = ec0[EC_LDS ? 0 : g]; if (MODE == 1) e1 = ec1[(MODE == 1 && !EC_LDS) ? g : 0]; }
                    if (MODE == 0) { v0 += e0.x; v1 += e0.y; v2 += e0.z; v3 += e0.w; }
                    else {
                        v0 = fmaxf(v0, 0.f) * e0.x + e1.x; v1 = fmaxf(v1, 0.f) * e0.y + e1.y;
                        v2 = fmaxf(v2, 0.f) * e0.z + e1.z; v3 = fmaxf(v3, 0.f) * e0.w + e1.w;
                    }
                    pk[g] = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                    if (EC_LDS && row < a.M) *(uint2*)(ob + (long)row * a.ldo + 8 * g) = pk[g];      // (8 waves: no registers for the trade below)
                }
                if (!EC_LDS) store_block_mfma_layout(ob + (long)row * a.ldo, pk, lane, row < a.M);
                if (pool) {
                    const bool pv = row < a.M && col < wlen;
#pragma unroll
                    for (int e = 0; e < 16; e++) ps[e] = (j ? ps[e] : 0.f) + (pv ? acc[0][j][e] : 0.f);
                    col += 32; if (col >= win) col -= win;
                }
            }
            if (pool) {
                // fold the 32 rows of each half-wave (lanes 0-31 and 32-63 hold different channels) with DPP adds: xor 1, xor 2 (quad
                // permutes), half-row mirror, row mirror -> every lane of a 16-lane row holds the row's sum; row_bcast:15 adds row 0's
                // to row 1 and row 2's to row 3.  Lanes 16 and 48 write 16 sums each.
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    float v = ps[e];
                    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));
                    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));
                    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xf, 0xf, true));
                    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xf, 0xf, true));
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));
                    ps[e] = v;
                }
                if ((lane & 31) == 16) {
                    float* pp = a.se_part + ((long)b * (ntm * WM) + mt * WM + wr) * C + wc * 32 + 4 * (lane >> 5);
#pragma unroll
                    for (int g = 0; g < 4; g++) *(float4*)(pp + 8 * g) = make_float4(ps[4 * g], ps[4 * g + 1], ps[4 * g + 2], ps[4 * g + 3]);
                }
            }
        }
        t = tn;
    }
}

template <int C, int BM, int WM, int WN, int MAXH, int WGPC>
static void launch_conv2d_persist(const GemmArgs& a, hipStream_t stream) {
    const size_t lds = (((size_t)(BM + a.halo_l + a.halo_r) * (C * 2 + 16) + 15) & ~(size_t)15) + 2 * C * sizeof(float);
    const int ntm = (a.M + BM - 1) / BM, ntiles = ntm * a.nbatch;
    int G = (WGPC * persistent_cus()) & ~7;
    if (G < 8) G = 8;
    if (ntiles < G) G = (ntiles + 7) & ~7;
    (void)lds_opt_in((const void*)conv2d_persist_kernel<C, BM, WM, WN, MAXH, 0, WGPC>);        // (per device; a refusal shows up as the launch's own error)
    (void)lds_opt_in((const void*)conv2d_persist_kernel<C, BM, WM, WN, MAXH, 1, WGPC>);
    if (a.post_scale) ZVX_LAUNCH((conv2d_persist_kernel<C, BM, WM, WN, MAXH, 1, WGPC>), dim3(G), dim3(WM * WN * 64), lds, stream, a, ntm, ntiles);
    else if (C == 32 && a.se_part && a.se_part_S) {
        // (C = 64: the fused pool cost the 8-wave kernel 12-50 spilled registers and measured slower; that instantiation is gone -- round 6)
        if constexpr (C == 32) {
            (void)lds_opt_in((const void*)conv2d_persist_kernel<C, BM, WM, WN, MAXH, 0, WGPC, true>);
            ZVX_LAUNCH((conv2d_persist_kernel<C, BM, WM, WN, MAXH, 0, WGPC, true>), dim3(G), dim3(WM * WN * 64), lds, stream, a, ntm, ntiles);
            if (!g_dry_run) *a.se_part_S = ntm * WM;                         // tells the caller that (and in how many partials) the pool was written
        }
    } else ZVX_LAUNCH((conv2d_persist_kernel<C, BM, WM, WN, MAXH, 0, WGPC>), dim3(G), dim3(WM * WN * 64), lds, stream, a, ntm, ntiles);
}

// ================================================================================================
// conv2d-s2 kernel (round 5): the level transitions of the speaker encoder (ResNetSE34V2.py:74-76, 94-95): the 3 x 3 / stride-2 / pad-1
// convolution C -> 2C of a block's conv1 (ReLU, BatchNorm) and, in the same launch (FUSE_DS), the block's 1 x 1 / stride-2 shortcut
// convolution (+ folded BatchNorm) -- it reads the centre tap's rows.  Persistent workgroups of 8 waves like conv2d_persist_kernel.
// The input map [hin][win] is staged as its four PARITY PLANES P(pr, pc)[u][v] = x[2u + pr][2v + pc], each flattened over the OUTPUT
// map's rows (pitch Wo = wout): tap (du, dv) reads plane (du != 0, dv != 0) at flat offset -(du < 0) Wo - (dv < 0).  The output map is
// one column wider than the widest utterance, so v - 1 = -1 wraps onto a column whose input position 2 (Wo - 1) + pc lies beyond every
// utterance's width: staged as zero, like every position outside the map.  Every input row is fetched once per tile (plus the one-row
// halo): the generic gathered-row GEMM ran these launches at 230 TFLOP/s and 1.2 TB/s.
// ================================================================================================
template <int C, int BM, int WM, int WN, int MAXHP, bool FUSE_DS>
__global__ __launch_bounds__(512, 2) void conv2d_s2_kernel(const GemmArgs a, const int ntm, const int ntiles) {
    constexpr int NTHR = 512, N = 2 * C;
    constexpr int TM = BM / WM / 32, KS = C / 16, PITCH_ = C * 2 + 16, CPR = C / 8, SRP = BM + MAXHP;
    constexpr int NCH = 4 * SRP * CPR, NIT = (NCH + NTHR - 1) / NTHR;
    static_assert(WM * WN == 8 && WN * 32 == N && BM % (WM * 32) == 0, "wave layout");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave % WM, wc = wave / WM;
    const int G = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;      // G is a multiple of 8
    auto tile_of = [&](int r) {
        const int base = r * G, n = ntiles - base < G ? ntiles - base : G;
        if (n <= 0) return ntiles;
        const int per = (n + 7) >> 3, t = xcd * per + slot;
        return (slot < per && t < n) ? base + t : ntiles;
    };
    const int Wo = a.wout, win = a.win, hin = a.hin, M = a.M;
    const float rWo = 1.0f / (float)Wo;

    // C = 64: 36 fragments = 144 registers next to 13 in-flight row requests and the accumulators overflowed the 256-register budget by 8
    // (round 5 shipped that spill); the LAST tap's four fragments now live in LDS (4 KiB per channel tile, read back per tile: 4 ds_reads)
    constexpr bool WLDS = C == 64;
    constexpr int NTR = WLDS ? 8 : 9;
    uint4 w[NTR][KS], wd[FUSE_DS ? KS : 1];
    unsigned char* const wl = slab + ((4 * SRP * PITCH_ + 15) & ~15) + 3 * N * sizeof(float);
    {
        const uint4* Wq = (const uint4*)a.Wp + ((long)wc * 9 * 4) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NTR; t++)
#pragma unroll
            for (int kk = 0; kk < KS; kk++) w[t][kk] = Wq[(t * 4 + kk) * 64];
        if (WLDS && wr == 0) {
#pragma unroll
            for (int kk = 0; kk < KS; kk++) *(uint4*)(wl + ((wc * KS + kk) * 64 + lane) * 16) = Wq[(8 * 4 + kk) * 64];
        }
        if (FUSE_DS) {
            const uint4* Dq = (const uint4*)a.ds_Wp + ((long)wc * 4) * 64 + lane;
#pragma unroll
            for (int kk = 0; kk < KS; kk++) wd[kk] = Dq[kk * 64];
        }
    }
    // epilogue constants in LDS behind the planes: [N] scale, [N] shift (conv1: ReLU -> x scale + shift), [N] shortcut bias
    float* const ecl = (float*)(slab + ((4 * SRP * PITCH_ + 15) & ~15));
    if (tid < N) { ecl[tid] = a.post_scale[tid]; ecl[N + tid] = a.post_shift[tid]; if (FUSE_DS) ecl[2 * N + tid] = a.ds_bias[tid]; }

    u32x4 sv[NIT];
    auto request = [&](int t) __attribute__((always_inline)) {
        const int b = t / ntm, m0 = (t - b * ntm) * BM;
        const int in_len = a.in_len[b];
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)((const unsigned short*)a.X + (long)b * a.x_bs), 0, hin * win * a.ldx * 2, 0x00020000);
        int tq = tid;
        asm volatile("" : "+v"(tq));                  // opaque: keeps the per-iteration (plane, row) arithmetic inside the call (hoisted out of the tile loop it cost 24 spilled registers)
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int c = tq + it * NTHR, q = c % CPR, rr = c / CPR, plane = rr / SRP, r = rr - plane * SRP;
            const int g = m0 - MAXHP + r;                                  // flat position of the output map
            const int gc = g < 0 ? 0 : g;
            int u = (int)(((float)gc + 0.5f) * rWo);                       // exact for g < 2^22
            const int v = gc - u * Wo;
            const int iu = 2 * u + (plane >> 1), iv = 2 * v + (plane & 1);
            const bool ok = c < NCH && g >= 0 && g < M && iu < hin && iv < in_len;
            sv[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? ((iu * win + iv) * a.ldx + q * 8) * 2 : (int)0x80000000, 0, 0);
        }
    };
    int r = 0, t = tile_of(0);
    if (t < ntiles) request(t);
    const int xrow0 = MAXHP + wr * (BM / WM) + (lane & 31);
    const int koff = (lane >> 5) * 16;
    while (t < ntiles) {
        const int b = t / ntm, mt = t - b * ntm, m0 = mt * BM;
        if (r) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is done with the previous tile's rows
        int ts = tid;
        asm volatile("" : "+v"(ts));                  // (opaque, as in request())
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int c = ts + it * NTHR;
            if (c < NCH) *(u32x4*)(slab + (c / CPR) * PITCH_ + (c % CPR) * 16) = sv[it];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const int tn = tile_of(++r);
        if (tn < ntiles) request(tn);

        f32x16 acc[TM], accd[FUSE_DS ? TM : 1];
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) { acc[j][e] = 0.f; if (FUSE_DS) accd[j][e] = 0.f; }
#pragma unroll
        for (int tp = 0; tp < 9; tp++) {
            const int du = tp / 3 - 1, dv = tp % 3 - 1;
            const int plane = (du != 0 ? 2 : 0) + (dv != 0 ? 1 : 0);
            const int off = (du < 0 ? -Wo : 0) + (dv < 0 ? -1 : 0);
            const unsigned char* rowp = slab + (plane * SRP + xrow0 + off) * PITCH_ + koff;
#pragma unroll
            for (int kk = 0; kk < KS; kk++) {
                uint4 wt;
                if (WLDS && tp == 8) wt = *(const uint4*)(wl + ((wc * KS + kk) * 64 + lane) * 16);
                else wt = w[tp < NTR ? tp : 0][kk];
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    const uint4 xf = *(const uint4*)(rowp + j * 32 * PITCH_ + kk * 32);
                    acc[j] = mfma16<false>(wt, xf, acc[j]);
                    if (FUSE_DS && tp == 4) accd[j] = mfma16<false>(wd[kk], xf, accd[j]);
                }
            }
        }
        {
            unsigned short* const ob = (unsigned short*)a.out + (long)b * a.o_bs + wc * 32 + 4 * (lane >> 5);
            unsigned short* const db = FUSE_DS ? (unsigned short*)a.ds_out + (long)b * a.o_bs + wc * 32 + 4 * (lane >> 5) : nullptr;
#pragma unroll
            for (int j = 0; j < TM; j++) {
                const int row = m0 + wr * (BM / WM) + j * 32 + (lane & 31);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int ch = wc * 32 + 8 * g + 4 * (lane >> 5);
                    const float4 e0 = *(const float4*)(ecl + ch), e1 = *(const float4*)(ecl + N + ch);
                    const float v0 = fmaxf(acc[j][4 * g], 0.f) * e0.x + e1.x, v1 = fmaxf(acc[j][4 * g + 1], 0.f) * e0.y + e1.y;
                    const float v2 = fmaxf(acc[j][4 * g + 2], 0.f) * e0.z + e1.z, v3 = fmaxf(acc[j][4 * g + 3], 0.f) * e0.w + e1.w;
                    if (row < M) *(uint2*)(ob + (long)row * a.ldo + 8 * g) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                    if (FUSE_DS) {
                        const float4 e2 = *(const float4*)(ecl + 2 * N + ch);
                        if (row < M) *(uint2*)(db + (long)row * a.ldo + 8 * g) =
                            make_uint2(pack_bf16x2(accd[j][4 * g] + e2.x, accd[j][4 * g + 1] + e2.y), pack_bf16x2(accd[j][4 * g + 2] + e2.z, accd[j][4 * g + 3] + e2.w));
                    }
                }
            }
        }
        t = tn;
    }
}

// the level-transition launch: C = 32 -> 64 with the shortcut convolution fused (GemmArgs::ds_out set), C = 64 -> 128 without (the 144
// registers of weight fragments leave no room for the shortcut's accumulators).  true if the shape is covered (and dispatched, unless
// this is a dry run)
template <int C, int BM, int WM, int WN, int MAXHP, bool FUSE_DS>
static void launch_conv2d_s2_variant(const GemmArgs& a, hipStream_t stream) {
    const size_t lds = (((size_t)4 * (BM + MAXHP) * (C * 2 + 16) + 15) & ~(size_t)15) + 3 * 2 * C * sizeof(float) + (C == 64 ? (size_t)WN * (C / 16) * 1024 : 0);
    const int ntm = (a.M + BM - 1) / BM, ntiles = ntm * a.nbatch;
    int G = persistent_cus() & ~7;
    if (G < 8) G = 8;
    if (ntiles < G) G = (ntiles + 7) & ~7;
    auto kfn = conv2d_s2_kernel<C, BM, WM, WN, MAXHP, FUSE_DS>;
    (void)lds_opt_in((const void*)kfn);
    ZVX_LAUNCH(kfn, dim3(G), dim3(512), lds, stream, a, ntm, ntiles);
}
static bool launch_conv2d_s2(const GemmArgs& a, hipStream_t stream) {
    bool ok9 = a.ntaps == 9;
    for (int t = 0; ok9 && t < 9; t++) ok9 = a.du[t] == t / 3 - 1 && a.dv[t] == t % 3 - 1;
    if (!ok9 || a.dtype != DT_BF16 || a.stride != 2 || a.N != 2 * a.K || !a.Wp || !a.in_len ||
        a.wout <= 0 || a.M != ((a.hin - 1) / 2 + 1) * a.wout || a.ldx != a.K || a.ldo % 8 || !a.out || a.out_dtype != DT_BF16 ||
        !a.post_scale || !a.post_shift || a.bias_mode != 0 || a.act != ACT_RELU || a.alpha != 1.f || a.out_scale != 1.f || a.res_mode || a.accum_mode || a.out_split3 ||
        a.nheads != 1 || a.w_bs || (long)a.hin * a.win * a.ldx * 2 >= 0x7fffffffL || (a.slab_small & 32))
        return false;
    if (a.K == 32 && a.ds_out && a.ds_Wp && a.ds_bias && a.wout + 1 <= 136) { launch_conv2d_s2_variant<32, 256, 4, 2, 136, true>(a, stream); return true; }
    if (a.K == 64 && !a.ds_out && a.wout + 1 <= 72) { launch_conv2d_s2_variant<64, 128, 2, 4, 72, false>(a, stream); return true; }
    return false;
}

template <int C, int BM, int WM, int WN, int MINW>
static bool launch_convreg_c(const GemmArgs& a, hipStream_t stream) {
    dim3 grid((a.M + BM - 1) / BM, a.nbatch);
    size_t lds = (size_t)(BM + a.halo_l + a.halo_r) * (C * 2 + 16);
    const size_t stage = (size_t)4 * 32 * (32 * 4 + 16);
    if (lds < stage) lds = stage;
    if (a.flat_win) {                                     // 3 x 3 over a flattened map: halo = flat_win + 1 rows either side (speaker encoder: bf16)
        if (a.dtype != DT_BF16) return false;
        if (a.ntaps != 9 || a.halo_l + a.halo_r > 544 || lds > 160 * 1024) return false;
        auto kfn = convreg_kernel<C, 9, BM, WM, WN, MINW, 544>;
        if (!lds_opt_in((const void*)kfn)) return false;
        ZVX_LAUNCH(kfn, grid, dim3(256), lds, stream, a);
        return true;
    }
    // (k = 5 and the 96-row halo: HiFi-GAN V3's ResBlock2 convolutions -- kernel sizes 3 / 5 / 7 with dilations (1, 2) / (2, 6) / (3, 12),
    // hifigan.py:60-81 with config_v3: its k = 7, dilation-12 taps span 72 rows and used to fall through to the gathered-row GEMM)
    if (a.halo_l + a.halo_r > 64) {
        if (a.ntaps != 7 || a.halo_l + a.halo_r > 96) return false;
        if (a.dtype == DT_F16) ZVX_LAUNCH((convreg_kernel<C, 7, BM, WM, WN, MINW, 96, true>), grid, dim3(256), lds, stream, a);
        else ZVX_LAUNCH((convreg_kernel<C, 7, BM, WM, WN, MINW, 96>), grid, dim3(256), lds, stream, a);
        return true;
    }
    if (a.dtype == DT_F16) {
        switch (a.ntaps) {
            case 3: ZVX_LAUNCH((convreg_kernel<C, 3, BM, WM, WN, MINW, 64, true>), grid, dim3(256), lds, stream, a); return true;
            case 5: ZVX_LAUNCH((convreg_kernel<C, 5, BM, WM, WN, MINW, 64, true>), grid, dim3(256), lds, stream, a); return true;
            case 7: ZVX_LAUNCH((convreg_kernel<C, 7, BM, WM, WN, MINW, 64, true>), grid, dim3(256), lds, stream, a); return true;
            case 11: ZVX_LAUNCH((convreg_kernel<C, 11, BM, WM, WN, MINW, 64, true>), grid, dim3(256), lds, stream, a); return true;
        }
        return false;
    }
    switch (a.ntaps) {
        case 3: ZVX_LAUNCH((convreg_kernel<C, 3, BM, WM, WN, MINW>), grid, dim3(256), lds, stream, a); return true;
        case 5: ZVX_LAUNCH((convreg_kernel<C, 5, BM, WM, WN, MINW>), grid, dim3(256), lds, stream, a); return true;
        case 7: ZVX_LAUNCH((convreg_kernel<C, 7, BM, WM, WN, MINW>), grid, dim3(256), lds, stream, a); return true;
        case 11: ZVX_LAUNCH((convreg_kernel<C, 11, BM, WM, WN, MINW>), grid, dim3(256), lds, stream, a); return true;
    }
    return false;
}

#endif  // ZVX_PART_MAIN
#if ZVX_PART_RESFUSE
// ================================================================================================
// rb2fuse kernel (round 6): a whole HiFi-GAN ResBlock2 (hifigan.py:77-82 with two dilations, config_v3) in ONE launch for C = 32 / 64:
//     x1 = x + conv_d1(lrelu(x));   x2 = x1 + conv_d2(lrelu(x1))
// Tensors live in the activated domain (lrelu(x) is what is stored), so lrelu(x1) -- exactly what the second convolution consumes
// and what the unfused path writes to HBM between its two launches -- stays in LDS (16-bit, same rounding), and the block's result
// leaves through the shared row-major epilogue (running sum / stage mean / next activation as the launch asks).  Rounds 1-5 ran
// every convolution as its own launch: six trips of the stage tensor per block, two now (x in, result out; + the running sum where
// it applies).  One tile per workgroup, all weight fragments of both convolutions in registers; the second convolution's dilation (up to 12 at k = 7: 36 halo rows
// either side) is what the first one over-computes: BM rows of x1 for BM - 2 h2 rows of x2.
// ================================================================================================
template <int C, int NT, int BM, int WM, int WN, int MINW, bool F16 = false>
__global__ __launch_bounds__(256, MINW) void rb2fuse_kernel(const GemmArgs a, const int H2, const int ntm, const int ntiles) {
    constexpr int TM = BM / WM / 32;
    constexpr int KS = C / 16;
    constexpr int PITCH_ = C * 2 + 16;
    constexpr int CPR = C / 8;
    constexpr int NIT = ((BM + 32) * CPR + 255) / 256;     // conv1 halo <= 16 rows either side
    static_assert(WM * WN == 4 && WN * 32 == C, "wave layout");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave % WM, wc = wave / WM;
    const int BMO = BM - 2 * H2;                           // output rows per tile
    const int H1 = a.halo_l;                               // conv1 halo = d1 (NT-1)/2 (symmetric)
    const int SR = BM + 2 * H1;
    unsigned char* t1 = slab + ((SR * PITCH_ + 15) & ~15);

    // One tile per workgroup, 3-4 workgroups per CU: a PERSISTENT form with the fragments of both convolutions resident across tiles was
    // measured and lost (C = 32: 0.41 / 0.63 / 0.82 ms against 0.33 / 0.53 / 0.64 for k = 3 / 5 / 7) -- the registers it holds across the
    // row-major epilogue halve the occupancy, and these tiles are bound by their serial phases (fill, conv, epilogue), not by the weight fetch.
    // conv1's fragments -> registers; conv2's go to a second set when both fit (NT KS <= 24), else they replace conv1's tap by tap.
    constexpr bool TWO_SETS = (NT * KS <= 24);
    uint4 w[NT][KS];
    uint4 w2[TWO_SETS ? NT : 1][TWO_SETS ? KS : 1];
    const uint4* W1q = (const uint4*)a.Wp2 + ((long)wc * NT * 4) * 64 + lane;
    const uint4* W2q = (const uint4*)a.Wp + ((long)wc * NT * 4) * 64 + lane;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            w[t][kk] = W1q[(t * 4 + kk) * 64];
            if (TWO_SETS) w2[t][kk] = W2q[(t * 4 + kk) * 64];
        }
    const int koff = (lane >> 5) * 16;
    const int wrow = wr * (BM / WM);
    int tile;
    {   // every XCD walks a contiguous range of tiles (neighbouring tiles share halo rows in its L2)
        const int nwg = gridDim.x, id = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    {
        const int b = tile / ntm, m0 = (tile - b * ntm) * BMO;
        const int out_len = a.out_len ? a.out_len[b] : a.M;
        const int in_len = a.in_len ? a.in_len[b] : a.in_len_static;
        if (tile >= ntiles || m0 >= out_len || m0 >= a.M) return;
        const unsigned short* Xp = (const unsigned short*)a.X + (long)b * a.x_bs;
        {   // slab rows s <-> global row m0 - H2 - H1 + s
            uint4 sv[NIT];
            const int tq = tid;
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int c = tq + it * 256;
                const int row = c / CPR, q = c % CPR;
                const int g = m0 - H2 - H1 + row;
                sv[it] = make_uint4(0, 0, 0, 0);
                if (c < SR * CPR && g >= 0 && g < in_len) sv[it] = *(const uint4*)(Xp + (long)g * a.ldx + q * 8);
            }
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int c = tq + it * 256;
                if (c < SR * CPR) *(uint4*)(slab + (c / CPR) * PITCH_ + (c % CPR) * 16) = sv[it];
            }
        }
        __syncthreads();

        f32x16 acc[1][TM];
        // ---- conv1 (dilation d1): x1 row i <-> global row m0 - H2 + i, reads slab rows i + H1 + dv1[t] ----
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const unsigned char* rowp = slab + (wrow + (lane & 31) + H1 + a.dv1[t]) * PITCH_ + koff;
#pragma unroll
            for (int kk = 0; kk < KS; kk++)
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    const uint4 xf = *(const uint4*)(rowp + j * 32 * PITCH_ + kk * 32);
                    acc[0][j] = mfma16<F16>(w[t][kk], xf, acc[0][j]);
                }
            if (!TWO_SETS) {
#pragma unroll
                for (int kk = 0; kk < KS; kk++) w[t][kk] = W2q[(t * 4 + kk) * 64];   // conv2's fragments take the freed registers
            }
        }
        // ---- lrelu(x1) = lrelu(acc + b1 + x) as 16 bit (x = inverse lrelu of the slab's centre rows), zero outside the sequence (the second
        //      convolution zero-pads ITS input, hifigan.py:68-75).  Same operation order as the unfused launch's epilogue: bias, residual, activation
#pragma unroll
        for (int j = 0; j < TM; j++) {
            const int i = wrow + j * 32 + (lane & 31);
            const int g = m0 - H2 + i;
            const bool inside = g >= 0 && g < in_len;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int co = wc * 32 + 8 * q + 4 * (lane >> 5);
                const float4 bb = *(const float4*)(a.bias1 + co);
                const uint2 xr = *(const uint2*)(slab + (i + H1) * PITCH_ + co * 2);
                const f32x2 r01 = inv_lrelu2(F16 ? unpack_f16x2(xr.x) : unpack_bf16x2(xr.x), a.res_inv_slope);
                const f32x2 r23 = inv_lrelu2(F16 ? unpack_f16x2(xr.y) : unpack_bf16x2(xr.y), a.res_inv_slope);
                f32x2 v01 = (f32x2){acc[0][j][4 * q] + bb.x, acc[0][j][4 * q + 1] + bb.y} + r01;
                f32x2 v23 = (f32x2){acc[0][j][4 * q + 2] + bb.z, acc[0][j][4 * q + 3] + bb.w} + r23;
                v01 = lrelu2(v01, a.slope1); v23 = lrelu2(v23, a.slope1);
                if (!inside) { v01 = (f32x2){0.f, 0.f}; v23 = (f32x2){0.f, 0.f}; }
                uint2 pk;
                if (F16) { pk.x = pack_f16x2_sat(v01.x, v01.y); pk.y = pack_f16x2_sat(v23.x, v23.y); }
                else { pk.x = pack_bf16x2(v01.x, v01.y); pk.y = pack_bf16x2(v23.x, v23.y); }
                *(uint2*)(t1 + i * PITCH_ + co * 2) = pk;
            }
        }
        __syncthreads();
        // ---- conv2 (dilation d2): output row j <-> global m0 + j, reads x1 rows j + H2 + dv[t] ----
#pragma unroll
        for (int j = 0; j < TM; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const unsigned char* rowp = t1 + (wrow + (lane & 31) + H2 + a.dv[t]) * PITCH_ + koff;
#pragma unroll
            for (int kk = 0; kk < KS; kk++)
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    const uint4 xf = *(const uint4*)(rowp + j * 32 * PITCH_ + kk * 32);
                    acc[0][j] = mfma16<F16>(TWO_SETS ? w2[TWO_SETS ? t : 0][TWO_SETS ? kk : 0] : w[t][kk], xf, acc[0][j]);
                }
        }
        // (no barrier: the x slab has been dead since the barrier above -- its area becomes the transpose stage; x1 stays readable)
        const int lim = (m0 + BMO < out_len) ? m0 + BMO : out_len;
        // residual x1 = inverse lrelu of the x1 rows of this tile (output row j <-> x1 row j + H2): no global re-read
        epilogue_rows<TM, 1, 1, -1, F16>(a, acc, b, m0 + wrow, wc * 32, lim, lane, slab + wave * (32 * (32 * 4 + 16)),
                                   t1 + (wrow + H2) * PITCH_, PITCH_);
    }
}

template <int C, int NT, int BM, int WM, int WN, int MINW>
static bool launch_rb2fuse_c(const GemmArgs& a, int h2, hipStream_t stream) {
    const int bmo = BM - 2 * h2;
    if (bmo < 32 || a.halo_l > 16) return false;
    const size_t pitch = C * 2 + 16;
    const size_t sb = (((size_t)(BM + 2 * a.halo_l) * pitch + 15) & ~(size_t)15);
    if (sb < (size_t)4 * 32 * (32 * 4 + 16)) return false;           // the slab's area doubles as the epilogue's transpose stage
    const size_t lds = sb + (size_t)(BM + 2 * h2) * pitch;
    if (lds > 160 * 1024) return false;
    const int ntm = (a.M + bmo - 1) / bmo, ntiles = ntm * a.nbatch;
    const dim3 grid(ntiles);
    if (a.dtype == DT_F16) { auto kfn = rb2fuse_kernel<C, NT, BM, WM, WN, MINW, true>; if (!lds_opt_in((const void*)kfn)) return false; ZVX_LAUNCH(kfn, grid, dim3(256), lds, stream, a, h2, ntm, ntiles); }
    else { auto kfn = rb2fuse_kernel<C, NT, BM, WM, WN, MINW, false>; if (!lds_opt_in((const void*)kfn)) return false; ZVX_LAUNCH(kfn, grid, dim3(256), lds, stream, a, h2, ntm, ntiles); }
    return true;
}

// a.fused == 2: both convolutions of a ResBlock2 (conv1: Wp2 / bias1 / dv1, conv2: Wp / bias / dv; same kernel size, two dilations) + the
// block's residual epilogue.  Variant id, or -1 when the shape is not covered (the caller then runs the two launches)
int launch_rb2fuse(GemmArgs a, hipStream_t stream) {
    if (a.dtype == DT_F32 || !a.Wp || !a.Wp2 || a.N != a.K || a.nheads != 1 || a.wout > 0 || a.bflat || a.K2) return -1;
    if (!(a.ntaps == 3 || a.ntaps == 5 || a.ntaps == 7) || !(a.N == 32 || a.N == 64)) return -1;
    const int h = (a.ntaps - 1) / 2, d1 = a.dv1[1] - a.dv1[0], d2 = a.dv[1] - a.dv[0];
    if (d1 < 1 || d2 < 1) return -1;
    for (int t = 0; t < a.ntaps; t++) if (a.dv1[t] != (t - h) * d1 || a.dv[t] != (t - h) * d2) return -1;
    // the shared run-time epilogue with the residual taken from LDS: what the vocoder asks of a ResBlock's closing convolution
    if (a.alpha != 1.f || a.bias_mode != 1 || !a.bias || !a.bias1 || a.post_scale || a.res_mode != 2 || a.res != a.X || a.res_dtype != a.dtype || a.ldo % 8 ||
        (a.out && a.out_dtype != a.dtype) || (a.accum && (a.lda % 8 || a.accum_dtype != a.dtype)) || a.in_len != a.out_len || a.ldx != a.N) return -1;
    a.halo_l = a.halo_r = h * d1;
    a.fused = 2;
    // (C = 64, k = 7 -- second dilation 12, 36 halo rows either side, 87 KiB of LDS = one workgroup per CU -- measured 0.72 ms fused
    // against 0.49 ms as two launches: the caller runs that block's convolutions separately)
    if (a.N == 32) {
        if (a.ntaps == 3 && launch_rb2fuse_c<32, 3, 256, 4, 1, 2>(a, h * d2, stream)) return 30;
        if (a.ntaps == 5 && launch_rb2fuse_c<32, 5, 256, 4, 1, 2>(a, h * d2, stream)) return 30;
        if (a.ntaps == 7 && launch_rb2fuse_c<32, 7, 256, 4, 1, 2>(a, h * d2, stream)) return 30;
    } else {
        if (a.ntaps == 3 && launch_rb2fuse_c<64, 3, 256, 2, 2, 2>(a, h * d2, stream)) return 31;
        if (a.ntaps == 5 && launch_rb2fuse_c<64, 5, 256, 2, 2, 2>(a, h * d2, stream)) return 31;
    }
    return -1;
}

// ================================================================================================
// resfuse, persistent form: the same fused ResBlock1 pair, but the weights are loaded ONCE per CU.
// The per-tile version above re-fetches both convs' fragments (up to 88 KiB per wave) for every tile of
// ~118 rows.  Here one 8-wave workgroup per CU loops over its tiles q_0, q_1, ... with wave-specialised roles;
// in iteration i
//     waves 0-3 (conv1, dilated):  request slab(q_i+2) by LDS-DMA;  T1(q_i) = lrelu(acc + b1) -> LDS;  acc = conv1(slab(q_i+1))
//     waves 4-7 (conv2):           acc = conv2(T1(q_i-1));  out(q_i-1) = acc + b2 + x   (residual from slab(q_i-1), row-major epilogue)
// so that on every SIMD (waves w and w+4 share one) the MFMA phase of one role runs beside the VALU/LDS/store
// phase of the other.  Each wave keeps the weight fragments of ITS conv and ITS 32 output channels in registers
// for the whole launch.  Slabs (4 rotating buffers, padded rows) are filled by `buffer_load_dwordx4 ... lds`
// (bounds-checked: rows outside the utterance arrive as zeros; the pad slot of each row fetches nothing); the
// DMA is inline asm, so hipcc schedules no waits for it -- the only vmcnt wait is the one in front of the
// barrier that ends the iteration, a full iteration after the request.  T1 is double-buffered.
// ================================================================================================
// AM = accum_mode (bit0: += xs, bit1: xs = result), HAS_OUT: a bf16 output is written (act = leaky-relu with a.slope, or none).
// Compile-time, because a run-time mode switch inside the epilogue makes hipcc merge the paths' `s_waitcnt vmcnt`s
// (accumulator loads) into every launch, where they then wait for the previous tile's stores.
template <int C, int NT, int AM, bool HAS_OUT, int TM, bool F16 = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void resfuse_persist_kernel(const GemmArgs a, int ntm, int ntiles) {
    if (F16) f16_saturate_mode();                          // the 16-bit tensors are IEEE half: f32 -> f16 converts clamp to +-65504 (mfma_util.h)
    // C = 16 / 8 (HiFi-GAN V2's last stages): one half-empty 32-channel tile per wave, and for C = 8 a k16 step whose
    // second 8-channel half is the (zeroed) pad slot of the row -- these stages are HBM-bound, the idle MFMA rows are free
    constexpr int KS = C >= 16 ? C / 16 : 1, CPR = C / 8, NTL = C >= 32 ? C / 32 : 1, RG = 4 / NTL;
    constexpr int QN = C >= 32 ? 4 : C / 8;               // 8-channel groups of the wave's tile that exist
    constexpr int BM1 = 32 * TM * RG;                          // T1 rows per tile (conv2's input incl. its halo)
    constexpr int H2 = (NT - 1) / 2, BMO = BM1 - 2 * H2;  // output rows per tile
    constexpr int P = C * 2 + 16, CPP = CPR + 1;          // padded row pitch (conflict-free b128 reads), 16-byte slots per row
    constexpr int NW = NT * KS;
    constexpr bool LEAN = NW > 36 || (F16 && NW >= 28 && TM == 2 && (AM & 1) && HAS_OUT);   // C = 64, k = 11: 44 fragments per wave -> 36 resident, register-lean epilogue (half, C = 64, k = 7, running sum read + an output: lean too)
    constexpr int NRES = LEAN ? (NW < 36 ? NW : 36) : NW; // fragments per wave / of those resident in registers (the rest: re-read from L2 per tile)
    typedef __attribute__((ext_vector_type(4))) int i32x4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPRs, scalar branches
    const int role = wave >> 2, w4 = wave & 3;
    const int wc = w4 % NTL, wr = w4 / NTL, wrow = wr * 32 * TM;
    const int H1 = a.halo_l, SR = BM1 + 2 * H1;
    const int dil = a.dv1[1] - a.dv1[0];
    const float slope1 = a.slope1;
    const int SB = (SR * P + 1023) & ~1023;               // bytes per slab buffer (whole 1-KiB DMA pieces)
    const int TB = ((BM1 + 2 * H2) * P + 15) & ~15;
    unsigned char* const t1base = lds + 4 * SB;
    unsigned char* const stage = t1base + 2 * TB + w4 * (32 * 80);          // conv2 waves: 32 rows x 32 ch bf16, pitch 80
    float* const bias1_l = (float*)(t1base + 2 * TB + 4 * (32 * 80));
    float* const bias2_l = bias1_l + C;
    int* const lens_l = (int*)(bias2_l + C);                // [2][128]: out_len, in_len per utterance (nbatch <= 128)
    const unsigned lds_addr0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const int G = gridDim.x;
    if (C < 32) {                                            // row pads are read as operands (C = 8) / never written (T1): start from zeros
        for (int i = tid * 16; i < 4 * SB + 2 * TB; i += 512 * 16) *(uint4*)(lds + i) = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    if (tid < C) { bias1_l[tid] = a.bias1[tid]; bias2_l[tid] = a.bias[tid]; }
    if (a.nbatch <= 128 && tid < a.nbatch) { lens_l[tid] = a.out_len ? a.out_len[tid] : a.M; lens_l[128 + tid] = a.in_len ? a.in_len[tid] : a.in_len_static; }

    // this wave's weights: conv1 <- Wp2, conv2 <- Wp (packed stream [nt32][tap][4 k16 slots], 1 KiB fragments)
    constexpr int NKC = (C + 63) / 64;                      // 64-channel K-chunks of the packed stream [nt32][chunk][tap][4 k16 slots]
    const uint4* const Wq = (const uint4*)(role ? a.Wp : a.Wp2) + ((long)wc * NKC * NT * 4) * 64 + lane;
    auto wfrag = [](int t, int kk) { return (((kk >> 2) * NT + t) * 4 + (kk & 3)) * 64; };
    uint4 w[NRES];
#pragma unroll
    for (int i = 0; i < NRES; i++) w[i] = Wq[wfrag(i / KS, i % KS)];

    // this wave's bias (conv1: b1, conv2: b2) for its 16 channels per lane: registers when they are to spare, else LDS
    constexpr bool BIAS_REG = NW <= 22;
    const int h4 = 4 * (lane >> 5);
    float4 bq[4];
    if (BIAS_REG) {
#pragma unroll
        for (int q = 0; q < 4; q++) bq[q] = q < QN ? *(const float4*)((role ? a.bias : a.bias1) + wc * 32 + 8 * q + h4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // Settle every load issued so far HERE: a compiler-placed `s_waitcnt vmcnt(n)` at a first use inside the tile loop
    // would also wait for the (hidden, in-order) slab DMAs of the conv1 waves and expose their full latency.
#pragma unroll
    for (int i = 0; i < NRES; i++) asm volatile("" :: "v"(w[i].x));
    if (BIAS_REG) {
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("" :: "v"(bq[q].x));
    }
    __syncthreads();                                        // bias1_l / bias2_l visible
    struct Tile { int t, b, mt, m0, in_len, out_len; };
    // Tile walk: tile t <-> (utterance b, row tile mt), advanced by G tiles without divisions.  Per-utterance lengths come
    // from an LDS table (<= 128 utterances) or through the scalar cache: a vector load here would make hipcc wait
    // vmcnt(0) inside the tile loop, i.e. for every store (conv2 waves) or slab DMA (conv1 waves) still in flight.
    const bool use_tab = a.nbatch <= 128;
    auto sload = [&](const int* p) { int v; asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory"); return v; };
    auto len_of = [&](const int* g, int which, int b, int dflt) {
        if (!g) return dflt;
        return use_tab ? __builtin_amdgcn_readfirstlane(lens_l[which * 128 + b]) : sload(g + b);
    };
    const int gq = G / ntm, gr = G % ntm;
    auto load_tile = [&](int t, int b, int mt) {             // first valid tile at or after (t, b, mt), stepping by G
        Tile q; q.t = -1; q.b = q.mt = q.m0 = q.in_len = q.out_len = 0;
        for (; t < ntiles; t += G, b += gq, mt += gr) {
            if (mt >= ntm) { mt -= ntm; b++; }
            const int m0 = mt * BMO, ol = len_of(a.out_len, 0, b, a.M);
            if (m0 < ol) { q.t = t; q.b = b; q.mt = mt; q.m0 = m0; q.out_len = ol; q.in_len = len_of(a.in_len, 1, b, a.in_len_static); break; }
        }
        q.t = __builtin_amdgcn_readfirstlane(q.t); q.b = __builtin_amdgcn_readfirstlane(q.b); q.mt = __builtin_amdgcn_readfirstlane(q.mt);
        q.m0 = __builtin_amdgcn_readfirstlane(q.m0);
        q.in_len = __builtin_amdgcn_readfirstlane(q.in_len); q.out_len = __builtin_amdgcn_readfirstlane(q.out_len);
        return q;
    };
    auto next_tile = [&](const Tile& q) {
        int b = q.b + gq, mt = q.mt + gr;
        return load_tile(q.t + G, b, mt);
    };
    // LDS-DMA of a tile's slab (global rows g0 = m0-H2-H1 ..) into buffer `buf`: piece p = 64 lanes x 16 B, lane-linear in
    // LDS (padded rows: the 9th / 5th 16-byte slot of a row is the pad and fetches nothing).  The buffer descriptor is
    // based at row g0, so the lane offsets are tile-independent (computed once); num_records ends at the utterance's last
    // row (rows past it -> zeros), rows before its first row are sent out of range by hand.
    constexpr int MAXP = C == 128 ? 10 : 8;
    constexpr bool VREL_REG = NW <= 22;
    const int npieces = SB >> 10;
    auto vrel_of = [&](int n) {
        const int cp = (w4 + 4 * n) * 64 + lane, row = cp / CPP, qs = cp % CPP;
        return qs == CPR ? -(1 << 30) : (row * a.ldx + (qs << 3)) * 2;
    };
    int vrel[VREL_REG ? MAXP : 1];
    if (VREL_REG) {
#pragma unroll
        for (int n = 0; n < MAXP; n++) vrel[n] = vrel_of(n);
    }
    auto dma_slab = [&](const Tile& q, int buf) {
        const int g0 = q.m0 - H2 - H1;
        const unsigned long long pa = (unsigned long long)((const unsigned short*)a.X + (long)q.b * a.x_bs + (long)g0 * a.ldx);
        const i32x4 rs = {__builtin_amdgcn_readfirstlane((int)(unsigned)pa), __builtin_amdgcn_readfirstlane((int)((pa >> 32) & 0xffff)),
                          __builtin_amdgcn_readfirstlane((q.in_len - g0) * a.ldx * 2), 0x00020000};
        const int thr = -g0 * a.ldx * 2;                    // offsets below this belong to rows before the utterance
        const unsigned la0 = lds_addr0 + buf * SB + w4 * 1024;
#pragma unroll
        for (int n = 0; n < MAXP; n++) {
            if (w4 + 4 * n < npieces) {
                const int vr = VREL_REG ? vrel[VREL_REG ? n : 0] : vrel_of(n);
                const int voff = vr < thr ? -16 : vr;
                const unsigned la = __builtin_amdgcn_readfirstlane(la0 + n * 4096);
                asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(la), "v"(voff), "s"(rs) : "memory", "m0");
            }
        }
    };

    Tile qA, qB, qC, qD;                                    // q_i-1 (conv2), q_i (T1 epilogue), q_i+1 (conv1 MFMA), q_i+2 (DMA)
    qA = load_tile(ntiles, 0, 0); qB = qA;
    qC = load_tile(blockIdx.x, blockIdx.x / ntm, blockIdx.x % ntm);
    qD = qC.t >= 0 ? next_tile(qC) : qA;
    if (role == 0 && qC.t >= 0) dma_slab(qC, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int koff = (lane >> 5) * 16;
    f32x16 acc[1][TM];
    for (int ph = 0; qA.t >= 0 || qB.t >= 0 || qC.t >= 0; ph++) {
        // slab buffer of q_n is n & 3 (q_i+1 <-> ph); T1 buffer of q_i is (ph-1) & 1
        const Tile qE = qD.t >= 0 ? next_tile(qD) : qD;      // looked up early: its scalar loads hide behind the iteration
        if (role == 0) {
            if (qD.t >= 0) dma_slab(qD, (ph + 1) & 3);
            if (qB.t >= 0) {
                // ---- T1 = lrelu(acc + b1) as bf16, zero outside the sequence (conv2 zero-pads ITS input, hifigan.py:39-44) ----
                unsigned char* t1 = t1base + ((ph - 1) & 1) * TB;
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    const int i = wrow + j * 32 + (lane & 31);
                    const int g = qB.m0 - H2 + i;
                    const bool inside = g >= 0 && g < qB.in_len;
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        const int co = wc * 32 + 8 * q + h4;
                        const float4 bb = BIAS_REG ? bq[q] : *(const float4*)(bias1_l + co);
                        const f32x2 v01 = lrelu2((f32x2){acc[0][j][4 * q], acc[0][j][4 * q + 1]} + (f32x2){bb.x, bb.y}, slope1);
                        const f32x2 v23 = lrelu2((f32x2){acc[0][j][4 * q + 2], acc[0][j][4 * q + 3]} + (f32x2){bb.z, bb.w}, slope1);
                        uint2 pk;
                        pk.x = inside ? pack16<F16>(v01.x, v01.y) : 0u;
                        pk.y = inside ? pack16<F16>(v23.x, v23.y) : 0u;
                        *(uint2*)(t1 + i * P + co * 2) = pk;
                    }
                }
            }
            if (qC.t >= 0) {
                // ---- conv1 (dilated): T1 row i <-> global row m0 - H2 + i, reads slab rows i + H1 + (t - H2) * dil ----
#pragma unroll
                for (int j = 0; j < TM; j++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
                const unsigned char* rowp0 = lds + (ph & 3) * SB + (wrow + (lane & 31) + H1 - H2 * dil) * P + koff;
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const unsigned char* rowp = rowp0 + t * dil * P;
#pragma unroll
                    for (int kk = 0; kk < KS; kk++) {
                        const uint4 wf = (t * KS + kk < NRES) ? w[t * KS + kk < NRES ? t * KS + kk : 0] : Wq[wfrag(t, kk)];
#pragma unroll
                        for (int j = 0; j < TM; j++) {
                            const uint4 xf = *(const uint4*)(rowp + j * 32 * P + kk * 32);
                            acc[0][j] = mfma16<F16>(wf, xf, acc[0][j]);
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this iteration's slab request has landed
        } else if (qA.t >= 0) {
            // ---- conv2 (dilation 1): output row j <-> global m0 + j, reads T1 rows j + t ----
#pragma unroll
            for (int j = 0; j < TM; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[0][j][e] = 0.f;
            const unsigned char* rowp = t1base + (ph & 1) * TB + (wrow + (lane & 31)) * P + koff;
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int kk = 0; kk < KS; kk++) {
                    const uint4 wf = (t * KS + kk < NRES) ? w[t * KS + kk < NRES ? t * KS + kk : 0] : Wq[wfrag(t, kk)];
#pragma unroll
                    for (int j = 0; j < TM; j++) {
                        const uint4 xf = *(const uint4*)(rowp + (t + j * 32) * P + kk * 32);
                        acc[0][j] = mfma16<F16>(wf, xf, acc[0][j]);
                    }
                }
            const int lim_rows = (qA.m0 + BMO < qA.out_len) ? qA.m0 + BMO : qA.out_len;
            const int lim = (C >= 32 || (lane & 3) < CPR) ? lim_rows : -(1 << 30);   // row-major phase: lanes past the last channel chunk idle
            // ---- epilogue in the MFMA layout (lane = time row, 4 consecutive channels per quad): + b2, + x (inverse lrelu of
            //      the slab rows of this tile: output row j <-> slab row j + H2 + H1), xs accumulation, activation; the bf16
            //      results pass through a per-wave LDS stage only to be stored as whole 64-byte row segments ----
            {
                const float rinv = a.res_inv_slope, oscale = a.out_scale, slope = a.act == ACT_LRELU ? a.slope : 1.f;
                const unsigned char* resp = lds + ((ph + 2) & 3) * SB + (wrow + H2 + H1 + (lane & 31)) * P + (wc * 32 + h4) * 2;
                const long rm_off = wc * 32 + (lane & 3) * 8;       // row-major phase: this lane's 8 channels
                unsigned short* accp = (unsigned short*)a.accum + (long)qA.b * a.a_bs + rm_off;
                unsigned short* outp = (unsigned short*)a.out + (long)qA.b * a.o_bs + rm_off;
                float4 bb[LEAN ? 1 : 4];
                if (!LEAN) {
#pragma unroll
                    for (int q = 0; q < QN; q++) bb[LEAN ? 0 : q] = BIAS_REG ? bq[q] : *(const float4*)(bias2_l + wc * 32 + 8 * q + h4);
                }
                // running sum xs of the resblocks (bf16, row-major): requested up front, consumed in the copy-out phase
                constexpr bool XS_EARLY = NW < 28 || TM == 1;   // registers permitting, for the whole tile at once
                uint4 xs[TM][2];
                if ((AM & 1) && XS_EARLY) {
#pragma unroll
                    for (int j = 0; j < TM; j++)
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int gr = qA.m0 + wrow + j * 32 + h * 16 + (lane >> 2);
                            xs[j][h] = *(const uint4*)(accp + (gr < lim ? (long)gr * a.lda : 0));
                        }
                }
#pragma unroll
                for (int j = 0; j < TM; j++) {
                    if ((AM & 1) && !XS_EARLY) {
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int gr = qA.m0 + wrow + j * 32 + h * 16 + (lane >> 2);
                            xs[j][h] = *(const uint4*)(accp + (gr < lim ? (long)gr * a.lda : 0));
                        }
                    }
                    // MFMA layout: y = acc + b2 + x;  without xs the activation is applied here, with xs in the row-major phase
                    uint2 rrj[LEAN ? 1 : 4];
                    if (!LEAN) {
#pragma unroll
                        for (int q = 0; q < QN; q++) rrj[LEAN ? 0 : q] = *(const uint2*)(resp + j * 32 * P + q * 16);
                    }
                    uint2 pk[LEAN ? 1 : 4];
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        const float4 bq_ = LEAN ? *(const float4*)(bias2_l + wc * 32 + 8 * q + h4) : bb[LEAN ? 0 : q];
                        const uint2 rq_ = LEAN ? *(const uint2*)(resp + j * 32 * P + q * 16) : rrj[LEAN ? 0 : q];
                        f32x2 v01 = (f32x2){acc[0][j][4 * q], acc[0][j][4 * q + 1]} + (f32x2){bq_.x, bq_.y} + inv_lrelu2(unpack16<F16>(rq_.x), rinv);
                        f32x2 v23 = (f32x2){acc[0][j][4 * q + 2], acc[0][j][4 * q + 3]} + (f32x2){bq_.z, bq_.w} + inv_lrelu2(unpack16<F16>(rq_.y), rinv);
                        if (!AM) { v01 = lrelu2(v01, slope); v23 = lrelu2(v23, slope); }      // slope 1 = no activation
                        uint2 pq;
                        pq.x = pack16<F16>(v01.x, v01.y);
                        pq.y = pack16<F16>(v23.x, v23.y);
                        if (LEAN) *(uint2*)(stage + (lane & 31) * 80 + (8 * q + h4) * 2) = pq;
                        else pk[LEAN ? 0 : q] = pq;
                    }
                    if (!LEAN) {
#pragma unroll
                        for (int q = 0; q < QN; q++) *(uint2*)(stage + (lane & 31) * 80 + (8 * q + h4) * 2) = pk[LEAN ? 0 : q];
                    }
                    // row-major: 16 rows x 64 bytes per instruction
                    uint4 o[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) o[h] = *(const uint4*)(stage + (h * 16 + (lane >> 2)) * 80 + (lane & 3) * 16);
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int gr = qA.m0 + wrow + j * 32 + h * 16 + (lane >> 2);
                        if (AM) {
                            f32x2 t[4] = {unpack16<F16>(o[h].x), unpack16<F16>(o[h].y), unpack16<F16>(o[h].z), unpack16<F16>(o[h].w)};
                            if (AM & 1) {
                                t[0] += unpack16<F16>(xs[j][h].x); t[1] += unpack16<F16>(xs[j][h].y);
                                t[2] += unpack16<F16>(xs[j][h].z); t[3] += unpack16<F16>(xs[j][h].w);
                            }
                            if ((AM & 2) && gr < lim)
                                *(u32x4*)(accp + (long)gr * a.lda) = (u32x4){pack16<F16>(t[0].x, t[0].y), pack16<F16>(t[1].x, t[1].y),
                                                                            pack16<F16>(t[2].x, t[2].y), pack16<F16>(t[3].x, t[3].y)};
                            if (HAS_OUT) {
#pragma unroll
                                for (int e = 0; e < 4; e++) t[e] = lrelu2(t[e] * oscale, slope);
                                o[h] = make_uint4(pack16<F16>(t[0].x, t[0].y), pack16<F16>(t[1].x, t[1].y), pack16<F16>(t[2].x, t[2].y), pack16<F16>(t[3].x, t[3].y));
                            }
                        }
                        if (HAS_OUT && gr < lim) *(uint4*)(outp + (long)gr * a.ldo) = o[h];
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        qA = qB; qB = qC; qC = qD; qD = qE;
    }
}

template <int C, int TM = 2>
static bool launch_resfuse_persist_c(const GemmArgs& a, hipStream_t stream) {
    // 32*TM rows per wave; C = 64, k = 11 (44 fragments = 176 registers per wave) only fits with one row block per wave
    constexpr int BM1 = 32 * TM * (4 / (C >= 32 ? C / 32 : 1));
    const int h2 = (a.ntaps - 1) / 2, bmo = BM1 - 2 * h2;
    const int ntm = (a.M + bmo - 1) / bmo, ntiles = ntm * a.nbatch;
    const int ncu = persistent_cus();
    dim3 grid(ntiles < ncu ? ntiles : ncu);
    for (int t = 0; t < a.ntaps; t++)                      // the kernel derives the taps from (kernel size, dilation)
        if (a.dv[t] != t - h2 || a.dv1[t] != (t - h2) * (a.dv1[1] - a.dv1[0])) return false;
    const size_t sb = ((size_t)(BM1 + 2 * a.halo_l) * (C * 2 + 16) + 1023) & ~(size_t)1023;
    const size_t tb = ((size_t)(BM1 + 2 * h2) * (C * 2 + 16) + 15) & ~(size_t)15;
    const size_t lds = 4 * sb + 2 * tb + 4 * 32 * 80 + 2 * C * 4 + 2 * 128 * 4;
    if (lds > 160 * 1024) return false;
    // the in-kernel epilogue covers exactly what the vocoder asks for
    if (a.alpha != 1.f || a.bias_mode != 1 || a.post_scale || (a.out && a.out_dtype != a.dtype) || a.res_mode != 2 || a.res_dtype != a.dtype || a.ldo % 8 || (a.accum && (a.lda % 8 || a.accum_dtype != a.dtype))) return false;
    if (a.act != ACT_NONE && a.act != ACT_LRELU) return false;
    if (!a.accum_mode && a.out_scale != 1.f) return false;
    const int am = a.accum ? a.accum_mode : 0;
    if (!a.out && !(am & 2)) return false;
#define ZVX_RFP(NT_, AM_, HO_) if (a.dtype == DT_F16) ZVX_LAUNCH((resfuse_persist_kernel<C, NT_, AM_, HO_, TM, true>), grid, dim3(512), lds, stream, a, ntm, ntiles); else ZVX_LAUNCH((resfuse_persist_kernel<C, NT_, AM_, HO_, TM>), grid, dim3(512), lds, stream, a, ntm, ntiles); return true
#define ZVX_RFP_MODE(NT_) \
    if (a.out) { if (am == 0) { ZVX_RFP(NT_, 0, true); } if (am == 1) { ZVX_RFP(NT_, 1, true); } if (am == 2) { ZVX_RFP(NT_, 2, true); } ZVX_RFP(NT_, 3, true); } \
    else { if (am == 2) { ZVX_RFP(NT_, 2, false); } ZVX_RFP(NT_, 3, false); }
    if constexpr (TM == 1) {
        if (a.ntaps == 11) { ZVX_RFP_MODE(11) }
    } else {
        if (a.ntaps == 3) { ZVX_RFP_MODE(3) }
        if (a.ntaps == 7) { ZVX_RFP_MODE(7) }
        if constexpr (C <= 32) { if (a.ntaps == 11) { ZVX_RFP_MODE(11) } }
    }
#undef ZVX_RFP_MODE
#undef ZVX_RFP
    return false;
}

int launch_resfuse(GemmArgs a, hipStream_t stream) {
    if (a.dtype == DT_F32 || !a.Wp || !a.Wp2 || a.N != a.K || a.nheads != 1 || a.wout > 0) return -1;
    if (!(a.ntaps == 3 || a.ntaps == 7 || a.ntaps == 11)) return -1;
    int h1 = 0;
    for (int i = 0; i < a.ntaps; i++) { const int d = a.dv1[i] < 0 ? -a.dv1[i] : a.dv1[i]; if (d > h1) h1 = d; }
    if (h1 > 32) return -1;
    a.halo_l = a.halo_r = h1;
    a.fused = 1;
    if (a.N == 128 && a.no_pairstream != 1) {
        // C = 128: the streaming pair kernel (pairstream.hip); its epilogue covers exactly what the vocoder asks for
        const int h2 = (a.ntaps - 1) / 2, dil = a.dv1[1] - a.dv1[0];
        bool ok = a.alpha == 1.f && a.bias_mode == 1 && !a.post_scale && (!a.out || a.out_dtype == a.dtype) && a.res_mode == 2 && a.res_dtype == a.dtype &&
                  a.res == a.X && a.r_bs == a.x_bs && a.ldr == a.ldx && (!a.accum || a.accum_dtype == a.dtype) && (a.act == ACT_NONE || a.act == ACT_LRELU) &&
                  (a.accum_mode || a.out_scale == 1.f) && a.in_len == a.out_len;
        for (int t = 0; t < a.ntaps; t++) ok = ok && a.dv[t] == t - h2 && a.dv1[t] == (t - h2) * dil;
        if (ok) {
            PairArgs p;
            memset(&p, 0, sizeof p);
            p.X = a.X; p.x_bs = a.x_bs; p.ldx = a.ldx; p.W1 = a.Wp2; p.W2 = a.Wp; p.b1 = a.bias1; p.b2 = a.bias;
            p.C = a.N; p.ntaps = a.ntaps; p.dil = dil;
            p.out = a.out; p.o_bs = a.o_bs; p.ldo = a.ldo;
            p.accum = a.accum; p.a_bs = a.a_bs; p.lda = a.lda; p.accum_mode = a.accum ? a.accum_mode : 0;
            p.slope1 = a.slope1; p.res_inv_slope = a.res_inv_slope; p.out_scale = a.out_scale; p.slope = a.act == ACT_LRELU ? a.slope : 1.f;
            p.f16 = a.dtype == DT_F16;
            p.len = a.out_len; p.M = a.M; p.nbatch = a.nbatch; p.force = a.no_pairstream == 2;
            if (launch_pairstream(p, stream, g_dry_run)) return 23;
        }
    }
    {
        if (a.N == 32 && launch_resfuse_persist_c<32>(a, stream)) return 16;
        if (a.N == 64 && a.ntaps != 11 && launch_resfuse_persist_c<64>(a, stream)) return 17;
        // C = 64, k = 11 (44 fragments = 176 registers per wave): one 32-row block per wave, 36 fragments resident and 8
        // re-read from L2 per tile, register-lean epilogue -- 0.85 ms against 0.95 ms for the per-tile kernel
        if (a.N == 64 && a.ntaps == 11 && launch_resfuse_persist_c<64, 1>(a, stream)) return 17;
        // (round 6: the C = 128 / 16 / 8 instantiations of this kernel are gone -- C = 128 pairs run on pairstream.hip or as the two conv-slab
        // launches it is bit-identical to, C = 16 / 8 stages on narrowstage.hip or, where that declines, as two launches per pair: 84 fewer
        // instantiations, none of them on a default path since round 5)
    }
    return -1;                                                 // (round 6: the per-tile fallback kernel is gone -- the caller runs the pair as two launches)
}
#endif  // ZVX_PART_RESFUSE
#if ZVX_PART_MAIN

struct Variant { const char* name; int dt, bm, bn; };
static const Variant kVariants[] = {
    {"gemm_bf16_128x128", DT_BF16, 128, 128}, {"gemm_bf16_256x64", DT_BF16, 256, 64},
    {"gemm_bf16_256x32", DT_BF16, 256, 32},   {"gemm_f32_128x128", DT_F32, 128, 128},
    {"gemm_f32_256x64", DT_F32, 256, 64},     {"gemm_f32_256x32", DT_F32, 256, 32},
    {"convslab_bf16_128x256", DT_BF16, 128, 256}, {"convslab_bf16_256x128", DT_BF16, 256, 128},
    {"convslab_bf16_256x64", DT_BF16, 256, 64},   {"convslab_bf16_256x32", DT_BF16, 256, 32},
    {"(unused)", DT_BF16, 0, 0}, {"resfuse_bf16_c8", DT_BF16, 256, 8}, {"resfuse_bf16_c16", DT_BF16, 256, 16}, {"resfuse_bf16_c128", DT_BF16, 64, 128},
    {"convreg_bf16_c32", DT_BF16, 512, 32},       {"convreg_bf16_c64", DT_BF16, 256, 64},
    {"resfuse_bf16_c32", DT_BF16, 256, 32},       {"resfuse_bf16_c64", DT_BF16, 128, 64},
    {"gemm_bf16_64x64", DT_BF16, 64, 64},         {"gemm_f32_64x64", DT_F32, 64, 64},
    {"resstream_bf16_c32", DT_BF16, 64, 32},      {"resstream_bf16_c64", DT_BF16, 32, 64},
    {"convslab_bf16_128x128", DT_BF16, 128, 128},
    {"pairstream_bf16_c128", DT_BF16, 128, 128},
    {"narrowstage_c16", DT_BF16, 256, 16}, {"narrowstage_c8", DT_BF16, 512, 8},      // whole narrow stages in one launch (narrowstage.hip)
    {"conv2d_persist_c32", DT_BF16, 384, 32}, {"conv2d_persist_c64", DT_BF16, 256, 64},   // persistent 3 x 3 convolutions of the speaker encoder (26, 27)
    {"conv2d_s2_c32", DT_BF16, 256, 64}, {"conv2d_s2_c64", DT_BF16, 128, 128},            // ... its stride-2 level transitions (28: + shortcut, 29)
    {"rb2fuse_bf16_c32", DT_BF16, 256, 32}, {"rb2fuse_bf16_c64", DT_BF16, 256, 64},       // a whole ResBlock2 per launch (30, 31; HiFi-GAN V3)
};
const char* gemm_variant_name(int id) { return kVariants[id].name; }
int gemm_num_variants() { return (int)(sizeof(kVariants) / sizeof(kVariants[0])); }


template <int BM, int BN, int WM, int WN, int MINW, int R, int EPI = -1>
static void launch_slab_variant(const GemmArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
    const bool fullk = a.K % SLAB_KC == 0 && a.K2 == 0;            // (a second source rides the partial-chunk variants: its K2 is any multiple of 16)
    // IEEE-half operands: every epilogue of the register-ring tiles (the vocoder's and the decoders' launches); on the other tile shapes the
    // run-time epilogue and the "bias + activation -> 16 bit" one
    if constexpr (R == 0 || EPI == -1 || EPI == ZVX_EPI(0, 0, 1) || EPI == ZVX_EPI_FLIP) {
        if (a.dtype == DT_F16) {
            if (fullk) ZVX_LAUNCH((convslab_kernel<BM, BN, WM, WN, true, MINW, R, EPI, 64, true>), grid, dim3(256), lds, stream, a);
            else if constexpr (EPI != ZVX_EPI_FLIP) ZVX_LAUNCH((convslab_kernel<BM, BN, WM, WN, false, MINW, R, EPI, 64, true>), grid, dim3(256), lds, stream, a);
            return;
        }
    }
    if constexpr (EPI < 0 || !(EPI & 16)) {                        // (the decoders' compile-time form exists in half only)
        if (fullk) ZVX_LAUNCH((convslab_kernel<BM, BN, WM, WN, true, MINW, R, EPI>), grid, dim3(256), lds, stream, a);
        else if constexpr (EPI != ZVX_EPI_FLIP) ZVX_LAUNCH((convslab_kernel<BM, BN, WM, WN, false, MINW, R, EPI>), grid, dim3(256), lds, stream, a);   // (the flipped-output form: whole K chunks only, gemm_epi_mode_of)
    }
}

// compile-time epilogue mode of a launch (see ZVX_EPI / ZVX_EPI_DEC), or -1 when it needs the run-time epilogue
int gemm_epi_mode_of(const GemmArgs& a) {
    if (a.alpha == 1.f && !a.post_scale && a.out && a.out_dtype != a.dtype && a.dtype != DT_F32 && a.out_dtype != DT_F32 && !a.out_split3 && a.bias_mode == 1 && a.bias &&
        (a.act == ACT_NONE || a.act == ACT_LRELU) && !a.res_mode && !(a.accum && a.accum_mode) && a.out_scale == 1.f && a.K % SLAB_KC == 0 && !a.K2) return ZVX_EPI_FLIP;
    if (a.alpha != 1.f || a.post_scale || (a.out && a.out_dtype != a.dtype) || a.dtype == DT_F32 || a.out_split3 || a.bias_mode == 2) return -1;
    const int am = a.accum ? a.accum_mode : 0;
    // the mel decoders' residual form (half only): (conv [+ raw residual]) x out_scale, no activation, 16-bit output
    if (a.dtype == DT_F16 && a.out && !am && a.act == ACT_NONE && a.res_mode <= 1 && (!a.res_mode || a.res_dtype == DT_F16) && (a.res_mode || a.out_scale != 1.f) &&
        (a.bias_mode == 0 || a.bias)) return ZVX_EPI_DEC(a.res_mode ? 1 : 0);
    if (a.bias_mode != 1 || !a.bias) return -1;
    if (a.act != ACT_NONE && a.act != ACT_LRELU) return -1;
    if (a.res_mode && (a.res_mode != 2 || a.res_dtype != a.dtype)) return -1;
    if (am && a.accum_dtype != a.dtype) return -1;
    if (!am && a.out_scale != 1.f) return -1;
    if (!a.out && !(am & 2)) return -1;
    const int e = ZVX_EPI(a.res_mode ? 1 : 0, am, a.out ? 1 : 0);
    switch (e) {
        case ZVX_EPI(0, 0, 1): case ZVX_EPI(1, 0, 1): case ZVX_EPI(1, 2, 0): case ZVX_EPI(1, 3, 0): case ZVX_EPI(1, 1, 1): return e;
    }
    return -1;
}

// a.xcd_flat (zvx_set_int "slab_flat", default 1): tile -> XCD remap over batch x tiles (decoder convs -2 %, bit-identical; tools/ab_slab_flat.sh)
// a.slab_small (zvx_set_int "slab_small", default 2): single-request tile choice: 0 none, 1 small row tiles, 2 + 32-channel tiles for one-row-tile launches
// Both are the CONTEXT's switches (zvx_ctx::gemm fills them): no process-wide state.
static int launch_convslab(GemmArgs a, hipStream_t stream) {
    const bool bflat_hint = a.bflat != 0;                              // the mel decoders' launches (their buffers carry padding rows)
    if (a.K2) {
        if (!a.X2 || a.K2 % 16 || a.ldx2 % 8 || a.flat_win || (a.bflat && a.x2_bs != (long)a.bflat * a.ldx2)) return -5;
    }
    if (a.bflat) {
        // batch-flattened: one row axis over all utterances (see GemmArgs::bflat); anything it does not cover runs per utterance
        int h = 0;
        for (int i = 0; i < a.ntaps; i++) { const int d = a.dv[i] < 0 ? -a.dv[i] : a.dv[i]; if (d > h) h = d; }
        const bool ok = a.in_len && a.out_len && a.nbatch > 1 && a.bflat >= a.M + h && a.x_bs == (long)a.bflat * a.ldx && (!a.out || a.o_bs == (long)a.bflat * a.ldo) &&
                        (!a.res_mode || a.r_bs == (long)a.bflat * a.ldr) && !a.accum_mode && a.bias_mode != 2 && !a.flat_win && a.M > 128 && a.N >= 128 &&
                        (long)a.nbatch * a.bflat < (1l << 30);
        if (!ok) a.bflat = 0;                               // (decided below, once the tile shape is known)
    }
    const int g_slab_small = a.slab_small & 7;                       // (name kept from when this was a process-wide static)
    int hl = 0, hr = 0;
    for (int i = 0; i < a.ntaps; i++) { hl = a.dv[i] < -hl ? -a.dv[i] : hl; hr = a.dv[i] > hr ? a.dv[i] : hr; }
    a.halo_l = hl; a.halo_r = hr;
    if (a.flat_win && !a.bflat) {
        // stride-1 3 x 3 convolution over flattened [H][W] maps (ResNetSE34V2.py:74-76): weights in registers for C = 32 / 64, the
        // 256 x 128 register-ring tile with a 160-row halo budget for C = 128 / 256
        // persistent form (slab_small bit 5: A/B switch, off): needs the per-utterance widths, the symmetric one-row halo and a map at
        // least one staging step wide
        if (a.N == a.K && (a.N == 32 || a.N == 64) && !(a.slab_small & 32) && a.dtype == DT_BF16 && a.ntaps == 9 && a.in_len && !a.out_len && hl == a.flat_win + 1 && hr == hl &&
            a.flat_win >= 64 && (long)a.flat_rows * a.ldx * 2 < 0x7fffffffL &&
            // ... and one of the block's two epilogue forms: conv1 -> ReLU -> BatchNorm (no bias), or conv2 + bias (folded BatchNorm)
            a.out && a.out_dtype == DT_BF16 && a.alpha == 1.f && a.out_scale == 1.f && !a.res_mode && !a.accum_mode && !a.out_split3 && a.ldo % 8 == 0 &&
            ((a.post_scale && a.post_shift && a.bias_mode == 0 && a.act == ACT_RELU) || (!a.post_scale && a.bias_mode == 1 && a.bias && a.act == ACT_NONE))) {
            if (a.N == 32 && hl + hr <= 544) { launch_conv2d_persist<32, 384, 4, 1, 544, 2>(a, stream); return 26; }
            if (a.N == 64 && hl + hr <= 288) { launch_conv2d_persist<64, 256, 4, 2, 288, 1>(a, stream); return 27; }
        }
        if (a.N == a.K && a.N == 32 && launch_convreg_c<32, 384, 4, 1, 2>(a, stream)) return 14;      // 384 rows: 2.35x halo over-read instead of 3x, two workgroups per CU still fit
        if (a.N == a.K && a.N == 64 && launch_convreg_c<64, 256, 2, 2, 2>(a, stream)) return 15;
        if (a.N % 128 || a.K % SLAB_KC || hl + hr > 160) return -4;
        // maps whose rows fill 256-row tiles badly (the last level of the speaker encoder: 10 x 34 = 340 positions are 1.33 tiles of
        // 256 -- a third of the matrix steps on padding -- and 2.66 of 128): 128-row tiles of the same kernel (same K order per output
        // row: bit-identical): config 5 6.44 -> 6.32 ms.  The level before it (1340 positions: 9 % padding against 5 %) measured 1.85 -> 1.88 ms with
        // 128-row tiles: not taken.
        const int pad256 = ((a.M + 255) / 256) * 256, pad128 = ((a.M + 127) / 128) * 128;
        if ((long)pad256 * 100 > (long)pad128 * 115) {
            dim3 g128((a.N / 128) * (pad128 / 128), a.nbatch);
            size_t lds128 = ((size_t)(128 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
            const size_t stage128 = (size_t)4 * 32 * (2 * 128 + 16);
            if (lds128 < stage128) lds128 = stage128;
            ZVX_LAUNCH((convslab_kernel<128, 128, 2, 2, true, 2, 0, -1, 160>), g128, dim3(256), lds128, stream, a);
            return 22;
        }
        dim3 grid((a.N / 128) * ((a.M + 255) / 256), a.nbatch);
        size_t lds = ((size_t)(256 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
        ZVX_LAUNCH((convslab_kernel<256, 128, 2, 2, true, 2, 0, -1, 160>), grid, dim3(256), lds, stream, a);
        return 7;
    }
    if (a.dtype != DT_F32 && a.N == a.K && !a.K2 && (a.ntaps == 3 || a.ntaps == 5 || a.ntaps == 7 || a.ntaps == 11)) {   // (a second source exists on the slab kernel only: round 5, found on a reduced-width model whose fused shortcut convolutions are square with C = 32 / 64)
        if (a.N == 32 && launch_convreg_c<32, 512, 4, 1, 2>(a, stream)) return 14;
        if (a.N == 64 && launch_convreg_c<64, 256, 2, 2, 2>(a, stream)) return 15;
    }
    if (hl + hr > 64) {
        // every tile kernel below stages at most 64 halo rows -- but for the 256 x 128 register-ring tile with the 160-row budget of the
        // flattened 2-D convolutions, here for the closing launch of V3's first stage (C = 128, k = 7, dilation 12: residual + running sum + output)
        if (hl + hr <= 160 && a.N % 128 == 0 && a.K % SLAB_KC == 0 && !a.K2 && !a.bflat && !a.flat_win && gemm_epi_mode_of(a) == ZVX_EPI(1, 1, 1)) {
            dim3 grid((a.N / 128) * ((a.M + 255) / 256), a.nbatch);
            const size_t lds = ((size_t)(256 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
            if (a.dtype == DT_F16) ZVX_LAUNCH((convslab_kernel<256, 128, 2, 2, true, 2, 0, ZVX_EPI(1, 1, 1), 160, true>), grid, dim3(256), lds, stream, a);
            else ZVX_LAUNCH((convslab_kernel<256, 128, 2, 2, true, 2, 0, ZVX_EPI(1, 1, 1), 160>), grid, dim3(256), lds, stream, a);
            return 7;
        }
        return -4;
    }
    // tile choice: padded N weighted by the tile's MFMA efficiency
    static const int bns[4] = {256, 128, 64, 32};
    static const double eff[4] = {0.95, 1.0, 0.7, 0.4};
    int best = 0; double best_cost = -1;
    for (int i = 0; i < 4; i++) {
        const double cost = (double)((a.N + bns[i] - 1) / bns[i]) * bns[i] / eff[i];
        if (best_cost < 0 || cost < best_cost - 1e-9) { best_cost = cost; best = i; }
    }
    static const int bms[4] = {128, 256, 256, 256};
    const int ncu = num_cus();
    // single requests (a launch whose 256-row tiles would occupy a fraction of the CUs): 64- / 128-row tiles, 128 channels wide.  The
    // K loop of a tile is the same whatever its shape, so results do not depend on this choice.
    // a launch of ONE row tile and a handful of 128-channel tiles (a single request's encoder GEMMs): the workgroups stream their
    // weights at the ~11 B/clk a CU sustains from HBM / Infinity Cache, so the launch is paced by how many CUs take part --
    // 32-channel tiles put four times as many on the weight stream
    if (g_slab_small >= 2 && a.M <= 64 && a.nbatch * ((a.N + 127) / 128) * 4 <= ncu && a.N >= 64 && hl + hr <= 64) {
        a.bflat = 0;
        dim3 g32((a.N + 31) / 32, a.nbatch);
        const size_t lds32 = (((size_t)(256 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023) + (size_t)8 * 1024;
        launch_slab_variant<256, 32, 4, 1, 2, 8>(a, g32, lds32, stream);
        return 9;
    }
    if (g_slab_small && a.M > 128 && a.N >= 128 && hl + hr <= 64) {
        const long wg256 = (long)((a.N + 127) / 128) * ((a.M + 255) / 256) * a.nbatch;
        if (wg256 * 2 <= ncu) {
            a.bflat = 0;
            const bool r64 = wg256 * 4 <= ncu;
            const int bm = r64 ? 64 : 128;
            dim3 gs(((a.N + 127) / 128) * ((a.M + bm - 1) / bm), a.nbatch);
            size_t lds = ((size_t)(bm + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
            const size_t stage = (size_t)4 * 32 * (2 * 128 + 16);
            if (lds < stage) lds = stage;
            if (r64) launch_slab_variant<64, 128, 2, 2, 2, 0>(a, gs, lds, stream);
            else launch_slab_variant<128, 128, 2, 2, 2, 0>(a, gs, lds, stream);
            return 22;
        }
    }
    // short utterances (the phoneme encoder: M <= 128 rows each): 256-row tiles would be half empty.  128-row tiles, 128 or 256
    // channels wide, whichever puts more workgroups on the chip while it is not yet full
    if (a.M <= 128 && a.N >= 128) {
        a.bflat = 0;
        const int wide = ((a.N + 255) / 256) * a.nbatch;
        const bool narrow = wide < 2 * ncu;
        const int bn = narrow ? 128 : 256;
        dim3 grid((a.N + bn - 1) / bn, a.nbatch);
        size_t lds = ((size_t)(128 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
        const size_t stage = (size_t)4 * 32 * (2 * 128 + 16);
        if (lds < stage) lds = stage;
        // fewer than two 128 x 128 workgroups per CU: 64-row tiles double the count, and the second workgroup of a CU is what
        // covers the first one's slab fills (these launches are latency-paced, not MFMA-paced)
        if (narrow && a.M > (g_slab_small ? 32 : 64) && ((a.N + 127) / 128) * a.nbatch < 2 * ncu) {   // (M <= 64 with half-empty 128-row tiles: single requests)
            dim3 g64(((a.N + 127) / 128) * ((a.M + 63) / 64), a.nbatch);
            launch_slab_variant<64, 128, 2, 2, 2, 0>(a, g64, lds, stream);
            return 22;
        }
        if (narrow) { launch_slab_variant<128, 128, 2, 2, 2, 0>(a, grid, lds, stream); return 22; }
        launch_slab_variant<128, 256, 1, 4, 2, 0>(a, grid, lds, stream);
        return 6;
    }
    // 1x1 convs (StyleTTS decoder) have no tap reuse of the slab: the wider channel tile halves the re-reads of the input
    // rows, and 128-row tiles divide the decoder's 896 frames exactly
    // ... unless the 256 x 128 tiling (batch-flattened where the caller allows it) takes a whole round of workgroups off the launch:
    // 32 x 896 frames x 1056 channels are 1125 tiles of 128 x 256 (3 rounds on 512 slots) and 1017 of 256 x 128 (2 rounds): 0.152 -> 0.136 ms
    if (a.ntaps == 1 && a.N >= 512) {
        const long slots = 2L * ncu;
        auto rounds = [&](int bm_, int bn_) {
            const long ntn_ = (a.N + bn_ - 1) / bn_, utt = ntn_ * ((a.M + bm_ - 1) / bm_) * a.nbatch;
            const long flat = a.bflat ? ntn_ * (((long)a.nbatch * a.bflat + bm_ - 1) / bm_) : utt;
            return ((flat < utt ? flat : utt) + slots - 1) / slots;
        };
        best = rounds(256, 128) <= rounds(128, 256) ? 1 : 0;      // (ties -> 256 x 128: the FFT-block decoder's N = 528 projections 4.68 -> 4.58 ms per call)
    }
    // 256x128 / 128x256 tiles take their weights through per-wave register rings (see the kernel)
    const bool wreg = best <= 1;
    const int ring_slots = wreg ? 0 : (best == 0 ? 4 : 8);
    const int bn = bns[best], bm = bms[best];
    const int ntn = (a.N + bn - 1) / bn;
    if (a.bflat) {
        // flatten when that takes a round of workgroups off the launch (two per CU are resident): 32 x 896 frames x 1056 channels are
        // 1152 tiles per utterance (every utterance ends in a half-empty tile) against 1017 flattened -- 3 rounds against 2; where the
        // count of rounds stays, the per-utterance launch (whose partial tiles stage and store less) is kept
        const long slots = 2L * ncu;
        const long wg_utt = (long)ntn * ((a.M + bm - 1) / bm) * a.nbatch, wg_flat = (long)ntn * (((long)a.nbatch * a.bflat + bm - 1) / bm);
        if ((wg_flat + slots - 1) / slots < (wg_utt + slots - 1) / slots) { a.flat_win = a.bflat; a.flat_rows = a.nbatch * a.bflat; a.M = a.flat_rows; a.nbatch = 1; }
        else a.bflat = 0;
    }
    // 256 x 128 tiles whose count quantises badly over the chip's 2 x CUs workgroup slots (N = 528 over 32 x 896 frames: 565 flattened
    // tiles = one full round and a tenth of a second one; per utterance 640 tiles, every utterance ending in a half-empty tile): 128-row
    // tiles of the same kernel (same K order per output row: bit-identical) where they take less time by the slot count -- a round of
    // 128-row tiles counts half a round of 256-row ones.
    if (best == 1 && bflat_hint && a.M > 256 && hl + hr <= 64) {   // (the mel decoders' launches: the vocoder's 256 x 128 launches are power-, not slot-limited)
        const long slots = 2L * ncu;
        const long t256 = (long)ntn * ((a.M + 255) / 256) * a.nbatch, t128 = (long)ntn * ((a.M + 127) / 128) * a.nbatch;
        const long eff256 = 2 * ((t256 + slots - 1) / slots), eff128 = (t128 + slots - 1) / slots;
        if (eff128 < eff256) {
            dim3 g128(ntn * ((a.M + 127) / 128), a.nbatch);
            size_t lds128 = ((size_t)(128 + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023;
            const size_t stage128 = (size_t)4 * 32 * (2 * 128 + 16);
            if (lds128 < stage128) lds128 = stage128;
            switch (gemm_epi_mode_of(a)) {
                case ZVX_EPI(0, 0, 1): launch_slab_variant<128, 128, 2, 2, 2, 0, ZVX_EPI(0, 0, 1)>(a, g128, lds128, stream); break;
                case ZVX_EPI_DEC(0): launch_slab_variant<128, 128, 2, 2, 2, 0, ZVX_EPI_DEC(0)>(a, g128, lds128, stream); break;
                case ZVX_EPI_DEC(1): launch_slab_variant<128, 128, 2, 2, 2, 0, ZVX_EPI_DEC(1)>(a, g128, lds128, stream); break;
                default: launch_slab_variant<128, 128, 2, 2, 2, 0>(a, g128, lds128, stream);
            }
            return 22;
        }
    }
    const int ntm = (a.M + bm - 1) / bm;
    dim3 grid(ntn * ntm, a.nbatch);
    const int tn = (bn >= 128) ? 2 : 1;
    if (a.accum_mode && a.accum && a.accum_dtype == DT_F16 && tn == 2 && !(best == 1 && gemm_epi_mode_of(a) >= 0)) return -6;   // (see epilogue_rows: acc_f16; the small-tile shapes above take it)
    size_t lds = (((size_t)(bm + hl + hr) * SLAB_PITCH + 1023) & ~(size_t)1023) + (size_t)ring_slots * (bn / 32) * 1024;      // slab + weight ring (R slots x bn/32 KiB)
    const size_t stage = (size_t)4 * 32 * (tn * 128 + 16);
    if (lds < stage) lds = stage;
    switch (best) {
        case 0: launch_slab_variant<128, 256, 1, 4, 2, 0>(a, grid, lds, stream); break;      // (register-ring variant)
        case 1: switch (gemm_epi_mode_of(a)) {                   // (always the register-ring variant: wreg)
                    case ZVX_EPI(0, 0, 1): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI(0, 0, 1)>(a, grid, lds, stream); break;
                    case ZVX_EPI_FLIP: launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI_FLIP>(a, grid, lds, stream); break;
                    case ZVX_EPI(1, 0, 1): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI(1, 0, 1)>(a, grid, lds, stream); break;
                    case ZVX_EPI(1, 2, 0): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI(1, 2, 0)>(a, grid, lds, stream); break;
                    case ZVX_EPI(1, 3, 0): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI(1, 3, 0)>(a, grid, lds, stream); break;
                    case ZVX_EPI(1, 1, 1): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI(1, 1, 1)>(a, grid, lds, stream); break;
                    case ZVX_EPI_DEC(0): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI_DEC(0)>(a, grid, lds, stream); break;
                    case ZVX_EPI_DEC(1): launch_slab_variant<256, 128, 2, 2, 2, 0, ZVX_EPI_DEC(1)>(a, grid, lds, stream); break;
                    default: launch_slab_variant<256, 128, 2, 2, 2, 0>(a, grid, lds, stream);
                }
                break;
        case 2: launch_slab_variant<256, 64, 2, 2, 2, 8>(a, grid, lds, stream); break;
        case 3: launch_slab_variant<256, 32, 4, 1, 2, 8>(a, grid, lds, stream); break;
    }
    return 6 + best;
}


int launch_gemm(const GemmArgs& a, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0 || a.nbatch <= 0) return -1;
    if (a.ds_out) return launch_conv2d_s2(a, stream) ? 28 : -7;      // the fused level transition is asked for explicitly (the caller probes with gemm_variant_of)
    if (a.stride == 2 && a.wout > 0 && a.ntaps == 9 && a.K == 64 && a.Wp && launch_conv2d_s2(a, stream)) return 29;
    if (a.ntaps < 1 || a.ntaps > ZVX_MAX_TAPS) return -2;
    if (a.out_split3 && (a.out_dtype != DT_F32 || a.N % 8 || a.flat_win || a.wout > 0)) return -2;
    // N not a multiple of 4: the last 4-wide store spills into [N, roundup4(N)) of the row (ldo must cover it)
    if (a.N % 4 && (a.bias_mode == 1 || a.res_mode || a.accum_mode || a.post_scale || a.ldo < ((a.N + 3) & ~3))) return -2;
    if (a.Wp && a.dtype == DT_BF16 && a.wout > 0 && a.stride == 1 && a.ntaps == 9 && a.wout == a.win && a.M == a.hin * a.win && a.nheads == 1 && a.w_bs == 0 &&
        !a.k_len && a.K % 16 == 0 && a.N % 32 == 0 && a.ldo % 8 == 0 && a.ldx == a.K && !a.res_mode && !a.accum_mode && a.bias_mode != 2 && a.win <= 271) {
        // 3 x 3 / stride 1 / pad 1 over [hin][win] maps whose LAST column is never a valid position (win = widest utterance + 1, see
        // run_spkemb): as a 9-tap 1-D convolution over the flattened map.  Columns beyond an utterance's width are masked on the
        // way into LDS, so the output's invalid columns hold finite junk that every consumer masks the same way.
        bool ok9 = true;
        for (int t = 0; t < 9; t++) ok9 = ok9 && a.du[t] == t / 3 - 1 && a.dv[t] == t % 3 - 1;
        if (ok9 && (a.N == a.K ? (a.N == 32 || a.N == 64 || (a.N % 128 == 0 && 2 * (a.win + 1) <= 160)) : false)) {
            GemmArgs f = a;
            f.flat_win = a.win; f.flat_rows = a.hin * a.win;
            for (int t = 0; t < 9; t++) { f.dv[t] = a.du[t] * a.win + a.dv[t]; f.du[t] = 0; }
            f.wout = 0; f.out_len = nullptr;               // every row of the flattened map is written
            const int id = launch_convslab(f, stream);
            if (id >= 0) return id;
        }
    }
    if (a.Wp && a.dtype != DT_F32 && a.wout <= 0 && a.nheads == 1 && a.w_bs == 0 && !a.k_len && a.K % 16 == 0 && a.N % 8 == 0 && a.ldo % 8 == 0) {
        int lo = 0, hi = 0;
        for (int i = 0; i < a.ntaps; i++) { if (a.dv[i] < lo) lo = a.dv[i]; if (a.dv[i] > hi) hi = a.dv[i]; }
        if (hi - lo <= 64 && hi >= 0 && lo <= 0) return launch_convslab(a, stream);
        // a 96-row halo on the register-weight kernel only (C = 32 / 64, k = 7: HiFi-GAN V3's dilation-12 convolutions)
        // (... and the 256 x 128 tile's 160-row variant for C = 128)
        if (hi - lo <= 96 && hi >= 0 && lo <= 0 && a.ntaps == 7 && a.N == a.K && (a.N == 32 || a.N == 64 || a.N == 128) && !a.K2 && !a.out_split3 && !a.bflat) {
            const int id = launch_convslab(a, stream);
            if (id >= 0) return id;
        }
    }
    if (a.out_split3 || a.K2) return -2;                        // only the conv-slab kernel writes split planes / takes a second source
    // tile choice: padded N weighted by the tile's MFMA efficiency, ties -> wider BN
    static const int bns[3] = {128, 64, 32};
    static const double eff[3] = {1.0, 0.75, 0.45};
    int best = 0; double best_cost = -1;
    for (int i = 0; i < 3; i++) {
        const double cost = (double)((a.N + bns[i] - 1) / bns[i]) * bns[i] / eff[i];
        if (best_cost < 0 || cost < best_cost - 1e-9) { best_cost = cost; best = i; }
    }
    int bn = bns[best], bm = (bn == 128) ? 128 : 256;
    int ntn = (a.N + bn - 1) / bn, ntm = (a.M + bm - 1) / bm;
    // small problems (e.g. the f32 phoneme encoder: 128 rows per utterance): a 64x64 tile fills the 256 CUs
    if ((long)ntn * ntm * a.nbatch * a.nheads < 512 && a.N >= 64) {
        bm = bn = 64; ntn = (a.N + 63) / 64; ntm = (a.M + 63) / 64;
        dim3 grid(ntn * ntm, a.nbatch * a.nheads), block(256);
        if (a.dtype == DT_BF16) { ZVX_LAUNCH((gemm_kernel<DT_BF16, 64, 64, 2, 2>), grid, block, 0, stream, a); return 18; }
        if (a.dtype == DT_F16) { ZVX_LAUNCH((gemm_kernel<DT_F16, 64, 64, 2, 2>), grid, block, 0, stream, a); return 18; }
        ZVX_LAUNCH((gemm_kernel<DT_F32, 64, 64, 2, 2>), grid, block, 0, stream, a);
        return 19;
    }
    dim3 grid(ntn * ntm, a.nbatch * a.nheads), block(256);
    const int base = (a.dtype != DT_F32) ? 0 : 3;
    const int id = base + best;
    if (a.dtype == DT_F16) {                                    // IEEE-half operands (the vocoder's odd shapes): the bf16 tilings on the f16 MFMA
        switch (id) {
            case 0: ZVX_LAUNCH((gemm_kernel<DT_F16, 128, 128, 2, 2>), grid, block, 0, stream, a); break;
            case 1: ZVX_LAUNCH((gemm_kernel<DT_F16, 256, 64, 4, 1>), grid, block, 0, stream, a); break;
            case 2: ZVX_LAUNCH((gemm_kernel<DT_F16, 256, 32, 4, 1>), grid, block, 0, stream, a); break;
        }
        return id;
    }
    switch (id) {
        case 0: ZVX_LAUNCH((gemm_kernel<DT_BF16, 128, 128, 2, 2>), grid, block, 0, stream, a); break;
        case 1: ZVX_LAUNCH((gemm_kernel<DT_BF16, 256, 64, 4, 1>), grid, block, 0, stream, a); break;
        case 2: ZVX_LAUNCH((gemm_kernel<DT_BF16, 256, 32, 4, 1>), grid, block, 0, stream, a); break;
        case 3: ZVX_LAUNCH((gemm_kernel<DT_F32, 128, 128, 2, 2>), grid, block, 0, stream, a); break;
        case 4: ZVX_LAUNCH((gemm_kernel<DT_F32, 256, 64, 4, 1>), grid, block, 0, stream, a); break;
        case 5: ZVX_LAUNCH((gemm_kernel<DT_F32, 256, 32, 4, 1>), grid, block, 0, stream, a); break;
    }
    return id;
}

int gemm_variant_of(const GemmArgs& a) {
    g_dry_run = true;
    const int id = a.fused == 2 ? launch_rb2fuse(a, nullptr) : (a.fused ? launch_resfuse(a, nullptr) : launch_gemm(a, nullptr));
    g_dry_run = false;
    return id;
}

#endif  // ZVX_PART_MAIN
}  // namespace zvx
