// ops.hip -- the HBM-bound kernels of the synthesis path (norms, softmax, gathers, pooling, conv_post).
// All tensors are time-major [row][channel]; 64-lane waves; one wave per row for row reductions,
// channel-contiguous vector loads elsewhere.
#include "zvx_kernels.h"

#include <algorithm>

namespace zvx {

__device__ __forceinline__ float ld(const void* p, int dt, long i) {
    if (dt == DT_F16) return (float)((const _Float16*)p)[i];
    return dt == DT_F32 ? ((const float*)p)[i] : __uint_as_float(((unsigned)((const unsigned short*)p)[i]) << 16);
}
__device__ __forceinline__ unsigned short tobf(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
// 8 consecutive 16-bit values (one 16-byte load) -> f32, and back; dt = DT_BF16 or DT_F16
__device__ __forceinline__ void unpack8(const uint4 t, int dt, float v[8]) {
    if (dt == DT_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 a = __builtin_bit_cast(h2, t.x), b = __builtin_bit_cast(h2, t.y), c = __builtin_bit_cast(h2, t.z), d = __builtin_bit_cast(h2, t.w);
        v[0] = (float)a.x; v[1] = (float)a.y; v[2] = (float)b.x; v[3] = (float)b.y; v[4] = (float)c.x; v[5] = (float)c.y; v[6] = (float)d.x; v[7] = (float)d.y;
    } else {
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
        v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u);
        v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
    }
}
__device__ __forceinline__ float clamp_h(float v) { return __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }   // f16 stores saturate instead of producing Inf
__device__ __forceinline__ uint4 pack8(const float v[8], int dt) {
    uint4 o;
    if (dt == DT_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        o.x = __builtin_bit_cast(unsigned, (h2){(_Float16)clamp_h(v[0]), (_Float16)clamp_h(v[1])}); o.y = __builtin_bit_cast(unsigned, (h2){(_Float16)clamp_h(v[2]), (_Float16)clamp_h(v[3])});
        o.z = __builtin_bit_cast(unsigned, (h2){(_Float16)clamp_h(v[4]), (_Float16)clamp_h(v[5])}); o.w = __builtin_bit_cast(unsigned, (h2){(_Float16)clamp_h(v[6]), (_Float16)clamp_h(v[7])});
    } else {
        o.x = (unsigned)tobf(v[0]) | ((unsigned)tobf(v[1]) << 16); o.y = (unsigned)tobf(v[2]) | ((unsigned)tobf(v[3]) << 16);
        o.z = (unsigned)tobf(v[4]) | ((unsigned)tobf(v[5]) << 16); o.w = (unsigned)tobf(v[6]) | ((unsigned)tobf(v[7]) << 16);
    }
    return o;
}
__device__ __forceinline__ void st(void* p, int dt, long i, float v) {
    if (dt == DT_F16) { ((_Float16*)p)[i] = (_Float16)clamp_h(v); return; }
    if (dt == DT_F32) ((float*)p)[i] = v; else ((unsigned short*)p)[i] = tobf(v);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float act_apply(float v, int act, float slope) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_LRELU) return v >= 0.f ? v : v * slope;
    if (act == ACT_TANH) return tanhf(v);
    return v;
}

// ---------------------------------------------------------------- casts
__global__ void k_cast(const void* in, int idt, void* out, int odt, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) st(out, odt, i, ld(in, idt, i));
}
void launch_cast(const void* in, int in_dt, void* out, int out_dt, size_t n, hipStream_t s) {
    if (!n) return;
    int blocks = (int)((n + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_cast, dim3(blocks), dim3(256), 0, s, in, in_dt, out, out_dt, n);
}
// ---------------------------------------------------------------- 16-bit transpose  [b][rows][ld_in] -> [b][C][ld_out]
__global__ __launch_bounds__(256) void k_transpose16(const unsigned short* in, int ld_in, unsigned short* out, int ld_out, int rows_max, int C, const int* len) {
    __shared__ unsigned short tile[64][66];
    const int b = blockIdx.z, r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    // rows past the utterance's own length are never written by the producing GEMM (it masks by out_len): they read as zeros here,
    // whatever an earlier call (or another precision's use of the shared buffer) left there -- 0 * stale NaN = NaN in P.V otherwise
    const int rows = len ? min(len[b], rows_max) : rows_max;
    const unsigned short* ip = in + (long)b * rows_max * ld_in;
    unsigned short* op = out + (long)b * C * ld_out;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        tile[r][c] = (r0 + r < rows && c0 + c < C) ? ip[(long)(r0 + r) * ld_in + c0 + c] : (unsigned short)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < C && r0 + r < ld_out) op[(long)(c0 + c) * ld_out + r0 + r] = (r0 + r < rows) ? tile[r][c] : (unsigned short)0;
    }
}
void launch_transpose16(const void* in, int ld_in, void* out, int ld_out, int B, int rows, int C, hipStream_t s, const int* len) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_transpose16, dim3((C + 63) / 64, (ld_out + 63) / 64, B), dim3(256), 0, s, (const unsigned short*)in, ld_in, (unsigned short*)out, ld_out, rows, C, len);
}

void launch_f32_to_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s) { launch_cast(in, DT_F32, out, DT_BF16, n, s); }

// ---------------------------------------------------------------- 16-bit split planes of an f32 tensor
// f32-class GEMMs on the 16-bit MFMA: x = hi + lo, w = wh + wl, and
//     x.w ~= hi.wh + hi.wl + lo.wh
// is ONE 16-bit GEMM over a K axis of three planes: activations [hi | hi | lo] against weights [wh | wl | wh], accumulated in
// f32 by the MFMA.  k_split3 writes the activation planes (rows past an utterance's length as zeros), k_split3_w the weights.
//   bf16 planes (f16 = 0, the round-2/3 path, kept as an A/B): 8-bit significands, hi + lo carries 16 bits, the dropped lo.wl
//     term is 2^-18 relative -- 5e-5 on the encoder output.
//   IEEE-half planes (f16 = 1, default): 11-bit significands, hi + lo carries 22 bits + sign (2^-24 relative: an f32 half-ulp),
//     the dropped term is 2^-24.  Half has 5 exponent bits, so the planes are SCALED by powers of two to stay normal:
//       activations [xh | xh | xl * 2^11]           (xl = x - xh is 2^-12 |x| at most; x itself sits behind a LayerNorm)
//       weights     [wh | wl | w * 2^-11] * 2^s     (s per tensor: max |w| 2^s in [2^14, 2^15); the epilogue multiplies by 2^-s)
//     every product pair shares the scale 2^s: xh.wh, xh.wl, (xl 2^11).(w 2^(s-11)).
__device__ __forceinline__ void split2(float v, unsigned short& hi, unsigned short& lo) {
    hi = tobf(v);
    lo = tobf(v - __uint_as_float(((unsigned)hi) << 16));
}
__device__ __forceinline__ void split2h(float v, unsigned short& hi, unsigned short& lo) {
    const _Float16 h = (_Float16)clamp_h(v);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, (_Float16)clamp_h((v - (float)h) * 2048.f));
}
__device__ __forceinline__ void split2x(float v, int f16, unsigned short& hi, unsigned short& lo) { if (f16) split2h(v, hi, lo); else split2(v, hi, lo); }
__global__ __launch_bounds__(256) void k_split3(const float* x, int ldx, unsigned short* out, int rows_max, const int* rows, int C, int f16) {
    const int b = blockIdx.y, r = blockIdx.x;
    const bool live = r < (rows ? rows[b] : rows_max);
    const float* xr = x + ((long)b * rows_max + r) * ldx;
    unsigned short* o = out + ((long)b * rows_max + r) * 3 * C;
    for (int c = threadIdx.x * 4; c < C; c += blockDim.x * 4) {                 // C % 4 == 0
        unsigned short h[4], l[4];
        if (live) { const float4 v = *(const float4*)(xr + c); split2x(v.x, f16, h[0], l[0]); split2x(v.y, f16, h[1], l[1]); split2x(v.z, f16, h[2], l[2]); split2x(v.w, f16, h[3], l[3]); }
        else { for (int e = 0; e < 4; e++) h[e] = l[e] = 0; }
        const uint2 hv = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        const uint2 lv = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
        *(uint2*)(o + c) = hv; *(uint2*)(o + C + c) = hv; *(uint2*)(o + 2 * C + c) = lv;
    }
}
void launch_split3(const float* x, int ldx, void* out, int B, int rows_max, const int* rows, int C, hipStream_t s, int f16) {
    if (rows_max <= 0) return;
    hipLaunchKernelGGL(k_split3, dim3(rows_max, B), dim3(C >= 1024 ? 256 : 128), 0, s, x, ldx, (unsigned short*)out, rows_max, rows, C, f16);
}
__global__ void k_split3_w(const float* w, unsigned short* out, long nrows, int K, int f16, float scale) {
    const long r = blockIdx.x;
    if (r >= nrows) return;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        unsigned short h, l, h3;
        if (f16) {
            const float v = w[r * K + k] * scale;                                // scale = 2^s: exact
            const _Float16 wh = (_Float16)clamp_h(v);
            h = __builtin_bit_cast(unsigned short, wh);
            l = __builtin_bit_cast(unsigned short, (_Float16)(v - (float)wh));
            h3 = __builtin_bit_cast(unsigned short, (_Float16)clamp_h(v * (1.0f / 2048.f)));
        } else { split2(w[r * K + k], h, l); h3 = h; }
        out[r * 3 * K + k] = h; out[r * 3 * K + K + k] = l; out[r * 3 * K + 2 * K + k] = h3;
    }
}
void launch_split3_weights(const float* w, void* out, long nrows, int K, hipStream_t s, int f16, float scale) {
    hipLaunchKernelGGL(k_split3_w, dim3((unsigned)nrows), dim3(256), 0, s, w, (unsigned short*)out, nrows, K, f16, scale);
}
// max |x| over n floats (load-time: the per-tensor scale of the half-precision weight planes); out must be zeroed
__global__ void k_absmax(const float* x, size_t n, unsigned* out) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));           // non-negative floats order like their bit patterns
}
void launch_absmax(const float* x, size_t n, float* out, hipStream_t s) {
    (void)hipMemsetAsync(out, 0, 4, s);
    if (!n) return;
    int blocks = (int)((n + 255) / 256); if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_absmax, dim3(blocks), dim3(256), 0, s, x, n, (unsigned*)out);
}

// ---------------------------------------------------------------- embedding + positional encoding
__global__ void k_embed(const int* ph, const int* pu, const float* emb, int ed, const float* pemb, int pd,
                        const float* pe, float* out, int Tmax, const int* T) {
    const int b = blockIdx.y, t = blockIdx.x;
    if (t >= T[b]) return;
    const int H = ed + pd;
    const int p = ph[b * Tmax + t], q = pu[b * Tmax + t];
    float* o = out + ((long)b * Tmax + t) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        float v = c < ed ? emb[(long)p * ed + c] : pemb[(long)q * pd + (c - ed)];
        o[c] = v + pe[(long)t * H + c];
    }
}
void launch_embed(const int* phoneme, const int* puncts, const float* emb, int emb_dim, const float* pemb,
                  int pemb_dim, const float* pe, float* out, int B, int Tmax, const int* T, hipStream_t s) {
    hipLaunchKernelGGL(k_embed, dim3(Tmax, B), dim3(128), 0, s, phoneme, puncts, emb, emb_dim, pemb, pemb_dim, pe, out, Tmax, T);
}

// ---------------------------------------------------------------- LayerNorm / SCLN, one wave per row
__global__ void k_layernorm(const void* x, int xdt, int ldx, void* y, int ydt, int ldy, int rows_max, const int* rows,
                            int C, int mode, float eps, const float* gamma, const float* beta, const float* bg,
                            long bg_bs, const float* post_add, unsigned short* planes, int planes_f16) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int nr = rows ? rows[b] : rows_max;
    if (r >= nr) {
        // planes: the [hi | hi | lo] 16-bit split of the result for the next split-product GEMM (what k_split3 would write), zeros past the utterance
        if (planes && r < rows_max) { unsigned short* o = planes + ((long)b * rows_max + r) * 3 * C; for (int c = lane; c < 3 * C; c += 64) o[c] = 0; }
        return;
    }
    const long xo = ((long)b * rows_max + r) * ldx, yo = ((long)b * rows_max + r) * ldy;
    if ((C & 7) == 0 && C <= 1024 && (ldx & 7) == 0 && (ldy & 7) == 0) {
        // (round 6: every output form takes this path -- the phoneme encoder's f32 rows + 16-bit split planes and the variance predictors' f32 rows too)
        // 16-bit output rows (the FFT-block decoder's 12 LayerNorm / SCLN passes per call, f32 or 16-bit in): the row is read ONCE, as
        // 16-byte vectors (8 elements per lane and round, one or two rounds), and stays in registers for the mean, the centred second
        // moment and the affine -- the element-wise form below reads it three times, element by element: 52 us for 28672 x 528 (1.7 TB/s)
        float v[2][8];
        bool has[2];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = (lane + 64 * i) * 8;
            has[i] = c < C;
            if (has[i] && xdt == DT_F32) {
                const float4 t0 = *(const float4*)((const float*)x + xo + c), t1 = *(const float4*)((const float*)x + xo + c + 4);
                v[i][0] = t0.x; v[i][1] = t0.y; v[i][2] = t0.z; v[i][3] = t0.w; v[i][4] = t1.x; v[i][5] = t1.y; v[i][6] = t1.z; v[i][7] = t1.w;
            } else if (has[i]) unpack8(*(const uint4*)((const unsigned short*)x + xo + c), xdt, v[i]);
            else { for (int e = 0; e < 8; e++) v[i][e] = 0.f; }
#pragma unroll
            for (int e = 0; e < 8; e++) s += v[i][e];
        }
        const float mu = wave_sum(s) / C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 8; e++) { const float d = has[i] ? v[i][e] - mu : 0.f; q += d * d; }
        q = wave_sum(q);
        const float inv = mode == 0 ? 1.0f / sqrtf(q / C + eps) : 1.0f / (sqrtf(q / (C - 1)) + eps);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (!has[i]) continue;
            const int c = (lane + 64 * i) * 8;
            const float* gp = mode == 0 ? gamma + c : bg + (long)b * bg_bs + C + c;
            const float* bp = mode == 0 ? beta + c : bg + (long)b * bg_bs + c;
            const float4 g0 = *(const float4*)gp, g1 = *(const float4*)(gp + 4), b0 = *(const float4*)bp, b1 = *(const float4*)(bp + 4);
            const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, be[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = (v[i][e] - mu) * inv * g[e] + be[e];
            if (post_add) {
                const float4 p0 = *(const float4*)(post_add + (long)b * C + c), p1 = *(const float4*)(post_add + (long)b * C + c + 4);
                o[0] += p0.x; o[1] += p0.y; o[2] += p0.z; o[3] += p0.w; o[4] += p1.x; o[5] += p1.y; o[6] += p1.z; o[7] += p1.w;
            }
            if (ydt != DT_F32) *(uint4*)((unsigned short*)y + yo + c) = pack8(o, ydt);
            else {
                *(float4*)((float*)y + yo + c) = make_float4(o[0], o[1], o[2], o[3]);
                *(float4*)((float*)y + yo + c + 4) = make_float4(o[4], o[5], o[6], o[7]);
            }
            if (planes) {                                    // [hi | hi | lo] of the result: the next split-product GEMM's operand (what k_split3 would write)
                unsigned short hh[8], ll[8];
#pragma unroll
                for (int e = 0; e < 8; e++) split2x(o[e], planes_f16, hh[e], ll[e]);
                const uint4 hv = make_uint4(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16), hh[4] | ((unsigned)hh[5] << 16), hh[6] | ((unsigned)hh[7] << 16));
                const uint4 lv = make_uint4(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16), ll[4] | ((unsigned)ll[5] << 16), ll[6] | ((unsigned)ll[7] << 16));
                unsigned short* po = planes + ((long)b * rows_max + r) * 3 * C + c;
                *(uint4*)po = hv; *(uint4*)(po + C) = hv; *(uint4*)(po + 2 * C) = lv;
            }
        }
        return;
    }
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += ld(x, xdt, xo + c);
    const float mu = wave_sum(s) / C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { float d = ld(x, xdt, xo + c) - mu; q += d * d; }
    q = wave_sum(q);
    float inv;
    if (mode == 0) inv = 1.0f / sqrtf(q / C + eps);            // torch LayerNorm: biased var, eps inside sqrt
    else inv = 1.0f / (sqrtf(q / (C - 1)) + eps);              // SCLN: unbiased std, (sigma + eps)  fs2.py:79-81
    for (int c = lane; c < C; c += 64) {
        float g, be;
        if (mode == 0) { g = gamma[c]; be = beta[c]; }
        else { be = bg[(long)b * bg_bs + c]; g = bg[(long)b * bg_bs + C + c]; }   // b = first half (fs2.py:85)
        float v = (ld(x, xdt, xo + c) - mu) * inv * g + be;
        if (post_add) v += post_add[(long)b * C + c];
        st(y, ydt, yo + c, v);
        if (planes) {
            unsigned short hi, lo;
            split2x(v, planes_f16, hi, lo);
            unsigned short* o = planes + ((long)b * rows_max + r) * 3 * C;
            o[c] = hi; o[C + c] = hi; o[2 * C + c] = lo;
        }
    }
}
void launch_layernorm(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int rows_max,
                      const int* rows, int C, int mode, float eps, const float* gamma, const float* beta,
                      const float* bg, long bg_bs, const float* post_add, hipStream_t s, void* split_planes, int planes_f16) {
    hipLaunchKernelGGL(k_layernorm, dim3((rows_max + 3) / 4, B), dim3(256), 0, s, x, x_dt, ldx, y, y_dt, ldy, rows_max,
                       rows, C, mode, eps, gamma, beta, bg, bg_bs, post_add, (unsigned short*)split_planes, planes_f16);
}

// ---------------------------------------------------------------- row softmax with key-length mask
__global__ void k_softmax_rows(const float* sc, int lds, void* P, int pdt, int ldp, int nheads, int Lmax, const int* len) {
    const int z = blockIdx.y, b = z / nheads;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int L = len[b];
    if (r >= L) return;
    const float* row = sc + ((long)z * Lmax + r) * lds;
    const long po = ((long)z * Lmax + r) * ldp;
    float m = -INFINITY;
    for (int c = lane; c < L; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < L; c += 64) s += expf(row[c] - m);
    s = wave_sum(s);
    const float inv = 1.0f / s;
    const int Lp = (L + 7) & ~7;
    for (int c = lane; c < Lp; c += 64) st(P, pdt, po + c, c < L ? expf(row[c] - m) * inv : 0.f);
}
void launch_softmax_rows(const float* scores, int lds, void* P, int p_dt, int ldp, int nbatch, int nheads,
                         int Lmax, const int* len, hipStream_t s) {
    hipLaunchKernelGGL(k_softmax_rows, dim3((Lmax + 3) / 4, nbatch * nheads), dim3(256), 0, s, scores, lds, P, p_dt, ldp, nheads, Lmax, len);
}

// ---------------------------------------------------------------- row dot (variance predictor head)
__global__ void k_rowdot(const float* x, int ldx, const float* w, float bias, float* out, int Tmax, const int* T, int C) {
    const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T[b]) return;
    const float* row = x + ((long)b * Tmax + t) * ldx;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += row[c] * w[c];
    s = wave_sum(s);
    if (lane == 0) out[b * Tmax + t] = s + bias;
}
void launch_rowdot(const float* x, int ldx, const float* w, float bias, float* out, int B, int Tmax,
                   const int* T, int C, hipStream_t s) {
    hipLaunchKernelGGL(k_rowdot, dim3((Tmax + 3) / 4, B), dim3(256), 0, s, x, ldx, w, bias, out, Tmax, T, C);
}

// ---------------------------------------------------------------- bucketise + embedding add
__global__ void k_bucket_embed_add(const float* pred, const float* table, int nb, float* x, int ldx, int C, int* idx_out,
                                   int Tmax, const int* T) {
    const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T[b]) return;
    float p = rintf(pred[b * Tmax + t] * (float)(nb - 1));        // torch.round: half-to-even
    p = fminf(fmaxf(p, 0.f), (float)(nb - 1));
    const int idx = (int)p;
    if (lane == 0 && idx_out) idx_out[b * Tmax + t] = idx;
    float* row = x + ((long)b * Tmax + t) * ldx;
    for (int c = lane; c < C; c += 64) row[c] += table[(long)idx * C + c];
}
void launch_bucket_embed_add(const float* pred, const float* table, int nbins, float* x, int ldx, int C,
                             int* idx_out, int B, int Tmax, const int* T, hipStream_t s) {
    hipLaunchKernelGGL(k_bucket_embed_add, dim3((Tmax + 3) / 4, B), dim3(256), 0, s, pred, table, nbins, x, ldx, C, idx_out, Tmax, T);
}

// ---------------------------------------------------------------- prosody control: controlled bucketise + embedding add
// The launch geometry of k_bucket_embed_add (4 phonemes per workgroup).  With a range, wave 0 of every workgroup first forms the
// utterance mean of the predictions (f64 accumulation in a fixed order, rounded once to f32: every workgroup of the utterance gets
// the same value; T_b floats, a few hundred bytes from cache) -- one pass instead of a mean pass and a [B] buffer.
// Each wave then controls its row: v = (p + (range - 1) * (p - m)) + shift, replaced by a non-NaN target, bucketised as above.
// Each operation is its own rounded f32 op (no contraction), so range 1 / shift 0 gives back p bit for bit (include/zvx.h).
__global__ void k_bucket_embed_add_ctl(const float* pred, const float* shift, const float* range, const float* target,
                                       const float* table, int nb, float* x, int ldx, int C, int* idx_out, int Tmax, const int* T) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = T[b];
    const float* pb = pred + (long)b * Tmax;
    if (blockIdx.x * 4 >= n) return;                            // (whole workgroup: no barrier is skipped by only some waves)
    __shared__ float mean_s;
    if (range) {
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int u = lane; u < n; u += 64) s += (double)pb[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) mean_s = (float)(s / (double)n);
        }
        __syncthreads();
    }
    if (t >= n) return;
    const float r1 = range ? range[b] - 1.0f : 0.f, sh = shift ? shift[b] : 0.f;
    float v = pb[t];
    if (range) v = v + r1 * (v - mean_s);
    if (shift) v = v + sh;
    if (target) { const float g = target[(long)b * Tmax + t]; if (g == g) v = g; }
    float p = rintf(v * (float)(nb - 1));
    p = fminf(fmaxf(p, 0.f), (float)(nb - 1));
    const int idx = (int)p;
    if (lane == 0 && idx_out) idx_out[b * Tmax + t] = idx;
    float* row = x + ((long)b * Tmax + t) * ldx;
    for (int c = lane; c < C; c += 64) row[c] += table[(long)idx * C + c];
}
void launch_bucket_embed_add_ctl(const float* pred, const float* shift, const float* range, const float* target, const float* table,
                                 int nbins, float* x, int ldx, int C, int* idx_out, int B, int Tmax, const int* T, hipStream_t s) {
    hipLaunchKernelGGL(k_bucket_embed_add_ctl, dim3((Tmax + 3) / 4, B), dim3(256), 0, s, pred, shift, range, target, table, nbins, x, ldx, C, idx_out, Tmax, T);
}

// ---------------------------------------------------------------- durations + inclusive scan (one wave / utterance)
__global__ void k_durations(const int* forced, const float* logd, int* dur, int* cum, int* mel_len, int Tmax, const int* T) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = T[b];
    long long carry = 0;                                        // 64-bit: the sum saturates instead of wrapping
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        int d = 0;
        if (t < n) {
            if (forced) d = min(max(forced[b * Tmax + t], 0), 65536);                     // fs2.py:452 max(int(d),0)
            else d = (int)fminf(fmaxf(rintf(expf(logd[b * Tmax + t]) - 1.0f), 0.f), 65536.f);   // fs2.py:678-681; NaN -> 0; the upper
                                                                     // clamp only keeps the int conversion and the prefix sum defined
            dur[b * Tmax + t] = d;
        }
        int v = d;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
        if (t < n) cum[b * Tmax + t] = (int)min(carry + v, 0x7fffffffLL);
        carry += __shfl(v, 63, 64);
    }
    if (lane == 0) mel_len[b] = (int)min(carry, 0x7fffffffLL);
}
void launch_durations(const int* forced, const float* logd, int* dur, int* cum, int* mel_len, int B, int Tmax,
                      const int* T, hipStream_t s) {
    hipLaunchKernelGGL(k_durations, dim3(B), dim3(64), 0, s, forced, logd, dur, cum, mel_len, Tmax, T);
}

// Same durations scaled by per-phoneme Q16 factors q (65536 = 1): P_t = sum_{u<=t} d_u q_u (int64 wave scan), C_t = (P_t + 2^15) >> 16,
// dur = C_t - C_{t-1}, cum = C_t (saturated to int32), mel_len = C_{T-1}.  Rounding the running sum keeps the total within half a frame.
__global__ void k_durations_q16(const int* forced, const float* logd, const int* q, int* dur, int* cum, int* mel_len, int Tmax, const int* T) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = T[b];
    long long carry = 0;                                        // P of the previous chunk's last phoneme
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        long long wgt = 0;
        if (t < n) {
            int d;
            if (forced) d = min(max(forced[b * Tmax + t], 0), 65536);
            else d = (int)fminf(fmaxf(rintf(expf(logd[b * Tmax + t]) - 1.0f), 0.f), 65536.f);
            wgt = (long long)d * q[b * Tmax + t];
        }
        long long v = wgt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { long long u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
        if (t < n) {
            const long long P = carry + v;
            const long long Cn = (P + 32768) >> 16, Cp = (P - wgt + 32768) >> 16;
            dur[b * Tmax + t] = (int)(Cn - Cp);
            cum[b * Tmax + t] = (int)min(Cn, 0x7fffffffLL);
        }
        carry += __shfl(v, 63, 64);
    }
    if (lane == 0) mel_len[b] = (int)min((carry + 32768) >> 16, 0x7fffffffLL);
}
void launch_durations_q16(const int* forced, const float* logd, const int* q, int* dur, int* cum, int* mel_len, int B, int Tmax,
                          const int* T, hipStream_t s) {
    hipLaunchKernelGGL(k_durations_q16, dim3(B), dim3(64), 0, s, forced, logd, q, dur, cum, mel_len, Tmax, T);
}

// ---------------------------------------------------------------- length regulator: scan-indexed coalesced row gather
__global__ void k_length_regulate(const float* x, int ldx, const int* cum, const int* T, const int* mel_len, float* feats,
                                  int Tmax, int Lmax, int C) {
    const int b = blockIdx.y, l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= mel_len[b]) return;
    const int* cb = cum + b * Tmax;
    int lo = 0, hi = T[b] - 1;                 // first t with cum[t] > l
    while (lo < hi) { int mid = (lo + hi) >> 1; if (cb[mid] > l) hi = mid; else lo = mid + 1; }
    const float4* src = (const float4*)(x + ((long)b * Tmax + lo) * ldx);
    float4* dst = (float4*)(feats + ((long)b * Lmax + l) * C);
    for (int c = lane; c < C / 4; c += 64) dst[c] = src[c];
}
void launch_length_regulate(const float* x, int ldx, const int* cum, const int* T, const int* mel_len,
                            float* feats, int B, int Tmax, int Lmax, int C, hipStream_t s) {
    if (Lmax <= 0) return;
    hipLaunchKernelGGL(k_length_regulate, dim3((Lmax + 3) / 4, B), dim3(256), 0, s, x, ldx, cum, T, mel_len, feats, Tmax, Lmax, C);
}

__global__ void k_add_pe_cast(const float* x, const float* pe, void* y, int ydt, int ldy, int Lmax, const int* L, int C, int out_rows) {
    const int b = blockIdx.y, l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= L[b]) return;
    const float* row = x + ((long)b * Lmax + l) * C;
    const long yo = ((long)b * out_rows + l) * ldy;
    for (int c = lane; c < C; c += 64) st(y, ydt, yo + c, row[c] + (pe ? pe[(long)l * C + c] : 0.f));
}
void launch_add_pe_cast(const float* x, const float* pe, void* y, int y_dt, int ldy, int B, int Lmax,
                        const int* L, int C, hipStream_t s, int out_rows_max) {
    if (Lmax <= 0) return;
    hipLaunchKernelGGL(k_add_pe_cast, dim3((Lmax + 3) / 4, B), dim3(256), 0, s, x, pe, y, y_dt, ldy, Lmax, L, C, out_rows_max > 0 ? out_rows_max : Lmax);
}

// ---------------------------------------------------------------- per-(utterance, channel) statistics over valid rows
// x [b][H*Wmax][ldx]; row r valid iff (r % Wmax) < W[b].  Block = 32 row-groups x 8 lanes, each lane owns 8
// consecutive channels (one 16-byte load per row for bf16); single pass with a per-channel shift (the first
// valid row) so that sum / sum-of-squares do not cancel; LDS tree over the row-groups.
__global__ __launch_bounds__(256) void k_colstats(const void* x, int xdt, int ldx, int H, int Wmax, const int* W, int C, float eps,
                                                  float* mean, float* rstd) {
    __shared__ float red[2][32][65];
    const int b = blockIdx.y, cl = (threadIdx.x & 7) * 8, c0 = blockIdx.x * 64 + cl, g = threadIdx.x >> 3;
    const int Wb = W[b];
    const long base = (long)b * H * Wmax * ldx;
    float s1[8], s2[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; e++) { s1[e] = 0.f; s2[e] = 0.f; sh[e] = 0.f; }
    const bool cok = c0 < C;                                  // C % 8 == 0 for every caller
    auto load8 = [&](long off, float v[8]) {
        if (xdt != DT_F32) {
            unpack8(*(const uint4*)((const unsigned short*)x + off), xdt, v);
        } else {
            const float4 t0 = *(const float4*)((const float*)x + off), t1 = *(const float4*)((const float*)x + off + 4);
            v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
        }
    };
    if (cok && Wb > 0) load8(base + c0, sh);                  // shift = row 0 of this utterance (valid: Wb > 0)
    if (cok && xdt != DT_F32) {
        // four rows of the thread in flight per iteration (same rows, same order of accumulation as the plain loop below); a single
        // request would otherwise pay one memory round trip per row of its chain (14 for a 448-frame utterance)
        const unsigned short* xp = (const unsigned short*)x + base + c0;
        for (int hh = 0; hh < H; hh++)
            for (int w = g; w < Wb; w += 128) {
                uint4 t[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int wu = w + 32 * u < Wb ? w + 32 * u : w; t[u] = *(const uint4*)(xp + ((long)hh * Wmax + wu) * ldx); }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (w + 32 * u >= Wb) break;
                    float v[8];
                    unpack8(t[u], xdt, v);
#pragma unroll
                    for (int e = 0; e < 8; e++) { const float d = v[e] - sh[e]; s1[e] += d; s2[e] += d * d; }
                }
            }
    } else if (cok)
        for (int hh = 0; hh < H; hh++)
            for (int w = g; w < Wb; w += 32) {
                float v[8];
                load8(base + ((long)hh * Wmax + w) * ldx + c0, v);
#pragma unroll
                for (int e = 0; e < 8; e++) { const float d = v[e] - sh[e]; s1[e] += d; s2[e] += d * d; }
            }
#pragma unroll
    for (int e = 0; e < 8; e++) { red[0][g][cl + e] = s1[e]; red[1][g][cl + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        float a1 = 0.f, a2 = 0.f;
        for (int i = 0; i < 32; i++) { a1 += red[0][i][threadIdx.x]; a2 += red[1][i][threadIdx.x]; }
        if (c < C) {
            const float cnt = (float)H * (float)Wb;
            const float shift = ld(x, xdt, base + c);
            const float m1 = a1 / cnt;
            mean[(long)b * C + c] = shift + m1;
            if (rstd) rstd[(long)b * C + c] = 1.0f / sqrtf(fmaxf(a2 / cnt - m1 * m1, 0.f) + eps);   // biased var (InstanceNorm1d)
        }
    }
}
// Single requests: statistics AND normalise-affine-activation of a 16-bit [L][C] tensor in one launch (one workgroup per
// (utterance, 64 channels): the same 32 row groups x 8 lanes as k_colstats, then the same threads walk the rows again).  Saves the
// second launch (~12 us of a ~25 us pair at batch 1); bit-identical to k_colstats + k_norm_affine_act (same accumulation order, same
// scale / shift expressions).  Larger batches keep the two kernels: the apply pass wants more workgroups than 17 per utterance.
__global__ __launch_bounds__(256) void k_instnorm_fused(const void* x, int xdt, int ldx, void* y, int ydt, int ldy, int Lmax, const int* L, int C, float eps,
                                                        float* mean, float* rstd, const float* gamma, const float* beta, long g_bs, int one_plus,
                                                        int act, float slope) {
    __shared__ float red[2][32][65];
    __shared__ float stat[2][64];
    const int b = blockIdx.y, cl = (threadIdx.x & 7) * 8, c0 = blockIdx.x * 64 + cl, g = threadIdx.x >> 3;
    const int Wb = L[b];
    const long base = (long)b * Lmax * ldx;
    float s1[8], s2[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; e++) { s1[e] = 0.f; s2[e] = 0.f; sh[e] = 0.f; }
    const bool cok = c0 < C;
    const unsigned short* xp = (const unsigned short*)x + base + c0;
    if (cok && Wb > 0) unpack8(*(const uint4*)xp, xdt, sh);
    if (cok)
        for (int w = g; w < Wb; w += 128) {
            uint4 t[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int wu = w + 32 * u < Wb ? w + 32 * u : w; t[u] = *(const uint4*)(xp + (long)wu * ldx); }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (w + 32 * u >= Wb) break;
                float v[8];
                unpack8(t[u], xdt, v);
#pragma unroll
                for (int e = 0; e < 8; e++) { const float d = v[e] - sh[e]; s1[e] += d; s2[e] += d * d; }
            }
        }
#pragma unroll
    for (int e = 0; e < 8; e++) { red[0][g][cl + e] = s1[e]; red[1][g][cl + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        float a1 = 0.f, a2 = 0.f;
        for (int i = 0; i < 32; i++) { a1 += red[0][i][threadIdx.x]; a2 += red[1][i][threadIdx.x]; }
        float m = 0.f, r = 0.f;
        if (c < C) {
            const float cnt = (float)Wb;
            const float shift = ld(x, xdt, base + c);
            const float m1 = a1 / cnt;
            m = shift + m1;
            r = 1.0f / sqrtf(fmaxf(a2 / cnt - m1 * m1, 0.f) + eps);
            mean[(long)b * C + c] = m; rstd[(long)b * C + c] = r;
        }
        stat[0][threadIdx.x] = m; stat[1][threadIdx.x] = r;
    }
    __syncthreads();
    if (!cok) return;
    float sc[8], sf[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float m = stat[0][cl + e], r = stat[1][cl + e];
        float gg = 1.f, be = 0.f;
        if (gamma) { gg = (one_plus ? 1.f : 0.f) + gamma[b * g_bs + c0 + e]; be = beta[b * g_bs + c0 + e]; }
        sc[e] = r * gg; sf[e] = be - m * r * gg;                // (x - m) * r * g + be
    }
    unsigned short* yp = (unsigned short*)y + (long)b * Lmax * ldy + c0;
    for (int w = g; w < Wb; w += 128) {
        uint4 t[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int wu = w + 32 * u < Wb ? w + 32 * u : w; t[u] = *(const uint4*)(xp + (long)wu * ldx); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (w + 32 * u >= Wb) break;
            float v[8];
            unpack8(t[u], xdt, v);
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = act_apply(v[e] * sc[e] + sf[e], act, slope);
            *(uint4*)(yp + (long)(w + 32 * u) * ldy) = pack8(v, ydt);
        }
    }
}
void launch_instnorm_fused(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax, const int* L, int C, float eps,
                           float* mean, float* rstd, const float* gamma, const float* beta, long g_bs, int one_plus, int act, float slope, hipStream_t s) {
    if (Lmax <= 0) return;
    hipLaunchKernelGGL(k_instnorm_fused, dim3((C + 63) / 64, B), dim3(256), 0, s, x, x_dt, ldx, y, y_dt, ldy, Lmax, L, C, eps, mean, rstd, gamma, beta,
                       g_bs, one_plus, act, slope);
}
void launch_instnorm_stats(const void* x, int x_dt, int ldx, int B, int Lmax, const int* L, int C, float eps,
                           float* mean, float* rstd, hipStream_t s) {
    hipLaunchKernelGGL(k_colstats, dim3((C + 63) / 64, B), dim3(256), 0, s, x, x_dt, ldx, 1, Lmax, L, C, eps, mean, rstd);
}
// SE global average pool over an [H][Wmax][C] map (valid columns w < W[b]): the map can be 20 000+ positions of only 32
// channels, so the rows are split over S blocks per utterance; partial[b][s][c] holds each block's plain sum and
// k_se_fc folds the S partial sums in a fixed order (deterministic) before the squeeze-excite MLP.
__global__ __launch_bounds__(256) void k_se_pool_partial(const void* x, int xdt, int H, int Wmax, const int* W, int C, int rows_per_blk, float* partial) {
    __shared__ float red[256][9];
    const int b = blockIdx.y, sblk = blockIdx.x, S = gridDim.x;
    const int lpr = C >> 3, rpp = 256 / lpr;                  // lanes per row (8 channels each), rows per pass
    const int c8 = threadIdx.x % lpr, rg = threadIdx.x / lpr;
    const int Wb = W[b], total = H * Wmax;
    const long base = (long)b * total * C;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.f;
    const int r0 = sblk * rows_per_blk, r1 = min(total, r0 + rows_per_blk);
    if (rg < rpp && xdt == DT_BF16) {
        // four rows of the thread in flight per iteration (the pass is HBM-bound: one dependent 16-byte load per iteration left
        // most of the bandwidth idle), the column of a row tracked incrementally instead of one integer division per row
        const unsigned short* xp = (const unsigned short*)x + base + c8 * 8;
        int r = r0 + rg, w = r % Wmax;
        const int step_w = rpp % Wmax;
        for (; r < r1; r += 4 * rpp) {
            uint4 t[4]; bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int ru = r + u * rpp;
                ok[u] = ru < r1 && w < Wb;
                t[u] = ok[u] ? *(const uint4*)(xp + (long)ru * C) : make_uint4(0, 0, 0, 0);
                w += step_w; if (w >= Wmax) w -= Wmax;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {                                           // (same order of additions as the one-row loop: rows ascending)
                if (!ok[u]) continue;
                acc[0] += __uint_as_float(t[u].x << 16); acc[1] += __uint_as_float(t[u].x & 0xffff0000u);
                acc[2] += __uint_as_float(t[u].y << 16); acc[3] += __uint_as_float(t[u].y & 0xffff0000u);
                acc[4] += __uint_as_float(t[u].z << 16); acc[5] += __uint_as_float(t[u].z & 0xffff0000u);
                acc[6] += __uint_as_float(t[u].w << 16); acc[7] += __uint_as_float(t[u].w & 0xffff0000u);
            }
        }
    } else if (rg < rpp)
        for (int r = r0 + rg; r < r1; r += rpp) {
            if (r % Wmax >= Wb) continue;
            const long off = base + (long)r * C + c8 * 8;
            {
                const float4 t0 = *(const float4*)((const float*)x + off), t1 = *(const float4*)((const float*)x + off + 4);
                acc[0] += t0.x; acc[1] += t0.y; acc[2] += t0.z; acc[3] += t0.w; acc[4] += t1.x; acc[5] += t1.y; acc[6] += t1.z; acc[7] += t1.w;
            }
        }
#pragma unroll
    for (int e = 0; e < 8; e++) red[threadIdx.x][e] = acc[e];
    __syncthreads();
    if (threadIdx.x < C) {                                    // C <= 256
        const int cc = threadIdx.x >> 3, e = threadIdx.x & 7;
        float a = 0.f;
        for (int g = 0; g < rpp; g++) a += red[g * lpr + cc][e];
        partial[((long)b * S + sblk) * C + threadIdx.x] = a;
    }
}
int se_pool_splits(int H, int Wmax) { const int total = H * Wmax; int S = (total + 511) / 512; return S < 1 ? 1 : (S > 64 ? 64 : S); }
void launch_se_pool(const void* x, int x_dt, int B, int H, int Wmax, const int* W, int C, float* partial, hipStream_t s) {
    const int S = se_pool_splits(H, Wmax), total = H * Wmax;
    hipLaunchKernelGGL(k_se_pool_partial, dim3(S, B), dim3(256), 0, s, x, x_dt, H, Wmax, W, C, (total + S - 1) / S, partial);
}

// One wave = 64 x 8-channel vectors of a row (1 KiB of bf16); a block covers 64 rows x 512 channels, each lane keeps the
// per-(utterance, channel) scale/shift of its 8 channels in registers for all of its rows.
__global__ __launch_bounds__(256) void k_norm_affine_act(const void* x, int xdt, int ldx, void* y, int ydt, int ldy, int Lmax, const int* L, int C,
                                                         const float* mean, const float* rstd, const float* gamma, const float* beta, long g_bs,
                                                         int one_plus, int act, float slope) {
    const int b = blockIdx.z;
    const int Lb = L[b];
    const int l0 = blockIdx.y * 64;
    if (l0 >= Lb) return;
    const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
    if (c >= C) return;                                       // C % 8 == 0 for every caller
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float m = mean[(long)b * C + c + e], r = rstd[(long)b * C + c + e];
        float g = 1.f, be = 0.f;
        if (gamma) { g = (one_plus ? 1.f : 0.f) + gamma[b * g_bs + c + e]; be = beta[b * g_bs + c + e]; }
        sc[e] = r * g; sh[e] = be - m * r * g;                // (x - m) * r * g + be
    }
    const int lend = (l0 + 64 < Lb) ? l0 + 64 : Lb;
    if (xdt != DT_F32 && ydt != DT_F32) {
        // 16-bit -> 16-bit (the decoder's InstanceNorm / AdaIN passes): four rows of the wave in flight per iteration.  Neutral at batch 32
        // (the pass is bandwidth-bound there); a single request runs 16 dependent row round trips per wave otherwise.
        const unsigned short* xp = (const unsigned short*)x + (long)b * Lmax * ldx + c;
        unsigned short* yp = (unsigned short*)y + (long)b * Lmax * ldy + c;
        for (int l = l0 + (threadIdx.x >> 6); l < lend; l += 16) {
            uint4 t[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int lu = l + 4 * u < lend ? l + 4 * u : l; t[u] = *(const uint4*)(xp + (long)lu * ldx); }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (l + 4 * u >= lend) break;
                float v[8];
                unpack8(t[u], xdt, v);
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = act_apply(v[e] * sc[e] + sh[e], act, slope);
                *(uint4*)(yp + (long)(l + 4 * u) * ldy) = pack8(v, ydt);
            }
        }
        return;
    }
    for (int l = l0 + (threadIdx.x >> 6); l < lend; l += 4) {
        const long xo = ((long)b * Lmax + l) * ldx + c, yo = ((long)b * Lmax + l) * ldy + c;
        float v[8];
        if (xdt != DT_F32) {
            unpack8(*(const uint4*)((const unsigned short*)x + xo), xdt, v);
        } else {
            const float4 t0 = *(const float4*)((const float*)x + xo), t1 = *(const float4*)((const float*)x + xo + 4);
            v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = act_apply(v[e] * sc[e] + sh[e], act, slope);
        if (ydt != DT_F32) {
            *(uint4*)((unsigned short*)y + yo) = pack8(v, ydt);
        } else {
            *(float4*)((float*)y + yo) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)((float*)y + yo + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}
void launch_norm_affine_act(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax,
                            const int* L, int C, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, long g_bs, int one_plus, int act, float slope, hipStream_t s) {
    if (Lmax <= 0) return;
    hipLaunchKernelGGL(k_norm_affine_act, dim3((C / 8 + 63) / 64, (Lmax + 63) / 64, B), dim3(256), 0, s, x, x_dt, ldx, y, y_dt, ldy, Lmax,
                       L, C, mean, rstd, gamma, beta, g_bs, one_plus, act, slope);
}

// ---------------------------------------------------------------- mel -> zero-padded vocoder input
__global__ void k_mel_pad(const void* mel, int mdt, int ldm, int Lmax, const int* mel_len, void* v, int vdt, int ldv, int Pmax,
                          const int* P, int nm) {
    const int b = blockIdx.y, p = blockIdx.x;
    if (p >= P[b]) return;
    const bool real = p < mel_len[b];
    for (int c = threadIdx.x; c < nm; c += blockDim.x)
        st(v, vdt, ((long)b * Pmax + p) * ldv + c, real ? ld(mel, mdt, ((long)b * Lmax + p) * ldm + c) : 0.f);
}
void launch_mel_pad(const void* mel, int m_dt, int ldm, int Lmax, const int* mel_len, void* v, int v_dt,
                    int ldv, int Pmax, const int* P, int B, int nm, hipStream_t s) {
    hipLaunchKernelGGL(k_mel_pad, dim3(Pmax, B), dim3(128), 0, s, mel, m_dt, ldm, Lmax, mel_len, v, v_dt, ldv, Pmax, P, nm);
}

__global__ void k_copy_rows_f32(const void* src, int sdt, int lds, long s_bs, float* dst, long ldd, long d_bs, int rows_max,
                                const int* rows, int C) {
    const int b = blockIdx.y, r = blockIdx.x;
    if (r >= (rows ? rows[b] : rows_max)) return;
    for (int c = threadIdx.x; c < C; c += blockDim.x) dst[b * d_bs + r * ldd + c] = ld(src, sdt, b * s_bs + (long)r * lds + c);
}
void launch_copy_rows_f32(const void* src, int s_dt, int lds, long s_bs, float* dst, long ldd, long d_bs,
                          int B, int rows_max, const int* rows, int C, hipStream_t s) {
    if (rows_max <= 0) return;
    hipLaunchKernelGGL(k_copy_rows_f32, dim3(rows_max, B), dim3(128), 0, s, src, s_dt, lds, s_bs, dst, ldd, d_bs, rows_max, rows, C);
}

// rows [rows[b], rows_max) of x [b][rows_max][ldx] (first C columns) := 0 -- outputs handed to the caller never carry
// what an earlier, longer call left in the reused buffer
__global__ void k_zero_tail_rows(float* x, int ldx, int rows_max, const int* rows, int C) {
    const int b = blockIdx.y, r = blockIdx.x;
    if (r < rows[b]) return;
    for (int c = threadIdx.x; c < C; c += blockDim.x) x[((long)b * rows_max + r) * ldx + c] = 0.f;
}
void launch_zero_tail_rows(float* x, int ldx, int B, int rows_max, const int* rows, int C, hipStream_t s) {
    if (rows_max <= 0) return;
    hipLaunchKernelGGL(k_zero_tail_rows, dim3(rows_max, B), dim3(128), 0, s, x, ldx, rows_max, rows, C);
}

// Saturation audit of the IEEE-half mode (zvx_set_int "f16_sat_check"): every 16-bit store of that mode clamps at +-65504
// (MODE.FP16_OVFL), so a clamped result IS the bit pattern 0x7BFF / 0xFBFF.  Counts those patterns (and Inf / NaN patterns, which the
// clamp should have made impossible) in the valid rows of a stored tensor x[b][r][0:C]; one 64-bit atomic per workgroup that found any.
__global__ void k_count_sat16(const unsigned short* x, long bs, int ld, int rows_max, const int* rows, int C, unsigned long long* count) {
    const int b = blockIdx.y;
    const int nr = rows ? min(rows[b], rows_max) : rows_max;
    unsigned n = 0;
    for (int r = blockIdx.x; r < nr; r += gridDim.x) {
        const unsigned short* row = x + (long)b * bs + (long)r * ld;
        for (int c = threadIdx.x; c < C; c += blockDim.x) n += (row[c] & 0x7FFF) >= 0x7BFF;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) { const unsigned t = part[0] + part[1] + part[2] + part[3]; if (t) atomicAdd(count, (unsigned long long)t); }
}
void launch_count_sat16(const void* x, long bs, int ld, int B, int rows_max, const int* rows, int C, unsigned long long* count, hipStream_t s) {
    if (B <= 0 || rows_max <= 0 || C <= 0) return;
    hipLaunchKernelGGL(k_count_sat16, dim3(rows_max < 1024 ? rows_max : 1024, B), dim3(256), 0, s, (const unsigned short*)x, bs, ld, rows_max, rows, C, count);
}

// x[b][r][c] = 0 for len[b] <= c < cols (element size es = 2 / 4 bytes): the key-contiguous V^T of the unfused attention path, whose
// columns past an utterance's length come from rows nothing has defined (0 x NaN would not be 0 in the P.V product)
__global__ void k_zero_tail_cols(unsigned char* x, int es, long ld, long bs, int rows, int cols, const int* len) {
    const int b = blockIdx.z, r = blockIdx.y;
    const int l0 = len[b];
    for (int c = l0 + blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x) {
        unsigned char* p = x + ((long)b * bs + (long)r * ld + c) * es;
        if (es == 4) *(unsigned*)p = 0u; else *(unsigned short*)p = (unsigned short)0;
    }
}
void launch_zero_tail_cols(void* x, int es, long ld, long bs, int B, int rows, int cols, const int* len, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_zero_tail_cols, dim3(1, rows, B), dim3(256), 0, s, (unsigned char*)x, es, ld, bs, rows, cols, len);
}

// ---------------------------------------------------------------- conv_post (C -> 1) + tanh      hifigan.py:127-128
// x is the activated last stage [b][Nmax][ldx]; one thread per output sample, weights broadcast from LDS.
// conv_post (C -> 1, k taps) + tanh: a block of 256 samples stages its (256 + k - 1) input rows in LDS once (coalesced
// 16-byte loads, padded pitch) instead of every thread pulling its k rows through L1; the accumulation order per sample
// is unchanged (tap-major, then channel groups), so results are bit-identical to the direct form.
// Samples in [out_len*out_mul, Nmax) of every row are written as zeros, so the caller's row never depends on what an
// earlier call left in a reused buffer.  pcm16: the row is int16 PCM, (short)trunc(tanh(.) * 32760) (demo.py:29-35).
template <int KT, int CC>
__global__ __launch_bounds__(256) void k_conv_post_tanh(const void* x, int xdt, int ldx, long x_bs, const float* __restrict__ w, float bias, int kt, int C,
                                 void* wav, long wav_bs, int Nmax, int pcm16, const int* in_len, int len_mul, const int* out_len, int out_mul) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int es = xdt != DT_F32 ? 2 : 4, rowb = C * es, pitch = rowb + 16, half = (kt - 1) / 2, nrows = 256 + kt - 1;
    // KT, CC > 0 (HiFi-GAN: 7 taps x 32 channels, bf16): the tap / channel loops unroll and the weights are read with uniform
    // addresses straight from `w` (scalar loads, SGPR operands) instead of 56 LDS reads per sample; otherwise staged in LDS
    float* wl = (float*)(sm + (size_t)nrows * pitch);
    if (KT == 0) for (int i = threadIdx.x; i < kt * C; i += blockDim.x) wl[i] = w[i];
    const int b = blockIdx.y;
    const long n0 = (long)blockIdx.x * 256;
    const long nin = (long)in_len[b] * len_mul, nout = (long)out_len[b] * out_mul;
    auto put = [&](long n, float v) {
        if (pcm16) ((short*)wav)[b * wav_bs + n] = (short)(v * 32760.0f);      // float -> int conversion truncates (numpy astype)
        else ((float*)wav)[b * wav_bs + n] = v;
    };
    if (n0 >= nout) {                                        // whole block past the utterance's end: zero tail
        if (n0 + threadIdx.x < Nmax) put(n0 + threadIdx.x, 0.f);
        return;
    }
    const int cpr = rowb >> 4;                               // 16-byte chunks per row
    for (int i = threadIdx.x; i < nrows * cpr; i += 256) {
        const int r = i / cpr, q = i % cpr;
        const long m = n0 + r - half;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m >= 0 && m < nin) v = *(const uint4*)((const unsigned char*)x + (b * x_bs + m * ldx) * es + q * 16);
        *(uint4*)(sm + r * pitch + q * 16) = v;
    }
    __syncthreads();
    const long n = n0 + threadIdx.x;
    if (n >= nout) { if (n < Nmax) put(n, 0.f); return; }
    float acc = bias;
    if (KT > 0) {
#pragma unroll
        for (int k = 0; k < KT; k++) {
            const long m = n + k - half;
            if (m < 0 || m >= nin) continue;
            const unsigned char* row = sm + (threadIdx.x + k) * pitch;
#pragma unroll
            for (int c = 0; c < CC; c += 8) {
                const uint4 t = *(const uint4*)(row + c * 2);
                const float* ww = w + k * CC + c;
                float v[8];
                unpack8(t, xdt, v);                                            // bf16 or IEEE half (the vocoder's 16-bit dtype)
                acc += v[0] * ww[0] + v[1] * ww[1] + v[2] * ww[2] + v[3] * ww[3] + v[4] * ww[4] + v[5] * ww[5] + v[6] * ww[6] + v[7] * ww[7];
            }
        }
        put(n, tanhf(acc));
        return;
    }
    for (int k = 0; k < kt; k++) {
        const long m = n + k - half;
        if (m < 0 || m >= nin) continue;
        const unsigned char* row = sm + (threadIdx.x + k) * pitch;
        if (xdt != DT_F32) {
            for (int c = 0; c < C; c += 8) {
                const uint4 t = *(const uint4*)(row + c * 2);
                const float* ww = wl + k * C + c;
                float v[8];
                unpack8(t, xdt, v);
                acc += v[0] * ww[0] + v[1] * ww[1] + v[2] * ww[2] + v[3] * ww[3] + v[4] * ww[4] + v[5] * ww[5] + v[6] * ww[6] + v[7] * ww[7];
            }
        } else {
            for (int c = 0; c < C; c += 4) {
                const float4 t = *(const float4*)(row + c * 4);
                const float* ww = wl + k * C + c;
                acc += t.x * ww[0] + t.y * ww[1] + t.z * ww[2] + t.w * ww[3];
            }
        }
    }
    put(n, tanhf(acc));
}
void launch_conv_post_tanh(const void* x, int x_dt, int ldx, long x_bs, const float* w, float bias,
                           int ktaps, int C, void* wav, long wav_bs, int pcm16, int B, int Nmax, const int* in_len,
                           int len_mul, const int* out_len, int out_mul, hipStream_t s) {
    if (Nmax <= 0) return;
    const size_t es = x_dt != DT_F32 ? 2 : 4;
    const size_t lds = (size_t)(256 + ktaps - 1) * (C * es + 16) + (size_t)ktaps * C * sizeof(float);
    if (x_dt != DT_F32 && ktaps == 7 && C == 32)
        hipLaunchKernelGGL((k_conv_post_tanh<7, 32>), dim3((Nmax + 255) / 256, B), dim3(256), lds, s, x, x_dt, ldx, x_bs, w,
                           bias, ktaps, C, wav, wav_bs, Nmax, pcm16, in_len, len_mul, out_len, out_mul);
    else
        hipLaunchKernelGGL((k_conv_post_tanh<0, 0>), dim3((Nmax + 255) / 256, B), dim3(256), lds, s, x, x_dt, ldx, x_bs, w,
                           bias, ktaps, C, wav, wav_bs, Nmax, pcm16, in_len, len_mul, out_len, out_mul);
}

// ---------------------------------------------------------------- speaker encoder pieces
// first layer: InstanceNorm1d(F) over time folded in (mean/rstd given) + Conv2d(1->C0,3x3,p1) + ReLU + BN affine
// One workgroup = one clip x SF_TB consecutive time positions x ALL frequency rows.  The normalised input patch [F + 2][SF_TB + 2] is
// staged in LDS with COALESCED reads of the [time][F] log-mel (a row of F floats per time step); round 4's kernel gathered it with one
// thread per (f, t): consecutive lanes read 320 bytes apart, 4 useful bytes per 128-byte line, every frequency row's workgroups pulling
// the whole mel through L2 again -- ~3 GB of L2 traffic for a 21 MB input, and the launch wrote its 333 MB of output at 0.85 TB/s.
// A thread owns 8 output channels (72 weights + 24 bias / BN values in registers) of one time position and walks the frequency rows;
// a wave's store covers 16 consecutive positions x 64 bytes.  Same arithmetic order per output as before (bit-identical).
#define SF_TB 64
__global__ __launch_bounds__(256) void k_spk_front(const float* mels, int Tmax, const int* lens, int F, const float* mean, const float* rstd,
                            const float* w, const float* bias, const float* bs, const float* bt, int C0, void* out, int odt, int Wout) {
    extern __shared__ float patch[];                             // [F + 2][SF_TB + 2]: frequency rows -1 .. F, times t0 - 1 .. t0 + SF_TB
    constexpr int PW = SF_TB + 2;
    const int b = blockIdx.y, t0 = blockIdx.x * SF_TB, cpp = C0 >> 3;
    const int Tb = lens[b];
    if (t0 >= Tb) return;
    for (int i = threadIdx.x; i < (F + 2) * PW; i += blockDim.x) patch[i] = 0.f;
    __syncthreads();
    // coalesced: consecutive threads read consecutive frequencies of one time step
    for (int i = threadIdx.x; i < PW * F; i += blockDim.x) {
        const int j = i / F, ff = i - j * F, tt = t0 + j - 1;
        if (tt >= 0 && tt < Tb) patch[(ff + 1) * PW + j] = (mels[((long)b * Tmax + tt) * F + ff] - mean[b * F + ff]) * rstd[b * F + ff];
    }
    __syncthreads();
    for (int id = threadIdx.x; id < SF_TB * cpp; id += blockDim.x) {
        const int tl = id / cpp, c0 = (id - tl * cpp) * 8, t = t0 + tl;
        if (t >= Tb) continue;
        float wk[9][8], bb[8], sc[8], sh[8];
#pragma unroll
        for (int e = 0; e < 8; e++) { bb[e] = bias[c0 + e]; sc[e] = bs[c0 + e]; sh[e] = bt[c0 + e]; }
#pragma unroll
        for (int k = 0; k < 9; k++)
#pragma unroll
            for (int e = 0; e < 8; e++) wk[k][e] = w[k * C0 + c0 + e];
        float x0[3], x1[3], x2[3];                               // rows f - 1, f, f + 1 of the patch at times t - 1 .. t + 1
#pragma unroll
        for (int j = 0; j < 3; j++) { x0[j] = patch[0 * PW + tl + j]; x1[j] = patch[1 * PW + tl + j]; }
        for (int f = 0; f < F; f++) {
#pragma unroll
            for (int j = 0; j < 3; j++) x2[j] = patch[(f + 2) * PW + tl + j];
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float a = bb[e];
#pragma unroll
                for (int j = 0; j < 3; j++) a += x0[j] * wk[j][e];
#pragma unroll
                for (int j = 0; j < 3; j++) a += x1[j] * wk[3 + j][e];
#pragma unroll
                for (int j = 0; j < 3; j++) a += x2[j] * wk[6 + j][e];
                r[e] = fmaxf(a, 0.f) * sc[e] + sh[e];           // conv -> ReLU -> BN  (ResNetSE34V2.py:184-186)
            }
            const long o = (((long)b * F + f) * Wout + t) * C0 + c0;      // output map rows are Wout >= Tmax positions wide
            if (odt == DT_BF16) {
                uint4 pk;
                pk.x = tobf(r[0]) | ((unsigned)tobf(r[1]) << 16); pk.y = tobf(r[2]) | ((unsigned)tobf(r[3]) << 16);
                pk.z = tobf(r[4]) | ((unsigned)tobf(r[5]) << 16); pk.w = tobf(r[6]) | ((unsigned)tobf(r[7]) << 16);
                *(uint4*)((unsigned short*)out + o) = pk;
            } else {
                *(float4*)((float*)out + o) = make_float4(r[0], r[1], r[2], r[3]);
                *(float4*)((float*)out + o + 4) = make_float4(r[4], r[5], r[6], r[7]);
            }
#pragma unroll
            for (int j = 0; j < 3; j++) { x0[j] = x1[j]; x1[j] = x2[j]; }
        }
    }
}
void launch_spk_front(const float* mels, int Tmax, const int* lens, int F, const float* mean, const float* rstd,
                      const float* w, const float* bias, const float* bn_scale, const float* bn_shift, int C0,
                      void* out, int o_dt, int B, int Wout, hipStream_t s) {
    const size_t lds = (size_t)(F + 2) * (SF_TB + 2) * sizeof(float);                 // C0 % 8 == 0
    hipLaunchKernelGGL(k_spk_front, dim3((Tmax + SF_TB - 1) / SF_TB, B), dim3(256), lds, s, mels, Tmax, lens, F, mean, rstd, w, bias,
                       bn_scale, bn_shift, C0, out, o_dt, Wout);
}

// pool_bias (optional): the partial sums were taken BEFORE the convolution's per-channel bias (the pool fused into conv2d_persist_kernel): the
// mean over the valid positions carries it once
__global__ void k_se_fc(const float* partial, int S, int H, const int* W, const float* w1, const float* b1, const float* w2, const float* b2, int C, int Cr, float* scale,
                        const float* pool_bias) {
    extern __shared__ float hbuf[];                           // [Cr] hidden + [C] mean + [256] partial folds
    const int b = blockIdx.x;
    float* m = hbuf + Cr;
    float* red = m + C;
    const float cnt = (float)H * (float)W[b];
    // fold the S partial sums in a FIXED order (deterministic) with all 256 threads: thread (g, c) takes partials g, g + G, ... of channel
    // c (four independent loads in flight: the fused pool of the persistent convolution leaves ~200 partials per utterance, and one
    // dependent L2 round trip per partial was 60 us of a 10 us kernel), then channel c's G folds are added in order
    if (C <= (int)blockDim.x) {
        const int G = blockDim.x / C, g = threadIdx.x / C, c = threadIdx.x % C;
        if (g < G) {
            const float* pp = partial + (long)b * S * C + c;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int i = g;
            for (; i + 3 * G < S; i += 4 * G) { a0 += pp[(long)i * C]; a1 += pp[(long)(i + G) * C]; a2 += pp[(long)(i + 2 * G) * C]; a3 += pp[(long)(i + 3 * G) * C]; }
            for (; i < S; i += G) a0 += pp[(long)i * C];
            red[g * C + c] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        if (threadIdx.x < C) {
            float a = 0.f;
            for (int q = 0; q < G; q++) a += red[q * C + threadIdx.x];
            m[threadIdx.x] = a / cnt + (pool_bias ? pool_bias[threadIdx.x] : 0.f);
        }
    } else {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float a = 0.f;
            for (int i = 0; i < S; i++) a += partial[((long)b * S + i) * C + c];
            m[c] = a / cnt + (pool_bias ? pool_bias[c] : 0.f);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Cr; j += blockDim.x) {
        float a = b1[j];
        for (int c = 0; c < C; c++) a += w1[(long)j * C + c] * m[c];
        hbuf[j] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float a = b2[c];
        for (int j = 0; j < Cr; j++) a += w2[(long)c * Cr + j] * hbuf[j];
        scale[(long)b * C + c] = 1.0f / (1.0f + expf(-a));
    }
}
void launch_se_fc(const float* partial, int S, int H, const int* W, const float* w1, const float* b1, const float* w2, const float* b2, int C,
                  int Cr, float* scale, int B, hipStream_t s, const float* pool_bias) {
    hipLaunchKernelGGL(k_se_fc, dim3(B), dim3(256), (Cr + C + 256) * sizeof(float), s, partial, S, H, W, w1, b1, w2, b2, C, Cr, scale, pool_bias);
}

// y = relu(x * scale[b][c] + res): 8 channels (16 bytes of bf16) per thread, grid-stride over the map's vectors
// bf16 maps: a thread owns 8 channels (its scale factors stay in registers) of four positions PP = 256 / lpr apart; all eight loads are
// in flight before the first use, 32-bit index arithmetic, one modulo per thread (the column advances incrementally)
__global__ __launch_bounds__(256) void k_se_apply_bf16(const unsigned short* x, const unsigned short* res, unsigned short* y, const float* scale, int H, int Wmax,
                                                       const int* W, int C, int lpr_shift) {
    const int b = blockIdx.y, lpr = 1 << lpr_shift, PP = 256 >> lpr_shift;
    const int total = H * Wmax, Wb = W[b];
    const int c = (threadIdx.x & (lpr - 1)) * 8;
    const long base = (long)b * total * C + c;
    const float4 s0 = *(const float4*)(scale + (long)b * C + c), s1 = *(const float4*)(scale + (long)b * C + c + 4);
    const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    int pos = blockIdx.x * (4 * PP) + (threadIdx.x >> lpr_shift);
    int w = pos % Wmax;
    const int step_w = PP % Wmax;
    uint4 a[4], r[4]; bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int pu = pos + u * PP;
        ok[u] = pu < total && w < Wb;
        const long o = base + (long)(ok[u] ? pu : 0) * C;
        a[u] = *(const uint4*)(x + o); r[u] = *(const uint4*)(res + o);
        w += step_w; if (w >= Wmax) w -= Wmax;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (!ok[u]) continue;
        const unsigned au[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, ru[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
        unsigned short ov[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ov[2 * i] = tobf(fmaxf(__uint_as_float(au[i] << 16) * sc[2 * i] + __uint_as_float(ru[i] << 16), 0.f));
            ov[2 * i + 1] = tobf(fmaxf(__uint_as_float(au[i] & 0xffff0000u) * sc[2 * i + 1] + __uint_as_float(ru[i] & 0xffff0000u), 0.f));
        }
        uint4 out;
        out.x = ov[0] | ((unsigned)ov[1] << 16); out.y = ov[2] | ((unsigned)ov[3] << 16);
        out.z = ov[4] | ((unsigned)ov[5] << 16); out.w = ov[6] | ((unsigned)ov[7] << 16);
        *(uint4*)(y + base + (long)(pos + u * PP) * C) = out;
    }
}
__global__ __launch_bounds__(256) void k_se_apply(const void* x, const void* res, void* y, int dt, const float* scale, int H, int Wmax, const int* W, int C) {
    const int b = blockIdx.y, lpr = C >> 3;
    const long nvec = (long)H * Wmax * lpr;
    const long base = (long)b * H * Wmax * C;
    const int Wb = W[b];
    for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < nvec; v += (long)gridDim.x * blockDim.x) {
        const long pos = v / lpr; const int c = (int)(v % lpr) * 8;
        if ((int)(pos % Wmax) >= Wb) continue;
        const long o = base + pos * C + c;
        const float4 s0 = *(const float4*)(scale + (long)b * C + c), s1 = *(const float4*)(scale + (long)b * C + c + 4);
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        float xv[8], rv[8];
        if (dt == DT_BF16) {
            const uint4 a = *(const uint4*)((const unsigned short*)x + o), r = *(const uint4*)((const unsigned short*)res + o);
            const unsigned au[4] = {a.x, a.y, a.z, a.w}, ru[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                xv[2 * i] = __uint_as_float(au[i] << 16); xv[2 * i + 1] = __uint_as_float(au[i] & 0xffff0000u);
                rv[2 * i] = __uint_as_float(ru[i] << 16); rv[2 * i + 1] = __uint_as_float(ru[i] & 0xffff0000u);
            }
            unsigned short ov[8];
#pragma unroll
            for (int e = 0; e < 8; e++) ov[e] = tobf(fmaxf(xv[e] * sc[e] + rv[e], 0.f));
            uint4 out;
            out.x = ov[0] | ((unsigned)ov[1] << 16); out.y = ov[2] | ((unsigned)ov[3] << 16);
            out.z = ov[4] | ((unsigned)ov[5] << 16); out.w = ov[6] | ((unsigned)ov[7] << 16);
            *(uint4*)((unsigned short*)y + o) = out;
        } else {
            const float4 a0 = *(const float4*)((const float*)x + o), a1 = *(const float4*)((const float*)x + o + 4);
            const float4 r0 = *(const float4*)((const float*)res + o), r1 = *(const float4*)((const float*)res + o + 4);
            *(float4*)((float*)y + o) = make_float4(fmaxf(a0.x * sc[0] + r0.x, 0.f), fmaxf(a0.y * sc[1] + r0.y, 0.f), fmaxf(a0.z * sc[2] + r0.z, 0.f), fmaxf(a0.w * sc[3] + r0.w, 0.f));
            *(float4*)((float*)y + o + 4) = make_float4(fmaxf(a1.x * sc[4] + r1.x, 0.f), fmaxf(a1.y * sc[5] + r1.y, 0.f), fmaxf(a1.z * sc[6] + r1.z, 0.f), fmaxf(a1.w * sc[7] + r1.w, 0.f));
        }
    }
}
void launch_se_apply(const void* x, const void* res, void* y, int dt, const float* scale, int B, int H, int Wmax,
                     const int* W, int C, hipStream_t s) {
    const int lpr = C >> 3;
    if (dt == DT_BF16 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0 && (long)H * Wmax < (1l << 30)) {
        int sh = 0; while ((1 << sh) < lpr) sh++;
        const int per_blk = 4 * (256 >> sh);                                        // positions per block
        hipLaunchKernelGGL(k_se_apply_bf16, dim3((unsigned)((H * Wmax + per_blk - 1) / per_blk), B), dim3(256), 0, s, (const unsigned short*)x,
                           (const unsigned short*)res, (unsigned short*)y, scale, H, Wmax, W, C, sh);
        return;
    }
    const long nvec = (long)H * Wmax * (C >> 3);
    const long blocks = (nvec + 255) / 256;
    hipLaunchKernelGGL(k_se_apply, dim3((unsigned)(blocks < 2048 ? blocks : 2048), B), dim3(256), 0, s, x, res, y, dt, scale, H, Wmax, W, C);
}

// attentive statistics pooling: softmax over time per feature column, weighted mean / std
__global__ void k_asp_pool(const void* x, int xdt, const float* logits, int F, int Wmax, const int* W, int C, float* out, int with_std) {
    const int b = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    const int D = F * C;
    if (j >= D) return;
    const int f = j / C, c = j - f * C, Wb = W[b];
    float m = -INFINITY;
    for (int t = 0; t < Wb; t++) m = fmaxf(m, logits[((long)b * Wmax + t) * D + j]);
    float s = 0.f, sx = 0.f, sxx = 0.f;
    for (int t = 0; t < Wb; t++) {
        const float e = expf(logits[((long)b * Wmax + t) * D + j] - m);
        const float v = ld(x, xdt, (((long)b * F + f) * Wmax + t) * C + c);
        s += e; sx += e * v; sxx += e * v * v;
    }
    const float mu = sx / s;
    const float sg = sqrtf(fmaxf(sxx / s - mu * mu, 1e-5f));      // ResNetSE34V2.py:204 clamp(min=1e-5)
    if (with_std) { out[(long)b * 2 * D + j] = mu; out[(long)b * 2 * D + D + j] = sg; }      // ASP: [mu | sg]
    else out[(long)b * D + j] = mu;                                                              // SAP: the weighted mean only
}
void launch_asp_pool(const void* x, int x_dt, const float* logits, int B, int F, int Wmax, const int* W, int C,
                     float* out, int with_std, hipStream_t s) {
    hipLaunchKernelGGL(k_asp_pool, dim3((F * C + 255) / 256, B), dim3(256), 0, s, x, x_dt, logits, F, Wmax, W, C, out, with_std);
}

__global__ void k_l2norm_rows(float* x, int C) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float* row = x + (long)b * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += row[c] * row[c];
    s = wave_sum(s);
    const float inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);              // F.normalize eps
    for (int c = lane; c < C; c += 64) row[c] *= inv;
}
void launch_l2norm_rows(float* x, int B, int C, hipStream_t s) { hipLaunchKernelGGL(k_l2norm_rows, dim3(B), dim3(64), 0, s, x, C); }

// ------------------------------------------------------------------------------------------------
// log-mel front end (mels.py:357-395): reflect padding, |STFT| from the DFT GEMM's (re, im) columns, log(clip)
// ------------------------------------------------------------------------------------------------
__global__ void k_reflect_pad(const float* wav, long w_bs, const int* n, float* out, long o_bs, int pad, int out_cols) {
    const int b = blockIdx.y, nb = n[b];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < out_cols; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < nb + 2 * pad) {
            int src = i - pad;
            if (src < 0) src = -src;
            if (src >= nb) src = 2 * (nb - 1) - src;
            v = wav[b * w_bs + src];
        }
        out[b * o_bs + i] = v;
    }
}
void launch_reflect_pad(const float* wav, long w_bs, const int* n, float* out, long o_bs, int pad, int B, int out_cols, hipStream_t s) {
    dim3 grid((out_cols + 255) / 256 < 1024 ? (out_cols + 255) / 256 : 1024, B);
    hipLaunchKernelGGL(k_reflect_pad, grid, dim3(256), 0, s, wav, w_bs, n, out, o_bs, pad, out_cols);
}

// One thread per 16-byte group of the destination row (rows and out_cols are multiples of 4 floats).  Groups wholly inside the window copy 4
// consecutive source samples; the groups over the mirrored edges and the zero tail are built sample by sample.
__global__ __launch_bounds__(256) void k_window_pad(const float* wav, long w_bs, const int* bounds, int max_samples, float* out, long o_bs, int pad,
                                                    int out_cols) {
    const int b = blockIdx.y, begin = bounds[2 * b];
    int m = bounds[2 * b + 1] - begin;
    if (max_samples > 0 && m > max_samples) m = max_samples;
    if (m <= pad) m = 0;                                      // no mirror exists (refused on the host): zeros, nothing is read
    const float* src = wav + (long)b * w_bs + begin;
    float* row = out + (long)b * o_bs;
    const long total = m > 0 ? (long)m + 2 * pad : 0;
    for (long i = 4L * (blockIdx.x * blockDim.x + threadIdx.x); i < out_cols; i += 4L * gridDim.x * blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= pad && i + 4 <= (long)pad + m) {
            const float* p = src + (i - pad);
            if (((size_t)p & 15) == 0) v = *(const float4*)p;
            else { v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3]; }
        } else if (i < total) {
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                r[e] = 0.f;
                if (i + e < total) {
                    long k = i + e - pad;
                    if (k < 0) k = -k;
                    if (k >= m) k = 2L * (m - 1) - k;
                    r[e] = src[k];
                }
            }
            v = make_float4(r[0], r[1], r[2], r[3]);
        }
        *(float4*)(row + i) = v;
    }
}
void launch_window_pad(const float* wav, long w_bs, const int* bounds, int max_samples, float* out, long o_bs, int pad, int B, int out_cols,
                       hipStream_t s) {
    if (B <= 0 || out_cols <= 0) return;
    const int groups = (out_cols + 3) / 4;
    dim3 grid((groups + 255) / 256 < 1024 ? (groups + 255) / 256 : 1024, B);
    hipLaunchKernelGGL(k_window_pad, grid, dim3(256), 0, s, wav, w_bs, bounds, max_samples, out, o_bs, pad, out_cols);
}

__global__ void k_stft_mag(const float* spec, int lds_, float* mag, int ldm, int nf, int Tmax, const int* frames) {
    const int b = blockIdx.z, t = blockIdx.y;
    const bool live = t < frames[b];
    const float* sp = spec + ((long)b * Tmax + t) * lds_;
    float* mp = mag + ((long)b * Tmax + t) * ldm;
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < ldm; f += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (live && f < nf) { const float re = sp[f], im = sp[nf + f]; v = sqrtf(re * re + im * im); }
        mp[f] = v;
    }
}
void launch_stft_mag(const float* spec, int lds_, float* mag, int ldm, int nf, int B, int Tmax, const int* frames, hipStream_t s) {
    hipLaunchKernelGGL(k_stft_mag, dim3((ldm + 255) / 256, Tmax, B), dim3(256), 0, s, spec, lds_, mag, ldm, nf, Tmax, frames);
}

__global__ void k_log_clip(float* x, int ldx, int C, float lo, int Tmax, const int* frames) {
    const int b = blockIdx.y;
    const long total = (long)Tmax * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i / C), c = (int)(i % C);
        float* p = x + ((long)b * Tmax + t) * ldx + c;
        *p = t < frames[b] ? logf(fmaxf(*p, lo)) : 0.f;
    }
}
void launch_log_clip(float* x, int ldx, int C, float lo, int B, int Tmax, const int* frames, hipStream_t s) {
    const long total = (long)Tmax * C;
    hipLaunchKernelGGL(k_log_clip, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096), B), dim3(256), 0, s, x, ldx, C, lo, Tmax, frames);
}

// ------------------------------------------------------------------------------------------------
// out[b][n] = bias[n] + dot(x[b][0:K], w[n][0:K]) for a handful of rows b and a long K (speaker-encoder head: 50 x 5120 -> 528):
// one wave per (output column, block of 16 rows), the K axis spread over the lanes (float4).
// ------------------------------------------------------------------------------------------------
// The four products of one K step as ONE fixed expression -- an explicit fma chain, nothing left to the compiler's contraction -- shared by
// k_fc_rows and k_fc_rows4: left to itself the compiler fused the two kernels' sums differently and their results differed in the last bit.
__device__ __forceinline__ float fc_dot4(const float4 x, const float4 w) {
    return __builtin_fmaf(x.w, w.w, __builtin_fmaf(x.z, w.z, __builtin_fmaf(x.y, w.y, x.x * w.x)));
}
__global__ __launch_bounds__(64) void k_fc_rows(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int ldo, int B, int N, int K) {
    const int n = blockIdx.x, b0 = blockIdx.y * 16, lane = threadIdx.x;
    const float* wn = w + (long)n * ldw;
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {                 // K % 4 == 0
        const float4 wv = *(const float4*)(wn + k);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int b = b0 + r < B ? b0 + r : B - 1;        // clamp: branch-free loads, surplus rows discarded below
            const float4 xv = *(const float4*)(x + (long)b * ldx + k);
            acc[r] += fc_dot4(xv, wv);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float t = wave_sum(acc[r]);
        if (lane == 0 && b0 + r < B) out[(long)(b0 + r) * ldo + n] = t + (bias ? bias[n] : 0.f);
    }
}
// Many rows (config 5: 250 clips per call): FOUR output columns per wave -- the 16 rows' x vectors are fetched once per four columns (the
// one-column kernel re-read them per column: 2.8 GB through L1 / L2 for a 5 MB operand, 115 us).  Same additions in the same order per
// output (fc_dot4): bit-identical to k_fc_rows, which tests/test_ops_gpu.py holds it to.
__global__ __launch_bounds__(64) void k_fc_rows4(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int ldo, int B, int N, int K) {
    const int n0 = blockIdx.x * 4, b0 = blockIdx.y * 16, lane = threadIdx.x;
    const float* wn[4];
#pragma unroll
    for (int c = 0; c < 4; c++) wn[c] = w + (long)(n0 + c < N ? n0 + c : N - 1) * ldw;
    float acc[4][16];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[c][r] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        float4 wv[4];
#pragma unroll
        for (int c = 0; c < 4; c++) wv[c] = *(const float4*)(wn[c] + k);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int b = b0 + r < B ? b0 + r : B - 1;
            const float4 xv = *(const float4*)(x + (long)b * ldx + k);
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c][r] += fc_dot4(xv, wv[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float t = wave_sum(acc[c][r]);
            if (lane == 0 && b0 + r < B && n0 + c < N) out[(long)(b0 + r) * ldo + n0 + c] = t + (bias ? bias[n0 + c] : 0.f);
        }
}
void launch_fc_rows(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int ldo, int B, int N, int K, hipStream_t s) {
    if (B > 32) hipLaunchKernelGGL(k_fc_rows4, dim3((N + 3) / 4, (B + 15) / 16), dim3(64), 0, s, x, ldx, w, ldw, bias, out, ldo, B, N, K);
    else hipLaunchKernelGGL(k_fc_rows, dim3(N, (B + 15) / 16), dim3(64), 0, s, x, ldx, w, ldw, bias, out, ldo, B, N, K);
}

// ---------------------------------------------------------------- band-limited rational resampler (polyphase FIR)
// y[n] = sum_k h[n M - k L] x[k] over the window described in zvx_kernels.h (ResampleArgs).  One workgroup loads the polyphase bank
// [L][pitch] into LDS once and then produces `tpb` tiles of `tile` consecutive outputs of one row; per tile the input span
// [kstart(first n), kstart(last n) + T) is staged in LDS with 16-byte loads (zeros outside the row's samples), every thread computes 4
// consecutive outputs (which 4: see `strided` below).  kstart(n) = ceil((n M - half) / L) = k0 - joff[p] with n M = k0 L + p; joff[p] sits
// in column T of the bank row, so a thread divides once per tile (64 bits) and steps (k0, p) from there by its output stride times M.
// The sum of one output: acc = bank[p][0] * x[ks]; acc = fma(bank[p][t], x[ks + t], acc) for t = 1 .. T-1 -- one order, fixed by (L, M)
// alone; a tap outside the row's samples multiplies a staged 0.0f.  Nothing in it depends on the tile, the batch or the window.
__global__ __launch_bounds__(256) void k_resample_poly(const ResampleArgs a, int tile, int tpb, int xcap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    float* bk = (float*)sm;
    const int nbank = (a.L * a.pitch + 3) & ~3;
    float* xs = bk + nbank;
    const int b = blockIdx.y, tid = threadIdx.x;
    const ResampleRow r = a.rows[b];                         // (b is the same for every lane: the entry arrives through scalar loads)
    if ((long)blockIdx.x * tpb * tile >= r.zend) return;     // past the row's extent: uniform over the workgroup, before the bank load and every barrier
    for (int i = tid * 4; i < nbank; i += 1024) *(float4*)(bk + i) = *(const float4*)(a.bank + i);      // (the device bank is padded to 4 floats)
    const long nin = r.n, cnt = r.cnt;                       // the row's samples; its outputs, counted from out_begin
    const float* xrow = r.x;
    const bool vec_in = ((size_t)r.x & 15) == 0;
    const bool vec_out = ((size_t)r.out & (a.pcm16 ? 7 : 15)) == 0;
    // which 4 outputs of a tile a lane takes.  Up-conversion (M < L): tid + 256 q -- neighbouring lanes take neighbouring outputs, whose input
    // windows start at most one sample apart (LDS reads of one address broadcast) and whose phases step by M mod L; each lane stores 4 bytes of
    // a 256-byte run.  Down-conversion: 4 tid + q -- a lane's windows start 4 M / L samples after its neighbour's, and the lane stores its
    // 4 outputs as one vector.  The bank's pitch is chosen for the same step (resample_bank_pitch below); an output's sum does not depend on it.
    const bool strided = a.M < a.L;
    const int step = strided ? 256 * a.M : a.M, dk = step / a.L, dp = step % a.L;
    auto put = [&](long i, float v) {
        if (a.pcm16) ((short*)r.out)[i] = (short)fminf(fmaxf(v * 32760.0f, -32768.0f), 32767.0f);     // clamp, then truncate
        else ((float*)r.out)[i] = v;
    };
    for (int tt = 0; tt < tpb; tt++) {
        const long i0 = ((long)blockIdx.x * tpb + tt) * tile;
        if (i0 >= r.zend) break;
        const long iend = i0 + tile < r.zend ? i0 + tile : r.zend;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        auto idx = [&](int q) { return strided ? i0 + tid + 256 * q : i0 + 4 * tid + q; };
        if (i0 < cnt) {                                      // (uniform over the workgroup)
            const long ilast = (iend < cnt ? iend : cnt) - 1;
            auto kstart_floor = [&](long n) { const long t = n * a.M - a.half; return t >= 0 ? t / a.L : -((-t + a.L - 1) / a.L); };
            const long k_lo = kstart_floor(r.out_begin + i0) & ~3L;                // a lower bound of kstart, on a 4-sample boundary of the signal
            const long k_hi = kstart_floor(r.out_begin + ilast) + 1 + a.T;         // exclusive upper bound
            const long li_lo = k_lo - r.in_origin;                                 // row index of xs[0]
            const bool vin = vec_in && (r.in_origin & 3) == 0;
            const int span = (int)(k_hi - k_lo);                                   // <= xcap by the launcher's choice of `tile`
            __syncthreads();                                                        // the previous tile's readers are done (first tile: the bank is in)
            for (int j = tid * 4; j < span && j < xcap; j += 1024) {
                const long li = li_lo + j;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (vin && li >= 0 && li + 3 < nin) t = *(const float4*)(xrow + li);
                else {
                    if (li >= 0 && li < nin) t.x = xrow[li];
                    if (li + 1 >= 0 && li + 1 < nin) t.y = xrow[li + 1];
                    if (li + 2 >= 0 && li + 2 < nin) t.z = xrow[li + 2];
                    if (li + 3 >= 0 && li + 3 < nin) t.w = xrow[li + 3];
                }
                *(float4*)(xs + j) = t;
            }
            __syncthreads();
            if (idx(0) < iend && idx(0) < cnt) {
                const unsigned long nM = (unsigned long)(r.out_begin + idx(0)) * (unsigned long)a.M;
                long k0 = (long)(nM / (unsigned long)a.L);
                int p = (int)(nM - (unsigned long)k0 * (unsigned long)a.L);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (idx(q) < iend && idx(q) < cnt) {
                        const float* br = bk + p * a.pitch;
                        const float* xp = xs + (int)(k0 - __float_as_int(br[a.T]) - k_lo);
                        float acc = br[0] * xp[0];
                        for (int t = 1; t < a.T; t++) acc = __builtin_fmaf(br[t], xp[t], acc);
                        v[q] = acc;
                    }
                    k0 += dk; p += dp;
                    if (p >= a.L) { p -= a.L; k0++; }
                }
            }
        }
        if (idx(0) >= iend) continue;
        if (!strided && vec_out && idx(3) < iend) {
            const long i = idx(0);
            if (a.pcm16) {
                short4 o;
                o.x = (short)fminf(fmaxf(v[0] * 32760.0f, -32768.0f), 32767.0f); o.y = (short)fminf(fmaxf(v[1] * 32760.0f, -32768.0f), 32767.0f);
                o.z = (short)fminf(fmaxf(v[2] * 32760.0f, -32768.0f), 32767.0f); o.w = (short)fminf(fmaxf(v[3] * 32760.0f, -32768.0f), 32767.0f);
                *(short4*)((short*)r.out + i) = o;
            } else *(float4*)((float*)r.out + i) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int q = 0; q < 4; q++) if (idx(q) < iend) put(idx(q), v[q]);
        }
    }
}
// The row pitch of the bank in LDS: lanes of a wave read bank[p_i][t] with one t and phases p_i stepping by M mod L (up-conversion:
// neighbouring lanes take neighbouring outputs) or 4 M mod L (down-conversion: 4 consecutive outputs per lane), 32 lanes per
// ds_read_b32 group over 32 banks.  The worst pile-up over all start phases is counted for each pitch in
// [T + 1, T + 8] and the smallest sum wins (an odd pitch spreads distinct phases over the banks; which odd one depends on L and M).
int resample_bank_pitch(int L, int M, int T) {
    const int step = (int)(((M < L ? 1L : 4L) * M) % L);
    int best = T + 1; long best_cost = -1;
    for (int pitch = T + 1; pitch <= T + 8; pitch++) {
        long cost = 0;
        for (int p0 = 0; p0 < L; p0++) {
            int owner[32][8], n[32] = {0}, worst = 1;
            for (int i = 0, p = p0; i < 32; i++, p = (p + step) % L) {
                const int bank = (int)(((long)p * pitch) % 32);
                bool seen = false;
                for (int j = 0; j < n[bank] && j < 8; j++) seen |= owner[bank][j] == p;      // one address: a broadcast
                if (!seen) { if (n[bank] < 8) owner[bank][n[bank]] = p; n[bank]++; worst = std::max(worst, n[bank]); }
            }
            cost += worst;
        }
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = pitch; }
    }
    return best;
}
// The launch geometry, decided from (L, M, T, pitch, B, out_max) alone.  false: the bank and one tile's input span do not fit the LDS a
// workgroup may have.
bool resample_geometry_of(const ResampleArgs& a, ResampleGeometry* g) {
    const size_t nbank = ((size_t)a.L * a.pitch + 3) & ~(size_t)3;
    // tile: outputs per pass (a multiple of 4, 1024 where the span fits); its input span is at most (tile - 1) M / L + T + 2 samples, + 3 for
    // the aligned start, rounded up to whole float4s
    int tile = 1024;
    auto cap = [&](int t) { return (int)((((long)(t - 1) * a.M) / a.L + a.T + 2 + 3 + 4 + 3) & ~3L); };
    while (tile > 4 && (nbank + cap(tile)) * 4 > 96 * 1024) tile >>= 1;
    g->tile = tile; g->xcap = cap(tile);
    g->lds = (long)((nbank + g->xcap) * 4);
    // the bank is read once per workgroup: long rows take several tiles per workgroup, short ones keep the grid wide
    g->tiles = (a.out_max + tile - 1) / tile;
    g->tpb = (int)std::min<long>(8, std::max<long>(1, g->tiles * a.B / 2048));
    return g->lds <= 160 * 1024;
}
// false (nothing launched): the bank and one tile's input span do not fit the LDS a workgroup may have
bool launch_resample_poly(const ResampleArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.out_max <= 0) return true;
    ResampleGeometry g;
    if (!resample_geometry_of(a, &g)) return false;
    if (g.lds > 64 * 1024 && !lds_opt_in((const void*)k_resample_poly)) return false;
    hipLaunchKernelGGL(k_resample_poly, dim3((unsigned)((g.tiles + g.tpb - 1) / g.tpb), a.B), dim3(256), (size_t)g.lds, s, a, g.tile, g.tpb, g.xcap);
    return true;
}

// ---------------------------------------------------------------- trim-and-join of waveform rows (zvx_kernels.h, include/zvx.h: zvx_join)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
constexpr int JOIN_UNITS_PER_WAVE = 2;       // k_join_powers: 4 waves x 2 units per workgroup
// One wave per unit.  The unit's samples [lo, hi) of the row are walked in groups of 4 that are 16-byte aligned as ADDRESSES (the row may
// start anywhere: odd Nmax, an offset pointer): a group wholly inside [lo, hi) is one float4 load, a group that straddles an end is read
// sample by sample.
__global__ __launch_bounds__(256) void k_join_powers(const JoinBoundsArgs a) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.nsamples[b];
    if (n < a.frame) return;
    const int pad = a.frame / 2;
    const long nf = 1 + ((long)n + 2 * pad - a.frame) / a.hop;
    const long units = a.tiled ? nf - 1 + a.frame / a.hop : nf;
    const int ulen = a.tiled ? a.hop : a.frame;
    const float* xrow = a.x + (long)b * a.x_bs;
    const int mis = (int)(((size_t)xrow >> 2) & 3);          // xrow - mis is 16-byte aligned
    for (int j = 0; j < JOIN_UNITS_PER_WAVE; j++) {
        const long q = ((long)blockIdx.x * 4 + wave) * JOIN_UNITS_PER_WAVE + j;
        if (q >= units) return;                               // (uniform over the wave)
        long lo = q * a.hop - pad, hi = lo + ulen;
        if (lo < 0) lo = 0;
        if (hi > n) hi = n;
        double acc = 0.0;
        if (lo < hi) {
            const long g1 = (hi + mis + 3) >> 2;
            for (long g = ((lo + mis) >> 2) + lane; g < g1; g += 64) {
                const long i = 4 * g - mis;
                if (i >= lo && i + 4 <= hi) {
                    const float4 t = *(const float4*)(xrow + i);
                    acc += (double)t.x * (double)t.x + (double)t.y * (double)t.y + (double)t.z * (double)t.z + (double)t.w * (double)t.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (i + e >= lo && i + e < hi) { const double v = (double)xrow[i + e]; acc += v * v; }
                }
            }
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) a.unit[(long)b * a.upitch + q] = acc;
    }
}
void launch_join_powers(const JoinBoundsArgs& a, long units_max, hipStream_t s) {
    if (a.B <= 0 || units_max <= 0 || !a.trim) return;
    const long per = 4 * JOIN_UNITS_PER_WAVE;
    hipLaunchKernelGGL(k_join_powers, dim3((unsigned)((units_max + per - 1) / per), a.B), dim3(256), 0, s, a);
}

// One workgroup per row.  Pass 1: pmax over the nf frame powers; pass 2: first / last frame above pmax * k.  A frame's power is the sum of
// its units in ascending order, the same in both passes.
__global__ __launch_bounds__(256) void k_join_bounds(const JoinBoundsArgs a) {
    __shared__ double red_d[4];
    __shared__ long red_lo[4], red_hi[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = a.nsamples[b];
    int begin = 0, end = n;
    if (a.trim && n >= a.frame) {                            // (uniform over the workgroup)
        const int pad = a.frame / 2, r = a.tiled ? a.frame / a.hop : 1;
        const long nf = 1 + ((long)n + 2 * pad - a.frame) / a.hop;
        const double* u = a.unit + (long)b * a.upitch;
        auto power = [&](long f) { double p = u[f]; for (int j = 1; j < r; j++) p += u[f + j]; return p; };
        double pm = 0.0;
        for (long f = tid; f < nf; f += 256) pm = fmax(pm, power(f));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pm = fmax(pm, __shfl_xor(pm, o, 64));
        if (lane == 0) red_d[wave] = pm;
        __syncthreads();
        const double pmax = fmax(fmax(red_d[0], red_d[1]), fmax(red_d[2], red_d[3]));
        if (!(pmax < a.floor)) {
            const double thr = pmax * a.k;
            long first = nf, last = -1;
            for (long f = tid; f < nf; f += 256)
                if (power(f) > thr) { if (f < first) first = f; last = f; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long of = __shfl_xor(first, o, 64), ol = __shfl_xor(last, o, 64);
                first = of < first ? of : first; last = ol > last ? ol : last;
            }
            if (lane == 0) { red_lo[wave] = first; red_hi[wave] = last; }
            __syncthreads();
            for (int w = 0; w < 4; w++) { first = red_lo[w] < first ? red_lo[w] : first; last = red_hi[w] > last ? red_hi[w] : last; }
            if (last < 0) { begin = 0; end = 0; }
            else {
                const long bb = first * a.hop - a.keep, ee = (last + 1) * a.hop + a.keep;
                begin = (int)(bb < 0 ? 0 : bb); end = (int)(ee > n ? n : ee);
            }
        }
    }
    if (tid == 0) { a.bounds[2 * b] = begin; a.bounds[2 * b + 1] = end; }
}
void launch_join_bounds(const JoinBoundsArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_join_bounds, dim3(a.B), dim3(256), 0, s, a);
}

// pos: an inclusive scan of len[b] + gap[b] in chunks of 256 (shuffle scan per wave, the four wave totals through LDS, a running carry)
__global__ __launch_bounds__(256) void k_join_layout(const int* bounds, const int* gap, int B, long* pos, int* seg_begin, int* seg_len) {
    __shared__ long wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long carry = 0;
    if (tid == 0) pos[0] = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid;
        long v = 0;
        if (b < B) {
            const int bg = bounds[2 * b], m = bounds[2 * b + 1] - bg;
            seg_begin[b] = bg; seg_len[b] = m;
            v = (long)m + (gap ? gap[b] : 0);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const long t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
        __syncthreads();                                      // the previous chunk's readers of wsum are done
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long base = carry;
        for (int w = 0; w < wave; w++) base += wsum[w];
        if (b < B) pos[b + 1] = base + v;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}
void launch_join_layout(const int* bounds, const int* gap, int B, long* pos, int* seg_begin, int* seg_len, hipStream_t s) {
    if (B <= 0) return;
    hipLaunchKernelGGL(k_join_layout, dim3(1), dim3(256), 0, s, bounds, gap, B, pos, seg_begin, seg_len);
}

constexpr int JOIN_LDS_B = 2047;             // position tables of up to this many segments are searched in LDS, longer ones in global memory
constexpr int JOIN_TILE = 4096;              // outputs per workgroup: 4 groups of 4 per thread
__device__ __forceinline__ float join_gain(long i, int F) { return __fdiv_rn((float)(2 * i + 1), (float)(2 * (long)F)); }
__device__ __forceinline__ short join_pcm(float v) { return (short)fminf(fmaxf(v * 32760.0f, -32768.0f), 32767.0f); }   // clamp, then truncate
// Output groups of 4 are aligned as ADDRESSES of the destination (v = o + omis): a group wholly inside [0, pos[B]) is one vector store.  A
// group wholly inside the untouched middle of one segment is one float4 load when the source address allows, else 4 scalar loads; every other
// group (a fade, a segment edge, a gap, the ends of the row) is built sample by sample.
__global__ __launch_bounds__(256) void k_join_copy(const JoinCopyArgs a) {
    __shared__ long tab[JOIN_LDS_B + 1];
    const int tid = threadIdx.x;
    const bool in_lds = a.B <= JOIN_LDS_B;
    if (in_lds) for (int i = tid; i <= a.B; i += 256) tab[i] = a.pos[i];
    __syncthreads();
    const long* pos = in_lds ? tab : a.pos;
    const long total = pos[a.B];
    if (total > a.cap) return;
    const int omis = a.pcm16 ? (int)(((size_t)a.out >> 1) & 3) : (int)(((size_t)a.out >> 2) & 3);
    const long v0 = (long)blockIdx.x * JOIN_TILE;
    for (long v = v0 + 4 * tid; v < v0 + JOIN_TILE; v += 1024) {
        const long o = v - omis;
        if (o >= total) break;
        const long oo = o < 0 ? 0 : o;
        int s = 0, hi = a.B;                                  // the last s with pos[s] <= oo (pos[s + 1] > oo then holds: pos[B] = total > oo)
        while (hi - s > 1) { const int mid = (s + hi) >> 1; if (pos[mid] <= oo) s = mid; else hi = mid; }
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        const bool whole = o >= 0 && o + 4 <= total;
        const long rel = o - pos[s];
        int m = a.seg_len[s], F = a.fade < m / 2 ? a.fade : m / 2;
        if (whole && rel >= F && rel + 4 <= (long)m - F) {
            const float* src = a.x + (long)s * a.x_bs + a.seg_begin[s] + rel;
            if (((size_t)src & 15) == 0) { const float4 t = *(const float4*)src; r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
            else { r[0] = src[0]; r[1] = src[1]; r[2] = src[2]; r[3] = src[3]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const long oe = o + e;
                if (oe < 0 || oe >= total) continue;
                while (oe >= pos[s + 1]) s++;
                const long i = oe - pos[s];
                m = a.seg_len[s];
                if (i < m) {
                    F = a.fade < m / 2 ? a.fade : m / 2;
                    const float x = a.x[(long)s * a.x_bs + a.seg_begin[s] + i];
                    r[e] = i < F ? x * join_gain(i, F) : (i >= (long)m - F ? x * join_gain(m - 1 - i, F) : x);
                }
            }
        }
        if (whole) {
            if (a.pcm16) { short4 q; q.x = join_pcm(r[0]); q.y = join_pcm(r[1]); q.z = join_pcm(r[2]); q.w = join_pcm(r[3]); *(short4*)((short*)a.out + o) = q; }
            else *(float4*)((float*)a.out + o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            for (int e = 0; e < 4; e++) {
                if (o + e < 0 || o + e >= total) continue;
                if (a.pcm16) ((short*)a.out)[o + e] = join_pcm(r[e]); else ((float*)a.out)[o + e] = r[e];
            }
        }
    }
}
void launch_join_copy(const JoinCopyArgs& a, long upper, hipStream_t s) {
    if (a.B <= 0 || upper <= 0) return;
    const long tiles = (upper + 3 + JOIN_TILE - 1) / JOIN_TILE;        // (+ 3: the address alignment shifts the groups by up to 3 outputs)
    hipLaunchKernelGGL(k_join_copy, dim3((unsigned)tiles), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- the gathers of a stream step (zvx_kernels.h, include/zvx.h: zvx_stream_next, zvx_stream_next_many)
// One thread per group of 4 floats, groups aligned as addresses of the destination (as k_join_copy aligns its): a whole group is one
// vector store, and one vector load where the source address allows; a group at an edge is built element by element.
// Every row has its own source mel / its own destination, so the per-row entries come from a table in device memory -- one small entry
// per row, indexed by blockIdx.y, the same for every lane of a workgroup (a scalar load).  Rows of one call differ a lot in length: a
// block past its row's end leaves before it touches anything else.
__global__ __launch_bounds__(256) void k_stream_rows(const StreamRowTab a) {
    const int b = blockIdx.y;
    const StreamRow t = a.tab[b];
    const long row = (long)a.Pmax * a.nm, valid = (long)t.P * a.nm;
    const float* src = t.src;
    float* dst = a.out + (long)b * row;
    const int mis = (int)(((size_t)dst >> 2) & 3);
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4 - mis;
    if (e >= row) return;
    if (e >= 0 && e + 4 <= row) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e + 4 <= valid) {
            if (((size_t)(src + e) & 15) == 0) v = *(const float4*)(src + e);
            else v = make_float4(src[e], src[e + 1], src[e + 2], src[e + 3]);
        } else if (e < valid) {
            v.x = src[e];
            if (e + 1 < valid) v.y = src[e + 1];
            if (e + 2 < valid) v.z = src[e + 2];
        }
        *(float4*)(dst + e) = v;
    } else {
        for (int k = 0; k < 4; k++)
            if (e + k >= 0 && e + k < row) dst[e + k] = e + k < valid ? src[e + k] : 0.f;
    }
}
void launch_stream_rows(const StreamRowTab& a, hipStream_t s) {
    if (a.R <= 0 || a.Pmax <= 0) return;
    const long groups = ((long)a.Pmax * a.nm + 3 + 3) / 4;             // (+ 3: the address alignment shifts the groups by up to 3 elements)
    hipLaunchKernelGGL(k_stream_rows, dim3((unsigned)((groups + 255) / 256), a.R), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void k_stream_interiors(const StreamInteriorTab a) {
    const int b = blockIdx.y;
    const StreamInterior t = a.tab[b];
    const long cnt = t.cnt;
    if ((long)blockIdx.x * 1024 - 3 >= cnt) return;                    // the whole block lies past this row's interior
    const float* src = (t.src ? t.src : a.wav + (long)b * a.w_bs) + t.off;
    float* dst = t.dst;
    const int mis = (int)(((size_t)dst >> 2) & 3);
    const long o = ((long)blockIdx.x * 256 + threadIdx.x) * 4 - mis;
    if (o >= cnt) return;
    if (o >= 0 && o + 4 <= cnt) {
        float4 v;
        if (((size_t)(src + o) & 15) == 0) v = *(const float4*)(src + o);
        else v = make_float4(src[o], src[o + 1], src[o + 2], src[o + 3]);
        *(float4*)(dst + o) = v;
    } else {
        for (int k = 0; k < 4; k++)
            if (o + k >= 0 && o + k < cnt) dst[o + k] = src[o + k];
    }
}
void launch_stream_interiors(const StreamInteriorTab& a, long cnt_max, hipStream_t s) {
    if (a.R <= 0 || cnt_max <= 0) return;
    const long groups = (cnt_max + 3 + 3) / 4;
    hipLaunchKernelGGL(k_stream_interiors, dim3((unsigned)((groups + 255) / 256), a.R), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- integrated loudness and gain (zvx_kernels.h, include/zvx.h: zvx_loudness)
constexpr int LOUD_T = 32;                   // samples per lane in one staged chunk
constexpr int LOUD_G = LOUD_T / 4 + 1;       // 16-byte groups that cover LOUD_T samples whatever their alignment
constexpr int LOUD_LD = 4 * LOUD_G + 1;      // LDS floats per lane: odd, so that the 64 lanes' reads of one step fall on distinct banks
// The recurrence is a dependent chain of double FMAs per sample, so the parallelism is (row, unit): lane l of workgroup (blk, b) owns unit
// q = 64 blk + l of row b and walks samples [(q - 2) h, (q + 1) h) from zero state -- two units of warm-up, samples in front of the row are
// the zeros the definition puts there -- summing y^2 over the last h of them.  A lane's samples are h floats from its neighbour's: per chunk
// of LOUD_T steps the wave loads the 64 spans as 16-byte groups aligned as ADDRESSES (a group that straddles an end of the row is read
// sample by sample, nothing outside [0, n) is read), next chunk's loads in flight under this chunk's arithmetic, and the lanes walk LDS.
__global__ __launch_bounds__(64) void k_loud_units(const LoudArgs a) {
    __shared__ float st[64 * LOUD_LD];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int n = a.nsamples[b], h = a.h;
    const long U = n / h, q0 = (long)blockIdx.x * 64, q = q0 + lane;
    const float* xrow = a.x + (long)b * a.x_bs;
    const int mis = (int)(((size_t)xrow >> 2) & 3);          // xrow - mis is 16-byte aligned
    float pk = 0.f;
    if (q0 < U) {                                            // (uniform over the workgroup)
        const int nact = (int)(U - q0 < 64 ? U - q0 : 64);
        const bool active = lane < nact;
        const long steps = 3L * h, nchunks = (steps + LOUD_T - 1) / LOUD_T;
        const int off = (int)(((q - 2) * h + mis) & 3);      // where the lane's span begins inside its first group (LOUD_T % 4 == 0: in every chunk)
        float4 r[LOUD_G];
        auto fetch = [&](long c) {
#pragma unroll
            for (int k = 0; k < LOUD_G; k++) {
                const int item = k * 64 + lane, seg = item / LOUD_G, g = item - seg * LOUD_G;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (seg < nact) {
                    const long sp = (q0 + seg - 2) * h + c * LOUD_T;
                    const long pg = sp - ((sp + mis) & 3) + 4 * g;
                    if (pg >= 0 && pg + 4 <= n) v = *(const float4*)(xrow + pg);
                    else {
                        if (pg >= 0 && pg < n) v.x = xrow[pg];
                        if (pg + 1 >= 0 && pg + 1 < n) v.y = xrow[pg + 1];
                        if (pg + 2 >= 0 && pg + 2 < n) v.z = xrow[pg + 2];
                        if (pg + 3 >= 0 && pg + 3 < n) v.w = xrow[pg + 3];
                    }
                }
                r[k] = v;
            }
        };
        const LoudCoef k = a.k;
        double s1 = 0.0, s2 = 0.0, r1 = 0.0, r2 = 0.0, acc = 0.0;
        fetch(0);
        for (long c = 0; c < nchunks; c++) {
#pragma unroll
            for (int kk = 0; kk < LOUD_G; kk++) {
                const int item = kk * 64 + lane, seg = item / LOUD_G, g = item - seg * LOUD_G;
                float* d = st + seg * LOUD_LD + 4 * g;
                d[0] = r[kk].x; d[1] = r[kk].y; d[2] = r[kk].z; d[3] = r[kk].w;
            }
            __syncthreads();
            if (c + 1 < nchunks) fetch(c + 1);
            if (active) {
                const float* my = st + lane * LOUD_LD + off;
                const long t0 = c * LOUD_T;
#pragma unroll 8
                for (int t = 0; t < LOUD_T; t++) {
                    const float xf = my[t];
                    const double x = (double)xf;
                    const double y1 = fma(k.b0, x, s1);
                    s1 = fma(-k.a1, y1, fma(k.b1, x, s2));
                    s2 = fma(-k.a2, y1, k.b2 * x);
                    const double y2 = y1 + r1;
                    r1 = fma(-k.c1, y2, fma(-2.0, y1, r2));
                    r2 = fma(-k.c2, y2, y1);
                    if (t0 + t >= 2L * h && t0 + t < steps) { acc = fma(y2, y2, acc); pk = fmaxf(pk, fabsf(xf)); }
                }
            }
            __syncthreads();
        }
        if (active) a.unit[(long)b * a.upitch + q] = acc;
    }
    if (blockIdx.x == 0)                                     // the tail behind the last whole unit counts for the peak only
        for (long i = U * h + lane; i < n; i += 64) pk = fmaxf(pk, fabsf(xrow[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if (lane == 0) a.part_peak[(long)b * a.ppitch + blockIdx.x] = pk;
}
void launch_loud_units(const LoudArgs& a, long units_max, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_loud_units, dim3((unsigned)a.ppitch, a.B), dim3(64), 0, s, a);
    (void)units_max;
}

// sum over the workgroup's 256 threads in a fixed order (shuffle tree per wave, the four wave sums through LDS)
__device__ __forceinline__ double wg_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();                                          // the previous sum's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double loud_block(const double* u, long j, double four_h) { return (((u[j] + u[j + 1]) + u[j + 2]) + u[j + 3]) / four_h; }
__device__ __forceinline__ double loud_lufs(double sum, double cnt) { return cnt > 0.0 ? -0.691 + 10.0 * log10(sum / cnt) : -INFINITY; }
__device__ double loud_gain(double L, double peak, const LoudArgs& a) {
    if (!(L > -INFINITY) || !(peak > 0.0)) return 1.0;
    double g = pow(10.0, (a.target - L) / 20.0);
    g = fmin(g, pow(10.0, a.max_gain_db / 20.0));
    if (a.ceiling > 0.0 && peak * g > a.ceiling) g = a.ceiling / peak;
    return g;
}
// One workgroup per row.  Pass 1: sum and count of the blocks above the absolute gate; pass 2: of those also above a tenth of their mean.
__global__ __launch_bounds__(256) void k_loud_gates(const LoudArgs a) {
    __shared__ double red[4];
    __shared__ float redp[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = a.nsamples[b];
    const long U = n / a.h, nb = U >= 4 ? U - 3 : 0;
    const double* u = a.unit + (long)b * a.upitch;
    const double four_h = 4.0 * (double)a.h;
    float pk = 0.f;
    for (int i = tid; i < a.ppitch; i += 256) pk = fmaxf(pk, a.part_peak[(long)b * a.ppitch + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if ((tid & 63) == 0) redp[tid >> 6] = pk;
    double s = 0.0, cnt = 0.0;
    for (long j = tid; j < nb; j += 256) { const double z = loud_block(u, j, four_h); if (z > a.abs_gate) { s += z; cnt += 1.0; } }
    const double S1 = wg_sum_f64(s, red), C1 = wg_sum_f64(cnt, red);
    pk = fmaxf(fmaxf(redp[0], redp[1]), fmaxf(redp[2], redp[3]));
    double L = -INFINITY;
    if (C1 > 0.0) {                                          // (uniform over the workgroup)
        const double thr = 0.1 * (S1 / C1);
        s = 0.0; cnt = 0.0;
        for (long j = tid; j < nb; j += 256) { const double z = loud_block(u, j, four_h); if (z > a.abs_gate && z > thr) { s += z; cnt += 1.0; } }
        const double S2 = wg_sum_f64(s, red), C2 = wg_sum_f64(cnt, red);
        L = loud_lufs(S2, C2);
    }
    if (tid == 0) {
        a.lufs[b] = L; a.peak[b] = pk; a.row_sum[b] = S1; a.row_cnt[b] = (long)C1;
        a.gain[b] = a.want_gain ? (float)loud_gain(L, (double)pk, a) : 1.0f;
    }
}
void launch_loud_gates(const LoudArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_loud_gates, dim3(a.B), dim3(256), 0, s, a);
}
// One workgroup over all rows: the rows measured as one programme (blocks never span two rows).
__global__ __launch_bounds__(256) void k_loud_common(const LoudArgs a) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double s = 0.0, cnt = 0.0, pk = 0.0;
    for (int b = tid; b < a.B; b += 256) { s += a.row_sum[b]; cnt += (double)a.row_cnt[b]; pk = fmax(pk, (double)a.peak[b]); }
    const double S1 = wg_sum_f64(s, red), C1 = wg_sum_f64(cnt, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmax(pk, __shfl_xor(pk, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = pk;
    __syncthreads();
    pk = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double L = -INFINITY;
    if (C1 > 0.0) {
        const double thr = 0.1 * (S1 / C1), four_h = 4.0 * (double)a.h;
        s = 0.0; cnt = 0.0;
        for (int b = 0; b < a.B; b++) {
            const long U = a.nsamples[b] / a.h, nb = U >= 4 ? U - 3 : 0;
            const double* u = a.unit + (long)b * a.upitch;
            for (long j = tid; j < nb; j += 256) { const double z = loud_block(u, j, four_h); if (z > a.abs_gate && z > thr) { s += z; cnt += 1.0; } }
        }
        const double S2 = wg_sum_f64(s, red), C2 = wg_sum_f64(cnt, red);
        L = loud_lufs(S2, C2);
    }
    const float g = (float)loud_gain(L, pk, a);
    for (int b = tid; b < a.B; b += 256) a.gain[b] = g;
}
void launch_loud_common(const LoudArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_loud_common, dim3(1), dim3(256), 0, s, a);
}

// ---- programme loudness report (zvx_kernels.h, include/zvx.h: zvx_loudness_stats)
__device__ __forceinline__ double loud_lu(double p) { return p > 0.0 ? -0.691 + 10.0 * log10(p) : -INFINITY; }
// maximum over the workgroup's 256 threads (exact: any order)
__device__ __forceinline__ double wg_max_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();                                          // the previous reduction's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
// does short-term window power s pass both LRA gates
__device__ __forceinline__ bool loud_lra_gated(double s, double abs_gate, double thr) { return s > abs_gate && s > thr; }
// One workgroup per row.  Thread t owns the blocks and windows j with j % 256 == t in every pass, so it reads back from `win` only what it
// wrote itself.  A tile of 256 windows reads 285 units, staged in LDS once; a window's 30 units are summed in ascending index.
__global__ __launch_bounds__(256) void k_loud_windows(const LoudStatsArgs a) {
    __shared__ double red[4];
    __shared__ double us[256 + LOUD_ST_UNITS - 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long U = a.nsamples[b] / a.h, nb = U >= 4 ? U - 3 : 0, W = U >= LOUD_ST_UNITS ? U - (LOUD_ST_UNITS - 1) : 0;
    const double* u = a.unit + (long)b * a.upitch;
    double* win = a.win + (long)b * a.wpitch;
    const double four_h = 4.0 * (double)a.h, st_h = (double)LOUD_ST_UNITS * (double)a.h;
    double zmax = 0.0, smax = 0.0;                            // powers: never negative
    for (long j0 = 0; j0 < nb; j0 += 256) {                  // (nb >= W: the blocks' tiles cover the windows')
        __syncthreads();                                      // the previous tile's readers are done
        for (int i = tid; i < 256 + LOUD_ST_UNITS - 1; i += 256) us[i] = j0 + i < U ? u[j0 + i] : 0.0;
        __syncthreads();
        const long j = j0 + tid;
        if (j < nb) {
            const double z = loud_block(us, tid, four_h);
            zmax = fmax(zmax, z);
            if (a.mom) a.mom[(long)b * a.cpitch + j] = loud_lu(z);
        }
        if (j < W) {
            double acc = us[tid];
#pragma unroll
            for (int k = 1; k < LOUD_ST_UNITS; k++) acc += us[tid + k];
            const double s = acc / st_h;
            win[j] = s;
            smax = fmax(smax, s);
            if (a.sht) a.sht[(long)b * a.cpitch + j] = loud_lu(s);
        }
    }
    double sum = 0.0, cnt = 0.0;
    for (long j = tid; j < W; j += 256) { const double s = win[j]; if (s > a.abs_gate) { sum += s; cnt += 1.0; } }
    const double S1 = wg_sum_f64(sum, red), C1 = wg_sum_f64(cnt, red);
    double thr = 0.0, ng = 0.0;
    if (C1 > 0.0) {                                          // (uniform over the workgroup)
        thr = 0.01 * (S1 / C1);
        cnt = 0.0;
        for (long j = tid; j < W; j += 256) if (loud_lra_gated(win[j], a.abs_gate, thr)) cnt += 1.0;
        ng = wg_sum_f64(cnt, red);
    }
    zmax = wg_max_f64(zmax, red);
    smax = wg_max_f64(smax, red);
    if (tid == 0) {
        double* r = a.res + (long)b * LOUD_RES_WORDS;
        const long n = (long)ng;
        r[LOUD_RES_MOM_MAX] = loud_lu(zmax); r[LOUD_RES_SHORT_MAX] = loud_lu(smax);
        r[LOUD_RES_REL_THR] = thr; r[LOUD_RES_GATED] = ng;
        r[LOUD_RES_RANK_LO] = (double)(((n - 1) * 10 + 50) / 100); r[LOUD_RES_RANK_HI] = (double)(((n - 1) * 95 + 50) / 100);
        r[LOUD_RES_POW_LO] = 0.0; r[LOUD_RES_POW_HI] = 0.0;
    }
}
void launch_loud_windows(const LoudStatsArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_loud_windows, dim3(a.B), dim3(256), 0, s, a);
}
// Thread j owns window j.  Where it is gated it counts the gated windows i with s[i] < s[j], or s[i] == s[j] and i < j: its rank in an
// ascending sort whose ties break by index, so exactly one thread holds each rank.  The row's windows pass through LDS in tiles of 256, an
// ungated one as +INFINITY, which precedes nothing; every lane reads the same word of the tile at a time.
__global__ __launch_bounds__(256) void k_loud_rank(const LoudStatsArgs a) {
    __shared__ double tile[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long U = a.nsamples[b] / a.h, W = U >= LOUD_ST_UNITS ? U - (LOUD_ST_UNITS - 1) : 0;
    double* r = a.res + (long)b * LOUD_RES_WORDS;
    if ((long)blockIdx.x * 256 >= W || !(r[LOUD_RES_GATED] > 0.0)) return;       // (uniform over the workgroup)
    const double thr = r[LOUD_RES_REL_THR];
    const int lo = (int)r[LOUD_RES_RANK_LO], hi = (int)r[LOUD_RES_RANK_HI];
    const double* win = a.win + (long)b * a.wpitch;
    const long j = (long)blockIdx.x * 256 + tid;
    const double sj = j < W ? win[j] : 0.0;
    const bool mine = j < W && loud_lra_gated(sj, a.abs_gate, thr);
    int cnt = 0;
    for (long i0 = 0; i0 < W; i0 += 256) {
        __syncthreads();                                      // the previous tile's readers are done
        double v = INFINITY;
        if (i0 + tid < W) { const double s = win[i0 + tid]; if (loud_lra_gated(s, a.abs_gate, thr)) v = s; }
        tile[tid] = v;
        __syncthreads();
        if (mine) {
#pragma unroll 8
            for (int k = 0; k < 256; k++) { const double s = tile[k]; cnt += (s < sj || (s == sj && i0 + k < j)) ? 1 : 0; }
        }
    }
    if (mine && cnt == lo) r[LOUD_RES_POW_LO] = sj;
    if (mine && cnt == hi) r[LOUD_RES_POW_HI] = sj;
}
void launch_loud_rank(const LoudStatsArgs& a, long w_max, hipStream_t s) {
    if (a.B <= 0 || w_max <= 0) return;
    hipLaunchKernelGGL(k_loud_rank, dim3((unsigned)((w_max + 255) / 256), a.B), dim3(256), 0, s, a);
}

// ---- pitch report (zvx_kernels.h, include/zvx.h: zvx_pitch)
// smallest value over the workgroup's 256 threads (exact: any order); `red` holds 4 ints
__device__ __forceinline__ int wg_min_i32(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();                                          // the previous reduction's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}
__device__ __forceinline__ double wg_min_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}
// Workgroup (blk, b) takes frames [blk G, blk G + G) of row b.  Their samples -- positions [f0 H - c, f0 H - c + span) of the row, zeros
// where the position lies outside [0, n) -- are staged once in LDS as doubles: 16-byte groups aligned as ADDRESSES, a group that straddles
// an end of the row sample by sample.  Per frame lane l owns the lags l + 1 + 256 k, k < KL, each with its own accumulator: v[j] is one
// address for the whole wave (a broadcast), v[j + tau] consecutive doubles across the lanes (no bank conflict).  A lane whose lag lies
// beyond tau_max reads lag 1 instead and drops the sum.  d goes to LDS; thread t then owns lags t KL + 1 .. (t + 1) KL for the scan, d' and
// the crossing.  Every step of a frame is the same whatever its place in the run: a row's bits do not depend on the grid.
template <int KL>
__global__ __launch_bounds__(256) void k_pitch_track(const PitchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];      // (no static LDS: the opt-in beyond 64 KiB is for the dynamic block)
    const PitchRow r = a.rows[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long fb = (long)blockIdx.x * a.G;
    if (fb >= r.F) return;                                    // (uniform over the workgroup, before any barrier)
    const int W = a.W, H = a.H, tmax = a.tau_max, tmin = a.tau_min, n = r.n;
    double* vs = (double*)sm;                                 // [span]
    double* dl = vs + a.span;                                 // [tau_max + 1], d then d' by lag (entry 0 unused)
    double* red = dl + tmax + 1;                              // [4]
    int* redi = (int*)(red + 4);                              // [4]
    const int nf = (int)(r.F - fb < a.G ? r.F - fb : a.G);
    {
        const long s0 = fb * H - a.c;                         // the row position of vs[0]
        const int mis = (int)(((size_t)r.x >> 2) & 3);        // r.x - mis is 16-byte aligned
        const long base = s0 - ((s0 + mis) & 3);              // the aligned group that holds s0
        const int groups = (int)((s0 + a.span - base + 3) >> 2);
        for (int g = tid; g < groups; g += 256) {
            const long pg = base + 4L * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pg >= 0 && pg + 4 <= n) v = *(const float4*)(r.x + pg);
            else {
                if (pg >= 0 && pg < n) v.x = r.x[pg];
                if (pg + 1 >= 0 && pg + 1 < n) v.y = r.x[pg + 1];
                if (pg + 2 >= 0 && pg + 2 < n) v.z = r.x[pg + 2];
                if (pg + 3 >= 0 && pg + 3 < n) v.w = r.x[pg + 3];
            }
            const long i = pg - s0;                           // -3 .. span - 1
            if (i >= 0 && i < a.span) vs[i] = (double)v.x;
            if (i + 1 >= 0 && i + 1 < a.span) vs[i + 1] = (double)v.y;
            if (i + 2 >= 0 && i + 2 < a.span) vs[i + 2] = (double)v.z;
            if (i + 3 >= 0 && i + 3 < a.span) vs[i + 3] = (double)v.w;
        }
    }
    __syncthreads();
    int lag[KL];
#pragma unroll
    for (int k = 0; k < KL; k++) { const int t = tid + 1 + 256 * k; lag[k] = t <= tmax ? t : 1; }
    for (int g = 0; g < nf; g++) {
        const double* v = vs + (long)g * H;
        double acc[KL];
#pragma unroll
        for (int k = 0; k < KL; k++) acc[k] = 0.0;
        int j = 0;
        for (; j + 4 <= W; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double x0 = v[j + u];
#pragma unroll
                for (int k = 0; k < KL; k++) { const double t = x0 - v[j + u + lag[k]]; acc[k] = fma(t, t, acc[k]); }
            }
        }
        for (; j < W; j++) {
            const double x0 = v[j];
#pragma unroll
            for (int k = 0; k < KL; k++) { const double t = x0 - v[j + lag[k]]; acc[k] = fma(t, t, acc[k]); }
        }
        double pw = 0.0;
        for (int i = tid; i < W; i += 256) pw = fma(v[i], v[i], pw);
        const double P = wg_sum_f64(pw, red) / (double)W;     // (its first barrier: the previous frame's readers of dl are done)
#pragma unroll
        for (int k = 0; k < KL; k++) { const int t = tid + 1 + 256 * k; if (t <= tmax) dl[t] = acc[k]; }
        __syncthreads();
        // inclusive scan over the lags: thread t sums its KL lags, the threads' sums are scanned in a fixed order
        const int t0 = tid * KL + 1;
        double mine[KL], part = 0.0;
#pragma unroll
        for (int k = 0; k < KL; k++) { mine[k] = t0 + k <= tmax ? dl[t0 + k] : 0.0; part += mine[k]; }
        double inc = part;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
        if (lane == 63) red[wave] = inc;
        __syncthreads();
        const double before = __shfl_up(inc, 1, 64);          // the lanes in front of this one in its wave: an exclusive scan, nothing is subtracted
        double run = lane > 0 ? before : 0.0;                 // -> the sum of every lag in front of t0
        for (int w = 0; w < wave; w++) run += red[w];
        int first = 0x7fffffff;
        double dmin = INFINITY;
#pragma unroll
        for (int k = 0; k < KL; k++) {
            const int t = t0 + k;
            run += mine[k];
            if (t <= tmax) {
                const double dn = run > 0.0 ? mine[k] * (double)t / run : 1.0;
                dl[t] = dn;
                if (t >= tmin) {
                    dmin = fmin(dmin, dn);
                    if (dn < a.threshold && t < first) first = t;
                }
            }
        }
        first = wg_min_i32(first, redi);
        dmin = wg_min_f64(dmin, red);                        // (its barriers also publish d')
        if (tid == 0) {
            float f0 = 0.f, ap = (float)dmin;
            if (P > a.gate && first <= tmax) {
                int T = first;
                while (T + 1 <= tmax && dl[T + 1] < dl[T]) T++;
                double delta = 0.0;
                if (T - 1 >= 1 && T + 1 <= tmax) {
                    const double aa = dl[T - 1], bb = dl[T], ee = dl[T + 1], den = aa - 2.0 * bb + ee;
                    if (den > 0.0) { const double q = (aa - ee) / (2.0 * den); if (fabs(q) <= 1.0) delta = q; }
                }
                f0 = (float)(a.fs / ((double)T + delta));
                ap = (float)dl[T];
            }
            r.f0[fb + g] = f0;
            r.aper[fb + g] = ap;
        }
    }
}
bool launch_pitch_track(const PitchArgs& a, long f_max, hipStream_t s, bool dry_run) {
    if (a.B <= 0 || f_max <= 0) return true;
    if (a.W > PITCH_MAX_W || a.tau_max > PITCH_MAX_TAU || a.span > PITCH_SPAN || a.G < 1) return false;
    const size_t lds = ((size_t)a.span + (size_t)a.tau_max + 1 + 4) * sizeof(double) + 4 * sizeof(int);
    const dim3 grid((unsigned)((f_max + a.G - 1) / a.G), a.B);
    const int kl = (a.tau_max + 255) / 256;
    auto go = [&](auto kfn) {
        if (lds > 64 * 1024 && !lds_opt_in((const void*)kfn)) return false;
        if (!dry_run) hipLaunchKernelGGL(kfn, grid, dim3(256), lds, s, a);
        return true;
    };
    if (kl <= 1) return go(k_pitch_track<1>);
    if (kl <= 2) return go(k_pitch_track<2>);
    if (kl <= 4) return go(k_pitch_track<4>);
    return go(k_pitch_track<8>);
}
// One workgroup per row: thread t owns the frames f with f % 256 == t; an unvoiced frame has f0 == 0.
__global__ __launch_bounds__(256) void k_pitch_stats(const PitchArgs a) {
    __shared__ double red[4];
    const PitchRow r = a.rows[blockIdx.x];
    const int tid = threadIdx.x;
    double sum = 0.0, cnt = 0.0;
    for (long f = tid; f < r.F; f += 256) { const float v = r.f0[f]; if (v > 0.f) { sum += (double)v; cnt += 1.0; } }
    const double S = wg_sum_f64(sum, red), C = wg_sum_f64(cnt, red);
    if (tid == 0) {
        double* w = a.res + (long)blockIdx.x * PITCH_RES_WORDS;
        const long nv = (long)C;
        w[PITCH_RES_VOICED] = C; w[PITCH_RES_MEAN] = nv > 0 ? S / C : 0.0;
        w[PITCH_RES_RANK_MED] = (double)(((nv - 1) * 50 + 50) / 100); w[PITCH_RES_RANK_LO] = (double)(((nv - 1) * 5 + 50) / 100);
        w[PITCH_RES_RANK_HI] = (double)(((nv - 1) * 95 + 50) / 100);
        w[PITCH_RES_MED] = 0.0; w[PITCH_RES_LO] = 0.0; w[PITCH_RES_HI] = 0.0;
    }
}
void launch_pitch_stats(const PitchArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_pitch_stats, dim3(a.B), dim3(256), 0, s, a);
}
// Thread j owns frame j.  Where it is voiced it counts the voiced frames i with f0[i] < f0[j], or f0[i] == f0[j] and i < j: k_loud_rank's
// selection.  The row's track passes through LDS in tiles of 256, an unvoiced frame as +INFINITY, which precedes nothing.
__global__ __launch_bounds__(256) void k_pitch_rank(const PitchArgs a) {
    __shared__ float tile[256];
    const PitchRow r = a.rows[blockIdx.y];
    const int tid = threadIdx.x;
    double* w = a.res + (long)blockIdx.y * PITCH_RES_WORDS;
    if ((long)blockIdx.x * 256 >= r.F || !(w[PITCH_RES_VOICED] > 0.0)) return;       // (uniform over the workgroup)
    const int med = (int)w[PITCH_RES_RANK_MED], lo = (int)w[PITCH_RES_RANK_LO], hi = (int)w[PITCH_RES_RANK_HI];
    const long j = (long)blockIdx.x * 256 + tid;
    const float vj = j < r.F ? r.f0[j] : 0.f;
    const bool mine = vj > 0.f;
    int cnt = 0;
    for (long i0 = 0; i0 < r.F; i0 += 256) {
        __syncthreads();                                      // the previous tile's readers are done
        float v = INFINITY;
        if (i0 + tid < r.F) { const float q = r.f0[i0 + tid]; if (q > 0.f) v = q; }
        tile[tid] = v;
        __syncthreads();
        if (mine) {
#pragma unroll 8
            for (int k = 0; k < 256; k++) { const float q = tile[k]; cnt += (q < vj || (q == vj && i0 + k < j)) ? 1 : 0; }
        }
    }
    if (mine && cnt == med) w[PITCH_RES_MED] = (double)vj;
    if (mine && cnt == lo) w[PITCH_RES_LO] = (double)vj;
    if (mine && cnt == hi) w[PITCH_RES_HI] = (double)vj;
}
void launch_pitch_rank(const PitchArgs& a, long f_max, hipStream_t s) {
    if (a.B <= 0 || f_max <= 0) return;
    hipLaunchKernelGGL(k_pitch_rank, dim3((unsigned)((f_max + 255) / 256), a.B), dim3(256), 0, s, a);
}

constexpr int LOUD_TILE = 4096;              // samples per workgroup: 4 groups of 4 per thread
__global__ __launch_bounds__(256) void k_loud_apply(const LoudApplyArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = a.nsamples[b];
    const float g = a.gain[b];
    const float* x = a.x + (long)b * a.x_bs;
    float* of = (float*)a.out + (long)b * a.out_bs;
    short* os = (short*)a.out + (long)b * a.out_bs;
    const int omis = a.pcm16 ? (int)(((size_t)os >> 1) & 3) : (int)(((size_t)of >> 2) & 3);
    const long v0 = (long)blockIdx.x * LOUD_TILE;
    for (long v = v0 + 4 * tid; v < v0 + LOUD_TILE; v += 1024) {
        const long o = v - omis;
        if (o >= n) break;
        if (o >= 0 && o + 4 <= n) {
            const float* src = x + o;
            float4 t;
            if (((size_t)src & 15) == 0) t = *(const float4*)src;
            else { t.x = src[0]; t.y = src[1]; t.z = src[2]; t.w = src[3]; }
            t.x *= g; t.y *= g; t.z *= g; t.w *= g;
            if (a.pcm16) { short4 q; q.x = join_pcm(t.x); q.y = join_pcm(t.y); q.z = join_pcm(t.z); q.w = join_pcm(t.w); *(short4*)(os + o) = q; }
            else *(float4*)(of + o) = t;
        } else {
            for (int e = 0; e < 4; e++) {
                if (o + e < 0 || o + e >= n) continue;
                const float r = x[o + e] * g;
                if (a.pcm16) os[o + e] = join_pcm(r); else of[o + e] = r;
            }
        }
    }
}
void launch_loud_apply(const LoudApplyArgs& a, long n_max, hipStream_t s) {
    if (a.B <= 0 || n_max <= 0) return;
    const long tiles = (n_max + 3 + LOUD_TILE - 1) / LOUD_TILE;        // (+ 3: the address alignment shifts the groups by up to 3 samples)
    hipLaunchKernelGGL(k_loud_apply, dim3((unsigned)tiles, a.B), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- true-peak envelope and look-ahead limiter (zvx_kernels.h, include/zvx.h: zvx_limit)
constexpr int LIM_T = 21;                    // taps per oversampled point: ceil((20 os + 1) / os) for every os
constexpr int LIM_LO = 10, LIM_HI = LIMIT_ENV_REACH;      // phase 0 starts 10 samples in front of its sample; the others 9 in front, 11 behind (the last tap is a 0)
constexpr int LIM_XS = LIMIT_TILE + 1 + LIM_LO + LIM_HI;
constexpr int LIM_BP = 24;                   // pitch of the bank's copy in LDS
__device__ __forceinline__ float wg_max_f32(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();                                          // the previous reduction's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// the largest f32 of magnitude <= |g|
__device__ __forceinline__ float f32_toward_zero(double g) {
    float f = (float)g;
    if (fabs((double)f) > fabs(g)) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}
// Oversampled point m = os k0 + p is the resampler's output for (L, M) = (os, 1): its window starts at x[k0 - 10] for p = 0 and at
// x[k0 - 9] otherwise, and it is summed as k_resample_poly sums it -- acc = bank[p][0] * x[ks]; acc = fma(bank[p][t], x[ks + t], acc).
// The workgroup evaluates the points of samples t0 - 1 .. t0 + LIMIT_TILE - 1 (those of t0 - 1 count for the envelope of t0) and keeps,
// per sample, eo = max(|x|, |y[os k0]|) and uo = the largest |y| strictly between k0 and k0 + 1.
template <int OS>
__global__ __launch_bounds__(256) void k_limit_env(const LimitArgs a) {
    __shared__ float xs[LIM_XS];
    __shared__ float eo[LIMIT_TILE + 1], uo[LIMIT_TILE + 1];
    __shared__ __attribute__((aligned(16))) float bks[8 * LIM_BP];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const LimitRow r = a.rows[b];                            // (b is the same for every lane: the entry arrives through scalar loads)
    const int n = r.n;
    const long t0 = (long)blockIdx.x * LIMIT_TILE;
    float pk = 0.f;
    if (t0 < n) {                                            // (uniform over the workgroup)
        const float* xrow = r.x;
        const long base = t0 - 1 - LIM_LO;                   // xs[j] = x[base + j], 0 outside the row
        for (int j = tid; j < LIM_XS; j += 256) { const long g = base + j; xs[j] = (g >= 0 && g < n) ? xrow[g] : 0.f; }
        if (OS > 1)
            for (int i = tid; i < OS * LIM_T; i += 256) { const int p = i / LIM_T, t = i - p * LIM_T; bks[p * LIM_BP + t] = a.bank[p * a.pitch + t]; }
        __syncthreads();
        for (int j = tid; j < LIMIT_TILE + 1; j += 256) {
            const long k0 = t0 - 1 + j;
            float e = 0.f, u = 0.f;
            if (k0 >= 0 && k0 < n) {
                float xr[LIM_T + 1];                         // x[k0 - 10 .. k0 + 11]
#pragma unroll
                for (int t = 0; t < LIM_T + 1; t++) xr[t] = xs[j + t];
                e = fabsf(xr[LIM_LO]);
#pragma unroll
                for (int p = 0; p < (OS > 1 ? OS : 0); p++) {
                    const float* br = bks + p * LIM_BP;
                    const int sh = p ? 1 : 0;
                    float acc = br[0] * xr[sh];
#pragma unroll
                    for (int t = 1; t < LIM_T; t++) acc = __builtin_fmaf(br[t], xr[sh + t], acc);
                    if (p == 0) e = fmaxf(e, fabsf(acc)); else u = fmaxf(u, fabsf(acc));
                }
            }
            eo[j] = e; uo[j] = u;
        }
        __syncthreads();
        float* erow = r.env;
        const long o0 = r.off, o1 = o0 + r.cnt;              // the partial maximum runs over the emitted samples only
#pragma unroll
        for (int q = 0; q < LIMIT_TILE / 256; q++) {
            const int j = 1 + tid + 256 * q;
            const long i = t0 + j - 1;
            if (i < n) {
                const float e = fmaxf(fmaxf(eo[j], uo[j]), uo[j - 1]);
                if (erow) erow[i] = e;
                if (i >= o0 && i < o1) pk = fmaxf(pk, e);
            }
        }
    }
    pk = wg_max_f32(pk, red);
    if (tid == 0) a.part_max[(long)b * a.ppitch + blockIdx.x] = pk;
}
void launch_limit_env(const LimitArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    const dim3 grid((unsigned)a.ppitch, a.B), block(256);
    if (a.os == 1) hipLaunchKernelGGL(k_limit_env<1>, grid, block, 0, s, a);
    else if (a.os == 2) hipLaunchKernelGGL(k_limit_env<2>, grid, block, 0, s, a);
    else if (a.os == 4) hipLaunchKernelGGL(k_limit_env<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_limit_env<8>, grid, block, 0, s, a);
}

// LDS (all of it dynamic): Ds[LIMIT_TILE + 2 W] doubles -- the held depths of samples t0 - W .. t0 + LIMIT_TILE + W - 1, at the clamped index where that lies
// outside the row --, then es[LIMIT_TILE + 4 W] floats -- the envelope of samples t0 - 2 W .. t0 + LIMIT_TILE + 2 W - 1, 0 outside the row.
// Running maximum by doubling, in place: after the pass with step p, es[j] = max e over [j, j + 2 p).  A pass goes through es in chunks of
// 1024 in ascending order; a chunk reads es[j] and es[j + p] into registers, waits, and writes es[j]: what it reads ahead of itself has not
// been written in this pass.  With P the largest power of two <= 2 W + 1 the window [g - W, g + W] is the union of [g - W, g - W + P) and
// [g + W + 1 - P, g + W + 1).
__global__ __launch_bounds__(256) void k_limit_gain(const LimitArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int W = a.W, SE = LIMIT_TILE + 4 * W, SD = LIMIT_TILE + 2 * W;
    double* Ds = (double*)sm;
    float* es = (float*)(Ds + SD);
    float* red = es + SE;                                    // (no static LDS: the opt-in beyond 64 KiB covers the dynamic part alone)
    const int b = blockIdx.y, tid = threadIdx.x;
    const LimitRow r = a.rows[b];                            // (b is the same for every lane: the entry arrives through scalar loads)
    const int n = r.n;
    const long t0 = r.off + (long)blockIdx.x * LIMIT_TILE;   // the tiles cover the emitted range [off, iend), wherever `off` lies
    const long iend = min((long)n, (long)r.off + r.cnt);
    constexpr int Q = LIMIT_TILE / 256;
    float gmin = 1.f;
    if (t0 < iend) {                                         // (uniform over the workgroup)
        const float* erow = r.env;
        const float* xrow = r.x;
        const long eb = t0 - 2L * W;                         // es[j] = e[eb + j]
        float mx = 0.f;
        for (int j = tid; j < SE; j += 256) {
            const long g = eb + j;
            const float v = (g >= 0 && g < n) ? erow[g] : 0.f;
            es[j] = v; mx = fmaxf(mx, v);
        }
        mx = wg_max_f32(mx, red);                            // (its barriers also complete es)
        float g32[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) g32[q] = 1.f;
        if (mx > a.c) {                                      // otherwise every depth in reach is 0: s = r = 1 exactly
            float eown[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) eown[q] = es[2 * W + tid + 256 * q];
            int P = 1;
            for (; 2 * P <= 2 * W + 1; P *= 2) {
                for (int c0 = 0; c0 < SE; c0 += 1024) {
                    float r[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int j = c0 + tid + 256 * q;
                        r[q] = 0.f;
                        if (j < SE) { r[q] = es[j]; if (j + P < SE) r[q] = fmaxf(r[q], es[j + P]); }
                    }
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < 4; q++) { const int j = c0 + tid + 256 * q; if (j < SE) es[j] = r[q]; }
                }
                __syncthreads();
            }
            for (int j = tid; j < SD; j += 256) {
                long g = t0 - W + j;
                g = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
                const int a1 = (int)(g - W - eb), a2 = a1 + 2 * W + 1 - P;
                const float H = fmaxf(es[a1], es[a2]);
                Ds[j] = H > a.c ? 1.0 - (double)a.c / (double)H : 0.0;
            }
            __syncthreads();
            double acc[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) acc[q] = 0.0;
            const double* dp = Ds + tid;
            for (int kk = 0; kk <= 2 * W; kk++) {
                const double w = a.win[kk];
#pragma unroll
                for (int q = 0; q < Q; q++) acc[q] = fma(w, dp[kk + 256 * q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const double sm1 = 1.0 - acc[q];
                const double d = eown[q] > a.c ? 1.0 - (double)a.c / (double)eown[q] : 0.0;
                g32[q] = f32_toward_zero(fmin(sm1, 1.0 - d));
            }
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const long i = t0 + tid + 256 * q;
            if (i < iend) {
                const float v = xrow[i] * g32[q];
                if (a.pcm16) ((short*)r.out)[i - r.off] = join_pcm(v);
                else ((float*)r.out)[i - r.off] = v;
                gmin = fminf(gmin, g32[q]);
            }
        }
    }
    gmin = -wg_max_f32(-gmin, red);
    if (tid == 0) a.part_min[(long)b * a.ppitch + blockIdx.x] = gmin;
}
bool launch_limit_gain(const LimitArgs& a, hipStream_t s) {
    if (a.B <= 0) return true;
    const size_t lds = (size_t)(LIMIT_TILE + 2 * a.W) * 8 + (size_t)(LIMIT_TILE + 4 * a.W) * 4 + 16;
    if (lds > 160 * 1024) return false;
    if (lds > 64 * 1024 && !lds_opt_in((const void*)k_limit_gain)) return false;
    hipLaunchKernelGGL(k_limit_gain, dim3((unsigned)a.gtiles, a.B), dim3(256), lds, s, a);
    return true;
}

__global__ __launch_bounds__(256) void k_limit_reduce(const LimitArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float mx = 0.f, mn = 1.f;
    for (int i = tid; i < a.ppitch; i += 256) {
        mx = fmaxf(mx, a.part_max[(long)b * a.ppitch + i]);
        if (a.part_min && i < a.gtiles) mn = fminf(mn, a.part_min[(long)b * a.ppitch + i]);
    }
    mx = wg_max_f32(mx, red);
    mn = -wg_max_f32(-mn, red);
    if (tid == 0) { a.res[b] = mx; a.res[a.B + b] = mn; }
}
void launch_limit_reduce(const LimitArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_limit_reduce, dim3(a.B), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- leveler (zvx_kernels.h, include/zvx.h: zvx_level)
// k_loud_units' walk on a window: lane l of workgroup (blk, b) owns unit q = q_first + 64 blk + l of row b's SIGNAL and walks the signal's
// samples [(q - 2) h, (q + 1) h) from zero state; the row holds the signal from in_origin on, so position s is x[s - in_origin], and a
// position outside [0, n) of the row reads as 0.  The host admits a window only where that happens in front of sample 0 alone: the support
// condition of include/zvx.h, and for a last window that begins inside its signal the check of the oldest needed unit itself
// (host_post.hip, level_clamped_support_check: the clamp of the nodes to the last unit can move that unit to the left of what RL covers).
// Same chunks, same 16-byte groups aligned as ADDRESSES with scalar edges, same fma chain; p = u / h goes to p[q - q_first].
__global__ __launch_bounds__(64) void k_level_units(const LevelArgs a) {
    __shared__ float st[64 * LOUD_LD];
    const int b = blockIdx.y, lane = threadIdx.x;
    const LevelRow r = a.rows[b];                            // (b is the same for every lane: the entry arrives through scalar loads)
    const long q0 = r.q_first + (long)blockIdx.x * 64;
    if (q0 > r.q_last) return;                               // (uniform over the workgroup)
    const int n = r.n, h = a.h;
    const long q = q0 + lane;
    const float* xrow = r.x;
    const int mis = (int)(((size_t)xrow >> 2) & 3);          // xrow - mis is 16-byte aligned
    const int nact = (int)(r.q_last - q0 + 1 < 64 ? r.q_last - q0 + 1 : 64);
    const bool active = lane < nact;
    const long steps = 3L * h, nchunks = (steps + LOUD_T - 1) / LOUD_T;
    const int off = (int)(((q - 2) * h - r.in_origin + mis) & 3);      // where the lane's span begins inside its first group (LOUD_T % 4 == 0: in every chunk)
    float4 rg[LOUD_G];
    auto fetch = [&](long c) {
#pragma unroll
        for (int k = 0; k < LOUD_G; k++) {
            const int item = k * 64 + lane, seg = item / LOUD_G, g = item - seg * LOUD_G;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (seg < nact) {
                const long sp = (q0 + seg - 2) * h + c * LOUD_T - r.in_origin;       // relative to the row from here on
                const long pg = sp - ((sp + mis) & 3) + 4 * g;
                if (pg >= 0 && pg + 4 <= n) v = *(const float4*)(xrow + pg);
                else {
                    if (pg >= 0 && pg < n) v.x = xrow[pg];
                    if (pg + 1 >= 0 && pg + 1 < n) v.y = xrow[pg + 1];
                    if (pg + 2 >= 0 && pg + 2 < n) v.z = xrow[pg + 2];
                    if (pg + 3 >= 0 && pg + 3 < n) v.w = xrow[pg + 3];
                }
            }
            rg[k] = v;
        }
    };
    const LoudCoef k = a.k;
    double s1 = 0.0, s2 = 0.0, r1 = 0.0, r2 = 0.0, acc = 0.0;
    fetch(0);
    for (long c = 0; c < nchunks; c++) {
#pragma unroll
        for (int kk = 0; kk < LOUD_G; kk++) {
            const int item = kk * 64 + lane, seg = item / LOUD_G, g = item - seg * LOUD_G;
            float* d = st + seg * LOUD_LD + 4 * g;
            d[0] = rg[kk].x; d[1] = rg[kk].y; d[2] = rg[kk].z; d[3] = rg[kk].w;
        }
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
        if (active) {
            const float* my = st + lane * LOUD_LD + off;
            const long t0 = c * LOUD_T;
#pragma unroll 8
            for (int t = 0; t < LOUD_T; t++) {
                const double x = (double)my[t];
                const double y1 = fma(k.b0, x, s1);
                s1 = fma(-k.a1, y1, fma(k.b1, x, s2));
                s2 = fma(-k.a2, y1, k.b2 * x);
                const double y2 = y1 + r1;
                r1 = fma(-k.c1, y2, fma(-2.0, y1, r2));
                r2 = fma(-k.c2, y2, y1);
                if (t0 + t >= 2L * h && t0 + t < steps) acc = fma(y2, y2, acc);
            }
        }
        __syncthreads();
    }
    if (active) r.p[q - r.q_first] = acc / (double)h;
}
void launch_level_units(const LevelArgs& a, long units_max, hipStream_t s) {
    if (a.B <= 0 || units_max <= 0) return;
    hipLaunchKernelGGL(k_level_units, dim3((unsigned)((units_max + 63) / 64), a.B), dim3(64), 0, s, a);
}

__device__ __forceinline__ long level_clamp(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// A tile is LEVEL_TILE emitted samples of one row, shifted left by the destination's misalignment so that its groups of 4 are 16-byte (int16:
// 8-byte) stores.  Its samples lie in units qa .. qa + nT - 2 of the signal; node j is G[clamp(j + a - 1, 0, U - 1)] and G[m] sums the p of
// units [max(0, m - S + 1), m] above the gate in ascending order: the p of all of the tile's nodes, at most S + nT - 1 units, are staged in
// LDS once and thread t forms node qa + t.  Every position is a long; what indexes LDS or the row is a difference.
__global__ __launch_bounds__(256) void k_level_apply(const LevelArgs a) {
    __shared__ double ps[LEVEL_MAX_S + LEVEL_NODES];
    __shared__ double Ts[LEVEL_NODES];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const LevelRow r = a.rows[b];                            // (b is the same for every lane: the entry arrives through scalar loads)
    const int cnt = r.cnt, h = a.h;
    const float* x = r.x + r.off;                            // emitted sample e is x[e] * g32
    float* of = (float*)r.out;
    short* os = (short*)r.out;
    const int omis = a.pcm16 ? (int)(((size_t)os >> 1) & 3) : (int)(((size_t)of >> 2) & 3);
    const long v0 = (long)blockIdx.x * LEVEL_TILE;
    const long e0 = v0 - omis > 0 ? v0 - omis : 0, e1 = v0 - omis + LEVEL_TILE < cnt ? v0 - omis + LEVEL_TILE : cnt;      // the tile's emitted samples [e0, e1)
    float lo = INFINITY, hi = -INFINITY;
    if (e0 < e1) {                                           // (uniform over the workgroup)
        const long i0 = r.in_origin + r.off + e0;            // the signal position of emitted sample e0
        const long qa = i0 / h;
        const int ra = (int)(i0 - qa * h);
        const int nT = (ra + (int)(e1 - e0 - 1)) / h + 2;    // nodes qa .. qa + nT - 1 (<= LEVEL_NODES: h >= LEVEL_MIN_H)
        const bool none = r.U == 0;                          // a last window of a signal without a whole unit: every node is 1
        const long um1 = r.U - 1;
        const long mlo = level_clamp(qa + a.a - 1, um1), mhi = level_clamp(qa + nT - 1 + a.a - 1, um1);
        const long k0 = mlo - a.S + 1 > 0 ? mlo - a.S + 1 : 0;
        if (!none)
            for (long kq = k0 + tid; kq <= mhi; kq += 256) ps[kq - k0] = r.p[kq - r.q_first];
        __syncthreads();
        if (tid < nT) {
            double T = 1.0;
            if (!none) {
                const long m = level_clamp(qa + tid + a.a - 1, um1);
                const long ka = m - a.S + 1 > 0 ? m - a.S + 1 : 0;
                double sum = 0.0, c = 0.0;
                for (long kq = ka; kq <= m; kq++) { const double p = ps[kq - k0]; if (p > a.gate) { sum += p; c += 1.0; } }
                if (c > 0.0) {
                    const double L = -0.691 + 10.0 * log10(sum / c);
                    T = fmin(pow(10.0, (a.target - L) / 20.0), a.gmax);
                }
            }
            Ts[tid] = T;
        }
        __syncthreads();
        const double hd = (double)h;
        auto gain = [&](long e) -> float {
            const int d = ra + (int)(e - e0), dq = d / h, rem = d - dq * h;
            const double t0 = Ts[dq], t1 = Ts[dq + 1];
            return (float)fma(t1 - t0, (double)rem / hd, t0);
        };
        for (long v = v0 + 4 * tid; v < v0 + LEVEL_TILE; v += 1024) {
            const long o = v - omis;
            if (o >= cnt) break;
            if (o >= 0 && o + 4 <= cnt) {
                const float* src = x + o;
                float4 t;
                if (((size_t)src & 15) == 0) t = *(const float4*)src;
                else { t.x = src[0]; t.y = src[1]; t.z = src[2]; t.w = src[3]; }
                const float g0 = gain(o), g1 = gain(o + 1), g2 = gain(o + 2), g3 = gain(o + 3);
                t.x *= g0; t.y *= g1; t.z *= g2; t.w *= g3;
                if (a.pcm16) { short4 w; w.x = join_pcm(t.x); w.y = join_pcm(t.y); w.z = join_pcm(t.z); w.w = join_pcm(t.w); *(short4*)(os + o) = w; }
                else *(float4*)(of + o) = t;
                lo = fminf(fminf(lo, g0), fminf(fminf(g1, g2), g3));
                hi = fmaxf(fmaxf(hi, g0), fmaxf(fmaxf(g1, g2), g3));
            } else {
                for (int e = 0; e < 4; e++) {
                    if (o + e < 0 || o + e >= cnt) continue;
                    const float g = gain(o + e);
                    const float w = x[o + e] * g;
                    if (a.pcm16) os[o + e] = join_pcm(w); else of[o + e] = w;
                    lo = fminf(lo, g); hi = fmaxf(hi, g);
                }
            }
        }
    }
    lo = -wg_max_f32(-lo, red);
    hi = wg_max_f32(hi, red);
    if (tid == 0) { a.part_lo[(long)b * a.ppitch + blockIdx.x] = lo; a.part_hi[(long)b * a.ppitch + blockIdx.x] = hi; }
}
void launch_level_apply(const LevelArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_level_apply, dim3((unsigned)a.ppitch, a.B), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void k_level_reduce(const LevelArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < a.ppitch; i += 256) {
        lo = fminf(lo, a.part_lo[(long)b * a.ppitch + i]);
        hi = fmaxf(hi, a.part_hi[(long)b * a.ppitch + i]);
    }
    lo = -wg_max_f32(-lo, red);
    hi = wg_max_f32(hi, red);
    if (tid == 0) {
        const bool any = lo <= hi;                           // no emitted sample: 1 and 1
        a.res[b] = any ? lo : 1.0f; a.res[a.B + b] = any ? hi : 1.0f;
    }
}
void launch_level_reduce(const LevelArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_level_reduce, dim3(a.B), dim3(256), 0, s, a);
}

}  // namespace zvx
