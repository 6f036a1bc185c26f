// fir.hip -- the equaliser's FIR filter over waveform rows (include/zvx.h: zvx_fir, zvx_fir_ex, zvx_fir_rows).  zvx_kernels.h: FirRow,
// FirArgs, FIR_TILE.
//
//   y[i] = sum over k = 0 .. K-1 of h[k] * x[i + D - k],  acc a double from +0.0, the terms added in ASCENDING k, one rounding to f32.
//
// The product of two f32 values is exact in double, so a fused multiply-add and a multiply followed by an add give the same bits and a
// result depends on the order of k alone.  That order is written out below: nothing is split, reassociated or handed to a matrix unit.
//
// k_fir: grid (tiles of the longest emitted range, B), 256 lanes, FIR_TILE = 256 * FIR_R emitted samples per workgroup.  The workgroup
// reads rows[blockIdx.y] at its top and works from it alone (a workgroup past its row's extent returns at once), so the whole-row call, the
// _ex call and the per-row call run the same instructions.  It stages the slab x[j0 .. j0 + FIR_TILE + Kp - 2] of its tile in LDS as f32,
// zero wherever the index lies outside the row [0, n) -- the host's support condition makes those true zeros of the signal -- with j0 =
// off + tile * FIR_TILE + D - (Kp - 1) and Kp = K rounded up to FIR_R (the table holds zero taps behind K: a zero term changes no bit).
// Lane l keeps the FIR_R outputs of the CONSECUTIVE indices FIR_R l .. FIR_R l + FIR_R - 1 in registers.  Output r at tap k = FIR_R g + j
// reads slab[FIR_R l + FIR_R (G - 1 - g) + (r - j + FIR_R - 1)], G = Kp / FIR_R: a group of FIR_R taps needs 2 FIR_R - 1 samples, of which
// FIR_R - 1 are the previous group's, so a group costs FIR_R LDS reads and conversions for FIR_R^2 double FMAs, FIR_R independent chains.
// Slab position p lives at word p + (p >> 6): the lanes of a wave read words FIR_R apart, and the one word of padding per 64 moves every
// run of 64 positions to its own residue of the bank number, so the 64 lanes of a read land on 64 banks.
// The taps are uniform over the wave: doubles in a device table, read through uniform loads.  Results leave through vector stores, 16
// bytes where the destination's address allows, chosen per lane from the address alone: no bit changes.
// LDS: (FIR_TILE + FIR_MAX_TAPS) words and their padding, 20.3 KiB.  No atomics, no workgroup waits for another.
//
// k_fir_copy: the in-place form's second launch, out[e] = tmp[e] for e < cnt of every row.
#include "zvx_kernels.h"

namespace zvx {

constexpr int FIR_R = 4;
static_assert(FIR_TILE == 256 * FIR_R, "a workgroup of 256 lanes emits FIR_R samples per lane");
static_assert(FIR_MAX_TAPS % FIR_R == 0, "the tap table is padded to groups of FIR_R");
constexpr int FIR_SLAB = FIR_TILE + FIR_MAX_TAPS;            // >= FIR_TILE + Kp - 1
constexpr int FIR_SLAB_WORDS = FIR_SLAB + (FIR_SLAB >> 6) + 1;

__device__ __forceinline__ int fir_word(int p) { return p + (p >> 6); }
__device__ __forceinline__ short fir_pcm(float v) { return (short)fminf(fmaxf(v * 32760.0f, -32768.0f), 32767.0f); }   // the resampler's rule

__global__ __launch_bounds__(256) void k_fir(FirArgs a) {
    const FirRow r = a.rows[blockIdx.y];
    const long e0 = (long)blockIdx.x * FIR_TILE;             // the tile's first emitted sample
    if (e0 >= r.cnt) return;
    __shared__ float slab[FIR_SLAB_WORDS];
    const int Kp = a.Kp, G = Kp / FIR_R, tid = threadIdx.x;
    const int S = FIR_TILE + Kp - 1;
    const long j0 = (long)r.off + e0 + a.D - (Kp - 1);       // the row index of slab position 0
    const float* __restrict__ x = r.x;
    for (int p = tid; p < S; p += 256) {
        const long j = j0 + p;
        slab[fir_word(p)] = (j >= 0 && j < r.n) ? x[j] : 0.0f;
    }
    __syncthreads();
    const double* __restrict__ h = a.taps;
    double acc[FIR_R], v[2 * FIR_R - 1];
#pragma unroll
    for (int i = 0; i < FIR_R; i++) acc[i] = 0.0;
    {   // what group -1 would have read first: the samples group 0 inherits
        const int w = fir_word(FIR_R * tid + FIR_R * G);
#pragma unroll
        for (int m = 0; m < FIR_R - 1; m++) v[m] = (double)slab[w + m];
    }
    for (int g = 0; g < G; g++) {
#pragma unroll
        for (int m = FIR_R - 2; m >= 0; m--) v[m + FIR_R] = v[m];
        const int w = fir_word(FIR_R * tid + FIR_R * (G - 1 - g));       // FIR_R positions of one run of 64: consecutive words
#pragma unroll
        for (int m = 0; m < FIR_R; m++) v[m] = (double)slab[w + m];
        double hk[FIR_R];
#pragma unroll
        for (int j = 0; j < FIR_R; j++) hk[j] = h[FIR_R * g + j];
#pragma unroll
        for (int j = 0; j < FIR_R; j++)                      // ascending k; the FIR_R outputs are independent chains
#pragma unroll
            for (int i = 0; i < FIR_R; i++) acc[i] = __builtin_fma(hk[j], v[i - j + FIR_R - 1], acc[i]);
    }
    const long e = e0 + (long)FIR_R * tid;
    if (e >= r.cnt) return;
    float y[FIR_R];
#pragma unroll
    for (int i = 0; i < FIR_R; i++) y[i] = (float)acc[i];
    const bool whole = e + FIR_R <= r.cnt;
    if (a.pcm16) {
        short* o = (short*)r.out + e;
        if (whole && ((uintptr_t)o & 7) == 0) {
            short4 q; q.x = fir_pcm(y[0]); q.y = fir_pcm(y[1]); q.z = fir_pcm(y[2]); q.w = fir_pcm(y[3]);
            *(short4*)o = q;
        } else {
#pragma unroll
            for (int i = 0; i < FIR_R; i++) if (e + i < r.cnt) o[i] = fir_pcm(y[i]);
        }
    } else {
        float* o = (float*)r.out + e;
        if (whole && ((uintptr_t)o & 15) == 0) *(float4*)o = make_float4(y[0], y[1], y[2], y[3]);
        else {
#pragma unroll
            for (int i = 0; i < FIR_R; i++) if (e + i < r.cnt) o[i] = y[i];
        }
    }
}

__global__ __launch_bounds__(256) void k_fir_copy(const FirCopyRow* __restrict__ rows) {
    const FirCopyRow r = rows[blockIdx.y];
    for (long e = (long)blockIdx.x * FIR_TILE + threadIdx.x; e < r.cnt && e < ((long)blockIdx.x + 1) * FIR_TILE; e += 256) r.dst[e] = r.src[e];
}

void launch_fir(const FirArgs& a, long cnt_max, hipStream_t s) {
    if (cnt_max <= 0 || a.B <= 0) return;
    const dim3 grid((unsigned)((cnt_max + FIR_TILE - 1) / FIR_TILE), (unsigned)a.B);
    hipLaunchKernelGGL(k_fir, grid, dim3(256), 0, s, a);
}

void launch_fir_copy(const FirCopyRow* rows, int B, long cnt_max, hipStream_t s) {
    if (cnt_max <= 0 || B <= 0) return;
    const dim3 grid((unsigned)((cnt_max + FIR_TILE - 1) / FIR_TILE), (unsigned)B);
    hipLaunchKernelGGL(k_fir_copy, grid, dim3(256), 0, s, rows);
}

}  // namespace zvx
