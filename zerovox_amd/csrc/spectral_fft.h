// spectral_fft.h -- what the kernels on the STFT frame grid share (spectral.hip: the denoiser; watermark.hip: the watermark and its detector):
// the FFT that lives in LDS and the frame counts of a row's window.  Device code only; include it inside a .hip file after zvx_kernels.h.
#pragma once
#include "zvx_kernels.h"
#include <climits>

namespace zvx {

constexpr int DN_THREADS = 256;
constexpr int DN_PLANE = DENOISE_POINTS + DENOISE_POINTS / 32;

__device__ __forceinline__ int dn_at(int i) { return i + (i >> 5); }

// All DENOISE_POINTS / n_fft frames of the workgroup at once: 1024 radix-4 butterflies per pass, 4 per thread.
template <bool INV>
__device__ __forceinline__ void dn_fft(float* sre, float* sim, const float2* __restrict__ twid, int log2n, int tid) {
    const int N = 1 << log2n;
    int p = 1, log2p = 0;
    if (log2n & 1) {                                         // radix 2, p = 1: no twiddles; 2048 butterflies, 8 per thread
        const int half = N >> 1;
        float ar[8], ai[8], br[8], bi[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int g = tid + DN_THREADS * u, base = (g >> (log2n - 1)) << log2n, j = g & (half - 1);
            ar[u] = sre[dn_at(base + j)]; ai[u] = sim[dn_at(base + j)];
            br[u] = sre[dn_at(base + j + half)]; bi[u] = sim[dn_at(base + j + half)];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int g = tid + DN_THREADS * u, base = (g >> (log2n - 1)) << log2n, j = g & (half - 1);
            sre[dn_at(base + 2 * j)] = ar[u] + br[u]; sim[dn_at(base + 2 * j)] = ai[u] + bi[u];
            sre[dn_at(base + 2 * j + 1)] = ar[u] - br[u]; sim[dn_at(base + 2 * j + 1)] = ai[u] - bi[u];
        }
        __syncthreads();
        p = 2; log2p = 1;
    }
    const int quarter = N >> 2;
    for (; p < N; p <<= 2, log2p += 2) {
        float vr[4][4], vi[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int g = tid + DN_THREADS * u, base = (g >> (log2n - 2)) << log2n, j = g & (quarter - 1);
#pragma unroll
            for (int r = 0; r < 4; r++) { vr[u][r] = sre[dn_at(base + j + r * quarter)]; vi[u][r] = sim[dn_at(base + j + r * quarter)]; }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int g = tid + DN_THREADS * u, base = (g >> (log2n - 2)) << log2n, j = g & (quarter - 1), k = j & (p - 1);
            if (p > 1) {                                     // e^(-+ 2 pi i r k / (4 p)) = twid[r k n_fft / (4 p)] (conjugated for the inverse)
                const int sh = log2n - 2 - log2p;
#pragma unroll
                for (int r = 1; r < 4; r++) {
                    const float2 w = twid[(r * k) << sh];
                    const float wr = w.x, wi = INV ? -w.y : w.y, xr = vr[u][r], xi = vi[u][r];
                    vr[u][r] = xr * wr - xi * wi; vi[u][r] = xr * wi + xi * wr;
                }
            }
            const float t0r = vr[u][0] + vr[u][2], t0i = vi[u][0] + vi[u][2], t1r = vr[u][0] - vr[u][2], t1i = vi[u][0] - vi[u][2];
            const float t2r = vr[u][1] + vr[u][3], t2i = vi[u][1] + vi[u][3];
            float t3r = vr[u][1] - vr[u][3], t3i = vi[u][1] - vi[u][3];
            // forward: -i t3 = (t3i, -t3r); inverse: +i t3 = (-t3i, t3r)
            const float qr = INV ? -t3i : t3i, qi = INV ? t3r : -t3r;
            const int o = base + ((j - k) << 2) + k;
            sre[dn_at(o)] = t0r + t2r;         sim[dn_at(o)] = t0i + t2i;
            sre[dn_at(o + p)] = t1r + qr;      sim[dn_at(o + p)] = t1i + qi;
            sre[dn_at(o + 2 * p)] = t0r - t2r; sim[dn_at(o + 2 * p)] = t0i - t2i;
            sre[dn_at(o + 3 * p)] = t1r - qr;  sim[dn_at(o + 3 * p)] = t1i - qi;
        }
        __syncthreads();
    }
}

// The window of a row of n samples (zvx_kernels.h, DenoiseArgs): the emitted count; the signal's frames from f_first on (all there will be
// where the signal goes on); the frames transformed, i.e. those up to the last one that begins at or before the last emitted sample.
__device__ __forceinline__ int dn_count(const DenoiseRow& r) {
    const int room = max(0, r.n - r.off);
    return r.cnt >= 0 ? min(r.cnt, room) : room;
}
__device__ __forceinline__ int dn_frames_from_first(const DenoiseArgs& a, const DenoiseRow& r) {
    if (r.n <= 0) return 0;
    if (!(r.mirrors & 2)) return INT_MAX;
    const long span = r.origin + r.n + 2 * a.pad - a.n_fft;   // absolute: 64 bits
    const long F = span >= 0 ? 1 + span / a.hop - r.f_first : 0;
    return (int)min(max(F, 0L), (long)INT_MAX);
}
__device__ __forceinline__ int dn_frames_used(const DenoiseArgs& a, const DenoiseRow& r) {
    const int cnt = dn_count(r);
    if (cnt <= 0) return 0;
    return min(dn_frames_from_first(a, r), (r.off + cnt - 1 - r.rel) / a.hop + 1);
}

}  // namespace zvx
