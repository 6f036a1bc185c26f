// spectral.hip -- the vocoder-bias denoiser (include/zvx.h: zvx_denoise, zvx_denoise_ex, zvx_denoise_bias): STFT frames of a waveform row through an FFT
// that lives in LDS, a per-bin gain, the inverse FFT, and the overlap-add of the windowed frames.  zvx_kernels.h: DenoiseArgs.
//
// The transform: Stockham autosort, radix 4 (one radix-2 pass first where log2 n_fft is odd), decimation in time.  A pass with sub-transform
// size p takes butterfly j < n_fft / 4, k = j mod p: inputs x[j + r n_fft / 4] times e^(-+ 2 pi i r k / (4 p)), r = 0 .. 3, outputs
// y[4 (j - k) + k + r p]; the result of the last pass is in natural order, so the gain reads bin k at index k.  In place: every thread reads
// the inputs of its 4 butterflies into registers, the workgroup synchronises, then the outputs are written.
//
// LDS: split re / im planes of DENOISE_POINTS floats, index i stored at i + (i >> 5): the reads of a pass are consecutive (conflict-free);
// the writes of the first radix-4 pass have stride 4, which the extra word per 32 spreads over all 32 banks of a ds_write_b32 group (later
// passes write runs of p consecutive words: at most 2-way).  33 KB per workgroup: 4 workgroups, 16 waves, per CU of 160 KB.
#include "zvx_kernels.h"
#include "spectral_fft.h"

namespace zvx {

__global__ __launch_bounds__(DN_THREADS) void k_denoise_frames(const DenoiseArgs a) {
    __shared__ float sre[DN_PLANE], sim[DN_PLANE];
    const int tid = threadIdx.x, b = blockIdx.y, N = a.n_fft, lg = a.log2n;
    const DenoiseRow r = a.rows[b];                          // (b is the same for every lane: the entry arrives through scalar loads)
    const int n = r.n;
    const int F = dn_frames_used(a, r);                      // frames f_first .. f_first + F - 1 of the signal, f below counted from f_first
    const int f0 = blockIdx.x * (DENOISE_POINTS >> lg);
    if (f0 >= F) return;                                     // (uniform over the workgroup)
    const float* x = r.x;
    const bool left = r.mirrors & 1, right = r.mirrors & 2;
    for (int i = tid; i < DENOISE_POINTS; i += DN_THREADS) {
        const int f = f0 + (i >> lg), t = i & (N - 1);
        float v = 0.f;
        if (f < F && f >= r.skip) {
            int s = r.rel + f * a.hop + t;                   // numpy 'reflect' where the signal's end is in the window; inside the window for every
            if (left && s < 0) s = -s;                       // validated length and support, clamped all the same
            if (right && s >= n) s = 2 * (n - 1) - s;
            s = min(max(s, 0), n - 1);
            v = a.win[t] * x[s];
        }
        sre[dn_at(i)] = v; sim[dn_at(i)] = 0.f;
    }
    __syncthreads();
    dn_fft<false>(sre, sim, (const float2*)a.twid, lg, tid);
    const int nf = N / 2 + 1, items = (DENOISE_POINTS >> lg) * nf;
    if (a.mag) {                                             // magnitude-out mode (zvx_denoise_bias)
        for (int g = tid; g < items; g += DN_THREADS) {
            const int q = g / nf, k = g - q * nf, i = dn_at((q << lg) + k);
            if (f0 + q < F && f0 + q >= r.skip) a.mag[((long)b * a.Fmax + f0 + q) * nf + k] = sqrtf(sre[i] * sre[i] + sim[i] * sim[i]);
        }
        return;
    }
    // X' = G X on bins 0 .. n_fft / 2, mirrored as the conjugate into the upper half (DC and Nyquist: imaginary part dropped); item (q, k)
    // touches entries k and n_fft - k of frame q only
    for (int g = tid; g < items; g += DN_THREADS) {
        const int q = g / nf, k = g - q * nf, i1 = dn_at((q << lg) + k), i2 = dn_at((q << lg) + ((N - k) & (N - 1)));
        float re = sre[i1], im = sim[i1];
        const float m = sqrtf(re * re + im * im);
        const float G = m > 0.f ? fmaxf(a.floor, 1.f - a.strength * a.bias[k] / m) : a.floor;
        re *= G; im *= G;
        if (k == 0 || 2 * k == N) im = 0.f;
        sre[i1] = re; sim[i1] = im;
        if (i2 != i1) { sre[i2] = re; sim[i2] = -im; }
    }
    __syncthreads();
    dn_fft<true>(sre, sim, (const float2*)a.twid, lg, tid);
    const float inv_n = 1.f / (float)N;                      // a power of two: exact
    for (int i = tid; i < DENOISE_POINTS; i += DN_THREADS) {
        const int f = f0 + (i >> lg), t = i & (N - 1);
        if (f < F && f >= r.skip) r.work[(long)f * N + t] = a.win[t] * (sre[dn_at(i)] * inv_n);
    }
}

__device__ __forceinline__ short dn_pcm(float v) { return (short)fminf(fmaxf(v * 32760.0f, -32768.0f), 32767.0f); }   // the resampler's rule

__global__ __launch_bounds__(256) void k_denoise_ola(const DenoiseArgs a) {
    const int b = blockIdx.y, N = a.n_fft;
    const DenoiseRow r = a.rows[b];                          // (b is the same for every lane: the entry arrives through scalar loads)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dn_count(r)) return;
    const int i = r.off + e;                                 // the sample's index in the window
    const float xi = r.x[i];
    float v = xi;
    if (!a.copy) {
        const int F = dn_frames_from_first(a, r), p = i - r.rel;                             // p: the padded position, counted from frame f_first's
        const int f_hi = min(F - 1, p / a.hop), f_lo = p < N ? 0 : (p - N) / a.hop + 1;      // frames f with f hop <= p < f hop + n_fft
        const float* w = r.work;
        float num = 0.f;
        double den = 0.0;
        for (int f = f_lo; f <= f_hi; f++) {                 // ascending f: the order is part of the contract
            const int t = p - f * a.hop;
            num += w[(long)f * N + t];
            den += a.win2[t];
        }
        if (den >= a.den_min) v = num / (float)den;
    }
    if (a.pcm16) ((short*)r.out)[e] = dn_pcm(v);
    else ((float*)r.out)[e] = v;
}

void launch_denoise_frames(const DenoiseArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.Fmax <= 0) return;
    const int per = DENOISE_POINTS >> a.log2n;
    hipLaunchKernelGGL(k_denoise_frames, dim3((unsigned)((a.Fmax + per - 1) / per), (unsigned)a.B), dim3(DN_THREADS), 0, s, a);
}

void launch_denoise_ola(const DenoiseArgs& a, long n_max, hipStream_t s) {
    if (a.B <= 0 || n_max <= 0) return;
    hipLaunchKernelGGL(k_denoise_ola, dim3((unsigned)((n_max + 255) / 256), (unsigned)a.B), dim3(256), 0, s, a);
}

}  // namespace zvx
