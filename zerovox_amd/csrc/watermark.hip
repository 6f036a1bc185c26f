// watermark.hip -- the keyed audio watermark and its detector (include/zvx.h: zvx_watermark, zvx_watermark_ex, zvx_watermark_rows,
// zvx_watermark_detect, zvx_watermark_identify) on the denoiser's STFT frame grid.  watermark_kernels.h: WatermarkArgs, WmDetectArgs, WmKeysArgs.  The FFT in LDS, its layout and the frame counts of a row's window
// are the denoiser's (spectral_fft.h); the embedder's overlap-add is the denoiser's launch (launch_denoise_ola).
//
// The search kernel's LDS: the folded table T[P][JC] of f32, JC = min(J - 2, WM_TABLE / P) bands at a time (48 KB), and two arrays of 256
// doubles for the reductions: 52 KB per workgroup, 3 workgroups per CU of 160 KB.  In the shift pass thread t serves shift s = t mod P and
// the t / P-th slice of the table's rows: the lanes of a slice read ONE table word at a time (a broadcast: no bank conflict), and their
// sign bytes come from P consecutive rows of a table that stays in the vector cache (P x J bytes: 5.7 KB at the defaults).
//
// The search over many keys (k_wm_search_keys, zvx_watermark_identify): a workgroup serves WM_KEYS = 8 keys of one (window, row).  T and
// den are built once per phase and band run for the 8; in the shift pass a thread reads one table word and adds it, signed, to 8 sums it
// carries in registers, so the LDS traffic and the table build per key fall to an eighth.  The signs come PACKED, 32 to a word
// ([K][P][ceil(J / 32)], k_wm_signs): k_wm_search's byte loads, whose lanes lie J bytes apart and so touch a cache line each, are what
// bounds that kernel -- with them a workgroup of 8 keys took 8 times one key's time, and three workgroups on a CU three times as long
// each (measured: 32 rows x 1024 frames, 256 keys, 346 ms against 314 ms for 256 single-key calls).  Packed, a lane fetches 32 signs of
// its row with one load and the lanes of a wave read one contiguous run (12 bytes apart at the defaults).  The summand is +-(double)T in
// place of (double)(+-1.f * T): the same number.
// The per-key slice sums go through the ONE array sa in turn (two barriers per key and phase, nothing next to a shift pass of
// P J / nparts steps) instead of an array per key: 8 arrays would add 14 KB and cost the third workgroup of a CU.  LDS: T 48 KB + sa 2 KB
// + sb 2 KB + so 1 KB = 53 KB, 3 workgroups (12 waves) per CU as k_wm_search.  8 keys and not 16: a 10 s row has 6 windows, and at 256
// keys 8 per workgroup gives 192 workgroups for 256 CUs where 16 would give 96.  The best over a row's windows is taken on the host from
// the [B][NW][K] results (zvx.hip, do_watermark_identify): no second launch.
#include "watermark_kernels.h"
#include "spectral_fft.h"

namespace zvx {

// The denoiser's frames kernel with the keyed gain: row descriptor at the top, DENOISE_POINTS / n_fft slots, the same loads and stores.
__global__ __launch_bounds__(DN_THREADS) void k_watermark_frames(const WatermarkArgs wa) {
    __shared__ float sre[DN_PLANE], sim[DN_PLANE];
    const DenoiseArgs& a = wa.dn;
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
            int s = r.rel + f * a.hop + t;
            if (left && s < 0) s = -s;
            if (right && s >= n) s = 2 * (n - 1) - s;
            s = min(max(s, 0), n - 1);
            v = a.win[t] * x[s];
        }
        sre[dn_at(i)] = v; sim[dn_at(i)] = 0.f;
    }
    __syncthreads();
    dn_fft<false>(sre, sim, (const float2*)a.twid, lg, tid);
    // X' = g X on the bins of the bands, X elsewhere (no multiply), mirrored as the conjugate into the upper half (DC and Nyquist: imaginary
    // part dropped); item (q, k) touches entries k and n_fft - k of frame q only
    const int nf = N / 2 + 1, items = (DENOISE_POINTS >> lg) * nf, k_hi = wa.k_lo + wa.J * wa.KB;
    // the row's own table of the stack (uniform over the workgroup, as the row entry is)
    const signed char* sign = wa.sign_of_row ? wa.sign + (long)wa.sign_of_row[b] * wa.P * wa.J : wa.sign;
    for (int g = tid; g < items; g += DN_THREADS) {
        const int q = g / nf, k = g - q * nf, i1 = dn_at((q << lg) + k), i2 = dn_at((q << lg) + ((N - k) & (N - 1)));
        float re = sre[i1], im = sim[i1];
        if (k >= wa.k_lo && k < k_hi) {
            const int j = (k - wa.k_lo) / wa.KB;
            const int c = (int)(((r.f_first + f0 + q) / wa.TB) % wa.P);      // the SIGNAL's frame index: 64 bits
            const float gn = sign[c * wa.J + j] > 0 ? wa.g_up : wa.g_dn;
            re *= gn; im *= gn;
        }
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

// Detector, first launch: whole rows (frame f begins at sample f hop - pad, both mirrors).  per * J <= DENOISE_POINTS / 2 since J <= n_fft / 2.
__global__ __launch_bounds__(DN_THREADS) void k_wm_bands(const WmDetectArgs a) {
    __shared__ float sre[DN_PLANE], sim[DN_PLANE];
    __shared__ float slb[DENOISE_POINTS / 2];
    const int tid = threadIdx.x, b = blockIdx.y, N = a.n_fft, lg = a.log2n, per = DENOISE_POINTS >> lg;
    const WmDetectRow r = a.rows[b];
    const int n = r.n, F = r.F;
    const int f0 = blockIdx.x * per;
    if (f0 >= F) return;                                     // (uniform over the workgroup)
    for (int i = tid; i < DENOISE_POINTS; i += DN_THREADS) {
        const int f = f0 + (i >> lg), t = i & (N - 1);
        float v = 0.f;
        if (f < F) {
            int s = f * a.hop - a.pad + t;                   // numpy 'reflect'; inside the row for every validated length, clamped all the same
            if (s < 0) s = -s;
            if (s >= n) s = 2 * (n - 1) - s;
            s = min(max(s, 0), n - 1);
            v = a.win[t] * r.x[s];
        }
        sre[dn_at(i)] = v; sim[dn_at(i)] = 0.f;
    }
    __syncthreads();
    dn_fft<false>(sre, sim, (const float2*)a.twid, lg, tid);
    const int J = a.J;
    for (int g = tid; g < per * J; g += DN_THREADS) {
        const int q = g / J, j = g - q * J, k0 = a.k_lo + j * a.KB;
        float s = 0.f;
        for (int u = 0; u < a.KB; u++) {                     // ascending bins
            const int i = dn_at((q << lg) + k0 + u);
            s += log2f(fmaxf(sre[i] * sre[i] + sim[i] * sim[i], 1e-6f));
        }
        slb[g] = s;
    }
    __syncthreads();
    const int JD = J - 2;
    for (int g = tid; g < per * JD; g += DN_THREADS) {
        const int q = g / JD, j = g - q * JD + 1;
        if (f0 + q < F) r.d[(long)(f0 + q) * JD + (j - 1)] = slb[q * J + j] - 0.5f * (slb[q * J + j - 1] + slb[q * J + j + 1]);
    }
}

constexpr int WM_THREADS = 256;

// Detector, second launch: one workgroup per (window, row).
__global__ __launch_bounds__(WM_THREADS) void k_wm_search(const WmDetectArgs a) {
    __shared__ float T[WM_TABLE];
    __shared__ double sa[WM_THREADS], sb[WM_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y, w = blockIdx.x;
    const WmDetectRow r = a.rows[b];
    if (w >= wm_windows(r.F, a.WF)) return;                  // (uniform over the workgroup)
    const int P = a.P, TB = a.TB, J = a.J, JD = J - 2;
    const int fa = a.WF > 0 ? w * (a.WF / 2) : 0, fb = a.WF > 0 ? min(fa + a.WF, r.F) : r.F;     // the window's frames [fa, fb)
    const int JC = min(JD, WM_TABLE / P);
    const int nparts = max(1, WM_THREADS / P), s = tid % P, part = tid / P;
    const bool shifts = part < nparts;
    const int c_lo = shifts ? (int)((long)part * P / nparts) : 0, c_hi = shifts ? (int)((long)(part + 1) * P / nparts) : 0;
    double best = 0.0;                                       // thread s < P: the largest z of its shift over the phases, and its offset
    int best_o = 0;
    bool have = false;
    for (int ph = 0; ph < TB; ph++) {
        const int m0 = (fa + ph) / TB, m1 = (fb - 1 + ph) / TB;              // the blocks that meet the window
        double num = 0.0, den = 0.0;
        for (int j0 = 0; j0 < JD; j0 += JC) {
            const int jc = min(JC, JD - j0);
            __syncthreads();                                 // the table's readers of the chunk before are done
            for (int g = tid; g < P * jc; g += WM_THREADS) {
                const int c = g / jc, jj = g - c * jc;
                float t = 0.f;
                for (int m = m0 + ((c - m0 % P) % P + P) % P; m <= m1; m += P) {          // ascending blocks m = c (mod P)
                    const int f_lo = max(fa, m * TB - ph), f_hi = min(fb, (m + 1) * TB - ph);
                    float e = 0.f;
                    for (int f = f_lo; f < f_hi; f++) e += r.d[(long)f * JD + j0 + jj];
                    t += e;
                    den += (double)e * (double)e;
                }
                T[c * jc + jj] = t;
            }
            __syncthreads();
            if (shifts)
                for (int c = c_lo; c < c_hi; c++) {
                    int row = c + s; if (row >= P) row -= P;
                    const signed char* sg = a.sign + row * J + j0 + 1;       // D's column j0 + jj is band j0 + jj + 1
                    const float* tr = T + c * jc;
                    for (int jj = 0; jj < jc; jj++) num += (double)((float)sg[jj] * tr[jj]);
                }
        }
        sa[tid] = num; sb[tid] = den;
        __syncthreads();
        for (int h = WM_THREADS / 2; h > 0; h >>= 1) {       // the denominator: a tree over the workgroup
            if (tid < h) sb[tid] += sb[tid + h];
            __syncthreads();
        }
        if (tid < P) {
            double v = 0.0;
            for (int q = 0; q < nparts; q++) v += sa[q * P + tid];           // ascending slices
            const double dd = sb[0];
            const double z = dd > 0.0 ? v / sqrt(dd) : 0.0;
            const int o = ph + TB * tid;
            if (!have || z > best || (z == best && o < best_o)) { best = z; best_o = o; have = true; }
        }
        __syncthreads();
    }
    // the largest z over the shifts, the smallest offset among equals (P <= WM_THREADS)
    __shared__ int so[WM_THREADS];
    sa[tid] = tid < P && have ? best : -1e300; so[tid] = tid < P && have ? best_o : 0x7fffffff;
    __syncthreads();
    for (int h = WM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double z2 = sa[tid + h]; const int o2 = so[tid + h];
            if (z2 > sa[tid] || (z2 == sa[tid] && o2 < so[tid])) { sa[tid] = z2; so[tid] = o2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool ok = sa[0] > -1e299;                      // (a NaN row: nothing compared true; 0 / 0)
        a.win_score[(long)b * a.NW + w] = ok ? (float)sa[0] : 0.f;
        a.win_offset[(long)b * a.NW + w] = ok ? so[0] : 0;
    }
}

// Sign tables from keys; the hash is the host's (host_post.hip, wm_mix64), in 64-bit integer arithmetic.  packed == 0: one thread per byte of
// out[n][P][J], +1 / -1 (the embedder's form).  packed != 0: one thread per word of out[n][P][W], W = ceil(J / 32), bit j % 32 of word
// j / 32 set where the sign is +1 (the form k_wm_search_keys reads: a lane fetches 32 signs of its table row with one load).
__device__ inline bool wm_sign_plus(unsigned long long key, int c, int j) {
    unsigned long long z = key ^ (((unsigned long long)c << 32) | (unsigned long long)j);
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z >> 63) != 0;
}
__global__ __launch_bounds__(WM_THREADS) void k_wm_signs(const unsigned long long* keys, void* out, long total, int P, int J, int packed) {
    const long i = (long)blockIdx.x * WM_THREADS + threadIdx.x;
    if (i >= total) return;                                  // total: n P J bytes, or n P W words
    const int per_row = packed ? (J + 31) / 32 : J;
    const long tc = i / per_row;                             // (table, row)
    const int u = (int)(i - tc * per_row), c = (int)(tc % P);
    const unsigned long long key = keys[tc / P];
    if (!packed) { ((signed char*)out)[i] = wm_sign_plus(key, c, u) ? 1 : -1; return; }
    unsigned bits = 0;
    for (int q = 0; q < 32 && u * 32 + q < J; q++) bits |= wm_sign_plus(key, c, u * 32 + q) ? 1u << q : 0u;
    ((unsigned*)out)[i] = bits;
}

// The search over the keys k0 .. k0 + WM_KEYS - 1 of one (window, row): k_wm_search with the key-independent work done once.  Every sum of a
// key runs in k_wm_search's order -- T and den are built by the same statements, a key's num adds the same products over the same c, jj
// and band runs, the slices are summed ascending, z and the tie rules are the same -- so entry (b, w, k) has that kernel's bits.  The
// keys past K of the last run repeat key K - 1 and write nothing.
__global__ __launch_bounds__(WM_THREADS) void k_wm_search_keys(const WmKeysArgs ka) {
    __shared__ float T[WM_TABLE];
    __shared__ double sa[WM_THREADS], sb[WM_THREADS];
    __shared__ int so[WM_THREADS];
    const WmDetectArgs& a = ka.d;
    const int tid = threadIdx.x, b = blockIdx.y, w = blockIdx.x, K = ka.K, k0 = blockIdx.z * WM_KEYS;
    const WmDetectRow r = a.rows[b];
    if (w >= wm_windows(r.F, a.WF)) return;                  // (uniform over the workgroup)
    const int P = a.P, TB = a.TB, J = a.J, JD = J - 2;
    const int fa = a.WF > 0 ? w * (a.WF / 2) : 0, fb = a.WF > 0 ? min(fa + a.WF, r.F) : r.F;     // the window's frames [fa, fb)
    const int JC = min(JD, WM_TABLE / P);
    const int nparts = max(1, WM_THREADS / P), s = tid % P, part = tid / P;
    const bool shifts = part < nparts;
    const int c_lo = shifts ? (int)((long)part * P / nparts) : 0, c_hi = shifts ? (int)((long)(part + 1) * P / nparts) : 0;
    const int W = (J + 31) / 32;                             // words per row of a packed table
    long koff[WM_KEYS];                                      // each key's table in the stack (uniform)
#pragma unroll
    for (int k = 0; k < WM_KEYS; k++) koff[k] = (long)min(k0 + k, K - 1) * P * W;
    double best[WM_KEYS];                                    // thread s < P: per key the largest z of its shift over the phases, and its offset
    int best_o[WM_KEYS];
#pragma unroll
    for (int k = 0; k < WM_KEYS; k++) { best[k] = 0.0; best_o[k] = 0; }
    bool have = false;
    for (int ph = 0; ph < TB; ph++) {
        const int m0 = (fa + ph) / TB, m1 = (fb - 1 + ph) / TB;              // the blocks that meet the window
        double num[WM_KEYS], den = 0.0;
#pragma unroll
        for (int k = 0; k < WM_KEYS; k++) num[k] = 0.0;
        for (int j0 = 0; j0 < JD; j0 += JC) {
            const int jc = min(JC, JD - j0);
            __syncthreads();                                 // the table's readers of the chunk before are done
            for (int g = tid; g < P * jc; g += WM_THREADS) {
                const int c = g / jc, jj = g - c * jc;
                float t = 0.f;
                for (int m = m0 + ((c - m0 % P) % P + P) % P; m <= m1; m += P) {          // ascending blocks m = c (mod P)
                    const int f_lo = max(fa, m * TB - ph), f_hi = min(fb, (m + 1) * TB - ph);
                    float e = 0.f;
                    for (int f = f_lo; f < f_hi; f++) e += r.d[(long)f * JD + j0 + jj];
                    t += e;
                    den += (double)e * (double)e;
                }
                T[c * jc + jj] = t;
            }
            __syncthreads();
            if (shifts)
                for (int c = c_lo; c < c_hi; c++) {
                    int row = c + s; if (row >= P) row -= P;
                    const unsigned* sg = ka.sign_bits + row * W;
                    const float* tr = T + c * jc;
                    unsigned sw[WM_KEYS];
                    for (int jj = 0; jj < jc; jj++) {
                        const int j = j0 + 1 + jj;                           // D's column j0 + jj is band j0 + jj + 1
                        if (jj == 0 || (j & 31) == 0) {                      // (uniform) the next 32 signs of the row, for every key of the run
#pragma unroll
                            for (int k = 0; k < WM_KEYS; k++) sw[k] = sg[koff[k] + (j >> 5)];
                        }
                        const double t = (double)tr[jj], nt = -t;            // (double)(+-1.f * x) is +-(double)x: k_wm_search's summand, exactly
                        const unsigned bit = 1u << (j & 31);
#pragma unroll
                        for (int k = 0; k < WM_KEYS; k++) num[k] += (sw[k] & bit) ? t : nt;
                    }
                }
        }
        sb[tid] = den;
        __syncthreads();
        for (int h = WM_THREADS / 2; h > 0; h >>= 1) {       // the denominator: a tree over the workgroup
            if (tid < h) sb[tid] += sb[tid + h];
            __syncthreads();
        }
        const double dd = sb[0];
#pragma unroll
        for (int k = 0; k < WM_KEYS; k++) {                  // the keys take the one array of slice sums in turn
            sa[tid] = num[k];
            __syncthreads();
            if (tid < P) {
                double v = 0.0;
                for (int q = 0; q < nparts; q++) v += sa[q * P + tid];       // ascending slices
                const double z = dd > 0.0 ? v / sqrt(dd) : 0.0;
                const int o = ph + TB * tid;
                if (!have || z > best[k] || (z == best[k] && o < best_o[k])) { best[k] = z; best_o[k] = o; }
            }
            __syncthreads();
        }
        if (tid < P) have = true;
    }
    // per key the largest z over the shifts, the smallest offset among equals (P <= WM_THREADS)
#pragma unroll
    for (int k = 0; k < WM_KEYS; k++) {
        __syncthreads();
        sa[tid] = tid < P && have ? best[k] : -1e300; so[tid] = tid < P && have ? best_o[k] : 0x7fffffff;
        __syncthreads();
        for (int h = WM_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) {
                const double z2 = sa[tid + h]; const int o2 = so[tid + h];
                if (z2 > sa[tid] || (z2 == sa[tid] && o2 < so[tid])) { sa[tid] = z2; so[tid] = o2; }
            }
            __syncthreads();
        }
        if (tid == 0 && k0 + k < K) {
            const bool ok = sa[0] > -1e299;                  // (a NaN row: nothing compared true; 0 / 0)
            const long at = ((long)b * a.NW + w) * K + k0 + k;
            a.win_score[at] = ok ? (float)sa[0] : 0.f;
            a.win_offset[at] = ok ? so[0] : 0;
        }
    }
}

void launch_watermark_frames(const WatermarkArgs& a, hipStream_t s) {
    if (a.dn.B <= 0 || a.dn.Fmax <= 0) return;
    const int per = DENOISE_POINTS >> a.dn.log2n;
    hipLaunchKernelGGL(k_watermark_frames, dim3((unsigned)((a.dn.Fmax + per - 1) / per), (unsigned)a.dn.B), dim3(DN_THREADS), 0, s, a);
}

void launch_wm_bands(const WmDetectArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.Fmax <= 0) return;
    const int per = DENOISE_POINTS >> a.log2n;
    hipLaunchKernelGGL(k_wm_bands, dim3((unsigned)((a.Fmax + per - 1) / per), (unsigned)a.B), dim3(DN_THREADS), 0, s, a);
}

void launch_wm_search(const WmDetectArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.NW <= 0) return;
    hipLaunchKernelGGL(k_wm_search, dim3((unsigned)a.NW, (unsigned)a.B), dim3(WM_THREADS), 0, s, a);
}

void launch_wm_signs(const unsigned long long* keys, void* out, int n, int P, int J, bool packed, hipStream_t s) {
    const long total = (long)n * P * (packed ? (J + 31) / 32 : J);
    if (total <= 0) return;
    hipLaunchKernelGGL(k_wm_signs, dim3((unsigned)((total + WM_THREADS - 1) / WM_THREADS)), dim3(WM_THREADS), 0, s, keys, out, total, P, J, packed ? 1 : 0);
}

void launch_wm_search_keys(const WmKeysArgs& a, hipStream_t s) {
    if (a.d.B <= 0 || a.d.NW <= 0 || a.K <= 0) return;
    hipLaunchKernelGGL(k_wm_search_keys, dim3((unsigned)a.d.NW, (unsigned)a.d.B, (unsigned)((a.K + WM_KEYS - 1) / WM_KEYS)), dim3(WM_THREADS), 0, s, a);
}

}  // namespace zvx
