// voicematch.hip -- cosine scores of query embeddings against a device-resident library of embeddings, and the best `top` of them
// (include/zvx.h: zvx_spk_score, zvx_spk_topk).  voicematch_kernels.h: SpkArgs, the slab / group plan and the LDS budget.
//
// The library is the one large stream: K x dim f32, read once per group of up to 64 queries.  At 64 queries the arithmetic (2 B K dim
// flops) is of the order of the f32 matrix rate, so the products run on the exact-f32 MFMA, v_mfma_f32_16x16x4_f32: 16 queries (A) x 16
// library rows (B) per tile, up to four query tiles a wave = four independent accumulators, which is what the instruction's 40-cycle
// dependent latency asks for.  The 16 x 16 shape and not 32 x 32 because the group must shrink to 16 queries at dim 2048 (LDS), and
// because a remainder of few queries then costs one tile's steps and not two.  A packed-f32 VALU form would run the same arithmetic at
// under half the rate and leave no issue slots for the norms.
//
// A lane holds library row j = lane & 15 and the k-slice g = lane >> 4: per step of 16 columns it loads the float4 at columns
// 16 t + 4 g .. + 3 (one 16-byte load; the 64 lanes cover 16 rows x 64 bytes) and feeds component c of it to MFMA c of the step, against
// the same float4 of the query rows from LDS.  The order in which the products of one (query, row) pair are added is therefore a function
// of dim alone -- step t, component c, slice g -- whatever tile, slab, group or call the pair is in: the position contract.  Two
// sets of 8 loads per lane alternate, across the wave's row tiles: one is in flight while the other feeds the MFMAs, so one wave per SIMD
// keeps 32 KB a CU in flight.
//
// Norms, in the same pass: three sums of squares per row -- of x, of x 2^-70 and of x 2^70 -- so that a row scaled by 1e-20 or 1e+18
// neither underflows nor overflows (spk_norm picks the sum whose range holds); the four slices' sums are added in a fixed order through
// two lane exchanges.  The queries are divided by their norm when they are staged, so a dot product is bounded by the row's norm.
//
// Top-k: after a tile each wave says whether any of its scores beats the tail of its query's list (one barrier); the waves that have one
// take turns (two barriers each) to put their 16 scores per query into LDS, and thread q of the workgroup inserts those that beat the
// tail of query q's list.  Rows arrive in ascending index order, so a strict comparison keeps the lower index
// first among equal scores.  No atomics; the lists of a (query, slab) go to memory once, k_spk_merge selects over the slabs.
#include "voicematch_kernels.h"
#include "mfma_util.h"
#include <cfloat>
#include <climits>

namespace zvx {


struct Sq3 { float b, m, s; };                               // sums of (x 2^-70)^2, x^2, (x 2^70)^2
__device__ __forceinline__ void sq_add(Sq3& a, float x) {
    const float xb = x * 0x1p-70f, xs = x * 0x1p70f;
    a.b = fmaf(xb, xb, a.b); a.m = fmaf(x, x, a.m); a.s = fmaf(xs, xs, a.s);
}
__device__ __forceinline__ Sq3 sq_sum(Sq3 a, Sq3 o) { return Sq3{a.b + o.b, a.m + o.m, a.s + o.s}; }
__device__ __forceinline__ Sq3 sq_xor(Sq3 a, int mask) {
    return sq_sum(a, Sq3{__shfl_xor(a.b, mask), __shfl_xor(a.m, mask), __shfl_xor(a.s, mask)});
}
// the norm from the three sums: the plain one where it lies in [2^-60, FLT_MAX], the up-scaled one below (every |x| < 2^-30: no overflow),
// the down-scaled one above; NaN and inf come through
__device__ __forceinline__ float spk_norm(Sq3 a) {
    if (a.m >= 0x1p-60f && a.m <= FLT_MAX) return sqrtf(a.m);
    if (a.m < 0x1p-60f) return sqrtf(a.s) * 0x1p-70f;
    return sqrtf(a.b) * 0x1p70f;
}
// score = dot(q, e) / max(|q| |e|, FLT_MIN) from d = dot(q / |q|, e); what is not finite (a norm above FLT_MAX included) is -2
__device__ __forceinline__ float spk_final(float d, float nq, float ne) {
    const float s = (nq * ne >= FLT_MIN) ? d / ne : (d * 0x1p126f) * nq;
    return (fabsf(s) <= FLT_MAX && nq <= FLT_MAX && ne <= FLT_MAX) ? s : -2.f;
}

template <int NT, bool TOPK>
__global__ __launch_bounds__(SPK_THREADS) void k_spk_match(const SpkArgs a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
    const int dim = a.dim, steps = (dim + 15) >> 4, pitch = steps * 16 + 4, top = a.top;
    constexpr int GQ = NT * 16;
    constexpr int SPK_RING = 8;                              // loads per set and lane (8 KB a wave in flight)
    const int b0 = a.b0 + blockIdx.y * a.nq, nq = min(a.nq, a.B - b0);
    float* sq = smem;                                        // [GQ][pitch]: q / |q|, zero beyond dim and beyond nq
    float* snq = sq + GQ * pitch;                            // [GQ]: |q|
    float* tile = snq + GQ;                                  // [GQ][17]: one wave's scores
    float* ls = tile + GQ * 17;                              // [GQ][top]
    int* li = (int*)(ls + GQ * top);                         // [GQ][top]
    float* thr = (float*)(li + GQ * top);                    // [GQ]: the score a candidate of the query has to beat (SPK_EMPTY_SCORE: any)
    int* flags = (int*)(thr + GQ);                           // [2][4]: which waves have a candidate in their tile

    // ---- stage the group: a wave per query, the norm first
    for (int i = w; i < GQ; i += 4) {
        float* dst = sq + i * pitch;
        if (i >= nq) {
            for (int k = lane; k < pitch; k += 64) dst[k] = 0.f;
            if (lane == 0) { snq[i] = 0.f; thr[i] = SPK_EMPTY_SCORE; }
            continue;
        }
        const float* src = a.q + (size_t)(b0 + i) * dim;
        Sq3 acc{0.f, 0.f, 0.f};
        for (int k = lane; k < dim; k += 64) sq_add(acc, src[k]);
        for (int m = 1; m < 64; m <<= 1) acc = sq_xor(acc, m);
        const float n = spk_norm(acc);
        // q (pre) / (n pre) with pre a power of two that keeps 1 / (n pre) in range; n == 0: a zero query, n NaN: NaN stays in q
        const float pre = n < 0x1p-64f ? 0x1p64f : n > 0x1p64f ? 0x1p-64f : 1.f;
        const float inv = n > 0.f ? 1.f / (n * pre) : 0.f;
        for (int k = lane; k < pitch; k += 64) dst[k] = k < dim ? (src[k] * pre) * inv : 0.f;
        if (lane == 0) { snq[i] = n; thr[i] = SPK_EMPTY_SCORE; }
    }
    __syncthreads();

    const long R0 = (long)blockIdx.x * SPK_SLAB;
    const int rows_here = (int)min((long)SPK_SLAB, a.K - R0);
    const int n_it = (rows_here + SPK_ITER_ROWS - 1) / SPK_ITER_ROWS;
    const int S = (n_it * steps + 2 * SPK_RING - 1) / (2 * SPK_RING) * (2 * SPK_RING);     // whole rounds: the steps past the last tile run on zeros
    const int col = 4 * g;
    // The lane's loads: two sets of SPK_RING float4.  While the steps of one set run, the other set's loads are in flight; where a set
    // begins, ONE explicit wait for everything outstanding stands in front of the loads issued for the set after it.  What was tried
    // first: a ring refilled slot by slot (1.70 against 1.53 ms at 64 queries x 10^6 rows, profiles/voice_match.txt).  In the ISA a load
    // under a branch, a select right behind a load, or a tile's conditional stores between the loads each left the compiler unsure how many
    // memory operations are in flight: it waited for all of them, the one just issued included.  So the load is unconditional, from a clamped address; whether its
    // words count (zero beyond the library's rows and beyond dim) is kept beside them (bit of `live`) and applied when they are used.
    float4 ring[2][SPK_RING];
    unsigned live = 0;
    int pit = 0, pt = 0;                                     // the next (iteration, step) to fetch
    auto fetch_set = [&](int set) {
#pragma unroll
        for (int i = 0; i < SPK_RING; i++) {
            const long row = R0 + pit * SPK_ITER_ROWS + w * 16 + j;
            const int k = 16 * pt + col;
            ring[set][i] = *(const float4*)(a.lib + (size_t)min(row, a.K - 1) * dim + min(k, dim - 4));
            const bool ok = pit < n_it && row < a.K && k < dim;
            const int bit = set * SPK_RING + i;
            live = (live & ~(1u << bit)) | ((ok ? 1u : 0u) << bit);
            if (++pt == steps) { pt = 0; pit++; }
        }
    };
    fetch_set(0);
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Sq3 nrm{0.f, 0.f, 0.f};
    int it = 0, t = 0, n_list = 0;                           // n_list: entries of the list of query tid (threads below nq)
    const float* aq = sq + j * pitch + col;
    for (int s0 = 0; s0 < S; s0 += 2 * SPK_RING) {
#pragma unroll
        for (int i = 0; i < 2 * SPK_RING; i++) {
            if (i % SPK_RING == 0) {
                __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): this set has arrived (and the last tile's stores are out)
                fetch_set(1 - i / SPK_RING);
            }
            {
                const bool ok = (live >> i) & 1u;
                const float4 raw = ring[i / SPK_RING][i % SPK_RING];
                const float4 v = make_float4(ok ? raw.x : 0.f, ok ? raw.y : 0.f, ok ? raw.z : 0.f, ok ? raw.w : 0.f);
                float4 qa[NT];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) qa[nt] = *(const float4*)(aq + nt * 16 * pitch + 16 * t);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nt].x, v.x, acc[nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nt].y, v.y, acc[nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nt].z, v.z, acc[nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[nt].w, v.w, acc[nt], 0, 0, 0);
                sq_add(nrm, v.x); sq_add(nrm, v.y); sq_add(nrm, v.z); sq_add(nrm, v.w);
                if (++t == steps && it >= n_it) { t = 0; it++; }          // (past the last tile; uniform over the workgroup)
                else if (t == steps) {
                    // ---- the tile is complete: row j's norm from its four slices (g, g ^ 1) + (g ^ 2, g ^ 3), then 4 NT scores a lane:
                    // row j against queries 16 nt + 4 g + r
                    const float ne = spk_norm(sq_xor(sq_xor(nrm, 16), 32));
                    const int tile0 = it * SPK_ITER_ROWS;    // rows counted within the slab: 32-bit
                    const int row = tile0 + w * 16 + j;
                    const bool row_ok = row < rows_here;
                    float sc[NT][4];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
#pragma unroll
                        for (int r = 0; r < 4; r++) sc[nt][r] = spk_final(acc[nt][r], snq[nt * 16 + 4 * g + r], ne);
                    if constexpr (!TOPK) {
#pragma unroll
                        for (int nt = 0; nt < NT; nt++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const int q = nt * 16 + 4 * g + r;
                                if (q < nq && row_ok) a.score[(size_t)(b0 + q) * (size_t)a.K + (size_t)(R0 + row)] = sc[nt][r];
                            }
                    } else {
                        // does any score of this wave beat its query's tail?  (thr lags behind the list at most downwards: it only lets more through)
                        bool pass = false;
#pragma unroll
                        for (int nt = 0; nt < NT; nt++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const int q = nt * 16 + 4 * g + r;
                                pass |= q < nq && row_ok && sc[nt][r] > thr[q];
                            }
                        int* fl = flags + (it & 1) * 4;      // (two sets: a wave may be a tile ahead of the slowest reader)
                        const bool wave_pass = __any(pass);
                        if (lane == 0) fl[w] = wave_pass;
                        __syncthreads();
                        for (int ph = 0; ph < 4; ph++) {
                            if (!__builtin_amdgcn_readfirstlane(fl[ph])) continue;         // (uniform over the workgroup: a scalar branch)
                            if (w == ph) {
#pragma unroll
                                for (int nt = 0; nt < NT; nt++)
#pragma unroll
                                    for (int r = 0; r < 4; r++) tile[(nt * 16 + 4 * g + r) * 17 + j] = sc[nt][r];
                            }
                            __syncthreads();
                            if (tid < nq) {
                                const int base = tile0 + ph * 16;
                                const int cnt = max(0, min(16, rows_here - base));
                                float* qs = ls + tid * top; int* qi = li + tid * top;
                                float cand[16];              // all 16 reads first: they do not wait for one another
#pragma unroll
                                for (int c = 0; c < 16; c++) cand[c] = c < cnt ? tile[tid * 17 + c] : SPK_EMPTY_SCORE;
#pragma unroll
                                for (int c = 0; c < 16; c++) {
                                    const float v2 = cand[c];
                                    if (v2 > SPK_EMPTY_SCORE && (n_list < top || v2 > qs[top - 1])) {
                                        int p = min(n_list, top - 1);
                                        while (p > 0 && qs[p - 1] < v2) { qs[p] = qs[p - 1]; qi[p] = qi[p - 1]; p--; }
                                        qs[p] = v2; qi[p] = (int)R0 + base + c;
                                        if (n_list < top) n_list++;
                                    }
                                }
                                thr[tid] = n_list == top ? qs[top - 1] : SPK_EMPTY_SCORE;
                            }
                            __syncthreads();
                        }
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    nrm = Sq3{0.f, 0.f, 0.f};
                    t = 0; it++;
                }
            }
        }
    }
    if constexpr (TOPK) {
        if (tid < nq) {                                      // (the thread's own list: written by itself, no barrier needed)
            const size_t o = ((size_t)(b0 + tid) * (size_t)gridDim.x + blockIdx.x) * (size_t)top;
            for (int p = 0; p < top; p++) {
                a.cand_s[o + p] = p < n_list ? ls[tid * top + p] : SPK_EMPTY_SCORE;
                a.cand_i[o + p] = p < n_list ? li[tid * top + p] : INT_MAX;
            }
        }
    }
}

// (score, index) a before b: the larger score, the lower index among equal scores
__device__ __forceinline__ bool spk_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// One workgroup per query: `top` rounds, each the best candidate that comes after the round before's pick (the candidates' indices are
// distinct, so the order is total and nothing has to be marked as taken).
__global__ __launch_bounds__(SPK_THREADS) void k_spk_merge(const float* cand_s, const int* cand_i, long n, int top, float* out_s, int* out_i) {
    __shared__ float rs[SPK_THREADS];
    __shared__ int ri[SPK_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* cs = cand_s + (size_t)b * (size_t)n;
    const int* ci = cand_i + (size_t)b * (size_t)n;
    float ps = FLT_MAX; int pi = -1;                         // the pick before: every candidate comes after it
    for (int p = 0; p < top; p++) {
        float bs = SPK_EMPTY_SCORE; int bi = INT_MAX;
        for (long c = tid; c < n; c += SPK_THREADS) {
            const float s = cs[c]; const int i = ci[c];
            if (spk_before(ps, pi, s, i) && spk_before(s, i, bs, bi)) { bs = s; bi = i; }
        }
        rs[tid] = bs; ri[tid] = bi;
        __syncthreads();
        for (int h = SPK_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h && spk_before(rs[tid + h], ri[tid + h], rs[tid], ri[tid])) { rs[tid] = rs[tid + h]; ri[tid] = ri[tid + h]; }
            __syncthreads();
        }
        ps = rs[0]; pi = ri[0];
        __syncthreads();
        if (tid == 0) { out_s[(size_t)b * top + p] = ps; out_i[(size_t)b * top + p] = pi; }
    }
}

template <int NT, bool TOPK>
static bool spk_launch_one(SpkArgs a, int groups, hipStream_t s, bool probe) {
    const size_t lds = spk_lds_bytes(NT * 16, a.dim, a.top);
    if (!lds_opt_in((const void*)k_spk_match<NT, TOPK>)) return false;
    if (!probe)
        hipLaunchKernelGGL((k_spk_match<NT, TOPK>), dim3((unsigned)spk_slabs(a.K), (unsigned)groups), dim3(SPK_THREADS), lds, s, a);
    return true;
}
template <bool TOPK>
static bool spk_launch_nt(const SpkArgs& a, int nt, int groups, hipStream_t s, bool probe) {
    switch (nt) {
        case 1: return spk_launch_one<1, TOPK>(a, groups, s, probe);
        case 2: return spk_launch_one<2, TOPK>(a, groups, s, probe);
        case 3: return spk_launch_one<3, TOPK>(a, groups, s, probe);
        default: return spk_launch_one<4, TOPK>(a, groups, s, probe);
    }
}

bool launch_spk_match(const SpkArgs& args, hipStream_t s, bool probe) {
    SpkArgs a = args;
    const int G = spk_group(a.dim, a.top), whole = a.B / G, rest = a.B - whole * G;
    bool ok = true;
    if (whole) {
        a.b0 = 0; a.nq = G;
        ok = a.top ? spk_launch_nt<true>(a, G / 16, whole, s, probe) : spk_launch_nt<false>(a, G / 16, whole, s, probe);
    }
    if (ok && rest) {
        a.b0 = whole * G; a.nq = rest;
        ok = a.top ? spk_launch_nt<true>(a, (rest + 15) / 16, 1, s, probe) : spk_launch_nt<false>(a, (rest + 15) / 16, 1, s, probe);
    }
    return ok;
}

void launch_spk_merge(const float* cand_s, const int* cand_i, int B, long nslab, int top, float* out_s, int* out_i, hipStream_t s) {
    hipLaunchKernelGGL(k_spk_merge, dim3((unsigned)B), dim3(SPK_THREADS), 0, s, cand_s, cand_i, nslab * top, top, out_s, out_i);
}

}  // namespace zvx
