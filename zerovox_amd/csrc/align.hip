// align.hip -- dynamic time warping of feature rows, pair by pair, and the DCT cepstra it runs on in zvx_align_wav
// (include/zvx.h: zvx_dtw, zvx_align_wav).  zvx_kernels.h: DtwPair, DtwArgs and the limits.
//
// Forward (k_dtw_forward): one workgroup per pair, `lanes` threads (64 .. 1024, 512 above 16 columns: the call's longest Ta rounded up to a wave, dtw_lanes).  The rows of a are
// taken in bands of `lanes`: lane l of a band owns row i = i0 + l and keeps a[i] in registers, zero-filled to the next of 4 / 8 / 16 / 32
// columns (adding +0 changes no bit of the sum of squares).  The band sweeps its anti-diagonals: at step s lane l works on j = s - l.  Its left
// neighbour C(i, j-1) is its own previous value, its up neighbour C(i-1, j) is what lane l - 1 wrote to a double-buffered LDS line one
// step earlier, its diagonal neighbour C(i-1, j-1) is the up value it read one step earlier, kept in a register.  One barrier per step: a
// line is read in step s and written again in step s + 1, behind that barrier.  The last row of a band goes to an LDS edge of Tb doubles,
// which lane 0 of the next band reads as its up neighbour; the edge is rewritten in place, because the band's last lane writes edge[j]
// n - 1 steps after lane 0 read it (n = 1: the same thread, the read first).  The b rows are read from memory as they come (the 64 lanes of a
// wave read 64 consecutive rows), two steps before their cell, and the distance is formed one step before it.  Every value of C is formed by the same instructions whatever the band width: a pair's bits depend on
// its own rows and dim alone.
//
// Direction codes: one byte per cell (0 diagonal, 1 up = (i-1, j), 2 left = (i, j-1)), diagonal-major -- anti-diagonal s of the pair's own
// Ta x Tb matrix is contiguous and starts at dtw_diag_off(s), row i sits at i - max(0, s - (Tb - 1)) in it --, so the lanes of a step
// write neighbouring bytes.  Exactly Ta Tb bytes per pair.
//
// Backtrack (k_dtw_backtrack): one wave per pair.  Lane 0 walks the codes from (Ta-1, Tb-1) to (0, 0), one dependent load per step, and
// writes the cells in reverse; then the wave turns them round into `path` and fills a2b from the path's own neighbours.  Row 0 forces a left
// step and column 0 an up step, so the walk ends after at most Ta + Tb - 1 cells whatever the codes hold (non-finite input).
//
// No atomics, no workgroup waits for another.  LDS: 32 KiB (edge) + 16 KiB (line) = 48 KiB per workgroup.
#include "zvx_kernels.h"
#include <cmath>

namespace zvx {

__device__ __forceinline__ long dtw_diag_off(int s, int Ta, int Tb) {
    const long m = Ta < Tb ? Ta : Tb, M = Ta < Tb ? Tb : Ta;
    if (s <= m) return (long)s * (s + 1) / 2;
    if (s <= M) return m * (m + 1) / 2 + (long)(s - m) * m;
    const long r = (long)Ta + Tb - 1 - s;
    return (long)Ta * Tb - r * (r + 1) / 2;
}
__device__ __forceinline__ long dtw_cell(int i, int j, int Ta, int Tb) {
    const int s = i + j, lo = s - (Tb - 1);
    return dtw_diag_off(s, Ta, Tb) + (i - (lo > 0 ? lo : 0));
}

// DP: the columns a lane keeps; MAXL: the most lanes of the workgroup (32 columns at 1024 lanes would not fit the 128 registers a lane has there)
template <int DP, int MAXL>
__global__ __launch_bounds__(MAXL) void k_dtw_forward(DtwArgs g) {
    __shared__ double edge[DTW_MAX_T];
    __shared__ double line[2][DTW_MAX_LANES];
    const DtwPair p = g.pairs[blockIdx.x];
    const int W = (int)blockDim.x, l = (int)threadIdx.x, Ta = p.Ta, Tb = p.Tb, dim = g.dim;
    unsigned char* dir = g.dir + p.dir_off;
    for (int i0 = 0; i0 < Ta; i0 += W) {
        const int n = Ta - i0 < W ? Ta - i0 : W, i = i0 + l;
        const bool row = l < n;
        float ar[DP];
#pragma unroll
        for (int k = 0; k < DP; k++) ar[k] = (row && k < dim) ? p.a[(long)i * dim + k] : 0.f;
        double left = INFINITY, diag = INFINITY, d_cur = 0.0;
        float bq[DP];                                        // row j + 1 of b, loaded one step before its distance is formed
#pragma unroll
        for (int k = 0; k < DP; k++) bq[k] = 0.f;
        // The distance of a cell does not depend on its neighbours, so it is formed one step ahead of the cell and its row of b is loaded two
        // steps ahead: between two barriers only the LDS read, the minimum, the addition and the stores wait for each other.  Steps -2 and -1
        // fill that pipeline.
        const int steps = n + Tb - 1;
        for (int s = -2; s < steps; s++) {
            const int j = s - l;
            if (row && j >= 0 && j < Tb) {
                double up = INFINITY;
                if (l > 0) up = line[s & 1][l - 1];
                else if (i0 > 0) up = edge[j];
                double best = diag;
                unsigned char code = 0;
                if (up < best) { best = up; code = 1; }
                if (left < best) { best = left; code = 2; }
                const double cur = (i | j) ? d_cur + best : d_cur;
                dir[dtw_cell(i, j, Ta, Tb)] = code;
                line[(s + 1) & 1][l] = cur;
                if (l == n - 1) edge[j] = cur;
                if (i == Ta - 1 && j == Tb - 1) g.cost[blockIdx.x] = cur;
                diag = up; left = cur;
            }
            if (row && j + 1 >= 0 && j + 1 < Tb) {           // d(i, j + 1) from the row loaded in the step before
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < DP; k++) {
                    const double df = (double)ar[k] - (double)bq[k];
                    acc = fma(df, df, acc);
                }
                d_cur = sqrt(acc);
            }
            if (row && j + 2 >= 0 && j + 2 < Tb) {
                const float* br = p.b + (long)(j + 2) * dim;
#pragma unroll
                for (int k = 0; k < DP; k++) bq[k] = k < dim ? br[k] : 0.f;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void k_dtw_backtrack(DtwArgs g) {
    __shared__ int len_s;
    const DtwPair p = g.pairs[blockIdx.x];
    const int Ta = p.Ta, Tb = p.Tb, lane = (int)threadIdx.x;
    const unsigned char* dir = g.dir + p.dir_off;
    int* rev = g.rev + 2 * p.path_off;
    int* path = g.path + 2 * p.path_off;
    int* a2b = g.a2b + 2 * p.a2b_off;
    if (lane == 0) {
        int i = Ta - 1, j = Tb - 1, n = 0;
        for (;;) {
            rev[2 * n] = i; rev[2 * n + 1] = j; n++;
            if (!(i | j)) break;
            const int code = i == 0 ? 2 : j == 0 ? 1 : (int)dir[dtw_cell(i, j, Ta, Tb)];
            if (code != 2) i--;
            if (code != 1) j--;
        }
        len_s = n;
        g.path_len[blockIdx.x] = n;
    }
    __syncthreads();
    const int L = len_s;
    for (int q = lane; q < L; q += 64) {
        const int r = L - 1 - q, i = rev[2 * r], j = rev[2 * r + 1];
        path[2 * q] = i; path[2 * q + 1] = j;
        if (q == 0 || rev[2 * (r + 1)] != i) a2b[2 * i] = j;
        if (q == L - 1 || rev[2 * (r - 1)] != i) a2b[2 * i + 1] = j;
    }
}

// one thread per (row, frame, coefficient); frames past a row's own count are written as 0
__global__ __launch_bounds__(256) void k_cepstra(const float* mel, int Tp, const int* frames, int B, int M, int n_cep, const double* table, double scale,
                                                 float* cep) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * Tp * n_cep;
    if (idx >= total) return;
    const int k = (int)(idx % n_cep);
    const long bt = idx / n_cep;
    const int t = (int)(bt % Tp), b = (int)(bt / Tp);
    float out = 0.f;
    if (t < frames[b]) {
        const float* L = mel + bt * M;
        const double* c = table + (long)k * M;
        double acc = 0.0;
        for (int m = 0; m < M; m++) acc = fma((double)L[m], c[m], acc);
        out = (float)(scale * acc);
    }
    cep[idx] = out;
}

void launch_dtw_forward(const DtwArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.B), block((unsigned)a.lanes);
    if (a.dim <= 4) hipLaunchKernelGGL((k_dtw_forward<4, DTW_MAX_LANES>), grid, block, 0, s, a);
    else if (a.dim <= 8) hipLaunchKernelGGL((k_dtw_forward<8, DTW_MAX_LANES>), grid, block, 0, s, a);
    else if (a.dim <= 16) hipLaunchKernelGGL((k_dtw_forward<16, DTW_MAX_LANES>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_dtw_forward<32, DTW_MAX_LANES / 2>), grid, block, 0, s, a);
}

void launch_dtw_backtrack(const DtwArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_dtw_backtrack, dim3((unsigned)a.B), dim3(64), 0, s, a);
}

void launch_cepstra(const float* mel, int Tp, const int* frames, int B, int M, int n_cep, const double* table, double scale, float* cep, hipStream_t s) {
    const long total = (long)B * Tp * n_cep;
    hipLaunchKernelGGL(k_cepstra, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mel, Tp, frames, B, M, n_cep, table, scale, cep);
}

}  // namespace zvx
