// watermark_kernels.h -- launch arguments and launchers of the keyed audio watermark and its detector (watermark.hip), on top of the
// denoiser's (zvx_kernels.h: DenoiseArgs, launch_denoise_ola).
#pragma once
#include "zvx_kernels.h"

namespace zvx {

// Keyed audio watermark (include/zvx.h, zvx_watermark, zvx_watermark_detect; watermark.hip): a multiplicative spread-spectrum mark on the
// denoiser's frame grid.  The embedder is the denoiser's frames kernel with a keyed gain in place of the bias gain -- the row table, the
// window, the slot rule and the overlap-add launch (launch_denoise_ola on `dn`) are the denoiser's own; `dn.copy` is depth_db == 0.
// `sign` is the P x J pattern of +1 / -1 bytes, built on the host -- or a stack [n_tables][P][J] of them built by launch_wm_signs, row b
// reading table sign_of_row[b] (zvx_watermark_rows: a key per row, rows of equal keys share a table); band j is bins
// [k_lo + j KB, k_lo + (j + 1) KB); frame f of the SIGNAL is in block (f / TB) mod P, f formed in 64 bits from the row's f_first.
struct WatermarkArgs {
    DenoiseArgs dn;                          // rows, geometry, tables; bias / strength / floor / mag are not read
    const signed char* sign;                 // [n_tables][P][J]
    const int* sign_of_row;                  // [B] on the device: the table of each row; nullptr: table 0 for every row
    int k_lo, KB, J, TB, P;
    float g_up, g_dn;
};
void launch_watermark_frames(const WatermarkArgs& a, hipStream_t s);
// Sign tables on the device: sign(t, c, j) = +1 where bit 63 of mix64(keys[t] ^ ((uint64)c << 32 | j)) is set, else -1 (mix64: the
// splitmix64 finaliser of include/zvx.h, in 64-bit integer arithmetic), for t < n, c < P, j < J.  out: [n][P][J] bytes of +1 / -1 (the
// embedder's form), or with `packed` [n][P][wm_sign_words(J)] 32-bit words, bit j % 32 of word j / 32 set for +1 (the form
// launch_wm_search_keys reads).  keys and out on the device.
inline int wm_sign_words(int J) { return (J + 31) / 32; }
void launch_wm_signs(const unsigned long long* keys, void* out, int n, int P, int J, bool packed, hipStream_t s);
// The detector, whole rows only.  launch_wm_bands: frame load, forward FFT, Pw = re^2 + im^2, LB[f][j] = sum over the band's bins of
// log2(max(Pw, 1e-6)), D[f][j] = LB[f][j] - (LB[f][j - 1] + LB[f][j + 1]) / 2 -> the row's d[F][J - 2] (column j - 1); no spectrum goes to
// memory.  grid = (ceil(Fmax / frames per workgroup), B).
// launch_wm_search: one workgroup per (window, row).  Window w is frames [w (WF / 2), min(w (WF / 2) + WF, F)) (WF == 0: the row).  For
// each of the TB phases ph the blocks' sums E[m][j] (block m = (f + ph) / TB) are folded by m mod P into a table in LDS, WM_TABLE floats,
// a run of bands at a time; the shift s then costs one pass over the table, and offset o = ph + TB s.  The denominator sum E^2 is formed
// per phase from the unfolded E.  -> win_score[b][w] = the largest z, win_offset[b][w] = the smallest o that attains it, for w below the
// row's window count (wm_windows), nothing elsewhere.  grid = (NW, B).
constexpr int WM_TABLE = 12288;
constexpr int WM_MAX_BANDS = 512, WM_MAX_PERIOD = 256;
struct WmDetectRow { const float* x; float* d; int n, F; };
struct WmDetectArgs {
    const WmDetectRow* rows;                 // [B], on the device
    int B;
    int n_fft, log2n, hop, pad, Fmax;
    const float* twid; const float* win;     // the denoiser's tables
    const signed char* sign;                 // [P][J]
    int k_lo, KB, J, TB, P;
    int WF, NW;                              // NW: the most windows of a row (the grid; the pitch of the results)
    float* win_score; int* win_offset;       // [B][NW]
};
// the windows of a row of F frames: 0 for none, 1 where WF == 0 or F <= WF, else 1 + ceil((F - WF) / (WF / 2)) (the last one clipped)
__host__ __device__ inline int wm_windows(int F, int WF) {
    if (F <= 0) return 0;
    if (WF <= 0 || F <= WF) return 1;
    const int H = WF / 2;
    return 1 + (F - WF + H - 1) / H;
}
void launch_wm_bands(const WmDetectArgs& a, hipStream_t s);
void launch_wm_search(const WmDetectArgs& a, hipStream_t s);
// The search over K keys at once (zvx_watermark_identify): sign_bits is the packed stack [K][P][wm_sign_words(J)] (d.sign is not read),
// d.win_score / d.win_offset are [B][NW][K]; the
// entry (b, w, k) receives bit for bit what launch_wm_search writes to (b, w) with table k.  One workgroup per (window, row, run of
// WM_KEYS keys): the folded table and the denominator of a phase are built once for the run, then each key has its own shift pass.
// grid = (NW, B, ceil(K / WM_KEYS)).
constexpr int WM_KEYS = 8;
struct WmKeysArgs { WmDetectArgs d; const unsigned* sign_bits; int K; };
void launch_wm_search_keys(const WmKeysArgs& a, hipStream_t s);

}  // namespace zvx
