// zvx_kernels.h -- launcher declarations for the gfx950 kernels of libzvx.
// Activations are time-major [row = time][channel] in HBM, fp32 or bf16 (precision mode).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <set>
#include <utility>

// Per-launch timing without marker packets: when the caller has armed a pair of events (profile_events), the dispatch itself
// carries them (hipExtLaunchKernelGGL start / stop events = the kernel's own begin / end timestamps).  ONE thread-local pair serves
// every launcher (defined in gemm.hip); each launcher dispatches through ZVX_DISPATCH, and a dry run never reads the pair.
extern thread_local hipEvent_t zvx_gemm_ev_start, zvx_gemm_ev_stop;
#define ZVX_DISPATCH(kernel, grid, block, lds, stream, ...) \
    do { if (zvx_gemm_ev_start) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, zvx_gemm_ev_start, zvx_gemm_ev_stop, 0, __VA_ARGS__); \
         else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); } while (0)

namespace zvx {

// arm (or disarm with nullptrs) the pair of events that the NEXT dispatch of a launch_gemm / launch_resfuse / launch_rb2fuse /
// launch_resstream / launch_pairstream / launch_narrowstage carries as its own start / stop timestamps
inline void profile_events(hipEvent_t start, hipEvent_t stop) { zvx_gemm_ev_start = start; zvx_gemm_ev_stop = stop; }

typedef unsigned short bf16_t;   // raw bf16 bits

enum DType { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };   // DT_F16: IEEE half activations + weights of the StyleTTS decoder (11-bit significand: 8x
                                                        // smaller rounding error than bf16 at the same MFMA rate; every value there is O(1) behind a norm)
static inline size_t dtype_size(int dt) { return dt == DT_F32 ? 4 : 2; }
// compute units of the current device, read once (a function-local static: initialisation is thread-safe -- several contexts may be
// driven from several host threads)
inline int num_cus() {
    static const int n = [] { int dev = 0, v = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256; return v; }();
    return n;
}
// CUs the PERSISTENT kernels size their grids for (round 5's spatial split of the chip between the two streams -- ZVX_CU_SPLIT, a
// process-wide override -- measured as a dead end and is gone: DESIGN.md section 4)
inline int persistent_cus() { return num_cus(); }

// Opt-in to more than 64 KiB of dynamic LDS for a kernel: hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of the
// function, so it is set once per (function, device) -- a second context on another device of the same process opts in again.
// false when the runtime refuses (the launcher then declines the shape instead of launching into an error).
inline bool lds_opt_in(const void* kfn) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({kfn, dev})) return true;
    if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;
    done.insert({kfn, dev});
    return true;
}

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_TANH = 3 };

#define ZVX_MAX_TAPS 16

// ------------------------------------------------------------------------------------------------
// Gathered-row GEMM ("conv-GEMM"), the workhorse:
//
//   out[z][r][n] = epilogue( alpha * sum_tap sum_k X[z][rowmap(r, tap)][k] * W[tap][n][k] )
//
// X ("row operand", usually activations) and W ("col operand", usually weights, [tap][N][ldw]) are both
// K-contiguous.  rowmap() implements 1-D convolution taps (dilated Conv1d, polyphase ConvTranspose1d,
// plain Linear with one tap) and 2-D taps with stride (ResNet Conv2d on a [H][W][C] map):
//     r -> (u, v) = (r / wout, r % wout);  in_u = u*stride + du[tap];  in_v = v*stride + dv[tap]
//     valid iff 0 <= in_u < hin and 0 <= in_v < in_len[z];  X row = in_u*win + in_v  (else zero)
// Both operands may be batched (z = batch*nheads + head) with batch and head strides, which also covers
// Q.K^T and P.V of the attention (W := K or V^T of that (utterance, head)).
// ------------------------------------------------------------------------------------------------
struct GemmArgs {
    // operands
    const void* X; long x_bs, x_hs; int ldx;
    const void* W; long w_bs, w_hs, w_ts; int ldw;
    const void* Wp;            // optional: W pre-packed in MFMA-fragment order (launch_pack_weights) -> conv-slab kernel
    int halo_l, halo_r;        // filled by the launcher
    // fused ResBlock1 pair (resfuse kernel): out = epilogue(conv2(lrelu(conv1(X) + bias1)) + bias + inverse_lrelu(X))
    const void* Wp2; const float* bias1; int dv1[ZVX_MAX_TAPS]; int fused; float slope1;   // conv1: Wp2/bias1/dv1 (dilated); conv2: Wp/bias/dv
    int no_pairstream;         // fused: 1 = never the streaming pair kernel of pairstream.hip (the bit-equality reference), 2 = use it even for small jobs (tests)
    int dtype;                 // DType of X and W (same)
    int M, N, K;               // M = max rows per z, N cols, K per tap (multiple of 8 elements bf16 / 4 f32)
    int nbatch, nheads;
    const int* in_len;         // [nbatch] valid input width (1-D: valid rows of X); NULL -> in_len_static
    const int* out_len;        // [nbatch] valid output width (1-D: valid rows of out); NULL -> M
    const int* k_len;          // [nbatch] per-batch K (rounded up to 8 internally); NULL -> K
    int in_len_static;
    // row map
    int ntaps; int du[ZVX_MAX_TAPS], dv[ZVX_MAX_TAPS];   // int (not short): uniform-indexed kernarg reads become s_load
    int stride, wout, hin, win; // wout <= 0 -> 1-D (u = 0, v = r)
    // Filled by launch_gemm when a stride-1 2-D convolution over [hin][win] maps is run on the 1-D conv-slab / conv-reg kernels as a
    // convolution over the FLATTENED map (tap offset du * win + dv): input row g is valid iff 0 <= g < flat_rows and
    // (g % flat_win) < in_len[z] (the columns of an utterance's true width); every output row of the map is written
    int flat_win, flat_rows;
    // Batch-flattened 1-D convolution (conv-slab kernel only; a HINT: every other kernel ignores it and runs the per-utterance
    // launch the other fields describe).  The nbatch utterances lie `bflat` rows apart in X, out and res (x_bs = bflat * ldx,
    // o_bs = bflat * ldo, r_bs = bflat * ldr) with bflat >= M + max |tap offset|, so the batch is ONE row axis of nbatch * bflat
    // rows: row tiles run across utterance boundaries (no half-empty last tile per utterance: 896 frames are 3.5 tiles of 256),
    // rows g with (g % bflat) >= in_len[g / bflat] are staged as zeros.  EVERY row of the flattened axis is written (rows past an
    // utterance's length receive finite-or-not junk): every consumer of such a tensor masks by the utterance lengths on the way in.
    int bflat;
    // Second source (conv-slab kernel only): out += X2 . W2^T, a 1-tap product over K2 more input channels accumulated into the SAME
    // f32 accumulators after the K chunks of X -- a residual block's 1x1 shortcut convolution inside its last k = 3 convolution
    // (styletts.py:60-68: (conv2(.) + conv1x1(x)) / sqrt(2)).  X2 rows map like X rows (same batch stride rule under bflat); Wp
    // is then the COMBINED fragment stream: per 32-channel tile the fragments of W, then those of W2 (pack_weights_pair).
    const void* X2; long x2_bs; int ldx2, K2;
    int xcd_flat;                                                  // conv-slab: remap over the WHOLE grid (batch x tiles), not per utterance (zvx_set_int "slab_flat"; the context's switch)
    int slab_small;                                                // conv-slab tile choice for single requests (zvx_set_int "slab_small"; the context's switch): 0 none, 1 small row tiles, 2 + 32-channel tiles
    int out_split3;            // f32 result written as 16-bit split planes [hi | hi | lo] (row = 3 N, ldo elements apart): the input of the next 3-plane GEMM; 1 = bf16, 2 = IEEE half (lo x 2^11)
    // epilogue: v = alpha*acc + bias; v += res; v += accum; [accum = v]; v *= out_scale; v = act(v);
    //           v = v*post_scale[n] + post_shift[n]; out = (T)v
    float alpha;
    const float* bias; int bias_mode;            // 0 none, 1 per n, 2 per row r
    const void* res; long r_bs, r_hs; int ldr; int res_dtype; int res_mode;  // 0 none, 1 raw, 2 inverse leaky-relu
    float res_inv_slope;                         // res_mode 2: x = y >= 0 ? y : y * res_inv_slope
    void* accum; long a_bs; int lda; int accum_mode;   // bit0: v += accum, bit1: accum = v (after add)
    int accum_dtype;                             // DT_F32 / DT_BF16 storage of the running sum
    float out_scale;
    int act; float slope;
    const float* post_scale; const float* post_shift;
    void* out; long o_bs, o_hs; int ldo; int out_dtype;   // out may be NULL (accum only)
    // squeeze-excite pool fused into the persistent 2-D convolution (conv2d_persist_kernel, MODE 0): partial sums over the valid
    // positions of the f32 results before the bias, [nbatch][S][N]; the launcher writes S to *se_part_S (a HOST int the caller
    // zeroed) when the launch it chose fills them -- otherwise the caller runs the pool pass (launch_se_pool)
    float* se_part; int* se_part_S;
    // level transition of the speaker encoder in one launch (conv2d_s2_kernel): besides the 3 x 3 / stride-2 convolution these
    // arguments describe, the block's 1 x 1 / stride-2 shortcut convolution of the SAME input: packed weights [1][N][K], bias [N],
    // 16-bit output laid out like `out`.  launch_gemm returns -7 when the shape is not covered (probe with gemm_variant_of).
    void* ds_out; const void* ds_Wp; const float* ds_bias;
    // accounting
    double flops;              // algorithmic FLOPs of this launch (filled by the launcher)
};

// Returns the kernel-variant id used (index into gemm_variant_name) or <0 on error.
int launch_gemm(const GemmArgs& a, hipStream_t stream);
// the kernel variant launch_gemm / launch_resfuse would pick for these arguments (nothing is dispatched)
int gemm_variant_of(const GemmArgs& a);
// the compile-time epilogue a conv-slab launch of these arguments selects (ZVX_EPI / ZVX_EPI_DEC / ZVX_EPI_FLIP of gemm.hip), -1 = the
// run-time epilogue.  Which tiles have the compile-time form is launch_convslab's choice; this is the mode it asks them for.
int gemm_epi_mode_of(const GemmArgs& a);
// fused HiFi-GAN ResBlock1 pair (conv1 -> lrelu -> conv2 -> + x) for C = 32 / 64 bf16; -1 if the shape is not covered
int launch_resfuse(GemmArgs a, hipStream_t stream);
// fused HiFi-GAN ResBlock2 (two dilated convolutions with their residuals, hifigan.py:77-82) for C = 32 / 64, k = 3 / 5 / 7; -1 if not covered
int launch_rb2fuse(GemmArgs a, hipStream_t stream);
// fragment-order packing of a bf16 weight [ntaps][N][K] for the conv-slab kernel
size_t packed_weight_elems(int ntaps, int N, int K);
// combined stream of two packed weights with the same N (GemmArgs::X2): per 32-channel tile the fragments of A, then those of B
void launch_pack_pair(const void* packedA, int ntapsA, int KA, const void* packedB, int ntapsB, int KB, int N, void* out, hipStream_t s);
void launch_pack_weights(const void* w_bf16, int ntaps, int N, int K, void* out, hipStream_t s);
const char* gemm_variant_name(int id);
int gemm_num_variants();

// ------------------------------------------------------------------------------------------------
// Streaming ResBlock1 chain (resstream.hip): up to three (dilated conv -> lrelu -> conv -> + x) pairs of one HiFi-GAN
// ResBlock (hifigan.py:49-56) in ONE launch for C = 32 / 64.  Every intermediate tensor lives in LDS ring buffers; the
// stage tensor is read once and the result (next input, running sum xs, or the stage mean) written once.
// ------------------------------------------------------------------------------------------------
struct StreamArgs {
    const void* X; long x_bs; int ldx;             // stage input [b][M][ldx] bf16, activated domain (lrelu(x))
    const void* W1[3]; const void* W2[3];          // fragment-packed bf16 weights of pair t: conv1 (dilated), conv2 (dilation 1)
    const float* b1[3]; const float* b2[3];
    int dil[3];
    int C, ntaps, npair;
    void* out; long o_bs; int ldo;                 // bf16 output, activated with `slope` (NULL: running sum only)
    void* accum; long a_bs; int lda; int accum_mode;   // bf16 running sum xs: bit0 v += xs, bit1 xs = v
    float slope1, res_inv_slope, out_scale, slope; // slope1: lrelu between the convs; slope: output activation (1 = none)
    const int* len; int M, nbatch;                 // valid rows per utterance (NULL -> M)
    int S, nseg;                                   // filled by the launcher: rows per segment, segments per utterance
    int dX0, dT, dX[3];                            // filled by the launcher: ring sizes in rows
    double flops;                                  // filled by the launcher
    long long* prof;                               // RS_PROFILE builds: per-wave cycle counters of workgroup 0
    int seg_min;                                   // 0: segments as short as 256 rows when the job cannot fill the chip; < 0: never below 2048 (A/B)
    int f16;                                       // the 16-bit tensors (x, rings, weights, xs, output) are IEEE half instead of bf16
};
// variant id (index into gemm_variant_name) or -1 when the shape is not covered; dry_run: decide only, launch nothing
int launch_resstream(StreamArgs a, hipStream_t stream, bool dry_run);

// ------------------------------------------------------------------------------------------------
// Streaming ResBlock1 PAIR for the wide stages (pairstream.hip): x' = conv2(lrelu(conv1_dilated(x_act) + b1)) + b2 + x in ONE
// launch for C = 128 (hifigan.py:51-55).  conv1 and conv2 are two wave groups of a persistent workgroup that walk a segment
// of one utterance in 128-row steps; T = lrelu(conv1) lives only in an LDS ring, weights stream through per-wave register rings.
// ------------------------------------------------------------------------------------------------
struct PairArgs {
    const void* X; long x_bs; int ldx;             // stage input [b][M][ldx] bf16, activated domain; also the residual
    const void* W1; const void* W2;                // fragment-packed bf16 weights: conv1 (dilated), conv2 (dilation 1)
    const float* b1; const float* b2;
    int C, ntaps, dil;
    void* out; long o_bs; int ldo;                 // bf16 output activated with `slope` (NULL: running sum only)
    void* accum; long a_bs; int lda; int accum_mode;   // bf16 running sum xs: bit0 v += xs, bit1 xs = v
    float slope1, res_inv_slope, out_scale, slope; // slope 1 = no output activation
    const int* len; int M, nbatch;
    int force;                                     // 1: also for jobs below the size where the kernel pays (tests)
    int f16;                                       // the 16-bit tensors (x, T, weights, xs, output) are IEEE half instead of bf16
    int S, nseg, DX, DT, G0;                       // filled by the launcher: segment rows, segments per utterance, ring rows
    long long* prof;                               // PS_PROFILE builds: [8 waves][main, epilogue, barrier, -] cycle totals of workgroup 0
};
// true when the shape is covered (and, unless dry_run, launched); ev_start / ev_stop: optional dispatch-carried events
bool launch_pairstream(PairArgs a, hipStream_t stream, bool dry_run);

// ------------------------------------------------------------------------------------------------
// A whole narrow HiFi-GAN stage (narrowstage.hip): the nk ResBlock1 blocks (three dilated pairs each) of a stage with C = 16 / 8
// channels, their sum / nk and the next stage's input activation in ONE launch; every intermediate lives in LDS, the stage tensor
// crosses HBM once in and once out (hifigan.py:116-125; HiFi-GAN V2's last two stages).
// ------------------------------------------------------------------------------------------------
struct StageArgs {
    const void* X; long x_bs; int ldx;             // stage input [b][M][C] 16-bit, activated domain (lrelu(x, 0.1))
    const void* W;                                 // weight fragments in this kernel's own order (launch_pack_narrow): conv 6 j + 2 t + {0: conv1, 1: conv2}
    int woff[18];                                  // first 1-KiB fragment of each convolution in W
    const float* bias;                             // [6 nk][C], same convolution order
    int C, nk, ks[3], dil[3][3];
    void* out; long o_bs; int ldo;                 // lrelu(mean over the ResBlocks, slope) [b][M][C] 16-bit
    float slope1, res_inv_slope, slope;
    const int* len; int M, nbatch;
    int f16;                                       // the 16-bit tensors are IEEE half instead of bf16
};
bool launch_narrowstage(const StageArgs& a, hipStream_t stream, bool dry_run);
int narrowstage_steps(int C, int k);               // 1-KiB fragments per convolution
void launch_pack_narrow(const void* w16 /*[k][C][C] 16-bit*/, int k, int C, void* out, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Fused attention of the FS2 / SCLN decoder (attention.hip): out = softmax(Q K^T * scale, keys < len) V per (utterance, head),
// bf16 operands, no [L][L] tensor in HBM.  Q and K live in one projection buffer (K at element offset k_off of a row), V
// arrives TRANSPOSED ([head*D + j][key], key-contiguous) from its projection GEMM.
// ------------------------------------------------------------------------------------------------
struct FlashArgs {
    const void* qk; long qk_bs; int ldq; int k_off;     // [b][L][ldq] bf16: Q at column h*D, K at column k_off + h*D
    const void* vt; long vt_bs; int ldv;                 // [b][nheads*D][ldv] bf16 (ldv >= L rounded up to 8)
    void* out; long o_bs; int ldo;                       // [b][L][ldo] bf16, head h at column h*D
    const int* len; int L, D, nheads, nbatch;
    float scale;                                         // 1 / sqrt(D)   (fs2.py:49-50)
    int f16;                                             // the 16-bit tensors are IEEE half instead of bf16
    long long* prof;                                     // FA_PROFILE builds (tools/micro/fa_bench.hip): per-phase cycle totals of workgroup 0, wave 0
};
bool launch_flash_attention(const FlashArgs& a, hipStream_t stream, bool dry_run);
// exact-f32 fused attention of the phoneme encoder: Q | K | V columns of one projection buffer, head h at column off + h*D
struct AttnF32Args {
    const float* qkv; long bs; int ld; int q_off, k_off, v_off;   // [b][L][ld] f32
    float* out; long o_bs; int ldo;                               // [b][L][ldo] f32, head h at column h*D
    unsigned short* planes; int planes_C;                         // optional: the result also as 16-bit split planes [hi | hi | lo], rows of 3 planes_C
    int planes_f16;                                               // planes in IEEE half (lo scaled by 2^11) instead of bf16
    const int* len; int L, D, nheads, nbatch;
    float scale;
};
bool launch_attention_f32(const AttnF32Args& a, hipStream_t stream, bool dry_run);
// (both attention launches are plain dispatches: the caller records its events around the call)

// ------------------------------------------------------------------------------------------------
// Leveler (ops.hip, next to the loudness kernels whose recurrence and staging it shares).  A section of its own: the launchers of the
// section below are the registry of the kernel-level spec tests (tests/ops_ref.py); these three are checked through the C-ABI against
// their float64 restatement (tests/level_ref.py, tests/test_level_gpu.py), as the other post-processing kernels are.
// ------------------------------------------------------------------------------------------------
// K-weighting (zvx_loudness, zvx_level): two biquads in transposed direct form II, double state.  Stage 1 b0..b2, a1, a2; stage 2 has b = [1, -2, 1].
struct LoudCoef { double b0, b1, b2, a1, a2, c1, c2; };
// Leveler (include/zvx.h, zvx_level): a gain curve from the gated short-term loudness of the S units up to and including a unit, a units
// ahead, interpolated linearly between unit nodes.  `rows` is a device table with one LevelRow per row, uploaded by every call through the
// context's pinned staging arena (host_post.hip, run_level_rows); every kernel reads rows[blockIdx.y] at its top and works from it alone, so
// zvx_level, zvx_level_ex and zvx_level_rows run the same instructions.  A row holds samples [in_origin, in_origin + n) of its signal; the
// unit grid is the SIGNAL's (unit q = samples [q h, (q + 1) h)).  Positions on the signal are 64-bit throughout; what indexes memory is
// the position minus in_origin (samples) or minus q_first (units).  Nothing outside [0, n) of a row is read.
constexpr int LEVEL_TILE = 4096;             // emitted samples per workgroup of launch_level_apply: 4 groups of 4 per thread
constexpr int LEVEL_MAX_S = 600;             // the longest window, in units (include/zvx.h: ZVX_E_UNSUPPORTED beyond)
constexpr int LEVEL_MIN_H = 400;             // h at the lowest rate (4000 Hz): a tile spans at most LEVEL_TILE / 400 + 2 units
constexpr int LEVEL_NODES = LEVEL_TILE / LEVEL_MIN_H + 4;    // unit nodes a tile can touch (12 units incl. the alignment shift, + 1, rounded up)
struct LevelRow {
    const float* x; void* out; double* p;    // the row's samples; where emitted sample `off` goes (f32 or int16); p[q - q_first], the needed units
    long in_origin;                          // the signal position of x[0]
    long q_first, q_last;                    // the needed units [q_first, q_last] (q_last < q_first: none)
    long U;                                  // the window is last: the signal's whole units (in_origin + n) / h, the clamp of the nodes;
                                             // otherwise LEVEL_OPEN (the signal continues: nothing clamps on the right)
    int n, off, cnt, pad_;                   // the row's length; the emitted range [off, off + cnt) of the row
};
constexpr long LEVEL_OPEN = 0x7fffffffffffffffL;
struct LevelArgs {
    const LevelRow* rows;                    // [B], on the device
    int B;
    int h, S, a;                             // samples per unit; window and look-ahead in units
    LoudCoef k;
    double gate;                             // 10^((-70 + 0.691) / 10): a unit counts where p > gate
    double target, gmax;                     // target_lufs; 10^(max_gain_db / 20), computed on the host in double
    int pcm16;
    float* part_lo; float* part_hi; int ppitch;      // [b][tile]: min / max of g32 over the tile's emitted samples (+INF / -INF where it has none)
    float* res;                              // launch_level_reduce: res[b] = gain_lo, res[B + b] = gain_hi (1 and 1 for an empty range)
};
// p of every needed unit: one LANE per unit, the recurrence of launch_loud_units (zero state two units early, the same fma chain, the same
// staging of 16-byte groups aligned as ADDRESSES through LDS) over samples read relative to in_origin; zeros stand where the position lies
// outside the row, which the host's checks (the support condition, and the oldest unit of a last window whose nodes are clamped) confine to
// the front of sample 0.  grid.x covers units_max units.
void launch_level_units(const LevelArgs& a, long units_max, hipStream_t s);
// one tile of a row's emitted range: the p the tile's nodes need are staged in LDS, one thread per node forms its G (gated ascending sum,
// log10 / pow in double), every sample takes g = fma(T[q + 1] - T[q], frac, T[q]), rounds it to f32 and multiplies once.  Groups of 4
// aligned as ADDRESSES of the destination, 16-byte loads where the source address allows; a thread reads its samples before it writes them
// and no other thread touches them: safe in place (off = 0).  grid.x = ppitch tiles over cnt_max.
void launch_level_apply(const LevelArgs& a, hipStream_t s);
// one workgroup per row over the tiles' partial results
void launch_level_reduce(const LevelArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Programme loudness report (ops.hip, behind the loudness kernels whose unit powers it reads).  A section of its own, as the leveler's:
// its two launchers are checked through the C-ABI against their float64 restatement (tests/loudness_stats_ref.py,
// tests/test_loudness_stats_gpu.py), as the other post-processing kernels are.
// ------------------------------------------------------------------------------------------------
// include/zvx.h, zvx_loudness_stats: momentary and short-term loudness and the loudness range of EBU Tech 3342 from the unit powers
// launch_loud_units left, LoudArgs (below) describes.  Row b has U = nsamples[b] / h units, U - 3 blocks and W = U - 29 short-term windows.
constexpr int LOUD_ST_UNITS = 30;            // units of a short-term window: 3 s
enum { LOUD_RES_MOM_MAX = 0, LOUD_RES_SHORT_MAX, LOUD_RES_REL_THR, LOUD_RES_GATED, LOUD_RES_RANK_LO, LOUD_RES_RANK_HI, LOUD_RES_POW_LO,
       LOUD_RES_POW_HI, LOUD_RES_WORDS };
struct LoudStatsArgs {
    const double* unit; long upitch; const int* nsamples; int B;     // LoudArgs' units, lengths and rows
    int h;
    double abs_gate;                         // LoudArgs' constant
    double* win; long wpitch;                // win[b][j]: the power s[j] of short-term window j < W
    double* mom; double* sht; long cpitch;   // the LUFS curves M[j], j < U - 3, and S[j], j < W, [b][cpitch]; NULL: not asked for
    // res[b][LOUD_RES_WORDS]: max M and max S in LUFS (-INFINITY without one), the relative gate 0.01 Gamma as a power, n_g and the two
    // nearest-rank indices as whole doubles, the powers of those ranks (0 where n_g == 0)
    double* res;
};
// one workgroup per row: s[j] into win, the curves where asked for, the two maxima, both LRA gates in the fixed order of wg_sum_f64 ->
// res[b][0 .. 5], and zeros into the two powers
void launch_loud_windows(const LoudStatsArgs& a, hipStream_t s);
// selection without a sort, grid (ceil(w_max / 256), B): thread j counts the gated windows that precede its own in (power, index) order,
// streaming win[b] through LDS tiles; the one thread whose count is a target rank stores its power.  No atomics, no workgroup that waits.
void launch_loud_rank(const LoudStatsArgs& a, long w_max, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Pitch report (ops.hip, behind the loudness report).  A section of its own, as the two above: its three launchers are checked through the
// C-ABI against their float64 restatement (tests/pitch_ref.py, tests/test_pitch_gpu.py).
// ------------------------------------------------------------------------------------------------
// include/zvx.h, zvx_pitch: YIN on a frame grid.  `rows` is a device table with one PitchRow per row, uploaded by every call through the
// context's pinned staging arena; every kernel reads rows[blockIdx.y] at its top and works from it alone.  Nothing outside [0, n) of a
// row is read; positions on a row are 64-bit.
constexpr int PITCH_MAX_W = 4096;            // the longest window, in samples (include/zvx.h: ZVX_E_UNSUPPORTED beyond)
constexpr int PITCH_MAX_TAU = 2048;          // the longest lag: 8 lags per lane
constexpr int PITCH_MAX_G = 8;               // frames per workgroup at the most
constexpr int PITCH_SPAN = PITCH_MAX_W + PITCH_MAX_TAU;      // staged doubles at the most: G is the largest with (G - 1) H + W + tau_max <= this
enum { PITCH_RES_VOICED = 0, PITCH_RES_MEAN, PITCH_RES_RANK_MED, PITCH_RES_RANK_LO, PITCH_RES_RANK_HI, PITCH_RES_MED, PITCH_RES_LO,
       PITCH_RES_HI, PITCH_RES_WORDS };
struct PitchRow {
    const float* x;                          // the row's samples
    float* f0; float* aper;                  // the row's curves in device staging, F entries each
    int n, F;                                // samples; frames = n / H
};
struct PitchArgs {
    const PitchRow* rows;                    // [B], on the device
    int B;
    int W, H, tau_min, tau_max, c;           // window, hop, the lag range, the centring offset (W + tau_max) / 2
    int G, span;                             // frames per workgroup; (G - 1) H + W + tau_max
    double fs, threshold, gate;              // the rate; the threshold on d'; 10^(gate_db / 10), computed on the host in double
    // res[b][PITCH_RES_WORDS]: n_v, the mean of the voiced f0, the three nearest-rank indices as whole doubles, the f0 of those ranks (0
    // where n_v == 0)
    double* res;
};
// grid (ceil(f_max / G), B): f0 and aper of G consecutive frames per workgroup.  false where the geometry does not fit or the runtime
// refuses the LDS opt-in; dry_run: those checks (and the opt-in) alone, nothing is launched and `rows` is not looked at
bool launch_pitch_track(const PitchArgs& a, long f_max, hipStream_t s, bool dry_run = false);
// one workgroup per row: n_v, the mean in the fixed order of wg_sum_f64, the rank indices -> res[b][0 .. 4], zeros into the three values
void launch_pitch_stats(const PitchArgs& a, hipStream_t s);
// selection without a sort, as launch_loud_rank: grid (ceil(f_max / 256), B), thread j counts the voiced frames that precede its own in
// (f0, index) order; the one thread whose count is a target rank stores its f0
void launch_pitch_rank(const PitchArgs& a, long f_max, hipStream_t s);

// ---- alignment (include/zvx.h, zvx_dtw / zvx_align_wav; align.hip) ----
constexpr int DTW_MAX_T = 4096;              // frames of one side of a pair
constexpr int DTW_MAX_DIM = 32;              // columns a lane keeps of its row of a
constexpr int DTW_MAX_LANES = 1024;          // rows of a band = threads of the forward workgroup
// one pair: its rows (a: [Ta][dim], b: [Tb][dim], f32, contiguous), and where its part of the call's work buffers starts -- dir_off in
// bytes (Ta Tb of them), path_off in cells of rev / path (Ta + Tb - 1 of them), a2b_off in rows of a2b (Ta of them)
struct DtwPair { const float* a; const float* b; int Ta, Tb; long dir_off, path_off, a2b_off; };
struct DtwArgs {
    const DtwPair* pairs;                    // [B], on the device
    int B, dim, lanes;                       // lanes: a multiple of 64 in [64, DTW_MAX_LANES]; the results do not depend on it
    unsigned char* dir;                      // direction codes, diagonal-major per pair (align.hip)
    double* cost;                            // [B]
    int* path_len;                           // [B]
    int* rev;                                // the path from the end, (i, j) per cell
    int* path;                               // the path from (0, 0)
    int* a2b;                                // (first j, last j) per row of a
};
// the lanes of the forward workgroup: the call's longest Ta rounded up to a wave, at most 1024 (512 above 16 columns: the registers of a lane)
inline int dtw_lanes(int dim, int ta_max) { return std::min(dim > 16 ? DTW_MAX_LANES / 2 : DTW_MAX_LANES, (ta_max + 63) / 64 * 64); }
// grid = B workgroups of `lanes` = dtw_lanes(...) threads: B <= 65535
void launch_dtw_forward(const DtwArgs& a, hipStream_t s);
// grid = B waves; reads dir, writes path_len, rev, path and a2b
void launch_dtw_backtrack(const DtwArgs& a, hipStream_t s);
// cep[b][t][k] = (float)(scale * sum_m mel[b][t][m] table[k][m]) in double for t < frames[b], 0 beyond; mel is [B][Tp][M] f32, table [n_cep][M]
void launch_cepstra(const float* mel, int Tp, const int* frames, int B, int M, int n_cep, const double* table, double scale, float* cep, hipStream_t s);

// ---- equaliser (include/zvx.h, zvx_fir / zvx_fir_ex / zvx_fir_rows; fir.hip) ----
// The equaliser's FIR filter over waveform rows (include/zvx.h, zvx_fir; fir.hip): y[i] = sum_k h[k] x[i + D - k] with a double accumulator
// from +0.0, the terms in ascending k, one rounding to f32.  `rows` is a device table with one FirRow per row -- its input and output
// pointers, its length and its emitted range --, so that the rows of one launch may live in unrelated buffers and sit anywhere on their
// signals; every call uploads one through the context's pinned staging arena (host_post.hip, run_fir_rows).  A windowed row emits the
// samples [off, off + cnt) only and out[e] is output off + e.  Whatever lies outside [0, n) of a row is read as zero: the host's support
// condition (reach K - 1 - D to the left, D to the right) admits only windows in which those are the signal's own zeros.  The kernel reads
// rows[blockIdx.y] at its top and works from it alone: every form of the call runs the same instructions.
// (The descriptor carries no count of true zeros in front of and behind the row, which the design note of this filter listed: the
// support condition is checked on the host before anything is queued, and under it zero outside [0, n) IS the signal, so the two
// counts would never be read.)
// taps: Kp = K rounded up to a multiple of 4 doubles on the device, h[k] converted exactly, zeros behind K.
constexpr int FIR_TILE = 1024;               // emitted samples per workgroup (zvx_get_int("fir_tile"))
constexpr int FIR_MAX_TAPS = 4096;           // ZVX_FIR_MAX_TAPS
struct FirRow {
    const float* x; void* out;               // the row's samples; where emitted sample 0 goes (f32 or int16)
    int n, off, cnt, pad_;                   // the row's length; the emitted range [off, off + cnt)
};
struct FirArgs {
    const FirRow* rows;                      // [B], on the device
    const double* taps;                      // [Kp]
    int B, Kp, D, pcm16;
};
// grid.x covers cnt_max, the longest emitted range; nothing is launched where it is 0
void launch_fir(const FirArgs& a, long cnt_max, hipStream_t s);
// dst[e] = src[e] for e < cnt of every row: the copy-back of the in-place form (the filter reads its neighbours, so it writes a work buffer)
struct FirCopyRow { float* dst; const float* src; long cnt; };
void launch_fir_copy(const FirCopyRow* rows, int B, long cnt_max, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Small kernels (ops.hip).  T-typed pointers are void* + dtype.
// ------------------------------------------------------------------------------------------------
// single requests: InstanceNorm statistics + affine + activation of a 16-bit tensor (x and y both DT_BF16 or DT_F16) in ONE launch
// (bit-identical to the two-kernel path: launch_instnorm_stats + launch_norm_affine_act)
void launch_instnorm_fused(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax, const int* L, int C, float eps,
                           float* mean, float* rstd, const float* gamma, const float* beta, long g_bs, int one_plus, int act, float slope, hipStream_t s);
// 16-bit [b][rows][ld_in] (first C columns) -> [b][C][ld_out] (rows on the fast axis; ld_out >= rows): V -> V^T for the fused attention.
// Every element of [C][ld_out] is written: zeros from row min(len[b], rows) on
void launch_transpose16(const void* in, int ld_in, void* out, int ld_out, int B, int rows, int C, hipStream_t s, const int* len = nullptr);   // rows >= len[b] read as zeros
void launch_f32_to_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s);
// x[b][r][c] = 0 for len[b] <= c < cols; es = element size (2 / 4), ld / bs = row / batch strides in elements
void launch_zero_tail_cols(void* x, int es, long ld, long bs, int B, int rows, int cols, const int* len, hipStream_t s);
void launch_cast(const void* in, int in_dt, void* out, int out_dt, size_t n, hipStream_t s);

// f32 -> three 16-bit planes [hi | hi | lo] per row (out [b][rows_max][3C]; rows >= rows[b] -> zeros) and weights
// [nrows][K] -> [nrows][hi | lo | hi]: an f32-class GEMM as one 16-bit GEMM over 3K (see ops.hip).  f16 = 0: bf16 planes;
// f16 = 1: IEEE-half planes, lo scaled by 2^11, weights scaled by `scale` (a power of two; third plane w * scale * 2^-11)
void launch_split3(const float* x, int ldx, void* out, int B, int rows_max, const int* rows, int C, hipStream_t s, int f16 = 0);
void launch_split3_weights(const float* w, void* out, long nrows, int K, hipStream_t s, int f16 = 0, float scale = 1.f);
void launch_absmax(const float* x, size_t n, float* out /* device, 4 bytes */, hipStream_t s);

// encoder front: out[b][t][:] = cat(emb[ph], pemb[pu]) + pe[t]      (fs2.py:372-392)
void launch_embed(const int* phoneme, const int* puncts, const float* emb, int emb_dim, const float* pemb,
                  int pemb_dim, const float* pe, float* out, int B, int Tmax, const int* T, hipStream_t s);

// Row LayerNorm family over C channels, one wave per row.
//   mode 0: torch LayerNorm (biased var, eps in sqrt), gamma/beta [C]
//   mode 1: SCLN (unbiased std, /(sigma+eps)), bg rows of stride bg_bs: beta = bg[b][0:C], gamma = bg[b][C:2C]  (fs2.py:76-90)
// post_add [B][C] (may be NULL) is added after the affine (the style-embedding add, fs2.py:740-741).
// Rows >= rows[b] of y are not written; split_planes (f32 y only) receives what launch_split3 would write for y, zeros past rows[b] included.
// With C % 8 == 0, C <= 1024 and ldx, ldy multiples of 8 the row is handled as 16-byte vectors: x, y, gamma, beta, bg (bg_bs % 4 == 0) and
// post_add must then be 16-byte aligned; any other shape takes the element-wise path.
void launch_layernorm(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int rows_max,
                      const int* rows, int C, int mode, float eps, const float* gamma, const float* beta,
                      const float* bg, long bg_bs, const float* post_add, hipStream_t s, void* split_planes = nullptr, int planes_f16 = 0);

// scores [z][L][lds] f32 -> P (dtype) [z][L][ldp]: softmax over n < len[b]; zero-fill [len, roundup8(len))
void launch_softmax_rows(const float* scores, int lds, void* P, int p_dt, int ldp, int nbatch, int nheads,
                         int Lmax, const int* len, hipStream_t s);

// out[b][t] = dot(x[b][t][0:C], w) + bias            (VariancePredictor.linear_layer, fs2.py:553-558)
void launch_rowdot(const float* x, int ldx, const float* w, float bias, float* out, int B, int Tmax,
                   const int* T, int C, hipStream_t s);

// idx = clamp(rint(pred*(nb-1)), 0, nb-1); x[b][t][:] += table[idx][:]     (fs2.py:639,649,668,672)
void launch_bucket_embed_add(const float* pred, const float* table, int nbins, float* x, int ldx, int C,
                             int* idx_out, int B, int Tmax, const int* T, hipStream_t s);

// durations: forced (int) or max(rint(exp(logd)-1),0) (fs2.py:678-681) -> dur[b][t], cum[b][t] (inclusive
// prefix sum), mel_len[b].  A duration is clamped to [0, 65536] (NaN -> 0), cum and mel_len saturate at 2^31 - 1; T[b] == 0 writes
// mel_len[b] = 0 and nothing else
void launch_durations(const int* forced, const float* logd, int* dur, int* cum, int* mel_len, int B, int Tmax,
                      const int* T, hipStream_t s);

// prosody control (include/zvx.h, zvx_prosody): the bucketise + embedding add on v = (p + (range[b]-1)*(p - mean_b(p))) + shift[b],
// replaced by target[b][t] where that is not NaN (NULL pointers: neutral).  mean_b is the float64 mean of the utterance's predictions
// rounded once to f32; a NaN prediction makes it NaN, and with a range every index of that utterance 0 (a NaN value buckets to 0)
void launch_bucket_embed_add_ctl(const float* pred, const float* shift, const float* range, const float* target, const float* table,
                                 int nbins, float* x, int ldx, int C, int* idx_out, int B, int Tmax, const int* T, hipStream_t s);
// launch_durations with per-phoneme Q16 factors q[b][t] applied to the running sum: cum = (sum d*q + 2^15) >> 16, dur its differences
void launch_durations_q16(const int* forced, const float* logd, const int* q, int* dur, int* cum, int* mel_len, int B, int Tmax,
                          const int* T, hipStream_t s);

// length regulator (fs2.py:447-455): feats[b][l][:] = x[b][src(l)][:]; optional positional table add
// into a second output of dtype dt (decoder input): dec[b][l][:] = feats + pe[l]
void launch_length_regulate(const float* x, int ldx, const int* cum, const int* T, const int* mel_len,
                            float* feats, int B, int Tmax, int Lmax, int C, hipStream_t s);
// y[b][l][c] = (T)(x[b][l][c] + (pe ? pe[l][c] : 0));  out_rows_max > 0: y's utterances lie that many rows apart (x's: Lmax)
void launch_add_pe_cast(const float* x, const float* pe, void* y, int y_dt, int ldy, int B, int Lmax,
                        const int* L, int C, hipStream_t s, int out_rows_max = 0);

// InstanceNorm statistics over time for x [b][Lmax][ldx] channels [c0, c0+C): mean/rstd [B][C] (biased, eps); C % 8 == 0, ldx % 8 == 0.
// A zero-length utterance (L[b] == 0) gets UNSPECIFIED statistics (0 / 0: NaN today): nothing may consume them -- launch_norm_affine_act
// and launch_instnorm_fused write no row of such an utterance.  (k_colstats' H > 1 form, a [H][Wmax] map per utterance, has no caller.)
void launch_instnorm_stats(const void* x, int x_dt, int ldx, int B, int Lmax, const int* L, int C, float eps,
                           float* mean, float* rstd, hipStream_t s);
// y = act(((x-mean)*rstd) * g + b) with g = (one_plus ? 1 : 0) + gamma[b*g_bs + c], b = beta[b*g_bs + c]
// (gamma NULL -> plain normalisation); written to y[.. ldy] (may be a column slice of a wider buffer)
void launch_norm_affine_act(const void* x, int x_dt, int ldx, void* y, int y_dt, int ldy, int B, int Lmax,
                            const int* L, int C, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, long g_bs, int one_plus, int act, float slope, hipStream_t s);

// mel [b][Lmax][nm] (dtype) -> vocoder input [b][Pmax][ldv] dtype: rows >= mel_len zero up to P[b]
void launch_mel_pad(const void* mel, int m_dt, int ldm, int Lmax, const int* mel_len, void* v, int v_dt,
                    int ldv, int Pmax, const int* P, int B, int nm, hipStream_t s);
void launch_copy_rows_f32(const void* src, int s_dt, int lds, long s_bs, float* dst, long ldd, long d_bs,
                          int B, int rows_max, const int* rows, int C, hipStream_t s);

// conv_post (C -> 1, k taps) + tanh on the activated final stage [b][Nmax][C]: wav[b][n], n < nlen[b]*hop...
// samples in [out_len*out_mul, Nmax) are written as zeros; pcm16: wav is int16 PCM (x 32760, truncated)
void launch_conv_post_tanh(const void* x, int x_dt, int ldx, long x_bs, const float* w /*[k][C]*/, float bias,
                           int ktaps, int C, void* wav, long wav_bs, int pcm16, int B, int Nmax, const int* in_len,
                           int len_mul, const int* out_len, int out_mul, hipStream_t s);
// Band-limited rational resampler, rate_in -> rate_out with L = rate_out / gcd, M = rate_in / gcd (include/zvx.h, zvx_resample):
//   y[n] = sum_k h[n M - k L] x[k],  h = the Kaiser-windowed sinc of 2 * half + 1 taps designed by the context (host_post.hip, rs_bank).
// One launch converts the rows of a device table with one ResampleRow per row: its input and output pointers, its length, its own
// in_origin / out_begin / cnt and the bound `zend` up to which zeros follow the emitted samples, so that the rows of one launch may live in
// unrelated buffers and sit anywhere on their signals.  The row holds samples [in_origin, in_origin + n) of a signal that is zero elsewhere;
// outputs [out_begin, out_begin + cnt) go to positions [0, cnt) of `out`, then zeros up to zend; nothing beyond zend is written (zend = cnt:
// nothing outside [0, cnt); the calls with one window for all rows pass the longest row's cnt: the zero fill to the longest row).  Every
// length and count is formed on the HOST (host_post.hip, run_resample_rows) and travels in the table, which every call uploads through the
// context's pinned staging arena, queued like a launch.  out: f32, or with pcm16 int16 = trunc(clamp(v * 32760, -32768, 32767)).
// bank: [L][pitch] f32 on the device (padded to a multiple of 4 floats): row p holds the T = ceil((2 half + 1) / L) taps of phase p in
// ascending input order, bank[p][t] = h[p + (joff[p] - t) L] (0 where that index is below -half), and in column T the integer
// joff[p] = (half - p) / L as raw bits.  L = M = T = 1, half = 0, bank = {1.0f, 0}: a copy.
// The kernel reads rows[blockIdx.y] at its top and works from it alone: the sum of an output is the same instructions for every caller.
// The 16-byte load and store paths are chosen per row from that row's own pointers and in_origin & 3; they change no bit.
// The grid is sized by out_max, the largest zend; a workgroup whose first tile lies at or past its row's zend returns before the bank load.
struct ResampleRow {
    const float* x; void* out;               // the row's samples; where emitted sample 0 goes (f32 or int16)
    long n;                                  // the row's length
    long in_origin, out_begin, cnt;          // the window: outputs [out_begin, out_begin + cnt) go to [0, cnt)
    long zend;                               // zeros are written to [cnt, zend)
};
struct ResampleArgs {
    const ResampleRow* rows;                 // [B], on the device
    int pcm16;
    int B, L, M, half, T, pitch;
    const float* bank;
    long out_max;                            // the largest zend: the grid
};
// What launch_resample_poly decides before it launches, from a.L, a.M, a.T, a.pitch, a.B and a.out_max alone (no pointer is read): outputs
// per tile, tiles per workgroup, the staged input span in floats, the dynamic LDS in bytes, the tiles of the longest row.  The grid is
// (ceil(tiles / tpb), B).  false: the bank and one tile's input span exceed the LDS of a workgroup.
struct ResampleGeometry { int tile, tpb, xcap; long lds, tiles; };
bool resample_geometry_of(const ResampleArgs& a, ResampleGeometry* g);
// the row pitch (floats) the context gives the bank of (L, M) with T taps per phase
int resample_bank_pitch(int L, int M, int T);
// false (nothing launched) when the bank and one tile's input span exceed the LDS of a workgroup
bool launch_resample_poly(const ResampleArgs& a, hipStream_t s);
// Trim-and-join of a batch's waveform rows (include/zvx.h, zvx_join): three launches, every length and position read on the DEVICE.
// Frame powers.  In padded coordinates (pad = frame / 2 zeros in front of the row) frame f of row b covers [f hop, f hop + frame).  With
// `tiled` (hop divides frame) unit q is the hop-block [q hop, (q + 1) hop) and a frame is the sum of frame / hop neighbouring units, so the
// row is read once; otherwise unit q is frame q itself.  unit[b][q] (pitch upitch doubles) = the sum of the squares of the unit's samples
// inside [0, nsamples[b]), each f32 converted to double first; one wave per unit, 16-byte loads wherever the ADDRESS allows, a shuffle
// reduction in double -- no atomics.  Rows with nsamples[b] < frame are skipped (left whole by launch_join_bounds).
struct JoinBoundsArgs {
    const float* x; long x_bs; const int* nsamples; int B;
    int frame, hop, tiled;                   // tiled: frame % hop == 0 and a frame is few enough units
    double* unit; long upitch;
    double k, floor;                         // k = 10^(-top_db / 10), floor = 1e-20 * frame
    int trim, keep;                          // trim 0: every row whole, `unit` is not read
    int* bounds;                             // [B][2] = begin, end
};
void launch_join_powers(const JoinBoundsArgs& a, long units_max, hipStream_t s);
// pmax, first / last audio frame and bounds[b] = {begin, end} of every row: one workgroup per row over its nf frame powers (two passes in a
// fixed order: the result does not depend on scheduling)
void launch_join_bounds(const JoinBoundsArgs& a, hipStream_t s);
// One workgroup: pos[0] = 0, pos[b + 1] = pos[b] + (end - begin) + gap[b] in int64 (gap may be NULL), seg_begin[b], seg_len[b]
void launch_join_layout(const int* bounds, const int* gap, int B, long* pos, int* seg_begin, int* seg_len, hipStream_t s);
// The copy: out[pos[b] + i] = x[b][seg_begin[b] + i] * g(i) for i < seg_len[b] (g: the linear ramp of include/zvx.h over the F = min(fade,
// len / 2) edge samples, no multiply in between), zeros in the gaps, for every output index below pos[B]; NOTHING is written when pos[B] >
// cap.  The grid covers `upper` >= pos[B] outputs (the host's bound: it does not know pos[B]).  out: f32, or int16 with pcm16.  16-byte
// loads / stores where source and destination addresses allow, scalar at segment edges; vector stores only.
struct JoinCopyArgs {
    const float* x; long x_bs; int B;
    const long* pos; const int* seg_begin; const int* seg_len;
    void* out; long cap; int pcm16, fade;
};
void launch_join_copy(const JoinCopyArgs& a, long upper, hipStream_t s);
// The two gathers of a stream step (include/zvx.h, zvx_stream_next / zvx_stream_next_many): pure data movement, 16-byte loads / stores
// where source and destination addresses allow, scalar otherwise.  A step serves up to STREAM_MANY_MAX_ROWS rows of up to
// STREAM_MANY_MAX_SESSIONS sessions, each row with a source / destination POINTER of its own, so the per-row tables live in device memory:
// built on the host and uploaded through the context's pinned arena (queued like a launch, no host wait) -- a step of ONE session uploads
// its small table the same way.  One small entry per row.
constexpr int STREAM_MAX_ROWS = 64;          // zvx_stream_params.chunks_per_call
constexpr int STREAM_MANY_MAX_SESSIONS = 64;  // ZVX_STREAM_MANY_MAX_SESSIONS
constexpr int STREAM_MANY_MAX_ROWS = 256;     // ZVX_STREAM_MANY_MAX_ROWS
// Rows: row r of out [R][Pmax][nm] = the P frames at src ([P][nm], inside the owning session's mel), then zeros up to Pmax frames.
struct StreamRow { const float* src; int P; int pad_; };
struct StreamRowTab { const StreamRow* tab; float* out; int R, Pmax, nm; };
void launch_stream_rows(const StreamRowTab& a, hipStream_t s);
// Interiors: dst[i] = wav[r][off + i] for i < cnt; dst lies in memory of the owning session (or is the caller's), rows of one session back to back.
// An entry with a source of its own (src != NULL) copies src[off + i] instead: the history drops of the sessions' stages are such a table,
// one launch for all of them, each retained tail into its stage's OTHER buffer (source and destination never overlap).
struct StreamInterior { float* dst; const float* src; int off, cnt; };
struct StreamInteriorTab { const StreamInterior* tab; const float* wav; long w_bs; int R; };
void launch_stream_interiors(const StreamInteriorTab& a, long cnt_max, hipStream_t s);
// Integrated loudness (ITU-R BS.1770 / EBU R128) and gain of a batch's waveform rows (include/zvx.h, zvx_loudness / zvx_normalize): every
// decision is made on the DEVICE, in double, in the power domain.
// K-weighting: struct LoudCoef, declared with the leveler above (it shares the coefficients).
struct LoudArgs {
    const float* x; long x_bs; const int* nsamples; int B;
    int h;                                   // samples per 100 ms unit
    LoudCoef k;
    double* unit; long upitch;               // unit[b][q]: sum of the squares of the K-weighted samples [q h, (q + 1) h), q < nsamples[b] / h
    float* part_peak; int ppitch;            // part_peak[b][workgroup of launch_loud_units]: max |x| over what that workgroup looked at
    double abs_gate;                         // 10^((-70 + 0.691) / 10)
    double* row_sum; long* row_cnt;          // [B]: sum and count of the row's blocks above the absolute gate (the pooled gate's input)
    double* lufs; float* peak; float* gain;  // [B] results
    double target; double max_gain_db; double ceiling;   // ceiling <= 0: none
    int want_gain;                           // 0: measure only, gain stays 1
};
// unit powers and partial peaks: one LANE per unit, started from zero state two units early (or at the row's first sample); a workgroup is
// one wave over 64 neighbouring units of one row and stages its lanes' spans through LDS in chunks of LOUD_T samples, loaded as 16-byte
// groups aligned as ADDRESSES.  Workgroup 0 of a row also takes the peak of the tail behind the last whole unit.  grid.x covers units_max.
void launch_loud_units(const LoudArgs& a, long units_max, hipStream_t s);
// one workgroup per row: both gates over the row's blocks -> lufs[b], peak[b], row_sum / row_cnt, and gain[b] of ZVX_LOUD_PER_ROW
void launch_loud_gates(const LoudArgs& a, hipStream_t s);
// ZVX_LOUD_COMMON, one workgroup: both gates over the blocks of all rows, the maximum of the peaks, one gain written to every gain[b]
void launch_loud_common(const LoudArgs& a, hipStream_t s);
// The programme loudness report's two launches (launch_loud_windows, launch_loud_rank) stand in a section of their own, behind the leveler.
// out[b][i] = x[b][i] * gain[b] for i < nsamples[b], ONE f32 multiply; f32 rows, or int16 by the resampler's rule with pcm16.  Groups of 4
// aligned as ADDRESSES of the destination; a thread reads its group before it writes it and no other thread touches it: safe in place.
struct LoudApplyArgs {
    const float* x; long x_bs; const int* nsamples; int B;
    const float* gain; void* out; long out_bs; int pcm16;
};
void launch_loud_apply(const LoudApplyArgs& a, long n_max, hipStream_t s);
// True-peak envelope and look-ahead limiter of a batch's waveform rows (include/zvx.h, zvx_true_peak / zvx_limit).  Both kernels work on
// tiles of LIMIT_TILE samples of one row, 256 threads each; nothing outside [0, n) of a row is read or written.  `rows` is a device
// table with one LimitRow per row -- its input, output and envelope pointers, its length and its emitted range --, so that the rows of one
// launch may live in unrelated buffers and sit anywhere on their signals; every call uploads one through the context's pinned staging arena
// (host_post.hip, run_limit_rows).  A windowed row emits the samples [off, off + cnt) only: the envelope is still evaluated over the whole row,
// the gain tiles start at `off` -- any sample offset from the envelope's tile grid -- and write out[i - off]; the arithmetic of a sample
// depends on neither grid.  A whole row is off = 0, cnt = n.  Every kernel reads rows[blockIdx.y] at its top and works from it alone, so
// the whole-row call, the _ex call and the per-row call run the same instructions.  Grids are sized by the longest row; a workgroup past
// its row's extent only writes its neutral partial result.
constexpr int LIMIT_TILE = 1024;             // (zerovox_amd/_lib.py carries the same figure for the tests' tile-edge rows)
constexpr int LIMIT_MAX_W = 4096;
constexpr int LIMIT_ENV_REACH = 11;          // e[j] reads x[j - 11 .. j + 11] where os > 1 (include/zvx.h, zvx_limit_ex: H; _lib.py: LIMIT_ENV_REACH)
struct LimitRow {
    const float* x; void* out; float* env;   // the row's samples; where emitted sample `off` goes (f32 or int16); e[i] (NULL: not stored)
    int n, off, cnt, pad_;                   // the row's length; the emitted range [off, off + cnt)
};
struct LimitArgs {
    const LimitRow* rows;                    // [B], on the device
    int B;
    int os, T, pitch; const float* bank;     // os > 1: the resampler's bank of (L, M) = (os, 1) (ResampleArgs), T = 21; os == 1: unused
    float* part_max; float* part_min; int ppitch;   // [b][tile]: max e / min g32 over the tile's EMITTED samples (0 / 1 where it has none)
    int gtiles;                              // tiles of the gain launch (<= ppitch)
    float c; int W; const double* win;       // the ceiling; the smoothing weights win[k + W], k = -W .. W
    int pcm16;
    float* res;                              // launch_limit_reduce: res[b] = max over part_max[b][.], res[B + b] = min over part_min[b][.]
};
// e[b][i] = max(|x[i]|, |y[m]| for os (i - 1) < m < os (i + 1), 0 <= m < os n): the tile plus a halo of 10 samples in front and 11 behind
// is staged in LDS, every thread holds one sample's 22 inputs in registers and sums the os phases in the resampler's own order (so y has
// the bits zvx_resample gives), nothing of y reaches memory.  grid.x = ppitch tiles over the whole row.
void launch_limit_env(const LimitArgs& a, hipStream_t s);
// hold, smooth, gain and multiply of one tile: the envelope of the tile and 2 W samples on either side is held in LDS, its running maximum
// over 2 W + 1 samples is built by doubling (the depth is monotone in e, so the maximum of the depths is the depth of the maximum), the
// depths D of the tile and W on either side follow in double, then s, g, g32 and out = x * g32.  A tile whose whole span stays at or
// below the ceiling copies its samples.  It reads e, never a neighbour's x: safe in place (off = 0).  grid.x = gtiles tiles from `off` on.
// false: the span does not fit the LDS.
bool launch_limit_gain(const LimitArgs& a, hipStream_t s);
// one workgroup per row over the tiles' partial results (part_max / part_min are [b][ppitch], and a tile past a row's own extent holds the
// neutral 0 / 1, so this launch needs no row descriptor; part_min NULL: no gain launch ran, res[B + b] = 1)
void launch_limit_reduce(const LimitArgs& a, hipStream_t s);
// Vocoder-bias denoiser (include/zvx.h, zvx_denoise; spectral.hip): spectral subtraction over the STFT frames of zvx_melspec, the frames
// transformed by an FFT that lives in LDS.  A workgroup of 256 threads holds DENOISE_POINTS complex f32 points, i.e. DENOISE_POINTS / n_fft
// frames of ONE row (4 at 1024), as split re / im planes; every pass of the radix-4 Stockham transform (one radix-2 pass first where
// log2 n_fft is odd) reads its inputs into registers, synchronises, and writes its outputs to the same planes.  The host has validated
// the lengths (zvx_melspec's conditions), so every reflected index lies inside the row.
// `rows` is a device table with one DenoiseRow per row -- its input, output and work-buffer pointers, its length and its window --, so that
// the rows of one launch may live in unrelated buffers and sit anywhere on their signals; every call uploads one through the context's
// pinned staging arena (host_post.hip, run_denoise_rows).
// The window: a row holds samples [origin, origin + n) of its signal and the frame grid is the SIGNAL's.  The kernels work in
// window-relative ints: frame j of the work buffer is frame f_first + j of the signal and reads the window from sample rel + j hop on
// (rel = f_first hop - pad - origin; negative: in the left mirror); the one absolute quantity, the signal's frame count, is formed in 64
// bits from origin and f_first.  f_first is a multiple of the frames per workgroup, rounded down per ROW, so that a frame sits in the
// slot it has in the whole-row call and runs through the same instructions: the first `skip` frames cover no emitted sample and are neither
// loaded nor stored.  A whole row is origin 0, f_first 0, skip 0, rel -pad, both mirrors, off 0, cnt n: the indices it forms are the ones
// it always formed.  Both kernels read rows[blockIdx.y] at their top and work from it alone, so every call runs the same instructions
// through the transforms (two instantiations of one source need not contract their multiply-adds alike; one body cannot differ from itself).
constexpr int DENOISE_POINTS = 4096;         // also the largest n_fft
struct DenoiseRow {
    const float* x; void* out; float* work;  // the row's samples; where emitted sample `off` goes (f32 or int16); its frames [F][n_fft], from f_first
    long origin, f_first;
    int n, skip, rel, off, cnt, mirrors;     // the emitted range [off, off + cnt), cnt -1: to the end of the row; mirrors: bit 0 left, bit 1 right --
                                             // the reflect at sample 0 exists (origin == 0); the signal ends with the window, so the one at its end does
};
struct DenoiseArgs {
    const DenoiseRow* rows;                  // [B], on the device
    int B;
    int n_fft, log2n, hop, pad, Fmax;        // Fmax: the most frames transformed of a row (the grid; the pitch of `mag`, in frames)
    const float* twid;                       // [n_fft][2]: cos, -sin of 2 pi m / n_fft, designed in double, rounded once
    const float* win;                        // [n_fft]: the analysis / synthesis window, likewise
    const double* win2;                      // [n_fft]: its square, from the double window
    double den_min;                          // the pass-through threshold on den (include/zvx.h)
    const float* bias; float strength, floor;
    float* mag;                              // launch_denoise_frames: non-NULL = magnitude-out mode, |X[f][k]| -> mag[B][Fmax][n_fft / 2 + 1], nothing else
    int pcm16;
    int copy;                                // launch_denoise_ola: strength == 0, out[i] = x[i] and the rows' `work` is not read
};
// frame load (reflect padding, window), forward FFT, gain, inverse FFT, window, store of w[t] y_f[t]; no spectrum goes to memory.  Only the
// frames that cover an emitted sample are transformed.  grid = (ceil(Fmax / frames per workgroup), B): B <= 65535.
void launch_denoise_frames(const DenoiseArgs& a, hipStream_t s);
// gather-form overlap-add: one thread per output sample sums the frames that cover it in ascending f (num in f32 from +0, den in double
// from win2), divides once, or passes x[i] through where den < den_min; emitted sample e of a row goes to out[e].  Reads x at its own index
// only: safe in place where off == 0.  n_max: the longest emitted range.
void launch_denoise_ola(const DenoiseArgs& a, long n_max, hipStream_t s);
// half-mode saturation audit: *count += number of elements of x[b][r < rows[b]][0:C] (16-bit, batch stride bs, row stride ld) whose
// magnitude bits are >= 0x7BFF (+-65504 = a clamped store, or Inf / NaN)
void launch_count_sat16(const void* x, long bs, int ld, int B, int rows_max, const int* rows, int C, unsigned long long* count, hipStream_t s);
// x[b][r][0:C] = 0 for rows[b] <= r < rows_max
void launch_zero_tail_rows(float* x, int ldx, int B, int rows_max, const int* rows, int C, hipStream_t s);

// ---- speaker encoder ----
// InstanceNorm1d(80) over time + Conv2d(1->C0, 3x3, pad 1) + ReLU + BN affine -> map [b][F][Wout][C0] (Wout >= Tmax); frames >= lens[b] read
// as zero padding and columns >= lens[b] of the map are not written.  o_dt: DT_BF16 or DT_F32 (anything else is written as f32: no DT_F16)
void launch_spk_front(const float* mels, int Tmax, const int* lens, int F, const float* mean, const float* rstd,
                      const float* w /*[9][C0]*/, const float* bias, const float* bn_scale, const float* bn_shift,
                      int C0, void* out, int o_dt, int B, int Wout, hipStream_t s);
// SE global average pool, first half: partial[b][s][c] = sum over the s-th of S = se_pool_splits(H, Wmax) row blocks of the
// valid (f, t) positions of map [b][H][Wmax][C]   (C % 8 == 0, C <= 256).  x_dt: DT_BF16 or DT_F32 -- every other value is read as f32, so
// DT_F16 is not a valid argument
int se_pool_splits(int H, int Wmax);
void launch_se_pool(const void* x, int x_dt, int B, int H, int Wmax, const int* W, int C, float* partial, hipStream_t s);
// second half + MLP: m = sum_s partial / (H * W[b]);  scale = sigmoid(W2 relu(W1 m + b1) + b2) per clip
void launch_se_fc(const float* partial, int S, int H, const int* W, const float* w1, const float* b1, const float* w2, const float* b2, int C,
                  int Cr, float* scale, int B, hipStream_t s, const float* pool_bias = nullptr);
// y = relu(x * scale[b][c] + res)
void launch_se_apply(const void* x, const void* res, void* y, int dt, const float* scale, int B, int H, int Wmax,
                     const int* W, int C, hipStream_t s);
// ASP pooling (ResNetSE34V2.py:197-205): x map [b][F][Wmax][C] viewed as [t][f*C+c]; logits [b][Wmax][F*C] f32
// out [b][2*F*C] = [mu | sg] in (f*C+c) order
// with_std = 0: self-attentive pooling (SAP, ResNetSE34V2.py:199-200): out [b][F*C] = mu only
void launch_asp_pool(const void* x, int x_dt, const float* logits, int B, int F, int Wmax, const int* W, int C,
                     float* out, int with_std, hipStream_t s);
void launch_l2norm_rows(float* x, int B, int C, hipStream_t s);

// ---- log-mel front end (mels.py:357-395) ----
// out[b][i] = wav[b][reflect(i - pad)] for i < n[b] + 2*pad (numpy 'reflect': no edge repeat), 0 beyond
void launch_reflect_pad(const float* wav, long w_bs, const int* n, float* out, long o_bs, int pad, int B, int out_cols, hipStream_t s);
// The same for a WINDOW of each row that only the device knows (include/zvx.h, zvx_spkemb_wav): with begin = bounds[2 b], end = bounds[2 b + 1]
// (as launch_join_bounds leaves them), cut to end = min(end, begin + max_samples) where max_samples > 0, and m = end - begin,
// out[b][i] = wav[b][begin + reflect(i - pad)] for i < m + 2 pad with the mirror about the window's own samples 0 and m - 1, 0 for
// m + 2 pad <= i < out_cols; nothing outside [begin, end) is read.  out rows are 16-byte aligned (o_bs % 4 == 0, out_cols % 4 == 0) and
// written as 16-byte groups; the source may start at any alignment: a group inside the window is one 16-byte load where its ADDRESS
// allows, four scalar loads otherwise.  A window of m <= pad samples (the host refuses it before the launch) is written as zeros.
void launch_window_pad(const float* wav, long w_bs, const int* bounds, int max_samples, float* out, long o_bs, int pad, int B, int out_cols,
                       hipStream_t s);
// mag[b][t][f] = sqrt(re^2 + im^2), re = spec[b][t][f], im = spec[b][t][nf + f]; columns [nf, ldm) and rows >= frames[b] -> 0
void launch_stft_mag(const float* spec, int lds_, float* mag, int ldm, int nf, int B, int Tmax, const int* frames, hipStream_t s);
// x[b][t][c] = log(max(x, lo)) for t < frames[b], 0 beyond
void launch_log_clip(float* x, int ldx, int C, float lo, int B, int Tmax, const int* frames, hipStream_t s);

// skinny f32 linear: out[b][n] = bias[n] + dot(x[b], w[n]) for few rows b and long K (K % 4 == 0)
void launch_fc_rows(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int ldo, int B, int N, int K, hipStream_t s);

}  // namespace zvx
