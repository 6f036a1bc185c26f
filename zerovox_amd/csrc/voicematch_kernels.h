// voicematch_kernels.h -- launch arguments and launchers of the voice matching calls (voicematch.hip; include/zvx.h: zvx_spk_score,
// zvx_spk_topk): cosine scores of B query embeddings against a device-resident library of K embeddings, and the `top` best of them.
#pragma once
#include "zvx_kernels.h"

namespace zvx {

// One workgroup of SPK_THREADS (4 waves) serves one SLAB of SPK_SLAB library rows and one GROUP of up to SPK_GROUP_MAX queries.  The group
// (divided by its norms, zero-padded to whole 16 x 16 tiles) is staged in LDS once; a wave then takes 16 library rows at a time through
// v_mfma_f32_16x16x4_f32 against every query tile, reading each row once in 16-byte loads and forming its norm in the same pass.
// zvx_spk_topk keeps, per (query, slab), a list of `top` candidates in LDS, sorted by descending score and ascending index, and writes it
// to cand_s / cand_i [B][nslab][top] (unused places: SPK_EMPTY_SCORE / INT32_MAX); launch_spk_merge selects over the slabs' lists.
constexpr int SPK_THREADS = 256;
constexpr int SPK_SLAB = 512;                // library rows per workgroup (voices.SLAB_ROWS)
constexpr int SPK_ITER_ROWS = 64;            // ... of which the 4 waves take 16 each at a time
constexpr int SPK_GROUP_MAX = 64;            // queries per group: the library is read once per group
constexpr int SPK_TOP_MAX = 32;              // ZVX_SPK_TOP_MAX
constexpr int SPK_DIM_MAX = 2048;
constexpr int SPK_LDS_BYTES = 160 * 1024;
constexpr float SPK_EMPTY_SCORE = -3.f;      // below every score (a score that is not finite is delivered as -2)

// LDS of a group of g queries (g a multiple of 16): the queries at a row pitch of ceil(dim / 16) 16 + 4 floats, their norms, one wave's
// 16 scores per query (pitch 17) and, for the top-k form, the lists, their thresholds and the waves' flags
inline size_t spk_lds_bytes(int g, int dim, int top) {
    const size_t pitch = (size_t)((dim + 15) / 16) * 16 + 4;
    return (size_t)g * (pitch * 4 + 4 + 17 * 4 + (size_t)top * 8 + 4) + 32;
}
// the largest group, a multiple of 16 up to SPK_GROUP_MAX, whose LDS fits (16 always does: 16 queries of dim 2048 with 32 places are 134 KB)
inline int spk_group(int dim, int top) {
    int g = SPK_GROUP_MAX;
    while (g > 16 && spk_lds_bytes(g, dim, top) > (size_t)SPK_LDS_BYTES) g -= 16;
    return g;
}
inline long spk_slabs(long K) { return (K + SPK_SLAB - 1) / SPK_SLAB; }

struct SpkArgs {
    const float* q;                          // [B][dim] on the device
    const float* lib;                        // [K][dim] on the device, 16-byte aligned
    long K;
    int B, dim, top;                         // top == 0: the score form
    float* score;                            // the score form: [B][K]
    float* cand_s; int* cand_i;              // the top-k form: [B][nslab][top]
    int b0, nq;                              // (set by the launcher: the launch's first query and queries per group)
};
// The match launch(es): every whole group of spk_group(dim, top) queries in one launch (grid.y: the groups), a remainder of fewer in a
// second one with as many query tiles as it needs.  false where the runtime refuses the LDS opt-in (`probe`: only ask).
bool launch_spk_match(const SpkArgs& a, hipStream_t s, bool probe = false);
// out_s / out_i [B][top] from the lists: the best `top` of B x nslab x top candidates under (score descending, index ascending)
void launch_spk_merge(const float* cand_s, const int* cand_i, int B, long nslab, int top, float* out_s, int* out_i, hipStream_t s);

}  // namespace zvx
