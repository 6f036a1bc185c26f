// stream_group_main.cpp -- drives the group arithmetic of zerovox_amd/csrc/stream_plan.h (group_rows: what zvx_stream_next and
// zvx_stream_next_many vocode per call) from stdin, for tests/test_stream_many.py.  Host C++ only (no HIP): the test compiles it with the
// sanitizers of the host compiler and compares every printed row with the rows ZeroVox._vocode_stream_native builds.
//
// Input, one stream per line:   FRAMES CHUNK HALO CPC HOP
// Output per stream: for every group a line "group FIRST ROWS LAST PMAX CNT_MAX N_NEW", then one line "LO P OFF CNT POS" per row; the
// groups are walked as a session walks them (the next group starts behind the last), until the one flagged last.
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "../../zerovox_amd/csrc/stream_plan.h"

int main() {
    int64_t frames, chunk, halo, hop;
    int cpc;
    while (scanf("%" SCNd64 " %" SCNd64 " %" SCNd64 " %d %" SCNd64, &frames, &chunk, &halo, &cpc, &hop) == 5) {
        if (frames < 1 || chunk < 1 || halo < 0 || cpc < 1 || hop < 1) return 2;
        std::vector<zvx_plan::Row> rows((size_t)cpc);
        int next = 0;
        for (;;) {
            const zvx_plan::Group g = zvx_plan::group_rows(frames, chunk, halo, hop, next, cpc, rows.data());
            if (g.rows < 1 || g.rows > cpc) return 3;
            printf("group %d %d %d %" PRId64 " %" PRId64 " %" PRId64 "\n", g.first, g.rows, g.last, g.Pmax, g.cnt_max, g.n_new);
            for (int i = 0; i < g.rows; i++)
                printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", rows[i].lo, rows[i].P, rows[i].off, rows[i].cnt, rows[i].pos);
            next += g.rows;
            if (g.last) break;
        }
        if (next != zvx_plan::chunk_count(frames, chunk)) return 4;
    }
    return 0;
}
