// stream_stages_main.cpp -- drives zvx_plan::LevelPlanner and a session's five-stage chain (zerovox_amd/csrc/stream_plan.h) from stdin, for
// tests/test_stream_stages.py.  Host C++ only (no HIP): the test compiles it with the sanitizers of the host compiler and compares every
// printed step with the Python planners (zerovox_amd/leveler.py, zerovox_amd/stream.py, zerovox_amd/resample.py).
//
// Input, one command per line:
//     level RL RR                              start a LevelPlanner
//     chain R0 RL RR R1 R2 RATE_IN RATE_OUT    start the chain reach(R0) -> level(RL, RR) -> reach(R1) -> reach(R2) -> resample, stepped
//                                              as a session steps it: every stage is pushed with the count the stage before it emitted
//                                              and with the same `last`
//     push N LAST                              push N new samples (LAST: 0 / 1)
// Output: one line "in_origin out_begin out_count keep_from" per push of a planner, five of them (stage by stage) per push of a chain.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../zerovox_amd/csrc/stream_plan.h"

static void show(const zvx_plan::Step& s) {
    printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", s.in_origin, s.out_begin, s.out_count, s.keep_from);
}

int main() {
    zvx_plan::LevelPlanner level;
    zvx_plan::ReachPlanner reach[3];
    zvx_plan::ResamplePlanner rate;
    int kind = -1;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "level")) {
            int64_t RL, RR;
            if (scanf("%" SCNd64 " %" SCNd64, &RL, &RR) != 2) return 2;
            level = zvx_plan::LevelPlanner(RL, RR); kind = 0;
        } else if (!strcmp(cmd, "chain")) {
            int64_t v[7];
            for (int i = 0; i < 7; i++) if (scanf("%" SCNd64, &v[i]) != 1) return 2;
            reach[0] = zvx_plan::ReachPlanner(v[0]); level = zvx_plan::LevelPlanner(v[1], v[2]);
            reach[1] = zvx_plan::ReachPlanner(v[3]); reach[2] = zvx_plan::ReachPlanner(v[4]);
            rate = zvx_plan::ResamplePlanner(v[5], v[6]); kind = 1;
        } else if (!strcmp(cmd, "push") && kind >= 0) {
            int64_t n; int last;
            if (scanf("%" SCNd64 " %d", &n, &last) != 2) return 2;
            const bool l = last != 0;
            if (kind == 0) { show(level.push(n, l)); continue; }
            zvx_plan::Step s = reach[0].push(n, l); show(s);
            s = level.push(s.out_count, l); show(s);
            s = reach[1].push(s.out_count, l); show(s);
            s = reach[2].push(s.out_count, l); show(s);
            s = rate.push(s.out_count, l); show(s);
        } else {
            return 2;
        }
    }
    return 0;
}
