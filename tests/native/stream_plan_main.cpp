// stream_plan_main.cpp -- drives the window planners of zerovox_amd/csrc/stream_plan.h from stdin, for tests/test_stream_session.py.
// Host C++ only (no HIP): the test compiles it with the sanitizers of the host compiler and compares every printed step with the Python
// planners (zerovox_amd/stream.py, zerovox_amd/resample.py).
//
// Input, one command per line:
//     reach R               start a ReachPlanner of reach R
//     rate RATE_IN RATE_OUT start a ResamplePlanner
//     push N LAST           push N new samples (LAST: 0 / 1) on the current planner
// Output: one line "in_origin out_begin out_count keep_from" per push.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../zerovox_amd/csrc/stream_plan.h"

int main() {
    zvx_plan::ReachPlanner reach;
    zvx_plan::ResamplePlanner rate;
    int kind = -1;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "reach")) {
            int64_t R;
            if (scanf("%" SCNd64, &R) != 1) return 2;
            reach = zvx_plan::ReachPlanner(R); kind = 0;
        } else if (!strcmp(cmd, "rate")) {
            int64_t a, b;
            if (scanf("%" SCNd64 " %" SCNd64, &a, &b) != 2) return 2;
            rate = zvx_plan::ResamplePlanner(a, b); kind = 1;
        } else if (!strcmp(cmd, "push") && kind >= 0) {
            int64_t n; int last;
            if (scanf("%" SCNd64 " %d", &n, &last) != 2) return 2;
            const zvx_plan::Step s = kind == 0 ? reach.push(n, last != 0) : rate.push(n, last != 0);
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", s.in_origin, s.out_begin, s.out_count, s.keep_from);
        } else {
            return 2;
        }
    }
    return 0;
}
