// stream_classes_main.cpp -- drives partition_classes of zerovox_amd/csrc/stream_plan.h (how zvx_stream_next_many batches one kind of
// post stage over its sessions) from stdin, for tests/test_rows_windows.py.  Host C++ only (no HIP): the test compiles it with the
// sanitizers of the host compiler and compares every printed group with a Python restatement.
//
// Input, one call per line:   N CLS_0 ... CLS_(N-1)      (a negative class: the session runs no such stage)
// Output per call: a line "groups G MEMBERS", then one line per group with its members in order.
#include <stdio.h>

#include <vector>

#include "../../zerovox_amd/csrc/stream_plan.h"

int main() {
    int n;
    while (scanf("%d", &n) == 1) {
        if (n < 0 || n > 4096) return 2;
        // exactly the sizes the contract names: a write past them is the sanitizer's to find
        std::vector<int> cls((size_t)n), order((size_t)n), start((size_t)n + 1);
        for (int i = 0; i < n; i++) if (scanf("%d", &cls[(size_t)i]) != 1) return 3;
        const int groups = zvx_plan::partition_classes(cls.data(), n, order.data(), start.data());
        if (groups < 0 || groups > n) return 4;
        printf("groups %d %d\n", groups, start[(size_t)groups]);
        for (int g = 0; g < groups; g++) {
            for (int m = start[(size_t)g]; m < start[(size_t)g + 1]; m++) printf(m == start[(size_t)g] ? "%d" : " %d", order[(size_t)m]);
            printf("\n");
        }
    }
    return 0;
}
