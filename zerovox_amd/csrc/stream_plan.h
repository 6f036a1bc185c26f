// stream_plan.h -- the window planners of a stream session (include/zvx.h: zvx_stream_next), header-only and free of HIP so that they
// compile with any host C++ compiler (tests/native/stream_plan_main.cpp checks them against the Python planners on the CPU).
//
// A literal restatement of zerovox_amd/stream.py (ReachPlanner: the limiter's, the denoiser's and the watermark's windows),
// zerovox_amd/leveler.py (LevelPlanner: the leveler's) and zerovox_amd/resample.py (StreamPlanner: the rate conversion's).  push(n_new, last) takes the count of newly received input samples and returns
// (in_origin, out_begin, out_count, keep_from): run the step on the retained samples [in_origin, received) for the outputs
// [out_begin, out_begin + out_count) -- nothing to do when out_count is 0 -- then drop the history before keep_from.
// Every position is an int64_t: a stream may run past 2^32 samples.
// group_rows, at the end, is the arithmetic of one group's rows -- the frames with halo, the kept interior, the running position -- that
// zvx_stream_next and zvx_stream_next_many share (tests/native/stream_group_main.cpp checks it against ZeroVox._vocode_stream_native).
// partition_classes is how zvx_stream_next_many batches one kind of post stage over its sessions (tests/native/stream_classes_main.cpp).
#ifndef ZVX_STREAM_PLAN_H
#define ZVX_STREAM_PLAN_H

#include <stdint.h>

namespace zvx_plan {

struct Step { int64_t in_origin, out_begin, out_count, keep_from; };

inline int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
// ceil(a / b) for b > 0 and any sign of a (Python's -((-a) // b))
inline int64_t ceil_div(int64_t a, int64_t b) { return a / b + ((a % b != 0 && a > 0) ? 1 : 0); }

// A step of fixed reach R: output i is final once i + R <= received - 1 (everything on the last push); the next output next_out
// needs no sample before next_out - R.
struct ReachPlanner {
    int64_t R = 0, received = 0, next_out = 0, origin = 0;
    explicit ReachPlanner(int64_t R_ = 0) : R(R_) {}
    Step push(int64_t n_new, bool last) {
        received += n_new;
        const int64_t end = last ? received : imax(next_out, received - R);
        const Step s{origin, next_out, end - next_out, imax(origin, imin(end - R, received))};
        next_out = end;
        origin = s.keep_from;
        return s;
    }
};

// The leveler's step (zerovox_amd/leveler.py, LevelPlanner): a reach of RL to the left and RR to the right.  Output i is final once
// i + RR <= received - 1 (everything on the last push); the next output next_out needs no sample before next_out - RL.
struct LevelPlanner {
    int64_t RL = 0, RR = 0, received = 0, next_out = 0, origin = 0;
    LevelPlanner() {}
    LevelPlanner(int64_t RL_, int64_t RR_) : RL(RL_), RR(RR_) {}
    Step push(int64_t n_new, bool last) {
        received += n_new;
        const int64_t end = last ? received : imax(next_out, received - RR);
        const Step s{origin, next_out, end - next_out, imax(origin, imin(end - RL, received))};
        next_out = end;
        origin = s.keep_from;
        return s;
    }
};

// rate_in -> rate_out in lowest terms, half = 10 max(L, M) as the library designs its filter; equal rates are a copy: (1, 1, 0)
struct RatePair { int64_t L = 1, M = 1, half = 0; };
inline RatePair rate_pair(int64_t rate_in, int64_t rate_out) {
    int64_t a = rate_in, b = rate_out;
    while (b) { const int64_t t = a % b; a = b; b = t; }
    RatePair p;
    p.L = rate_out / a; p.M = rate_in / a;
    p.half = p.L == p.M ? 0 : 10 * imax(p.L, p.M);
    return p;
}

// The rate conversion: output n needs the input samples k with |n M - k L| <= half, so n is final once n M + half <= (received - 1) L
// (everything, ceil(received L / M) outputs, on the last push); the next output n_next needs no sample before
// ceil((n_next M - half) / L).
struct ResamplePlanner {
    int64_t L = 1, M = 1, half = 0, received = 0, n_next = 0, origin = 0;
    ResamplePlanner() {}
    ResamplePlanner(int64_t rate_in, int64_t rate_out) { const RatePair p = rate_pair(rate_in, rate_out); L = p.L; M = p.M; half = p.half; }
    Step push(int64_t n_new, bool last) {
        received += n_new;
        int64_t end;
        if (last) end = ceil_div(received * L, M);
        else { const int64_t top = (received - 1) * L - half; end = top >= 0 ? top / M + 1 : 0; }
        end = imax(end, n_next);
        const int64_t keep = imax(origin, ceil_div(end * M - half, L));
        const Step s{origin, n_next, end - n_next, imin(keep, received)};
        n_next = end;
        origin = s.keep_from;
        return s;
    }
};

// The rows of one group (zvx_stream_next, zvx_stream_next_many): chunk number q starts at frame st = q chunk and is vocoded on the frames
// [max(0, st - halo), min(frames, st + chunk + halo)) -- the rows ZeroVox._vocode_stream_native builds --; of the row's samples only the
// interior [off, off + cnt) is kept, cnt = min(chunk, frames - st) hop, and lands at the running position pos of the group's new samples.
struct Row { int64_t lo, P, off, cnt, pos; };
struct Group { int first, rows, last; int64_t Pmax, cnt_max, n_new; };
inline int chunk_count(int64_t frames, int64_t chunk) { return (int)((frames + chunk - 1) / chunk); }
// the group that starts at chunk `next`: at most cpc chunks, fewer at the end; rows[] takes min(cpc, chunks left) entries
inline Group group_rows(int64_t frames, int64_t chunk, int64_t halo, int64_t hop, int next, int cpc, Row* rows) {
    const int nchunks = chunk_count(frames, chunk);
    Group g{next, 0, 0, 0, 0, 0};
    g.rows = (int)imin(cpc, nchunks - next);
    if (g.rows < 0) g.rows = 0;
    g.last = next + g.rows == nchunks ? 1 : 0;
    for (int i = 0; i < g.rows; i++) {
        const int64_t st = (int64_t)(next + i) * chunk;
        const int64_t lo = imax(0, st - halo), hi = imin(frames, st + chunk + halo);
        const int64_t n = imin(chunk, frames - st);
        rows[i] = Row{lo, hi - lo, (st - lo) * hop, n * hop, g.n_new};
        g.Pmax = imax(g.Pmax, hi - lo); g.cnt_max = imax(g.cnt_max, n * hop); g.n_new += n * hop;
    }
    return g;
}

// The batches of ONE kind of post stage over the n sessions of a zvx_stream_next_many call.  cls[i] is the class of session i's stage --
// sessions whose stage has bitwise-equal parameters carry the same id, any int >= 0 -- or negative where session i runs no such stage in
// this call.  Sessions of one class form one group, i.e. one call of the per-row form; the groups come in the order of their first member
// and the members of a group in call order.  order[] (n entries at most) takes the members group by group, start[g] is where group g begins
// in it and start[groups] the number of members (n + 1 entries at most).  Returns the number of groups.
inline int partition_classes(const int* cls, int n, int* order, int* start) {
    int groups = 0, m = 0;
    for (int i = 0; i < n; i++) {
        if (cls[i] < 0) continue;
        bool seen = false;
        for (int j = 0; j < i && !seen; j++) seen = cls[j] == cls[i];
        if (seen) continue;
        start[groups++] = m;
        for (int j = i; j < n; j++) if (cls[j] == cls[i]) order[m++] = j;
    }
    start[groups] = m;
    return groups;
}

}  // namespace zvx_plan
#endif /* ZVX_STREAM_PLAN_H */
