// host_post.hip -- the post-processing calls that write waveform rows: the rows-call and window contracts, resampler, join / trim,
// limiter, leveler, denoiser and its bias, watermark embedding, equaliser.
#include "zvx_host.h"

namespace zvx::host {

// ------------------------------------------------------------------------------------------------
// the rows-call contract of the post-processing entry points (include/zvx.h): a batch of waveform rows [B][Nmax] f32 + nsamples[B], on
// the host or on the device.  The checks are pure: an entry point runs all of its checks before it allocates, uploads or launches.
// ------------------------------------------------------------------------------------------------

namespace {
// (on its own in zvx_resample, whose ZVX_E_UNSUPPORTED rate pairs rank between this and the lengths)
void rows_args(const char* who, const void* in, const int32_t* nsamples, int B, int Nmax) {
    if (!in || !nsamples || B <= 0 || Nmax <= 0) fail(ZVX_E_INVALID, "%s: bad arguments (NULL pointer, B = %d, Nmax = %d)", who, B, Nmax);
}
}  // namespace

RowsInfo rows_check(const char* who, const void* in, const int32_t* nsamples, int B, int Nmax, int max_rows) {
    rows_args(who, in, nsamples, B, Nmax);
    if (B > max_rows) fail(ZVX_E_UNSUPPORTED, "%s: B = %d rows (at most %d per call)", who, B, max_rows);
    RowsInfo r;
    for (int b = 0; b < B; b++) {
        if (nsamples[b] < 0 || nsamples[b] > Nmax) fail(ZVX_E_INVALID, "%s: nsamples[%d]=%d out of range (0..%d)", who, b, nsamples[b], Nmax);
        r.n_max = std::max<long>(r.n_max, nsamples[b]); r.n_sum += nsamples[b];
    }
    return r;
}
void flags_check(const char* who, int flags, int allowed) {
    if (flags & ~allowed) fail(ZVX_E_INVALID, "%s: unknown flag in %d", who, flags);
    if ((flags & ZVX_NO_SYNC) && !(flags & ZVX_DEVICE_OUT)) fail(ZVX_E_INVALID, "%s: ZVX_NO_SYNC needs ZVX_DEVICE_OUT", who);
}
// output rows [B][out_stride] of the input's shape (zvx_normalize, zvx_limit), which may be the input rows themselves
void out_rows_check(const char* who, const void* in, const void* out, int64_t out_stride, int Nmax, int flags) {
    if (!out) fail(ZVX_E_INVALID, "%s: out is NULL", who);
    if (out_stride < Nmax) fail(ZVX_E_INVALID, "%s: out_stride %lld is smaller than Nmax %d", who, (long long)out_stride, Nmax);
    if (out != in) return;
    if (flags & ZVX_PCM16) fail(ZVX_E_INVALID, "%s: ZVX_PCM16 cannot run in place", who);
    if (out_stride != Nmax || !(flags & ZVX_DEVICE_IN) != !(flags & ZVX_DEVICE_OUT))
        fail(ZVX_E_INVALID, "%s: in place needs out_stride == Nmax and both pointers on the same side", who);
}

// host rows go to "<prefix>.in" on the device, device rows (ZVX_DEVICE_IN) are used where they are
const float* rows_to_device(zvx_ctx* c, const std::string& prefix, const float* in, int B, int Nmax, int flags) {
    if (flags & ZVX_DEVICE_IN) return in;
    float* xd = c->fbuf(prefix + ".in", (size_t)B * Nmax);
    HIPCHK(hipMemcpyAsync(xd, in, (size_t)B * Nmax * 4, hipMemcpyHostToDevice, c->stream));
    return xd;
}
DevRows stage_rows(zvx_ctx* c, const std::string& prefix, const float* in, const int32_t* nsamples, int B, int Nmax, int flags) {
    const float* x = rows_to_device(c, prefix, in, B, Nmax, flags);
    return {x, c->upload_ints(prefix + ".len", nsamples, B)};
}

// ------------------------------------------------------------------------------------------------
// sample-rate conversion (include/zvx.h: zvx_resample, "out_rate")
// ------------------------------------------------------------------------------------------------
constexpr int RS_MAX_PHASES = 640;       // max(L, M) a bank is built for: every pair between 22050 and 8000 ... 48000
constexpr int RS_ZEROS = 10;             // half = RS_ZEROS * max(L, M): the filter spans 10 zero crossings of the sinc on each side
constexpr double RS_BETA = 5.0;          // Kaiser window (both as scipy.signal.resample_poly's defaults)

// rate_in -> rate_out as (L, M); equal rates: (1, 1).  ZVX_E_INVALID / ZVX_E_UNSUPPORTED as include/zvx.h states them.
void rs_pair(int rate_in, int rate_out, int* L, int* M) {
    for (int r : {rate_in, rate_out}) if (r < 4000 || r > 192000) fail(ZVX_E_INVALID, "sampling rate %d Hz outside [4000, 192000]", r);
    int a = rate_in, b = rate_out;
    while (b) { const int t = a % b; a = b; b = t; }
    *L = rate_out / a; *M = rate_in / a;
    if (std::max(*L, *M) > RS_MAX_PHASES)
        fail(ZVX_E_UNSUPPORTED, "resampling %d -> %d Hz needs L = %d, M = %d: the polyphase bank is built for max(L, M) <= %d", rate_in, rate_out, *L, *M, RS_MAX_PHASES);
}

namespace {
long rs_out_len(long n, int L, int M) { return (n * L + M - 1) / M; }
// the strided rows of a public call as PostRows
std::vector<PostRow> post_rows(const float* x, long x_bs, void* out, long out_bs, size_t ss, const int32_t* nsamples, const RowsWindows& rw, int B) {
    std::vector<PostRow> rows((size_t)B);
    for (int b = 0; b < B; b++)
        rows[(size_t)b] = PostRow{x + (size_t)b * x_bs, (char*)out + (size_t)b * out_bs * ss, nsamples[b], rw.at(b), rw.cnt[(size_t)b]};
    return rows;
}
// What every windowed effect does once its own checks have passed: the rows go to the device ("<prefix>.in"), the outputs are staged where
// the host wants them ("<prefix>.out"), `run(rows)` issues the effect's launches over the PostRows and gives its device result words (or
// nullptr), and RowsReturn brings rows and words over behind the call's one wait.  writes_rows false: a measuring call, `out` is not looked at (zvx_true_peak).
// -> the `res_bytes` of result words on the host; nullptr where the host wants none
template <typename Run>
const float* post_call(zvx_ctx* c, const char* prefix, const float* in, const int32_t* nsamples, int B, int Nmax, void* out, int64_t out_stride, bool writes_rows,
                       int flags, const RowsWindows& rw, size_t res_bytes, bool want_host, Run&& run) {
    const std::string px(prefix);
    RowsReturn ret(c, B, res_bytes, want_host, writes_rows, rw.cnt_max, flags);
    const float* x = rows_to_device(c, px, in, B, Nmax, flags);
    long out_bs = 0;
    void* od = ret.out_rows((px + ".out").c_str(), out, out_stride, &out_bs);
    const std::vector<PostRow> rows = post_rows(x, Nmax, od, out_bs, ret.ss, nsamples, rw, B);
    const float* res = run(rows.data());
    return (const float*)ret.finish(res, out, out_stride, rw.cnt.data(), flags);
}
// two [B] result arrays of the host's, either may be NULL, from the words [2][B]
void copy_word_pairs(const float* words, int B, float* first, float* second) {
    if (!words) return;
    if (first) memcpy(first, words, (size_t)B * sizeof(float));
    if (second) memcpy(second, words + B, (size_t)B * sizeof(float));
}
}  // namespace

RsPlan rs_plan(const int* len, int mul, int B, int L, int M, long in_origin, long out_begin, long out_count) {
    RsPlan p;
    p.w = RowsWindow{in_origin, out_begin, out_count, 1}; p.cnt.resize(B);
    for (int b = 0; b < B; b++) {
        p.cnt[b] = out_count >= 0 ? out_count : std::max(0L, rs_out_len(in_origin + (long)len[b] * mul, L, M) - out_begin);
        p.out_max = std::max(p.out_max, p.cnt[b]);
    }
    return p;
}
// the strided rows of such a call as PostRows (the caller has checked that the counts fit an int32)
std::vector<PostRow> plan_rows(const RsPlan& p, const float* x, long x_bs, void* out, long out_bs, size_t ss, const int* len, int mul, int B) {
    std::vector<PostRow> rows((size_t)B);
    for (int b = 0; b < B; b++)
        rows[(size_t)b] = PostRow{x + (size_t)b * x_bs, (char*)out + (size_t)b * out_bs * ss, len[b] * mul, p.w, (int32_t)p.cnt[(size_t)b]};
    return rows;
}

namespace {
double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; k++) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-20 * s) break; }
    return s;
}
}  // namespace

// The filter of include/zvx.h, designed in double and rounded once to f32, as the polyphase bank launch_resample_poly reads
// (zvx_kernels.h).  Built and uploaded on first use of (L, M), then kept for the life of the context.
const zvx_ctx::RsBank& rs_bank(zvx_ctx* c, int L, int M) {
    auto it = c->rs_banks.find({L, M});
    if (it != c->rs_banks.end()) return it->second;
    zvx_ctx::RsBank bk;
    bk.L = L; bk.M = M;
    std::vector<float> host;
    if (L == 1 && M == 1) {                                  // equal rates: one tap of 1.0f, a copy
        bk.half = 0; bk.T = 1; bk.pitch = 2;
        host = {1.0f, 0.0f, 0.0f, 0.0f};
    } else {
        const int mx = std::max(L, M), half = RS_ZEROS * mx, N = 2 * half + 1;
        std::vector<double> h(N);
        const double fc = 1.0 / mx, i0b = bessel_i0(RS_BETA);
        double sum = 0.0;
        for (int i = 0; i < N; i++) {
            const double m = i - half, r = m / half, px = M_PI * fc * m;
            const double w = bessel_i0(RS_BETA * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            h[i] = fc * (m == 0 ? 1.0 : sin(px) / px) * w;
            sum += h[i];
        }
        for (double& v : h) v = v / sum * L;
        bk.half = half; bk.T = (N + L - 1) / L; bk.pitch = resample_bank_pitch(L, M, bk.T);
        host.assign(((size_t)L * bk.pitch + 3) & ~(size_t)3, 0.0f);
        for (int p = 0; p < L; p++) {
            const int joff = (half - p) / L;
            for (int t = 0; t < bk.T; t++) {
                const long m = p + (long)(joff - t) * L;
                if (m >= -half) host[(size_t)p * bk.pitch + t] = (float)h[m + half];
            }
            memcpy(&host[(size_t)p * bk.pitch + bk.T], &joff, 4);
        }
    }
    float* d = c->fbuf("rs.bank." + std::to_string(L) + "." + std::to_string(M), host.size());
    HIPCHK(hipMemcpyAsync(d, host.data(), host.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // `host` goes away; once per (L, M)
    bk.dev = d;
    return c->rs_banks[{L, M}] = bk;
}

// The rate conversion over B rows with a window each, every caller's one resampling launch: ONE table upload, one launch, one timed group;
// stage tag "voc.resample", slot ZVX_T_RESAMPLE.  A row's window is the resampler's own contract -- zero outside the row's samples, no
// support condition; `last` takes no part.  Zeros follow a row's outputs up to `zero_to` (-1: the row's own cnt, nothing outside [0, cnt) is
// written; the calls with one window for all rows pass the longest row).  Algorithmic bytes = samples read + samples written, a row's
// input counted when it has outputs or zeros to write (a row that writes nothing counts nothing; a call that writes nothing launches
// nothing).  The caller has validated the rows.
void run_resample_rows(zvx_ctx* c, const zvx_ctx::RsBank& bk, const PostRow* rows, int B, int pcm16, long zero_to) {
    std::vector<ResampleRow> tab((size_t)B);
    double nin = 0, nout = 0;
    long zend_max = 0;
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        ResampleRow& t = tab[(size_t)b];
        t.x = r.in; t.out = r.out; t.n = r.n;
        t.in_origin = (long)r.w.in_origin; t.out_begin = (long)r.w.out_begin; t.cnt = r.cnt; t.zend = zero_to < 0 ? r.cnt : zero_to;
        zend_max = std::max(zend_max, t.zend);
        if (t.zend > 0) { nin += (double)r.n; nout += (double)r.cnt; }
    }
    if (zend_max <= 0) return;
    ResampleArgs a{};
    a.B = B; a.pcm16 = pcm16; a.L = bk.L; a.M = bk.M; a.half = bk.half; a.T = bk.T; a.pitch = bk.pitch; a.bank = bk.dev;
    a.out_max = zend_max;                                    // the grid; every row's own bound is its zend
    ResampleRow* tab_d = (ResampleRow*)c->buf("rs.rows", (size_t)B * sizeof(ResampleRow));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(ResampleRow));
    a.rows = tab_d;
    TagScope scope(c, "voc.resample", ZVX_T_RESAMPLE);
    c->timed(2.0 * nout * bk.T, nin * 4.0 + nout * (pcm16 ? 2.0 : 4.0), [&] {
        if (!launch_resample_poly(a, c->stream)) fail(ZVX_E_UNSUPPORTED, "resampler: L = %d, M = %d does not fit the LDS of a workgroup", bk.L, bk.M);
    });
    scope.close();
}

int model_rate(const zvx_ctx* c) {
    auto it = c->cfg.find("sampling_rate");
    if (it == c->cfg.end()) fail(ZVX_E_MANIFEST, "manifest: missing cfg 'sampling_rate'");
    return atoi(it->second.c_str());
}

// zvx_resample / zvx_resample_ex
void do_resample(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out, int64_t out_stride,
                 int32_t* out_len, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count) {
    rows_args("zvx_resample", in, nsamples, B, Nmax);
    if (!out) fail(ZVX_E_INVALID, "zvx_resample: out is NULL");
    flags_check("zvx_resample", flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    if (in_origin < 0 || out_begin < 0 || out_count < -1 || in_origin > ((int64_t)1 << 40) || out_begin > ((int64_t)1 << 40) || out_count > INT32_MAX)
        fail(ZVX_E_INVALID, "zvx_resample_ex: window out of range");
    int L = 1, M = 1;
    rs_pair(rate_in, rate_out, &L, &M);                     // (its ZVX_E_UNSUPPORTED ranks before a bad length)
    rows_check("zvx_resample", in, nsamples, B, Nmax);
    const RsPlan plan = rs_plan(nsamples, 1, B, L, M, in_origin, out_begin, out_count);
    const long out_max = plan.out_max;
    if (out_max > INT32_MAX) fail(ZVX_E_INVALID, "zvx_resample: %ld output samples per row", out_max);
    if (out_stride < out_max) fail(ZVX_E_BUFFER, "zvx_resample: out_stride %lld < %ld samples", (long long)out_stride, out_max);
    const zvx_ctx::RsBank& bk = rs_bank(c, L, M);
    const int pcm16 = (flags & ZVX_PCM16) ? 1 : 0;
    const size_t ss = pcm16 ? 2 : 4;
    const float* x = rows_to_device(c, "rs", in, B, Nmax, flags);
    void* odev = out; long ostride = out_stride;
    if (!(flags & ZVX_DEVICE_OUT)) { ostride = (std::max(out_max, 1L) + 7) & ~7L; odev = c->buf("rs.out", (size_t)B * ostride * ss); }
    run_resample_rows(c, bk, plan_rows(plan, x, Nmax, odev, ostride, ss, nsamples, 1, B).data(), B, pcm16, out_max);
    if (!(flags & ZVX_DEVICE_OUT) && out_max > 0)
        HIPCHK(hipMemcpy2DAsync(out, (size_t)out_stride * ss, odev, (size_t)ostride * ss, (size_t)out_max * ss, B, hipMemcpyDeviceToHost, c->stream));
    if (out_len) for (int b = 0; b < B; b++) out_len[b] = (int32_t)plan.cnt[b];
    if (!((flags & ZVX_DEVICE_OUT) && (flags & ZVX_NO_SYNC))) c->sync();
}

// ------------------------------------------------------------------------------------------------
// trim-and-join of a batch's waveform rows (include/zvx.h: zvx_join, zvx_trim_bounds)
// ------------------------------------------------------------------------------------------------
constexpr int JOIN_MAX_UNITS_PER_FRAME = 32;   // hop-block sums serve frames of up to this many blocks; longer ratios take the per-frame path

void join_check(const char* who, const void* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap, const zvx_join_params* p) {
    rows_check(who, in, nsamples, B, Nmax);
    if (!p) fail(ZVX_E_INVALID, "%s: params is NULL", who);
    if (p->frame < 2 || p->hop < 1 || p->hop > p->frame) fail(ZVX_E_INVALID, "%s: frame %d / hop %d (frame >= 2, 1 <= hop <= frame)", who, p->frame, p->hop);
    if (p->keep < 0 || p->fade < 0) fail(ZVX_E_INVALID, "%s: keep %d / fade %d must not be negative", who, p->keep, p->fade);
    if (!std::isfinite(p->top_db)) fail(ZVX_E_INVALID, "%s: top_db is not finite", who);
    for (int b = 0; gap && b < B; b++) if (gap[b] < 0) fail(ZVX_E_INVALID, "%s: gap[%d]=%d is negative", who, b, gap[b]);
}

namespace {
// queues the frame-power and bounds launches; "join.bounds" then holds {begin, end} per row.  Returns the device rows and the samples read.
const float* join_bounds(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* p, int flags, double* read) {
    const DevRows rows = stage_rows(c, "join", in, nsamples, B, Nmax, flags);
    JoinBoundsArgs a{};
    a.x = rows.x; a.x_bs = Nmax; a.nsamples = rows.len; a.B = B;
    a.frame = p->frame; a.hop = p->hop; a.keep = p->keep;
    a.tiled = (p->frame % p->hop == 0 && p->frame / p->hop <= JOIN_MAX_UNITS_PER_FRAME) ? 1 : 0;
    a.trim = p->top_db > 0.f ? 1 : 0;
    a.k = pow(10.0, -(double)p->top_db / 10.0); a.floor = 1e-20 * (double)p->frame;
    long units_max = 0; double nin = 0;
    for (int b = 0; b < B; b++) {
        if (nsamples[b] < p->frame) continue;
        const long nf = 1 + ((long)nsamples[b] + 2 * (p->frame / 2) - p->frame) / p->hop;
        units_max = std::max(units_max, a.tiled ? nf - 1 + p->frame / p->hop : nf);
        nin += nsamples[b];
    }
    a.upitch = units_max;
    a.unit = a.trim && units_max > 0 ? (double*)c->buf("join.unit", (size_t)B * units_max * sizeof(double)) : nullptr;
    a.bounds = c->ibuf("join.bounds", (size_t)2 * B);
    launch_join_powers(a, units_max, c->stream);
    launch_join_bounds(a, c->stream);
    *read = a.trim ? nin : 0.0;
    return rows.x;
}

// the launches of one call as ONE timed group under "post.join"; its byte count is only known after the call's wait
struct JoinTimer {
    zvx_ctx* c; TagScope scope; GemmEvent ev{}; bool prof;
    explicit JoinTimer(zvx_ctx* c_) : c(c_), scope(c_, "post.join", ZVX_T_JOIN), prof(c_->profile >= 2 && c_->profile_only < 0) {
        if (prof) { ev.a = c->new_event(); ev.b = c->new_event(); HIPCHK(hipEventRecord(ev.a, c->stream)); }
    }
    void stop() { if (prof) HIPCHK(hipEventRecord(ev.b, c->stream)); scope.close(); }
    void commit(double bytes) { if (prof) { ev.variant = -1; ev.flops = 0; ev.bytes = bytes; ev.tag = "post.join"; c->pending.push_back(ev); prof = false; } }
};
}  // namespace

// join_bounds as a call's whole timed group, then the wait for its result.  Returns the pinned {begin, end} words of every row.
const int* bounds_to_host(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* p, int flags) {
    int* host = (int*)c->join_pinned((size_t)2 * B * sizeof(int));
    JoinTimer t(c);
    double read = 0;
    join_bounds(c, in, nsamples, B, Nmax, p, flags, &read);
    t.stop();
    HIPCHK(hipMemcpyAsync(host, c->ibuf("join.bounds", 0), (size_t)2 * B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    t.commit(read * 4.0);
    return host;
}

void do_trim_bounds(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* p, int32_t* begin, int32_t* end, int flags) {
    join_check("zvx_trim_bounds", in, nsamples, B, Nmax, nullptr, p);
    if (!begin || !end) fail(ZVX_E_INVALID, "zvx_trim_bounds: NULL output");
    flags_check("zvx_trim_bounds", flags, ZVX_DEVICE_IN);
    const int* host = bounds_to_host(c, in, nsamples, B, Nmax, p, flags);
    for (int b = 0; b < B; b++) { begin[b] = host[2 * b]; end[b] = host[2 * b + 1]; }
    c->sync();
}

void do_join(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap, const zvx_join_params* p, void* out,
             int64_t out_capacity, int64_t* out_len, int64_t* seg_pos, int32_t* seg_begin, int32_t* seg_len, int flags) {
    join_check("zvx_join", in, nsamples, B, Nmax, gap, p);
    if (!out || !out_len || out_capacity < 0) fail(ZVX_E_INVALID, "zvx_join: bad output arguments");
    flags_check("zvx_join", flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_PCM16);
    const int pcm16 = (flags & ZVX_PCM16) ? 1 : 0;
    const size_t ss = pcm16 ? 2 : 4;
    long upper = 0;                                          // what the row can hold at most: nothing trimmed
    for (int b = 0; b < B; b++) upper += (long)nsamples[b] + (gap ? gap[b] : 0);
    // layout words in one block: pos [B + 1] int64, then seg_begin [B], seg_len [B]
    const size_t lay_bytes = (size_t)(B + 1) * 8 + (size_t)B * 8;
    const bool host_out = !(flags & ZVX_DEVICE_OUT);
    const long stage = std::min<long>(upper, out_capacity);  // a host row is staged: at most this much can be delivered
    const size_t lay_pad = (lay_bytes + 255) & ~(size_t)255;
    char* host = (char*)c->join_pinned(lay_pad + (host_out ? (size_t)stage * ss : 0));
    char* lay = (char*)c->buf("join.layout", lay_bytes);
    long* pos_d = (long*)lay; int* begin_d = (int*)(lay + (size_t)(B + 1) * 8); int* len_d = begin_d + B;
    const int* gap_d = gap ? c->upload_ints("join.gap", gap, B) : nullptr;
    void* odev = host_out ? c->buf("join.out", (size_t)std::max(stage, 1L) * ss + 16) : out;
    JoinTimer t(c);
    double read = 0;
    const float* x_dev = join_bounds(c, in, nsamples, B, Nmax, p, flags, &read);
    launch_join_layout(c->ibuf("join.bounds", 0), gap_d, B, pos_d, begin_d, len_d, c->stream);
    JoinCopyArgs a{};
    a.x = x_dev; a.x_bs = Nmax; a.B = B; a.pos = pos_d; a.seg_begin = begin_d; a.seg_len = len_d;
    a.out = odev; a.cap = out_capacity; a.pcm16 = pcm16; a.fade = p->fade;
    launch_join_copy(a, upper, c->stream);
    t.stop();
    HIPCHK(hipMemcpyAsync(host, lay, lay_bytes, hipMemcpyDeviceToHost, c->stream));
    if (host_out && stage > 0) HIPCHK(hipMemcpyAsync(host + lay_pad, odev, (size_t)stage * ss, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // the call's one wait
    const int64_t* pos_h = (const int64_t*)host;
    const int32_t* begin_h = (const int32_t*)(host + (size_t)(B + 1) * 8); const int32_t* len_h = begin_h + B;
    const int64_t total = pos_h[B];
    *out_len = total;
    double kept = 0;
    for (int b = 0; b < B; b++) {
        if (seg_pos) seg_pos[b] = pos_h[b];
        if (seg_begin) seg_begin[b] = begin_h[b];
        if (seg_len) seg_len[b] = len_h[b];
        kept += len_h[b];
    }
    const bool fits = total <= out_capacity;
    t.commit(read * 4.0 + (fits ? kept * 4.0 + (double)total * ss : 0.0));
    c->sync();
    if (!fits) fail(ZVX_E_BUFFER, "zvx_join: the joined row has %lld samples, out_capacity is %lld", (long long)total, (long long)out_capacity);
    if (host_out && total > 0) memcpy(out, host + lay_pad, (size_t)total * ss);
}

// ------------------------------------------------------------------------------------------------
// true-peak metering and the look-ahead limiter (include/zvx.h: zvx_true_peak, zvx_limit)
// ------------------------------------------------------------------------------------------------
// w[k] = (1 + cos(pi k / (W + 1))) / (2 (W + 1)), k = -W .. W, divided by their own sum; uploaded on first use of W, then kept.
const double* limit_win(zvx_ctx* c, int W) {
    auto it = c->lim_wins.find(W);
    if (it != c->lim_wins.end()) return it->second;
    std::vector<double> w(2 * (size_t)W + 1);
    double sum = 0.0;
    for (int k = -W; k <= W; k++) sum += w[k + W] = (1.0 + cos(M_PI * (double)k / (double)(W + 1))) / (2.0 * (double)(W + 1));
    for (double& v : w) v /= sum;
    double* d = (double*)c->buf("lim.win." + std::to_string(W), w.size() * sizeof(double));
    HIPCHK(hipMemcpyAsync(d, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // `w` goes away; once per W
    return c->lim_wins[W] = d;
}

namespace {
// The window of the denoiser and the limiter (RowsWindow): the checks of its own numbers, then per row the emitted count after the support
// condition of include/zvx.h for the reach R (the limiter: 2 W + H; the denoiser: n_fft - 1)
// (`row` >= 0: the window is that row's own -- zvx_denoise_rows, zvx_limit_rows -- and every message names it)
void window_args_check(const char* who, const RowsWindow& w, int row) {
    char at[32] = "";
    if (row >= 0) snprintf(at, sizeof at, "row %d: ", row);
    if (w.in_origin < 0 || w.out_begin < 0) fail(ZVX_E_INVALID, "%s: %sin_origin %lld / out_begin %lld is negative", who, at, (long long)w.in_origin, (long long)w.out_begin);
    if (w.out_count < -1) fail(ZVX_E_INVALID, "%s: %sout_count %lld (-1: to the end of the signal)", who, at, (long long)w.out_count);
    if (w.last != 0 && w.last != 1) fail(ZVX_E_INVALID, "%s: %slast is %d (0 or 1)", who, at, w.last);
    if (w.out_count == -1 && !w.last) fail(ZVX_E_INVALID, "%s: %sout_count -1 needs last: the signal's end is not in the window", who, at);
}
}  // namespace

// (Rr >= 0: the reach is asymmetric -- R to the left, Rr to the right, the leveler's RL / RR -- and the messages name the side's own)
int32_t window_count_row(const char* who, const RowsWindow& w, int32_t nsamples, int b, int64_t R, int64_t Rr) {
    const char* ln = Rr >= 0 ? "RL" : "R";
    const char* rn = Rr >= 0 ? "RR" : "R";
    if (Rr < 0) Rr = R;
    const int64_t end_in = w.in_origin + nsamples;
    const int64_t n = w.out_count >= 0 ? w.out_count : std::max<int64_t>(0, end_in - w.out_begin);
    if (n > 0) {
        const int64_t end_out = w.out_begin + n;
        if (w.in_origin > w.out_begin || end_out > end_in)
            fail(ZVX_E_INVALID, "%s: row %d: outputs [%lld, %lld) lie outside the window's samples [%lld, %lld)", who, b, (long long)w.out_begin,
                 (long long)end_out, (long long)w.in_origin, (long long)end_in);
        if (w.in_origin != 0 && w.out_begin - R < w.in_origin)
            fail(ZVX_E_INVALID, "%s: row %d: the reach %s = %lld needs %lld more samples in front of the window (in_origin %lld, out_begin %lld)", who, b,
                 ln, (long long)R, (long long)(w.in_origin - (w.out_begin - R)), (long long)w.in_origin, (long long)w.out_begin);
        if (!w.last && end_out - 1 + Rr > end_in - 1)
            fail(ZVX_E_INVALID, "%s: row %d: the reach %s = %lld needs %lld more samples behind the window (outputs end at %lld, samples at %lld; or last)", who, b,
                 rn, (long long)Rr, (long long)(end_out + Rr - end_in), (long long)end_out, (long long)end_in);
    }
    return (int32_t)n;                                       // n <= nsamples where n > 0
}

namespace {
// What those calls check of their windows, all before anything is queued -> the windows and per row the emitted count.  A call-wide window
// is checked once and reported without a row number; the whole rows are their own window and out_rows_check has covered their stride.
RowsWindows rows_windows_check(const char* who, const WindowsIn& win, const int32_t* nsamples, int B, int64_t R, const float* in, const void* out,
                               int64_t out_stride, int64_t Rr = -1) {
    const bool per_row = win.form == WindowsIn::PER_ROW;
    if (per_row && !win.rows) fail(ZVX_E_INVALID, "%s: win is NULL", who);
    RowsWindows rw;
    rw.w.assign(per_row ? (size_t)B : 1, win.one); rw.cnt.resize((size_t)B);
    if (!per_row) window_args_check(who, win.one, -1);
    for (int b = 0; b < B; b++) {
        if (per_row) {
            if (win.rows[b].reserved != 0) fail(ZVX_E_INVALID, "%s: row %d: reserved is %d (must be 0)", who, b, win.rows[b].reserved);
            rw.w[(size_t)b] = RowsWindow{win.rows[b].in_origin, win.rows[b].out_begin, win.rows[b].out_count, win.rows[b].last};
            window_args_check(who, rw.w[(size_t)b], b);
        }
        rw.cnt[(size_t)b] = window_count_row(who, rw.at(b), nsamples[b], b, R, Rr);
        rw.cnt_max = std::max<long>(rw.cnt_max, rw.cnt[(size_t)b]);
    }
    if (win.form == WindowsIn::WHOLE) return rw;
    if (out_stride < rw.cnt_max) fail(ZVX_E_INVALID, "%s: out_stride %lld is smaller than the longest output row %ld", who, (long long)out_stride, rw.cnt_max);
    if (out == (const void*)in)
        for (int b = 0; b < B; b++) {
            const RowsWindow& w = rw.at(b);
            if (rw.cnt[(size_t)b] <= 0 || w.out_begin == w.in_origin) continue;
            if (!per_row) fail(ZVX_E_INVALID, "%s: in place needs out_begin == in_origin", who);
            fail(ZVX_E_INVALID, "%s: row %d: in place needs out_begin == in_origin (%lld, %lld)", who, b, (long long)w.out_begin, (long long)w.in_origin);
        }
    return rw;
}
}  // namespace

// the checks of the limiter's own parameters (zvx_limit, zvx_limit_ex, zvx_stream_open) -> W
void limit_os_check(const char* who, int os) {
    if (os != 1 && os != 2 && os != 4 && os != 8) fail(ZVX_E_INVALID, "%s: oversample %d is none of 1, 2, 4, 8", who, os);
}
int limit_params_check(const char* who, int rate, const zvx_limit_params* p) {
    if (!std::isfinite(p->ceiling) || !(p->ceiling > 0.f) || p->ceiling > 8.f) fail(ZVX_E_INVALID, "%s: ceiling must be finite and lie in (0, 8]", who);
    if (!std::isfinite(p->window_ms) || !(p->window_ms > 0.f)) fail(ZVX_E_INVALID, "%s: window_ms must be finite and positive", who);
    const double w = std::max(1.0, rint((double)rate * (double)p->window_ms / 1000.0));
    if (w > (double)LIMIT_MAX_W) fail(ZVX_E_UNSUPPORTED, "%s: window of %.0f samples (at most %d)", who, w, LIMIT_MAX_W);
    return (int)w;
}

// The limiter over B rows with a window each, every caller's launches: ONE table upload, the envelope, gain and reduce launches under one
// timed group -> the device words res[b] = peak, res[B + b] = min gain.  p == nullptr: measure only (zvx_true_peak) at oversampling
// `measure_os` -- no gain launch, no envelope stored, res[B + b] = 1.  The caller has validated the rows.
const float* run_limit_rows(zvx_ctx* c, const char* who, const PostRow* rows, int B, const zvx_limit_params* p, int W, int pcm16, int measure_os) {
    const bool lim = p != nullptr;
    LimitArgs a{};
    a.os = lim ? p->oversample : measure_os;
    if (a.os > 1) {
        const zvx_ctx::RsBank& bk = rs_bank(c, a.os, 1);
        if (bk.T != 21 || bk.half != 10 * a.os) fail(ZVX_E_STATE, "%s: the (%d, 1) bank has %d taps per output", who, a.os, bk.T);
        a.T = bk.T; a.pitch = bk.pitch; a.bank = bk.dev;
    }
    if (lim) { a.c = p->ceiling; a.W = W; a.win = limit_win(c, W); }
    std::vector<LimitRow> tab((size_t)B);
    double n_sum = 0, cnt_sum = 0;
    long n_max = 0, cnt_max = 0;
    size_t env_floats = 0;
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        n_max = std::max<long>(n_max, r.n); cnt_max = std::max<long>(cnt_max, r.cnt);
        n_sum += r.n; cnt_sum += r.cnt; env_floats += (size_t)r.n;
    }
    float* env = lim ? c->fbuf("lim.env", std::max<size_t>(env_floats, 1)) : nullptr;
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        LimitRow& t = tab[(size_t)b];
        t.x = r.in; t.out = r.out; t.env = env;
        t.n = r.n; t.off = r.cnt > 0 ? (int)(r.w.out_begin - r.w.in_origin) : 0; t.cnt = r.cnt; t.pad_ = 0;
        if (env) env += r.n;
    }
    a.B = B; a.pcm16 = pcm16;
    a.ppitch = (int)std::max(1L, (n_max + LIMIT_TILE - 1) / LIMIT_TILE);
    a.gtiles = (int)std::max(1L, (cnt_max + LIMIT_TILE - 1) / LIMIT_TILE);                // <= ppitch: cnt <= n in every row
    a.part_max = c->fbuf("lim.part", (size_t)2 * B * a.ppitch);
    a.part_min = lim ? a.part_max + (size_t)B * a.ppitch : nullptr;
    a.res = c->fbuf("lim.res", (size_t)2 * B);
    LimitRow* tab_d = (LimitRow*)c->buf("lim.rows", (size_t)B * sizeof(LimitRow));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(LimitRow));
    a.rows = tab_d;
    TagScope scope(c, "post.limit");
    c->timed(0.0, 4.0 * n_sum + (lim ? (pcm16 ? 2.0 : 4.0) * cnt_sum : 0.0), [&] {
        launch_limit_env(a, c->stream);
        if (lim && !launch_limit_gain(a, c->stream)) fail(ZVX_E_UNSUPPORTED, "%s: a window of %d samples does not fit the LDS of a workgroup", who, W);
        launch_limit_reduce(a, c->stream);
    });
    return a.res;
}

// zvx_true_peak (p == nullptr: the envelope's maximum only, results in peak_in), zvx_limit, zvx_limit_ex and zvx_limit_rows: every check before
// anything is allocated, uploaded or queued
void do_limit(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_limit_params* p,
              int oversample, void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags, const WindowsIn& win) {
    const bool lim = p != nullptr;
    if (!lim && !peak_in) fail(ZVX_E_INVALID, "%s: tpeak is NULL", who);
    rows_check(who, in, nsamples, B, Nmax, 65535);
    if (rate < 4000 || rate > 192000) fail(ZVX_E_INVALID, "%s: rate %d outside [4000, 192000]", who, rate);
    flags_check(who, flags, lim ? (ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16) : ZVX_DEVICE_IN);
    const int os = lim ? p->oversample : oversample;
    limit_os_check(who, os);
    if (lim) out_rows_check(who, in, out, out_stride, Nmax, flags);
    const int W = lim ? limit_params_check(who, rate, p) : 0;
    const RowsWindows rw = rows_windows_check(who, win, nsamples, B, 2 * (int64_t)W + (os > 1 ? LIMIT_ENV_REACH : 0), in, out, out_stride);
    const float* words = post_call(c, "lim", in, nsamples, B, Nmax, out, out_stride, lim, flags, rw, (size_t)B * 8, peak_in || min_gain,
        [&](const PostRow* rows) { return run_limit_rows(c, who, rows, B, p, W, (flags & ZVX_PCM16) ? 1 : 0, os); });
    copy_word_pairs(words, B, peak_in, min_gain);            // words: peak [B], then min gain [B]
}

// ------------------------------------------------------------------------------------------------
// leveler (include/zvx.h: zvx_level, zvx_level_ex, zvx_level_rows)
// ------------------------------------------------------------------------------------------------
// the K-weighting biquads of the leveler and of the loudness measurements (zvx.hip), designed in double, per sampling rate
const LoudCoef& loud_coef(zvx_ctx* c, int rate) {
    auto it = c->loud_coefs.find(rate);
    if (it != c->loud_coefs.end()) return it->second;
    const double pi = 3.14159265358979323846, fs = (double)rate;
    LoudCoef k{};
    {   // stage 1: high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        k.b0 = (Vh + Vb * K / Q + K * K) / a0; k.b1 = 2.0 * (K * K - Vh) / a0; k.b2 = (Vh - Vb * K / Q + K * K) / a0;
        k.a1 = 2.0 * (K * K - 1.0) / a0; k.a2 = (1.0 - K / Q + K * K) / a0;
    }
    {   // stage 2: high pass, b = [1, -2, 1]
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        k.c1 = 2.0 * (K * K - 1.0) / a0; k.c2 = (1.0 - K / Q + K * K) / a0;
    }
    return c->loud_coefs[rate] = k;
}

// the checks of the leveler's own parameters -> S and a, in units of 100 ms (on the host in double)
LevelGeom level_params_check(const char* who, int rate, const zvx_level_params* p) {
    if (!std::isfinite(p->target_lufs) || p->target_lufs < -70.f || p->target_lufs > 0.f) fail(ZVX_E_INVALID, "%s: target_lufs must lie in [-70, 0]", who);
    if (!std::isfinite(p->max_gain_db) || p->max_gain_db < 0.f) fail(ZVX_E_INVALID, "%s: max_gain_db must be finite and not negative", who);
    if (!std::isfinite(p->window_ms) || p->window_ms < 0.f) fail(ZVX_E_INVALID, "%s: window_ms must be finite and not negative", who);
    if (!std::isfinite(p->lookahead_ms) || p->lookahead_ms < 0.f) fail(ZVX_E_INVALID, "%s: lookahead_ms must be finite and not negative", who);
    const double S = std::max(1.0, rint((double)p->window_ms / 100.0)), a = rint((double)p->lookahead_ms / 100.0);
    if (S > (double)LEVEL_MAX_S) fail(ZVX_E_UNSUPPORTED, "%s: a window of %.0f units of 100 ms (at most %d)", who, S, LEVEL_MAX_S);
    if (a > S) fail(ZVX_E_INVALID, "%s: the look-ahead of %.0f units exceeds the window of %.0f units (a <= S)", who, a, S);
    LevelGeom g{};
    g.h = (rate + 5) / 10; g.S = (int)S; g.a = (int)a;
    g.RL = (int64_t)(g.S + 3 - g.a) * g.h - 1; g.RR = (int64_t)(g.a + 1) * g.h - 1;
    return g;
}

namespace {
// The units under the nodes of a row's emitted range (k_level_apply forms the same per tile): [first, last], last < first where none is
// needed; U = the signal's whole units where the window is last (the clamp of the nodes), LEVEL_OPEN otherwise.
struct LevelUnits { long first = 0, last = -1, U = LEVEL_OPEN; };
LevelUnits level_units(const RowsWindow& w, int32_t n, int32_t cnt, const LevelGeom& g) {
    LevelUnits u;
    const int64_t h = g.h;
    u.U = w.last ? (long)((w.in_origin + n) / h) : LEVEL_OPEN;
    if (cnt > 0 && u.U > 0) {
        auto clampu = [](int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : (v > hi ? hi : v); };
        const int64_t q0 = w.out_begin / h, q1 = (w.out_begin + cnt - 1) / h;
        const int64_t mlo = clampu(q0 + g.a - 1, u.U - 1), mhi = clampu(q1 + g.a, u.U - 1);
        u.first = (long)std::max<int64_t>(0, mlo - g.S + 1); u.last = (long)mhi;
    }
    return u;
}
}  // namespace

// The left support of a LAST window that begins inside its signal: where the outputs begin in the signal's last a units (or its tail) the
// clamp to U - 1 moves the first node's window to the left of where RL assumes it, so the oldest needed unit is checked itself -- its
// warm-up starts at (first - 2) h, which must lie inside the window.  (Without last, and wherever the clamp does not act, RL implies it.)
void level_clamped_support_check(const char* who, const RowsWindows& rw, const int32_t* nsamples, int B, const LevelGeom& g) {
    for (int b = 0; b < B; b++) {
        const RowsWindow& w = rw.at(b);
        if (!w.last || w.in_origin == 0) continue;
        const LevelUnits u = level_units(w, nsamples[b], rw.cnt[(size_t)b], g);
        if (u.last < u.first) continue;
        const int64_t start = ((int64_t)u.first - 2) * g.h;
        if (start < w.in_origin)
            fail(ZVX_E_INVALID, "%s: row %d: the window is last and its first node is clamped to the signal's last unit %ld: unit %ld of its window needs %lld more samples "
                 "in front of the window (in_origin %lld, out_begin %lld)", who, b, u.U - 1, u.first, (long long)(w.in_origin - std::max<int64_t>(start, 0)), (long long)w.in_origin,
                 (long long)w.out_begin);
    }
}

// The leveler over B rows with a window each, every caller's launches: ONE table upload, the unit, apply and reduce launches under one timed
// group -> the device words res[b] = gain_lo, res[B + b] = gain_hi.  The caller has validated the rows (the support condition included:
// it is what keeps every needed unit inside the row).
const float* run_level_rows(zvx_ctx* c, const PostRow* rows, int B, int rate, const zvx_level_params* p, const LevelGeom& g, int pcm16) {
    LevelArgs a{};
    a.B = B; a.h = g.h; a.S = g.S; a.a = g.a; a.pcm16 = pcm16;
    a.k = loud_coef(c, rate);
    a.gate = pow(10.0, (-70.0 + 0.691) / 10.0);
    a.target = (double)p->target_lufs; a.gmax = pow(10.0, (double)p->max_gain_db / 20.0);
    std::vector<LevelRow> tab((size_t)B);
    double n_sum = 0, cnt_sum = 0;
    long cnt_max = 0, units_max = 0;
    size_t units = 0;
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        LevelRow& t = tab[(size_t)b];
        t.x = r.in; t.out = r.out; t.p = nullptr;
        t.in_origin = (long)r.w.in_origin;
        t.n = r.n; t.off = r.cnt > 0 ? (int)(r.w.out_begin - r.w.in_origin) : 0; t.cnt = r.cnt; t.pad_ = 0;
        const LevelUnits u = level_units(r.w, r.n, r.cnt, g);
        t.U = u.U; t.q_first = u.first; t.q_last = u.last;
        const long nu = t.q_last - t.q_first + 1;
        units += (size_t)nu; units_max = std::max(units_max, nu);
        cnt_max = std::max<long>(cnt_max, r.cnt); n_sum += r.n; cnt_sum += r.cnt;
    }
    double* pbuf = (double*)c->buf("lvl.p", std::max<size_t>(units, 1) * sizeof(double));
    for (int b = 0; b < B; b++) {
        LevelRow& t = tab[(size_t)b];
        t.p = pbuf; pbuf += t.q_last - t.q_first + 1;
    }
    a.ppitch = (int)std::max(1L, (cnt_max + 3 + LEVEL_TILE - 1) / LEVEL_TILE);          // (+ 3: the address alignment shifts the groups by up to 3 samples)
    a.part_lo = c->fbuf("lvl.part", (size_t)2 * B * a.ppitch);
    a.part_hi = a.part_lo + (size_t)B * a.ppitch;
    a.res = c->fbuf("lvl.res", (size_t)2 * B);
    LevelRow* tab_d = (LevelRow*)c->buf("lvl.rows", (size_t)B * sizeof(LevelRow));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(LevelRow));
    a.rows = tab_d;
    TagScope scope(c, "post.level");
    c->timed(0.0, 4.0 * n_sum + (pcm16 ? 2.0 : 4.0) * cnt_sum, [&] {
        launch_level_units(a, units_max, c->stream);
        launch_level_apply(a, c->stream);
        launch_level_reduce(a, c->stream);
    });
    return a.res;
}

// zvx_level, zvx_level_ex and zvx_level_rows: every check before anything is allocated, uploaded or queued
void do_level(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* p,
              void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags, const WindowsIn& win) {
    if (!p) fail(ZVX_E_INVALID, "%s: params is NULL", who);
    rows_check(who, in, nsamples, B, Nmax, 65535);
    if (rate < 4000 || rate > 192000) fail(ZVX_E_INVALID, "%s: rate %d outside [4000, 192000]", who, rate);
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    out_rows_check(who, in, out, out_stride, Nmax, flags);
    const LevelGeom g = level_params_check(who, rate, p);
    const RowsWindows rw = rows_windows_check(who, win, nsamples, B, g.RL, in, out, out_stride, g.RR);
    level_clamped_support_check(who, rw, nsamples, B, g);
    const float* words = post_call(c, "lvl", in, nsamples, B, Nmax, out, out_stride, true, flags, rw, (size_t)B * 8, gain_lo || gain_hi,
        [&](const PostRow* rows) { return run_level_rows(c, rows, B, rate, p, g, (flags & ZVX_PCM16) ? 1 : 0); });
    copy_word_pairs(words, B, gain_lo, gain_hi);             // words: gain_lo [B], then gain_hi [B]
}

// ------------------------------------------------------------------------------------------------
// vocoder-bias denoiser (include/zvx.h: zvx_denoise, zvx_denoise_bias; kernels: spectral.hip)
// ------------------------------------------------------------------------------------------------
DnGeom dn_geom(const zvx_ctx* c, const char* who) {
    const int n_fft = c->t("mel.dft").dim(2), hop = c->hop;
    int lg = 0;
    while ((1 << lg) < n_fft && lg < 30) lg++;
    if (n_fft < 4 || n_fft > DENOISE_POINTS || (1 << lg) != n_fft)
        fail(ZVX_E_UNSUPPORTED, "%s: the model's n_fft = %d is not a power of two in 4 .. %d", who, n_fft, DENOISE_POINTS);
    if (hop < 1 || hop > n_fft) fail(ZVX_E_UNSUPPORTED, "%s: hop %d with n_fft %d", who, hop, n_fft);
    return {n_fft, lg, hop, (n_fft - hop) / 2, n_fft / 2 + 1};
}
// zvx_melspec's length conditions hold for the whole SIGNAL of row b: known where it ends with the window (no window: the row is its signal)
void stft_len_check(const char* who, const DnGeom& g, int b, int32_t n, const RowsWindow& w) {
    if (w.last && n > 0 && w.in_origin + n < dn_min_samples(g))
        fail(ZVX_E_INVALID, "%s: row %d has %lld samples; a row that is not empty needs at least %d (zvx_melspec's conditions)", who, b,
             (long long)(w.in_origin + n), dn_min_samples(g));
}

// Twiddles, window and squared window, designed in double and kept for the life of the context.  win_length is not a manifest key: it is
// read off the window inside mel.dft (row 0 of the cosine block is the window itself; a periodic Hann is zero at its first sample only).
const zvx_ctx::DnTables& dn_tables(zvx_ctx* c, const DnGeom& g) {
    if (c->dn_tab.n_fft == g.n_fft) return c->dn_tab;
    const int N = g.n_fft;
    const float* row0 = c->t("mel.dft").host;
    int t0 = -1, t1 = -1;
    for (int t = 0; row0 && t < N; t++) if (row0[t] != 0.f) { if (t0 < 0) t0 = t; t1 = t; }
    const int WL = t1 - t0 + 2, lp = t0 - 1;
    if (t0 < 1 || WL > N || lp != (N - WL) / 2) fail(ZVX_E_MANIFEST, "zvx_denoise: mel.dft does not carry a centred periodic Hann window");
    std::vector<double> w(N, 0.0), w2(N);
    for (int i = 0; i < WL; i++) w[lp + i] = 0.5 + 0.5 * cos(M_PI * (double)(2 * i - WL) / (double)WL);     // numpy.hanning(WL + 1)[:-1]
    w[lp] = 0.0;
    for (int t = 0; t < N; t++) w2[t] = w[t] * w[t];
    double top = 0.0;
    for (int t = 0; t < g.hop; t++) { double s = 0.0; for (int u = t; u < N; u += g.hop) s += w2[u]; top = std::max(top, s); }
    std::vector<float> f(3 * (size_t)N);
    for (int m = 0; m < N; m++) {
        const double ang = 2.0 * M_PI * (double)m / (double)N;
        f[2 * (size_t)m] = (float)cos(ang); f[2 * (size_t)m + 1] = (float)-sin(ang);
        f[2 * (size_t)N + m] = (float)w[m];
    }
    char* d = (char*)c->buf("dn.tab", (size_t)N * 8 + (size_t)N * 12);
    HIPCHK(hipMemcpyAsync(d, w2.data(), (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d + (size_t)N * 8, f.data(), (size_t)N * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // the host vectors go away; once per context
    zvx_ctx::DnTables& tb = c->dn_tab;
    tb.n_fft = N; tb.log2n = g.log2n; tb.win_length = WL; tb.den_min = 1e-3 * top;
    tb.win2 = (const double*)d; tb.twid = (const float*)(d + (size_t)N * 8); tb.win = tb.twid + 2 * (size_t)N;
    return tb;
}

namespace {
void dn_fill(DenoiseArgs& a, const DnGeom& g, const zvx_ctx::DnTables& tb) {
    a.n_fft = g.n_fft; a.log2n = g.log2n; a.hop = g.hop; a.pad = g.pad;
    a.twid = tb.twid; a.win = tb.win; a.win2 = tb.win2; a.den_min = tb.den_min;
}
}  // namespace

// the checks of the denoiser's own parameters and bias (zvx_denoise, zvx_denoise_ex, zvx_stream_open) -> the model's STFT geometry
DnGeom denoise_params_check(const zvx_ctx* c, const char* who, const float* bias, const zvx_denoise_params* p) {
    if (!bias || !p) fail(ZVX_E_INVALID, "%s: %s is NULL", who, !bias ? "bias" : "params");
    if (!std::isfinite(p->strength) || p->strength < 0.f) fail(ZVX_E_INVALID, "%s: strength must be finite and not negative", who);
    if (!(p->floor >= 0.f && p->floor <= 1.f)) fail(ZVX_E_INVALID, "%s: floor must lie in [0, 1]", who);
    const DnGeom g = dn_geom(c, who);
    for (int k = 0; k < g.nf; k++) if (!(bias[k] >= 0.f)) fail(ZVX_E_INVALID, "%s: bias[%d] is negative or NaN", who, k);
    return g;
}

namespace {
// The denoiser over B rows with a window each, every caller's launches: ONE table upload, ONE bias upload, the frames and overlap-add
// launches under one timed group.  The frames transformed of a row: from the first one that covers sample out_begin to the last one that
// begins at or before the row's last emitted sample, on the signal's grid.  The kernels count frames from f_first, that first frame
// rounded DOWN per ROW to a multiple of the frames per workgroup: every frame then sits in the slot of its workgroup it has in the
// whole-row call and runs through the same instructions (the unrolled copies of a pass need not contract their multiply-adds alike), which
// is what makes the bits equal.  The `skip` frames in front are neither loaded nor stored.  (spectral.hip, dn_frames_used)
// The caller has validated the rows.
// (the row table and its sums, shared with the watermark's embedder: run_watermark_rows)
struct DnRowsPlan {
    std::vector<DenoiseRow> tab; std::vector<size_t> work_at;
    double frames = 0, n_sum = 0, cnt_sum = 0; long Fmax = 0, cnt_max = 0; size_t work_floats = 0;
};
DnRowsPlan dn_rows_plan(const DnGeom& g, const PostRow* rows, int B, bool copy) {
    const int per = DENOISE_POINTS >> g.log2n;
    DnRowsPlan pl;
    pl.tab.resize((size_t)B); pl.work_at.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        const RowsWindow& w = r.w;
        const bool any = r.cnt > 0;
        const int64_t off = any ? w.out_begin - w.in_origin : 0;
        const int64_t p0 = w.out_begin + g.pad;
        const int64_t f_need = any && p0 >= g.n_fft ? (p0 - g.n_fft) / g.hop + 1 : 0;
        const int64_t f_first = f_need - f_need % per;
        // where frame f_first begins, as an index into the window: in (off - n_fft - per hop, off + hop - n_fft], an int
        const int64_t rel = any ? f_first * g.hop - g.pad - w.in_origin : -(int64_t)g.pad;
        int64_t F = 0;
        if (any) {
            F = (off + r.cnt - 1 - rel) / g.hop + 1;
            if (w.last) F = std::min<int64_t>(F, std::max<int64_t>(0, dn_frames(g, w.in_origin + r.n) - f_first));
            pl.frames += (double)std::max<int64_t>(0, F - (f_need - f_first));
        }
        DenoiseRow& t = pl.tab[(size_t)b];
        t.x = r.in; t.out = r.out; t.work = nullptr;
        t.origin = (long)w.in_origin; t.f_first = (long)f_first;
        t.n = r.n; t.skip = (int)(f_need - f_first); t.rel = (int)rel; t.off = (int)off; t.cnt = r.cnt;
        t.mirrors = (w.in_origin == 0 ? 1 : 0) | (w.last ? 2 : 0);
        pl.work_at[(size_t)b] = pl.work_floats;
        if (!copy) pl.work_floats += (size_t)F * g.n_fft;
        pl.Fmax = std::max<long>(pl.Fmax, (long)F); pl.cnt_max = std::max<long>(pl.cnt_max, r.cnt);
        pl.n_sum += r.n; pl.cnt_sum += r.cnt;
    }
    return pl;
}
// the plan's rows on the device with their work buffers, and the launch arguments' geometry and tables
void dn_rows_upload(zvx_ctx* c, const DnGeom& g, DnRowsPlan& pl, int B, bool copy, int pcm16, DenoiseArgs& a) {
    a.copy = copy;                                           // a copy: the input's bits, nothing is transformed
    if (!copy) {
        dn_fill(a, g, dn_tables(c, g));
        float* work = c->fbuf("dn.work", std::max<size_t>(pl.work_floats, 1));
        for (int b = 0; b < B; b++) pl.tab[(size_t)b].work = work + pl.work_at[(size_t)b];
    } else { a.n_fft = g.n_fft; a.log2n = g.log2n; a.hop = g.hop; a.pad = g.pad; }
    a.Fmax = (int)pl.Fmax; a.B = B; a.pcm16 = pcm16;
    DenoiseRow* tab_d = (DenoiseRow*)c->buf("dn.rows", (size_t)B * sizeof(DenoiseRow));
    c->upload(tab_d, pl.tab.data(), (size_t)B * sizeof(DenoiseRow));
    a.rows = tab_d;
}
}  // namespace

void run_denoise_rows(zvx_ctx* c, const DnGeom& g, const PostRow* rows, int B, const float* bias, const zvx_denoise_params* p, int pcm16) {
    const bool copy = p->strength == 0.f;
    DnRowsPlan pl = dn_rows_plan(g, rows, B, copy);
    DenoiseArgs a{};
    if (!copy) {
        float* bias_d = c->fbuf("dn.bias", g.nf);
        c->upload(bias_d, bias, (size_t)g.nf * 4);
        a.bias = bias_d; a.strength = p->strength; a.floor = p->floor;
    }
    dn_rows_upload(c, g, pl, B, copy, pcm16, a);
    TagScope scope(c, "post.denoise");
    c->timed(copy ? 0.0 : dn_fft_flops(g, pl.frames, 2), 4.0 * pl.n_sum + (pcm16 ? 2.0 : 4.0) * pl.cnt_sum, [&] {
        if (!copy) launch_denoise_frames(a, c->stream);
        launch_denoise_ola(a, pl.cnt_max, c->stream);
    });
}

// zvx_denoise, zvx_denoise_ex and zvx_denoise_rows: every check before anything is allocated, uploaded or queued
void do_denoise(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias, const zvx_denoise_params* p,
                void* out, int64_t out_stride, int flags, const WindowsIn& win) {
    rows_check(who, in, nsamples, B, Nmax, 65535);
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    out_rows_check(who, in, out, out_stride, Nmax, flags);
    const DnGeom g = denoise_params_check(c, who, bias, p);
    const RowsWindows rw = rows_windows_check(who, win, nsamples, B, g.n_fft - 1, in, out, out_stride);
    for (int b = 0; b < B; b++) stft_len_check(who, g, b, nsamples[b], rw.at(b));
    post_call(c, "dn", in, nsamples, B, Nmax, out, out_stride, true, flags, rw, 0, false, [&](const PostRow* rows) {
        run_denoise_rows(c, g, rows, B, bias, p, (flags & ZVX_PCM16) ? 1 : 0);
        return nullptr;
    });
}

// ------------------------------------------------------------------------------------------------
// keyed audio watermark (include/zvx.h: zvx_watermark, zvx_watermark_ex, zvx_watermark_detect; kernels: watermark.hip)
// ------------------------------------------------------------------------------------------------

namespace {
uint64_t wm_mix64(uint64_t z) {                              // the splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

// the checks of the watermark's own parameters (embedder and detector) -> the model's STFT geometry and the bands
WmPlan watermark_params_check(const zvx_ctx* c, const char* who, const zvx_watermark_params* p) {
    if (!p) fail(ZVX_E_INVALID, "%s: params is NULL", who);
    if (!std::isfinite(p->depth_db) || p->depth_db < 0.f || p->depth_db > 6.f) fail(ZVX_E_INVALID, "%s: depth_db must be finite and lie in [0, 6]", who);
    if (!std::isfinite(p->lo_hz) || !std::isfinite(p->hi_hz) || p->lo_hz < 0.f || !(p->lo_hz < p->hi_hz))
        fail(ZVX_E_INVALID, "%s: band %g .. %g Hz needs finite 0 <= lo_hz < hi_hz", who, (double)p->lo_hz, (double)p->hi_hz);
    if (p->block_frames < 1) fail(ZVX_E_INVALID, "%s: block_frames %d must be at least 1", who, p->block_frames);
    if (p->band_bins < 1) fail(ZVX_E_INVALID, "%s: band_bins %d must be at least 1", who, p->band_bins);
    if (p->period_blocks < 1 || p->period_blocks > WM_MAX_PERIOD) fail(ZVX_E_INVALID, "%s: period_blocks %d outside [1, %d]", who, p->period_blocks, WM_MAX_PERIOD);
    if (p->reserved != 0) fail(ZVX_E_INVALID, "%s: reserved is %d (must be 0)", who, p->reserved);
    const DnGeom g = dn_geom(c, who);
    const double rate = (double)model_rate(c), N = (double)g.n_fft;
    const double k_lo = ceil((double)p->lo_hz * N / rate), top = std::min((double)p->hi_hz * N / rate, N / 2.0);
    const double J = floor((top - k_lo) / (double)p->band_bins);
    if (!(J >= 3.0)) fail(ZVX_E_INVALID, "%s: %g .. %g Hz in bands of %d bins gives %.0f bands (at least 3)", who, (double)p->lo_hz, (double)p->hi_hz, p->band_bins, std::max(J, 0.0));
    if (J > (double)WM_MAX_BANDS) fail(ZVX_E_UNSUPPORTED, "%s: %.0f bands (at most %d)", who, J, WM_MAX_BANDS);
    return {g, (int)k_lo, (int)J};
}
// the P x J pattern of +1 / -1 bytes on the device, through the pinned staging arena
const signed char* wm_sign_table(zvx_ctx* c, const zvx_watermark_params* p, int J) {
    const int P = p->period_blocks;
    std::vector<signed char> sg((size_t)P * J);
    for (int ci = 0; ci < P; ci++)
        for (int j = 0; j < J; j++)
            sg[(size_t)ci * J + j] = (wm_mix64(p->key ^ (((uint64_t)ci << 32) | (uint64_t)j)) >> 63) ? 1 : -1;
    signed char* d = (signed char*)c->buf("wm.sign", sg.size());
    c->upload(d, sg.data(), sg.size());
    return d;
}

// The embedder over B rows with a window each: the denoiser's row table, its overlap-add launch, the keyed gain in the frames launch.
// The caller has validated the rows.
// `keys` (zvx_watermark_rows): a key per row -- the distinct keys' tables are built on the device (launch_wm_signs) into one stack, rows of
// equal keys share a table; nullptr: p->key for every row, its table built on the host.
void run_watermark_rows(zvx_ctx* c, const WmPlan& wp, const PostRow* rows, int B, const zvx_watermark_params* p, int pcm16,
                        const uint64_t* keys) {
    const DnGeom& g = wp.g;
    const bool copy = p->depth_db == 0.f;
    DnRowsPlan pl = dn_rows_plan(g, rows, B, copy);
    WatermarkArgs a{};
    dn_rows_upload(c, g, pl, B, copy, pcm16, a.dn);
    const unsigned long long* keys_d = nullptr;
    signed char* signs_d = nullptr;
    int n_tables = 0;
    if (!copy) {
        if (keys) {
            std::vector<unsigned long long> uniq;
            std::vector<int> of_row((size_t)B);
            std::map<uint64_t, int> seen;
            for (int b = 0; b < B; b++) {
                const auto it = seen.emplace(keys[b], (int)uniq.size());
                if (it.second) uniq.push_back(keys[b]);
                of_row[(size_t)b] = it.first->second;
            }
            n_tables = (int)uniq.size();
            unsigned long long* kd = (unsigned long long*)c->buf("wm.keys", uniq.size() * 8);
            int* od = (int*)c->buf("wm.sign_of_row", (size_t)B * sizeof(int));
            signs_d = (signed char*)c->buf("wm.signs", uniq.size() * (size_t)p->period_blocks * wp.J);
            c->upload(kd, uniq.data(), uniq.size() * 8);
            c->upload(od, of_row.data(), (size_t)B * sizeof(int));
            keys_d = kd; a.sign = signs_d; a.sign_of_row = od;
        } else a.sign = wm_sign_table(c, p, wp.J);
        a.k_lo = wp.k_lo; a.KB = p->band_bins; a.J = wp.J; a.TB = p->block_frames; a.P = p->period_blocks;
        a.g_up = (float)pow(10.0, (double)p->depth_db / 20.0); a.g_dn = (float)pow(10.0, -(double)p->depth_db / 20.0);
    }
    TagScope scope(c, "post.watermark");
    c->timed(copy ? 0.0 : dn_fft_flops(g, pl.frames, 2), 4.0 * pl.n_sum + (pcm16 ? 2.0 : 4.0) * pl.cnt_sum, [&] {
        if (keys_d) launch_wm_signs(keys_d, signs_d, n_tables, a.P, a.J, false, c->stream);
        if (!copy) launch_watermark_frames(a, c->stream);
        launch_denoise_ola(a.dn, pl.cnt_max, c->stream);
    });
}

// zvx_watermark, zvx_watermark_ex and zvx_watermark_rows (`keys`: a key per row, or nullptr): every check before anything is allocated, uploaded or queued
void do_watermark(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* p,
                  void* out, int64_t out_stride, int flags, const WindowsIn& win, const uint64_t* keys) {
    rows_check(who, in, nsamples, B, Nmax, 65535);
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    out_rows_check(who, in, out, out_stride, Nmax, flags);
    const WmPlan wp = watermark_params_check(c, who, p);
    const DnGeom& g = wp.g;
    const RowsWindows rw = rows_windows_check(who, win, nsamples, B, g.n_fft - 1, in, out, out_stride);
    for (int b = 0; b < B; b++) stft_len_check(who, wp.g, b, nsamples[b], rw.at(b));
    post_call(c, "wm", in, nsamples, B, Nmax, out, out_stride, true, flags, rw, 0, false, [&](const PostRow* rows) {
        run_watermark_rows(c, wp, rows, B, p, (flags & ZVX_PCM16) ? 1 : 0, keys);
        return nullptr;
    });
}

// ------------------------------------------------------------------------------------------------
// equaliser (include/zvx.h: zvx_fir, zvx_fir_ex, zvx_fir_rows; kernel: fir.hip)
// ------------------------------------------------------------------------------------------------
namespace {
// The filter over B rows with a window each, every caller's launches: ONE table upload, ONE tap upload (doubles, padded with zero taps to
// the kernel's group of 4), the filter launch and, in place, the copy-back under one timed group.  In place the filter writes
// "fir.tmp", row after row, and the copy launch brings every emitted range back: the bits are the out-of-place call's.
// The caller has validated the rows, the taps and the support condition (which is what makes a sample outside a row a true zero).
// In place is decided from the DEVICE rows: a host call with out == in has been staged into two buffers and needs no work buffer.
void run_fir_rows(zvx_ctx* c, const PostRow* rows, int B, const float* taps, int K, int D, int pcm16) {
    const bool in_place = rows[0].out == (const void*)rows[0].in;
    const int Kp = (K + 3) & ~3;
    std::vector<double> h((size_t)Kp, 0.0);
    for (int k = 0; k < K; k++) h[(size_t)k] = (double)taps[k];
    std::vector<FirRow> tab((size_t)B);
    std::vector<FirCopyRow> back(in_place ? (size_t)B : 0);
    double n_sum = 0, cnt_sum = 0;
    long cnt_max = 0;
    size_t tmp_floats = 0;
    for (int b = 0; b < B; b++) { cnt_sum += rows[b].cnt; tmp_floats += (size_t)std::max(rows[b].cnt, 0); }
    float* tmp = in_place ? c->fbuf("fir.tmp", std::max<size_t>(tmp_floats, 1)) : nullptr;
    for (int b = 0; b < B; b++) {
        const PostRow& r = rows[b];
        FirRow& t = tab[(size_t)b];
        t.x = r.in; t.out = in_place ? (void*)tmp : r.out;
        t.n = r.n; t.off = r.cnt > 0 ? (int)(r.w.out_begin - r.w.in_origin) : 0; t.cnt = r.cnt; t.pad_ = 0;
        if (in_place) { back[(size_t)b] = FirCopyRow{(float*)r.out, tmp, (long)r.cnt}; tmp += std::max(r.cnt, 0); }
        n_sum += r.n; cnt_max = std::max<long>(cnt_max, r.cnt);
    }
    FirArgs a{};
    a.B = B; a.Kp = Kp; a.D = D; a.pcm16 = pcm16;
    double* taps_d = (double*)c->buf("fir.taps", (size_t)Kp * sizeof(double));
    c->upload(taps_d, h.data(), (size_t)Kp * sizeof(double));
    FirRow* tab_d = (FirRow*)c->buf("fir.rows", (size_t)B * sizeof(FirRow));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(FirRow));
    FirCopyRow* back_d = nullptr;
    if (in_place) {
        back_d = (FirCopyRow*)c->buf("fir.back", (size_t)B * sizeof(FirCopyRow));
        c->upload(back_d, back.data(), (size_t)B * sizeof(FirCopyRow));
    }
    a.rows = tab_d; a.taps = taps_d;
    TagScope scope(c, "post.fir");
    c->timed(2.0 * K * cnt_sum, 4.0 * n_sum + (pcm16 ? 2.0 : 4.0) * cnt_sum, [&] {
        launch_fir(a, cnt_max, c->stream);
        if (in_place) launch_fir_copy(back_d, B, cnt_max, c->stream);
    });
}
}  // namespace

// zvx_fir, zvx_fir_ex and zvx_fir_rows: every check before anything is allocated, uploaded or queued
void do_fir(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay,
            void* out, int64_t out_stride, int flags, const WindowsIn& win) {
    rows_check(who, in, nsamples, B, Nmax, 65535);
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    out_rows_check(who, in, out, out_stride, Nmax, flags);
    if (!taps) fail(ZVX_E_INVALID, "%s: taps is NULL", who);
    if (ntaps < 1) fail(ZVX_E_INVALID, "%s: ntaps %d must be at least 1", who, ntaps);
    if (ntaps > FIR_MAX_TAPS) fail(ZVX_E_UNSUPPORTED, "%s: %d taps (at most %d)", who, ntaps, FIR_MAX_TAPS);
    if (delay < 0 || delay > ntaps - 1) fail(ZVX_E_INVALID, "%s: delay %d outside [0, %d]", who, delay, ntaps - 1);
    for (int k = 0; k < ntaps; k++) if (!std::isfinite(taps[k])) fail(ZVX_E_INVALID, "%s: taps[%d] is not finite", who, k);
    const RowsWindows rw = rows_windows_check(who, win, nsamples, B, (int64_t)ntaps - 1 - delay, in, out, out_stride, delay);
    post_call(c, "fir", in, nsamples, B, Nmax, out, out_stride, true, flags, rw, 0, false, [&](const PostRow* rows) {
        run_fir_rows(c, rows, B, taps, ntaps, delay, (flags & ZVX_PCM16) ? 1 : 0);
        return nullptr;
    });
}

// zvx_resample_rows: every check before anything is allocated, uploaded or queued
void do_resample_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out, int64_t out_stride,
                      int32_t* out_len, int flags, const zvx_row_window* win) {
    const char* who = "zvx_resample_rows";
    rows_args(who, in, nsamples, B, Nmax);
    if (!out) fail(ZVX_E_INVALID, "%s: out is NULL", who);
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16);
    if (!win) fail(ZVX_E_INVALID, "%s: win is NULL", who);
    for (int b = 0; b < B; b++) {
        const zvx_row_window& w = win[b];
        if (w.reserved != 0) fail(ZVX_E_INVALID, "%s: row %d: reserved is %d (must be 0)", who, b, w.reserved);
        if (w.last != 0 && w.last != 1) fail(ZVX_E_INVALID, "%s: row %d: last is %d (0 or 1)", who, b, w.last);
        if (w.in_origin < 0 || w.out_begin < 0 || w.out_count < -1 || w.in_origin > ((int64_t)1 << 40) || w.out_begin > ((int64_t)1 << 40) || w.out_count > INT32_MAX)
            fail(ZVX_E_INVALID, "%s: row %d: window out of range (in_origin %lld, out_begin %lld, out_count %lld)", who, b, (long long)w.in_origin,
                 (long long)w.out_begin, (long long)w.out_count);
    }
    int L = 1, M = 1;
    rs_pair(rate_in, rate_out, &L, &M);                     // (its ZVX_E_UNSUPPORTED ranks before a bad length, as in zvx_resample)
    rows_check(who, in, nsamples, B, Nmax);
    RowsWindows rw;
    rw.w.resize((size_t)B); rw.cnt.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const zvx_row_window& w = win[b];
        const int64_t n = w.out_count >= 0 ? w.out_count : std::max<int64_t>(0, rs_out_len((long)(w.in_origin + nsamples[b]), L, M) - w.out_begin);
        if (n > INT32_MAX) fail(ZVX_E_INVALID, "%s: row %d: %lld output samples", who, b, (long long)n);
        rw.w[(size_t)b] = RowsWindow{w.in_origin, w.out_begin, w.out_count, w.last};
        rw.cnt[(size_t)b] = (int32_t)n;
        rw.cnt_max = std::max<long>(rw.cnt_max, (long)n);
    }
    if (out_stride < rw.cnt_max) fail(ZVX_E_BUFFER, "%s: out_stride %lld < %ld samples, the longest output row", who, (long long)out_stride, rw.cnt_max);
    const zvx_ctx::RsBank& bk = rs_bank(c, L, M);
    post_call(c, "rs", in, nsamples, B, Nmax, out, out_stride, true, flags, rw, 0, false, [&](const PostRow* rows) {
        run_resample_rows(c, bk, rows, B, (flags & ZVX_PCM16) ? 1 : 0);
        return nullptr;
    });
    if (out_len) for (int b = 0; b < B; b++) out_len[b] = rw.cnt[(size_t)b];
}

constexpr int DN_BIAS_FRAMES = 88;      // mel frames of silence the bias is measured on

void do_denoise_bias(zvx_ctx* c, float* bias) {
    const char* who = "zvx_denoise_bias";
    if (!bias) fail(ZVX_E_INVALID, "%s: bias is NULL", who);
    const DnGeom g = dn_geom(c, who);
    const int P = DN_BIAS_FRAMES, nm = c->n_mels, n = P * c->hop;
    if (n < dn_min_samples(g)) fail(ZVX_E_UNSUPPORTED, "%s: %d samples of silence are shorter than one frame (%d)", who, n, dn_min_samples(g));
    const zvx_ctx::DnTables& tb = dn_tables(c, g);
    float* zmel = c->fbuf("dn.zmel", (size_t)P * nm);
    HIPCHK(hipMemsetAsync(zmel, 0, (size_t)P * nm * 4, c->stream));
    float* wav = c->fbuf("dn.bwav", (size_t)n);
    run_vocoder(c, zmel, nm, P, &P, &P, 1, wav, n, 0);       // what zvx_vocode_mel runs for one row of P zero frames at the native rate
    const int F = dn_frames(g, n);
    DenoiseArgs a{};
    dn_fill(a, g, tb);
    DenoiseRow row{};                                        // the whole row, magnitude-out mode: no output, no work buffer
    row.x = wav; row.n = n; row.rel = -g.pad; row.cnt = n; row.mirrors = 3;
    DenoiseRow* row_d = (DenoiseRow*)c->buf("dn.rows", sizeof(DenoiseRow));
    c->upload(row_d, &row, sizeof(DenoiseRow));
    a.rows = row_d; a.B = 1; a.Fmax = F;
    a.mag = c->fbuf("dn.mag", (size_t)F * g.nf);
    {
        TagScope scope(c, "post.denoise");
        c->timed(dn_fft_flops(g, F, 1), 4.0 * n + 4.0 * F * g.nf, [&] { launch_denoise_frames(a, c->stream); });
    }
    const float* host = (const float*)c->join_pinned((size_t)F * g.nf * 4);
    HIPCHK(hipMemcpyAsync((void*)host, a.mag, (size_t)F * g.nf * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    for (int k = 0; k < g.nf; k++) {                         // the mean over all frames, in double, rounded once
        double s = 0.0;
        for (int f = 0; f < F; f++) s += (double)host[(size_t)f * g.nf + k];
        bias[k] = (float)(s / (double)F);
    }
}

}  // namespace zvx::host
