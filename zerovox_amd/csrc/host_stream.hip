// host_stream.hip -- stream sessions (include/zvx.h: zvx_stream_open / zvx_stream_next / zvx_stream_next_many).
#include "zvx_host.h"

namespace zvx::host {

// ------------------------------------------------------------------------------------------------
// stream sessions (include/zvx.h: zvx_stream_open / zvx_stream_next / zvx_stream_info / zvx_stream_close)
// ------------------------------------------------------------------------------------------------
void stream_free(zvx_stream* s) {
    zvx_ctx* c = s->c;
    auto it = std::find(c->streams.begin(), c->streams.end(), s);
    if (it != c->streams.end()) c->streams.erase(it);
    if (s->dev || s->pinned) {                               // work queued on the context may still read or write the session's memory
        (void)hipStreamSynchronize(c->stream);
        for (hipStream_t s2 : {c->main0, c->voc_aux[0], c->voc_aux[1]}) if (s2 && s2 != c->stream) (void)hipStreamSynchronize(s2);
    }
    if (s->dev) (void)hipFree(s->dev);
    if (s->pinned) (void)hipHostFree(s->pinned);
    delete s;
}

namespace {
// the native samples the rate conversion runs behind its input: output n is final once n M + half <= (received - 1) L
int64_t rs_reach(const zvx_plan::RatePair& p) { return p.half ? zvx_plan::ceil_div(p.half, p.L) + 1 : 0; }

// The step's one table on the device (stream_step): the rows' gather entries, their scatter entries, then the history drops (one per stage
// at most, STREAM_MAX_DROPS per session).  The buffer is taken at its largest size at once: it never grows behind a queued call.
constexpr int STREAM_MAX_DROPS = 5;                          // denoiser, leveler, watermark, limiter, rate conversion
constexpr size_t STREAM_TAB_BYTES = (size_t)STREAM_MANY_MAX_ROWS * (sizeof(StreamRow) + sizeof(StreamInterior)) +
                                    (size_t)STREAM_MANY_MAX_SESSIONS * STREAM_MAX_DROPS * sizeof(StreamInterior);
}  // namespace

// zvx_stream_open (more == nullptr) and zvx_stream_open_ex
void do_stream_open(zvx_ctx* c, const char* who, const float* mel, int frames, const zvx_stream_params* p, const zvx_stream_stages* more, int flags,
                    zvx_stream** out) {
    // ---- every check, before anything is allocated
    if (!p || !out) fail(ZVX_E_INVALID, "%s: %s is NULL", who, !p ? "params" : "out");
    *out = nullptr;
    if (flags & ~(ZVX_DEVICE_IN | ZVX_PCM16)) fail(ZVX_E_INVALID, "%s: unknown flag in %d", who, flags);
    if (flags & ZVX_PCM16) fail(ZVX_E_UNSUPPORTED, "%s: a session hands out f32 pieces (no ZVX_PCM16)", who);
    if (!mel) {
        if (frames != 0) fail(ZVX_E_INVALID, "%s: mel is NULL (the context's mel) and frames is %d, not 0", who, frames);
        if (!c->have_mel) fail(ZVX_E_STATE, "%s: no mel in the context (call zvx_decode first, or pass a mel)", who);
        if (c->B != 1) fail(ZVX_E_UNSUPPORTED, "%s: the context holds a batch of %d utterances (a session streams one)", who, c->B);
        frames = c->mel_len_host[0];
    }
    if (frames < 2) fail(ZVX_E_INVALID, "%s: %d mel frames (at least 2)", who, frames);
    if (p->chunk_frames < 1) fail(ZVX_E_INVALID, "%s: chunk_frames %d (at least 1)", who, p->chunk_frames);
    if (p->chunks_per_call < 1 || p->chunks_per_call > STREAM_MAX_ROWS)
        fail(ZVX_E_INVALID, "%s: chunks_per_call %d outside 1 .. %d", who, p->chunks_per_call, STREAM_MAX_ROWS);
    if (p->halo < 0) fail(ZVX_E_INVALID, "%s: halo %d is negative", who, p->halo);
    if (!p->denoise != !p->denoise_bias) fail(ZVX_E_INVALID, "%s: denoise and denoise_bias go together (one of them is NULL)", who);
    const int native = model_rate(c), hop = c->hop, nm = c->n_mels;
    const int out_rate = c->out_rate && c->out_rate != native ? c->out_rate : native;
    const int64_t total_native = (int64_t)frames * hop;
    DnGeom g{};
    if (p->denoise) {
        g = denoise_params_check(c, who, p->denoise_bias, p->denoise);
        if (total_native < dn_min_samples(g))
            fail(ZVX_E_INVALID, "%s: %d frames are %lld samples; the denoiser needs at least %d (zvx_melspec's conditions)", who, frames,
                 (long long)total_native, dn_min_samples(g));
    }
    const zvx_level_params* lvl = more ? more->level : nullptr;
    const zvx_watermark_params* wm = more ? more->watermark : nullptr;
    if (more && (more->reserved[0] != 0 || more->reserved[1] != 0))
        fail(ZVX_E_INVALID, "%s: stages: reserved is %lld, %lld (must be 0)", who, (long long)more->reserved[0], (long long)more->reserved[1]);
    LevelGeom lg{};
    if (lvl) lg = level_params_check(who, native, lvl);
    WmPlan wp{};
    if (wm) {
        wp = watermark_params_check(c, who, wm);
        if (total_native < dn_min_samples(wp.g))
            fail(ZVX_E_INVALID, "%s: %d frames are %lld samples; the watermark needs at least %d (zvx_melspec's conditions)", who, frames,
                 (long long)total_native, dn_min_samples(wp.g));
    }
    int W = 0;
    if (p->limit) { limit_os_check(who, p->limit->oversample); W = limit_params_check(who, native, p->limit); }
    zvx_plan::RatePair rp;
    if (out_rate != native) {
        int L = 1, M = 1;
        rs_pair(native, out_rate, &L, &M);
        rp = zvx_plan::rate_pair(native, out_rate);
    }
    // ---- geometry: a group's rows, the stages' buffers, the longest piece
    const int chunk = std::min(p->chunk_frames, frames), halo = std::min(p->halo, frames);
    const int nchunks = (int)(((int64_t)frames + p->chunk_frames - 1) / p->chunk_frames);
    const int rows = std::min(p->chunks_per_call, nchunks);
    const int Pcap = (int)std::min<int64_t>(frames, (int64_t)chunk + 2 * (int64_t)halo);
    const int64_t G = (int64_t)rows * chunk * hop;           // the most new samples one call brings
    struct Want { int kind; int64_t R, keep; };              // R: the reach to the right; keep: the most history a stage retains between two calls
    std::vector<Want> want;
    if (p->denoise) want.push_back({zvx_stream::DENOISE, (int64_t)g.n_fft - 1, 2 * ((int64_t)g.n_fft - 1)});
    if (lvl) want.push_back({zvx_stream::LEVEL, lg.RR, lg.RL + lg.RR});
    if (wm) want.push_back({zvx_stream::WATERMARK, (int64_t)wp.g.n_fft - 1, 2 * ((int64_t)wp.g.n_fft - 1)});
    if (p->limit) { const int64_t R = 2 * (int64_t)W + (p->limit->oversample > 1 ? LIMIT_ENV_REACH : 0); want.push_back({zvx_stream::LIMIT, R, 2 * R}); }
    if (out_rate != native) want.push_back({zvx_stream::RESAMPLE, rs_reach(rp), 2 * rp.half / rp.L + 2});
    int64_t delay = 0;
    for (const Want& w : want) delay += w.R;
    if (G + delay > (int64_t)1 << 28 || (int64_t)rows * Pcap * std::max(hop, nm) > (int64_t)1 << 28)
        fail(ZVX_E_UNSUPPORTED, "%s: a group of %d chunks of %d frames is %lld samples (at most 2^28 per call)", who, rows, chunk, (long long)G);
    const int64_t max_piece = zvx_plan::ceil_div((G + delay) * rp.L, rp.M) + 1;
    const long wstride = ((long)Pcap * hop + 7) & ~7L;
    // ---- the tables a stage needs on first use: no zvx_stream_next waits for an upload
    if (p->denoise && p->denoise->strength != 0.f) dn_tables(c, g);
    if (p->limit) { limit_win(c, W); if (p->limit->oversample > 1) rs_bank(c, p->limit->oversample, 1); }
    if (out_rate != native) rs_bank(c, (int)rp.L, (int)rp.M);
    {   // ... and what the leveler's and the watermark's bodies take on first use, at the session's largest step: a stage holds at most
        // keep + (the group + the reaches in front of it) samples and emits no more than it holds
        int64_t in_max = G;
        for (const Want& w : want) {
            const int64_t held = w.keep + in_max;
            if (w.kind == zvx_stream::LEVEL) {
                loud_coef(c, native);
                c->buf("lvl.p", (size_t)(held / lg.h + lg.S + 4) * sizeof(double));
                c->fbuf("lvl.part", (size_t)2 * (size_t)((held + 3 + LEVEL_TILE - 1) / LEVEL_TILE));
                c->fbuf("lvl.res", 2); c->buf("lvl.rows", sizeof(LevelRow));
            }
            if (w.kind == zvx_stream::WATERMARK) {
                c->buf("dn.rows", sizeof(DenoiseRow));
                if (wm->depth_db != 0.f) {
                    dn_tables(c, wp.g);
                    const int64_t F = (held + wp.g.n_fft) / wp.g.hop + (DENOISE_POINTS >> wp.g.log2n) + 2;
                    c->fbuf("dn.work", (size_t)F * wp.g.n_fft);
                    c->buf("wm.keys", 8); c->buf("wm.sign_of_row", sizeof(int)); c->buf("wm.signs", (size_t)wm->period_blocks * wp.J);
                }
            }
            in_max += w.R;
        }
    }
    c->buf("stream.tab", STREAM_TAB_BYTES); c->fbuf("stream.rows", (size_t)rows * Pcap * nm); c->fbuf("stream.wav", (size_t)rows * wstride);   // what a step of the largest group takes
    // ---- the session and its memory
    zvx_stream* s = new zvx_stream();
    s->c = c;
    try {
        s->frames = frames; s->chunk = p->chunk_frames; s->cpc = p->chunks_per_call; s->halo = p->halo; s->hop = hop; s->native = native; s->out_rate = out_rate;
        s->nchunks = nchunks; s->Pcap = Pcap; s->delay = delay; s->max_piece = max_piece;
        s->total = zvx_plan::ceil_div(total_native * rp.L, rp.M);
        if (p->denoise) { s->dn = *p->denoise; s->bias.assign(p->denoise_bias, p->denoise_bias + g.nf); }
        if (p->limit) { s->lim = *p->limit; s->lim_W = W; }
        if (lvl) { s->lvl = *lvl; s->lvl_g = lg; }
        if (wm) { s->wm = *wm; s->wm_plan = wp; }
        auto pad = [](int64_t floats) { return (size_t)((floats * 4 + 255) & ~(int64_t)255); };
        size_t bytes = pad((int64_t)frames * nm) + pad(max_piece);
        int64_t in_max = G;
        for (const Want& w : want) {
            zvx_stream::Stage st;
            st.kind = w.kind;
            if (w.kind == zvx_stream::RESAMPLE) st.rate = zvx_plan::ResamplePlanner(native, out_rate);
            else if (w.kind == zvx_stream::LEVEL) st.level = zvx_plan::LevelPlanner(lg.RL, lg.RR);
            else st.reach = zvx_plan::ReachPlanner(w.R);
            st.cap = w.keep + in_max + 8;
            in_max += w.R;
            bytes += 2 * pad(st.cap);
            s->stages.push_back(st);
        }
        HIPCHK(hipMalloc((void**)&s->dev, bytes));
        HIPCHK(hipHostMalloc((void**)&s->pinned, (size_t)max_piece * 4, hipHostMallocDefault));
        HIPCHK(hipMemsetAsync(s->dev, 0, bytes, c->stream));
        char* q = s->dev;
        auto take = [&](int64_t floats) { float* r = (float*)q; q += pad(floats); return r; };
        s->mel = take((int64_t)frames * nm); s->ostage = take(max_piece);
        for (auto& st : s->stages) { st.buf[0] = take(st.cap); st.buf[1] = take(st.cap); }
        const size_t mbytes = (size_t)frames * nm * 4;
        if (!mel) HIPCHK(hipMemcpyAsync(s->mel, c->fbuf("mel", 0), mbytes, hipMemcpyDeviceToDevice, c->stream));       // utterance 0: the first rows
        else if (flags & ZVX_DEVICE_IN) HIPCHK(hipMemcpyAsync(s->mel, mel, mbytes, hipMemcpyDeviceToDevice, c->stream));
        else {
            HIPCHK(hipMemcpyAsync(s->mel, mel, mbytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));         // the caller's mel may be reused when the call returns
        }
    } catch (...) {
        stream_free(s);
        throw;
    }
    c->streams.push_back(s);
    *out = s;
}

namespace {
// the checks every stepping call makes on its flags (zvx_stream_next, zvx_stream_next_many)
void stream_flags_check(const char* who, int flags) {
    if (flags & ~(ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16)) fail(ZVX_E_INVALID, "%s: unknown flag in %d", who, flags);
    if (flags & ZVX_PCM16) fail(ZVX_E_UNSUPPORTED, "%s: a session hands out f32 pieces (no ZVX_PCM16)", who);
    if ((flags & ZVX_NO_SYNC) && !(flags & ZVX_DEVICE_OUT)) fail(ZVX_E_INVALID, "%s: ZVX_NO_SYNC needs ZVX_DEVICE_OUT", who);
}

// What a session's next step does, worked out before anything is queued: the group's rows (stream_plan.h) and the stages' windows on
// COPIES of the planners -- host integer arithmetic, so the piece's size n is known up front and a refused call has consumed nothing.
struct StreamStep {
    zvx_plan::Group g{};
    zvx_plan::Row rows[STREAM_MAX_ROWS];
    int P[STREAM_MAX_ROWS];
    std::vector<zvx_stream::Stage> plan;
    std::vector<zvx_plan::Step> steps;
    int64_t n = 0;                         // the piece's samples at the session's output rate
};
void stream_plan_step(const char* who, const zvx_stream* s, StreamStep& p) {
    // ---- the group: chunk st is vocoded on frames [max(0, st - halo), min(frames, st + chunk + halo)), its interior kept
    p.g = zvx_plan::group_rows(s->frames, s->chunk, s->halo, s->hop, s->next_chunk, s->cpc, p.rows);
    for (int i = 0; i < p.g.rows; i++) p.P[i] = (int)p.rows[i].P;
    if (p.g.Pmax > s->Pcap) fail(ZVX_E_STATE, "%s: a row of %d frames exceeds the session's %d", who, (int)p.g.Pmax, s->Pcap);
    // ---- the plan, on copies of the planners
    const size_t K = s->stages.size();
    p.plan = s->stages;
    p.steps.resize(K);
    int64_t n = p.g.n_new;
    for (size_t k = 0; k < K; k++) {
        p.steps[k] = p.plan[k].push(n, p.g.last != 0);
        const int64_t held = p.plan[k].hist + n;
        if (held != p.plan[k].received() - p.steps[k].in_origin || held > p.plan[k].cap)
            fail(ZVX_E_STATE, "%s: stage %zu holds %lld samples (buffer %lld, window from %lld)", who, k, (long long)held, (long long)p.plan[k].cap, (long long)p.steps[k].in_origin);
        // the plan's self-check: a denoiser's, leveler's, watermark's or limiter's window must be one the rows calls accept (their support
        // condition, on the host).  The leveler's is its own: RL to the left, RR to the right, and the clamped left rule of a last window.
        // That rule never bites here although a session flags its last group `last` WITH new samples (the Python stream closes with an
        // empty push): the last push's out_begin is what the push before left, max(0, prev_received - RR), RR = (a + 1) h - 1, so
        // out_begin / h + a - 1 <= (prev_received + 1) / h - 2 <= prev_received / h - 1 <= U - 1 -- the first node is not clamped, and
        // where it is not, RL (in_origin = out_begin - RL whenever in_origin > 0) implies the oldest unit's support.
        if (p.plan[k].kind != zvx_stream::RESAMPLE && p.steps[k].out_count > 0) {
            const RowsWindow w{p.steps[k].in_origin, p.steps[k].out_begin, p.steps[k].out_count, p.g.last ? 1 : 0};
            const bool level = p.plan[k].kind == zvx_stream::LEVEL;
            int64_t cnt = -1;
            try {
                if (level) {
                    cnt = window_count_row(who, w, (int32_t)held, 0, s->lvl_g.RL, s->lvl_g.RR);
                    RowsWindows rw;
                    rw.w.assign(1, w); rw.cnt.assign(1, (int32_t)cnt); rw.cnt_max = (long)cnt;
                    const int32_t held32 = (int32_t)held;
                    level_clamped_support_check(who, rw, &held32, 1, s->lvl_g);
                } else cnt = window_count_row(who, w, (int32_t)held, 0, p.plan[k].reach.R);
            }
            catch (const ZvxError& e) { fail(ZVX_E_STATE, "%s (stage %zu of the session's plan)", e.what(), k); }
            if (cnt != w.out_count) fail(ZVX_E_STATE, "%s: stage %zu emits %lld samples, its plan says %lld", who, k, (long long)cnt, (long long)w.out_count);
        }
        n = p.steps[k].out_count;
    }
    p.n = n;
    if (n > s->max_piece) fail(ZVX_E_STATE, "%s: a piece of %lld samples exceeds max_piece %lld", who, (long long)n, (long long)s->max_piece);
}

// One step of n sessions of ONE context, the only stepping path (zvx_stream_next is its n = 1): the callers have made their own checks
// and planned every session (stream_plan_step), so from here on the call consumes the groups and a failure ends every session of it.
// The rows of all sessions are gathered by one launch, vocoded as ONE batch by one run_vocoder and scattered by one launch to where each
// session's first stage reads them.  The stages then run kind by kind -- all denoisers, then the levelers, the watermarks, the limiters, the
// rate conversions; a session's chain order is kept and everything is on the one stream.  Within a kind the sessions whose stage has
// bitwise-equal parameters (the bias by content; the leveler by its four parameters; the watermark by everything but the key, the members'
// keys go to the one call as keys[]; the limiter by W, oversampling and ceiling; the rate conversion by its two rates, i.e. the polyphase bank) form
// one group (stream_plan.h, partition_classes), and a group is ONE call of the per-row form: its rows are the sessions' [history | new]
// buffers with each session's own window, each output goes straight behind the next stage's history or to the piece's destination.
// All history drops of the call are ONE launch over a table.  Every session's stages are walked once, before anything is queued: the
// walk yields the stages' rows, the drops and -- in the plan's copies of the stages -- the state the session takes on at the end.
void stream_step(const char* who, zvx_ctx* c, zvx_stream* const* ss, StreamStep* plans, int n, void* const* out, const int64_t* n_out,
                 int32_t* done, int flags) {
    try {
        c->have_features = false; c->have_mel = false;      // as zvx_vocode_mel: the context's intermediates are void
        const int nm = c->n_mels, hop = c->hop;
        int R = 0, Pmax = 0; long cnt_max = 0, move_max = 0; double rows_bytes = 0, new_bytes = 0, move_bytes = 0;
        for (int i = 0; i < n; i++) {
            const StreamStep& p = plans[i];
            R += p.g.rows; Pmax = std::max(Pmax, (int)p.g.Pmax); cnt_max = std::max(cnt_max, (long)p.g.cnt_max);
            for (int j = 0; j < p.g.rows; j++) rows_bytes += (double)p.P[j] * nm * 4.0;
            rows_bytes += (double)p.g.rows * (double)p.g.Pmax * nm * 4.0;
            new_bytes += 8.0 * (double)p.g.n_new;
        }
        const long wstride = ((long)Pmax * hop + 7) & ~7L;
        // ---- the table, and every stage's input, window and destination, from the sessions' state as it stands
        std::vector<char> tab((size_t)R * (sizeof(StreamRow) + sizeof(StreamInterior)) + (size_t)n * STREAM_MAX_DROPS * sizeof(StreamInterior));
        StreamRow* tr = (StreamRow*)tab.data();
        StreamInterior* ti = (StreamInterior*)(tr + R);
        StreamInterior* moves = ti + R;
        int M = 0, r = 0;
        std::vector<int> P((size_t)R);
        struct Slot { bool run = false; PostRow row{}; };
        std::vector<Slot> slot[zvx_stream::KINDS];
        for (auto& v : slot) v.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const zvx_stream* s = ss[i];
            StreamStep& p = plans[i];
            const size_t K = s->stages.size();
            const bool last = p.g.last != 0;
            // where stage k's new input goes: straight behind the history of its buffer; behind the last stage, the piece's destination
            auto dst_of = [&](size_t k) { return k < K ? s->stages[k].buf[s->stages[k].cur] + s->stages[k].hist : (flags & ZVX_DEVICE_OUT) ? (float*)out[i] : s->ostage; };
            float* base = dst_of(0);
            for (int j = 0; j < p.g.rows; j++, r++) {
                P[(size_t)r] = p.P[j];
                tr[r] = StreamRow{s->mel + p.rows[j].lo * nm, p.P[j], 0};
                ti[r] = StreamInterior{base + p.rows[j].pos, nullptr, (int)p.rows[j].off, (int)p.rows[j].cnt};
            }
            int64_t n_in = p.g.n_new;
            for (size_t k = 0; k < K; k++) {
                const zvx_stream::Stage& st = s->stages[k];
                zvx_stream::Stage& next = p.plan[k];         // (the planners in it have taken the step already)
                const zvx_plan::Step& sp = p.steps[k];
                const int64_t held = st.hist + n_in;
                float* in = st.buf[st.cur];
                if (sp.out_count > 0 && held > 0)
                    slot[st.kind][(size_t)i] = Slot{true, PostRow{in, dst_of(k + 1), (int32_t)held, RowsWindow{sp.in_origin, sp.out_begin, sp.out_count, last ? 1 : 0}, (int32_t)sp.out_count}};
                const int64_t drop = sp.keep_from - sp.in_origin, keep = held - drop;
                if (drop > 0) {                              // into the other buffer: never an overlapping copy
                    if (keep > 0) {
                        moves[M++] = StreamInterior{st.buf[st.cur ^ 1], in + drop, 0, (int)keep};
                        move_bytes += 8.0 * (double)keep; move_max = std::max<long>(move_max, (long)keep);
                    }
                    next.cur = st.cur ^ 1;
                }
                next.hist = keep;
                n_in = sp.out_count;
            }
        }
        char* tab_d = (char*)c->buf("stream.tab", STREAM_TAB_BYTES);
        float* rows_d = c->fbuf("stream.rows", (size_t)R * Pmax * nm);
        float* wav_d = c->fbuf("stream.wav", (size_t)R * wstride);
        c->upload(tab_d, tab.data(), (size_t)((char*)(moves + M) - tab.data()));
        const StreamRowTab ra{(const StreamRow*)tab_d, rows_d, R, Pmax, nm};
        const StreamInteriorTab ia{(const StreamInterior*)(ra.tab + R), wav_d, wstride, R};
        const StreamInteriorTab ma{ia.tab + R, nullptr, 0, M};               // (the scatter's kernel: every entry has its own source)
        // ---- gather, ONE batch of the vocoder at the native rate (the rows of ZeroVox._vocode_stream_native), scatter
        {
            TagScope scope(c, "voc.stream");
            c->timed(0.0, rows_bytes, [&] { launch_stream_rows(ra, c->stream); });
        }
        c->stage_begin(ZVX_T_VOCODER);
        run_vocoder(c, rows_d, nm, Pmax, P.data(), P.data(), R, wav_d, wstride, 0);
        c->stage_end(ZVX_T_VOCODER);
        {
            TagScope scope(c, "voc.stream");
            c->timed(0.0, new_bytes, [&] { launch_stream_interiors(ia, cnt_max, c->stream); });
        }
        // ---- the stages of one kind: a class is named by its first member, and is one call of the per-row form
        std::vector<int> cls((size_t)n), order((size_t)n), start((size_t)n + 1);
        std::vector<PostRow> rows;
        std::vector<uint64_t> keys;                          // (WATERMARK: the members' keys, in call order)
        auto per_class = [&](int kind, auto same, auto run) {
            for (int i = 0; i < n; i++) {
                cls[(size_t)i] = -1;
                if (!slot[kind][(size_t)i].run) continue;
                cls[(size_t)i] = i;
                for (int j = 0; j < i; j++)
                    if (cls[(size_t)j] == j && same(ss[j], ss[i])) { cls[(size_t)i] = j; break; }
            }
            const int groups = zvx_plan::partition_classes(cls.data(), n, order.data(), start.data());
            for (int gi = 0; gi < groups; gi++) {
                rows.clear(); keys.clear();
                for (int m = start[(size_t)gi]; m < start[(size_t)gi + 1]; m++) {
                    rows.push_back(slot[kind][(size_t)order[(size_t)m]].row);
                    keys.push_back(ss[order[(size_t)m]]->wm.key);
                }
                run(ss[order[(size_t)start[(size_t)gi]]]);
            }
        };
        per_class(zvx_stream::DENOISE, [](const zvx_stream* a, const zvx_stream* b) {
            return !memcmp(&a->dn, &b->dn, sizeof a->dn) && a->bias.size() == b->bias.size() && !memcmp(a->bias.data(), b->bias.data(), a->bias.size() * 4);
        }, [&](const zvx_stream* first) { run_denoise_rows(c, dn_geom(c, who), rows.data(), (int)rows.size(), first->bias.data(), &first->dn, 0); });
        per_class(zvx_stream::LEVEL, [](const zvx_stream* a, const zvx_stream* b) {
            return a->native == b->native && !memcmp(&a->lvl, &b->lvl, sizeof a->lvl);
        }, [&](const zvx_stream* first) { run_level_rows(c, rows.data(), (int)rows.size(), first->native, &first->lvl, first->lvl_g, 0); });   // (the gain words are not read)
        per_class(zvx_stream::WATERMARK, [](const zvx_stream* a, const zvx_stream* b) {
            // every field but the key, bit for bit (the key is the member's own: one call marks every key of the class)
            const float fa[3] = {a->wm.depth_db, a->wm.lo_hz, a->wm.hi_hz}, fb[3] = {b->wm.depth_db, b->wm.lo_hz, b->wm.hi_hz};
            return !memcmp(fa, fb, sizeof fa) && a->wm.block_frames == b->wm.block_frames && a->wm.band_bins == b->wm.band_bins &&
                   a->wm.period_blocks == b->wm.period_blocks && a->wm.reserved == b->wm.reserved;
        }, [&](const zvx_stream* first) { run_watermark_rows(c, first->wm_plan, rows.data(), (int)rows.size(), &first->wm, 0, keys.data()); });
        per_class(zvx_stream::LIMIT, [](const zvx_stream* a, const zvx_stream* b) {
            return a->lim_W == b->lim_W && a->lim.oversample == b->lim.oversample && !memcmp(&a->lim.ceiling, &b->lim.ceiling, sizeof(float));
        }, [&](const zvx_stream* first) { run_limit_rows(c, who, rows.data(), (int)rows.size(), &first->lim, first->lim_W, 0); });
        per_class(zvx_stream::RESAMPLE, [](const zvx_stream* a, const zvx_stream* b) { return a->native == b->native && a->out_rate == b->out_rate; },
                  [&](const zvx_stream* first) {
            int L = 1, Mr = 1;
            rs_pair(first->native, first->out_rate, &L, &Mr);
            run_resample_rows(c, rs_bank(c, L, Mr), rows.data(), (int)rows.size(), 0);
        });
        // ---- every history drop of the call in one launch
        if (M > 0) {
            TagScope scope(c, "post.stream");
            c->timed(0.0, move_bytes, [&] { launch_stream_interiors(ma, move_max, c->stream); });
        }
        // ---- everything is queued: the sessions' state
        for (int i = 0; i < n; i++) {
            zvx_stream* s = ss[i];
            StreamStep& p = plans[i];
            s->stages.swap(p.plan);
            s->next_chunk = p.g.first + p.g.rows; s->emitted += p.n; s->done = p.g.last ? 1 : 0;
            done[i] = s->done;
        }
        if (!(flags & ZVX_DEVICE_OUT)) {
            for (int i = 0; i < n; i++)
                if (n_out[i] > 0) HIPCHK(hipMemcpyAsync(ss[i]->pinned, ss[i]->ostage, (size_t)n_out[i] * 4, hipMemcpyDeviceToHost, c->stream));
            c->sync();                                       // the call's one wait
            for (int i = 0; i < n; i++)
                if (n_out[i] > 0) memcpy(out[i], ss[i]->pinned, (size_t)n_out[i] * 4);
        } else if (!(flags & ZVX_NO_SYNC)) c->sync();
    } catch (...) {
        for (int i = 0; i < n; i++) ss[i]->done = 1;
        throw;
    }
}
}  // namespace

// zvx_stream_next (include/zvx.h): its own checks, then the step of one session
void do_stream_next(zvx_stream* s, void* out, int64_t capacity, int64_t* n_out, int32_t* done, int flags) {
    const char* who = "zvx_stream_next";
    if (!n_out || !done) fail(ZVX_E_INVALID, "%s: %s is NULL", who, !n_out ? "n_out" : "done");
    stream_flags_check(who, flags);
    if (capacity < 0) fail(ZVX_E_INVALID, "%s: capacity %lld is negative", who, (long long)capacity);
    if (s->done) fail(ZVX_E_STATE, "%s: the stream is done (its last piece has been handed out)", who);
    StreamStep p;
    stream_plan_step(who, s, p);
    const int64_t n = p.n;
    *n_out = n;
    if (n > 0 && !out) fail(ZVX_E_INVALID, "%s: out is NULL", who);
    if (capacity < n) fail(ZVX_E_BUFFER, "%s: capacity %lld < %lld samples of this piece (nothing was consumed)", who, (long long)capacity, (long long)n);
    stream_step(who, s->c, &s, &p, 1, &out, n_out, done, flags);
}

// zvx_stream_next_many (include/zvx.h): its own checks and every session's plan, then the step of all of them
void do_stream_next_many(zvx_ctx* c, zvx_stream* const* ss, int n, void* const* out, const int64_t* capacity, int64_t* n_out, int32_t* done,
                         int flags) {
    const char* who = "zvx_stream_next_many";
    // ---- every check, before anything is planned or queued
    if (!capacity || !n_out || !done) fail(ZVX_E_INVALID, "%s: %s is NULL", who, !capacity ? "capacity" : !n_out ? "n_out" : "done");
    stream_flags_check(who, flags);
    if (n > STREAM_MANY_MAX_SESSIONS) fail(ZVX_E_UNSUPPORTED, "%s: %d sessions (at most %d per call)", who, n, STREAM_MANY_MAX_SESSIONS);
    for (int i = 0; i < n; i++) {
        if (!ss[i]) fail(ZVX_E_INVALID, "%s: sessions[%d] is NULL", who, i);
        if (ss[i]->c != c) fail(ZVX_E_INVALID, "%s: sessions[%d] belongs to another context than sessions[0]", who, i);
        for (int j = 0; j < i; j++) if (ss[j] == ss[i]) fail(ZVX_E_INVALID, "%s: sessions[%d] and sessions[%d] are the same session", who, j, i);
        if (capacity[i] < 0) fail(ZVX_E_INVALID, "%s: capacity[%d] %lld is negative", who, i, (long long)capacity[i]);
    }
    for (int i = 0; i < n; i++)
        if (ss[i]->done) fail(ZVX_E_STATE, "%s: sessions[%d] is done (its last piece has been handed out; nothing was consumed)", who, i);
    // ---- the plans of all sessions: every piece's size is known before anything is queued
    std::vector<StreamStep> plans((size_t)n);
    int R = 0, Pmax = 0;
    for (int i = 0; i < n; i++) R += std::min(ss[i]->cpc, ss[i]->nchunks - ss[i]->next_chunk);
    if (R > STREAM_MANY_MAX_ROWS) fail(ZVX_E_UNSUPPORTED, "%s: the groups of %d sessions are %d rows (at most %d per call)", who, n, R, STREAM_MANY_MAX_ROWS);
    for (int i = 0; i < n; i++) {
        stream_plan_step(who, ss[i], plans[(size_t)i]);
        n_out[i] = plans[(size_t)i].n;
        Pmax = std::max(Pmax, (int)plans[(size_t)i].g.Pmax);
    }
    if ((int64_t)R * Pmax * std::max(c->hop, c->n_mels) > (int64_t)1 << 28)
        fail(ZVX_E_UNSUPPORTED, "%s: %d rows of %d frames are %lld samples (at most 2^28 per call)", who, R, Pmax, (long long)R * Pmax * c->hop);
    for (int i = 0; i < n; i++)
        if (n_out[i] > 0 && (!out || !out[i])) fail(ZVX_E_INVALID, "%s: %s is NULL", who, !out ? "out" : ("out[" + std::to_string(i) + "]").c_str());
    for (int i = 0; i < n; i++)
        if (capacity[i] < n_out[i])
            fail(ZVX_E_BUFFER, "%s: capacity[%d] %lld < %lld samples of this piece (nothing was consumed in any session)", who, i,
                 (long long)capacity[i], (long long)n_out[i]);
    stream_step(who, c, ss, plans.data(), n, out, n_out, done, flags);
}

void do_stream_info(const zvx_stream* s, int64_t* info, int n_info) {
    if (!info || n_info < 1) fail(ZVX_E_INVALID, "zvx_stream_info: info is NULL or n_info %d < 1", n_info);
    const int64_t v[5] = {s->total, s->emitted, s->out_rate, s->delay, s->max_piece};
    for (int i = 0; i < n_info && i < 5; i++) info[i] = v[i];
}

}  // namespace zvx::host
