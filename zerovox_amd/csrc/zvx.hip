// zvx.hip -- libzvx weight loading, launch sequences (encoder, variance adaptor, mel decoders, vocoder, speaker encoder, log-mel front end,
// the measuring calls) and the C-ABI (include/zvx.h) but for zvx_comm_* (host_comm.hip).  The post-processing calls are in host_post.hip, the
// stream sessions in host_stream.hip; what the units share is in zvx_host.h.
#include "zvx_host.h"

namespace zvx::host {

thread_local std::string g_create_error;

// ------------------------------------------------------------------------------------------------
// manifest
// ------------------------------------------------------------------------------------------------

namespace {
void parse_manifest(zvx_ctx* c, const char* manifest, const void* weights, size_t nbytes) {
    if (!manifest || !weights) fail(ZVX_E_MANIFEST, "manifest/weights pointer is NULL");
    const size_t nfloats = nbytes / 4;
    c->host_blob.assign((const float*)weights, (const float*)weights + nfloats);
    std::stringstream ss(manifest);
    std::string line;
    bool first = true;
    while (std::getline(ss, line)) {
        if (line.empty()) continue;
        std::stringstream ls(line);
        std::string kw; ls >> kw;
        if (first) { if (kw != "zvx_manifest") fail(ZVX_E_MANIFEST, "manifest: bad magic '%s'", kw.c_str()); first = false; continue; }
        if (kw == "cfg") {
            std::string k, v; ls >> k; std::getline(ls, v);
            size_t p = v.find_first_not_of(' ');
            c->cfg[k] = p == std::string::npos ? "" : v.substr(p);
        } else if (kw == "tensor") {
            std::string name, kind; int nd = 0; ls >> name >> kind >> nd;
            Tensor t; t.kind = kind.empty() ? 'p' : kind[0]; t.numel = 1;
            for (int i = 0; i < nd; i++) { int d; ls >> d; t.dims.push_back(d); t.numel *= (size_t)d; }
            ls >> t.off;
            if (ls.fail() || t.off + t.numel > nfloats) fail(ZVX_E_MANIFEST, "manifest: tensor '%s' out of blob bounds", name.c_str());
            c->tensors[name] = t;
        } else {
            fail(ZVX_E_MANIFEST, "manifest: unknown line '%s'", line.c_str());
        }
    }
    if (first) fail(ZVX_E_MANIFEST, "manifest: empty");
}

// phoneme encoder (kept in f32 because it feeds discrete decisions): in the 16-bit mode its static-weight GEMMs run on the 16-bit
// MFMA as 3-plane split products (ops.hip: k_split3), f32-class accuracy at ~5x the f32 MFMA rate.
// Weights [taps][N][K] f32 -> 16-bit [taps][N][wh | wl | wh], fragment-packed like every other slab-kernel weight.  f16: IEEE-half
// planes scaled by 2^s per tensor (".s3h", Tensor.alpha = 2^-s), else bf16 planes (".s3").  Built from the f32 copies on the
// device, at load for the default mode and on the first zvx_set_int("enc_split", other mode).
void build_split_weights(zvx_ctx* c, bool f16) {
    const char* sfx = f16 ? ".s3h" : ".s3";
    if (c->has(std::string("enc.0.wqk") + sfx)) return;
    std::vector<std::pair<std::string, Tensor>> add;
    size_t stotal = 0;
    for (auto& kv : c->tensors) {
        const Tensor& t = kv.second;
        const bool mine = kv.first.rfind("enc.", 0) == 0;      // the variance predictors stay on the exact-f32 MFMA: N = 256 gives the
                                                                 // slab tiling too few workgroups to win, and their outputs are the decisions
        if (!mine || t.kind != 'f' || t.dtype != DT_F32 || t.dims.size() != 3 || (3 * t.dim(2)) % 16 || t.dim(1) % 8) continue;
        Tensor s3 = t;
        s3.kind = 's'; s3.dtype = f16 ? DT_F16 : DT_BF16; s3.dims = {t.dim(0), t.dim(1), 3 * t.dim(2)}; s3.numel = t.numel * 3; s3.host = nullptr;
        stotal += ((s3.numel * 2 + 255) & ~(size_t)255) + ((packed_weight_elems(s3.dim(0), s3.dim(1), s3.dim(2)) * 2 + 255) & ~(size_t)255);
        add.emplace_back(kv.first + sfx, s3);
    }
    char* sarena = stotal ? (char*)c->buf(f16 ? "weights_split_h" : "weights_split", stotal) : nullptr;
    float* mx_d = f16 ? c->fbuf("weights_split_absmax", 64) : nullptr;
    size_t soff = 0;
    for (auto& kv : add) {
        Tensor& s3 = kv.second;
        const Tensor& src = c->tensors[kv.first.substr(0, kv.first.size() - strlen(sfx))];
        float scale = 1.f;
        if (f16) {
            // s: max |w| 2^s in [2^14, 2^15) -- the hi plane uses the top of half's range, wl = w 2^s - wh stays normal down to
            // |w| ~ 2^-9 max |w| and the third plane (w 2^(s-11)) down to 2^-17 max |w|; below that the planes lose bits of an
            // element whose contribution is already < 2^-24 of the row's largest
            float mx = 0.f;
            launch_absmax((const float*)src.dev, src.numel, mx_d, c->stream);
            HIPCHK(hipMemcpyAsync(&mx, mx_d, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (!(mx > 0.f) || !std::isfinite(mx)) mx = 1.f;
            int e = 0; (void)frexpf(mx, &e);                 // mx = m 2^e, m in [0.5, 1)
            int sh = 15 - e; sh = std::max(-24, std::min(sh, 40));
            scale = ldexpf(1.f, sh);
            s3.alpha = ldexpf(1.f, -sh);
        }
        s3.dev = sarena + soff; soff += (s3.numel * 2 + 255) & ~(size_t)255;
        launch_split3_weights((const float*)src.dev, s3.dev, (long)src.dim(0) * src.dim(1), src.dim(2), c->stream, f16 ? 1 : 0, scale);
        void* pk = sarena + soff; soff += (packed_weight_elems(s3.dim(0), s3.dim(1), s3.dim(2)) * 2 + 255) & ~(size_t)255;
        launch_pack_weights(s3.dev, s3.dim(0), s3.dim(1), s3.dim(2), pk, c->stream);
        c->packed[s3.dev] = pk;
        c->tensors[kv.first] = s3;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
}

void upload_weights(zvx_ctx* c) {
    // one device arena for all tensors; 'w' tensors are converted to the context precision on device
    size_t total = 0;
    for (auto& kv : c->tensors) {
        Tensor& t = kv.second;
        t.dtype = (t.kind == 'w') ? c->dt : DT_F32;
        total += (t.numel * dtype_size(t.dtype) + 255) & ~(size_t)255;
    }
    char* arena = (char*)c->buf("weights", total);
    float* staging = c->fbuf("weights_staging", c->host_blob.size());
    HIPCHK(hipMemcpyAsync(staging, c->host_blob.data(), c->host_blob.size() * 4, hipMemcpyHostToDevice, c->stream));
    size_t off = 0;
    for (auto& kv : c->tensors) {
        Tensor& t = kv.second;
        t.dev = arena + off;
        t.host = c->host_blob.data() + t.off;
        launch_cast(staging + t.off, DT_F32, t.dev, t.dtype, t.numel, c->stream);
        off += (t.numel * dtype_size(t.dtype) + 255) & ~(size_t)255;
    }
    // fragment-order copies of every bf16 contraction weight [taps][N][K] with K % 16 == 0
    size_t ptotal = 0;
    for (auto& kv : c->tensors) {
        Tensor& t = kv.second;
        if (t.kind == 'w' && t.dtype == DT_BF16 && t.dims.size() == 3 && t.dim(2) % 8 == 0)
            ptotal += (packed_weight_elems(t.dim(0), t.dim(1), t.dim(2)) * 2 + 255) & ~(size_t)255;
    }
    if (ptotal) {
        char* parena = (char*)c->buf("weights_packed", ptotal);
        size_t poff = 0;
        for (auto& kv : c->tensors) {
            Tensor& t = kv.second;
            if (t.kind == 'w' && t.dtype == DT_BF16 && t.dims.size() == 3 && t.dim(2) % 8 == 0) {
                launch_pack_weights(t.dev, t.dim(0), t.dim(1), t.dim(2), parena + poff, c->stream);
                c->packed[t.dev] = parena + poff;
                poff += (packed_weight_elems(t.dim(0), t.dim(1), t.dim(2)) * 2 + 255) & ~(size_t)255;
            }
        }
    }
    // The mel decoders in IEEE half (bf16 mode): a second, f16 copy of their convolution / projection weights (cast from the f32 blob, fragment-packed
    // like the bf16 ones).  Same MFMA rate, 8x smaller rounding error on weights and activations (every tensor there sits behind a
    // norm: O(1..100), nowhere near 65504; stores saturate).  zvx_set_int("dec_f16", 0) runs the bf16 copies (A/B).
    if (c->dt == DT_BF16) {
        std::vector<std::pair<std::string, Tensor>> add16;
        size_t htotal = 0;
        for (auto& kv : c->tensors) {
            const Tensor& t = kv.second;
            // (round 5: the HiFi-GAN vocoder's weights too -- "voc.": its 16-bit tensors are IEEE half unless zvx_set_int("voc_f16", 0))
            if ((kv.first.rfind("sty.", 0) != 0 && kv.first.rfind("dec.", 0) != 0 && kv.first.rfind("voc.", 0) != 0) || t.kind != 'w' || t.dtype != DT_BF16 || t.dims.size() != 3 || t.dim(2) % 8) continue;
            Tensor hcopy = t; hcopy.dtype = DT_F16; hcopy.kind = 'h';
            htotal += ((t.numel * 2 + 255) & ~(size_t)255) + ((packed_weight_elems(t.dim(0), t.dim(1), t.dim(2)) * 2 + 255) & ~(size_t)255);
            add16.emplace_back(kv.first + ".h16", hcopy);
        }
        char* harena = htotal ? (char*)c->buf("weights_f16", htotal) : nullptr;
        size_t hoff = 0;
        for (auto& kv : add16) {
            Tensor& t = kv.second;
            t.dev = harena + hoff; hoff += (t.numel * 2 + 255) & ~(size_t)255;
            launch_cast(staging + t.off, DT_F32, t.dev, DT_F16, t.numel, c->stream);
            void* pk = harena + hoff; hoff += (packed_weight_elems(t.dim(0), t.dim(1), t.dim(2)) * 2 + 255) & ~(size_t)255;
            launch_pack_weights(t.dev, t.dim(0), t.dim(1), t.dim(2), pk, c->stream);
            c->packed[t.dev] = pk;
            c->tensors[kv.first] = t;
        }
    }
    // StyleTTS residual blocks with a learned shortcut (styletts.py:60-68, 130-139): out = (conv2(t) + conv1x1(x)) / sqrt(2).  The
    // shortcut runs INSIDE the k = 3 convolution as a second source of its K loop (GemmArgs::X2), which needs the two fragment
    // streams interleaved per 32-channel tile -- built once here, for the bf16 and the half copies
    for (const char* blk : {"sty.enc0", "sty.dec0", "sty.dec1", "sty.dec2"})
        for (const char* sfx : {"", ".h16"}) {
            const std::string n2 = std::string(blk) + ".c2" + sfx, ns = std::string(blk) + ".sc" + sfx;
            if (!c->has(n2) || !c->has(ns) || c->has(std::string(blk) + ".sc_b")) continue;
            const Tensor& t2 = c->t(n2); const Tensor& ts = c->t(ns);
            if (t2.dims.size() != 3 || ts.dims.size() != 3 || ts.dim(0) != 1 || ts.dim(1) != t2.dim(1) || !c->packed.count(t2.dev) || !c->packed.count(ts.dev)) continue;
            if (t2.dim(2) % 16 || ts.dim(2) % 16) continue;          // the conv-slab kernel alone takes a second source, in K chunks of 16 (launch_gemm): a hidden width of 72 runs the two launches
            const size_t bytes = (packed_weight_elems(t2.dim(0), t2.dim(1), t2.dim(2)) + packed_weight_elems(1, ts.dim(1), ts.dim(2))) * 2;
            void* comb = c->buf("weights_pair." + n2, bytes);
            launch_pack_pair(c->packed[t2.dev], t2.dim(0), t2.dim(2), c->packed[ts.dev], 1, ts.dim(2), t2.dim(1), comb, c->stream);
            c->pair_packed[t2.dev] = comb;
        }
    // f32 FFT blocks: Q, K and V projections as ONE GEMM (fs2.py:143-145) -- [Wq; Wk; Wv] and the biases concatenated once here
    {
        std::vector<std::pair<std::string, Tensor>> add;
        for (auto& kv : c->tensors) {
            const std::string& nm = kv.first;
            if (nm.size() < 5 || nm.compare(nm.size() - 4, 4, ".wqk") != 0) continue;          // every f32 FFT block: the encoder's, and the FS2 decoder's in f32 mode
            const std::string pre = nm.substr(0, nm.size() - 4);
            const Tensor& wqk = kv.second;
            if (!c->has(pre + ".wv") || !c->has(pre + ".bqk") || !c->has(pre + ".bv") || wqk.dtype != DT_F32 || wqk.dims.size() != 3) continue;
            const Tensor& wv = c->t(pre + ".wv");
            if (wv.dtype != DT_F32 || wv.dims.size() != 3 || wv.dim(2) != wqk.dim(2)) continue;
            Tensor w = wqk; w.dims = {1, wqk.dim(1) + wv.dim(1), wqk.dim(2)}; w.numel = wqk.numel + wv.numel; w.host = nullptr;
            w.dev = c->buf(pre + ".wqkv", w.numel * 4);
            HIPCHK(hipMemcpyAsync(w.dev, wqk.dev, wqk.numel * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync((float*)w.dev + wqk.numel, wv.dev, wv.numel * 4, hipMemcpyDeviceToDevice, c->stream));
            const Tensor& bqk = c->t(pre + ".bqk"); const Tensor& bv = c->t(pre + ".bv");
            Tensor bb = bqk; bb.dims = {(int)(bqk.numel + bv.numel)}; bb.numel = bqk.numel + bv.numel; bb.host = nullptr;
            bb.dev = c->buf(pre + ".bqkv", bb.numel * 4);
            HIPCHK(hipMemcpyAsync(bb.dev, bqk.dev, bqk.numel * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync((float*)bb.dev + bqk.numel, bv.dev, bv.numel * 4, hipMemcpyDeviceToDevice, c->stream));
            add.emplace_back(pre + ".wqkv", w); add.emplace_back(pre + ".bqkv", bb);
        }
        for (auto& kv : add) c->tensors[kv.first] = kv.second;
    }
    // half FFT blocks (the FS2 / SCLN decoder in the 16-bit mode): Q, K and V projections as ONE GEMM too (round 6) -- [Wq; Wk; Wv] in IEEE half,
    // fragment-packed, and the concatenated f32 biases
    {
        std::vector<std::pair<std::string, Tensor>> add;
        for (auto& kv : c->tensors) {
            const std::string& nm = kv.first;
            const std::string sfx = ".wqk.h16";
            if (nm.size() <= sfx.size() || nm.compare(nm.size() - sfx.size(), sfx.size(), sfx) != 0) continue;
            const std::string pre = nm.substr(0, nm.size() - sfx.size());
            if (!c->has(pre + ".wv.h16") || !c->has(pre + ".bqk") || !c->has(pre + ".bv")) continue;
            const Tensor& wqk = kv.second; const Tensor& wv = c->t(pre + ".wv.h16");
            if (wqk.dims.size() != 3 || wv.dims.size() != 3 || wqk.dim(0) != 1 || wv.dim(0) != 1 || wv.dim(2) != wqk.dim(2) || wqk.dim(2) % 8) continue;
            Tensor w = wqk; w.dims = {1, wqk.dim(1) + wv.dim(1), wqk.dim(2)}; w.numel = wqk.numel + wv.numel; w.host = nullptr;
            w.dev = c->buf(pre + ".wqkv.h16", w.numel * 2);
            HIPCHK(hipMemcpyAsync(w.dev, wqk.dev, wqk.numel * 2, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync((char*)w.dev + wqk.numel * 2, wv.dev, wv.numel * 2, hipMemcpyDeviceToDevice, c->stream));
            void* pk = c->buf(pre + ".wqkv.h16.packed", packed_weight_elems(1, w.dim(1), w.dim(2)) * 2);
            launch_pack_weights(w.dev, 1, w.dim(1), w.dim(2), pk, c->stream);
            c->packed[w.dev] = pk;
            add.emplace_back(pre + ".wqkv.h16", w);
            if (!c->has(pre + ".bqkv")) {
                const Tensor& bqk = c->t(pre + ".bqk"); const Tensor& bv = c->t(pre + ".bv");
                Tensor bb = bqk; bb.dims = {(int)(bqk.numel + bv.numel)}; bb.numel = bqk.numel + bv.numel; bb.host = nullptr;
                bb.dev = c->buf(pre + ".bqkv", bb.numel * 4);
                HIPCHK(hipMemcpyAsync(bb.dev, bqk.dev, bqk.numel * 4, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(hipMemcpyAsync((float*)bb.dev + bqk.numel, bv.dev, bv.numel * 4, hipMemcpyDeviceToDevice, c->stream));
                add.emplace_back(pre + ".bqkv", bb);
            }
        }
        for (auto& kv : add) c->tensors[kv.first] = kv.second;
    }
    if (c->enc_split) build_split_weights(c, c->enc_split == 2);
    HIPCHK(hipStreamSynchronize(c->stream));
    DevBuf& st = c->bufs["weights_staging"];
    HIPCHK(hipFree(st.base)); st.base = nullptr; st.p = nullptr; st.cap = 0;
}

void read_config(zvx_ctx* c) {
    auto it = c->cfg.find("precision");
    if (it == c->cfg.end()) fail(ZVX_E_MANIFEST, "manifest: missing cfg 'precision'");
    if (it->second == "bf16") c->dt = DT_BF16; else if (it->second == "f32") c->dt = DT_F32;
    else fail(ZVX_E_MANIFEST, "manifest: unknown precision '%s'", it->second.c_str());
    c->enc_split = c->dt == DT_BF16 ? (c->cfg.count("enc_split") ? std::max(0, std::min(2, c->cfg_int("enc_split"))) : 2) : 0;
    c->H = c->cfg_int("hidden"); c->emb_dim = c->cfg_int("emb_dim"); c->punct_dim = c->cfg_int("punct_dim");
    c->n_phone_rows = c->cfg_int("n_phone_rows"); c->n_punct_rows = c->cfg_int("n_punct_rows");
    c->max_txt_len = c->cfg_int("max_txt_len"); c->max_mel_len = c->cfg_int("max_mel_len");
    c->enc_layers = c->cfg_int("enc_layers"); c->enc_heads = c->cfg_int("enc_heads"); c->ffn_dim = c->cfg_int("ffn_dim");
    auto fk = c->cfg_list("ffn_k"); if (fk.size() != 2) fail(ZVX_E_MANIFEST, "manifest: ffn_k needs 2 entries");
    c->ffn_k0 = fk[0]; c->ffn_k1 = fk[1];
    c->vp_dim = c->cfg_int("vp_dim"); c->vp_k = c->cfg_int("vp_k"); c->n_bins = c->cfg_int("n_bins");
    c->dec_layers = c->cfg_int("dec_layers"); c->dec_heads = c->cfg_int("dec_heads"); c->dec_scln = c->cfg_int("dec_scln");
    c->n_mels = c->cfg_int("n_mels"); c->hop = c->cfg_int("hop"); c->res_dim = c->cfg_int("res_dim");
    c->rn_layers = c->cfg_list("rn_layers"); c->rn_filters = c->cfg_list("rn_filters"); c->rn_asp = c->cfg_int("rn_asp");
    const std::string dk = c->cfg["dec_kind"];
    if (dk == "fastspeech2") c->dec_kind = 0; else if (dk == "styletts") c->dec_kind = 1;
    else fail(ZVX_E_MANIFEST, "unknown decoder kind: '%s'", dk.c_str());                 // model.py:244
    c->voc_resblock = c->cfg_int("voc_resblock"); c->voc_c0 = c->cfg_int("voc_c0");
    c->voc_rates = c->cfg_list("voc_rates"); c->voc_ksizes = c->cfg_list("voc_ksizes"); c->voc_rb_k = c->cfg_list("voc_rb_k");
    {
        std::stringstream ss(c->cfg["voc_rb_d"]); std::string grp;
        while (std::getline(ss, grp, ';')) {
            std::vector<int> v; std::stringstream gs(grp); std::string tok;
            while (std::getline(gs, tok, ',')) if (!tok.empty()) v.push_back(atoi(tok.c_str()));
            c->voc_rb_d.push_back(v);
        }
    }
    int prod = 1; for (int r : c->voc_rates) prod *= r;
    if (prod != c->hop) fail(ZVX_E_MANIFEST, "prod(voc_rates)=%d != hop=%d", prod, c->hop);
    if (c->voc_rb_d.size() != c->voc_rb_k.size()) fail(ZVX_E_MANIFEST, "voc_rb_d / voc_rb_k size mismatch");
    // The generator shapes the device runs (pack.check_generator_config makes the same checks and derives them; a manifest can be written
    // by hand).  ConvTranspose1d(stride u, kernel k, padding (k - u) / 2) yields T u rows only for an even k - u, and the three polyphase
    // taps (input rows t - 1, t, t + 1) cover the kernel iff (k - u) / 2 <= u, i.e. k <= 3u; the channel width halves per stage and the
    // 16-bit kernels (and conv_post) read the channel axis in 16-byte groups: 8 elements, 4 in f32
    const int ns = (int)c->voc_rates.size();
    if (c->voc_resblock != 1 && c->voc_resblock != 2) fail(ZVX_E_MANIFEST, "voc_resblock=%d is neither 1 nor 2", c->voc_resblock);
    if (ns < 1 || ns > 16 || c->voc_ksizes.size() != c->voc_rates.size()) fail(ZVX_E_MANIFEST, "voc_ksizes has %d entries for %d voc_rates", (int)c->voc_ksizes.size(), ns);
    for (int i = 0; i < ns; i++) {
        const int u = c->voc_rates[i], k = c->voc_ksizes[i];
        if (u < 1 || k < u) fail(ZVX_E_MANIFEST, "voc_ksizes[%d]=%d is smaller than voc_rates[%d]=%d", i, k, i, u);
        if ((k - u) % 2) fail(ZVX_E_UNSUPPORTED, "voc_ksizes[%d]=%d with voc_rates[%d]=%d: k - u is odd, the ConvTranspose1d would yield T*u + 1 rows", i, k, i, u);
        if (k > 3 * u) fail(ZVX_E_UNSUPPORTED, "voc_ksizes[%d]=%d exceeds 3 * voc_rates[%d]=%d: three polyphase taps do not cover the kernel", i, k, i, 3 * u);
    }
    const int cunit = c->dt == DT_F32 ? 4 : 8;
    if (c->voc_c0 < 1 || c->voc_c0 % (1 << ns) || (c->voc_c0 >> ns) % cunit)
        fail(ZVX_E_UNSUPPORTED, "voc_c0=%d: the last of %d stages needs a multiple of %d channels in precision %s", c->voc_c0, ns, cunit, c->cfg["precision"].c_str());
    if (c->voc_rb_k.empty()) fail(ZVX_E_MANIFEST, "voc_rb_k is empty");
    for (size_t j = 0; j < c->voc_rb_k.size(); j++) {
        if (c->voc_rb_k[j] < 1 || c->voc_rb_k[j] % 2 == 0) fail(ZVX_E_MANIFEST, "voc_rb_k[%d]=%d must be odd", (int)j, c->voc_rb_k[j]);
        if (c->voc_rb_k[j] > ZVX_MAX_TAPS) fail(ZVX_E_UNSUPPORTED, "voc_rb_k[%d]=%d exceeds the %d taps of a convolution launch", (int)j, c->voc_rb_k[j], ZVX_MAX_TAPS);
        if (c->voc_rb_d[j].empty()) fail(ZVX_E_MANIFEST, "voc_rb_d[%d] is empty", (int)j);
        for (int d : c->voc_rb_d[j]) if (d < 1) fail(ZVX_E_MANIFEST, "voc_rb_d[%d] holds the dilation %d", (int)j, d);
    }
    // The front-end shapes the device runs (pack.check_model_config makes the same checks; a manifest can be written by hand).  What the
    // launchers need of each width:
    //   hidden, head depth   multiples of 8: 16-byte groups of the 16-bit kernels (gemm_kernel's K chunks, k_colstats / k_instnorm_fused /
    //                        k_norm_affine_act: 8 channels per lane, in f32 too); a head's columns start at h * depth inside a Q | K row
    //   ffn_k                odd (fs2.py:189-196 pads (k - 1) / 2) and <= ZVX_MAX_TAPS (launch_gemm)
    //   vp_dim               a multiple of 4: the predictors run in f32 (launch_gemm: N % 4 with a bias; float4 K chunks)
    //   ffn_dim              as N and K of the FFT blocks: 8 elements in the 16-bit precision (the FS2 decoder), 4 floats in f32
    //   n_mels               a multiple of 8 (k_colstats over the reference mel; the pooled map has n_mels / 8 frequency rows, one tap each
    //                        of the first attention projection: <= 8 * ZVX_MAX_TAPS), and conv_pre's K
    //   rn_filters           multiples of 8 (k_spk_front, k_se_pool_partial, k_se_apply: 8 channels per thread), <= 256 (k_se_pool_partial
    //                        folds with one thread per channel)
    // vp_k != 3 is refused by the first zvx_encode (ZVX_E_UNSUPPORTED), as before.
    if (c->H < 8 || c->H % 8) fail(ZVX_E_UNSUPPORTED, "hidden=%d must be a multiple of 8", c->H);
    if (c->emb_dim + c->punct_dim != c->H) fail(ZVX_E_MANIFEST, "hidden=%d is not emb_dim + punct_dim = %d + %d", c->H, c->emb_dim, c->punct_dim);
    const struct { const char* key; int heads; } hd[2] = {{"enc_heads", c->enc_heads}, {"dec_heads", c->dec_heads}};
    for (const auto& h : hd) {
        if (h.heads < 1 || c->H % h.heads) fail(ZVX_E_UNSUPPORTED, "%s=%d does not divide hidden=%d", h.key, h.heads, c->H);
        if ((c->H / h.heads) % 8) fail(ZVX_E_UNSUPPORTED, "%s=%d: head depth %d (hidden=%d) must be a multiple of 8", h.key, h.heads, c->H / h.heads, c->H);
    }
    for (int i = 0; i < 2; i++) {
        const int k = i ? c->ffn_k1 : c->ffn_k0;
        if (k < 1 || k % 2 == 0) fail(ZVX_E_UNSUPPORTED, "ffn_k[%d]=%d must be odd", i, k);
        if (k > ZVX_MAX_TAPS) fail(ZVX_E_UNSUPPORTED, "ffn_k[%d]=%d exceeds the %d taps of a convolution launch", i, k, ZVX_MAX_TAPS);
    }
    if (c->vp_dim < 4 || c->vp_dim % 4) fail(ZVX_E_UNSUPPORTED, "vp_dim=%d must be a multiple of 4", c->vp_dim);
    if (c->ffn_dim < cunit || c->ffn_dim % cunit) fail(ZVX_E_UNSUPPORTED, "ffn_dim=%d must be a multiple of %d in precision %s", c->ffn_dim, cunit, c->cfg["precision"].c_str());
    if (c->n_bins < 2) fail(ZVX_E_UNSUPPORTED, "n_bins=%d must be at least 2", c->n_bins);
    if (c->enc_layers < 1 || c->dec_layers < 1) fail(ZVX_E_MANIFEST, "enc_layers=%d / dec_layers=%d must be positive", c->enc_layers, c->dec_layers);
    if (c->n_mels < 8 || c->n_mels % 8 || c->n_mels > 8 * ZVX_MAX_TAPS) fail(ZVX_E_UNSUPPORTED, "n_mels=%d must be a multiple of 8, at most %d", c->n_mels, 8 * ZVX_MAX_TAPS);
    if (c->rn_filters.size() != 4 || c->rn_layers.size() != 4) fail(ZVX_E_MANIFEST, "rn_filters / rn_layers need 4 entries each");
    for (int i = 0; i < 4; i++) {
        if (c->rn_layers[i] < 1) fail(ZVX_E_MANIFEST, "rn_layers[%d]=%d must be positive", i, c->rn_layers[i]);
        if (c->rn_filters[i] < 8 || c->rn_filters[i] % 8 || c->rn_filters[i] > 256) fail(ZVX_E_UNSUPPORTED, "rn_filters[%d]=%d must be a multiple of 8, at most 256", i, c->rn_filters[i]);
    }
    if (c->has("voc.pre_w") && (c->t("voc.pre_w").dims.size() != 3 || c->t("voc.pre_w").dim(2) != c->n_mels))
        fail(ZVX_E_MANIFEST, "n_mels=%d, but voc.pre_w (the generator's conv_pre) takes %d channels", c->n_mels, c->t("voc.pre_w").dims.size() == 3 ? c->t("voc.pre_w").dim(2) : -1);
    // The STFT the log-mel front end runs (mel_from_padded; pack.check_model_config makes the same checks).  The frame GEMM reads a frame as
    // K = fft_size floats in 16-byte chunks guarded per chunk (gemm_kernel: k < Kb): a fft_size that is no multiple of 4 would let the last
    // chunk of a frame read on into the signal, against basis elements of the NEXT basis row.  hop > fft_size makes the reflect padding
    // (fft_size - hop) / 2 negative.  The two constant matrices have the shapes these two numbers give.
    if (c->cfg.count("fft_size") || c->has("mel.dft")) {
        const int n_fft = c->cfg_int("fft_size"), nf = n_fft / 2 + 1;
        if (n_fft < 4 || n_fft % 4) fail(ZVX_E_UNSUPPORTED, "fft_size=%d must be a multiple of 4 (the frame GEMM reads a frame in groups of 4 floats)", n_fft);
        if (c->hop < 1 || c->hop > n_fft) fail(ZVX_E_UNSUPPORTED, "hop=%d must lie in 1..fft_size=%d (the reflect padding is (fft_size - hop) / 2)", c->hop, n_fft);
        const Tensor& dft = c->t("mel.dft");
        if (dft.dims.size() != 3 || dft.dim(2) != n_fft || dft.dim(1) != ((2 * nf + 3) & ~3))
            fail(ZVX_E_MANIFEST, "mel.dft is not [1][%d][fft_size=%d]", (2 * nf + 3) & ~3, n_fft);
        const Tensor& mb = c->t("mel.basis");
        if (mb.dims.size() != 3 || mb.dim(1) != c->n_mels || mb.dim(2) != ((nf + 3) & ~3))
            fail(ZVX_E_MANIFEST, "mel.basis is not [1][n_mels=%d][%d] (fft_size=%d)", c->n_mels, (nf + 3) & ~3, n_fft);
    }
}

// ------------------------------------------------------------------------------------------------
// FFT block (fs2.py:221-230): x [B][Lmax][H] (dtype dt) -> x, in place.
// ------------------------------------------------------------------------------------------------
struct FftWeights { std::string p; bool scln; const float* bg; long bg_bs; const float* post_add; };

// Ls: rows per utterance of x and of every row-major buffer below (>= Lmax).  Ls > Lmax + the k = 9 convolution's halo lets the
// static-weight GEMMs run batch-flattened (GemmArgs::bflat; `flat`): the FS2 decoder's 896 frames are 3.5 tiles of 256 rows.
void fft_block(zvx_ctx* c, void* x, int dt, int B, int Lmax, const int* len_dev, int nheads, const FftWeights& w, int Ls = 0, bool flat = false) {
    if (Ls <= 0) Ls = Lmax;
    const int H = c->H, d = H / nheads, Lp = (Lmax + 7) & ~7, F = c->ffn_dim;
    const size_t es = dtype_size(dt);
    const bool h16 = dt == DT_F16;                                               // the 16-bit tensors of this block are IEEE half (weights: the ".h16" copies)
    auto wdev = [&](const char* n) { return c->t(w.p + n + (h16 ? ".h16" : "")).dev; };
    void* qk = c->buf("fft.qk", (size_t)B * Ls * 2 * H * es);
    void* vt = c->buf("fft.vt", (size_t)B * H * Lp * es);
    float* sc = c->fbuf("fft.scores", (size_t)B * nheads * Lmax * Lp);
    void* P = c->buf("fft.P", (size_t)B * nheads * Lmax * Lp * es);
    void* o = c->buf("fft.o", (size_t)B * Ls * H * es);
    float* y = c->fbuf("fft.y", (size_t)B * Ls * H);
    // half blocks (the FS2 / SCLN decoder in the 16-bit mode; round 6): the pre-norm sums y = fc(O) + x and y = conv_k1(h) + x leave their GEMMs
    // as IEEE half through the compile-time decoder epilogue (raw 16-bit residual, ZVX_EPI_DEC) instead of f32 through the run-time one, and the
    // LayerNorm / SCLN pass reads 2 bytes per element instead of 4: one more rounding at 2^-11 of a value the norm then rescales
    void* const yv = h16 ? c->buf("fft.y16", (size_t)B * Ls * H * 2) : (void*)y;
    const int ydt = h16 ? (int)DT_F16 : (int)DT_F32;
    void* hbuf = c->buf("fft.h", (size_t)B * Ls * F * es);

    // f32 blocks (phoneme encoder) in bf16 mode: the static-weight GEMMs take bf16 split planes [hi | hi | lo] of their f32 input
    // against [wh | wl | wh] weights (K = 3 x the logical K): f32-class results from the bf16 MFMA
    const bool sp16 = c->enc_split == 2;                                          // IEEE-half planes (f32-class to 2^-24) / bf16 planes (2^-17)
    const char* const s3 = sp16 ? ".s3h" : ".s3";
    // (all four static-weight GEMMs or none: build_split_weights makes planes of a tensor only where 3 K is a multiple of 16)
    const bool split = dt == DT_F32 && c->enc_split && c->has(w.p + ".wqk" + s3) && c->has(w.p + ".wo" + s3) && c->has(w.p + ".w1" + s3) && c->has(w.p + ".w2" + s3);
    void* xs = split ? c->buf("fft.xs", (size_t)B * Ls * 3 * H * 2) : nullptr;
    auto split_of = [&](const float* src, int C, void* dst) { launch_split3(src, C, dst, B, Ls, len_dev, C, c->stream, sp16); };
    auto as_split = [&](GemmArgs& a, const void* planes, int C, const std::string& wname) {      // operand swap: same GEMM, 3-plane K axis
        const Tensor& ws = c->t(wname + s3);
        a.dtype = sp16 ? DT_F16 : DT_BF16; a.X = planes; a.x_bs = (long)Ls * 3 * C; a.ldx = 3 * C; a.K = 3 * C;
        a.alpha = ws.alpha;                                                                        // half planes carry w 2^s
        a.W = ws.dev; a.ldw = 3 * C; a.w_ts = (long)ws.dim(1) * 3 * C;
        a.flops = 2.0 * (double)a.M * a.nbatch * a.N * C * a.ntaps;                                 // algorithmic (f32) work, not the 3x issued
    };
    // exact-f32 blocks with merged projection weights: one Q | K | V GEMM + one fused attention launch (attention.hip)
    AttnF32Args af;
    memset(&af, 0, sizeof af);
    af.ld = 3 * H; af.bs = (long)Ls * 3 * H; af.q_off = 0; af.k_off = H; af.v_off = 2 * H;
    af.out = (float*)o; af.o_bs = (long)Ls * H; af.ldo = H; af.len = len_dev; af.L = Lmax; af.D = d; af.nheads = nheads; af.nbatch = B;
    af.scale = (float)(1.0 / pow((double)d, 0.5));
    const bool fused_f32 = dt == DT_F32 && c->use_attn_f32 && c->has(w.p + ".wqkv") && launch_attention_f32(af, c->stream, true);
    // split planes of a GEMM input come from its PRODUCER where that is one of ours (LayerNorm, the fused attention, the k = 9
    // convolution's epilogue); k_split3 runs only for the block input of the first layer and on the unfused attention path
    const bool xs_from_producer = split && c->fft_xs_ready == x;
    if (split && !xs_from_producer) split_of((const float*)x, H, xs);
    c->fft_xs_ready = nullptr;
    if (fused_f32) {
        float* qkv = c->fbuf("fft.qkv", (size_t)B * Ls * 3 * H);
        GemmArgs a = gemm_base(dt);
        a.X = x; a.x_bs = (long)Ls * H; a.ldx = H; a.W = c->t(w.p + ".wqkv").dev; a.ldw = H;
        a.M = Lmax; a.N = 3 * H; a.K = H; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        if (split) { as_split(a, xs, H, w.p + ".wqkv"); a.out_dtype = DT_F32; }
        a.bias = c->pf(w.p + ".bqkv"); a.bias_mode = 1;
        a.out = qkv; a.o_bs = (long)Ls * 3 * H; a.ldo = 3 * H;
        c->gemm(a);
        af.qkv = qkv;
        if (split) { af.planes = (unsigned short*)xs; af.planes_C = H; af.planes_f16 = sp16; }   // o as split planes for the output projection
        c->timed(4.0 * B * nheads * (double)Lmax * Lmax * d, (double)B * Lmax * 4.0 * H * 4, [&] { launch_attention_f32(af, c->stream, false); }, "attention_f32");
    } else {
    if (split) split_of((const float*)x, H, xs);
    // half blocks: [Q | K | V] = x [Wq; Wk; Wv]^T + b in ONE launch (round 6), then the 16-bit transpose of its V columns
    // (upload_weights builds ".wqkv.h16" for every half block the packer writes)
    void* qkvbuf = h16 ? c->buf("fft.qkv16", (size_t)B * Ls * 3 * H * es) : nullptr;
    if (h16) {
        GemmArgs a = gemm_base(dt);
        a.X = x; a.x_bs = (long)Ls * H; a.ldx = H; a.W = c->t(w.p + ".wqkv.h16").dev; a.ldw = H;
        a.M = Lmax; a.N = 3 * H; a.K = H; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        a.bias = c->pf(w.p + ".bqkv"); a.bias_mode = 1;
        a.out = qkvbuf; a.o_bs = (long)Ls * 3 * H; a.ldo = 3 * H;
        c->gemm(a);
        c->timed(0, (double)B * Lmax * H * 4.0, [&] { launch_transpose16((const char*)qkvbuf + (size_t)2 * H * es, 3 * H, vt, Lp, B, Ls, H, c->stream, len_dev); });
    } else {
    {   // [Q | K] = x Wqk^T + b                                       fs2.py:143-144
        GemmArgs a = gemm_base(dt);
        a.X = x; a.x_bs = (long)Ls * H; a.ldx = H; a.W = wdev(".wqk"); a.ldw = H;
        a.M = Lmax; a.N = 2 * H; a.K = H; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        if (split) { as_split(a, xs, H, w.p + ".wqk"); a.out_dtype = DT_F32; }
        a.bias = c->pf(w.p + ".bqk"); a.bias_mode = 1;
        a.out = qk; a.o_bs = (long)Ls * 2 * H; a.ldo = 2 * H;
        c->gemm(a);
    }
    {   // V^T[h*d + j][l] = Wv x^T + b  (stored transposed so that P.V is K-contiguous)   fs2.py:145
        GemmArgs a = gemm_base(dt);
        a.X = c->t(w.p + ".wv").dev; a.x_bs = 0; a.ldx = H; a.W = x; a.w_bs = (long)Ls * H; a.ldw = H;
        a.M = H; a.N = Lmax; a.K = H; a.nbatch = B; a.in_len_static = H;
        a.bias = c->pf(w.p + ".bv"); a.bias_mode = 2;
        a.out = vt; a.o_bs = (long)H * Lp; a.ldo = Lp;
        // columns in [len, Lmax) hold finite junk (x rows beyond len are never NaN: buffers start zeroed and
        // only ever receive finite values); P is exactly zero there, so they never contribute.  The pad columns [Lmax, Lp) are not
        // written by this GEMM and the buffer is shared between the f32 encoder and the bf16 decoder (stale bits of one can read
        // as Inf / NaN in the other, and 0 * NaN = NaN in the P.V product): zero them
        if (Lp > Lmax) HIPCHK(hipMemset2DAsync((char*)vt + (size_t)Lmax * es, (size_t)Lp * es, 0, (size_t)(Lp - Lmax) * es, (size_t)B * H, c->stream));
        c->gemm(a);
        // ... and round 5: the columns [len, Lmax) as well -- "finite junk" held only as long as every row of x past an
        // utterance's length had been defined by something; nothing guarantees that (tests: zvx_set_int("poison_pads", 1))
        launch_zero_tail_cols(vt, (int)es, Lp, (long)H * Lp, B, H, Lmax, len_dev, c->stream);
    }
    }
    FlashArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.qk = qk; fa.qk_bs = (long)Ls * 2 * H; fa.ldq = 2 * H; fa.k_off = H; fa.vt = vt;
    if (h16) { fa.qk = qkvbuf; fa.qk_bs = (long)Ls * 3 * H; fa.ldq = 3 * H; } fa.vt_bs = (long)H * Lp; fa.ldv = Lp;
    fa.out = o; fa.o_bs = (long)Ls * H; fa.ldo = H; fa.len = len_dev; fa.L = Lmax; fa.D = d; fa.nheads = nheads; fa.nbatch = B;
    fa.scale = (float)(1.0 / pow((double)d, 0.5));
    fa.f16 = h16;
    const bool flash = (dt == DT_BF16 || h16) && c->use_flash && launch_flash_attention(fa, c->stream, true);
    if (h16 && !flash) fail(ZVX_E_UNSUPPORTED, "half-precision FFT block without the fused attention (head depth %d)", d);
    if (flash) {
        // softmax(Q K^T / sqrt(d)) V in one launch, scores and probabilities stay on chip            fs2.py:47-58
        c->timed(4.0 * B * nheads * (double)Lmax * Lmax * d, (double)B * Lmax * (3.0 * H + H) * es, [&] { launch_flash_attention(fa, c->stream, false); }, h16 ? "flash_attention_f16" : "flash_attention_bf16");
        c->sat_scan(o, dt, (long)Ls * H, H, B, Lmax, len_dev, H);
    } else {
    {   // scores = Q K^T / sqrt(d)                                    fs2.py:49-50
        GemmArgs a = gemm_base(dt);
        a.X = qk; a.x_bs = (long)Ls * 2 * H; a.x_hs = d; a.ldx = 2 * H;
        a.W = (const char*)qk + (size_t)H * es; a.w_bs = (long)Ls * 2 * H; a.w_hs = d; a.ldw = 2 * H;
        a.M = Lmax; a.N = Lmax; a.K = d; a.nbatch = B; a.nheads = nheads; a.in_len = len_dev; a.out_len = len_dev;
        a.alpha = (float)(1.0 / pow((double)d, 0.5));
        a.out = sc; a.out_dtype = DT_F32; a.o_bs = (long)nheads * Lmax * Lp; a.o_hs = (long)Lmax * Lp; a.ldo = Lp;
        a.flops = 2.0 * B * nheads * (double)Lmax * Lmax * d;
        c->gemm(a);
    }
    c->timed(0, (double)B * nheads * Lmax * Lp * (4.0 + es), [&] { launch_softmax_rows(sc, Lp, P, dt, Lp, B, nheads, Lmax, len_dev, c->stream); });      // fs2.py:52-55
    {   // O = P V                                                      fs2.py:56
        GemmArgs a = gemm_base(dt);
        a.X = P; a.x_bs = (long)nheads * Lmax * Lp; a.x_hs = (long)Lmax * Lp; a.ldx = Lp;
        a.W = vt; a.w_bs = (long)H * Lp; a.w_hs = (long)d * Lp; a.ldw = Lp;
        a.M = Lmax; a.N = d; a.K = Lp; a.k_len = len_dev; a.nbatch = B; a.nheads = nheads; a.in_len = len_dev; a.out_len = len_dev;
        a.out = o; a.o_bs = (long)Ls * H; a.o_hs = d; a.ldo = H;
        a.flops = 2.0 * B * nheads * (double)Lmax * Lmax * d;
        c->gemm(a);
    }
    }
    }
    {   // y = fc(O) + residual                                         fs2.py:158-162
        GemmArgs a = gemm_base(dt);
        a.X = o; a.x_bs = (long)Ls * H; a.ldx = H; a.W = wdev(".wo"); a.ldw = H;
        a.M = Lmax; a.N = H; a.K = H; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        a.bias = c->pf(w.p + ".bo"); a.bias_mode = 1;
        a.res = x; a.r_bs = (long)Ls * H; a.ldr = H; a.res_mode = 1; a.res_dtype = dt;
        a.out = yv; a.out_dtype = ydt; a.o_bs = (long)Ls * H; a.ldo = H;
        if (split) { if (!fused_f32) split_of((const float*)o, H, xs); as_split(a, xs, H, w.p + ".wo"); }
        c->gemm(a);
    }
    const double ln_bytes = (double)B * Lmax * H * ((h16 ? 2.0 : 4.0) + es);
    c->timed(0, ln_bytes, [&] {
        if (w.scln) launch_layernorm(yv, ydt, H, x, dt, H, B, Ls, len_dev, H, 1, 1e-8f, nullptr, nullptr, w.bg, w.bg_bs, nullptr, c->stream);
        else launch_layernorm(yv, ydt, H, x, dt, H, B, Ls, len_dev, H, 0, 1e-5f, c->pf(w.p + ".ln1_g"), c->pf(w.p + ".ln1_b"), nullptr, 0, nullptr, c->stream, split ? xs : nullptr, sp16);
    });
    c->sat_scan(x, dt, (long)Ls * H, H, B, Lmax, len_dev, H);
    {   // h = relu(conv_k9(x))                                         fs2.py:198-200
        GemmArgs a = gemm_base(dt);
        a.X = x; a.x_bs = (long)Ls * H; a.ldx = H; a.W = wdev(".w1"); a.ldw = H; a.w_ts = (long)F * H;
        a.M = Lmax; a.N = F; a.K = H; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        set_taps_1d(a, c->ffn_k0, 1);
        a.bias = c->pf(w.p + ".b1"); a.bias_mode = 1; a.act = ACT_RELU;
        a.out = hbuf; a.o_bs = (long)Ls * F; a.ldo = F;
        void* hs = split ? c->buf("fft.hs", (size_t)B * Ls * 3 * F * 2) : nullptr;
        if (split) {
            if (w.scln) split_of((const float*)x, H, xs);                           // (SCLN blocks are never f32 + split today; kept correct)
            as_split(a, xs, H, w.p + ".w1");
            a.out_dtype = DT_F32; a.out_split3 = sp16 ? 2 : 1; a.out = hs; a.o_bs = (long)Ls * 3 * F; a.ldo = 3 * F;   // h straight into the planes of the k = 1 convolution
        }
        c->gemm(a);
    }
    {   // y = conv_k1(h) + residual                                    fs2.py:201-207
        GemmArgs a = gemm_base(dt);
        a.X = hbuf; a.x_bs = (long)Ls * F; a.ldx = F; a.W = wdev(".w2"); a.ldw = F; a.w_ts = (long)H * F;
        a.M = Lmax; a.N = H; a.K = F; a.nbatch = B; a.in_len = len_dev; a.out_len = len_dev; if (flat) a.bflat = Ls;
        set_taps_1d(a, c->ffn_k1, 1);
        a.bias = c->pf(w.p + ".b2"); a.bias_mode = 1;
        a.res = x; a.r_bs = (long)Ls * H; a.ldr = H; a.res_mode = 1; a.res_dtype = dt;
        a.out = yv; a.out_dtype = ydt; a.o_bs = (long)Ls * H; a.ldo = H;
        if (split) as_split(a, c->buf("fft.hs", (size_t)B * Ls * 3 * F * 2), F, w.p + ".w2");
        c->gemm(a);
    }
    c->timed(0, ln_bytes, [&] {
        if (w.scln) launch_layernorm(yv, ydt, H, x, dt, H, B, Ls, len_dev, H, 1, 1e-8f, nullptr, nullptr, w.bg + 2 * H, w.bg_bs, w.post_add, c->stream);
        else launch_layernorm(yv, ydt, H, x, dt, H, B, Ls, len_dev, H, 0, 1e-5f, c->pf(w.p + ".ln2_g"), c->pf(w.p + ".ln2_b"), nullptr, 0, w.post_add, c->stream, split ? xs : nullptr, sp16);
    });
    c->sat_scan(x, dt, (long)Ls * H, H, B, Lmax, len_dev, H);
    if (split && !w.scln) c->fft_xs_ready = x;                                       // the next block on the same buffer finds its input planes in fft.xs
}

// ------------------------------------------------------------------------------------------------
// encoder + variance adaptor + length regulator   (fs2.py:732-775)
// ------------------------------------------------------------------------------------------------
void variance_predictor(zvx_ctx* c, const char* nm, const float* x, int B, int Tmax, const int* T_dev, float* pred, const char* bufsfx = "") {
    const int H = c->H, Fv = c->vp_dim;
    const std::string p = std::string("va.") + nm;
    float* h1 = c->fbuf(std::string("va.h1") + bufsfx, (size_t)B * Tmax * Fv);      // (own buffers when it runs beside another predictor)
    float* h2 = c->fbuf(std::string("va.h2") + bufsfx, (size_t)B * Tmax * Fv);
    {
        GemmArgs a = gemm_base(DT_F32);
        a.X = x; a.x_bs = (long)Tmax * H; a.ldx = H; a.W = c->t(p + ".c1").dev; a.ldw = H; a.w_ts = (long)Fv * H;
        a.M = Tmax; a.N = Fv; a.K = H; a.nbatch = B; a.in_len = T_dev; a.out_len = T_dev;
        set_taps_1d(a, c->vp_k, 1);
        a.bias = c->pf(p + ".b1"); a.bias_mode = 1; a.act = ACT_RELU;
        a.out = h1; a.o_bs = (long)Tmax * Fv; a.ldo = Fv;
        c->gemm(a);
    }
    launch_layernorm(h1, DT_F32, Fv, h1, DT_F32, Fv, B, Tmax, T_dev, Fv, 0, 1e-5f, c->pf(p + ".ln1_g"), c->pf(p + ".ln1_b"), nullptr, 0, nullptr, c->stream);
    {
        GemmArgs a = gemm_base(DT_F32);
        a.X = h1; a.x_bs = (long)Tmax * Fv; a.ldx = Fv; a.W = c->t(p + ".c2").dev; a.ldw = Fv; a.w_ts = (long)Fv * Fv;
        a.M = Tmax; a.N = Fv; a.K = Fv; a.nbatch = B; a.in_len = T_dev; a.out_len = T_dev;
        // fs2.py:543 hard-codes padding=1: taps are k - 1 for k in [0, vp_k)
        a.ntaps = c->vp_k;
        for (int k = 0; k < c->vp_k; k++) { a.du[k] = 0; a.dv[k] = (int)(k - 1); }
        a.bias = c->pf(p + ".b2"); a.bias_mode = 1; a.act = ACT_RELU;
        a.out = h2; a.o_bs = (long)Tmax * Fv; a.ldo = Fv;
        c->gemm(a);
    }
    launch_layernorm(h2, DT_F32, Fv, h2, DT_F32, Fv, B, Tmax, T_dev, Fv, 0, 1e-5f, c->pf(p + ".ln2_g"), c->pf(p + ".ln2_b"), nullptr, 0, nullptr, c->stream);
    launch_rowdot(h2, Fv, c->pf(p + ".lw"), c->t(p + ".lb").host[0], pred, B, Tmax, T_dev, Fv, c->stream);
}

// zvx_prosody checks (include/zvx.h), over the valid phonemes only: before anything is queued
void check_prosody(const zvx_prosody* p, const int32_t* T, int B, int Tmax) {
    const float* per_utt[4] = {p->pitch_shift, p->pitch_range, p->energy_shift, p->energy_range};
    const char* nm[4] = {"pitch_shift", "pitch_range", "energy_shift", "energy_range"};
    for (int i = 0; i < 4; i++)
        if (per_utt[i])
            for (int b = 0; b < B; b++) {
                const float v = per_utt[i][b];
                if (!std::isfinite(v)) fail(ZVX_E_INVALID, "prosody %s[%d] is not finite", nm[i], b);
                if ((i & 1) && (v < 0.f || v > 4.f)) fail(ZVX_E_INVALID, "prosody %s[%d]=%g outside [0, 4]", nm[i], b, v);
            }
    const float* tg[2] = {p->pitch_target, p->energy_target};
    for (int i = 0; i < 2; i++)
        if (tg[i])
            for (int b = 0; b < B; b++)
                for (int t = 0; t < T[b]; t++) {
                    const float v = tg[i][(size_t)b * Tmax + t];
                    if (v == v && !(v >= 0.f && v <= 1.f)) fail(ZVX_E_INVALID, "prosody %s_target[%d][%d]=%g is neither NaN nor in [0, 1]", i ? "energy" : "pitch", b, t, v);
                }
    if (p->dur_scale_q16)
        for (int b = 0; b < B; b++)
            for (int t = 0; t < T[b]; t++) {
                const int q = p->dur_scale_q16[(size_t)b * Tmax + t];
                if (q < 4096 || q > 1048576) fail(ZVX_E_INVALID, "prosody dur_scale_q16[%d][%d]=%d outside [4096, 1048576]", b, t, q);
            }
}

void run_encode(zvx_ctx* c, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration, const int32_t* T,
                int B, int Tmax, const float* spk, int32_t* mel_len_out, int Lmax_cap, const zvx_prosody* pros = nullptr, bool spk_dev = false) {
    const int H = c->H;
    c->have_features = false; c->have_mel = false;
    if (c->stream != c->front_stream) c->front_dirty_main = true;
    if (B <= 0 || Tmax <= 0) fail(ZVX_E_INVALID, "B and Tmax must be positive");
    if (c->vp_k != 3) fail(ZVX_E_UNSUPPORTED, "vp_kernel_size != 3 changes the sequence length (fs2.py:543 padding=1)");
    c->T_host.assign(T, T + B);
    for (int b = 0; b < B; b++) {
        if (T[b] <= 0 || T[b] > Tmax) fail(ZVX_E_INVALID, "T[%d]=%d out of range (1..%d)", b, T[b], Tmax);
        for (int t = 0; t < T[b]; t++) {
            const int ph = phoneme[b * Tmax + t], pu = puncts[b * Tmax + t];
            if (ph < 0 || ph >= c->n_phone_rows) fail(ZVX_E_INVALID, "phoneme id %d out of range at [%d][%d]", ph, b, t);   // nn.Embedding IndexError
            if (pu < 0 || pu >= c->n_punct_rows) fail(ZVX_E_INVALID, "punct id %d out of range at [%d][%d]", pu, b, t);
        }
    }
    if (pros) check_prosody(pros, T, B, Tmax);
    c->B = B; c->Tmax = Tmax; c->have_features = false; c->have_mel = false;
    const size_t nid = (size_t)B * Tmax;
    // the call's small inputs (ids, lengths, forced durations, speaker embeddings, the prosody controls present) travel as ONE upload
    std::vector<std::string> planes = {"in.phoneme", "in.puncts", "in.duration", "in.T", "in.spk"};
    // prosody: one plane for the four per-utterance vectors ([4][B] floats), one per per-phoneme array given
    const void* pros_src[3] = {pros ? pros->pitch_target : nullptr, pros ? pros->energy_target : nullptr, pros ? pros->dur_scale_q16 : nullptr};
    int pros_plane[3] = {-1, -1, -1};
    if (pros) {
        planes.push_back("in.pros_utt");
        const char* nm[3] = {"in.pitch_target", "in.energy_target", "in.dur_scale"};
        for (int i = 0; i < 3; i++) if (pros_src[i]) { pros_plane[i] = (int)planes.size(); planes.push_back(nm[i]); }
    }
    const size_t np = planes.size();
    size_t in_stride = 0;
    char* in_base = c->carve("in.all", planes, std::max(std::max(nid, (size_t)B * 4), (size_t)B * H) * 4, &in_stride);
    c->in_stage.resize(in_stride * np / sizeof(int));
    {
        int* hs = c->in_stage.data();
        const size_t st = in_stride / sizeof(int);
        memcpy(hs, phoneme, nid * 4); memcpy(hs + st, puncts, nid * 4);
        if (duration) memcpy(hs + 2 * st, duration, nid * 4);
        memcpy(hs + 3 * st, T, (size_t)B * 4);
        if (!spk_dev) memcpy(hs + 4 * st, spk, (size_t)B * H * 4);
        if (pros) {
            const float* per_utt[4] = {pros->pitch_shift, pros->pitch_range, pros->energy_shift, pros->energy_range};
            for (int i = 0; i < 4; i++) if (per_utt[i]) memcpy(hs + 5 * st + (size_t)i * B, per_utt[i], (size_t)B * 4);
            for (int i = 0; i < 3; i++) if (pros_src[i]) memcpy(hs + pros_plane[i] * st, pros_src[i], nid * 4);
        }
        c->upload(in_base, hs, in_stride * np);
    }
    int* ph_d = (int*)in_base; int* pu_d = (int*)(in_base + in_stride);
    int* dur_in = duration ? (int*)(in_base + 2 * in_stride) : nullptr;
    int* T_d = (int*)(in_base + 3 * in_stride);
    float* spk_d = (float*)(in_base + 4 * in_stride);
    // ZVX_DEVICE_SPK: the embeddings are on the device already -- into their plane behind the upload, in stream order
    if (spk_dev) HIPCHK(hipMemcpyAsync(spk_d, spk, (size_t)B * H * 4, hipMemcpyDeviceToDevice, c->stream));
    // device views of the controls (NULL: neutral)
    const float* pros_utt = pros ? (const float*)(in_base + 5 * in_stride) : nullptr;
    const float* p_shift = (pros && pros->pitch_shift) ? pros_utt : nullptr;
    const float* p_range = (pros && pros->pitch_range) ? pros_utt + B : nullptr;
    const float* e_shift = (pros && pros->energy_shift) ? pros_utt + 2 * B : nullptr;
    const float* e_range = (pros && pros->energy_range) ? pros_utt + 3 * B : nullptr;
    const float* p_tgt = pros_src[0] ? (const float*)(in_base + pros_plane[0] * in_stride) : nullptr;
    const float* e_tgt = pros_src[1] ? (const float*)(in_base + pros_plane[1] * in_stride) : nullptr;
    const int* dq = pros_src[2] ? (const int*)(in_base + pros_plane[2] * in_stride) : nullptr;
    const bool pitch_ctl = p_shift || p_range || p_tgt, energy_ctl = e_shift || e_range || e_tgt;

    c->stage_begin(ZVX_T_ENCODER);
    c->tag = "encoder";
    // positional table: stored rows cover max_txt_len; longer inputs recompute it (fs2.py:383-388)
    const float* pe = c->pf("enc.pe");
    if (Tmax > c->t("enc.pe").dim(0)) {
        std::vector<float> tab((size_t)Tmax * H);
        for (int pos = 0; pos < Tmax; pos++)
            for (int j = 0; j < H; j++) {
                const double ang = pos / pow(10000.0, 2.0 * (j / 2) / H);
                tab[(size_t)pos * H + j] = (float)((j & 1) ? cos(ang) : sin(ang));
            }
        float* d = c->fbuf("enc.pe_ext", tab.size());
        HIPCHK(hipMemcpyAsync(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        pe = d;
    }
    float* x = c->fbuf("enc.x", nid * H);
    launch_embed(ph_d, pu_d, c->pf("enc.emb"), c->emb_dim, c->pf("enc.pemb"), c->punct_dim, pe, x, B, Tmax, T_d, c->stream);
    c->fft_xs_ready = nullptr;
    for (int i = 0; i < c->enc_layers; i++) {
        FftWeights w{"enc." + std::to_string(i), false, nullptr, 0, (i == c->enc_layers - 1) ? spk_d : nullptr};   // + style (fs2.py:740-741)
        fft_block(c, x, DT_F32, B, Tmax, T_d, c->enc_heads, w);
    }
    c->fft_xs_ready = nullptr;                                                                       // valid only between consecutive blocks of one stack
    c->stage_end(ZVX_T_ENCODER);

    c->stage_begin(ZVX_T_VARIANCE);
    c->tag = "variance";
    HIPCHK(hipMemcpyAsync(c->fbuf("enc.out", nid * H), x, nid * H * 4, hipMemcpyDeviceToDevice, c->stream));
    // the per-phoneme outputs that padding positions must read as zero: one zero-fill for all six
    size_t va_stride = 0;
    char* va_base = c->carve("va.zeroed", {"va.logd", "va.pitch", "va.energy", "va.pitch_idx", "va.energy_idx", "va.dur"}, nid * 4, &va_stride);
    HIPCHK(hipMemsetAsync(va_base, 0, va_stride * 6, c->stream));
    float* logd = (float*)va_base; float* pitch = (float*)(va_base + va_stride); float* energy = (float*)(va_base + 2 * va_stride);
    int* pidx = (int*)(va_base + 3 * va_stride); int* eidx = (int*)(va_base + 4 * va_stride);
    // The duration and the pitch predictor read the same x and are independent (fs2.py:663-668): the duration predictor runs on a
    // second stream beside the pitch predictor.  Their exact-f32 convolutions are chains of dependent matrix instructions on a
    // fraction of the CUs at any batch size (64 workgroups at B = 32 x 128), so this pays everywhere: the stage 0.43 -> 0.32-0.36 ms
    // for B = 1 ... 32 (tools/ab_va_overlap.py).  Same kernels, same arithmetic; x is only modified (pitch embedding) after both
    // have read it.
    if (B <= c->va_overlap_maxb) {
        if (!c->aux_stream) {
            HIPCHK(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->ev_aux[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_aux[1], hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(c->ev_aux[0], c->stream));
        HIPCHK(hipStreamWaitEvent(c->aux_stream, c->ev_aux[0], 0));
        {
            struct Swap { zvx_ctx* c; hipStream_t keep; ~Swap() { c->stream = keep; } } sw{c, c->stream};   // restored on every path out
            c->stream = c->aux_stream;
            variance_predictor(c, "dur", x, B, Tmax, T_d, logd, ".dur");
            HIPCHK(hipEventRecord(c->ev_aux[1], c->aux_stream));
        }
        variance_predictor(c, "pitch", x, B, Tmax, T_d, pitch);
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_aux[1], 0));
    } else {
        variance_predictor(c, "dur", x, B, Tmax, T_d, logd);                                           // fs2.py:663
        variance_predictor(c, "pitch", x, B, Tmax, T_d, pitch);                                        // fs2.py:665-668
    }
    // the energy predictor reads x with the CONTROLLED pitch embedding (fs2.py:665-671)
    if (pitch_ctl) c->timed(0, (double)nid * H * 12.0, [&] { launch_bucket_embed_add_ctl(pitch, p_shift, p_range, p_tgt, c->pf("va.pitch_emb"), c->n_bins, x, H, H, pidx, B, Tmax, T_d, c->stream); }, "bucket_embed_add_ctl");
    else launch_bucket_embed_add(pitch, c->pf("va.pitch_emb"), c->n_bins, x, H, H, pidx, B, Tmax, T_d, c->stream);
    variance_predictor(c, "energy", x, B, Tmax, T_d, energy);                                          // fs2.py:669-672
    if (energy_ctl) c->timed(0, (double)nid * H * 12.0, [&] { launch_bucket_embed_add_ctl(energy, e_shift, e_range, e_tgt, c->pf("va.energy_emb"), c->n_bins, x, H, H, eidx, B, Tmax, T_d, c->stream); }, "bucket_embed_add_ctl");
    else launch_bucket_embed_add(energy, c->pf("va.energy_emb"), c->n_bins, x, H, H, eidx, B, Tmax, T_d, c->stream);
    c->stage_end(ZVX_T_VARIANCE);

    c->stage_begin(ZVX_T_LENREG);
    c->tag = "lenreg";
    int* dur = (int*)(va_base + 5 * va_stride); int* cum = c->ibuf("va.cum", nid); int* ml = c->ibuf("va.mel_len", B);
    if (dq) c->timed(0, (double)nid * 16.0, [&] { launch_durations_q16(dur_in, logd, dq, dur, cum, ml, B, Tmax, T_d, c->stream); }, "durations_q16");
    else launch_durations(dur_in, logd, dur, cum, ml, B, Tmax, T_d, c->stream);
    c->mel_len_host.resize(B);
    if (duration) {
        // forced durations: the mel lengths are their sums (same clamps as k_durations; with dur_scale_q16 the same Q16 rule as
        // k_durations_q16) -- nothing to wait for
        const int32_t* q = pros ? pros->dur_scale_q16 : nullptr;
        for (int b = 0; b < B; b++) {
            long long sum = 0;
            for (int t = 0; t < T[b]; t++) {
                const long long d = std::min(std::max(duration[(size_t)b * Tmax + t], 0), 65536);
                sum += q ? d * q[(size_t)b * Tmax + t] : d;
            }
            if (q) sum = (sum + 32768) >> 16;
            c->mel_len_host[b] = (int)std::min(sum, 0x7fffffffLL);
        }
    } else {
        HIPCHK(hipMemcpyAsync(c->mel_len_host.data(), ml, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));        // predicted durations: the one data-dependent host sync (model.py:325)
    }
    if (mel_len_out) memcpy(mel_len_out, c->mel_len_host.data(), B * sizeof(int));
    int Lmax = 0; for (int b = 0; b < B; b++) Lmax = std::max(Lmax, c->mel_len_host[b]);
    // checked BEFORE anything is sized by it: a garbage log-duration must not drive an allocation
    const int cap = Lmax_cap > 0 ? std::min(Lmax_cap, c->max_frames) : c->max_frames;
    if (Lmax > cap) fail(ZVX_E_BUFFER, "predicted mel length %d exceeds %s %d", Lmax, Lmax_cap > 0 && Lmax_cap <= c->max_frames ? "Lmax_cap" : "the context's max_frames", cap);
    c->Lmax = Lmax;
    if (Lmax > 0) {
        float* feats = c->fbuf("features", (size_t)B * Lmax * H);
        double rows_out = 0; for (int b = 0; b < B; b++) rows_out += c->mel_len_host[b];
        c->timed(0, (rows_out + (double)B * Tmax) * H * 4.0, [&] { launch_length_regulate(x, H, cum, T_d, ml, feats, B, Tmax, Lmax, H, c->stream); });   // fs2.py:447-455: pure copy
    }
    c->stage_end(ZVX_T_LENREG);
    c->have_features = true;
}

// ------------------------------------------------------------------------------------------------
// mel decoders
// ------------------------------------------------------------------------------------------------
void decoder_fs2(zvx_ctx* c, const float* feats, const float* spk_d, const int* L_d, int B, int Lmax, float* mel) {
    const int H = c->H;
    // 16-bit mode: IEEE half like the StyleTTS decoder (needs the fused attention: head depth 264), zvx_set_int("dec_f16", 0): bf16
    const int dt = (c->dt == DT_BF16 && c->dec_f16 && c->use_flash && H / c->dec_heads == 264 && c->has("dec.mel_w.h16")) ? DT_F16 : c->dt;
    const float* pe = c->pf("dec.pe");
    if (Lmax > c->t("dec.pe").dim(0)) {                   // fs2.py:287-294: table recomputed for longer inputs
        std::vector<float> tab((size_t)Lmax * H);
        for (int pos = 0; pos < Lmax; pos++)
            for (int j = 0; j < H; j++) {
                const double ang = pos / pow(10000.0, 2.0 * (j / 2) / H);
                tab[(size_t)pos * H + j] = (float)((j & 1) ? cos(ang) : sin(ang));
            }
        float* d = c->fbuf("dec.pe_ext", tab.size());
        HIPCHK(hipMemcpyAsync(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        pe = d;
    }
    // 16-bit mode: every utterance gets ffn_k / 2 padding rows so that the FFT blocks' static-weight GEMMs run batch-flattened (fft_block)
    const bool flat = dt != DT_F32 && c->dec_flat && B > 1;
    const int Ls = flat ? Lmax + std::max(c->ffn_k0, c->ffn_k1) / 2 : Lmax;
    void* x = c->buf("dec.x", (size_t)B * Ls * H * dtype_size(dt));
    launch_add_pe_cast(feats, pe, x, dt, H, B, Lmax, L_d, H, c->stream, Ls);
    c->sat_scan(x, dt, (long)Ls * H, H, B, Lmax, L_d, H);
    float* bg = nullptr; long bg_bs = 0;
    if (c->dec_scln) {      // all 2*layers SCLN affine vectors of the call in one GEMM: [b | g] = W s   (fs2.py:85)
        const int NA = 2 * c->dec_layers * 2 * H;
        bg = c->fbuf("dec.bg", (size_t)B * NA); bg_bs = NA;
        GemmArgs a = gemm_base(DT_F32);
        a.X = spk_d; a.ldx = H; a.W = c->t("dec.scln_all").dev; a.ldw = H; a.M = B; a.N = NA; a.K = H; a.in_len_static = B;
        a.out = bg; a.ldo = NA;
        c->gemm(a);
    }
    for (int i = 0; i < c->dec_layers; i++) {
        FftWeights w{"dec." + std::to_string(i), c->dec_scln != 0, bg ? bg + (long)i * 4 * H : nullptr, bg_bs, nullptr};
        fft_block(c, x, dt, B, Lmax, L_d, c->dec_heads, w, Ls, flat);
    }
    GemmArgs a = gemm_base(dt);                             // mel_linear   fs2.py:313
    a.X = x; a.x_bs = (long)Ls * H; a.ldx = H; a.W = c->t(dt == DT_F16 ? "dec.mel_w.h16" : "dec.mel_w").dev; a.ldw = H;
    a.M = Lmax; a.N = c->n_mels; a.K = H; a.nbatch = B; a.in_len = L_d; a.out_len = L_d;
    a.bias = c->pf("dec.mel_b"); a.bias_mode = 1;
    a.out = mel; a.out_dtype = DT_F32; a.o_bs = (long)Lmax * c->n_mels; a.ldo = c->n_mels;
    c->gemm(a);
}

// Lmax: rows per utterance of every buffer of the decoder = longest utterance + one padding row (never a valid position), so that
// its k = 3 / 1x1 convolutions may run BATCH-FLATTENED (GemmArgs::bflat): row tiles cross utterance boundaries, no utterance ends in
// a half-empty tile.  Lrows: the longest utterance.  dt: the decoder's activation dtype (bf16 / f16 / f32)
struct StyCtx { zvx_ctx* c; int B, Lmax; const int* L_d; float* mean; float* rstd; int dt; int Lrows; int flat; const void* mel; };

// x2 / ldx2 / Cin2: the block's 1x1 shortcut as a second source of this convolution (the caller has checked can_fuse_shortcut)
void sty_conv(const StyCtx& s, const std::string& wname, const void* x, int ldx, int Cin, void* out, int ldo, int out_dt,
              int Cout, const void* res, int ldr, float out_scale, const void* x2 = nullptr, int ldx2 = 0, int Cin2 = 0) {
    zvx_ctx* c = s.c;
    const Tensor& w = c->t(s.dt == DT_F16 ? wname + ".h16" : wname);
    GemmArgs a = gemm_base(s.dt);
    if (x2) { a.X2 = x2; a.x2_bs = (long)s.Lmax * ldx2; a.ldx2 = ldx2; a.K2 = Cin2; a.Wp = c->pair_packed.at(w.dev); }
    a.X = x; a.x_bs = (long)s.Lmax * ldx; a.ldx = ldx; a.W = w.dev; a.ldw = Cin; a.w_ts = (long)Cout * Cin;
    a.M = s.Lrows; a.N = Cout; a.K = Cin; a.nbatch = s.B; a.in_len = s.L_d; a.out_len = s.L_d;
    const bool to_mel = out == s.mel;                              // the mel projection writes the caller-visible [B][Lrows][n_mels] layout: per utterance
    a.bflat = (s.flat && !to_mel) ? s.Lmax : 0;
    set_taps_1d(a, w.dim(0), 1);
    if (c->has(wname + "_b")) { a.bias = c->pf(wname + "_b"); a.bias_mode = 1; }
    if (res) { a.res = res; a.r_bs = (long)s.Lmax * ldr; a.ldr = ldr; a.res_mode = 1; a.res_dtype = s.dt; }
    a.out_scale = out_scale;
    a.out = out; a.o_bs = (long)(to_mel ? s.Lrows : s.Lmax) * ldo; a.ldo = ldo; a.out_dtype = out_dt;
    c->gemm(a);
}
// y = lrelu_0.2(affine(IN(x)))  (InstanceNorm over each utterance's true length only)
void sty_norm(const StyCtx& s, const void* x, int ldx, int C, void* y, int ldy, const float* gamma, const float* beta,
              long g_bs, int one_plus, int act) {
    const std::string keep = s.c->tag;
    s.c->tag = "decoder.norm";
    s.c->timed(0, (double)s.B * s.Lmax * C * s.c->es() * 3.0, [&] {          // statistics pass (read) + normalise pass (read + write)
        // One launch (statistics, then the same workgroup walks its rows again: bit-identical) where it measures faster
        // (tools/ab_norm_fuse.py): short utterances at any batch size, and any length once B x C / 64 workgroups fill a fair part
        // of the chip.  A few workgroups walking many rows twice (B <= 4 at 896 frames) lose to the wide second launch.
        const bool fuse_pays = s.Lmax <= 512 || (long)s.B * ((C + 63) / 64) >= 64;
        if (s.dt != DT_F32 && s.B <= s.c->norm_fuse_maxb && fuse_pays) {
            launch_instnorm_fused(x, s.dt, ldx, y, s.dt, ldy, s.B, s.Lmax, s.L_d, C, 1e-5f, s.mean, s.rstd, gamma, beta, g_bs, one_plus, act, 0.2f, s.c->stream);
            return;
        }
        launch_instnorm_stats(x, s.dt, ldx, s.B, s.Lmax, s.L_d, C, 1e-5f, s.mean, s.rstd, s.c->stream);
        launch_norm_affine_act(x, s.dt, ldx, y, s.dt, ldy, s.B, s.Lmax, s.L_d, C, s.mean, s.rstd, gamma, beta, g_bs, one_plus,
                               act, 0.2f, s.c->stream);
    });
    s.c->sat_scan(y, s.dt, (long)s.Lmax * ldy, ldy, s.B, s.Lmax, s.L_d, C);
    s.c->tag = keep;
}

void decoder_styletts(zvx_ctx* c, const float* feats, const float* spk_d, const int* L_d, int B, int Lrows, float* mel) {
    const int H = c->H, H2 = 2 * H, R = c->res_dim, CW = H2 + R;
    const int dt = (c->dt == DT_BF16 && c->dec_f16 && c->has("sty.out.h16")) ? DT_F16 : c->dt;      // 16-bit mode: IEEE half unless switched off
    const int Lmax = Lrows + 1;                           // row stride of every buffer below (see StyCtx)
    const size_t es = dtype_size(dt), rows = (size_t)B * Lmax;
    const float inv_sqrt2 = (float)(1.0 / sqrt(2.0));
    StyCtx s{c, B, Lmax, L_d, c->fbuf("sty.mean", (size_t)B * CW), c->fbuf("sty.rstd", (size_t)B * CW), dt, Lrows, c->dec_flat, mel};
    void* e = c->buf("sty.e", rows * H * es);
    void* t0 = c->buf("sty.t0", rows * CW * es);
    void* t1 = c->buf("sty.t1", rows * H2 * es);
    void* r = c->buf("sty.r", rows * H2 * es);
    void* catA = c->buf("sty.catA", rows * CW * es);
    void* catB = c->buf("sty.catB", rows * CW * es);
    launch_add_pe_cast(feats, nullptr, e, dt, H, B, Lrows, L_d, H, c->stream, Lmax);
    c->sat_scan(e, dt, (long)Lmax * H, H, B, Lmax, L_d, H);

    // AdaIN affine vectors for all 10 norms: h = fc(s)          styletts.py:89-91
    const Tensor& aw = c->t("sty.adain_w");
    const int NA = aw.dim(1);
    float* hall = c->fbuf("sty.adain_h", (size_t)B * NA);
    {
        GemmArgs a = gemm_base(DT_F32);
        a.X = spk_d; a.ldx = H; a.W = aw.dev; a.ldw = H; a.M = B; a.N = NA; a.K = H; a.in_len_static = B;
        a.bias = c->pf("sty.adain_b"); a.bias_mode = 1; a.out = hall; a.ldo = NA;
        c->gemm(a);
    }
    // encode.0: ResBlk1d(H -> 2H, normalize)                       styletts.py:44-69
    sty_norm(s, e, H, H, t0, H, c->pf("sty.enc0.norm1_g"), c->pf("sty.enc0.norm1_b"), 0, 0, ACT_LRELU);
    sty_conv(s, "sty.enc0.c1", t0, H, H, t1, H, dt, H, nullptr, 0, 1.f);
    sty_norm(s, t1, H, H, t0, H, c->pf("sty.enc0.norm2_g"), c->pf("sty.enc0.norm2_b"), 0, 0, ACT_LRELU);
    auto can_fuse_shortcut = [&](const std::string& blk) {
        return c->dec_sc_fuse && dt != DT_F32 && c->has(blk + ".c2") && c->pair_packed.count(c->t(dt == DT_F16 ? blk + ".c2.h16" : blk + ".c2").dev) != 0;
    };
    if (can_fuse_shortcut("sty.enc0")) {
        sty_conv(s, "sty.enc0.c2", t0, H, H, catA, CW, dt, H2, nullptr, 0, inv_sqrt2, e, H, H);       // (conv2(t) + conv1x1(e)) / sqrt(2) in one launch
    } else {
        sty_conv(s, "sty.enc0.c2", t0, H, H, r, H2, dt, H2, nullptr, 0, 1.f);
        sty_conv(s, "sty.enc0.sc", e, H, H, catA, CW, dt, H2, r, H2, inv_sqrt2);
    }
    // encode.1: ResBlk1d(2H -> 2H), identity shortcut (in place on catA[:, 0:2H])
    sty_norm(s, catA, CW, H2, t0, H2, c->pf("sty.enc1.norm1_g"), c->pf("sty.enc1.norm1_b"), 0, 0, ACT_LRELU);
    sty_conv(s, "sty.enc1.c1", t0, H2, H2, t1, H2, dt, H2, nullptr, 0, 1.f);
    sty_norm(s, t1, H2, H2, t0, H2, c->pf("sty.enc1.norm2_g"), c->pf("sty.enc1.norm2_b"), 0, 0, ACT_LRELU);
    sty_conv(s, "sty.enc1.c2", t0, H2, H2, catA, CW, dt, H2, catA, CW, inv_sqrt2);
    // asr_res = IN_affine(conv1x1(e)) -> columns [2H, 2H+R) of both concat buffers (concat-free torch.cat, styletts.py:195)
    sty_conv(s, "sty.asr", e, H, H, t1, R, dt, R, nullptr, 0, 1.f);
    launch_instnorm_stats(t1, dt, R, B, Lmax, L_d, R, 1e-5f, s.mean, s.rstd, c->stream);
    for (void* cat : {catA, catB})
        launch_norm_affine_act(t1, dt, R, (char*)cat + (size_t)H2 * es, dt, CW, B, Lmax, L_d, R, s.mean, s.rstd, c->pf("sty.asr_g"),
                               c->pf("sty.asr_beta"), 0, 0, ACT_NONE, 0.f, c->stream);
    c->sat_scan((char*)catA + (size_t)H2 * es, dt, (long)Lmax * CW, CW, B, Lmax, L_d, R);
    // decode.0..4: AdainResBlk1d                                    styletts.py:119-139
    struct Blk { int cin, cout; bool cat_out; };
    const Blk blks[5] = {{CW, H2, true}, {CW, H2, true}, {CW, H, false}, {H, H, false}, {H, H, false}};
    void* cur = catA; int cur_ld = CW;
    void* nxtcat = catB;
    void* xa = c->buf("sty.xa", rows * H * es);
    void* xb = c->buf("sty.xb", rows * H * es);
    long hoff = 0;
    for (int i = 0; i < 5; i++) {
        const Blk& bk = blks[i];
        const std::string p = "sty.dec" + std::to_string(i);
        const float* g1 = hall + hoff;            const float* b1 = g1 + bk.cin;  hoff += 2 * bk.cin;
        const float* g2 = hall + hoff;            const float* b2 = g2 + bk.cout; hoff += 2 * bk.cout;
        sty_norm(s, cur, cur_ld, bk.cin, t0, bk.cin, g1, b1, NA, 1, ACT_LRELU);
        sty_conv(s, p + ".c1", t0, bk.cin, bk.cin, t1, bk.cout, dt, bk.cout, nullptr, 0, 1.f);
        sty_norm(s, t1, bk.cout, bk.cout, t0, bk.cout, g2, b2, NA, 1, ACT_LRELU);
        void* out; int out_ld;
        if (bk.cat_out) { out = nxtcat; out_ld = CW; } else { out = (cur == xa) ? xb : xa; out_ld = H; }
        if (c->has(p + ".sc") && can_fuse_shortcut(p)) {
            sty_conv(s, p + ".c2", t0, bk.cout, bk.cout, out, out_ld, dt, bk.cout, nullptr, 0, inv_sqrt2, cur, cur_ld, bk.cin);
        } else if (c->has(p + ".sc")) {
            sty_conv(s, p + ".c2", t0, bk.cout, bk.cout, r, bk.cout, dt, bk.cout, nullptr, 0, 1.f);
            sty_conv(s, p + ".sc", cur, cur_ld, bk.cin, out, out_ld, dt, bk.cout, r, bk.cout, inv_sqrt2);
        } else {
            sty_conv(s, p + ".c2", t0, bk.cout, bk.cout, out, out_ld, dt, bk.cout, cur, cur_ld, inv_sqrt2);
        }
        if (bk.cat_out) { nxtcat = cur; }
        cur = out; cur_ld = out_ld;
    }
    sty_conv(s, "sty.out", cur, cur_ld, H, mel, c->n_mels, DT_F32, c->n_mels, nullptr, 0, 1.f);
}

void run_decode(zvx_ctx* c, const float* feats, const float* spk_d, const int* L_d, int B, int Lmax) {
    if (c->stream != c->front_stream) c->front_dirty_main = true;
    c->stage_begin(ZVX_T_DECODER);
    c->tag = "decoder";
    float* mel = c->fbuf("mel", (size_t)B * std::max(Lmax, 1) * c->n_mels);
    if (c->poison_pads) {
        // every work buffer of the decoders starts as NaN patterns (0xFF bytes: NaN as f32, half and bf16): batch-flattened launches write
        // junk into padding rows and read rows past an utterance's length by design -- every consumer must MASK them (select), never
        // multiply them by zero.  With this switch a violation shows up as NaN in the mel (the test compares with the clean run bit for bit).
        for (auto& kv : c->bufs) {
            const std::string& nm = kv.first;
            const bool mine = nm.rfind("sty.", 0) == 0 || nm.rfind("fft.", 0) == 0 || nm == "dec.x";
            if (mine && kv.second.p && kv.second.base == kv.second.p && nm != "sty.adain_h" && nm != "dec.bg") HIPCHK(hipMemsetAsync(kv.second.p, 0xFF, kv.second.cap, c->stream));
        }
    }
    if (Lmax > 0) {
        if (c->dec_kind == 0) decoder_fs2(c, feats, spk_d, L_d, B, Lmax, mel);
        else decoder_styletts(c, feats, spk_d, L_d, B, Lmax, mel);
        launch_zero_tail_rows(mel, c->n_mels, B, Lmax, L_d, c->n_mels, c->stream);     // rows >= mel_len[b]: zeros, whatever ran before
    }
    c->stage_end(ZVX_T_DECODER);
    c->have_mel = true;
}

// ------------------------------------------------------------------------------------------------
// HiFi-GAN generator (hifigan.py:114-130).  Activations are stored in the *activated* domain:
// every tensor a later conv consumes through leaky_relu(., 0.1) is written as leaky_relu(x); the raw
// residual is recovered exactly-enough by the inverse map in the consumer's epilogue (res_mode 2).
// ------------------------------------------------------------------------------------------------
// The dtype of every arithmetic domain of the generator (0 .. number of stages).
// 16-bit mode: IEEE half -- f16 copies of the weights, f16 activations / running sum, the f16 MFMA at the bf16 rate and 8x
// less rounding error per tensor; every store saturates (MODE.FP16_OVFL inside the kernels).  zvx_set_int("voc_f16", 0): bf16 (A/B)
// The 16-bit arithmetic is chosen PER STAGE (zvx_set_int("voc_f16_stages", mask)): domain 0 = the padded mel, conv_pre and its
// output; domain i = everything of upsampling stage i (the ConvTranspose's OUTPUT, the ResBlocks' tensors, weights and running sum, the
// stage's result).  A ConvTranspose reads domain i - 1 with that domain's weights and writes domain i (the run-time epilogue converts:
// one rounding either way).  Bit k of the mask: domain k in IEEE half, else bf16.
// Default (mask -1): half everywhere except a ResBlock1 stage of 128 channels -- the pair kernel's stage (HiFi-GAN V1's second): 43 % of
// that generator's matrix work, where the f16 multiplier array's extra power is 0.3 of the 0.8-1.0 ms the all-half generator costs at
// the board's power limit, for 1/5 of the error budget (tools/ab_voc_stages.py, tools/vocoder_error_budget.py)
std::vector<int> voc_domains(zvx_ctx* c) {
    if (c->voc_h16_ok < 0) {
        // decided once: the half copies exist only for 3-D weights with K % 8 == 0 (upload_weights); a generator with a narrower tensor
        // (e.g. a 4-channel last stage) runs entirely on the bf16 kernels, which need no packed copies
        c->voc_h16_ok = 1;
        for (auto& kv : c->tensors)
            if (kv.first.rfind("voc.", 0) == 0 && kv.second.kind == 'w' && kv.second.dims.size() == 3 && !c->has(kv.first + ".h16")) c->voc_h16_ok = 0;
    }
    const bool half_ok = c->dt == DT_BF16 && c->voc_f16 && c->voc_h16_ok == 1 && c->has("voc.pre_w.h16");
    int mask = c->voc_f16_stages;
    if (mask < 0) {
        mask = 0x7fffffff;
        int cw = c->voc_c0;
        for (int i = 0; i < (int)c->voc_rates.size(); i++) { cw /= 2; if (cw == 128 && c->voc_resblock == 1) mask &= ~(1 << (i + 1)); }
    }
    std::vector<int> dom(c->voc_rates.size() + 1);
    for (size_t k = 0; k < dom.size(); k++) dom[k] = (half_ok && ((mask >> k) & 1)) ? (int)DT_F16 : c->dt;
    return dom;
}
const Tensor& voc_weight(zvx_ctx* c, const std::string& n, int d) { return c->t(d == DT_F16 ? n + ".h16" : n); }      // a contraction weight in a domain's dtype

// what the steps of one run_vocoder call share: the batch, the ResBlocks per stage, the per-stage row counts and the work buffers
struct VocCall {
    int B, Pmax, nk;
    const int* lens_d;                     // [mel_len | P | P x rate_0 | P x rate_0 x rate_1 ...][B]: the input rows of stage i start at (i + 1) B
    void *A, *X0, *T1, *PP[2], *XS;        // stage input / upsampled stage tensor (both activated), pair temporaries, running sum over the ResBlocks of a stage
    bool side_ok;                          // single requests: the 2nd / 3rd ResBlock of a stage run beside the 1st (SideHop), on temporaries of their own
    void* sideT1[2]; void* sidePP[2][2];
};
// upsampling stage i: Cin channels x rows_in rows (valid: len_in[b]) of domain dt_in -> Cout x rows (len[b]) of domain dt
struct VocStage {
    int i, Cin, Cout, rows_in, rows;
    const int* len_in; const int* len;
    int dt_in, dt;
    float next_slope;                      // the leaky-ReLU the stage's result is stored under (its consumer's)
};

// The convolutions of ResBlock j of a stage, in the stage's dtype: per dilation t the (c1, c2) pair of a ResBlock1 (hifigan.py:49-56) or
// the one convolution of a ResBlock2 (c1; c2 stays empty -- hifigan.py:77-82).  The ONE place that spells the tensors' names.
struct RbConv { std::string name; const Tensor* w = nullptr; const void* packed = nullptr; const float* bias = nullptr; };   // packed: the fragment-order copy, if any
struct RbWeights { std::string name; std::vector<RbConv> c1, c2; };
RbWeights voc_rb_weights(zvx_ctx* c, const VocCall& v, const VocStage& s, int j) {
    RbWeights w;
    w.name = "voc.rb" + std::to_string(s.i * v.nk + j);
    auto conv = [&](const char* which, int t) {
        RbConv r;
        r.name = w.name + which + std::to_string(t);
        r.w = &voc_weight(c, r.name + "_w", s.dt);
        auto it = c->packed.find(r.w->dev);
        if (it != c->packed.end()) r.packed = it->second;
        r.bias = c->pf(r.name + "_b");
        return r;
    };
    for (int t = 0; t < (int)c->voc_rb_d[j].size(); t++) {
        if (c->voc_resblock == 1) { w.c1.push_back(conv(".c1_", t)); w.c2.push_back(conv(".c2_", t)); }
        else w.c1.push_back(conv(".c_", t));
    }
    return w;
}

// How the LAST launch of ResBlock j closes a stage of nk blocks: xs (+)= resblock output -- the first block writes the running sum, the
// middle ones add to it, the last adds, scales by 1 / nk, applies the next stage's leaky-ReLU and writes the stage output (x = xs /
// num_kernels, stored activated for the next stage); a single block needs no running sum.
struct StageClose { int accum_mode; bool writes_out; };   // accum_mode: bit 0 v += xs, bit 1 xs = v
StageClose stage_close(int j, int nk) {
    if (nk == 1) return {0, true};
    return {j == 0 ? 2 : (j < nk - 1 ? 3 : 1), j == nk - 1};
}
template <typename Args>                                  // GemmArgs or StreamArgs (which has no act / accum_dtype: its output is always activated with `slope`)
void close_stage(Args& a, const StageClose& cl, const VocCall& v, const VocStage& s) {
    a.accum = cl.accum_mode ? v.XS : nullptr; a.accum_mode = cl.accum_mode; a.a_bs = (long)s.rows * s.Cout; a.lda = s.Cout;
    if (cl.writes_out) { a.out = v.A; a.out_scale = 1.0f / v.nk; a.slope = s.next_slope; }
    else a.out = nullptr;
    if constexpr (std::is_same<Args, GemmArgs>::value) { a.accum_dtype = s.dt; if (cl.writes_out) a.act = ACT_LRELU; }
}

// conv_pre, stored as leaky_relu(x, 0.1) (its only consumer, hifigan.py:115-117)
void voc_conv_pre(zvx_ctx* c, const VocCall& v, const void* vin, int dt) {
    const int nm = c->n_mels, Pmax = v.Pmax;
    const int* P_d = v.lens_d + v.B;
    GemmArgs a = gemm_base(dt);
    a.X = vin; a.x_bs = (long)Pmax * nm; a.ldx = nm; a.W = voc_weight(c, "voc.pre_w", dt).dev; a.ldw = nm; a.w_ts = (long)c->voc_c0 * nm;
    a.M = Pmax; a.N = c->voc_c0; a.K = nm; a.nbatch = v.B; a.in_len = P_d; a.out_len = P_d;
    set_taps_1d(a, c->t("voc.pre_w").dim(0), 1);
    a.bias = c->pf("voc.pre_b"); a.bias_mode = 1; a.act = ACT_LRELU; a.slope = 0.1f;
    a.out = v.A; a.o_bs = (long)Pmax * c->voc_c0; a.ldo = c->voc_c0;
    c->gemm(a);
}

// ConvTranspose1d as a polyphase GEMM: out[t][ph*Cout+co]                  hifigan.py:118
void voc_upsample(zvx_ctx* c, const VocCall& v, const VocStage& s) {
    const int u = c->voc_rates[s.i], ku = c->voc_ksizes[s.i], B = v.B, Cin = s.Cin, Cout = s.Cout, rows_in = s.rows_in, dt_in = s.dt_in;
    const std::string up = "voc.up" + std::to_string(s.i);
    GemmArgs a = gemm_base(dt_in);
    a.out_dtype = s.dt;
    a.X = v.A; a.x_bs = (long)rows_in * Cin; a.ldx = Cin; a.ldw = Cin;
    a.M = rows_in; a.K = Cin; a.nbatch = B; a.in_len = s.len_in; a.out_len = s.len_in;
    a.bias_mode = 1; a.act = ACT_LRELU; a.slope = 0.1f;
    a.o_bs = (long)rows_in * u * Cout; a.ldo = u * Cout;
    if (dt_in != DT_F32 && c->has(up + "_wlo")) {
        // k = 2u: two 2-tap GEMMs over half the phases each (rows t-1, t / rows t, t+1) instead of one 3-tap GEMM
        const int hc = (u / 2) * Cout;
        a.N = hc; a.ntaps = 2; a.w_ts = (long)hc * Cin; a.flops = 2.0 * B * (double)rows_in * Cin * Cout * ku / 2;
        a.W = voc_weight(c, up + "_wlo", dt_in).dev; a.dv[0] = -1; a.dv[1] = 0;
        a.bias = c->pf(up + "_b"); a.out = v.X0;
        c->gemm(a);
        a.Wp = nullptr;
        a.W = voc_weight(c, up + "_whi", dt_in).dev; a.dv[0] = 0; a.dv[1] = 1;
        a.bias = c->pf(up + "_b") + hc; a.out = (char*)v.X0 + (size_t)hc * c->es();
        c->gemm(a);
    } else {
        a.W = voc_weight(c, up + "_w", dt_in).dev; a.w_ts = (long)u * Cout * Cin; a.N = u * Cout;
        a.ntaps = 3; a.dv[0] = -1; a.dv[1] = 0; a.dv[2] = 1;
        a.bias = c->pf(up + "_b"); a.out = v.X0;
        a.flops = 2.0 * B * (double)rows_in * Cin * Cout * ku;
        c->gemm(a);
    }
}

// narrowstage.hip's fragment-order weights and biases of a stage (convolution 6 j + 2 t + {0: conv1, 1: conv2}), per (stage, dtype): built on first use
const zvx_ctx::NsWeights& voc_narrow_weights(zvx_ctx* c, const VocCall& v, const VocStage& s) {
    const int Cout = s.Cout, nk = v.nk;
    const std::string key = "voc.ns." + std::to_string(s.i) + (s.dt == DT_F16 ? ".h16" : "");
    auto it = c->ns_weights.find(key);
    if (it != c->ns_weights.end()) return it->second;
    zvx_ctx::NsWeights nw;
    int nfrag = 0;
    for (int j = 0; j < nk; j++) for (int q = 0; q < 6; q++) { nw.woff[6 * j + q] = nfrag; nfrag += narrowstage_steps(Cout, c->voc_rb_k[j]); }
    nw.W = c->buf(key + ".w", (size_t)nfrag * 1024);
    nw.bias = c->fbuf(key + ".b", (size_t)6 * nk * Cout);
    for (int j = 0; j < nk; j++) {
        const RbWeights w = voc_rb_weights(c, v, s, j);
        for (int t = 0; t < 3; t++)
            for (int q = 0; q < 2; q++) {
                const RbConv& cv = q ? w.c2[t] : w.c1[t];
                if (cv.w->dims.size() != 3 || cv.w->dim(0) != c->voc_rb_k[j] || cv.w->dim(1) != Cout || cv.w->dim(2) != Cout) fail(ZVX_E_MANIFEST, "weights: '%s' has an unexpected shape", cv.name.c_str());
                const int ci = 6 * j + 2 * t + q;
                launch_pack_narrow(cv.w->dev, c->voc_rb_k[j], Cout, (char*)nw.W + (size_t)nw.woff[ci] * 1024, c->stream);
                HIPCHK(hipMemcpyAsync(nw.bias + (size_t)ci * Cout, cv.bias, (size_t)Cout * 4, hipMemcpyDeviceToDevice, c->stream));
            }
    }
    return c->ns_weights.emplace(key, nw).first->second;
}

// narrow stages (C = 16 / 8: HiFi-GAN V2's last two): all ResBlocks of the stage, their mean and the next stage's activation in ONE
// launch -- the stage tensor crosses HBM once in, once out (narrowstage.hip).  false: not covered, nothing launched
bool voc_narrow_stage(zvx_ctx* c, const VocCall& v, const VocStage& s) {
    const int Cout = s.Cout, nk = v.nk, rows = s.rows;
    if (!c->use_stagefuse || c->sat_check || c->voc_resblock != 1 || s.dt == DT_F32 || (Cout != 16 && Cout != 8) || nk < 1 || nk > 3) return false;
    for (int j = 0; j < nk; j++) if (c->voc_rb_d[j].size() != 3) return false;
    const zvx_ctx::NsWeights& nw = voc_narrow_weights(c, v, s);
    StageArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.X = v.X0; sa.x_bs = (long)rows * Cout; sa.ldx = Cout; sa.W = nw.W; sa.bias = nw.bias;
    memcpy(sa.woff, nw.woff, sizeof sa.woff);
    sa.C = Cout; sa.nk = nk;
    for (int j = 0; j < nk; j++) { sa.ks[j] = c->voc_rb_k[j]; for (int t = 0; t < 3; t++) sa.dil[j][t] = c->voc_rb_d[j][t]; }
    sa.out = v.A; sa.o_bs = (long)rows * Cout; sa.ldo = Cout;
    sa.slope1 = 0.1f; sa.res_inv_slope = 10.0f; sa.slope = s.next_slope;
    sa.len = s.len; sa.M = rows; sa.nbatch = v.B; sa.f16 = s.dt == DT_F16;
    if (!launch_narrowstage(sa, c->stream, true)) return false;
    const int vid = Cout == 16 ? 24 : 25;
    c->profiled([&] { return vid; }, [&] {
        if (!launch_narrowstage(sa, c->stream, false)) fail(ZVX_E_INVALID, "launch_narrowstage rejected a stage its dry run accepted (C=%d)", Cout);
        return vid;
    }, [&](GemmEvent& ev) {
        double ksum = 0; for (int j = 0; j < nk; j++) ksum += c->voc_rb_k[j];
        const double rws = (double)rows * v.B;
        ev.flops = 2.0 * rws * Cout * Cout * 6.0 * ksum; ev.rows = (long)rws; ev.N = Cout; ev.K = Cout; ev.taps = (int)ksum; ev.fused = 100 + nk;
        ev.bytes = rws * Cout * 2.0 * 2.0;
    });
    return true;
}

// Single requests: the ResBlocks of a stage only meet in the running sum, which their LAST pair updates.  Everything
// before that (two of three pairs) runs on a stream of its own for the 2nd and 3rd ResBlock, with its own temporaries;
// the last pairs stay on the main stream in the order 1, 2, 3, so xs accumulates exactly as before (bit-identical).
// The critical path of a per-pair stage drops from 18 to 10 launches.
// voc_side_begin: once per stage, behind the upsampling; SideHop: one per ResBlock, owns c->stream while the block is issued and puts
// the main stream back when it leaves scope (an exception included).  aux == nullptr: the block stays on the main stream.
void voc_side_begin(zvx_ctx* c) {
    for (int q = 0; q < 2; q++) if (!c->voc_aux[q]) HIPCHK(hipStreamCreateWithFlags(&c->voc_aux[q], hipStreamNonBlocking));
    for (int q = 0; q < 3; q++) if (!c->voc_ev[q]) HIPCHK(hipEventCreateWithFlags(&c->voc_ev[q], hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->voc_ev[0], c->stream));      // the stage input (and everything the previous stage read) is settled
}
struct SideHop {
    zvx_ctx* const c; hipStream_t const main_stream, aux; hipEvent_t const done; bool on_aux = false;
    SideHop(zvx_ctx* c_, hipStream_t aux_, hipEvent_t done_) : c(c_), main_stream(c_->stream), aux(aux_), done(done_) {
        if (aux) HIPCHK(hipStreamWaitEvent(aux, c->voc_ev[0], 0));
    }
    ~SideHop() { c->stream = main_stream; }
    void to_aux() { if (aux && !on_aux) { c->stream = aux; on_aux = true; } }
    void to_main() {
        if (on_aux) {
            HIPCHK(hipEventRecord(done, aux));
            c->stream = main_stream; on_aux = false;
            HIPCHK(hipStreamWaitEvent(main_stream, done, 0));
        }
    }
};

// ResBlock j of a stage: reads X0, and closes the stage (stage_close) with its last launch.  Tried in this order: the whole block as one
// streaming launch; for three pairs the first two + the last one as streaming launches; a fused ResBlock2; then pair by pair (a fused pair
// or two launches each).  A new way to run a block belongs HERE, on top of voc_rb_weights, close_stage and the context's profiled launches.
void voc_resblock(zvx_ctx* c, const VocCall& v, const VocStage& s, int j) {
    const int B = v.B, rows = s.rows, Cout = s.Cout, dt = s.dt;
    const bool side = v.side_ok && j >= 1;
    SideHop hop(c, side ? c->voc_aux[j - 1] : nullptr, side ? c->voc_ev[j] : nullptr);
    void* const T1s = side ? v.sideT1[j - 1] : v.T1;
    void* const* const PPs = side ? v.sidePP[j - 1] : v.PP;
    const int k = c->voc_rb_k[j];
    const std::vector<int>& dil = c->voc_rb_d[j];
    const int nd = (int)dil.size();
    const RbWeights w = voc_rb_weights(c, v, s, j);
    const StageClose close = stage_close(j, v.nk);
    const void* cur = v.X0;
    int pp = 0;
    int t_first = 0;
    if (c->voc_resblock == 1 && dt != DT_F32 && c->use_resstream && !c->sat_check && nd >= 1 && nd <= 3) {
        // whole ResBlock (or its first two pairs + the last one) as streaming launches: the stage tensor crosses HBM once
        bool packed_ok = true;
        for (int t = 0; t < nd; t++) packed_ok = packed_ok && w.c1[t].packed && w.c2[t].packed;
        auto chain = [&](int t0, int np, const void* in, bool closes) {
            StreamArgs sa;
            memset(&sa, 0, sizeof sa);
            sa.X = in; sa.x_bs = (long)rows * Cout; sa.ldx = Cout; sa.C = Cout; sa.ntaps = k; sa.npair = np;
            for (int q = 0; q < np; q++) {
                sa.W1[q] = w.c1[t0 + q].packed; sa.W2[q] = w.c2[t0 + q].packed;
                sa.b1[q] = w.c1[t0 + q].bias; sa.b2[q] = w.c2[t0 + q].bias;
                sa.dil[q] = dil[t0 + q];
            }
            sa.seg_min = c->rs_seg_min; sa.f16 = dt == DT_F16;
            if (c->rs_prof) sa.prof = (long long*)c->buf("rs.prof." + w.name + "." + std::to_string(t0), 16 * 16 * 8);   // RS_PROFILE builds only
            sa.slope1 = 0.1f; sa.res_inv_slope = 10.0f; sa.out_scale = 1.f; sa.slope = 0.1f;
            sa.len = s.len; sa.M = rows; sa.nbatch = B; sa.o_bs = (long)rows * Cout; sa.ldo = Cout; sa.a_bs = (long)rows * Cout; sa.lda = Cout;
            if (closes) close_stage(sa, close, v, s);
            else sa.out = PPs[pp];
            return sa;
        };
        if (packed_ok) {
            StreamArgs whole = chain(0, nd, v.X0, true);
            hop.to_main();
            if (c->run_stream(whole)) t_first = nd;
            else if (nd == 3) {
                StreamArgs head = chain(0, 2, v.X0, false);
                StreamArgs probe = chain(2, 1, PPs[pp], true);
                if (launch_resstream(head, c->stream, true) >= 0 && launch_resstream(probe, c->stream, true) >= 0) {
                    hop.to_aux();
                    c->run_stream(head);
                    cur = PPs[pp]; pp ^= 1;
                    StreamArgs tail = chain(2, 1, cur, true);
                    hop.to_main();
                    c->run_stream(tail);
                    t_first = nd;
                }
            }
        }
    }
    auto rb_base = [&] {
        GemmArgs a = gemm_base(dt);
        a.M = rows; a.N = Cout; a.K = Cout; a.nbatch = B; a.in_len = s.len; a.out_len = s.len; a.ldw = Cout; a.w_ts = (long)Cout * Cout;
        a.x_bs = (long)rows * Cout; a.ldx = Cout; a.o_bs = (long)rows * Cout; a.ldo = Cout;
        return a;
    };
    if (c->voc_resblock == 2 && nd == 2 && dt != DT_F32 && c->use_rb2fuse && !c->sat_check && (Cout == 32 || Cout == 64) && w.c1[0].packed && w.c1[1].packed) {
        // a whole ResBlock2 (hifigan.py:77-82: x1 = x + c_0(lrelu(x)); x2 = x1 + c_1(lrelu(x1))) as ONE launch: lrelu(x1) stays in LDS
        // (rb2fuse_kernel) -- two trips of the stage tensor per block instead of six
        GemmArgs a = rb_base();
        a.X = v.X0; a.W = w.c1[1].w->dev; a.Wp = w.c1[1].packed; a.Wp2 = w.c1[0].packed;
        a.bias1 = w.c1[0].bias; a.slope1 = 0.1f; a.fused = 2;
        set_taps_1d(a, k, dil[1]);
        for (int q = 0; q < k; q++) a.dv1[q] = (q - (k - 1) / 2) * dil[0];
        a.bias = w.c1[1].bias; a.bias_mode = 1;
        a.res = v.X0; a.r_bs = (long)rows * Cout; a.ldr = Cout; a.res_mode = 2; a.res_inv_slope = 10.0f; a.res_dtype = dt;
        close_stage(a, close, v, s);
        a.flops = 2.0 * 2.0 * B * (double)rows * Cout * Cout * k;
        if (gemm_variant_of(a) >= 0) { hop.to_main(); c->gemm(a); t_first = nd; }
    }
    for (int t = t_first; t < nd; t++) {
        const bool last = (t == nd - 1);
        if (last) hop.to_main(); else hop.to_aux();
        // what the LAST conv of the iteration does with its result: + bias + x (raw residual recovered from the activated
        // input), then either the next iteration's input (activated) or the stage's running sum / mean
        auto rb_tail = [&](GemmArgs& a) {
            a.bias_mode = 1;
            a.res = cur; a.r_bs = (long)rows * Cout; a.ldr = Cout; a.res_mode = 2; a.res_inv_slope = 10.0f; a.res_dtype = dt;
            if (last) close_stage(a, close, v, s);
            else { a.act = ACT_LRELU; a.slope = 0.1f; a.out = PPs[pp]; }
        };
        GemmArgs a = rb_base();
        if (c->voc_resblock == 1) {
            const RbConv& c1 = w.c1[t]; const RbConv& c2 = w.c2[t];
            bool fuse = dt != DT_F32 && !c->sat_check && c1.packed && c2.packed;
            if (fuse) {
                // one launch: xt = lrelu(c1(x_act)+b1) stays in LDS; x' = c2(xt) + b2 + x      hifigan.py:51-55
                a.X = cur; a.W = c2.w->dev; a.Wp = c2.packed; a.Wp2 = c1.packed;
                a.bias1 = c1.bias; a.slope1 = 0.1f; a.fused = 1;
                a.no_pairstream = c->use_pairstream <= 0 ? 1 : (c->use_pairstream == 3 ? 2 : 0);
                set_taps_1d(a, k, 1);
                for (int q = 0; q < k; q++) a.dv1[q] = (q - (k - 1) / 2) * dil[t];
                a.bias = c2.bias;
                a.flops = 2.0 * 2.0 * B * (double)rows * Cout * Cout * k;
                rb_tail(a);
                // the fused kernels cover a subset of (C, k, dilation, LDS footprint): ask the launcher (dry run) first
                const int fv = gemm_variant_of(a);
                // C = 128: the pair kernel, or -- where it declines (small jobs) -- the two conv-slab launches it is bit-identical to:
                // an utterance must come out the same alone and inside a large batch
                fuse = fv >= 0 && !(Cout == 128 && fv != 23);
            }
            if (!fuse) {
                // xt = c1(lrelu(x)); stored as lrelu(xt)                       hifigan.py:51-53
                a = rb_base();
                a.X = cur; a.W = c1.w->dev;
                set_taps_1d(a, k, dil[t]);
                a.bias = c1.bias; a.bias_mode = 1; a.act = ACT_LRELU; a.slope = 0.1f;
                a.out = T1s;
                c->gemm(a);
                // x = c2(.) + x                                                hifigan.py:54-55
                a = rb_base();
                a.X = T1s; a.W = c2.w->dev;
                set_taps_1d(a, k, 1);
                a.bias = c2.bias;
                rb_tail(a);
            }
        } else {
            // x = c(lrelu(x)) + x                                          hifigan.py:78-81
            a.X = cur; a.W = w.c1[t].w->dev;
            set_taps_1d(a, k, dil[t]);
            a.bias = w.c1[t].bias;
            rb_tail(a);
        }
        c->gemm(a);
        if (!last) { cur = PPs[pp]; pp ^= 1; }
    }
}
}  // namespace

void run_vocoder(zvx_ctx* c, const float* mel, int ldm, int Lmel_max, const int* mel_len_host, const int* P_host, int B,
                 void* wav_dev, long wav_stride, int pcm16) {
    const std::vector<int> dom = voc_domains(c);
    const int nm = c->n_mels;
    const size_t es = dtype_size(c->dt);
    int Pmax = 0; for (int b = 0; b < B; b++) Pmax = std::max(Pmax, P_host[b]);
    if (Pmax <= 0) return;
    const int ns = (int)c->voc_rates.size(), nk = (int)c->voc_rb_k.size();
    // per-stage valid row counts
    std::vector<int> lens((size_t)(ns + 2) * B);
    for (int b = 0; b < B; b++) { lens[b] = mel_len_host[b]; lens[B + b] = P_host[b]; }
    int mul = 1;
    for (int i = 0; i < ns; i++) { mul *= c->voc_rates[i]; for (int b = 0; b < B; b++) lens[(size_t)(i + 2) * B + b] = P_host[b] * mul; }
    VocCall v{};
    v.B = B; v.Pmax = Pmax; v.nk = nk;
    v.lens_d = c->upload_ints("voc.lens", lens.data(), lens.size());
    const int* mel_len_d = v.lens_d; const int* P_d = v.lens_d + B;

    size_t maxel = (size_t)Pmax * c->voc_c0; mul = 1;
    for (int i = 0; i < ns; i++) { mul *= c->voc_rates[i]; maxel = std::max(maxel, (size_t)Pmax * mul * (size_t)(c->voc_c0 >> (i + 1))); }
    maxel *= B;
    void* vin = c->buf("voc.in", (size_t)B * Pmax * nm * es);
    v.A = c->buf("voc.A", maxel * es);
    v.X0 = c->buf("voc.X0", maxel * es);
    v.T1 = c->buf("voc.T1", maxel * es);
    v.PP[0] = c->buf("voc.PP0", maxel * es); v.PP[1] = c->buf("voc.PP1", maxel * es);
    v.XS = c->buf("voc.XS", maxel * es);         // in the activation dtype
    // temporaries of the ResBlocks that run beside the first one (single requests, SideHop).  Taken HERE: a new buffer is zero-filled
    // on the main stream, which the side streams only follow from the stage-input event on
    // tools/ab_voc_overlap.py: -5 ... -24 % for every batch below the headline's size (most where B leaves a ragged last round of
    // workgroups: B = 6 / 12), +-1 % at 32 x 896 frames, which therefore keeps the serial schedule
    v.side_ok = nk >= 2 && nk <= 3 && B <= c->voc_overlap_maxb && (long)B * Pmax < c->voc_overlap_frames;
    if (v.side_ok)
        for (int j = 1; j < nk; j++) {
            v.sideT1[j - 1] = c->buf("voc.T1." + std::to_string(j), maxel * es);
            v.sidePP[j - 1][0] = c->buf("voc.PP0." + std::to_string(j), maxel * es); v.sidePP[j - 1][1] = c->buf("voc.PP1." + std::to_string(j), maxel * es);
        }

    c->tag = "voc.pre";
    launch_mel_pad(mel, DT_F32, ldm, Lmel_max, mel_len_d, vin, dom[0], nm, Pmax, P_d, B, nm, c->stream);     // model.py:331-335
    c->sat_scan(vin, dom[0], (long)Pmax * nm, nm, B, Pmax, P_d, nm);
    if (c->front_stream && c->stream != c->front_stream) {   // the mel buffer is free again: a queued call's decoder (front stream) may overwrite it
        HIPCHK(hipEventRecord(c->ev_mel_free, c->stream));
        c->mel_free_pending = true;
    }
    voc_conv_pre(c, v, vin, dom[0]);
    int Cin = c->voc_c0, rows = Pmax;
    for (int i = 0; i < ns; i++) {
        VocStage s;
        s.i = i; s.Cin = Cin; s.Cout = Cin / 2; s.rows_in = rows; s.rows = rows * c->voc_rates[i];
        s.len_in = v.lens_d + (size_t)(i + 1) * B; s.len = v.lens_d + (size_t)(i + 2) * B;
        s.dt_in = dom[i]; s.dt = dom[i + 1];
        s.next_slope = (i == ns - 1) ? 0.01f : 0.1f;          // hifigan.py:126 uses the default slope 0.01
        c->tag = "voc.up" + std::to_string(i + 1);
        voc_upsample(c, v, s);
        c->tag = "voc.res" + std::to_string(i + 1);
        if (!voc_narrow_stage(c, v, s)) {
            if (v.side_ok) voc_side_begin(c);
            for (int j = 0; j < nk; j++) voc_resblock(c, v, s, j);
        }
        Cin = s.Cout; rows = s.rows;
    }
    // conv_post + tanh on the first mel_len*hop samples            hifigan.py:127-128, model.py:347
    c->tag = "voc.post";
    {
        double nout = 0; for (int b = 0; b < B; b++) nout += (double)mel_len_host[b] * c->hop;
        // rows are zero-filled up to max_b(mel_len) * hop, the extent include/zvx.h promises (and the caller's wav_stride covers):
        // Lmel_max is only the input's row stride and may be larger
        int nmax = 0; for (int b = 0; b < B; b++) nmax = std::max(nmax, mel_len_host[b] * c->hop);
        if ((long)nmax > wav_stride) nmax = (int)wav_stride;
        const int kp = c->t("voc.post_w").dim(0);
        c->timed(2.0 * nout * Cin * kp, nout * (Cin * es + (pcm16 ? 2.0 : 4.0)), [&] {
            launch_conv_post_tanh(v.A, dom[ns], Cin, (long)rows * Cin, c->pf("voc.post_w"), c->t("voc.post_b").host[0], kp,
                                  Cin, wav_dev, wav_stride, pcm16, B, nmax, P_d, c->hop, mel_len_d, c->hop, c->stream);
        });
    }
    c->tag = "other";
}

// ------------------------------------------------------------------------------------------------
// speaker encoder (ResNetSE34V2.py:176-212)
// ------------------------------------------------------------------------------------------------

namespace {
// The encoder behind the mels: mels_d [B][Tmax][n_mels] f32 on the device, lens[b] in 2..Tmax (checked by the caller) -> "spk.emb" [B][hidden],
// queued on the context's stream.  Shared by zvx_spkemb / zvx_spkemb_ex (run_spkemb) and zvx_spkemb_wav.
float* spkemb_from_mels(zvx_ctx* c, const float* mels_d, const int32_t* lens, int B, int Tmax) {
    const int dt = c->dt, F0 = c->n_mels, H = c->H;
    const size_t es = c->es();
    // widths per resolution level: w0 = T, w_{l+1} = (w_l - 1)/2 + 1  (3x3 stride-2 pad-1 conv)
    std::vector<int> W(4 * (size_t)B);
    int Wmax[4] = {Tmax, 0, 0, 0};
    for (int b = 0; b < B; b++) { int w = lens[b]; for (int l = 0; l < 4; l++) { W[(size_t)l * B + b] = w; w = (w - 1) / 2 + 1; } }
    for (int l = 1; l < 4; l++) Wmax[l] = (Wmax[l - 1] - 1) / 2 + 1;
    // Map rows are stored one position wider than the widest utterance: that last column is never a valid position, so a
    // stride-1 3 x 3 convolution may run over the FLATTENED map (the neighbour of a row's last position is masked, not the next
    // row's first) -- see launch_gemm.  Every consumer masks columns >= W[b] on the way in.
    int WS[4]; for (int l = 0; l < 4; l++) WS[l] = Wmax[l] + 1;
    int Fh[4]; Fh[0] = F0; for (int l = 1; l < 4; l++) Fh[l] = (Fh[l - 1] - 1) / 2 + 1;
    int* W_d = c->upload_ints("spk.W", W.data(), W.size());

    const int C0 = c->rn_filters[0];
    size_t maxel = 0;
    for (int l = 0; l < 4; l++) maxel = std::max(maxel, (size_t)B * Fh[l] * WS[l] * c->rn_filters[l]);
    void* mA = c->buf("spk.mA", maxel * es); void* mB = c->buf("spk.mB", maxel * es);
    void* mC = c->buf("spk.mC", maxel * es); void* mD = c->buf("spk.mD", maxel * es);
    float* mean = c->fbuf("spk.mean", (size_t)B * 256 * 16); float* rstd = c->fbuf("spk.rstd", (size_t)B * 256 * 16);
    float* sescale = c->fbuf("spk.sescale", (size_t)B * 1024);

    // InstanceNorm1d over time (no affine) folded into the first conv          ResNetSE34V2.py:182-186
    launch_instnorm_stats(mels_d, DT_F32, F0, B, Tmax, W_d, F0, 1e-5f, mean, rstd, c->stream);
    launch_spk_front(mels_d, Tmax, W_d, F0, mean, rstd, c->pf("spk.c1_w"), c->pf("spk.c1_b"), c->pf("spk.bn1_s"), c->pf("spk.bn1_t"), C0,
                     mA, dt, B, WS[0], c->stream);
    void* x = mA; void* o1 = mB; void* o2 = mC; void* rs = mD;
    int lvl = 0, Cin = C0;
    for (size_t li = 0; li < c->rn_layers.size(); li++) {
        const int planes = c->rn_filters[li];
        for (int bi = 0; bi < c->rn_layers[li]; bi++) {
            const std::string p = "spk.l" + std::to_string(li + 1) + "." + std::to_string(bi);
            const int stride = (li > 0 && bi == 0) ? 2 : 1;
            const int lin = lvl, lout = (stride == 2) ? lvl + 1 : lvl;
            const int Hin = Fh[lin], Win = WS[lin], Hout = Fh[lout], Wout = WS[lout];
            const int* win_d = W_d + (size_t)lin * B; const int* wout_d = W_d + (size_t)lout * B;
            int pool_S = 0;                                                   // > 0: conv2's launch wrote the SE pool's partial sums itself
            auto conv3 = [&](const std::string& wn, const void* in, int cin, int hin, int win, const int* inlen, int st, void* out,
                             const float* bias, int act, const float* ps, const float* pt, int ksz, float* se_part = nullptr) {
                GemmArgs a = gemm_base(dt);
                a.X = in; a.x_bs = (long)hin * win * cin; a.ldx = cin; a.W = c->t(wn).dev; a.ldw = cin; a.w_ts = (long)planes * cin;
                a.M = Hout * Wout; a.N = planes; a.K = cin; a.nbatch = B; a.in_len = inlen; a.out_len = wout_d;
                a.stride = st; a.wout = Wout; a.hin = hin; a.win = win;
                a.ntaps = ksz * ksz;
                for (int i = 0; i < ksz; i++) for (int j = 0; j < ksz; j++) { a.du[i * ksz + j] = (int)(i - ksz / 2); a.dv[i * ksz + j] = (int)(j - ksz / 2); }
                if (bias) { a.bias = bias; a.bias_mode = 1; }
                a.act = act; a.post_scale = ps; a.post_shift = pt;
                a.out = out; a.o_bs = (long)Hout * Wout * planes; a.ldo = planes;
                if (se_part) { a.se_part = se_part; a.se_part_S = &pool_S; }
                c->gemm(a);
            };
            // conv1 -> ReLU -> BN1                                          ResNetSE34V2.py:86-88
            // (level transition: conv1 and the shortcut's 1 x 1 convolution, both stride 2 over the same input, in one launch where
            // conv2d_s2_kernel covers the shape)
            bool ds_done = false;
            if (stride == 2 && c->has(p + ".ds") && dt == DT_BF16 && c->spk_s2_fuse) {
                GemmArgs a = gemm_base(dt);
                a.X = x; a.x_bs = (long)Hin * Win * Cin; a.ldx = Cin; a.W = c->t(p + ".c1").dev; a.ldw = Cin; a.w_ts = (long)planes * Cin;
                a.M = Hout * Wout; a.N = planes; a.K = Cin; a.nbatch = B; a.in_len = win_d; a.out_len = wout_d;
                a.stride = 2; a.wout = Wout; a.hin = Hin; a.win = Win; a.ntaps = 9;
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { a.du[i * 3 + j] = i - 1; a.dv[i * 3 + j] = j - 1; }
                a.act = ACT_RELU; a.post_scale = c->pf(p + ".bn1_s"); a.post_shift = c->pf(p + ".bn1_t");
                a.out = o1; a.o_bs = (long)Hout * Wout * planes; a.ldo = planes;
                auto itp = c->packed.find(c->t(p + ".ds").dev);
                if (itp != c->packed.end()) {
                    a.ds_out = rs; a.ds_Wp = itp->second; a.ds_bias = c->pf(p + ".ds_b");
                    a.flops = 2.0 * (double)a.M * B * planes * (double)Cin * 10;
                    auto itw = c->packed.find(a.W); if (itw != c->packed.end()) a.Wp = itw->second;
                    a.slab_small = c->slab_small;
                    if (gemm_variant_of(a) >= 0) { c->gemm(a); ds_done = true; }
                }
            }
            if (!ds_done)
            conv3(p + ".c1", x, Cin, Hin, Win, win_d, stride, o1, nullptr, ACT_RELU, c->pf(p + ".bn1_s"), c->pf(p + ".bn1_t"), 3);
            // conv2 (+ folded BN2)                                           :90-91
            // SE: global average pool -> fc -> relu -> fc -> sigmoid        :63-67
            // (the persistent 2-D convolution of the C = 32 / 64 levels leaves the pool's partial sums itself -- one per (row tile, wave):
            // at most ceil(H W / 256) x 4 of them; every other launch is followed by the pool pass)
            const int nsplit = se_pool_splits(Hout, Wout);
            const size_t part_max = std::max((size_t)nsplit, (size_t)((Hout * Wout + 255) / 256) * 4);
            float* separt = c->fbuf("spk.separt", (size_t)B * part_max * planes);
            conv3(p + ".c2", o1, planes, Hout, Wout, wout_d, 1, o2, c->pf(p + ".c2_b"), ACT_NONE, nullptr, nullptr, 3, c->spk_pool_fuse ? separt : nullptr);
            if (pool_S > 0) {
                if ((size_t)pool_S > part_max) fail(ZVX_E_STATE, "fused SE pool wrote %d partials, %zu allocated", pool_S, part_max);
                launch_se_fc(separt, pool_S, Hout, wout_d, c->pf(p + ".se_w1"), c->pf(p + ".se_b1"), c->pf(p + ".se_w2"), c->pf(p + ".se_b2"), planes, planes / 8, sescale, B, c->stream, c->pf(p + ".c2_b"));
            } else {
                launch_se_pool(o2, dt, B, Hout, Wout, wout_d, planes, separt, c->stream);
                launch_se_fc(separt, nsplit, Hout, wout_d, c->pf(p + ".se_w1"), c->pf(p + ".se_b1"), c->pf(p + ".se_w2"), c->pf(p + ".se_b2"), planes, planes / 8, sescale, B, c->stream);
            }
            const void* resid = x;
            if (c->has(p + ".ds")) {                                          // 1x1 stride-s conv + folded BN   :94-95
                if (!ds_done) conv3(p + ".ds", x, Cin, Hin, Win, win_d, stride, rs, c->pf(p + ".ds_b"), ACT_NONE, nullptr, nullptr, 1);
                resid = rs;
            }
            launch_se_apply(o2, resid, o1, dt, sescale, B, Hout, Wout, wout_d, planes, c->stream);     // out*y + residual -> ReLU  :97-98
            std::swap(x, o1);
            lvl = lout; Cin = planes;
        }
    }
    // attention + ASP pooling                                               ResNetSE34V2.py:195-205
    const int Fp = Fh[3], Wp = WS[3], C4 = c->rn_filters[3], D = Fp * C4;
    const int* w3_d = W_d + (size_t)3 * B;
    void* ah = c->buf("spk.ah", (size_t)B * Wp * 128 * es);
    float* logits = c->fbuf("spk.logits", (size_t)B * Wp * D);
    {
        GemmArgs a = gemm_base(dt);       // Conv1d(D -> 128) over features (f, c): one tap per frequency row of the map
        a.X = x; a.x_bs = (long)Fp * Wp * C4; a.ldx = C4; a.W = c->t("spk.att1_w").dev; a.ldw = C4; a.w_ts = (long)128 * C4;
        a.M = Wp; a.N = 128; a.K = C4; a.nbatch = B; a.in_len = w3_d; a.out_len = w3_d;
        a.wout = Wp; a.hin = Fp; a.win = Wp; a.stride = 1;
        a.ntaps = Fp; for (int f = 0; f < Fp; f++) { a.du[f] = (int)f; a.dv[f] = 0; }
        a.bias = c->pf("spk.att1_b"); a.bias_mode = 1; a.act = ACT_RELU; a.post_scale = c->pf("spk.att_bn_s"); a.post_shift = c->pf("spk.att_bn_t");
        a.out = ah; a.o_bs = (long)Wp * 128; a.ldo = 128;
        c->gemm(a);
    }
    {
        GemmArgs a = gemm_base(dt);
        a.X = ah; a.x_bs = (long)Wp * 128; a.ldx = 128; a.W = c->t("spk.att2_w").dev; a.ldw = 128;
        a.M = Wp; a.N = D; a.K = 128; a.nbatch = B; a.in_len = w3_d; a.out_len = w3_d;
        a.bias = c->pf("spk.att2_b"); a.bias_mode = 1;
        a.out = logits; a.out_dtype = DT_F32; a.o_bs = (long)Wp * D; a.ldo = D;
        c->gemm(a);
    }
    const int PD = c->rn_asp ? 2 * D : D;                 // ASP: [mu | sg], SAP: mu     ResNetSE34V2.py:135-143, 199-205
    if (c->t("spk.fc_w").dim(2) != PD) fail(ZVX_E_MANIFEST, "spk.fc_w has %d inputs, the %s pooling produces %d", c->t("spk.fc_w").dim(2), c->rn_asp ? "ASP" : "SAP", PD);
    float* pooled = c->fbuf("spk.pooled", (size_t)B * PD);
    launch_asp_pool(x, dt, logits, B, Fp, Wp, w3_d, C4, pooled, c->rn_asp, c->stream);
    float* emb = c->fbuf("spk.emb", (size_t)B * H);
    // Linear(PD -> hidden): a few rows against a 5120-long K -- one wave per output column      ResNetSE34V2.py:207
    launch_fc_rows(pooled, PD, (const float*)c->t("spk.fc_w").dev, PD, c->pf("spk.fc_b"), emb, H, B, H, PD, c->stream);
    launch_l2norm_rows(emb, B, H, c->stream);                                  // F.normalize   :209-210
    return emb;
}

void run_spkemb(zvx_ctx* c, const float* ref_mels, const int32_t* lens, int B, int Tmax, float* out, int flags) {
    const int F0 = c->n_mels, H = c->H;
    for (int b = 0; b < B; b++) if (lens[b] < 2 || lens[b] > Tmax) fail(ZVX_E_INVALID, "ref mel length %d out of range (2..%d)", lens[b], Tmax);
    c->stage_begin(ZVX_T_SPKEMB);
    c->tag = "spkemb";
    float* mels_d = c->fbuf("spk.mels", (size_t)B * Tmax * F0);
    HIPCHK(hipMemcpyAsync(mels_d, ref_mels, (size_t)B * Tmax * F0 * 4, (flags & ZVX_DEVICE_IN) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    const float* emb = spkemb_from_mels(c, mels_d, lens, B, Tmax);
    c->stage_end(ZVX_T_SPKEMB);
    HIPCHK(hipMemcpyAsync(out, emb, (size_t)B * H * 4, (flags & ZVX_DEVICE_OUT) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!((flags & ZVX_DEVICE_OUT) && (flags & ZVX_NO_SYNC))) c->sync();
}

// copy device rows [B][rows_max][C] (f32 contiguous) to a caller buffer with row stride
void copy_out_rows(zvx_ctx* c, const float* src, int rows_max, int C, float* dst, long dst_rows_stride, int B, bool device_out) {
    if (!dst) return;
    if (dst_rows_stride < rows_max) fail(ZVX_E_BUFFER, "output row stride %ld < %d rows", dst_rows_stride, rows_max);
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_rows_stride * C * 4, src, (size_t)rows_max * C * 4, (size_t)rows_max * C * 4, B,
                            device_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
}

// ------------------------------------------------------------------------------------------------
// log-mel front end of the reference audio (mels.py:357-395 get_mel_from_wav), f32 throughout:
// reflect pad -> |STFT| as a GEMM against the windowed DFT basis (rows = hop-strided frames of the padded signal)
// -> mel basis GEMM -> log(clip(., 1e-5))
// ------------------------------------------------------------------------------------------------
// The front end behind the padding: padded [B][Npad] f32 (row b: its reflect-padded signal, then zeros), fr_d[b] frames on the device, Tf = the
// most frames of a row -> "mel.out" [B][Tf][n_mels], queued on the context's stream.  Shared by zvx_melspec (run_melspec) and zvx_spkemb_wav.
float* mel_from_padded(zvx_ctx* c, const float* padded, long Npad, const int* fr_d, int B, int Tf) {
    const Tensor& dft = c->t("mel.dft");
    const Tensor& basis = c->t("mel.basis");
    const int n_fft = dft.dim(2), NR = dft.dim(1), KP = basis.dim(2), nf = n_fft / 2 + 1, nm = c->n_mels, hop = c->hop;
    float* spec = c->fbuf("mel.spec", (size_t)B * Tf * NR);
    {
        GemmArgs a = gemm_base(DT_F32);
        a.X = padded; a.x_bs = Npad; a.ldx = hop; a.W = dft.dev; a.ldw = n_fft; a.w_ts = (long)NR * n_fft;
        a.M = Tf; a.N = NR; a.K = n_fft; a.nbatch = B; a.in_len = fr_d; a.out_len = fr_d;
        a.out = spec; a.o_bs = (long)Tf * NR; a.ldo = NR;
        c->gemm(a);
    }
    float* mag = c->fbuf("mel.mag", (size_t)B * Tf * KP);
    launch_stft_mag(spec, NR, mag, KP, nf, B, Tf, fr_d, c->stream);
    float* mel_d = c->fbuf("mel.out", (size_t)B * Tf * nm);
    {
        GemmArgs a = gemm_base(DT_F32);
        a.X = mag; a.x_bs = (long)Tf * KP; a.ldx = KP; a.W = basis.dev; a.ldw = KP; a.w_ts = (long)nm * KP;
        a.M = Tf; a.N = nm; a.K = KP; a.nbatch = B; a.in_len = fr_d; a.out_len = fr_d;
        a.out = mel_d; a.o_bs = (long)Tf * nm; a.ldo = nm;
        c->gemm(a);
    }
    launch_log_clip(mel_d, nm, nm, 1e-5f, B, Tf, fr_d, c->stream);
    return mel_d;
}

// The lengths of a batch of waveforms as the front end takes them: frames per row and the most of them.  `side` NULL: zvx_melspec's own message;
// otherwise the caller's name and the side of its pair of batches (zvx_align_wav)
int melspec_frames(zvx_ctx* c, const char* who, const char* side, const int32_t* nsamples, int B, int Nmax, std::vector<int>& frames, int* b_long) {
    const int n_fft = c->t("mel.dft").dim(2), hop = c->hop;
    const int pad = (n_fft - hop) / 2;
    frames.assign((size_t)B, 0);
    int Tf = 0;
    *b_long = 0;
    for (int b = 0; b < B; b++) {
        const int n = nsamples[b];
        if (n > Nmax || n < pad + 1 || n + 2 * pad < n_fft) {
            if (!side) fail(ZVX_E_INVALID, "zvx_melspec: utterance %d has %d samples (need %d..%d)", b, n, std::max(pad + 1, n_fft - 2 * pad), Nmax);
            fail(ZVX_E_INVALID, "%s: side %s, row %d has %d samples (need %d..%d)", who, side, b, n, std::max(pad + 1, n_fft - 2 * pad), Nmax);
        }
        frames[b] = 1 + (n + 2 * pad - n_fft) / hop;
        if (frames[b] > Tf) { Tf = frames[b]; *b_long = b; }
    }
    return Tf;
}
// Upload (or, device_in, copy) the rows, pad, and queue the front end: "mel.out" [B][Tf][n_mels]; *fr_out: the frames on the device
float* melspec_queue(zvx_ctx* c, const float* wav, const int32_t* nsamples, const std::vector<int>& frames, int B, int Nmax, int Tf, bool device_in, int** fr_out) {
    const int n_fft = c->t("mel.dft").dim(2), hop = c->hop;
    const int pad = (n_fft - hop) / 2;
    const long Npad = ((long)Nmax + 2 * pad + 3) & ~3L;
    float* wav_d = c->fbuf("mel.wav", (size_t)B * Nmax);
    HIPCHK(hipMemcpyAsync(wav_d, wav, (size_t)B * Nmax * 4, device_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    int* n_d = c->upload_ints("mel.n", nsamples, B);
    int* fr_d = c->upload_ints("mel.frames", frames.data(), B);
    float* padded = c->fbuf("mel.pad", (size_t)B * Npad);
    launch_reflect_pad(wav_d, Nmax, n_d, padded, Npad, pad, B, (int)Npad, c->stream);
    if (fr_out) *fr_out = fr_d;
    return mel_from_padded(c, padded, Npad, fr_d, B, Tf);
}

void run_melspec(zvx_ctx* c, const float* wav, const int32_t* nsamples, int B, int Nmax, float* mel_out, int Tmax, int32_t* frames_out) {
    const int nm = c->n_mels;
    std::vector<int> frames;
    int b_long = 0;
    const int Tf = melspec_frames(c, "zvx_melspec", nullptr, nsamples, B, Nmax, frames, &b_long);
    if (Tf > Tmax) fail(ZVX_E_BUFFER, "zvx_melspec: the %d frames of utterance %d do not fit Tmax = %d", Tf, b_long, Tmax);
    c->stage_begin(ZVX_T_SPKEMB);
    float* mel_d = melspec_queue(c, wav, nsamples, frames, B, Nmax, Tf, false, nullptr);
    c->stage_end(ZVX_T_SPKEMB);
    if (mel_out) {
        if (Tmax > Tf) memset(mel_out, 0, (size_t)B * Tmax * nm * 4);
        copy_out_rows(c, mel_d, Tf, nm, mel_out, Tmax, B, false);
    }
    if (frames_out) memcpy(frames_out, frames.data(), B * sizeof(int));
    c->sync();
}

// ------------------------------------------------------------------------------------------------
// speaker enrolment from raw audio (include/zvx.h: zvx_spkemb_wav): resample -> trim bounds -> [the call's one wait] -> window cut with
// reflect padding -> log-mel -> speaker encoder.  Every step but the window cut is the launch sequence of the entry point that defines it.
// ------------------------------------------------------------------------------------------------
void do_spkemb_wav(zvx_ctx* c, const float* wav, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_ref_params* p, float* out,
                   int32_t* begin, int32_t* end, int32_t* frames_out, int flags) {
    if (!out) fail(ZVX_E_INVALID, "zvx_spkemb_wav: out is NULL");
    zvx_join_params jp{};
    if (p) { jp.frame = p->frame; jp.hop = p->hop; jp.top_db = p->top_db; jp.keep = p->keep; }
    join_check("zvx_spkemb_wav", wav, nsamples, B, Nmax, nullptr, p ? &jp : nullptr);
    if (p->max_samples < 0) fail(ZVX_E_INVALID, "zvx_spkemb_wav: max_samples %d must not be negative", p->max_samples);
    flags_check("zvx_spkemb_wav", flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC);
    const int native = model_rate(c);
    int L = 1, M = 1;
    rs_pair(rate, native, &L, &M);
    const RsPlan plan = rs_plan(nsamples, 1, B, L, M);
    std::vector<int> n(B);                                   // the rows' lengths at the model's rate
    for (int b = 0; b < B; b++) {
        if (rate != native && plan.cnt[b] > INT32_MAX - 8) fail(ZVX_E_INVALID, "zvx_spkemb_wav: row %d has %ld samples at the model's rate", b, plan.cnt[b]);
        n[b] = (int)plan.cnt[b];
    }
    const int n_fft = c->t("mel.dft").dim(2), hop = c->hop, pad = (n_fft - hop) / 2, H = c->H;
    // 1. the rows at the model's rate: as given, or each converted as a signal of its own length into a work buffer
    const float* rows = rows_to_device(c, "ref", wav, B, Nmax, flags);      // (each step uploads the lengths it reads)
    long rows_bs = Nmax;
    if (rate != native) {
        const zvx_ctx::RsBank& bk = rs_bank(c, L, M);
        const long ostride = (std::max(plan.out_max, 1L) + 7) & ~7L;
        float* conv = c->fbuf("ref.rs", (size_t)B * ostride);
        run_resample_rows(c, bk, plan_rows(plan, rows, rows_bs, conv, ostride, 4, nsamples, 1, B).data(), B, 0, plan.out_max);
        rows = conv; rows_bs = ostride;
    }
    // 2. the bounds, and the call's one wait
    const int* host = bounds_to_host(c, rows, n.data(), B, (int)rows_bs, &jp, ZVX_DEVICE_IN);
    // 3. / 4. crop, frame counts, and what zvx_melspec / zvx_spkemb ask of a signal
    std::vector<int> frames(B);
    int Mmax = 0, Tf = 0, bad = -1;
    const int m_min = std::max(std::max(pad + 1, n_fft - 2 * pad), n_fft - 2 * pad + hop);      // melspec's conditions, and 2 frames
    for (int b = 0; b < B; b++) {
        const int bg = host[2 * b];
        int en = host[2 * b + 1];
        if (p->max_samples > 0 && en - bg > p->max_samples) en = bg + p->max_samples;
        const int m = en - bg;
        frames[b] = m + 2 * pad >= n_fft ? 1 + (m + 2 * pad - n_fft) / hop : 0;
        if (begin) begin[b] = bg;
        if (end) end[b] = en;
        if (frames_out) frames_out[b] = frames[b];
        if (bad < 0 && (m < pad + 1 || frames[b] < 2)) bad = b;
        Mmax = std::max(Mmax, m); Tf = std::max(Tf, frames[b]);
    }
    if (bad >= 0) {
        const int bg = host[2 * bad], en = std::min(host[2 * bad + 1], p->max_samples > 0 ? bg + p->max_samples : INT32_MAX);
        c->sync();
        fail(ZVX_E_INVALID, "zvx_spkemb_wav: row %d is left with samples [%d, %d) of %d at the model's rate: %d, the speaker encoder needs at least %d",
             bad, bg, en, n[bad], en - bg, m_min);
    }
    // 5. everything behind the wait is queued: the window cut, the front end, the encoder, the copy of the result
    c->stage_begin(ZVX_T_SPKEMB);
    const long Npad = ((long)Mmax + 2 * pad + 3) & ~3L;
    int* fr_d = c->upload_ints("mel.frames", frames.data(), B);
    float* padded = c->fbuf("mel.pad", (size_t)B * Npad);
    launch_window_pad(rows, rows_bs, c->ibuf("join.bounds", 0), p->max_samples, padded, Npad, pad, B, (int)Npad, c->stream);
    const float* mel_d = mel_from_padded(c, padded, Npad, fr_d, B, Tf);
    c->tag = "spkemb";
    const float* emb = spkemb_from_mels(c, mel_d, frames.data(), B, Tf);
    c->stage_end(ZVX_T_SPKEMB);
    HIPCHK(hipMemcpyAsync(out, emb, (size_t)B * H * 4, (flags & ZVX_DEVICE_OUT) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!((flags & ZVX_DEVICE_OUT) && (flags & ZVX_NO_SYNC))) c->sync();
}

// ------------------------------------------------------------------------------------------------
// integrated loudness and gain of a batch's waveform rows (include/zvx.h: zvx_loudness, zvx_normalize)
// ------------------------------------------------------------------------------------------------

// The measuring half of zvx_loudness / zvx_normalize / zvx_loudness_stats: the rows on the device, the unit and result buffers, and the
// arguments of launch_loud_units / launch_loud_gates (measure only: the caller of zvx_normalize adds its gain parameters).
// Result words in one block: lufs [B] double, then peak [B], gain [B] float; behind them row_sum / row_cnt.
struct LoudMeasure { LoudArgs a; long units_max; char* res; size_t res_bytes; };
LoudMeasure loud_measure(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, long n_max, int flags) {
    LoudMeasure m{};
    LoudArgs& a = m.a;
    m.res_bytes = (size_t)B * 16;
    a.h = (rate + 5) / 10;
    a.k = loud_coef(c, rate);
    const long units_max = m.units_max = std::max(n_max / a.h, 1L);
    a.upitch = units_max; a.ppitch = (int)((units_max + 63) / 64);
    const DevRows rows = stage_rows(c, "loud", in, nsamples, B, Nmax, flags);
    a.x = rows.x; a.x_bs = Nmax; a.nsamples = rows.len; a.B = B;
    a.unit = (double*)c->buf("loud.unit", (size_t)B * units_max * sizeof(double));
    a.part_peak = c->fbuf("loud.ppeak", (size_t)B * a.ppitch);
    char* res = m.res = (char*)c->buf("loud.res", m.res_bytes + (size_t)B * 16);
    a.lufs = (double*)res; a.peak = (float*)(res + (size_t)B * 8); a.gain = a.peak + B;
    a.row_sum = (double*)(res + m.res_bytes); a.row_cnt = (long*)(res + m.res_bytes + (size_t)B * 8);
    a.abs_gate = pow(10.0, (-70.0 + 0.691) / 10.0);
    a.want_gain = 0;
    return m;
}
void loud_rate_check(const char* who, int rate) {
    if (rate < 4000 || rate > 192000) fail(ZVX_E_INVALID, "%s: rate %d outside [4000, 192000]", who, rate);
}

// zvx_loudness (p == nullptr: measure only) and zvx_normalize
void do_loudness(zvx_ctx* c, const char* who, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_loudness_params* p,
                 void* out, int64_t out_stride, double* lufs, float* peak, float* gain, int flags) {
    const bool norm = p != nullptr;
    const RowsInfo r = rows_check(who, in, nsamples, B, Nmax, 65535);
    loud_rate_check(who, rate);
    flags_check(who, flags, norm ? (ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC | ZVX_PCM16) : ZVX_DEVICE_IN);
    if (norm) {
        out_rows_check(who, in, out, out_stride, Nmax, flags);
        if (!std::isfinite(p->target_lufs) || p->target_lufs < -70.f || p->target_lufs > 0.f) fail(ZVX_E_INVALID, "%s: target_lufs must lie in [-70, 0]", who);
        if (!std::isfinite(p->max_gain_db) || p->max_gain_db < 0.f) fail(ZVX_E_INVALID, "%s: max_gain_db must be finite and not negative", who);
        if (std::isnan(p->peak_ceiling)) fail(ZVX_E_INVALID, "%s: peak_ceiling is NaN", who);
        if (p->mode != ZVX_LOUD_PER_ROW && p->mode != ZVX_LOUD_COMMON) fail(ZVX_E_INVALID, "%s: unknown mode %d", who, p->mode);
    }
    RowsReturn ret(c, B, (size_t)B * 16, lufs || peak || gain, norm, r.n_max, flags);
    LoudMeasure m = loud_measure(c, in, nsamples, B, Nmax, rate, r.n_max, flags);
    LoudArgs& a = m.a;
    a.want_gain = norm ? 1 : 0;
    if (norm) { a.target = (double)p->target_lufs; a.max_gain_db = (double)p->max_gain_db; a.ceiling = (double)p->peak_ceiling; }
    LoudApplyArgs w{};
    w.x = a.x; w.x_bs = Nmax; w.nsamples = a.nsamples; w.B = B; w.gain = a.gain; w.pcm16 = (flags & ZVX_PCM16) ? 1 : 0;
    w.out = ret.out_rows("loud.out", out, out_stride, &w.out_bs);
    TagScope scope(c, "post.loudness");
    c->timed(0.0, 4.0 * r.n_sum + (norm ? (4.0 + (double)ret.ss) * r.n_sum : 0.0), [&] {
        launch_loud_units(a, m.units_max, c->stream);
        launch_loud_gates(a, c->stream);
        if (norm && p->mode == ZVX_LOUD_COMMON) launch_loud_common(a, c->stream);
        if (norm) launch_loud_apply(w, r.n_max, c->stream);
    });
    const char* words = ret.finish(m.res, out, out_stride, nsamples, flags);
    if (!words) return;
    const double* l_h = (const double*)words; const float* p_h = (const float*)(words + (size_t)B * 8); const float* g_h = p_h + B;
    for (int b = 0; b < B; b++) {
        if (lufs) lufs[b] = l_h[b];
        if (peak) peak[b] = p_h[b];
        if (gain) gain[b] = g_h[b];
    }
}

// zvx_loudness_stats: zvx_loudness's two launches, unchanged, then the short-term windows with their gates and the rank selection; the
// result words, the per-row report words and the curves come to pinned host memory behind the call's one wait.
constexpr long LOUD_STATS_MAX_UNITS = 65536;
void run_loudness_stats(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, double* stats, double* momentary,
                        double* short_term, int64_t curve_stride, int flags) {
    const char* who = "zvx_loudness_stats";
    const RowsInfo r = rows_check(who, in, nsamples, B, Nmax, 65535);
    loud_rate_check(who, rate);
    flags_check(who, flags, ZVX_DEVICE_IN);
    if (!stats) fail(ZVX_E_INVALID, "%s: stats is NULL", who);
    const int h = (rate + 5) / 10;
    const bool curves = momentary || short_term;
    if (curves && curve_stride < std::max<int64_t>(1, (int64_t)(Nmax / h) - 3))
        fail(ZVX_E_INVALID, "%s: curve_stride %lld is smaller than max(1, Nmax / h - 3) = %lld", who, (long long)curve_stride,
             (long long)std::max<int64_t>(1, (int64_t)(Nmax / h) - 3));
    for (int b = 0; b < B; b++)
        if (nsamples[b] / h > LOUD_STATS_MAX_UNITS)
            fail(ZVX_E_UNSUPPORTED, "%s: row %d has %d units of %d samples (at most %ld per row)", who, b, nsamples[b] / h, h, LOUD_STATS_MAX_UNITS);
    const long units_max = std::max(r.n_max / h, 1L);
    const long cp = std::max(units_max - 3, 1L), w_max = std::max(units_max - (LOUD_ST_UNITS - 1), 0L);
    // pinned: the result words of zvx_loudness, the report words, then the two curves where asked for
    const size_t words_pad = ((size_t)B * 16 + 255) & ~(size_t)255, rep_bytes = (size_t)B * LOUD_RES_WORDS * sizeof(double);
    const size_t rep_pad = (rep_bytes + 255) & ~(size_t)255, curve_bytes = (size_t)B * cp * sizeof(double);
    char* host = (char*)c->join_pinned(words_pad + rep_pad + (momentary ? curve_bytes : 0) + (short_term ? curve_bytes : 0));
    LoudMeasure m = loud_measure(c, in, nsamples, B, Nmax, rate, r.n_max, flags);
    LoudStatsArgs s{};
    s.unit = m.a.unit; s.upitch = m.a.upitch; s.nsamples = m.a.nsamples; s.B = B; s.h = h; s.abs_gate = m.a.abs_gate;
    s.wpitch = std::max(w_max, 1L); s.cpitch = cp;
    s.win = (double*)c->buf("loud.win", (size_t)B * s.wpitch * sizeof(double));
    s.mom = momentary ? (double*)c->buf("loud.mom", curve_bytes) : nullptr;
    s.sht = short_term ? (double*)c->buf("loud.sht", curve_bytes) : nullptr;
    s.res = (double*)c->buf("loud.rep", rep_bytes);
    TagScope scope(c, "post.loudness");
    c->timed(0.0, 4.0 * r.n_sum, [&] {
        launch_loud_units(m.a, m.units_max, c->stream);
        launch_loud_gates(m.a, c->stream);
        launch_loud_windows(s, c->stream);
        launch_loud_rank(s, w_max, c->stream);
    });
    char* mom_h = host + words_pad + rep_pad; char* sht_h = mom_h + (momentary ? curve_bytes : 0);
    HIPCHK(hipMemcpyAsync(host, m.res, (size_t)B * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(host + words_pad, s.res, rep_bytes, hipMemcpyDeviceToHost, c->stream));
    if (momentary) HIPCHK(hipMemcpyAsync(mom_h, s.mom, curve_bytes, hipMemcpyDeviceToHost, c->stream));
    if (short_term) HIPCHK(hipMemcpyAsync(sht_h, s.sht, curve_bytes, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                               // the call's one wait
    const double* l_h = (const double*)host; const float* p_h = (const float*)(host + (size_t)B * 8);
    const double* rep = (const double*)(host + words_pad);
    auto lu = [](double p) { return p > 0.0 ? -0.691 + 10.0 * log10(p) : -INFINITY; };
    for (int b = 0; b < B; b++) {
        const double* w = rep + (size_t)b * LOUD_RES_WORDS;
        double* o = stats + (size_t)b * ZVX_LS_COUNT;
        const bool any = w[LOUD_RES_GATED] > 0.0;
        o[ZVX_LS_INTEGRATED] = l_h[b]; o[ZVX_LS_PEAK] = (double)p_h[b];
        o[ZVX_LS_MOMENTARY_MAX] = w[LOUD_RES_MOM_MAX]; o[ZVX_LS_SHORT_MAX] = w[LOUD_RES_SHORT_MAX];
        o[ZVX_LS_LRA] = any ? 10.0 * log10(w[LOUD_RES_POW_HI] / w[LOUD_RES_POW_LO]) : 0.0;
        o[ZVX_LS_LRA_LOW] = any ? lu(w[LOUD_RES_POW_LO]) : -INFINITY; o[ZVX_LS_LRA_HIGH] = any ? lu(w[LOUD_RES_POW_HI]) : -INFINITY;
        o[ZVX_LS_SHORT_GATED] = w[LOUD_RES_GATED];
        const long U = nsamples[b] / h;
        if (momentary && U >= 4) memcpy(momentary + (size_t)b * curve_stride, mom_h + (size_t)b * cp * sizeof(double), (size_t)(U - 3) * sizeof(double));
        if (short_term && U >= LOUD_ST_UNITS)
            memcpy(short_term + (size_t)b * curve_stride, sht_h + (size_t)b * cp * sizeof(double), (size_t)(U - (LOUD_ST_UNITS - 1)) * sizeof(double));
    }
}

// ------------------------------------------------------------------------------------------------
// pitch report (include/zvx.h: zvx_pitch): every check, then the row table, three launches, and the result words and curves to pinned
// host memory behind the call's one wait
// ------------------------------------------------------------------------------------------------
constexpr long PITCH_MAX_FRAMES = 65536;
void do_pitch(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_pitch_params* p, float* f0, float* aper,
              int64_t f_stride, int32_t* frames, double* stats, int flags) {
    const char* who = "zvx_pitch";
    const RowsInfo r = rows_check(who, in, nsamples, B, Nmax, 65535);
    loud_rate_check(who, rate);
    flags_check(who, flags, ZVX_DEVICE_IN);
    if (!p) fail(ZVX_E_INVALID, "%s: params is NULL", who);
    if (!stats) fail(ZVX_E_INVALID, "%s: stats is NULL", who);
    if (!std::isfinite(p->fmin) || !std::isfinite(p->fmax) || !(p->fmin > 0.f) || !(p->fmin < p->fmax))
        fail(ZVX_E_INVALID, "%s: fmin %g / fmax %g must be finite with 0 < fmin < fmax", who, (double)p->fmin, (double)p->fmax);
    if (!std::isfinite(p->threshold) || !(p->threshold > 0.f) || p->threshold > 1.f)
        fail(ZVX_E_INVALID, "%s: threshold %g must lie in (0, 1]", who, (double)p->threshold);
    if (!std::isfinite(p->gate_db) || p->gate_db > 0.f) fail(ZVX_E_INVALID, "%s: gate_db %g must be finite and not positive", who, (double)p->gate_db);
    if (p->window < 2) fail(ZVX_E_INVALID, "%s: window %d must be at least 2", who, p->window);
    if (p->hop < 1) fail(ZVX_E_INVALID, "%s: hop %d must be at least 1", who, p->hop);
    const double fs = (double)rate;
    const double tmin_d = std::max(2.0, floor(fs / (double)p->fmax)), tmax_d = ceil(fs / (double)p->fmin);
    if (tmax_d < tmin_d + 2.0)
        fail(ZVX_E_INVALID, "%s: fmin %g / fmax %g at %d Hz give tau_max %.0f < tau_min %.0f + 2", who, (double)p->fmin, (double)p->fmax, rate, tmax_d, tmin_d);
    const int W = p->window, H = p->hop;
    const bool curves = f0 || aper;
    if (curves && f_stride < std::max<int64_t>(1, Nmax / H))
        fail(ZVX_E_INVALID, "%s: f_stride %lld is smaller than max(1, Nmax / hop) = %lld", who, (long long)f_stride, (long long)std::max<int64_t>(1, Nmax / H));
    if (W > PITCH_MAX_W) fail(ZVX_E_UNSUPPORTED, "%s: window %d (at most %d)", who, W, PITCH_MAX_W);
    if (tmax_d > (double)PITCH_MAX_TAU) fail(ZVX_E_UNSUPPORTED, "%s: fmin %g at %d Hz gives tau_max %.0f (at most %d)", who, (double)p->fmin, rate, tmax_d, PITCH_MAX_TAU);
    for (int b = 0; b < B; b++)
        if (nsamples[b] / H > PITCH_MAX_FRAMES)
            fail(ZVX_E_UNSUPPORTED, "%s: row %d has %d frames of %d samples (at most %ld per row)", who, b, nsamples[b] / H, H, PITCH_MAX_FRAMES);
    PitchArgs a{};
    a.B = B; a.W = W; a.H = H; a.tau_min = (int)tmin_d; a.tau_max = (int)tmax_d; a.c = (W + a.tau_max) / 2;
    a.fs = fs; a.threshold = (double)p->threshold; a.gate = pow(10.0, (double)p->gate_db / 10.0);
    const long reach = (long)W + a.tau_max;
    a.G = (int)std::max(1L, std::min<long>(PITCH_MAX_G, (PITCH_SPAN - reach) / H + 1));
    a.span = (int)((long)(a.G - 1) * H + reach);
    const long f_max = r.n_max / H, fpitch = std::max(f_max, 1L);
    if (!launch_pitch_track(a, f_max, c->stream, true))       // (the last check: the LDS opt-in, before anything is allocated or queued)
        fail(ZVX_E_UNSUPPORTED, "%s: window %d / tau_max %d do not fit the kernel's LDS plan", who, W, a.tau_max);
    // pinned: the result words, then the two curves where asked for
    const size_t res_bytes = (size_t)B * PITCH_RES_WORDS * sizeof(double), res_pad = (res_bytes + 255) & ~(size_t)255;
    const size_t curve_bytes = (size_t)B * fpitch * sizeof(float);
    char* host = (char*)c->join_pinned(res_pad + (f0 ? curve_bytes : 0) + (aper ? curve_bytes : 0));
    const float* x = rows_to_device(c, "pitch", in, B, Nmax, flags);
    float* f0_d = c->fbuf("pitch.f0", (size_t)2 * B * fpitch);
    float* ap_d = f0_d + (size_t)B * fpitch;
    a.res = (double*)c->buf("pitch.res", res_bytes);
    std::vector<PitchRow> tab((size_t)B);
    for (int b = 0; b < B; b++)
        tab[(size_t)b] = PitchRow{x + (size_t)b * Nmax, f0_d + (size_t)b * fpitch, ap_d + (size_t)b * fpitch, nsamples[b], nsamples[b] / H};
    PitchRow* tab_d = (PitchRow*)c->buf("pitch.rows", (size_t)B * sizeof(PitchRow));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(PitchRow));
    a.rows = tab_d;
    TagScope scope(c, "post.pitch");
    c->timed(0.0, 4.0 * r.n_sum, [&] {
        if (!launch_pitch_track(a, f_max, c->stream)) fail(ZVX_E_UNSUPPORTED, "%s: window %d / tau_max %d do not fit the kernel's LDS plan", who, W, a.tau_max);
        launch_pitch_stats(a, c->stream);
        launch_pitch_rank(a, f_max, c->stream);
    });
    char* f0_h = host + res_pad; char* ap_h = f0_h + (f0 ? curve_bytes : 0);
    HIPCHK(hipMemcpyAsync(host, a.res, res_bytes, hipMemcpyDeviceToHost, c->stream));
    if (f0 && f_max > 0) HIPCHK(hipMemcpyAsync(f0_h, f0_d, curve_bytes, hipMemcpyDeviceToHost, c->stream));
    if (aper && f_max > 0) HIPCHK(hipMemcpyAsync(ap_h, ap_d, curve_bytes, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                               // the call's one wait
    const double* rep = (const double*)host;
    for (int b = 0; b < B; b++) {
        const double* w = rep + (size_t)b * PITCH_RES_WORDS;
        double* o = stats + (size_t)b * ZVX_PS_COUNT;
        const int F = nsamples[b] / H;
        o[ZVX_PS_FRAMES] = (double)F; o[ZVX_PS_VOICED] = w[PITCH_RES_VOICED];
        o[ZVX_PS_MEDIAN] = w[PITCH_RES_MED]; o[ZVX_PS_LOW] = w[PITCH_RES_LO]; o[ZVX_PS_HIGH] = w[PITCH_RES_HI]; o[ZVX_PS_MEAN] = w[PITCH_RES_MEAN];
        if (frames) frames[b] = F;
        if (f0 && F > 0) memcpy(f0 + (size_t)b * f_stride, f0_h + (size_t)b * fpitch * sizeof(float), (size_t)F * sizeof(float));
        if (aper && F > 0) memcpy(aper + (size_t)b * f_stride, ap_h + (size_t)b * fpitch * sizeof(float), (size_t)F * sizeof(float));
    }
}

// The analysis zvx_watermark_detect and zvx_watermark_identify share: every row's frames into band differences d [F][J - 2], searched in
// windows of WF frames; the window results are [B][NWp][K] scores and as many offsets, K = 1 for the detector.  wm_analysis is pure (an
// entry point plans among its checks); wm_analysis_fill sets the launch arguments' geometry, table and band fields; wm_analysis_rows
// takes "wm.d", the caller's result buffer and "wm.rows", in the order the entry points always took them, and uploads the row table.
struct WmAnalysis {
    std::vector<WmDetectRow> tab; std::vector<size_t> d_at;
    int WF = 0, NW = 0, NWp = 1; long Fmax = 0; double frames = 0; size_t d_floats = 0;
    int windows(int b) const { return wm_windows(tab[(size_t)b].F, WF); }
    size_t res_pad(int K) const { return (tab.size() * NWp * K * 4 + 255) & ~(size_t)255; }      // scores or offsets, padded in the pinned block
};
WmAnalysis wm_analysis(const WmPlan& wp, const int32_t* nsamples, int B, int window_frames) {
    WmAnalysis an;
    an.WF = window_frames; an.tab.resize((size_t)B); an.d_at.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const int F = dn_frames(wp.g, nsamples[b]);
        an.tab[(size_t)b] = WmDetectRow{nullptr, nullptr, nsamples[b], F};
        an.d_at[(size_t)b] = an.d_floats; an.d_floats += (size_t)F * (wp.J - 2);
        an.NW = std::max(an.NW, an.windows(b)); an.Fmax = std::max<long>(an.Fmax, F); an.frames += F;
    }
    an.NWp = std::max(an.NW, 1);
    return an;
}
void wm_analysis_fill(zvx_ctx* c, const WmPlan& wp, const zvx_watermark_params* p, const WmAnalysis& an, WmDetectArgs& a) {
    const DnGeom& g = wp.g;
    const zvx_ctx::DnTables& tb = dn_tables(c, g);
    a.B = (int)an.tab.size(); a.n_fft = g.n_fft; a.log2n = g.log2n; a.hop = g.hop; a.pad = g.pad; a.Fmax = (int)an.Fmax;
    a.twid = tb.twid; a.win = tb.win;
    a.k_lo = wp.k_lo; a.KB = p->band_bins; a.J = wp.J; a.TB = p->block_frames; a.P = p->period_blocks;
    a.WF = an.WF; a.NW = an.NWp;
}
// -> the device results in the caller's buffer `res_name`: res_pad bytes of window scores, then as many of window offsets
char* wm_analysis_rows(zvx_ctx* c, WmAnalysis& an, const float* x, int Nmax, const char* res_name, size_t res_pad, WmDetectArgs& a) {
    const int B = (int)an.tab.size();
    float* d = c->fbuf("wm.d", std::max<size_t>(an.d_floats, 1));
    char* res = (char*)c->buf(res_name, 2 * res_pad);
    a.win_score = (float*)res; a.win_offset = (int*)(res + res_pad);
    for (int b = 0; b < B; b++) { an.tab[(size_t)b].x = x + (size_t)b * Nmax; an.tab[(size_t)b].d = d + an.d_at[(size_t)b]; }
    WmDetectRow* tab_d = (WmDetectRow*)c->buf("wm.rows", (size_t)B * sizeof(WmDetectRow));
    c->upload(tab_d, an.tab.data(), (size_t)B * sizeof(WmDetectRow));
    a.rows = tab_d;
    return res;
}
// the best window of row b under key k (the first of equals; a row without windows: 0 at offset 0, window 0)
struct WmBest { float score = 0.f; int32_t offset = 0, window = 0; };
WmBest wm_best_window(const WmAnalysis& an, const float* hs, const int32_t* ho, int b, int K, int k) {
    WmBest r;
    for (int w = 0, nw = an.windows(b); w < nw; w++) {
        const size_t at = ((size_t)b * an.NWp + w) * K + k;
        if (w == 0 || hs[at] > r.score) { r.score = hs[at]; r.offset = ho[at]; r.window = w; }
    }
    return r;
}

// zvx_watermark_detect: every check before anything is allocated, uploaded or queued; the call's one wait brings every window's result over
void do_watermark_detect(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* p, int window_frames,
                         float* score, int32_t* offset, int32_t* window, float* win_score, int32_t* win_offset, int NWmax, int flags) {
    const char* who = "zvx_watermark_detect";
    const RowsInfo ri = rows_check(who, in, nsamples, B, Nmax, 65535);
    flags_check(who, flags, ZVX_DEVICE_IN);
    const WmPlan wp = watermark_params_check(c, who, p);
    const DnGeom& g = wp.g;
    if (!score || !offset || !window) fail(ZVX_E_INVALID, "%s: score, offset or window is NULL", who);
    if (window_frames < 0 || window_frames == 1) fail(ZVX_E_INVALID, "%s: window_frames %d (0: the row; otherwise at least 2)", who, window_frames);
    if (!win_score != !win_offset) fail(ZVX_E_INVALID, "%s: win_score and win_offset go together (one of them is NULL)", who);
    if (NWmax < 0) fail(ZVX_E_INVALID, "%s: NWmax %d is negative", who, NWmax);
    for (int b = 0; b < B; b++) {
        stft_len_check(who, g, b, nsamples[b]);
        const int nw = wm_windows(dn_frames(g, nsamples[b]), window_frames);
        if (win_score && nw > NWmax) fail(ZVX_E_BUFFER, "%s: row %d has %d windows, NWmax is %d", who, b, nw, NWmax);
    }
    WmAnalysis an = wm_analysis(wp, nsamples, B, window_frames);
    const size_t res_pad = an.res_pad(1);
    char* host = (char*)c->join_pinned(2 * res_pad);
    const float* x = rows_to_device(c, "wm", in, B, Nmax, flags);
    WmDetectArgs a{};
    wm_analysis_fill(c, wp, p, an, a);
    a.sign = wm_sign_table(c, p, wp.J);
    const char* res = wm_analysis_rows(c, an, x, Nmax, "wm.res", res_pad, a);
    {
        TagScope scope(c, "post.wmdetect");
        c->timed(dn_fft_flops(g, an.frames, 1), 4.0 * ri.n_sum + 8.0 * an.frames * (wp.J - 2), [&] {
            launch_wm_bands(a, c->stream);
            if (an.NW > 0) launch_wm_search(a, c->stream);
        });
    }
    if (an.NW > 0) HIPCHK(hipMemcpyAsync(host, res, 2 * res_pad, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                               // the call's one wait
    const float* hs = (const float*)host;
    const int32_t* ho = (const int32_t*)(host + res_pad);
    for (int b = 0; b < B; b++) {
        const WmBest r = wm_best_window(an, hs, ho, b, 1, 0);
        score[b] = r.score; offset[b] = r.offset; window[b] = r.window;
        for (int w = 0; win_score && w < an.windows(b); w++) {
            win_score[(size_t)b * NWmax + w] = hs[(size_t)b * an.NWp + w]; win_offset[(size_t)b * NWmax + w] = ho[(size_t)b * an.NWp + w];
        }
    }
}

// zvx_watermark_identify: zvx_watermark_detect's analysis once, the search with K keys' tables built on the device; every check before anything
// is allocated, uploaded or queued; the call's one wait brings the [B][NW][K] window results over, and the best over a row's windows (the
// first of equals, as the detector's) and over the keys is taken here
constexpr long WM_IDENTIFY_TABLE_BYTES = 1L << 26;           // K P J signs at most (include/zvx.h); they are stored a bit each
constexpr int WM_IDENTIFY_MAX_KEYS = 1 << 16;
void do_watermark_identify(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* p, const uint64_t* keys,
                           int K, int window_frames, float* score, int32_t* offset, int32_t* window, int32_t* best, int flags) {
    const char* who = "zvx_watermark_identify";
    const RowsInfo ri = rows_check(who, in, nsamples, B, Nmax, 65535);
    flags_check(who, flags, ZVX_DEVICE_IN);
    const WmPlan wp = watermark_params_check(c, who, p);
    const DnGeom& g = wp.g;
    if (!keys) fail(ZVX_E_INVALID, "%s: keys is NULL", who);
    if (!score || !offset || !window || !best) fail(ZVX_E_INVALID, "%s: score, offset, window or best is NULL", who);
    if (K < 1) fail(ZVX_E_INVALID, "%s: K %d must be at least 1", who, K);
    if (window_frames < 0 || window_frames == 1) fail(ZVX_E_INVALID, "%s: window_frames %d (0: the row; otherwise at least 2)", who, window_frames);
    const int P = p->period_blocks, J = wp.J;
    for (int b = 0; b < B; b++) stft_len_check(who, g, b, nsamples[b]);
    if ((long)K * P * J > WM_IDENTIFY_TABLE_BYTES)
        fail(ZVX_E_UNSUPPORTED, "%s: K P J = %d x %d x %d = %lld signs in the tables (at most %ld)", who, K, P, J, (long long)K * P * J, WM_IDENTIFY_TABLE_BYTES);
    if (K > WM_IDENTIFY_MAX_KEYS) fail(ZVX_E_UNSUPPORTED, "%s: K %d (at most %d keys a call)", who, K, WM_IDENTIFY_MAX_KEYS);
    WmAnalysis an = wm_analysis(wp, nsamples, B, window_frames);
    const size_t res_pad = an.res_pad(K);
    char* host = (char*)c->join_pinned(2 * res_pad);
    const float* x = rows_to_device(c, "wm", in, B, Nmax, flags);
    WmKeysArgs ka{};
    WmDetectArgs& a = ka.d;
    wm_analysis_fill(c, wp, p, an, a);
    ka.K = K;
    unsigned long long* keys_d = (unsigned long long*)c->buf("wm.keys", (size_t)K * 8);
    unsigned* signs_d = (unsigned*)c->buf("wm.signbits", (size_t)K * P * wm_sign_words(J) * sizeof(unsigned));      // packed: 32 signs a word
    ka.sign_bits = signs_d;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "keys are uploaded as they are");
    c->upload(keys_d, keys, (size_t)K * 8);
    const char* res = wm_analysis_rows(c, an, x, Nmax, "wm.kres", res_pad, a);
    {
        TagScope scope(c, "post.wmidentify");
        c->timed(dn_fft_flops(g, an.frames, 1), 4.0 * ri.n_sum + 8.0 * an.frames * (J - 2) + 4.0 * K * P * wm_sign_words(J), [&] {
            launch_wm_signs(keys_d, signs_d, K, P, J, true, c->stream);
            launch_wm_bands(a, c->stream);
            if (an.NW > 0) launch_wm_search_keys(ka, c->stream);
        });
    }
    if (an.NW > 0) HIPCHK(hipMemcpyAsync(host, res, 2 * res_pad, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                               // the call's one wait
    const float* hs = (const float*)host;
    const int32_t* ho = (const int32_t*)(host + res_pad);
    for (int b = 0; b < B; b++) {
        int32_t kb = 0;
        for (int k = 0; k < K; k++) {
            const WmBest r = wm_best_window(an, hs, ho, b, K, k);
            score[(size_t)b * K + k] = r.score; offset[(size_t)b * K + k] = r.offset; window[(size_t)b * K + k] = r.window;
            if (r.score > score[(size_t)b * K + kb]) kb = k;
        }
        best[b] = kb;
    }
}

// ------------------------------------------------------------------------------------------------
// voice matching (include/zvx.h: zvx_spk_score, zvx_spk_topk; voicematch.hip): every check before anything is allocated, uploaded or
// queued.  topk false: the score form (top and index are not read).
// ------------------------------------------------------------------------------------------------
void do_spk_match(zvx_ctx* c, const char* who, const float* query, int B, const float* lib, int64_t K, int dim, int top, float* score, int32_t* index,
                  int flags, bool topk) {
    flags_check(who, flags, ZVX_DEVICE_IN | ZVX_DEVICE_OUT | ZVX_NO_SYNC);
    if (!query) fail(ZVX_E_INVALID, "%s: query is NULL", who);
    if (!lib) fail(ZVX_E_INVALID, "%s: lib is NULL", who);
    if (!score) fail(ZVX_E_INVALID, "%s: score is NULL", who);
    if (topk && !index) fail(ZVX_E_INVALID, "%s: index is NULL", who);
    if (B <= 0) fail(ZVX_E_INVALID, "%s: B = %d must be positive", who, B);
    if (K <= 0 || K > (int64_t)INT32_MAX) fail(ZVX_E_INVALID, "%s: K = %lld must lie in [1, 2^31 - 1]", who, (long long)K);
    if (dim < 4 || dim > SPK_DIM_MAX || dim % 4) fail(ZVX_E_INVALID, "%s: dim %d must be a multiple of 4 in [4, %d]", who, dim, SPK_DIM_MAX);
    if (topk && (top < 1 || top > ZVX_SPK_TOP_MAX || top > K))
        fail(ZVX_E_INVALID, "%s: top %d must lie in [1, min(K, %d)] (K = %lld)", who, top, ZVX_SPK_TOP_MAX, (long long)K);
    if ((uintptr_t)lib & 15) fail(ZVX_E_INVALID, "%s: lib %p is not aligned to 16 bytes", who, (const void*)lib);
    if (B > 65535) fail(ZVX_E_UNSUPPORTED, "%s: B = %d queries (at most 65535 per call)", who, B);
    static_assert(ZVX_SPK_TOP_MAX == SPK_TOP_MAX, "the header's cap is the kernels'");
    SpkArgs a{};
    a.K = (long)K; a.B = B; a.dim = dim; a.top = topk ? top : 0;
    if (!launch_spk_match(a, c->stream, true)) fail(ZVX_E_UNSUPPORTED, "%s: the device refuses the kernel's LDS plan", who);
    const bool dev_out = flags & ZVX_DEVICE_OUT;
    const long nslab = spk_slabs(a.K);
    const size_t n_out = (size_t)B * (topk ? (size_t)top : (size_t)K);
    char* host = topk && !dev_out ? (char*)c->join_pinned(2 * n_out * 4) : nullptr;
    a.q = rows_to_device(c, "spk", query, B, dim, flags);
    a.lib = lib;
    float* out_s = dev_out ? score : c->fbuf(topk ? "spk.top_s" : "spk.score", n_out);
    int* out_i = !topk ? nullptr : dev_out ? (int*)index : (int*)c->buf("spk.top_i", n_out * 4);
    if (topk) {
        a.cand_s = c->fbuf("spk.cand_s", (size_t)B * nslab * top);
        a.cand_i = (int*)c->buf("spk.cand_i", (size_t)B * nslab * top * 4);
    } else a.score = out_s;
    {
        TagScope scope(c, "spk.match");
        const double groups = (double)((B + spk_group(dim, a.top) - 1) / spk_group(dim, a.top));
        c->timed(2.0 * B * (double)K * dim, 4.0 * groups * (double)K * dim + (topk ? 0.0 : 4.0 * B * (double)K), [&] {
            launch_spk_match(a, c->stream);
            if (topk) launch_spk_merge(a.cand_s, a.cand_i, B, nslab, top, out_s, out_i, c->stream);
        });
    }
    if (dev_out) {
        if (!(flags & ZVX_NO_SYNC)) c->sync();
        return;
    }
    if (topk) {
        HIPCHK(hipMemcpyAsync(host, out_s, n_out * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(host + n_out * 4, out_i, n_out * 4, hipMemcpyDeviceToHost, c->stream));
        c->sync();                                           // the call's one wait
        memcpy(score, host, n_out * 4); memcpy(index, host + n_out * 4, n_out * 4);
    } else {
        HIPCHK(hipMemcpyAsync(score, out_s, n_out * 4, hipMemcpyDeviceToHost, c->stream));     // (B x K may be large: straight to the caller)
        c->sync();
    }
}

// ------------------------------------------------------------------------------------------------
// alignment (include/zvx.h: zvx_dtw, zvx_align_wav; align.hip).  dtw_check holds every check of the lengths and is pure; dtw_run works on
// device rows, queues the two launches and delivers the host outputs behind the call's one wait.
// ------------------------------------------------------------------------------------------------
struct DtwPlan { long cells = 0, pcells = 0, rows = 0; int ta_max = 0, p_max = 0; double row_bytes = 0; };
DtwPlan dtw_check(const char* who, const int32_t* Ta, int Tamax, const int32_t* Tb, int Tbmax, int B, int dim, bool want_path, int64_t path_stride) {
    if (B < 1) fail(ZVX_E_INVALID, "%s: B = %d must be positive", who, B);
    if (dim < 1) fail(ZVX_E_INVALID, "%s: dim = %d must be positive", who, dim);
    DtwPlan pl;
    for (int b = 0; b < B; b++) {
        if (Ta[b] < 1 || Ta[b] > Tamax) fail(ZVX_E_INVALID, "%s: pair %d: Ta = %d out of range (1..%d)", who, b, Ta[b], Tamax);
        if (Tb[b] < 1 || Tb[b] > Tbmax) fail(ZVX_E_INVALID, "%s: pair %d: Tb = %d out of range (1..%d)", who, b, Tb[b], Tbmax);
        pl.p_max = std::max<long>(pl.p_max, std::min<long>((long)Ta[b] + Tb[b] - 1, INT32_MAX));
    }
    if (want_path && path_stride < pl.p_max)
        fail(ZVX_E_INVALID, "%s: path_stride %lld is smaller than the longest possible path, %d cells", who, (long long)path_stride, pl.p_max);
    if (dim > DTW_MAX_DIM) fail(ZVX_E_UNSUPPORTED, "%s: dim = %d (at most %d)", who, dim, DTW_MAX_DIM);
    for (int b = 0; b < B; b++)
        if (Ta[b] > DTW_MAX_T || Tb[b] > DTW_MAX_T)
            fail(ZVX_E_UNSUPPORTED, "%s: pair %d has %d x %d frames (at most %d a side)", who, b, Ta[b], Tb[b], DTW_MAX_T);
    if (B > 65535) fail(ZVX_E_UNSUPPORTED, "%s: B = %d pairs (at most 65535 per call)", who, B);
    for (int b = 0; b < B; b++) {
        pl.cells += (long)Ta[b] * Tb[b]; pl.pcells += Ta[b] + Tb[b] - 1; pl.rows += Ta[b];
        pl.ta_max = std::max(pl.ta_max, (int)Ta[b]);
        pl.row_bytes += 4.0 * dim * ((double)Ta[b] + Tb[b]);
        if (pl.cells > (1L << 30)) fail(ZVX_E_UNSUPPORTED, "%s: more than 2^30 cells in the call (reached at pair %d)", who, b);
    }
    return pl;
}
void dtw_run(zvx_ctx* c, const DtwPlan& pl, const float* a_d, const int32_t* Ta, int Tamax, const float* b_d, const int32_t* Tb, int Tbmax, int B, int dim,
             double* cost, int32_t* path_len, int32_t* path, int64_t path_stride, int32_t* a2b, int64_t a2b_stride) {
    const size_t cost_b = ((size_t)B * 8 + 255) & ~(size_t)255, len_b = ((size_t)B * 4 + 255) & ~(size_t)255;
    const size_t path_b = (size_t)pl.pcells * 8, a2b_b = (size_t)pl.rows * 8;
    char* host = (char*)c->join_pinned(cost_b + len_b + (path ? path_b : 0) + (a2b ? a2b_b : 0));
    DtwArgs g{};
    g.B = B; g.dim = dim; g.lanes = dtw_lanes(dim, pl.ta_max);
    g.dir = (unsigned char*)c->buf("al.dir", (size_t)pl.cells);
    g.cost = (double*)c->buf("al.cost", (size_t)B * 8);
    g.path_len = (int*)c->buf("al.len", (size_t)B * 4);
    g.rev = (int*)c->buf("al.rev", path_b);
    g.path = (int*)c->buf("al.path", path_b);
    g.a2b = (int*)c->buf("al.a2b", a2b_b);
    std::vector<DtwPair> tab((size_t)B);
    long d_off = 0, p_off = 0, r_off = 0;
    for (int b = 0; b < B; b++) {
        tab[(size_t)b] = DtwPair{a_d + (size_t)b * Tamax * dim, b_d + (size_t)b * Tbmax * dim, Ta[b], Tb[b], d_off, p_off, r_off};
        d_off += (long)Ta[b] * Tb[b]; p_off += Ta[b] + Tb[b] - 1; r_off += Ta[b];
    }
    DtwPair* tab_d = (DtwPair*)c->buf("al.pairs", (size_t)B * sizeof(DtwPair));
    c->upload(tab_d, tab.data(), (size_t)B * sizeof(DtwPair));
    g.pairs = tab_d;
    {
        TagScope scope(c, "post.align");
        // one group per call under "post.align"; inside it each launch is a group of its own under a tag of its own (tools/align_bench.py)
        c->timed(0.0, pl.row_bytes + (double)pl.cells, [&] {
            { TagScope fwd(c, "post.align.forward"); c->timed(0.0, pl.row_bytes + (double)pl.cells, [&] { launch_dtw_forward(g, c->stream); }); }
            { TagScope back(c, "post.align.backtrack"); c->timed(0.0, (double)pl.cells, [&] { launch_dtw_backtrack(g, c->stream); }); }
        });
    }
    char* len_h = host + cost_b; char* path_h = len_h + len_b; char* a2b_h = path_h + (path ? path_b : 0);
    HIPCHK(hipMemcpyAsync(host, g.cost, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(len_h, g.path_len, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    if (path) HIPCHK(hipMemcpyAsync(path_h, g.path, path_b, hipMemcpyDeviceToHost, c->stream));
    if (a2b) HIPCHK(hipMemcpyAsync(a2b_h, g.a2b, a2b_b, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                               // the call's one wait
    memcpy(cost, host, (size_t)B * 8);
    memcpy(path_len, len_h, (size_t)B * 4);
    for (int b = 0; b < B; b++) {
        const DtwPair& p = tab[(size_t)b];
        if (path) memcpy(path + (size_t)b * path_stride * 2, path_h + (size_t)p.path_off * 8, (size_t)path_len[b] * 8);
        if (a2b) memcpy(a2b + (size_t)b * a2b_stride * 2, a2b_h + (size_t)p.a2b_off * 8, (size_t)p.Ta * 8);
    }
}
void do_dtw(zvx_ctx* c, const float* a, const int32_t* Ta, int Tamax, const float* b, const int32_t* Tb, int Tbmax, int B, int dim,
            const zvx_dtw_params* params, double* cost, int32_t* path_len, int32_t* path, int64_t path_stride, int32_t* a2b, int flags) {
    const char* who = "zvx_dtw";
    if (!a || !b || !Ta || !Tb) fail(ZVX_E_INVALID, "%s: a, b, Ta or Tb is NULL", who);
    if (!cost || !path_len) fail(ZVX_E_INVALID, "%s: cost or path_len is NULL", who);
    flags_check(who, flags, ZVX_DEVICE_IN);
    if (params) for (int k = 0; k < 4; k++) if (params->reserved[k]) fail(ZVX_E_INVALID, "%s: params->reserved[%d] is %d (must be 0)", who, k, params->reserved[k]);
    const DtwPlan pl = dtw_check(who, Ta, Tamax, Tb, Tbmax, B, dim, path != nullptr, path_stride);
    const float* a_d = a;
    const float* b_d = b;
    if (!(flags & ZVX_DEVICE_IN)) {
        const size_t na = (size_t)B * Tamax * dim, nb = (size_t)B * Tbmax * dim;
        float* ad = c->fbuf("al.a", na);
        float* bd = c->fbuf("al.b", nb);
        HIPCHK(hipMemcpyAsync(ad, a, na * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(bd, b, nb * 4, hipMemcpyHostToDevice, c->stream));
        a_d = ad; b_d = bd;
    }
    dtw_run(c, pl, a_d, Ta, Tamax, b_d, Tb, Tbmax, B, dim, cost, path_len, path, path_stride, a2b, Tamax);
}
void do_align_wav(zvx_ctx* c, const float* wav_a, const int32_t* n_a, int Nmax_a, const float* wav_b, const int32_t* n_b, int Nmax_b, int B,
                  const zvx_align_params* params, double* stats, int32_t* path, int64_t path_stride, int32_t* a2b, int64_t a2b_stride, float* cep_a,
                  float* cep_b, int64_t cep_stride, int flags) {
    const char* who = "zvx_align_wav";
    if (!wav_a || !wav_b || !n_a || !n_b || B <= 0 || Nmax_a <= 0 || Nmax_b <= 0)
        fail(ZVX_E_INVALID, "%s: bad arguments (NULL pointer, B = %d, Nmax_a = %d, Nmax_b = %d)", who, B, Nmax_a, Nmax_b);
    if (!params) fail(ZVX_E_INVALID, "%s: params is NULL", who);
    if (!stats) fail(ZVX_E_INVALID, "%s: stats is NULL", who);
    flags_check(who, flags, ZVX_DEVICE_IN);
    const int nm = c->n_mels, K = params->n_cep;
    if (K < 1 || K > std::min(DTW_MAX_DIM, nm - 1)) fail(ZVX_E_INVALID, "%s: n_cep %d must lie in [1, %d]", who, K, std::min(DTW_MAX_DIM, nm - 1));
    for (int k = 0; k < 3; k++) if (params->reserved[k]) fail(ZVX_E_INVALID, "%s: params->reserved[%d] is %d (must be 0)", who, k, params->reserved[k]);
    std::vector<int> fa, fb;
    int bl = 0;
    const int Tfa = melspec_frames(c, who, "a", n_a, B, Nmax_a, fa, &bl);
    const int Tfb = melspec_frames(c, who, "b", n_b, B, Nmax_b, fb, &bl);
    if (a2b && a2b_stride < Tfa) fail(ZVX_E_INVALID, "%s: a2b_stride %lld is smaller than the %d frames of the longest row of a", who, (long long)a2b_stride, Tfa);
    if ((cep_a || cep_b) && cep_stride < std::max(Tfa, Tfb))
        fail(ZVX_E_INVALID, "%s: cep_stride %lld is smaller than the %d frames of the longest row", who, (long long)cep_stride, std::max(Tfa, Tfb));
    const DtwPlan pl = dtw_check(who, fa.data(), Tfa, fb.data(), Tfb, B, K, path != nullptr, path_stride);
    // the cosine table, in double on the host: table[k - 1][m] = cos(pi k (m + 1/2) / M)
    std::vector<double> tab((size_t)K * nm);
    for (int k = 1; k <= K; k++) for (int m = 0; m < nm; m++) tab[(size_t)(k - 1) * nm + m] = cos(M_PI * (double)k * ((double)m + 0.5) / (double)nm);
    double* tab_d = (double*)c->buf("al.dct", tab.size() * 8);
    c->upload(tab_d, tab.data(), tab.size() * 8);
    const double scale = sqrt(2.0 / (double)nm);
    float* cep[2] = {c->fbuf("al.cep_a", (size_t)B * Tfa * K), c->fbuf("al.cep_b", (size_t)B * Tfb * K)};
    {
        TagScope scope(c, "post.align.mel");
        for (int side = 0; side < 2; side++) {
            int* fr_d = nullptr;
            const int Tf = side ? Tfb : Tfa;
            const float* mel_d = melspec_queue(c, side ? wav_b : wav_a, side ? n_b : n_a, side ? fb : fa, B, side ? Nmax_b : Nmax_a, Tf,
                                               (flags & ZVX_DEVICE_IN) != 0, &fr_d);
            c->timed(2.0 * B * (double)Tf * nm * K, 4.0 * B * (double)Tf * (nm + K), [&] { launch_cepstra(mel_d, Tf, fr_d, B, nm, K, tab_d, scale, cep[side], c->stream); });
        }
    }
    if (cep_a) copy_out_rows(c, cep[0], Tfa, K, cep_a, (long)cep_stride, B, false);
    if (cep_b) copy_out_rows(c, cep[1], Tfb, K, cep_b, (long)cep_stride, B, false);
    std::vector<double> cost((size_t)B);
    std::vector<int32_t> plen((size_t)B);
    dtw_run(c, pl, cep[0], fa.data(), Tfa, cep[1], fb.data(), Tfb, B, K, cost.data(), plen.data(), path, path_stride, a2b, a2b_stride);
    for (int b = 0; b < B; b++) {
        double* o = stats + (size_t)b * ZVX_AL_COUNT;
        o[ZVX_AL_FRAMES_A] = (double)fa[(size_t)b]; o[ZVX_AL_FRAMES_B] = (double)fb[(size_t)b]; o[ZVX_AL_PATH_LEN] = (double)plen[(size_t)b];
        o[ZVX_AL_COST] = cost[(size_t)b];
        o[ZVX_AL_MCD_DB] = (10.0 / log(10.0)) * sqrt(2.0) * cost[(size_t)b] / (double)plen[(size_t)b];
    }
}

// wav: float rows, or int16 PCM rows with ZVX_PCM16 (stride counted in samples either way).  Row b receives
// mel_len[b]*hop samples followed by zeros up to max_b(mel_len[b])*hop; nothing beyond that is touched.
void do_vocode(zvx_ctx* c, const int32_t* pad_to, void* wav, int64_t wav_stride, int flags) {
    if (!c->have_mel) fail(ZVX_E_STATE, "zvx_vocode: no mel in the context (call zvx_decode first)");
    const int B = c->B;
    // an output rate (zvx_set_int "out_rate") other than the model's: the generator writes f32 rows into a work buffer and the resampler
    // writes the rows the caller sees -- `need`, the strides and the host slot's `valid` are then in OUTPUT samples.  ZVX_NATIVE_RATE
    // takes the call out of it.
    int rs_L = 1, rs_M = 1;
    const bool rs = c->out_rate && !(flags & ZVX_NATIVE_RATE) && c->out_rate != model_rate(c);
    if (rs) rs_pair(model_rate(c), c->out_rate, &rs_L, &rs_M);
    else { c->stage_used[ZVX_T_RESAMPLE] = false; c->stage_ms[ZVX_T_RESAMPLE] = 0.f; }
    std::vector<int> P(B);
    int need = 0, need_native = 0;
    for (int b = 0; b < B; b++) { P[b] = std::max(pad_to ? pad_to[b] : 0, c->mel_len_host[b]); need_native = std::max(need_native, c->mel_len_host[b] * c->hop); }
    // each utterance is resampled as a signal of its own length, mel_len[b] * hop
    const RsPlan plan = rs ? rs_plan(c->mel_len_host.data(), c->hop, B, rs_L, rs_M) : RsPlan{};
    need = rs ? (int)plan.out_max : need_native;
    const bool host_async = flags & ZVX_HOST_ASYNC;
    if (!host_async && wav_stride < need) fail(ZVX_E_BUFFER, "wav_stride %lld < %d samples", (long long)wav_stride, need);
    const zvx_ctx::RsBank* bank = rs ? &rs_bank(c, rs_L, rs_M) : nullptr;
    c->stage_begin(ZVX_T_VOCODER);
    void* wdev; long wstride;
    const bool dev_out = (flags & ZVX_DEVICE_OUT) && !host_async;
    const int pcm16 = (flags & ZVX_PCM16) ? 1 : 0;
    const size_t ss = pcm16 ? 2 : 4;
    zvx_ctx::HostSlot* hs = nullptr;
    if (host_async) {
        // slot i & 1 of call i: its previous copy (two calls back) has normally long landed and been read; the device-side staging rows are
        // per slot as well, so this vocoder's conv_post never writes what the previous call's copy is still reading
        const int slot = c->host_next; c->host_next ^= 1; c->host_last = slot;
        hs = &c->host_slot[slot];
        // The copies ride the communication stream where the context has one (world 1: it is idle; a multi-GPU rank gathers on the device
        // instead of delivering to its host): the runtime maps streams onto FOUR hardware queues by default (GPU_MAX_HW_QUEUES), and the
        // context's main / front / predictor / communication streams are four -- a fifth stream shares a queue with one of them, and its
        // wait-for-the-vocoder barrier then holds up that stream's launches too (measured: the whole front-end overlap lost, +1.2 ms)
        if (!c->copy_stream) { if (c->comm_stream) { c->copy_stream = c->comm_stream; c->copy_is_comm = true; } else HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)); }
        if (!hs->ready) { HIPCHK(hipEventCreateWithFlags(&hs->ready, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&hs->done, hipEventDisableTiming)); }
        if (hs->pending) { HIPCHK(hipEventSynchronize(hs->done)); hs->pending = false; }
        wstride = (std::max(need, 1) + 7) & ~7;
        const size_t bytes = (size_t)B * wstride * ss;
        if (bytes > hs->cap) {
            if (hs->p) { HIPCHK(hipHostFree(hs->p)); hs->p = nullptr; hs->cap = 0; }
            const size_t cap = bytes + bytes / 8 + 256;
            HIPCHK(hipHostMalloc(&hs->p, cap, hipHostMallocDefault));
            hs->cap = cap;
        }
        wdev = c->buf(slot ? "wav.async1" : "wav.async0", bytes);
        hs->B = B; hs->pcm16 = pcm16; hs->stride = wstride; hs->need = need;
    } else if (dev_out) {
        wdev = wav; wstride = wav_stride;
        auto f = c->gather_fence.find(wav);                 // a gather still reading this buffer: the vocoder's writes queue behind it
        if (f != c->gather_fence.end()) HIPCHK(hipStreamWaitEvent(c->stream, f->second, 0));
    }
    else { wstride = (std::max(need, 1) + 7) & ~7; wdev = c->buf("wav", (size_t)B * wstride * ss); }
    if (rs) {
        // on the main stream behind conv_post (no stream of its own: the context's four fill the hardware queues a process gets, see above)
        const long nstride = (std::max(need_native, 1) + 7) & ~7;
        float* native = c->fbuf("wav.native", (size_t)B * nstride);
        run_vocoder(c, c->fbuf("mel", 0), c->n_mels, c->Lmax, c->mel_len_host.data(), P.data(), B, native, nstride, 0);
        c->stage_end(ZVX_T_VOCODER);
        run_resample_rows(c, *bank, plan_rows(plan, native, nstride, wdev, wstride, ss, c->mel_len_host.data(), c->hop, B).data(), B, pcm16, plan.out_max);
    } else {
        run_vocoder(c, c->fbuf("mel", 0), c->n_mels, c->Lmax, c->mel_len_host.data(), P.data(), B, wdev, wstride, pcm16);
        c->stage_end(ZVX_T_VOCODER);
    }
    if (host_async) {
        HIPCHK(hipEventRecord(hs->ready, c->stream));
        HIPCHK(hipStreamWaitEvent(c->copy_stream, hs->ready, 0));
        if (need > 0) HIPCHK(hipMemcpyAsync(hs->p, wdev, (size_t)B * wstride * ss, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(hipEventRecord(hs->done, c->copy_stream));
        hs->pending = true;
        return;                                              // queued: zvx_wait_host(slot) is where the host meets the rows
    }
    if (!dev_out && need > 0)
        HIPCHK(hipMemcpy2DAsync(wav, (size_t)wav_stride * ss, wdev, (size_t)wstride * ss, (size_t)need * ss, B, hipMemcpyDeviceToHost, c->stream));
    if (!(dev_out && (flags & ZVX_NO_SYNC))) c->sync();
}
}  // namespace

}  // namespace zvx::host


// ================================================================================================
// C-ABI
// ================================================================================================
extern "C" {

zvx_status zvx_create(const char* manifest, const void* weights, size_t nbytes, int device, zvx_ctx** out) {
    if (!out) return ZVX_E_INVALID;
    *out = nullptr;
    zvx_ctx* c = new zvx_ctx();
    try {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) fail(ZVX_E_HIP, "no HIP device available (%s)", hipGetErrorString(e));
        if (device < 0 || device >= ndev) fail(ZVX_E_INVALID, "device %d out of range (%d visible)", device, ndev);
        c->device = device;
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreate(&c->stream));
        c->main0 = c->stream;
        for (int s = 0; s < ZVX_T_COUNT; s++) { HIPCHK(hipEventCreate(&c->stage_ev[s][0])); HIPCHK(hipEventCreate(&c->stage_ev[s][1])); c->stage_used[s] = false; c->stage_ms[s] = 0.f; }
        parse_manifest(c, manifest, weights, nbytes);
        read_config(c);
        upload_weights(c);
        *out = c;
        return ZVX_OK;
    } catch (const ZvxError& e) {
        g_create_error = e.what();
        delete c;
        return e.code;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        delete c;
        return ZVX_E_INVALID;
    }
}

void zvx_destroy(zvx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->front_stream) (void)hipStreamSynchronize(c->front_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    while (!c->streams.empty()) stream_free(c->streams.back());      // the open stream sessions go first
    zvx_comm_destroy(c);
    for (int i = 0; i < 2; i++) { if (c->arena[i].p) (void)hipHostFree(c->arena[i].p); if (c->arena[i].ev) (void)hipEventDestroy(c->arena[i].ev); }
    if (c->copy_stream && !c->copy_is_comm) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    for (auto& hs : c->host_slot) { if (hs.p) (void)hipHostFree(hs.p); if (hs.ready) (void)hipEventDestroy(hs.ready); if (hs.done) (void)hipEventDestroy(hs.done); }
    if (c->join_host) (void)hipHostFree(c->join_host);
    for (int i = 0; i < 2; i++) if (c->voc_aux[i]) { (void)hipStreamSynchronize(c->voc_aux[i]); (void)hipStreamDestroy(c->voc_aux[i]); }
    for (int i = 0; i < 3; i++) if (c->voc_ev[i]) (void)hipEventDestroy(c->voc_ev[i]);
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); (void)hipEventDestroy(c->ev_aux[0]); (void)hipEventDestroy(c->ev_aux[1]); }
    if (c->front_stream) {
        (void)hipStreamSynchronize(c->front_stream); (void)hipStreamDestroy(c->front_stream);
        (void)hipEventDestroy(c->ev_front_done); (void)hipEventDestroy(c->ev_mel_free); (void)hipEventDestroy(c->ev_main_join);
    }
    for (auto& kv : c->bufs) if (kv.second.base) (void)hipFree(kv.second.base);
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->stream) {
        for (int s = 0; s < ZVX_T_COUNT; s++) { (void)hipEventDestroy(c->stage_ev[s][0]); (void)hipEventDestroy(c->stage_ev[s][1]); }
        (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

const char* zvx_last_error(const zvx_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

namespace {

// The run-time switches of zvx_set_int / zvx_get_int: the context member behind each key and the values it accepts
struct Switch { const char* key; int zvx_ctx::*v; bool (*ok)(int64_t); };
bool flag(int64_t v) { return v == 0 || v == 1; }
bool count(int64_t v) { return v >= 0 && v <= INT32_MAX; }
const Switch kSwitches[] = {
    {"profile", &zvx_ctx::profile, [](int64_t v) { return v >= 0 && v <= 2; }},
    {"profile_only", &zvx_ctx::profile_only, [](int64_t v) { return v >= -1 && v < gemm_num_variants(); }},
    {"shape_log", &zvx_ctx::shape_log, flag},
    {"rs_prof", &zvx_ctx::rs_prof, flag},
    {"f16_sat_check", &zvx_ctx::sat_check, flag},
    {"poison_pads", &zvx_ctx::poison_pads, flag},
    {"max_frames", &zvx_ctx::max_frames, [](int64_t v) { return v >= 1 && v <= (1 << 24); }},
    {"enc_split", &zvx_ctx::enc_split, [](int64_t v) { return v >= 0 && v <= 2; }},
    {"attn_f32", &zvx_ctx::use_attn_f32, flag},
    {"flash", &zvx_ctx::use_flash, flag},
    {"front_overlap", &zvx_ctx::front_overlap, [](int64_t v) { return v >= 0 && v <= 2; }},
    {"va_overlap_maxb", &zvx_ctx::va_overlap_maxb, count},
    {"dec_f16", &zvx_ctx::dec_f16, flag},
    {"dec_flat", &zvx_ctx::dec_flat, flag},
    {"dec_sc_fuse", &zvx_ctx::dec_sc_fuse, flag},
    {"norm_fuse_maxb", &zvx_ctx::norm_fuse_maxb, count},
    {"voc_f16", &zvx_ctx::voc_f16, flag},
    {"voc_f16_stages", &zvx_ctx::voc_f16_stages, [](int64_t v) { return v >= -1 && v <= INT32_MAX; }},
    {"voc_overlap_maxb", &zvx_ctx::voc_overlap_maxb, count},
    {"voc_overlap_frames", &zvx_ctx::voc_overlap_frames, count},
    {"stagefuse", &zvx_ctx::use_stagefuse, flag},
    {"rb2fuse", &zvx_ctx::use_rb2fuse, flag},
    {"resstream", &zvx_ctx::use_resstream, flag},
    {"rs_seg_min", &zvx_ctx::rs_seg_min, [](int64_t v) { return v >= -1 && v <= INT32_MAX; }},
    {"pairstream", &zvx_ctx::use_pairstream, [](int64_t v) { return v == -1 || v == 0 || v == 1 || v == 3; }},
    {"slab_small", &zvx_ctx::slab_small, [](int64_t v) { return (v & ~32) >= 0 && (v & ~32) <= 2; }},
    {"slab_flat", &zvx_ctx::slab_flat, flag},
    {"spk_pool_fuse", &zvx_ctx::spk_pool_fuse, flag},
    {"spk_s2_fuse", &zvx_ctx::spk_s2_fuse, flag},
    {"out_rate", &zvx_ctx::out_rate, count},
};
const Switch* find_switch(const char* key) {
    for (const Switch& s : kSwitches) if (!strcmp(s.key, key)) return &s;
    return nullptr;
}

}  // namespace

int64_t zvx_get_int(const zvx_ctx* c, const char* key) {
    if (!c || !key) return -1;
    if (const Switch* s = find_switch(key)) return c->*s->v;
    const std::string k(key);
    if (k == "precision") return c->dt == DT_F32 ? 1 : 0;
    if (k == "hidden") return c->H;
    if (k == "n_mels") return c->n_mels;
    if (k == "hop") return c->hop;
    if (k == "device") return c->device;
    if (k == "dec_kind") return c->dec_kind;
    if (k == "Lmax") return c->Lmax;
    if (k == "f16_sat_events") {                             // clamped 16-bit stores seen since zvx_set_int("f16_sat_check", 1); drains the context's streams
        zvx_ctx* m = const_cast<zvx_ctx*>(c);
        unsigned long long n = 0;
        if (hipSetDevice(m->device) != hipSuccess) return -1;
        try { unsigned long long* d = m->sat_count_dev(); m->sync(); if (hipMemcpy(&n, d, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return -1; } catch (...) { return -1; }
        return (int64_t)n;
    }
    if (k == "fir_tile") return FIR_TILE;                   // emitted samples per workgroup of zvx_fir (the tests' tile-edge rows)
    if (k == "host_slot") return c->host_last;             // the slot the last ZVX_HOST_ASYNC call writes (-1: none yet)
    if (k.rfind("variant_id:", 0) == 0) { for (int i = 0; i < gemm_num_variants(); i++) if (k.substr(11) == gemm_variant_name(i)) return i; return -1; }
    auto it = c->cfg.find(k);
    if (it != c->cfg.end()) return atoll(it->second.c_str());
    return -1;
}

zvx_status zvx_set_int(zvx_ctx* c, const char* key, int64_t value) {
    return guarded(c, [&] {
        if (!key) fail(ZVX_E_INVALID, "key is NULL");
        const Switch* s = find_switch(key);
        if (!s) fail(ZVX_E_INVALID, "unknown option '%s'", key);
        if (!s->ok(value)) fail(ZVX_E_INVALID, "option '%s' does not take the value %lld", key, (long long)value);
        const std::string k(key);
        if (k == "out_rate" && value) {                       // the predicate sees only the value: this key is checked against the model's rate,
            int L = 1, M = 1;                                  // and its bank is built here, so that a queued call never designs or uploads one
            rs_pair(model_rate(c), (int)value, &L, &M);
            if ((int)value != model_rate(c)) rs_bank(c, L, M);
        }
        if (k == "profile" || k == "profile_only" || k == "f16_sat_check" || k == "front_overlap") c->sync();
        c->*s->v = (int)value;
        if (k == "f16_sat_check") HIPCHK(hipMemsetAsync(c->sat_count_dev(), 0, 64, c->stream));      // (re)arms the audit and zeroes its counter
        if (k == "front_overlap") c->front_dirty_main = true;
        if (k == "enc_split") {
            if (c->dt != DT_BF16) c->enc_split = 0;                                                   // the f32 mode has no split planes
            if (c->enc_split) { c->sync(); build_split_weights(c, c->enc_split == 2); }
        }
    });
}

zvx_status zvx_spkemb(zvx_ctx* c, const float* ref_mels, const int32_t* lens, int B, int Tmax, float* out) {
    return guarded(c, [&] {
        if (!ref_mels || !lens || !out || B <= 0 || Tmax <= 0) fail(ZVX_E_INVALID, "zvx_spkemb: bad arguments");
        run_spkemb(c, ref_mels, lens, B, Tmax, out, 0);
    });
}

zvx_status zvx_spkemb_ex(zvx_ctx* c, const float* ref_mels, const int32_t* lens, int B, int Tmax, float* out, int flags) {
    return guarded(c, [&] {
        if (!ref_mels || !lens || !out || B <= 0 || Tmax <= 0) fail(ZVX_E_INVALID, "zvx_spkemb_ex: bad arguments");
        run_spkemb(c, ref_mels, lens, B, Tmax, out, flags);
    });
}

zvx_status zvx_melspec(zvx_ctx* c, const float* wav, const int32_t* nsamples, int B, int Nmax, float* mel, int Tmax, int32_t* frames) {
    return guarded(c, [&] {
        if (!wav || !nsamples || B <= 0 || Nmax <= 0 || Tmax <= 0) fail(ZVX_E_INVALID, "zvx_melspec: bad arguments");
        run_melspec(c, wav, nsamples, B, Nmax, mel, Tmax, frames);
    });
}

zvx_status zvx_spkemb_wav(zvx_ctx* c, const float* wav, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_ref_params* params, float* out,
                          int32_t* begin, int32_t* end, int32_t* frames, int flags) {
    return guarded(c, [&] { do_spkemb_wav(c, wav, nsamples, B, Nmax, rate, params, out, begin, end, frames, flags); });
}

zvx_status zvx_encode(zvx_ctx* c, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration, const int32_t* T,
                      int B, int Tmax, const float* spk, int32_t* mel_len, float* log_duration, float* pitch, float* energy) {
    return zvx_encode_ex(c, phoneme, puncts, duration, T, B, Tmax, spk, mel_len, log_duration, pitch, energy, nullptr);
}

zvx_status zvx_encode_ex(zvx_ctx* c, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration, const int32_t* T,
                         int B, int Tmax, const float* spk, int32_t* mel_len, float* log_duration, float* pitch, float* energy,
                         const zvx_prosody* prosody) {
    return guarded(c, [&] {
        if (!phoneme || !puncts || !T || !spk) fail(ZVX_E_INVALID, "zvx_encode: NULL input");
        run_encode(c, phoneme, puncts, duration, T, B, Tmax, spk, mel_len, 0, prosody);
        const size_t nid = (size_t)B * Tmax;
        if (log_duration) HIPCHK(hipMemcpyAsync(log_duration, c->fbuf("va.logd", nid), nid * 4, hipMemcpyDeviceToHost, c->stream));
        if (pitch) HIPCHK(hipMemcpyAsync(pitch, c->fbuf("va.pitch", nid), nid * 4, hipMemcpyDeviceToHost, c->stream));
        if (energy) HIPCHK(hipMemcpyAsync(energy, c->fbuf("va.energy", nid), nid * 4, hipMemcpyDeviceToHost, c->stream));
        c->sync();
    });
}

zvx_status zvx_decode(zvx_ctx* c, float* mel_out, int Lstride, int flags) {
    return guarded(c, [&] {
        if (!c->have_features) fail(ZVX_E_STATE, "zvx_decode: no features in the context (call zvx_encode first)");
        const int B = c->B;
        int* L_d = c->upload_ints("dec.L", c->mel_len_host.data(), B);
        run_decode(c, c->fbuf("features", 0), c->fbuf("in.spk", 0), L_d, B, c->Lmax);
        if (mel_out && c->Lmax > 0) copy_out_rows(c, c->fbuf("mel", 0), c->Lmax, c->n_mels, mel_out, Lstride, B, flags & ZVX_DEVICE_OUT);
        c->sync();
    });
}

zvx_status zvx_decode_features(zvx_ctx* c, const float* features, const int32_t* L, int B, int Lmax, const float* spk,
                               float* mel_out, int Lstride) {
    return guarded(c, [&] {
        if (!features || !L || !spk || B <= 0 || Lmax <= 0) fail(ZVX_E_INVALID, "zvx_decode_features: bad arguments");
        for (int b = 0; b < B; b++) if (L[b] < 2 || L[b] > Lmax) fail(ZVX_E_INVALID, "L[%d]=%d out of range (2..%d)", b, L[b], Lmax);
        c->B = B; c->Lmax = Lmax; c->mel_len_host.assign(L, L + B); c->Tmax = 0;
        c->have_features = false; c->have_mel = false;
        float* f = c->fbuf("features", (size_t)B * Lmax * c->H);
        HIPCHK(hipMemcpyAsync(f, features, (size_t)B * Lmax * c->H * 4, hipMemcpyHostToDevice, c->stream));
        float* spk_d = c->fbuf("in.spk", (size_t)B * c->H);
        HIPCHK(hipMemcpyAsync(spk_d, spk, (size_t)B * c->H * 4, hipMemcpyHostToDevice, c->stream));
        int* L_d = c->upload_ints("dec.L", L, B);
        c->have_features = true;
        run_decode(c, f, spk_d, L_d, B, Lmax);
        if (mel_out) copy_out_rows(c, c->fbuf("mel", 0), Lmax, c->n_mels, mel_out, Lstride, B, false);
        c->sync();
    });
}

zvx_status zvx_vocode(zvx_ctx* c, const int32_t* pad_to, void* wav, int64_t wav_stride, int flags) {
    return guarded(c, [&] {
        if (!wav && !(flags & ZVX_HOST_ASYNC)) fail(ZVX_E_INVALID, "zvx_vocode: wav is NULL");
        do_vocode(c, pad_to, wav, wav_stride, flags);
    });
}

zvx_status zvx_vocode_mel(zvx_ctx* c, const float* mel, const int32_t* P, int B, int Pmax, void* wav, int64_t wav_stride, int flags) {
    return guarded(c, [&] {
        if (!mel || !P || (!wav && !(flags & ZVX_HOST_ASYNC)) || B <= 0 || Pmax <= 0) fail(ZVX_E_INVALID, "zvx_vocode_mel: bad arguments");
        for (int b = 0; b < B; b++) if (P[b] < 1 || P[b] > Pmax) fail(ZVX_E_INVALID, "P[%d]=%d out of range (1..%d)", b, P[b], Pmax);
        c->B = B; c->Lmax = Pmax; c->Tmax = 0; c->mel_len_host.assign(P, P + B);
        c->have_features = false; c->have_mel = false;             // the context's batch geometry changes: earlier intermediates are void
        float* m = c->fbuf("mel", (size_t)B * Pmax * c->n_mels);
        HIPCHK(hipMemcpyAsync(m, mel, (size_t)B * Pmax * c->n_mels * 4, (flags & ZVX_DEVICE_IN) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        c->have_mel = true;
        do_vocode(c, nullptr, wav, wav_stride, flags);
    });
}

zvx_status zvx_resample(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out,
                        int64_t out_stride, int32_t* out_len, int flags) {
    return guarded(c, [&] { do_resample(c, in, nsamples, B, Nmax, rate_in, rate_out, out, out_stride, out_len, flags, 0, 0, -1); });
}

zvx_status zvx_resample_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out,
                           int64_t out_stride, int32_t* out_len, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count) {
    return guarded(c, [&] { do_resample(c, in, nsamples, B, Nmax, rate_in, rate_out, out, out_stride, out_len, flags, in_origin, out_begin, out_count); });
}

zvx_status zvx_resample_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate_in, int rate_out, void* out,
                             int64_t out_stride, int32_t* out_len, int flags, const zvx_row_window* win) {
    return guarded(c, [&] { do_resample_rows(c, in, nsamples, B, Nmax, rate_in, rate_out, out, out_stride, out_len, flags, win); });
}

zvx_status zvx_trim_bounds(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_join_params* params, int32_t* begin,
                           int32_t* end, int flags) {
    return guarded(c, [&] { do_trim_bounds(c, in, nsamples, B, Nmax, params, begin, end, flags); });
}

zvx_status zvx_join(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const int32_t* gap, const zvx_join_params* params,
                    void* out, int64_t out_capacity, int64_t* out_len, int64_t* seg_pos, int32_t* seg_begin, int32_t* seg_len, int flags) {
    return guarded(c, [&] { do_join(c, in, nsamples, B, Nmax, gap, params, out, out_capacity, out_len, seg_pos, seg_begin, seg_len, flags); });
}

zvx_status zvx_loudness(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, double* lufs, float* peak, int flags) {
    return guarded(c, [&] { do_loudness(c, "zvx_loudness", in, nsamples, B, Nmax, rate, nullptr, nullptr, 0, lufs, peak, nullptr, flags); });
}

zvx_status zvx_normalize(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_loudness_params* params,
                         void* out, int64_t out_stride, double* lufs, float* peak, float* gain, int flags) {
    return guarded(c, [&] {
        if (!params) fail(ZVX_E_INVALID, "zvx_normalize: params is NULL");
        do_loudness(c, "zvx_normalize", in, nsamples, B, Nmax, rate, params, out, out_stride, lufs, peak, gain, flags);
    });
}
zvx_status zvx_loudness_stats(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, double* stats, double* momentary,
                              double* short_term, int64_t curve_stride, int flags) {
    return guarded(c, [&] { run_loudness_stats(c, in, nsamples, B, Nmax, rate, stats, momentary, short_term, curve_stride, flags); });
}
zvx_status zvx_pitch(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_pitch_params* params, float* f0,
                     float* aper, int64_t f_stride, int32_t* frames, double* stats, int flags) {
    return guarded(c, [&] { do_pitch(c, in, nsamples, B, Nmax, rate, params, f0, aper, f_stride, frames, stats, flags); });
}

zvx_status zvx_dtw(zvx_ctx* c, const float* a, const int32_t* Ta, int Tamax, const float* b, const int32_t* Tb, int Tbmax, int B, int dim,
                   const zvx_dtw_params* params, double* cost, int32_t* path_len, int32_t* path, int64_t path_stride, int32_t* a2b, int flags) {
    return guarded(c, [&] { do_dtw(c, a, Ta, Tamax, b, Tb, Tbmax, B, dim, params, cost, path_len, path, path_stride, a2b, flags); });
}
zvx_status zvx_align_wav(zvx_ctx* c, const float* wav_a, const int32_t* n_a, int Nmax_a, const float* wav_b, const int32_t* n_b, int Nmax_b, int B,
                         const zvx_align_params* params, double* stats, int32_t* path, int64_t path_stride, int32_t* a2b, int64_t a2b_stride,
                         float* cep_a, float* cep_b, int64_t cep_stride, int flags) {
    return guarded(c, [&] {
        do_align_wav(c, wav_a, n_a, Nmax_a, wav_b, n_b, Nmax_b, B, params, stats, path, path_stride, a2b, a2b_stride, cep_a, cep_b, cep_stride, flags);
    });
}

zvx_status zvx_true_peak(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, int oversample, float* tpeak, int flags) {
    return guarded(c, [&] { do_limit(c, "zvx_true_peak", in, nsamples, B, Nmax, rate, nullptr, oversample, nullptr, 0, tpeak, nullptr, flags); });
}

zvx_status zvx_limit(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_limit_params* params,
                     void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags) {
    return guarded(c, [&] {
        if (!params) fail(ZVX_E_INVALID, "zvx_limit: params is NULL");
        do_limit(c, "zvx_limit", in, nsamples, B, Nmax, rate, params, 0, out, out_stride, peak_in, min_gain, flags);
    });
}

zvx_status zvx_limit_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_limit_params* params,
                        void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags,
                        int64_t in_origin, int64_t out_begin, int64_t out_count, int last) {
    return guarded(c, [&] {
        if (!params) fail(ZVX_E_INVALID, "zvx_limit_ex: params is NULL");
        const WindowsIn win{WindowsIn::ONE, RowsWindow{in_origin, out_begin, out_count, last}};
        do_limit(c, "zvx_limit_ex", in, nsamples, B, Nmax, rate, params, 0, out, out_stride, peak_in, min_gain, flags, win);
    });
}

zvx_status zvx_denoise_bias(zvx_ctx* c, float* bias) {
    return guarded(c, [&] { do_denoise_bias(c, bias); });
}

zvx_status zvx_denoise(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                       const zvx_denoise_params* params, void* out, int64_t out_stride, int flags) {
    return guarded(c, [&] { do_denoise(c, "zvx_denoise", in, nsamples, B, Nmax, bias, params, out, out_stride, flags); });
}

zvx_status zvx_denoise_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                          const zvx_denoise_params* params, void* out, int64_t out_stride, int flags,
                          int64_t in_origin, int64_t out_begin, int64_t out_count, int last) {
    return guarded(c, [&] {
        const WindowsIn win{WindowsIn::ONE, RowsWindow{in_origin, out_begin, out_count, last}};
        do_denoise(c, "zvx_denoise_ex", in, nsamples, B, Nmax, bias, params, out, out_stride, flags, win);
    });
}

zvx_status zvx_watermark(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params, void* out,
                         int64_t out_stride, int flags) {
    return guarded(c, [&] { do_watermark(c, "zvx_watermark", in, nsamples, B, Nmax, params, out, out_stride, flags); });
}

zvx_status zvx_watermark_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params, void* out,
                            int64_t out_stride, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count, int last) {
    return guarded(c, [&] {
        const WindowsIn win{WindowsIn::ONE, RowsWindow{in_origin, out_begin, out_count, last}};
        do_watermark(c, "zvx_watermark_ex", in, nsamples, B, Nmax, params, out, out_stride, flags, win);
    });
}

zvx_status zvx_watermark_detect(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                                int window_frames, float* score, int32_t* offset, int32_t* window, float* win_score, int32_t* win_offset,
                                int NWmax, int flags) {
    return guarded(c, [&] {
        do_watermark_detect(c, in, nsamples, B, Nmax, params, window_frames, score, offset, window, win_score, win_offset, NWmax, flags);
    });
}

zvx_status zvx_watermark_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                              const uint64_t* keys, void* out, int64_t out_stride, int flags, const zvx_row_window* win) {
    return guarded(c, [&] {
        const WindowsIn w{WindowsIn::PER_ROW, RowsWindow{}, win};
        do_watermark(c, "zvx_watermark_rows", in, nsamples, B, Nmax, params, out, out_stride, flags, w, keys);
    });
}

zvx_status zvx_watermark_identify(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const zvx_watermark_params* params,
                                  const uint64_t* keys, int K, int window_frames, float* score, int32_t* offset, int32_t* window, int32_t* best,
                                  int flags) {
    return guarded(c, [&] { do_watermark_identify(c, in, nsamples, B, Nmax, params, keys, K, window_frames, score, offset, window, best, flags); });
}

zvx_status zvx_spk_score(zvx_ctx* c, const float* query, int B, const float* lib, int64_t K, int dim, float* score, int flags) {
    return guarded(c, [&] { do_spk_match(c, "zvx_spk_score", query, B, lib, K, dim, 0, score, nullptr, flags, false); });
}

zvx_status zvx_spk_topk(zvx_ctx* c, const float* query, int B, const float* lib, int64_t K, int dim, int top, float* score, int32_t* index, int flags) {
    return guarded(c, [&] { do_spk_match(c, "zvx_spk_topk", query, B, lib, K, dim, top, score, index, flags, true); });
}

zvx_status zvx_denoise_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* bias,
                            const zvx_denoise_params* params, void* out, int64_t out_stride, int flags, const zvx_row_window* win) {
    return guarded(c, [&] {
        const WindowsIn w{WindowsIn::PER_ROW, RowsWindow{}, win};
        do_denoise(c, "zvx_denoise_rows", in, nsamples, B, Nmax, bias, params, out, out_stride, flags, w);
    });
}

zvx_status zvx_limit_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_limit_params* params,
                          void* out, int64_t out_stride, float* peak_in, float* min_gain, int flags, const zvx_row_window* win) {
    return guarded(c, [&] {
        if (!params) fail(ZVX_E_INVALID, "zvx_limit_rows: params is NULL");
        const WindowsIn w{WindowsIn::PER_ROW, RowsWindow{}, win};
        do_limit(c, "zvx_limit_rows", in, nsamples, B, Nmax, rate, params, 0, out, out_stride, peak_in, min_gain, flags, w);
    });
}

zvx_status zvx_level(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* params,
                     void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags) {
    return guarded(c, [&] { do_level(c, "zvx_level", in, nsamples, B, Nmax, rate, params, out, out_stride, gain_lo, gain_hi, flags); });
}

zvx_status zvx_level_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* params,
                        void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags,
                        int64_t in_origin, int64_t out_begin, int64_t out_count, int last) {
    return guarded(c, [&] {
        const WindowsIn win{WindowsIn::ONE, RowsWindow{in_origin, out_begin, out_count, last}};
        do_level(c, "zvx_level_ex", in, nsamples, B, Nmax, rate, params, out, out_stride, gain_lo, gain_hi, flags, win);
    });
}

zvx_status zvx_level_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, int rate, const zvx_level_params* params,
                          void* out, int64_t out_stride, float* gain_lo, float* gain_hi, int flags, const zvx_row_window* win) {
    return guarded(c, [&] {
        const WindowsIn w{WindowsIn::PER_ROW, RowsWindow{}, win};
        do_level(c, "zvx_level_rows", in, nsamples, B, Nmax, rate, params, out, out_stride, gain_lo, gain_hi, flags, w);
    });
}

zvx_status zvx_fir(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay, void* out,
                   int64_t out_stride, int flags) {
    return guarded(c, [&] { do_fir(c, "zvx_fir", in, nsamples, B, Nmax, taps, ntaps, delay, out, out_stride, flags); });
}

zvx_status zvx_fir_ex(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay, void* out,
                      int64_t out_stride, int flags, int64_t in_origin, int64_t out_begin, int64_t out_count, int last) {
    return guarded(c, [&] {
        const WindowsIn win{WindowsIn::ONE, RowsWindow{in_origin, out_begin, out_count, last}};
        do_fir(c, "zvx_fir_ex", in, nsamples, B, Nmax, taps, ntaps, delay, out, out_stride, flags, win);
    });
}

zvx_status zvx_fir_rows(zvx_ctx* c, const float* in, const int32_t* nsamples, int B, int Nmax, const float* taps, int ntaps, int delay, void* out,
                        int64_t out_stride, int flags, const zvx_row_window* win) {
    return guarded(c, [&] {
        const WindowsIn w{WindowsIn::PER_ROW, RowsWindow{}, win};
        do_fir(c, "zvx_fir_rows", in, nsamples, B, Nmax, taps, ntaps, delay, out, out_stride, flags, w);
    });
}

zvx_status zvx_stream_open(zvx_ctx* c, const float* mel, int frames, const zvx_stream_params* params, int flags, zvx_stream** out) {
    return guarded(c, [&] { do_stream_open(c, "zvx_stream_open", mel, frames, params, nullptr, flags, out); });
}

zvx_status zvx_stream_open_ex(zvx_ctx* c, const float* mel, int frames, const zvx_stream_params* params, const zvx_stream_stages* more, int flags,
                              zvx_stream** out) {
    return guarded(c, [&] { do_stream_open(c, more ? "zvx_stream_open_ex" : "zvx_stream_open", mel, frames, params, more, flags, out); });
}

zvx_status zvx_stream_next(zvx_stream* s, void* out, int64_t capacity, int64_t* n_out, int32_t* done, int flags) {
    if (!s) return ZVX_E_INVALID;
    return guarded(s->c, [&] { do_stream_next(s, out, capacity, n_out, done, flags); });
}

zvx_status zvx_stream_next_many(zvx_stream* const* sessions, int n, void* const* out, const int64_t* capacity, int64_t* n_out, int32_t* done,
                                int flags) {
    if (!sessions || n < 1) return ZVX_E_INVALID;
    zvx_ctx* c = nullptr;                                    // errors are reported through the sessions' context: the first session names it
    for (int i = 0; i < n && i < STREAM_MANY_MAX_SESSIONS && !c; i++) if (sessions[i]) c = sessions[i]->c;
    return guarded(c, [&] { do_stream_next_many(c, sessions, n, out, capacity, n_out, done, flags); });
}

zvx_status zvx_stream_info(const zvx_stream* s, int64_t* info, int n_info) {
    if (!s) return ZVX_E_INVALID;
    return guarded(s->c, [&] { do_stream_info(s, info, n_info); });
}

zvx_status zvx_stream_close(zvx_stream* s) {
    if (!s) return ZVX_E_INVALID;
    return guarded(s->c, [&] { stream_free(s); });
}

zvx_status zvx_synthesize(zvx_ctx* c, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration, const int32_t* T,
                          int B, int Tmax, const float* spk, const int32_t* pad_to, int Lmax_cap, void* wav, int64_t wav_stride,
                          int32_t* mel_len, float* mel_out, int Lstride, float* log_duration, int flags) {
    return zvx_synthesize_ex(c, phoneme, puncts, duration, T, B, Tmax, spk, pad_to, Lmax_cap, wav, wav_stride, mel_len, mel_out, Lstride,
                             log_duration, flags, nullptr);
}

zvx_status zvx_synthesize_ex(zvx_ctx* c, const int32_t* phoneme, const int32_t* puncts, const int32_t* duration, const int32_t* T,
                             int B, int Tmax, const float* spk, const int32_t* pad_to, int Lmax_cap, void* wav, int64_t wav_stride,
                             int32_t* mel_len, float* mel_out, int Lstride, float* log_duration, int flags, const zvx_prosody* prosody) {
    return guarded(c, [&] {
        const bool host_async = flags & ZVX_HOST_ASYNC;
        if (!phoneme || !puncts || !T || !spk || (!wav && !host_async)) fail(ZVX_E_INVALID, "zvx_synthesize: NULL input");
        if (host_async && ((mel_out && !(flags & ZVX_DEVICE_OUT)) || log_duration)) fail(ZVX_E_INVALID, "zvx_synthesize: ZVX_HOST_ASYNC takes no host mel / log_duration output (they would make the call wait)");
        auto front_end = [&] {
            run_encode(c, phoneme, puncts, duration, T, B, Tmax, spk, mel_len, Lmax_cap, prosody, flags & ZVX_DEVICE_SPK);
            if (log_duration) HIPCHK(hipMemcpyAsync(log_duration, c->fbuf("va.logd", 0), (size_t)B * Tmax * 4, hipMemcpyDeviceToHost, c->stream));
            int* L_d = c->upload_ints("dec.L", c->mel_len_host.data(), B);
            run_decode(c, c->fbuf("features", 0), c->fbuf("in.spk", 0), L_d, B, c->Lmax);
            if (mel_out && c->Lmax > 0) copy_out_rows(c, c->fbuf("mel", 0), c->Lmax, c->n_mels, mel_out, Lstride, B, flags & ZVX_DEVICE_OUT);
        };
        // a call that waits for its own result (no ZVX_NO_SYNC) has nothing to overlap with: it stays on the one stream (two streams
        // cost an event round trip, which a single short request would see); front_overlap 2 forces the two-stream schedule (tests)
        if (c->front_overlap == 2 || (c->front_overlap == 1 && (host_async || ((flags & ZVX_NO_SYNC) && (flags & ZVX_DEVICE_OUT))))) {
            // the front end on its own stream (see zvx_ctx::front_stream): ordered behind (1) whatever other entry points did to the
            // front-end buffers on the main stream, (2) the previous vocoder's read of the mel buffer -- and NOT behind that vocoder
            c->front_setup();
            hipStream_t const main_stream = c->stream;
            // (3) with ZVX_DEVICE_SPK, whatever wrote the embeddings on the main stream: the same join, an event and no host wait
            if (flags & ZVX_DEVICE_SPK) c->front_dirty_main = true;
            if (c->front_dirty_main) {
                HIPCHK(hipEventRecord(c->ev_main_join, main_stream));
                HIPCHK(hipStreamWaitEvent(c->front_stream, c->ev_main_join, 0));
                c->front_dirty_main = false; c->mel_free_pending = false;       // (the join covers the mel read too)
            }
            if (c->mel_free_pending) { HIPCHK(hipStreamWaitEvent(c->front_stream, c->ev_mel_free, 0)); c->mel_free_pending = false; }
            {
                struct Swap { zvx_ctx* c; hipStream_t keep; ~Swap() { c->stream = keep; } } sw{c, main_stream};   // restored on every path out
                c->stream = c->front_stream;
                front_end();
                HIPCHK(hipEventRecord(c->ev_front_done, c->front_stream));
            }
            HIPCHK(hipStreamWaitEvent(main_stream, c->ev_front_done, 0));
        } else {
            front_end();
        }
        do_vocode(c, pad_to, wav, wav_stride, flags);
    });
}

zvx_status zvx_fetch(zvx_ctx* c, const char* what, float* out, size_t out_floats) {
    return guarded(c, [&] {
        if (!what || !out) fail(ZVX_E_INVALID, "zvx_fetch: NULL argument");
        const std::string w(what);
        const size_t nid = (size_t)c->B * c->Tmax;
        auto copy_f = [&](const char* name, size_t n) {
            if (out_floats < n) fail(ZVX_E_BUFFER, "zvx_fetch('%s'): need %zu floats", what, n);
            HIPCHK(hipMemcpyAsync(out, c->fbuf(name, n), n * 4, hipMemcpyDeviceToHost, c->stream));
            c->sync();
        };
        auto copy_i = [&](const char* name, size_t n) {
            if (out_floats < n) fail(ZVX_E_BUFFER, "zvx_fetch('%s'): need %zu floats", what, n);
            std::vector<int> tmp(n);
            HIPCHK(hipMemcpyAsync(tmp.data(), c->ibuf(name, n), n * 4, hipMemcpyDeviceToHost, c->stream));
            c->sync();
            for (size_t i = 0; i < n; i++) out[i] = (float)tmp[i];
        };
        if (w == "encoder_out") copy_f("enc.out", nid * c->H);
        else if (w == "features") copy_f("features", (size_t)c->B * c->Lmax * c->H);
        else if (w == "mel") copy_f("mel", (size_t)c->B * c->Lmax * c->n_mels);
        else if (w == "pitch") copy_f("va.pitch", nid);
        else if (w == "energy") copy_f("va.energy", nid);
        else if (w == "log_duration") copy_f("va.logd", nid);
        else if (w == "pitch_idx") copy_i("va.pitch_idx", nid);
        else if (w == "energy_idx") copy_i("va.energy_idx", nid);
        else if (w == "duration") copy_i("va.dur", nid);
        else if (w.rfind("buf:", 0) == 0) {                              // raw bytes of a named context buffer (development aid)
            auto it = c->bufs.find(w.substr(4));
            if (it == c->bufs.end()) fail(ZVX_E_INVALID, "zvx_fetch: no buffer '%s'", what);
            const size_t nb = std::min(out_floats * 4, it->second.cap);
            HIPCHK(hipMemcpyAsync(out, it->second.p, nb, hipMemcpyDeviceToHost, c->stream));
            c->sync();
        }
        else fail(ZVX_E_INVALID, "zvx_fetch: unknown tensor '%s'", what);
    });
}

zvx_status zvx_sync(zvx_ctx* c) { return guarded(c, [&] { c->sync(); }); }

zvx_status zvx_wait_host(zvx_ctx* c, int slot, const void** rows, int64_t* stride, int32_t* nrows, int64_t* valid) {
    return guarded(c, [&] {
        if (slot < 0 || slot > 1) fail(ZVX_E_INVALID, "zvx_wait_host: slot %d (0 or 1)", slot);
        zvx_ctx::HostSlot& hs = c->host_slot[slot];
        if (!hs.done || !hs.p) fail(ZVX_E_STATE, "zvx_wait_host: no ZVX_HOST_ASYNC call has used slot %d", slot);
        if (hs.pending) { HIPCHK(hipEventSynchronize(hs.done)); hs.pending = false; }
        if (rows) *rows = hs.p;
        if (stride) *stride = hs.stride;
        if (nrows) *nrows = hs.B;
        if (valid) *valid = hs.need;
    });
}


zvx_status zvx_dev_alloc(zvx_ctx* c, size_t bytes, void** out) {
    return guarded(c, [&] {
        if (!out || !bytes) fail(ZVX_E_INVALID, "zvx_dev_alloc: bad arguments");
        HIPCHK(hipMalloc(out, bytes));
        HIPCHK(hipMemsetAsync(*out, 0, bytes, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

zvx_status zvx_dev_free(zvx_ctx* c, void* p) {
    return guarded(c, [&] {
        c->sync();
        auto f = c->gather_fence.find(p);
        if (f != c->gather_fence.end()) { if (f->second) (void)hipEventDestroy(f->second); c->gather_fence.erase(f); }
        if (p) HIPCHK(hipFree(p));
    });
}

zvx_status zvx_dev_from_host(zvx_ctx* c, void* dst, const void* src, size_t bytes) {
    return guarded(c, [&] {
        if (!dst || !src) fail(ZVX_E_INVALID, "zvx_dev_from_host: NULL pointer");
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

zvx_status zvx_dev_copy(zvx_ctx* c, void* dst, const void* src, size_t bytes) {
    return guarded(c, [&] {
        if (!dst || !src) fail(ZVX_E_INVALID, "zvx_dev_copy: NULL pointer");
        const char* d = (const char*)dst; const char* s = (const char*)src;
        if (d < s + bytes && s < d + bytes) fail(ZVX_E_INVALID, "zvx_dev_copy: the ranges overlap");
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

zvx_status zvx_dev_to_host(zvx_ctx* c, void* dst, const void* src, size_t bytes) {
    return guarded(c, [&] {
        if (!dst || !src) fail(ZVX_E_INVALID, "zvx_dev_to_host: NULL pointer");
        c->sync();
        HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    });
}

zvx_status zvx_stage_times(zvx_ctx* c, float ms[ZVX_T_COUNT]) {
    return guarded(c, [&] { c->sync(); for (int s = 0; s < ZVX_T_COUNT; s++) ms[s] = c->stage_ms[s]; });
}

int zvx_kernel_stats(zvx_ctx* c, zvx_kernel_stat* out, int max_out) {
    if (!c) return 0;
    int n = 0;
    guarded(c, [&] {
        c->sync();
        for (auto& s : c->stats) if (s.launches > 0 && n < max_out) out[n++] = s;
        for (auto& kv : c->namedstats) if (kv.second.launches > 0 && n < max_out) out[n++] = kv.second;
    });
    return n;
}

int zvx_tag_stats(zvx_ctx* c, zvx_kernel_stat* out, int max_out) {
    if (!c) return 0;
    int n = 0;
    guarded(c, [&] {
        c->sync();
        for (auto& kv : c->tagstats) if (kv.second.launches > 0 && n < max_out) out[n++] = kv.second;
    });
    return n;
}

zvx_status zvx_reset_stats(zvx_ctx* c) {
    return guarded(c, [&] { c->sync(); for (auto& s : c->stats) { s.launches = 0; s.ms = s.flops = s.bytes = 0; } c->tagstats.clear(); c->namedstats.clear(); });
}

}  // extern "C"
