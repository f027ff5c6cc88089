// model.hip -- handle, weight packing and the stage-level entry points of libdimx_hip (generation: generate.hip; the kernel-level
// entry points: ops.hip; what the three share: stages.hpp).
//
// Stage <-> reference map (paths relative to /root/reference):
//   vq_encode   : SLMFT.forward_vq / VQAutoEncoder.encode      code/seq2seq_pretrain.py:480-494,
//                                                               code/models/stage1_BIWI.py:22-27,307-317
//   vq_decode   : forward_vq_decoder / VQAutoEncoder.decode     code/seq2seq_pretrain.py:454-464,
//                                                               code/models/stage1_BIWI.py:29-37,376-393
//   encode_ctx  : forward_encoder + context concat              code/seq2seq_pretrain.py:431-446
//   decode_tf   : AutoregressiveWrapper.forward                 code/seq2seq_pretrain.py:448
//   generate    : AutoregressiveWrapper.generate                code/seq2seq_pretrain.py:450
// The per-sample Python loop of forward_vq becomes one batched launch sequence over ragged clips
// (per-clip length vectors instead of batch-1 calls); the one-hot matmul of forward_vq_decoder becomes
// a gather; the T-1 sequential decoder steps are one captured hipGraph replayed T-1 times with a
// device-resident step counter.
#include <stdarg.h>
#include <stdlib.h>
#include <set>

#include "stages.hpp"

namespace dimx {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

// ------------------------------------------------------------------ key names
static std::string vq_prefix(int which) { return which == 0 ? "speaker_vq." : "listener_vq."; }

struct KeySpec {
    std::string name;
    std::vector<int64_t> shape;
};

static void vq_keys(const dimx_dims& d, int which, std::vector<KeySpec>& out) {
    const int64_t H = d.vq_hidden, I = d.vq_inter;
    const std::string p = vq_prefix(which);
    auto stack = [&](const std::string& pre) {
        for (int i = 0; i < d.vq_layers; ++i) {
            const std::string a = pre + "net." + std::to_string(2 * i) + ".fn.";
            out.push_back({a + "norm.weight", {H}});
            out.push_back({a + "norm.bias", {H}});
            out.push_back({a + "fn.to_qkv.weight", {3 * H, H}});
            out.push_back({a + "fn.to_out.weight", {H, H}});
            out.push_back({a + "fn.to_out.bias", {H}});
            const std::string m = pre + "net." + std::to_string(2 * i + 1) + ".fn.";
            out.push_back({m + "norm.weight", {H}});
            out.push_back({m + "norm.bias", {H}});
            out.push_back({m + "fn.l1.weight", {I, H}});
            out.push_back({m + "fn.l1.bias", {I}});
            out.push_back({m + "fn.l2.weight", {H, I}});
            out.push_back({m + "fn.l2.bias", {H}});
        }
    };
    const std::string e = p + "encoder.", c = p + "decoder.";
    out.push_back({e + "vertice_mapping.0.weight", {H, d.vq_in_dim}});
    out.push_back({e + "vertice_mapping.0.bias", {H}});
    out.push_back({e + "squasher.0.0.weight", {H, H, 5}});
    out.push_back({e + "squasher.0.0.bias", {H}});
    stack(e + "encoder_transformer.");
    out.push_back({e + "encoder_pos_embedding.pe", {5000, 1, H}});
    out.push_back({e + "encoder_linear_embedding.net.weight", {H, H}});
    out.push_back({e + "encoder_linear_embedding.net.bias", {H}});
    out.push_back({e + "encoder_linear_embedding_post.net.weight", {d.vq_zdim, H}});
    out.push_back({e + "encoder_linear_embedding_post.net.bias", {d.vq_zdim}});
    out.push_back({c + "expander.0.0.weight", {H, H, 5}});
    out.push_back({c + "expander.0.0.bias", {H}});
    stack(c + "decoder_transformer.");
    out.push_back({c + "decoder_pos_embedding.pe", {5000, 1, H}});
    out.push_back({c + "decoder_linear_embedding.net.weight", {H, H}});
    out.push_back({c + "decoder_linear_embedding.net.bias", {H}});
    out.push_back({c + "decoder_linear_embedding_pre.net.weight", {H, d.vq_zdim}});
    out.push_back({c + "decoder_linear_embedding_pre.net.bias", {H}});
    out.push_back({c + "vertice_map_reverse.weight", {d.vq_in_dim, H}});
    out.push_back({p + "quantize.embedding.weight", {d.vq_n_embed, d.vq_zdim}});
}

static std::string xl(const std::string& pre, int li) { return pre + "attn_layers.layers." + std::to_string(li) + "."; }

static void xattn_keys(const std::string& p, int64_t dim, int64_t inner, std::vector<KeySpec>& out) {
    out.push_back({p + "0.0.weight", {dim}});
    out.push_back({p + "1.to_q.weight", {inner, dim}});
    out.push_back({p + "1.to_k.weight", {inner, dim}});
    out.push_back({p + "1.to_v.weight", {inner, dim}});
    out.push_back({p + "1.to_out.weight", {dim, inner}});
}
static void xff_keys(const std::string& p, int64_t dim, int64_t mult, std::vector<KeySpec>& out) {
    out.push_back({p + "0.0.weight", {dim}});
    out.push_back({p + "1.ff.0.0.weight", {dim * mult, dim}});
    out.push_back({p + "1.ff.0.0.bias", {dim * mult}});
    out.push_back({p + "1.ff.2.weight", {dim, dim * mult}});
    out.push_back({p + "1.ff.2.bias", {dim}});
}
static void xenc_keys(const dimx_dims& d, const std::string& pre, int64_t dim_in, std::vector<KeySpec>& out) {
    const int64_t inner = (int64_t)d.heads * d.dim_head;
    out.push_back({pre + "project_in.weight", {d.dim, dim_in}});
    out.push_back({pre + "pos_emb.emb.weight", {d.max_seq_len, d.dim}});
    for (int i = 0; i < d.enc_depth; ++i) {
        xattn_keys(xl(pre, 2 * i), d.dim, inner, out);
        xff_keys(xl(pre, 2 * i + 1), d.dim, d.ff_mult, out);
    }
    out.push_back({pre + "attn_layers.final_norm.weight", {d.dim}});
}
static void xdec_keys(const dimx_dims& d, const std::string& pre, std::vector<KeySpec>& out) {
    const int64_t D = d.dim + d.dim_a, inner = (int64_t)d.heads * d.dim_head;
    out.push_back({pre + "token_emb.emb.weight", {d.num_tokens, D}});
    for (int i = 0; i < d.dec_depth; ++i) {
        xattn_keys(xl(pre, 3 * i), D, inner, out);
        xattn_keys(xl(pre, 3 * i + 1), D, inner, out);
        xff_keys(xl(pre, 3 * i + 2), D, d.ff_mult, out);
    }
    out.push_back({pre + "attn_layers.final_norm.weight", {D}});
    out.push_back({pre + "to_logits.weight", {d.num_tokens, D}});
}

// legacy variant: encoder half + codebook of VQSpeakerAutoEncoder (code/models/stage1_BIWI.py:140-157)
static void legacy_speaker_vq_keys(const dimx_dims& d, std::vector<KeySpec>& out) {
    dimx_dims t = d;
    t.vq_in_dim = d.spk_in_dim;
    t.vq_hidden = d.spk_hidden;
    t.vq_heads = d.spk_heads;
    t.vq_inter = d.spk_inter;
    std::vector<KeySpec> all;
    vq_keys(t, 0, all);
    for (auto& k : all) {
        if (k.name.find(".decoder.") != std::string::npos) continue;
        if (k.name == "speaker_vq.encoder.encoder_linear_embedding_post.net.weight")
            k.shape = {(int64_t)d.spk_face_quan_num * d.vq_zdim, d.spk_hidden};
        if (k.name == "speaker_vq.encoder.encoder_linear_embedding_post.net.bias")
            k.shape = {(int64_t)d.spk_face_quan_num * d.vq_zdim};
        out.push_back(k);
    }
}

static void legacy_keys(const dimx_dims& d, std::vector<KeySpec>& k) {
    legacy_speaker_vq_keys(d, k);
    vq_keys(d, 1, k);
    xenc_keys(d, "generator.encoder.", (int64_t)d.spk_face_quan_num * d.vq_zdim, k);
    xdec_keys(d, "generator.decoder.net.", k);
    k.push_back({"generator.decoder.net.pos_emb.emb.weight", {d.max_seq_len, d.dim + d.dim_a}});
}

// what SLM (code/seq2seq_pretrain.py:58-165) uses on top of the SLMFT tensors; which: 1 encoder side, 2 decoder side
static void slm_extra_keys(const dimx_dims& d, std::vector<KeySpec>& k, int which) {
    if (which & 1) {
        xenc_keys(d, "encoder_l.", d.dim_in, k);
        k.push_back({"patch_embed_l", {1, 1, d.dim_in}});
        k.push_back({"patch_embed_dec_l", {1, 1, d.dim}});
        for (const char* n : {"norm_l", "norm"}) {
            k.push_back({std::string(n) + ".weight", {d.dim}});
            k.push_back({std::string(n) + ".bias", {d.dim}});
        }
    }
    if (which & 2) k.push_back({"decoder_joint.net.pos_emb.emb.weight", {d.max_seq_len, d.dim + d.dim_a}});
}

// converter head of SpeakerSLMFT / EmocaConverter (code/seq2seq_pretrain.py:801-819): nn.LSTM(56, 384, 2, bidirectional) and
// Sequential(Linear(768, 768), LeakyReLU, Linear(768, mesh_dim))
static const char* lstm_suffix(int dir) { return dir ? "_reverse" : ""; }
static void mesh_keys(const dimx_dims& d, std::vector<KeySpec>& k) {
    const std::string p = "vertice_map_reverse_lstm.";
    const int64_t H = 384;
    for (int l = 0; l < 2; ++l)
        for (int dir = 0; dir < 2; ++dir) {
            const std::string s = "_l" + std::to_string(l) + lstm_suffix(dir);
            k.push_back({p + "weight_ih" + s, {4 * H, l == 0 ? (int64_t)d.vq_in_dim : 2 * H}});
            k.push_back({p + "weight_hh" + s, {4 * H, H}});
            k.push_back({p + "bias_ih" + s, {4 * H}});
            k.push_back({p + "bias_hh" + s, {4 * H}});
        }
    k.push_back({"vertice_map_reverse.0.weight", {2 * H, 2 * H}});
    k.push_back({"vertice_map_reverse.0.bias", {2 * H}});
    k.push_back({"vertice_map_reverse.2.weight", {d.mesh_dim, 2 * H}});
    k.push_back({"vertice_map_reverse.2.bias", {d.mesh_dim}});
}

static std::vector<KeySpec> all_keys(const dimx_dims& d) {
    std::vector<KeySpec> k;
    if (d.variant == 1) {
        legacy_keys(d, k);
        return k;
    }
    vq_keys(d, 0, k);
    vq_keys(d, 1, k);
    xenc_keys(d, "encoder_s.", d.dim_in, k);
    xenc_keys(d, "encoder_joint.", d.dim, k);
    xdec_keys(d, "decoder_joint.net.", k);
    k.push_back({"patch_embed_s", {1, 1, d.dim_in}});
    k.push_back({"patch_embed_dec_s", {1, 1, d.dim}});
    k.push_back({"norm_s.weight", {d.dim}});
    k.push_back({"norm_s.bias", {d.dim}});
    if (d.variant == 2) slm_extra_keys(d, k, 3);
    if (d.mesh_dim > 0) mesh_keys(d, k);
    return k;
}

static bool ends_with(const std::string& n, const char* suf) {
    const size_t l = strlen(suf);
    return n.size() >= l && n.compare(n.size() - l, l, suf) == 0;
}

// SURVEY A.2 marks three details of x-transformers 1.30.16 [XT?] (restated from the library's published source, not verifiable
// here): project_in and to_logits are bias-free Linears and LayerNorm has no bias.  A checkpoint written by another release
// of the library carries them, so they are OPTIONAL tensors: a project_in.bias / to_logits.bias is applied when it is loaded;
// a LayerNorm bias (the zero `beta` buffer the reference's loader renames to `bias`, code/finetune_s2s_pretrain.py:49-57) is
// accepted when it is zero and refused otherwise -- never dropped in silence.
enum { OPT_NONE = 0, OPT_LINEAR_BIAS = 1, OPT_NORM_BIAS = 2 };
static int optional_key(const std::map<std::string, std::vector<int64_t>>& spec, const std::string& n, std::vector<int64_t>* shape) {
    if (!ends_with(n, ".bias")) return OPT_NONE;
    const std::string w = n.substr(0, n.size() - 4) + "weight";
    auto it = spec.find(w);
    if (it == spec.end()) return OPT_NONE;
    *shape = {it->second[0]};
    if (ends_with(w, "project_in.weight") || ends_with(w, "to_logits.weight")) return OPT_LINEAR_BIAS;
    if (w.find("attn_layers.") != std::string::npos && it->second.size() == 1) return OPT_NORM_BIAS;
    return OPT_NONE;
}

static bool ignorable_key(const std::string& n) {
    static const char* pre[] = {"encoder_l.", "norm_l.", "norm.", "patch_embed_l", "patch_embed_dec_l",
                                // legacy ListenerGenerator tensors that are not on the ids=None path
                                "speaker_vq.decoder_v.", "speaker_vq.decoder_a.", "speaker_embeddings.",
                                "listener_embeddings.", "fc_speaker.", "fc_listener.",
                                // SpeakerSLMFT / EmocaConverter tensors the reference's forward never applies (vertice_mapping and
                                // squasher feed an encoding nobody reads, the _2 head is dead code, code/seq2seq_pretrain.py:712-727)
                                // or that the host applies (speaker_embed)
                                "vertice_mapping.", "squasher.", "vertice_map_reverse_lstm_2.", "vertice_map_reverse2.",
                                "speaker_embed."};
    if (n == "W") return true;
    for (const char* p : pre)
        if (n.rfind(p, 0) == 0) return true;
    return ends_with(n, ".project_out.weight") || ends_with(n, ".project_out.bias");
}

// ------------------------------------------------------------------ packing
static int dev_upload(dimx_ctx* c, const void* src, size_t bytes, void** out) {
    void* p = nullptr;
    DIMX_HIP(hipMalloc(&p, bytes < 16 ? 16 : bytes));
    c->dev_allocs.push_back(p);
    DIMX_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *out = p;
    return DIMX_OK;
}

static int upload_f32(dimx_ctx* c, const std::string& name, const float** out) {
    auto it = c->host.find(name);
    DIMX_REQUIRE(it != c->host.end(), DIMX_ERR_WEIGHT, "missing weight %s", name.c_str());
    void* p;
    DIMX_TRY(dev_upload(c, it->second.data.data(), it->second.data.size() * 4, &p));
    *out = (const float*)p;
    return DIMX_OK;
}

// rows of `parts` concatenated; conv = true permutes [N][C][5] -> [N][5][C]
static int pack_linear(dimx_ctx* c, const std::vector<std::string>& parts, const std::string& bias, bool conv,
                       Linear* out) {
    const int bk = c->at == DIMX_BF16 ? 64 : 32;
    int N = 0, K = -1;
    for (const auto& n : parts) {
        auto it = c->host.find(n);
        DIMX_REQUIRE(it != c->host.end(), DIMX_ERR_WEIGHT, "missing weight %s", n.c_str());
        const auto& sh = it->second.shape;
        const int k = conv ? (int)(sh[1] * sh[2]) : (int)sh[1];
        DIMX_REQUIRE(K < 0 || K == k, DIMX_ERR_WEIGHT, "fused parts of %s disagree on K", n.c_str());
        K = k;
        N += (int)sh[0];
    }
    const int Kp = (K + bk - 1) / bk * bk;
    std::vector<float> w((size_t)N * Kp, 0.f);
    int row = 0;
    for (const auto& n : parts) {
        const HostTensor& t = c->host[n];
        const int rows = (int)t.shape[0];
        if (conv) {
            const int C = (int)t.shape[1];
            for (int r = 0; r < rows; ++r)
                for (int ci = 0; ci < C; ++ci)
                    for (int j = 0; j < 5; ++j)
                        w[(size_t)(row + r) * Kp + j * C + ci] = t.data[((size_t)r * C + ci) * 5 + j];
        } else {
            for (int r = 0; r < rows; ++r)
                memcpy(&w[(size_t)(row + r) * Kp], &t.data[(size_t)r * K], (size_t)K * 4);
        }
        row += rows;
    }
    void* p;
    if (c->at == DIMX_BF16) {
        std::vector<uint16_t> wb(w.size());
        for (size_t i = 0; i < w.size(); ++i) wb[i] = host_f32_to_bf16(w[i]);
        DIMX_TRY(dev_upload(c, wb.data(), wb.size() * 2, &p));
    } else {
        DIMX_TRY(dev_upload(c, w.data(), w.size() * 4, &p));
    }
    out->w = p;
    out->N = N;
    out->K = K;
    out->Kp = Kp;
    out->bias = nullptr;
    if (!bias.empty()) DIMX_TRY(upload_f32(c, bias, &out->bias));
    return DIMX_OK;
}

// f32 parity mode: the three bf16 planes of a packed f32 Linear (gemm_x3.hip; DIMX_NO_X3=1 keeps the f32 MFMA kernel, for A/B runs)
static int make_x3(dimx_ctx* c, Linear* L) {
    static const bool off = getenv("DIMX_NO_X3") != nullptr;
    L->w3 = nullptr;
    if (off || c->at != DIMX_F32 || !L->w || L->Kp % 32 != 0) return DIMX_OK;
    const size_t n = (size_t)L->N * L->Kp;
    void* p = nullptr;
    DIMX_HIP(hipMalloc(&p, 3 * n * 2));
    c->dev_allocs.push_back(p);
    DIMX_TRY(launch_split_x3((const float*)L->w, p, n, nullptr));
    DIMX_HIP(hipStreamSynchronize(nullptr));
    L->w3 = p;
    return DIMX_OK;
}

// W' = gamma o W (columns scaled by the LayerNorm weight that precedes the projection) in bf16, plus the f32 row sums of
// the ROUNDED W': LN(x) . W^T = rstd * (x . W'^T - mean * colsum(W')) (deferred LayerNorm of the decode step, bf16 mode)
static int pack_linear_scaled(dimx_ctx* c, const std::string& wname, const std::string& gname, const std::string& bias,
                              Linear* out, const float** colsum) {
    auto wi = c->host.find(wname), gi = c->host.find(gname);
    DIMX_REQUIRE(wi != c->host.end() && gi != c->host.end(), DIMX_ERR_WEIGHT, "missing weight %s / %s", wname.c_str(), gname.c_str());
    const int N = (int)wi->second.shape[0], K = (int)wi->second.shape[1];
    DIMX_REQUIRE((int)gi->second.data.size() == K && K % 64 == 0, DIMX_ERR_WEIGHT, "%s: gamma / K mismatch", wname.c_str());
    std::vector<uint16_t> wb((size_t)N * K);
    std::vector<float> cs(N);
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            const uint16_t b = host_f32_to_bf16(wi->second.data[(size_t)n * K + k] * gi->second.data[k]);
            wb[(size_t)n * K + k] = b;
            const uint32_t u = (uint32_t)b << 16;
            float f;
            memcpy(&f, &u, 4);
            acc += f;
        }
        cs[n] = (float)acc;
    }
    void *p, *q;
    DIMX_TRY(dev_upload(c, wb.data(), wb.size() * 2, &p));
    DIMX_TRY(dev_upload(c, cs.data(), cs.size() * 4, &q));
    out->w = p;
    out->N = N;
    out->K = K;
    out->Kp = K;
    out->bias = nullptr;
    if (!bias.empty()) DIMX_TRY(upload_f32(c, bias, &out->bias));
    *colsum = (const float*)q;
    return DIMX_OK;
}

// the feed-forward sublayer's weights as the chunk images of mlp_fused.hip (bf16 perf mode, width 384; the f32 mode and other
// widths keep the LayerNorm + two-GEMM form)
static int pack_mlp(dimx_ctx* c, const std::string& w1, const std::string& b1, const std::string& w2, const void** out) {
    *out = nullptr;
    if (c->at != DIMX_BF16) return DIMX_OK;
    auto i1 = c->host.find(w1), ib = c->host.find(b1), i2 = c->host.find(w2);
    DIMX_REQUIRE(i1 != c->host.end() && ib != c->host.end() && i2 != c->host.end(), DIMX_ERR_WEIGHT, "missing weight %s", w1.c_str());
    const int F = (int)i1->second.shape[0], C = (int)i1->second.shape[1];
    const size_t bytes = mlp_fused_packed_bytes(C, F);
    if (bytes == 0 || (int)i2->second.shape[0] != C || (int)i2->second.shape[1] != F) return DIMX_OK;   // another geometry: the GEMM form
    std::vector<uint16_t> img(bytes / 2);
    DIMX_TRY(mlp_fused_pack(i1->second.data.data(), ib->second.data.data(), i2->second.data.data(), C, F, img.data()));
    void* p;
    DIMX_TRY(dev_upload(c, img.data(), bytes, &p));
    *out = p;
    return DIMX_OK;
}

static int pack_vq(dimx_ctx* c, int which) {
    VQNet& v = c->vq[which];
    const VQGeom& vg = c->vqg[which];
    const std::string p = vq_prefix(which), e = p + "encoder.", d = p + "decoder.";
    DIMX_TRY(pack_linear(c, {e + "vertice_mapping.0.weight"}, e + "vertice_mapping.0.bias", false, &v.vm));
    DIMX_TRY(pack_linear(c, {e + "squasher.0.0.weight"}, e + "squasher.0.0.bias", true, &v.conv));
    DIMX_TRY(pack_linear(c, {e + "encoder_linear_embedding.net.weight"}, e + "encoder_linear_embedding.net.bias", false, &v.le));
    DIMX_TRY(pack_linear(c, {e + "encoder_linear_embedding_post.net.weight"}, e + "encoder_linear_embedding_post.net.bias", false, &v.post));
    if (vg.has_decoder) {
        DIMX_TRY(pack_linear(c, {d + "decoder_linear_embedding_pre.net.weight"}, d + "decoder_linear_embedding_pre.net.bias", false, &v.pre));
        DIMX_TRY(pack_linear(c, {d + "expander.0.0.weight"}, d + "expander.0.0.bias", true, &v.dconv));
        DIMX_TRY(pack_linear(c, {d + "decoder_linear_embedding.net.weight"}, d + "decoder_linear_embedding.net.bias", false, &v.dle));
        DIMX_TRY(pack_linear(c, {d + "vertice_map_reverse.weight"}, "", false, &v.rev));
    }
    for (int s = 0; s < (vg.has_decoder ? 2 : 1); ++s) {
        const std::string pre = s == 0 ? e + "encoder_transformer." : d + "decoder_transformer.";
        VQBlock* blk = s == 0 ? v.enc : v.dec;
        for (int i = 0; i < vg.layers; ++i) {
            const std::string a = pre + "net." + std::to_string(2 * i) + ".fn.";
            const std::string m = pre + "net." + std::to_string(2 * i + 1) + ".fn.";
            DIMX_TRY(upload_f32(c, a + "norm.weight", &blk[i].ln1_g));
            DIMX_TRY(upload_f32(c, a + "norm.bias", &blk[i].ln1_b));
            DIMX_TRY(pack_linear(c, {a + "fn.to_qkv.weight"}, "", false, &blk[i].qkv));
            DIMX_TRY(pack_linear(c, {a + "fn.to_out.weight"}, a + "fn.to_out.bias", false, &blk[i].out));
            DIMX_TRY(upload_f32(c, m + "norm.weight", &blk[i].ln2_g));
            DIMX_TRY(upload_f32(c, m + "norm.bias", &blk[i].ln2_b));
            DIMX_TRY(pack_linear(c, {m + "fn.l1.weight"}, m + "fn.l1.bias", false, &blk[i].l1));
            DIMX_TRY(pack_linear(c, {m + "fn.l2.weight"}, m + "fn.l2.bias", false, &blk[i].l2));
            DIMX_TRY(pack_mlp(c, m + "fn.l1.weight", m + "fn.l1.bias", m + "fn.l2.weight", &blk[i].mlp));
        }
    }
    DIMX_TRY(upload_f32(c, e + "encoder_pos_embedding.pe", &v.pe_enc));
    if (vg.has_decoder) DIMX_TRY(upload_f32(c, d + "decoder_pos_embedding.pe", &v.pe_dec));
    DIMX_TRY(upload_f32(c, p + "quantize.embedding.weight", &v.E));
    // k-major codebook + squared norms (k-ascending fmaf chain, mirrored by oracle/vq_argmin.c)
    const HostTensor& E = c->host[p + "quantize.embedding.weight"];
    const int ne = vg.n_embed, zd = vg.zdim;
    std::vector<float> Et((size_t)zd * ne), ee(ne);
    for (int j = 0; j < ne; ++j) {
        float s = 0.f;
        for (int k = 0; k < zd; ++k) {
            const float x = E.data[(size_t)j * zd + k];
            Et[(size_t)k * ne + j] = x;
            s = fmaf(x, x, s);
        }
        ee[j] = s;
    }
    void* pp;
    DIMX_TRY(dev_upload(c, Et.data(), Et.size() * 4, &pp));
    v.Et = (const float*)pp;
    DIMX_TRY(dev_upload(c, ee.data(), ee.size() * 4, &pp));
    v.ee = (const float*)pp;
    return DIMX_OK;
}

static int pack_xattn(dimx_ctx* c, const std::string& p, bool cross, XAttn* a) {
    DIMX_TRY(upload_f32(c, p + "0.0.weight", &a->ln_g));
    if (cross) {  // K/V of all layers are packed as one matrix by the caller (cross_kv_all)
        DIMX_TRY(pack_linear(c, {p + "1.to_q.weight"}, "", false, &a->qkv));
    } else {
        DIMX_TRY(pack_linear(c, {p + "1.to_q.weight", p + "1.to_k.weight", p + "1.to_v.weight"}, "", false, &a->qkv));
    }
    DIMX_TRY(pack_linear(c, {p + "1.to_out.weight"}, "", false, &a->out));
    return DIMX_OK;
}
static int pack_xff(dimx_ctx* c, const std::string& p, XFF* f) {
    DIMX_TRY(upload_f32(c, p + "0.0.weight", &f->ln_g));
    DIMX_TRY(pack_linear(c, {p + "1.ff.0.0.weight"}, p + "1.ff.0.0.bias", false, &f->f1));
    DIMX_TRY(pack_linear(c, {p + "1.ff.2.weight"}, p + "1.ff.2.bias", false, &f->f2));
    DIMX_TRY(pack_mlp(c, p + "1.ff.0.0.weight", p + "1.ff.0.0.bias", p + "1.ff.2.weight", &f->mlp));
    return DIMX_OK;
}
static int pack_xenc(dimx_ctx* c, const std::string& pre, XEnc* e) {
    DIMX_TRY(pack_linear(c, {pre + "project_in.weight"}, c->host.count(pre + "project_in.bias") ? pre + "project_in.bias" : "", false,
                         &e->proj_in));   // the bias: optional tensor ([XT?], see optional_key)
    DIMX_TRY(upload_f32(c, pre + "pos_emb.emb.weight", &e->pos_emb));
    for (int i = 0; i < c->encg[0].depth; ++i) {
        DIMX_TRY(pack_xattn(c, xl(pre, 2 * i), false, &e->attn[i]));
        DIMX_TRY(pack_xff(c, xl(pre, 2 * i + 1), &e->ff[i]));
    }
    DIMX_TRY(upload_f32(c, pre + "attn_layers.final_norm.weight", &e->final_g));
    return DIMX_OK;
}

static void free_packed(dimx_ctx* c) {
    for (void* p : c->dev_allocs) (void)hipFree(p);
    c->dev_allocs.clear();
    c->packed_mask = 0;
    ++c->dec_epoch;   // every path that rewrites decoder weights on the device comes through here and re-packs (qkv0 table)
}


static std::vector<KeySpec> comp_keys(const dimx_dims& d, int comp) {
    std::vector<KeySpec> k;
    if (comp == COMP_MESH) {
        mesh_keys(d, k);
        return k;
    }
    if (d.variant == 1) {
        if (comp == COMP_VQ0) legacy_speaker_vq_keys(d, k);
        if (comp == COMP_VQ1) vq_keys(d, 1, k);
        if (comp == COMP_ENC) xenc_keys(d, "generator.encoder.", (int64_t)d.spk_face_quan_num * d.vq_zdim, k);
        if (comp == COMP_DEC) {
            xdec_keys(d, "generator.decoder.net.", k);
            k.push_back({"generator.decoder.net.pos_emb.emb.weight", {d.max_seq_len, d.dim + d.dim_a}});
        }
        return k;
    }
    if (comp == COMP_VQ0) vq_keys(d, 0, k);
    if (comp == COMP_VQ1) vq_keys(d, 1, k);
    if (comp == COMP_ENC) {
        xenc_keys(d, "encoder_s.", d.dim_in, k);
        xenc_keys(d, "encoder_joint.", d.dim, k);
        k.push_back({"patch_embed_s", {1, 1, d.dim_in}});
        k.push_back({"patch_embed_dec_s", {1, 1, d.dim}});
        k.push_back({"norm_s.weight", {d.dim}});
        k.push_back({"norm_s.bias", {d.dim}});
        if (d.variant == 2) slm_extra_keys(d, k, 1);
    }
    if (comp == COMP_DEC) {
        xdec_keys(d, "decoder_joint.net.", k);
        if (d.variant == 2) slm_extra_keys(d, k, 2);
    }
    return k;
}

// pack the components in `need` that are not packed yet (each stage asks only for what it uses)
static int ensure_packed(dimx_ctx* c, int need) {
    if ((c->packed_mask & need) == need) return DIMX_OK;
    DIMX_HIP(hipSetDevice(c->device));
    for (int comp = 1; comp <= COMP_MESH; comp <<= 1) {
        if (!(need & comp) || (c->packed_mask & comp)) continue;
        int missing = 0;
        std::string first;
        for (const auto& k : comp_keys(c->d, comp))
            if (!c->host.count(k.name)) {
                if (!missing) first = k.name;
                ++missing;
            }
        DIMX_REQUIRE(missing == 0, DIMX_ERR_WEIGHT, "%d weights of this stage not loaded (first: %s)", missing,
                     first.c_str());
        if (comp == COMP_VQ0) DIMX_TRY(pack_vq(c, 0));
        if (comp == COMP_VQ1) DIMX_TRY(pack_vq(c, 1));
        if (comp == COMP_ENC && c->variant == 1) {
            DIMX_TRY(pack_xenc(c, "generator.encoder.", &c->enc_s));
        } else if (comp == COMP_ENC) {
            DIMX_TRY(pack_xenc(c, "encoder_s.", &c->enc_s));
            DIMX_TRY(pack_xenc(c, "encoder_joint.", &c->enc_joint));
            DIMX_TRY(upload_f32(c, "patch_embed_s", &c->patch_s));
            DIMX_TRY(upload_f32(c, "patch_embed_dec_s", &c->patch_dec_s));
            DIMX_TRY(upload_f32(c, "norm_s.weight", &c->norm_s_g));
            DIMX_TRY(upload_f32(c, "norm_s.bias", &c->norm_s_b));
            if (c->variant == 2) {
                DIMX_TRY(pack_xenc(c, "encoder_l.", &c->enc_l));
                DIMX_TRY(upload_f32(c, "patch_embed_l", &c->patch_l));
                DIMX_TRY(upload_f32(c, "patch_embed_dec_l", &c->patch_dec_l));
                DIMX_TRY(upload_f32(c, "norm_l.weight", &c->norm_l_g));
                DIMX_TRY(upload_f32(c, "norm_l.bias", &c->norm_l_b));
                DIMX_TRY(upload_f32(c, "norm.weight", &c->norm_j_g));
                DIMX_TRY(upload_f32(c, "norm.bias", &c->norm_j_b));
            }
        }
        if (comp == COMP_DEC) {
            const std::string dp = c->variant == 1 ? "generator.decoder.net." : "decoder_joint.net.";
            if (c->decg.abs_pos) DIMX_TRY(upload_f32(c, dp + "pos_emb.emb.weight", &c->dec.pos_emb));
            DIMX_TRY(upload_f32(c, dp + "token_emb.emb.weight", &c->dec.tok_emb));
            for (int i = 0; i < c->decg.depth; ++i) {
                DIMX_TRY(pack_xattn(c, xl(dp, 3 * i), false, &c->dec.self_[i]));
                DIMX_TRY(pack_xattn(c, xl(dp, 3 * i + 1), true, &c->dec.cross[i]));
                DIMX_TRY(pack_xff(c, xl(dp, 3 * i + 2), &c->dec.ff[i]));
                // the projections of the decode step (M = clips) in the parity mode: bf16 planes for gemm_x3_kernel (the cross K/V
                // projection, M = clips x frames, stays on the f32 MFMA kernel)
                DIMX_TRY(make_x3(c, &c->dec.self_[i].qkv));
                DIMX_TRY(make_x3(c, &c->dec.self_[i].out));
                DIMX_TRY(make_x3(c, &c->dec.cross[i].qkv));
                DIMX_TRY(make_x3(c, &c->dec.cross[i].out));
                DIMX_TRY(make_x3(c, &c->dec.ff[i].f1));
                DIMX_TRY(make_x3(c, &c->dec.ff[i].f2));
                if (c->at == DIMX_BF16 && c->decg.dim % 64 == 0) {
                    const std::string cp = xl(dp, 3 * i + 1), fp = xl(dp, 3 * i + 2);
                    DIMX_TRY(pack_linear_scaled(c, cp + "1.to_q.weight", cp + "0.0.weight", "", &c->dec.cross[i].q_ln,
                                                &c->dec.cross[i].q_ln_colsum));
                    DIMX_TRY(pack_linear_scaled(c, fp + "1.ff.0.0.weight", fp + "0.0.weight", fp + "1.ff.0.0.bias",
                                                &c->dec.ff[i].f1_ln, &c->dec.ff[i].f1_ln_colsum));
                }
            }
            DIMX_TRY(upload_f32(c, dp + "attn_layers.final_norm.weight", &c->dec.final_g));
            DIMX_TRY(pack_linear(c, {dp + "to_logits.weight"}, c->host.count(dp + "to_logits.bias") ? dp + "to_logits.bias" : "", false,
                                 &c->dec.logits));
            DIMX_TRY(make_x3(c, &c->dec.logits));
            {
                std::vector<std::string> parts;
                for (int i = 0; i < c->decg.depth; ++i) {
                    parts.push_back(xl(dp, 3 * i + 1) + "1.to_k.weight");
                    parts.push_back(xl(dp, 3 * i + 1) + "1.to_v.weight");
                }
                DIMX_TRY(pack_linear(c, parts, "", false, &c->dec.cross_kv_all));
                const Linear& all = c->dec.cross_kv_all;
                const int per = all.N / c->decg.depth;
                for (int i = 0; i < c->decg.depth; ++i) {
                    Linear& kv = c->dec.cross[i].kv;
                    kv = all;
                    kv.N = per;
                    kv.w = (unsigned char*)all.w + (size_t)i * per * all.Kp * dtype_size(c->at);
                }
            }
        }
        if (comp == COMP_MESH) {
            const std::string p = "vertice_map_reverse_lstm.";
            for (int l = 0; l < 2; ++l)
                for (int dir = 0; dir < 2; ++dir) {
                    const std::string sfx = "_l" + std::to_string(l) + lstm_suffix(dir);
                    DIMX_TRY(upload_f32(c, p + "weight_ih" + sfx, &c->mesh.w_ih[l][dir]));
                    DIMX_TRY(upload_f32(c, p + "weight_hh" + sfx, &c->mesh.w_hh[l][dir]));
                    DIMX_TRY(upload_f32(c, p + "bias_ih" + sfx, &c->mesh.b_ih[l][dir]));
                    DIMX_TRY(upload_f32(c, p + "bias_hh" + sfx, &c->mesh.b_hh[l][dir]));
                }
            DIMX_TRY(pack_linear(c, {"vertice_map_reverse.0.weight"}, "vertice_map_reverse.0.bias", false, &c->mesh.l1));
            DIMX_TRY(pack_linear(c, {"vertice_map_reverse.2.weight"}, "vertice_map_reverse.2.bias", false, &c->mesh.l2));
        }
        c->packed_mask |= comp;
        if (comp == COMP_DEC) ++c->dec_epoch;
    }
    c->graph_valid = false;
    return DIMX_OK;
}

// the positional buffers of VQ-VAE slot `which` (packed on first use): the VQ-VAE training step (train.hip) adds them
int vq_pe_buffers(dimx_ctx* c, int which, const float** pe_enc, const float** pe_dec) {
    DIMX_REQUIRE(which == 0 || which == 1, DIMX_ERR_ARG, "vq_pe_buffers: which must be 0 or 1");
    DIMX_HIP(hipSetDevice(c->device));
    DIMX_TRY(ensure_packed(c, which == 0 ? COMP_VQ0 : COMP_VQ1));
    *pe_enc = c->vq[which].pe_enc;
    *pe_dec = c->vq[which].pe_dec;
    return DIMX_OK;
}

// ------------------------------------------------------------------ small helpers

int gemm_lin(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, GemmArgs& g) {
    gemm_args_init(g);
    g.in_dtype = c->at;
    g.A = A;
    g.lda = lda;
    g.W = L.w;
    g.ldw = L.Kp;
    g.M = M;
    g.N = L.N;
    g.K = L.K;
    g.bias = L.bias;
    g.allow_splitk = c->at == DIMX_BF16 ? 1 : 0;  // parity mode keeps a fixed summation order
    g.w3 = L.w3;
    g.w3_plane = (long)L.N * L.Kp;
    return DIMX_OK;
}

// Perf mode (round 3): V leaves the fused q/k/v projection row-major like q and k -- three row-contiguous destinations, which
// is what the two-phase 256 x 256 GEMM stores -- and the attention of attention_tr.hip reads it that way.  The f32 parity mode
// and the 96-column heads of the legacy speaker VQ-VAE keep the transposed destination.
bool qkv_row_v(int at, int D) {
    return at == DIMX_BF16 && D <= 64;
}

// q / k row-major [M, segw]; v transposed [B,H,D,Tp], or row-major too (rowv)
static void set_qkv_out(GemmArgs& g, void* q, void* k, void* vt, int T, int H, int D, int Tp, bool rowv = false) {
    const int segw = H * D;
    g.rowT = T;
    g.nseg = 3;
    g.seg_width = segw;
    for (int i = 0; i < (rowv ? 3 : 2); ++i) {
        g.seg[i].ptr = i == 0 ? q : (i == 1 ? k : vt);
        g.seg[i].sb = (long)T * segw;
        g.seg[i].st = segw;
        g.seg[i].sh = D;
        g.seg[i].sd = 1;
        g.seg[i].D = D;
    }
    if (rowv) return;
    g.seg[2].ptr = vt;
    g.seg[2].sb = (long)H * D * Tp;
    g.seg[2].sh = (long)D * Tp;
    g.seg[2].sd = Tp;
    g.seg[2].st = 1;
    g.seg[2].D = D;
}

void set_attn_packed(AttnArgs& a, int dtype, const void* q, const void* k, const void* vt, void* o, int B,
                            int H, int Lq, int Lk, int D, int Tp_k, bool rowv) {
    memset(&a, 0, sizeof(a));
    const int segw = H * D;
    a.dtype = dtype;
    a.q = q;
    a.k = k;
    a.vt = vt;
    a.o = o;
    a.q_sb = (long)Lq * segw;
    a.q_st = segw;
    a.q_sh = D;
    a.k_sb = (long)Lk * segw;
    a.k_st = segw;
    a.k_sh = D;
    a.v_sb = (long)H * D * Tp_k;
    a.v_sh = (long)D * Tp_k;
    a.v_sd = Tp_k;
    if (rowv) {
        a.v_rows = 1;
        a.v_sb = (long)Lk * segw;
        a.v_st = segw;
        a.v_sh = D;
    }
    a.o_sb = (long)Lq * segw;
    a.o_st = segw;
    a.o_sh = D;
    a.B = B;
    a.H = H;
    a.Lq = Lq;
    a.Lk = Lk;
    a.D = D;
}

// ------------------------------------------------------------------ sublayers of a transformer block
// The four stacks (run_vq_blocks, run_xenc, dimx_decode_tf, generate.hip's gen_prefill) are sequences of these calls over the
// buffers of a block (BlockBufs, stages.hpp).

// out[M, ldo] = act(A . W^T + bias) (+ residual [M, ldo], f32) as plain rows of out_dtype
int linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, int out_dtype, void* out, int ldo, hipStream_t st, int act,
           const float* residual) {
    GemmArgs g;
    gemm_lin(c, A, lda, L, M, g);
    g.out_dtype = out_dtype; g.act = act;
    g.residual = residual; g.ldr = residual ? ldo : 0;
    gemm_set_plain_out(g, out, ldo);
    return launch_gemm(g, st);
}
// h[M, ld] += A . W^T (+ bias), f32
int residual_linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, float* h, int ld, hipStream_t st) {
    return linear(c, A, lda, L, M, DIMX_F32, h, ld, st, ACT_NONE, h);
}

// below this many rows a fused-MLP launch leaves most CUs idle (one block = 128 rows): the GEMM form's 64 x 64 tiles spread better
constexpr int kFusedMlpMinRows = 8192;

// h += f2(act(f1(LayerNorm(h)))); with mlp (the weights as mlp_fused.hip chunk images; the decoder stacks pass nullptr) and
// kFusedMlpMinRows rows the whole sublayer is one launch
int ff_sublayer(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& f1,
                       const Linear& f2, const void* mlp, int act, int M, int C, hipStream_t st) {
    if (mlp && M >= kFusedMlpMinRows) return launch_mlp_fused(b.h, mlp, f2.bias, ln_g, ln_b, M, C, f1.N, act, st);
    DIMX_TRY(launch_layernorm(c->at, b.h, b.y, ln_g, ln_b, M, C, st));
    DIMX_TRY(linear(c, b.y, C, f1, M, c->at, b.f, f1.N, st, act));
    return residual_linear(c, b.f, f1.N, f2, M, b.h, C, st);
}

// Self attention, first half: LayerNorm -> fused q/k/v projection into b.q / b.k / b.vt.  `a` leaves as the attention over them;
// the caller adds scale and its stack's mask fields (lens, kmask / kmask_ld, causal) and hands it to attn_out.
int self_attn_qkv(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& qkv, int B,
                         int T, int C, int heads, int D, AttnArgs& a, hipStream_t st) {
    const bool rowv = qkv_row_v(c->at, D);
    DIMX_TRY(launch_layernorm(c->at, b.h, b.y, ln_g, ln_b, B * T, C, st));
    GemmArgs g;
    gemm_lin(c, b.y, C, qkv, B * T, g);
    g.out_dtype = c->at;
    set_qkv_out(g, b.q, b.k, b.vt, T, heads, D, tpad(T), rowv);
    DIMX_TRY(launch_gemm(g, st));
    set_attn_packed(a, c->at, b.q, b.k, b.vt, b.o, B, heads, T, T, D, tpad(T), rowv);
    return DIMX_OK;
}

// second half of both attentions: attention `a` (output b.o) -> h += o . Wout^T (+ bias)
int attn_out(const dimx_ctx* c, const BlockBufs& b, AttnArgs& a, const Linear& out, int C, hipStream_t st) {
    a.kwords = b.kw; a.kwords_cap = b.kw_cap;
    DIMX_TRY(launch_attention(a, st));
    return residual_linear(c, b.o, a.H * a.D, out, a.B * a.Lq, b.h, C, st);
}

// Cross attention of the decoder stacks: LayerNorm -> q projection into b.q -> attention over the context K / V, which the caller
// describes in `a` -> out-projection.  v_rows (gen_prefill, f32): V [B*H, Tp, 64] to transpose into the scratch a.vt before the attention.
int cross_attn_sublayer(const dimx_ctx* c, const BlockBufs& b, const XAttn& x, AttnArgs& a, const uint8_t* ctx_mask, int C,
                               hipStream_t st, const float* v_rows) {
    const int M = a.B * a.Lq, Tp = tpad(a.Lk);
    DIMX_TRY(launch_layernorm(c->at, b.h, b.y, x.ln_g, nullptr, M, C, st));
    DIMX_TRY(linear(c, b.y, C, x.qkv, M, c->at, b.q, a.H * a.D, st));
    if (v_rows) DIMX_TRY(launch_kv_rows_to_vt(v_rows, Tp, (float*)a.vt, Tp, a.B, a.Lk, a.H, st));
    a.scale = 1.0f / sqrtf((float)a.D); a.kmask = ctx_mask; a.kmask_ld = a.Lk;
    return attn_out(c, b, a, x.out, C, st);
}

// The f32 query rows [B * n, inner] of a windowed cross attention (win_attn.hip) in a decoder stack's block buffers: the self
// attention's k | vt, which a layer's cross attention no longer needs and which lie back to back in the arena (k: B * n rows, vt:
// B * tpad(n)), hold two operand-type rows per query row -- one f32 row.  nullptr if a plan ever stops laying them out that way.
float* win_q_rows(const BlockBufs& b, int B, int n, int inner, size_t es) {
    const unsigned char *lo = (const unsigned char*)b.k, *hi = (const unsigned char*)b.vt + (size_t)B * inner * tpad(n) * es;
    return lo && b.vt && lo < hi && (size_t)(hi - lo) >= (size_t)B * n * inner * 4 ? (float*)b.k : nullptr;
}

// ------------------------------------------------------------------ VQ-VAE stacks
struct VQScratch : BlockBufs {
    void *xa, *h1;
    float *conv, *z;
    int32_t* idx_tmp;
};

static void plan_vq(const dimx_ctx* c, const VQGeom& vg, Arena& ar, int B, int T, VQScratch& s) {
    const size_t M = (size_t)B * T, es = es_of(c);
    const int H = vg.hidden, I = vg.inter, Tp = tpad(T);
    s.xa = ar.take(M * (vg.in_pad > 128 ? vg.in_pad : 128) * es);  // padded input or codebook rows (128)
    s.h1 = ar.take(M * H * es);
    s.conv = (float*)ar.take(M * H * 4);
    s.y = ar.take(M * H * es);
    s.h = (float*)ar.take(M * H * 4);
    s.q = ar.take(M * H * es);
    s.k = ar.take(M * H * es);
    s.vt = ar.take((size_t)B * H * Tp * es);
    s.o = ar.take(M * H * es);
    s.f = ar.take(M * I * es);
    s.z = (float*)ar.take(M * vg.out_dim * 4);
    s.idx_tmp = (int32_t*)ar.take(M * vg.fqn * 4);
}

static int run_vq_blocks(const dimx_ctx* c, const VQGeom& vg, const VQBlock* blk, VQScratch& s, int B, int T,
                         const int32_t* lens, hipStream_t st) {
    const int M = B * T, Hd = vg.hidden, heads = vg.heads, D = Hd / heads;
    const float scale = 1.0f / sqrtf((float)Hd);  // hidden^-0.5 (code/models/lib/base_models.py:116)
    for (int l = 0; l < vg.layers; ++l) {
        const VQBlock& b = blk[l];
        AttnArgs a;
        DIMX_TRY(self_attn_qkv(c, s, b.ln1_g, b.ln1_b, b.qkv, B, T, Hd, heads, D, a, st));
        a.scale = scale; a.lens = lens;
        DIMX_TRY(attn_out(c, s, a, b.out, Hd, st));
        DIMX_TRY(ff_sublayer(c, s, b.ln2_g, b.ln2_b, b.l1, b.l2, b.mlp, ACT_GELU_TANH, M, Hd, st));
    }
    return DIMX_OK;
}

// conv(k5, replicate) + LeakyReLU -> InstanceNorm -> Linear + bias + positional row -> s.h
static int run_vq_front(const dimx_ctx* c, const VQGeom& vg, const void* x_in, int ld_in, const Linear& conv,
                        const Linear& le, const float* pe, int pe_mode, int row_off, VQScratch& s, int B, int T,
                        const int32_t* lens, hipStream_t st, int row_div = 1) {
    const int M = B * T, Hd = vg.hidden;
    GemmArgs g;
    gemm_lin(c, x_in, ld_in, conv, M, g);
    g.conv_T = T;
    g.conv_lens = lens;
    g.conv_C = Hd;
    g.act = ACT_LEAKY;
    g.out_dtype = DIMX_F32;
    gemm_set_plain_out(g, s.conv, Hd);
    DIMX_TRY(launch_gemm(g, st));
    DIMX_TRY(launch_instnorm(c->at, s.conv, s.y, lens, B, T, Hd, st));
    gemm_lin(c, s.y, Hd, le, M, g);
    g.out_dtype = DIMX_F32;
    g.rowT = T;
    g.rowadd = pe;
    g.ld_rowadd = Hd;
    g.rowadd_mode = pe_mode == 0 ? 3 : 2;
    g.rowadd_off = pe_mode == 0 ? 0 : row_off;
    g.rowadd_div = row_div;
    gemm_set_plain_out(g, s.h, Hd);
    DIMX_TRY(launch_gemm(g, st));
    return DIMX_OK;
}

// features -> z [B*T, out_dim] -> nearest codebook row of every zdim-wide group: idx [B*T*fqn]
// (code/models/stage1_BIWI.py:152-157 speaker, :282-302 listener; quantizer.py:52-60)
static int run_vq_encode(const dimx_ctx* c, int which, const float* x, const int32_t* lens, int B, int T, int pe_mode,
                         int row_off, VQScratch& s, float* z, int32_t* idx, hipStream_t st) {
    const VQGeom& vg = c->vqg[which];
    const VQNet& v = c->vq[which];
    const int M = B * T, Hd = vg.hidden;
    DIMX_TRY(launch_cast_pad(c->at, x, vg.in_dim, nullptr, s.xa, vg.in_pad, M, vg.in_dim, st));
    DIMX_TRY(linear(c, s.xa, vg.in_pad, v.vm, M, c->at, s.h1, Hd, st, ACT_LEAKY));
    DIMX_TRY(run_vq_front(c, vg, s.h1, Hd, v.conv, v.le, v.pe_enc, pe_mode, row_off, s, B, T, lens, st));
    DIMX_TRY(run_vq_blocks(c, vg, v.enc, s, B, T, lens, st));
    // post projection consumes the f32 residual stream directly (no final norm in this stack)
    DIMX_TRY(launch_cast_pad(c->at, s.h, Hd, nullptr, s.y, Hd, M, Hd, st));
    DIMX_TRY(linear(c, s.y, Hd, v.post, M, DIMX_F32, z, vg.out_dim, st));
    DIMX_TRY(launch_vq_argmin(z, M * vg.fqn, v.Et, v.ee, idx, nullptr, nullptr, st));
    return DIMX_OK;
}

}  // namespace dimx

using namespace dimx;

// ====================================================================== C-ABI
extern "C" {

int dimx_version(void) { return 100; }
const char* dimx_last_error(void) { return get_error(); }

void dimx_legacy_dims(dimx_dims* d) {
    if (!d) return;
    dimx_default_dims(d);
    d->variant = 1;
    d->dim_in = 1024; d->dim = 512; d->dim_a = 0; d->enc_depth = 6; d->dec_depth = 6; d->heads = 8;
    d->max_seq_len = 1024;
    d->spk_in_dim = 824; d->spk_hidden = 768; d->spk_heads = 8; d->spk_inter = 1536; d->spk_face_quan_num = 8;
}

void dimx_default_dims(dimx_dims* d) {
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->vq_in_dim = 56; d->vq_hidden = 384; d->vq_layers = 6; d->vq_heads = 8; d->vq_inter = 1536;
    d->vq_n_embed = 512; d->vq_zdim = 128;
    d->dim_in = 56; d->dim = 384; d->dim_a = 768; d->enc_depth = 4; d->dec_depth = 4; d->heads = 12;
    d->dim_head = 64; d->num_tokens = 512; d->max_seq_len = 2048; d->ff_mult = 4;
}

int dimx_create(dimx_handle* h, int device_id, const dimx_dims* dims, int numeric_mode) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "dimx_create: null handle pointer");
    DIMX_REQUIRE(numeric_mode == DIMX_MODE_PARITY_F32 || numeric_mode == DIMX_MODE_PERF_BF16, DIMX_ERR_ARG,
                 "dimx_create: numeric_mode %d", numeric_mode);
    dimx_dims d;
    dimx_default_dims(&d);
    if (dims) d = *dims;
    DIMX_REQUIRE(d.vq_hidden == 384 && d.vq_heads == 8 && d.vq_zdim == 128 && d.vq_n_embed == 512 && d.vq_in_dim == 56,
                 DIMX_ERR_ARG, "dimx_create: only the DIM-Listener VQ geometry (56/384/8/128/512) is built");
    if (d.variant == 0 || d.variant == 2) {
        DIMX_REQUIRE(d.dim == 384 && d.dim_a == 768 && d.dim_head == 64 && d.heads == 12 && d.num_tokens == 512 &&
                         d.vq_layers <= 8 && d.enc_depth <= 8 && d.dec_depth <= 8 && d.max_seq_len <= 2048,
                     DIMX_ERR_ARG, "dimx_create: only the SLMFT geometry (384+768, 12x64, 512 tokens) is built");
    } else {
        DIMX_REQUIRE(d.variant == 1 && d.dim == 512 && d.dim_a == 0 && d.dim_head == 64 && d.heads == 8 &&
                         d.num_tokens == 512 && d.enc_depth <= 8 && d.dec_depth <= 8 && d.max_seq_len <= 2048 &&
                         d.spk_hidden == 768 && d.spk_heads == 8 && d.spk_in_dim == 824 && d.spk_face_quan_num == 8,
                     DIMX_ERR_ARG, "dimx_create: only the legacy ListenerGenerator geometry (824/768 VQ, 512, 8x64) is built");
    }
    DIMX_REQUIRE(d.mesh_dim == 0 || (d.variant == 2 && d.mesh_dim > 0), DIMX_ERR_ARG,
                 "dimx_create: the mesh head (mesh_dim %d) belongs to a handle of variant 2", d.mesh_dim);
    int ndev = 0;
    DIMX_HIP(hipGetDeviceCount(&ndev));
    DIMX_REQUIRE(device_id >= 0 && device_id < ndev, DIMX_ERR_ARG, "dimx_create: device %d of %d", device_id, ndev);
    DIMX_HIP(hipSetDevice(device_id));
    dimx_ctx* c = new dimx_ctx();
    c->device = device_id;
    c->d = d;
    c->mode = numeric_mode;
    c->at = numeric_mode == DIMX_MODE_PERF_BF16 ? DIMX_BF16 : DIMX_F32;
    c->variant = d.variant;
    const VQGeom lvq = {d.vq_in_dim, 64, d.vq_hidden, d.vq_heads, d.vq_inter, d.vq_layers, d.vq_zdim, 1, d.vq_zdim,
                        d.vq_n_embed, true};
    c->vqg[0] = c->vqg[1] = lvq;
    if (d.variant == 1) {
        c->vqg[0] = {d.spk_in_dim, (d.spk_in_dim + 63) / 64 * 64, d.spk_hidden, d.spk_heads, d.spk_inter, d.vq_layers,
                     d.spk_face_quan_num * d.vq_zdim, d.spk_face_quan_num, d.vq_zdim, d.vq_n_embed, false};
        const int din = d.spk_face_quan_num * d.vq_zdim;
        c->encg[0] = c->encg[1] = {din, din, d.dim, d.heads, d.dim_head, d.enc_depth, d.ff_mult, 0};
        c->decg = {d.dim, d.heads, d.dim_head, d.dec_depth, d.ff_mult, 1, d.num_tokens, d.dim};
    } else {
        // SLMFT: causal encoders (attn_mask, :435), decoder without positional embedding (:386);
        // SLM (variant 2): mask-only (bidirectional) encoders (:213-218), decoder with abs. pos. embedding (:131)
        const int causal = d.variant == 2 ? 0 : 1, abs_pos = d.variant == 2 ? 1 : 0;
        c->encg[0] = {d.dim_in, 64, d.dim, d.heads, d.dim_head, d.enc_depth, d.ff_mult, causal};
        c->encg[1] = {d.dim, d.dim, d.dim, d.heads, d.dim_head, d.enc_depth, d.ff_mult, causal};
        c->decg = {d.dim + d.dim_a, d.heads, d.dim_head, d.dec_depth, d.ff_mult, abs_pos, d.num_tokens, d.dim + d.dim_a};
    }
    for (const auto& k : all_keys(d)) c->required.push_back(k.name);
    const char* ng = getenv("DIMX_NO_GRAPH");
    c->use_graph = (ng && ng[0] == '1') ? 0 : 1;
    const char* nc = getenv("DIMX_NO_CHAIN");
    c->use_chain = (nc && nc[0] == '1') ? 0 : 1;
    c->use_layer_chain = getenv("DIMX_NO_LAYER_CHAIN") ? 0 : 1;
    c->multi_tr = getenv("DIMX_NO_MULTI_TR") ? 0 : 1;
    c->use_qkv0_table = getenv("DIMX_NO_QKV0_TABLE") ? 0 : 1;
    c->use_kv0_table = getenv("DIMX_NO_KV0_TABLE") ? 0 : 1;
    c->use_sample_head = getenv("DIMX_NO_SAMPLE_HEAD") ? 0 : 1;
    if (getenv("DIMX_LAYER_PROF")) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)8 * 256 * 16 * 8) == hipSuccess) {
            (void)hipMemset(p, 0, (size_t)8 * 256 * 16 * 8);
            c->layer_prof_dev = (unsigned long long*)p;
        }
    }
    if (const char* pg = getenv("DIMX_PREFILL_GROUPS")) {
        const int v = atoi(pg);
        if (v >= 1 && v <= dimx_ctx::kPreGroups) c->prefill_groups = v;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess) c->cu_count = cus;
    }
    const char* gg = getenv("DIMX_GEN_GROUPS");
    if (gg && atoi(gg) >= 1 && atoi(gg) <= dimx_ctx::kMaxGroups) c->gen_groups = atoi(gg);
    *h = c;
    return DIMX_OK;
}

int dimx_destroy(dimx_handle h) {
    if (!h) return DIMX_OK;
    (void)hipSetDevice(h->device);
    for (int g = 0; g < dimx_ctx::kMaxGroups; ++g) {
        if (h->graph_multi[g]) (void)hipGraphExecDestroy(h->graph_multi[g]);
        if (h->graph_exec[g]) (void)hipGraphExecDestroy(h->graph_exec[g]);
        if (h->grp_stream[g]) (void)hipStreamDestroy(h->grp_stream[g]);
        if (h->ev_join[g]) (void)hipEventDestroy(h->ev_join[g]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (int g = 0; g < dimx_ctx::kPreGroups - 1; ++g) {
        if (h->pre_stream[g]) (void)hipStreamDestroy(h->pre_stream[g]);
        if (h->pre_join[g]) (void)hipEventDestroy(h->pre_join[g]);
    }
    if (h->pre_fork) (void)hipEventDestroy(h->pre_fork);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->chain_err_ev) (void)hipEventDestroy(h->chain_err_ev);
    if (h->chain_err_dev) (void)hipFree(h->chain_err_dev);
    if (h->chain_stats_dev) (void)hipFree(h->chain_stats_dev);
    if (h->layer_prof_dev) (void)hipFree(h->layer_prof_dev);
    if (h->qkv0_table) (void)hipFree(h->qkv0_table);
    if (h->kv0_image) (void)hipFree(h->kv0_image);
    if (h->chain_err_host) (void)hipHostFree(h->chain_err_host);
    free_packed(h);
    stream_forget(h);  // an open streaming session
    train_forget(h);   // the training plan cached for this handle (a later handle may reuse the address)
    delete h;
    return DIMX_OK;
}

int dimx_numeric_mode(dimx_handle h) { return h ? h->mode : DIMX_ERR_ARG; }

int dimx_set_shard(dimx_handle h, int row_offset, int rows_total) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "set_shard: null handle");
    DIMX_REQUIRE(row_offset >= 0 && (rows_total == 0 || rows_total > row_offset), DIMX_ERR_ARG,
                 "set_shard: row_offset %d, rows_total %d", row_offset, rows_total);
    h->shard_row_off = row_offset;
    h->shard_rows_total = rows_total;
    return DIMX_OK;
}

// A new checkpoint begins: the OPTIONAL tensors an earlier checkpoint brought (project_in.bias / to_logits.bias, SURVEY A.2 [XT?])
// are forgotten; required tensors stay until they are overwritten.  dimx_load_weights itself never drops a tensor (round 6, ADVICE
// round 5: it used to forget a bias when a later call named the Linear's weight without it, which made a chunked or key-sorted
// loader's result depend on the order of its calls).
int dimx_begin_checkpoint(dimx_handle h) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "dimx_begin_checkpoint: null handle");
    std::set<std::string> spec;
    for (const auto& k : all_keys(h->d)) spec.insert(k.name);
    bool dirty = false;
    for (auto it = h->host.begin(); it != h->host.end();) {
        if (!spec.count(it->first)) {
            it = h->host.erase(it);
            dirty = true;
        } else {
            ++it;
        }
    }
    if (dirty) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        free_packed(h);
        h->graph_valid = false;
        h->ctx_ready = false;
    }
    return DIMX_OK;
}

int dimx_load_weights(dimx_handle h, const dimx_weight_desc* descs, int n) {
    DIMX_REQUIRE(h && descs && n >= 0, DIMX_ERR_ARG, "dimx_load_weights: null argument");
    static thread_local std::map<std::string, std::vector<int64_t>> spec;
    spec.clear();
    for (const auto& k : all_keys(h->d)) spec[k.name] = k.shape;
    bool dirty = false;
    for (int i = 0; i < n; ++i) {
        const dimx_weight_desc& w = descs[i];
        DIMX_REQUIRE(w.name && w.data && w.ndim >= 1 && w.ndim <= 4, DIMX_ERR_ARG, "dimx_load_weights: bad desc %d", i);
        const std::string name(w.name);
        auto it = spec.find(name);
        if (it == spec.end()) {
            std::vector<int64_t> oshape;
            const int opt = optional_key(spec, name, &oshape);
            if (opt != OPT_NONE) {
                DIMX_REQUIRE(w.ndim == 1 && w.shape[0] == oshape[0], DIMX_ERR_WEIGHT, "%s: expected %lld values", w.name, (long long)oshape[0]);
                if (opt == OPT_NORM_BIAS) {
                    for (int64_t k = 0; k < w.shape[0]; ++k)
                        DIMX_REQUIRE(w.data[k] == 0.f, DIMX_ERR_WEIGHT,
                                     "%s: a non-zero LayerNorm bias -- this x-transformers variant is not the one the path implements", w.name);
                    continue;
                }
                HostTensor& t = h->host[name];
                t.shape.assign(w.shape, w.shape + 1);
                t.data.assign(w.data, w.data + w.shape[0]);
                dirty = true;
                continue;
            }
            DIMX_REQUIRE(ignorable_key(name), DIMX_ERR_WEIGHT, "unknown weight key %s", w.name);
            // the speaker-id embedding stays on the host side of inference; only its row count is kept (dimx_train_spk_*)
            if (name == "speaker_embed.weight" && w.ndim == 2 && w.shape[1] == h->d.dim && w.shape[0] >= 1 && w.shape[0] <= (1 << 20))
                h->spk_embed_rows = (int)w.shape[0];
            continue;
        }
        DIMX_REQUIRE((int)it->second.size() == w.ndim, DIMX_ERR_WEIGHT, "%s: rank %d, expected %d", w.name, w.ndim,
                     (int)it->second.size());
        size_t cnt = 1;
        for (int k = 0; k < w.ndim; ++k) {
            DIMX_REQUIRE(it->second[k] == w.shape[k], DIMX_ERR_WEIGHT, "%s: dim %d is %lld, expected %lld", w.name, k,
                         (long long)w.shape[k], (long long)it->second[k]);
            cnt *= (size_t)w.shape[k];
        }
        HostTensor& t = h->host[name];
        t.shape.assign(w.shape, w.shape + w.ndim);
        t.data.assign(w.data, w.data + cnt);
        dirty = true;
    }
    if (dirty) {  // re-pack lazily; device copies of the old tensors are released now
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        free_packed(h);
        h->graph_valid = false;
        h->ctx_ready = false;
    }
    return DIMX_OK;
}

int dimx_missing_weights(dimx_handle h) {
    if (!h) return DIMX_ERR_ARG;
    int m = 0;
    for (const auto& k : h->required) m += h->host.count(k) ? 0 : 1;
    return m;
}

}  // extern "C"

// ====================================================================== stages
namespace dimx {

struct EncScratch : BlockBufs {
    void* xa;
    float* tmp;
};
struct DecScratch : BlockBufs {
    int32_t *inp, *tgt;
    uint8_t* kvm;
};

static void plan_persist(const dimx_ctx* c, Arena& ar, int B, int T, CtxPersist& p) {
    const size_t es = es_of(c);
    const size_t per = (size_t)B * c->decg.heads * c->decg.dim_head * tpad(T) * es;
    for (int l = 0; l < c->decg.depth; ++l) {
        p.ck[l] = ar.take(per);
        p.cv[l] = ar.take(per);
    }
}
static void plan_enc(const dimx_ctx* c, Arena& ar, int B, int T, EncScratch& s) {
    const size_t M = (size_t)B * T, es = es_of(c);
    const EncGeom& eg = c->encg[0];
    const int dim = eg.dim, inner = eg.heads * eg.dim_head, Tp = tpad(T);
    const int wide = c->decg.ctx_dim > eg.in_pad ? c->decg.ctx_dim : eg.in_pad;
    s.xa = ar.take(M * wide * es);  // padded encoder input, later the decoder's cross-attention context
    s.h = (float*)ar.take(M * dim * 4);
    s.tmp = (float*)ar.take(M * dim * 4);
    s.y = ar.take(M * dim * es);
    s.q = ar.take(M * inner * es);
    s.k = ar.take(M * inner * es);
    s.vt = ar.take((size_t)B * inner * Tp * es);
    s.o = ar.take(M * inner * es);
    s.f = ar.take(M * dim * eg.ff_mult * es);
    s.kw_cap = (size_t)B * ((T + 63) / 64);
    s.kw = (unsigned long long*)ar.take(s.kw_cap * 8);
}
static void plan_dec(const dimx_ctx* c, Arena& ar, int B, int T, DecScratch& s) {
    const int n = T - 1;
    const size_t M = (size_t)B * n, es = es_of(c);
    const int D = c->decg.dim, inner = c->decg.heads * c->decg.dim_head, np = tpad(n);
    s.h = (float*)ar.take(M * D * 4);
    s.y = ar.take(M * D * es);
    s.q = ar.take(M * inner * es);
    s.k = ar.take(M * inner * es);
    s.vt = ar.take((size_t)B * inner * np * es);
    s.o = ar.take(M * inner * es);
    s.f = ar.take(M * D * c->decg.ff_mult * es);
    s.inp = (int32_t*)ar.take(M * 4);
    s.tgt = (int32_t*)ar.take(M * 4);
    s.kvm = (uint8_t*)ar.take(M);
    s.kw_cap = (size_t)B * ((T + 63) / 64);
    s.kw = (unsigned long long*)ar.take(s.kw_cap * 8);
}
void plan_gen(const dimx_ctx* c, Arena& ar, int B, int T, GenScratch& s) {
    const size_t es = es_of(c);
    const int D = c->decg.dim, inner = c->decg.heads * c->decg.dim_head;
    const size_t per = (size_t)B * inner * T * es;
    for (int l = 0; l < c->decg.depth; ++l) {
        s.sk[l] = ar.take(per);
        s.sv[l] = ar.take(per);
    }
    s.x = (float*)ar.take((size_t)B * D * 4);
    s.y = ar.take((size_t)B * D * es);
    constexpr int kMaxSlabs = 8;
    s.st_qkv = (long)B * 3 * inner;
    s.st_qc = (long)B * inner;
    s.st_xr = (long)B * D;
    s.st_lg = (long)B * c->decg.num_tokens;
    s.qkv = (float*)ar.take((size_t)kMaxSlabs * s.st_qkv * 4);
    s.qc = (float*)ar.take((size_t)kMaxSlabs * s.st_qc * 4);
    s.xr = (float*)ar.take((size_t)kMaxSlabs * s.st_xr * 4);
    s.o = ar.take((size_t)B * inner * es);
    s.f = ar.take((size_t)B * D * c->decg.ff_mult * es);
    s.logits = (float*)ar.take((size_t)kMaxSlabs * B * c->decg.num_tokens * 4);
    s.step = (int32_t*)ar.take(64 * dimx_ctx::kMaxGroups);  // one counter per clip group, 64 B apart
    s.chain_ctr = (unsigned*)ar.take((size_t)kChainSites * kChainSiteWords * 4);
    s.qcb = ar.take((size_t)B * inner * es);
    s.kw_cap = (size_t)B * ((T + 63) / 64);
    s.kw = (unsigned long long*)ar.take(s.kw_cap * 8);
    s.hist = (int32_t*)ar.take((size_t)B * T * 4);
}

// The scratch is sized for the WHOLE batch (B clips x n0 positions), not for a chunk of clips, and lies behind the generation
// scratch: the prefill writes the K/V cache, which must outlive it, and nothing else of the generation scratch.
void plan_prefill(const dimx_ctx* c, Arena& ar, int B, int n0, int T, PrefillScratch& s) {
    const size_t M = (size_t)B * n0, es = es_of(c);
    const int D = c->decg.dim, inner = c->decg.heads * c->decg.dim_head, np = tpad(n0);
    s.h = (float*)ar.take(M * D * 4);
    s.y = ar.take(M * D * es);
    s.q = ar.take(M * inner * es);
    s.k = ar.take(M * inner * es);
    s.vt = ar.take((size_t)B * inner * np * es);
    s.o = ar.take(M * inner * es);
    s.f = ar.take(M * D * c->decg.ff_mult * es);
    s.inp = (int32_t*)ar.take(M * 4);
    s.kw_cap = (size_t)B * ((T + 63) / 64);
    s.kw = (unsigned long long*)ar.take(s.kw_cap * 8);
    s.cvt = c->at == DIMX_BF16 ? nullptr : (float*)ar.take((size_t)B * inner * tpad(T) * 4);
}

// SLM.forward_encoder: the encoder scratch is sized for the joint 2T pass; xs / xl keep the two first-stage
// outputs (operand type), xj their time-concatenation, m2 the doubled padding mask
struct MeshScratch {
    float *y0, *y1;
    void *a, *l1;
    void* lstm;
    size_t lstm_bytes;
};
static void plan_mesh(const dimx_ctx* c, Arena& ar, int B, int L, MeshScratch& s) {
    const size_t M = (size_t)B * L, W = 768;
    s.y0 = (float*)ar.take(M * W * 4);
    s.y1 = (float*)ar.take(M * W * 4);
    s.a = c->at == DIMX_BF16 ? ar.take(M * W * 2) : nullptr;
    s.l1 = ar.take(M * W * dtype_size(c->at));
    const size_t b0 = lstm_scratch_bytes(B, L, c->d.vq_in_dim), b1 = lstm_scratch_bytes(B, L, (int)W);
    s.lstm_bytes = b0 > b1 ? b0 : b1;
    s.lstm = ar.take(s.lstm_bytes);
}

struct SlmScratch {
    EncScratch e;
    void *xs, *xl, *xj;
    uint8_t* m2;
};
static void plan_slm(const dimx_ctx* c, Arena& ar, int B, int T, SlmScratch& s) {
    const size_t es = es_of(c);
    plan_enc(c, ar, B, 2 * T, s.e);
    s.xs = ar.take((size_t)B * T * c->encg[0].dim * es);
    s.xl = ar.take((size_t)B * T * c->encg[0].dim * es);
    s.xj = ar.take((size_t)B * 2 * T * c->encg[0].dim * es);
    s.m2 = (uint8_t*)ar.take((size_t)B * 2 * T);
}

static size_t workspace_bytes(const dimx_ctx* c, int B, int T, int S = 1) {
    Arena p(nullptr, 0);
    CtxPersist cp;
    plan_persist(c, p, B, T, cp);
    const size_t persist = align_up(p.off, 256);
    size_t scratch = 0;
    for (int w = 0; w < 2; ++w) {
        Arena a(nullptr, 0);
        VQScratch s;
        plan_vq(c, c->vqg[w], a, B, T, s);
        scratch = a.off > scratch ? a.off : scratch;
    }
    {
        Arena a(nullptr, 0);
        EncScratch s;
        plan_enc(c, a, B, T, s);
        if (c->variant == 0) a.take((size_t)B * T * c->decg.ctx_dim * es_of(c));  // the shared context buffer of dimx_encode_ctx's clip groups
        if (c->variant == 1) {  // the speaker VQ-VAE runs inside encode_ctx, next to the encoder buffers
            VQScratch v;
            plan_vq(c, c->vqg[0], a, B, T, v);
            a.take((size_t)B * 4);
        }
        scratch = a.off > scratch ? a.off : scratch;
    }
    if (c->variant == 2) {
        Arena a(nullptr, 0);
        SlmScratch s;
        plan_slm(c, a, B, T, s);
        scratch = a.off > scratch ? a.off : scratch;
    }
    if (c->d.mesh_dim > 0) {
        Arena a(nullptr, 0);
        MeshScratch s;
        plan_mesh(c, a, B, T, s);
        scratch = a.off > scratch ? a.off : scratch;
    }
    if (T >= 2) {
        Arena a(nullptr, 0);
        DecScratch s;
        plan_dec(c, a, B, T, s);
        scratch = a.off > scratch ? a.off : scratch;
        Arena g(nullptr, 0);
        GenScratch gs;
        plan_gen(c, g, B * S, T, gs);
        scratch = g.off > scratch ? g.off : scratch;
    }
    // + 64 KiB: the prefill stages plan their scratch once per clip group (ClipGroups below), every buffer 256-byte aligned
    return persist + align_up(scratch, 256) + 4096 + 65536;
}

// workspace of dimx_encode_ctx(for_generate = 1) + a prompted generation that prefills P0 - 1 positions: the generation
// scratch and the prefill scratch behind it
size_t workspace_bytes_prompt(const dimx_ctx* c, int B, int T, int S, int P0) {
    const size_t base = workspace_bytes(c, B, T, S);
    if (P0 <= 1 || T < 2) return base;
    Arena p(nullptr, 0);
    CtxPersist cp;
    plan_persist(c, p, B, T, cp);
    Arena g(nullptr, 0);
    GenScratch gs;
    plan_gen(c, g, B * S, T, gs);
    PrefillScratch ps;
    plan_prefill(c, g, B, P0 - 1, T, ps);
    const size_t need = align_up(p.off, 256) + align_up(g.off, 256) + 4096 + 65536;
    return need > base ? need : base;
}

// x-transformers encoder stack (ContinuousTransformerWrapper, return_embeddings=True)
static int run_xenc(const dimx_ctx* c, const EncGeom& eg, const XEnc& e, const void* x_in, int ld_in, EncScratch& s,
                    int B, int T, const uint8_t* mask, int out_dtype, void* out, hipStream_t st) {
    const int M = B * T, dim = eg.dim, heads = eg.heads, D = eg.dim_head;
    GemmArgs g;
    gemm_lin(c, x_in, ld_in, e.proj_in, M, g);
    g.out_dtype = DIMX_F32;
    g.rowT = T;
    g.rowadd = e.pos_emb;
    g.ld_rowadd = dim;
    g.rowadd_mode = 1;
    g.rowadd_scale = 1.0f / sqrtf((float)dim);
    gemm_set_plain_out(g, s.h, dim);
    DIMX_TRY(launch_gemm(g, st));
    for (int l = 0; l < eg.depth; ++l) {
        AttnArgs a;
        DIMX_TRY(self_attn_qkv(c, s, e.attn[l].ln_g, nullptr, e.attn[l].qkv, B, T, dim, heads, D, a, st));
        a.scale = 1.0f / sqrtf((float)D); a.causal = eg.causal; a.kmask = mask; a.kmask_ld = T;
        DIMX_TRY(attn_out(c, s, a, e.attn[l].out, dim, st));
        DIMX_TRY(ff_sublayer(c, s, e.ff[l].ln_g, nullptr, e.ff[l].f1, e.ff[l].f2, e.ff[l].mlp, ACT_GELU_ERF, M, dim, st));
    }
    DIMX_TRY(launch_layernorm(out_dtype, s.h, out, e.final_g, nullptr, M, dim, st));
    return DIMX_OK;
}

int check_common(dimx_handle h, int B, int T, void* ws, size_t ws_bytes, int need, int S) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(B >= 1 && T >= 1 && T <= h->d.max_seq_len, DIMX_ERR_ARG, "B=%d T=%d out of range (T <= %d)", B, T,
                 h->d.max_seq_len);
    DIMX_REQUIRE(ws && ((uintptr_t)ws % 256) == 0, DIMX_ERR_ARG, "workspace must be 256-byte aligned");
    const size_t need_bytes = workspace_bytes(h, B, T, S);
    DIMX_REQUIRE(ws_bytes >= need_bytes, DIMX_ERR_WORKSPACE, "workspace %zu < required %zu", ws_bytes, need_bytes);
    DIMX_HIP(hipSetDevice(h->device));
    DIMX_TRY(ensure_packed(h, need));
    return DIMX_OK;
}

int project_cross_kv(dimx_handle h, const void* ctx, const CtxPersist& cp, int B, int T, int for_generate,
                     hipStream_t st);
int legacy_encode_ctx(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T, int for_generate,
                      float* enc_out, float* x_speaker_out, int32_t* idx_out, void* ws, size_t ws_bytes,
                      hipStream_t st);

// The prefill-sized stages of a forward are independent per clip, and their kernels leave CUs idle at the end of every launch (the
// fused feed-forward kernel runs 600 blocks of 128 rows on 256 CUs: the third round is a third full; 128 x 128 and 256 x 256 GEMM
// tiles end the same way).  As G clip groups on G streams the tails of one group's kernels are filled by another group's blocks:
// 15.8 -> 14.2 ms for the three stages at 256 x 300 with G = 4 (profiles/r05_prefill_groups.txt).
// Group 0 runs on the caller's stream, the others on the handle's side streams between a fork and a join event; every group
// has its own scratch (the same arena, planned group by group).  Both numeric modes: a clip's results do not depend on the batch it is
// computed in (the f32 mode by contract -- test_c3_batch_and_shard_invariance compares the grouped whole batch with its shards bit for bit).
struct ClipGroups {
    int G;
    int b0[dimx_ctx::kPreGroups + 1];
    hipStream_t st[dimx_ctx::kPreGroups];
};
static int clip_groups_fork(dimx_handle h, int B, int T, hipStream_t st, ClipGroups& cg, bool one_group = false) {
    int G = one_group ? 1 : h->prefill_groups;
    if (G == 0) {
        // what the groups buy is the idle tail of every launch: nothing once a stage runs many rounds of blocks anyway (2 560
        // sequences x 299 rows, the best-of-10 protocol's VQ decode: 4 groups measured 5 % SLOWER than one batch)
        const size_t rows = (size_t)B * T;
        G = rows > 196608 ? 1 : rows >= 32768 ? 4 : rows >= 16384 ? 2 : 1;
    }
    if (G > B) G = B;
    cg.G = G;
    for (int g = 0; g <= G; ++g) cg.b0[g] = (int)((long)B * g / G);
    cg.st[0] = st;
    if (G == 1) return DIMX_OK;
    {
        // a stream that is being captured keeps one batch (a query would invalidate the capture)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            cg.G = 1;
            cg.b0[1] = B;
            return DIMX_OK;
        }
        // The side streams must not sit behind the fork event for long: with a whole generation still queued on the caller's
        // stream (the best-of-10 pass, no host synchronisation between forwards: 600 ms) the following generation ran 5 % slower
        // (3 580 against 3 820 sequences/s, profiles/r05_prefill_groups.txt).  So when the caller's stream still has work in
        // flight the call waits for it here, on the host, and forks from an idle stream; the stage's own launches then run ahead
        // of the GPU as before.
        if (hipStreamQuery(st) != hipSuccess) (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
    }
    if (!h->pre_fork) DIMX_HIP(hipEventCreateWithFlags(&h->pre_fork, hipEventDisableTiming));
    DIMX_HIP(hipEventRecord(h->pre_fork, st));
    for (int g = 1; g < G; ++g) {
        if (!h->pre_stream[g - 1]) DIMX_HIP(hipStreamCreateWithFlags(&h->pre_stream[g - 1], hipStreamNonBlocking));
        if (!h->pre_join[g - 1]) DIMX_HIP(hipEventCreateWithFlags(&h->pre_join[g - 1], hipEventDisableTiming));
        cg.st[g] = h->pre_stream[g - 1];
        DIMX_HIP(hipStreamWaitEvent(cg.st[g], h->pre_fork, 0));
    }
    return DIMX_OK;
}
static int clip_groups_join(dimx_handle h, const ClipGroups& cg) {
    hipError_t bad = hipSuccess;
    for (int g = 1; g < cg.G; ++g) {   // every side stream is joined even when one of the calls fails
        hipError_t e = hipEventRecord(h->pre_join[g - 1], cg.st[g]);
        if (e == hipSuccess) e = hipStreamWaitEvent(cg.st[0], h->pre_join[g - 1], 0);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(cg.st[g]);   // last resort: the caller's stream cannot wait for it, the host does
            bad = e;
        }
    }
    DIMX_HIP(bad);
    return DIMX_OK;
}

// join whatever the stage did: the stage's own error wins, the side streams are always folded back into the caller's stream
static int clip_groups_close(dimx_handle h, const ClipGroups& cg, int rc) {
    const int jrc = clip_groups_join(h, cg);
    return rc != DIMX_OK ? rc : jrc;
}

Arena scratch_arena(const dimx_ctx* c, void* ws, size_t ws_bytes, int B, int T, CtxPersist* cp) {
    Arena p(ws, ws_bytes);
    CtxPersist tmp;
    plan_persist(c, p, B, T, cp ? *cp : tmp);
    const size_t persist = align_up(p.off, 256);
    return Arena((unsigned char*)ws + persist, ws_bytes - persist);
}

}  // namespace dimx

extern "C" {

size_t dimx_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1 || T > h->d.max_seq_len) return 0;  // 0 = shape not supported
    return workspace_bytes(h, B, T);
}

size_t dimx_workspace_bytes_samples(dimx_handle h, int B, int T, int n_samples) {
    if (!h || B < 1 || T < 1 || n_samples < 1 || T > h->d.max_seq_len) return 0;
    return workspace_bytes(h, B, T, n_samples);
}

size_t dimx_workspace_bytes_prompt(dimx_handle h, int B, int T, int n_samples, int P0) {
    if (!h || B < 1 || T < 1 || n_samples < 1 || T > h->d.max_seq_len || P0 < 1 || P0 > (T > 1 ? T - 1 : 1)) return 0;
    return workspace_bytes_prompt(h, B, T, n_samples, P0);
}

size_t dimx_workspace_bytes_guided(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 2 || T > h->d.max_seq_len) return 0;
    return workspace_bytes(h, B, T, 2);   // the persistent part (cross K / V) for B clips, the generation scratch (self caches) for 2B rows
}

int dimx_vq_argmin(dimx_handle h, int which, const float* z, int N, int32_t* idx, float* best_d, float* margin,
                   void* stream) {
    DIMX_REQUIRE(h && (which == 0 || which == 1), DIMX_ERR_ARG, "vq_argmin: bad handle/which");
    DIMX_HIP(hipSetDevice(h->device));
    DIMX_TRY(ensure_packed(h, which == 0 ? COMP_VQ0 : COMP_VQ1));
    return launch_vq_argmin(z, N, h->vq[which].Et, h->vq[which].ee, idx, best_d, margin, (hipStream_t)stream);
}

int dimx_vq_encode(dimx_handle h, int which, const float* x, const int32_t* lens, int B, int T, int pe_mode,
                   int batch_row_offset, int32_t pad_value, int32_t* idx, float* z_out, void* ws, size_t ws_bytes,
                   void* stream) {
    DIMX_REQUIRE(which == 0 || which == 1, DIMX_ERR_ARG, "vq_encode: which must be 0 or 1");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, which == 0 ? COMP_VQ0 : COMP_VQ1));
    DIMX_REQUIRE(x && idx, DIMX_ERR_ARG, "vq_encode: null argument");
    DIMX_REQUIRE(pe_mode == 0 || B + batch_row_offset <= 5000, DIMX_ERR_ARG, "vq_encode: positional row out of range");
    hipStream_t st = (hipStream_t)stream;
    const VQGeom& vg = h->vqg[which];
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, nullptr);
    ClipGroups cg;
    DIMX_TRY(clip_groups_fork(h, B, T, st, cg));
    VQScratch s[dimx_ctx::kPreGroups];
    for (int g = 0; g < cg.G; ++g) plan_vq(h, vg, ar, cg.b0[g + 1] - cg.b0[g], T, s[g]);
    // from the fork on every return goes through the join (an error between the two left the side streams
    // writing into a workspace the caller may free)
    const int rc = [&]() -> int {
        DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "vq_encode: workspace overflow");
        for (int g = 0; g < cg.G; ++g) {
            const int b0 = cg.b0[g], nb = cg.b0[g + 1] - b0;
            const size_t r0 = (size_t)b0 * T;
            DIMX_TRY(run_vq_encode(h, which, x + r0 * vg.in_dim, lens ? lens + b0 : nullptr, nb, T, pe_mode, batch_row_offset + b0, s[g],
                                   z_out ? z_out + r0 * vg.out_dim : s[g].z, idx + r0 * vg.fqn, cg.st[g]));
        }
        return DIMX_OK;
    }();
    DIMX_TRY(clip_groups_close(h, cg, rc));
    DIMX_TRY(launch_finalize_idx(idx, lens, B, T, pad_value, st, vg.fqn));
    return DIMX_OK;
}

// shared body of dimx_vq_decode (codebook rows gathered from idx) and dimx_vq_decode_latent (z given)
static int vq_decode_impl(dimx_handle h, int which, const int32_t* idx, const float* z, int B, int L,
                          int batch_row_offset, int rows_per_clip, float* out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(which == 0 || which == 1, DIMX_ERR_ARG, "vq_decode: which must be 0 or 1");
    DIMX_TRY(check_common(h, B, L, ws, ws_bytes, which == 0 ? COMP_VQ0 : COMP_VQ1));
    DIMX_REQUIRE((idx || z) && out, DIMX_ERR_ARG, "vq_decode: null argument");
    DIMX_REQUIRE(B + batch_row_offset <= 5000 && batch_row_offset >= 0, DIMX_ERR_ARG,
                 "vq_decode: positional row %d out of range", B + batch_row_offset);
    hipStream_t st = (hipStream_t)stream;
    const VQNet& v = h->vq[which];
    const VQGeom& vg = h->vqg[which];
    DIMX_REQUIRE(vg.has_decoder, DIMX_ERR_ARG, "vq_decode: this variant's VQ-VAE %d has no decoder on the path", which);
    DIMX_REQUIRE(rows_per_clip >= 1, DIMX_ERR_ARG, "vq_decode: rows_per_clip must be >= 1");
    Arena ar = scratch_arena(h, ws, ws_bytes, B, L, nullptr);
    ClipGroups cg;
    if (rows_per_clip == 1) {
        DIMX_TRY(clip_groups_fork(h, B, L, st, cg));
    } else {  // several rows share a clip's positional row: one batch (the groups would have to be cut at clip boundaries)
        cg.G = 1;
        cg.b0[0] = 0;
        cg.b0[1] = B;
        cg.st[0] = st;
    }
    VQScratch sg[dimx_ctx::kPreGroups];
    for (int g = 0; g < cg.G; ++g) plan_vq(h, vg, ar, cg.b0[g + 1] - cg.b0[g], L, sg[g]);
    const int Hd = vg.hidden, zd = vg.zdim;
    const int rc = [&]() -> int {
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "vq_decode: workspace overflow");
    for (int gi = 0; gi < cg.G; ++gi) {
        VQScratch& s = sg[gi];
        hipStream_t gs = cg.st[gi];
        const int b0 = cg.b0[gi], nb = cg.b0[gi + 1] - b0, M = nb * L;
        const size_t r0 = (size_t)b0 * L;
        if (idx)
            DIMX_TRY(launch_gather_rows(h->at, v.E, zd, vg.n_embed, idx + r0, s.xa, zd, M, zd, gs));
        else
            DIMX_TRY(launch_cast_pad(h->at, z + r0 * zd, zd, nullptr, s.xa, zd, M, zd, gs));
        DIMX_TRY(linear(h, s.xa, zd, v.pre, M, h->at, s.h1, Hd, gs));
        DIMX_TRY(run_vq_front(h, vg, s.h1, Hd, v.dconv, v.dle, v.pe_dec, 1, batch_row_offset + b0, s, nb, L, nullptr, gs, rows_per_clip));
        DIMX_TRY(run_vq_blocks(h, vg, v.dec, s, nb, L, nullptr, gs));
        DIMX_TRY(launch_cast_pad(h->at, s.h, Hd, nullptr, s.y, Hd, M, Hd, gs));
        DIMX_TRY(linear(h, s.y, Hd, v.rev, M, DIMX_F32, out + r0 * vg.in_dim, vg.in_dim, gs));
    }
    return DIMX_OK;
    }();
    return clip_groups_close(h, cg, rc);
}

int dimx_vq_decode(dimx_handle h, int which, const int32_t* idx, int B, int L, int batch_row_offset, int rows_per_clip,
                   float* out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(idx, DIMX_ERR_ARG, "vq_decode: null argument");
    return vq_decode_impl(h, which, idx, nullptr, B, L, batch_row_offset, rows_per_clip, out, ws, ws_bytes, stream);
}

int dimx_vq_decode_latent(dimx_handle h, int which, const float* z, int B, int L, int batch_row_offset, float* out,
                          void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(z, DIMX_ERR_ARG, "vq_decode_latent: null argument");
    return vq_decode_impl(h, which, nullptr, z, B, L, batch_row_offset, 1, out, ws, ws_bytes, stream);
}

// SLMFT.forward_encoder alone (code/seq2seq_pretrain.py:431-442): x_s = norm_s(encoder_joint(encoder_s(v + patch)))
int dimx_encode_speaker(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T, float* x_s_out, void* ws,
                        size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && h->variant == 0, DIMX_ERR_ARG, "encode_speaker: SLMFT variant only");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_ENC));
    DIMX_REQUIRE(v_speaker && mask && x_s_out, DIMX_ERR_ARG, "encode_speaker: null argument");
    hipStream_t st = (hipStream_t)stream;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, nullptr);
    EncScratch s;
    plan_enc(h, ar, B, T, s);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "encode_speaker: workspace overflow");
    const int M = B * T, dim = h->d.dim;
    DIMX_TRY(launch_cast_pad(h->at, v_speaker, h->d.dim_in, h->patch_s, s.xa, 64, M, h->d.dim_in, st));
    DIMX_TRY(run_xenc(h, h->encg[0], h->enc_s, s.xa, 64, s, B, T, mask, h->at, s.xa, st));
    DIMX_TRY(run_xenc(h, h->encg[1], h->enc_joint, s.xa, dim, s, B, T, mask, DIMX_F32, s.tmp, st));
    DIMX_TRY(launch_layernorm(DIMX_F32, s.tmp, x_s_out, h->norm_s_g, h->norm_s_b, M, dim, st));
    h->ctx_ready = false;  // the encoder scratch overlaps a previously built context
    return DIMX_OK;
}

int dimx_encode_ctx(dimx_handle h, const float* v_speaker, const float* v_audio, const uint8_t* mask, int B, int T,
                    int for_generate, float* x_s_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_NO_SESSION(h, "encode_ctx");
    DIMX_REQUIRE(!h || h->variant != 2, DIMX_ERR_ARG,
                 "encode_ctx: the SLM variant builds its contexts with dimx_slm_encode + dimx_set_context");
    if (h && h->variant == 1)
        return legacy_encode_ctx(h, v_speaker, mask, B, T, for_generate, x_s_out, nullptr, nullptr, ws, ws_bytes,
                                 (hipStream_t)stream);
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_ENC | COMP_DEC));
    DIMX_REQUIRE(v_speaker && v_audio && mask, DIMX_ERR_ARG, "encode_ctx: null argument");
    hipStream_t st = (hipStream_t)stream;
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    const int dim = h->d.dim, dim_a = h->d.dim_a;
    // the encoders run per clip group (ClipGroups above); the context rows of all groups land in ONE [B T, ctx] buffer (the first
    // group's `xa`, sized for the whole batch) so that the K/V projection of the four decoder layers stays one launch
    ClipGroups cg;
    DIMX_TRY(clip_groups_fork(h, B, T, st, cg, h->decg.ctx_dim < h->encg[0].in_pad));  // a group's rows of `xa` are context rows
    EncScratch sg[dimx_ctx::kPreGroups];
    void* xa_all = nullptr;
    const size_t xa_row = (size_t)h->decg.ctx_dim * es_of(h);
    if (cg.G > 1) xa_all = ar.take((size_t)B * T * xa_row);
    for (int g = 0; g < cg.G; ++g) {
        plan_enc(h, ar, cg.b0[g + 1] - cg.b0[g], T, sg[g]);
        if (cg.G > 1) sg[g].xa = (unsigned char*)xa_all + (size_t)cg.b0[g] * T * xa_row;   // the group's own `xa` stays unused
    }
    const int grc = [&]() -> int {
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "encode_ctx: workspace overflow");
    for (int gi = 0; gi < cg.G; ++gi) {
        EncScratch& s = sg[gi];
        hipStream_t gs = cg.st[gi];
        const int b0 = cg.b0[gi], nb = cg.b0[gi + 1] - b0, M = nb * T;
        const size_t r0 = (size_t)b0 * T;
        const uint8_t* gmask = mask + r0;
        // v_speaker + patch_embed_s, padded 56 -> 64
        DIMX_TRY(launch_cast_pad(h->at, v_speaker + r0 * h->d.dim_in, h->d.dim_in, h->patch_s, s.xa, 64, M, h->d.dim_in, gs));
        DIMX_TRY(run_xenc(h, h->encg[0], h->enc_s, s.xa, 64, s, nb, T, gmask, h->at, s.xa, gs));  // output reuses xa
        DIMX_TRY(run_xenc(h, h->encg[1], h->enc_joint, s.xa, dim, s, nb, T, gmask, DIMX_F32, s.tmp, gs));
        // norm_s = nn.LayerNorm(dim) with bias (code/seq2seq_pretrain.py:411,441); in place when no copy is wanted
        float* x_s = x_s_out ? x_s_out + r0 * dim : (float*)s.h;
        DIMX_TRY(launch_layernorm(DIMX_F32, s.tmp, x_s, h->norm_s_g, h->norm_s_b, M, dim, gs));
        DIMX_TRY(launch_context_concat(h->at, x_s, h->patch_dec_s, v_audio + r0 * dim_a, s.xa, M, dim, dim_a, gs));
    }
    return DIMX_OK;
    }();
    DIMX_TRY(clip_groups_close(h, cg, grc));
    DIMX_TRY(project_cross_kv(h, sg[0].xa, cp, B, T, for_generate, st));
    h->ctx_ready = true;
    h->ctx_B = B;
    h->ctx_T = T;
    h->ctx_for_generate = for_generate ? 1 : 0;
    h->ctx_ws = ws;
    return DIMX_OK;
}

int dimx_legacy_speaker_features(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T,
                                 float* x_speaker_out, int32_t* idx_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && h->variant == 1, DIMX_ERR_ARG, "legacy_speaker_features: handle is not the legacy variant");
    DIMX_REQUIRE(x_speaker_out || idx_out, DIMX_ERR_ARG, "legacy_speaker_features: no output requested");
    return legacy_encode_ctx(h, v_speaker, mask, B, T, -1, nullptr, x_speaker_out, idx_out, ws, ws_bytes,
                             (hipStream_t)stream);
}

// SLM.forward_encoder (code/seq2seq_pretrain.py:200-221).  mask_speaker / mask_listener: 1 = frame masked
// (input row zeroed after the patch embedding is added).  Outputs f32: x_s, x_l [B,T,384], x_joint [B,2T,384].
int dimx_slm_encode(dimx_handle h, const float* v_speaker, const float* v_listener, const uint8_t* mask,
                    const uint8_t* mask_speaker, const uint8_t* mask_listener, int B, int T, float* x_s, float* x_l,
                    float* x_joint, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && h->variant == 2, DIMX_ERR_ARG, "slm_encode: handle is not the SLM variant");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_ENC));
    DIMX_REQUIRE(2 * T <= h->d.max_seq_len, DIMX_ERR_ARG, "slm_encode: 2T=%d exceeds max_seq_len", 2 * T);
    DIMX_REQUIRE(v_speaker && v_listener && mask && x_s && x_l && x_joint, DIMX_ERR_ARG, "slm_encode: null argument");
    hipStream_t st = (hipStream_t)stream;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, nullptr);
    SlmScratch s;
    plan_slm(h, ar, B, T, s);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "slm_encode: workspace overflow");
    const int M = B * T, dim = h->encg[0].dim;
    const size_t es = es_of(h), rowb = (size_t)T * dim * es;
    const EncGeom& e0 = h->encg[0];
    const EncGeom& e1 = h->encg[1];
    // first stage: encoder_s / encoder_l on the patch-embedded, randomly zeroed streams
    DIMX_TRY(launch_cast_pad(h->at, v_speaker, h->d.dim_in, h->patch_s, s.e.xa, e0.in_pad, M, h->d.dim_in, st, mask_speaker));
    DIMX_TRY(run_xenc(h, e0, h->enc_s, s.e.xa, e0.in_pad, s.e, B, T, mask, h->at, s.xs, st));
    DIMX_TRY(launch_cast_pad(h->at, v_listener, h->d.dim_in, h->patch_l, s.e.xa, e0.in_pad, M, h->d.dim_in, st, mask_listener));
    DIMX_TRY(run_xenc(h, e0, h->enc_l, s.e.xa, e0.in_pad, s.e, B, T, mask, h->at, s.xl, st));
    // joint pass over cat([x_s, x_l], time) with cat([mask, mask])
    DIMX_HIP(hipMemcpy2DAsync(s.xj, 2 * rowb, s.xs, rowb, rowb, B, hipMemcpyDeviceToDevice, st));
    DIMX_HIP(hipMemcpy2DAsync((unsigned char*)s.xj + rowb, 2 * rowb, s.xl, rowb, rowb, B, hipMemcpyDeviceToDevice, st));
    DIMX_HIP(hipMemcpy2DAsync(s.m2, 2 * T, mask, T, T, B, hipMemcpyDeviceToDevice, st));
    DIMX_HIP(hipMemcpy2DAsync(s.m2 + T, 2 * T, mask, T, T, B, hipMemcpyDeviceToDevice, st));
    DIMX_TRY(run_xenc(h, e1, h->enc_joint, s.xj, dim, s.e, B, 2 * T, s.m2, DIMX_F32, s.e.tmp, st));
    DIMX_TRY(launch_layernorm(DIMX_F32, s.e.tmp, x_joint, h->norm_j_g, h->norm_j_b, 2 * M, dim, st));
    // encoder_joint on each stream alone
    DIMX_TRY(run_xenc(h, e1, h->enc_joint, s.xl, dim, s.e, B, T, mask, DIMX_F32, s.e.tmp, st));
    DIMX_TRY(launch_layernorm(DIMX_F32, s.e.tmp, x_l, h->norm_l_g, h->norm_l_b, M, dim, st));
    DIMX_TRY(run_xenc(h, e1, h->enc_joint, s.xs, dim, s.e, B, T, mask, DIMX_F32, s.e.tmp, st));
    DIMX_TRY(launch_layernorm(DIMX_F32, s.e.tmp, x_s, h->norm_s_g, h->norm_s_b, M, dim, st));
    h->ctx_ready = false;
    return DIMX_OK;
}

// context = cat(x + patch_embed_dec_{s|l}, audio) -> cross K/V of every decoder layer
// (SLM.forward_decoder, code/seq2seq_pretrain.py:223-229; SLMFT :445-446).  x: [B,T,dim] f32 with row stride ldx.
int dimx_set_context(dimx_handle h, const float* x, int ldx_rows, int which_patch, const float* v_audio, int B, int T,
                     int for_generate, void* ws, size_t ws_bytes, void* stream) {
    DIMX_NO_SESSION(h, "set_context");
    DIMX_REQUIRE(h && h->variant != 1, DIMX_ERR_ARG, "set_context: not available for the legacy variant");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_ENC | COMP_DEC));
    DIMX_REQUIRE(x && v_audio && (which_patch == 0 || (which_patch == 1 && h->variant == 2)) && ldx_rows >= T,
                 DIMX_ERR_ARG, "set_context: bad argument");
    hipStream_t st = (hipStream_t)stream;
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    EncScratch s;
    plan_enc(h, ar, B, T, s);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "set_context: workspace overflow");
    const int M = B * T, dim = h->d.dim, dim_a = h->d.dim_a;
    const float* xr = x;
    if (ldx_rows != T) {  // a [B, ldx_rows, dim] tensor of which the first T rows per clip are used (x_joint halves)
        DIMX_HIP(hipMemcpy2DAsync(s.h, (size_t)T * dim * 4, x, (size_t)ldx_rows * dim * 4, (size_t)T * dim * 4, B,
                                  hipMemcpyDeviceToDevice, st));
        xr = s.h;
    }
    DIMX_TRY(launch_context_concat(h->at, xr, which_patch ? h->patch_dec_l : h->patch_dec_s, v_audio, s.xa, M, dim, dim_a, st));
    DIMX_TRY(project_cross_kv(h, s.xa, cp, B, T, for_generate, st));
    h->ctx_ready = true;
    h->ctx_B = B;
    h->ctx_T = T;
    h->ctx_for_generate = for_generate ? 1 : 0;
    h->ctx_ws = ws;
    return DIMX_OK;
}

}  // extern "C"

namespace dimx {

// K / V of every decoder layer's cross-attention from the [B*T, ctx_dim] context (row-major, operand type)
int project_cross_kv(dimx_handle h, const void* ctx, const CtxPersist& cp, int B, int T, int for_generate,
                     hipStream_t st) {
    const int M = B * T, D = h->decg.dim_head, heads = h->decg.heads, Tp = tpad(T);
    if (for_generate && h->at == DIMX_BF16 && 2 * h->decg.depth <= 8 && D % 8 == 0) {
        // every layer's K | V cache in ONE launch of the phase-pipelined kernel: the context panel is read once
        GemmArgs g;
        gemm_lin(h, ctx, h->decg.ctx_dim, h->dec.cross_kv_all, M, g);
        g.out_dtype = h->at;
        g.rowT = T;
        OutSeg segs[8];
        for (int l = 0; l < h->decg.depth; ++l)
            for (int i = 0; i < 2; ++i) {
                OutSeg& sg = segs[2 * l + i];
                sg.ptr = i == 0 ? cp.ck[l] : cp.cv[l];
                sg.sb = (long)heads * Tp * D;
                sg.sh = (long)Tp * D;
                sg.st = D;
                sg.sd = 1;
                sg.D = D;
            }
        GemmArgs probe = g;
        gemm_set_plain_out(probe, cp.ck[0], g.N);
        if (gemm256_eligible(probe)) return launch_gemm256_segs(g, segs, 2 * h->decg.depth, heads * D, st);
    }
    for (int l = 0; l < h->decg.depth; ++l) {
        GemmArgs g;
        gemm_lin(h, ctx, h->decg.ctx_dim, h->dec.cross[l].kv, M, g);
        g.out_dtype = h->at;
        g.rowT = T;
        g.nseg = 2;
        g.seg_width = heads * D;
        if (for_generate) {  // K and V both [B,H,T(p),64]
            for (int i = 0; i < 2; ++i) {
                g.seg[i].ptr = i == 0 ? cp.ck[l] : cp.cv[l];
                g.seg[i].sb = (long)heads * Tp * D;
                g.seg[i].sh = (long)Tp * D;
                g.seg[i].st = D;
                g.seg[i].sd = 1;
                g.seg[i].D = D;
            }
        } else {  // K row-major [B,T,768]; V transposed [B,H,64,Tp]
            g.seg[0].ptr = cp.ck[l];
            g.seg[0].sb = (long)T * heads * D;
            g.seg[0].st = heads * D;
            g.seg[0].sh = D;
            g.seg[0].sd = 1;
            g.seg[0].D = D;
            g.seg[1].ptr = cp.cv[l];
            g.seg[1].sb = (long)heads * D * Tp;
            g.seg[1].sh = (long)D * Tp;
            g.seg[1].sd = Tp;
            g.seg[1].st = 1;
            g.seg[1].D = D;
        }
        DIMX_TRY(launch_gemm(g, st));
    }
    return DIMX_OK;
}

// Legacy ListenerGenerator context (code/seq2seq.py:224-249): per-clip speaker VQ-VAE encode of the valid
// frames -> code vectors -> the channel-major re-view -> 6-layer bidirectional encoder -> cross K/V.
// for_generate < 0: stop after x_speaker (test hook behind dimx_legacy_speaker_features).
int legacy_encode_ctx(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T, int for_generate,
                      float* enc_out, float* x_speaker_out, int32_t* idx_out, void* ws, size_t ws_bytes,
                      hipStream_t st) {
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, for_generate < 0 ? COMP_VQ0 : (COMP_VQ0 | COMP_ENC | COMP_DEC)));
    DIMX_REQUIRE(v_speaker && mask, DIMX_ERR_ARG, "encode_ctx: null argument");
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    EncScratch s;
    VQScratch v;
    plan_enc(h, ar, B, T, s);
    plan_vq(h, h->vqg[0], ar, B, T, v);
    int32_t* lens = (int32_t*)ar.take((size_t)B * 4);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "encode_ctx: workspace overflow");
    const VQGeom& vg = h->vqg[0];
    const EncGeom& eg = h->encg[0];
    const int M = B * T;
    DIMX_TRY(launch_mask_lens(mask, lens, B, T, st));
    // batch-1 encodes in the reference -> positional row 0 for every clip (pe_mode 0)
    DIMX_TRY(run_vq_encode(h, 0, v_speaker, lens, B, T, 0, 0, v, v.z, v.idx_tmp, st));
    if (idx_out) {
        DIMX_HIP(hipMemcpyAsync(idx_out, v.idx_tmp, (size_t)M * vg.fqn * 4, hipMemcpyDeviceToDevice, st));
        DIMX_TRY(launch_finalize_idx(idx_out, lens, B, T, -100, st, vg.fqn));
    }
    if (x_speaker_out)
        DIMX_TRY(launch_legacy_scramble(DIMX_F32, h->vq[0].E, v.idx_tmp, lens, x_speaker_out, B, T, vg.fqn, vg.zdim,
                                        vg.n_embed, st));
    if (for_generate < 0) return DIMX_OK;
    DIMX_TRY(launch_legacy_scramble(h->at, h->vq[0].E, v.idx_tmp, lens, s.xa, B, T, vg.fqn, vg.zdim, vg.n_embed, st));
    // encoder output (final-normed) is the decoder context; keep an f32 copy for the caller if asked
    DIMX_TRY(run_xenc(h, eg, h->enc_s, s.xa, eg.in_pad, s, B, T, mask, h->at, s.y, st));
    if (enc_out) DIMX_TRY(launch_layernorm(DIMX_F32, s.h, enc_out, h->enc_s.final_g, nullptr, M, eg.dim, st));
    DIMX_TRY(project_cross_kv(h, s.y, cp, B, T, for_generate, st));
    h->ctx_ready = true;
    h->ctx_B = B;
    h->ctx_T = T;
    h->ctx_for_generate = for_generate ? 1 : 0;
    h->ctx_ws = ws;
    return DIMX_OK;
}

}  // namespace dimx

extern "C" {

int dimx_decode_tf(dimx_handle h, const int32_t* z_l, const uint8_t* ctx_mask, const uint8_t* kv_mask, int B, int T,
                   float* logits, float* row_loss, int32_t* argmax_tok, void* ws, size_t ws_bytes, void* stream) {
    DIMX_NO_SESSION(h, "decode_tf");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_DEC));
    DIMX_REQUIRE(z_l && ctx_mask && logits && T >= 2, DIMX_ERR_ARG, "decode_tf: null argument or T < 2");
    DIMX_REQUIRE(h->ctx_ready && h->ctx_B == B && h->ctx_T == T && h->ctx_ws == ws && !h->ctx_for_generate,
                 DIMX_ERR_STATE, "decode_tf: call dimx_encode_ctx(for_generate=0) with the same B, T, ws first");
    hipStream_t st = (hipStream_t)stream;
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    DecScratch s;
    plan_dec(h, ar, B, T, s);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "decode_tf: workspace overflow");
    const DecGeom& dg = h->decg;
    const int n = T - 1, M = B * n, DD = dg.dim, heads = dg.heads, D = dg.dim_head;
    const int Tp = tpad(T), V = dg.num_tokens;
    DIMX_TRY(launch_shift_tokens(z_l, s.inp, s.tgt, B, T, st));
    DIMX_TRY(launch_gather_rows(DIMX_F32, h->dec.tok_emb, DD, V, s.inp, s.h, DD, M, DD, st));
    if (dg.abs_pos) DIMX_TRY(launch_add_pos_rows(s.h, h->dec.pos_emb, M, n, DD, 1.0f / sqrtf((float)DD), st));
    for (int l = 0; l < dg.depth; ++l) {
        AttnArgs a;
        // causal self attention (+ AutoregressiveWrapper's random key mask)
        DIMX_TRY(self_attn_qkv(h, s, h->dec.self_[l].ln_g, nullptr, h->dec.self_[l].qkv, B, n, DD, heads, D, a, st));
        a.scale = 1.0f / sqrtf((float)D); a.causal = 1; a.kmask = kv_mask; a.kmask_ld = n;
        DIMX_TRY(attn_out(h, s, a, h->dec.self_[l].out, DD, st));
        // cross attention over the speaker context: K row-major [B,T,inner], V transposed [B,H,64,Tp] (project_cross_kv)
        set_attn_packed(a, h->at, s.q, cp.ck[l], cp.cv[l], s.o, B, heads, n, T, D, Tp);
        DIMX_TRY(cross_attn_sublayer(h, s, h->dec.cross[l], a, ctx_mask, DD, st));
        DIMX_TRY(ff_sublayer(h, s, h->dec.ff[l].ln_g, nullptr, h->dec.ff[l].f1, h->dec.ff[l].f2, nullptr, ACT_GELU_ERF, M, DD, st));
    }
    DIMX_TRY(launch_layernorm(h->at, s.h, s.y, h->dec.final_g, nullptr, M, DD, st));
    DIMX_TRY(linear(h, s.y, DD, h->dec.logits, M, DIMX_F32, logits, V, st));
    if (row_loss || argmax_tok) DIMX_TRY(launch_ce_argmax(logits, s.tgt, row_loss, argmax_tok, M, V, st));
    return DIMX_OK;
}

int dimx_decode_tf_win(dimx_handle h, const int32_t* z_l, const uint8_t* ctx_mask, int B, int T, int lookahead, float* logits,
                       float* row_loss, int32_t* argmax_tok, void* ws, size_t ws_bytes, void* stream) {
    DIMX_NO_SESSION(h, "decode_tf_win");
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_DEC));
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "decode_tf_win: implemented for variant 0 (SLMFT) only; this handle is variant %d", h->variant);
    DIMX_REQUIRE(z_l && ctx_mask && logits && T >= 2, DIMX_ERR_ARG, "decode_tf_win: null argument or T < 2");
    DIMX_REQUIRE(h->ctx_ready && h->ctx_B == B && h->ctx_T == T && h->ctx_ws == ws && h->ctx_for_generate, DIMX_ERR_STATE,
                 "decode_tf_win: call dimx_encode_ctx(for_generate=1) with the same B, T, ws first");
    hipStream_t st = (hipStream_t)stream;
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    DecScratch s;
    plan_dec(h, ar, B, T, s);
    const DecGeom& dg = h->decg;
    const int n = T - 1, M = B * n, DD = dg.dim, heads = dg.heads, D = dg.dim_head, inner = heads * D;
    const int V = dg.num_tokens;
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "decode_tf_win: workspace overflow");
    float* qf = win_q_rows(s, B, n, inner, es_of(h));
    DIMX_REQUIRE(qf, DIMX_ERR_WORKSPACE, "decode_tf_win: no room for the f32 queries");
    DIMX_REQUIRE(D == 64, DIMX_ERR_ARG, "decode_tf_win: needs 64-wide heads (dim_head %d)", D);
    DIMX_TRY(launch_shift_tokens(z_l, s.inp, s.tgt, B, T, st));
    DIMX_TRY(launch_gather_rows(DIMX_F32, h->dec.tok_emb, DD, V, s.inp, s.h, DD, M, DD, st));
    if (dg.abs_pos) DIMX_TRY(launch_add_pos_rows(s.h, h->dec.pos_emb, M, n, DD, 1.0f / sqrtf((float)DD), st));
    for (int l = 0; l < dg.depth; ++l) {
        AttnArgs a;
        DIMX_TRY(self_attn_qkv(h, s, h->dec.self_[l].ln_g, nullptr, h->dec.self_[l].qkv, B, n, DD, heads, D, a, st));
        a.scale = 1.0f / sqrtf((float)D); a.causal = 1;
        DIMX_TRY(attn_out(h, s, a, h->dec.self_[l].out, DD, st));
        // cross attention under the window: f32 queries against the generation-layout K / V [B,H,Tp,64] (win_attn.hip)
        const XAttn& x = h->dec.cross[l];
        DIMX_TRY(launch_layernorm(h->at, s.h, s.y, x.ln_g, nullptr, M, DD, st));
        DIMX_TRY(linear(h, s.y, DD, x.qkv, M, DIMX_F32, qf, inner, st));
        WinAttnArgs w;
        w.dtype = h->at;
        w.q = qf; w.ld = inner;
        w.kcache = cp.ck[l]; w.vcache = cp.cv[l]; w.Tp = tpad(T);
        w.out = s.o; w.o_ld = inner;
        w.B = B; w.H = heads; w.Lq = n; w.t0 = 0; w.n_keys = T; w.lookahead = lookahead;
        w.kmask = ctx_mask; w.kmask_ld = T;
        w.scale = 1.0f / sqrtf((float)D);
        DIMX_TRY(launch_win_attn(w, st));
        DIMX_TRY(residual_linear(h, s.o, inner, x.out, M, s.h, DD, st));
        DIMX_TRY(ff_sublayer(h, s, h->dec.ff[l].ln_g, nullptr, h->dec.ff[l].f1, h->dec.ff[l].f2, nullptr, ACT_GELU_ERF, M, DD, st));
    }
    DIMX_TRY(launch_layernorm(h->at, s.h, s.y, h->dec.final_g, nullptr, M, DD, st));
    DIMX_TRY(linear(h, s.y, DD, h->dec.logits, M, DIMX_F32, logits, V, st));
    if (row_loss || argmax_tok) DIMX_TRY(launch_ce_argmax(logits, s.tgt, row_loss, argmax_tok, M, V, st));
    return DIMX_OK;
}

int dimx_lstm_faults(dimx_handle h) { return h ? h->lstm_faults : 0; }

int dimx_mesh_head(dimx_handle h, const float* motion, const float* templ, int B, int L, float* mesh_out, int flags, void* ws,
                   size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && h->d.mesh_dim > 0, DIMX_ERR_STATE, "mesh_head: the handle was created without a mesh head (dimx_dims.mesh_dim = 0)");
    DIMX_TRY(check_common(h, B, L, ws, ws_bytes, COMP_MESH));
    DIMX_REQUIRE(motion && mesh_out, DIMX_ERR_ARG, "mesh_head: null argument");
    hipStream_t st = (hipStream_t)stream;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, L, nullptr);
    MeshScratch s;
    plan_mesh(h, ar, B, L, s);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "mesh_head: workspace overflow");
    const MeshHead& m = h->mesh;
    const int M = B * L, V = h->d.mesh_dim;
    DIMX_TRY(lstm_layer_run(motion, B, L, h->d.vq_in_dim, 384, m.w_ih[0], m.w_hh[0], m.b_ih[0], m.b_hh[0], s.y0, s.lstm, s.lstm_bytes, flags,
                            h->cu_count, &h->lstm_faults, st));
    DIMX_TRY(lstm_layer_run(s.y0, B, L, 768, 384, m.w_ih[1], m.w_hh[1], m.b_ih[1], m.b_hh[1], s.y1, s.lstm, s.lstm_bytes, flags, h->cu_count,
                            &h->lstm_faults, st));
    const void* A = s.y1;
    if (h->at == DIMX_BF16) {
        DIMX_TRY(launch_cast_pad(h->at, s.y1, 768, nullptr, s.a, 768, M, 768, st));
        A = s.a;
    }
    GemmArgs g;
    DIMX_TRY(linear(h, A, 768, m.l1, M, h->at, s.l1, 768, st, ACT_LEAKY));
    // N = mesh_dim is no multiple of any tile (70110 % 4 = 2): the kernels clamp the W rows they load to N - 1 and store no
    // column >= N, the staged and 256 x 256 epilogues (N % 4 / N % 8) are not taken; the template row of the clip rides the epilogue
    gemm_lin(h, s.l1, 768, m.l2, M, g);
    g.out_dtype = DIMX_F32;
    g.rowT = L;
    if (templ) {
        g.rowadd = templ;
        g.ld_rowadd = V;
        g.rowadd_mode = 2;
        g.rowadd_off = 0;
    }
    gemm_set_plain_out(g, mesh_out, V);
    DIMX_TRY(launch_gemm(g, st));
    return DIMX_OK;
}

}  // extern "C"
