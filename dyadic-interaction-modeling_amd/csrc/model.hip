// model.hip -- handle, weight packing and the stage-level entry points of libdimx_hip.
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

#include "model.hpp"

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

enum { COMP_VQ0 = 1, COMP_VQ1 = 2, COMP_ENC = 4, COMP_DEC = 8, COMP_ALL = 15, COMP_MESH = 16 };

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
static inline size_t es_of(const dimx_ctx* c) { return dtype_size(c->at); }
static inline int tpad(int T) { return (T + 7) / 8 * 8; }

static int gemm_lin(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, GemmArgs& g) {
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
static bool qkv_row_v(int at, int D) {
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

static void set_attn_packed(AttnArgs& a, int dtype, const void* q, const void* k, const void* vt, void* o, int B,
                            int H, int Lq, int Lk, int D, int Tp_k, bool rowv = false) {
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
// The four stacks (run_vq_blocks, run_xenc, dimx_decode_tf, gen_prefill) are sequences of these calls.  The buffers of a block, the
// base of every stack's scratch struct: the f32 residual stream h [M, C]; in the operand type the LayerNorm output y, q / k / v(t),
// the attention output o and the feed-forward hidden f; kw: the packed key-mask words of the prefill attention (AttnArgs.kwords)
struct BlockBufs {
    float* h;
    void *y, *q, *k, *vt, *o, *f;
    unsigned long long* kw = nullptr;   // the VQ stacks have none
    size_t kw_cap = 0;
};

// out[M, ldo] = act(A . W^T + bias) (+ residual [M, ldo], f32) as plain rows of out_dtype
static int linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, int out_dtype, void* out, int ldo, hipStream_t st,
                  int act = ACT_NONE, const float* residual = nullptr) {
    GemmArgs g;
    gemm_lin(c, A, lda, L, M, g);
    g.out_dtype = out_dtype; g.act = act;
    g.residual = residual; g.ldr = residual ? ldo : 0;
    gemm_set_plain_out(g, out, ldo);
    return launch_gemm(g, st);
}
// h[M, ld] += A . W^T (+ bias), f32
static int residual_linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, float* h, int ld, hipStream_t st) {
    return linear(c, A, lda, L, M, DIMX_F32, h, ld, st, ACT_NONE, h);
}

// below this many rows a fused-MLP launch leaves most CUs idle (one block = 128 rows): the GEMM form's 64 x 64 tiles spread better
constexpr int kFusedMlpMinRows = 8192;

// h += f2(act(f1(LayerNorm(h)))); with mlp (the weights as mlp_fused.hip chunk images; the decoder stacks pass nullptr) and
// kFusedMlpMinRows rows the whole sublayer is one launch
static int ff_sublayer(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& f1,
                       const Linear& f2, const void* mlp, int act, int M, int C, hipStream_t st) {
    if (mlp && M >= kFusedMlpMinRows) return launch_mlp_fused(b.h, mlp, f2.bias, ln_g, ln_b, M, C, f1.N, act, st);
    DIMX_TRY(launch_layernorm(c->at, b.h, b.y, ln_g, ln_b, M, C, st));
    DIMX_TRY(linear(c, b.y, C, f1, M, c->at, b.f, f1.N, st, act));
    return residual_linear(c, b.f, f1.N, f2, M, b.h, C, st);
}

// Self attention, first half: LayerNorm -> fused q/k/v projection into b.q / b.k / b.vt.  `a` leaves as the attention over them;
// the caller adds scale and its stack's mask fields (lens, kmask / kmask_ld, causal) and hands it to attn_out.
static int self_attn_qkv(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& qkv, int B,
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
static int attn_out(const dimx_ctx* c, const BlockBufs& b, AttnArgs& a, const Linear& out, int C, hipStream_t st) {
    a.kwords = b.kw; a.kwords_cap = b.kw_cap;
    DIMX_TRY(launch_attention(a, st));
    return residual_linear(c, b.o, a.H * a.D, out, a.B * a.Lq, b.h, C, st);
}

// Cross attention of the decoder stacks: LayerNorm -> q projection into b.q -> attention over the context K / V, which the caller
// describes in `a` -> out-projection.  v_rows (gen_prefill, f32): V [B*H, Tp, 64] to transpose into the scratch a.vt before the attention.
static int cross_attn_sublayer(const dimx_ctx* c, const BlockBufs& b, const XAttn& x, AttnArgs& a, const uint8_t* ctx_mask, int C,
                               hipStream_t st, const float* v_rows = nullptr) {
    const int M = a.B * a.Lq, Tp = tpad(a.Lk);
    DIMX_TRY(launch_layernorm(c->at, b.h, b.y, x.ln_g, nullptr, M, C, st));
    DIMX_TRY(linear(c, b.y, C, x.qkv, M, c->at, b.q, a.H * a.D, st));
    if (v_rows) DIMX_TRY(launch_kv_rows_to_vt(v_rows, Tp, (float*)a.vt, Tp, a.B, a.Lk, a.H, st));
    a.scale = 1.0f / sqrtf((float)a.D); a.kmask = ctx_mask; a.kmask_ld = a.Lk;
    return attn_out(c, b, a, x.out, C, st);
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
struct CtxPersist {
    void* ck[8];
    void* cv[8];
};
struct DecScratch : BlockBufs {
    int32_t *inp, *tgt;
    uint8_t* kvm;
};
struct GenScratch {
    void* sk[8];
    void* sv[8];
    float *x, *logits;
    void *y, *o, *f;
    float *qkv, *qc, *xr;  // f32 split-K slabs [kMaxSlabs][B, N] of the qkv / cross-q / residual projections
    long st_qkv, st_qc, st_xr, st_lg;  // slab strides (elements)
    int32_t* step;
    unsigned* chain_ctr;  // [kChainSites][8][16] per-XCD arrival counters of the chain launch sites
    void* qcb;                 // several samples per clip, bf16: the cross-attention queries [rows, inner] in the operand type
    unsigned long long* kw;    // ... and the context mask as 64-bit validity words [clips][ceil(T / 64)] (attention_tr.hip)
    size_t kw_cap;
    int32_t* hist;             // [rows][T] the first layer's input token of every position (its self attention's table form)
};
constexpr int kChainSites = 32;
constexpr int kChainSiteWords = 8 * 16 + 8 * 32;  // arrival counters [8][16] + claim stamps [8][32]

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
// number of decoder positions: SLMFT feeds / generates T-1 tokens (code/seq2seq_pretrain.py:469,500);
// the legacy generator is teacher-forced on T-1 tokens but generates seq_len = T (code/seq2seq.py:256,300)
static inline int gen_steps(const dimx_ctx* c, int T) { return c->variant == 1 ? T : T - 1; }
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
static void plan_gen(const dimx_ctx* c, Arena& ar, int B, int T, GenScratch& s) {
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

// Prompted generation (dimx_generate_prompted): the prompt of a call and the teacher-forced scratch of its prefill.
// dimx_generate is the ld = Pmax = 1, step0 = 0 case.
struct GenPrompt {
    const int32_t* tok;  // [B, ld] the prompt's tokens, one row per CLIP
    int ld, Pmax;
    const int32_t* len;  // [B] prompt lengths (clamped to [step0 + 1, Pmax] by the sampler) or nullptr = Pmax
    int step0;           // P0 - 1: positions 0 .. step0 - 1 are prefilled, the first decode step is step0
};
struct PrefillScratch : BlockBufs {
    float* cvt;          // f32 mode: one layer's context V transposed to [B,H,64,Tp] (the f32 prefill attention reads V^T)
    int32_t* inp;
};
// The scratch is sized for the WHOLE batch (B clips x n0 positions), not for a chunk of clips, and lies behind the generation
// scratch: the prefill writes the K/V cache, which must outlive it, and nothing else of the generation scratch.
static void plan_prefill(const dimx_ctx* c, Arena& ar, int B, int n0, int T, PrefillScratch& s) {
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
static size_t workspace_bytes_prompt(const dimx_ctx* c, int B, int T, int S, int P0) {
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

static int check_common(dimx_handle h, int B, int T, void* ws, size_t ws_bytes, int need, int S = 1) {
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

static Arena scratch_arena(const dimx_ctx* c, void* ws, size_t ws_bytes, int B, int T, CtxPersist* cp) {
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

}  // extern "C"

namespace dimx {

static void chain_desc(ChainGemmDesc& d, const Linear& L) { d.W = L.w; d.N = L.N; d.K = L.K; d.ldw = L.Kp; }

// The chain kernels run when: bf16 operands, one sample per clip, a single clip group, <= 256 rows, a 256-CU device on
// which the placement probe passed, and every launch site's LDS plan fits.
static bool gen_use_chain(dimx_handle h, int B, int S, int grp) {
    if (!h->use_chain || h->at != DIMX_BF16 || S != 1 || grp != 0 || h->gen_groups > 1 || !h->chain_err_dev) return false;
    const DecGeom& dg = h->decg;
    ChainArgs c;
    memset(&c, 0, sizeof(c));
    c.B = B;
    c.C = dg.dim;
    const XAttn& sa = h->dec.self_[0];
    const XAttn& ca = h->dec.cross[0];
    chain_desc(c.g1, sa.out);
    c.lda1 = dg.heads * dg.dim_head;
    chain_desc(c.g2, ca.qkv);
    if (!chain_supported(c, h->cu_count)) return false;
    chain_desc(c.g2, h->dec.logits);
    c.g1.W = nullptr;
    return chain_supported(c, h->cu_count) && 3 * dg.depth + 1 <= kChainSites;
}

// several samples per clip in the bf16 mode: the decode cross attention runs on attention_tr.hip (64-wide heads)
static bool gen_multi_tr(dimx_handle h, int S) {
    return S > 1 && h->multi_tr && h->at == DIMX_BF16 && h->decg.dim_head == 64;
}

// Every projection of the decode step whose output is a small [B, N] f32 matrix is a split-K GEMM writing per-split slabs;
// the consumer (LayerNorm / attention / sampler) adds the slabs in order: deterministic, no atomics, and
// the residual add rides along in the pre-norm kernel.
static int slab_gemm_rows(dimx_handle h, int B, hipStream_t st, const void* A, int lda, const Linear& L, float* out, long stride,
                          int* nsl) {
    GemmArgs g;
    gemm_lin(h, A, lda, L, B, g);
    g.x3_decode = 1;   // f32 parity mode: the split-bf16 kernel, whatever B is
    g.out_dtype = DIMX_F32;
    g.out_slabs = 1;
    // round 4: the f32 parity mode splits K too.  Slabs are plain stores added in slab order by the consumer -- deterministic,
    // no atomics -- which is all "fixed summation order" asks for; without the split the mode's 64 x 64 tiles left most of
    // the chip idle (M = 256: 72 blocks for the 1152-wide projections, 48 for cross-q, 32 for the logits; the K = 4608
    // feed-forward projection ran 144 k-tiles on 72 CUs = 70 us): 261 of the mode's 505 ms per batch (profiles/r04_parity_*).
    static const bool f32_split = getenv("DIMX_F32_NO_SPLIT") == nullptr;
    if (f32_split) g.allow_splitk = 1;
    g.slab_stride = stride;
    gemm_set_plain_out(g, out, L.N);
    *nsl = gemm_plan_splits(g);
    g.force_splitk = *nsl;
    return launch_gemm(g, st);
}

// May the first layer's q/k/v come from the table?  Only a decoder whose layer-0 input is the token embedding alone.
static bool qkv0_table_supported(dimx_handle h) {
    const DecGeom& dg = h->decg;
    const int N = 3 * dg.heads * dg.dim_head;
    return h->use_qkv0_table && !dg.abs_pos && h->dec.self_[0].qkv.N == N && N % 4 == 0 && N <= 12 * 256 && dg.dim % 4 == 0 &&
           dg.dim / 2 <= 16 * 64;
}

// The table for projection launches of M rows: ceil(num_tokens / M) rounds of {embedding rows of the next M ids, the first layer's
// pre-norm, the step's own q/k/v projection at M rows, slabs added in order into the table rows}; the last round (and M >
// num_tokens) is padded by repeating the last id.  M is the step's M because the split count, hence the summation order,
// follows from it (gemm_plan_splits).  Runs on the generation scratch, which is free before the first step; s.step must read step0.
static int qkv0_table_build(dimx_handle h, const GenScratch& s, int M, hipStream_t st, int step0 = 0) {
    const DecGeom& dg = h->decg;
    const int DD = dg.dim, V = dg.num_tokens, N = h->dec.self_[0].qkv.N;
    if (h->qkv0_table && h->qkv0_M == M && h->qkv0_at == h->at && h->qkv0_epoch == h->dec_epoch) return DIMX_OK;
    if (!h->qkv0_table) {
        DIMX_HIP(hipMalloc((void**)&h->qkv0_table, (size_t)V * N * sizeof(float)));
        h->graph_valid = false;
    }
    h->qkv0_epoch = 0;
    const int rounds = (V + M - 1) / M;
    int32_t* ids = (int32_t*)s.logits;   // rounds * M < V + M ids; the logits slabs hold 8 * M * V words
    DIMX_TRY(launch_iota_clamp(ids, rounds * M, V, st));
    for (int r = 0; r < rounds; ++r) {
        int ns = 0;
        DIMX_TRY(launch_embed_step(h->dec.tok_emb, DD, V, ids + (size_t)r * M, nullptr, 0, s.step, s.x, M, 1, st, nullptr, 0.f, 1, step0));
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s.st_xr, s.y, h->dec.self_[0].ln_g, M, DD, st));
        DIMX_TRY(slab_gemm_rows(h, M, st, s.y, DD, h->dec.self_[0].qkv, s.qkv, s.st_qkv, &ns));
        DIMX_TRY(launch_sum_slabs_rows(s.qkv, ns, s.st_qkv, h->qkv0_table, r * M, V, M, N, st));
    }
    // the K / V columns in the operand type for the first layer's self attention in the table form (bf16 mode; the f32 mode reads
    // the table): same key and invalidation as the table, because it is rebuilt whenever the table is
    if (h->use_kv0_table && h->at == DIMX_BF16) {
        const int inner = N / 3;
        if (!h->kv0_image) {
            DIMX_HIP(hipMalloc(&h->kv0_image, (size_t)V * 2 * inner * sizeof(bf16)));
            h->graph_valid = false;
        }
        DIMX_TRY(launch_kv0_image(h->qkv0_table, N, V, inner, 2 * inner, h->kv0_image, st));
    }
    h->qkv0_M = M;
    h->qkv0_at = h->at;
    h->qkv0_epoch = h->dec_epoch;
    ++h->qkv0_builds;
    return DIMX_OK;
}

// what every gen_step of one generate call shares (built once in generate_impl)
struct GenCall {
    const CtxPersist& cp;
    const GenScratch& s;
    const GenPrompt& pr;
    const uint8_t* ctx_mask;
    int Btot, T, S, top_k;   // sequences of the batch, frames, samples per clip
    float temperature;
    const float* noise;
    uint64_t seed;
    int32_t* tokens;
    float* logits_out;
    const float* qkv0;   // the first layer's q/k/v table or nullptr
    const BeamCall* beam = nullptr;   // beam search: the selection and the cache reorder end the step in the sampler's place
    const void* kv0 = nullptr;        // the first layer's K / V table (the bf16 image, or the q/k/v table itself in the f32 mode): its self
                                      // attention reads rows of it through s.hist and keeps no cache; nullptr = the cache
};

// one decoder step for the clip group `grp` = rows [row0, row0 + B) of a batch of gc.Btot sequences:
// x = emb(token) -> 4 x {self, cross, ff} -> logits -> sample -> step += 1
static int gen_step(dimx_handle h, const GenCall& gc, int row0, int B, int grp, hipStream_t st, bool embed_only) {
    const GenScratch& s0 = gc.s;
    const GenPrompt& pr = gc.pr;
    const int T = gc.T, S = gc.S;
    const uint8_t* ctx_mask = gc.ctx_mask;   // advanced to this group's rows below, like tokens and logits_out
    int32_t* tokens = gc.tokens;
    float* logits_out = gc.logits_out;
    const DecGeom& dg = h->decg;
    const int DD = dg.dim, heads = dg.heads, D = dg.dim_head, inner = heads * D;
    const int V = dg.num_tokens, n = gen_steps(h, T), Tp = tpad(T);
    const float* pos = dg.abs_pos ? h->dec.pos_emb : nullptr;
    const float pos_scale = 1.0f / sqrtf((float)DD);
    const size_t es = es_of(h);
    const float scale = 1.0f / sqrtf((float)D);
    // this group's slices of every per-clip buffer
    GenScratch s = s0;
    auto boff = [&](void* p, size_t per_row_bytes) { return (void*)((unsigned char*)p + (size_t)row0 * per_row_bytes); };
    s.x = s0.x + (size_t)row0 * DD;
    s.y = boff(s0.y, DD * es);
    s.qkv = s0.qkv + (size_t)row0 * 3 * inner;
    s.qc = s0.qc + (size_t)row0 * inner;
    s.xr = s0.xr + (size_t)row0 * DD;
    s.o = boff(s0.o, inner * es);
    s.f = boff(s0.f, (size_t)DD * dg.ff_mult * es);
    s.logits = s0.logits + (size_t)row0 * V;
    s.step = s0.step + 16 * grp;
    s.hist = s0.hist + (size_t)row0 * T;
    // with S samples per clip, rows are samples (row = clip * S + sample); start / mask / cross K/V are per clip
    const int clip0 = row0 / S, nclip = B / S;
    // the first step's input is column step0 of the prompt; later steps inside a clip's prompt are forced by the sampler
    const int32_t* start = pr.tok + (size_t)clip0 * pr.ld + pr.step0;
    const int32_t* forced = pr.Pmax > 1 ? pr.tok + (size_t)clip0 * pr.ld : nullptr;
    const int32_t* forced_len = pr.len ? pr.len + clip0 : nullptr;
    ctx_mask += (size_t)clip0 * T;
    tokens += (size_t)row0 * n;
    if (logits_out) logits_out += (size_t)row0 * n * V;
    // round 4: the sampler that writes the next step's embedding row also writes the first layer's pre-norm of it, so a step
    // starts with y = LayerNorm(x) in place.  With the first layer's q/k/v table (gc.qkv0) both write the token's table row into slab 0
    // of s.qkv instead, and layer 0 starts at its attention.
    if (embed_only) {  // step 0 input = embedding of the start token (later steps: fused into the sampler)
        DIMX_TRY(launch_embed_step(h->dec.tok_emb, DD, V, start, tokens, n, s.step, s.x, B, S, st, pos, pos_scale, pr.ld, pr.step0));
        if (gc.qkv0)   // the first layer's q/k/v of the start token: a table row into slab 0 (nothing reads y before the layer rewrites it)
            DIMX_TRY(launch_gather_start_rows(gc.qkv0, 3 * inner, V, start, S, s.qkv, B, st, pr.ld, gc.kv0 ? s.hist : nullptr, T));
        else
            DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s0.st_xr, s.y, h->dec.self_[0].ln_g, B, DD, st));
        return DIMX_OK;
    }
    auto slab_gemm = [&](const void* A, int lda, const Linear& L, float* out, long stride, int* nsl) -> int {
        return slab_gemm_rows(h, B, st, A, lda, L, out, stride, nsl);
    };
    // XCD-local chain kernels (chain.hip) replace {projection, residual + LayerNorm, projection} triples by one launch
    const bool chain = gen_use_chain(h, B, S, grp);
    // deferred LayerNorm (chain.hip): the two chain launches of a layer write x and bf16(x) un-normalised + partial row
    // sums; cross-q (inside chain A) and ff1 (the next launch) run on gamma-scaled weights and correct their results
    const bool defer = chain && h->defer_ln && h->chain_stats_dev && h->dec.cross[0].q_ln.w && h->dec.ff[0].f1_ln.w;
    auto chain_site = [&](int site, const void* A1, int lda1, const Linear* W1, int nslab, const float* gamma,
                          const Linear* W2, float* out2, int ld_out2, const float* colsum2 = nullptr) -> int {
        ChainArgs c;
        memset(&c, 0, sizeof(c));
        c.B = B;
        if (defer && W1) {
            c.defer = 1;
            c.stats = h->chain_stats_dev;
            c.colsum2 = colsum2;
        }
        if (W1) {
            chain_desc(c.g1, *W1);
            c.A1 = A1;
            c.lda1 = lda1;
            c.xr = s.xr;
        }
        c.x = s.x;
        c.C = DD;
        c.slabs = nslab ? s.xr : nullptr;
        c.nslab = nslab;
        c.slab_stride = s0.st_xr;
        c.y = s.y;
        c.gamma = gamma;
        if (W2) {
            chain_desc(c.g2, *W2);
            c.out2 = out2;
            c.ld_out2 = ld_out2;
        }
        c.counters = s0.chain_ctr + (size_t)site * kChainSiteWords;
        c.seen = c.counters + 8 * 16;
        c.step = s.step + 9;   // steps done in this call (== the step counter unless a prompt was prefilled)
        c.err = h->chain_err_dev;
        c.fault = h->chain_fault_inject > 0 ? 1 : 0;
        return launch_chain(c, st);
    };
    // round 5: the attention half of a layer as one XCD-local launch (chain.hip xcd_layer_kernel; DIMX_NO_LAYER_CHAIN=1: the four
    // launches, for A/B runs)
    // Online generation: the cross attention's key count follows the step counter.  Only the one-query kernels of decode_attn.hip
    // have that form, so the layer kernel and the MFMA multi-query route below are not taken.
    const bool win = h->xwin_on != 0;
    const bool layer_kernel = h->use_layer_chain && chain && defer && S == 1 && 4 * dg.depth + 1 <= kChainSites && !win;
    auto layer_args = [&](int l, const DecodeAttnArgs& sa, const DecodeAttnArgs& ca, LayerChainArgs& lc) -> bool {
        const Linear& so = h->dec.self_[l].out;
        const Linear& cq = h->dec.cross[l].q_ln;
        const Linear& co = h->dec.cross[l].out;
        if (!so.w || !cq.w || !co.w || !h->dec.cross[l].q_ln_colsum) return false;
        lc.B = B;
        lc.C = DD;
        lc.sa = sa;
        lc.ca = ca;
        chain_desc(lc.g_so, so);
        chain_desc(lc.g_cq, cq);
        chain_desc(lc.g_co, co);
        lc.o = s.o;
        lc.ld_o = inner;
        lc.x = s.x;
        lc.y = s.y;
        lc.stats = h->chain_stats_dev;
        lc.colsum_cq = h->dec.cross[l].q_ln_colsum;
        lc.qc = s.qc;
        lc.ld_qc = inner;
        lc.counters = s0.chain_ctr + (size_t)(3 * dg.depth + 1 + l) * kChainSiteWords;
        lc.seen = lc.counters + 8 * 16;
        lc.step = s.step + 9;
        lc.err = h->chain_err_dev;
        lc.fault = h->chain_fault_inject > 0 ? 1 : 0;
        lc.sc_stride = (T + 15) / 16 * 16;
        lc.prof = h->layer_prof_dev ? h->layer_prof_dev + (size_t)l * 256 * 16 : nullptr;
        return true;
    };
    int pending = 0;  // slabs of the previous residual projection not yet folded into x
    for (int l = 0; l < dg.depth; ++l) {
        GemmArgs g;
        DecodeAttnArgs a;
        int ns = 0;
        if (l > 0)
            DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, pending, s0.st_xr, s.y, h->dec.self_[l].ln_g, B, DD, st));
        if (l == 0 && gc.qkv0)
            ns = 1;   // slab 0 already holds this token's q/k/v (the sampler / the start-token step copied the table row)
        else
            DIMX_TRY(slab_gemm(s.y, DD, h->dec.self_[l].qkv, s.qkv, s0.st_qkv, &ns));
        // the two attentions' arguments (self: q / new k / new v are the projection's split-K slabs; cross: the context K/V)
        DecodeAttnArgs sa, ca;
        memset(&sa, 0, sizeof(sa));
        sa.dtype = h->at;
        sa.q = s.qkv;
        sa.q_ld = 3 * inner;
        sa.q_f32 = 1;
        sa.nslab = ns;
        sa.slab_stride = s0.st_qkv;
        sa.knew = s.qkv + inner;
        sa.vnew = s.qkv + 2 * inner;
        sa.kv_ld = 3 * inner;
        sa.kcache = boff(s0.sk[l], (size_t)heads * T * 64 * es);
        sa.vcache = boff(s0.sv[l], (size_t)heads * T * 64 * es);
        sa.Tmax = T;
        sa.out = s.o;
        sa.o_ld = inner;
        sa.B = B;
        sa.H = heads;
        sa.step = s.step;
        sa.scale = scale;
        if (l == 0 && gc.kv0) {   // K / V of position j = the table row of the row's j-th input token; no append
            sa.tab = gc.kv0;
            sa.tab_rows = V;
            if (h->at == DIMX_BF16) { sa.tab_ld = 2 * inner; sa.tab_koff = 0; sa.tab_voff = inner; }
            else { sa.tab_ld = 3 * inner; sa.tab_koff = inner; sa.tab_voff = 2 * inner; }
            sa.hist = s.hist;
            sa.hist_ld = T;
        }
        memset(&ca, 0, sizeof(ca));
        ca.dtype = h->at;
        ca.q = s.qc;
        ca.q_ld = inner;
        ca.q_f32 = 1;
        ca.nslab = 1;
        ca.slab_stride = s0.st_qc;
        ca.kcache = (unsigned char*)gc.cp.ck[l] + (size_t)clip0 * heads * Tp * 64 * es;
        ca.vcache = (unsigned char*)gc.cp.cv[l] + (size_t)clip0 * heads * Tp * 64 * es;
        ca.Tmax = Tp;
        ca.out = s.o;
        ca.o_ld = inner;
        ca.B = S > 1 ? nclip : B;
        ca.rows_per_clip = S;
        ca.H = heads;
        ca.n_keys = T;
        ca.kmask = ctx_mask;
        ca.kmask_ld = T;
        ca.scale = scale;
        if (win) {
            ca.win = 1;
            ca.lookahead = h->xwin_lookahead;
            ca.step = s.step;
        }
        if (defer && layer_kernel) {
            // round 5: self attention -> out-projection -> cross-q -> cross attention -> out-projection as ONE XCD-local launch
            LayerChainArgs lc;
            memset(&lc, 0, sizeof(lc));
            if (layer_args(l, sa, ca, lc) && layer_chain_supported(lc, h->cu_count)) {
                DIMX_TRY(launch_layer_chain(lc, st));
                goto feed_forward;
            }
        }
        DIMX_TRY(launch_decode_attn(sa, st));
        if (chain) {  // self out-projection -> x += . -> LayerNorm -> cross q-projection
            if (defer)
                DIMX_TRY(chain_site(3 * l, s.o, inner, &h->dec.self_[l].out, 0, h->dec.cross[l].ln_g, &h->dec.cross[l].q_ln,
                                    s.qc, inner, h->dec.cross[l].q_ln_colsum));
            else
                DIMX_TRY(chain_site(3 * l, s.o, inner, &h->dec.self_[l].out, 0, h->dec.cross[l].ln_g, &h->dec.cross[l].qkv,
                                    s.qc, inner));
            ns = 1;
        } else {
            DIMX_TRY(slab_gemm(s.o, inner, h->dec.self_[l].out, s.xr, s0.st_xr, &pending));
            DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, pending, s0.st_xr, s.y, h->dec.cross[l].ln_g, B, DD, st));
            if (gen_multi_tr(h, S) && !win) {
                // round 6, best-of-N in one pass (code/x_engine_pt.py:257), bf16: the S queries of a clip against its context K/V on the
                // matrix cores -- the prefill attention kernel with Lq = S (one 128-query item per (clip, head), K / V streamed once),
                // queries in the operand type from a plain projection (rows = clips x S: no split-K needed).  The VALU multi-query
                // kernel it replaces ran 118 us per launch at 256 clips x 10 samples, 3 x its HBM floor (profiles/r06_samples10.txt).
                gemm_lin(h, s.y, DD, h->dec.cross[l].qkv, B, g);
                g.out_dtype = h->at;
                gemm_set_plain_out(g, (unsigned char*)s0.qcb + (size_t)row0 * inner * es, inner);
                DIMX_TRY(launch_gemm(g, st));
                AttnArgs ta;
                memset(&ta, 0, sizeof(ta));
                ta.dtype = h->at;
                ta.q = (unsigned char*)s0.qcb + (size_t)row0 * inner * es;
                ta.q_sb = (long)S * inner; ta.q_st = inner; ta.q_sh = D;
                ta.k = ca.kcache; ta.k_sb = (long)heads * Tp * D; ta.k_sh = (long)Tp * D; ta.k_st = D;
                ta.vt = ca.vcache; ta.v_rows = 1; ta.v_sb = (long)heads * Tp * D; ta.v_sh = (long)Tp * D; ta.v_st = D;
                ta.o = s.o; ta.o_sb = (long)S * inner; ta.o_st = inner; ta.o_sh = D;
                ta.B = nclip; ta.H = heads; ta.Lq = S; ta.Lk = T; ta.D = D;
                ta.scale = scale;
                ta.kmask = ctx_mask; ta.kmask_ld = T;
                ta.kwords = s0.kw + (size_t)clip0 * ((T + 63) / 64); ta.kwords_cap = s0.kw_cap - (size_t)clip0 * ((T + 63) / 64);
                ta.kwords_ready = 1;   // packed once per generation (generate_impl)
                DIMX_TRY(launch_attention_tr(ta, st));
                goto cross_out;
            }
            DIMX_TRY(slab_gemm(s.y, DD, h->dec.cross[l].qkv, s.qc, s0.st_qc, &ns));
        }
        ca.nslab = ns;
        DIMX_TRY(launch_decode_attn(ca, st));
    cross_out:
        if (chain) {  // cross out-projection -> x += . -> LayerNorm (feed-forward input)
            DIMX_TRY(chain_site(3 * l + 1, s.o, inner, &h->dec.cross[l].out, 0, h->dec.ff[l].ln_g, nullptr, nullptr, 0));
        } else {
            DIMX_TRY(slab_gemm(s.o, inner, h->dec.cross[l].out, s.xr, s0.st_xr, &pending));
            DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, pending, s0.st_xr, s.y, h->dec.ff[l].ln_g, B, DD, st));
        }
    feed_forward:
        gemm_lin(h, s.y, DD, defer ? h->dec.ff[l].f1_ln : h->dec.ff[l].f1, B, g);
        g.x3_decode = 1;
        if (defer) {
            g.ln_stats = h->chain_stats_dev;
            g.ln_err = h->chain_err_dev;
            g.ln_colsum = h->dec.ff[l].f1_ln_colsum;
            g.ln_C = DD;
        }
        g.out_dtype = h->at;
        g.act = ACT_GELU_ERF;
        gemm_set_plain_out(g, s.f, DD * dg.ff_mult);
        DIMX_TRY(launch_gemm(g, st));
        DIMX_TRY(slab_gemm(s.f, DD * dg.ff_mult, h->dec.ff[l].f2, s.xr, s0.st_xr, &pending));
    }
    int nlg = 0;
    if (chain && !h->dec.logits.bias) {  // x += feed-forward slabs -> final LayerNorm -> logits (the chain kernel has no bias input:
                                         // a checkpoint with the optional to_logits.bias takes the two launches below)
        DIMX_TRY(chain_site(3 * dg.depth, nullptr, 0, nullptr, pending, h->dec.final_g, &h->dec.logits, s.logits, V));
        nlg = 1;
    } else {
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, pending, s0.st_xr, s.y, h->dec.final_g, B, DD, st));
        DIMX_TRY(slab_gemm(s.y, DD, h->dec.logits, s.logits, s0.st_lg, &nlg));
    }
    if (gc.beam) {
        // Beam search (beam.hip): rows clip * S + w are the S hypotheses of a clip.  The selection writes column c of the token rows in
        // the new order, the next step's embedding / q/k/v table rows, and advances the step word; the reorder then permutes cache
        // positions 0 .. c and token columns < c by parent beam, reading c as the advanced word - 1.
        const BeamCall& bm = *gc.beam;
        BeamSelectArgs bs;
        bs.logits = s.logits; bs.nslab = nlg; bs.slab_stride = s0.st_lg; bs.nclip = nclip; bs.W = S;
        bs.step_dev = s.step; bs.step_rw = s.step; bs.done_ctr = (unsigned*)(s.step + 8); bs.epoch_rw = s.step + 9; bs.dev_params = s.step + 2;
        bs.prompt = forced; bs.prompt_ld = pr.ld; bs.prompt_max = pr.Pmax; bs.prompt_len = forced_len;
        bs.lens = bm.lens ? bm.lens + clip0 : nullptr; bs.len_off = T - n;
        bs.cum_in = bm.cum + row0; bs.cum_out = bm.cum + row0; bs.parent = bm.parent + row0;
        bs.tokens = tokens; bs.backptr = bm.backptr ? bm.backptr + (size_t)row0 * n : nullptr; bs.tok_ld = n; bs.logits_out = logits_out;
        bs.emb_table = h->dec.tok_emb; bs.emb_C = DD; bs.x_next = s.x;
        bs.qkv0_table = gc.qkv0; bs.qkv0_out = s.qkv; bs.qkv0_N = 3 * inner;
        DIMX_TRY(launch_beam_select(bs, st));
        if (!gc.qkv0) DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s0.st_xr, s.y, h->dec.self_[0].ln_g, B, DD, st));
        BeamReorderArgs br;
        for (int l = 0; l < dg.depth; ++l) {
            br.buf[2 * l] = boff(s0.sk[l], (size_t)heads * T * 64 * es);
            br.buf[2 * l + 1] = boff(s0.sv[l], (size_t)heads * T * 64 * es);
        }
        br.nbuf = 2 * dg.depth; br.es = (int)es; br.nclip = nclip; br.W = S; br.H = heads; br.T = T;
        br.parent = bs.parent; br.step_dev = s.step; br.step_back = 1;
        br.tokens = tokens; br.backptr = bs.backptr; br.tok_ld = n;
        return launch_beam_reorder(br, st);
    }
    SampleArgs sm;
    sm.logits = s.logits; sm.ld_logits = V; sm.R = B; sm.nslab = nlg; sm.slab_stride = s0.st_lg; sm.row0 = row0; sm.rows_total = gc.Btot;
    sm.top_k = gc.top_k; sm.noise = gc.noise; sm.filt.kind = h->filter_kind;
    sm.temperature = gc.temperature; sm.seed = gc.seed;   // read from the parameter block (dev_params) instead, like filt.a / b
    sm.step_dev = s.step; sm.step_rw = s.step; sm.dev_params = s.step + 2; sm.done_ctr = (unsigned*)(s.step + 8); sm.epoch_rw = s.step + 9;
    sm.tokens = tokens; sm.tok_ld = n; sm.tok_col_from_step = 1; sm.logits_out = logits_out; sm.logits_out_ld = n;
    sm.emb_table = h->dec.tok_emb; sm.emb_C = DD; sm.x_next = s.x; sm.pos_table = pos; sm.pos_scale = pos_scale; sm.pos_rows = n;
    sm.y_next = gc.qkv0 ? nullptr : s.y; sm.y_gamma = gc.qkv0 ? nullptr : h->dec.self_[0].ln_g; sm.y_dtype = h->at;
    sm.qkv0_table = gc.qkv0; sm.qkv0_out = s.qkv; sm.qkv0_N = 3 * inner;
    if (gc.kv0) { sm.hist = s.hist; sm.hist_ld = T; }
    sm.prompt = forced; sm.prompt_ld = pr.ld; sm.prompt_max = pr.Pmax; sm.prompt_len = forced_len; sm.prompt_div = S;
    return launch_sample(sm, st);
}

// Prefill of a prompted generation: the teacher-forced decoder stack of dimx_decode_tf over the positions 0 .. n0 - 1 of every
// clip (no key mask), every layer's self-attention K / V stored into the generation cache [B*S, H, T, 64] (kv_prefill.hip), no
// output head, and the last layer stops after its q/k/v projection -- its attentions and feed-forward feed nothing.
// Cross attention reads the context K / V where dimx_encode_ctx(for_generate = 1) left them, [B, H, Tp, 64]: the bf16
// attention takes that layout as it is (row-major V); the f32 attention reads V^T, so the f32 mode transposes one layer's V
// into scratch first (a copy, not a second projection of the context).
static int gen_prefill(dimx_handle h, const CtxPersist& cp, const GenScratch& gs, const PrefillScratch& s, const GenPrompt& pr,
                       const uint8_t* ctx_mask, int B, int T, int S, int32_t* tokens, hipStream_t st) {
    const DecGeom& dg = h->decg;
    const int n0 = pr.step0, M = B * n0, DD = dg.dim, heads = dg.heads, D = dg.dim_head;
    const int np = tpad(n0), Tp = tpad(T), V = dg.num_tokens;
    DIMX_TRY(launch_prompt_rows(pr.tok, pr.ld, B, n0, V, S, s.inp, tokens, gen_steps(h, T), st));
    DIMX_TRY(launch_gather_rows(DIMX_F32, h->dec.tok_emb, DD, V, s.inp, s.h, DD, M, DD, st));
    const bool rowv = qkv_row_v(h->at, D);
    for (int l = 0; l < dg.depth; ++l) {
        AttnArgs a;
        DIMX_TRY(self_attn_qkv(h, s, h->dec.self_[l].ln_g, nullptr, h->dec.self_[l].qkv, B, n0, DD, heads, D, a, st));
        DIMX_TRY(launch_kv_rows_to_cache(h->at, s.k, gs.sk[l], B, n0, heads, T, S, st));
        if (rowv)
            DIMX_TRY(launch_kv_rows_to_cache(h->at, s.vt, gs.sv[l], B, n0, heads, T, S, st));
        else
            DIMX_TRY(launch_kv_vt_to_cache((const float*)s.vt, np, (float*)gs.sv[l], B, n0, heads, T, S, st));
        if (l == dg.depth - 1) break;
        a.scale = 1.0f / sqrtf((float)D); a.causal = 1;
        DIMX_TRY(attn_out(h, s, a, h->dec.self_[l].out, DD, st));
        // cross attention over the context K / V of the generation layout [B,H,Tp,64]; the f32 attention reads V^T from s.cvt
        set_attn_packed(a, h->at, s.q, cp.ck[l], rowv ? cp.cv[l] : s.cvt, s.o, B, heads, n0, T, D, Tp, rowv);
        a.k_sb = (long)heads * Tp * D; a.k_sh = (long)Tp * D; a.k_st = D;
        if (rowv) { a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_st = D; }
        DIMX_TRY(cross_attn_sublayer(h, s, h->dec.cross[l], a, ctx_mask, DD, st, rowv ? nullptr : (const float*)cp.cv[l]));
        DIMX_TRY(ff_sublayer(h, s, h->dec.ff[l].ln_g, nullptr, h->dec.ff[l].f1, h->dec.ff[l].f2, nullptr, ACT_GELU_ERF, M, DD, st));
    }
    return DIMX_OK;
}

}  // namespace dimx

extern "C" {

// One implementation for dimx_generate (pr = {start, 1, 1, NULL, 0}) and dimx_generate_prompted.  keep_prefill: the call repeats
// a generation whose prefill already ran in this workspace (the regeneration after a chain fault): the decode steps write cache
// positions >= step0 and token / logit columns >= step0 only, so the prefix is intact and only the counters start over.
static int generate_impl(dimx_handle h, const dimx::GenPrompt& pr, bool keep_prefill, const uint8_t* ctx_mask, int B, int T, int n_samples,
                         float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens,
                         float* logits_out, void* ws, size_t ws_bytes, void* stream, bool* chain_used, bool prefill_only = false,
                         const dimx::BeamCall* beam = nullptr) {
    const int32_t* start = pr.tok;
    const int S = n_samples < 1 ? 1 : n_samples;
    if (h && h->filter_kind != DIMX_FILTER_TOP_K) top_k = 0;   // the other kinds ignore the call's k (and it keys the step graph)
    DIMX_REQUIRE(S == 1 || S == 2 || S == 4 || S == 5 || S == 8 || S == 10, DIMX_ERR_ARG,
                 "generate: n_samples %d not in {1,2,4,5,8,10}", n_samples);
    DIMX_TRY(check_common(h, B, T, ws, ws_bytes, COMP_DEC, S));
    DIMX_REQUIRE(start && ctx_mask && tokens && T >= 2, DIMX_ERR_ARG, "generate: null argument or T < 2");
    DIMX_REQUIRE(h->ctx_ready && h->ctx_B == B && h->ctx_T == T && h->ctx_ws == ws && h->ctx_for_generate,
                 DIMX_ERR_STATE, "generate: call dimx_encode_ctx(for_generate=1) with the same B, T, ws first");
    hipStream_t st = (hipStream_t)stream;
    CtxPersist cp;
    Arena ar = scratch_arena(h, ws, ws_bytes, B, T, &cp);
    GenScratch s;
    const int R = B * S;  // sequences generated in this call
    plan_gen(h, ar, R, T, s);
    PrefillScratch ps;
    if (pr.step0 > 0) plan_prefill(h, ar, B, pr.step0, T, ps);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "generate: workspace overflow");
    const int n = gen_steps(h, T);
    const int nrun = n - pr.step0;   // decode steps of this call
    if (h->use_chain && h->at == DIMX_BF16 && !h->chain_err_dev) {
        DIMX_HIP(hipMalloc((void**)&h->chain_err_dev, 64));
        DIMX_HIP(hipMemset(h->chain_err_dev, 0, 64));
        DIMX_HIP(hipMalloc((void**)&h->chain_stats_dev, 8 * 32 * 32 * 2 * sizeof(float)));
        DIMX_HIP(hipMemset(h->chain_stats_dev, 0, 8 * 32 * 32 * 2 * sizeof(float)));
        DIMX_HIP(hipHostMalloc((void**)&h->chain_err_host, 64, hipHostMallocDefault));
        *h->chain_err_host = 0;
        DIMX_HIP(hipEventCreateWithFlags(&h->chain_err_ev, hipEventDisableTiming));
    }
    DIMX_HIP(hipMemsetAsync(s.chain_ctr, 0, (size_t)kChainSites * kChainSiteWords * 4, st));
    // step / done counters = 0; temperature, seed and the sampler's global row window go to device memory so that
    // the captured step graph is independent of them
    DIMX_TRY(launch_gen_params(s.step, dimx_ctx::kMaxGroups, temperature, seed, h->shard_row_off * S,
                               h->shard_rows_total * S, st, pr.step0, h->filter_a, h->filter_b));
    if (gen_multi_tr(h, S)) DIMX_TRY(launch_pack_key_words(ctx_mask, T, nullptr, B, T, s.kw, s.kw_cap, st));
    if (beam) {   // every run of the call (a regeneration after a chain fault too) starts the search over
        DIMX_REQUIRE(h->decg.dim_head == 64 && h->decg.depth <= 8 && !h->decg.abs_pos, DIMX_ERR_ARG,
                     "generate_beam: needs 64-wide heads, at most 8 layers and a decoder without positional embedding");
        DIMX_TRY(launch_beam_init(beam->cum, beam->parent, R, S, st));
        if (beam->backptr && pr.step0 > 0)   // no step ran on the prefilled columns: -1
            DIMX_HIP(hipMemset2DAsync(beam->backptr, (size_t)n * 4, 0xFF, (size_t)pr.step0 * 4, R, st));
    }
    // Independent clip groups run as separate step graphs on separate streams: every decode kernel is
    // latency-bound at these sizes, so two groups in flight let one group's GEMM/LayerNorm chain overlap the
    // other group's HBM-bound attention.  Results do not depend on the grouping (per-clip state only; the
    // sampler's noise / counter-based RNG is indexed by the global clip row).
    int G = h->gen_groups < 1 ? 1 : h->gen_groups;
    if (G > B) G = B;
    if (S > 1 || beam) G = 1;  // samples of a clip stay together (they share the clip's cross K/V pass)
    // one group: every projection launch of the generation has R rows, and so has the table's build
    const float* qkv0 = nullptr;
    if (G == 1 && qkv0_table_supported(h)) {
        DIMX_TRY(qkv0_table_build(h, s, R, st, pr.step0));
        qkv0 = h->qkv0_table;
    }
    // the first layer's self attention from the table: no beam search (the cache reorder would have to permute the history) and
    // no prompt (a prefill fills the cache, not the history); any number of samples per clip: rows are samples
    const void* kv0 = nullptr;
    if (qkv0 && h->use_kv0_table && !beam && pr.step0 == 0 && pr.Pmax <= 1 && h->decg.dim_head == 64 && h->decg.num_tokens <= 512) {
        kv0 = h->at == DIMX_BF16 ? h->kv0_image : (const void*)h->qkv0_table;
        if (kv0) ++h->kv0_generations;
    }
    if (pr.step0 > 0 && !keep_prefill) {
        // the prefill forms no logits: those columns of logits_out read zero
        if (logits_out)
            DIMX_HIP(hipMemset2DAsync(logits_out, (size_t)n * h->decg.num_tokens * 4, 0, (size_t)pr.step0 * h->decg.num_tokens * 4, R, st));
        DIMX_TRY(gen_prefill(h, cp, s, ps, pr, ctx_mask, B, T, S, tokens, st));
    }
    if (prefill_only) {   // tools/bench_prompt.py: the prefill stage alone
        *chain_used = false;
        return DIMX_OK;
    }
    int lo[dimx_ctx::kMaxGroups + 1];
    for (int g = 0; g <= G; ++g) lo[g] = (int)((long)R * g / G);
    hipStream_t gs[dimx_ctx::kMaxGroups];
    if (G == 1) {
        gs[0] = st;
    } else {
        if (!h->ev_fork) DIMX_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        DIMX_HIP(hipEventRecord(h->ev_fork, st));
        for (int g = 0; g < G; ++g) {
            if (!h->grp_stream[g]) DIMX_HIP(hipStreamCreateWithFlags(&h->grp_stream[g], hipStreamNonBlocking));
            if (!h->ev_join[g]) DIMX_HIP(hipEventCreateWithFlags(&h->ev_join[g], hipEventDisableTiming));
            gs[g] = h->grp_stream[g];
            DIMX_HIP(hipStreamWaitEvent(gs[g], h->ev_fork, 0));
        }
    }
    const GenCall gc{cp, s, pr, ctx_mask, R, T, S, top_k, temperature, exp_noise, seed, tokens, logits_out, qkv0, beam, kv0};
    for (int g = 0; g < G; ++g) DIMX_TRY(gen_step(h, gc, lo[g], lo[g + 1] - lo[g], g, gs[g], true));
    if (!h->use_graph) {
        for (int t = 0; t < nrun; ++t)
            for (int g = 0; g < G; ++g) DIMX_TRY(gen_step(h, gc, lo[g], lo[g + 1] - lo[g], g, gs[g], false));
    } else {
        // greedy vs sampling is decided from the device-side parameters; only shapes and pointers key the graph.  The prompt's
        // pointers, row stride and width are kernel arguments of the sampler; P0 is not (the counters' start value and the
        // number of launches below), so a call with another P0 replays the same graphs.
        GraphKey key{ws, B, T, top_k, 0.f, exp_noise, 0, start, ctx_mask, tokens, logits_out, G * 100 + S + (h->use_chain ? 1000 : 0) + (h->chain_fault_inject > 0 ? 2000 : 0) + (qkv0 ? 4000 : 0) + (kv0 ? 8000 : 0),
                     pr.len, pr.ld, pr.Pmax, h->filter_kind, beam ? *beam : dimx::BeamCall{}, h->xwin_on, h->xwin_on ? h->xwin_lookahead : 0};
        if (!(h->graph_valid && h->graph_key == key)) {
            h->graph_valid = false;
            if (!h->cap_stream) DIMX_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
            for (int g = 0; g < dimx_ctx::kMaxGroups; ++g) {
                if (h->graph_exec[g]) {
                    (void)hipGraphExecDestroy(h->graph_exec[g]);
                    h->graph_exec[g] = nullptr;
                }
                if (h->graph_multi[g]) {
                    (void)hipGraphExecDestroy(h->graph_multi[g]);
                    h->graph_multi[g] = nullptr;
                }
            }
            // The step does not depend on the step index (it lives in device memory), so the same launches can be captured
            // several times in a row: consecutive graph launches leave ~8 us of idle GPU between them (kernel trace of
            // round 2: 299 gaps = 2.5 ms per batch), kernels inside one graph follow each other without a gap.  `reps` = 1
            // for the remainder steps, graph_unroll for the bulk.
            for (int g = 0; g < G; ++g) {
                for (int pass = 0; pass < 2; ++pass) {
                    const int reps = pass == 0 ? 1 : h->graph_unroll;
                    if (pass == 1 && (reps <= 1 || n < reps)) continue;
                    hipGraph_t graph = nullptr;
                    DIMX_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
                    int rc = DIMX_OK;
                    for (int r = 0; r < reps && rc == DIMX_OK; ++r)
                        rc = gen_step(h, gc, lo[g], lo[g + 1] - lo[g], g, h->cap_stream, false);
                    const hipError_t ce = hipStreamEndCapture(h->cap_stream, &graph);
                    if (rc != DIMX_OK) {
                        if (graph) (void)hipGraphDestroy(graph);
                        return rc;
                    }
                    DIMX_HIP(ce);
                    DIMX_HIP(hipGraphInstantiate(pass == 0 ? &h->graph_exec[g] : &h->graph_multi[g], graph, nullptr, nullptr, 0));
                    (void)hipGraphDestroy(graph);
                }
            }
            h->graph_key = key;
            h->graph_valid = true;
        }
        {
            const int U = h->graph_unroll;
            int t = 0;
            for (; U > 1 && t + U <= nrun; t += U)
                for (int g = 0; g < G; ++g)
                    if (h->graph_multi[g]) DIMX_HIP(hipGraphLaunch(h->graph_multi[g], gs[g]));
                    else
                        for (int r = 0; r < U; ++r) DIMX_HIP(hipGraphLaunch(h->graph_exec[g], gs[g]));
            for (; t < nrun; ++t)
                for (int g = 0; g < G; ++g) DIMX_HIP(hipGraphLaunch(h->graph_exec[g], gs[g]));
        }
    }
    if (G > 1) {
        for (int g = 0; g < G; ++g) {
            DIMX_HIP(hipEventRecord(h->ev_join[g], gs[g]));
            DIMX_HIP(hipStreamWaitEvent(st, h->ev_join[g], 0));
        }
    }
    *chain_used = G == 1 && gen_use_chain(h, lo[1] - lo[0], S, 0);
    if (*chain_used) {
        DIMX_HIP(hipMemcpyAsync(h->chain_err_host, h->chain_err_dev, 4, hipMemcpyDeviceToHost, st));
        DIMX_HIP(hipEventRecord(h->chain_err_ev, st));
    }
    return DIMX_OK;
}

// DIMX_LAYER_PROF=1 (tuning): the phase stamps of the LAST step's layer launches (100 MHz wall clock), mean / max over blocks
static int print_layer_prof(dimx_handle h) {
    DIMX_HIP(hipEventSynchronize(h->chain_err_ev));
    static const char* names[13] = {"start", "self attention done", "barrier 1", "rows + W1 landed", "out-proj stored", "barrier 2",
                                    "y rows + W2 landed", "cross-q stored", "barrier 3", "cross attention done", "barrier 4",
                                    "rows + W3 landed", "out-proj stored"};
    std::vector<unsigned long long> hp((size_t)8 * 256 * 16);
    DIMX_HIP(hipMemcpy(hp.data(), h->layer_prof_dev, hp.size() * 8, hipMemcpyDeviceToHost));
    for (int l = 0; l < h->decg.depth; ++l) {
        const unsigned long long* p = hp.data() + (size_t)l * 256 * 16;
        unsigned long long t0 = ~0ull;
        for (int b = 0; b < 256; ++b)
            if (p[b * 16] && p[b * 16] < t0) t0 = p[b * 16];
        if (t0 == ~0ull) continue;
        fprintf(stderr, "dimx layer-kernel stamps, layer %d (us after the first block's start; mean / max over blocks)\n", l);
        double prev = 0;
        for (int i = 0; i < 13; ++i) {
            double sum = 0, mx = 0;
            int n = 0;
            for (int b = 0; b < 256; ++b)
                if (p[b * 16 + i]) {
                    const double v = (double)(p[b * 16 + i] - t0) / 100.0;
                    sum += v;
                    mx = v > mx ? v : mx;
                    ++n;
                }
            if (!n) continue;
            fprintf(stderr, "  %-24s %7.2f / %7.2f  (+%.2f)\n", names[i], sum / n, mx, sum / n - prev);
            prev = sum / n;
        }
    }
    return DIMX_OK;
}

// Waits for the generation that ran chain kernels and returns its flag word (or a negative DIMX_ERR_*).  Non-zero flags are
// cleared on both sides, the step graph is dropped and the fault is counted: the caller regenerates the batch.
static int take_chain_flags(dimx_handle h, void* stream) {
    DIMX_HIP(hipEventSynchronize(h->chain_err_ev));
    const unsigned e = *h->chain_err_host;
    if (!e) return 0;
    *h->chain_err_host = 0;
    DIMX_HIP(hipMemsetAsync(h->chain_err_dev, 0, 64, (hipStream_t)stream));
    h->graph_valid = false;
    ++h->chain_faults;
    return (int)e;
}

// The XCD-local chain kernels need their 256 blocks co-resident, one per CU, on the XCD whose rows they own; another
// process, handle or stream on the same GPU can break that.  They detect it (claim stamps, bounded barriers) but cannot
// repair it, so the call that used them checks their flags before it returns: it waits for its own generation (the caller
// is about to read the tokens anyway) and, on a fault, regenerates the same batch on the one-kernel-per-op step and keeps
// the chain path off for this handle.  Round 2 reported the fault one call late.
static int generate_checked(dimx_handle h, const dimx::GenPrompt& pr, const uint8_t* ctx_mask, int B, int T, int n_samples,
                            float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out,
                            void* ws, size_t ws_bytes, void* stream, const dimx::BeamCall* beam = nullptr) {
    bool chain_used = false;
    auto run = [&](bool keep_prefill) {
        return generate_impl(h, pr, keep_prefill, ctx_mask, B, T, n_samples, temperature, top_k, exp_noise, seed, tokens, logits_out, ws,
                             ws_bytes, stream, &chain_used, false, beam);
    };
    DIMX_TRY(run(false));
    if (h->chain_fault_inject > 0) --h->chain_fault_inject;
    if (!chain_used) return DIMX_OK;
    if (h->layer_prof_dev) DIMX_TRY(print_layer_prof(h));
    const int e = take_chain_flags(h, stream);
    if (e <= 0) return e;
    if (e & 3) {
        h->use_chain = 0;
        fprintf(stderr, "dimx: the XCD-local chain kernels reported %s%s; this batch is regenerated on the one-kernel-per-op "
                        "step and the chain path stays off for this handle (DIMX_NO_CHAIN=1 avoids it from the start)\n",
                (e & 1) ? "two blocks on one (XCD, CU slot) " : "", (e & 2) ? "a group-barrier timeout" : "");
    } else {
        // bit 2 alone: a residual row with |mean| > 8 standard deviations -- the deferred LayerNorm multiplies bf16(x), not
        // bf16(x - mean), and its rounding noise is no longer small against the row's spread.  Same repair: the batch is
        // regenerated with the row-phase LayerNorm (chain kernels stay on).
        h->defer_ln = 0;
        fprintf(stderr, "dimx: a residual row's mean exceeds 8 standard deviations; this batch is regenerated with the row-phase "
                        "LayerNorm and the deferred form stays off for this handle\n");
    }
    DIMX_TRY(run(true));
    if (!chain_used) return DIMX_OK;
    // the regeneration may still have run chain kernels (the bit-2 case keeps them on): it answers for its own flags too
    //  -- a second fault takes the chain path off and regenerates once more on the one-kernel-per-op step
    const int e2 = take_chain_flags(h, stream);
    if (e2 <= 0) return e2;
    h->use_chain = 0;
    fprintf(stderr, "dimx: the regenerated batch reported chain flags 0x%x again; regenerating on the one-kernel-per-op step, the "
                    "chain path stays off for this handle\n", e2);
    DIMX_TRY(run(true));
    DIMX_REQUIRE(!chain_used, DIMX_ERR_STATE, "generate: the chain path is still active after it was switched off");
    return DIMX_OK;
}

int dimx_generate(dimx_handle h, const int32_t* start, const uint8_t* ctx_mask, int B, int T, int n_samples,
                  float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out,
                  void* ws, size_t ws_bytes, void* stream) {
    const dimx::GenPrompt pr{start, 1, 1, nullptr, 0};
    return generate_checked(h, pr, ctx_mask, B, T, n_samples, temperature, top_k, exp_noise, seed, tokens, logits_out, ws, ws_bytes,
                            stream);
}

int dimx_generate_prompted(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                           const uint8_t* ctx_mask, int B, int T, int n_samples, float temperature, int top_k,
                           const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out, int flags, void* ws,
                           size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "generate_prompted: prompts are implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(prompt && T >= 2 && Pmax >= 1 && Pmax <= T - 1 && ld_prompt >= Pmax, DIMX_ERR_ARG,
                 "generate_prompted: need 1 <= Pmax <= T - 1 and ld_prompt >= Pmax (Pmax=%d T=%d ld_prompt=%d)", Pmax, T, ld_prompt);
    DIMX_REQUIRE(P0 >= 1 && P0 <= Pmax, DIMX_ERR_ARG, "generate_prompted: need 1 <= P0 <= Pmax (P0=%d Pmax=%d)", P0, Pmax);
    DIMX_REQUIRE((flags & ~3) == 0, DIMX_ERR_ARG, "generate_prompted: unknown flags 0x%x", flags);
    const int S = n_samples < 1 ? 1 : n_samples;
    // bit 0: no prefill, the whole prompt goes through forced decode steps.  Online generation (dimx_set_cross_lookahead) too: the
    // prefill's attention has no per-query key bound, the decode step's has
    const int p0 = ((flags & 1) || h->xwin_on) ? 1 : P0;
    // bit 1 is not part of the public flag set: tools/bench_prompt.py times the prefill stage alone with it
    DIMX_REQUIRE(!(flags & 2) || p0 >= 2, DIMX_ERR_ARG, "generate_prompted: flags bit 1 (the prefill stage alone) without a prefill (P0=%d, flags 0x%x)",
                 P0, flags);
    DIMX_REQUIRE(p0 == 1 || h->decg.dim_head == 64, DIMX_ERR_ARG, "generate_prompted: the prefill needs 64-wide heads");
    DIMX_REQUIRE(B >= 1 && T <= h->d.max_seq_len, DIMX_ERR_ARG, "B=%d T=%d out of range (T <= %d)", B, T, h->d.max_seq_len);
    const size_t need = dimx::workspace_bytes_prompt(h, B, T, S, p0);
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "generate_prompted: workspace %zu < required %zu (dimx_workspace_bytes_prompt)",
                 ws_bytes, need);
    const dimx::GenPrompt pr{prompt, ld_prompt, Pmax, prompt_len, p0 - 1};
    if (flags & 2) {   // the prefill stage alone, nothing is generated
        bool chain_used = false;
        return generate_impl(h, pr, false, ctx_mask, B, T, n_samples, temperature, top_k, exp_noise, seed, tokens, logits_out, ws,
                             ws_bytes, stream, &chain_used, true);
    }
    return generate_checked(h, pr, ctx_mask, B, T, n_samples, temperature, top_k, exp_noise, seed, tokens, logits_out, ws, ws_bytes,
                            stream);
}

int dimx_generate_beam(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                       const uint8_t* ctx_mask, const int32_t* lens, int B, int T, int beam_width, int32_t* tokens, double* scores,
                       int32_t* backptr, float* logits_out, void* beam_state, size_t beam_state_bytes, int flags, void* ws, size_t ws_bytes,
                       void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "generate_beam: beam search is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(!h->xwin_on, DIMX_ERR_ARG, "generate_beam: not available while the cross-attention window is on (dimx_set_cross_lookahead)");
    DIMX_REQUIRE(dimx::beam_width_supported(beam_width), DIMX_ERR_ARG, "generate_beam: beam_width %d not in {1,2,4,5,8,10}", beam_width);
    DIMX_REQUIRE(prompt && scores && T >= 2 && Pmax >= 1 && Pmax <= T - 1 && ld_prompt >= Pmax, DIMX_ERR_ARG,
                 "generate_beam: need scores, 1 <= Pmax <= T - 1 and ld_prompt >= Pmax (Pmax=%d T=%d ld_prompt=%d)", Pmax, T, ld_prompt);
    DIMX_REQUIRE(P0 >= 1 && P0 <= Pmax, DIMX_ERR_ARG, "generate_beam: need 1 <= P0 <= Pmax (P0=%d Pmax=%d)", P0, Pmax);
    DIMX_REQUIRE((flags & ~1) == 0, DIMX_ERR_ARG, "generate_beam: unknown flags 0x%x", flags);
    DIMX_REQUIRE(B >= 1 && T <= h->d.max_seq_len, DIMX_ERR_ARG, "B=%d T=%d out of range (T <= %d)", B, T, h->d.max_seq_len);
    const size_t R = (size_t)B * beam_width;
    DIMX_REQUIRE(beam_state && ((uintptr_t)beam_state % 8) == 0 && beam_state_bytes >= DIMX_BEAM_STATE_BYTES(B, beam_width), DIMX_ERR_ARG,
                 "generate_beam: the beam state needs %zu bytes, 8-byte aligned (DIMX_BEAM_STATE_BYTES); got %zu", (size_t)DIMX_BEAM_STATE_BYTES(B, beam_width),
                 beam_state_bytes);
    const int p0 = (flags & 1) ? 1 : P0;
    DIMX_REQUIRE(p0 == 1 || h->decg.dim_head == 64, DIMX_ERR_ARG, "generate_beam: the prefill needs 64-wide heads");
    const size_t need = dimx::workspace_bytes_prompt(h, B, T, beam_width, p0);
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "generate_beam: workspace %zu < required %zu (dimx_workspace_bytes_prompt)", ws_bytes, need);
    const dimx::GenPrompt pr{prompt, ld_prompt, Pmax, prompt_len, p0 - 1};
    dimx::BeamCall bm;
    bm.cum = (double*)beam_state;
    bm.parent = (int32_t*)((double*)beam_state + R);
    bm.backptr = backptr;
    bm.lens = lens;
    DIMX_TRY(generate_checked(h, pr, ctx_mask, B, T, beam_width, 0.f, 0, nullptr, 0, tokens, logits_out, ws, ws_bytes, stream, &bm));
    DIMX_HIP(hipMemcpyAsync(scores, bm.cum, R * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DIMX_OK;
}

// x-transformers' own parameter ranges; the kernel treats thres >= 1 and min_p = 0 as "keep everything"
static int check_sampler_filter(int kind, float a, float b) {
    DIMX_REQUIRE(kind >= DIMX_FILTER_TOP_K && kind <= DIMX_FILTER_TOP_A, DIMX_ERR_ARG, "sampler filter: unknown kind %d", kind);
    if (kind == DIMX_FILTER_TOP_K) return DIMX_OK;
    DIMX_REQUIRE(a == a && (kind != DIMX_FILTER_TOP_A || b == b), DIMX_ERR_ARG, "sampler filter: NaN parameter");
    if (kind == DIMX_FILTER_TOP_P) DIMX_REQUIRE(a >= 0.f, DIMX_ERR_ARG, "sampler filter: top_p thres %g < 0", (double)a);
    if (kind == DIMX_FILTER_MIN_P) DIMX_REQUIRE(a >= 0.f && a <= 1.f, DIMX_ERR_ARG, "sampler filter: min_p %g outside [0, 1]", (double)a);
    if (kind == DIMX_FILTER_TOP_A)
        DIMX_REQUIRE(a >= 0.f && b >= 0.f, DIMX_ERR_ARG, "sampler filter: top_a min_p_pow %g or min_p_ratio %g < 0", (double)a, (double)b);
    return DIMX_OK;
}

int dimx_set_sampler_filter(dimx_handle h, int kind, float a, float b) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_TRY(check_sampler_filter(kind, a, b));
    h->filter_kind = kind;
    h->filter_a = kind == DIMX_FILTER_TOP_K ? 0.f : a;
    h->filter_b = kind == DIMX_FILTER_TOP_A ? b : 0.f;
    return DIMX_OK;
}

int dimx_set_cross_lookahead(dimx_handle h, int on, int lookahead) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_cross_lookahead: online generation is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    h->xwin_on = on ? 1 : 0;
    h->xwin_lookahead = on ? lookahead : 0;
    return DIMX_OK;
}

int dimx_cross_lookahead(dimx_handle h, int* on, int* lookahead) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (on) *on = h->xwin_on;
    if (lookahead) *lookahead = h->xwin_lookahead;
    return DIMX_OK;
}

int dimx_chain_faults(dimx_handle h) { return h ? h->chain_faults : 0; }
int dimx_qkv0_table_builds(dimx_handle h) { return h ? h->qkv0_builds : 0; }
int dimx_kv0_table_generations(dimx_handle h) { return h ? h->kv0_generations : 0; }

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

int dimx_op_lstm_layer(int dtype, const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                       const float* const* b_ih, const float* const* b_hh, float* y, int flags, int* faults_out, void* stream) {
    DIMX_REQUIRE(dtype == DIMX_F32, DIMX_ERR_ARG, "lstm_layer: only the f32 recurrence is built (dtype %d)", dtype);
    DIMX_REQUIRE(B >= 1 && T >= 1 && In >= 4, DIMX_ERR_ARG, "lstm_layer: bad shape");
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const size_t bytes = lstm_scratch_bytes(B, T, In);
    void* scratch = nullptr;
    DIMX_HIP(hipMalloc(&scratch, bytes));
    int faults = 0;
    const int rc = lstm_layer_run(x, B, T, In, H, w_ih, w_hh, b_ih, b_hh, y, scratch, bytes, flags, cus, &faults, st);
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (faults_out) *faults_out = faults;
    DIMX_TRY(rc);
    DIMX_HIP(e);
    return DIMX_OK;
}

int dimx_debug_chain_fault(dimx_handle h, int n_calls) {
    DIMX_REQUIRE(h && n_calls >= 0, DIMX_ERR_ARG, "debug_chain_fault: bad argument");
    h->chain_fault_inject = n_calls;
    h->graph_valid = false;
    return DIMX_OK;
}

// ---------------------------------------------------------------- kernel-level entry points
int dimx_op_gemm(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M,
                 int N, int K, const float* bias, int act, const float* residual, int ldr, int conv_T,
                 const int32_t* conv_lens, int flags, void* stream) {
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = in_dtype;
    g.out_dtype = out_dtype;
    g.A = A;
    g.lda = lda;
    g.W = W;
    g.ldw = ldw;
    g.M = M;
    g.N = N;
    g.K = K;
    g.bias = bias;
    g.act = act;
    g.residual = residual;
    g.ldr = ldr;
    g.allow_splitk = flags & 1;
    g.force_simple = (flags >> 1) & 1;
    g.out_slabs = (flags >> 2) & 1;        /* C = [splits][M, ldc] f32 slabs (split count = flags bits 16..23) */
    g.w_tiled = (flags >> 3) & 1;          /* W in 8-row x 128-byte blocks (tools/gemm_ab.py; N % 8 == 0) */
    g.slab_stride = (long)M * ldc;
    g.cfg = (flags >> 8) & 0xff;           /* tuning: tile/stage config id */
    g.force_splitk = (flags >> 16) & 0xff; /* tuning: split count */
    if (ldw > K && K % (in_dtype == DIMX_BF16 ? 64 : 32) == 0) g.kloop = K; /* padded row stride, exact k extent */
    if (conv_T > 0) {
        g.conv_T = conv_T;
        g.conv_lens = conv_lens;
        g.conv_C = K / 5;
    }
    gemm_set_plain_out(g, C, ldc);
    return launch_gemm(g, (hipStream_t)stream);
}

/* the f32 parity mode's split-bf16 decode GEMM alone (csrc/gemm_x3.hip): dimx_op_split_x3 makes the three bf16 planes of an f32 matrix
 * (what the weight packing does once per Linear), dimx_op_gemm_x3 multiplies f32 activations with them */
int dimx_op_split_x3(const float* w, void* planes, long n, void* stream) {
    DIMX_REQUIRE(n > 0, DIMX_ERR_ARG, "op_split_x3: empty matrix");
    return launch_split_x3(w, planes, (size_t)n, (hipStream_t)stream);
}

int dimx_op_gemm_x3(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K, const float* bias, int act,
                    const float* residual, int ldr, int flags, void* stream) {
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = DIMX_F32;
    g.out_dtype = DIMX_F32;
    g.A = A;
    g.lda = lda;
    g.W = planes;   /* the f32 matrix itself is not needed by this kernel */
    g.w3 = planes;
    g.w3_plane = (long)N * K;
    g.x3_decode = 1;
    g.ldw = K;
    g.M = M;
    g.N = N;
    g.K = K;
    g.bias = bias;
    g.act = act;
    g.residual = residual;
    g.ldr = ldr;
    g.allow_splitk = 1;
    g.out_slabs = (flags >> 2) & 1;
    g.slab_stride = (long)M * ldc;
    g.force_splitk = (flags >> 16) & 0xff;
    gemm_set_plain_out(g, C, ldc);
    if (act != 0 && g.out_slabs) {   // an activation applies to the whole sum, never to one split's partial sum
        GemmArgs g1 = g;
        g1.act = 0;
        int bn = 0, sp = 1;
        DIMX_REQUIRE(!(gemm_use_x3(g1) && gemm_x3_plan(g1, &bn, &sp) && sp > 1), DIMX_ERR_ARG,
                     "op_gemm_x3: activation %d with %d split-K slabs (M=%d N=%d K=%d): an activation needs the unsplit sum", act, sp, M,
                     N, K);
    }
    DIMX_REQUIRE(planes && gemm_use_x3(g), DIMX_ERR_ARG, "op_gemm_x3: M=%d N=%d K=%d is not a shape of the split-bf16 kernel (K %% 32 == 0, "
                 "N a multiple of 36 / 64 / 72 / 96)", M, N, K);
    return launch_gemm_x3(g, (hipStream_t)stream);
}

/* number of split-K slabs an out_slabs dimx_op_gemm call with these arguments writes (tests: the f32 kernels plan it themselves) */
int dimx_op_gemm_slabs(int in_dtype, int M, int N, int K, int flags) {
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = in_dtype;
    g.out_dtype = DIMX_F32;
    g.A = g.W = (const void*)16;
    g.lda = g.ldw = K;
    g.M = M;
    g.N = N;
    g.K = K;
    g.allow_splitk = flags & 1;
    g.out_slabs = 1;
    g.force_splitk = (flags >> 16) & 0xff;
    if ((flags >> 4) & 1) {
        g.w3 = (const void*)16;
        g.w3_plane = (long)N * K;
        g.x3_decode = 1;
    }
    float dummy;
    gemm_set_plain_out(g, &dummy, N);
    return gemm_plan_splits(g);
}

int dimx_op_gemm_headmajor(int dtype, const void* A, int lda, const void* W, int ldw, void* out, int M, int N, int K,
                           int rowT, int Tp, int nlayers, void* stream) {
    DIMX_REQUIRE(nlayers >= 1 && nlayers <= 4 && N % (nlayers * 128) == 0, DIMX_ERR_ARG, "op_gemm_headmajor: bad shape");
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = dtype;
    g.out_dtype = dtype;
    g.A = A;
    g.lda = lda;
    g.W = W;
    g.ldw = ldw;
    g.M = M;
    g.N = N;
    g.K = K;
    g.rowT = rowT;
    // column segments K_0 | V_0 | K_1 | V_1 ... each a [B, H, Tp, 64] cache (project_cross_kv's for_generate layout)
    const int nseg = 2 * nlayers, segw = N / nseg, H = segw / 64;
    OutSeg segs[8];
    for (int i = 0; i < nseg; ++i) {
        segs[i].ptr = (unsigned char*)out + (size_t)i * (M / rowT) * H * Tp * 64 * dtype_size(dtype);
        segs[i].sb = (long)H * Tp * 64;
        segs[i].sh = (long)Tp * 64;
        segs[i].st = 64;
        segs[i].sd = 1;
        segs[i].D = 64;
    }
    GemmArgs probe = g;
    gemm_set_plain_out(probe, out, N);
    if (dtype == DIMX_BF16 && gemm256_eligible(probe)) return launch_gemm256_segs(g, segs, nseg, segw, (hipStream_t)stream);
    DIMX_REQUIRE(nlayers == 1, DIMX_ERR_ARG, "op_gemm_headmajor: the fused multi-layer form needs the bf16 256-tile kernel");
    g.nseg = 2;
    g.seg_width = segw;
    g.seg[0] = segs[0];
    g.seg[1] = segs[1];
    return launch_gemm(g, (hipStream_t)stream);
}

int dimx_op_layernorm(int out_dtype, const float* x, void* y, const float* gamma, const float* beta, int M, int C,
                      void* stream) {
    return launch_layernorm(out_dtype, x, y, gamma, beta, M, C, (hipStream_t)stream);
}

int dimx_op_instnorm(int out_dtype, const float* x, void* y, const int32_t* lens, int B, int T, int C, void* stream) {
    return launch_instnorm(out_dtype, x, y, lens, B, T, C, (hipStream_t)stream);
}

// operator entry points (tests / tools): the key-mask scratch of attention_tr.hip is a stream-ordered allocation around the call
static int op_attention_with_scratch(AttnArgs& a, hipStream_t st) {
    void* kw = nullptr;
    if (a.kmask && a.v_rows && a.dtype == DIMX_BF16) {
        a.kwords_cap = (size_t)a.B * ((a.Lk + 63) / 64);
        DIMX_HIP(hipMallocAsync(&kw, a.kwords_cap * 8, st));
        a.kwords = (unsigned long long*)kw;
    }
    const int rc = launch_attention(a, st);
    if (kw) DIMX_HIP(hipFreeAsync(kw, st));
    return rc;
}

int dimx_op_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int H, int Lq, int Lk,
                      int D, int ldq, int ldk, int ld_vt, int ldo, float scale, int causal, const int32_t* lens,
                      const uint8_t* kmask, void* stream) {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    a.q = q; a.k = k; a.vt = vt; a.o = out;
    a.q_sb = (long)Lq * ldq; a.q_st = ldq; a.q_sh = D;
    a.k_sb = (long)Lk * ldk; a.k_st = ldk; a.k_sh = D;
    a.v_sb = (long)H * D * ld_vt; a.v_sh = (long)D * ld_vt; a.v_sd = ld_vt;
    a.o_sb = (long)Lq * ldo; a.o_st = ldo; a.o_sh = D;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.D = D;
    a.scale = scale;
    a.causal = causal;
    a.lens = lens;
    a.kmask = kmask;
    a.kmask_ld = Lk;
    return op_attention_with_scratch(a, (hipStream_t)stream);
}

int dimx_op_attention_rowv(const void* q, const void* k, const void* v, void* out, int B, int H, int Lq, int Lk, int D, int ldq,
                           int ldk, int ldv, int ldo, float scale, int causal, const int32_t* lens, const uint8_t* kmask,
                           void* stream) {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = DIMX_BF16;
    a.q = q; a.k = k; a.vt = v; a.o = out;
    a.q_sb = (long)Lq * ldq; a.q_st = ldq; a.q_sh = D;
    a.k_sb = (long)Lk * ldk; a.k_st = ldk; a.k_sh = D;
    a.v_rows = 1;
    a.v_sb = (long)Lk * ldv; a.v_st = ldv; a.v_sh = D;
    a.o_sb = (long)Lq * ldo; a.o_st = ldo; a.o_sh = D;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.D = D;
    a.scale = scale;
    a.causal = causal;
    a.lens = lens;
    a.kmask = kmask;
    a.kmask_ld = Lk;
    return op_attention_with_scratch(a, (hipStream_t)stream);
}

int dimx_op_decode_attn(int dtype, const void* q, const void* kcache, const void* vcache, void* out, int B, int H,
                        int Tmax, int n_keys, float scale, const uint8_t* kmask, int nsplit, int q_is_f32,
                        void* stream) {
    DecodeAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    a.q = q;
    a.q_ld = H * 64;
    a.kcache = const_cast<void*>(kcache);
    a.vcache = const_cast<void*>(vcache);
    a.Tmax = Tmax;
    a.out = out;
    a.o_ld = H * 64;
    a.B = B;
    a.H = H;
    a.n_keys = n_keys;
    a.kmask = kmask;
    a.kmask_ld = n_keys;
    a.scale = scale;
    a.force_nsplit = nsplit;
    a.q_f32 = q_is_f32 ? 1 : 0;
    a.nslab = 1;
    return launch_decode_attn(a, (hipStream_t)stream);
}

int dimx_op_decode_attn_self(int dtype, const void* qkv, int ld, void* kcache, void* vcache, void* out, int B, int H,
                             int Tmax, const int32_t* step_dev, float scale, int q_is_f32, void* stream) {
    DecodeAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    const size_t es = q_is_f32 ? 4 : dtype_size(dtype);
    a.q = qkv;
    a.q_ld = ld;
    a.knew = (const unsigned char*)qkv + (size_t)H * 64 * es;
    a.vnew = (const unsigned char*)qkv + (size_t)2 * H * 64 * es;
    a.kv_ld = ld;
    a.kcache = kcache;
    a.vcache = vcache;
    a.Tmax = Tmax;
    a.out = out;
    a.o_ld = H * 64;
    a.B = B;
    a.H = H;
    a.step = step_dev;
    a.scale = scale;
    a.q_f32 = q_is_f32 ? 1 : 0;
    a.nslab = 1;
    return launch_decode_attn(a, (hipStream_t)stream);
}

/* every decode-attention form dimx_generate launches (tests): q / knew / vnew as the cache type or as nslab f32 split-K slabs,
 * the self form reading this step's k / v at q + H*64 / q + 2*H*64 of each slab row, the cross form with a strided key mask,
 * several query rows per clip and a forced wave count */
static int op_decode_attn_ex(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, int self_attn, void* kcache,
                             void* vcache, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys,
                             const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit, int win, int lookahead,
                             void* stream) {
    const int S = rows_per_clip > 1 ? rows_per_clip : 1;
    DIMX_REQUIRE(B > 0 && H > 0 && Tmax > 0, DIMX_ERR_ARG, "op_decode_attn_ex: empty shape");
    DIMX_REQUIRE(nslab >= 1 && nslab <= 8 && (nslab == 1 || q_is_f32), DIMX_ERR_ARG, "op_decode_attn_ex: nslab=%d (1..8, > 1 for f32 q only)",
                 nslab);
    DIMX_REQUIRE(q_ld >= (self_attn ? 3 : 1) * H * 64 && o_ld >= H * 64, DIMX_ERR_ARG, "op_decode_attn_ex: q_ld=%d o_ld=%d too small",
                 q_ld, o_ld);
    DIMX_REQUIRE(nslab == 1 || slab_stride >= (long)B * S * q_ld, DIMX_ERR_ARG, "op_decode_attn_ex: slabs overlap (stride %ld)",
                 slab_stride);
    DIMX_REQUIRE(self_attn ? (step_dev != nullptr && kmask == nullptr && S == 1) : (n_keys >= 1 && n_keys <= Tmax), DIMX_ERR_ARG,
                 "op_decode_attn_ex: self form needs a step counter (no mask, one row per clip); cross form 1 <= n_keys (%d) <= Tmax",
                 n_keys);
    DIMX_REQUIRE(kmask == nullptr || kmask_ld >= n_keys, DIMX_ERR_ARG, "op_decode_attn_ex: kmask_ld=%d < n_keys=%d", kmask_ld, n_keys);
    DecodeAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    a.q = q;
    a.q_ld = q_ld;
    a.q_f32 = q_is_f32 ? 1 : 0;
    a.nslab = nslab;
    a.slab_stride = slab_stride;
    if (self_attn) {
        const size_t es = q_is_f32 ? 4 : dtype_size(dtype);
        a.knew = (const unsigned char*)q + (size_t)H * 64 * es;
        a.vnew = (const unsigned char*)q + (size_t)2 * H * 64 * es;
        a.kv_ld = q_ld;
        a.step = step_dev;
    } else {
        a.n_keys = n_keys;
        a.kmask = kmask;
        a.kmask_ld = kmask_ld;
    }
    a.kcache = kcache;
    a.vcache = vcache;
    a.Tmax = Tmax;
    a.out = out;
    a.o_ld = o_ld;
    a.B = B;
    a.H = H;
    a.rows_per_clip = rows_per_clip;
    a.scale = scale;
    a.force_nsplit = nsplit;
    if (win) {
        a.win = 1;
        a.lookahead = lookahead;
        a.step = step_dev;
    }
    return launch_decode_attn(a, (hipStream_t)stream);
}

int dimx_op_decode_attn_ex(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, int self_attn, void* kcache,
                           void* vcache, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys,
                           const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit, void* stream) {
    return op_decode_attn_ex(dtype, q, q_ld, q_is_f32, nslab, slab_stride, self_attn, kcache, vcache, out, o_ld, B, H, Tmax, step_dev, n_keys,
                             kmask, kmask_ld, rows_per_clip, scale, nsplit, 0, 0, stream);
}

/* the windowed cross form: the keys j < clamp(*step_dev + 2 + lookahead, 1, n_keys) */
int dimx_op_decode_attn_win(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, void* kcache, void* vcache,
                            void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys, const uint8_t* kmask,
                            int kmask_ld, int rows_per_clip, float scale, int nsplit, int lookahead, void* stream) {
    DIMX_REQUIRE(step_dev != nullptr, DIMX_ERR_ARG, "op_decode_attn_win: the windowed form needs a step counter");
    return op_decode_attn_ex(dtype, q, q_ld, q_is_f32, nslab, slab_stride, 0, kcache, vcache, out, o_ld, B, H, Tmax, step_dev, n_keys, kmask,
                             kmask_ld, rows_per_clip, scale, nsplit, 1, lookahead, stream);
}

size_t dimx_mlp_fused_packed_bytes(int C, int F) { return mlp_fused_packed_bytes(C, F); }

int dimx_mlp_fused_pack(const float* w1_host, const float* b1_host, const float* w2_host, int C, int F, void* out_host, size_t out_bytes) {
    DIMX_REQUIRE(w1_host && w2_host && out_host, DIMX_ERR_ARG, "mlp_fused_pack: null argument");
    DIMX_REQUIRE(mlp_fused_packed_bytes(C, F) > 0 && out_bytes >= mlp_fused_packed_bytes(C, F), DIMX_ERR_ARG,
                 "mlp_fused_pack: C = %d F = %d unsupported or the output buffer is too small", C, F);
    return mlp_fused_pack(w1_host, b1_host, w2_host, C, F, (uint16_t*)out_host);
}

int dimx_op_mlp_fused_packed(float* x, const void* packed, const float* b2, const float* ln_g, const float* ln_b, int M, int C, int F, int act,
                             void* stream) {
    return launch_mlp_fused(x, packed, b2, ln_g, ln_b, M, C, F, act, (hipStream_t)stream);
}

int dimx_op_mlp_fused(float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2, const float* ln_g,
                      const float* ln_b, int M, int C, int F, int act, void* stream) {
    DIMX_REQUIRE(x && w1_host && w2_host && b2 && ln_g && M > 0, DIMX_ERR_ARG, "op_mlp_fused: null argument");
    const size_t bytes = mlp_fused_packed_bytes(C, F);
    DIMX_REQUIRE(bytes > 0, DIMX_ERR_ARG, "op_mlp_fused: C = %d F = %d not supported", C, F);
    std::vector<uint16_t> img(bytes / 2);
    DIMX_TRY(mlp_fused_pack(w1_host, b1_host, w2_host, C, F, img.data()));
    void* p = nullptr;
    DIMX_HIP(hipMalloc(&p, bytes));
    int rc = DIMX_OK;
    if (hipMemcpy(p, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) rc = DIMX_ERR_HIP;
    if (rc == DIMX_OK) rc = launch_mlp_fused(x, p, b2, ln_g, ln_b, M, C, F, act, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == DIMX_OK) rc = DIMX_ERR_HIP;
    (void)hipFree(p);
    return rc;
}

int dimx_op_add_slabs_layernorm(int out_dtype, float* x, const float* slabs, int nslab, long slab_stride, void* y,
                                const float* gamma, int M, int C, void* stream) {
    return launch_add_slabs_layernorm(out_dtype, x, slabs, nslab, slab_stride, y, gamma, M, C, (hipStream_t)stream);
}

int dimx_op_chain(const void* A1, int K1, const void* W1, float* x, const float* slabs, int nslab, const float* gamma,
                  void* y, const void* W2, int N2, float* out2, int B, int C, void* scratch, void* stream) {
    DIMX_REQUIRE(scratch && x && y && gamma, DIMX_ERR_ARG, "op_chain: null argument");
    int dev = 0, cus = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    ChainArgs c;
    memset(&c, 0, sizeof(c));
    unsigned* u = (unsigned*)scratch;  // [0..127] counters, [128] step, [129] error flags, [256..511] claim stamps, then xr
    c.B = B;
    c.C = C;
    if (W1) {
        c.g1.W = W1; c.g1.N = C; c.g1.K = K1; c.g1.ldw = K1;
        c.A1 = A1; c.lda1 = K1;
        c.xr = (float*)(u + 512);
    }
    c.x = x;
    c.slabs = slabs;
    c.nslab = nslab;
    c.slab_stride = (long)B * C;
    c.y = y;
    c.gamma = gamma;
    if (W2) {
        c.g2.W = W2; c.g2.N = N2; c.g2.K = C; c.g2.ldw = C;
        c.out2 = out2; c.ld_out2 = N2;
    }
    c.counters = u;
    c.seen = u + 256;
    c.step = (const int32_t*)(u + 128);
    c.err = u + 129;
    DIMX_REQUIRE(chain_supported(c, cus), DIMX_ERR_ARG, "op_chain: shape not supported on this device (%d CUs)", cus);
    DIMX_HIP(hipMemsetAsync(u, 0, 512 * 4, (hipStream_t)stream));
    return launch_chain(c, (hipStream_t)stream);
}

int dimx_op_chain_ln(const void* A1, int K1, const void* W1, float* x, void* y, float* stats, const void* W2s,
                     const float* colsum2, int N2, float* out2, int B, int C, void* scratch, void* stream) {
    DIMX_REQUIRE(scratch && x && y && stats && A1 && W1, DIMX_ERR_ARG, "op_chain_ln: null argument");
    int dev = 0, cus = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    ChainArgs c;
    memset(&c, 0, sizeof(c));
    unsigned* u = (unsigned*)scratch;
    c.B = B;
    c.C = C;
    c.g1.W = W1; c.g1.N = C; c.g1.K = K1; c.g1.ldw = K1;
    c.A1 = A1; c.lda1 = K1;
    c.xr = (float*)(u + 512);
    c.x = x;
    c.y = y;
    c.gamma = (const float*)x;  /* unused by the deferred form, must be non-null */
    c.defer = 1;
    c.stats = stats;
    if (W2s) {
        c.g2.W = W2s; c.g2.N = N2; c.g2.K = C; c.g2.ldw = C;
        c.out2 = out2; c.ld_out2 = N2;
        c.colsum2 = colsum2;
    }
    c.counters = u;
    c.seen = u + 256;
    c.step = (const int32_t*)(u + 128);
    c.err = u + 129;
    DIMX_REQUIRE(chain_supported(c, cus), DIMX_ERR_ARG, "op_chain_ln: shape not supported on this device (%d CUs)", cus);
    DIMX_HIP(hipMemsetAsync(u, 0, 512 * 4, (hipStream_t)stream));
    return launch_chain(c, (hipStream_t)stream);
}

int dimx_op_gemm_ln(int out_dtype, const void* A, const void* Ws, void* C, int M, int N, int K, const float* bias, int act,
                    const float* stats, const float* colsum, void* stream) {
    DIMX_REQUIRE(A && Ws && C && stats && colsum && M >= 1 && M <= 256, DIMX_ERR_ARG, "op_gemm_ln: bad argument");
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = DIMX_BF16;
    g.out_dtype = out_dtype;
    g.A = A; g.lda = K;
    g.W = Ws; g.ldw = K;
    g.M = M; g.N = N; g.K = K;
    g.bias = bias;
    g.act = act;
    g.ln_stats = stats;
    g.ln_colsum = colsum;
    g.ln_C = K;
    gemm_set_plain_out(g, C, N);
    return launch_gemm(g, (hipStream_t)stream);
}

int dimx_op_layer_chain(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                        int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                        const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                        int call_index, float scale, void* scratch, void* prof, void* stream) {
    DIMX_REQUIRE(qkv && sk && sv && ck && cv && w_so && w_cq && colsum_cq && w_co && x && y && o && qc && stats && step && scratch,
                 DIMX_ERR_ARG, "op_layer_chain: null argument");
    constexpr int H = 12, D = 64, inner = H * D, C = 1152;
    LayerChainArgs lc;
    memset(&lc, 0, sizeof(lc));
    lc.B = B;
    lc.C = C;
    DecodeAttnArgs& sa = lc.sa;
    sa.dtype = DIMX_BF16;
    sa.q = qkv; sa.q_ld = 3 * inner; sa.q_f32 = 1; sa.nslab = nslab; sa.slab_stride = slab_stride;
    sa.knew = qkv + inner; sa.vnew = qkv + 2 * inner; sa.kv_ld = 3 * inner;
    sa.kcache = sk; sa.vcache = sv; sa.Tmax = T;
    sa.out = o; sa.o_ld = inner; sa.B = B; sa.H = H; sa.step = step; sa.scale = scale;
    DecodeAttnArgs& ca = lc.ca;
    ca.dtype = DIMX_BF16;
    ca.q = qc; ca.q_ld = inner; ca.q_f32 = 1; ca.nslab = 1; ca.slab_stride = (long)B * inner;
    ca.kcache = (void*)ck; ca.vcache = (void*)cv; ca.Tmax = Tp;
    ca.out = o; ca.o_ld = inner; ca.B = B; ca.H = H; ca.n_keys = n_keys; ca.kmask = kmask; ca.kmask_ld = n_keys; ca.scale = scale;
    lc.g_so.W = w_so; lc.g_so.N = C; lc.g_so.K = inner; lc.g_so.ldw = inner;
    lc.g_cq.W = w_cq; lc.g_cq.N = inner; lc.g_cq.K = C; lc.g_cq.ldw = C;
    lc.g_co.W = w_co; lc.g_co.N = C; lc.g_co.K = inner; lc.g_co.ldw = inner;
    lc.o = o; lc.ld_o = inner;
    lc.x = x; lc.y = y; lc.stats = stats; lc.colsum_cq = colsum_cq;
    lc.qc = qc; lc.ld_qc = inner;
    lc.counters = (unsigned*)scratch;
    lc.seen = lc.counters + 8 * 16;
    lc.err = lc.counters + 768;
    lc.step = nullptr;          // the counters' epoch is the call index; the self-attention reads its own step pointer (sa.step)
    lc.epoch_add = call_index;
    lc.prof = (unsigned long long*)prof;
    lc.sc_stride = ((T > n_keys ? T : n_keys) + 15) / 16 * 16;
    int cu = 0, dev = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
    DIMX_REQUIRE(layer_chain_supported(lc, cu), DIMX_ERR_ARG, "op_layer_chain: not supported here (B = %d needs 129..256 clips, a 256-CU device)", B);
    return launch_layer_chain(lc, (hipStream_t)stream);
}

int dimx_op_sample(const float* logits, int R, int top_k, float temperature, const float* exp_noise, uint64_t seed,
                   uint64_t step, int32_t* tokens, void* stream) {
    return dimx_op_sample_filtered(logits, R, DIMX_FILTER_TOP_K, top_k, 0.f, 0.f, temperature, exp_noise, seed, step, tokens, nullptr,
                                   stream);
}

int dimx_op_sample_filtered(const float* logits, int R, int kind, int top_k, float a, float b, float temperature,
                            const float* exp_noise, uint64_t seed, uint64_t step, int32_t* tokens, uint8_t* keep_out,
                            void* stream) {
    DIMX_TRY(check_sampler_filter(kind, a, b));
    SampleArgs sm;
    sm.logits = logits; sm.ld_logits = 512; sm.R = R; sm.nslab = 1; sm.rows_total = R; sm.tokens = tokens; sm.tok_ld = 1;
    sm.top_k = kind == DIMX_FILTER_TOP_K ? top_k : 0; sm.temperature = temperature; sm.seed = seed;
    sm.noise = exp_noise; sm.step_host = exp_noise ? 0 : step;   // the [R,512] slice of this step (step only salts the generator)
    sm.filt = SampleFilter{kind, a, b, keep_out};
    return launch_sample(sm, (hipStream_t)stream);
}

}  // extern "C"
