// train.hip -- the training step of the DIM-Listener fine-tuning model on hand-written HIP kernels.
//
// Reference: train_epoch (code/x_engine_pt.py:9-60) as driven by code/finetune_s2s_pretrain.py:105-143 (AdamW lr 1e-5,
// clip 1.0, both VQ-VAEs frozen :348-366).  What carries gradient is the teacher-forced path of SLMFT.forward(mode='train')
// (code/seq2seq_pretrain.py:496-514): encoder_s -> encoder_joint -> norm_s -> context -> AutoregressiveWrapper.forward ->
// cross entropy (the continuous loss has no gradient path in the reference either: its `pred` comes from an argmax).
//
// The reference leaves the backward pass to autograd; here forward and backward are explicit:
//   * every Linear, forward and both adjoints, is the library's GEMM C = A[M,K] . W[N,K]^T (gemm.hip / gemm256.hip; exact-f32
//     MFMA in the parity mode, bf16 MFMA with f32 accumulation in the perf mode): y = x . W^T directly, dx = dy . (W^T)^T
//     with a transposed operand copy of W made once per step, dW = dy^T . (x^T)^T with transposed copies of dy and x
//     (zero-padded along the contraction, train_kernels.hip);
//   * attention, LayerNorm, GELU, cross entropy, the embedding / positional / patch tables and the optimiser are the kernels of
//     train_kernels.hip;
//   * parameters, gradients and the AdamW moments live in FLAT f32 arenas owned by the caller (one float per parameter, the
//     layout is reported by dimx_train_param_info), so the multi-GPU gradient average is ONE all-reduce of one buffer
//     (RCCL over xGMI is per-link bound: one large collective, no per-tensor traffic), and the master weights stay f32.
// Activations needed by the backward pass are kept in the caller's workspace (dimx_train_workspace_bytes).
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <string>
#include <vector>

#include "model.hpp"
#include "train.hpp"

namespace dimx {
namespace {

struct PInfo {
    std::string name;
    long off, numel;
    int rows, cols;  // matrices: [rows, cols]; vectors: rows = 1
};

struct Lin {          // one Linear of the stack
    long w = -1, b = -1;  // offsets into the flat arenas (b < 0: no bias)
    int N = 0, K = 0;
    void* w_op = nullptr;   // [N][Kp] operand copy (this step)
    void* wt_op = nullptr;  // [K][Np] transposed operand copy
    // head-padded weights of the VQ attention: the operand copies are made from an f32 scratch copy of the weight (src) and the
    // weight gradient lands in a scratch of the same shape (gdst) before it is compacted into the arena
    const float* src = nullptr;
    float* gdst = nullptr;
};

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

struct TrainPlan {
    std::vector<PInfo> params;
    std::map<std::string, int> index;
    long total = 0;
};

// ---------------------------------------------------------------------------------------------------------------- plan builder
// Lays a step's tensors out in its flat arenas in the order they are added (deterministic: the caller's arenas follow it).  `tag`
// is the step's prefix in error messages.  Name lists that several steps share are written here once.
struct PlanBuilder {
    TrainPlan& p;
    dimx_handle h;
    const char* tag;
    const dimx_dims& d;
    PlanBuilder(TrainPlan& p_, dimx_handle h_, const char* tag_) : p(p_), h(h_), tag(tag_), d(h_->d) {}

    // held = false: a tensor the engine itself does not hold (training-only tables), laid out at the shape given
    int add(const std::string& name, int rows, int cols, bool held = true) {
        const long n = (long)rows * cols;
        if (held) {
            auto it = h->host.find(name);
            DIMX_REQUIRE(it != h->host.end(), DIMX_ERR_WEIGHT, "%s: weight %s was not loaded", tag, name.c_str());
            long have = 1;
            for (auto sz : it->second.shape) have *= sz;
            DIMX_REQUIRE(have == n, DIMX_ERR_WEIGHT, "%s: %s has %ld elements, expected %d x %d", tag, name.c_str(), have, rows, cols);
        }
        p.index[name] = (int)p.params.size();
        p.params.push_back(PInfo{name, p.total, n, rows, cols});
        p.total += (n + 3) / 4 * 4;  // 16-byte aligned tensors
        return DIMX_OK;
    }
    // the optional tensors of another x-transformers release (model.hip: optional_key) are on the inference path only: the steps
    // have no gradient for them, so they refuse them instead of training around them
    int refuse_optional_biases() {
        for (const auto& kv : h->host) {
            const std::string& nm = kv.first;
            const bool opt = nm.size() > 16 && (nm.compare(nm.size() - 15, 15, "project_in.bias") == 0 || nm.compare(nm.size() - 14, 14, "to_logits.bias") == 0);
            DIMX_REQUIRE(!opt, DIMX_ERR_STATE, "%s: %s is loaded; the training step implements the bias-free project_in / to_logits only", tag, nm.c_str());
        }
        return DIMX_OK;
    }
    // x-transformers sublayers of width C: pre-norm gain + attention, pre-norm gain + feed-forward
    int xt_attn(const std::string& l, int C) {
        const int inner = d.heads * d.dim_head;
        DIMX_TRY(add(l + "0.0.weight", 1, C));
        DIMX_TRY(add(l + "1.to_q.weight", inner, C));
        DIMX_TRY(add(l + "1.to_k.weight", inner, C));
        DIMX_TRY(add(l + "1.to_v.weight", inner, C));
        return add(l + "1.to_out.weight", C, inner);
    }
    int xt_ff(const std::string& l, int C) {
        DIMX_TRY(add(l + "0.0.weight", 1, C));
        DIMX_TRY(add(l + "1.ff.0.0.weight", C * d.ff_mult, C));
        DIMX_TRY(add(l + "1.ff.0.0.bias", 1, C * d.ff_mult));
        DIMX_TRY(add(l + "1.ff.2.weight", C, C * d.ff_mult));
        return add(l + "1.ff.2.bias", 1, C);
    }
    // an encoder (width d.dim, layers: self, ff) over inputs of in_cols columns
    int xt_encoder(const std::string& e, int in_cols) {
        DIMX_TRY(add(e + "project_in.weight", d.dim, in_cols));
        DIMX_TRY(add(e + "pos_emb.emb.weight", d.max_seq_len, d.dim));
        for (int i = 0; i < d.enc_depth; ++i) {
            DIMX_TRY(xt_attn(e + "attn_layers.layers." + std::to_string(2 * i) + ".", d.dim));
            DIMX_TRY(xt_ff(e + "attn_layers.layers." + std::to_string(2 * i + 1) + ".", d.dim));
        }
        return add(e + "attn_layers.final_norm.weight", 1, d.dim);
    }
    // a decoder (width DD = context width, layers: self, cross, ff); abs_pos: it has an absolute positional table
    int xt_decoder(const std::string& dn, int DD, bool abs_pos) {
        DIMX_TRY(add(dn + "token_emb.emb.weight", d.num_tokens, DD));
        if (abs_pos) DIMX_TRY(add(dn + "pos_emb.emb.weight", d.max_seq_len, DD));
        for (int i = 0; i < d.dec_depth; ++i) {
            DIMX_TRY(xt_attn(dn + "attn_layers.layers." + std::to_string(3 * i) + ".", DD));
            DIMX_TRY(xt_attn(dn + "attn_layers.layers." + std::to_string(3 * i + 1) + ".", DD));
            DIMX_TRY(xt_ff(dn + "attn_layers.layers." + std::to_string(3 * i + 2) + ".", DD));
        }
        DIMX_TRY(add(dn + "attn_layers.final_norm.weight", 1, DD));
        return add(dn + "to_logits.weight", d.num_tokens, DD);
    }
    // the transformer blocks of a VQ-VAE half (net = "...encoder_transformer.net." / "...decoder_transformer.net.")
    int vq_blocks(const std::string& net) {
        const int H = d.vq_hidden, I = d.vq_inter;
        for (int i = 0; i < d.vq_layers; ++i) {
            const std::string a = net + std::to_string(2 * i) + ".fn.";
            const std::string m = net + std::to_string(2 * i + 1) + ".fn.";
            DIMX_TRY(add(a + "norm.weight", 1, H));
            DIMX_TRY(add(a + "norm.bias", 1, H));
            DIMX_TRY(add(a + "fn.to_qkv.weight", 3 * H, H));
            DIMX_TRY(add(a + "fn.to_out.weight", H, H));
            DIMX_TRY(add(a + "fn.to_out.bias", 1, H));
            DIMX_TRY(add(m + "norm.weight", 1, H));
            DIMX_TRY(add(m + "norm.bias", 1, H));
            DIMX_TRY(add(m + "fn.l1.weight", I, H));
            DIMX_TRY(add(m + "fn.l1.bias", 1, I));
            DIMX_TRY(add(m + "fn.l2.weight", H, I));
            DIMX_TRY(add(m + "fn.l2.bias", 1, H));
        }
        return DIMX_OK;
    }
    // a VQ-VAE decoder that trains behind a frozen codebook (c = "speaker_vq.decoder." / "listener_vq.decoder."), state-dict order
    int vq_decoder(const std::string& c) {
        const int H = d.vq_hidden;
        DIMX_TRY(add(c + "decoder_linear_embedding_pre.net.weight", H, d.vq_zdim));
        DIMX_TRY(add(c + "decoder_linear_embedding_pre.net.bias", 1, H));
        DIMX_TRY(add(c + "expander.0.0.weight", H, 5 * H));   // [out][in][5]: rows of in * 5 + tap
        DIMX_TRY(add(c + "expander.0.0.bias", 1, H));
        DIMX_TRY(add(c + "decoder_linear_embedding.net.weight", H, H));
        DIMX_TRY(add(c + "decoder_linear_embedding.net.bias", 1, H));
        DIMX_TRY(vq_blocks(c + "decoder_transformer.net."));
        return add(c + "vertice_map_reverse.weight", d.vq_in_dim, H);
    }
};

// The DIM-Listener steps (fine-tuning, legacy generator, SLM pre-training: one per handle variant): every tensor the reference's
// optimiser would update with a non-zero gradient on that path, in state-dict order of the stack
int build_plan(dimx_handle h, TrainPlan& p) {
    PlanBuilder b(p, h, "train");
    const dimx_dims& d = h->d;
    DIMX_TRY(b.refuse_optional_biases());
    const int DD = d.dim + d.dim_a;  // decoder width = context width
    if (d.variant == 1) {
        // legacy ListenerGenerator (code/seq2seq.py:165-176): the generator, the listener VQ-VAE's DECODER and the id-conditioning
        // layers train; both VQ encoders / codebooks are frozen
        DIMX_TRY(b.xt_encoder("generator.encoder.", d.spk_face_quan_num * d.vq_zdim));
        DIMX_TRY(b.xt_decoder("generator.decoder.net.", DD, true));
        DIMX_TRY(b.vq_decoder("listener_vq.decoder."));
        // the id-conditioning tables are training-only (the engine does not hold them): fixed shape, code/seq2seq.py:205-210
        DIMX_TRY(b.add("listener_embeddings.weight", 100, 256, false));
        DIMX_TRY(b.add("fc_listener.weight", d.dim, 256, false));
        return b.add("fc_listener.bias", 1, d.dim, false);
    }
    if (d.variant == 2) {
        // SLM pre-training (code/seq2seq_pretrain.py:98-113): everything but the VQ-VAEs' encoders and codebooks trains -- the three
        // encoders, the decoder with its absolute positional table, the stream norms / patch embeddings and BOTH VQ-VAE decoders
        // (project_out of the encoders is never called: no gradient, not in the arena)
        for (const char* n : {"patch_embed_s", "patch_embed_l"}) DIMX_TRY(b.add(n, 1, d.dim_in));
        for (const char* n : {"patch_embed_dec_s", "patch_embed_dec_l", "norm_s.weight", "norm_s.bias", "norm_l.weight", "norm_l.bias", "norm.weight",
                              "norm.bias"})
            DIMX_TRY(b.add(n, 1, d.dim));
        DIMX_TRY(b.xt_encoder("encoder_s.", d.dim_in));
        DIMX_TRY(b.xt_encoder("encoder_l.", d.dim_in));
        DIMX_TRY(b.xt_encoder("encoder_joint.", d.dim));
        DIMX_TRY(b.xt_decoder("decoder_joint.net.", DD, true));
        DIMX_TRY(b.vq_decoder("speaker_vq.decoder."));
        return b.vq_decoder("listener_vq.decoder.");
    }
    DIMX_TRY(b.add("patch_embed_s", 1, d.dim_in));
    DIMX_TRY(b.add("patch_embed_dec_s", 1, d.dim));
    DIMX_TRY(b.add("norm_s.weight", 1, d.dim));
    DIMX_TRY(b.add("norm_s.bias", 1, d.dim));
    DIMX_TRY(b.xt_encoder("encoder_s.", d.dim_in));
    DIMX_TRY(b.xt_encoder("encoder_joint.", d.dim));
    return b.xt_decoder("decoder_joint.net.", DD, false);
}

// The VQ-VAE's own step (slot `which` of the handle: 0 = speaker_vq., 1 = listener_vq.): every parameter of VQAutoEncoder
// (code/models/stage1_BIWI.py:10-20) -- encoder, decoder, codebook; the two pe buffers are not parameters.
int build_vq_plan(dimx_handle h, int which, TrainPlan& p) {
    const dimx_dims& d = h->d;
    const VQGeom& vg = h->vqg[which];
    DIMX_REQUIRE(vg.in_dim == 56 && vg.hidden == 384 && vg.heads == 8 && vg.zdim == 128 && vg.fqn == 1 && vg.n_embed == 512 &&
                     vg.has_decoder && d.vq_hidden == 384 && d.vq_heads == 8 && d.vq_zdim == 128,
                 DIMX_ERR_ARG, "train_vq: slot %d is not the 56 / 384 / 8 x 48 / 128 VQ-VAE the step is written for", which);
    PlanBuilder b(p, h, "train_vq");
    const int H = d.vq_hidden;
    const std::string pre = which == 0 ? "speaker_vq." : "listener_vq.", e = pre + "encoder.", c = pre + "decoder.";
    DIMX_TRY(b.add(e + "vertice_mapping.0.weight", H, vg.in_dim));
    DIMX_TRY(b.add(e + "vertice_mapping.0.bias", 1, H));
    DIMX_TRY(b.add(e + "squasher.0.0.weight", H, 5 * H));   // [out][in][5]: rows of in * 5 + tap
    DIMX_TRY(b.add(e + "squasher.0.0.bias", 1, H));
    DIMX_TRY(b.vq_blocks(e + "encoder_transformer.net."));
    DIMX_TRY(b.add(e + "encoder_linear_embedding.net.weight", H, H));
    DIMX_TRY(b.add(e + "encoder_linear_embedding.net.bias", 1, H));
    DIMX_TRY(b.add(e + "encoder_linear_embedding_post.net.weight", vg.zdim, H));
    DIMX_TRY(b.add(e + "encoder_linear_embedding_post.net.bias", 1, vg.zdim));
    DIMX_TRY(b.add(c + "expander.0.0.weight", H, 5 * H));
    DIMX_TRY(b.add(c + "expander.0.0.bias", 1, H));
    DIMX_TRY(b.vq_blocks(c + "decoder_transformer.net."));
    DIMX_TRY(b.add(c + "decoder_linear_embedding.net.weight", H, H));
    DIMX_TRY(b.add(c + "decoder_linear_embedding.net.bias", 1, H));
    DIMX_TRY(b.add(c + "decoder_linear_embedding_pre.net.weight", H, vg.zdim));
    DIMX_TRY(b.add(c + "decoder_linear_embedding_pre.net.bias", 1, H));
    DIMX_TRY(b.add(c + "vertice_map_reverse.weight", vg.in_dim, H));
    return b.add(pre + "quantize.embedding.weight", vg.n_embed, vg.zdim);
}

// The DIM-Speaker converter's step: the head of EmocaConverter that dimx_mesh_head runs (code/seq2seq_pretrain.py:801-819), in
// state-dict order.  Every tensor is padded to 16 bytes inside the arena; the V-wide bias relies on that pad (conv_run).
int build_conv_plan(dimx_handle h, TrainPlan& p) {
    DIMX_REQUIRE(h->d.mesh_dim > 0, DIMX_ERR_STATE, "train_conv: the handle was created without a mesh head (dimx_dims.mesh_dim = 0)");
    DIMX_REQUIRE(h->d.mesh_dim % 3 == 0 && h->d.vq_in_dim % 4 == 0, DIMX_ERR_ARG, "train_conv: mesh_dim %d must be 3 x vertices", h->d.mesh_dim);
    PlanBuilder b(p, h, "train_conv");
    const std::string l = "vertice_map_reverse_lstm.";
    for (int layer = 0; layer < 2; ++layer)
        for (int dir = 0; dir < 2; ++dir) {
            const std::string sfx = "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
            DIMX_TRY(b.add(l + "weight_ih" + sfx, 1536, layer ? 768 : h->d.vq_in_dim));
            DIMX_TRY(b.add(l + "weight_hh" + sfx, 1536, 384));
            DIMX_TRY(b.add(l + "bias_ih" + sfx, 1, 1536));
            DIMX_TRY(b.add(l + "bias_hh" + sfx, 1, 1536));
        }
    DIMX_TRY(b.add("vertice_map_reverse.0.weight", 768, 768));
    DIMX_TRY(b.add("vertice_map_reverse.0.bias", 1, 768));
    DIMX_TRY(b.add("vertice_map_reverse.2.weight", h->d.mesh_dim, 768));
    return b.add("vertice_map_reverse.2.bias", 1, h->d.mesh_dim);
}

// The DIM-Speaker fine-tuning step: what SpeakerSLMFT.forward(mode='train') (code/seq2seq_pretrain.py:708-757) leaves a gradient
// on -- the cross entropy reaches decoder_joint.* (positional table included), patch_embed_dec_l and speaker_embed.weight (dense:
// AdamW decays the rows no clip names too), the EMOCA loss reaches speaker_vq.decoder.* only (the arg-max cuts the graph).
// Everything else keeps grad = None in the reference (its AdamW and its clip norm skip those tensors) and is not in the arena.
int build_spk_plan(dimx_handle h, TrainPlan& p) {
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(h->variant == 2 && d.mesh_dim > 0, DIMX_ERR_STATE,
                 "train_spk: the handle is not a speaker handle (variant 2 with dimx_dims.mesh_dim > 0)");
    DIMX_REQUIRE(h->spk_embed_rows > 0, DIMX_ERR_WEIGHT, "train_spk: speaker_embed.weight [rows, %d] was not loaded", d.dim);
    PlanBuilder b(p, h, "train_spk");
    DIMX_TRY(b.refuse_optional_biases());
    DIMX_TRY(b.add("patch_embed_dec_l", 1, d.dim));
    DIMX_TRY(b.xt_decoder("decoder_joint.net.", d.dim + d.dim_a, true));
    DIMX_TRY(b.vq_decoder("speaker_vq.decoder."));
    return b.add("speaker_embed.weight", h->spk_embed_rows, d.dim, false);   // not held by the engine: the shape it was loaded with
}

// State of a handle's DIM-Listener steps: the side stream the weight-gradient GEMMs run on, and the captured step.
constexpr int kSideSlots = 3;
struct StepGraphKey {
    const void *params, *grads, *v_speaker, *v_audio, *mask, *z_l, *kv_mask, *loss_out, *logits_out, *ws;
    size_t ws_bytes;
    int B, T, at, side;
    int win_on, win_lookahead;   // dimx_set_train_lookahead: a step captured under one setting is never replayed under another
    const void* cond_keep;       // dimx_set_train_cond_keep: the pointer is a kernel argument, its contents are read on the device
    bool operator==(const StepGraphKey& o) const {
        return params == o.params && grads == o.grads && v_speaker == o.v_speaker && v_audio == o.v_audio && mask == o.mask && z_l == o.z_l &&
               kv_mask == o.kv_mask && loss_out == o.loss_out && logits_out == o.logits_out && ws == o.ws && ws_bytes == o.ws_bytes &&
               B == o.B && T == o.T && at == o.at && side == o.side && win_on == o.win_on && win_lookahead == o.win_lookahead &&
               cond_keep == o.cond_keep;
    }
};
struct TrainState {
    const TrainPlan* plan = nullptr;   // the handle's kPlanMain plan
    hipStream_t side = nullptr, cap = nullptr;
    hipEvent_t ev_main[kSideSlots] = {}, ev_side[kSideSlots] = {}, ev_join = nullptr;
    StepGraphKey last_key{}, graph_key{};
    bool have_last = false;
    hipGraphExec_t exec = nullptr;
    long graph_launches = 0, eager_runs = 0, graph_nodes = 0;
    void drop_graph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    ~TrainState() {
        drop_graph();
        for (int i = 0; i < kSideSlots; ++i) {
            if (ev_main[i]) (void)hipEventDestroy(ev_main[i]);
            if (ev_side[i]) (void)hipEventDestroy(ev_side[i]);
        }
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (side) (void)hipStreamDestroy(side);
        if (cap) (void)hipStreamDestroy(cap);
    }
};

// the side stream and its events (first live step of a handle)
int side_ready(TrainState& ts) {
    if (ts.side) return DIMX_OK;
    DIMX_HIP(hipStreamCreateWithFlags(&ts.side, hipStreamNonBlocking));
    for (int i = 0; i < kSideSlots; ++i) {
        DIMX_HIP(hipEventCreateWithFlags(&ts.ev_main[i], hipEventDisableTiming));
        DIMX_HIP(hipEventCreateWithFlags(&ts.ev_side[i], hipEventDisableTiming));
    }
    DIMX_HIP(hipEventCreateWithFlags(&ts.ev_join, hipEventDisableTiming));
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- per-handle registry
// Everything the training steps keep for a handle: the plans of the steps it was asked for (built on first use) and the state of
// the DIM-Listener steps.  Handles are few and long-lived; dimx_destroy erases the entry (train_forget).
enum PlanKind { kPlanMain, kPlanVqSpeaker, kPlanVqListener, kPlanConv, kPlanSpk, kPlanVqNoSlot /* a `which` that names no slot */ };
inline PlanKind vq_plan_kind(int which) { return which == 0 ? kPlanVqSpeaker : which == 1 ? kPlanVqListener : kPlanVqNoSlot; }
const char* const kPlanTag[] = {"train", "train_vq", "train_vq", "train_conv", "train_spk", "train_vq"};   // a kind's prefix in messages
struct HandleTrain {
    std::map<int, TrainPlan> plans;   // by PlanKind
    TrainState state;
};
std::mutex g_plans_mu;
std::map<dimx_handle, HandleTrain>& train_map() {
    static std::map<dimx_handle, HandleTrain> m;
    return m;
}
int plan_of(dimx_handle h, PlanKind kind, TrainPlan** out) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "%s: null handle", kPlanTag[kind]);
    DIMX_REQUIRE(kind != kPlanVqNoSlot, DIMX_ERR_ARG, "train_vq: which must be 0 (speaker_vq.) or 1 (listener_vq.)");
    std::lock_guard<std::mutex> lock(g_plans_mu);
    auto& plans = train_map()[h].plans;
    auto it = plans.find(kind);
    // the DIM-Speaker plan ends with speaker_embed.weight at the row count it was loaded with: a reload with another count replaces it
    if (it != plans.end() && kind == kPlanSpk && it->second.params.back().rows != h->spk_embed_rows) {
        plans.erase(it);
        it = plans.end();
    }
    if (it == plans.end()) {
        TrainPlan p;
        switch (kind) {
            case kPlanMain: DIMX_TRY(build_plan(h, p)); break;
            case kPlanConv: DIMX_TRY(build_conv_plan(h, p)); break;
            case kPlanSpk: DIMX_TRY(build_spk_plan(h, p)); break;
            default: DIMX_TRY(build_vq_plan(h, kind == kPlanVqListener ? 1 : 0, p)); break;
        }
        it = plans.emplace(kind, std::move(p)).first;
    }
    *out = &it->second;
    return DIMX_OK;
}
int state_of(dimx_handle h, TrainState** out) {
    TrainPlan* plan;
    DIMX_TRY(plan_of(h, kPlanMain, &plan));
    std::lock_guard<std::mutex> lock(g_plans_mu);
    TrainState& ts = train_map()[h].state;
    ts.plan = plan;
    *out = &ts;
    return DIMX_OK;
}
// one body each behind the dimx_<tag>_num_params / _total / _param_info entry points
int layout_num_params(dimx_handle h, PlanKind kind) {
    TrainPlan* p;
    const int rc = plan_of(h, kind, &p);
    return rc == DIMX_OK ? (int)p->params.size() : rc;
}
int64_t layout_total(dimx_handle h, PlanKind kind) {
    TrainPlan* p;
    const int rc = plan_of(h, kind, &p);
    return rc == DIMX_OK ? (int64_t)p->total : (int64_t)rc;
}
int layout_param_info(dimx_handle h, PlanKind kind, int i, const char** name, int64_t* offset, int64_t* numel) {
    TrainPlan* p;
    DIMX_TRY(plan_of(h, kind, &p));
    DIMX_REQUIRE(i >= 0 && i < (int)p->params.size() && name && offset && numel, DIMX_ERR_ARG, "%s_param_info: bad index", kPlanTag[kind]);
    *name = p->params[i].name.c_str();
    *offset = p->params[i].off;
    *numel = p->params[i].numel;
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- step context
struct Step {
    dimx_handle h;
    const TrainPlan* plan;
    const float* P;  // parameters (flat, device)
    float* G;        // gradients (flat, device)
    Arena* ar;
    hipStream_t st;
    int at;          // operand type of the GEMMs
    int bk;          // k-tile of the operand type (64 bf16 / 32 f32)
    FinTable fin;    // column reductions whose partial rows are added by ONE launch at the end of the backward pass
    float* pool = nullptr;   // their partial rows: a region of its own (they outlive the sublayers' rolled-back scratch)
    size_t pool_off = 0, pool_cap = 0;
    bool pool_overflow = false;
    // An overflow hands the pool base back so that the walk can finish, and the run ends in DIMX_ERR_STATE.  No kernel ever
    // writes through such a pointer: every entry point runs the sizing pass (ws == nullptr, nothing launched) first, that pass
    // makes the same pool_f32 calls with the same pool_cap, and its failure returns before the live pass starts.
    float* pool_f32(size_t n_) {
        n_ = (n_ + 63) / 64 * 64;
        if (pool_off + n_ > pool_cap) {
            pool_overflow = true;
            return pool;
        }
        float* q = pool + pool_off;
        pool_off += n_;
        return q;
    }
    int B, T, M, n, Md;
    // weight gradients on a side stream: dW = dy^T . x^T^T does not feed the rest of the backward pass, and at 4 800 rows most of
    // these GEMMs leave CUs idle (81 tiles for a 1152 x 1152 weight), so they run beside the dX chain.  The transposed dy operand
    // lives in one of kSideSlots rotating buffers (the sublayer scratch is rolled back while the side stream may still read it);
    // events order slot reuse.  The same calls build the fork / join edges of the captured graph.
    TrainState* ts = nullptr;
    bool use_side = false;
    void* slot_buf[kSideSlots] = {};
    int slot_n = 0;

    size_t peak = 0;  // high-water mark of the arena: the sizing pass (ws == NULL) walks the same allocation sequence
    PrepTable prep;   // weight operand copies queued by prep_lin, made by ONE launch in flush_prep
    // operand copies of the forward pass's Linear inputs {cast [M][Kp], transposed cast [K][Mp]}, made by one launch per distinct
    // input and kept for the backward pass (dW = dy^T . x needs the transposed one): q / k / v share theirs, the context is copied
    // once for all four cross-attention layers.  Persistent arena allocations: never made inside a region that is rolled back.
    struct OpCopy {
        void* o;
        void* t;
        int Kp, Mp;
    };
    std::map<std::tuple<const float*, int, int, int>, OpCopy> ops;

    // n: rows per clip on the decoder side (T - 1 for the teacher-forced steps)
    Step(dimx_handle h_, const TrainPlan* plan_, const float* P_, float* G_, Arena* ar_, hipStream_t st_, int at_, int B_, int T_, int n_)
        : h(h_), plan(plan_), P(P_), G(G_), ar(ar_), st(st_), at(at_), bk(at_ == DIMX_BF16 ? 64 : 32), B(B_), T(T_), M(B_ * T_), n(n_), Md(B_ * n_) {
        fin.n = 0;
        fin.total_blocks = 0;
        prep.n = 0;
        prep.total_tiles = 0;
    }
    // What a step allocates before its first layer, in this order (the sizing pass and the captured graph depend on the sequence):
    // 2 * kTrSlabs rows of its widest activation -- the column-reduction scratch of the first kernels; nothing reads it any more,
    // it stays because the workspace sizes callers see must not move
    void reserve_part(int width) { (void)f32((size_t)2 * kTrSlabs * width); }
    // the rotating dy^T buffers of the side stream, for the step's widest weight gradient ([widest][rows])
    int use_side_stream(TrainState& ts_, int widest, int rows) {
        ts = &ts_;
        use_side = true;
        const size_t slot = (size_t)widest * pad_to(rows, bk) * es();
        for (int i = 0; i < kSideSlots; ++i) slot_buf[i] = take(slot);
        return live() ? side_ready(ts_) : DIMX_OK;
    }
    // the pool of the deferred column reductions' partial rows (the capacity formula is each step's own knowledge)
    void alloc_pool(size_t cap) {
        pool_cap = cap;
        pool = f32(cap);
        pool_off = 0;
    }
    int zero_grads() {
        if (live()) DIMX_HIP(hipMemsetAsync(G, 0, (size_t)plan->total * sizeof(float), st));
        return DIMX_OK;
    }

    bool live() const { return ar->base != nullptr; }
    size_t es() const { return dtype_size(at); }
    long off(const std::string& name) const { return plan->params[plan->index.at(name)].off; }
    const float* p(const std::string& name) const { return P + off(name); }
    float* g(const std::string& name) const { return G + off(name); }
    void* take(size_t bytes) {
        void* q = ar->take(bytes);
        peak = ar->off > peak ? ar->off : peak;
        // sizing pass (no workspace yet): a distinct, never dereferenced token per allocation instead of NULL, so that
        // everything keyed by a buffer's address (the operand cache below) takes the same path as in the live pass
        if (!q) q = (void*)(uintptr_t)((1ull << 44) + (ar->off - bytes));
        return q;
    }
    float* f32(size_t n_) { return (float*)take(n_ * sizeof(float)); }
};

// a device launch: skipped by the sizing pass, which only walks the allocations
#define TR(expr)                          \
    do {                                  \
        if (s.live()) DIMX_TRY(expr);     \
    } while (0)

int flush_fin(Step& s) {
    if (s.live() && s.fin.n > 0) DIMX_TRY(tr_multi_finish(s.fin, s.st));
    s.fin.n = 0;
    s.fin.total_blocks = 0;
    return DIMX_OK;
}
int queue_fin(Step& s, const float* part, float* out, int C, int nslab) {
    if (s.fin.n == kFinMax) DIMX_TRY(flush_fin(s));
    FinDesc& d = s.fin.d[s.fin.n++];
    d.part = part;
    d.out = out;
    d.C = C;
    d.nslab = nslab;
    d.blk0 = s.fin.total_blocks;
    s.fin.total_blocks += ceil_div(C, 64);
    return DIMX_OK;
}
// dx (+)= LN'(x) dy, d gamma (and d beta) queued; the partial rows come from the step's pool (read at the end of the backward pass).
int ln_adjoint(Step& s, const float* x, const float* gamma, const float* dy, float* dx, int accumulate, int M, int C, float* dg, float* db) {
    int rows = ceil_div(M, kLnBlocks);
    rows = (rows + 3) / 4 * 4;
    const int blocks = ceil_div(M, rows);
    float* pg = s.pool_f32((size_t)blocks * C);
    float* pb = db ? s.pool_f32((size_t)blocks * C) : nullptr;
    int n = blocks;
    if (s.live()) DIMX_TRY(tr_layernorm_bwd_fused(x, gamma, dy, dx, accumulate, M, C, pg, pb, &n, s.st));
    DIMX_TRY(queue_fin(s, pg, dg, C, n));
    if (db) DIMX_TRY(queue_fin(s, pb, db, C, n));
    return DIMX_OK;
}
int bias_adjoint(Step& s, const float* dy, float* out, int M, int C) {
    const int slabs = M < kTrSlabs * 8 ? 1 : kTrSlabs;
    float* part = s.pool_f32((size_t)slabs * C);
    int n = slabs;
    if (s.live()) DIMX_TRY(tr_colsum_partial(dy, M, C, part, &n, s.st));
    return queue_fin(s, part, out, C, n);
}

Lin make_lin(const Step& s, const std::string& wname, const std::string& bname = std::string()) {
    Lin l;
    const PInfo& pi = s.plan->params[s.plan->index.at(wname)];
    l.w = pi.off;
    l.N = pi.rows;
    l.K = pi.cols;
    if (!bname.empty()) l.b = s.off(bname);
    return l;
}

// operand copies of a weight for this step: [N][Kp] and its transpose [K][Np]
int flush_prep(Step& s) {
    if (s.live() && s.prep.n > 0) DIMX_TRY(tr_prep_weights(s.at, s.prep, s.st));
    s.prep.n = 0;
    s.prep.total_tiles = 0;
    return DIMX_OK;
}
// queued: the copies exist after the next flush_prep (every *_prepare group ends with one)
int prep_lin(Step& s, Lin& l) {
    const int Kp = pad_to(l.K, s.bk), Np = pad_to(l.N, s.bk);
    l.w_op = s.take((size_t)l.N * Kp * s.es());
    l.wt_op = s.take((size_t)l.K * Np * s.es());
    if (s.prep.n == kPrepMax) DIMX_TRY(flush_prep(s));
    PrepDesc& d = s.prep.d[s.prep.n++];
    d.src = l.src ? l.src : s.P + l.w;
    d.w = l.w_op;
    d.wt = l.wt_op;
    d.N = l.N;
    d.K = l.K;
    d.Kp = Kp;
    d.Np = Np;
    d.lds = l.K;
    d.gelu = 0;
    d.tile0 = s.prep.total_tiles;
    d.tiles_k = ceil_div(Kp, 32);
    s.prep.total_tiles += ceil_div(Np, 32) * d.tiles_k;
    return DIMX_OK;
}

// C[M,N] f32 = A_op[M,Kp] . W_op[N,Kp]^T (+ bias) (+ residual, which may be C itself)
int gemm_f32(Step& s, const void* A_op, int Kp, const void* W_op, int M, int N, int K, float* C, int ldc, const float* bias,
             const float* residual, int ldr, hipStream_t on = nullptr) {
    if (!s.live()) return DIMX_OK;
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = s.at;
    g.out_dtype = DIMX_F32;
    g.A = A_op;
    g.lda = Kp;
    g.W = W_op;
    g.ldw = Kp;
    g.M = M;
    g.N = N;
    g.K = K;
    g.bias = bias;
    g.residual = residual;
    g.ldr = ldr;
    gemm_set_plain_out(g, C, ldc);
    return launch_gemm(g, on ? on : s.st);
}

// the cached operand pair of a forward input (made on first use; see Step::ops).  mode 1: the operand is erf-GELU(x); mode 2: the
// operand is LayerNorm(ln_src) * ln_gamma and x is only the NAME of that tensor (an arena buffer that is never written: the f32
// pre-norm output is not stored, the backward pass finds the copies through the same name)
int fwd_operands(Step& s, const float* x, int ldx, int M, int K, const Step::OpCopy** out, int mode = 0, const float* ln_src = nullptr,
                 const float* ln_gamma = nullptr, const float* ln_beta = nullptr) {
    const auto key = std::make_tuple(x, ldx, M, K);
    auto it = s.ops.find(key);
    if (it == s.ops.end()) {
        Step::OpCopy c;
        c.Kp = pad_to(K, s.bk);
        c.Mp = pad_to(M, s.bk);
        c.o = s.take((size_t)M * c.Kp * s.es());
        c.t = s.take((size_t)K * c.Mp * s.es());
        TR(tr_prep_fused(s.at, mode, mode == 2 ? ln_src : x, ldx, nullptr, 0, ln_gamma, M, K, c.o, c.Kp, c.t, c.Mp, nullptr, nullptr, s.st, ln_beta));
        it = s.ops.emplace(key, c).first;
    }
    if (out) *out = &it->second;
    return DIMX_OK;
}

// y = x . W^T (+ b) (+ residual)
// (mode 1: the operand is erf-GELU(x) -- applied inside the operand copy, the activation itself is never stored in f32;
//  mode 2: the operand is the pre-norm LayerNorm(ln_src) * ln_gamma, x names it)
int lin_fwd(Step& s, const Lin& l, const float* x, int ldx, int M, float* y, int ldy, const float* residual = nullptr, int ldr = 0,
            int mode = 0, const float* ln_src = nullptr, const float* ln_gamma = nullptr, const float* ln_beta = nullptr) {
    const Step::OpCopy* c;
    DIMX_TRY(fwd_operands(s, x, ldx, M, l.K, &c, mode, ln_src, ln_gamma, ln_beta));
    return gemm_f32(s, c->o, c->Kp, l.w_op, M, l.N, c->Kp, y, ldy, l.b >= 0 ? s.P + l.b : nullptr, residual, ldr);  // K padded with zeros
}

// dx (+)= dy . W ; dW = dy^T . x ; db = colsum(dy).  x [M,K] (ldx), dy [M,N] (ldy) f32.  dx may be null.
// gelu_pre: the gradient that enters is dy * GELU'(gelu_pre) (ff1's adjoint: d pre-activation is formed inside the operand copy)
int lin_bwd(Step& s, const Lin& l, const float* x, int ldx, const float* dy, int ldy, int M, float* dx, int lddx, bool accumulate_dx,
            bool x_from_cache_only = false, const float* gelu_pre = nullptr, int ld_pre = 0, bool gelu_tanh = false) {
    float* const dW = l.gdst ? l.gdst : s.G + l.w;
    float* bias_part = nullptr;   // d bias = column sums of the gradient: partial rows from the operand copy's pass over dy
    if (l.b >= 0) bias_part = s.pool_f32((size_t)ceil_div(M, 32) * l.N);
    const size_t mark = s.ar->off;
    const int Mp = pad_to(M, s.bk), Np = pad_to(l.N, s.bk);
    const auto it = s.ops.find(std::make_tuple(x, ldx, M, l.K));
    const bool side = s.use_side && it != s.ops.end() && !l.gdst;   // a padded weight's gradient is compacted on this stream right after
    const int k = s.slot_n % kSideSlots;
    void* dyo = s.take((size_t)M * Np * s.es());     // dy and dy^T in the operand type: one pass over dy
    void* dyT = side ? s.slot_buf[k] : s.take((size_t)l.N * Mp * s.es());
    if (side && s.live() && s.slot_n >= kSideSlots) DIMX_HIP(hipStreamWaitEvent(s.st, s.ts->ev_side[k], 0));  // the slot's last reader
    int n_part = ceil_div(M, 32);
    TR(tr_prep_fused(s.at, gelu_pre ? (gelu_tanh ? 5 : 3) : 0, dy, ldy, gelu_pre, ld_pre, nullptr, M, l.N, dyo, Np, dyT, Mp, bias_part, &n_part, s.st));
    if (bias_part) DIMX_TRY(queue_fin(s, bias_part, s.G + l.b, l.N, n_part));
    if (side && s.live()) {
        DIMX_HIP(hipEventRecord(s.ts->ev_main[k], s.st));
        DIMX_HIP(hipStreamWaitEvent(s.ts->side, s.ts->ev_main[k], 0));
        DIMX_TRY(gemm_f32(s, dyT, Mp, it->second.t, l.N, l.K, Mp, dW, l.K, nullptr, nullptr, 0, s.ts->side));
        DIMX_HIP(hipEventRecord(s.ts->ev_side[k], s.ts->side));
    }
    if (side) ++s.slot_n;
    if (dx) DIMX_TRY(gemm_f32(s, dyo, Np, l.wt_op, M, l.K, Np, dx, lddx, nullptr, accumulate_dx ? dx : nullptr, lddx));
    if (!side) {
        const void* xT;
        if (it != s.ops.end()) {
            xT = it->second.t;                            // made by the forward pass
        } else {
            DIMX_REQUIRE(!x_from_cache_only, DIMX_ERR_STATE, "train: the forward pass left no operand copy of a transformed input");
            void* t = s.take((size_t)l.K * Mp * s.es());
            TR(tr_transpose_pad(s.at, x, ldx, t, Mp, M, l.K, s.st));
            xT = t;
        }
        TR(gemm_f32(s, dyT, Mp, xT, l.N, l.K, Mp, dW, l.K, nullptr, nullptr, 0));  // contraction over the zero-padded rows
    }
    s.ar->off = mark;
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- sublayers
// a self-attention sublayer over rows that hold several batches of different lengths (the joint encoder of SLM runs [B, 2T] and
// [2B, T] through the same weights): every row-wise operator sees all rows at once, the attention runs once per segment
struct AttnSeg {
    int row0, B, L;
    const uint8_t* kmask;   // [B, L] keep-mask of the segment's keys
};
struct AttnSave {
    std::string pre;      // "...layers.N." prefix
    std::vector<AttnSeg> segs;
    // round 4: to_q / to_k / to_v are consecutive [inner, C] tensors of the flat arenas, so the projections are ONE Linear with
    // 3 inner rows for self-attention (one forward GEMM, one dX GEMM over K = 3 inner, one dW GEMM, one operand copy of the
    // joint gradient) and q + a joint k / v Linear for cross-attention (their inputs differ)
    Lin qkv, q, kv, o;
    const float* h_in;    // residual stream before the sublayer [M, C]
    float *y, *qb, *kb, *vb, *ob, *lse;  // LN output, projections (views of the joint buffers), attention output, row LSE
    int ldq, ldkv;        // row strides of qb and of kb / vb
    const float* src;     // key/value source rows (y for self-attention, the context for cross-attention)
    int M, Mk, C, Ck;     // query rows, key rows, widths
    TrAttn shape;
    const uint8_t* qmask; // zero-fill of padded query rows after to_out (encoders)
    bool cross;
};
struct FFSave {
    std::string pre;
    Lin f1, f2;
    const float* h_in;
    float *y, *pre_act;   // (the activation exists only as the next Linear's operand copies)
    int M, C, F;
};

int attn_prepare(Step& s, AttnSave& a, const std::string& pre, bool cross) {
    a.pre = pre;
    a.cross = cross;
    const Lin q = make_lin(s, pre + "1.to_q.weight"), k = make_lin(s, pre + "1.to_k.weight"), v = make_lin(s, pre + "1.to_v.weight");
    DIMX_REQUIRE(k.w == q.w + (long)q.N * q.K && v.w == k.w + (long)k.N * k.K && q.K == k.K && k.K == v.K, DIMX_ERR_STATE,
                 "train: to_q / to_k / to_v of %s are not consecutive in the arena", pre.c_str());
    a.o = make_lin(s, pre + "1.to_out.weight");
    if (!cross) {
        a.qkv = q;
        a.qkv.N = q.N + k.N + v.N;
        DIMX_TRY(prep_lin(s, a.qkv));
    } else {
        a.q = q;
        a.kv = k;
        a.kv.N = k.N + v.N;
        DIMX_TRY(prep_lin(s, a.q));
        DIMX_TRY(prep_lin(s, a.kv));
    }
    DIMX_TRY(prep_lin(s, a.o));
    return DIMX_OK;
}
int ff_prepare(Step& s, FFSave& f, const std::string& pre) {
    f.pre = pre;
    f.f1 = make_lin(s, pre + "1.ff.0.0.weight", pre + "1.ff.0.0.bias");
    f.f2 = make_lin(s, pre + "1.ff.2.weight", pre + "1.ff.2.bias");
    DIMX_TRY(prep_lin(s, f.f1));
    DIMX_TRY(prep_lin(s, f.f2));
    return DIMX_OK;
}

// h_out = h_in + to_out(attn(LN(h_in) Wq, src Wk, src Wv)); src = LN(h_in) (self) or ctx (cross, Mk rows of width Ck)
int attn_fwd(Step& s, AttnSave& a, const float* h_in, float* h_out, int M, int C, bool cross, const float* ctx, int Mk, int Ck,
             const TrAttn& shape, const uint8_t* qmask) {
    const int inner = a.o.K;
    DIMX_REQUIRE(a.cross == cross, DIMX_ERR_STATE, "train: attention sublayer prepared for the other kind");
    a.h_in = h_in;
    a.M = M;
    a.C = C;
    a.Mk = cross ? Mk : M;
    a.Ck = cross ? Ck : C;
    a.qmask = qmask;
    a.y = s.f32((size_t)M * C);
    if (!cross) {
        a.qb = s.f32((size_t)M * 3 * inner);     // [M][q | k | v]
        a.kb = a.qb + inner;
        a.vb = a.qb + 2 * inner;
        a.ldq = a.ldkv = 3 * inner;
    } else {
        a.qb = s.f32((size_t)M * inner);
        a.kb = s.f32((size_t)a.Mk * 2 * inner);  // [Mk][k | v]
        a.vb = a.kb + inner;
        a.ldq = inner;
        a.ldkv = 2 * inner;
    }
    a.ob = s.f32((size_t)M * inner);
    a.lse = s.f32(a.segs.empty() ? (size_t)shape.B * shape.H * shape.Lq : (size_t)shape.H * M);
    a.src = cross ? ctx : a.y;
    a.shape = shape;
    a.shape.ldq = a.ldq;
    a.shape.ldk = a.shape.ldv = a.ldkv;
    a.shape.ldo = inner;
    // attention and its adjoints on the matrix cores (train_attn.hip): bf16 MFMA in the perf mode, exact-f32 MFMA in the parity
    // mode (the one-wave-per-row f32 VALU kernels both are checked against stay reachable through dimx_op_train_attention)
    a.shape.mfma = s.at == DIMX_BF16 ? 1 : 2;
    // the pre-norm is formed inside the operand copy of its projection (a.y only names it)
    if (!cross) {
        DIMX_TRY(lin_fwd(s, a.qkv, a.y, C, M, a.qb, 3 * inner, nullptr, 0, 2, h_in, s.p(a.pre + "0.0.weight")));
    } else {
        DIMX_TRY(lin_fwd(s, a.q, a.y, C, M, a.qb, inner, nullptr, 0, 2, h_in, s.p(a.pre + "0.0.weight")));
        DIMX_TRY(lin_fwd(s, a.kv, a.src, a.Ck, a.Mk, a.kb, 2 * inner));
    }
    if (a.segs.empty()) {
        TR(tr_attn_fwd(a.shape, a.qb, a.kb, a.vb, a.ob, a.lse, s.st));
    } else {
        size_t lse_off = 0;
        for (const AttnSeg& g : a.segs) {
            TrAttn t = a.shape;
            t.B = g.B; t.Lq = t.Lk = g.L; t.kmask = g.kmask;
            TR(tr_attn_fwd(t, a.qb + (size_t)g.row0 * a.ldq, a.kb + (size_t)g.row0 * a.ldkv, a.vb + (size_t)g.row0 * a.ldkv,
                           a.ob + (size_t)g.row0 * inner, a.lse + lse_off, s.st));
            lse_off += (size_t)g.B * t.H * g.L;
        }
    }
    // encoders: to_out(o) with the padded query rows zero-filled, then the residual.  to_out has no bias, so zero rows of o give
    // zero rows of to_out(o): the attention output's padded rows are zeroed in place and the projection keeps its residual epilogue
    // (before round 4: projection into a temporary, zero_rows, copy, add)
    if (qmask) TR(tr_zero_rows(a.ob, qmask, M, inner, s.st));
    DIMX_TRY(lin_fwd(s, a.o, a.ob, inner, M, h_out, C, h_in, C));
    return DIMX_OK;
}

// dh: gradient wrt h_out on entry, wrt h_in on return (in place); dctx (cross-attention) accumulates the context gradient
int attn_bwd(Step& s, AttnSave& a, float* dh, float* dctx) {
    const size_t mark = s.ar->off;
    const int inner = a.o.K, M = a.M, C = a.C;
    // the padded query rows of o are zero (forward), so dW_out = dh^T . o needs no masked copy of dh; the gradient that reaches
    // the attention through those rows is zeroed after the projection's dX instead
    float* d_o = s.f32((size_t)M * inner);
    DIMX_TRY(lin_bwd(s, a.o, a.ob, inner, dh, C, M, d_o, inner, false));
    if (a.qmask) TR(tr_zero_rows(d_o, a.qmask, M, inner, s.st));
    float *dq, *dk, *dv;     // the same joint layouts as the forward projections
    if (!a.cross) {
        dq = s.f32((size_t)M * 3 * inner);
        dk = dq + inner;
        dv = dq + 2 * inner;
    } else {
        dq = s.f32((size_t)M * inner);
        dk = s.f32((size_t)a.Mk * 2 * inner);
        dv = dk + inner;
    }
    float* delta = s.f32(a.segs.empty() ? (size_t)a.shape.B * a.shape.H * a.shape.Lq : (size_t)a.shape.H * M);
    if (a.segs.empty()) {
        TR(tr_attn_bwd(a.shape, a.qb, a.kb, a.vb, a.ob, d_o, a.lse, delta, dq, a.ldq, dk, a.ldkv, dv, a.ldkv, s.st));
    } else {
        size_t lse_off = 0;
        for (const AttnSeg& g : a.segs) {
            TrAttn t = a.shape;
            t.B = g.B; t.Lq = t.Lk = g.L; t.kmask = g.kmask;
            const size_t rq = (size_t)g.row0 * a.ldq, rk = (size_t)g.row0 * a.ldkv, ro = (size_t)g.row0 * inner;
            TR(tr_attn_bwd(t, a.qb + rq, a.kb + rk, a.vb + rk, a.ob + ro, d_o + ro, a.lse + lse_off, delta + lse_off, dq + rq, a.ldq, dk + rk,
                           a.ldkv, dv + rk, a.ldkv, s.st));
            lse_off += (size_t)g.B * t.H * g.L;
        }
    }
    float* dy = s.f32((size_t)M * C);
    if (!a.cross) {
        DIMX_TRY(lin_bwd(s, a.qkv, a.y, C, dq, 3 * inner, M, dy, C, false));
    } else {
        DIMX_TRY(lin_bwd(s, a.q, a.y, C, dq, inner, M, dy, C, false));
        DIMX_TRY(lin_bwd(s, a.kv, a.src, a.Ck, dk, 2 * inner, a.Mk, dctx, a.Ck, true));
    }
    // LayerNorm: d gamma = colsum(dy o xhat), dh += LN'(h_in) dy
    DIMX_TRY(ln_adjoint(s, a.h_in, s.p(a.pre + "0.0.weight"), dy, dh, 1, M, C, s.g(a.pre + "0.0.weight"), nullptr));
    s.ar->off = mark;
    return DIMX_OK;
}

int ff_fwd(Step& s, FFSave& f, const float* h_in, float* h_out, int M, int C) {
    f.h_in = h_in;
    f.M = M;
    f.C = C;
    f.F = f.f1.N;
    f.y = s.f32((size_t)M * C);
    f.pre_act = s.f32((size_t)M * f.F);
    DIMX_TRY(lin_fwd(s, f.f1, f.y, C, M, f.pre_act, f.F, nullptr, 0, 2, h_in, s.p(f.pre + "0.0.weight")));
    DIMX_TRY(lin_fwd(s, f.f2, f.pre_act, f.F, M, h_out, C, h_in, C, 1));
    return DIMX_OK;
}
int ff_bwd(Step& s, FFSave& f, float* dh) {
    const size_t mark = s.ar->off;
    const int M = f.M, C = f.C, F = f.F;
    float* da = s.f32((size_t)M * F);
    DIMX_TRY(lin_bwd(s, f.f2, f.pre_act, F, dh, C, M, da, F, false, true));   // x^T = gelu(pre_act)^T from the forward pass
    float* dy = s.f32((size_t)M * C);
    DIMX_TRY(lin_bwd(s, f.f1, f.y, C, da, F, M, dy, C, false, false, f.pre_act, F));   // d pre-activation = da * GELU'(pre_act), in the copy
    DIMX_TRY(ln_adjoint(s, f.h_in, s.p(f.pre + "0.0.weight"), dy, dh, 1, M, C, s.g(f.pre + "0.0.weight"), nullptr));
    s.ar->off = mark;
    return DIMX_OK;
}

// final / stand-alone LayerNorm: y = LN(x) gamma (+ beta)
int ln_bwd_full(Step& s, const float* x, const std::string& gname, const std::string& bname, const float* dy, float* dx, int M, int C) {
    return ln_adjoint(s, x, s.p(gname), dy, dx, 0, M, C, s.g(gname), bname.empty() ? nullptr : s.g(bname));
}

// ---------------------------------------------------------------------------------------------------------------- encoder
struct EncSave {
    std::string pre;
    Lin pin;
    const float* x_in;   // [M, Cin]
    int Cin;
    std::vector<AttnSave> attn;
    std::vector<FFSave> ff;
    std::vector<float*> h;  // residual stream after every sublayer (h[0] = after project_in + pos)
    float* out;             // final norm output
    int M;                  // rows
    std::vector<AttnSeg> segs;   // empty: one [s.B, s.T] batch
};

int enc_fwd(Step& s, EncSave& e, const std::string& pre, const float* x_in, int Cin, const uint8_t* mask_rows, const uint8_t* mask_bt,
            int causal = 1, const std::vector<AttnSeg>* segs = nullptr) {
    const dimx_dims& d = s.h->d;
    const int C = d.dim;
    int M = s.M;
    e.segs.clear();
    if (segs) {
        e.segs = *segs;
        M = 0;
        for (const AttnSeg& g : e.segs) {
            DIMX_REQUIRE(g.row0 == M, DIMX_ERR_STATE, "train: encoder segments must tile the rows in order");
            M += g.B * g.L;
        }
    }
    e.M = M;
    e.pre = pre;
    e.x_in = x_in;
    e.Cin = Cin;
    e.pin = make_lin(s, pre + "project_in.weight");
    DIMX_TRY(prep_lin(s, e.pin));
    e.attn.resize(d.enc_depth);
    e.ff.resize(d.enc_depth);
    for (int i = 0; i < d.enc_depth; ++i) {
        DIMX_TRY(attn_prepare(s, e.attn[i], pre + "attn_layers.layers." + std::to_string(2 * i) + ".", false));
        DIMX_TRY(ff_prepare(s, e.ff[i], pre + "attn_layers.layers." + std::to_string(2 * i + 1) + "."));
    }
    DIMX_TRY(flush_prep(s));
    e.h.assign(2 * d.enc_depth + 1, nullptr);
    for (auto& p : e.h) p = s.f32((size_t)M * C);
    e.out = s.f32((size_t)M * C);
    {
        DIMX_TRY(fwd_operands(s, x_in, Cin, M, Cin, nullptr));  // persistent: before the mark
        const size_t mark = s.ar->off;
        float* t = s.f32((size_t)M * C);
        DIMX_TRY(lin_fwd(s, e.pin, x_in, Cin, M, t, C));
        if (e.segs.empty()) {
            TR(tr_add_rows(t, C, nullptr, s.p(pre + "pos_emb.emb.weight"), 1.0f / sqrtf((float)C), s.T, e.h[0], C, M, C, s.st));
        } else {
            for (const AttnSeg& g : e.segs)
                TR(tr_add_rows(t + (size_t)g.row0 * C, C, nullptr, s.p(pre + "pos_emb.emb.weight"), 1.0f / sqrtf((float)C), g.L,
                               e.h[0] + (size_t)g.row0 * C, C, g.B * g.L, C, s.st));
        }
        s.ar->off = mark;
    }
    TrAttn sh;
    memset(&sh, 0, sizeof(sh));
    sh.B = s.B; sh.H = d.heads; sh.Lq = s.T; sh.Lk = s.T;
    sh.scale = 1.0f / sqrtf((float)d.dim_head);
    sh.causal = causal;
    sh.kmask = mask_bt;
    for (int i = 0; i < d.enc_depth; ++i) {
        e.attn[i].segs = e.segs;
        DIMX_TRY(attn_fwd(s, e.attn[i], e.h[2 * i], e.h[2 * i + 1], M, C, false, nullptr, 0, 0, sh, mask_rows));
        DIMX_TRY(ff_fwd(s, e.ff[i], e.h[2 * i + 1], e.h[2 * i + 2], M, C));
    }
    TR(launch_layernorm(DIMX_F32, e.h[2 * d.enc_depth], e.out, s.p(pre + "attn_layers.final_norm.weight"), nullptr, M, C, s.st));
    return DIMX_OK;
}

// d_out: gradient wrt the encoder output [M, C]; dx_in (optional): gradient wrt its input [M, Cin]
int enc_bwd(Step& s, EncSave& e, const float* d_out, float* dx_in) {
    const dimx_dims& d = s.h->d;
    const int M = e.M, C = d.dim;
    const size_t mark = s.ar->off;
    float* dh = s.f32((size_t)M * C);
    DIMX_TRY(ln_bwd_full(s, e.h[2 * d.enc_depth], e.pre + "attn_layers.final_norm.weight", "", d_out, dh, M, C));
    for (int i = d.enc_depth - 1; i >= 0; --i) {
        DIMX_TRY(ff_bwd(s, e.ff[i], dh));
        DIMX_TRY(attn_bwd(s, e.attn[i], dh, nullptr));
    }
    // h0 = project_in(x) + pos[:T] * C^-0.5.  Rows beyond T of the table get no gradient (the caller zeroed G).
    if (e.segs.empty()) {
        TR(tr_pos_grad(dh, s.g(e.pre + "pos_emb.emb.weight"), s.B, s.T, C, 1.0f / sqrtf((float)C), s.st));
    } else {   // the segments share the table (zeroed with the arena at the start of the step): each adds its rows, in stream order
        for (const AttnSeg& g : e.segs) {
            TR(tr_pos_grad(dh + (size_t)g.row0 * C, s.g(e.pre + "pos_emb.emb.weight"), g.B, g.L, C, 1.0f / sqrtf((float)C), s.st, 1));
        }
    }
    DIMX_TRY(lin_bwd(s, e.pin, e.x_in, e.Cin, dh, C, M, dx_in, e.Cin, false));
    s.ar->off = mark;
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- decoder stack
// TransformerWrapper(num_tokens, Decoder(cross_attend = True)) on a token prefix, teacher-forced: token (+ positional) embedding,
// depth x {causal self-attention, cross-attention over the context, feed-forward}, final norm, logits.
struct DecSave {
    std::string pre;
    std::vector<AttnSave> sa, ca;
    std::vector<FFSave> ff;
    std::vector<float*> hd;
    Lin lg;
    float* yf;
    const int32_t* inp;
    int B, n, Md, DD, depth;
    bool pos_emb;
};
int dec_prepare(Step& s, DecSave& D, const std::string& pre, int depth) {
    D.pre = pre;
    D.depth = depth;
    D.sa.resize(depth);
    D.ca.resize(depth);
    D.ff.resize(depth);
    for (int i = 0; i < depth; ++i) {
        DIMX_TRY(attn_prepare(s, D.sa[i], pre + "attn_layers.layers." + std::to_string(3 * i) + ".", false));
        DIMX_TRY(attn_prepare(s, D.ca[i], pre + "attn_layers.layers." + std::to_string(3 * i + 1) + ".", true));
        DIMX_TRY(ff_prepare(s, D.ff[i], pre + "attn_layers.layers." + std::to_string(3 * i + 2) + "."));
    }
    D.lg = make_lin(s, pre + "to_logits.weight");
    DIMX_TRY(prep_lin(s, D.lg));
    return DIMX_OK;
}
// inp [B, n] token ids; ctx [B * Lk, Ck] with key keep-mask ctx_mask [B, Lk]; logits [B * n, num_tokens]
int dec_fwd(Step& s, DecSave& D, const int32_t* inp, int B, int n, const float* ctx, int Lk, int Ck, const uint8_t* ctx_mask,
            const uint8_t* kv_mask, bool pos_emb, float* logits) {
    const dimx_dims& d = s.h->d;
    const int DD = d.dim + d.dim_a, Md = B * n;
    D.B = B; D.n = n; D.Md = Md; D.DD = DD; D.inp = inp; D.pos_emb = pos_emb;
    D.hd.assign(3 * D.depth + 1, nullptr);
    for (auto& p : D.hd) p = s.f32((size_t)Md * DD);
    TR(launch_gather_rows(DIMX_F32, s.p(D.pre + "token_emb.emb.weight"), DD, d.num_tokens, inp, D.hd[0], DD, Md, DD, s.st));
    if (pos_emb)   // AbsolutePositionalEmbedding: + emb[:n] * dim^-0.5
        TR(tr_add_rows(D.hd[0], DD, nullptr, s.p(D.pre + "pos_emb.emb.weight"), 1.0f / sqrtf((float)DD), n, D.hd[0], DD, Md, DD, s.st));
    TrAttn self_sh, cross_sh;
    memset(&self_sh, 0, sizeof(self_sh));
    self_sh.B = B; self_sh.H = d.heads; self_sh.Lq = n; self_sh.Lk = n;
    self_sh.scale = 1.0f / sqrtf((float)d.dim_head);
    self_sh.causal = 1;
    self_sh.kmask2 = kv_mask;
    cross_sh = self_sh;
    cross_sh.Lk = Lk;
    cross_sh.causal = 0;
    cross_sh.kmask = ctx_mask;
    cross_sh.kmask2 = nullptr;
    for (int i = 0; i < D.depth; ++i) {
        DIMX_TRY(attn_fwd(s, D.sa[i], D.hd[3 * i], D.hd[3 * i + 1], Md, DD, false, nullptr, 0, 0, self_sh, nullptr));
        DIMX_TRY(attn_fwd(s, D.ca[i], D.hd[3 * i + 1], D.hd[3 * i + 2], Md, DD, true, ctx, B * Lk, Ck, cross_sh, nullptr));
        DIMX_TRY(ff_fwd(s, D.ff[i], D.hd[3 * i + 2], D.hd[3 * i + 3], Md, DD));
    }
    D.yf = s.f32((size_t)Md * DD);   // names the final norm's output (formed inside the logits projection's operand copy)
    DIMX_TRY(lin_fwd(s, D.lg, D.yf, DD, Md, logits, d.num_tokens, nullptr, 0, 2, D.hd[3 * D.depth], s.p(D.pre + "attn_layers.final_norm.weight")));
    return DIMX_OK;
}
// dlogits -> every decoder gradient; dctx [B * Lk, Ck] accumulates the context gradient (zeroed by the caller)
int dec_bwd(Step& s, DecSave& D, const float* dlogits, float* dctx) {
    const dimx_dims& d = s.h->d;
    const int DD = D.DD, Md = D.Md;
    float* dyf = s.f32((size_t)Md * DD);
    float* dh = s.f32((size_t)Md * DD);
    DIMX_TRY(lin_bwd(s, D.lg, D.yf, DD, dlogits, d.num_tokens, Md, dyf, DD, false));
    DIMX_TRY(ln_bwd_full(s, D.hd[3 * D.depth], D.pre + "attn_layers.final_norm.weight", "", dyf, dh, Md, DD));
    for (int i = D.depth - 1; i >= 0; --i) {
        DIMX_TRY(ff_bwd(s, D.ff[i], dh));
        DIMX_TRY(attn_bwd(s, D.ca[i], dh, dctx));
        DIMX_TRY(attn_bwd(s, D.sa[i], dh, nullptr));
    }
    if (D.pos_emb) TR(tr_pos_grad(dh, s.g(D.pre + "pos_emb.emb.weight"), D.B, D.n, DD, 1.0f / sqrtf((float)DD), s.st));
    {   // d token_emb = onehot(inp)^T . dh on the library GEMM
        const size_t mark = s.ar->off;
        const int Mp = pad_to(Md, s.bk);
        void* ohT = s.take((size_t)d.num_tokens * Mp * s.es());
        void* dhT = s.take((size_t)DD * Mp * s.es());
        TR(tr_onehot_t(s.at, D.inp, ohT, Mp, Md, d.num_tokens, s.st));
        TR(tr_transpose_pad(s.at, dh, DD, dhT, Mp, Md, DD, s.st));
        TR(gemm_f32(s, ohT, Mp, dhT, d.num_tokens, DD, Mp, s.g(D.pre + "token_emb.emb.weight"), DD, nullptr, nullptr, 0));
        s.ar->off = mark;
    }
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- VQ-VAE decoder
// TransformerDecoder of the listener VQ-VAE (code/models/stage1_BIWI.py:376-393), trainable in the legacy loop: linear, Conv1d(k 5,
// replicate) as im2col + GEMM, LeakyReLU(0.2) + InstanceNorm over time, linear, + pe[clip], layers x {pre-LN attention with a
// packed qkv projection and scale hidden^-0.5, pre-LN tanh-GELU MLP}, bias-free output map.  The 8 heads of 48 run on the
// 64-wide attention kernels as zero-padded heads: the qkv / out weights are padded into scratch copies per step (zero rows /
// columns), every padded activation column is then zero by construction, and the weight gradients are compacted back.
struct VqLayerSave {
    std::string a, m;   // "...net.2i.fn." / "...net.2i+1.fn."
    Lin qkv, out, l1, l2;
    float *h_in, *h_mid;            // residual stream before the attention / before the MLP
    float *ya, *ym;                 // names of the two pre-norm outputs
    float *qkvb, *ob, *lse, *pre_act;
    float *wq_pad, *wo_pad, *gq_pad, *go_pad;
    TrAttn shape;
};
// Dropout(p) after a positional encoding (train mode): the keep mask is regenerated from (seed, step, site), train_vq.hip
struct VqDrop {
    float p = 0.f;
    uint64_t seed = 0;
    long step = 0;
    int site = 0;
};
// the pre-LN blocks of a VQ-VAE Transformer (encoder_transformer / decoder_transformer; code/models/lib/base_models.py):
// weight operand copies queued (the caller flushes), head-padded qkv / out scratch made
int vq_blocks_prepare(Step& s, std::vector<VqLayerSave>& L, const std::string& net) {
    const dimx_dims& d = s.h->d;
    const int H = d.vq_hidden, G = d.vq_heads;
    L.resize(d.vq_layers);
    for (int i = 0; i < d.vq_layers; ++i) {
        VqLayerSave& l = L[i];
        l.a = net + std::to_string(2 * i) + ".fn.";
        l.m = net + std::to_string(2 * i + 1) + ".fn.";
        l.qkv = make_lin(s, l.a + "fn.to_qkv.weight");
        l.out = make_lin(s, l.a + "fn.to_out.weight", l.a + "fn.to_out.bias");
        l.l1 = make_lin(s, l.m + "fn.l1.weight", l.m + "fn.l1.bias");
        l.l2 = make_lin(s, l.m + "fn.l2.weight", l.m + "fn.l2.bias");
        l.wq_pad = s.f32((size_t)3 * G * 64 * H);
        l.wo_pad = s.f32((size_t)H * G * 64);
        TR(tr_pad_head_rows(s.P + l.qkv.w, l.wq_pad, 3 * G, H, 0, s.st));
        TR(tr_pad_head_cols(s.P + l.out.w, l.wo_pad, H, G, 0, s.st));
        l.qkv.src = l.wq_pad;
        l.qkv.N = 3 * G * 64;
        l.out.src = l.wo_pad;
        l.out.K = G * 64;
        DIMX_TRY(prep_lin(s, l.qkv));
        DIMX_TRY(prep_lin(s, l.out));
        DIMX_TRY(prep_lin(s, l.l1));
        DIMX_TRY(prep_lin(s, l.l2));
    }
    return DIMX_OK;
}
// h [B * n, H] -> *h_out (a new buffer); the activations the backward pass needs stay in L
int vq_blocks_fwd(Step& s, std::vector<VqLayerSave>& L, float* h, int B, int n, float** h_out) {
    const dimx_dims& d = s.h->d;
    const int H = d.vq_hidden, I = d.vq_inter, M = B * n, G = d.vq_heads;
    for (size_t i = 0; i < L.size(); ++i) {
        VqLayerSave& l = L[i];
        l.h_in = h;
        l.ya = s.f32((size_t)M * H);
        l.qkvb = s.f32((size_t)M * 3 * G * 64);
        l.ob = s.f32((size_t)M * G * 64);
        l.lse = s.f32((size_t)B * G * n);
        DIMX_TRY(lin_fwd(s, l.qkv, l.ya, H, M, l.qkvb, 3 * G * 64, nullptr, 0, 2, h, s.p(l.a + "norm.weight"), s.p(l.a + "norm.bias")));
        memset(&l.shape, 0, sizeof(l.shape));
        l.shape.B = B; l.shape.H = G; l.shape.Lq = n; l.shape.Lk = n;
        l.shape.ldq = l.shape.ldk = l.shape.ldv = 3 * G * 64;
        l.shape.ldo = G * 64;
        l.shape.scale = 1.0f / sqrtf((float)H);   // hidden^-0.5, not head^-0.5 (code/models/lib/base_models.py:131)
        l.shape.mfma = s.at == DIMX_BF16 ? 1 : 2;
        TR(tr_attn_fwd(l.shape, l.qkvb, l.qkvb + G * 64, l.qkvb + 2 * G * 64, l.ob, l.lse, s.st));
        l.h_mid = s.f32((size_t)M * H);
        DIMX_TRY(lin_fwd(s, l.out, l.ob, G * 64, M, l.h_mid, H, h, H));
        l.ym = s.f32((size_t)M * H);
        l.pre_act = s.f32((size_t)M * I);
        DIMX_TRY(lin_fwd(s, l.l1, l.ym, H, M, l.pre_act, I, nullptr, 0, 2, l.h_mid, s.p(l.m + "norm.weight"), s.p(l.m + "norm.bias")));
        float* h2 = s.f32((size_t)M * H);
        DIMX_TRY(lin_fwd(s, l.l2, l.pre_act, I, M, h2, H, l.h_mid, H, 4));
        h = h2;
    }
    *h_out = h;
    return DIMX_OK;
}
// dh [B * n, H]: gradient wrt the blocks' output on entry, wrt their input on return (in place)
int vq_blocks_bwd(Step& s, std::vector<VqLayerSave>& L, float* dh, int B, int n) {
    const dimx_dims& d = s.h->d;
    const int H = d.vq_hidden, I = d.vq_inter, M = B * n, G = d.vq_heads;
    for (int i = (int)L.size() - 1; i >= 0; --i) {
        VqLayerSave& l = L[i];
        const size_t mark = s.ar->off;
        float* da = s.f32((size_t)M * I);
        DIMX_TRY(lin_bwd(s, l.l2, l.pre_act, I, dh, H, M, da, I, false, true));
        float* dy = s.f32((size_t)M * H);
        DIMX_TRY(lin_bwd(s, l.l1, l.ym, H, da, I, M, dy, H, false, false, l.pre_act, I, true));
        DIMX_TRY(ln_adjoint(s, l.h_mid, s.p(l.m + "norm.weight"), dy, dh, 1, M, H, s.g(l.m + "norm.weight"), s.g(l.m + "norm.bias")));
        // attention sublayer
        l.go_pad = s.f32((size_t)H * G * 64);
        l.out.gdst = l.go_pad;
        float* d_o = s.f32((size_t)M * G * 64);
        DIMX_TRY(lin_bwd(s, l.out, l.ob, G * 64, dh, H, M, d_o, G * 64, false));
        TR(tr_pad_head_cols(l.go_pad, s.G + l.out.w, H, G, 1, s.st));
        float* dqkv = s.f32((size_t)M * 3 * G * 64);
        float* delta = s.f32((size_t)B * G * n);
        TR(tr_attn_bwd(l.shape, l.qkvb, l.qkvb + G * 64, l.qkvb + 2 * G * 64, l.ob, d_o, l.lse, delta, dqkv, 3 * G * 64, dqkv + G * 64, 3 * G * 64,
                       dqkv + 2 * G * 64, 3 * G * 64, s.st));
        l.gq_pad = s.f32((size_t)3 * G * 64 * H);
        l.qkv.gdst = l.gq_pad;
        DIMX_TRY(lin_bwd(s, l.qkv, l.ya, H, dqkv, 3 * G * 64, M, dy, H, false));
        TR(tr_pad_head_rows(l.gq_pad, s.G + l.qkv.w, 3 * G, H, 1, s.st));
        DIMX_TRY(ln_adjoint(s, l.h_in, s.p(l.a + "norm.weight"), dy, dh, 1, M, H, s.g(l.a + "norm.weight"), s.g(l.a + "norm.bias")));
        s.ar->off = mark;
    }
    return DIMX_OK;
}

struct VqDecSave {
    std::string c;
    Lin pre, conv, emb, rev;
    std::vector<VqLayerSave> L;
    const float* zq;
    float *h0, *x5, *xc, *yn, *h_out;
    int B, n, M, H, I;
    const VqDrop* drop;
};
// The decoder's input is the codebook gather of idx (legacy / SLM steps: arg-max codes, no gradient) or, when zq_in is given,
// that latent [B * n, 128] itself (the VQ-VAE's own step: the straight-through latent, whose gradient vqdec_bwd returns).
// drop: the PositionalEncoding's dropout (the VQ-VAE's own step in train mode); nullptr = none.
int vqdec_fwd(Step& s, VqDecSave& V, const std::string& c, const int32_t* idx, const float* codebook, const float* pe, int B, int n, float* pred,
              const float* zq_in = nullptr, const VqDrop* drop = nullptr) {
    const dimx_dims& d = s.h->d;
    const int H = d.vq_hidden, I = d.vq_inter, M = B * n, G = d.vq_heads;
    DIMX_REQUIRE(H == 8 * 48 && G == 8 && d.vq_zdim == 128, DIMX_ERR_ARG, "train: the VQ decoder step is written for 8 heads of 48, 128-wide codes");
    V.c = c; V.B = B; V.n = n; V.M = M; V.H = H; V.I = I; V.drop = drop;
    V.pre = make_lin(s, c + "decoder_linear_embedding_pre.net.weight", c + "decoder_linear_embedding_pre.net.bias");
    V.conv = make_lin(s, c + "expander.0.0.weight", c + "expander.0.0.bias");
    V.emb = make_lin(s, c + "decoder_linear_embedding.net.weight", c + "decoder_linear_embedding.net.bias");
    V.rev = make_lin(s, c + "vertice_map_reverse.weight");
    DIMX_TRY(prep_lin(s, V.pre));
    DIMX_TRY(prep_lin(s, V.conv));
    DIMX_TRY(prep_lin(s, V.emb));
    DIMX_TRY(prep_lin(s, V.rev));
    DIMX_TRY(vq_blocks_prepare(s, V.L, c + "decoder_transformer.net."));
    DIMX_TRY(flush_prep(s));
    float* zq = zq_in ? nullptr : s.f32((size_t)M * 128);
    V.h0 = s.f32((size_t)M * H);
    V.x5 = s.f32((size_t)M * 5 * H);
    V.xc = s.f32((size_t)M * H);
    V.yn = s.f32((size_t)M * H);
    float* h = s.f32((size_t)M * H);
    if (!zq_in) TR(tr_gather128(codebook, idx, zq, M, s.st));
    V.zq = zq_in ? zq_in : zq;
    DIMX_TRY(lin_fwd(s, V.pre, V.zq, 128, M, V.h0, H));
    TR(tr_im2col5(V.h0, V.x5, B, n, H, s.st));
    DIMX_TRY(lin_fwd(s, V.conv, V.x5, 5 * H, M, V.xc, H));
    TR(tr_lrelu_inorm_fwd(V.xc, V.yn, B, n, H, s.st));
    DIMX_TRY(lin_fwd(s, V.emb, V.yn, H, M, h, H));
    if (drop)
        TR(tr_pe_dropout_fwd(h, pe, h, M, n, H, drop->p, drop->seed, drop->step, drop->site, s.st));
    else
        TR(tr_add_clip_rows(h, pe, h, M, n, H, s.st));
    DIMX_TRY(vq_blocks_fwd(s, V.L, h, B, n, &V.h_out));
    DIMX_TRY(lin_fwd(s, V.rev, V.h_out, H, M, pred, d.vq_in_dim));
    return DIMX_OK;
}
// dzq (optional, [B * n, 128]): the gradient wrt the decoder's input latent
int vqdec_bwd(Step& s, VqDecSave& V, const float* dpred, float* dzq = nullptr) {
    const dimx_dims& d = s.h->d;
    const int H = V.H, M = V.M, B = V.B, n = V.n;
    float* dh = s.f32((size_t)M * H);
    DIMX_TRY(lin_bwd(s, V.rev, V.h_out, H, dpred, d.vq_in_dim, M, dh, H, false));
    DIMX_TRY(vq_blocks_bwd(s, V.L, dh, B, n));
    // (+ pe: a buffer, no gradient; dropout: the same mask) -> linear -> InstanceNorm / LeakyReLU -> conv -> linear
    if (V.drop) TR(tr_dropout_bwd(dh, M, n, H, V.drop->p, V.drop->seed, V.drop->step, V.drop->site, s.st));
    float* d_yn = s.f32((size_t)M * H);
    DIMX_TRY(lin_bwd(s, V.emb, V.yn, H, dh, H, M, d_yn, H, false));
    float* d_xc = s.f32((size_t)M * H);
    TR(tr_lrelu_inorm_bwd(V.xc, d_yn, d_xc, B, n, H, s.st));
    float* d_x5 = s.f32((size_t)M * 5 * H);
    DIMX_TRY(lin_bwd(s, V.conv, V.x5, 5 * H, d_xc, H, M, d_x5, 5 * H, false));
    float* d_h0 = s.f32((size_t)M * H);
    TR(tr_col2im5(d_x5, d_h0, B, n, H, s.st));
    // the legacy / SLM steps' codes carry no gradient (arg-max): dzq == nullptr there
    DIMX_TRY(lin_bwd(s, V.pre, V.zq, 128, d_h0, H, M, dzq, 128, false));
    return DIMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- VQ-VAE encoder
// TransformerEncoder (code/models/stage1_BIWI.py:254-317, quant_factor 0): vertice_mapping = Linear + LeakyReLU(0.2) (in place),
// squasher = Conv1d(k 5, replicate) + LeakyReLU + InstanceNorm (no affine), encoder_linear_embedding, + pe[clip] (then the
// PositionalEncoding's Dropout), the pre-LN blocks (shared with the decoder), encoder_linear_embedding_post -> z [B * n, 128].
struct VqEncSave {
    Lin vm, conv, le, post;
    std::vector<VqLayerSave> L;
    const float* x;
    float *h1, *x5, *xc, *yn, *h_out;
    int B, n, M, H;
    VqDrop drop;
};
int vqenc_fwd(Step& s, VqEncSave& E, const std::string& c, const float* x, const float* pe, const VqDrop& drop, int B, int n, float* z) {
    const dimx_dims& d = s.h->d;
    const int H = d.vq_hidden, M = B * n;
    E.B = B; E.n = n; E.M = M; E.H = H; E.x = x; E.drop = drop;
    E.vm = make_lin(s, c + "vertice_mapping.0.weight", c + "vertice_mapping.0.bias");
    E.conv = make_lin(s, c + "squasher.0.0.weight", c + "squasher.0.0.bias");
    E.le = make_lin(s, c + "encoder_linear_embedding.net.weight", c + "encoder_linear_embedding.net.bias");
    E.post = make_lin(s, c + "encoder_linear_embedding_post.net.weight", c + "encoder_linear_embedding_post.net.bias");
    DIMX_TRY(prep_lin(s, E.vm));
    DIMX_TRY(prep_lin(s, E.conv));
    DIMX_TRY(prep_lin(s, E.le));
    DIMX_TRY(prep_lin(s, E.post));
    DIMX_TRY(vq_blocks_prepare(s, E.L, c + "encoder_transformer.net."));
    DIMX_TRY(flush_prep(s));
    E.h1 = s.f32((size_t)M * H);
    E.x5 = s.f32((size_t)M * 5 * H);
    E.xc = s.f32((size_t)M * H);
    E.yn = s.f32((size_t)M * H);
    float* h = s.f32((size_t)M * H);
    DIMX_TRY(lin_fwd(s, E.vm, x, d.vq_in_dim, M, E.h1, H));
    TR(tr_lrelu(E.h1, (long)M * H, 0.2f, s.st));
    TR(tr_im2col5(E.h1, E.x5, B, n, H, s.st));
    DIMX_TRY(lin_fwd(s, E.conv, E.x5, 5 * H, M, E.xc, H));
    TR(tr_lrelu_inorm_fwd(E.xc, E.yn, B, n, H, s.st));
    DIMX_TRY(lin_fwd(s, E.le, E.yn, H, M, h, H));
    TR(tr_pe_dropout_fwd(h, pe, h, M, n, H, drop.p, drop.seed, drop.step, drop.site, s.st));
    DIMX_TRY(vq_blocks_fwd(s, E.L, h, B, n, &E.h_out));
    DIMX_TRY(lin_fwd(s, E.post, E.h_out, H, M, z, d.vq_zdim));
    return DIMX_OK;
}
// dz [B * n, 128] -> every encoder gradient (the input motion needs none)
int vqenc_bwd(Step& s, VqEncSave& E, const float* dz) {
    const dimx_dims& d = s.h->d;
    const int H = E.H, M = E.M, B = E.B, n = E.n;
    float* dh = s.f32((size_t)M * H);
    DIMX_TRY(lin_bwd(s, E.post, E.h_out, H, dz, d.vq_zdim, M, dh, H, false));
    DIMX_TRY(vq_blocks_bwd(s, E.L, dh, B, n));
    TR(tr_dropout_bwd(dh, M, n, H, E.drop.p, E.drop.seed, E.drop.step, E.drop.site, s.st));
    float* d_yn = s.f32((size_t)M * H);
    DIMX_TRY(lin_bwd(s, E.le, E.yn, H, dh, H, M, d_yn, H, false));
    float* d_xc = s.f32((size_t)M * H);
    TR(tr_lrelu_inorm_bwd(E.xc, d_yn, d_xc, B, n, H, s.st));
    float* d_x5 = s.f32((size_t)M * 5 * H);
    DIMX_TRY(lin_bwd(s, E.conv, E.x5, 5 * H, d_xc, H, M, d_x5, 5 * H, false));
    float* d_h1 = s.f32((size_t)M * H);
    TR(tr_col2im5(d_x5, d_h1, B, n, H, s.st));
    TR(tr_lrelu_bwd_out(E.h1, d_h1, (long)M * H, 0.2f, s.st));
    DIMX_TRY(lin_bwd(s, E.vm, E.x, d.vq_in_dim, d_h1, H, M, nullptr, 0, false));
    return DIMX_OK;
}


// ---------------------------------------------------------------------------------------------------------------- converter head
struct LstmLayerP {
    Lin ih[2], hh[2];   // [direction]; the bias of ih is bias_ih, the bias of hh is bias_hh (their gradients are equal)
    int In = 0;
};
LstmLayerP make_lstm_layer(const Step& s, int layer) {
    LstmLayerP L;
    const std::string l = "vertice_map_reverse_lstm.";
    for (int dir = 0; dir < 2; ++dir) {
        const std::string sfx = "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
        L.ih[dir] = make_lin(s, l + "weight_ih" + sfx, l + "bias_ih" + sfx);
        L.hh[dir] = make_lin(s, l + "weight_hh" + sfx, l + "bias_hh" + sfx);
    }
    L.In = L.ih[0].K;
    return L;
}
// the training forward of one layer: lstm.hip's own call (same kernels, same y) with the save switch
int lstm_layer_fwd(Step& s, const LstmLayerP& L, const float* x, float* y, float* save, void* scr, size_t scr_bytes, int flags, int cu,
                   int* faults) {
    if (!s.live()) return DIMX_OK;
    const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2];
    for (int d = 0; d < 2; ++d) {
        w_ih[d] = s.P + L.ih[d].w;
        w_hh[d] = s.P + L.hh[d].w;
        b_ih[d] = s.P + L.ih[d].b;
        b_hh[d] = s.P + L.hh[d].b;
    }
    return lstm_layer_run(x, s.B, s.T, L.In, 384, w_ih, w_hh, b_ih, b_hh, y, scr, scr_bytes, flags, cu, faults, s.st, save);
}
// its adjoint: the recurrence leaves dG [M][2][4H]; per direction dW_ih = dG^T x, dW_hh = dG^T h_prev, d bias = colsum(dG),
// dx (+)= dG W_ih on the library's GEMM.  dx may be null (the first layer's input carries no gradient).
int lstm_layer_bwd(Step& s, const LstmLayerP& L, const float* x, const float* y, const float* save, const float* dy, float* dx, void* scr,
                   size_t scr_bytes, int flags, int cu, int* faults) {
    const int M = s.M, G4 = 1536;
    float* dG = s.f32((size_t)M * 2 * G4);
    float* hp = s.f32((size_t)M * 768);
    if (s.live()) {
        const float* w_hh[2] = {s.P + L.hh[0].w, s.P + L.hh[1].w};
        DIMX_TRY(lstm_bwd_run(dy, save, w_hh, s.B, s.T, dG, scr, scr_bytes, flags, cu, faults, s.st));
        DIMX_TRY(tr_lstm_hprev(y, hp, s.B, s.T, s.st));
    }
    for (int d = 0; d < 2; ++d) {
        DIMX_TRY(lin_bwd(s, L.ih[d], x, L.In, dG + d * G4, 2 * G4, M, dx, L.In, d == 1));
        DIMX_TRY(lin_bwd(s, L.hh[d], hp + d * 384, 768, dG + d * G4, 2 * G4, M, nullptr, 0, false));
    }
    return DIMX_OK;
}
size_t lstm_train_scratch_bytes(int B, int T, int In) {
    return std::max(std::max(lstm_scratch_bytes(B, T, In), lstm_scratch_bytes(B, T, 768)), lstm_bwd_scratch_bytes(B, T));
}
// ---------------------------------------------------------------------------------------------------------------- step scaffold
// The end of every step: the queued column reductions, the join of the side stream (in order: its last event covers every weight
// gradient), the arena's high-water mark for the sizing pass, and the two overflow checks.
int step_finish(Step& s, const char* tag, size_t* need) {
    DIMX_TRY(flush_fin(s));   // every queued column reduction: one launch
    if (s.use_side && s.live() && s.slot_n > 0) {
        DIMX_HIP(hipEventRecord(s.ts->ev_join, s.ts->side));
        DIMX_HIP(hipStreamWaitEvent(s.st, s.ts->ev_join, 0));
    }
    if (need) *need = s.peak + 256;
    DIMX_REQUIRE(!s.pool_overflow, DIMX_ERR_STATE, "%s: the partial-row pool of the column reductions is too small", tag);
    DIMX_REQUIRE(!s.ar->overflow, DIMX_ERR_WORKSPACE, "%s: workspace %zu < required %zu", tag, s.ar->cap, s.peak);
    return DIMX_OK;
}
// The arena is planned while kernels are being launched, so every entry point first walks its step without a workspace -- a pure
// host walk of the same allocation sequence with the same arguments, nothing launched -- and checks the caller's workspace against
// it: an undersized workspace used to be reported only after kernels had written past its end.
// run(ws, ws_bytes, stream, need) is the step with every other argument bound.
template <class Run>
int check_workspace(const char* tag, size_t ws_bytes, Run run) {
    size_t need = 0;
    DIMX_TRY(run(nullptr, 0, nullptr, &need));
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "%s: workspace %zu < required %zu (dimx_%s_workspace_bytes)", tag, ws_bytes, need, tag);
    return DIMX_OK;
}
// dimx_*_workspace_bytes has no arguments to walk with: an optional input or output it sizes for stands in as this never
// dereferenced address (the steps only ask whether it is there)
template <class T> T* present() { return (T*)0x100; }
}  // namespace

void train_forget(dimx_handle h) {
    std::lock_guard<std::mutex> lock(g_plans_mu);
    train_map().erase(h);
}

}  // namespace dimx

using namespace dimx;

extern "C" {

int dimx_train_num_params(dimx_handle h) { return layout_num_params(h, kPlanMain); }
int64_t dimx_train_total(dimx_handle h) { return layout_total(h, kPlanMain); }
int dimx_train_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel) {
    return layout_param_info(h, kPlanMain, i, name, offset, numel);
}

static int train_run(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_audio, const uint8_t* mask,
                     const int32_t* z_l, const uint8_t* kv_mask, int B, int T, float* loss_out, float* logits_out, void* ws,
                     size_t ws_bytes, hipStream_t st, size_t* need, bool use_side) {
    TrainState* ts;
    DIMX_TRY(state_of(h, &ts));
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "train: only the SLMFT variant is trained");
    DIMX_REQUIRE(B >= 1 && T >= 2 && T <= d.max_seq_len, DIMX_ERR_ARG, "train: B=%d T=%d out of range", B, T);
    Arena ar(ws, ws_bytes);
    Step s(h, ts->plan, params, grads, &ar, st, h->at, B, T, T - 1);
    const int DD = d.dim + d.dim_a, F = DD * d.ff_mult, inner = d.heads * d.dim_head;
    s.reserve_part(F);
    if (use_side) DIMX_TRY(s.use_side_stream(*ts, std::max(F, 3 * inner), s.M));   // the widest dy^T of the step: ff1's [F][rows]
    {   // partial rows of the deferred column reductions: LayerNorm adjoints (<= kLnBlocks + 3 rows of <= DD each, two for norm_s) and
        // bias / patch-embedding gradients (<= kTrSlabs rows of <= F)
        const size_t n_ln = (size_t)(4 * d.enc_depth + 3 * d.dec_depth + 12), n_b = (size_t)(4 * d.enc_depth + 2 * d.dec_depth + 4);
        s.alloc_pool(n_ln * (kLnBlocks + 4) * (size_t)DD + n_b * (size_t)std::max(kTrSlabs, ceil_div(s.M, 32) + 1) * (size_t)F + 4096);
    }
    const bool live = ws != nullptr;
    DIMX_TRY(s.zero_grads());

    // ---------------- encoders: x0 = v_speaker + patch_embed_s -> encoder_s -> encoder_joint -> norm_s
    float* x0 = s.f32((size_t)s.M * d.dim_in);
    TR(tr_add_rows(v_speaker, d.dim_in, s.p("patch_embed_s"), nullptr, 0.f, T, x0, d.dim_in, s.M, d.dim_in, st));
    EncSave es, ej;
    DIMX_TRY(enc_fwd(s, es, "encoder_s.", x0, d.dim_in, mask, mask));
    DIMX_TRY(enc_fwd(s, ej, "encoder_joint.", es.out, d.dim, mask, mask));
    float* x_s = s.f32((size_t)s.M * d.dim);
    TR(launch_layernorm(DIMX_F32, ej.out, x_s, s.p("norm_s.weight"), s.p("norm_s.bias"), s.M, d.dim, st));
    // context = cat(x_s + patch_embed_dec_s, audio)
    float* ctx = s.f32((size_t)s.M * DD);
    TR(tr_add_rows(x_s, d.dim, s.p("patch_embed_dec_s"), nullptr, 0.f, T, ctx, DD, s.M, d.dim, st));
    TR(tr_copy_cols(v_audio, d.dim_a, ctx + d.dim, DD, s.M, d.dim_a, 0, st));
    // condition dropout (dimx_set_train_cond_keep): a dropped clip is trained under the null context -- zero rows after the concat,
    // before the cross K / V projections read them -- and sends nothing back into its context (below)
    const uint8_t* cond_keep = h->tcond_keep;
    if (cond_keep) TR(tr_zero_clip_rows(ctx, cond_keep, B, T, DD, st));

    // ---------------- decoder, teacher-forced: inp = z[:, :-1] (ignored -> 0), target = z[:, 1:]
    const std::string dn = "decoder_joint.net.";
    int32_t* inp = (int32_t*)s.take((size_t)s.Md * 4);
    int32_t* tgt = (int32_t*)s.take((size_t)s.Md * 4);
    TR(launch_shift_tokens(z_l, inp, tgt, B, T, st));
    std::vector<AttnSave> sa(d.dec_depth), ca(d.dec_depth);
    std::vector<FFSave> ff(d.dec_depth);
    for (int i = 0; i < d.dec_depth; ++i) {
        DIMX_TRY(attn_prepare(s, sa[i], dn + "attn_layers.layers." + std::to_string(3 * i) + ".", false));
        DIMX_TRY(attn_prepare(s, ca[i], dn + "attn_layers.layers." + std::to_string(3 * i + 1) + ".", true));
        DIMX_TRY(ff_prepare(s, ff[i], dn + "attn_layers.layers." + std::to_string(3 * i + 2) + "."));
    }
    Lin lg = make_lin(s, dn + "to_logits.weight");
    DIMX_TRY(prep_lin(s, lg));
    DIMX_TRY(flush_prep(s));
    std::vector<float*> hd(3 * d.dec_depth + 1);
    for (auto& p : hd) p = s.f32((size_t)s.Md * DD);
    TR(launch_gather_rows(DIMX_F32, s.p(dn + "token_emb.emb.weight"), DD, d.num_tokens, inp, hd[0], DD, s.Md, DD, st));
    TrAttn self_sh, cross_sh;
    memset(&self_sh, 0, sizeof(self_sh));
    self_sh.B = B; self_sh.H = d.heads; self_sh.Lq = s.n; self_sh.Lk = s.n;
    self_sh.scale = 1.0f / sqrtf((float)d.dim_head);
    self_sh.causal = 1;
    self_sh.kmask2 = kv_mask;
    cross_sh = self_sh;
    cross_sh.Lk = T;
    cross_sh.causal = 0;
    cross_sh.kmask = mask;
    cross_sh.kmask2 = nullptr;
    // online fine-tuning (dimx_set_train_lookahead): decoder row i is generation step t = i and sees the context rows
    // j < clamp(i + 2 + L, 1, T); the adjoints read the same shape back from the AttnSave
    tr_attn_window(cross_sh, h->twin_on, h->twin_lookahead);
    for (int i = 0; i < d.dec_depth; ++i) {
        DIMX_TRY(attn_fwd(s, sa[i], hd[3 * i], hd[3 * i + 1], s.Md, DD, false, nullptr, 0, 0, self_sh, nullptr));
        DIMX_TRY(attn_fwd(s, ca[i], hd[3 * i + 1], hd[3 * i + 2], s.Md, DD, true, ctx, s.M, DD, cross_sh, nullptr));
        DIMX_TRY(ff_fwd(s, ff[i], hd[3 * i + 2], hd[3 * i + 3], s.Md, DD));
    }
    float* yf = s.f32((size_t)s.Md * DD);
    float* logits = logits_out ? logits_out : s.f32((size_t)s.Md * d.num_tokens);
    float* dlogits = s.f32((size_t)s.Md * d.num_tokens);
    float* row_loss = s.f32((size_t)s.Md);
    DIMX_REQUIRE(d.num_tokens == 512, DIMX_ERR_ARG, "train: the cross-entropy kernel is written for 512 codes");
    TR(launch_layernorm(DIMX_F32, hd[3 * d.dec_depth], yf, s.p(dn + "attn_layers.final_norm.weight"), nullptr, s.Md, DD, st));
    DIMX_TRY(lin_fwd(s, lg, yf, DD, s.Md, logits, d.num_tokens));
    TR(tr_cross_entropy(logits, tgt, row_loss, dlogits, s.Md, loss_out, st));

    // ---------------- backward
    float* dyf = s.f32((size_t)s.Md * DD);
    float* dh = s.f32((size_t)s.Md * DD);
    float* dctx = s.f32((size_t)s.M * DD);
    float* dx_s = s.f32((size_t)s.M * d.dim);
    float* d_ej = s.f32((size_t)s.M * d.dim);
    float* d_es = s.f32((size_t)s.M * d.dim);
    float* d_x0 = s.f32((size_t)s.M * d.dim_in);
    if (live) DIMX_HIP(hipMemsetAsync(dctx, 0, (size_t)s.M * DD * sizeof(float), st));
    DIMX_TRY(lin_bwd(s, lg, yf, DD, dlogits, d.num_tokens, s.Md, dyf, DD, false));
    DIMX_TRY(ln_bwd_full(s, hd[3 * d.dec_depth], dn + "attn_layers.final_norm.weight", "", dyf, dh, s.Md, DD));
    for (int i = d.dec_depth - 1; i >= 0; --i) {
        DIMX_TRY(ff_bwd(s, ff[i], dh));
        DIMX_TRY(attn_bwd(s, ca[i], dh, dctx));
        DIMX_TRY(attn_bwd(s, sa[i], dh, nullptr));
    }
    {   // d token_emb = onehot(inp)^T . dh on the library GEMM
        const size_t mark = s.ar->off;
        const int Mp = pad_to(s.Md, s.bk);
        void* ohT = s.take((size_t)d.num_tokens * Mp * s.es());
        void* dhT = s.take((size_t)DD * Mp * s.es());
        TR(tr_onehot_t(s.at, inp, ohT, Mp, s.Md, d.num_tokens, st));
        TR(tr_transpose_pad(s.at, dh, DD, dhT, Mp, s.Md, DD, st));
        TR(gemm_f32(s, ohT, Mp, dhT, d.num_tokens, DD, Mp, s.g(dn + "token_emb.emb.weight"), DD, nullptr, nullptr, 0));
        s.ar->off = mark;
    }
    if (cond_keep) TR(tr_zero_clip_rows(dctx, cond_keep, B, T, DD, st));
    // context -> x_s (+ patch_embed_dec_s) ; the audio half has no parameters behind it
    TR(tr_copy_cols(dctx, DD, dx_s, d.dim, s.M, d.dim, 0, st));
    DIMX_TRY(bias_adjoint(s, dx_s, s.g("patch_embed_dec_s"), s.M, d.dim));
    DIMX_TRY(ln_bwd_full(s, ej.out, "norm_s.weight", "norm_s.bias", dx_s, d_ej, s.M, d.dim));
    DIMX_TRY(enc_bwd(s, ej, d_ej, d_es));
    DIMX_TRY(enc_bwd(s, es, d_es, d_x0));
    DIMX_TRY(bias_adjoint(s, d_x0, s.g("patch_embed_s"), s.M, d.dim_in));
    return step_finish(s, "train", need);
}

// How a step is launched (measured on MI355X, profiles/r04_train_step.txt): the step is GPU-bound at every batch size (B = 2: 5.2 ms
// for ~450 dependent kernels), so replaying it from a hipGraph costs the same GPU time as launching it kernel by kernel and only
// frees the host thread; the weight-gradient side stream buys 3-5 % from 4 096 rows up and costs as much below (its event
// edges), and as parallel BRANCHES of a captured graph it is slower than either (12.5 vs 11.8 / 12.1 ms at B = 16).  Hence:
//   rows >= 4096: kernel by kernel, weight gradients on the side stream;   rows < 4096: captured graph, one stream.
// DIMX_TRAIN_GRAPH=0|1 and DIMX_TRAIN_SIDE=0|1 force either choice (read per call: tests flip them).
static int env_flag(const char* name) {
    const char* v = getenv(name);
    return (v && v[0]) ? (atoi(v) != 0 ? 1 : 0) : -1;
}
static bool train_use_graph(int rows) {
    const int f = env_flag("DIMX_TRAIN_GRAPH");
    return f >= 0 ? f == 1 : rows < 4096;
}
static bool train_use_side(int rows) {
    const int f = env_flag("DIMX_TRAIN_SIDE");
    return f >= 0 ? f == 1 : !train_use_graph(rows);
}

// ---------------------------------------------------------------------------------------------------------------- legacy generator
// One forward + backward pass of ListenerGenerator.forward as the reference's loop calls it (code/x_engine.py:8-36 ->
// code/seq2seq.py:235-278 with Transformer.forward :46-67): bidirectional encoder over the frozen speaker VQ-VAE's features, the
// listener-id row in front of the context, the teacher-forced decoder with absolute positions, cross entropy + the continuous loss
// of the decoded arg-max codes, which trains the listener VQ-VAE's DECODER.
static int legacy_run(dimx_handle h, const float* params, float* grads, const float* x_speaker, const int32_t* z_l, const float* v_listener,
                      const uint8_t* mask, const int32_t* listener_ids, const float* codebook, const float* pe, int B, int T, float* loss_out,
                      float* pred_out, float* logits_out, void* ws, size_t ws_bytes, hipStream_t st, size_t* need, bool use_side) {
    TrainState* ts;
    DIMX_TRY(state_of(h, &ts));
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(h->variant == 1, DIMX_ERR_ARG, "train_legacy: the handle is not the legacy variant");
    DIMX_REQUIRE(B >= 1 && T >= 2 && T + 1 <= d.max_seq_len, DIMX_ERR_ARG, "train_legacy: B=%d T=%d out of range", B, T);
    DIMX_REQUIRE(d.num_tokens == 512 && d.dim_a == 0, DIMX_ERR_ARG, "train_legacy: 512 codes, no audio stream");
    Arena ar(ws, ws_bytes);
    Step s(h, ts->plan, params, grads, &ar, st, h->at, B, T, T - 1);
    const bool ids = listener_ids != nullptr;
    const int DD = d.dim, F = std::max(DD * d.ff_mult, d.vq_inter), inner = d.heads * d.dim_head, H = d.vq_hidden;
    const int Lk = ids ? T + 1 : T, nd = ids ? T : T - 1, n = T - 1, E = 256;
    const int rows_max = B * (T + 1);
    s.reserve_part(F);
    if (use_side) DIMX_TRY(s.use_side_stream(*ts, std::max(F, 3 * inner), rows_max));   // the widest dy^T of the step: ff1's [F][rows]
    {
        const size_t n_ln = (size_t)(2 * d.enc_depth + 3 * d.dec_depth + 4 * d.vq_layers + 8);
        const size_t n_b = (size_t)(2 * d.enc_depth + 2 * d.dec_depth + 3 * d.vq_layers + 8);
        s.alloc_pool(n_ln * (kLnBlocks + 4) * (size_t)DD + n_b * (size_t)std::max(kTrSlabs, ceil_div(rows_max, 32) + 1) * (size_t)F + 4096);
    }
    const bool live = ws != nullptr;
    DIMX_TRY(s.zero_grads());

    // ---------------- encoder (mask-only attention: Encoder, not causal) over x_speaker [B, T, 8 x 128]
    EncSave e;
    DIMX_TRY(enc_fwd(s, e, "generator.encoder.", x_speaker, d.spk_face_quan_num * d.vq_zdim, mask, mask, 0));
    // ---------------- context (+ the listener-id row in front), tokens
    DecSave D;
    DIMX_TRY(dec_prepare(s, D, "generator.decoder.net.", d.dec_depth));
    Lin fc;
    if (ids) {
        fc = make_lin(s, "fc_listener.weight", "fc_listener.bias");
        DIMX_TRY(prep_lin(s, fc));
    }
    DIMX_TRY(flush_prep(s));
    const float* ctx = e.out;
    const uint8_t* cmask = mask;
    const int32_t* zsrc = z_l;
    float *e_relu = nullptr, *lid = nullptr;
    if (ids) {
        e_relu = s.f32((size_t)B * E);
        lid = s.f32((size_t)B * DD);
        float* cj = s.f32((size_t)B * Lk * DD);
        int32_t* z_ext = (int32_t*)s.take((size_t)B * Lk * 4);
        uint8_t* m_ext = (uint8_t*)s.take((size_t)B * Lk);
        TR(tr_emb_relu(s.p("listener_embeddings.weight"), listener_ids, e_relu, B, E, st));
        DIMX_TRY(lin_fwd(s, fc, e_relu, E, B, lid, DD));
        TR(tr_prepend_row(lid, e.out, cj, B, T, DD, 0, st));
        TR(tr_prepend_tokens(z_l, mask, z_ext, m_ext, B, T, st));
        ctx = cj;
        cmask = m_ext;
        zsrc = z_ext;
    }
    int32_t* inp = (int32_t*)s.take((size_t)B * nd * 4);
    int32_t* tgt = (int32_t*)s.take((size_t)B * nd * 4);
    TR(launch_shift_tokens(zsrc, inp, tgt, B, nd + 1, st));
    float* logits = logits_out ? logits_out : s.f32((size_t)B * nd * d.num_tokens);
    DIMX_TRY(dec_fwd(s, D, inp, B, nd, ctx, Lk, DD, cmask, nullptr, true, logits));
    float* dlogits = s.f32((size_t)B * nd * d.num_tokens);
    float* row_loss = s.f32((size_t)B * nd);
    TR(tr_cross_entropy(logits, tgt, row_loss, dlogits, B * nd, loss_out, st));
    // ---------------- decoded arg-max codes -> continuous loss (logits[:, 1:] when the id row shifted them)
    int32_t* idx = (int32_t*)s.take((size_t)B * n * 4);
    TR(tr_argmax512(logits, idx, B, nd, n, ids ? 1 : 0, st));
    float* pred = pred_out ? pred_out : s.f32((size_t)B * n * d.vq_in_dim);
    VqDecSave V;
    DIMX_TRY(vqdec_fwd(s, V, "listener_vq.decoder.", idx, codebook, pe, B, n, pred));
    float* rown = s.f32((size_t)2 * B * n);
    float* dpred = s.f32((size_t)B * n * d.vq_in_dim);
    DIMX_REQUIRE(d.vq_in_dim == 56, DIMX_ERR_ARG, "train_legacy: the continuous loss is written for 56 coefficients");
    TR(tr_cont_loss(pred, v_listener, mask, B, T, n, rown, dpred, loss_out ? loss_out + 2 : nullptr, st));

    // ---------------- backward
    DIMX_TRY(vqdec_bwd(s, V, dpred));
    float* dctx = s.f32((size_t)B * Lk * DD);
    if (live) DIMX_HIP(hipMemsetAsync(dctx, 0, (size_t)B * Lk * DD * sizeof(float), st));
    DIMX_TRY(dec_bwd(s, D, dlogits, dctx));
    float* d_enc = dctx;
    if (ids) {
        float* d_lid = s.f32((size_t)B * DD);
        d_enc = s.f32((size_t)s.M * DD);
        TR(tr_prepend_row(d_lid, d_enc, dctx, B, T, DD, 1, st));
        float* d_e = s.f32((size_t)B * E);
        DIMX_TRY(lin_bwd(s, fc, e_relu, E, d_lid, DD, B, d_e, E, false));
        TR(tr_emb_relu_bwd(s.p("listener_embeddings.weight"), listener_ids, d_e, s.g("listener_embeddings.weight"), B, E, st));
    }
    DIMX_TRY(enc_bwd(s, e, d_enc, nullptr));
    return step_finish(s, "train_legacy", need);
}

size_t dimx_train_legacy_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 2) return 0;
    size_t need = 0;   // sized with the listener-id row and the side stream's slots: the branches that allocate the most
    return legacy_run(h, nullptr, nullptr, nullptr, nullptr, nullptr, present<const uint8_t>(), present<const int32_t>(), nullptr, nullptr, B, T,
                      nullptr, nullptr, nullptr, nullptr, 0, nullptr, &need, true) == DIMX_OK ? need : 0;
}

int dimx_train_legacy_forward_backward(dimx_handle h, const float* params, float* grads, const float* x_speaker, const int32_t* z_l,
                                       const float* v_listener, const uint8_t* mask, const int32_t* listener_ids, const float* codebook,
                                       const float* pe, int B, int T, float* loss_out, float* pred_out, float* logits_out, void* ws,
                                       size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && params && grads && x_speaker && z_l && v_listener && mask && codebook && pe && loss_out && ws, DIMX_ERR_ARG,
                 "train_legacy: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)x_speaker % 16) == 0 &&
                     ((uintptr_t)codebook % 16) == 0 && ((uintptr_t)pe % 16) == 0,
                 DIMX_ERR_ARG, "train_legacy: workspace must be 256-byte aligned, arenas / inputs 16-byte aligned");
    DIMX_HIP(hipSetDevice(h->device));
    const bool side = train_use_side(B * T);
    auto run = [&](void* w, size_t w_bytes, hipStream_t st, size_t* need) {
        return legacy_run(h, params, grads, x_speaker, z_l, v_listener, mask, listener_ids, codebook, pe, B, T, loss_out, pred_out, logits_out, w,
                          w_bytes, st, need, side);
    };
    DIMX_TRY(check_workspace("train_legacy", ws_bytes, run));
    return run(ws, ws_bytes, (hipStream_t)stream, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- SLM pre-training
// One forward + backward pass of SLM.forward (code/seq2seq_pretrain.py:300-323) as the reference's pre-training loop differentiates it
// (code/train_s2s_pretrain.py:41-64 -> x_engine_pt.train_epoch): masked speaker / listener streams through encoder_s / encoder_l
// (bidirectional), encoder_joint over the 2T concatenation AND over each stream alone (:200-221 -- one pass over 4 B T rows here:
// every Linear / LayerNorm / feed-forward sees all rows, the attention runs per segment [B, 2T] and [2B, T], so each weight is used
// once and its gradient is ONE GEMM), InfoNCE between the clip means (:270-289), the decoder twice (z_s from the listener half of
// x_joint, z_l from the speaker half, :223-243 -- one pass over a batch of 2 B), two cross entropies, and the continuous losses of
// the decoded arg-max codes through BOTH VQ-VAE decoders, which they train.
static int slm_run(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_listener, const float* v_audio,
                   const uint8_t* mask, const uint8_t* mask_speaker, const uint8_t* mask_listener, const int32_t* z_s, const int32_t* z_l,
                   const float* codebook_s, const float* codebook_l, const float* pe_s, const float* pe_l, int B, int T, float* loss_out, void* ws,
                   size_t ws_bytes, hipStream_t st, size_t* need, bool use_side) {
    TrainState* ts;
    DIMX_TRY(state_of(h, &ts));
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(h->variant == 2, DIMX_ERR_ARG, "train_slm: the handle is not the SLM variant");
    DIMX_REQUIRE(B >= 1 && T >= 2 && 2 * T <= d.max_seq_len, DIMX_ERR_ARG, "train_slm: B=%d T=%d out of range (2 T <= %d)", B, T, d.max_seq_len);
    DIMX_REQUIRE(d.num_tokens == 512 && d.vq_in_dim == 56 && d.dim_in == 56, DIMX_ERR_ARG, "train_slm: 512 codes, 56 coefficients");
    Arena ar(ws, ws_bytes);
    Step s(h, ts->plan, params, grads, &ar, st, h->at, B, T, T - 1);
    const int C = d.dim, DD = d.dim + d.dim_a, F = std::max(DD * d.ff_mult, d.vq_inter), inner = d.heads * d.dim_head, n = T - 1;
    const int BT = B * T, rows_max = 4 * BT;
    s.reserve_part(F);
    if (use_side) DIMX_TRY(s.use_side_stream(*ts, std::max(F, 3 * inner), rows_max));   // the widest dy^T of the step: ff1's [F][rows]
    {   // partial rows of the deferred column reductions
        const size_t n_ln_c = (size_t)(3 * (2 * d.enc_depth + 1) + 6 + 2 * 4 * d.vq_layers + 8), n_ln_dd = (size_t)(3 * d.dec_depth + 2);
        const size_t n_b = (size_t)(3 * 2 * d.enc_depth + 2 * d.dec_depth + 2 * 3 * d.vq_layers + 16);
        s.alloc_pool(n_ln_c * (kLnBlocks + 4) * (size_t)std::max(C, d.vq_hidden) + n_ln_dd * (kLnBlocks + 4) * (size_t)DD +
                     n_b * (size_t)std::max(kTrSlabs, ceil_div(rows_max, 32) + 1) * (size_t)F + 4096);
    }
    const bool live = ws != nullptr;
    DIMX_TRY(s.zero_grads());

    // ---------------- masks: keep-masks of the masked-out input rows, the joint encoder's key masks
    uint8_t* keep_s = (uint8_t*)s.take((size_t)BT);
    uint8_t* keep_l = (uint8_t*)s.take((size_t)BT);
    uint8_t* mj = (uint8_t*)s.take((size_t)4 * BT);   // [B, 2T] = cat(mask, mask) along time | [2B, T] = mask twice
    TR(tr_copy_bt_u8(mask_speaker, T, keep_s, T, B, T, 1, st));
    TR(tr_copy_bt_u8(mask_listener, T, keep_l, T, B, T, 1, st));
    TR(tr_copy_bt_u8(mask, T, mj, 2 * T, B, T, 0, st));
    TR(tr_copy_bt_u8(mask, T, mj + T, 2 * T, B, T, 0, st));
    TR(tr_copy_bt_u8(mask, T, mj + 2 * BT, T, B, T, 0, st));
    TR(tr_copy_bt_u8(mask, T, mj + 3 * BT, T, B, T, 0, st));
    // ---------------- stream encoders on (v + patch_embed) with the masked-out frames zeroed
    float* x0s = s.f32((size_t)BT * d.dim_in);
    float* x0l = s.f32((size_t)BT * d.dim_in);
    TR(tr_add_rows(v_speaker, d.dim_in, s.p("patch_embed_s"), nullptr, 0.f, T, x0s, d.dim_in, BT, d.dim_in, st));
    TR(tr_zero_rows(x0s, keep_s, BT, d.dim_in, st));
    TR(tr_add_rows(v_listener, d.dim_in, s.p("patch_embed_l"), nullptr, 0.f, T, x0l, d.dim_in, BT, d.dim_in, st));
    TR(tr_zero_rows(x0l, keep_l, BT, d.dim_in, st));
    EncSave es, el, ej;
    DIMX_TRY(enc_fwd(s, es, "encoder_s.", x0s, d.dim_in, mask, mask, 0));
    DIMX_TRY(enc_fwd(s, el, "encoder_l.", x0l, d.dim_in, mask, mask, 0));
    // ---------------- joint encoder: rows [0, 2BT) = cat(x_s, x_l) along time, [2BT, 3BT) = x_s, [3BT, 4BT) = x_l
    float* xin = s.f32((size_t)4 * BT * C);
    TR(tr_copy_bt(es.out, (long)T * C, C, xin, (long)2 * T * C, C, B, T, C, nullptr, 0, st));
    TR(tr_copy_bt(el.out, (long)T * C, C, xin + (size_t)T * C, (long)2 * T * C, C, B, T, C, nullptr, 0, st));
    TR(tr_copy_cols(es.out, C, xin + (size_t)2 * BT * C, C, BT, C, 0, st));
    TR(tr_copy_cols(el.out, C, xin + (size_t)3 * BT * C, C, BT, C, 0, st));
    const std::vector<AttnSeg> segs = {{0, B, 2 * T, mj}, {2 * BT, 2 * B, T, mj + 2 * BT}};
    DIMX_TRY(enc_fwd(s, ej, "encoder_joint.", xin, C, mj, mj, 0, &segs));
    float* xn = s.f32((size_t)4 * BT * C);   // norm(x_joint) | norm_s(x_s) | norm_l(x_l)
    TR(launch_layernorm(DIMX_F32, ej.out, xn, s.p("norm.weight"), s.p("norm.bias"), 2 * BT, C, st));
    TR(launch_layernorm(DIMX_F32, ej.out + (size_t)2 * BT * C, xn + (size_t)2 * BT * C, s.p("norm_s.weight"), s.p("norm_s.bias"), BT, C, st));
    TR(launch_layernorm(DIMX_F32, ej.out + (size_t)3 * BT * C, xn + (size_t)3 * BT * C, s.p("norm_l.weight"), s.p("norm_l.bias"), BT, C, st));
    // ---------------- InfoNCE (forward and adjoint: the whole thing is a few [B, C] reductions)
    float* d_xn = s.f32((size_t)4 * BT * C);
    float* nce_scr = s.f32(tr_nce_scratch_floats(B, C));
    TR(tr_nce(xn + (size_t)2 * BT * C, xn + (size_t)3 * BT * C, mask, B, T, C, nce_scr, loss_out ? loss_out + 8 : nullptr, d_xn + (size_t)2 * BT * C,
              d_xn + (size_t)3 * BT * C, st));
    // ---------------- decoder over 2B sequences: rows [0, B) predict z_s from the LISTENER half of x_joint, rows [B, 2B) z_l from the speaker half
    float* ctx = s.f32((size_t)2 * BT * DD);
    TR(tr_copy_bt(xn + (size_t)T * C, (long)2 * T * C, C, ctx, (long)T * DD, DD, B, T, C, s.p("patch_embed_dec_l"), 0, st));
    TR(tr_copy_bt(xn, (long)2 * T * C, C, ctx + (size_t)BT * DD, (long)T * DD, DD, B, T, C, s.p("patch_embed_dec_s"), 0, st));
    TR(tr_copy_cols(v_audio, d.dim_a, ctx + C, DD, BT, d.dim_a, 0, st));
    TR(tr_copy_cols(v_audio, d.dim_a, ctx + (size_t)BT * DD + C, DD, BT, d.dim_a, 0, st));
    int32_t* zc = (int32_t*)s.take((size_t)2 * BT * 4);
    TR(tr_mask_tokens(z_s, mask_speaker, zc, (long)BT, st));
    TR(tr_mask_tokens(z_l, mask_listener, zc + BT, (long)BT, st));
    int32_t* inp = (int32_t*)s.take((size_t)2 * B * n * 4);
    int32_t* tgt = (int32_t*)s.take((size_t)2 * B * n * 4);
    TR(launch_shift_tokens(zc, inp, tgt, 2 * B, T, st));
    DecSave D;
    DIMX_TRY(dec_prepare(s, D, "decoder_joint.net.", d.dec_depth));
    DIMX_TRY(flush_prep(s));
    float* logits = s.f32((size_t)2 * B * n * d.num_tokens);
    DIMX_TRY(dec_fwd(s, D, inp, 2 * B, n, ctx, T, DD, mj + 2 * BT, nullptr, true, logits));
    float* dlogits = s.f32((size_t)2 * B * n * d.num_tokens);
    float* row_loss = s.f32((size_t)2 * B * n);
    const size_t half = (size_t)B * n;
    TR(tr_cross_entropy(logits, tgt, row_loss, dlogits, B * n, loss_out, st));
    TR(tr_cross_entropy(logits + half * d.num_tokens, tgt + half, row_loss + half, dlogits + half * d.num_tokens, B * n, loss_out ? loss_out + 2 : nullptr, st));
    // ---------------- decoded arg-max codes -> continuous losses over the masked-out frames, through the two VQ-VAE decoders
    int32_t* idx = (int32_t*)s.take((size_t)2 * B * n * 4);
    TR(tr_argmax512(logits, idx, 2 * B, n, n, 0, st));
    float* pred_s = s.f32((size_t)B * n * d.vq_in_dim);
    float* pred_l = s.f32((size_t)B * n * d.vq_in_dim);
    VqDecSave Vs, Vl;
    DIMX_TRY(vqdec_fwd(s, Vs, "speaker_vq.decoder.", idx, codebook_s, pe_s, B, n, pred_s));
    DIMX_TRY(vqdec_fwd(s, Vl, "listener_vq.decoder.", idx + half, codebook_l, pe_l, B, n, pred_l));
    float* rown = s.f32((size_t)2 * B * n);
    float* dpred_s = s.f32((size_t)B * n * d.vq_in_dim);
    float* dpred_l = s.f32((size_t)B * n * d.vq_in_dim);
    TR(tr_cont_loss(pred_s, v_speaker, mask_speaker, B, T, n, rown, dpred_s, loss_out ? loss_out + 4 : nullptr, st));
    TR(tr_cont_loss(pred_l, v_listener, mask_listener, B, T, n, rown, dpred_l, loss_out ? loss_out + 6 : nullptr, st));

    // ---------------- backward
    DIMX_TRY(vqdec_bwd(s, Vs, dpred_s));
    DIMX_TRY(vqdec_bwd(s, Vl, dpred_l));
    float* dctx = s.f32((size_t)2 * BT * DD);
    if (live) DIMX_HIP(hipMemsetAsync(dctx, 0, (size_t)2 * BT * DD * sizeof(float), st));
    DIMX_TRY(dec_bwd(s, D, dlogits, dctx));
    {   // context -> the two halves of norm(x_joint) (+ the decoder-side patch embeddings); the audio columns have no parameters behind them
        float* dc = s.f32((size_t)2 * BT * C);
        TR(tr_copy_cols(dctx, DD, dc, C, 2 * BT, C, 0, st));
        DIMX_TRY(bias_adjoint(s, dc, s.g("patch_embed_dec_l"), BT, C));
        DIMX_TRY(bias_adjoint(s, dc + (size_t)BT * C, s.g("patch_embed_dec_s"), BT, C));
        TR(tr_copy_bt(dc, (long)T * C, C, d_xn + (size_t)T * C, (long)2 * T * C, C, B, T, C, nullptr, 0, st));
        TR(tr_copy_bt(dc + (size_t)BT * C, (long)T * C, C, d_xn, (long)2 * T * C, C, B, T, C, nullptr, 0, st));
    }
    float* d_ej = s.f32((size_t)4 * BT * C);
    DIMX_TRY(ln_bwd_full(s, ej.out, "norm.weight", "norm.bias", d_xn, d_ej, 2 * BT, C));
    DIMX_TRY(ln_bwd_full(s, ej.out + (size_t)2 * BT * C, "norm_s.weight", "norm_s.bias", d_xn + (size_t)2 * BT * C, d_ej + (size_t)2 * BT * C, BT, C));
    DIMX_TRY(ln_bwd_full(s, ej.out + (size_t)3 * BT * C, "norm_l.weight", "norm_l.bias", d_xn + (size_t)3 * BT * C, d_ej + (size_t)3 * BT * C, BT, C));
    float* d_xin = s.f32((size_t)4 * BT * C);
    DIMX_TRY(enc_bwd(s, ej, d_ej, d_xin));
    // x_s / x_l fed the joint pass twice: the stand-alone rows + their half of the concatenation
    TR(tr_copy_bt(d_xin, (long)2 * T * C, C, d_xin + (size_t)2 * BT * C, (long)T * C, C, B, T, C, nullptr, 1, st));
    TR(tr_copy_bt(d_xin + (size_t)T * C, (long)2 * T * C, C, d_xin + (size_t)3 * BT * C, (long)T * C, C, B, T, C, nullptr, 1, st));
    float* d_x0s = s.f32((size_t)BT * d.dim_in);
    float* d_x0l = s.f32((size_t)BT * d.dim_in);
    DIMX_TRY(enc_bwd(s, es, d_xin + (size_t)2 * BT * C, d_x0s));
    DIMX_TRY(enc_bwd(s, el, d_xin + (size_t)3 * BT * C, d_x0l));
    TR(tr_zero_rows(d_x0s, keep_s, BT, d.dim_in, st));
    TR(tr_zero_rows(d_x0l, keep_l, BT, d.dim_in, st));
    DIMX_TRY(bias_adjoint(s, d_x0s, s.g("patch_embed_s"), BT, d.dim_in));
    DIMX_TRY(bias_adjoint(s, d_x0l, s.g("patch_embed_l"), BT, d.dim_in));
    return step_finish(s, "train_slm", need);
}

size_t dimx_train_slm_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 2) return 0;
    size_t need = 0;
    return slm_run(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, T,
                   nullptr, nullptr, 0, nullptr, &need, true) == DIMX_OK ? need : 0;
}

int dimx_train_slm_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_listener,
                                    const float* v_audio, const uint8_t* mask, const uint8_t* mask_speaker, const uint8_t* mask_listener,
                                    const int32_t* z_s, const int32_t* z_l, const float* codebook_s, const float* codebook_l, const float* pe_s,
                                    const float* pe_l, int B, int T, float* loss_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && params && grads && v_speaker && v_listener && v_audio && mask && mask_speaker && mask_listener && z_s && z_l && codebook_s &&
                     codebook_l && pe_s && pe_l && loss_out && ws,
                 DIMX_ERR_ARG, "train_slm: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)codebook_s % 16) == 0 &&
                     ((uintptr_t)codebook_l % 16) == 0 && ((uintptr_t)pe_s % 16) == 0 && ((uintptr_t)pe_l % 16) == 0,
                 DIMX_ERR_ARG, "train_slm: workspace must be 256-byte aligned, arenas / codebooks / pe 16-byte aligned");
    DIMX_HIP(hipSetDevice(h->device));
    const bool side = train_use_side(4 * B * T);
    auto run = [&](void* w, size_t w_bytes, hipStream_t st, size_t* need) {
        return slm_run(h, params, grads, v_speaker, v_listener, v_audio, mask, mask_speaker, mask_listener, z_s, z_l, codebook_s, codebook_l, pe_s,
                       pe_l, B, T, loss_out, w, w_bytes, st, need, side);
    };
    DIMX_TRY(check_workspace("train_slm", ws_bytes, run));
    return run(ws, ws_bytes, (hipStream_t)stream, nullptr);
}

size_t dimx_train_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 2) return 0;
    size_t need = 0;   // sized with both masks and the side stream's slots (that choice may differ between calls): the most a call takes
    return train_run(h, nullptr, nullptr, nullptr, nullptr, present<const uint8_t>(), nullptr, present<const uint8_t>(), B, T, nullptr, nullptr,
                     nullptr, 0, nullptr, &need, true) == DIMX_OK ? need : 0;
}

// The step as a hipGraph.  Shapes are static per (B, T) and the step reads nothing from the host, so a call whose arguments
// (every pointer, B, T) equal the previous call's is captured once -- the caller's stream forks into the side stream inside the
// capture, so the graph keeps the dX chain and the weight-gradient GEMMs as parallel branches -- and replayed from then on: one
// hipGraphLaunch instead of ~540 kernel launches.  A caller that hands over new buffers every step (or DIMX_TRAIN_NO_GRAPH=1)
// stays on the kernel-by-kernel path; dimx.train_hip.HipTrainer stages its batch in persistent buffers for this reason.
int dimx_train_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_audio,
                                const uint8_t* mask, const int32_t* z_l, const uint8_t* kv_mask, int B, int T, float* loss_out,
                                float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && params && grads && v_speaker && v_audio && mask && z_l && loss_out && ws, DIMX_ERR_ARG, "train: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0, DIMX_ERR_ARG,
                 "train: workspace must be 256-byte aligned, arenas 16-byte aligned");
    DIMX_HIP(hipSetDevice(h->device));
    const bool side = train_use_side(B * T);
    auto run = [&](void* w, size_t w_bytes, hipStream_t on, size_t* need) {
        return train_run(h, params, grads, v_speaker, v_audio, mask, z_l, kv_mask, B, T, loss_out, logits_out, w, w_bytes, on, need, side);
    };
    DIMX_TRY(check_workspace("train", ws_bytes, run));
    TrainState* ts;
    DIMX_TRY(state_of(h, &ts));
    hipStream_t st = (hipStream_t)stream;
    const StepGraphKey key{params, grads, v_speaker, v_audio, mask, z_l, kv_mask, loss_out, logits_out, ws, ws_bytes, B, T, h->at, side ? 1 : 0,
                           h->twin_on, h->twin_lookahead, h->tcond_keep};
    if (train_use_graph(B * T)) {
        if (ts->exec && ts->graph_key == key) {
            ++ts->graph_launches;
            DIMX_HIP(hipGraphLaunch(ts->exec, st));
            return DIMX_OK;
        }
        if (ts->have_last && ts->last_key == key) {   // second call in a row with these arguments: capture (the first one warmed every kernel up)
            ts->drop_graph();
            if (!ts->cap) DIMX_HIP(hipStreamCreateWithFlags(&ts->cap, hipStreamNonBlocking));
            hipGraph_t graph = nullptr;
            DIMX_HIP(hipStreamBeginCapture(ts->cap, hipStreamCaptureModeThreadLocal));
            const int rc2 = run(ws, ws_bytes, ts->cap, nullptr);
            const hipError_t ce = hipStreamEndCapture(ts->cap, &graph);
            if (rc2 != DIMX_OK || ce != hipSuccess) {
                if (graph) (void)hipGraphDestroy(graph);
                (void)hipGetLastError();
                ts->have_last = false;   // do not try again with these arguments
                if (rc2 != DIMX_OK) return rc2;
                fprintf(stderr, "dimx: the training step could not be captured (%s); it stays on the kernel-by-kernel path\n", hipGetErrorString(ce));
            } else {
                size_t nodes = 0;
                (void)hipGraphGetNodes(graph, nullptr, &nodes);
                ts->graph_nodes = (long)nodes;
                const hipError_t ie = hipGraphInstantiate(&ts->exec, graph, nullptr, nullptr, 0);
                (void)hipGraphDestroy(graph);
                DIMX_HIP(ie);
                ts->graph_key = key;
                ++ts->graph_launches;
                DIMX_HIP(hipGraphLaunch(ts->exec, st));
                return DIMX_OK;
            }
        }
    }
    ts->last_key = key;
    ts->have_last = true;
    ++ts->eager_runs;
    return run(ws, ws_bytes, st, nullptr);
}

// {graph launches, kernel-by-kernel runs, nodes of the captured step} of this handle's training steps
int dimx_train_graph_stats(dimx_handle h, int64_t* out3) {
    DIMX_REQUIRE(h && out3, DIMX_ERR_ARG, "train_graph_stats: null argument");
    TrainState* ts;
    DIMX_TRY(state_of(h, &ts));
    out3[0] = ts->graph_launches;
    out3[1] = ts->eager_runs;
    out3[2] = ts->graph_nodes;
    return DIMX_OK;
}

int dimx_train_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float max_norm, float* scratch, void* stream) {
    DIMX_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch && n > 0 && step >= 1, DIMX_ERR_ARG, "train_adamw: bad argument");
    // adamw_kernel reads all four arenas as float4 (tr_grad_norm checks grads once more): refused before any launch
    DIMX_REQUIRE(((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)exp_avg % 16) == 0 && ((uintptr_t)exp_avg_sq % 16) == 0,
                 DIMX_ERR_ARG, "train_adamw: params, grads, exp_avg and exp_avg_sq must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    DIMX_TRY(tr_grad_norm(grads, (long)n, max_norm, scratch, scratch + 1024, st));
    return tr_adamw(params, grads, exp_avg, exp_avg_sq, (long)n, lr, beta1, beta2, eps, weight_decay, step, scratch + 1024, st);
}

int dimx_set_train_lookahead(dimx_handle h, int on, int lookahead) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_train_lookahead: online fine-tuning is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    h->twin_on = on ? 1 : 0;
    h->twin_lookahead = on ? lookahead : 0;
    return DIMX_OK;
}

int dimx_set_train_cond_keep(dimx_handle h, const uint8_t* keep_dev) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_train_cond_keep: condition dropout is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    h->tcond_keep = keep_dev;
    return DIMX_OK;
}

int dimx_train_cond_keep(dimx_handle h, const uint8_t** keep_dev) {
    DIMX_REQUIRE(h && keep_dev, DIMX_ERR_ARG, "train_cond_keep: null argument");
    *keep_dev = h->tcond_keep;
    return DIMX_OK;
}

int dimx_train_lookahead(dimx_handle h, int* on, int* lookahead) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (on) *on = h->twin_on;
    if (lookahead) *lookahead = h->twin_lookahead;
    return DIMX_OK;
}

int dimx_op_train_attention(int mfma, const float* q, const float* k, const float* v, const float* d_o, const uint8_t* kmask,
                            const uint8_t* kmask2, int B, int H, int Lq, int Lk, int causal, float scale, float* o, float* lse,
                            float* delta, float* dq, float* dk, float* dv, void* stream) {
    return dimx_op_train_attention_win(mfma, q, k, v, d_o, kmask, kmask2, B, H, Lq, Lk, causal, scale, 0, 0, o, lse, delta, dq, dk, dv, stream);
}

int dimx_op_train_attention_win(int mfma, const float* q, const float* k, const float* v, const float* d_o, const uint8_t* kmask,
                                const uint8_t* kmask2, int B, int H, int Lq, int Lk, int causal, float scale, int win, int lookahead,
                                float* o, float* lse, float* delta, float* dq, float* dk, float* dv, void* stream) {
    DIMX_REQUIRE(q && k && v && o && lse && B > 0 && H > 0 && Lq > 0 && Lk > 0, DIMX_ERR_ARG, "op_train_attention: bad argument");
    DIMX_REQUIRE(!(win && causal), DIMX_ERR_ARG, "op_train_attention: the window replaces causal; set one of them");
    DIMX_REQUIRE(!d_o || (delta && dq && dk && dv), DIMX_ERR_ARG, "op_train_attention: the backward pass needs delta, dq, dk, dv");
    TrAttn t;
    memset(&t, 0, sizeof(t));
    t.B = B; t.H = H; t.Lq = Lq; t.Lk = Lk;
    t.ldq = t.ldk = t.ldv = t.ldo = H * 64;
    t.scale = scale;
    t.causal = causal;
    tr_attn_window(t, win, lookahead);
    t.kmask = kmask;
    t.kmask2 = kmask2;
    t.mfma = mfma < 0 ? 0 : (mfma > 2 ? 2 : mfma);
    hipStream_t st = (hipStream_t)stream;
    DIMX_TRY(tr_attn_fwd(t, q, k, v, o, lse, st));
    if (d_o) DIMX_TRY(tr_attn_bwd(t, q, k, v, o, d_o, lse, delta, dq, H * 64, dk, H * 64, dv, H * 64, st));
    return DIMX_OK;
}

}  // extern "C"

// The row-count-dependent operators of the step alone (unit parity).  Each entry builds a Step over the caller's scratch and calls
// the step's own helper (ln_adjoint, bias_adjoint, tr_prep_fused with the padding of fwd_operands / lin_bwd, tr_cross_entropy), so
// rows per block, slab counts, chunk widths and the deferred multi_finish are planned by the code the training step runs.
// walk(s): the helper calls, made twice -- without memory first (nothing launched: an undersized scratch is refused before a kernel
// writes), then live.
template <class Walk>
static int op_with_pool(const char* tag, int at, float* scratch, size_t scratch_floats, hipStream_t st, Walk walk) {
    DIMX_REQUIRE(scratch && ((uintptr_t)scratch % 256) == 0, DIMX_ERR_ARG, "%s: scratch must be 256-byte aligned", tag);
    for (int pass = 0; pass < 2; ++pass) {
        Arena ar(pass ? (void*)scratch : nullptr, pass ? scratch_floats * sizeof(float) : 0);
        Step s(nullptr, nullptr, nullptr, nullptr, &ar, st, at, 1, 1, 1);
        s.alloc_pool(scratch_floats);
        DIMX_TRY(walk(s));
        DIMX_TRY(flush_fin(s));
        DIMX_REQUIRE(!s.pool_overflow, DIMX_ERR_WORKSPACE, "%s: scratch of %zu floats is too small", tag, scratch_floats);
    }
    return DIMX_OK;
}

extern "C" {

int dimx_op_train_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, int accumulate, int M, int C, float* dgamma,
                                float* dbeta, float* scratch, size_t scratch_floats, void* stream) {
    DIMX_REQUIRE(x && gamma && dy && dx && dgamma && M >= 1, DIMX_ERR_ARG, "op_train_layernorm_bwd: bad argument");
    DIMX_REQUIRE(C == 384 || C == 512 || C == 768 || C == 1152, DIMX_ERR_ARG, "op_train_layernorm_bwd: C=%d (384, 512, 768 or 1152)", C);
    return op_with_pool("op_train_layernorm_bwd", DIMX_F32, scratch, scratch_floats, (hipStream_t)stream,
                        [&](Step& s) { return ln_adjoint(s, x, gamma, dy, dx, accumulate ? 1 : 0, M, C, dgamma, dbeta); });
}

int dimx_op_train_colsum(const float* dy, int M, int C, float* out, float* scratch, size_t scratch_floats, void* stream) {
    DIMX_REQUIRE(dy && out && M >= 1 && C >= 1, DIMX_ERR_ARG, "op_train_colsum: bad argument");
    return op_with_pool("op_train_colsum", DIMX_F32, scratch, scratch_floats, (hipStream_t)stream,
                        [&](Step& s) { return bias_adjoint(s, dy, out, M, C); });
}

int dimx_op_train_prep(int dtype, int mode, const float* src, int lds, const float* src2, int lds2, const float* gamma, const float* beta,
                       int rows, int cols, void* o, size_t o_elems, void* t, size_t t_elems, float* colpart, size_t colpart_floats,
                       int* dims3, void* stream) {
    DIMX_REQUIRE(dtype == DIMX_F32 || dtype == DIMX_BF16, DIMX_ERR_ARG, "op_train_prep: operand type %d", dtype);
    DIMX_REQUIRE(src && o && t && dims3 && rows >= 1 && cols >= 1 && lds >= cols, DIMX_ERR_ARG, "op_train_prep: bad argument");
    Arena none(nullptr, 0);
    Step s(nullptr, nullptr, nullptr, nullptr, &none, (hipStream_t)stream, dtype, 1, rows, rows);
    const int Kp = pad_to(cols, s.bk), Mp = pad_to(rows, s.bk);   // fwd_operands: c.Kp / c.Mp; lin_bwd: Np / Mp
    int n_part = ceil_div(rows, 32);                               // lin_bwd: the rows of bias_part
    DIMX_REQUIRE(o_elems >= (size_t)rows * Kp && t_elems >= (size_t)cols * Mp && (!colpart || colpart_floats >= (size_t)n_part * cols),
                 DIMX_ERR_WORKSPACE, "op_train_prep: o needs %zu, t %zu elements, colpart %zu floats", (size_t)rows * Kp, (size_t)cols * Mp,
                 (size_t)n_part * cols);
    DIMX_TRY(tr_prep_fused(dtype, mode, src, lds, src2, lds2, gamma, rows, cols, o, Kp, t, Mp, colpart, &n_part, s.st, beta));
    dims3[0] = Kp;
    dims3[1] = Mp;
    dims3[2] = n_part;
    return DIMX_OK;
}

int dimx_op_train_cross_entropy(const float* logits, const int32_t* targets, int R, float* row_loss, float* dlogits, float* loss_out2,
                                void* stream) {
    DIMX_REQUIRE(logits && targets && row_loss && dlogits && loss_out2 && R >= 1, DIMX_ERR_ARG, "op_train_cross_entropy: bad argument");
    return tr_cross_entropy(logits, targets, row_loss, dlogits, R, loss_out2, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- VQ-VAE (stage 1)
// One forward + backward pass of the VQ-VAE's own training loop (code/train_vq.py:173-196): out, quant_loss, info = model(data);
// loss = calc_vq_loss(out, data, quant_loss, quant_loss_weight) (code/metrics/loss.py:6-11).  Encoder -> z; the inference
// argmin of vq.hip over a codebook copy made from the arena (same kernel, same summation order); straight-through latent; the
// decoder on it; L1 reconstruction.  Backward: the decoder down to d z_st, + the commitment term, the encoder; the codebook
// gradient from the codebook term alone.  Kernel by kernel on one stream (no captured graph, no side stream).
static int vq_run(dimx_handle h, int which, const float* params, float* grads, const float* x, int B, int T, float beta, float qw, float p,
                  uint64_t seed, long step, float* loss_out, float* pred_out, int32_t* idx_out, void* ws, size_t ws_bytes, hipStream_t st,
                  size_t* need) {
    TrainPlan* plan;
    DIMX_TRY(plan_of(h, vq_plan_kind(which), &plan));
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(B >= 1 && B <= 5000 && T >= 1 && T <= 65536 && (long)B * T <= (1l << 24), DIMX_ERR_ARG,
                 "train_vq: B=%d T=%d out of range (B <= 5000 positional rows)", B, T);
    DIMX_REQUIRE(p >= 0.f && p < 1.f && step >= 0, DIMX_ERR_ARG, "train_vq: dropout p=%g must be in [0, 1), step >= 0", p);
    const bool live = ws != nullptr;
    const float *pe_enc = nullptr, *pe_dec = nullptr;
    if (live) DIMX_TRY(vq_pe_buffers(h, which, &pe_enc, &pe_dec));
    Arena ar(ws, ws_bytes);
    Step s(h, plan, params, grads, &ar, st, h->at, B, T, T);
    const int H = d.vq_hidden, I = d.vq_inter, M = B * T, ZD = d.vq_zdim;
    s.reserve_part(I);
    {
        const size_t n_ln = (size_t)(4 * 2 * d.vq_layers + 8);
        const size_t n_b = (size_t)(3 * 2 * d.vq_layers + 12);
        s.alloc_pool(n_ln * (kLnBlocks + 4) * (size_t)H + n_b * (size_t)std::max(kTrSlabs, ceil_div(M, 32) + 1) * (size_t)I + 4096);
    }
    DIMX_TRY(s.zero_grads());
    const std::string pre = which == 0 ? "speaker_vq." : "listener_vq.";
    const float* book = s.p(pre + "quantize.embedding.weight");
    float* dbook = s.g(pre + "quantize.embedding.weight");

    // ---------------- encoder, quantiser
    VqDrop de, dd;
    de.p = dd.p = p;
    de.seed = dd.seed = seed;
    de.step = dd.step = step;
    de.site = 0;
    dd.site = 1;
    VqEncSave E;
    float* z = s.f32((size_t)M * ZD);
    DIMX_TRY(vqenc_fwd(s, E, pre + "encoder.", x, pe_enc, de, B, T, z));
    float* Et = s.f32((size_t)ZD * d.vq_n_embed);
    float* ee = s.f32((size_t)d.vq_n_embed);
    int32_t* idx = idx_out ? idx_out : (int32_t*)s.take((size_t)M * 4);
    float* zst = s.f32((size_t)M * ZD);
    float* part_q = s.f32(kVqPart);
    float* part_l = s.f32(kVqPart);
    int nq = 1, nl = 1;
    TR(tr_vq_book_prep(book, Et, ee, st));
    TR(launch_vq_argmin(z, M, Et, ee, idx, nullptr, nullptr, st));
    TR(tr_vq_quant_fwd(z, book, idx, zst, part_q, M, &nq, st));
    // ---------------- decoder on the straight-through latent, L1 reconstruction, the four scalars
    VqDecSave V;
    float* pred = pred_out ? pred_out : s.f32((size_t)M * d.vq_in_dim);
    DIMX_TRY(vqdec_fwd(s, V, pre + "decoder.", nullptr, nullptr, pe_dec, B, T, pred, zst, &dd));
    float* dpred = s.f32((size_t)M * d.vq_in_dim);
    TR(tr_l1_loss(pred, x, dpred, part_l, (long)M * d.vq_in_dim, &nl, st));
    TR(tr_vq_finish(part_q, nq, part_l, nl, idx, M, beta, qw, loss_out, st));

    // ---------------- backward
    float* dz = s.f32((size_t)M * ZD);
    DIMX_TRY(vqdec_bwd(s, V, dpred, dz));
    const float inv = 2.0f / ((float)M * (float)ZD);
    TR(tr_vq_commit_bwd(z, book, idx, dz, M, qw * beta * inv, st));
    TR(tr_vq_book_grad(z, book, idx, dbook, M, qw * inv, st));
    DIMX_TRY(vqenc_bwd(s, E, dz));
    return step_finish(s, "train_vq", need);
}

int dimx_train_vq_num_params(dimx_handle h, int which) { return layout_num_params(h, vq_plan_kind(which)); }
int64_t dimx_train_vq_total(dimx_handle h, int which) { return layout_total(h, vq_plan_kind(which)); }
int dimx_train_vq_param_info(dimx_handle h, int which, int i, const char** name, int64_t* offset, int64_t* numel) {
    return layout_param_info(h, vq_plan_kind(which), i, name, offset, numel);
}

size_t dimx_train_vq_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    const int which = h->vqg[1].in_dim == 56 ? 1 : 0;   // both slots of the 56-d geometry size alike
    size_t need = 0;
    return vq_run(h, which, nullptr, nullptr, nullptr, B, T, 0.25f, 1.f, 0.f, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &need) == DIMX_OK
               ? need
               : 0;
}

int dimx_train_vq_forward_backward(dimx_handle h, int which, const float* params, float* grads, const float* x, int B, int T, float beta,
                                   float quant_loss_weight, float dropout_p, uint64_t dropout_seed, int64_t step, float* loss_out,
                                   float* pred_out, int32_t* idx_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && params && grads && x && loss_out && ws, DIMX_ERR_ARG, "train_vq: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)x % 16) == 0,
                 DIMX_ERR_ARG, "train_vq: workspace must be 256-byte aligned, arenas / input 16-byte aligned");
    DIMX_HIP(hipSetDevice(h->device));
    auto run = [&](void* w, size_t w_bytes, hipStream_t st, size_t* need) {
        return vq_run(h, which, params, grads, x, B, T, beta, quant_loss_weight, dropout_p, dropout_seed, (long)step, loss_out, pred_out, idx_out, w,
                      w_bytes, st, need);
    };
    DIMX_TRY(check_workspace("train_vq", ws_bytes, run));
    return run(ws, ws_bytes, (hipStream_t)stream, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- DIM-Speaker converter
// One forward + loss + backward pass of EmocaConverter's head (code/seq2seq_pretrain.py:801-842 under code/train_converter.py:
// 17-96).  Forward: lstm.hip's layers with the save switch, then the two GEMMs of dimx_mesh_head with the same arguments (the f32
// mode's mesh is that call's bit for bit).  The loss kernel leaves dY [M][Vp], Vp = V rounded up to 4 with zero pad columns (V =
// 70110 is no multiple of 4; the operand copies move 16-byte groups).  Backward: the V-wide Linear by hand (its input adjoint
// contracts over V in deterministic split-K slabs), the rest through lin_bwd.  grads == NULL: forward and
// loss only; mesh_out == NULL: the mesh stays in the workspace.
static int conv_run(dimx_handle h, const float* params, float* grads, const float* motion, const float* templ, const float* target,
                    const float* vert_w, int n_mouth, int B, int T, int flags, float* loss_out, float* mesh_out, void* ws, size_t ws_bytes,
                    hipStream_t st, size_t* need) {
    TrainPlan* plan;
    DIMX_TRY(plan_of(h, kPlanConv, &plan));
    DIMX_REQUIRE(B >= 1 && T >= 1 && T <= 65536 && (long)B * T <= (1l << 20), DIMX_ERR_ARG, "train_conv: B=%d T=%d out of range", B, T);
    const int V = h->d.mesh_dim, Vp = pad_to(V, 4), M = B * T;
    const bool want_bwd = grads != nullptr;
    Arena ar(ws, ws_bytes);
    Step s(h, plan, params, grads, &ar, st, h->at, B, T, T);
    const int Np = pad_to(V, s.bk), Mp = pad_to(M, s.bk);
    s.alloc_pool(want_bwd ? (size_t)8 * (ceil_div(M, 32) + 1) * 1536 + (size_t)(ceil_div(M, 32) + 1) * 768 + (size_t)kTrSlabs * Vp + 4096 : 64);

    LstmLayerP L0 = make_lstm_layer(s, 0), L1 = make_lstm_layer(s, 1);
    Lin l1 = make_lin(s, "vertice_map_reverse.0.weight", "vertice_map_reverse.0.bias");
    Lin l2 = make_lin(s, "vertice_map_reverse.2.weight", "vertice_map_reverse.2.bias");
    DIMX_TRY(prep_lin(s, l1));
    DIMX_TRY(prep_lin(s, l2));
    if (want_bwd) {
        DIMX_TRY(prep_lin(s, L1.ih[0]));   // their transposed copies carry dG back to the first layer's output
        DIMX_TRY(prep_lin(s, L1.ih[1]));
    }
    DIMX_TRY(flush_prep(s));

    // ---------------- forward
    const size_t scr_bytes = lstm_train_scratch_bytes(B, T, L0.In);
    void* scr = s.take(scr_bytes);
    float* y0 = s.f32((size_t)M * 768);
    float* y1 = s.f32((size_t)M * 768);
    const size_t n_save = (size_t)M * 2 * kLstmSave * 384;
    float* save0 = want_bwd ? s.f32(n_save) : nullptr;
    float* save1 = want_bwd ? s.f32(n_save) : nullptr;
    DIMX_TRY(lstm_layer_fwd(s, L0, motion, y0, save0, scr, scr_bytes, flags, h->cu_count, &h->lstm_faults));
    DIMX_TRY(lstm_layer_fwd(s, L1, y0, y1, save1, scr, scr_bytes, flags, h->cu_count, &h->lstm_faults));
    float* a1 = s.f32((size_t)M * 768);
    float* mesh = mesh_out ? mesh_out : s.f32((size_t)M * V);
    const Step::OpCopy *c1, *c2;
    DIMX_TRY(fwd_operands(s, y1, 768, M, 768, &c1));
    if (s.live()) {
        GemmArgs g;
        gemm_args_init(g);
        g.in_dtype = s.at;
        g.out_dtype = DIMX_F32;
        g.A = c1->o;
        g.lda = c1->Kp;
        g.W = l1.w_op;
        g.ldw = c1->Kp;
        g.M = M;
        g.N = 768;
        g.K = 768;
        g.bias = s.P + l1.b;
        g.act = ACT_LEAKY;
        gemm_set_plain_out(g, a1, 768);
        DIMX_TRY(launch_gemm(g, st));
    }
    DIMX_TRY(fwd_operands(s, a1, 768, M, 768, &c2));
    if (s.live()) {
        // N = mesh_dim is no multiple of any tile: the kernels clamp the W rows they load to N - 1 and store no column >= N
        // (dimx_mesh_head); the template row of the clip rides the epilogue
        GemmArgs g;
        gemm_args_init(g);
        g.in_dtype = s.at;
        g.out_dtype = DIMX_F32;
        g.A = c2->o;
        g.lda = c2->Kp;
        g.W = l2.w_op;
        g.ldw = c2->Kp;
        g.M = M;
        g.N = V;
        g.K = 768;
        g.bias = s.P + l2.b;
        g.rowT = T;
        if (templ) {
            g.rowadd = templ;
            g.ld_rowadd = V;
            g.rowadd_mode = 2;
            g.rowadd_off = 0;
        }
        gemm_set_plain_out(g, mesh, V);
        DIMX_TRY(launch_gemm(g, st));
    }
    float* lpart = s.f32((size_t)2 * tr_mesh_loss_parts(M, Vp));
    float* dY = want_bwd ? s.f32((size_t)M * Vp) : nullptr;
    TR(tr_mesh_loss(mesh, target, vert_w, n_mouth, M, V, Vp, dY, lpart, loss_out, st));

    if (want_bwd) {
        // ---------------- backward
        DIMX_TRY(s.zero_grads());
        float* da1 = s.f32((size_t)M * 768);
        {
            const size_t mark = ar.off;
            void* dyo = s.take((size_t)M * Np * s.es());
            void* dyT = s.take((size_t)Vp * Mp * s.es());
            TR(tr_prep_fused(s.at, 0, dY, Vp, nullptr, 0, nullptr, M, Vp, dyo, Np, dyT, Mp, nullptr, nullptr, st));
            // d bias [V]: Vp columns are summed (the pad columns of dY are zero) into the tensor's 16-byte pad inside the arena
            {
                float* part = s.pool_f32((size_t)kTrSlabs * Vp);
                int n = M < kTrSlabs * 8 ? 1 : kTrSlabs;
                if (s.live()) DIMX_TRY(tr_colsum_partial(dY, M, Vp, part, &n, st));
                DIMX_TRY(queue_fin(s, part, s.G + l2.b, Vp, n));
            }
            // dW2 [V][768] = dY^T . A1 (contraction over the zero-padded rows)
            DIMX_TRY(gemm_f32(s, dyT, Mp, c2->t, V, 768, Mp, s.G + l2.w, 768, nullptr, nullptr, 0));
            // dA1 [M][768] = dY . W2: K = V.  Split into slabs of plain stores, added in slab order (no float atomics)
            constexpr int kSplit = 8;
            float* slabs = s.f32((size_t)kSplit * M * 768);
            if (s.live()) {
                GemmArgs g;
                gemm_args_init(g);
                g.in_dtype = s.at;
                g.out_dtype = DIMX_F32;
                g.A = dyo;
                g.lda = Np;
                g.W = l2.wt_op;
                g.ldw = Np;
                g.M = M;
                g.N = 768;
                g.K = Np;
                g.out_slabs = 1;
                g.force_splitk = kSplit;
                g.slab_stride = (long)M * 768;
                gemm_set_plain_out(g, slabs, 768);
                const int sp = gemm_plan_splits(g);
                DIMX_REQUIRE(sp >= 1 && sp <= kSplit, DIMX_ERR_STATE, "train_conv: %d split-K slabs planned", sp);
                DIMX_TRY(launch_gemm(g, st));
                DIMX_TRY(tr_sum_slabs(slabs, sp, (long)M * 768, da1, (long)M * 768, st));
            }
            ar.off = mark;
        }
        TR(tr_lrelu_bwd_out(a1, da1, (long)M * 768, 0.2f, st));
        float* dy1 = s.f32((size_t)M * 768);
        DIMX_TRY(lin_bwd(s, l1, y1, 768, da1, 768, M, dy1, 768, false));
        float* dy0 = s.f32((size_t)M * 768);
        DIMX_TRY(lstm_layer_bwd(s, L1, y0, y1, save1, dy1, dy0, scr, scr_bytes, flags, h->cu_count, &h->lstm_faults));
        DIMX_TRY(lstm_layer_bwd(s, L0, motion, y0, save0, dy0, nullptr, scr, scr_bytes, flags, h->cu_count, &h->lstm_faults));
    }
    return step_finish(s, "train_conv", need);
}

int dimx_train_conv_num_params(dimx_handle h) { return layout_num_params(h, kPlanConv); }
int64_t dimx_train_conv_total(dimx_handle h) { return layout_total(h, kPlanConv); }
int dimx_train_conv_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel) {
    return layout_param_info(h, kPlanConv, i, name, offset, numel);
}

size_t dimx_train_conv_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    size_t need = 0;   // sized for a step with gradients that keeps the mesh in the workspace
    return conv_run(h, nullptr, present<float>(), nullptr, nullptr, nullptr, nullptr, 0, B, T, 0, nullptr, nullptr, nullptr, 0, nullptr, &need) == DIMX_OK
               ? need
               : 0;
}

int dimx_train_conv_forward_backward(dimx_handle h, const float* params, float* grads, const float* motion, const float* templ,
                                     const float* target, const float* vert_w, int n_mouth, int B, int T, int flags, float* loss_out,
                                     float* mesh_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "train_conv: null handle");
    DIMX_REQUIRE(h->d.mesh_dim > 0, DIMX_ERR_STATE, "train_conv: the handle was created without a mesh head (dimx_dims.mesh_dim = 0)");
    DIMX_REQUIRE(params && motion && target && loss_out && ws, DIMX_ERR_ARG, "train_conv: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)motion % 16) == 0,
                 DIMX_ERR_ARG, "train_conv: workspace must be 256-byte aligned, arenas / input 16-byte aligned");
    DIMX_REQUIRE(!vert_w || n_mouth >= 1, DIMX_ERR_ARG, "train_conv: vert_w needs n_mouth >= 1 (%d)", n_mouth);
    DIMX_HIP(hipSetDevice(h->device));
    auto run = [&](void* w, size_t w_bytes, hipStream_t st, size_t* need) {
        return conv_run(h, params, grads, motion, templ, target, vert_w, n_mouth, B, T, flags, loss_out, mesh_out, w, w_bytes, st, need);
    };
    DIMX_TRY(check_workspace("train_conv", ws_bytes, run));
    return run(ws, ws_bytes, (hipStream_t)stream, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- DIM-Speaker fine-tuning
// One forward + backward pass of SpeakerSLMFT.forward(mode='train') as the reference's speaker branch differentiates it
// (code/finetune_s2s_pretrain.py -> train_epoch_biwi, code/x_engine_pt.py:62-132, over code/seq2seq_pretrain.py:708-757): the
// context cat(speaker_embed[id] + patch_embed_dec_l, audio), the teacher-forced decoder with absolute positions and no key masking,
// cross entropy over the listener VQ-VAE's codes of the EMOCA stream, and the mean squared error of the decoded arg-max codes
// through the SPEAKER VQ-VAE's decoder, which it trains.  The mesh head is not part of the step: it only reports a metric and no
// gradient reaches it.  Launched kernel by kernel on the caller's stream (no side stream, no captured graph).
static int spk_run(dimx_handle h, const float* params, float* grads, const float* v_emoca, const float* v_audio, const uint8_t* mask,
                   const int32_t* z, const int32_t* speaker_ids, const float* codebook_s, const float* pe_s, int B, int T, float* loss_out,
                   float* logits_out, int32_t* idx_out, float* pred_out, void* ws, size_t ws_bytes, hipStream_t st, size_t* need) {
    TrainPlan* plan;
    DIMX_TRY(plan_of(h, kPlanSpk, &plan));
    const dimx_dims& d = h->d;
    DIMX_REQUIRE(B >= 1 && T >= 2 && T - 1 <= d.max_seq_len, DIMX_ERR_ARG, "train_spk: B=%d T=%d out of range (T - 1 <= %d)", B, T, d.max_seq_len);
    DIMX_REQUIRE(d.num_tokens == 512 && d.vq_in_dim == 56 && d.dim % 4 == 0 && d.dim_a % 4 == 0 && d.dim_a > 0, DIMX_ERR_ARG,
                 "train_spk: 512 codes, 56 coefficients, an audio stream");
    Arena ar(ws, ws_bytes);
    Step s(h, plan, params, grads, &ar, st, h->at, B, T, T - 1);
    const int C = d.dim, DD = d.dim + d.dim_a, F = std::max(DD * d.ff_mult, d.vq_inter), n = T - 1, BT = B * T;
    const int rows = plan->params[plan->index.at("speaker_embed.weight")].rows;
    s.reserve_part(F);
    {   // partial rows of the deferred column reductions
        const size_t n_ln_c = (size_t)(4 * d.vq_layers + 8), n_ln_dd = (size_t)(3 * d.dec_depth + 2);
        const size_t n_b = (size_t)(2 * d.dec_depth + 3 * d.vq_layers + 16);
        s.alloc_pool(n_ln_c * (kLnBlocks + 4) * (size_t)std::max(C, d.vq_hidden) + n_ln_dd * (kLnBlocks + 4) * (size_t)DD +
                     n_b * (size_t)std::max(kTrSlabs, ceil_div(BT, 32) + 1) * (size_t)F + 4096);
    }
    const bool live = ws != nullptr;
    DIMX_TRY(s.zero_grads());

    // ---------------- context, tokens
    float* ctx = s.f32((size_t)BT * DD);
    TR(tr_spk_context(s.p("speaker_embed.weight"), speaker_ids, s.p("patch_embed_dec_l"), v_audio, ctx, B, T, C, d.dim_a, st));
    int32_t* inp = (int32_t*)s.take((size_t)B * n * 4);
    int32_t* tgt = (int32_t*)s.take((size_t)B * n * 4);
    TR(launch_shift_tokens(z, inp, tgt, B, T, st));
    DecSave D;
    DIMX_TRY(dec_prepare(s, D, "decoder_joint.net.", d.dec_depth));
    DIMX_TRY(flush_prep(s));
    float* logits = logits_out ? logits_out : s.f32((size_t)B * n * d.num_tokens);
    DIMX_TRY(dec_fwd(s, D, inp, B, n, ctx, T, DD, mask, nullptr, true, logits));
    float* dlogits = s.f32((size_t)B * n * d.num_tokens);
    float* row_loss = s.f32((size_t)B * n);
    TR(tr_cross_entropy(logits, tgt, row_loss, dlogits, B * n, loss_out, st));
    // ---------------- decoded arg-max codes -> the speaker VQ-VAE's decoder -> mean squared error against v_emoca[:, 1:], padded frames included
    int32_t* idx = idx_out ? idx_out : (int32_t*)s.take((size_t)B * n * 4);
    TR(tr_argmax512(logits, idx, B, n, n, 0, st));
    float* pred = pred_out ? pred_out : s.f32((size_t)B * n * d.vq_in_dim);
    VqDecSave V;
    DIMX_TRY(vqdec_fwd(s, V, "speaker_vq.decoder.", idx, codebook_s, pe_s, B, n, pred));
    float* dpred = s.f32((size_t)B * n * d.vq_in_dim);
    float* mse_part = s.f32((size_t)kSpkMseParts);
    TR(tr_spk_mse(pred, v_emoca, dpred, B, T, d.vq_in_dim, mse_part, loss_out + 2, st));

    // ---------------- backward
    DIMX_TRY(vqdec_bwd(s, V, dpred));
    float* dctx = s.f32((size_t)BT * DD);
    if (live) DIMX_HIP(hipMemsetAsync(dctx, 0, (size_t)BT * DD * sizeof(float), st));
    DIMX_TRY(dec_bwd(s, D, dlogits, dctx));
    // the audio columns of the context have no parameters behind them; the first dim columns are the embedding row + the patch
    float* cpart = s.f32(tr_spk_context_bwd_floats(B, C));
    TR(tr_spk_context_bwd(dctx, speaker_ids, s.g("speaker_embed.weight"), s.g("patch_embed_dec_l"), cpart, B, T, C, DD, rows, st));
    return step_finish(s, "train_spk", need);
}

int dimx_train_spk_num_params(dimx_handle h) { return layout_num_params(h, kPlanSpk); }
int64_t dimx_train_spk_total(dimx_handle h) { return layout_total(h, kPlanSpk); }
int dimx_train_spk_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel) {
    return layout_param_info(h, kPlanSpk, i, name, offset, numel);
}

size_t dimx_train_spk_workspace_bytes(dimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 2) return 0;
    size_t need = 0;
    return spk_run(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, T, nullptr, nullptr, nullptr, nullptr,
                   nullptr, 0, nullptr, &need) == DIMX_OK ? need : 0;
}

int dimx_train_spk_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_emoca, const float* v_audio,
                                    const uint8_t* mask, const int32_t* z, const int32_t* speaker_ids, const float* codebook_s,
                                    const float* pe_s, int B, int T, float* loss_out, float* logits_out, int32_t* idx_out, float* pred_out,
                                    void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h && params && grads && v_emoca && v_audio && mask && z && codebook_s && pe_s && loss_out && ws, DIMX_ERR_ARG,
                 "train_spk: null argument");
    DIMX_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0 && ((uintptr_t)v_emoca % 16) == 0 &&
                     ((uintptr_t)v_audio % 16) == 0 && ((uintptr_t)codebook_s % 16) == 0 && ((uintptr_t)pe_s % 16) == 0 &&
                     ((uintptr_t)pred_out % 16) == 0,
                 DIMX_ERR_ARG, "train_spk: workspace must be 256-byte aligned, arenas / inputs / codebook / pe / pred_out 16-byte aligned");
    DIMX_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    auto run = [&](void* w, size_t w_bytes, hipStream_t on, size_t* need) {
        return spk_run(h, params, grads, v_emoca, v_audio, mask, z, speaker_ids, codebook_s, pe_s, B, T, loss_out, logits_out, idx_out, pred_out, w,
                       w_bytes, on, need);
    };
    DIMX_TRY(check_workspace("train_spk", ws_bytes, run));
    if (speaker_ids) {   // an id outside the table is refused here, on the host: the kernels index with it unchecked
        TrainPlan* plan;
        DIMX_TRY(plan_of(h, kPlanSpk, &plan));
        const int rows = plan->params[plan->index.at("speaker_embed.weight")].rows;
        std::vector<int32_t> ids((size_t)B);
        DIMX_HIP(hipMemcpyAsync(ids.data(), speaker_ids, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        DIMX_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b)
            DIMX_REQUIRE(ids[b] >= 0 && ids[b] < rows, DIMX_ERR_ARG, "train_spk: speaker_ids[%d] = %d is outside [0, %d)", b, ids[b], rows);
    }
    return run(ws, ws_bytes, st, nullptr);
}

int dimx_op_lstm_layer_bwd(int dtype, const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                           const float* const* b_ih, const float* const* b_hh, const float* dy, float* dx, float* const* dw_ih,
                           float* const* dw_hh, float* const* db, int flags, int* faults_out, void* stream) {
    DIMX_REQUIRE(dtype == DIMX_F32, DIMX_ERR_ARG, "lstm_layer_bwd: only the f32 recurrence is built (dtype %d)", dtype);
    DIMX_REQUIRE(H == 384 && B >= 1 && T >= 1 && In >= 4 && In % 4 == 0 && (long)B * T <= (1l << 20), DIMX_ERR_ARG,
                 "lstm_layer_bwd: bad shape (B=%d T=%d In=%d H=%d)", B, T, In, H);
    DIMX_REQUIRE(x && dy && w_ih && w_hh && b_ih && b_hh && dw_ih && dw_hh && db, DIMX_ERR_ARG, "lstm_layer_bwd: null argument");
    for (int d = 0; d < 2; ++d)
        DIMX_REQUIRE(w_ih[d] && w_hh[d] && b_ih[d] && b_hh[d] && dw_ih[d] && dw_hh[d] && db[d], DIMX_ERR_ARG,
                     "lstm_layer_bwd: null tensor (direction %d)", d);
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // a one-layer plan over temporary arenas: the step's own helpers do the rest
    TrainPlan plan;
    LstmLayerP L;
    L.In = In;
    for (int d = 0; d < 2; ++d) {
        const long sizes[4] = {1536l * In, 1536l * 384, 1536, 1536};
        long offs[4];
        for (int k = 0; k < 4; ++k) {
            offs[k] = plan.total;
            plan.total += (sizes[k] + 3) / 4 * 4;
        }
        L.ih[d].w = offs[0]; L.ih[d].N = 1536; L.ih[d].K = In; L.ih[d].b = offs[2];
        L.hh[d].w = offs[1]; L.hh[d].N = 1536; L.hh[d].K = 384; L.hh[d].b = offs[3];
    }
    const int M = B * T;
    int faults = 0;
    float *P = nullptr, *G = nullptr;
    void* ws = nullptr;
    auto run = [&](Arena& ar, size_t* need) -> int {
        Step s(nullptr, &plan, P, G, &ar, st, DIMX_F32, B, T, T);
        s.alloc_pool((size_t)4 * (ceil_div(M, 32) + 1) * 1536 + 4096);
        LstmLayerP Lr = L;
        DIMX_TRY(prep_lin(s, Lr.ih[0]));
        DIMX_TRY(prep_lin(s, Lr.ih[1]));
        DIMX_TRY(flush_prep(s));
        const size_t scr_bytes = lstm_train_scratch_bytes(B, T, In);
        void* scr = s.take(scr_bytes);
        float* y = s.f32((size_t)M * 768);
        float* save = s.f32((size_t)M * 2 * kLstmSave * 384);
        DIMX_TRY(lstm_layer_fwd(s, Lr, x, y, save, scr, scr_bytes, flags, cus, &faults));
        DIMX_TRY(lstm_layer_bwd(s, Lr, x, y, save, dy, dx, scr, scr_bytes, flags, cus, &faults));
        DIMX_TRY(flush_fin(s));
        if (need) *need = s.peak + 256;
        DIMX_REQUIRE(!s.pool_overflow && !ar.overflow, DIMX_ERR_WORKSPACE, "lstm_layer_bwd: scratch overflow");
        return DIMX_OK;
    };
    size_t need = 0;
    {
        Arena dry(nullptr, 0);
        DIMX_TRY(run(dry, &need));
    }
    hipError_t e = hipMalloc((void**)&P, (size_t)plan.total * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&G, (size_t)plan.total * 4);
    if (e == hipSuccess) e = hipMalloc(&ws, need);
    int rc = DIMX_OK;
    if (e == hipSuccess) {
        for (int d = 0; d < 2 && e == hipSuccess; ++d) {
            e = hipMemcpyAsync(P + L.ih[d].w, w_ih[d], (size_t)1536 * In * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(P + L.hh[d].w, w_hh[d], (size_t)1536 * 384 * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(P + L.ih[d].b, b_ih[d], 1536 * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(P + L.hh[d].b, b_hh[d], 1536 * 4, hipMemcpyDeviceToDevice, st);
        }
        if (e == hipSuccess) e = hipMemsetAsync(G, 0, (size_t)plan.total * 4, st);
        if (e == hipSuccess) {
            Arena ar(ws, need);
            rc = run(ar, nullptr);
        }
        for (int d = 0; d < 2 && e == hipSuccess && rc == DIMX_OK; ++d) {
            e = hipMemcpyAsync(dw_ih[d], G + L.ih[d].w, (size_t)1536 * In * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(dw_hh[d], G + L.hh[d].w, (size_t)1536 * 384 * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(db[d], G + L.ih[d].b, 1536 * 4, hipMemcpyDeviceToDevice, st);
        }
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (P) (void)hipFree(P);
    if (G) (void)hipFree(G);
    if (ws) (void)hipFree(ws);
    if (faults_out) *faults_out = faults;
    DIMX_TRY(rc);
    DIMX_HIP(e);
    DIMX_HIP(e2);
    return DIMX_OK;
}

}  // extern "C"
