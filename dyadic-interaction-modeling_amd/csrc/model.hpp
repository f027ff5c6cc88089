// model.hpp -- handle layout of libdimx_hip: packed device weights + stage planners.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.hpp"

namespace dimx {

struct Linear {
    void* w = nullptr;  // [N][Kp] in the handle's operand type (bf16 / f32)
    const float* bias = nullptr;
    int N = 0, K = 0, Kp = 0;
    // round 6, f32 parity mode, decoder projections: W as three bf16 planes [3][N][Kp] whose sum is W exactly -- the decode-sized
    // GEMMs then run on the bf16 matrix cores, f32-equivalent (gemm_x3.hip)
    void* w3 = nullptr;
};

struct VQBlock {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    Linear qkv, out, l1, l2;
    const void* mlp = nullptr;   // bf16 mode, hidden 384: the MLP sublayer's weights as mlp_fused.hip chunk images
};

struct VQNet {
    Linear vm, conv, le, post;      // encoder
    VQBlock enc[8];
    Linear pre, dconv, dle, rev;    // decoder
    VQBlock dec[8];
    const float* pe_enc = nullptr;  // [5000][hidden]
    const float* pe_dec = nullptr;
    const float* E = nullptr;       // [n_embed][zdim]
    const float* Et = nullptr;      // [zdim][n_embed]
    const float* ee = nullptr;      // [n_embed]
};

struct XAttn {
    const float* ln_g;
    Linear qkv;  // self: fused [3*inner][dim]; cross: q only [inner][dim]
    Linear kv;   // cross: fused [2*inner][dim]
    Linear out;
    // decoder cross attention, bf16 mode: q projection with the pre-norm's gamma folded in (W' = gamma o W) and the row
    // sums of W' -- the deferred-LayerNorm form of the decode step (ChainArgs.defer)
    Linear q_ln;
    const float* q_ln_colsum = nullptr;
};
struct XFF {
    const float* ln_g;
    Linear f1, f2;
    Linear f1_ln;  // decoder, bf16 mode: gamma-scaled first projection + row sums (GemmArgs.ln_stats)
    const float* f1_ln_colsum = nullptr;
    const void* mlp = nullptr;   // encoders, bf16 mode, dim 384: mlp_fused.hip chunk images
};
struct XEnc {
    Linear proj_in;
    const float* pos_emb = nullptr;  // [max_seq_len][dim]
    XAttn attn[8];
    XFF ff[8];
    const float* final_g = nullptr;
};
struct XDec {
    const float* tok_emb = nullptr;  // [num_tokens][dec_dim]
    const float* pos_emb = nullptr;  // [max_seq_len][dec_dim] (legacy decoder: use_abs_pos_emb=True)
    XAttn self_[8], cross[8];
    XFF ff[8];
    const float* final_g = nullptr;
    Linear logits;
    Linear cross_kv_all;  // [depth * 2 * inner][Kp]: every layer's [Wk; Wv] stacked (cross[l].kv are views into it)
};

// DIM-Speaker converter head (EmocaConverter.vertice_map_reverse_lstm + vertice_map_reverse): the LSTM tensors as torch keeps
// them (f32 in both numeric modes, lstm.hip), the two Linear layers packed like every other one
struct MeshHead {
    const float *w_ih[2][2], *w_hh[2][2], *b_ih[2][2], *b_hh[2][2];   // [layer][direction]
    Linear l1, l2;
};

// geometry of the three network families of a handle (variant 0 = SLMFT, 1 = legacy ListenerGenerator,
// 2 = SLM pre-training model: SLMFT's dims, bidirectional encoders + encoder_l, decoder with abs. pos. embedding)
struct VQGeom {
    int in_dim, in_pad, hidden, heads, inter, layers, out_dim, fqn, zdim, n_embed;
    bool has_decoder;
};
struct EncGeom {
    int dim_in, in_pad, dim, heads, dim_head, depth, ff_mult, causal;
};
struct DecGeom {
    int dim, heads, dim_head, depth, ff_mult, abs_pos, num_tokens, ctx_dim;
};

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

// simple bump planner over the caller's workspace; base == nullptr -> dry run (size only)
struct Arena {
    unsigned char* base;
    size_t off;
    size_t cap;
    bool overflow;
    Arena(void* b, size_t c) : base((unsigned char*)b), off(0), cap(c), overflow(false) {}
    void* take(size_t bytes) {
        off = align_up(off, 256);
        void* p = base ? base + off : nullptr;
        off += bytes;
        if (base && off > cap) overflow = true;
        return p;
    }
};

// Beam search (dimx_generate_beam): what the step's two beam kernels read and write beside the generation's own buffers
struct BeamCall {
    double* cum = nullptr;         // [B*W] running scores
    int32_t* parent = nullptr;     // [B*W] the last selection's parent beams
    int32_t* backptr = nullptr;    // [B*W, n] or nullptr
    const int32_t* lens = nullptr; // [B] or nullptr: clip lengths (columns at or past len - (T - n) are frozen)
    bool operator==(const BeamCall& o) const { return cum == o.cum && parent == o.parent && backptr == o.backptr && lens == o.lens; }
};

// What the decode steps of one generate call launch (generate.hip resolve_route): decided once per call, read by the step, the
// key-word packing, the table counters, the graph key and the chain flag check after the call.
struct StepRoute {
    bool chain = false;            // the XCD-local chain kernels replace the projection / LayerNorm triples
    bool defer = false;            // ... in their deferred-LayerNorm form
    bool layer_kernel[8] = {};     // layer l's attention half is the one layer-kernel launch
    bool logits_chain = false;     // chain && no to_logits.bias: the final LayerNorm + logits is a chain site too
    bool multi_tr = false;         // several samples per clip, bf16: cross attention on the matrix cores (per-op branch, no window)
    bool win = false;              // online generation: the cross attention's key count follows the step counter
    int lookahead = 0;
    bool kv8 = false;              // the cross attention reads the FP8 copy of the context K/V (dimx_set_cross_kv8; decode_attn_kv8.hip)
    bool kv8_samples = false;      // kv8 with several samples per clip: the multi-query launch over the codes (dimx_set_cross_kv8_samples)
    bool self_kv8 = false;         // the self attention appends to and reads FP8 self caches (dimx_set_self_kv8; decode_attn_kv8.hip)
    const float* qkv0 = nullptr;   // the first layer's q/k/v table or nullptr
    const void* kv0 = nullptr;     // the first layer's K / V table (the bf16 image, or the q/k/v table itself in the f32 mode): its self
                                   // attention reads rows of it through the token history and keeps no cache; nullptr = the cache
    bool sample_head = false;      // the sampler is the first stage of layer 0's launch (chain.hip HEAD): a step is {head + layer 0,
                                   // ..., logits}, its first step skips the head, and one plain sampler launch ends the call
    const BeamCall* beam = nullptr;
    bool fault_inject = false;     // test hook: the chain kernels are launched with fault = 1
    int G = 1, S = 1;              // clip groups, samples per clip
    bool guided = false;           // classifier-free guidance: rows [0, R / 2) conditional, [R / 2, R) unconditional (no cross sublayer);
                                   // the per-op step, and the guided sampler ends it
};

// Everything a captured step bakes in: the call's pointers and shapes, and the route.  Equality is memberwise.
struct GraphKey {
    void* ws;
    int B, T, top_k;
    const void *noise, *start, *mask, *tokens, *logits_out;
    int G, S;
    bool chain, defer, logits_chain, multi_tr, fault_inject;
    unsigned layer_kernel;    // bit l = StepRoute::layer_kernel[l]
    const void *qkv0, *kv0;
    bool sample_head;
    const void* prompt_len;   // prompted generation: the sampler's other prompt arguments (`start` is the prompt itself)
    int ld_prompt, Pmax;
    int filter_kind;          // the sampler kernel's instantiation; the filter's real-valued parameters live in device memory
    BeamCall beam;            // beam search: the selection / reorder kernels' buffers, all null = the sampler ends the step
    int xwin_on, xwin_lookahead;   // online generation (dimx_set_cross_lookahead): other launches, and the look-ahead is a kernel argument
    bool guided;                   // the guided step's launches; the scale lives in device memory
    const void* branch_out;        // ... and its optional dump of both branches' logits
    const void* kv8;               // the FP8 cross K/V buffer the cross attention's launches read (dimx_set_cross_kv8), nullptr = off
    bool kv8_samples;              // dimx_set_cross_kv8_samples: the multi-query launch over the codes
    const void* self_kv8;          // the FP8 self K/V buffer the self attention's launches append to and read (dimx_set_self_kv8), nullptr = off
    bool beam_reorder_kv8;         // a beam step ends in launch_beam_reorder_kv8 on that buffer's planes, not in launch_beam_reorder on the caches
    bool operator==(const GraphKey& o) const {
        return ws == o.ws && B == o.B && T == o.T && top_k == o.top_k && noise == o.noise && start == o.start && mask == o.mask &&
               tokens == o.tokens && logits_out == o.logits_out && G == o.G && S == o.S && chain == o.chain && defer == o.defer &&
               logits_chain == o.logits_chain && multi_tr == o.multi_tr && fault_inject == o.fault_inject &&
               layer_kernel == o.layer_kernel && qkv0 == o.qkv0 && kv0 == o.kv0 && sample_head == o.sample_head && prompt_len == o.prompt_len &&
               ld_prompt == o.ld_prompt && Pmax == o.Pmax && filter_kind == o.filter_kind && beam == o.beam && xwin_on == o.xwin_on &&
               xwin_lookahead == o.xwin_lookahead && guided == o.guided && branch_out == o.branch_out && kv8 == o.kv8 && kv8_samples == o.kv8_samples && self_kv8 == o.self_kv8 &&
               beam_reorder_kv8 == o.beam_reorder_kv8;
    }
};

}  // namespace dimx

namespace dimx {
int vq_pe_buffers(dimx_ctx* c, int which, const float** pe_enc, const float** pe_dec);   // model.hip
void train_forget(dimx_ctx* h);   // train.hip: drop the training plan cached for a handle (dimx_destroy)
void stream_forget(dimx_ctx* h);  // stream.hip: drop the handle's streaming session (dimx_destroy)
}

struct dimx_ctx {
    int device = 0;
    dimx_dims d;
    int variant = 0;
    dimx::VQGeom vqg[2];
    dimx::EncGeom encg[2];  // SLMFT: encoder_s, encoder_joint; legacy: generator.encoder only
    dimx::DecGeom decg;
    int mode = 0;
    int at = DIMX_F32;  // operand storage type of GEMM/attention inputs
    std::map<std::string, dimx::HostTensor> host;
    std::vector<std::string> required;
    int packed_mask = 0;  // COMP_* bits of the components whose packed device copies are current
    std::vector<void*> dev_allocs;
    dimx::VQNet vq[2];  // 0 speaker, 1 listener
    dimx::XEnc enc_s, enc_joint, enc_l;  // enc_l: SLM pre-training variant only
    dimx::XDec dec;
    const float *patch_s = nullptr, *patch_dec_s = nullptr, *norm_s_g = nullptr, *norm_s_b = nullptr;
    const float *patch_l = nullptr, *patch_dec_l = nullptr, *norm_l_g = nullptr, *norm_l_b = nullptr;  // SLM
    const float *norm_j_g = nullptr, *norm_j_b = nullptr;                                              // SLM `norm`
    // encode_ctx -> decode hand-off
    bool ctx_ready = false;
    int ctx_B = 0, ctx_T = 0, ctx_for_generate = 0;
    void* ctx_ws = nullptr;
    // generate step graph
    static constexpr int kMaxGroups = 8;
    hipGraphExec_t graph_exec[kMaxGroups] = {};
    hipGraphExec_t graph_multi[kMaxGroups] = {};  // the same step captured graph_unroll times back to back
    int graph_unroll = 16;                        // steps per graph_multi launch
    // prefill (VQ encode, encoders + context, VQ decode) as clip groups on several streams (round 5, bf16 mode; DIMX_PREFILL_GROUPS)
    static constexpr int kPreGroups = 4;
    int prefill_groups = 0;             // 0 = automatic, 1 = one batch on the caller's stream, 2..4
    hipStream_t pre_stream[kPreGroups - 1] = {};
    hipEvent_t pre_fork = nullptr, pre_join[kPreGroups - 1] = {};
    hipStream_t grp_stream[kMaxGroups] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxGroups] = {};
    int gen_groups = 1;  // independent clip groups decoded concurrently on separate streams (DIMX_GEN_GROUPS;
                         // measured on MI355X: 1 is fastest, concurrent step graphs do not overlap usefully)
    hipStream_t cap_stream = nullptr;  // capture happens here (the caller's stream may be the null stream)
    dimx::GraphKey graph_key{};
    bool graph_valid = false;
    int use_graph = 1;
    // XCD-local chain kernels of the decode step (chain.hip): bf16 mode, one sample per clip, 256-CU device
    int use_chain = 1;                  // DIMX_NO_CHAIN=1 keeps the one-kernel-per-op step
    int cu_count = 0;
    float* chain_stats_dev = nullptr;   // [8][32][32][2] partial row sums of the deferred-LayerNorm chain kernels
    int defer_ln = 1;                   // 0 (after a row failed the deferred form's range check) keeps the row-phase LayerNorm inside the chain kernels
    unsigned long long* layer_prof_dev = nullptr;  // DIMX_LAYER_PROF=1 (tuning): [8 layers][256 blocks][16] phase stamps of xcd_layer_kernel
    int multi_tr = 1;                   // round 6: several samples per clip (best-of-N), bf16: the decode cross attention on the MFMA prefill
                                        // attention kernel (attention_tr.hip) instead of the VALU multi-query kernel (DIMX_NO_MULTI_TR=1: the latter)
    int use_layer_chain = 1;            // DIMX_NO_LAYER_CHAIN=1 keeps the attention half of a layer as four launches (round 5)
    unsigned* chain_err_dev = nullptr;  // bit 0: two blocks claimed one (XCD, CU slot), bit 1: a group barrier timed out
    unsigned* chain_err_host = nullptr; // pinned copy, refreshed at the end of every generate call
    hipEvent_t chain_err_ev = nullptr;
    int chain_faults = 0;               // generate calls whose chain kernels reported a fault and that were re-run without them
    int chain_fault_inject = 0;         // test hook: that many of the next generate calls launch the chain kernels with fault = 1
    // The first decoder layer's q/k/v as a table over the token ids (decoders without positional embedding: the layer's input is
    // LayerNorm(token_emb[tok]), one of num_tokens rows): built with the decode step's own kernels at the step's row count, read by
    // the sampler and the start-token step instead of a projection GEMM per token (DIMX_NO_QKV0_TABLE=1: the GEMM, for A/B runs)
    int use_qkv0_table = 1;
    float* qkv0_table = nullptr;        // [num_tokens][3 * heads * dim_head] f32, slabs already added in slab order
    int qkv0_M = 0, qkv0_at = -1;       // rows per projection launch and operand type the table was built at
    uint64_t qkv0_epoch = 0;            // dec_epoch the table was built at (0 = never)
    uint64_t dec_epoch = 1;             // bumped whenever the decoder's device weights are released or packed
    int qkv0_builds = 0;
    // The first layer's self attention in its table form (decode_attn_body.hpp, TAB): that layer's cached K / V of a position are
    // columns [inner, 3 * inner) of the table row of the position's input token, so the step reads them from the table through a
    // per-row token history instead of appending to and streaming a per-clip cache (DIMX_NO_KV0_TABLE=1: the cache, for A/B runs).
    // bf16 mode reads kv0_image, the table's K / V columns in the operand type, built and invalidated with the table; the f32 mode
    // reads the table itself.  Generations without beam search and without a prompt prefill only.
    int use_kv0_table = 1;
    void* kv0_image = nullptr;          // [num_tokens][2 * heads * dim_head] bf16
    int kv0_generations = 0;            // generate calls (regenerations included) that ran the table form
    // The sampler as the first stage of layer 0's launch (chain.hip, xcd_layer_kernel HEAD): one dependent launch less per token on
    // the route of the headline (resolve_route has the gate).  DIMX_NO_SAMPLE_HEAD=1: the sampler launch, for A/B runs.
    int use_sample_head = 1;
    int sample_head_generations = 0;    // generate calls (regenerations included) whose steps ran the head
    // sampler generator window of a sharded batch (dimx_set_shard): this handle generates clips
    // [shard_row_off, shard_row_off + B) of shard_rows_total (0 = the call's own B)
    int shard_row_off = 0, shard_rows_total = 0;
    // sampler filter of generate (dimx_set_sampler_filter): kind 0 = the call's top_k
    int filter_kind = 0;
    float filter_a = 0.f, filter_b = 0.f;
    // online generation (dimx_set_cross_lookahead): decode step t's cross attention sees the context rows
    // j < clamp(t + 2 + lookahead, 1, T) only; off = every row, as the reference generates
    int xwin_on = 0, xwin_lookahead = 0;
    // FP8 cross K/V (dimx_set_cross_kv8): the caller's buffer the generation quantises every layer's context K / V into and the
    // decode steps' cross attention reads; nullptr = off
    void* kv8_buf = nullptr;
    size_t kv8_bytes = 0;
    int kv8_samples_on = 0;   // dimx_set_cross_kv8_samples: generations with n_samples > 1 take the buffer too (decode_attn_mq_kv8_kernel)
    // FP8 self-attention K/V (dimx_set_self_kv8): the caller's buffer every decode step appends its quantised k / v row to and the
    // self attention reads, rows = sequences (clips x samples); nullptr = off
    void* self_kv8_buf = nullptr;
    size_t self_kv8_bytes = 0;
    // dimx_set_beam_kv8: dimx_generate_beam takes the two buffers above (the cross one through the multi-query launch, the self one
    // reordered by beam_reorder_kv8_kernel); off = it refuses them
    int beam_kv8_on = 0;
    // online fine-tuning (dimx_set_train_lookahead): the same visibility in the decoder cross attention of
    // dimx_train_forward_backward, query row i = step t.  Independent of xwin_*.
    int twin_on = 0, twin_lookahead = 0;
    // condition dropout of the SLMFT training step (dimx_set_train_cond_keep): [B] keep flags in device memory, read by the step's
    // kernels (a new draw replays the captured step); nullptr = off
    const uint8_t* tcond_keep = nullptr;
    // streaming session (stream.hip, dimx_stream_begin .. dimx_stream_end / dimx_stream_abort): one per handle; while it is
    // open the stages that rebuild the context or generate return DIMX_ERR_STATE
    void* stream_sess = nullptr;
    // FP8 K/V for sessions (dimx_stream_set_kv8): the caller's cross and self buffers the next session begins read; nullptr = that
    // route off.  Independent of kv8_buf / self_kv8_buf above: sessions ignore those, dimx_generate* ignores these.
    void* stream_kv8_buf = nullptr;
    size_t stream_kv8_bytes = 0;
    void* stream_self_kv8_buf = nullptr;
    size_t stream_self_kv8_bytes = 0;
    dimx::MeshHead mesh;              // handles created with dimx_dims.mesh_dim > 0
    int lstm_faults = 0;                // LSTM layers whose group kernel reported a fault and that were rerun on the safe path
    int spk_embed_rows = 0;             // rows of speaker_embed.weight as last loaded (the host applies it in inference; the
                                        // DIM-Speaker training step lays its arena out by it); 0 = never loaded
};
