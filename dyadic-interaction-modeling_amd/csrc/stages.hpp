// stages.hpp -- what generate.hip and ops.hip share with model.hip: the scratch layouts of a generate call and their planners,
// the argument checks and the sublayer helpers of the transformer stacks (all defined in model.hip unless noted).
#pragma once
#include "model.hpp"

namespace dimx {

enum { COMP_VQ0 = 1, COMP_VQ1 = 2, COMP_ENC = 4, COMP_DEC = 8, COMP_ALL = 15, COMP_MESH = 16 };   // packed components (ensure_packed)

static inline size_t es_of(const dimx_ctx* c) { return dtype_size(c->at); }
static inline int tpad(int T) { return (T + 7) / 8 * 8; }
// number of decoder positions: SLMFT feeds / generates T-1 tokens (code/seq2seq_pretrain.py:469,500);
// the legacy generator is teacher-forced on T-1 tokens but generates seq_len = T (code/seq2seq.py:256,300)
static inline int gen_steps(const dimx_ctx* c, int T) { return c->variant == 1 ? T : T - 1; }

int gemm_lin(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, GemmArgs& g);
bool qkv_row_v(int at, int D);
void set_attn_packed(AttnArgs& a, int dtype, const void* q, const void* k, const void* vt, void* o, int B, int H, int Lq, int Lk, int D,
                     int Tp_k, bool rowv = false);

// The buffers of a block, the base of every stack's scratch struct: the f32 residual stream h [M, C]; in the operand type the
// LayerNorm output y, q / k / v(t), the attention output o and the feed-forward hidden f; kw: the packed key-mask words of the
// prefill attention (AttnArgs.kwords)
struct BlockBufs {
    float* h;
    void *y, *q, *k, *vt, *o, *f;
    unsigned long long* kw = nullptr;   // the VQ stacks have none
    size_t kw_cap = 0;
};
int ff_sublayer(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& f1, const Linear& f2,
                const void* mlp, int act, int M, int C, hipStream_t st);
int self_attn_qkv(const dimx_ctx* c, const BlockBufs& b, const float* ln_g, const float* ln_b, const Linear& qkv, int B, int T, int C,
                  int heads, int D, AttnArgs& a, hipStream_t st);
int attn_out(const dimx_ctx* c, const BlockBufs& b, AttnArgs& a, const Linear& out, int C, hipStream_t st);
int cross_attn_sublayer(const dimx_ctx* c, const BlockBufs& b, const XAttn& x, AttnArgs& a, const uint8_t* ctx_mask, int C, hipStream_t st,
                        const float* v_rows = nullptr);

float* win_q_rows(const BlockBufs& b, int B, int n, int inner, size_t es);

struct CtxPersist {
    void* ck[8];
    void* cv[8];
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

// Prompted generation (dimx_generate_prompted): the prompt of a call and the teacher-forced scratch of its prefill.
// dimx_generate is the ld = Pmax = 1, step0 = 0 case.
struct GenPrompt {
    const int32_t* tok;  // [B, ld] the prompt's tokens, one row per CLIP
    int ld, Pmax;
    const int32_t* len;  // [B] prompt lengths (clamped to [step0 + 1, Pmax] by the sampler) or nullptr = Pmax
    int step0;           // P0 - 1: positions 0 .. step0 - 1 are prefilled, the first decode step is step0
    bool win = false;    // the prefill runs under the cross-attention window of the call's route (win_attn.hip)
};
struct PrefillScratch : BlockBufs {
    float* cvt;          // f32 mode: one layer's context V transposed to [B,H,64,Tp] (the f32 prefill attention reads V^T)
    int32_t* inp;
};
void plan_gen(const dimx_ctx* c, Arena& ar, int B, int T, GenScratch& s);
void plan_prefill(const dimx_ctx* c, Arena& ar, int B, int n0, int T, PrefillScratch& s);
size_t workspace_bytes_prompt(const dimx_ctx* c, int B, int T, int S, int P0);
Arena scratch_arena(const dimx_ctx* c, void* ws, size_t ws_bytes, int B, int T, CtxPersist* cp);
int check_common(dimx_handle h, int B, int T, void* ws, size_t ws_bytes, int need, int S = 1);

int check_sampler_filter(int kind, float a, float b);   // generate.hip

// out[M, ldo] = act(A . W^T + bias) (+ residual) as plain rows of out_dtype, and h[M, ld] += A . W^T (+ bias) in f32 (model.hip)
int linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, int out_dtype, void* out, int ldo, hipStream_t st,
           int act = ACT_NONE, const float* residual = nullptr);
int residual_linear(const dimx_ctx* c, const void* A, int lda, const Linear& L, int M, float* h, int ld, hipStream_t st);

// Append attention (stream_attn.hip): the c new rows of every clip against one encoder layer's K / V cache.  q / k / v: f32 rows
// [B * c, ld] (row b * c + i, head h at column h * 64); the k / v rows become cache rows [n0, n0 + c) in the cache type, query i
// attends over the rows 0 .. n0 + i; out [B * c, o_ld] in the cache type.
constexpr int kAppendMaxRows = 16;
struct AppendAttnArgs {
    int dtype;            // the cache's and the output's type
    const float *q, *k, *v;
    int ld;
    void *kcache, *vcache;   // [B, H, Tmax, 64]
    int Tmax;
    void* out;
    int o_ld;
    int B, H, n0, c;
    float scale;
};
int launch_append_attn(const AppendAttnArgs& a, hipStream_t s);

// Windowed cross attention for many queries (win_attn.hip): query row i of a clip (f32 rows [B * Lq, ld], head h at column h * 64)
// has position t0 + i and attends over the keys j < clamp(t0 + i + 2 + lookahead, 1, n_keys) that the clip's keep-mask keeps; K / V
// [B, H, Tp, 64] in the cache type (the generation layout); out [B * Lq, o_ld] in the cache type.
struct WinAttnArgs {
    int dtype;            // the caches' and the output's type
    const float* q;
    int ld;
    const void *kcache, *vcache;
    int Tp;
    void* out;
    int o_ld;
    int B, H, Lq, t0, n_keys, lookahead;
    const uint8_t* kmask;    // [B, kmask_ld] or nullptr
    int kmask_ld;
    float scale;
};
int launch_win_attn(const WinAttnArgs& a, hipStream_t s);

// A generation whose start and steps are driven across calls (generate.hip).  generate_impl opens one, runs all its steps and joins;
// a streaming session (stream.hip) keeps one open between its pushes.
struct GenRun;
struct GenSessionSpec {   // what a session asks of gen_open in place of the handle's settings
    int lookahead;        // the cross-attention window is on, with this look-ahead
    int n_keys;           // ... and this key bound (the cache length while the session is open)
    void* kv8_buf;        // dimx_stream_set_kv8: the session's FP8 cross K/V buffer (its pushes quantise the rows they append) or nullptr
    void* self_kv8_buf;   // ... and its FP8 self K/V buffer or nullptr
};

// FP8 K/V buffers (dimx_set_cross_kv8, dimx_set_self_kv8, dimx_stream_set_kv8; include/dimx.h has the layout): per layer K codes,
// V codes [B, H, Tp, 64] uint8, K scales, V scales [B, H, Tp] f32, each 256-byte aligned, layers in order.  B: the clips of the cross
// buffer, the R = B * S sequences of the self buffer.
struct Kv8Layer {
    uint8_t *kcodes, *vcodes;
    float *kscale, *vscale;
};
static inline size_t kv8_codes_bytes(const dimx_ctx* h, int B, int T) { return align_up((size_t)B * h->decg.heads * tpad(T) * 64, 256); }
static inline size_t kv8_scale_bytes(const dimx_ctx* h, int B, int T) { return align_up((size_t)B * h->decg.heads * tpad(T) * sizeof(float), 256); }
static inline size_t kv8_bytes(const dimx_ctx* h, int B, int T) {
    if (!h || h->variant != 0 || h->decg.dim_head != 64 || B < 1 || T < 2 || T > h->d.max_seq_len || tpad(T) > 2048) return 0;
    return (size_t)h->decg.depth * 2 * (kv8_codes_bytes(h, B, T) + kv8_scale_bytes(h, B, T));
}
static inline Kv8Layer kv8_layer_of(const dimx_ctx* h, void* buf, int B, int T, int l) {
    const size_t cb = kv8_codes_bytes(h, B, T), sb = kv8_scale_bytes(h, B, T);
    uint8_t* p = (uint8_t*)buf + (size_t)l * 2 * (cb + sb);
    return Kv8Layer{p, p + cb, (float*)(p + 2 * cb), (float*)(p + 2 * cb + sb)};
}
// start [B, ld_prompt]: the first P codes of every clip; P > 1: positions 0 .. P - 2 are prefilled under the session's window
GenRun* gen_run_new(const int32_t* start, const uint8_t* ctx_mask, int B, int T, float temperature, int top_k, const float* noise,
                    uint64_t seed, int32_t* tokens, float* logits_out, void* ws, size_t ws_bytes, hipStream_t st, int ld_prompt = 1,
                    int P = 1);
void gen_run_free(GenRun* r);
int gen_open(dimx_handle h, GenRun& run, bool keep_prefill, bool prefill_only, const GenSessionSpec* sess);
int gen_run_steps(dimx_handle h, GenRun& run, int nsteps);          // the next nsteps steps of every group
void gen_run_set_keys(GenRun& run, int n_keys, hipStream_t st);     // the cross attention's key bound and stream of the steps to come

// no stage that rebuilds the context or generates may run on a handle whose streaming session is open
#define DIMX_NO_SESSION(h, what) \
    DIMX_REQUIRE(!(h) || !(h)->stream_sess, DIMX_ERR_STATE, what ": a streaming session is open on this handle (dimx_stream_end / dimx_stream_abort first)")

}  // namespace dimx
