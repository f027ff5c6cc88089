// generate.hip -- autoregressive generation of libdimx_hip: the decode step as named stages, its route, the step graphs and the
// three generate entry points (dimx_generate, dimx_generate_prompted, dimx_generate_beam).
//
// A generate call is: plan, route, parameters, tables, prefill, start, steps, join (generate_impl).  What the step launches is
// decided once per call (resolve_route); gen_step and everything else that depends on that decision read the StepRoute.
#include <stdlib.h>

#include "stages.hpp"

namespace dimx {

static void chain_desc(ChainGemmDesc& d, const Linear& L) { d.W = L.w; d.N = L.N; d.K = L.K; d.ldw = L.Kp; }

// The chain kernels run when: bf16 operands, one sample per clip, a single clip group, <= 256 rows, a 256-CU device on
// which the placement probe passed, and every launch site's LDS plan fits.
static bool gen_use_chain(dimx_handle h, int B, int S) {
    if (!h->use_chain || h->at != DIMX_BF16 || S != 1 || h->gen_groups > 1 || !h->chain_err_dev) return false;
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

// The table's storage, and that of its K / V columns in the operand type for the first layer's self attention in the table form
// (bf16 mode; the f32 mode reads the table).  The route holds these pointers, so they exist before it is resolved; the contents
// are qkv0_table_build's.
static int qkv0_table_alloc(dimx_handle h) {
    const int V = h->decg.num_tokens, N = h->dec.self_[0].qkv.N;
    if (!h->qkv0_table) {
        DIMX_HIP(hipMalloc((void**)&h->qkv0_table, (size_t)V * N * sizeof(float)));
        h->qkv0_epoch = 0;
        h->graph_valid = false;
    }
    if (h->use_kv0_table && h->at == DIMX_BF16 && !h->kv0_image) {
        DIMX_HIP(hipMalloc(&h->kv0_image, (size_t)V * 2 * (N / 3) * sizeof(bf16)));
        h->qkv0_epoch = 0;
        h->graph_valid = false;
    }
    return DIMX_OK;
}

// The table for projection launches of M rows: ceil(num_tokens / M) rounds of {embedding rows of the next M ids, the first layer's
// pre-norm, the step's own q/k/v projection at M rows, slabs added in order into the table rows}; the last round (and M >
// num_tokens) is padded by repeating the last id.  M is the step's M because the split count, hence the summation order,
// follows from it (gemm_plan_splits).  Runs on the generation scratch, which is free before the first step; s.step must read step0.
static int qkv0_table_build(dimx_handle h, const GenScratch& s, int M, hipStream_t st, int step0 = 0) {
    const DecGeom& dg = h->decg;
    const int DD = dg.dim, V = dg.num_tokens, N = h->dec.self_[0].qkv.N;
    if (h->qkv0_M == M && h->qkv0_at == h->at && h->qkv0_epoch == h->dec_epoch) return DIMX_OK;
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
    // the K / V image: same key and invalidation as the table, because it is rebuilt whenever the table is
    if (h->kv0_image) DIMX_TRY(launch_kv0_image(h->qkv0_table, N, V, N / 3, 2 * (N / 3), h->kv0_image, st));
    h->qkv0_M = M;
    h->qkv0_at = h->at;
    h->qkv0_epoch = h->dec_epoch;
    ++h->qkv0_builds;
    return DIMX_OK;
}

// what a generate call was asked for; the public entry points fill it after their own argument checks
struct GenRequest {
    GenPrompt pr;
    const uint8_t* ctx_mask;
    int B, T, S;   // clips, frames, samples per clip (the beam width of a beam search)
    float temperature;
    int top_k;
    const float* noise;
    uint64_t seed;
    int32_t* tokens;
    float* logits_out;
    void* ws;
    size_t ws_bytes;
    hipStream_t st;
    const BeamCall* beam;   // beam search: the selection and the cache reorder end the step in the sampler's place; nullptr = the sampler
    // classifier-free guidance (dimx_generate_guided): the step runs 2B rows, the guided sampler ends it; tokens / logits_out hold B rows
    bool guided = false;
    float scale = 1.f;
    float* branch_out = nullptr;   // [2, B, n, V] or nullptr
};

// what every step of one generate call shares (built once in generate_impl)
struct GenCall {
    const GenRequest& req;
    const CtxPersist& cp;
    const GenScratch& s;
    int R;       // sequences of the batch: clips x samples
    int top_k;   // the request's k, 0 under a sampler filter of another kind
    // the FP8 K/V buffers of the call or nullptr (gen_open): the handle's (dimx_set_cross_kv8, dimx_set_self_kv8) for an offline
    // call, the session's own (dimx_stream_set_kv8) for a session's
    void* kv8_buf = nullptr;
    void* self_kv8_buf = nullptr;
};

// One clip group's view of a call: rows [row0, row0 + B) of the gc->R sequences.  `s` holds the group's slices of every per-row
// buffer (the slab strides stay the batch's); start / mask / cross K/V are per clip.  Built once per group and call (step_ctx).
struct StepCtx {
    dimx_handle h;
    const GenCall* gc;
    const StepRoute* r;
    hipStream_t st;
    int row0, B, grp;
    int clip0, nclip;   // with S samples per clip, rows are samples (row = clip * S + sample)
    int Bc;             // rows that run the cross sublayer: B, or the conditional half [0, B / 2) of a guided step
    int T, S, DD, heads, D, inner, V, n, Tp;
    int n_keys;   // the cross attention's key bound: T, or what a streaming session sets (gen_run_set_keys)
    size_t es;
    float scale, pos_scale;
    const float* pos;   // the legacy decoder's positional embedding or nullptr
    GenScratch s;
    const void *ck[8], *cv[8];   // the group's clips in the context K / V of every layer
    Kv8Layer kv8[8];             // route kv8: ... and in their FP8 copy
    Kv8Layer skv8[8];            // route self_kv8: the group's rows in the FP8 self caches of every layer
    const int32_t *start, *forced, *forced_len;
    const uint8_t* ctx_mask;
    int32_t* tokens;
    float* logits_out;
};

static StepCtx step_ctx(dimx_handle h, const GenCall& gc, const StepRoute& r, int row0, int B, int grp, hipStream_t st) {
    const GenRequest& q = gc.req;
    const GenScratch& s0 = gc.s;
    const GenPrompt& pr = q.pr;
    const DecGeom& dg = h->decg;
    StepCtx c;
    c.h = h; c.gc = &gc; c.r = &r; c.st = st;
    c.row0 = row0; c.B = B; c.grp = grp;
    c.T = q.T; c.S = q.S;
    c.clip0 = row0 / c.S; c.nclip = r.guided ? B / 2 : B / c.S;
    c.Bc = r.guided ? B / 2 : B;
    c.DD = dg.dim; c.heads = dg.heads; c.D = dg.dim_head; c.inner = c.heads * c.D;
    c.V = dg.num_tokens; c.n = gen_steps(h, c.T); c.Tp = tpad(c.T); c.n_keys = c.T;
    c.es = es_of(h); c.scale = 1.0f / sqrtf((float)c.D);
    c.pos = dg.abs_pos ? h->dec.pos_emb : nullptr; c.pos_scale = 1.0f / sqrtf((float)c.DD);
    const int T = c.T, DD = c.DD, heads = c.heads, inner = c.inner;
    const size_t es = c.es;
    auto boff = [&](void* p, size_t per_row_bytes) { return (void*)((unsigned char*)p + (size_t)row0 * per_row_bytes); };
    c.s = s0;
    for (int l = 0; l < dg.depth; ++l) {
        c.s.sk[l] = boff(s0.sk[l], (size_t)heads * T * 64 * es);
        c.s.sv[l] = boff(s0.sv[l], (size_t)heads * T * 64 * es);
        c.ck[l] = (unsigned char*)gc.cp.ck[l] + (size_t)c.clip0 * heads * c.Tp * 64 * es;
        c.cv[l] = (unsigned char*)gc.cp.cv[l] + (size_t)c.clip0 * heads * c.Tp * 64 * es;
        c.kv8[l] = Kv8Layer{};
        if (r.kv8) {
            const size_t row0 = (size_t)c.clip0 * heads * c.Tp;
            const Kv8Layer all = kv8_layer_of(h, gc.kv8_buf, q.B, T, l);
            c.kv8[l] = Kv8Layer{all.kcodes + row0 * 64, all.vcodes + row0 * 64, all.kscale + row0, all.vscale + row0};
        }
        c.skv8[l] = Kv8Layer{};
        if (r.self_kv8) {
            const size_t at = (size_t)row0 * heads * c.Tp;
            const Kv8Layer all = kv8_layer_of(h, gc.self_kv8_buf, gc.R, T, l);
            c.skv8[l] = Kv8Layer{all.kcodes + at * 64, all.vcodes + at * 64, all.kscale + at, all.vscale + at};
        }
    }
    c.s.x = s0.x + (size_t)row0 * DD;
    c.s.y = boff(s0.y, DD * es);
    c.s.qkv = s0.qkv + (size_t)row0 * 3 * inner;
    c.s.qc = s0.qc + (size_t)row0 * inner;
    c.s.xr = s0.xr + (size_t)row0 * DD;
    c.s.o = boff(s0.o, inner * es);
    c.s.f = boff(s0.f, (size_t)DD * dg.ff_mult * es);
    c.s.logits = s0.logits + (size_t)row0 * c.V;
    c.s.step = s0.step + 16 * grp;
    c.s.hist = s0.hist + (size_t)row0 * T;
    c.s.qcb = boff(s0.qcb, inner * es);
    c.s.kw = s0.kw + (size_t)c.clip0 * ((T + 63) / 64);
    c.s.kw_cap = s0.kw_cap - (size_t)c.clip0 * ((T + 63) / 64);
    // the first step's input is column step0 of the prompt; later steps inside a clip's prompt are forced by the sampler
    c.start = pr.tok + (size_t)c.clip0 * pr.ld + pr.step0;
    c.forced = pr.Pmax > 1 ? pr.tok + (size_t)c.clip0 * pr.ld : nullptr;
    c.forced_len = pr.len ? pr.len + c.clip0 : nullptr;
    c.ctx_mask = q.ctx_mask + (size_t)c.clip0 * T;
    c.tokens = q.tokens + (size_t)row0 * c.n;
    c.logits_out = q.logits_out ? q.logits_out + (size_t)row0 * c.n * c.V : nullptr;
    return c;
}

// Step 0's input = embedding of the start token (later steps: fused into the sampler).
// round 4: the sampler that writes the next step's embedding row also writes the first layer's pre-norm of it, so a step
// starts with y = LayerNorm(x) in place.  With the first layer's q/k/v table (route qkv0) both write the token's table row into slab 0
// of s.qkv instead, and layer 0 starts at its attention.
static int gen_start(const StepCtx& c) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const GenPrompt& pr = c.gc->req.pr;
    if (c.r->guided) {   // both halves start from their clip's token: the launches of a plain start, once per half
        for (int half = 0; half < 2; ++half) {
            const size_t r0 = (size_t)half * c.Bc;
            DIMX_TRY(launch_embed_step(h->dec.tok_emb, c.DD, c.V, c.start, c.tokens, c.n, s.step, s.x + r0 * c.DD, c.Bc, 1, c.st, c.pos,
                                       c.pos_scale, pr.ld, pr.step0));
            if (c.r->qkv0)
                DIMX_TRY(launch_gather_start_rows(c.r->qkv0, 3 * c.inner, c.V, c.start, 1, s.qkv + r0 * 3 * c.inner, c.Bc, c.st, pr.ld,
                                                  c.r->kv0 ? s.hist + r0 * c.T : nullptr, c.T));
        }
        if (c.r->qkv0) return DIMX_OK;
        return launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s.st_xr, s.y, h->dec.self_[0].ln_g, c.B, c.DD, c.st);
    }
    DIMX_TRY(launch_embed_step(h->dec.tok_emb, c.DD, c.V, c.start, c.tokens, c.n, s.step, s.x, c.B, c.S, c.st, c.pos, c.pos_scale, pr.ld, pr.step0));
    if (c.r->qkv0)   // the first layer's q/k/v of the start token: a table row into slab 0 (nothing reads y before the layer rewrites it)
        return launch_gather_start_rows(c.r->qkv0, 3 * c.inner, c.V, c.start, c.S, s.qkv, c.B, c.st, pr.ld, c.r->kv0 ? s.hist : nullptr, c.T);
    return launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s.st_xr, s.y, h->dec.self_[0].ln_g, c.B, c.DD, c.st);
}

static int slab_gemm(const StepCtx& c, const void* A, int lda, const Linear& L, float* out, long stride, int* nsl) {
    return slab_gemm_rows(c.h, c.B, c.st, A, lda, L, out, stride, nsl);
}

// XCD-local chain kernels (chain.hip) replace {projection, residual + LayerNorm, projection} triples by one launch.
// deferred LayerNorm (chain.hip, route defer): the two chain launches of a layer write x and bf16(x) un-normalised + partial row
// sums; cross-q (inside chain A) and ff1 (the next launch) run on gamma-scaled weights and correct their results
static int chain_site(const StepCtx& c, int site, const void* A1, int lda1, const Linear* W1, int nslab, const float* gamma,
                      const Linear* W2, float* out2, int ld_out2, const float* colsum2 = nullptr) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.B = c.B; a.C = c.DD;
    if (c.r->defer && W1) { a.defer = 1; a.stats = h->chain_stats_dev; a.colsum2 = colsum2; }
    if (W1) {
        chain_desc(a.g1, *W1);
        a.A1 = A1; a.lda1 = lda1; a.xr = s.xr;
    }
    a.x = s.x; a.y = s.y; a.gamma = gamma;
    a.slabs = nslab ? s.xr : nullptr; a.nslab = nslab; a.slab_stride = s.st_xr;
    if (W2) {
        chain_desc(a.g2, *W2);
        a.out2 = out2; a.ld_out2 = ld_out2;
    }
    a.counters = s.chain_ctr + (size_t)site * kChainSiteWords;
    a.seen = a.counters + 8 * 16; a.err = h->chain_err_dev; a.fault = c.r->fault_inject ? 1 : 0;
    a.step = s.step + 9;   // steps done in this call (== the step counter unless a prompt was prefilled)
    return launch_chain(a, c.st);
}

// the two attentions' arguments (self: q / new k / new v are the projection's split-K slabs; cross: the context K/V)
static DecodeAttnArgs self_args(const StepCtx& c, int l, int ns) {
    const GenScratch& s = c.s;
    const int inner = c.inner;
    DecodeAttnArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.dtype = c.h->at;
    sa.q = s.qkv; sa.q_ld = 3 * inner; sa.q_f32 = 1; sa.nslab = ns; sa.slab_stride = s.st_qkv;
    sa.knew = s.qkv + inner; sa.vnew = s.qkv + 2 * inner; sa.kv_ld = 3 * inner;
    sa.kcache = s.sk[l]; sa.vcache = s.sv[l]; sa.Tmax = c.T;
    sa.out = s.o; sa.o_ld = inner; sa.B = c.B; sa.H = c.heads; sa.step = s.step; sa.scale = c.scale;
    if (l == 0 && c.r->kv0) {   // K / V of position j = the table row of the row's j-th input token; no append
        sa.tab = c.r->kv0; sa.tab_rows = c.V;
        if (c.h->at == DIMX_BF16) { sa.tab_ld = 2 * inner; sa.tab_koff = 0; sa.tab_voff = inner; }
        else { sa.tab_ld = 3 * inner; sa.tab_koff = inner; sa.tab_voff = 2 * inner; }
        sa.hist = s.hist; sa.hist_ld = c.T;
    }
    return sa;
}

// Online generation (route win): the cross attention's key count follows the step counter.  Only the one-query kernels of
// decode_attn.hip have that form, so the layer kernel and the MFMA multi-query route are not taken.
static DecodeAttnArgs cross_args(const StepCtx& c, int l) {
    const GenScratch& s = c.s;
    DecodeAttnArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.dtype = c.h->at;
    ca.q = s.qc; ca.q_ld = c.inner; ca.q_f32 = 1; ca.nslab = 1; ca.slab_stride = s.st_qc;
    ca.kcache = (void*)c.ck[l]; ca.vcache = (void*)c.cv[l]; ca.Tmax = c.Tp;
    ca.out = s.o; ca.o_ld = c.inner; ca.B = c.S > 1 ? c.nclip : c.Bc; ca.rows_per_clip = c.S; ca.H = c.heads;
    ca.n_keys = c.n_keys; ca.kmask = c.ctx_mask; ca.kmask_ld = c.T; ca.scale = c.scale;
    if (c.r->win) { ca.win = 1; ca.lookahead = c.r->lookahead; ca.step = s.step; }
    return ca;
}

// The step's one-query cross attention: the cache form, or (route kv8) the same arguments over the FP8 copy of the context K/V
// With several samples per clip (route kv8_samples) it is the multi-query launch: ca.B clips of ca.rows_per_clip rows, q as the f32
// slabs of the projection, or (qb: the bf16 rows of a plain projection) in the operand type; the exact form on an f32 handle.
static int cross_attention(const StepCtx& c, int l, const DecodeAttnArgs& ca, const void* qb = nullptr) {
    if (!c.r->kv8) return launch_decode_attn(ca, c.st);
    Kv8AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = (const float*)ca.q; a.q_ld = ca.q_ld; a.nslab = ca.nslab; a.slab_stride = ca.slab_stride;
    a.kcodes = c.kv8[l].kcodes; a.kscale = c.kv8[l].kscale; a.vcodes = c.kv8[l].vcodes; a.vscale = c.kv8[l].vscale; a.Tmax = ca.Tmax;
    a.out = ca.out; a.out_dtype = ca.dtype; a.o_ld = ca.o_ld; a.B = ca.B; a.H = ca.H;
    a.n_keys = ca.n_keys; a.kmask = ca.kmask; a.kmask_ld = ca.kmask_ld; a.scale = ca.scale;
    a.win = ca.win; a.lookahead = ca.lookahead; a.step = ca.step;
    if (c.r->kv8_samples) {
        a.rows_per_clip = ca.rows_per_clip;
        a.exact = ca.dtype == DIMX_F32 ? 1 : 0;
        if (qb) { a.q = (const float*)qb; a.q_bf16 = 1; a.nslab = 1; a.slab_stride = 0; }
        return launch_decode_attn_mq_kv8(a, c.st);
    }
    return launch_decode_attn_kv8(a, c.st);
}

// The step's self attention: the cache (or table) form, or (route self_kv8) the same arguments over the FP8 self caches -- one launch
// quantises and appends this step's row and attends over the codes.  Layer 0 in its table form has no cache and keeps its launch.
static int self_attention(const StepCtx& c, int l, const DecodeAttnArgs& sa) {
    if (!c.r->self_kv8 || sa.tab) return launch_decode_attn(sa, c.st);
    Kv8SelfArgs a;
    memset(&a, 0, sizeof(a));
    a.q = (const float*)sa.q; a.knew = (const float*)sa.knew; a.vnew = (const float*)sa.vnew;
    a.ld = sa.q_ld; a.nslab = sa.nslab; a.slab_stride = sa.slab_stride;
    a.kcodes = c.skv8[l].kcodes; a.kscale = c.skv8[l].kscale; a.vcodes = c.skv8[l].vcodes; a.vscale = c.skv8[l].vscale; a.Tmax = c.Tp;
    a.out = sa.out; a.out_dtype = sa.dtype; a.o_ld = sa.o_ld; a.B = sa.B; a.H = sa.H;
    a.step = sa.step; a.n_max = (c.n < c.Tp ? c.n : c.Tp) - 1; a.scale = sa.scale;
    return launch_decode_attn_self_kv8(a, c.st);
}

// round 5: the attention half of a layer as one XCD-local launch (chain.hip xcd_layer_kernel; DIMX_NO_LAYER_CHAIN=1: the four
// launches, for A/B runs).  False when the layer has no deferred-LayerNorm weights.
static bool layer_args(const StepCtx& c, int l, const DecodeAttnArgs& sa, const DecodeAttnArgs& ca, LayerChainArgs& lc) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const Linear& so = h->dec.self_[l].out;
    const Linear& cq = h->dec.cross[l].q_ln;
    const Linear& co = h->dec.cross[l].out;
    if (!so.w || !cq.w || !co.w || !h->dec.cross[l].q_ln_colsum) return false;
    lc.B = c.B; lc.C = c.DD; lc.sa = sa; lc.ca = ca;
    chain_desc(lc.g_so, so);
    chain_desc(lc.g_cq, cq);
    chain_desc(lc.g_co, co);
    lc.o = s.o; lc.ld_o = c.inner; lc.x = s.x; lc.y = s.y;
    lc.stats = h->chain_stats_dev; lc.colsum_cq = h->dec.cross[l].q_ln_colsum;
    lc.qc = s.qc; lc.ld_qc = c.inner;
    lc.counters = s.chain_ctr + (size_t)(3 * h->decg.depth + 1 + l) * kChainSiteWords;
    lc.seen = lc.counters + 8 * 16; lc.step = s.step + 9; lc.err = h->chain_err_dev; lc.fault = c.r->fault_inject ? 1 : 0;
    lc.sc_stride = (c.T + 15) / 16 * 16;
    lc.prof = h->layer_prof_dev ? h->layer_prof_dev + (size_t)l * 256 * 16 : nullptr;
    return true;
}

// round 6, best-of-N in one pass (code/x_engine_pt.py:257), bf16: the S queries of a clip against its context K/V on the
// matrix cores -- the prefill attention kernel with Lq = S (one 128-query item per (clip, head), K / V streamed once),
// queries in the operand type from a plain projection (rows = clips x S: no split-K needed).  The VALU multi-query
// kernel it replaces ran 118 us per launch at 256 clips x 10 samples, 3 x its HBM floor (profiles/r06_samples10.txt).
static int cross_attention_multi(const StepCtx& c, int l, const DecodeAttnArgs& ca) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const int heads = c.heads, D = c.D, inner = c.inner, S = c.S, T = c.T, Tp = c.Tp;
    GemmArgs g;
    gemm_lin(h, s.y, c.DD, h->dec.cross[l].qkv, c.B, g);
    g.out_dtype = h->at;
    gemm_set_plain_out(g, s.qcb, inner);
    DIMX_TRY(launch_gemm(g, c.st));
    AttnArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.dtype = h->at;
    ta.q = s.qcb;
    ta.q_sb = (long)S * inner; ta.q_st = inner; ta.q_sh = D;
    ta.k = ca.kcache; ta.k_sb = (long)heads * Tp * D; ta.k_sh = (long)Tp * D; ta.k_st = D;
    ta.vt = ca.vcache; ta.v_rows = 1; ta.v_sb = (long)heads * Tp * D; ta.v_sh = (long)Tp * D; ta.v_st = D;
    ta.o = s.o; ta.o_sb = (long)S * inner; ta.o_st = inner; ta.o_sh = D;
    ta.B = c.nclip; ta.H = heads; ta.Lq = S; ta.Lk = T; ta.D = D;
    ta.scale = c.scale;
    ta.kmask = c.ctx_mask; ta.kmask_ld = T;
    ta.kwords = s.kw; ta.kwords_cap = s.kw_cap;
    ta.kwords_ready = 1;   // packed once per generation (generate_impl)
    return launch_attention_tr(ta, c.st);
}

// Route sample_head: what finish_sample would pass to the sampler launch, for the head of layer 0's launch (the logits are the
// final chain launch's single slab; the parameter block is the group's 16 words behind s.step)
static void head_args(const StepCtx& c, SampleHeadArgs& hd) {
    const GenScratch& s = c.s;
    const GenRequest& q = c.gc->req;
    memset(&hd, 0, sizeof(hd));
    hd.on = 1;
    hd.logits = s.logits; hd.ld_logits = c.V; hd.nslab = 1; hd.slab_stride = s.st_lg;
    hd.top_k = c.gc->top_k; hd.noise = q.noise; hd.row0 = c.row0; hd.rows_total = c.gc->R;
    hd.tokens = c.tokens; hd.tok_ld = c.n; hd.logits_out = c.logits_out; hd.logits_out_ld = c.n;
    hd.emb_table = c.h->dec.tok_emb; hd.qkv0 = c.r->qkv0; hd.qkv0_N = 3 * c.inner;
    hd.hist = s.hist; hd.hist_ld = c.T;
    hd.params = s.step;
}

// Self attention, cross attention and their out-projections; leaves y = the feed-forward's input.  *pending: the slabs of the
// previous residual projection not yet folded into x (in: the last layer's feed-forward; the two chain routes fold their own).
static int attention_half(const StepCtx& c, int l, int* pending) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const StepRoute& r = *c.r;
    const int B = c.B, DD = c.DD, inner = c.inner;
    int ns = 0;
    if (l > 0) DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, *pending, s.st_xr, s.y, h->dec.self_[l].ln_g, B, DD, c.st));
    if (l == 0 && r.qkv0)
        ns = 1;   // slab 0 already holds this token's q/k/v (the sampler / the start-token step copied the table row)
    else
        DIMX_TRY(slab_gemm(c, s.y, DD, h->dec.self_[l].qkv, s.qkv, s.st_qkv, &ns));
    const DecodeAttnArgs sa = self_args(c, l, ns);
    DecodeAttnArgs ca = cross_args(c, l);
    if (r.layer_kernel[l]) {
        // round 5: self attention -> out-projection -> cross-q -> cross attention -> out-projection as ONE XCD-local launch
        LayerChainArgs lc;
        memset(&lc, 0, sizeof(lc));
        DIMX_REQUIRE(layer_args(c, l, sa, ca, lc), DIMX_ERR_STATE, "generate: layer %d lost its layer-kernel weights after the route was resolved", l);
        if (l == 0 && r.sample_head) head_args(c, lc.head);
        DIMX_TRY(launch_layer_chain(lc, c.st));
    } else if (r.chain) {
        DIMX_TRY(self_attention(c, l, sa));
        // self out-projection -> x += . -> LayerNorm -> cross q-projection
        if (r.defer)
            DIMX_TRY(chain_site(c, 3 * l, s.o, inner, &h->dec.self_[l].out, 0, h->dec.cross[l].ln_g, &h->dec.cross[l].q_ln, s.qc, inner,
                                h->dec.cross[l].q_ln_colsum));
        else
            DIMX_TRY(chain_site(c, 3 * l, s.o, inner, &h->dec.self_[l].out, 0, h->dec.cross[l].ln_g, &h->dec.cross[l].qkv, s.qc, inner));
        ca.nslab = 1;
        DIMX_TRY(cross_attention(c, l, ca));
        // cross out-projection -> x += . -> LayerNorm (feed-forward input)
        DIMX_TRY(chain_site(c, 3 * l + 1, s.o, inner, &h->dec.cross[l].out, 0, h->dec.ff[l].ln_g, nullptr, nullptr, 0));
    } else if (r.guided) {
        // The unconditional rows [Bc, B) are the decoder without its cross sublayers (every cross projection is bias-free: a context
        // of zero rows gives K = V = 0 and W_o . 0 = 0, dimx/guidance.py): the q projection, the one-query attention and the out
        // projection run on the conditional rows alone, and no launch reads cross K / V for the others.
        const int Bc = c.Bc;
        const size_t es = c.es;
        DIMX_TRY(launch_decode_attn(sa, c.st));
        DIMX_TRY(slab_gemm(c, s.o, inner, h->dec.self_[l].out, s.xr, s.st_xr, pending));
        // folds the self slabs into x for all rows; y is the cross pre-norm, read for the conditional rows only
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, *pending, s.st_xr, s.y, h->dec.cross[l].ln_g, B, DD, c.st));
        DIMX_TRY(slab_gemm_rows(h, Bc, c.st, s.y, DD, h->dec.cross[l].qkv, s.qc, s.st_qc, &ns));
        ca.nslab = ns;
        DIMX_TRY(cross_attention(c, l, ca));
        DIMX_TRY(slab_gemm_rows(h, Bc, c.st, s.o, inner, h->dec.cross[l].out, s.xr, s.st_xr, pending));
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, *pending, s.st_xr, s.y, h->dec.ff[l].ln_g, Bc, DD, c.st));
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x + (size_t)Bc * DD, s.xr + (size_t)Bc * DD, 0, s.st_xr, (unsigned char*)s.y + (size_t)Bc * DD * es,
                                            h->dec.ff[l].ln_g, B - Bc, DD, c.st));
    } else {
        DIMX_TRY(self_attention(c, l, sa));
        DIMX_TRY(slab_gemm(c, s.o, inner, h->dec.self_[l].out, s.xr, s.st_xr, pending));
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, *pending, s.st_xr, s.y, h->dec.cross[l].ln_g, B, DD, c.st));
        if (r.multi_tr && !r.win && r.kv8_samples) {
            // the bf16 projection of cross_attention_multi (rows = clips x S: no split-K), then the S queries of a clip over its codes
            GemmArgs g;
            gemm_lin(h, s.y, DD, h->dec.cross[l].qkv, B, g);
            g.out_dtype = h->at;
            gemm_set_plain_out(g, s.qcb, inner);
            DIMX_TRY(launch_gemm(g, c.st));
            DIMX_TRY(cross_attention(c, l, ca, s.qcb));
        } else if (r.multi_tr && !r.win) {
            DIMX_TRY(cross_attention_multi(c, l, ca));
        } else {
            DIMX_TRY(slab_gemm(c, s.y, DD, h->dec.cross[l].qkv, s.qc, s.st_qc, &ns));
            ca.nslab = ns;
            DIMX_TRY(cross_attention(c, l, ca));
        }
        DIMX_TRY(slab_gemm(c, s.o, inner, h->dec.cross[l].out, s.xr, s.st_xr, pending));
        DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, *pending, s.st_xr, s.y, h->dec.ff[l].ln_g, B, DD, c.st));
    }
    return DIMX_OK;
}

// f = gelu(y . W1^T), then the second projection's slabs: *pending of them wait in s.xr for the next pre-norm to fold into x
static int feed_forward(const StepCtx& c, int l, int* pending) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const bool defer = c.r->defer;
    const int F = c.DD * h->decg.ff_mult;
    GemmArgs g;
    gemm_lin(h, s.y, c.DD, defer ? h->dec.ff[l].f1_ln : h->dec.ff[l].f1, c.B, g);
    g.x3_decode = 1;
    if (defer) {
        g.ln_stats = h->chain_stats_dev;
        g.ln_err = h->chain_err_dev;
        g.ln_colsum = h->dec.ff[l].f1_ln_colsum;
        g.ln_C = c.DD;
    }
    g.out_dtype = h->at;
    g.act = ACT_GELU_ERF;
    gemm_set_plain_out(g, s.f, F);
    DIMX_TRY(launch_gemm(g, c.st));
    return slab_gemm(c, s.f, F, h->dec.ff[l].f2, s.xr, s.st_xr, pending);
}

// x += feed-forward slabs -> final LayerNorm -> logits, *nlg slabs of them
static int logits(const StepCtx& c, int pending, int* nlg) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    if (c.r->logits_chain) {   // the chain kernel has no bias input: a checkpoint with the optional to_logits.bias takes the two launches below
        *nlg = 1;
        return chain_site(c, 3 * h->decg.depth, nullptr, 0, nullptr, pending, h->dec.final_g, &h->dec.logits, s.logits, c.V);
    }
    DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, pending, s.st_xr, s.y, h->dec.final_g, c.B, c.DD, c.st));
    return slab_gemm(c, s.y, c.DD, h->dec.logits, s.logits, s.st_lg, nlg);
}

// Beam search (beam.hip): rows clip * S + w are the S hypotheses of a clip.  The selection writes column c of the token rows in
// the new order, the next step's embedding / q/k/v table rows, and advances the step word; the reorder then permutes cache
// positions 0 .. c and token columns < c by parent beam, reading c as the advanced word - 1.
static int finish_beam(const StepCtx& c, int nlg) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const GenPrompt& pr = c.gc->req.pr;
    const BeamCall& bm = *c.r->beam;
    const int row0 = c.row0, n = c.n, depth = h->decg.depth;
    BeamSelectArgs bs;
    bs.logits = s.logits; bs.nslab = nlg; bs.slab_stride = s.st_lg; bs.nclip = c.nclip; bs.W = c.S;
    bs.step_dev = s.step; bs.step_rw = s.step; bs.done_ctr = (unsigned*)(s.step + 8); bs.epoch_rw = s.step + 9; bs.dev_params = s.step + 2;
    bs.prompt = c.forced; bs.prompt_ld = pr.ld; bs.prompt_max = pr.Pmax; bs.prompt_len = c.forced_len;
    bs.lens = bm.lens ? bm.lens + c.clip0 : nullptr; bs.len_off = c.T - n;
    bs.cum_in = bm.cum + row0; bs.cum_out = bm.cum + row0; bs.parent = bm.parent + row0;
    bs.tokens = c.tokens; bs.backptr = bm.backptr ? bm.backptr + (size_t)row0 * n : nullptr; bs.tok_ld = n; bs.logits_out = c.logits_out;
    bs.emb_table = h->dec.tok_emb; bs.emb_C = c.DD; bs.x_next = s.x;
    bs.qkv0_table = c.r->qkv0; bs.qkv0_out = s.qkv; bs.qkv0_N = 3 * c.inner;
    DIMX_TRY(launch_beam_select(bs, c.st));
    if (!c.r->qkv0) DIMX_TRY(launch_add_slabs_layernorm(h->at, s.x, s.xr, 0, s.st_xr, s.y, h->dec.self_[0].ln_g, c.B, c.DD, c.st));
    if (c.r->self_kv8) {   // every layer's self attention reads the codes (no table form under beam search): they are what moves
        // one launch holds kBeamKv8Pairs (code plane, scale plane) pairs: the K and V pairs of 4 layers.  A deeper decoder takes a
        // second launch; the first one moves the token / back-pointer columns
        constexpr int per = kBeamKv8Pairs / 2;
        for (int l0 = 0; l0 < depth; l0 += per) {
            BeamReorderKv8Args bk;
            const int nl = depth - l0 < per ? depth - l0 : per;
            for (int l = 0; l < nl; ++l) {
                bk.codes[2 * l] = c.skv8[l0 + l].kcodes; bk.scale[2 * l] = c.skv8[l0 + l].kscale;
                bk.codes[2 * l + 1] = c.skv8[l0 + l].vcodes; bk.scale[2 * l + 1] = c.skv8[l0 + l].vscale;
            }
            bk.nbuf = 2 * nl; bk.nclip = c.nclip; bk.W = c.S; bk.H = c.heads; bk.Tp = c.Tp;
            bk.parent = bs.parent; bk.step_dev = s.step; bk.step_back = 1;
            if (l0 == 0) { bk.tokens = c.tokens; bk.backptr = bs.backptr; bk.tok_ld = n; }
            DIMX_TRY(launch_beam_reorder_kv8(bk, c.st));
        }
        return DIMX_OK;
    }
    BeamReorderArgs br;
    for (int l = 0; l < depth; ++l) {
        br.buf[2 * l] = s.sk[l];
        br.buf[2 * l + 1] = s.sv[l];
    }
    br.nbuf = 2 * depth; br.es = (int)c.es; br.nclip = c.nclip; br.W = c.S; br.H = c.heads; br.T = c.T;
    br.parent = bs.parent; br.step_dev = s.step; br.step_back = 1;
    br.tokens = c.tokens; br.backptr = bs.backptr; br.tok_ld = n;
    return launch_beam_reorder(br, c.st);
}

// the sampler: token of this step, the next step's embedding row and its first-layer pre-norm (or q/k/v table row), step += 1
static int finish_sample(const StepCtx& c, int nlg) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const GenRequest& q = c.gc->req;
    const GenPrompt& pr = q.pr;
    const float* qkv0 = c.r->qkv0;
    SampleArgs sm;
    sm.logits = s.logits; sm.ld_logits = c.V; sm.R = c.B; sm.nslab = nlg; sm.slab_stride = s.st_lg; sm.row0 = c.row0; sm.rows_total = c.gc->R;
    sm.top_k = c.gc->top_k; sm.noise = q.noise; sm.filt.kind = h->filter_kind;
    sm.temperature = q.temperature; sm.seed = q.seed;   // read from the parameter block (dev_params) instead, like filt.a / b
    sm.step_dev = s.step; sm.step_rw = s.step; sm.dev_params = s.step + 2; sm.done_ctr = (unsigned*)(s.step + 8); sm.epoch_rw = s.step + 9;
    sm.tokens = c.tokens; sm.tok_ld = c.n; sm.tok_col_from_step = 1; sm.logits_out = c.logits_out; sm.logits_out_ld = c.n;
    sm.emb_table = h->dec.tok_emb; sm.emb_C = c.DD; sm.x_next = s.x; sm.pos_table = c.pos; sm.pos_scale = c.pos_scale; sm.pos_rows = c.n;
    sm.y_next = qkv0 ? nullptr : s.y; sm.y_gamma = qkv0 ? nullptr : h->dec.self_[0].ln_g; sm.y_dtype = h->at;
    sm.qkv0_table = qkv0; sm.qkv0_out = s.qkv; sm.qkv0_N = 3 * c.inner;
    if (c.r->kv0) { sm.hist = s.hist; sm.hist_ld = c.T; }
    sm.prompt = c.forced; sm.prompt_ld = pr.ld; sm.prompt_max = pr.Pmax; sm.prompt_len = c.forced_len; sm.prompt_div = c.S;
    return launch_sample(sm, c.st);
}

// The guided sampler in finish_sample's place: one wave per clip forms the guided row from rows b and b + Bc of the logits, samples
// it as row b of a Bc-row generation, and writes the token's embedding / pre-norm / table rows for both halves
static int finish_guided(const StepCtx& c, int nlg) {
    dimx_handle h = c.h;
    const GenScratch& s = c.s;
    const GenRequest& q = c.gc->req;
    const GenPrompt& pr = q.pr;
    const float* qkv0 = c.r->qkv0;
    SampleArgs sm;
    sm.logits = s.logits; sm.ld_logits = c.V; sm.R = c.Bc; sm.nslab = nlg; sm.slab_stride = s.st_lg; sm.row0 = 0; sm.rows_total = c.Bc;
    sm.top_k = c.gc->top_k; sm.noise = q.noise; sm.filt.kind = h->filter_kind;
    sm.temperature = q.temperature; sm.seed = q.seed;
    sm.step_dev = s.step; sm.step_rw = s.step; sm.dev_params = s.step + 2; sm.done_ctr = (unsigned*)(s.step + 8); sm.epoch_rw = s.step + 9;
    sm.tokens = c.tokens; sm.tok_ld = c.n; sm.tok_col_from_step = 1; sm.logits_out = c.logits_out; sm.logits_out_ld = c.n;
    sm.emb_table = h->dec.tok_emb; sm.emb_C = c.DD; sm.x_next = s.x; sm.pos_table = c.pos; sm.pos_scale = c.pos_scale; sm.pos_rows = c.n;
    sm.y_next = qkv0 ? nullptr : s.y; sm.y_gamma = qkv0 ? nullptr : h->dec.self_[0].ln_g; sm.y_dtype = h->at;
    sm.qkv0_table = qkv0; sm.qkv0_out = s.qkv; sm.qkv0_N = 3 * c.inner;
    if (c.r->kv0) { sm.hist = s.hist; sm.hist_ld = c.T; }
    sm.prompt = c.forced; sm.prompt_ld = pr.ld; sm.prompt_max = pr.Pmax; sm.prompt_len = c.forced_len; sm.prompt_div = 1;
    GuidedArgs g;
    g.logits_u = s.logits + (size_t)c.Bc * c.V; g.scale = q.scale; g.branch_out = q.branch_out;
    return launch_sample_guided(sm, g, c.st);
}

// one decoder step for a clip group: x = emb(token) -> depth x {attention half, feed-forward} -> logits -> sample -> step += 1
static int gen_step(const StepCtx& c) {
    int pending = 0;  // slabs of the previous residual projection not yet folded into x
    for (int l = 0; l < c.h->decg.depth; ++l) {
        DIMX_TRY(attention_half(c, l, &pending));
        DIMX_TRY(feed_forward(c, l, &pending));
    }
    int nlg = 0;
    DIMX_TRY(logits(c, pending, &nlg));
    if (c.r->sample_head) return DIMX_OK;   // the next step's first launch samples these logits; the call's last ones: generate_impl
    return c.r->beam ? finish_beam(c, nlg) : c.r->guided ? finish_guided(c, nlg) : finish_sample(c, nlg);
}

// What the steps of a call launch, decided once: from the handle's switches, the request and the shapes of the call's group 0 of
// `rows` sequences.  One route serves every group: with more than one group the chain is off, and nothing else depends on the
// group.  Needs chain_state_ensure before it (the chain predicate asks for the flag word); allocates the tables it points to.
static int resolve_route(dimx_handle h, const GenCall& gc, int G, int rows, StepRoute& r) {
    const GenRequest& q = gc.req;
    const DecGeom& dg = h->decg;
    r = StepRoute{};
    r.G = G;
    r.S = q.S;
    r.beam = q.beam;
    r.fault_inject = h->chain_fault_inject > 0;
    r.chain = gen_use_chain(h, rows, q.S);
    r.defer = r.chain && h->defer_ln && h->chain_stats_dev && h->dec.cross[0].q_ln.w && h->dec.ff[0].f1_ln.w;
    r.logits_chain = r.chain && !h->dec.logits.bias;
    r.multi_tr = gen_multi_tr(h, q.S);   // consulted on the per-op branch and without the window only
    r.win = h->xwin_on != 0;
    r.lookahead = r.win ? h->xwin_lookahead : 0;
    r.kv8 = gc.kv8_buf != nullptr;   // the layer kernel streams the caches itself: not taken, exactly as under the window
    r.kv8_samples = r.kv8 && q.S > 1;   // gen_open let S > 1 through under dimx_set_cross_kv8_samples (a beam: dimx_set_beam_kv8) only
    r.self_kv8 = gc.self_kv8_buf != nullptr;   // no layer kernel either: it streams the self caches itself
    r.guided = q.guided;
    if (r.guided) r.chain = r.defer = r.logits_chain = r.multi_tr = false;   // the per-op step, as a session takes it (no layer kernel either: it needs chain)
    // one group: every projection launch of the generation has R rows, and so has the table's build
    if (G == 1 && qkv0_table_supported(h)) {
        DIMX_TRY(qkv0_table_alloc(h));
        r.qkv0 = h->qkv0_table;
    }
    // the first layer's self attention from the table: no beam search (the cache reorder would have to permute the history) and
    // no prompt (a prefill fills the cache, not the history); any number of samples per clip: rows are samples
    if (r.qkv0 && h->use_kv0_table && !q.beam && q.pr.step0 == 0 && q.pr.Pmax <= 1 && dg.dim_head == 64 && dg.num_tokens <= 512)
        r.kv0 = h->at == DIMX_BF16 ? h->kv0_image : (const void*)h->qkv0_table;
    // the layer kernel depends on shapes only, so its per-layer support is settled here on the arguments the step will pass
    if (h->use_layer_chain && r.chain && r.defer && q.S == 1 && 4 * dg.depth + 1 <= kChainSites && !r.win && !r.kv8 && !r.self_kv8) {
        const StepCtx c = step_ctx(h, gc, r, 0, rows, 0, q.st);
        for (int l = 0; l < dg.depth; ++l) {
            LayerChainArgs lc;
            memset(&lc, 0, sizeof(lc));
            r.layer_kernel[l] = layer_args(c, l, self_args(c, l, 1), cross_args(c, l), lc) && layer_chain_supported(lc, h->cu_count);
        }
    }
    // The sampler as the head of layer 0's launch: that launch in its table form, the top-k sampler on the final chain launch's one
    // slab of logits (no to_logits.bias), every row its own clip in one group, and nothing else ending the step or forcing tokens
    r.sample_head = h->use_sample_head && r.kv0 && r.layer_kernel[0] && r.logits_chain && h->filter_kind == DIMX_FILTER_TOP_K && !q.beam &&
                    !r.guided && q.pr.step0 == 0 && q.pr.Pmax <= 1 && G == 1 && q.S == 1 && dg.num_tokens == 512 && dg.dim % 4 == 0;
    return DIMX_OK;
}

// greedy vs sampling is decided from the device-side parameters; only shapes, pointers and the route key the graph.  The prompt's
// pointers, row stride and width are kernel arguments of the sampler; P0 is not (the counters' start value and the
// number of launches), so a call with another P0 replays the same graphs.
static GraphKey graph_key(dimx_handle h, const GenCall& gc, const StepRoute& r) {
    const GenRequest& q = gc.req;
    GraphKey k{};
    k.ws = q.ws; k.B = q.B; k.T = q.T; k.top_k = gc.top_k;
    k.noise = q.noise; k.start = q.pr.tok; k.mask = q.ctx_mask; k.tokens = q.tokens; k.logits_out = q.logits_out;
    k.G = r.G; k.S = r.S;
    k.chain = r.chain; k.defer = r.defer; k.logits_chain = r.logits_chain; k.multi_tr = r.multi_tr; k.fault_inject = r.fault_inject;
    for (int l = 0; l < 8; ++l) k.layer_kernel |= r.layer_kernel[l] ? 1u << l : 0u;
    k.qkv0 = r.qkv0; k.kv0 = r.kv0; k.sample_head = r.sample_head;
    k.prompt_len = q.pr.len; k.ld_prompt = q.pr.ld; k.Pmax = q.pr.Pmax;
    k.filter_kind = h->filter_kind;
    k.beam = q.beam ? *q.beam : BeamCall{};
    k.xwin_on = r.win ? 1 : 0; k.xwin_lookahead = r.lookahead;
    k.guided = r.guided; k.branch_out = q.branch_out;
    k.kv8 = r.kv8 ? gc.kv8_buf : nullptr;
    k.kv8_samples = r.kv8_samples;
    k.self_kv8 = r.self_kv8 ? gc.self_kv8_buf : nullptr;
    k.beam_reorder_kv8 = q.beam && r.self_kv8;
    return k;
}

// Prefill of a prompted generation: the teacher-forced decoder stack of dimx_decode_tf over the positions 0 .. n0 - 1 of every
// clip (no key mask), every layer's self-attention K / V stored into the generation cache [B*S, H, T, 64] (kv_prefill.hip), no
// output head, and the last layer stops after its q/k/v projection -- its attentions and feed-forward feed nothing.
// Cross attention reads the context K / V where dimx_encode_ctx(for_generate = 1) left them, [B, H, Tp, 64]: the bf16
// attention takes that layout as it is (row-major V); the f32 attention reads V^T, so the f32 mode transposes one layer's V
// into scratch first (a copy, not a second projection of the context).
// win (pr.win): the cross attention is the windowed one (win_attn.hip) -- row t sees the keys below clamp(t + 2 + *win, 1, n_keys),
// what decode step t reads; f32 queries, V row-major as it lies, no transpose.
static int gen_prefill(dimx_handle h, const CtxPersist& cp, const GenScratch& gs, const PrefillScratch& s, const GenPrompt& pr,
                       const uint8_t* ctx_mask, int B, int T, int S, int32_t* tokens, hipStream_t st, const int* win = nullptr,
                       int n_keys = 0) {
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
        if (win) {
            const XAttn& x = h->dec.cross[l];
            float* qf = win_q_rows(s, B, n0, heads * D, es_of(h));
            DIMX_REQUIRE(qf, DIMX_ERR_WORKSPACE, "generate: no room for the windowed prefill's f32 queries");
            DIMX_TRY(launch_layernorm(h->at, s.h, s.y, x.ln_g, nullptr, M, DD, st));
            DIMX_TRY(linear(h, s.y, DD, x.qkv, M, DIMX_F32, qf, heads * D, st));
            WinAttnArgs w;
            w.dtype = h->at;
            w.q = qf; w.ld = heads * D;
            w.kcache = cp.ck[l]; w.vcache = cp.cv[l]; w.Tp = Tp;
            w.out = s.o; w.o_ld = heads * D;
            w.B = B; w.H = heads; w.Lq = n0; w.t0 = 0; w.n_keys = n_keys; w.lookahead = *win;
            w.kmask = ctx_mask; w.kmask_ld = T;
            w.scale = 1.0f / sqrtf((float)D);
            DIMX_TRY(launch_win_attn(w, st));
            DIMX_TRY(residual_linear(h, s.o, heads * D, x.out, M, s.h, DD, st));
            DIMX_TRY(ff_sublayer(h, s, h->dec.ff[l].ln_g, nullptr, h->dec.ff[l].f1, h->dec.ff[l].f2, nullptr, ACT_GELU_ERF, M, DD, st));
            continue;
        }
        // cross attention over the context K / V of the generation layout [B,H,Tp,64]; the f32 attention reads V^T from s.cvt
        set_attn_packed(a, h->at, s.q, cp.ck[l], rowv ? cp.cv[l] : s.cvt, s.o, B, heads, n0, T, D, Tp, rowv);
        a.k_sb = (long)heads * Tp * D; a.k_sh = (long)Tp * D; a.k_st = D;
        if (rowv) { a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_st = D; }
        DIMX_TRY(cross_attn_sublayer(h, s, h->dec.cross[l], a, ctx_mask, DD, st, rowv ? nullptr : (const float*)cp.cv[l]));
        DIMX_TRY(ff_sublayer(h, s, h->dec.ff[l].ln_g, nullptr, h->dec.ff[l].f1, h->dec.ff[l].f2, nullptr, ACT_GELU_ERF, M, DD, st));
    }
    return DIMX_OK;
}

// the one-time allocations of the chain kernels: flag word (device + pinned host copy + its event) and the deferred form's row sums
static int chain_state_ensure(dimx_handle h) {
    if (!(h->use_chain && h->at == DIMX_BF16 && !h->chain_err_dev)) return DIMX_OK;
    DIMX_HIP(hipMalloc((void**)&h->chain_err_dev, 64));
    DIMX_HIP(hipMemset(h->chain_err_dev, 0, 64));
    DIMX_HIP(hipMalloc((void**)&h->chain_stats_dev, 8 * 32 * 32 * 2 * sizeof(float)));
    DIMX_HIP(hipMemset(h->chain_stats_dev, 0, 8 * 32 * 32 * 2 * sizeof(float)));
    DIMX_HIP(hipHostMalloc((void**)&h->chain_err_host, 64, hipHostMallocDefault));
    *h->chain_err_host = 0;
    DIMX_HIP(hipEventCreateWithFlags(&h->chain_err_ev, hipEventDisableTiming));
    return DIMX_OK;
}

// Independent clip groups run as separate step graphs on separate streams: every decode kernel is
// latency-bound at these sizes, so two groups in flight let one group's GEMM/LayerNorm chain overlap the
// other group's HBM-bound attention.  Results do not depend on the grouping (per-clip state only; the
// sampler's noise / counter-based RNG is indexed by the global clip row).
static int gen_groups_fork(dimx_handle h, int G, hipStream_t st, hipStream_t* gs) {
    if (G == 1) {
        gs[0] = st;
        return DIMX_OK;
    }
    if (!h->ev_fork) DIMX_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    DIMX_HIP(hipEventRecord(h->ev_fork, st));
    for (int g = 0; g < G; ++g) {
        if (!h->grp_stream[g]) DIMX_HIP(hipStreamCreateWithFlags(&h->grp_stream[g], hipStreamNonBlocking));
        if (!h->ev_join[g]) DIMX_HIP(hipEventCreateWithFlags(&h->ev_join[g], hipEventDisableTiming));
        gs[g] = h->grp_stream[g];
        DIMX_HIP(hipStreamWaitEvent(gs[g], h->ev_fork, 0));
    }
    return DIMX_OK;
}

static int gen_groups_join(dimx_handle h, int G, hipStream_t st, const hipStream_t* gs) {
    if (G == 1) return DIMX_OK;
    for (int g = 0; g < G; ++g) {
        DIMX_HIP(hipEventRecord(h->ev_join[g], gs[g]));
        DIMX_HIP(hipStreamWaitEvent(st, h->ev_join[g], 0));
    }
    return DIMX_OK;
}

// The handle's step graphs are those of `key`: kept when they already are, otherwise destroyed, captured from ctx[0 .. G) on the
// capture stream and instantiated.  A capture that fails midway is ended and dropped, and leaves the handle without valid graphs.
static int step_graphs_ensure(dimx_handle h, const GraphKey& key, const StepCtx* ctx, int G, int n) {
    if (h->graph_valid && h->graph_key == key) return DIMX_OK;
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
        StepCtx c = ctx[g];
        c.st = h->cap_stream;
        for (int pass = 0; pass < 2; ++pass) {
            const int reps = pass == 0 ? 1 : h->graph_unroll;
            if (pass == 1 && (reps <= 1 || n < reps)) continue;
            hipGraph_t graph = nullptr;
            DIMX_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
            int rc = DIMX_OK;
            for (int r = 0; r < reps && rc == DIMX_OK; ++r) rc = gen_step(c);
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
    return DIMX_OK;
}

// nrun steps of every group: the unrolled graph for the bulk, the single-step graph for the remainder
static int step_graphs_replay(dimx_handle h, int nrun, int G, const hipStream_t* gs) {
    const int U = h->graph_unroll;
    int t = 0;
    for (; U > 1 && t + U <= nrun; t += U)
        for (int g = 0; g < G; ++g)
            if (h->graph_multi[g]) DIMX_HIP(hipGraphLaunch(h->graph_multi[g], gs[g]));
            else
                for (int r = 0; r < U; ++r) DIMX_HIP(hipGraphLaunch(h->graph_exec[g], gs[g]));
    for (; t < nrun; ++t)
        for (int g = 0; g < G; ++g) DIMX_HIP(hipGraphLaunch(h->graph_exec[g], gs[g]));
    return DIMX_OK;
}

// The device-side state every run of a call starts from (a regeneration after a chain fault too): chain counters, the parameter
// block, the packed key words of the multi-sample cross attention, the beam scores
static int gen_parameters(dimx_handle h, const GenCall& gc, const StepRoute& route, int n) {
    const GenRequest& q = gc.req;
    const GenScratch& s = gc.s;
    hipStream_t st = q.st;
    DIMX_HIP(hipMemsetAsync(s.chain_ctr, 0, (size_t)kChainSites * kChainSiteWords * 4, st));
    // step / done counters = 0; temperature, seed and the sampler's global row window go to device memory so that
    // the captured step graph is independent of them
    DIMX_TRY(launch_gen_params(s.step, dimx_ctx::kMaxGroups, q.temperature, q.seed, h->shard_row_off * q.S,
                               h->shard_rows_total * q.S, st, q.pr.step0, h->filter_a, h->filter_b, q.guided ? q.scale : 1.f));
    if (route.multi_tr) DIMX_TRY(launch_pack_key_words(q.ctx_mask, q.T, nullptr, q.B, q.T, s.kw, s.kw_cap, st));
    if (!q.beam) return DIMX_OK;
    DIMX_REQUIRE(h->decg.dim_head == 64 && h->decg.depth <= 8 && !h->decg.abs_pos, DIMX_ERR_ARG,
                 "generate_beam: needs 64-wide heads, at most 8 layers and a decoder without positional embedding");
    DIMX_TRY(launch_beam_init(q.beam->cum, q.beam->parent, gc.R, q.S, st));
    if (q.beam->backptr && q.pr.step0 > 0)   // no step ran on the prefilled columns: -1
        DIMX_HIP(hipMemset2DAsync(q.beam->backptr, (size_t)n * 4, 0xFF, (size_t)q.pr.step0 * 4, gc.R, st));
    return DIMX_OK;
}

// A generation from its plan to its last step: what generate_impl builds once per call, kept in one place so that the start and the
// steps can be driven across calls (a streaming session, stream.hip).  The steps' contexts point into it: it is never copied.
struct GenRun {
    GenRequest q;
    CtxPersist cp;
    GenScratch s;
    GenCall gc;
    StepRoute route;
    StepCtx ctx[dimx_ctx::kMaxGroups];
    hipStream_t gs[dimx_ctx::kMaxGroups];
    int G = 1, n = 0, nrun = 0;
    bool graphs = true;   // replay the handle's step graphs where use_graph is on (a session launches its steps directly)
    explicit GenRun(const GenRequest& r) : q(r), cp{}, s{}, gc{q, cp, s, 0, 0} {}
    GenRun(const GenRun&) = delete;
};

// plan, route, parameters, tables, prefill, start.  keep_prefill: the call repeats a generation whose prefill already ran in this
// workspace (the regeneration after a chain fault): the decode steps write cache positions >= step0 and token / logit columns >=
// step0 only, so the prefix is intact and only the counters start over.  prefill_only (tools/bench_prompt.py): the prefill stage
// alone.  sess: a streaming session's generation -- the context K / V are the session's (appended push by push, no
// dimx_encode_ctx), one clip group, the per-op step with the cross-attention window on, no step graphs.
int gen_open(dimx_handle h, GenRun& run, bool keep_prefill, bool prefill_only, const GenSessionSpec* sess) {
    const GenRequest& q = run.q;
    const GenPrompt& pr = q.pr;
    const int B = q.B, T = q.T, S = q.S;
    hipStream_t st = q.st;
    // the other kinds ignore the call's k (and it keys the step graph)
    const int top_k = h && h->filter_kind != DIMX_FILTER_TOP_K ? 0 : q.top_k;
    DIMX_REQUIRE(S == 1 || S == 2 || S == 4 || S == 5 || S == 8 || S == 10, DIMX_ERR_ARG,
                 "generate: n_samples %d not in {1,2,4,5,8,10}", S);
    if (h && h->kv8_buf && !sess) {   // FP8 cross K/V: one row per clip, the sampler ends the step; a session does not read the setting
        // a beam search takes the buffer under dimx_set_beam_kv8 only (its W hypotheses are the multi-query launch's rows)
        DIMX_REQUIRE(q.beam ? h->beam_kv8_on != 0 : (S == 1 || (h->kv8_samples_on && !q.guided)), DIMX_ERR_ARG,
                     "generate: n_samples > 1 and beam search are not available with dimx_set_cross_kv8");
        DIMX_REQUIRE(kv8_bytes(h, B, T) != 0, DIMX_ERR_ARG, "generate: B=%d T=%d is not supported with dimx_set_cross_kv8", B, T);
        DIMX_REQUIRE(h->kv8_bytes >= kv8_bytes(h, B, T), DIMX_ERR_WORKSPACE, "generate: the FP8 cross K/V buffer holds %zu bytes, B=%d T=%d needs %zu (dimx_cross_kv8_bytes)",
                     h->kv8_bytes, B, T, kv8_bytes(h, B, T));
    }
    if (h && h->self_kv8_buf && !sess) {   // FP8 self K/V: rows are sequences, the sampler ends the step; a session does not read the setting
        DIMX_REQUIRE((!q.beam || h->beam_kv8_on) && !q.guided, DIMX_ERR_ARG, "generate: beam search and guidance are not available with dimx_set_self_kv8");
        DIMX_REQUIRE(kv8_bytes(h, B * S, T) != 0, DIMX_ERR_ARG, "generate: B=%d n_samples=%d T=%d is not supported with dimx_set_self_kv8", B, S, T);
        DIMX_REQUIRE(h->self_kv8_bytes >= kv8_bytes(h, B * S, T), DIMX_ERR_WORKSPACE,
                     "generate: the FP8 self K/V buffer holds %zu bytes, B=%d n_samples=%d T=%d needs %zu (dimx_self_kv8_bytes)", h->self_kv8_bytes, B, S, T,
                     kv8_bytes(h, B * S, T));
    }
    const int halves = q.guided ? 2 : 1;   // a guided generation decodes every clip twice: 2B rows of self caches, B cross caches
    DIMX_TRY(check_common(h, B, T, q.ws, q.ws_bytes, COMP_DEC, S * halves));
    DIMX_REQUIRE(pr.tok && q.ctx_mask && q.tokens && T >= 2, DIMX_ERR_ARG, "generate: null argument or T < 2");
    DIMX_REQUIRE(sess || (h->ctx_ready && h->ctx_B == B && h->ctx_T == T && h->ctx_ws == q.ws && h->ctx_for_generate),
                 DIMX_ERR_STATE, "generate: call dimx_encode_ctx(for_generate=1) with the same B, T, ws first");
    // plan
    CtxPersist& cp = run.cp;
    Arena ar = scratch_arena(h, q.ws, q.ws_bytes, B, T, &cp);
    GenScratch& s = run.s;
    const int R = B * S * halves;  // rows of the decode step
    plan_gen(h, ar, R, T, s);
    PrefillScratch ps;
    if (pr.step0 > 0) plan_prefill(h, ar, B, pr.step0, T, ps);
    DIMX_REQUIRE(!ar.overflow, DIMX_ERR_WORKSPACE, "generate: workspace overflow");
    const int n = gen_steps(h, T);
    run.n = n;
    run.nrun = n - pr.step0;   // decode steps of this call
    DIMX_TRY(chain_state_ensure(h));
    int G = h->gen_groups < 1 ? 1 : h->gen_groups;
    if (G > B) G = B;
    if (S > 1 || q.beam || sess || q.guided) G = 1;  // samples of a clip stay together (they share the clip's cross K/V pass)
    run.G = G;
    int lo[dimx_ctx::kMaxGroups + 1];
    for (int g = 0; g <= G; ++g) lo[g] = (int)((long)R * g / G);
    // route
    run.gc.R = R;
    run.gc.top_k = top_k;
    // the FP8 buffers travel with the call: an offline call reads the handle's two settings and nothing of a session's, a session its
    // own pair (stream.hip checked their sizes against (B, Tmax)) and nothing of the handle's
    run.gc.kv8_buf = sess ? sess->kv8_buf : h->kv8_buf;
    run.gc.self_kv8_buf = sess ? sess->self_kv8_buf : h->self_kv8_buf;
    const GenCall& gc = run.gc;
    StepRoute& route = run.route;
    DIMX_TRY(resolve_route(h, gc, G, lo[1] - lo[0], route));
    if (sess) {
        // the chain kernels answer a fault by a regeneration of the whole call, which a session cannot offer
        route.chain = route.defer = route.logits_chain = route.multi_tr = false;
        for (bool& lk : route.layer_kernel) lk = false;
        route.sample_head = false;
        route.win = true;
        route.lookahead = sess->lookahead;
        route.kv8_samples = false;   // kv8 / self_kv8 follow the session's buffers (resolve_route read them from the call)
        run.graphs = false;
    }
    // parameters
    DIMX_TRY(gen_parameters(h, gc, route, n));
    // tables
    if (route.qkv0) DIMX_TRY(qkv0_table_build(h, s, R, st, pr.step0));
    if (route.kv0) ++h->kv0_generations;
    if (route.sample_head) ++h->sample_head_generations;
    // prefill
    if (pr.step0 > 0 && !keep_prefill) {
        // the prefill forms no logits: those columns of logits_out read zero
        if (q.logits_out)
            DIMX_HIP(hipMemset2DAsync(q.logits_out, (size_t)n * h->decg.num_tokens * 4, 0, (size_t)pr.step0 * h->decg.num_tokens * 4, R, st));
        DIMX_REQUIRE(!pr.win || route.win, DIMX_ERR_STATE, "generate: a windowed prefill without the cross-attention window");
        DIMX_TRY(gen_prefill(h, cp, s, ps, pr, q.ctx_mask, B, T, S, q.tokens, st, pr.win ? &route.lookahead : nullptr, sess ? sess->n_keys : T));
    }
    // FP8 self K/V: the rows 0 .. P0 - 2 the prefill stored in every layer's self cache [R, H, T, 64] -> codes + scales; the steps
    // append from position P0 - 1 on (the regeneration after a chain fault reuses these rows)
    if (route.self_kv8 && pr.step0 > 0 && !keep_prefill && !prefill_only) {
        for (int l = 0; l < h->decg.depth; ++l) {
            const Kv8Layer kl = kv8_layer_of(h, gc.self_kv8_buf, R, T, l);
            DIMX_TRY(launch_kv8_quant(h->at, s.sk[l], R, h->decg.heads, tpad(T), pr.step0, kl.kcodes, kl.kscale, st, T));
            DIMX_TRY(launch_kv8_quant(h->at, s.sv[l], R, h->decg.heads, tpad(T), pr.step0, kl.vcodes, kl.vscale, st, T));
        }
    }
    if (prefill_only) return DIMX_OK;
    // FP8 cross K/V: every layer's context K / V -> codes + scales, once per generation, ahead of the first step (the prefill above
    // read the unquantised caches; the regeneration after a chain fault reuses the codes).  A session's pushes quantise the rows
    // they append (stream.hip push_rows): nothing here.
    if (route.kv8 && !keep_prefill && !sess) {
        const int Tp = tpad(T), heads = h->decg.heads;
        for (int l = 0; l < h->decg.depth; ++l) {
            const Kv8Layer kl = kv8_layer_of(h, gc.kv8_buf, B, T, l);
            DIMX_TRY(launch_kv8_quant(h->at, cp.ck[l], B, heads, Tp, T, kl.kcodes, kl.kscale, st));
            DIMX_TRY(launch_kv8_quant(h->at, cp.cv[l], B, heads, Tp, T, kl.vcodes, kl.vscale, st));
        }
    }
    // start
    DIMX_TRY(gen_groups_fork(h, G, st, run.gs));
    for (int g = 0; g < G; ++g) {
        run.ctx[g] = step_ctx(h, gc, route, lo[g], lo[g + 1] - lo[g], g, run.gs[g]);
        if (sess) run.ctx[g].n_keys = sess->n_keys;
        DIMX_TRY(gen_start(run.ctx[g]));
    }
    return DIMX_OK;
}

// the next nsteps steps of every group
int gen_run_steps(dimx_handle h, GenRun& run, int nsteps) {
    const int G = run.G;
    if (!h->use_graph || !run.graphs) {
        for (int t = 0; t < nsteps; ++t)
            for (int g = 0; g < G; ++g) DIMX_TRY(gen_step(run.ctx[g]));
    } else {
        DIMX_TRY(step_graphs_ensure(h, graph_key(h, run.gc, run.route), run.ctx, G, run.n));
        DIMX_TRY(step_graphs_replay(h, nsteps, G, run.gs));
    }
    return DIMX_OK;
}

void gen_run_set_keys(GenRun& run, int n_keys, hipStream_t st) {
    run.ctx[0].n_keys = n_keys;
    run.ctx[0].st = run.gs[0] = st;
}

GenRun* gen_run_new(const int32_t* start, const uint8_t* ctx_mask, int B, int T, float temperature, int top_k, const float* noise,
                    uint64_t seed, int32_t* tokens, float* logits_out, void* ws, size_t ws_bytes, hipStream_t st, int ld_prompt, int P) {
    const GenRequest q{{start, ld_prompt, P, nullptr, P - 1, P > 1}, ctx_mask, B, T, 1, temperature, top_k, noise, seed, tokens, logits_out, ws, ws_bytes, st, nullptr};
    return new GenRun(q);
}
void gen_run_free(GenRun* r) { delete r; }

// One implementation for dimx_generate (pr = {start, 1, 1, NULL, 0}), dimx_generate_prompted and dimx_generate_beam: open, every
// step, join; *ran is the route its steps took.
static int generate_impl(dimx_handle h, const GenRequest& q, bool keep_prefill, bool prefill_only, StepRoute* ran) {
    *ran = StepRoute{};
    GenRun run(q);
    DIMX_TRY(gen_open(h, run, keep_prefill, prefill_only, nullptr));
    if (prefill_only) return DIMX_OK;
    // steps
    DIMX_TRY(gen_run_steps(h, run, run.nrun));
    // route sample_head: every step sampled its predecessor's logits; the last step's go through the plain sampler, once
    if (run.route.sample_head && run.nrun > 0) DIMX_TRY(finish_sample(run.ctx[0], 1));
    // join
    DIMX_TRY(gen_groups_join(h, run.G, q.st, run.gs));
    if (run.route.chain && run.G == 1) {
        DIMX_HIP(hipMemcpyAsync(h->chain_err_host, h->chain_err_dev, 4, hipMemcpyDeviceToHost, q.st));
        DIMX_HIP(hipEventRecord(h->chain_err_ev, q.st));
    }
    *ran = run.route;
    return DIMX_OK;
}

// x-transformers' own parameter ranges; the kernel treats thres >= 1 and min_p = 0 as "keep everything"
int check_sampler_filter(int kind, float a, float b) {
    DIMX_REQUIRE(kind >= DIMX_FILTER_TOP_K && kind <= DIMX_FILTER_TOP_A, DIMX_ERR_ARG, "sampler filter: unknown kind %d", kind);
    if (kind == DIMX_FILTER_TOP_K) return DIMX_OK;
    DIMX_REQUIRE(a == a && (kind != DIMX_FILTER_TOP_A || b == b), DIMX_ERR_ARG, "sampler filter: NaN parameter");
    if (kind == DIMX_FILTER_TOP_P) DIMX_REQUIRE(a >= 0.f, DIMX_ERR_ARG, "sampler filter: top_p thres %g < 0", (double)a);
    if (kind == DIMX_FILTER_MIN_P) DIMX_REQUIRE(a >= 0.f && a <= 1.f, DIMX_ERR_ARG, "sampler filter: min_p %g outside [0, 1]", (double)a);
    if (kind == DIMX_FILTER_TOP_A)
        DIMX_REQUIRE(a >= 0.f && b >= 0.f, DIMX_ERR_ARG, "sampler filter: top_a min_p_pow %g or min_p_ratio %g < 0", (double)a, (double)b);
    return DIMX_OK;
}

}  // namespace dimx

using namespace dimx;

extern "C" {

// DIMX_LAYER_PROF=1 (tuning): the phase stamps of the LAST step's layer launches (100 MHz wall clock), mean / max over blocks
static int print_layer_prof(dimx_handle h) {
    DIMX_HIP(hipEventSynchronize(h->chain_err_ev));
    static const char* names[14] = {"start", "self attention done", "barrier 1", "rows + W1 landed", "out-proj stored", "barrier 2",
                                    "y rows + W2 landed", "cross-q stored", "barrier 3", "cross attention done", "barrier 4",
                                    "rows + W3 landed", "out-proj stored", "head done"};
    static const int order[14] = {0, 13, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};   // the sampling head's stamp (layer 0) is slot 13
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
        for (int k = 0; k < 14; ++k) {
            const int i = order[k];
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
static int generate_checked(dimx_handle h, const GenRequest& q) {
    StepRoute route;
    auto chain_ran = [&] { return route.chain && route.G == 1; };
    DIMX_TRY(generate_impl(h, q, false, false, &route));
    if (h->chain_fault_inject > 0) --h->chain_fault_inject;
    if (!chain_ran()) return DIMX_OK;
    if (h->layer_prof_dev) DIMX_TRY(print_layer_prof(h));
    const int e = take_chain_flags(h, q.st);
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
    DIMX_TRY(generate_impl(h, q, true, false, &route));
    if (!chain_ran()) return DIMX_OK;
    // the regeneration may still have run chain kernels (the bit-2 case keeps them on): it answers for its own flags too
    //  -- a second fault takes the chain path off and regenerates once more on the one-kernel-per-op step
    const int e2 = take_chain_flags(h, q.st);
    if (e2 <= 0) return e2;
    h->use_chain = 0;
    fprintf(stderr, "dimx: the regenerated batch reported chain flags 0x%x again; regenerating on the one-kernel-per-op step, the "
                    "chain path stays off for this handle\n", e2);
    DIMX_TRY(generate_impl(h, q, true, false, &route));
    DIMX_REQUIRE(!chain_ran(), DIMX_ERR_STATE, "generate: the chain path is still active after it was switched off");
    return DIMX_OK;
}

int dimx_generate(dimx_handle h, const int32_t* start, const uint8_t* ctx_mask, int B, int T, int n_samples,
                  float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out,
                  void* ws, size_t ws_bytes, void* stream) {
    const GenRequest q{{start, 1, 1, nullptr, 0}, ctx_mask, B, T, n_samples < 1 ? 1 : n_samples, temperature, top_k, exp_noise, seed,
                       tokens, logits_out, ws, ws_bytes, (hipStream_t)stream, nullptr};
    DIMX_NO_SESSION(h, "generate");
    return generate_checked(h, q);
}

int dimx_generate_prompted(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                           const uint8_t* ctx_mask, int B, int T, int n_samples, float temperature, int top_k,
                           const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out, int flags, void* ws,
                           size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_NO_SESSION(h, "generate_prompted");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "generate_prompted: prompts are implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(prompt && T >= 2 && Pmax >= 1 && Pmax <= T - 1 && ld_prompt >= Pmax, DIMX_ERR_ARG,
                 "generate_prompted: need 1 <= Pmax <= T - 1 and ld_prompt >= Pmax (Pmax=%d T=%d ld_prompt=%d)", Pmax, T, ld_prompt);
    DIMX_REQUIRE(P0 >= 1 && P0 <= Pmax, DIMX_ERR_ARG, "generate_prompted: need 1 <= P0 <= Pmax (P0=%d Pmax=%d)", P0, Pmax);
    DIMX_REQUIRE((flags & ~7) == 0, DIMX_ERR_ARG, "generate_prompted: unknown flags 0x%x", flags);
    const int S = n_samples < 1 ? 1 : n_samples;
    // bit 0: no prefill, the whole prompt goes through forced decode steps.  Online generation (dimx_set_cross_lookahead) too, unless
    // bit 1 asks for the windowed prefill (win_attn.hip): the offline prefill's attention has no per-query key bound
    const bool win_prefill = h->xwin_on && (flags & 2) && !(flags & 1);
    const int p0 = ((flags & 1) || (h->xwin_on && !win_prefill)) ? 1 : P0;
    // bit 2 is not part of the public flag set: tools/bench_prompt.py times the prefill stage alone with it
    DIMX_REQUIRE(!(flags & 4) || p0 >= 2, DIMX_ERR_ARG, "generate_prompted: flags bit 2 (the prefill stage alone) without a prefill (P0=%d, flags 0x%x)",
                 P0, flags);
    DIMX_REQUIRE(p0 == 1 || h->decg.dim_head == 64, DIMX_ERR_ARG, "generate_prompted: the prefill needs 64-wide heads");
    DIMX_REQUIRE(B >= 1 && T <= h->d.max_seq_len, DIMX_ERR_ARG, "B=%d T=%d out of range (T <= %d)", B, T, h->d.max_seq_len);
    const size_t need = workspace_bytes_prompt(h, B, T, S, p0);
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "generate_prompted: workspace %zu < required %zu (dimx_workspace_bytes_prompt)",
                 ws_bytes, need);
    const GenRequest q{{prompt, ld_prompt, Pmax, prompt_len, p0 - 1, win_prefill && p0 >= 2}, ctx_mask, B, T, S, temperature, top_k, exp_noise, seed,
                       tokens, logits_out, ws, ws_bytes, (hipStream_t)stream, nullptr};
    if (flags & 4) {   // the prefill stage alone, nothing is generated
        StepRoute route;
        return generate_impl(h, q, false, true, &route);
    }
    return generate_checked(h, q);
}

int dimx_generate_guided(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, const uint8_t* ctx_mask,
                         int B, int T, float scale, float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens,
                         float* logits_out, float* branch_logits_out, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_NO_SESSION(h, "generate_guided");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "generate_guided: guidance is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(scale - scale == 0.f, DIMX_ERR_ARG, "generate_guided: the scale is NaN or infinite");
    DIMX_REQUIRE(prompt && T >= 2 && Pmax >= 1 && Pmax <= T - 1 && ld_prompt >= Pmax, DIMX_ERR_ARG,
                 "generate_guided: need 1 <= Pmax <= T - 1 and ld_prompt >= Pmax (Pmax=%d T=%d ld_prompt=%d)", Pmax, T, ld_prompt);
    DIMX_REQUIRE(B >= 1 && T <= h->d.max_seq_len, DIMX_ERR_ARG, "B=%d T=%d out of range (T <= %d)", B, T, h->d.max_seq_len);
    const size_t need = dimx_workspace_bytes_guided(h, B, T);
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "generate_guided: workspace %zu < required %zu (dimx_workspace_bytes_guided)", ws_bytes, need);
    // the whole prompt goes through forced decode steps (P0 = 1): both halves then see the same tokens by the same launches
    GenRequest q{{prompt, ld_prompt, Pmax, prompt_len, 0}, ctx_mask, B, T, 1, temperature, top_k, exp_noise, seed,
                 tokens, logits_out, ws, ws_bytes, (hipStream_t)stream, nullptr};
    q.guided = true;
    q.scale = scale;
    q.branch_out = branch_logits_out;
    return generate_checked(h, q);
}

int dimx_generate_beam(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                       const uint8_t* ctx_mask, const int32_t* lens, int B, int T, int beam_width, int32_t* tokens, double* scores,
                       int32_t* backptr, float* logits_out, void* beam_state, size_t beam_state_bytes, int flags, void* ws, size_t ws_bytes,
                       void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_NO_SESSION(h, "generate_beam");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "generate_beam: beam search is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(!h->xwin_on, DIMX_ERR_ARG, "generate_beam: not available while the cross-attention window is on (dimx_set_cross_lookahead)");
    DIMX_REQUIRE(beam_width_supported(beam_width), DIMX_ERR_ARG, "generate_beam: beam_width %d not in {1,2,4,5,8,10}", beam_width);
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
    const size_t need = workspace_bytes_prompt(h, B, T, beam_width, p0);
    DIMX_REQUIRE(ws_bytes >= need, DIMX_ERR_WORKSPACE, "generate_beam: workspace %zu < required %zu (dimx_workspace_bytes_prompt)", ws_bytes, need);
    BeamCall bm;
    bm.cum = (double*)beam_state;
    bm.parent = (int32_t*)((double*)beam_state + R);
    bm.backptr = backptr;
    bm.lens = lens;
    const GenRequest q{{prompt, ld_prompt, Pmax, prompt_len, p0 - 1}, ctx_mask, B, T, beam_width, 0.f, 0, nullptr, 0,
                       tokens, logits_out, ws, ws_bytes, (hipStream_t)stream, &bm};
    DIMX_TRY(generate_checked(h, q));
    DIMX_HIP(hipMemcpyAsync(scores, bm.cum, R * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
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
    DIMX_NO_SESSION(h, "set_cross_lookahead");
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

size_t dimx_cross_kv8_bytes(dimx_handle h, int B, int T) { return kv8_bytes(h, B, T); }

int dimx_set_cross_kv8(dimx_handle h, void* buf, size_t bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_NO_SESSION(h, "set_cross_kv8");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_cross_kv8: FP8 cross K/V is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(buf == nullptr || (h->decg.dim_head == 64 && (uintptr_t)buf % 256 == 0), DIMX_ERR_ARG,
                 "set_cross_kv8: the buffer must be 256-byte aligned and the decoder's heads 64 wide");
    h->kv8_buf = buf;
    h->kv8_bytes = buf ? bytes : 0;
    return DIMX_OK;
}

int dimx_cross_kv8(dimx_handle h, void** buf, size_t* bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (buf) *buf = h->kv8_buf;
    if (bytes) *bytes = h->kv8_bytes;
    return DIMX_OK;
}

int dimx_set_cross_kv8_samples(dimx_handle h, int on) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "set_cross_kv8_samples: null handle");
    DIMX_NO_SESSION(h, "set_cross_kv8_samples");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_cross_kv8_samples: FP8 cross K/V is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    h->kv8_samples_on = on ? 1 : 0;
    return DIMX_OK;
}

int dimx_cross_kv8_samples(dimx_handle h, int* on) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "cross_kv8_samples: null handle");
    if (on) *on = h->kv8_samples_on;
    return DIMX_OK;
}

int dimx_set_beam_kv8(dimx_handle h, int on) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "set_beam_kv8: null handle");
    DIMX_NO_SESSION(h, "set_beam_kv8");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_beam_kv8: FP8 K/V is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    h->beam_kv8_on = on ? 1 : 0;
    return DIMX_OK;
}

int dimx_beam_kv8(dimx_handle h, int* on) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "beam_kv8: null handle");
    if (on) *on = h->beam_kv8_on;
    return DIMX_OK;
}

size_t dimx_self_kv8_bytes(dimx_handle h, int R, int T) { return kv8_bytes(h, R, T); }

int dimx_set_self_kv8(dimx_handle h, void* buf, size_t bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_NO_SESSION(h, "set_self_kv8");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "set_self_kv8: FP8 self K/V is implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(buf == nullptr || (h->decg.dim_head == 64 && (uintptr_t)buf % 256 == 0), DIMX_ERR_ARG,
                 "set_self_kv8: the buffer must be 256-byte aligned and the decoder's heads 64 wide");
    h->self_kv8_buf = buf;
    h->self_kv8_bytes = buf ? bytes : 0;
    return DIMX_OK;
}

int dimx_self_kv8(dimx_handle h, void** buf, size_t* bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (buf) *buf = h->self_kv8_buf;
    if (bytes) *bytes = h->self_kv8_bytes;
    return DIMX_OK;
}

int dimx_chain_faults(dimx_handle h) { return h ? h->chain_faults : 0; }
int dimx_qkv0_table_builds(dimx_handle h) { return h ? h->qkv0_builds : 0; }
int dimx_kv0_table_generations(dimx_handle h) { return h ? h->kv0_generations : 0; }
int dimx_sample_head_generations(dimx_handle h) { return h ? h->sample_head_generations : 0; }

int dimx_debug_chain_fault(dimx_handle h, int n_calls) {
    DIMX_REQUIRE(h && n_calls >= 0, DIMX_ERR_ARG, "debug_chain_fault: bad argument");
    h->chain_fault_inject = n_calls;
    h->graph_valid = false;
    return DIMX_OK;
}

}  // extern "C"
