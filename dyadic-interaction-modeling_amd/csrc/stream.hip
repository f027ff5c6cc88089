// stream.hip -- streaming sessions of libdimx_hip: speaker frames arrive in pieces, listener tokens leave as soon as they are due.
//
// A session is one logical dimx_generate under the cross-attention window (dimx_set_cross_lookahead) whose context
// is built while it runs.  A push of c frames (dimx_stream_push)
//   1. runs both causal speaker encoders on the c new rows alone, every layer's self attention over that layer's K / V cache
//      (stream_attn.hip, append attention) -- row j of a causal encoder depends on the frames <= j only, so these are the rows
//      dimx_encode_ctx computes for the whole clip;
//   2. appends the new context rows' cross K / V to the [B, H, Tp, 64] caches the decode step reads -- and, under
//      dimx_stream_set_kv8, quantises those rows into the session's FP8 buffer in one launch (launch_kv8_append);
//   3. runs the decode steps that are now due (dimx/stream.py steps_due): step t as soon as the frames 0 .. t + 1 + max(L, 0)
//      exist.  The window bounds every read below the frames pushed.
// dimx_stream_end fixes T = the frames pushed and runs the remaining steps with the key bound T.
//
// dimx_stream_begin_prompted opens a session in the state another one was in after F frames: the encoder increments and the K / V
// append of the F given frames, one windowed prefill (generate.hip gen_prefill, win_attn.hip) over the positions 0 .. P - 2 of the
// P given codes, and the step counter at P - 1.  Its generate part is sized with the prefill scratch for Tmax - 1 positions.
//
// The generation is generate.hip's (gen_open / gen_run_steps): the same start, step and sampler launches, on the per-op route.
// The session's workspace is a dimx_generate workspace for (B, Tmax) followed by the session's own buffers.
#include "stages.hpp"

namespace dimx {

// the buffers of an encoder increment of at most B * kAppendMaxRows rows
struct IncScratch : BlockBufs {
    void* xa;              // padded encoder input, the first stack's output, then the context rows
    float *tmp, *xs, *qkv;
    float *vs, *va;        // a sub-chunk's speaker / audio rows gathered from a push of more than kAppendMaxRows frames
};

struct StreamSession {
    int B = 0, Tmax = 0, lookahead = 0;
    int frames = 0, steps = 0;
    void* ws = nullptr;
    size_t gen_bytes = 0;
    GenRun* run = nullptr;
    CtxPersist cp;
    int32_t *start = nullptr, *tokens = nullptr;
    uint8_t* mask = nullptr;
    float* logits = nullptr;
    void *ek[2][8], *ev[2][8];   // the per-layer K / V caches of encoder_s / encoder_joint, [B, H, Tmax, 64] in the operand type
    IncScratch inc;
    void *kv8_buf = nullptr, *self_kv8_buf = nullptr;   // dimx_stream_set_kv8 as it stood at the begin: the session's FP8 buffers or nullptr
    hipEvent_t evt[4] = {};       // dimx_stream_set_events: recorded by every push at its start and after each of its three parts
};

// prompted: with the prefill scratch of the longest prompt a session of Tmax frames can start from
static size_t gen_part_bytes(const dimx_ctx* c, int B, int Tmax, bool prompted = false) {
    return align_up(workspace_bytes_prompt(c, B, Tmax, 1, prompted ? Tmax : 1), 256);
}

// the session's own buffers behind the generate workspace; base == nullptr sizes them.  prompted: `start` holds [B, Tmax] codes
static size_t plan_stream(const dimx_ctx* c, void* base, size_t cap, int B, int Tmax, StreamSession& s, bool prompted = false) {
    Arena ar(base, cap);
    const size_t es = es_of(c);
    const int n = Tmax - 1, V = c->decg.num_tokens;
    s.start = (int32_t*)ar.take((size_t)B * (prompted ? Tmax : 1) * 4);
    s.mask = (uint8_t*)ar.take((size_t)B * Tmax);
    s.tokens = (int32_t*)ar.take((size_t)B * n * 4);
    s.logits = (float*)ar.take((size_t)B * n * V * 4);
    for (int w = 0; w < 2; ++w) {
        const EncGeom& eg = c->encg[w];
        const size_t per = (size_t)B * eg.heads * Tmax * 64 * es;
        for (int l = 0; l < eg.depth; ++l) {
            s.ek[w][l] = ar.take(per);
            s.ev[w][l] = ar.take(per);
        }
    }
    const EncGeom& eg = c->encg[0];
    const size_t M = (size_t)B * kAppendMaxRows;
    const int dim = eg.dim, inner = eg.heads * eg.dim_head;
    int wide = c->decg.ctx_dim > eg.in_pad ? c->decg.ctx_dim : eg.in_pad;
    wide = wide > dim ? wide : dim;
    IncScratch& i = s.inc;
    i.xa = ar.take(M * wide * es);
    i.h = (float*)ar.take(M * dim * 4);
    i.tmp = (float*)ar.take(M * dim * 4);
    i.xs = (float*)ar.take(M * dim * 4);
    i.y = ar.take(M * dim * es);
    i.qkv = (float*)ar.take(M * 3 * inner * 4);
    i.o = ar.take(M * inner * es);
    i.f = ar.take(M * dim * eg.ff_mult * es);
    i.vs = (float*)ar.take(M * c->d.dim_in * 4);
    i.va = (float*)ar.take(M * c->d.dim_a * 4);
    i.q = i.k = i.vt = nullptr;
    return align_up(ar.off, 256);
}

static bool stream_shape_ok(const dimx_ctx* c, int B, int Tmax) {
    return c && c->variant == 0 && B >= 1 && Tmax >= 2 && Tmax <= 2048 && Tmax <= c->d.max_seq_len;
}

// One causal encoder stack on the c new rows of every clip (run_xenc of model.hip at M = B * c, the attention over the cache)
static int enc_increment(dimx_handle h, const EncGeom& eg, const XEnc& e, const void* x_in, int ld_in, IncScratch& s, void* const* kc,
                         void* const* vc, int B, int c, int n0, int Tmax, int out_dtype, void* out, hipStream_t st) {
    const int M = B * c, dim = eg.dim, heads = eg.heads, inner = eg.heads * eg.dim_head;
    GemmArgs g;
    gemm_lin(h, x_in, ld_in, e.proj_in, M, g);
    g.out_dtype = DIMX_F32;
    g.rowT = c;
    g.rowadd = e.pos_emb + (size_t)n0 * dim;   // row i of a clip is position n0 + i
    g.ld_rowadd = dim;
    g.rowadd_mode = 1;
    g.rowadd_scale = 1.0f / sqrtf((float)dim);
    gemm_set_plain_out(g, s.h, dim);
    DIMX_TRY(launch_gemm(g, st));
    for (int l = 0; l < eg.depth; ++l) {
        DIMX_TRY(launch_layernorm(h->at, s.h, s.y, e.attn[l].ln_g, nullptr, M, dim, st));
        DIMX_TRY(linear(h, s.y, dim, e.attn[l].qkv, M, DIMX_F32, s.qkv, 3 * inner, st));
        AppendAttnArgs a;
        a.dtype = h->at;
        a.q = s.qkv; a.k = s.qkv + inner; a.v = s.qkv + 2 * inner; a.ld = 3 * inner;
        a.kcache = kc[l]; a.vcache = vc[l]; a.Tmax = Tmax;
        a.out = s.o; a.o_ld = inner;
        a.B = B; a.H = heads; a.n0 = n0; a.c = c;
        a.scale = 1.0f / sqrtf((float)eg.dim_head);
        DIMX_TRY(launch_append_attn(a, st));
        DIMX_TRY(residual_linear(h, s.o, inner, e.attn[l].out, M, s.h, dim, st));
        DIMX_TRY(ff_sublayer(h, s, e.ff[l].ln_g, nullptr, e.ff[l].f1, e.ff[l].f2, e.ff[l].mlp, ACT_GELU_ERF, M, dim, st));
    }
    return launch_layernorm(out_dtype, s.h, out, e.final_g, nullptr, M, dim, st);
}

// Rows [n0, n0 + c) of every clip: both encoders, norm_s, the context rows and their cross K / V in every decoder layer's cache.
// vs / va: the c rows of clip b at vs + b * ld_rows * width; xs_out as they are, or nullptr.
static int push_rows(dimx_handle h, StreamSession& S, const float* vs, const float* va, int ld_rows, int c, int n0, float* xs_out,
                     hipStream_t st) {
    const int B = S.B, M = B * c, dim = h->d.dim, dim_a = h->d.dim_a, dim_in = h->d.dim_in;
    IncScratch& s = S.inc;
    if (ld_rows != c) {   // a sub-chunk of a longer push: gather its rows
        DIMX_HIP(hipMemcpy2DAsync(s.vs, (size_t)c * dim_in * 4, vs, (size_t)ld_rows * dim_in * 4, (size_t)c * dim_in * 4, B, hipMemcpyDeviceToDevice, st));
        DIMX_HIP(hipMemcpy2DAsync(s.va, (size_t)c * dim_a * 4, va, (size_t)ld_rows * dim_a * 4, (size_t)c * dim_a * 4, B, hipMemcpyDeviceToDevice, st));
        vs = s.vs;
        va = s.va;
    }
    const int in_pad = h->encg[0].in_pad;
    DIMX_TRY(launch_cast_pad(h->at, vs, dim_in, h->patch_s, s.xa, in_pad, M, dim_in, st));
    DIMX_TRY(enc_increment(h, h->encg[0], h->enc_s, s.xa, in_pad, s, S.ek[0], S.ev[0], B, c, n0, S.Tmax, h->at, s.xa, st));
    DIMX_TRY(enc_increment(h, h->encg[1], h->enc_joint, s.xa, dim, s, S.ek[1], S.ev[1], B, c, n0, S.Tmax, DIMX_F32, s.tmp, st));
    float* x_s = xs_out && ld_rows == c ? xs_out : s.xs;
    DIMX_TRY(launch_layernorm(DIMX_F32, s.tmp, x_s, h->norm_s_g, h->norm_s_b, M, dim, st));
    if (xs_out && x_s != xs_out)
        DIMX_HIP(hipMemcpy2DAsync(xs_out, (size_t)ld_rows * dim * 4, x_s, (size_t)c * dim * 4, (size_t)c * dim * 4, B, hipMemcpyDeviceToDevice, st));
    if (S.evt[1]) DIMX_HIP(hipEventRecord(S.evt[1], st));
    DIMX_TRY(launch_context_concat(h->at, x_s, h->patch_dec_s, va, s.xa, M, dim, dim_a, st));
    // project_cross_kv's per-layer segment form, its base moved to row n0 and c rows per clip
    const int D = h->decg.dim_head, heads = h->decg.heads, Tp = tpad(S.Tmax);
    const size_t es = es_of(h);
    for (int l = 0; l < h->decg.depth; ++l) {
        GemmArgs g;
        gemm_lin(h, s.xa, h->decg.ctx_dim, h->dec.cross[l].kv, M, g);
        g.out_dtype = h->at;
        g.rowT = c;
        g.nseg = 2;
        g.seg_width = heads * D;
        for (int i = 0; i < 2; ++i) {
            g.seg[i].ptr = (unsigned char*)(i == 0 ? S.cp.ck[l] : S.cp.cv[l]) + (size_t)n0 * D * es;
            g.seg[i].sb = (long)heads * Tp * D;
            g.seg[i].sh = (long)Tp * D;
            g.seg[i].st = D;
            g.seg[i].sd = 1;
            g.seg[i].D = D;
        }
        DIMX_TRY(launch_gemm(g, st));
    }
    // FP8 cross K/V (dimx_stream_set_kv8): the rows just appended -> codes + scales, K and V of every layer in one launch.  A row's
    // codes are a function of that row alone (dimx/kv8.py append), so the buffer holds what quantising the finished caches would.
    if (S.kv8_buf) {
        Kv8AppendArgs a;
        memset(&a, 0, sizeof(a));
        for (int l = 0; l < h->decg.depth; ++l) {
            const Kv8Layer kl = kv8_layer_of(h, S.kv8_buf, B, S.Tmax, l);
            a.cache[2 * l] = S.cp.ck[l]; a.codes[2 * l] = kl.kcodes; a.scales[2 * l] = kl.kscale;
            a.cache[2 * l + 1] = S.cp.cv[l]; a.codes[2 * l + 1] = kl.vcodes; a.scales[2 * l + 1] = kl.vscale;
        }
        a.dtype = h->at; a.depth = h->decg.depth; a.B = B; a.H = heads; a.Tc = Tp; a.Tp = Tp; a.n0 = n0; a.c = c;
        DIMX_TRY(launch_kv8_append(a, st));
    }
    return DIMX_OK;
}

// decode steps that must have run once n frames are pushed (dimx/stream.py steps_due, the open form)
static int steps_due_open(int n, int lookahead) {
    const int L = lookahead > 0 ? lookahead : 0;
    const long v = (long)n - 1 - L;
    const int hi = n - 1 > 0 ? n - 1 : 0;
    return v < 0 ? 0 : (v > hi ? hi : (int)v);
}

// run the steps up to `due` and hand their token (and logit) columns to the caller
static int run_and_copy(dimx_handle h, StreamSession& S, int due, int n_keys, int32_t* tokens_out, int ld_tok, float* logits_out, int* n_new,
                        hipStream_t st) {
    const int done = S.steps, nn = due - done, n = S.Tmax - 1, V = h->decg.num_tokens;
    *n_new = nn;
    if (nn <= 0) return DIMX_OK;
    gen_run_set_keys(*S.run, n_keys, st);
    DIMX_TRY(gen_run_steps(h, *S.run, nn));
    S.steps = due;
    DIMX_HIP(hipMemcpy2DAsync(tokens_out + done, (size_t)ld_tok * 4, S.tokens + done, (size_t)n * 4, (size_t)nn * 4, S.B, hipMemcpyDeviceToDevice, st));
    if (logits_out)
        DIMX_HIP(hipMemcpy2DAsync(logits_out + (size_t)done * V, (size_t)ld_tok * V * 4, S.logits + (size_t)done * V, (size_t)n * V * 4,
                                  (size_t)nn * V * 4, S.B, hipMemcpyDeviceToDevice, st));
    return DIMX_OK;
}

static void close_session(dimx_ctx* h) {
    StreamSession* S = (StreamSession*)h->stream_sess;
    if (!S) return;
    gen_run_free(S->run);
    delete S;
    h->stream_sess = nullptr;
}

void stream_forget(dimx_ctx* h) { close_session(h); }

}  // namespace dimx

using namespace dimx;

extern "C" {

size_t dimx_stream_workspace_bytes(dimx_handle h, int B, int Tmax) {
    if (!stream_shape_ok(h, B, Tmax)) return 0;   // 0 = shape not supported
    StreamSession s;
    return gen_part_bytes(h, B, Tmax) + plan_stream(h, nullptr, 0, B, Tmax, s);
}

// dimx_stream_begin (P = 1, F = 0: `prompt` is start [B]) and dimx_stream_begin_prompted.  Every check comes before the first launch.
static int stream_open(dimx_handle h, const char* what, bool prompted, const int32_t* prompt, int ld_prompt, int P, const float* v_speaker,
                       const float* v_audio, int F, int B, int Tmax, int lookahead, float temperature, int top_k, const float* noise,
                       uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(!h->stream_sess, DIMX_ERR_STATE, "%s: a session is already open on this handle", what);
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "%s: sessions are implemented for variant 0 (SLMFT) only; this handle is variant %d", what,
                 h->variant);
    DIMX_REQUIRE(B >= 1 && Tmax >= 2 && Tmax <= 2048 && Tmax <= h->d.max_seq_len, DIMX_ERR_ARG,
                 "%s: B=%d Tmax=%d out of range (2 <= Tmax <= %d)", what, B, Tmax, h->d.max_seq_len < 2048 ? h->d.max_seq_len : 2048);
    DIMX_REQUIRE(prompt, DIMX_ERR_ARG, "%s: null start tokens", what);
    if (prompted) {
        DIMX_REQUIRE(v_speaker && v_audio, DIMX_ERR_ARG, "%s: null frames", what);
        // teacher-forced row P - 2 reads the keys below P + lookahead: they must be among the F frames given (dimx/stream.py prompt_fits)
        DIMX_REQUIRE(P >= 1 && F <= Tmax && (long)P + (lookahead > 0 ? lookahead : 0) <= (long)F && ld_prompt >= P, DIMX_ERR_ARG,
                     "%s: need 1 <= P, P + max(lookahead, 0) <= F <= Tmax and ld_prompt >= P (P=%d lookahead=%d F=%d Tmax=%d ld_prompt=%d)", what,
                     P, lookahead, F, Tmax, ld_prompt);
    }
    DIMX_REQUIRE(h->encg[0].causal && h->encg[1].causal && h->encg[0].dim_head == 64 && h->encg[1].dim_head == 64 && h->decg.dim_head == 64 &&
                     h->encg[0].dim == h->encg[1].dim && h->encg[0].heads == h->encg[1].heads && h->encg[0].depth <= 8 && h->encg[1].depth <= 8,
                 DIMX_ERR_ARG, "%s: needs causal encoders of one width with 64-wide heads", what);
    // dimx_stream_set_kv8: the buffers against this session's shape (self: one sequence per clip)
    if (h->stream_kv8_buf || h->stream_self_kv8_buf) {
        const size_t need = kv8_bytes(h, B, Tmax);
        DIMX_REQUIRE(need != 0 && h->decg.depth <= 8, DIMX_ERR_ARG, "%s: B=%d Tmax=%d is not supported with dimx_stream_set_kv8", what, B, Tmax);
        DIMX_REQUIRE(!h->stream_kv8_buf || h->stream_kv8_bytes >= need, DIMX_ERR_WORKSPACE,
                     "%s: the FP8 cross K/V buffer holds %zu bytes, B=%d Tmax=%d needs %zu (dimx_cross_kv8_bytes)", what, h->stream_kv8_bytes, B, Tmax,
                     need);
        DIMX_REQUIRE(!h->stream_self_kv8_buf || h->stream_self_kv8_bytes >= need, DIMX_ERR_WORKSPACE,
                     "%s: the FP8 self K/V buffer holds %zu bytes, B=%d Tmax=%d needs %zu (dimx_self_kv8_bytes)", what, h->stream_self_kv8_bytes, B,
                     Tmax, need);
    }
    const size_t gen_bytes = gen_part_bytes(h, B, Tmax, prompted);
    StreamSession* S = new StreamSession;
    const size_t own = plan_stream(h, nullptr, 0, B, Tmax, *S, prompted);
    if (ws_bytes < gen_bytes + own) {
        delete S;
        DIMX_REQUIRE(false, DIMX_ERR_WORKSPACE, "%s: workspace %zu < required %zu (%s)", what, ws_bytes, gen_bytes + own,
                     prompted ? "dimx_stream_workspace_bytes_prompt" : "dimx_stream_workspace_bytes");
    }
    const int rc = [&]() -> int {
        DIMX_TRY(check_common(h, B, Tmax, ws, gen_bytes, COMP_ENC | COMP_DEC));
        hipStream_t st = (hipStream_t)stream;
        plan_stream(h, (unsigned char*)ws + gen_bytes, ws_bytes - gen_bytes, B, Tmax, *S, prompted);
        S->B = B; S->Tmax = Tmax; S->lookahead = lookahead; S->ws = ws; S->gen_bytes = gen_bytes;
        S->kv8_buf = h->stream_kv8_buf; S->self_kv8_buf = h->stream_self_kv8_buf;
        (void)scratch_arena(h, ws, gen_bytes, B, Tmax, &S->cp);
        DIMX_HIP(hipMemsetAsync(S->mask, 1, (size_t)B * Tmax, st));   // every pushed frame is a context row
        const int ld = prompted ? Tmax : 1;
        if (prompted)
            DIMX_HIP(hipMemcpy2DAsync(S->start, (size_t)ld * 4, prompt, (size_t)ld_prompt * 4, (size_t)P * 4, B, hipMemcpyDeviceToDevice, st));
        else
            DIMX_HIP(hipMemcpyAsync(S->start, prompt, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
        // the given frames: the encoder increments and the K / V append of a push of F frames
        const int dim_in = h->d.dim_in, dim_a = h->d.dim_a;
        for (int o = 0; o < F; o += kAppendMaxRows) {
            const int cc = F - o < kAppendMaxRows ? F - o : kAppendMaxRows;
            DIMX_TRY(push_rows(h, *S, v_speaker + (size_t)o * dim_in, v_audio + (size_t)o * dim_a, F, cc, o, nullptr, st));
        }
        S->frames = F;
        S->run = gen_run_new(S->start, S->mask, B, Tmax, temperature, top_k, noise, seed, S->tokens, S->logits, ws, gen_bytes, st, ld, P);
        const GenSessionSpec spec{lookahead, Tmax, S->kv8_buf, S->self_kv8_buf};
        DIMX_TRY(gen_open(h, *S->run, false, false, &spec));   // P > 1: with the windowed prefill of the positions 0 .. P - 2
        S->steps = P - 1;
        return DIMX_OK;
    }();
    if (rc != DIMX_OK) {
        gen_run_free(S->run);
        delete S;
        return rc;
    }
    if (h->ctx_ws == ws) h->ctx_ready = false;   // the session's caches replace a context built in the same workspace
    h->stream_sess = S;
    return DIMX_OK;
}

int dimx_stream_begin(dimx_handle h, const int32_t* start, int B, int Tmax, int lookahead, float temperature, int top_k, const float* noise,
                      uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    return stream_open(h, "stream_begin", false, start, 1, 1, nullptr, nullptr, 0, B, Tmax, lookahead, temperature, top_k, noise, seed, ws,
                       ws_bytes, stream);
}

size_t dimx_stream_workspace_bytes_prompt(dimx_handle h, int B, int Tmax) {
    if (!stream_shape_ok(h, B, Tmax)) return 0;   // 0 = shape not supported
    StreamSession s;
    return gen_part_bytes(h, B, Tmax, true) + plan_stream(h, nullptr, 0, B, Tmax, s, true);
}

int dimx_stream_begin_prompted(dimx_handle h, const int32_t* prompt, int ld_prompt, int P, const float* v_speaker, const float* v_audio, int F,
                               int B, int Tmax, int lookahead, float temperature, int top_k, const float* noise, uint64_t seed, void* ws,
                               size_t ws_bytes, void* stream) {
    return stream_open(h, "stream_begin_prompted", true, prompt, ld_prompt, P, v_speaker, v_audio, F, B, Tmax, lookahead, temperature, top_k,
                       noise, seed, ws, ws_bytes, stream);
}

int dimx_stream_push(dimx_handle h, const float* v_speaker, const float* v_audio, int c, int32_t* tokens_out, int ld_tok, float* logits_out,
                     float* x_s_out, int* n_new, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (n_new) *n_new = 0;
    DIMX_REQUIRE(h->stream_sess, DIMX_ERR_STATE, "stream_push: no open session (dimx_stream_begin first; dimx_stream_end closes it)");
    StreamSession& S = *(StreamSession*)h->stream_sess;
    DIMX_REQUIRE(c >= 1, DIMX_ERR_ARG, "stream_push: c=%d frames", c);
    DIMX_REQUIRE(S.frames + c <= S.Tmax, DIMX_ERR_ARG, "stream_push: %d + %d frames exceed the session's Tmax %d", S.frames, c, S.Tmax);
    DIMX_REQUIRE(v_speaker && v_audio && tokens_out && n_new, DIMX_ERR_ARG, "stream_push: null argument");
    const int due = steps_due_open(S.frames + c, S.lookahead);
    DIMX_REQUIRE(ld_tok >= due, DIMX_ERR_ARG, "stream_push: ld_tok %d < %d token columns", ld_tok, due);
    DIMX_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int dim = h->d.dim, dim_a = h->d.dim_a, dim_in = h->d.dim_in;
    if (S.evt[0]) DIMX_HIP(hipEventRecord(S.evt[0], st));
    for (int o = 0; o < c; o += kAppendMaxRows) {
        const int cc = c - o < kAppendMaxRows ? c - o : kAppendMaxRows;
        DIMX_TRY(push_rows(h, S, v_speaker + (size_t)o * dim_in, v_audio + (size_t)o * dim_a, c, cc, S.frames + o,
                           x_s_out ? x_s_out + (size_t)o * dim : nullptr, st));
    }
    S.frames += c;
    if (S.evt[2]) DIMX_HIP(hipEventRecord(S.evt[2], st));
    DIMX_TRY(run_and_copy(h, S, due, S.Tmax, tokens_out, ld_tok, logits_out, n_new, st));
    if (S.evt[3]) DIMX_HIP(hipEventRecord(S.evt[3], st));
    return DIMX_OK;
}

int dimx_stream_set_events(dimx_handle h, void* ev_start, void* ev_encoded, void* ev_appended, void* ev_stepped) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    DIMX_REQUIRE(h->stream_sess, DIMX_ERR_STATE, "stream_set_events: no open session");
    StreamSession& S = *(StreamSession*)h->stream_sess;
    S.evt[0] = (hipEvent_t)ev_start; S.evt[1] = (hipEvent_t)ev_encoded; S.evt[2] = (hipEvent_t)ev_appended; S.evt[3] = (hipEvent_t)ev_stepped;
    return DIMX_OK;
}

int dimx_stream_end(dimx_handle h, int32_t* tokens_out, int ld_tok, float* logits_out, int* n_new, void* stream) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    if (n_new) *n_new = 0;
    DIMX_REQUIRE(h->stream_sess, DIMX_ERR_STATE, "stream_end: no open session");
    StreamSession& S = *(StreamSession*)h->stream_sess;
    DIMX_REQUIRE(tokens_out && n_new, DIMX_ERR_ARG, "stream_end: null argument");
    DIMX_REQUIRE(S.frames >= 2, DIMX_ERR_ARG, "stream_end: %d frames pushed, a clip has at least 2 (dimx_stream_abort drops the session)", S.frames);
    DIMX_REQUIRE(ld_tok >= S.frames - 1, DIMX_ERR_ARG, "stream_end: ld_tok %d < %d token columns", ld_tok, S.frames - 1);
    DIMX_HIP(hipSetDevice(h->device));
    const int rc = run_and_copy(h, S, S.frames - 1, S.frames, tokens_out, ld_tok, logits_out, n_new, (hipStream_t)stream);
    close_session(h);
    return rc;
}

int dimx_stream_abort(dimx_handle h) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    close_session(h);
    return DIMX_OK;
}

int dimx_stream_set_kv8(dimx_handle h, void* cross_buf, size_t cross_bytes, void* self_buf, size_t self_bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "stream_set_kv8: null handle");
    DIMX_NO_SESSION(h, "stream_set_kv8");
    DIMX_REQUIRE(h->variant == 0, DIMX_ERR_ARG, "stream_set_kv8: sessions are implemented for variant 0 (SLMFT) only; this handle is variant %d",
                 h->variant);
    DIMX_REQUIRE(((uintptr_t)cross_buf | (uintptr_t)self_buf) % 256 == 0 && h->decg.dim_head == 64, DIMX_ERR_ARG,
                 "stream_set_kv8: the buffers must be 256-byte aligned and the decoder's heads 64 wide");
    h->stream_kv8_buf = cross_buf;
    h->stream_kv8_bytes = cross_buf ? cross_bytes : 0;
    h->stream_self_kv8_buf = self_buf;
    h->stream_self_kv8_bytes = self_buf ? self_bytes : 0;
    return DIMX_OK;
}

int dimx_stream_kv8(dimx_handle h, void** cross_buf, size_t* cross_bytes, void** self_buf, size_t* self_bytes) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "stream_kv8: null handle");
    if (cross_buf) *cross_buf = h->stream_kv8_buf;
    if (cross_bytes) *cross_bytes = h->stream_kv8_bytes;
    if (self_buf) *self_buf = h->stream_self_kv8_buf;
    if (self_bytes) *self_bytes = h->stream_self_kv8_bytes;
    return DIMX_OK;
}

int dimx_stream_cross_kv(dimx_handle h, int layer, void** k, void** v) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "stream_cross_kv: null handle");
    DIMX_REQUIRE(h->stream_sess, DIMX_ERR_STATE, "stream_cross_kv: no open session");
    DIMX_REQUIRE(layer >= 0 && layer < h->decg.depth && layer < 8, DIMX_ERR_ARG, "stream_cross_kv: layer %d of %d", layer, h->decg.depth);
    const StreamSession& S = *(const StreamSession*)h->stream_sess;
    if (k) *k = S.cp.ck[layer];
    if (v) *v = S.cp.cv[layer];
    return DIMX_OK;
}

int dimx_stream_state(dimx_handle h, int* frames, int* steps, int* open) {
    DIMX_REQUIRE(h, DIMX_ERR_ARG, "null handle");
    const StreamSession* S = (const StreamSession*)h->stream_sess;
    if (frames) *frames = S ? S->frames : 0;
    if (steps) *steps = S ? S->steps : 0;
    if (open) *open = S ? 1 : 0;
    return DIMX_OK;
}

}  // extern "C"
