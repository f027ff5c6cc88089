// ops.hip -- the kernel-level entry points of libdimx_hip (dimx_op_*, dimx_mlp_fused_pack): one kernel or launcher each, for the
// unit tests and the tuning tools; no handle.
#include "stages.hpp"

using namespace dimx;

extern "C" {

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

}  // extern "C"

/* the GemmArgs of dimx_op_gemm_map / dimx_op_gemm_route: dimx_op_gemm's fields plus the output map and the row add */
static int gemm_map_args(GemmArgs& g, int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                         const float* bias, int act, const float* residual, int ldr, int rowT, int nseg, void* const* seg_ptr,
                         const int64_t* seg_strides, const int32_t* seg_D, const float* rowadd, int ld_rowadd, int rowadd_mode,
                         float rowadd_scale, int rowadd_off, int rowadd_div, int flags) {
    DIMX_REQUIRE(A && W && seg_ptr && seg_strides && seg_D, DIMX_ERR_ARG, "op_gemm_map: null operand or map");
    DIMX_REQUIRE(M > 0 && N > 0 && K > 0 && rowT >= 1, DIMX_ERR_ARG, "op_gemm_map: bad shape (M=%d N=%d K=%d rowT=%d)", M, N, K, rowT);
    DIMX_REQUIRE(nseg >= 1 && nseg <= 3 && N % nseg == 0 && nseg * (N / nseg) == N, DIMX_ERR_ARG,
                 "op_gemm_map: %d segments do not divide N=%d", nseg, N);
    DIMX_REQUIRE(rowadd_mode >= 0 && rowadd_mode <= 3 && (rowadd_mode == 0 || (rowadd && ld_rowadd >= N && rowadd_div >= 1 && rowadd_off >= 0)),
                 DIMX_ERR_ARG, "op_gemm_map: row-add mode %d needs a table with ld >= N, div >= 1, off >= 0", rowadd_mode);
    DIMX_REQUIRE(!residual || ldr >= N, DIMX_ERR_ARG, "op_gemm_map: residual row stride %d below N=%d", ldr, N);
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
    g.force_simple = (flags >> 1) & 1;
    g.cfg = (flags >> 8) & 0xff;
    if (ldw > K && K % (in_dtype == DIMX_BF16 ? 64 : 32) == 0) g.kloop = K; /* padded row stride, exact k extent */
    g.rowT = rowT;
    g.nseg = nseg;
    g.seg_width = N / nseg;
    for (int i = 0; i < nseg; ++i) {
        DIMX_REQUIRE(seg_ptr[i] && seg_D[i] > 0 && g.seg_width % seg_D[i] == 0, DIMX_ERR_ARG,
                     "op_gemm_map: segment %d is unset or its head width does not divide the segment", i);
        g.seg[i].ptr = seg_ptr[i];
        g.seg[i].sb = (long)seg_strides[4 * i + 0];
        g.seg[i].sh = (long)seg_strides[4 * i + 1];
        g.seg[i].st = (long)seg_strides[4 * i + 2];
        g.seg[i].sd = (long)seg_strides[4 * i + 3];
        g.seg[i].D = seg_D[i];
    }
    if (rowadd_mode) {
        g.rowadd = rowadd;
        g.ld_rowadd = ld_rowadd;
        g.rowadd_mode = rowadd_mode;
        g.rowadd_scale = rowadd_scale;
        g.rowadd_off = rowadd_off;
        g.rowadd_div = rowadd_div;
    }
    return DIMX_OK;
}

extern "C" {

int dimx_op_gemm_map(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                     int act, const float* residual, int ldr, int rowT, int nseg, void* const* seg_ptr, const int64_t* seg_strides,
                     const int32_t* seg_D, const float* rowadd, int ld_rowadd, int rowadd_mode, float rowadd_scale, int rowadd_off,
                     int rowadd_div, int flags, void* stream) {
    GemmArgs g;
    DIMX_TRY(gemm_map_args(g, in_dtype, out_dtype, A, lda, W, ldw, M, N, K, bias, act, residual, ldr, rowT, nseg, seg_ptr, seg_strides,
                           seg_D, rowadd, ld_rowadd, rowadd_mode, rowadd_scale, rowadd_off, rowadd_div, flags));
    return launch_gemm(g, (hipStream_t)stream);
}

/* what launch_gemm would run for a dimx_op_gemm_map call with these arguments; nothing is read or launched: every pointer is
 * replaced by a dummy of the same 16-byte alignment (as dimx_op_gemm_slabs plans with dummies) */
int dimx_op_gemm_route(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                       int act, const float* residual, int ldr, int rowT, int nseg, void* const* seg_ptr, const int64_t* seg_strides,
                       const int32_t* seg_D, const float* rowadd, int ld_rowadd, int rowadd_mode, float rowadd_scale, int rowadd_off,
                       int rowadd_div, int flags) {
    GemmArgs g;
    DIMX_TRY(gemm_map_args(g, in_dtype, out_dtype, A, lda, W, ldw, M, N, K, bias, act, residual, ldr, rowT, nseg, seg_ptr, seg_strides,
                           seg_D, rowadd, ld_rowadd, rowadd_mode, rowadd_scale, rowadd_off, rowadd_div, flags));
    auto dummy = [](const void* p) -> uintptr_t { return p ? (uintptr_t)256 + ((uintptr_t)p & 15) : 0; };
    g.A = (const void*)dummy(g.A);
    g.W = (const void*)dummy(g.W);
    g.bias = (const float*)dummy(g.bias);
    g.residual = (const float*)dummy(g.residual);
    g.rowadd = (const float*)dummy(g.rowadd);
    for (int i = 0; i < g.nseg; ++i) g.seg[i].ptr = (void*)dummy(g.seg[i].ptr);
    int route = 0;
    DIMX_TRY(gemm_route(g, &route));
    return route;
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
// (prepack: the key words are packed here, ahead of the launch, and handed over as ready -- the decode loop's order)
static int op_attention_with_scratch(AttnArgs& a, hipStream_t st, bool prepack = false) {
    void* kw = nullptr;
    if (a.kmask && a.v_rows && a.dtype == DIMX_BF16) {
        a.kwords_cap = (size_t)a.B * ((a.Lk + 63) / 64);
        DIMX_HIP(hipMallocAsync(&kw, a.kwords_cap * 8, st));
        a.kwords = (unsigned long long*)kw;
    }
    int rc = DIMX_OK;
    if (kw && prepack) {
        rc = launch_pack_key_words(a.kmask, a.kmask_ld, a.lens, a.B, a.Lk, a.kwords, a.kwords_cap, st);
        a.kwords_ready = 1;
    }
    if (rc == DIMX_OK) rc = launch_attention(a, st);
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

// attention_tr.hip with every AttnArgs stride given (tests: the head-major cross-attention caches, an output wider than H * D, a key
// mask with a row stride of its own, key words packed ahead of the launch)
int dimx_op_attention_strided(const void* q, const void* k, const void* v, void* out, int B, int H, int Lq, int Lk, int D,
                              const long* q_str, const long* k_str, const long* v_str, const long* o_str, float scale, int causal,
                              const int32_t* lens, const uint8_t* kmask, int kmask_ld, int prepacked, void* stream) {
    DIMX_REQUIRE(q_str && k_str && v_str && o_str, DIMX_ERR_ARG, "op_attention_strided: strides are (batch, row, head) triples");
    DIMX_REQUIRE(!kmask || kmask_ld >= Lk, DIMX_ERR_ARG, "op_attention_strided: kmask_ld %d below Lk %d", kmask_ld, Lk);
    for (int i = 0; i < 3; ++i)
        DIMX_REQUIRE(q_str[i] > 0 && k_str[i] > 0 && v_str[i] > 0 && o_str[i] > 0, DIMX_ERR_ARG, "op_attention_strided: stride <= 0");
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = DIMX_BF16;
    a.q = q; a.k = k; a.vt = v; a.o = out;
    a.q_sb = q_str[0]; a.q_st = q_str[1]; a.q_sh = q_str[2];
    a.k_sb = k_str[0]; a.k_st = k_str[1]; a.k_sh = k_str[2];
    a.v_rows = 1;
    a.v_sb = v_str[0]; a.v_st = v_str[1]; a.v_sh = v_str[2];
    a.o_sb = o_str[0]; a.o_st = o_str[1]; a.o_sh = o_str[2];
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.D = D;
    a.scale = scale;
    a.causal = causal;
    a.lens = lens;
    a.kmask = kmask;
    a.kmask_ld = kmask_ld;
    return op_attention_with_scratch(a, (hipStream_t)stream, prepacked != 0);
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

int dimx_op_append_attn(int dtype, const float* qkv, int ld, void* kcache, void* vcache, void* out, int B, int H, int Tmax, int n0, int c,
                        float scale, void* stream) {
    DIMX_REQUIRE(qkv && H >= 1 && ld >= 3 * H * 64, DIMX_ERR_ARG, "append_attn: qkv rows of %d for %d heads", ld, H);
    AppendAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    a.q = qkv; a.k = qkv + (size_t)H * 64; a.v = qkv + (size_t)2 * H * 64; a.ld = ld;
    a.kcache = kcache; a.vcache = vcache; a.Tmax = Tmax;
    a.out = out; a.o_ld = H * 64;
    a.B = B; a.H = H; a.n0 = n0; a.c = c;
    a.scale = scale;
    return launch_append_attn(a, (hipStream_t)stream);
}

/* the table form's arguments of the first layer's self attention (DecodeAttnArgs.tab .. hist_ld, as self_args of generate.hip sets them) */
struct OpTabArgs {
    const void* tab;
    int tab_ld, tab_koff, tab_voff, tab_rows;
    const int32_t* hist;
    int hist_ld;
};
static void set_tab(DecodeAttnArgs& a, const OpTabArgs& t) {
    a.tab = t.tab; a.tab_rows = t.tab_rows;
    a.tab_ld = t.tab_ld; a.tab_koff = t.tab_koff; a.tab_voff = t.tab_voff;
    a.hist = t.hist; a.hist_ld = t.hist_ld;
}

/* every decode-attention form dimx_generate launches (tests): q / knew / vnew as the cache type or as nslab f32 split-K slabs,
 * the self form reading this step's k / v at q + H*64 / q + 2*H*64 of each slab row, the cross form with a strided key mask,
 * several query rows per clip and a forced wave count */
static int op_decode_attn_ex(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, int self_attn, void* kcache,
                             void* vcache, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys,
                             const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit, int win, int lookahead,
                             void* stream, const OpTabArgs* tab = nullptr) {
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
    if (tab) set_tab(a, *tab);
    return launch_decode_attn(a, (hipStream_t)stream);
}

int dimx_op_decode_attn_ex(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, int self_attn, void* kcache,
                           void* vcache, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys,
                           const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit, void* stream) {
    return op_decode_attn_ex(dtype, q, q_ld, q_is_f32, nslab, slab_stride, self_attn, kcache, vcache, out, o_ld, B, H, Tmax, step_dev, n_keys,
                             kmask, kmask_ld, rows_per_clip, scale, nsplit, 0, 0, stream);
}

/* the self form with the first layer's table arguments: K / V of position j are row hist[b][j] of tab, nothing is appended */
int dimx_op_decode_attn_tab(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, void* kcache, void* vcache,
                            void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, float scale, int nsplit, const void* tab,
                            int tab_ld, int tab_koff, int tab_voff, int tab_rows, const int32_t* hist, int hist_ld, void* stream) {
    const OpTabArgs t = {tab, tab_ld, tab_koff, tab_voff, tab_rows, hist, hist_ld};
    return op_decode_attn_ex(dtype, q, q_ld, q_is_f32, nslab, slab_stride, 1, kcache, vcache, out, o_ld, B, H, Tmax, step_dev, 0, nullptr, 0,
                             1, scale, nsplit, 0, 0, stream, &t);
}

/* the windowed cross form: the keys j < clamp(*step_dev + 2 + lookahead, 1, n_keys) */
int dimx_op_decode_attn_win(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, void* kcache, void* vcache,
                            void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys, const uint8_t* kmask,
                            int kmask_ld, int rows_per_clip, float scale, int nsplit, int lookahead, void* stream) {
    DIMX_REQUIRE(step_dev != nullptr, DIMX_ERR_ARG, "op_decode_attn_win: the windowed form needs a step counter");
    return op_decode_attn_ex(dtype, q, q_ld, q_is_f32, nslab, slab_stride, 0, kcache, vcache, out, o_ld, B, H, Tmax, step_dev, n_keys, kmask,
                             kmask_ld, rows_per_clip, scale, nsplit, 1, lookahead, stream);
}

/* FP8 cross K/V (decode_attn_kv8.hip): one cache -> codes + per-row scales */
int dimx_op_kv8_quantize(int dtype, const void* cache, int B, int H, int Tp, int T, uint8_t* codes, float* scales, void* stream) {
    return launch_kv8_quant(dtype, cache, B, H, Tp, T, codes, scales, (hipStream_t)stream);
}

/* ... rows [n0, n0 + c) of the K and V caches of `depth` layers in one launch; caches / codes / scales: host arrays of 2 * depth
 * device pointers, K of layer 0, V of layer 0, K of layer 1, ... */
int dimx_op_kv8_append(int dtype, const void* const* caches, uint8_t* const* codes, float* const* scales, int depth, int B, int H, int Tc, int Tp,
                       int n0, int c, void* stream) {
    DIMX_REQUIRE(depth >= 1 && depth <= 8, DIMX_ERR_ARG, "op_kv8_append: depth %d outside 1 .. 8", depth);
    DIMX_REQUIRE(caches && codes && scales, DIMX_ERR_ARG, "op_kv8_append: null pointer array");
    Kv8AppendArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < 2 * depth; ++i) { a.cache[i] = caches[i]; a.codes[i] = codes[i]; a.scales[i] = scales[i]; }
    a.dtype = dtype; a.depth = depth; a.B = B; a.H = H; a.Tc = Tc; a.Tp = Tp; a.n0 = n0; a.c = c;
    return launch_kv8_append(a, (hipStream_t)stream);
}

/* ... and the step's one-query cross attention over them, plain (win = 0) or windowed */
int dimx_op_decode_attn_kv8(int out_dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, const uint8_t* kcodes,
                            const float* kscale, const uint8_t* vcodes, const float* vscale, void* out, int o_ld, int B, int H, int Tmax,
                            const int32_t* step_dev, int n_keys, const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit,
                            int lookahead, int win, void* stream) {
    DIMX_REQUIRE(q_is_f32, DIMX_ERR_ARG, "op_decode_attn_kv8: q must be f32 split-K slabs");
    DIMX_REQUIRE(rows_per_clip <= 1, DIMX_ERR_ARG, "op_decode_attn_kv8: one row per clip (rows_per_clip = %d)", rows_per_clip);
    DIMX_REQUIRE(!win || step_dev != nullptr, DIMX_ERR_ARG, "op_decode_attn_kv8: the windowed form needs a step counter");
    Kv8AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = (const float*)q; a.q_ld = q_ld; a.nslab = nslab; a.slab_stride = slab_stride;
    a.kcodes = kcodes; a.kscale = kscale; a.vcodes = vcodes; a.vscale = vscale; a.Tmax = Tmax;
    a.out = out; a.out_dtype = out_dtype; a.o_ld = o_ld; a.B = B; a.H = H;
    a.n_keys = n_keys; a.kmask = kmask; a.kmask_ld = kmask_ld; a.scale = scale; a.force_nsplit = nsplit;
    if (win) { a.win = 1; a.lookahead = lookahead; a.step = step_dev; }
    return launch_decode_attn_kv8(a, (hipStream_t)stream);
}

/* ... and S query rows per clip on the matrix cores (decode_attn_mq_kv8_kernel): q as f32 slabs or bf16 rows, exact = the three-plane form */
int dimx_op_decode_attn_kv8_multi(int out_dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, const uint8_t* kcodes,
                                  const float* kscale, const uint8_t* vcodes, const float* vscale, void* out, int o_ld, int B, int H, int Tmax,
                                  const int32_t* step_dev, int n_keys, const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale,
                                  int nsplit, int lookahead, int win, int exact, void* stream) {
    (void)nsplit;   // one wave per (clip, head) in both forms
    DIMX_REQUIRE(!win || step_dev != nullptr, DIMX_ERR_ARG, "op_decode_attn_kv8_multi: the windowed form needs a step counter");
    Kv8AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = (const float*)q; a.q_ld = q_ld; a.nslab = nslab; a.slab_stride = slab_stride; a.q_bf16 = q_is_f32 ? 0 : 1;
    a.kcodes = kcodes; a.kscale = kscale; a.vcodes = vcodes; a.vscale = vscale; a.Tmax = Tmax;
    a.out = out; a.out_dtype = out_dtype; a.o_ld = o_ld; a.B = B; a.H = H; a.rows_per_clip = rows_per_clip;
    a.n_keys = n_keys; a.kmask = kmask; a.kmask_ld = kmask_ld; a.scale = scale; a.exact = exact ? 1 : 0;
    if (win) { a.win = 1; a.lookahead = lookahead; a.step = step_dev; }
    return launch_decode_attn_mq_kv8(a, (hipStream_t)stream);
}

/* the self form over FP8 self caches: quantise and append this step's k / v row at position n, attend over the rows 0 .. n */
int dimx_op_decode_attn_self_kv8(int out_dtype, const float* qkv, int ld, int nslab, long slab_stride, uint8_t* kcodes, float* kscale,
                                 uint8_t* vcodes, float* vscale, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n,
                                 float scale, int nsplit, void* stream) {
    DIMX_REQUIRE(qkv, DIMX_ERR_ARG, "op_decode_attn_self_kv8: null operand");
    DIMX_REQUIRE(H >= 1 && ld >= 3 * H * 64, DIMX_ERR_ARG, "op_decode_attn_self_kv8: ld=%d < 3 * H * 64 (rows hold q | k | v)", ld);
    Kv8SelfArgs a;
    memset(&a, 0, sizeof(a));
    a.q = qkv; a.knew = qkv + H * 64; a.vnew = qkv + 2 * H * 64; a.ld = ld; a.nslab = nslab; a.slab_stride = slab_stride;
    a.kcodes = kcodes; a.kscale = kscale; a.vcodes = vcodes; a.vscale = vscale; a.Tmax = Tmax;
    a.out = out; a.out_dtype = out_dtype; a.o_ld = o_ld; a.B = B; a.H = H;
    a.step = step_dev; a.n_max = n; a.scale = scale; a.force_nsplit = nsplit;
    return launch_decode_attn_self_kv8(a, (hipStream_t)stream);
}

/* windowed cross attention for many queries (win_attn.hip): query row i at position t0 + i, keys j < clamp(t0 + i + 2 + lookahead, 1, n_keys) */
int dimx_op_cross_attn_win(int dtype, const float* q, int ld, const void* kcache, const void* vcache, int Tp, void* out, int o_ld, int B, int H,
                           int Lq, int t0, int n_keys, int lookahead, const uint8_t* kmask, int kmask_ld, float scale, void* stream) {
    WinAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = dtype;
    a.q = q; a.ld = ld;
    a.kcache = kcache; a.vcache = vcache; a.Tp = Tp;
    a.out = out; a.o_ld = o_ld;
    a.B = B; a.H = H; a.Lq = Lq; a.t0 = t0; a.n_keys = n_keys; a.lookahead = lookahead;
    a.kmask = kmask; a.kmask_ld = kmask_ld;
    a.scale = scale;
    return launch_win_attn(a, (hipStream_t)stream);
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

static int op_layer_chain(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                          int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                          const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                          int call_index, float scale, void* scratch, void* prof, void* stream, const OpTabArgs* tab,
                          const SampleHeadArgs* head = nullptr) {
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
    if (tab) set_tab(sa, *tab);   // launch_layer_chain then takes the table instantiation
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
    if (head) lc.head = *head;  // ... or, with the sampling head, both come from the head's parameter block
    lc.prof = (unsigned long long*)prof;
    lc.sc_stride = ((T > n_keys ? T : n_keys) + 15) / 16 * 16;
    int cu = 0, dev = 0;
    DIMX_HIP(hipGetDevice(&dev));
    DIMX_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
    DIMX_REQUIRE(layer_chain_supported(lc, cu), DIMX_ERR_ARG, "op_layer_chain: not supported here (B = %d needs 129..256 clips, a 256-CU device)", B);
    return launch_layer_chain(lc, (hipStream_t)stream);
}

int dimx_op_layer_chain(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                        int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                        const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                        int call_index, float scale, void* scratch, void* prof, void* stream) {
    return op_layer_chain(qkv, nslab, slab_stride, sk, sv, T, ck, cv, Tp, n_keys, kmask, w_so, w_cq, colsum_cq, w_co, x, y, o, qc, stats, B,
                          step, call_index, scale, scratch, prof, stream, nullptr);
}

/* the first layer's launch: the self attention reads K / V from the table over the token history (sk / sv are not touched) */
int dimx_op_layer_chain_tab(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                            int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                            const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                            int call_index, float scale, void* scratch, void* prof, const void* tab, int tab_ld, int tab_koff,
                            int tab_voff, int tab_rows, const int32_t* hist, int hist_ld, void* stream) {
    const OpTabArgs t = {tab, tab_ld, tab_koff, tab_voff, tab_rows, hist, hist_ld};
    return op_layer_chain(qkv, nslab, slab_stride, sk, sv, T, ck, cv, Tp, n_keys, kmask, w_so, w_cq, colsum_cq, w_co, x, y, o, qc, stats, B,
                          step, call_index, scale, scratch, prof, stream, &t);
}

/* the first layer's launch with the sampling head (SampleHeadArgs in common.hpp): `params` is a parameter block of 16 words laid
 * out as dimx_generate's (0 step, 2 temperature, 4-5 seed, 6 row offset, 7 rows of the whole batch, 8 arrival counter, 9 chain
 * epoch, 14 first-step flag); the counters' epoch is word 9 (+ 1 when the head runs), so a zeroed scratch wants -1 there (0 with
 * the flag set).  qkv0 [512][2304] f32: q | k | v of a token; logits [>= B, 512]; emb_table [512][1152]. */
int dimx_op_layer_chain_head(const float* qkv0, const float* logits, int top_k, const float* exp_noise, int rows_total, int32_t* tokens,
                             int tok_ld, float* logits_out, const float* emb_table, int32_t* params, void* sk, void* sv, int T, const void* ck,
                             const void* cv, int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq,
                             const float* colsum_cq, const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, float scale,
                             void* scratch, void* prof, const void* tab, int tab_ld, int tab_koff, int tab_voff, int tab_rows, int32_t* hist,
                             int hist_ld, void* stream) {
    DIMX_REQUIRE(qkv0 && logits && tokens && emb_table && params && hist && tab, DIMX_ERR_ARG, "op_layer_chain_head: null argument");
    const OpTabArgs t = {tab, tab_ld, tab_koff, tab_voff, tab_rows, hist, hist_ld};
    SampleHeadArgs hd;
    memset(&hd, 0, sizeof(hd));
    hd.on = 1;
    hd.logits = logits; hd.ld_logits = 512; hd.nslab = 1; hd.top_k = top_k; hd.noise = exp_noise; hd.rows_total = rows_total;
    hd.tokens = tokens; hd.tok_ld = tok_ld; hd.logits_out = logits_out; hd.logits_out_ld = tok_ld;
    hd.emb_table = emb_table; hd.qkv0 = qkv0; hd.qkv0_N = 3 * 12 * 64; hd.hist = hist; hd.hist_ld = hist_ld; hd.params = params;
    return op_layer_chain(qkv0, 1, 0, sk, sv, T, ck, cv, Tp, n_keys, kmask, w_so, w_cq, colsum_cq, w_co, x, y, o, qc, stats, B, params, 0, scale,
                          scratch, prof, stream, &t, &hd);
}

/* the sampler launch of a generation step, on a parameter block as above: token column = the step word, the next history
 * position, the token's embedding row into x_next and its q/k/v table row into qkv0_out, step word and epoch advanced */
int dimx_op_sample_step(const float* logits, int R, int top_k, const float* exp_noise, int rows_total, int32_t* tokens, int tok_ld,
                        float* logits_out, const float* emb_table, int C, float* x_next, const float* qkv0, float* qkv0_out, int qkv0_N,
                        int32_t* hist, int hist_ld, int32_t* params, void* stream) {
    DIMX_REQUIRE(logits && tokens && params && R > 0, DIMX_ERR_ARG, "op_sample_step: null argument or R < 1");
    SampleArgs sm;
    sm.logits = logits; sm.ld_logits = 512; sm.R = R; sm.nslab = 1; sm.rows_total = rows_total; sm.top_k = top_k; sm.noise = exp_noise;
    sm.step_dev = params; sm.step_rw = params; sm.dev_params = params + 2; sm.done_ctr = (unsigned*)(params + 8); sm.epoch_rw = params + 9;
    sm.tokens = tokens; sm.tok_ld = tok_ld; sm.tok_col_from_step = 1; sm.logits_out = logits_out; sm.logits_out_ld = tok_ld;
    sm.emb_table = emb_table; sm.emb_C = C; sm.x_next = x_next;
    sm.qkv0_table = qkv0; sm.qkv0_out = qkv0_out; sm.qkv0_N = qkv0_N;
    sm.hist = hist; sm.hist_ld = hist_ld;
    return launch_sample(sm, (hipStream_t)stream);
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

int dimx_op_sample_guided(const float* cond, const float* uncond, int R, int nslab, long slab_stride, float scale, int kind, int top_k,
                          float a, float b, float temperature, const float* exp_noise, uint64_t seed, uint64_t step, int32_t* tokens,
                          float* guided_out, void* stream) {
    DIMX_TRY(check_sampler_filter(kind, a, b));
    DIMX_REQUIRE(cond && uncond && tokens && R > 0, DIMX_ERR_ARG, "op_sample_guided: null argument or R < 1");
    DIMX_REQUIRE(scale - scale == 0.f, DIMX_ERR_ARG, "op_sample_guided: the scale is NaN or infinite");
    DIMX_REQUIRE(nslab >= 1 && nslab <= 8 && (nslab == 1 || slab_stride >= (long)R * 512), DIMX_ERR_ARG,
                 "op_sample_guided: 1 <= nslab <= 8 slabs of at least R * 512 elements each");
    SampleArgs sm;
    sm.logits = cond; sm.ld_logits = 512; sm.R = R; sm.nslab = nslab; sm.slab_stride = slab_stride; sm.rows_total = R;
    sm.tokens = tokens; sm.tok_ld = 1;
    sm.top_k = kind == DIMX_FILTER_TOP_K ? top_k : 0; sm.temperature = temperature; sm.seed = seed;
    sm.noise = exp_noise; sm.step_host = exp_noise ? 0 : step;
    sm.filt = SampleFilter{kind, a, b, nullptr};
    sm.logits_out = guided_out; sm.logits_out_ld = 1;
    GuidedArgs g;
    g.logits_u = uncond; g.scale = scale; g.tokens_u = tokens + R;
    return launch_sample_guided(sm, g, (hipStream_t)stream);
}

}  // extern "C"
