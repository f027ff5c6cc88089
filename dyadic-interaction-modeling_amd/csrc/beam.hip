// beam.hip -- beam search on the decode path: the per-step top-W selection and the reorder of the self-attention cache.
//
// The definition is dimx/beam.py (numpy float64).  Rows clip * W + w of a generation are the W hypotheses of a clip; a step ends with
//   beam_select_kernel<W>   one block per clip, wave w = beam w, lane l holds entries l + 64 k, k = 0..7 (the sampler's map).  Split-K
//                           slabs added in slab order, exact f32 row maximum, exp / wave sum (xor 32, 16, ... 1) / log in double,
//                           candidate (w, v) = cum[w] + lp[w, v]; W rounds of {lane best, wave best, best of the W waves through LDS},
//                           ties to the smaller flat index w * 512 + v.  Wave r writes new row r: token, parent, running score, the
//                           back-pointer, and the next step's embedding row (+ the first layer's q/k/v table row).
//   beam_reorder_kernel<W>  one thread per 16-byte chunk of one (cache, clip, head, position <= c): the chunk of all W rows goes into
//                           registers, row w gets the chunk of row parent[w].  A thread reads and writes only its own addresses, so
//                           the permutation is in place with no second cache and no ordering between threads.  Clips whose parent
//                           vector is the identity leave at once.  Token and back-pointer columns < c move the same way.
//   beam_reorder_kv8_kernel<W>  the same over FP8 self caches (dimx_set_beam_kv8; dimx/kv8.py reorder): a thread owns one of the 4
//                           chunks of a position's 64 codes, the first chunk's thread also moves the position's scale.
// No atomics on data (the step word's arrival counter is the sampler's), fixed summation orders: bit-reproducible.
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kVocab = 512;
constexpr int kReorderThreads = 256;

template <int O> __device__ __forceinline__ void argmax_step_f64(double& b, int& i) {
    const double ob = xor_lane_f64<O>(b);
    const int oi = xor_lane_i32<O>(i);
    if (ob > b || (ob == b && oi < i)) {
        b = ob;
        i = oi;
    }
}

// row[0 .. n) of a table into dst, n % 4 == 0, by one wave
__device__ __forceinline__ void wave_copy_row(const float* src, float* dst, int n, int lane) {
    for (int i = lane; i < n / 4; i += 64) ((float4*)dst)[i] = ((const float4*)src)[i];
}

template <int W> __global__ __launch_bounds__(W * 64) void beam_select_kernel(BeamSelectArgs a) {
    __shared__ double sh_b[W][W];
    __shared__ int sh_i[W][W];
    const int clip = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = clip * W + w;
    const int c = a.step_dev ? *a.step_dev : a.step_host;
    const int col = a.step_dev ? c : 0;
    const float* lr = a.logits + (size_t)row * kVocab;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = lr[lane + 64 * k];
        for (int s = 1; s < a.nslab; ++s) v[k] += lr[(size_t)s * a.slab_stride + lane + 64 * k];
    }
    if (a.logits_out) {   // the step's rows in the order they ran: the dump is not reordered afterwards
        float* lo = a.logits_out + ((size_t)row * a.tok_ld + col) * kVocab;
#pragma unroll
        for (int k = 0; k < 8; ++k) lo[lane + 64 * k] = v[k];
    }
    // the clip's mode (block-uniform)
    int mode = 0, ftok = 0;
    if (a.mode) {
        mode = a.mode[clip];
        ftok = a.forced_tok ? a.forced_tok[clip] : 0;
    } else {
        if (a.prompt) {
            int plen = a.prompt_len ? a.prompt_len[clip] : a.prompt_max;
            const int p0 = a.dev_params ? a.dev_params[8] + 1 : 1;
            plen = plen < p0 ? p0 : (plen > a.prompt_max ? a.prompt_max : plen);
            if (c + 1 < plen) {
                mode = 1;
                ftok = a.prompt[(size_t)clip * a.prompt_ld + c + 1];
            }
        }
        if (mode == 0 && a.lens && c >= a.lens[clip] - a.len_off) mode = 2;
    }
    ftok = ftok < 0 ? 0 : (ftok >= kVocab ? kVocab - 1 : ftok);   // the sampler's clamp of a prompt token
    const double cw = a.cum_in[row];
    int tok = ftok, par = w;
    double sc_new = cw;
    if (mode == 2) {   // frozen: the row's own arg-max, first maximum (the greedy sampler's)
        float mx = -3.0e38f;
        int mi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (v[k] > mx) {
                mx = v[k];
                mi = lane + 64 * k;
            }
        wave_argmax(mx, mi);
        tok = mi;
    } else if (mode == 0) {
        float m = v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) m = fmaxf(m, v[k]);
        m = wave_max(m);
        const double md = (double)m;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += exp((double)v[k] - md);
        const double lg = log(wave_sum_f64(s));
        double sc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sc[k] = cw + (((double)v[k] - md) - lg);
        const double ninf = -__builtin_inf();
        unsigned taken = 0;
        int win = w * kVocab;
        for (int r = 0; r < W; ++r) {
            double b = ninf;
            int bi = 0x7fffffff;   // "no candidate": a NaN score never enters, a real -inf does (its index is smaller)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int idx = w * kVocab + lane + 64 * k;
                if (!((taken >> k) & 1u) && (sc[k] > b || (sc[k] == b && idx < bi))) {
                    b = sc[k];
                    bi = idx;
                }
            }
            argmax_step_f64<32>(b, bi);
            argmax_step_f64<16>(b, bi);
            argmax_step_f64<8>(b, bi);
            argmax_step_f64<4>(b, bi);
            argmax_step_f64<2>(b, bi);
            argmax_step_f64<1>(b, bi);
            if (lane == 0) {
                sh_b[r][w] = b;
                sh_i[r][w] = bi;
            }
            __syncthreads();
            b = sh_b[r][0];
            bi = sh_i[r][0];
#pragma unroll
            for (int j = 1; j < W; ++j) {
                const double ob = sh_b[r][j];
                const int oi = sh_i[r][j];
                if (ob > b || (ob == b && oi < bi)) {
                    b = ob;
                    bi = oi;
                }
            }
            if ((unsigned)bi >= (unsigned)(W * kVocab)) bi = r * kVocab;   // every remaining score is NaN: keep the row, token 0
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (bi == w * kVocab + lane + 64 * k) taken |= 1u << k;
            if (r == w) {
                win = bi;
                sc_new = b;
            }
        }
        par = win / kVocab;
        tok = win - par * kVocab;
    }
    if (mode != 0) __syncthreads();   // every row's cum_in is read before any cum_out is written (the live rounds have barriers)
    if (lane == 0) {
        a.tokens[(size_t)row * a.tok_ld + col] = tok;
        a.parent[row] = par;
        a.cum_out[row] = sc_new;
        if (a.backptr) a.backptr[(size_t)row * a.tok_ld + col] = par;
    }
    if (a.x_next) wave_copy_row(a.emb_table + (size_t)tok * a.emb_C, a.x_next + (size_t)row * a.emb_C, a.emb_C, lane);
    if (a.qkv0_table) wave_copy_row(a.qkv0_table + (size_t)tok * a.qkv0_N, a.qkv0_out + (size_t)row * a.qkv0_N, a.qkv0_N, lane);
    if (a.step_rw) {   // the block that finishes last advances the step word (every block has read it by then)
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned prev = atomicAdd(a.done_ctr, 1u);
            if (prev == gridDim.x - 1) {
                *a.done_ctr = 0u;
                *a.step_rw = c + 1;
                if (a.epoch_rw) *a.epoch_rw += 1;
            }
        }
    }
}

__device__ __forceinline__ int pick(bool t, int x, int y) { return t ? x : y; }
__device__ __forceinline__ uint4 pick(bool t, const uint4& x, const uint4& y) {
    return make_uint4(t ? x.x : y.x, t ? x.y : y.y, t ? x.z : y.z, t ? x.w : y.w);
}

// base[w * row_stride] = base[par[w] * row_stride] for the W rows at once.  par is uniform and the gather is a chain of selects over
// registers: no runtime-indexed array (that would live in scratch)
template <int W, typename V> __device__ __forceinline__ void permute_rows(V* base, size_t row_stride, const int (&par)[W]) {
    V in[W];
#pragma unroll
    for (int w = 0; w < W; ++w) in[w] = base[(size_t)w * row_stride];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        V o = in[0];
#pragma unroll
        for (int j = 1; j < W; ++j) o = pick(par[w] == j, in[j], o);
        base[(size_t)w * row_stride] = o;
    }
}

template <int W> __global__ __launch_bounds__(kReorderThreads) void beam_reorder_kernel(BeamReorderArgs a) {
    const int clip = blockIdx.z;
    int par[W];
    bool ident = true, valid = true;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        par[w] = a.parent[clip * W + w];
        ident = ident && par[w] == w;
        valid = valid && (unsigned)par[w] < (unsigned)W;
    }
    if (ident || !valid) return;
    int c = a.step_dev ? *a.step_dev - a.step_back : a.c_host;
    c = c < 0 ? -1 : (c > a.T - 1 ? a.T - 1 : c);
    const int i = blockIdx.x * kReorderThreads + threadIdx.x;
    const int cpp = 64 * a.es / 16;   // 16-byte chunks per position
    if (i < (c + 1) * cpp) {
        const int b = blockIdx.y / a.H, hd = blockIdx.y - b * a.H;
        const size_t head16 = (size_t)a.T * cpp, row16 = (size_t)a.H * head16;
        void* cache = a.buf[0];   // a.buf[b] by selects: a runtime index would copy the argument block to scratch
#pragma unroll
        for (int j = 1; j < 16; ++j) cache = b == j ? a.buf[j] : cache;
        permute_rows<W>((uint4*)cache + (size_t)clip * W * row16 + (size_t)hd * head16 + i, row16, par);
    }
    if (blockIdx.y == 0 && i < c && i < a.tok_ld) {
        if (a.tokens) permute_rows<W>(a.tokens + (size_t)clip * W * a.tok_ld + i, (size_t)a.tok_ld, par);
        if (a.backptr) permute_rows<W>(a.backptr + (size_t)clip * W * a.tok_ld + i, (size_t)a.tok_ld, par);
    }
}

// The FP8 sibling: one thread per 16-byte chunk of the codes of one (plane pair, clip, head, position <= c), 4 chunks per position;
// the thread of a position's first chunk moves that position's scale (as its 32 bits: a permutation never forms a float) the same
// way.  Same grid, same step word, same early return, same in-place argument as beam_reorder_kernel.
template <int W> __global__ __launch_bounds__(kReorderThreads) void beam_reorder_kv8_kernel(BeamReorderKv8Args a) {
    const int clip = blockIdx.z;
    int par[W];
    bool ident = true, valid = true;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        par[w] = a.parent[clip * W + w];
        ident = ident && par[w] == w;
        valid = valid && (unsigned)par[w] < (unsigned)W;
    }
    if (ident || !valid) return;
    int c = a.step_dev ? *a.step_dev - a.step_back : a.c_host;
    c = c < 0 ? -1 : (c > a.Tp - 1 ? a.Tp - 1 : c);
    const int i = blockIdx.x * kReorderThreads + threadIdx.x;
    if (i < (c + 1) * 4) {
        const int b = blockIdx.y / a.H, hd = blockIdx.y - b * a.H;
        const size_t head16 = (size_t)a.Tp * 4, row16 = (size_t)a.H * head16;
        uint8_t* codes = a.codes[0];   // by selects, as in beam_reorder_kernel
        float* scale = a.scale[0];
#pragma unroll
        for (int j = 1; j < kBeamKv8Pairs; ++j) {
            codes = b == j ? a.codes[j] : codes;
            scale = b == j ? a.scale[j] : scale;
        }
        // permute_rows for the chunk and the scale in one select chain (each comparison feeds both and is dead after them)
        uint4* cb = (uint4*)codes + (size_t)clip * W * row16 + (size_t)hd * head16 + i;
        int* sb = (int*)scale + ((size_t)clip * W * a.H + hd) * a.Tp + (i >> 2);
        const size_t srow = (size_t)a.H * a.Tp;
        const bool first = (i & 3) == 0;
        uint4 in[W];
        int sc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            in[w] = cb[(size_t)w * row16];
            sc[w] = first ? sb[(size_t)w * srow] : 0;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint4 o = in[0];
            int os = sc[0];
#pragma unroll
            for (int j = 1; j < W; ++j) {
                o = pick(par[w] == j, in[j], o);
                os = pick(par[w] == j, sc[j], os);
            }
            cb[(size_t)w * row16] = o;
            if (first) sb[(size_t)w * srow] = os;
        }
    }
    if (blockIdx.y == 0 && i < c && i < a.tok_ld) {
        if (a.tokens) permute_rows<W>(a.tokens + (size_t)clip * W * a.tok_ld + i, (size_t)a.tok_ld, par);
        if (a.backptr) permute_rows<W>(a.backptr + (size_t)clip * W * a.tok_ld + i, (size_t)a.tok_ld, par);
    }
}

__global__ void beam_init_kernel(double* cum, int32_t* parent, int R, int W) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    cum[r] = r % W == 0 ? 0.0 : -__builtin_inf();
    parent[r] = r % W;
}

template <int W> void select_launch(const BeamSelectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_select_kernel<W>, dim3(a.nclip), dim3(W * 64), 0, s, a);
}
template <int W> void reorder_launch(const BeamReorderArgs& a, hipStream_t s) {
    const int cpp = 64 * a.es / 16;
    hipLaunchKernelGGL(beam_reorder_kernel<W>, dim3(ceil_div(a.T * cpp, kReorderThreads), a.nbuf * a.H, a.nclip), dim3(kReorderThreads), 0,
                       s, a);
}
template <int W> void reorder_kv8_launch(const BeamReorderKv8Args& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_reorder_kv8_kernel<W>, dim3(ceil_div(a.Tp * 4, kReorderThreads), a.nbuf * a.H, a.nclip), dim3(kReorderThreads),
                       0, s, a);
}

}  // namespace

bool beam_width_supported(int W) { return W == 1 || W == 2 || W == 4 || W == 5 || W == 8 || W == 10; }

int launch_beam_select(const BeamSelectArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.logits && a.cum_in && a.cum_out && a.parent && a.tokens, DIMX_ERR_ARG, "beam_select: null operand");
    DIMX_REQUIRE(beam_width_supported(a.W), DIMX_ERR_ARG, "beam_select: width %d not in {1,2,4,5,8,10}", a.W);
    DIMX_REQUIRE(a.nclip >= 1 && a.nslab >= 1 && a.tok_ld >= 1, DIMX_ERR_ARG, "beam_select: clips %d, slabs %d or row stride %d below 1", a.nclip,
                 a.nslab, a.tok_ld);
    DIMX_REQUIRE(a.step_dev || (a.step_host >= 0 && !a.prompt && !a.lens), DIMX_ERR_ARG, "beam_select: a host step carries no prompt / lens rule");
    DIMX_REQUIRE(!a.step_rw || (a.step_dev && a.done_ctr), DIMX_ERR_ARG, "beam_select: advancing the step word needs the word and its arrival counter");
    DIMX_REQUIRE(!a.prompt || (a.prompt_max >= 1 && a.prompt_ld >= a.prompt_max), DIMX_ERR_ARG, "beam_select: 1 <= prompt_max <= prompt_ld");
    DIMX_REQUIRE(!a.x_next || (a.emb_table && a.emb_C > 0 && a.emb_C % 4 == 0), DIMX_ERR_ARG, "beam_select: embedding width %d", a.emb_C);
    DIMX_REQUIRE(!a.qkv0_table || (a.qkv0_out && a.qkv0_N > 0 && a.qkv0_N % 4 == 0), DIMX_ERR_ARG, "beam_select: q/k/v table width %d", a.qkv0_N);
    switch (a.W) {
        case 1: select_launch<1>(a, s); break;
        case 2: select_launch<2>(a, s); break;
        case 4: select_launch<4>(a, s); break;
        case 5: select_launch<5>(a, s); break;
        case 8: select_launch<8>(a, s); break;
        default: select_launch<10>(a, s); break;
    }
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.parent && a.nbuf >= 0 && a.nbuf <= 16, DIMX_ERR_ARG, "beam_reorder: null parents or %d caches (at most 16)", a.nbuf);
    DIMX_REQUIRE(beam_width_supported(a.W), DIMX_ERR_ARG, "beam_reorder: width %d not in {1,2,4,5,8,10}", a.W);
    DIMX_REQUIRE(a.es == 2 || a.es == 4, DIMX_ERR_ARG, "beam_reorder: element size %d", a.es);
    DIMX_REQUIRE(a.nclip >= 1 && a.H >= 1 && a.T >= 1 && (long)a.nbuf * a.H <= 65535 && a.nclip <= 65535, DIMX_ERR_ARG,
                 "beam_reorder: clips %d, heads %d or positions %d out of range", a.nclip, a.H, a.T);
    DIMX_REQUIRE(a.step_dev || (a.c_host >= 0 && a.c_host < a.T), DIMX_ERR_ARG, "beam_reorder: c = %d outside [0, %d)", a.c_host, a.T);
    DIMX_REQUIRE((!a.tokens && !a.backptr) || (a.tok_ld >= 1 && a.tok_ld <= a.T * (64 * a.es / 16)), DIMX_ERR_ARG, "beam_reorder: token row stride %d",
                 a.tok_ld);
    for (int b = 0; b < a.nbuf; ++b)
        DIMX_REQUIRE(a.buf[b] && ((uintptr_t)a.buf[b] % 16) == 0, DIMX_ERR_ARG, "beam_reorder: cache %d is null or not 16-byte aligned", b);
    if (a.W == 1 || (a.nbuf == 0 && !a.tokens && !a.backptr)) return DIMX_OK;   // one beam per clip: every parent vector is the identity
    switch (a.W) {
        case 2: reorder_launch<2>(a, s); break;
        case 4: reorder_launch<4>(a, s); break;
        case 5: reorder_launch<5>(a, s); break;
        case 8: reorder_launch<8>(a, s); break;
        default: reorder_launch<10>(a, s); break;
    }
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_beam_reorder_kv8(const BeamReorderKv8Args& a, hipStream_t s) {
    DIMX_REQUIRE(a.parent && a.nbuf >= 1 && a.nbuf <= kBeamKv8Pairs, DIMX_ERR_ARG, "beam_reorder_kv8: null parents or %d plane pairs (1 .. %d)", a.nbuf,
                 kBeamKv8Pairs);
    DIMX_REQUIRE(beam_width_supported(a.W), DIMX_ERR_ARG, "beam_reorder_kv8: width %d not in {1,2,4,5,8,10}", a.W);
    DIMX_REQUIRE(a.nclip >= 1 && a.H >= 1 && a.Tp >= 1 && (long)a.nbuf * a.H <= 65535 && a.nclip <= 65535, DIMX_ERR_ARG,
                 "beam_reorder_kv8: clips %d, heads %d or positions %d out of range", a.nclip, a.H, a.Tp);
    DIMX_REQUIRE(a.step_dev || (a.c_host >= 0 && a.c_host < a.Tp), DIMX_ERR_ARG, "beam_reorder_kv8: c = %d outside [0, %d)", a.c_host, a.Tp);
    DIMX_REQUIRE((!a.tokens && !a.backptr) || (a.tok_ld >= 1 && a.tok_ld <= a.Tp * 4), DIMX_ERR_ARG, "beam_reorder_kv8: token row stride %d",
                 a.tok_ld);
    for (int b = 0; b < a.nbuf; ++b)
        DIMX_REQUIRE(a.codes[b] && ((uintptr_t)a.codes[b] % 16) == 0 && a.scale[b] && ((uintptr_t)a.scale[b] % 4) == 0, DIMX_ERR_ARG,
                     "beam_reorder_kv8: plane pair %d is null, its codes not 16-byte or its scales not 4-byte aligned", b);
    if (a.W == 1) return DIMX_OK;   // one beam per clip: every parent vector is the identity
    switch (a.W) {
        case 2: reorder_kv8_launch<2>(a, s); break;
        case 4: reorder_kv8_launch<4>(a, s); break;
        case 5: reorder_kv8_launch<5>(a, s); break;
        case 8: reorder_kv8_launch<8>(a, s); break;
        default: reorder_kv8_launch<10>(a, s); break;
    }
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_beam_init(double* cum, int32_t* parent, int R, int W, hipStream_t s) {
    DIMX_REQUIRE(cum && parent && R >= 1 && W >= 1, DIMX_ERR_ARG, "beam_init: bad arguments");
    hipLaunchKernelGGL(beam_init_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, s, cum, parent, R, W);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx

using namespace dimx;

int dimx_op_beam_step(const float* logits, const double* cum, const int32_t* mode, const int32_t* forced_tok, int B, int W,
                      int32_t* parent, int32_t* token, double* cum_out, void* stream) {
    DIMX_REQUIRE(logits && cum && mode && parent && token && cum_out, DIMX_ERR_ARG, "beam_step: null operand");
    DIMX_REQUIRE(B >= 1, DIMX_ERR_ARG, "beam_step: B=%d must be positive", B);
    BeamSelectArgs a;
    a.logits = logits, a.nclip = B, a.W = W;
    a.mode = mode, a.forced_tok = forced_tok;
    a.cum_in = cum, a.cum_out = cum_out, a.parent = parent, a.tokens = token;
    return launch_beam_select(a, (hipStream_t)stream);
}

int dimx_op_beam_reorder(void* cache, int dtype, const int32_t* parent, int R, int W, int H, int T, int c, void* stream) {
    DIMX_REQUIRE(cache && parent, DIMX_ERR_ARG, "beam_reorder: null operand");
    DIMX_REQUIRE(dtype == DIMX_F32 || dtype == DIMX_BF16, DIMX_ERR_ARG, "beam_reorder: unknown element type %d", dtype);
    DIMX_REQUIRE(W >= 1 && R >= 1 && R % W == 0, DIMX_ERR_ARG, "beam_reorder: R=%d is not a positive multiple of W=%d", R, W);
    BeamReorderArgs a;
    a.buf[0] = cache, a.nbuf = 1, a.es = dtype == DIMX_BF16 ? 2 : 4;
    a.nclip = R / W, a.W = W, a.H = H, a.T = T;
    a.parent = parent, a.c_host = c;
    return launch_beam_reorder(a, (hipStream_t)stream);
}

int dimx_op_beam_reorder_kv8(void* kcodes, void* kscale, const int32_t* parent, int R, int W, int H, int Tp, int c, void* stream) {
    DIMX_REQUIRE(kcodes && kscale && parent, DIMX_ERR_ARG, "beam_reorder_kv8: null operand");
    DIMX_REQUIRE(W >= 1 && R >= 1 && R % W == 0, DIMX_ERR_ARG, "beam_reorder_kv8: R=%d is not a positive multiple of W=%d", R, W);
    BeamReorderKv8Args a;
    a.codes[0] = (uint8_t*)kcodes, a.scale[0] = (float*)kscale, a.nbuf = 1;
    a.nclip = R / W, a.W = W, a.H = H, a.Tp = Tp;
    a.parent = parent, a.c_host = c;
    return launch_beam_reorder_kv8(a, (hipStream_t)stream);
}
