// retrieval.hip -- the retrieval baselines of reference code/baselines.py:30-103 (NN audio, NN motion, Random): clip descriptors,
// cosine k-nearest-neighbour search and the gather of the retrieved listener sequences.  The definition is dimx/retrieval.py.
//
// pool_desc_kernel (one block per clip): thread c takes the dimensions c, c + 256, ...; per dimension it walks the clip's valid
//   frames in order (a frame's loads are coalesced across the dimensions), the f32 maximum widened or the f64 sum / n.  The norm:
//   a thread adds the squares of its dimensions in ascending order (fma from zero), a wave adds by xor 32, 16, ... 1, the four
//   waves are added in wave order -- an order that depends on D alone.
// nn_search_kernel (block = (library chunk of 256 entries, tile of 16 queries), 8 waves): the tile's descriptors lie in LDS
//   [16][D]; a wave streams two library rows at a time, lane l holding the dimensions l, l + 64, ... of each in registers (the next
//   pair's loads are issued before this pair's sums are folded), and keeps 2 x 16 partial dot products (fma in ascending dimension from zero).  The 16 sums of a row are then folded across the wave: at the
//   xor-32 step the lower half keeps queries 0..7 and the upper half 8..15, at xor 16 / 8 / 4 the kept set halves again, xor 2 and
//   xor 1 finish -- every query's sum is the xor 32, 16, ... 1 butterfly of its lanes' partial sums (a + b == b + a), whatever slot of
//   the tile the query sits in.  sim = dot / (|q| |x|).  So the similarity of a pair is a function of the two descriptors (and norms)
//   alone: not of the chunk, the tile, the wave or the lane group.  The tile's similarities [16][256] go to LDS (and to sim_out when
//   given); wave w then selects the chunk's top K for the queries w and w + 8: K rounds of a wave-wide arg-best under the total order
//   (similarity descending, index ascending), a round admitting only what comes strictly after the previous pick, eligible = not NaN
//   and > -1.  The partial lists go to the workspace [Q][chunks][K].
// nn_merge_kernel (one wave per query): the same K rounds over the query's chunks x K candidates -> idx, sim, found.
// nn_gather_kernel (one block per (query, slot)): out_len = min(q_len, lib_len of the entry), the rows through gather_winner_rows.
// No atomics, no host synchronisation, no allocation; frames t >= lens are never loaded, library rows >= N are never loaded.
#include "pick_gather.hpp"

namespace dimx {
namespace {

constexpr int kPoolThreads = 256;
constexpr int kNsThreads = 512;
constexpr int kNsWaves = kNsThreads / 64;
constexpr int kNsChunk = 256;    // library entries per block
constexpr int kNsTile = 16;      // queries per block
constexpr int kNsRows = 2;       // library rows a wave holds at a time
constexpr int kNsMaxK = 16;
constexpr int kNsMaxD = 960;     // (16 * 960 + 16 * 256) * 8 B = 152 KiB of the CU's 160 KiB of LDS
constexpr int kNsMaxI = kNsMaxD / 64;   // dimensions a lane holds of one row, at most
constexpr int kGatherThreads = 256;

__device__ __forceinline__ int clamp_len(const int32_t* lens, int i, int hi) { return min(max(lens[i], 0), hi); }

struct PoolArgs {
    const float* x;
    long cs, fs;
    const int32_t* lens;
    int N, T, D, kind;
    double* desc;
    double* norm;
};

__global__ __launch_bounds__(kPoolThreads) void pool_desc_kernel(PoolArgs a) {
    __shared__ double sh[kPoolThreads / 64];
    const int i = blockIdx.x;
    const int n = clamp_len(a.lens, i, a.T);
    const float* x = a.x + (size_t)i * a.cs;
    double sq = 0.0;
    for (int c = threadIdx.x; c < a.D; c += kPoolThreads) {
        double v = 0.0;
        if (n > 0) {
            if (a.kind == 0) {
                float m = x[c];
                for (int t = 1; t < n; ++t) m = fmaxf(m, x[(size_t)t * a.fs + c]);
                v = (double)m;
            } else {
                double s = 0.0;
                for (int t = 0; t < n; ++t) s += (double)x[(size_t)t * a.fs + c];
                v = s / (double)n;
            }
        }
        a.desc[(size_t)i * a.D + c] = v;
        sq = fma(v, v, sq);
    }
    sq = wave_sum_f64(sq);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        for (int w = 1; w < kPoolThreads / 64; ++w) t += sh[w];
        a.norm[i] = sqrt(t);
    }
}

struct NsArgs {
    const double* qd;
    long q_ld;
    const double* qn;
    const double* xd;
    long x_ld;
    const double* xn;
    int Q, N, D, K, chunks;
    int32_t* idx;
    double* sim;
    int32_t* found;
    double* sim_out;     // [Q][N] or nullptr
    double* ws_sim;      // [Q][chunks][K]
    int32_t* ws_idx;     // [Q][chunks][K]
};

// in[0 .. 2H) -> out[0 .. H): the lanes whose bit O is clear keep the sums of in[0 .. H), the others those of in[H .. 2H)
template <int O, int H> __device__ __forceinline__ void ns_fold(const double* in, double* out, bool up) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double keep = up ? in[i + H] : in[i];
        const double send = up ? in[i] : in[i + H];
        out[i] = keep + xor_lane_f64<O>(send);
    }
}

// (v, i) of the wave's best candidate under (similarity descending, index ascending); i < 0 = no candidate (v is then ignored).
// Every lane ends with the same pair.  All 64 lanes must be active.
__device__ __forceinline__ void ns_wave_best(double& v, int& i) {
#define DIMX_NS_STEP(O)                                                   \
    do {                                                                  \
        const double ov_ = xor_lane_f64<O>(v);                            \
        const int oi_ = xor_lane_i32<O>(i);                               \
        if (oi_ >= 0 && (i < 0 || ov_ > v || (ov_ == v && oi_ < i))) {    \
            v = ov_;                                                      \
            i = oi_;                                                      \
        }                                                                 \
    } while (0)
    DIMX_NS_STEP(32);
    DIMX_NS_STEP(16);
    DIMX_NS_STEP(8);
    DIMX_NS_STEP(4);
    DIMX_NS_STEP(2);
    DIMX_NS_STEP(1);
#undef DIMX_NS_STEP
}

// does the eligible candidate (s, i) come strictly after the previous pick (ls, li) and before the lane's current best (v, bi)?
__device__ __forceinline__ void ns_consider(double s, int i, double ls, int li, double& v, int& bi) {
    if (!(s > -1.0)) return;                                   // NaN and <= -1 are not eligible
    if (!(s < ls || (s == ls && i > li))) return;              // already picked, or before the previous pick
    if (bi < 0 || s > v || (s == v && i < bi)) {
        v = s;
        bi = i;
    }
}

// NI: the dimensions a lane holds of one row, D <= 64 NI
template <int NI> __global__ __launch_bounds__(kNsThreads) void nn_search_kernel(NsArgs a) {
    extern __shared__ double ns_dyn[];
    __shared__ double sh_qn[kNsTile];
    const int D = a.D;
    double* qs = ns_dyn;                        // [kNsTile][D]
    double* sims = ns_dyn + (size_t)kNsTile * D;   // [kNsTile][kNsChunk]
    const int chunk = blockIdx.x, q0 = blockIdx.y * kNsTile, r0 = chunk * kNsChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < kNsTile * D; e += kNsThreads) {
        const int qi = e / D, d = e - qi * D;
        qs[e] = q0 + qi < a.Q ? a.qd[(size_t)(q0 + qi) * a.q_ld + d] : 0.0;
    }
    if (threadIdx.x < kNsTile) sh_qn[threadIdx.x] = q0 + threadIdx.x < a.Q ? a.qn[q0 + threadIdx.x] : 0.0;
    __syncthreads();
    // the query this lane ends up with after the folds, and its norm
    const int qsel = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
    const double qnorm = sh_qn[qsel];
    // a wave's rows rb, rb + 1 as registers: lane l holds the dimensions l + 64 i.  A row >= N is never read: its slot rereads row rb
    double xv[kNsRows][NI];
    auto load_rows = [&](int rb) {
#pragma unroll
        for (int r = 0; r < kNsRows; ++r) {
            const double* p = a.xd + (size_t)(r0 + rb + r < a.N ? r0 + rb + r : r0 + rb) * a.x_ld;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (64 * i < D) xv[r][i] = lane + 64 * i < D ? p[lane + 64 * i] : 0.0;   // the outer test is wave-uniform
        }
    };
    if (r0 + wave * kNsRows < a.N) load_rows(wave * kNsRows);
    for (int rb = wave * kNsRows; rb < kNsChunk; rb += kNsWaves * kNsRows) {   // wave-uniform
        if (r0 + rb >= a.N) break;
        double acc[kNsRows][kNsTile];
#pragma unroll
        for (int r = 0; r < kNsRows; ++r)
#pragma unroll
            for (int qi = 0; qi < kNsTile; ++qi) acc[r][qi] = 0.0;
        bool live[kNsRows];
#pragma unroll
        for (int r = 0; r < kNsRows; ++r) live[r] = r0 + rb + r < a.N;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int d = lane + 64 * i;
            if (64 * i < D && d < D) {
                double qv[kNsTile];   // the 16 LDS reads of a dimension in flight together, not one wait per read
#pragma unroll
                for (int qi = 0; qi < kNsTile; ++qi) qv[qi] = qs[qi * D + d];
#pragma unroll
                for (int qi = 0; qi < kNsTile; ++qi)
#pragma unroll
                    for (int r = 0; r < kNsRows; ++r) acc[r][qi] = fma(xv[r][i], qv[qi], acc[r][qi]);
            }
        }
        // the next pair's loads are issued before this pair's sums are folded: their latency lies under the folds
        const int rb_next = rb + kNsWaves * kNsRows;
        if (rb_next < kNsChunk && r0 + rb_next < a.N) load_rows(rb_next);
#pragma unroll
        for (int r = 0; r < kNsRows; ++r) {
            double b8[8], b4[4], b2[2], b1[1];
            ns_fold<32, 8>(acc[r], b8, (lane & 32) != 0);
            ns_fold<16, 4>(b8, b4, (lane & 16) != 0);
            ns_fold<8, 2>(b4, b2, (lane & 8) != 0);
            ns_fold<4, 1>(b2, b1, (lane & 4) != 0);
            double dot = b1[0];
            dot += xor_lane_f64<2>(dot);
            dot += xor_lane_f64<1>(dot);
            if (live[r] && (lane & 3) == 0) sims[qsel * kNsChunk + rb + r] = dot / (qnorm * a.xn[r0 + rb + r]);
        }
    }
    __syncthreads();
    const int rows = min(kNsChunk, a.N - r0);
    if (a.sim_out) {
        for (int e = threadIdx.x; e < kNsTile * kNsChunk; e += kNsThreads) {
            const int qi = e / kNsChunk, r = e - qi * kNsChunk;
            if (q0 + qi < a.Q && r < rows) a.sim_out[(size_t)(q0 + qi) * a.N + r0 + r] = sims[e];
        }
    }
    for (int qi = wave; qi < kNsTile; qi += kNsWaves) {   // wave-uniform
        if (q0 + qi >= a.Q) break;
        const double* s = sims + qi * kNsChunk;
        double* o_sim = a.ws_sim + ((size_t)(q0 + qi) * a.chunks + chunk) * a.K;
        int32_t* o_idx = a.ws_idx + ((size_t)(q0 + qi) * a.chunks + chunk) * a.K;
        double ls = __builtin_inf();
        int li = -1;
        for (int k = 0; k < a.K; ++k) {
            double v = 0.0;
            int bi = -1;
            if (li >= 0 || k == 0)   // after an empty round nothing is left
                for (int r = lane; r < rows; r += 64) ns_consider(s[r], r0 + r, ls, li, v, bi);
            ns_wave_best(v, bi);
            if (lane == 0) {
                o_sim[k] = bi >= 0 ? v : __builtin_nan("");
                o_idx[k] = bi;
            }
            ls = v, li = bi;
        }
    }
}

__global__ __launch_bounds__(64) void nn_merge_kernel(NsArgs a) {
    const int q = blockIdx.x, lane = threadIdx.x, total = a.chunks * a.K;
    const double* c_sim = a.ws_sim + (size_t)q * total;
    const int32_t* c_idx = a.ws_idx + (size_t)q * total;
    double ls = __builtin_inf();
    int li = -1, nfound = 0;
    for (int k = 0; k < a.K; ++k) {
        double v = 0.0;
        int bi = -1;
        if (li >= 0 || k == 0)
            for (int e = lane; e < total; e += 64) {
                const int i = c_idx[e];
                if (i >= 0) ns_consider(c_sim[e], i, ls, li, v, bi);
            }
        ns_wave_best(v, bi);
        if (lane == 0) {
            a.sim[(size_t)q * a.K + k] = bi >= 0 ? v : __builtin_nan("");
            a.idx[(size_t)q * a.K + k] = bi;
        }
        nfound += bi >= 0;
        ls = v, li = bi;
    }
    if (lane == 0) a.found[q] = nfound;
}

struct GatherArgs {
    const int32_t* idx;
    const float* lib;
    long cs, fs;
    const int32_t* lib_lens;
    const int32_t* q_lens;
    int Q, K, N, Lmax, L, W;
    float* out;
    int32_t* out_len;
};

__global__ __launch_bounds__(kGatherThreads) void nn_gather_kernel(GatherArgs a) {
    const int qk = blockIdx.x, q = qk / a.K;
    const int i = a.idx[qk];
    const bool have = i >= 0 && i < a.N;
    const int n = have ? min(min(clamp_len(a.q_lens, q, a.L), clamp_len(a.lib_lens, i, a.Lmax)), a.L) : 0;
    if (threadIdx.x == 0) a.out_len[qk] = n;
    gather_winner_rows<kGatherThreads>(a.lib + (size_t)(have ? i : 0) * a.cs, a.fs, a.out + (size_t)qk * a.L * a.W, a.L, a.W, n);
}

int ns_chunks(int N) { return (N + kNsChunk - 1) / kNsChunk; }

bool ns_shape_ok(int Q, int N, int D, int K) {
    return Q >= 1 && N >= 1 && D >= 1 && D <= kNsMaxD && K >= 1 && K <= kNsMaxK && (Q + kNsTile - 1) / kNsTile <= 65535;
}

}  // namespace
}  // namespace dimx

using namespace dimx;

int dimx_op_pool_desc(const float* x, long clip_stride, long frame_stride, const int32_t* lens, int N, int T, int D, int kind,
                      double* desc, double* norm, void* stream) {
    DIMX_REQUIRE(x && lens && desc && norm, DIMX_ERR_ARG, "pool_desc: null operand");
    DIMX_REQUIRE(kind == 0 || kind == 1, DIMX_ERR_ARG, "pool_desc: kind=%d is neither 0 (max) nor 1 (mean)", kind);
    DIMX_REQUIRE(N >= 1 && T >= 1 && D >= 1, DIMX_ERR_ARG, "pool_desc: N=%d T=%d D=%d must be positive", N, T, D);
    DIMX_REQUIRE(clip_stride >= 0 && frame_stride >= 0, DIMX_ERR_ARG, "pool_desc: negative stride");
    PoolArgs a;
    a.x = x, a.cs = clip_stride, a.fs = frame_stride, a.lens = lens, a.N = N, a.T = T, a.D = D, a.kind = kind;
    a.desc = desc, a.norm = norm;
    hipLaunchKernelGGL(pool_desc_kernel, dim3(N), dim3(kPoolThreads), 0, (hipStream_t)stream, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

size_t dimx_op_nn_search_ws_bytes(int Q, int N, int D, int K) {
    if (!ns_shape_ok(Q, N, D, K)) return 0;
    return align_up((size_t)Q * ns_chunks(N) * K * (sizeof(double) + sizeof(int32_t)), 8);
}

int dimx_op_nn_search(const double* q_desc, long q_row_stride, const double* q_norm, const double* x_desc, long x_row_stride,
                      const double* x_norm, int Q, int N, int D, int K, int32_t* idx, double* sim, int32_t* found, double* sim_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(K >= 1 && K <= kNsMaxK, DIMX_ERR_ARG, "nn_search: K=%d outside 1..%d", K, kNsMaxK);
    DIMX_REQUIRE(D >= 1 && D <= kNsMaxD, DIMX_ERR_ARG, "nn_search: D=%d outside 1..%d", D, kNsMaxD);
    DIMX_REQUIRE(N >= 1 && Q >= 1, DIMX_ERR_ARG, "nn_search: Q=%d N=%d must be positive", Q, N);
    DIMX_REQUIRE(ns_shape_ok(Q, N, D, K), DIMX_ERR_ARG, "nn_search: Q=%d is more queries than one launch takes", Q);
    DIMX_REQUIRE(q_row_stride >= 0 && x_row_stride >= 0, DIMX_ERR_ARG, "nn_search: negative stride");
    DIMX_REQUIRE(q_desc && q_norm && x_desc && x_norm && idx && sim && found && workspace, DIMX_ERR_ARG, "nn_search: null operand");
    DIMX_REQUIRE(((uintptr_t)workspace & 7) == 0, DIMX_ERR_ARG, "nn_search: workspace not 8-byte aligned");
    const size_t need = dimx_op_nn_search_ws_bytes(Q, N, D, K);
    DIMX_REQUIRE(workspace_bytes >= need, DIMX_ERR_WORKSPACE, "nn_search: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    NsArgs a;
    a.qd = q_desc, a.q_ld = q_row_stride, a.qn = q_norm, a.xd = x_desc, a.x_ld = x_row_stride, a.xn = x_norm;
    a.Q = Q, a.N = N, a.D = D, a.K = K, a.chunks = ns_chunks(N);
    a.idx = idx, a.sim = sim, a.found = found, a.sim_out = sim_out;
    a.ws_sim = (double*)workspace;
    a.ws_idx = (int32_t*)(a.ws_sim + (size_t)Q * a.chunks * K);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)kNsTile * D + (size_t)kNsTile * kNsChunk) * sizeof(double);
    const int lds_max = (int)(((size_t)kNsTile * kNsMaxD + (size_t)kNsTile * kNsChunk) * sizeof(double));   // never this call's own size
    const dim3 grid((unsigned)a.chunks, (unsigned)((Q + kNsTile - 1) / kNsTile));
    // the instantiation is a function of D alone, and so is the arithmetic of every one of them: the same sums in the same order
#define DIMX_NS_LAUNCH(NI)                                                                                                          \
    do {                                                                                                                            \
        DIMX_HIP(hipFuncSetAttribute((const void*)nn_search_kernel<NI>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));      \
        hipLaunchKernelGGL(nn_search_kernel<NI>, grid, dim3(kNsThreads), lds, st, a);                                               \
    } while (0)
    if (D <= 64) DIMX_NS_LAUNCH(1);
    else if (D <= 256) DIMX_NS_LAUNCH(4);
    else DIMX_NS_LAUNCH(kNsMaxI);
#undef DIMX_NS_LAUNCH
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)Q), dim3(64), 0, st, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int dimx_op_nn_gather(const int32_t* idx, const float* lib_seq, long clip_stride, long frame_stride, const int32_t* lib_lens,
                      const int32_t* q_lens, int Q, int K, int N, int Lmax, int L, int W, float* out, int32_t* out_len, void* stream) {
    DIMX_REQUIRE(idx && lib_seq && lib_lens && q_lens && out && out_len, DIMX_ERR_ARG, "nn_gather: null operand");
    DIMX_REQUIRE(K >= 1 && K <= kNsMaxK, DIMX_ERR_ARG, "nn_gather: K=%d outside 1..%d", K, kNsMaxK);
    DIMX_REQUIRE(Q >= 1 && N >= 1 && Lmax >= 1 && L >= 1 && W >= 1, DIMX_ERR_ARG, "nn_gather: Q=%d N=%d Lmax=%d L=%d W=%d must be positive",
                 Q, N, Lmax, L, W);
    DIMX_REQUIRE((long)Q * K <= 0x7fffffffL && (long)L * W <= 0x7fffffffL, DIMX_ERR_ARG, "nn_gather: Q * K or L * W beyond one launch");
    DIMX_REQUIRE(clip_stride >= 0 && frame_stride >= 0, DIMX_ERR_ARG, "nn_gather: negative stride");
    GatherArgs a;
    a.idx = idx, a.lib = lib_seq, a.cs = clip_stride, a.fs = frame_stride, a.lib_lens = lib_lens, a.q_lens = q_lens;
    a.Q = Q, a.K = K, a.N = N, a.Lmax = Lmax, a.L = L, a.W = W, a.out = out, a.out_len = out_len;
    hipLaunchKernelGGL(nn_gather_kernel, dim3((unsigned)(Q * K)), dim3(kGatherThreads), 0, (hipStream_t)stream, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
