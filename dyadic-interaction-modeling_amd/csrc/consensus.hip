// consensus.hip -- consensus (minimum-Bayes-risk, medoid) best-of-S selection: per clip the try with the smallest total distance
// to the other S - 1 tries.  No ground truth enters; the definition is dimx/consensus.py.
//
// kind 0 (fd): the distance is the Frechet distance of frechet.hpp, which holds the arithmetic and its derivation; D[i, j] for
// i < j has try i as the first operand (S_i = A_i A_i^T, M = A_i^T S_j A_i).  What is specific here is the pairwise structure:
//   cons_factor_kernel (one block per (clip, try)): mean, tr S and S of the try; S goes to the workspace before the Jacobi
//                      overwrites it, then the factor A (S = A A^T).  Each try is factorised once, not once per pair.
//   cons_pair_kernel   (one block per (clip, i < j)): S_j from the workspace into LDS, T = S_j A_i, M = A_i^T T, the Jacobi on M,
//                      the scalar distance -> D[i, j] and D[j, i] (the same bits).  Rank rule and top_r as fd_try_kernel.
// kind 1 (l2): cons_l2_kernel (one block per (clip, i < j)): mean over the valid frames and the window's columns of (x_i - x_j)^2,
//   float64; a thread sums its elements e = thread, thread + 256, ... in that order, a wave adds by xor 32, 16, ... 1, the four
//   waves are added in wave order.
// cons_pick_kernel (one block per clip): risk[i] = sum over j != i of D[i, j] in ascending j from zero, the zero diagonal of D,
//   the first minimum (NaN counts as +inf), the ok flag, the gather of the winner's rows and token row.
// No atomics, no host synchronisation, no allocation; frames t >= lens[j] are never loaded; every sum has an order that depends
// on the shapes only and a block's arithmetic depends on its own inputs only: repeated calls and identical tries give identical bits.
#include "frechet.hpp"
#include "pick_gather.hpp"

namespace dimx {
namespace {

using CsT = frechet::Traits<256, 64>;
constexpr int kCsThreads = CsT::THREADS;
constexpr int kCsMaxF = CsT::MAXF;
constexpr int kCsWaves = kCsThreads / 64;

struct CsArgs {
    const float* yp;
    long yp_cs, yp_ss, yp_fs;
    const int32_t* lens;
    int B, S, P, L, W, c0, F;   // P = S (S - 1) / 2 pairs per clip
    double* D;                  // [B][S][S]: the caller's dist, or the head of the workspace
    double* risk;
    int32_t* win;
    uint8_t* ok;
    float* best;
    const int32_t* tokens;
    long tok_rs;
    int n_tok;
    int32_t* best_tokens;
    double* wsA;        // [B*S][F*F]  A, column-major, dense
    double* wsS;        // [B*S][F*F]  S, column-major, dense
    double* wsMu;       // [B*S][F]
    double* wsTr;       // [B*S]
    int32_t* wsSweeps;  // [B*S + B*P]
};

struct CsRows {
    const float* x;
    long fs;
    __device__ __forceinline__ double at(int t, int c) const { return (double)x[(size_t)t * fs + c]; }
};

// pair p of a clip -> (i, j), i < j, in the order (0,1), (0,2), .., (0,S-1), (1,2), ..
__device__ __forceinline__ void pair_of(int p, int S, int& i, int& j) {
    i = 0;
    int row = S - 1;
    while (p >= row) {
        p -= row;
        ++i;
        --row;
    }
    j = i + 1 + p;
}

__device__ __forceinline__ void write_pair(double* D, int S, int i, int j, double d) {
    D[(size_t)i * S + j] = d;
    D[(size_t)j * S + i] = d;
}

__global__ __launch_bounds__(kCsThreads) void cons_factor_kernel(CsArgs a) {
    extern __shared__ double cs_dyn[];
    __shared__ frechet::Smem<CsT> sm;
    const int bs = blockIdx.x, b = bs / a.S, s = bs - b * a.S, F = a.F, ld = CsT::ld(F);
    const int n = frechet::valid_frames(a.lens, a.L, b);
    if (n < 2) {   // no covariance: every distance of the clip is NaN (cons_pair_kernel), nothing of the workspace is read
        if (threadIdx.x == 0) a.wsSweeps[bs] = 0;
        return;
    }
    double* tile = cs_dyn;                              // kTile x kTileLd
    double* G = cs_dyn + frechet::kTile * CsT::kTileLd; // F x ld: S
    const frechet::TileIdx<CsT> ix(F);
    const CsRows rw{a.yp + (size_t)b * a.yp_cs + (size_t)s * a.yp_ss + a.c0, a.yp_fs};
    frechet::mean<CsT>(rw, n, F, sm);
    frechet::cov<CsT>(rw, n, F, sm, ix, tile, G, ld);
    frechet::trace<CsT>(G, F, ld, sm, 0);
    frechet::store_dense<CsT>(G, F, ld, a.wsS + (size_t)bs * F * F);
    __syncthreads();   // S is out before the Jacobi rotates it
    const int sweeps = frechet::eigen<CsT>(G, F, ld, min(F, n - 1), sm);
    frechet::write_factor<CsT>(G, F, ld, sm, a.wsA + (size_t)bs * F * F);
    if (threadIdx.x < F) a.wsMu[(size_t)bs * F + threadIdx.x] = sm.mu[threadIdx.x];
    if (threadIdx.x == 0) {
        a.wsTr[bs] = sm.scal[0];
        a.wsSweeps[bs] = sweeps;
    }
}

__global__ __launch_bounds__(kCsThreads) void cons_pair_kernel(CsArgs a) {
    extern __shared__ double cs_dyn[];
    __shared__ frechet::Smem<CsT> sm;
    const int b = blockIdx.x / a.P, F = a.F, ld = CsT::ld(F);
    int i, j;
    pair_of(blockIdx.x - b * a.P, a.S, i, j);
    double* D = a.D + (size_t)b * a.S * a.S;
    const int n = frechet::valid_frames(a.lens, a.L, b);
    if (n < 2) {
        if (threadIdx.x == 0) {
            write_pair(D, a.S, i, j, __builtin_nan(""));
            a.wsSweeps[(size_t)a.B * a.S + blockIdx.x] = 0;
        }
        return;
    }
    const size_t ti = (size_t)b * a.S + i, tj = (size_t)b * a.S + j;
    double* tile = cs_dyn;                              // kTile x kTileLd
    double* G = cs_dyn + frechet::kTile * CsT::kTileLd; // F x ld: S_j, then T, M
    const double* A = a.wsA + ti * F * F;
    const frechet::TileIdx<CsT> ix(F);
    if (threadIdx.x < F) {
        sm.mu1[threadIdx.x] = a.wsMu[ti * F + threadIdx.x];
        sm.mu[threadIdx.x] = a.wsMu[tj * F + threadIdx.x];
    }
    if (threadIdx.x == 0) sm.scal[1] = a.wsTr[tj];
    frechet::load_dense<CsT>(a.wsS + tj * F * F, F, ld, G);
    frechet::mean_diff2<CsT>(F, sm);
    frechet::product<CsT>(A, F, ix, tile, G, ld, false);
    frechet::product<CsT>(A, F, ix, tile, G, ld, true);
    const int sweeps = frechet::eigen<CsT>(G, F, ld, min(F, n - 1), sm);
    if (threadIdx.x == 0) {
        write_pair(D, a.S, i, j, frechet::distance<CsT>(F, sm, a.wsTr[ti]));
        a.wsSweeps[(size_t)a.B * a.S + blockIdx.x] = sweeps;
    }
}

__global__ __launch_bounds__(kCsThreads) void cons_l2_kernel(CsArgs a) {
    __shared__ double sh[kCsWaves];
    const int b = blockIdx.x / a.P, F = a.F;
    int i, j;
    pair_of(blockIdx.x - b * a.P, a.S, i, j);
    double* D = a.D + (size_t)b * a.S * a.S;
    const int n = frechet::valid_frames(a.lens, a.L, b);
    if (n < 2) {
        if (threadIdx.x == 0) write_pair(D, a.S, i, j, __builtin_nan(""));
        return;
    }
    const float* xi = a.yp + (size_t)b * a.yp_cs + (size_t)i * a.yp_ss + a.c0;
    const float* xj = a.yp + (size_t)b * a.yp_cs + (size_t)j * a.yp_ss + a.c0;
    const int total = n * F;
    double acc = 0.0;
    for (int e = threadIdx.x; e < total; e += kCsThreads) {
        const int t = e / F, c = e - t * F;
        const double d = (double)xi[(size_t)t * a.yp_fs + c] - (double)xj[(size_t)t * a.yp_fs + c];
        acc = fma(d, d, acc);
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        for (int w = 1; w < kCsWaves; ++w) t += sh[w];
        write_pair(D, a.S, i, j, t / (double)total);
    }
}

__global__ __launch_bounds__(kCsThreads) void cons_pick_kernel(CsArgs a) {
    __shared__ int sh_win, sh_ok;
    const int b = blockIdx.x, S = a.S;
    double* D = a.D + (size_t)b * S * S;
    double* risk = a.risk + (size_t)b * S;
    for (int i = threadIdx.x; i < S; i += kCsThreads) {
        double r = 0.0;
        for (int j = 0; j < S; ++j)
            if (j != i) r += D[(size_t)i * S + j];
        risk[i] = r;
        D[(size_t)i * S + i] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double inf = __builtin_inf();
        double cur = inf;
        int w = 0, fin = 0;
        for (int s = 0; s < S; ++s) {
            double d = risk[s];
            if (d != d) d = inf;
            if (d > -inf && d < inf) fin = 1;
            if (d < cur) {
                cur = d;
                w = s;
            }
        }
        a.win[b] = w;
        a.ok[b] = (uint8_t)fin;
        sh_win = w;
        sh_ok = fin;
    }
    __syncthreads();
    if (a.best) {
        const int n = sh_ok ? frechet::valid_frames(a.lens, a.L, b) : 0;
        gather_winner_rows<kCsThreads>(a.yp + (size_t)b * a.yp_cs + (size_t)sh_win * a.yp_ss, a.yp_fs,
                                       a.best + (size_t)b * a.L * a.W, a.L, a.W, n);
    }
    if (a.best_tokens) {
        const int32_t* src = a.tokens + ((size_t)b * S + sh_win) * a.tok_rs;
        int32_t* dst = a.best_tokens + (size_t)b * a.n_tok;
        for (int c = threadIdx.x; c < a.n_tok; c += kCsThreads) dst[c] = sh_ok ? src[c] : -100;
    }
}

// blocks of the pair stage, or -1 when they (or the B * S blocks of the factor stage) do not fit a launch
long cs_pair_blocks(int B, int S) {
    const long P = (long)S * (S - 1) / 2;
    return (P > 0x7fffffffL / B || (long)B * S > 0x7fffffffL) ? -1 : P * B;
}

size_t cs_ws_doubles(int B, int S, int F, int kind) {
    const size_t BS = (size_t)B * S;
    return BS * S + (kind == 0 ? BS * (2 * (size_t)F * F + F + 1) : 0);
}

}  // namespace
}  // namespace dimx

using namespace dimx;

size_t dimx_op_consensus_select_ws_bytes(int B, int S, int F, int kind) {
    if (B <= 0 || S <= 0 || F < 1 || F > kCsMaxF || (kind != 0 && kind != 1) || cs_pair_blocks(B, S) < 0) return 0;
    const size_t sweeps = kind == 0 ? (size_t)B * S + (size_t)cs_pair_blocks(B, S) : 0;
    return cs_ws_doubles(B, S, F, kind) * sizeof(double) + sweeps * sizeof(int32_t);
}

int dimx_op_consensus_select(const float* y_pred, long yp_clip_stride, long yp_sample_stride, long yp_frame_stride,
                             const int32_t* lens, int B, int S, int L, int W, int c0, int F, int kind, double* dist, double* risk,
                             int32_t* win, uint8_t* ok, float* best, const int32_t* tokens, long tok_row_stride, int n_tok,
                             int32_t* best_tokens, void* workspace, size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(y_pred && lens && risk && win && ok && workspace, DIMX_ERR_ARG, "consensus_select: null operand");
    DIMX_REQUIRE(kind == 0 || kind == 1, DIMX_ERR_ARG, "consensus_select: kind=%d is neither 0 (fd) nor 1 (l2)", kind);
    DIMX_REQUIRE(B > 0 && S > 0 && L > 0 && W > 0, DIMX_ERR_ARG, "consensus_select: B=%d S=%d L=%d W=%d must be positive", B, S, L, W);
    DIMX_REQUIRE(F >= 1 && F <= kCsMaxF, DIMX_ERR_ARG, "consensus_select: F=%d outside 1..%d", F, kCsMaxF);
    DIMX_REQUIRE(c0 >= 0 && c0 <= W - F, DIMX_ERR_ARG, "consensus_select: columns [%d, %d) leave the row of %d", c0, c0 + F, W);
    DIMX_REQUIRE(yp_clip_stride >= 0 && yp_sample_stride >= 0 && yp_frame_stride >= 0 && tok_row_stride >= 0, DIMX_ERR_ARG,
                 "consensus_select: negative stride");
    DIMX_REQUIRE(!best_tokens || (tokens && n_tok >= 1), DIMX_ERR_ARG, "consensus_select: best_tokens needs tokens and n_tok=%d positive",
                 n_tok);
    const long pair_blocks = cs_pair_blocks(B, S);
    DIMX_REQUIRE(pair_blocks >= 0, DIMX_ERR_ARG, "consensus_select: B=%d clips of S=%d tries are more pairs than one launch takes", B, S);
    DIMX_REQUIRE(((uintptr_t)workspace & 7) == 0, DIMX_ERR_ARG, "consensus_select: workspace not 8-byte aligned");
    const size_t need = dimx_op_consensus_select_ws_bytes(B, S, F, kind);
    DIMX_REQUIRE(workspace_bytes >= need, DIMX_ERR_ARG, "consensus_select: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const size_t BS = (size_t)B * S;
    CsArgs a;
    a.yp = y_pred, a.yp_cs = yp_clip_stride, a.yp_ss = yp_sample_stride, a.yp_fs = yp_frame_stride;
    a.lens = lens, a.B = B, a.S = S, a.P = (int)((long)S * (S - 1) / 2), a.L = L, a.W = W, a.c0 = c0, a.F = F;
    a.D = dist ? dist : (double*)workspace;
    a.risk = risk, a.win = win, a.ok = ok, a.best = best;
    a.tokens = tokens, a.tok_rs = tok_row_stride, a.n_tok = n_tok, a.best_tokens = best_tokens;
    a.wsA = (double*)workspace + BS * S;
    a.wsS = a.wsA + BS * F * F;
    a.wsMu = a.wsS + BS * F * F;
    a.wsTr = a.wsMu + BS * F;
    a.wsSweeps = (int32_t*)(a.wsTr + BS);
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) {
        const size_t lds = CsT::lds_bytes(F);
        const int lds_max = (int)CsT::lds_bytes(kCsMaxF);   // never this call's own size: frechet.hpp, Traits::lds_bytes
        DIMX_HIP(hipFuncSetAttribute((const void*)cons_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        DIMX_HIP(hipFuncSetAttribute((const void*)cons_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        hipLaunchKernelGGL(cons_factor_kernel, dim3((unsigned)BS), dim3(kCsThreads), lds, st, a);
        if (pair_blocks > 0) hipLaunchKernelGGL(cons_pair_kernel, dim3((unsigned)pair_blocks), dim3(kCsThreads), lds, st, a);
    } else if (pair_blocks > 0) {
        hipLaunchKernelGGL(cons_l2_kernel, dim3((unsigned)pair_blocks), dim3(kCsThreads), 0, st, a);
    }
    hipLaunchKernelGGL(cons_pick_kernel, dim3(B), dim3(kCsThreads), 0, st, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
