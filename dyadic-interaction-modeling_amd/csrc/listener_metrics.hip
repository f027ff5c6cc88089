// listener_metrics.hip -- the listener evaluation metrics (print_metrics / print_metrics_full) per clip.
//
// Reference: code/mymetrics.py:7-120 around calculate_activation_statistics / calculate_frechet_distance / sts,
// code/metrics/eval_utils.py:6-46,85-91.  Everything the two functions print except SID is made of
//   (a) per clip and per column window the Frechet distance of [x | gt] against [x | pred]
//           fd = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2),  mean and unbiased covariance over the valid frames,
//   (b) per clip first and second moments of gt, pred, x and gt - pred over the pose (0:6) and exp (6:56) columns,
// and the operator leaves exactly these, in float64, for the accumulator on the Python side (dimx.metrics.ListenerMetrics).
//
// Two launches, no atomics, no host synchronisation, no block waits for another:
//   lm_moments_kernel (one block of 256 per clip): two passes over the clip's valid frames -- the means first, then the centred
//       sums, the squared error and the STS sum -- and the first and last row of gt - pred.  A lane owns one column and every
//       fourth frame; the per-lane partials are summed in lane order by one thread per quantity.
//   lm_fd_kernel (one block of 512 per (window, clip), the widest windows first): the arithmetic of fd_select.hip with F up to 112.
//       S1 -> one-sided Jacobi -> A = G Lambda^-1/2 (S1 = A A^T) -> workspace;  S2;  T = S2 A;  M = A^T T;  the same Jacobi on M;
//       tr sqrt(S1 S2) = sum of the square roots of the r = min(F, n - 1) largest eigenvalues of M (the rank rule of fd_select.hip).
// LDS: ONE F x F float64 matrix (column stride F | 1: 112 x 113 x 8 = 101 248 B) plus a 16-row panel (16 x 113 x 8 = 14 464 B) that
// is the frame tile of the covariance pass and the k-panel of A in the two products.  S1, S2, T and M take turns in the one matrix;
// A is the only second operand and comes back from the workspace, panel by panel, through L2 (the block wrote it itself: a
// workgroup-scope fence and the barrier order the write before the reads).  Two matrices of this size do not fit the 160 KiB of a CU.
// Block shape: 512 threads.  A Jacobi step rotates m/2 <= 56 disjoint column pairs with 8 lanes each = 448 lanes, so the step stays
// one round of LDS traffic and one barrier as in fd_select.hip; a lane holds F/8 <= 14 rows of its two columns.  The products and the
// covariance use the 512 threads as 16 x 32 with a 7 x 4 register tile.  The sweep loop is bounded (kLmMaxSweeps).
// Every sum has a fixed order that depends on the shapes only: two calls on the same inputs are bit-identical.
// Frames t >= lens[b] are never loaded.  All address arithmetic is 64-bit.
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kLmThreads = 512;
constexpr int kLmMomThreads = 256;
constexpr int kLmMaxF = 112;
constexpr int kLmMaxWin = 8;
constexpr int kLmTile = 16;               // rows of the panel: frames of the covariance pass, k of the products
constexpr int kLmTileLd = kLmMaxF + 1;    // panel row stride (doubles)
constexpr int kLmMaxSweeps = 30;
constexpr int kLmCols = 56, kLmPose = 6;
constexpr int kLmGroup = 10;              // moments per group, include/dimx.h
constexpr int kLmEdge = 1 + 2 * kLmGroup; // first column of the edge block
static_assert(kLmEdge + 2 * kLmCols == DIMX_LM_ROW, "moment row layout");

__host__ __device__ inline int lm_ld(int F) { return F | 1; }   // odd column stride, as fd_select.hip

struct LmArgs {
    const float* yt;
    long yt_cs, yt_fs;
    const float* yp;
    long yp_cs, yp_fs;
    const float* x;
    long x_cs, x_fs;
    const int32_t* lens;
    int B, L, n_win;
    int win[kLmMaxWin][4];   // (xc0, xF, yc0, yF)
    int order[kLmMaxWin];    // window indices, the widest first
    double* fd;              // [B][n_win]
    double* mom;             // [B][DIMX_LM_ROW]
    double* wsA;             // [n_win][B][Fmax*Fmax]  A, column-major, dense (stride F of its window)
    size_t a_stride;         // Fmax*Fmax
    int32_t* wsSweeps;       // [2][n_win][B]
};

__device__ __forceinline__ int lm_valid_frames(const LmArgs& a, int b) {
    const int n = a.lens[b];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

// ------------------------------------------------------------------------------------------------ moments
__global__ __launch_bounds__(kLmMomThreads) void lm_moments_kernel(LmArgs a) {
    __shared__ double part[7][kLmMomThreads];
    __shared__ double mean[2][3];
    const int b = blockIdx.x, n = lm_valid_frames(a, b);
    double* out = a.mom + (size_t)b * DIMX_LM_ROW;
    if (n < 1) {
        for (int e = threadIdx.x; e < DIMX_LM_ROW; e += kLmMomThreads) out[e] = 0.0;
        return;
    }
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool on = c < kLmCols;
    const float* gt = a.yt + (size_t)b * a.yt_cs + c;
    const float* pr = a.yp + (size_t)b * a.yp_cs + c;
    const float* xs = a.x + (size_t)b * a.x_cs + c;
    // pass 1: the sums of gt, pred, x per lane
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (on)
        for (int t = g; t < n; t += 4) {
            s0 += (double)gt[(size_t)t * a.yt_fs];
            s1 += (double)pr[(size_t)t * a.yp_fs];
            s2 += (double)xs[(size_t)t * a.x_fs];
        }
    part[0][threadIdx.x] = s0, part[1][threadIdx.x] = s1, part[2][threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < 6) {   // (group, quantity): frame groups outside, the group's columns inside, in index order
        const int grp = threadIdx.x / 3, q = threadIdx.x - 3 * grp;
        const int c0 = grp ? kLmPose : 0, c1 = grp ? kLmCols : kLmPose;
        double s = 0.0;
        for (int gg = 0; gg < 4; ++gg)
            for (int cc = c0; cc < c1; ++cc) s += part[q][gg * 64 + cc];
        mean[grp][q] = s / ((double)n * (double)(c1 - c0));
    }
    __syncthreads();
    // pass 2: the centred sums
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sse, m2 gt, m2 pred, m2 x, c(gt,x), c(pred,x), sts
    if (on) {
        const int grp = c < kLmPose ? 0 : 1;
        const double mg = mean[grp][0], mp = mean[grp][1], mx = mean[grp][2];
        for (int t = g; t < n; t += 4) {
            const double G = (double)gt[(size_t)t * a.yt_fs], P = (double)pr[(size_t)t * a.yp_fs], X = (double)xs[(size_t)t * a.x_fs];
            const double d = G - P, dg = G - mg, dp = P - mp, dx = X - mx;
            v[0] += d * d;
            v[1] += dg * dg;
            v[2] += dp * dp;
            v[3] += dx * dx;
            v[4] += dg * dx;
            v[5] += dp * dx;
            if (t >= 1) {
                const double G0 = (double)gt[(size_t)(t - 1) * a.yt_fs], P0 = (double)pr[(size_t)(t - 1) * a.yp_fs];
                const double e = (G - G0) - (P - P0);
                v[6] += e * e;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 7; ++q) part[q][threadIdx.x] = v[q];
    __syncthreads();
    if (threadIdx.x < 14) {
        const int grp = threadIdx.x / 7, q = threadIdx.x - 7 * grp;
        const int c0 = grp ? kLmPose : 0, c1 = grp ? kLmCols : kLmPose;
        double s = 0.0;
        for (int gg = 0; gg < 4; ++gg)
            for (int cc = c0; cc < c1; ++cc) s += part[q][gg * 64 + cc];
        // row slots: 0 sse | 1 mean gt, 2 m2 gt | 3 mean pred, 4 m2 pred | 5 mean x, 6 m2 x | 7 c(gt,x) | 8 c(pred,x) | 9 sts
        const int slot = q == 0 ? 0 : q == 1 ? 2 : q == 2 ? 4 : q == 3 ? 6 : q == 4 ? 7 : q == 5 ? 8 : 9;
        out[1 + kLmGroup * grp + slot] = s;
    }
    if (threadIdx.x < 6) {
        const int grp = threadIdx.x / 3, q = threadIdx.x - 3 * grp;
        out[1 + kLmGroup * grp + 1 + 2 * q] = mean[grp][q];
    }
    if (threadIdx.x == 0) out[0] = (double)n;
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kLmCols) {          // first valid row of d
        out[kLmEdge + c] = (double)gt[0] - (double)pr[0];
    }
    if (threadIdx.x >= 128 && threadIdx.x < 128 + kLmCols) {        // last valid row of d
        out[kLmEdge + kLmCols + c] = (double)gt[(size_t)(n - 1) * a.yt_fs] - (double)pr[(size_t)(n - 1) * a.yp_fs];
    }
}

// ------------------------------------------------------------------------------------------------ distances
struct LmSmem {
    double red[4][128];      // partial sums of lm_mean; red[0] is reused as the keep flags of lm_top_r
    double mu[kLmMaxF];
    double mu1[kLmMaxF];
    double sig[kLmMaxF];
    double scal[4];          // tr S1, tr S2, |mu1 - mu2|^2
};

// the operand rows [x[:, xc0:xc0+xF] | y[:, yc0:yc0+yF]] of one clip
struct LmRows {
    const float* x;
    long x_fs;
    const float* y;
    long y_fs;
    int xF;
    __device__ __forceinline__ double at(int t, int c) const {
        return c < xF ? (double)x[(size_t)t * x_fs + c] : (double)y[(size_t)t * y_fs + (c - xF)];
    }
};

// mean over the n valid frames of the F operand columns -> sm.mu
__device__ void lm_mean(const LmRows& rw, int n, int F, LmSmem& sm) {
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    double acc = 0.0;
    if (c < F)
        for (int t = g; t < n; t += 4) acc += rw.at(t, c);
    sm.red[g][c] = acc;
    __syncthreads();
    if (threadIdx.x < F) sm.mu[c] = (((sm.red[0][c] + sm.red[1][c]) + sm.red[2][c]) + sm.red[3][c]) / (double)n;
    __syncthreads();
}

// the 16 x 32 thread grid of the covariance and of the products: rows ti + 16 p (p < 7), columns tj + 32 q (q < 4), clamped to F - 1
struct LmTileIdx {
    int ti, tj, ri[7], cj[4], np, nq;
    __device__ explicit LmTileIdx(int F) {
        ti = threadIdx.x >> 5, tj = threadIdx.x & 31;
        np = (F + 15) >> 4, nq = (F + 31) >> 5;   // register tiles that hold a column of the window at all (block-uniform)
#pragma unroll
        for (int p = 0; p < 7; ++p) ri[p] = min(ti + 16 * p, F - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) cj[q] = min(tj + 32 * q, F - 1);
    }
};

__device__ __forceinline__ void lm_acc_zero(double (&acc)[7][4]) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
}

__device__ __forceinline__ void lm_acc_fma(const LmTileIdx& ix, const double (&u)[7], const double (&v)[4], double (&acc)[7][4]) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
        if (p < ix.np)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < ix.nq) acc[p][q] = fma(u[p], v[q], acc[p][q]);
}

// acc -> out[j * ld + i] * scale for the entries of the window; the caller has synchronised the readers of out
__device__ __forceinline__ void lm_acc_store(const LmTileIdx& ix, int F, const double (&acc)[7][4], double scale, double* out, int ld) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ix.ti + 16 * p < F && ix.tj + 32 * q < F) out[ix.cj[q] * ld + ix.ri[p]] = acc[p][q] * scale;
    __syncthreads();
}

// unbiased covariance of the centred frames -> out (column-major, stride ld); tile is the panel and does not alias out
__device__ void lm_cov(const LmRows& rw, int n, int F, const LmSmem& sm, const LmTileIdx& ix, double* tile, double* out, int ld) {
    double acc[7][4];
    lm_acc_zero(acc);
    for (int t0 = 0; t0 < n; t0 += kLmTile) {
        for (int e = threadIdx.x; e < kLmTile * 128; e += kLmThreads) {
            const int tt = e >> 7, c = e & 127;
            if (c < F) tile[tt * kLmTileLd + c] = t0 + tt < n ? rw.at(t0 + tt, c) - sm.mu[c] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int tt = 0; tt < kLmTile; ++tt) {
            double u[7], v[4];
#pragma unroll
            for (int p = 0; p < 7; ++p) u[p] = tile[tt * kLmTileLd + ix.ri[p]];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = tile[tt * kLmTileLd + ix.cj[q]];
            lm_acc_fma(ix, u, v, acc);
        }
        __syncthreads();
    }
    lm_acc_store(ix, F, acc, 1.0 / (double)(n - 1), out, ld);
}

// rows [k0, k0 + 16) of A (global, column-major, dense stride F) -> tile[kk][j]; a column's 16 values are one 128-byte run
__device__ __forceinline__ void lm_stage_a(const double* A, int F, int k0, double* tile) {
    for (int e = threadIdx.x; e < kLmTile * F; e += kLmThreads) {
        const int j = e >> 4, kk = e & 15;
        tile[kk * kLmTileLd + j] = k0 + kk < F ? A[(size_t)j * F + k0 + kk] : 0.0;
    }
    __syncthreads();
}

// G <- S A   (S = G on entry, symmetric: S[i][k] is read as G[k * ld + i])
// G <- A^T G (second = true)
__device__ void lm_product(const double* A, int F, const LmTileIdx& ix, double* tile, double* G, int ld, bool second) {
    double acc[7][4];
    lm_acc_zero(acc);
    for (int k0 = 0; k0 < F; k0 += kLmTile) {
        lm_stage_a(A, F, k0, tile);
        const int kn = min(kLmTile, F - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const int k = k0 + kk;
            double u[7], v[4];
            if (!second) {
#pragma unroll
                for (int p = 0; p < 7; ++p) u[p] = G[k * ld + ix.ri[p]];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tile[kk * kLmTileLd + ix.cj[q]];
            } else {
#pragma unroll
                for (int p = 0; p < 7; ++p) u[p] = tile[kk * kLmTileLd + ix.ri[p]];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = G[ix.cj[q] * ld + k];
            }
            lm_acc_fma(ix, u, v, acc);
        }
        __syncthreads();
    }
    lm_acc_store(ix, F, acc, 1.0, G, ld);
}

// trace of the F x F matrix m (stride ld), summed in index order -> sm.scal[slot]
__device__ void lm_trace(const double* m, int F, int ld, LmSmem& sm, int slot) {
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < F; ++i) t += m[i * ld + i];
        sm.scal[slot] = t;
    }
    __syncthreads();
}

// squared column norms of g -> sm.sig (thread c owns column c)
__device__ void lm_col_norms2(const double* g, int F, int ld, LmSmem& sm) {
    if (threadIdx.x < F) {
        double s = 0.0;
        for (int r = 0; r < F; ++r) s = fma(g[threadIdx.x * ld + r], g[threadIdx.x * ld + r], s);
        sm.sig[threadIdx.x] = s;
    }
    __syncthreads();
}

// One-sided cyclic Jacobi on the columns of g (F x F, column-major, stride ld), F <= 8 * NK: fd_select.hip's, with NK rows per lane.
// On return the columns are mutually orthogonal (g <- g V): for a symmetric positive semi-definite input their norms are its
// eigenvalues.  Returns the sweeps done.
template <int NK>
__device__ int lm_jacobi(double* g, int F, int ld, LmSmem& sm) {
    lm_col_norms2(g, F, ld, sm);
    double fro2 = 0.0;
    for (int c = 0; c < F; ++c) fro2 += sm.sig[c];
    const double tiny = 1e-28 * fro2;   // columns whose product is below this are orthogonal as far as the result can tell
    const int m = (F + 1) & ~1, pairs = m >> 1, pi = threadIdx.x >> 3, sub = threadIdx.x & 7;
    int sweeps = 0;
    for (int sw = 0; sw < kLmMaxSweeps; ++sw) {
        int rotated = 0;
        for (int r = 0; r < m - 1; ++r) {
            int p = 0, q = 0;
            bool live = pi < pairs;
            if (live) {
                if (pi == 0) {
                    p = m - 1;
                    q = r;
                } else {
                    p = (r + pi) % (m - 1);
                    q = (r - pi + (m - 1)) % (m - 1);
                }
                live = p < F && q < F;   // m - 1 is the bye of an odd F
            }
            double gp[NK], gq[NK];
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int row = sub + 8 * k;
                const bool in = live && row < F;
                gp[k] = in ? g[p * ld + row] : 0.0;
                gq[k] = in ? g[q * ld + row] : 0.0;
                al = fma(gp[k], gp[k], al);
                be = fma(gq[k], gq[k], be);
                ga = fma(gp[k], gq[k], ga);
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {   // butterfly over the pair's 8 lanes: every lane ends with the same bits
                al += __shfl_xor(al, o);
                be += __shfl_xor(be, o);
                ga += __shfl_xor(ga, o);
            }
            const double aga = fabs(ga);
            if (live && aga > tiny && aga * aga > 1e-26 * al * be) {
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int row = sub + 8 * k;
                    if (row < F) {
                        g[p * ld + row] = c * gp[k] - s * gq[k];
                        g[q * ld + row] = s * gp[k] + c * gq[k];
                    }
                }
                rotated = 1;
            }
            __syncthreads();
        }
        ++sweeps;
        if (!__syncthreads_or(rotated)) break;
    }
    return sweeps;
}

__device__ int lm_jacobi_any(double* g, int F, int ld, LmSmem& sm) {
    if (F <= 8) return lm_jacobi<1>(g, F, ld, sm);
    if (F <= 64) return lm_jacobi<8>(g, F, ld, sm);
    return lm_jacobi<14>(g, F, ld, sm);
}

// sm.sig holds F non-negative values; sm.red[0][c] = 1 when sig[c] is among the r largest (ties: the lower index first)
__device__ void lm_top_r(int F, int r, LmSmem& sm) {
    if (threadIdx.x < F) {
        const int c = threadIdx.x;
        const double v = sm.sig[c];
        int rank = 0;
        for (int d = 0; d < F; ++d) rank += (sm.sig[d] > v || (sm.sig[d] == v && d < c)) ? 1 : 0;
        sm.red[0][c] = rank < r ? 1.0 : 0.0;
    }
    __syncthreads();
}

// eigenvalues of the symmetric positive semi-definite g (Jacobi in place) -> sm.sig, keep flags of the r largest -> sm.red[0]
__device__ int lm_eigen(double* g, int F, int ld, int r, LmSmem& sm) {
    const int sweeps = lm_jacobi_any(g, F, ld, sm);
    lm_col_norms2(g, F, ld, sm);
    if (threadIdx.x < F) sm.sig[threadIdx.x] = sqrt(sm.sig[threadIdx.x]);
    __syncthreads();
    lm_top_r(F, r, sm);
    return sweeps;
}

__global__ __launch_bounds__(kLmThreads) void lm_fd_kernel(LmArgs a) {
    extern __shared__ double lm_dyn[];
    __shared__ LmSmem sm;
    const int pos = blockIdx.x / a.B, b = blockIdx.x - pos * a.B, w = a.order[pos];
    const int xc0 = a.win[w][0], xF = a.win[w][1], yc0 = a.win[w][2], F = xF + a.win[w][3], ld = lm_ld(F);
    const int n = lm_valid_frames(a, b);
    const size_t slot = (size_t)w * a.B + b;
    if (n < 2) {   // no covariance: nothing of the inputs or of the workspace is read
        if (threadIdx.x == 0) {
            a.fd[(size_t)b * a.n_win + w] = __builtin_nan("");
            a.wsSweeps[slot] = 0;
            a.wsSweeps[(size_t)a.n_win * a.B + slot] = 0;
        }
        return;
    }
    double* tile = lm_dyn;                         // kLmTile x kLmTileLd
    double* G = lm_dyn + kLmTile * kLmTileLd;      // F x ld: S1, then S2, T, M
    double* A = a.wsA + slot * a.a_stride;
    const LmTileIdx ix(F);
    const int r = min(F, n - 1);
    LmRows rw;
    rw.x = a.x + (size_t)b * a.x_cs + xc0, rw.x_fs = a.x_fs, rw.xF = xF;
    // target side: mu1, tr S1, A
    rw.y = a.yt + (size_t)b * a.yt_cs + yc0, rw.y_fs = a.yt_fs;
    lm_mean(rw, n, F, sm);
    lm_cov(rw, n, F, sm, ix, tile, G, ld);
    lm_trace(G, F, ld, sm, 0);
    if (threadIdx.x < F) sm.mu1[threadIdx.x] = sm.mu[threadIdx.x];
    const int sweeps1 = lm_eigen(G, F, ld, r, sm);   // sm.sig = lambda_i, columns of G = lambda_i v_i
    for (int e = threadIdx.x; e < F * F; e += kLmThreads) {
        const int c = e / F, rr = e - c * F;
        const double lam = sm.sig[c];
        A[e] = (sm.red[0][c] != 0.0 && lam > 0.0) ? G[c * ld + rr] / sqrt(lam) : 0.0;
    }
    __threadfence_block();   // A is read back by this block only
    __syncthreads();
    // candidate side: mu2, S2, T = S2 A, M = A^T T
    rw.y = a.yp + (size_t)b * a.yp_cs + yc0, rw.y_fs = a.yp_fs;
    lm_mean(rw, n, F, sm);
    lm_cov(rw, n, F, sm, ix, tile, G, ld);
    lm_trace(G, F, ld, sm, 1);
    if (threadIdx.x == 0) {   // |mu1 - mu2|^2 in column order
        double d2 = 0.0;
        for (int c = 0; c < F; ++c) {
            const double d = sm.mu1[c] - sm.mu[c];
            d2 = fma(d, d, d2);
        }
        sm.scal[2] = d2;
    }
    lm_product(A, F, ix, tile, G, ld, false);
    lm_product(A, F, ix, tile, G, ld, true);
    const int sweeps2 = lm_eigen(G, F, ld, r, sm);
    if (threadIdx.x == 0) {
        double trs = 0.0;
        for (int c = 0; c < F; ++c) trs += sm.red[0][c] != 0.0 ? sqrt(sm.sig[c]) : 0.0;
        a.fd[(size_t)b * a.n_win + w] = sm.scal[2] + sm.scal[0] + sm.scal[1] - 2.0 * trs;
        a.wsSweeps[slot] = sweeps1;
        a.wsSweeps[(size_t)a.n_win * a.B + slot] = sweeps2;
    }
}

}  // namespace
}  // namespace dimx

using namespace dimx;

size_t dimx_op_listener_metrics_ws_bytes(int B, int n_win, int F) {
    if (B < 1 || n_win < 1 || n_win > kLmMaxWin || F < 1 || F > kLmMaxF) return 0;
    return (size_t)B * n_win * ((size_t)F * F * sizeof(double) + 2 * sizeof(int32_t));
}

int dimx_op_listener_metrics(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                             long yp_frame_stride, const float* x, long x_clip_stride, long x_frame_stride, const int32_t* lens, int B,
                             int L, int Wy, int Wx, const int32_t* windows, int n_win, double* fd, double* moments, void* workspace,
                             size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(y_true && y_pred && x && lens && windows && fd && moments && workspace, DIMX_ERR_ARG, "listener_metrics: null operand");
    DIMX_REQUIRE(B > 0 && L > 0, DIMX_ERR_ARG, "listener_metrics: B=%d L=%d must be positive", B, L);
    DIMX_REQUIRE(n_win >= 1 && n_win <= kLmMaxWin, DIMX_ERR_ARG, "listener_metrics: n_win=%d outside 1..%d", n_win, kLmMaxWin);
    DIMX_REQUIRE(Wy >= kLmCols && Wx >= kLmCols, DIMX_ERR_ARG, "listener_metrics: rows of %d and %d columns, at least %d needed", Wy, Wx,
                 kLmCols);
    DIMX_REQUIRE(yt_clip_stride >= 0 && yt_frame_stride >= 0 && yp_clip_stride >= 0 && yp_frame_stride >= 0 && x_clip_stride >= 0 &&
                     x_frame_stride >= 0,
                 DIMX_ERR_ARG, "listener_metrics: negative stride");
    LmArgs a;
    int Fmax = 0;
    for (int w = 0; w < n_win; ++w) {
        const int xc0 = windows[4 * w], xF = windows[4 * w + 1], yc0 = windows[4 * w + 2], yF = windows[4 * w + 3];
        DIMX_REQUIRE(xc0 >= 0 && xF >= 0 && yc0 >= 0 && yF >= 0 && xF <= kLmMaxF && yF <= kLmMaxF, DIMX_ERR_ARG,
                     "listener_metrics: window %d = (%d, %d, %d, %d)", w, xc0, xF, yc0, yF);
        const int F = xF + yF;
        DIMX_REQUIRE(F >= 1 && F <= kLmMaxF, DIMX_ERR_ARG, "listener_metrics: window %d has F=%d outside 1..%d", w, F, kLmMaxF);
        DIMX_REQUIRE(xc0 <= Wx - xF && yc0 <= Wy - yF, DIMX_ERR_ARG,
                     "listener_metrics: window %d, columns [%d, %d) of x and [%d, %d) of y leave the rows of %d and %d", w, xc0, xc0 + xF,
                     yc0, yc0 + yF, Wx, Wy);
        a.win[w][0] = xc0, a.win[w][1] = xF, a.win[w][2] = yc0, a.win[w][3] = yF;
        Fmax = F > Fmax ? F : Fmax;
    }
    DIMX_REQUIRE(((uintptr_t)workspace & 7) == 0, DIMX_ERR_ARG, "listener_metrics: workspace not 8-byte aligned");
    const size_t need = dimx_op_listener_metrics_ws_bytes(B, n_win, Fmax);
    DIMX_REQUIRE(workspace_bytes >= need, DIMX_ERR_ARG, "listener_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    DIMX_REQUIRE((long long)B * n_win <= 0x7fffffffLL, DIMX_ERR_ARG, "listener_metrics: B=%d n_win=%d exceed the grid", B, n_win);
    // the widest windows first (insertion sort, stable): the blocks that run longest start first
    for (int w = 0; w < n_win; ++w) {
        int k = w;
        const int Fw = a.win[w][1] + a.win[w][3];
        while (k > 0 && a.win[a.order[k - 1]][1] + a.win[a.order[k - 1]][3] < Fw) {
            a.order[k] = a.order[k - 1];
            --k;
        }
        a.order[k] = w;
    }
    for (int w = n_win; w < kLmMaxWin; ++w) {
        a.order[w] = 0;
        a.win[w][0] = a.win[w][1] = a.win[w][2] = a.win[w][3] = 0;
    }
    a.yt = y_true, a.yt_cs = yt_clip_stride, a.yt_fs = yt_frame_stride;
    a.yp = y_pred, a.yp_cs = yp_clip_stride, a.yp_fs = yp_frame_stride;
    a.x = x, a.x_cs = x_clip_stride, a.x_fs = x_frame_stride;
    a.lens = lens, a.B = B, a.L = L, a.n_win = n_win;
    a.fd = fd, a.mom = moments;
    a.wsA = (double*)workspace;
    a.a_stride = (size_t)Fmax * Fmax;
    a.wsSweeps = (int32_t*)(a.wsA + (size_t)B * n_win * a.a_stride);
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = ((size_t)kLmTile * kLmTileLd + (size_t)Fmax * lm_ld(Fmax)) * sizeof(double);
    // the attribute belongs to (function, device): always the size of the widest window the kernel takes, never this call's own, so
    // that calls from several host threads cannot lower it under one another; the call is cheap
    const size_t lds_max = ((size_t)kLmTile * kLmTileLd + (size_t)kLmMaxF * lm_ld(kLmMaxF)) * sizeof(double);
    DIMX_HIP(hipFuncSetAttribute((const void*)lm_fd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    hipLaunchKernelGGL(lm_moments_kernel, dim3(B), dim3(kLmMomThreads), 0, s, a);
    DIMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_fd_kernel, dim3(B * n_win), dim3(kLmThreads), lds, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
