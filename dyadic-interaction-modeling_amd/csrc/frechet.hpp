// frechet.hpp -- the float64 Frechet distance of one clip, shared by fd_select.hip, listener_metrics.hip and consensus.hip.
//
// Reference: calculate_activation_statistics / calculate_frechet_distance, code/metrics/eval_utils.py:6-46:
//     mu, S  = mean and unbiased covariance over the valid frames,   fd = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)
// tr sqrt(S1 S2) = sum_i sqrt(lambda_i(M)), M = A^T S2 A with S1 = A A^T: a symmetric positive semi-definite matrix, so no
// non-symmetric eigenproblem is solved.  One block does, for one clip:
//     S1 -> one-sided (Hestenes) Jacobi -> G = S1 V = V Lambda, whose columns have the norms lambda_i -> A = G Lambda^-1/2;
//     S2;  T = S2 A;  M = A^T T;  the same Jacobi on M (its column norms converge to the eigenvalues of M);  the scalar fd.
// A covariance of n frames has rank <= n - 1, so at most r = min(F, n - 1) eigenvalues of S1 and of M are non-zero: only the r
// largest are kept.  On a full-rank clip that is all of them; on a clip shorter than F + 1 frames it drops what rounding leaves in
// eigenvalues that are exactly zero (1e-16 |M| each, 1e-8 after the square root, F - r of them).
// The Jacobi is the parallel cyclic one with round-robin pairing, held in LDS: F columns give m/2 disjoint pairs per step
// (m = F rounded up to even), 8 lanes per pair, m - 1 steps per sweep, one barrier per step; a lane holds NK = F/8 rounded up rows
// of its two columns.  Its loop is bounded (kMaxSweeps) and ends early when a sweep rotated nothing.
// LDS: one F x F matrix (column-major, odd stride F | 1) in which S1, S2, T and M take turns, plus a 16-row panel that is the frame
// tile of the covariance pass and the k-panel of A in the two products.  A is the only second operand and is read from global
// memory, panel by panel.
// Every sum has a fixed order that depends on the shapes only, and a block's arithmetic depends on its own inputs only: identical
// candidates get bit-identical distances, and so do repeated calls.  Frames t >= lens[j] are never loaded.
//
// Everything is a template over Traits<THREADS, MAXF>: the block size and the widest window of the operator that instantiates it.
#pragma once
#include "common.hpp"

namespace dimx {
namespace frechet {

constexpr int kTile = 16;        // rows of the panel: frames of the covariance pass, k of the products
constexpr int kMaxSweeps = 30;
// columns whose product is below kTinyRel |g|_F^2 are orthogonal as far as the result can tell: (1e-14 |g|)^2
constexpr double kTinyRel = 1e-28;
// |cos| of the angle above 1e-13: a rotation below it moves a norm by 1e-26 relative, 1e-13 when degenerate
constexpr double kCos2Min = 1e-26;

template <int THREADS_, int MAXF_>
struct Traits {
    static constexpr int THREADS = THREADS_, MAXF = MAXF_;
    static constexpr int CG = THREADS / 4;                   // lanes per frame group of the mean; columns of a staged frame
    static constexpr int TJ = THREADS / 16;                  // the thread grid of the covariance and the products is 16 x TJ
    static constexpr int RP = (MAXF + 15) / 16;              // register tile: rows ti + 16 p, p < RP
    static constexpr int CQ = (MAXF + TJ - 1) / TJ;          //                columns tj + TJ q, q < CQ
    static constexpr int kTileLd = MAXF + 1;                 // panel row stride (doubles)
    static constexpr int kCovUnroll = 16 / RP;               // frames of a tile in flight: 4 with 4 rows per thread, 2 with 7
    static constexpr int NKMAX = (MAXF + 7) / 8;             // rows per lane of the widest Jacobi
    static_assert(THREADS % 64 == 0 && MAXF <= CG && 8 * ((MAXF + 1) / 2) <= THREADS, "a lane per column, 8 lanes per column pair");
    // odd column stride: the 8 lanes of a pair and the pairs of a wave spread over the banks
    __host__ __device__ static int ld(int F) { return F | 1; }
    // dynamic LDS of a block: the panel, then the matrix.  The launch passes lds_bytes(F of the call).
    // hipFuncAttributeMaxDynamicSharedMemorySize is always set to lds_bytes(MAXF), never to the call's own size: the attribute
    // belongs to (function, device), so calls from several host threads with different F would lower it under one another; the
    // call is cheap.
    __host__ __device__ static size_t lds_bytes(int F) { return ((size_t)kTile * kTileLd + (size_t)F * ld(F)) * sizeof(double); }
};

template <class T>
struct Smem {
    double red[4][T::CG];   // partial sums of mean; red[0] is reused as the keep flags of top_r
    double mu[T::MAXF];
    double mu1[T::MAXF];    // the target side's mean while mu holds the candidate's
    double sig[T::MAXF];
    double scal[4];         // tr S1, tr S2, |mu1 - mu2|^2
};

__device__ __forceinline__ int valid_frames(const int32_t* lens, int L, int j) {
    const int n = lens[j];
    return n < 0 ? 0 : (n > L ? L : n);
}

// Rows: the operand rows of one clip, an object with double at(int t, int c) const.
// mean over the n valid frames of the F operand columns -> sm.mu
template <class T, class Rows>
__device__ void mean(const Rows& rw, int n, int F, Smem<T>& sm) {
    const int c = threadIdx.x % T::CG, g = threadIdx.x / T::CG;
    double acc = 0.0;
    if (c < F)
        for (int t = g; t < n; t += 4) acc += rw.at(t, c);
    sm.red[g][c] = acc;
    __syncthreads();
    if (threadIdx.x < F) sm.mu[c] = (((sm.red[0][c] + sm.red[1][c]) + sm.red[2][c]) + sm.red[3][c]) / (double)n;
    __syncthreads();
}

// the 16 x TJ thread grid of the covariance and of the products: rows ti + 16 p (p < RP), columns tj + TJ q (q < CQ), clamped to F - 1
template <class T>
struct TileIdx {
    int ti, tj, ri[T::RP], cj[T::CQ], np, nq;
    __device__ explicit TileIdx(int F) {
        ti = threadIdx.x / T::TJ, tj = threadIdx.x % T::TJ;
        np = (F + 15) / 16, nq = (F + T::TJ - 1) / T::TJ;   // register tiles that hold a column of the window at all (block-uniform)
#pragma unroll
        for (int p = 0; p < T::RP; ++p) ri[p] = min(ti + 16 * p, F - 1);
#pragma unroll
        for (int q = 0; q < T::CQ; ++q) cj[q] = min(tj + T::TJ * q, F - 1);
    }
};

template <class T>
__device__ __forceinline__ void acc_zero(double (&acc)[T::RP][T::CQ]) {
#pragma unroll
    for (int p = 0; p < T::RP; ++p)
#pragma unroll
        for (int q = 0; q < T::CQ; ++q) acc[p][q] = 0.0;
}

template <class T>
__device__ __forceinline__ void acc_fma(const TileIdx<T>& ix, const double (&u)[T::RP], const double (&v)[T::CQ],
                                        double (&acc)[T::RP][T::CQ]) {
#pragma unroll
    for (int p = 0; p < T::RP; ++p)
        if (p < ix.np)
#pragma unroll
            for (int q = 0; q < T::CQ; ++q)
                if (q < ix.nq) acc[p][q] = fma(u[p], v[q], acc[p][q]);
}

// acc -> out[j * ld + i] * scale for the entries of the window; the caller has synchronised the readers of out
template <class T>
__device__ __forceinline__ void acc_store(const TileIdx<T>& ix, int F, const double (&acc)[T::RP][T::CQ], double scale, double* out,
                                          int ld) {
#pragma unroll
    for (int p = 0; p < T::RP; ++p)
#pragma unroll
        for (int q = 0; q < T::CQ; ++q)
            if (ix.ti + 16 * p < F && ix.tj + T::TJ * q < F) out[ix.cj[q] * ld + ix.ri[p]] = acc[p][q] * scale;
    __syncthreads();
}

// unbiased covariance of the centred frames -> out (column-major, stride ld); tile is the panel and does not alias out
template <class T, class Rows>
__device__ void cov(const Rows& rw, int n, int F, const Smem<T>& sm, const TileIdx<T>& ix, double* tile, double* out, int ld) {
    double acc[T::RP][T::CQ];
    acc_zero<T>(acc);
    for (int t0 = 0; t0 < n; t0 += kTile) {
        for (int e = threadIdx.x; e < kTile * T::CG; e += T::THREADS) {
            const int tt = e / T::CG, c = e % T::CG;
            if (c < F) tile[tt * T::kTileLd + c] = t0 + tt < n ? rw.at(t0 + tt, c) - sm.mu[c] : 0.0;
        }
        __syncthreads();
#pragma unroll T::kCovUnroll
        for (int tt = 0; tt < kTile; ++tt) {
            double u[T::RP], v[T::CQ];
#pragma unroll
            for (int p = 0; p < T::RP; ++p) u[p] = tile[tt * T::kTileLd + ix.ri[p]];
#pragma unroll
            for (int q = 0; q < T::CQ; ++q) v[q] = tile[tt * T::kTileLd + ix.cj[q]];
            acc_fma<T>(ix, u, v, acc);
        }
        __syncthreads();
    }
    acc_store<T>(ix, F, acc, 1.0 / (double)(n - 1), out, ld);
}

// rows [k0, k0 + 16) of A (global, column-major, dense stride F) -> tile[kk][j]; a column's 16 values are one 128-byte run
template <class T>
__device__ __forceinline__ void stage_a(const double* A, int F, int k0, double* tile) {
    for (int e = threadIdx.x; e < kTile * F; e += T::THREADS) {
        const int j = e >> 4, kk = e & 15;
        tile[kk * T::kTileLd + j] = k0 + kk < F ? A[(size_t)j * F + k0 + kk] : 0.0;
    }
    __syncthreads();
}

// G <- S A   (S = G on entry, symmetric: S[i][k] is read as G[k * ld + i])
// G <- A^T G (second = true)
// Each entry is one fma per k, in increasing k, from zero.
template <class T>
__device__ void product(const double* A, int F, const TileIdx<T>& ix, double* tile, double* G, int ld, bool second) {
    double acc[T::RP][T::CQ];
    acc_zero<T>(acc);
    for (int k0 = 0; k0 < F; k0 += kTile) {
        stage_a<T>(A, F, k0, tile);
        const int kn = min(kTile, F - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const int k = k0 + kk;
            double u[T::RP], v[T::CQ];
            if (!second) {
#pragma unroll
                for (int p = 0; p < T::RP; ++p) u[p] = G[k * ld + ix.ri[p]];
#pragma unroll
                for (int q = 0; q < T::CQ; ++q) v[q] = tile[kk * T::kTileLd + ix.cj[q]];
            } else {
#pragma unroll
                for (int p = 0; p < T::RP; ++p) u[p] = tile[kk * T::kTileLd + ix.ri[p]];
#pragma unroll
                for (int q = 0; q < T::CQ; ++q) v[q] = G[ix.cj[q] * ld + k];
            }
            acc_fma<T>(ix, u, v, acc);
        }
        __syncthreads();
    }
    acc_store<T>(ix, F, acc, 1.0, G, ld);
}

// trace of the F x F matrix m (stride ld), summed in index order -> sm.scal[slot]
template <class T>
__device__ void trace(const double* m, int F, int ld, Smem<T>& sm, int slot) {
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < F; ++i) t += m[i * ld + i];
        sm.scal[slot] = t;
    }
    __syncthreads();
}

// squared column norms of g -> sm.sig (thread c owns column c)
template <class T>
__device__ void col_norms2(const double* g, int F, int ld, Smem<T>& sm) {
    if (threadIdx.x < F) {
        double s = 0.0;
        for (int r = 0; r < F; ++r) s = fma(g[threadIdx.x * ld + r], g[threadIdx.x * ld + r], s);
        sm.sig[threadIdx.x] = s;
    }
    __syncthreads();
}

// One-sided cyclic Jacobi on the columns of g (F x F, column-major, stride ld), F <= 8 * NK.  On return the columns are mutually
// orthogonal (g <- g V), so for a symmetric positive semi-definite input their norms are its eigenvalues.  Returns the sweeps done.
template <class T, int NK>
__device__ int jacobi(double* g, int F, int ld, Smem<T>& sm) {
    col_norms2<T>(g, F, ld, sm);
    double fro2 = 0.0;
    for (int c = 0; c < F; ++c) fro2 += sm.sig[c];
    const double tiny = kTinyRel * fro2;
    const int m = (F + 1) & ~1, pairs = m >> 1, pi = threadIdx.x >> 3, sub = threadIdx.x & 7;
    int sweeps = 0;
    for (int sw = 0; sw < kMaxSweeps; ++sw) {
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
            for (int o = 1; o < 8; o <<= 1) {   // butterfly over the pair's 8 lanes: a + b == b + a, every lane ends with the same bits
                al += __shfl_xor(al, o);
                be += __shfl_xor(be, o);
                ga += __shfl_xor(ga, o);
            }
            const double aga = fabs(ga);
            if (live && aga > tiny && aga * aga > kCos2Min * al * be) {
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

template <class T>
__device__ int jacobi_any(double* g, int F, int ld, Smem<T>& sm) {
    if (F <= 8) return jacobi<T, 1>(g, F, ld, sm);
    if constexpr (T::MAXF > 64)
        if (F > 64) return jacobi<T, T::NKMAX>(g, F, ld, sm);
    return jacobi<T, 8>(g, F, ld, sm);
}

// sm.sig holds F non-negative values; sm.red[0][c] = 1 when sig[c] is among the r largest (ties: the lower index first)
template <class T>
__device__ void top_r(int F, int r, Smem<T>& sm) {
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
template <class T>
__device__ int eigen(double* g, int F, int ld, int r, Smem<T>& sm) {
    const int sweeps = jacobi_any<T>(g, F, ld, sm);
    col_norms2<T>(g, F, ld, sm);
    if (threadIdx.x < F) sm.sig[threadIdx.x] = sqrt(sm.sig[threadIdx.x]);
    __syncthreads();
    top_r<T>(F, r, sm);
    return sweeps;
}

// after eigen on S1 (sm.sig = lambda_i, columns of G = lambda_i v_i): A = G Lambda^-1/2 over the kept columns, zero elsewhere
// -> A (global, column-major, dense stride F).  No barrier: the caller orders the write before its readers.
template <class T>
__device__ void write_factor(const double* G, int F, int ld, const Smem<T>& sm, double* A) {
    for (int e = threadIdx.x; e < F * F; e += T::THREADS) {
        const int c = e / F, r = e - c * F;
        const double lam = sm.sig[c];
        A[e] = (sm.red[0][c] != 0.0 && lam > 0.0) ? G[c * ld + r] / sqrt(lam) : 0.0;
    }
}

// the F x F matrix m (LDS, stride ld) -> dense (global, column-major, stride F), for a later block to read back with load_dense.
// No barrier: m is only read.
template <class T>
__device__ void store_dense(const double* m, int F, int ld, double* dense) {
    for (int e = threadIdx.x; e < F * F; e += T::THREADS) {
        const int c = e / F, r = e - c * F;
        dense[e] = m[c * ld + r];
    }
}

// dense (global, column-major, stride F) -> the LDS matrix m (stride ld)
template <class T>
__device__ void load_dense(const double* dense, int F, int ld, double* m) {
    for (int e = threadIdx.x; e < F * F; e += T::THREADS) {
        const int c = e / F, r = e - c * F;
        m[c * ld + r] = dense[e];
    }
    __syncthreads();
}

// |mu1 - mu2|^2 in column order -> sm.scal[2].  No barrier: thread 0 writes it and thread 0 reads it in the epilogue.
template <class T>
__device__ void mean_diff2(int F, Smem<T>& sm) {
    if (threadIdx.x == 0) {
        double d2 = 0.0;
        for (int c = 0; c < F; ++c) {
            const double d = sm.mu1[c] - sm.mu[c];
            d2 = fma(d, d, d2);
        }
        sm.scal[2] = d2;
    }
}

// after eigen on M, one thread: the distance from |mu1 - mu2|^2, the two traces and the sum over the kept columns, in column order
template <class T>
__device__ double distance(int F, const Smem<T>& sm, double tr1) {
    double trs = 0.0;
    for (int c = 0; c < F; ++c) trs += sm.red[0][c] != 0.0 ? sqrt(sm.sig[c]) : 0.0;
    return sm.scal[2] + tr1 + sm.scal[1] - 2.0 * trs;
}

}  // namespace frechet
}  // namespace dimx
