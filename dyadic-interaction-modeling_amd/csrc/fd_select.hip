// fd_select.hip -- best-of-S selection by Frechet distance (the test-time protocol's selection step).
//
// Reference: evaluate_test_epoch, code/x_engine_pt.py:255-270 (per clip keep the try with the smallest distance, strict '<' in try
// order) around calculate_activation_statistics / calculate_frechet_distance, code/metrics/eval_utils.py:6-46:
//     mu, S  = mean and unbiased covariance over the valid frames,   fd = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)
// Everything below is float64.  tr sqrt(S1 S2) = sum_i sqrt(lambda_i(M)), M = A^T S2 A with S1 = A A^T: a symmetric positive
// semi-definite matrix, so no non-symmetric eigenproblem is solved.
//
// Three launches, no atomics, no host synchronisation:
//   fd_clip_kernel  (one block per clip): mu1, S1, tr S1; a one-sided (Hestenes) Jacobi turns S1 into G = S1 V = V Lambda, whose
//       columns have the norms lambda_i, and A = G Lambda^-1/2 (S1 = A A^T) goes to the workspace.
//   fd_try_kernel   (one block per (clip, try)): mu2, S2, T = S2 A, M = A^T T, the same Jacobi on M (its column norms converge to
//       the eigenvalues of M), and the scalar fd.
//   fd_pick_kernel  (one block per clip): first minimum of the row (NaN counts as +inf), ok flag, gather of the winner.
// A covariance of n frames has rank <= n - 1, so at most r = min(F, n - 1) eigenvalues of S1 and of M are non-zero: only the r
// largest are kept.  On a full-rank clip that is all of them; on a clip shorter than F + 1 frames it drops what rounding leaves in
// eigenvalues that are exactly zero (1e-16 |M| each, 1e-8 after the square root, F - r of them).
// The Jacobi is the parallel cyclic one with round-robin pairing, held in LDS: F columns give m/2 disjoint pairs per step
// (m = F rounded up to even), 8 lanes per pair, m - 1 steps per sweep, one barrier per step.  Its loop is bounded (kMaxSweeps) and
// ends early when a sweep rotated nothing.  Every block's arithmetic depends on its own inputs only, in a fixed order: identical
// candidates get bit-identical distances, and so do repeated calls.
// Frames t >= lens[j] are never loaded.
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kFdThreads = 256;
constexpr int kMaxF = 64;
constexpr int kTile = 16;            // frames per LDS tile of the covariance pass
constexpr int kTileLd = kMaxF + 1;   // tile row stride (doubles)
constexpr int kMaxSweeps = 30;

__host__ __device__ inline int fd_ld(int F) { return F | 1; }   // odd column stride: the 8 lanes of a pair and the pairs of a wave spread over the banks
__host__ __device__ inline int fd_mat_doubles(int F) {
    const int m = F * fd_ld(F), t = kTile * kTileLd;
    return m > t ? m : t;
}

struct FdArgs {
    const float* yt;
    long yt_cs, yt_fs;
    const float* yp;
    long yp_cs, yp_ss, yp_fs;
    const int32_t* lens;
    int B, S, L, W, c0, F;
    double* fd;
    int32_t* win;
    uint8_t* ok;
    float* best;
    double* wsA;       // [B][F*F]  A, column-major, dense
    double* wsMu;      // [B][F]
    double* wsTr;      // [B]
    int32_t* wsSweeps; // [B + B*S]
};

struct FdSmem {
    double red[4][kMaxF];   // partial sums of fd_mean; red[0] is reused as the keep flags of fd_top_r
    double mu[kMaxF];
    double sig[kMaxF];
    double scal[4];
};

__device__ __forceinline__ int fd_valid_frames(const FdArgs& a, int j) {
    int n = a.lens[j];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

// mean over the n valid frames of the F window columns -> sm.mu; rows of x are fs elements apart
__device__ void fd_mean(const float* __restrict__ x, long fs, int n, int F, FdSmem& sm) {
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    double acc = 0.0;
    if (c < F)
        for (int t = g; t < n; t += 4) acc += (double)x[(size_t)t * fs + c];
    sm.red[g][c] = acc;
    __syncthreads();
    if (threadIdx.x < F) sm.mu[threadIdx.x] = (((sm.red[0][c] + sm.red[1][c]) + sm.red[2][c]) + sm.red[3][c]) / (double)n;
    __syncthreads();
}

// unbiased covariance of the centred frames -> out (column-major, stride ld); tile is kTile x kTileLd doubles and may not alias out
__device__ void fd_cov(const float* __restrict__ x, long fs, int n, int F, const FdSmem& sm, double* tile, double* out, int ld) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int t0 = 0; t0 < n; t0 += kTile) {
        for (int e = threadIdx.x; e < kTile * kMaxF; e += kFdThreads) {
            const int tt = e >> 6, c = e & 63;
            double v = 0.0;
            if (c < F && t0 + tt < n) v = (double)x[(size_t)(t0 + tt) * fs + c] - sm.mu[c];
            tile[tt * kTileLd + c] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < kTile; ++tt) {
            double xi[4], xj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                xi[a] = tile[tt * kTileLd + ti + 16 * a];
                xj[a] = tile[tt * kTileLd + tj + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(xi[a], xj[b], acc[a][b]);
        }
        __syncthreads();
    }
    const double inv = 1.0 / (double)(n - 1);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = ti + 16 * a, j = tj + 16 * b;
            if (i < F && j < F) out[j * ld + i] = acc[a][b] * inv;
        }
    __syncthreads();
}

// trace of the F x F matrix m (stride ld), summed in index order -> sm.scal[slot]
__device__ void fd_trace(const double* m, int F, int ld, FdSmem& sm, int slot) {
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < F; ++i) t += m[i * ld + i];
        sm.scal[slot] = t;
    }
    __syncthreads();
}

// squared column norms of g -> sm.sig (thread c owns column c)
__device__ void fd_col_norms2(const double* g, int F, int ld, FdSmem& sm) {
    if (threadIdx.x < F) {
        double s = 0.0;
        for (int r = 0; r < F; ++r) s = fma(g[threadIdx.x * ld + r], g[threadIdx.x * ld + r], s);
        sm.sig[threadIdx.x] = s;
    }
    __syncthreads();
}

// One-sided cyclic Jacobi on the columns of g (F x F, column-major, stride ld): on return the columns are mutually orthogonal
// (g <- g V), so for a symmetric positive semi-definite input their norms are its eigenvalues.  Returns the sweeps done.
__device__ int fd_jacobi(double* g, int F, int ld, FdSmem& sm) {
    fd_col_norms2(g, F, ld, sm);
    double fro2 = 0.0;
    for (int c = 0; c < F; ++c) fro2 += sm.sig[c];
    // columns whose product is below this are orthogonal as far as the result can tell: (1e-14 |g|)^2
    const double tiny = 1e-28 * fro2;
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
            double gp[8], gq[8];
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
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
            if (live && aga > tiny && aga * aga > 1e-26 * al * be) {   // |cos| of the angle above 1e-13: moves a norm by 1e-26 relative, 1e-13 when degenerate
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
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

// sm.sig holds F non-negative values; sm.red[0][c] = 1 when sig[c] is among the r largest (ties: the lower index first)
__device__ void fd_top_r(int F, int r, FdSmem& sm) {
    if (threadIdx.x < F) {
        const int c = threadIdx.x;
        const double v = sm.sig[c];
        int rank = 0;
        for (int d = 0; d < F; ++d) rank += (sm.sig[d] > v || (sm.sig[d] == v && d < c)) ? 1 : 0;
        sm.red[0][c] = rank < r ? 1.0 : 0.0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kFdThreads) void fd_clip_kernel(FdArgs a) {
    extern __shared__ double fd_dyn[];
    __shared__ FdSmem sm;
    const int j = blockIdx.x, F = a.F, ld = fd_ld(F);
    const int n = fd_valid_frames(a, j);
    double* bufA = fd_dyn;
    double* bufB = fd_dyn + fd_mat_doubles(F);
    if (n < 2) {   // no covariance: every distance of the clip is NaN (fd_try_kernel), nothing of the workspace is read
        if (threadIdx.x == 0) a.wsSweeps[j] = 0;
        return;
    }
    const float* x = a.yt + (size_t)j * a.yt_cs + a.c0;
    fd_mean(x, a.yt_fs, n, F, sm);
    fd_cov(x, a.yt_fs, n, F, sm, bufB, bufA, ld);
    fd_trace(bufA, F, ld, sm, 0);
    const int sweeps = fd_jacobi(bufA, F, ld, sm);
    fd_col_norms2(bufA, F, ld, sm);
    if (threadIdx.x < F) sm.sig[threadIdx.x] = sqrt(sm.sig[threadIdx.x]);   // lambda_i
    __syncthreads();
    fd_top_r(F, min(F, n - 1), sm);
    for (int e = threadIdx.x; e < F * F; e += kFdThreads) {
        const int c = e / F, r = e - c * F;
        const double lam = sm.sig[c];
        a.wsA[(size_t)j * F * F + e] = (sm.red[0][c] != 0.0 && lam > 0.0) ? bufA[c * ld + r] / sqrt(lam) : 0.0;
    }
    if (threadIdx.x < F) a.wsMu[(size_t)j * F + threadIdx.x] = sm.mu[threadIdx.x];
    if (threadIdx.x == 0) {
        a.wsTr[j] = sm.scal[0];
        a.wsSweeps[j] = sweeps;
    }
}

__global__ __launch_bounds__(kFdThreads) void fd_try_kernel(FdArgs a) {
    extern __shared__ double fd_dyn[];
    __shared__ FdSmem sm;
    const int j = blockIdx.x / a.S, s = blockIdx.x - j * a.S, F = a.F, ld = fd_ld(F);
    const int n = fd_valid_frames(a, j);
    double* bufA = fd_dyn;
    double* bufB = fd_dyn + fd_mat_doubles(F);
    if (n < 2) {
        if (threadIdx.x == 0) {
            a.fd[blockIdx.x] = __builtin_nan("");
            a.wsSweeps[a.B + blockIdx.x] = 0;
        }
        return;
    }
    const float* x = a.yp + (size_t)j * a.yp_cs + (size_t)s * a.yp_ss + a.c0;
    fd_mean(x, a.yp_fs, n, F, sm);
    fd_cov(x, a.yp_fs, n, F, sm, bufA, bufB, ld);   // S2 -> bufB
    fd_trace(bufB, F, ld, sm, 1);
    for (int e = threadIdx.x; e < F * F; e += kFdThreads) {
        const int c = e / F, r = e - c * F;
        bufA[c * ld + r] = a.wsA[(size_t)j * F * F + e];
    }
    if (threadIdx.x == 0) {   // |mu1 - mu2|^2 in column order
        double d2 = 0.0;
        for (int c = 0; c < F; ++c) {
            const double d = a.wsMu[(size_t)j * F + c] - sm.mu[c];
            d2 = fma(d, d, d2);
        }
        sm.scal[2] = d2;
    }
    __syncthreads();
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    int ri[4], cj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ri[k] = min(ti + 16 * k, F - 1);
        cj[k] = min(tj + 16 * k, F - 1);
    }
    double acc[4][4];
    // T = S2 A
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int k = 0; k < F; ++k) {
        double u[4], v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            u[p] = bufB[k * ld + ri[p]];
            v[p] = bufA[cj[p] * ld + k];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ti + 16 * p < F && tj + 16 * q < F) bufB[cj[q] * ld + ri[p]] = acc[p][q];
    __syncthreads();
    // M = A^T T
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int k = 0; k < F; ++k) {
        double u[4], v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            u[p] = bufA[ri[p] * ld + k];
            v[p] = bufB[cj[p] * ld + k];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ti + 16 * p < F && tj + 16 * q < F) bufA[cj[q] * ld + ri[p]] = acc[p][q];
    __syncthreads();
    const int sweeps = fd_jacobi(bufA, F, ld, sm);
    fd_col_norms2(bufA, F, ld, sm);
    if (threadIdx.x < F) sm.sig[threadIdx.x] = sqrt(sm.sig[threadIdx.x]);   // eigenvalues of M
    __syncthreads();
    fd_top_r(F, min(F, n - 1), sm);
    if (threadIdx.x == 0) {
        double trs = 0.0;
        for (int c = 0; c < F; ++c) trs += sm.red[0][c] != 0.0 ? sqrt(sm.sig[c]) : 0.0;
        a.fd[blockIdx.x] = sm.scal[2] + a.wsTr[j] + sm.scal[1] - 2.0 * trs;
        a.wsSweeps[a.B + blockIdx.x] = sweeps;
    }
}

__global__ __launch_bounds__(kFdThreads) void fd_pick_kernel(FdArgs a) {
    __shared__ int sh_win, sh_ok;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) {
        const double inf = __builtin_inf();
        double cur = inf;
        int w = 0;
        for (int s = 0; s < a.S; ++s) {
            double d = a.fd[(size_t)j * a.S + s];
            if (d != d) d = inf;
            if (d < cur) {
                cur = d;
                w = s;
            }
        }
        const int okv = (cur < inf && cur > -inf) ? 1 : 0;
        a.win[j] = w;
        a.ok[j] = (uint8_t)okv;
        sh_win = w;
        sh_ok = okv;
    }
    __syncthreads();
    if (!a.best) return;
    const int n = sh_ok ? fd_valid_frames(a, j) : 0;
    const float* src = a.yp + (size_t)j * a.yp_cs + (size_t)sh_win * a.yp_ss;
    float* dst = a.best + (size_t)j * a.L * a.W;
    const int total = a.L * a.W;
    for (int e = threadIdx.x; e < total; e += kFdThreads) {
        const int t = e / a.W, c = e - t * a.W;
        dst[e] = t < n ? src[(size_t)t * a.yp_fs + c] : 0.f;
    }
}

size_t fd_ws_doubles(int B, int F) { return (size_t)B * ((size_t)F * F + F + 1); }

}  // namespace
}  // namespace dimx

using namespace dimx;

size_t dimx_op_fd_select_ws_bytes(int B, int S, int F) {
    if (B <= 0 || S <= 0 || F < 1 || F > kMaxF) return 0;
    return fd_ws_doubles(B, F) * sizeof(double) + ((size_t)B + (size_t)B * S) * sizeof(int32_t);
}

int dimx_op_fd_select(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                      long yp_sample_stride, long yp_frame_stride, const int32_t* lens, int B, int S, int L, int W, int c0, int F,
                      double* fd, int32_t* win, uint8_t* ok, float* best, void* workspace, size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(y_true && y_pred && lens && fd && win && ok && workspace, DIMX_ERR_ARG, "fd_select: null operand");
    DIMX_REQUIRE(B > 0 && S > 0 && L > 0 && W > 0, DIMX_ERR_ARG, "fd_select: B=%d S=%d L=%d W=%d must be positive", B, S, L, W);
    DIMX_REQUIRE(F >= 1 && F <= kMaxF, DIMX_ERR_ARG, "fd_select: F=%d outside 1..%d", F, kMaxF);
    DIMX_REQUIRE(c0 >= 0 && c0 <= W - F, DIMX_ERR_ARG, "fd_select: columns [%d, %d) leave the row of %d", c0, c0 + F, W);
    DIMX_REQUIRE(yt_clip_stride >= 0 && yt_frame_stride >= 0 && yp_clip_stride >= 0 && yp_sample_stride >= 0 && yp_frame_stride >= 0,
                 DIMX_ERR_ARG, "fd_select: negative stride");
    DIMX_REQUIRE(((uintptr_t)workspace & 7) == 0, DIMX_ERR_ARG, "fd_select: workspace not 8-byte aligned");
    DIMX_REQUIRE(workspace_bytes >= dimx_op_fd_select_ws_bytes(B, S, F), DIMX_ERR_ARG, "fd_select: workspace of %zu bytes, %zu needed",
                 workspace_bytes, dimx_op_fd_select_ws_bytes(B, S, F));
    FdArgs a;
    a.yt = y_true, a.yt_cs = yt_clip_stride, a.yt_fs = yt_frame_stride;
    a.yp = y_pred, a.yp_cs = yp_clip_stride, a.yp_ss = yp_sample_stride, a.yp_fs = yp_frame_stride;
    a.lens = lens, a.B = B, a.S = S, a.L = L, a.W = W, a.c0 = c0, a.F = F;
    a.fd = fd, a.win = win, a.ok = ok, a.best = best;
    a.wsA = (double*)workspace;
    a.wsMu = a.wsA + (size_t)B * F * F;
    a.wsTr = a.wsMu + (size_t)B * F;
    a.wsSweeps = (int32_t*)(a.wsTr + B);
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = 2 * (size_t)fd_mat_doubles(F) * sizeof(double);
    // per launch: the attribute belongs to (function, device) and the call is cheap
    DIMX_HIP(hipFuncSetAttribute((const void*)fd_clip_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DIMX_HIP(hipFuncSetAttribute((const void*)fd_try_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fd_clip_kernel, dim3(B), dim3(kFdThreads), lds, s, a);
    hipLaunchKernelGGL(fd_try_kernel, dim3(B * S), dim3(kFdThreads), lds, s, a);
    hipLaunchKernelGGL(fd_pick_kernel, dim3(B), dim3(kFdThreads), 0, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
