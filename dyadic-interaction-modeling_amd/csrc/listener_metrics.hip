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
//   lm_fd_kernel (one block of 512 per (window, clip), the widest windows first): the Frechet distance of frechet.hpp with F up
//       to 112, both sides in one block.  The factor A of the target side goes to the workspace and comes back, panel by panel,
//       through L2 (the block wrote it itself: a workgroup-scope fence and the barrier order the write before the reads): two
//       112 x 113 float64 matrices (101 248 B each) do not fit the 160 KiB of a CU.
// Every sum has a fixed order that depends on the shapes only: two calls on the same inputs are bit-identical.
// Frames t >= lens[b] are never loaded.  All address arithmetic is 64-bit.
#include "frechet.hpp"

namespace dimx {
namespace {

using LmT = frechet::Traits<512, 112>;
constexpr int kLmThreads = LmT::THREADS;
constexpr int kLmMomThreads = 256;
constexpr int kLmMaxF = LmT::MAXF;
constexpr int kLmMaxWin = 8;
constexpr int kLmCols = 56, kLmPose = 6;
constexpr int kLmGroup = 10;              // moments per group, include/dimx.h
constexpr int kLmEdge = 1 + 2 * kLmGroup; // first column of the edge block
static_assert(kLmEdge + 2 * kLmCols == DIMX_LM_ROW, "moment row layout");

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

// ------------------------------------------------------------------------------------------------ moments
__global__ __launch_bounds__(kLmMomThreads) void lm_moments_kernel(LmArgs a) {
    __shared__ double part[7][kLmMomThreads];
    __shared__ double mean[2][3];
    const int b = blockIdx.x, n = frechet::valid_frames(a.lens, a.L, b);
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

__global__ __launch_bounds__(kLmThreads) void lm_fd_kernel(LmArgs a) {
    extern __shared__ double lm_dyn[];
    __shared__ frechet::Smem<LmT> sm;
    const int pos = blockIdx.x / a.B, b = blockIdx.x - pos * a.B, w = a.order[pos];
    const int xc0 = a.win[w][0], xF = a.win[w][1], yc0 = a.win[w][2], F = xF + a.win[w][3], ld = LmT::ld(F);
    const int n = frechet::valid_frames(a.lens, a.L, b);
    const size_t slot = (size_t)w * a.B + b;
    if (n < 2) {   // no covariance: nothing of the inputs or of the workspace is read
        if (threadIdx.x == 0) {
            a.fd[(size_t)b * a.n_win + w] = __builtin_nan("");
            a.wsSweeps[slot] = 0;
            a.wsSweeps[(size_t)a.n_win * a.B + slot] = 0;
        }
        return;
    }
    double* tile = lm_dyn;                                  // kTile x kTileLd
    double* G = lm_dyn + frechet::kTile * LmT::kTileLd;     // F x ld: S1, then S2, T, M
    double* A = a.wsA + slot * a.a_stride;
    const frechet::TileIdx<LmT> ix(F);
    const int r = min(F, n - 1);
    LmRows rw;
    rw.x = a.x + (size_t)b * a.x_cs + xc0, rw.x_fs = a.x_fs, rw.xF = xF;
    // target side: mu1, tr S1, A
    rw.y = a.yt + (size_t)b * a.yt_cs + yc0, rw.y_fs = a.yt_fs;
    frechet::mean<LmT>(rw, n, F, sm);
    frechet::cov<LmT>(rw, n, F, sm, ix, tile, G, ld);
    frechet::trace<LmT>(G, F, ld, sm, 0);
    if (threadIdx.x < F) sm.mu1[threadIdx.x] = sm.mu[threadIdx.x];
    const int sweeps1 = frechet::eigen<LmT>(G, F, ld, r, sm);
    frechet::write_factor<LmT>(G, F, ld, sm, A);
    __threadfence_block();   // A is read back by this block only
    __syncthreads();
    // candidate side: mu2, S2, T = S2 A, M = A^T T
    rw.y = a.yp + (size_t)b * a.yp_cs + yc0, rw.y_fs = a.yp_fs;
    frechet::mean<LmT>(rw, n, F, sm);
    frechet::cov<LmT>(rw, n, F, sm, ix, tile, G, ld);
    frechet::trace<LmT>(G, F, ld, sm, 1);
    frechet::mean_diff2<LmT>(F, sm);
    frechet::product<LmT>(A, F, ix, tile, G, ld, false);
    frechet::product<LmT>(A, F, ix, tile, G, ld, true);
    const int sweeps2 = frechet::eigen<LmT>(G, F, ld, r, sm);
    if (threadIdx.x == 0) {
        a.fd[(size_t)b * a.n_win + w] = frechet::distance<LmT>(F, sm, sm.scal[0]);
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
    const size_t lds = LmT::lds_bytes(Fmax);
    // never this call's own size: frechet.hpp, Traits::lds_bytes
    DIMX_HIP(hipFuncSetAttribute((const void*)lm_fd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LmT::lds_bytes(kLmMaxF)));
    hipLaunchKernelGGL(lm_moments_kernel, dim3(B), dim3(kLmMomThreads), 0, s, a);
    DIMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_fd_kernel, dim3(B * n_win), dim3(kLmThreads), lds, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
