// fd_select.hip -- best-of-S selection by Frechet distance (the test-time protocol's selection step).
//
// Reference: evaluate_test_epoch, code/x_engine_pt.py:255-270 (per clip keep the try with the smallest distance, strict '<' in try
// order) around the Frechet distance of frechet.hpp, which holds the arithmetic and its derivation; this file holds what is
// specific to the selection.  Three launches, no atomics, no host synchronisation:
//   fd_clip_kernel  (one block per clip): mu1, tr S1 and the factor A of the target (S1 = A A^T) go to the workspace.
//   fd_try_kernel   (one block per (clip, try)): mu2, S2, M = A^T S2 A with A read back from the workspace, and the scalar fd.
//   fd_pick_kernel  (one block per clip): first minimum of the row (NaN counts as +inf), ok flag, gather of the winner.
#include "frechet.hpp"
#include "pick_gather.hpp"

namespace dimx {
namespace {

using FdT = frechet::Traits<256, 64>;
constexpr int kFdThreads = FdT::THREADS;
constexpr int kMaxF = FdT::MAXF;

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

// the window columns of one clip (or try): rows are fs elements apart
struct FdRows {
    const float* x;
    long fs;
    __device__ __forceinline__ double at(int t, int c) const { return (double)x[(size_t)t * fs + c]; }
};

__global__ __launch_bounds__(kFdThreads) void fd_clip_kernel(FdArgs a) {
    extern __shared__ double fd_dyn[];
    __shared__ frechet::Smem<FdT> sm;
    const int j = blockIdx.x, F = a.F, ld = FdT::ld(F);
    const int n = frechet::valid_frames(a.lens, a.L, j);
    if (n < 2) {   // no covariance: every distance of the clip is NaN (fd_try_kernel), nothing of the workspace is read
        if (threadIdx.x == 0) a.wsSweeps[j] = 0;
        return;
    }
    double* tile = fd_dyn;                              // kTile x kTileLd
    double* G = fd_dyn + frechet::kTile * FdT::kTileLd; // F x ld: S1
    const frechet::TileIdx<FdT> ix(F);
    const FdRows rw{a.yt + (size_t)j * a.yt_cs + a.c0, a.yt_fs};
    frechet::mean<FdT>(rw, n, F, sm);
    frechet::cov<FdT>(rw, n, F, sm, ix, tile, G, ld);
    frechet::trace<FdT>(G, F, ld, sm, 0);
    const int sweeps = frechet::eigen<FdT>(G, F, ld, min(F, n - 1), sm);
    frechet::write_factor<FdT>(G, F, ld, sm, a.wsA + (size_t)j * F * F);
    if (threadIdx.x < F) a.wsMu[(size_t)j * F + threadIdx.x] = sm.mu[threadIdx.x];
    if (threadIdx.x == 0) {
        a.wsTr[j] = sm.scal[0];
        a.wsSweeps[j] = sweeps;
    }
}

__global__ __launch_bounds__(kFdThreads) void fd_try_kernel(FdArgs a) {
    extern __shared__ double fd_dyn[];
    __shared__ frechet::Smem<FdT> sm;
    const int j = blockIdx.x / a.S, s = blockIdx.x - j * a.S, F = a.F, ld = FdT::ld(F);
    const int n = frechet::valid_frames(a.lens, a.L, j);
    if (n < 2) {
        if (threadIdx.x == 0) {
            a.fd[blockIdx.x] = __builtin_nan("");
            a.wsSweeps[a.B + blockIdx.x] = 0;
        }
        return;
    }
    double* tile = fd_dyn;                              // kTile x kTileLd
    double* G = fd_dyn + frechet::kTile * FdT::kTileLd; // F x ld: S2, then T, M
    const double* A = a.wsA + (size_t)j * F * F;
    const frechet::TileIdx<FdT> ix(F);
    const FdRows rw{a.yp + (size_t)j * a.yp_cs + (size_t)s * a.yp_ss + a.c0, a.yp_fs};
    if (threadIdx.x < F) sm.mu1[threadIdx.x] = a.wsMu[(size_t)j * F + threadIdx.x];
    frechet::mean<FdT>(rw, n, F, sm);
    frechet::cov<FdT>(rw, n, F, sm, ix, tile, G, ld);
    frechet::trace<FdT>(G, F, ld, sm, 1);
    frechet::mean_diff2<FdT>(F, sm);
    frechet::product<FdT>(A, F, ix, tile, G, ld, false);
    frechet::product<FdT>(A, F, ix, tile, G, ld, true);
    const int sweeps = frechet::eigen<FdT>(G, F, ld, min(F, n - 1), sm);
    if (threadIdx.x == 0) {
        a.fd[blockIdx.x] = frechet::distance<FdT>(F, sm, a.wsTr[j]);
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
    const int n = sh_ok ? frechet::valid_frames(a.lens, a.L, j) : 0;
    const float* src = a.yp + (size_t)j * a.yp_cs + (size_t)sh_win * a.yp_ss;
    gather_winner_rows<kFdThreads>(src, a.yp_fs, a.best + (size_t)j * a.L * a.W, a.L, a.W, n);
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
    const size_t lds = FdT::lds_bytes(F);
    const int lds_max = (int)FdT::lds_bytes(kMaxF);   // never this call's own size: frechet.hpp, Traits::lds_bytes
    DIMX_HIP(hipFuncSetAttribute((const void*)fd_clip_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    DIMX_HIP(hipFuncSetAttribute((const void*)fd_try_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    hipLaunchKernelGGL(fd_clip_kernel, dim3(B), dim3(kFdThreads), lds, s, a);
    hipLaunchKernelGGL(fd_try_kernel, dim3(B * S), dim3(kFdThreads), lds, s, a);
    hipLaunchKernelGGL(fd_pick_kernel, dim3(B), dim3(kFdThreads), 0, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
