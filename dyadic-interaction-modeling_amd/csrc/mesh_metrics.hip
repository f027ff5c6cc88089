// mesh_metrics.hip -- the DIM-Speaker mesh metrics: Lip Vertex Error (LVE) and upper-Face Dynamics Deviation (FDD).
//
// Reference: print_biwi_metrics, code/mymetrics.py:122-182.  Per clip b with n = lens[b] valid frames, a mouth map M and an upper-face
// map U (vertex indices, unsorted, duplicates count):
//     d(b,t,m)   = sum_xyz (gt[b,t,m,:] - pred[b,t,m,:])^2                       LVE = mean over all frames of max_m d
//     s_x(b,t,u) = sum_xyz (x[b,t,u,:] - templ[b,u,:])^2,  x in {gt, pred}       sigma_x(b) = mean_u std_t s_x (population, ddof = 0)
//     FDD = mean over clips of sigma_gt - sigma_pred
// The operator is the float64 value of these formulas on the f32 inputs: every difference, square and sum below is float64.
//
// Three launches, no atomics, no host synchronisation (the lens travel host -> workspace with one hipMemcpyAsync in front of them):
//   mm_frame_kernel  (one block per (clip, frame)): lanes run over the mouth map, wave max on cross-lane shuffles, then an LDS max over
//       the block's waves -> max_m d of the frame (0 for a padded frame).
//   mm_upper_kernel  (one block per (clip, chunk of kChunk frames, 256 map entries)): a lane owns one entry of the upper map, keeps its
//       kChunk values of s in registers and leaves the chunk's (mean, sum of squared deviations from that mean) for gt and pred in the
//       workspace: two passes over registers, no E[s^2] - E[s]^2 anywhere.  Splitting the frame axis is what fills the chip at B = 1
//       (T = 300, 4996 entries: 38 chunks x 20 blocks).
//   mm_clip_kernel   (one block per clip): merges each entry's chunk partials in chunk order (Chan's pairwise update), takes the
//       standard deviation, sums it over the entries and the frame maxima over the frames -- per lane in index order, then over the
//       256 lanes in lane order by one thread.
// Every sum has a fixed order that depends on the shapes only: two calls on the same inputs are bit-identical.
// A vertex is a 12-byte granule at an arbitrary 4-byte alignment (rows of 3*Nv floats are no multiple of 16 bytes): three 4-byte
// loads per vertex, nothing wider.  All address arithmetic is 64-bit.  Frames t >= lens[b] are never loaded.  An index outside
// [0, n_vert) is skipped and sets the status word.
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kMmThreads = 256;
constexpr int kChunk = 8;   // frames per chunk of mm_upper_kernel

struct MmArgs {
    const float* yt;
    long yt_cs, yt_fs;
    const float* yp;
    long yp_cs, yp_fs;
    const float* templ;   // may be null: zero template
    long templ_cs;
    const int32_t* lens;  // device copy in the workspace
    int B, L, n_vert, n_mouth, n_upper, n_chunk;
    const int32_t* mouth;
    const int32_t* upper;
    double* clip_out;
    double* frame_max;    // may be null
    int32_t* status;
    double* ws_fmax;      // [B][L]
    double* ws_part;      // [B][n_chunk][n_upper][4] = {mean_gt, m2_gt, mean_pred, m2_pred}
};

__device__ __forceinline__ double mm_shfl_xor(double v, int o) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, o);
    hi = __shfl_xor(hi, o);
    return __hiloint2double(hi, lo);
}

// |v|^2 as numpy's np.sum(np.square(v), axis=-1) rounds it: three products, two additions, no fused multiply-add
__device__ __forceinline__ double mm_sq3(double a, double b, double c) {
#pragma clang fp contract(off)
    return (a * a + b * b) + c * c;
}

__global__ __launch_bounds__(kMmThreads) void mm_frame_kernel(MmArgs a) {
    __shared__ double wmax[kMmThreads / 64];
    const int b = blockIdx.x / a.L, t = blockIdx.x - b * a.L;
    const size_t o = (size_t)b * a.L + t;
    if (t >= a.lens[b]) {   // padded frame: nothing is read
        if (threadIdx.x == 0) {
            a.ws_fmax[o] = 0.0;
            if (a.frame_max) a.frame_max[o] = 0.0;
        }
        return;
    }
    const float* g = a.yt + (size_t)b * a.yt_cs + (size_t)t * a.yt_fs;
    const float* p = a.yp + (size_t)b * a.yp_cs + (size_t)t * a.yp_fs;
    double mx = 0.0;   // d >= 0
    bool bad = false;
    for (int m = threadIdx.x; m < a.n_mouth; m += kMmThreads) {
        const int v = a.mouth[m];
        if ((unsigned)v >= (unsigned)a.n_vert) {
            bad = true;
            continue;
        }
        const size_t e = (size_t)v * 3;
        const double dx = (double)g[e] - (double)p[e], dy = (double)g[e + 1] - (double)p[e + 1], dz = (double)g[e + 2] - (double)p[e + 2];
        const double d = mm_sq3(dx, dy, dz);
        mx = d > mx || d != d ? d : mx;   // a NaN in a valid frame reaches the result, as np.max lets it
    }
    if (bad) *a.status = 1;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double ov = mm_shfl_xor(mx, s);
        mx = (ov > mx || ov != ov) ? ov : mx;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = wmax[0];
        for (int w = 1; w < kMmThreads / 64; ++w) r = (wmax[w] > r || wmax[w] != wmax[w]) ? wmax[w] : r;
        a.ws_fmax[o] = r;
        if (a.frame_max) a.frame_max[o] = r;
    }
}

__global__ __launch_bounds__(kMmThreads) void mm_upper_kernel(MmArgs a) {
    const int nblk = (a.n_upper + kMmThreads - 1) / kMmThreads;
    const int ub = blockIdx.x % nblk, bc = blockIdx.x / nblk;
    const int c = bc % a.n_chunk, b = bc / a.n_chunk;
    const int n = a.lens[b], t0 = c * kChunk;
    if (t0 >= n) return;   // the chunk lies in the padding: mm_clip_kernel does not read its partials
    const int u = ub * kMmThreads + threadIdx.x;
    if (u >= a.n_upper) return;
    const int cnt = min(kChunk, n - t0);
    double* out = a.ws_part + (((size_t)b * a.n_chunk + c) * a.n_upper + u) * 4;
    const int v = a.upper[u];
    if ((unsigned)v >= (unsigned)a.n_vert) {   // skipped entry: contributes a zero deviation
        *a.status = 1;
        out[0] = out[1] = out[2] = out[3] = 0.0;
        return;
    }
    const size_t e = (size_t)v * 3;
    double tx = 0.0, ty = 0.0, tz = 0.0;
    if (a.templ) {
        const float* tp = a.templ + (size_t)b * a.templ_cs + e;
        tx = (double)tp[0], ty = (double)tp[1], tz = (double)tp[2];
    }
    const float* g = a.yt + (size_t)b * a.yt_cs + (size_t)t0 * a.yt_fs + e;
    const float* p = a.yp + (size_t)b * a.yp_cs + (size_t)t0 * a.yp_fs + e;
    double sg[kChunk], sp[kChunk];
    double sum_g = 0.0, sum_p = 0.0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
        sg[k] = 0.0, sp[k] = 0.0;
        if (k < cnt) {
            const float* gk = g + (size_t)k * a.yt_fs;
            const float* pk = p + (size_t)k * a.yp_fs;
            sg[k] = mm_sq3((double)gk[0] - tx, (double)gk[1] - ty, (double)gk[2] - tz);
            sp[k] = mm_sq3((double)pk[0] - tx, (double)pk[1] - ty, (double)pk[2] - tz);
            sum_g += sg[k];
            sum_p += sp[k];
        }
    }
    const double mean_g = sum_g / (double)cnt, mean_p = sum_p / (double)cnt;
    double m2_g = 0.0, m2_p = 0.0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
        if (k < cnt) {
            const double dg = sg[k] - mean_g, dp = sp[k] - mean_p;
            m2_g += dg * dg;
            m2_p += dp * dp;
        }
    out[0] = mean_g, out[1] = m2_g, out[2] = mean_p, out[3] = m2_p;
}

__global__ __launch_bounds__(kMmThreads) void mm_clip_kernel(MmArgs a) {
    __shared__ double red[3][kMmThreads];
    const int b = blockIdx.x, n = a.lens[b];
    const int chunks = (n + kChunk - 1) / kChunk;
    double acc_g = 0.0, acc_p = 0.0, acc_f = 0.0;
    if (a.n_upper > 0)
        for (int u = threadIdx.x; u < a.n_upper; u += kMmThreads) {
            double na = 0.0, mean_g = 0.0, m2_g = 0.0, mean_p = 0.0, m2_p = 0.0;
            for (int c = 0; c < chunks; ++c) {
                const double* q = a.ws_part + (((size_t)b * a.n_chunk + c) * a.n_upper + u) * 4;
                const double nb = (double)min(kChunk, n - c * kChunk), nn = na + nb, w = nb / nn, f = na * w;
                const double dg = q[0] - mean_g, dp = q[2] - mean_p;
                mean_g += dg * w;
                m2_g += q[1] + dg * dg * f;
                mean_p += dp * w;
                m2_p += q[3] + dp * dp * f;
                na = nn;
            }
            acc_g += sqrt(m2_g / (double)n);
            acc_p += sqrt(m2_p / (double)n);
        }
    if (a.n_mouth > 0)
        for (int t = threadIdx.x; t < n; t += kMmThreads) acc_f += a.ws_fmax[(size_t)b * a.L + t];
    red[0][threadIdx.x] = acc_g, red[1][threadIdx.x] = acc_p, red[2][threadIdx.x] = acc_f;
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int i = 0; i < kMmThreads; ++i) s += red[threadIdx.x][i];
        double* o = a.clip_out + (size_t)b * 4;
        if (threadIdx.x == 0) o[2] = a.n_upper > 0 ? s / (double)a.n_upper : 0.0;
        if (threadIdx.x == 1) o[3] = a.n_upper > 0 ? s / (double)a.n_upper : 0.0;
        if (threadIdx.x == 2) o[0] = s, o[1] = (double)n;
    }
}

// workspace: lens int32 [B] (padded to 8 bytes) | frame maxima f64 [B][L] | chunk partials f64 [B][n_chunk][n_upper][4]
size_t mm_lens_bytes(int B) { return align_up((size_t)B * sizeof(int32_t), 8); }
int mm_chunks(int L) { return (L + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace dimx

using namespace dimx;

size_t dimx_op_mesh_metrics_ws_bytes(int B, int L, int n_mouth, int n_upper) {
    if (B < 1 || L < 1 || n_mouth < 0 || n_upper < 0) return 0;
    return mm_lens_bytes(B) + ((size_t)B * L + (size_t)B * mm_chunks(L) * n_upper * 4) * sizeof(double);
}

int dimx_op_mesh_metrics(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                         long yp_frame_stride, const float* templ, long templ_clip_stride, const int32_t* lens, int B, int L, int n_vert,
                         const int32_t* mouth, int n_mouth, const int32_t* upper, int n_upper, double* clip_out, double* frame_max,
                         int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(B > 0 && L > 0 && n_vert > 0, DIMX_ERR_ARG, "mesh_metrics: B=%d L=%d n_vert=%d must be positive", B, L, n_vert);
    DIMX_REQUIRE(n_mouth >= 0 && n_upper >= 0, DIMX_ERR_ARG, "mesh_metrics: n_mouth=%d n_upper=%d must not be negative", n_mouth, n_upper);
    DIMX_REQUIRE(y_true && y_pred && lens && clip_out && status && workspace, DIMX_ERR_ARG, "mesh_metrics: null operand");
    DIMX_REQUIRE((n_mouth == 0 || mouth) && (n_upper == 0 || upper), DIMX_ERR_ARG, "mesh_metrics: null map");
    DIMX_REQUIRE(yt_clip_stride >= 0 && yt_frame_stride >= 0 && yp_clip_stride >= 0 && yp_frame_stride >= 0 && templ_clip_stride >= 0,
                 DIMX_ERR_ARG, "mesh_metrics: negative stride");
    for (int b = 0; b < B; ++b)
        DIMX_REQUIRE(lens[b] >= 1 && lens[b] <= L, DIMX_ERR_ARG, "mesh_metrics: lens[%d]=%d outside 1..%d", b, lens[b], L);
    DIMX_REQUIRE(((uintptr_t)workspace & 7) == 0, DIMX_ERR_ARG, "mesh_metrics: workspace not 8-byte aligned");
    const size_t need = dimx_op_mesh_metrics_ws_bytes(B, L, n_mouth, n_upper);
    DIMX_REQUIRE(workspace_bytes >= need, DIMX_ERR_ARG, "mesh_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int n_chunk = mm_chunks(L), nblk = ceil_div(n_upper, kMmThreads);
    DIMX_REQUIRE((long long)B * L <= 0x7fffffffLL && (long long)B * n_chunk * nblk <= 0x7fffffffLL, DIMX_ERR_ARG,
                 "mesh_metrics: B=%d L=%d n_upper=%d exceed the grid", B, L, n_upper);
    MmArgs a;
    a.yt = y_true, a.yt_cs = yt_clip_stride, a.yt_fs = yt_frame_stride;
    a.yp = y_pred, a.yp_cs = yp_clip_stride, a.yp_fs = yp_frame_stride;
    a.templ = templ, a.templ_cs = templ_clip_stride;
    a.B = B, a.L = L, a.n_vert = n_vert, a.n_mouth = n_mouth, a.n_upper = n_upper, a.n_chunk = n_chunk;
    a.mouth = mouth, a.upper = upper;
    a.clip_out = clip_out, a.frame_max = frame_max, a.status = status;
    a.lens = (const int32_t*)workspace;
    a.ws_fmax = (double*)((char*)workspace + mm_lens_bytes(B));
    a.ws_part = a.ws_fmax + (size_t)B * L;
    hipStream_t s = (hipStream_t)stream;
    DIMX_HIP(hipMemcpyAsync(workspace, lens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DIMX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_mouth > 0)
        hipLaunchKernelGGL(mm_frame_kernel, dim3(B * L), dim3(kMmThreads), 0, s, a);
    else if (frame_max)
        DIMX_HIP(hipMemsetAsync(frame_max, 0, (size_t)B * L * sizeof(double), s));
    if (n_upper > 0) hipLaunchKernelGGL(mm_upper_kernel, dim3(B * n_chunk * nblk), dim3(kMmThreads), 0, s, a);
    hipLaunchKernelGGL(mm_clip_kernel, dim3(B), dim3(kMmThreads), 0, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
