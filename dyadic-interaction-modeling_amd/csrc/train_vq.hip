// train_vq.hip -- the non-GEMM operators of the VQ-VAE's own training step (stage 1, reference code/train_vq.py:173-196 over
// VQAutoEncoder.forward, code/models/stage1_BIWI.py:10-137, and calc_vq_loss, code/metrics/loss.py:6-11).
//
// Every reduction here has a fixed order (per-block partials in a fixed tree, summed by one thread in block order; the code
// counts are integer), so a step is bit-identical on rerun:
//   * quantiser forward: after the argmin of vq.hip, one pass writes the straight-through latent z + (e - z) and the per-block
//     partials of sum (e - z)^2; the finisher turns them into quant_loss = beta * mean + mean, the L1 partials into the
//     reconstruction loss, and the code counts into the perplexity exp(-sum p log(p + 1e-10));
//   * quantiser backward: the commitment term q beta 2 (z - e) / (N 128) added into d z_st in place; the codebook gradient
//     q 2 sum_{i: idx_i = j} (e_j - z_i) / (N 128) as a per-code segmented reduction in row order (one block per code);
//   * L1 loss: partials of |pred - x| and d pred = sign(pred - x) / (N 56) (sign(0) = 0) in one pass;
//   * positional row + Dropout(p): the keep mask is a counter-based function of (seed, step, site, b, t, c) -- see
//     dimx.prng.dropout_keep, which restates it -- so the backward pass regenerates it from (seed, step) alone;
//   * the LeakyReLU of vertice_mapping (in place in the reference) and its adjoint from the saved output's sign.
#include "train.hpp"

namespace dimx {
namespace {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr int kNE = 512, kZD = 128;

__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct DropKey {
    uint64_t key;
    uint32_t thr;
    float scale;
};
DropKey drop_key(float p, uint64_t seed, long step, int site) {
    DropKey k;
    k.key = mix64(seed + (uint64_t)(2 * step + site + 1) * kGold);
    k.thr = (uint32_t)((double)p * 16777216.0);
    k.scale = 1.0f / (1.0f - p);
    return k;
}
__device__ __forceinline__ bool keep_elem(const DropKey& k, int b, int t, int c) {
    const uint64_t ctr = ((uint64_t)b * 65536ull + (uint64_t)t) * 512ull + (uint64_t)c;
    return (uint32_t)(mix64(k.key + (ctr + 1ull) * kGold) >> 40) >= k.thr;
}
__device__ __forceinline__ unsigned code_of(const int32_t* idx, long r) {
    const unsigned j = (unsigned)idx[r];
    return j < (unsigned)kNE ? j : 0u;   // the argmin writes 0..511; a NaN latent must not index outside the codebook
}

inline int ew_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
inline int part_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > kVqPart ? kVqPart : g));
}

// sum over the block (256 threads) in a fixed order; valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0) s = ((red[0] + red[1]) + red[2]) + red[3];
    return s;
}

// y = (a + pe[b]) (* keep / (1 - p)); rows m = b * n + t of width C
__global__ void pe_dropout_fwd_kernel(const float* __restrict__ a, const float* __restrict__ pe, float* __restrict__ y, long total, int n,
                                      int C, DropKey k, int drop) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C), b = (int)(m / n), t = (int)(m - (long)b * n);
        float v = a[i] + pe[(size_t)b * C + c];
        if (drop) v = keep_elem(k, b, t, c) ? v * k.scale : 0.f;
        y[i] = v;
    }
}
__global__ void dropout_bwd_kernel(float* __restrict__ dy, long total, int n, int C, DropKey k) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C), b = (int)(m / n), t = (int)(m - (long)b * n);
        dy[i] = keep_elem(k, b, t, c) ? dy[i] * k.scale : 0.f;
    }
}
__global__ void lrelu_kernel(float* __restrict__ y, long n, float slope) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = y[i];
        y[i] = v > 0.f ? v : v * slope;
    }
}
// torch's in-place LeakyReLU backward: result > 0 ? dy : dy * slope
__global__ void lrelu_bwd_out_kernel(const float* __restrict__ y, float* __restrict__ dy, long n, float slope) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dy[i] = y[i] > 0.f ? dy[i] : dy[i] * slope;
}
// the k-major codebook and its squared norms exactly as the inference engine packs them (model.hip pack_vq: k-ascending fmaf)
__global__ void book_prep_kernel(const float* __restrict__ book, float* __restrict__ Et, float* __restrict__ ee) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kNE) return;
    float s = 0.f;
    for (int k = 0; k < kZD; ++k) {
        const float x = book[(size_t)j * kZD + k];
        Et[(size_t)k * kNE + j] = x;
        s = fmaf(x, x, s);
    }
    ee[j] = s;
}
__global__ __launch_bounds__(256) void vq_quant_fwd_kernel(const float* __restrict__ z, const float* __restrict__ book,
                                                           const int32_t* __restrict__ idx, float* __restrict__ zst,
                                                           float* __restrict__ part, long total) {
    __shared__ float red[4];
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i >> 7;
        const int c = (int)(i & 127);
        const float zv = z[i], d = book[(size_t)code_of(idx, r) * kZD + c] - zv;
        zst[i] = zv + d;   // z + sg(e - z), not e: the rounding differs
        acc = fmaf(d, d, acc);
    }
    const float s = block_sum256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ pred, const float* __restrict__ x, float* __restrict__ dpred,
                                                 float* __restrict__ part, long total, float inv) {
    __shared__ float red[4];
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float d = pred[i] - x[i];
        acc += fabsf(d);
        dpred[i] = d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
    }
    const float s = block_sum256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// out4 = {q quant + rec, rec, quant, perplexity}
__global__ __launch_bounds__(512) void vq_finish_kernel(const float* __restrict__ part_q, int nq, const float* __restrict__ part_l, int nl,
                                                        const int32_t* __restrict__ idx, int M, float beta, float qw, float* __restrict__ out) {
    __shared__ int cnt[kNE];
    __shared__ float red[8];
    const int tid = threadIdx.x;
    cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < M; i += kNE) atomicAdd(&cnt[code_of(idx, i)], 1);   // integer counts: exact in any order
    __syncthreads();
    const float p = (float)cnt[tid] / (float)M;
    const float v = wave_sum(p * logf(p + 1e-10f));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        float h = 0.f;
        for (int w = 0; w < 8; ++w) h += red[w];
        float sq = 0.f, sl = 0.f;
        for (int k = 0; k < nq; ++k) sq += part_q[k];
        for (int k = 0; k < nl; ++k) sl += part_l[k];
        const float mq = sq / ((float)M * (float)kZD);
        const float quant = beta * mq + mq;
        const float rec = sl / ((float)M * 56.f);
        out[0] = qw * quant + rec;
        out[1] = rec;
        out[2] = quant;
        out[3] = expf(-h);
    }
}
__global__ void vq_commit_bwd_kernel(const float* __restrict__ z, const float* __restrict__ book, const int32_t* __restrict__ idx,
                                     float* __restrict__ dz, long total, float coef) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i >> 7;
        const int c = (int)(i & 127);
        dz[i] += coef * (z[i] - book[(size_t)code_of(idx, r) * kZD + c]);
    }
}
// one block per code j, one thread per column: rows in ascending order
__global__ __launch_bounds__(128) void vq_book_grad_kernel(const float* __restrict__ z, const float* __restrict__ book,
                                                           const int32_t* __restrict__ idx, float* __restrict__ dbook, int M, float coef) {
    constexpr int kChunk = 2048;
    __shared__ int sidx[kChunk];
    const int j = blockIdx.x, c = threadIdx.x;
    const float e = book[(size_t)j * kZD + c];
    float acc = 0.f;
    for (int base = 0; base < M; base += kChunk) {
        const int len = M - base < kChunk ? M - base : kChunk;
        for (int r = c; r < len; r += 128) sidx[r] = (int)code_of(idx, base + r);
        __syncthreads();
        for (int r = 0; r < len; ++r)
            if (sidx[r] == j) acc += e - z[(size_t)(base + r) * kZD + c];
        __syncthreads();
    }
    dbook[(size_t)j * kZD + c] = coef * acc;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers
int tr_pe_dropout_fwd(const float* a, const float* pe, float* y, int M, int n, int C, float p, uint64_t seed, long step, int site,
                      hipStream_t s) {
    DIMX_REQUIRE(a && pe && y && M > 0 && n > 0 && n <= 65536 && C > 0 && C <= 512 && p >= 0.f && p < 1.f, DIMX_ERR_ARG,
                 "pe_dropout: bad arguments");
    const long total = (long)M * C;
    hipLaunchKernelGGL(pe_dropout_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, s, a, pe, y, total, n, C, drop_key(p, seed, step, site),
                       p > 0.f ? 1 : 0);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_dropout_bwd(float* dy, int M, int n, int C, float p, uint64_t seed, long step, int site, hipStream_t s) {
    DIMX_REQUIRE(dy && M > 0 && n > 0 && n <= 65536 && C > 0 && C <= 512 && p >= 0.f && p < 1.f, DIMX_ERR_ARG, "dropout_bwd: bad arguments");
    if (p == 0.f) return DIMX_OK;
    const long total = (long)M * C;
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, s, dy, total, n, C, drop_key(p, seed, step, site));
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_lrelu(float* y, long n, float slope, hipStream_t s) {
    hipLaunchKernelGGL(lrelu_kernel, dim3(ew_grid(n)), dim3(256), 0, s, y, n, slope);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_lrelu_bwd_out(const float* y, float* dy, long n, float slope, hipStream_t s) {
    hipLaunchKernelGGL(lrelu_bwd_out_kernel, dim3(ew_grid(n)), dim3(256), 0, s, y, dy, n, slope);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_vq_book_prep(const float* book, float* Et, float* ee, hipStream_t s) {
    hipLaunchKernelGGL(book_prep_kernel, dim3(kNE / 128), dim3(128), 0, s, book, Et, ee);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_vq_quant_fwd(const float* z, const float* book, const int32_t* idx, float* zst, float* part, int M, int* n_part, hipStream_t s) {
    const long total = (long)M * kZD;
    const int g = part_grid(total);
    *n_part = g;
    hipLaunchKernelGGL(vq_quant_fwd_kernel, dim3(g), dim3(256), 0, s, z, book, idx, zst, part, total);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_l1_loss(const float* pred, const float* x, float* dpred, float* part, long n, int* n_part, hipStream_t s) {
    const int g = part_grid(n);
    *n_part = g;
    hipLaunchKernelGGL(l1_kernel, dim3(g), dim3(256), 0, s, pred, x, dpred, part, n, 1.0f / (float)n);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_vq_finish(const float* part_q, int nq, const float* part_l, int nl, const int32_t* idx, int M, float beta, float qw, float* out4,
                 hipStream_t s) {
    DIMX_REQUIRE(nq >= 1 && nq <= kVqPart && nl >= 1 && nl <= kVqPart && M > 0, DIMX_ERR_ARG, "vq_finish: bad arguments");
    hipLaunchKernelGGL(vq_finish_kernel, dim3(1), dim3(kNE), 0, s, part_q, nq, part_l, nl, idx, M, beta, qw, out4);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_vq_commit_bwd(const float* z, const float* book, const int32_t* idx, float* dz, int M, float coef, hipStream_t s) {
    const long total = (long)M * kZD;
    hipLaunchKernelGGL(vq_commit_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, s, z, book, idx, dz, total, coef);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
int tr_vq_book_grad(const float* z, const float* book, const int32_t* idx, float* dbook, int M, float coef, hipStream_t s) {
    hipLaunchKernelGGL(vq_book_grad_kernel, dim3(kNE), dim3(kZD), 0, s, z, book, idx, dbook, M, coef);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
