// train_spk.hip -- the small kernels of the DIM-Speaker fine-tuning step (SpeakerSLMFT.forward(mode='train'),
// code/seq2seq_pretrain.py:708-757, under train_epoch_biwi, code/x_engine_pt.py:62-132): the decoder's context
//     ctx[b, t] = cat(speaker_embed[ids[b]] + patch_embed_dec_l, audio[b, t])
// its adjoint (d patch_embed_dec_l, the dense d speaker_embed), and the mean squared error of the decoded arg-max codes against
// the EMOCA stream shifted by one frame, with its gradient.
//
// All f32.  No float atomics, every sum in a fixed order: a rerun is bit-identical.
//   context adjoint:  part[b][s][c] = sum of dctx[b, t, c] over the frames of time slice s, ascending in t;
//                     clip[b][c]    = sum of part[b][s][c], ascending in s;
//                     d patch[c]    = sum of clip[b][c], ascending in b;
//                     d embed[r][c] = sum of clip[b][c] over the clips with ids[b] == r, ascending in b (zero for a row no clip
//                                     names: a gather per destination row, so duplicated ids need no scatter).
//   loss:             per-block f32 partials of (pred - target)^2 (tree inside the block), added in block order in f64.
#include "common.hpp"
#include "train.hpp"

namespace dimx {

namespace {

// one float4 per thread; C4 / A4 = float4 columns of the embedding / audio part of a context row
__global__ __launch_bounds__(256) void spk_ctx_kernel(const float4* __restrict__ embed, const int32_t* __restrict__ ids,
                                                      const float4* __restrict__ patch, const float4* __restrict__ audio,
                                                      float4* __restrict__ ctx, int T, int C4, int A4, long total) {
    const int D4 = C4 + A4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / D4;
        const int col = (int)(i - row * D4);
        float4 v;
        if (col < C4) {
            v = patch[col];
            if (ids) {
                const float4 e = embed[(long)ids[row / T] * C4 + col];
                v.x += e.x;
                v.y += e.y;
                v.z += e.z;
                v.w += e.w;
            }
        } else {
            v = audio[row * A4 + (col - C4)];
        }
        ctx[i] = v;
    }
}

// grid (kSpkSlices, B), one thread per column: part[b][s][c] over the frames [s * per, min(T, (s + 1) * per))
__global__ void spk_ctx_bwd_part_kernel(const float* __restrict__ dctx, float* __restrict__ part, int T, int C, int DD, int per) {
    const int s = blockIdx.x, b = blockIdx.y;
    const int t0 = s * per, t1 = min(T, t0 + per);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int t = t0; t < t1; ++t) acc += dctx[((long)b * T + t) * DD + c];
        part[((long)b * kSpkSlices + s) * C + c] = acc;
    }
}

// grid rows + 1: block r < rows writes d embed[r] (when there is an embedding), block `rows` writes d patch
__global__ void spk_ctx_bwd_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ ids, float* __restrict__ d_embed,
                                          float* __restrict__ d_patch, int B, int C, int rows) {
    const int r = blockIdx.x;
    const bool is_patch = r == rows;
    if (!is_patch && !d_embed) return;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) {
            if (!is_patch && !(ids && ids[b] == r)) continue;
            float clip = 0.f;
            for (int s = 0; s < kSpkSlices; ++s) clip += part[((long)b * kSpkSlices + s) * C + c];
            acc += clip;
        }
        if (is_patch)
            d_patch[c] = acc;
        else
            d_embed[(long)r * C + c] = acc;
    }
}

// pred [B][n][F4 float4] against tgt [B][n + 1][F4 float4] read one frame ahead; dpred = coef (pred - tgt)
__global__ __launch_bounds__(256) void spk_mse_kernel(const float4* __restrict__ pred, const float4* __restrict__ tgt, float4* __restrict__ dpred,
                                                      int n, int F4, float coef, long total, float* __restrict__ part) {
    __shared__ float sm[256];
    float acc = 0.f;
    const long per_clip = (long)n * F4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / per_clip;
        const float4 p = pred[i];
        const float4 t = tgt[i + (b + 1) * F4];   // (b (n + 1) + t + 1) F4 + k  =  i + (b + 1) F4
        const float dx = p.x - t.x, dy = p.y - t.y, dz = p.z - t.z, dw = p.w - t.w;
        acc += dx * dx + dy * dy + dz * dz + dw * dw;
        dpred[i] = make_float4(coef * dx, coef * dy, coef * dz, coef * dw);
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// out2 = {mean squared error, 1 / elements}: the block partials added in block order (f64: they are few)
__global__ __launch_bounds__(64) void spk_mse_finish_kernel(const float* __restrict__ part, int nblk, double inv, float* __restrict__ out2) {
    if (threadIdx.x != 0) return;
    double s = 0.;
    for (int i = 0; i < nblk; ++i) s += (double)part[i];
    out2[0] = (float)(s * inv);
    out2[1] = (float)inv;
}

inline int spk_blocks(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > kSpkMseParts ? kSpkMseParts : b));
}

}  // namespace

int tr_spk_context(const float* embed, const int32_t* ids, const float* patch, const float* audio, float* ctx, int B, int T, int C, int A,
                   hipStream_t s) {
    DIMX_REQUIRE(patch && audio && ctx && (embed || !ids) && B >= 1 && T >= 1 && C >= 4 && A >= 4 && C % 4 == 0 && A % 4 == 0, DIMX_ERR_ARG,
                 "spk_context: bad arguments (B=%d T=%d C=%d A=%d)", B, T, C, A);
    DIMX_REQUIRE(((uintptr_t)embed % 16) == 0 && ((uintptr_t)patch % 16) == 0 && ((uintptr_t)audio % 16) == 0 && ((uintptr_t)ctx % 16) == 0,
                 DIMX_ERR_ARG, "spk_context: operands must be 16-byte aligned");
    const long total = (long)B * T * ((C + A) / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(spk_ctx_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, (const float4*)embed, ids,
                       (const float4*)patch, (const float4*)audio, (float4*)ctx, T, C / 4, A / 4, total);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

size_t tr_spk_context_bwd_floats(int B, int C) { return (size_t)B * kSpkSlices * C; }

int tr_spk_context_bwd(const float* dctx, const int32_t* ids, float* d_embed, float* d_patch, float* part, int B, int T, int C, int DD,
                       int rows, hipStream_t s) {
    DIMX_REQUIRE(dctx && d_patch && part && B >= 1 && T >= 1 && C >= 1 && DD >= C && rows >= 0 && (d_embed || rows == 0), DIMX_ERR_ARG,
                 "spk_context_bwd: bad arguments (B=%d T=%d C=%d rows=%d)", B, T, C, rows);
    const int per = ceil_div(T, kSpkSlices);
    const int threads = C >= 384 ? 384 : 64 * ceil_div(C, 64);
    hipLaunchKernelGGL(spk_ctx_bwd_part_kernel, dim3(kSpkSlices, B), dim3(threads), 0, s, dctx, part, T, C, DD, per);
    hipLaunchKernelGGL(spk_ctx_bwd_finish_kernel, dim3(rows + 1), dim3(threads), 0, s, part, ids, d_embed, d_patch, B, C, rows);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int tr_spk_mse(const float* pred, const float* tgt, float* dpred, int B, int T, int F, float* part, float* out2, hipStream_t s) {
    DIMX_REQUIRE(pred && tgt && dpred && part && out2 && B >= 1 && T >= 2 && F >= 4 && F % 4 == 0, DIMX_ERR_ARG,
                 "spk_mse: bad arguments (B=%d T=%d F=%d)", B, T, F);
    DIMX_REQUIRE(((uintptr_t)pred % 16) == 0 && ((uintptr_t)tgt % 16) == 0 && ((uintptr_t)dpred % 16) == 0, DIMX_ERR_ARG,
                 "spk_mse: operands must be 16-byte aligned");
    const int n = T - 1;
    const long total = (long)B * n * (F / 4);
    const double inv = 1.0 / ((double)B * n * F);
    const int blocks = spk_blocks(total);
    hipLaunchKernelGGL(spk_mse_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)pred, (const float4*)tgt, (float4*)dpred, n, F / 4,
                       (float)(2.0 * inv), total, part);
    hipLaunchKernelGGL(spk_mse_finish_kernel, dim3(1), dim3(64), 0, s, part, blocks, inv, out2);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
