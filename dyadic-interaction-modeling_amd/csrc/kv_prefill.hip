// kv_prefill.hip -- the layout moves of a prompted generation's prefill (dimx_generate_prompted, generate.hip):
//   * kv_rows_kernel: head rows that are contiguous on both sides -- the teacher-forced pass's self-attention K (and, in the
//     bf16 mode, V) [B, n, H*64] row-major -> the generation cache [B*S, H, T, 64], every clip's rows broadcast to its S samples;
//   * kv_tr_kernel (f32 mode only): a 64 x 64 transpose through LDS between a key-contiguous image [B, H, 64, ld_t] and a
//     channel-contiguous one [.., H, t, 64] -- the teacher-forced V^T -> the cache (broadcast to S rows), and the context V that
//     dimx_encode_ctx(for_generate = 1) left as [B, H, Tp, 64] -> the V^T the f32 prefill attention reads.
// Both move 16 bytes per lane on the global side; positions at or past n are neither read nor written on the channel-contiguous
// side (the cache beyond the prefix belongs to the decode steps), and only rows [b*S, b*S + S) of clip b are touched.
#include "common.hpp"

namespace dimx {
namespace {

// one 16-byte chunk per lane and (b, t, h): src chunk c of row (b, t, h) -> dst rows (b*S + s, h, t)
__global__ __launch_bounds__(256) void kv_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int B, int n, int H,
                                                      int cpr /*16-byte chunks per 64-element head row*/, int T, int S) {
    const long total = (long)B * n * H * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cpr);
        long r = i / cpr;                 // row-major source: r = (b*n + t)*H + h
        const int h = (int)(r % H);
        r /= H;
        const int t = (int)(r % n), b = (int)(r / n);
        const uint4 v = src[i];
        for (int s = 0; s < S; ++s) dst[((((size_t)b * S + s) * H + h) * T + t) * cpr + c] = v;
    }
}

// One block = one (b, h, 64-position tile).  TO_ROWS: src [B*H][64][ld_t] (key-contiguous) -> dst rows ((b*S + s)*H + h, t, 0:64)
// with row stride 64 and ld_rows positions per (row, head).  !TO_ROWS: src [(b*H + h)][ld_rows][64] -> dst [B*H][64][ld_t], S = 1.
// The tile lives in LDS as [64 t][65]: both the row-wise and the column-wise pass hit 64 distinct banks per wave.
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void kv_tr_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int n, int ld_t,
                                                    int ld_rows, int S) {
    __shared__ float tile[64][65];
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int t0 = blockIdx.x * 64;
    const int tid = threadIdx.x, q = tid & 15, r = tid >> 4;   // 16 lanes x 16 bytes = one 64-float row
    if (TO_ROWS) {
        const float* sp = src + (size_t)bh * 64 * ld_t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = r + 16 * k, t = t0 + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) v = *(const float4*)(sp + (size_t)d * ld_t + t);   // ld_t % 4 == 0 and >= n rounded up to 4 (launcher)
            tile[4 * q + 0][d] = v.x;
            tile[4 * q + 1][d] = v.y;
            tile[4 * q + 2][d] = v.z;
            tile[4 * q + 3][d] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tl = r + 16 * k, t = t0 + tl;
            if (t >= n) continue;
            const float4 v = make_float4(tile[tl][4 * q], tile[tl][4 * q + 1], tile[tl][4 * q + 2], tile[tl][4 * q + 3]);
            for (int s = 0; s < S; ++s)
                *(float4*)(dst + ((((size_t)b * S + s) * H + h) * ld_rows + t) * 64 + 4 * q) = v;
        }
    } else {
        const float* sp = src + (size_t)bh * ld_rows * 64;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tl = r + 16 * k, t = t0 + tl;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) v = *(const float4*)(sp + (size_t)t * 64 + 4 * q);
            tile[tl][4 * q + 0] = v.x;
            tile[tl][4 * q + 1] = v.y;
            tile[tl][4 * q + 2] = v.z;
            tile[tl][4 * q + 3] = v.w;
        }
        __syncthreads();
        float* dp = dst + (size_t)bh * 64 * ld_t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = r + 16 * k, t = t0 + 4 * q;
            if (t >= ld_t) continue;   // whole 4-position groups inside the padded row; positions >= n are written as 0
            *(float4*)(dp + (size_t)d * ld_t + t) = make_float4(tile[4 * q][d], tile[4 * q + 1][d], tile[4 * q + 2][d], tile[4 * q + 3][d]);
        }
    }
}

// inp[b*n0 + t] = clamp(prompt[b, t]) for the prefilled positions t < n0 (a negative entry -- forward_vq's -100 padding -- is
// token 0, as in dimx_decode_tf), and tokens[b*S + s, c] = clamp(prompt[b, c + 1]) for the columns c < n0 no decode step writes
__global__ void prompt_rows_kernel(const int32_t* __restrict__ prompt, int ld, int B, int n0, int V, int S, int32_t* __restrict__ inp,
                                   int32_t* __restrict__ tokens, int tok_ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n0) return;
    const int b = i / n0, t = i - b * n0;
    int a = prompt[(size_t)b * ld + t], c = prompt[(size_t)b * ld + t + 1];
    a = a < 0 ? 0 : (a >= V ? V - 1 : a);
    c = c < 0 ? 0 : (c >= V ? V - 1 : c);
    inp[i] = a;
    for (int s = 0; s < S; ++s) tokens[((size_t)b * S + s) * tok_ld + t] = c;
}

inline int grid_for(long total) {
    const long b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

}  // namespace

int launch_kv_rows_to_cache(int dtype, const void* src, void* cache, int B, int n, int H, int T, int S, hipStream_t st) {
    DIMX_REQUIRE(src && cache && B > 0 && n > 0 && n <= T && H > 0 && S > 0, DIMX_ERR_ARG, "kv_rows_to_cache: bad arguments (n=%d T=%d)", n, T);
    const int cpr = dtype == DIMX_BF16 ? 8 : 16;
    hipLaunchKernelGGL(kv_rows_kernel, dim3(grid_for((long)B * n * H * cpr)), dim3(256), 0, st, (const uint4*)src, (uint4*)cache, B, n, H,
                       cpr, T, S);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_kv_vt_to_cache(const float* vt, int ld_t, float* cache, int B, int n, int H, int T, int S, hipStream_t st) {
    DIMX_REQUIRE(vt && cache && B > 0 && n > 0 && n <= T && H > 0 && S > 0 && ld_t % 4 == 0 && ld_t >= (n + 3) / 4 * 4, DIMX_ERR_ARG,
                 "kv_vt_to_cache: bad arguments (n=%d T=%d ld=%d)", n, T, ld_t);
    hipLaunchKernelGGL((kv_tr_kernel<true>), dim3(ceil_div(n, 64), B * H), dim3(256), 0, st, vt, cache, H, n, ld_t, T, S);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_kv_rows_to_vt(const float* v_rows, int ld_rows, float* vt, int ld_t, int B, int n, int H, hipStream_t st) {
    DIMX_REQUIRE(v_rows && vt && B > 0 && n > 0 && n <= ld_rows && H > 0 && ld_t % 4 == 0 && ld_t >= n, DIMX_ERR_ARG,
                 "kv_rows_to_vt: bad arguments (n=%d rows=%d ld=%d)", n, ld_rows, ld_t);
    hipLaunchKernelGGL((kv_tr_kernel<false>), dim3(ceil_div(ld_t, 64), B * H), dim3(256), 0, st, v_rows, vt, H, n, ld_t, ld_rows, 1);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_prompt_rows(const int32_t* prompt, int ld, int B, int n0, int V, int S, int32_t* inp, int32_t* tokens, int tok_ld,
                       hipStream_t st) {
    DIMX_REQUIRE(prompt && inp && tokens && B > 0 && n0 > 0 && n0 < ld && n0 <= tok_ld && V > 0 && S > 0, DIMX_ERR_ARG,
                 "prompt_rows: bad arguments (n0=%d ld=%d)", n0, ld);
    hipLaunchKernelGGL(prompt_rows_kernel, dim3(ceil_div(B * n0, 256)), dim3(256), 0, st, prompt, ld, B, n0, V, S, inp, tokens, tok_ld);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
