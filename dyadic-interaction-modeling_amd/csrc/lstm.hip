// lstm.hip -- one bidirectional LSTM layer (hidden 384) for the DIM-Speaker mesh head.
//
// Reference arithmetic: torch.nn.LSTM(batch_first=True, bidirectional=True) in eval mode with zero initial state
// (EmocaConverter.vertice_map_reverse_lstm, code/seq2seq_pretrain.py:801-807, applied at :671 / :834).  Gate order in
// the weights i, f, g, o;  c = sigmoid(f) c + sigmoid(i) tanh(g);  h = sigmoid(o) tanh(c);  output [B, T, 2H], forward
// direction first.  THERE ARE NO PER-CLIP LENGTHS: the reference runs the LSTM over all T padded frames of a batch (the
// BIWI engines pass an all-ones mask), so the reverse direction starts at the last PADDED frame of every clip.  That is
// kept, as dimx_vq_decode keeps the reference's InstanceNorm over padded frames.
//
// The input projection x . W_ih^T + (b_ih + b_hh) of all T frames and both directions is ONE launch of the library's GEMM
// (N = 2 x 4H = 3072).  The recurrence is the new kernel, one launch per layer (per 128 clips):
//
//   group path (lstm_group_kernel): 256 blocks of 384 threads, one per CU.  Blocks with equal blockIdx % 8 form a
//     group (under the dispatcher's round-robin dealing they share an XCD: that is a speed bonus, the protocol below
//     does not depend on it).  A group owns up to 16 clips; its 32 blocks are 2 directions x 16 slices.  A slice holds
//     all four gates of 24 hidden units: 96 rows x 384 of W_hh = 144 KiB, kept in REGISTERS for all T steps (96 floats
//     per lane, thread (row, q) owns the 16-byte chunks 4 j + q of its row), so the cell update of a unit is local to
//     its block.  Per step the 16 blocks of a (group, direction) exchange h_t (clips x 384) through global memory as
//     8-byte {tag, value} granules written by one write-through store each and polled with L1-bypassing loads
//     (tag = step + 1; two buffers alternate by step parity: a block can be at most one step ahead of a block that
//     still reads).  Every poll is bounded; a timeout sets bit 1 of the fault word, every block leaves, and the caller
//     reruns the layer on the safe path.
//   safe path (lstm_safe_kernel): one block of 512 threads per (4 clips, direction), no communication between blocks;
//     W_hh (transposed once per call) is re-read from L2 every step.  It runs when the device does not have 256 CUs,
//     after a fault, or on request (flags bit 0), and it is the second implementation the tests cross-check.
//
// c, h, the gate sums and sigmoid / tanh are f32.  Both numeric modes run this f32 recurrence.
#include "common.hpp"

namespace dimx {

namespace {

constexpr int kH = 384;             // hidden size (the only one built)
constexpr int kG4 = 4 * kH;         // gate rows per direction
constexpr int kSlices = 16;         // blocks per (group, direction)
constexpr int kUnits = kH / kSlices;        // 24 hidden units per slice
constexpr int kRows = 4 * kUnits;           // 96 rows of W_hh per slice
constexpr int kGroupThreads = 4 * kRows;    // 384: thread = (row, quarter of K)
constexpr int kGroups = 8;
constexpr int kGroupClips = 16;             // clips per group: 24 units x 16 clips = one cell update per thread
constexpr int kGridBlocks = kGroups * 2 * kSlices;   // 256
constexpr int kSafeThreads = 512;
constexpr int kSafeClips = 4;
constexpr size_t kErrBytes = 256;
constexpr size_t kXchGranules = (size_t)kGroups * 2 * 2 * kGroupClips * kH;

typedef unsigned long long u64;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

struct LstmArgs {
    const float* pre;      // [B*T][2][4H]: x . W_ih^T + b_ih + b_hh, gate order i f g o
    const float* w_hh[2];  // [4H][H] row-major
    const float4* w_hh_t;  // safe path: [2][H/4][4H] float4, element (d, k4, row) = W_hh[d][row][4 k4 .. 4 k4 + 3]
    float* y;              // [B][T][2H]
    int B, T;
    int b0, nb;            // group path: the clips [b0, b0 + nb) of this launch, nb <= 128
    u64* xch;              // [8 groups][2 directions][2 parities][16 clips][H] granules, zeroed before every launch
    unsigned* err;         // bit 1: a poll timed out
    float* save;           // training forward (kSave): [B*T][2][kLstmSave][H] = i, f, g, o (post-activation), c_t, tanh c_t
};

// what the adjoint (train_lstm.hip) needs of one cell update; the arithmetic of y does not depend on kSave
template <bool kSave>
__device__ __forceinline__ void lstm_save(const LstmArgs& a, size_t row, int dir, int unit, float gi, float gf, float gg, float go, float c,
                                          float tc) {
    if (!kSave) return;
    float* sp = a.save + (row * 2 + dir) * (size_t)(kLstmSave * kH) + unit;
    sp[0] = gi;
    sp[kH] = gf;
    sp[2 * kH] = gg;
    sp[3 * kH] = go;
    sp[4 * kH] = c;
    sp[5 * kH] = tc;
}

template <bool kSave>
__global__ __launch_bounds__(kGroupThreads) void lstm_group_kernel(const LstmArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_h[kGroupClips][kH];
    __shared__ float sh_g[kGroupClips][kRows];
    __shared__ int sh_fail;
    const int tid = threadIdx.x;
    const int grp = blockIdx.x & (kGroups - 1), mem = blockIdx.x >> 3;
    const int dir = mem >> 4, sl = mem & (kSlices - 1);
    // clips of this group: the launch's nb clips dealt in equal runs over min(8, nb) groups
    const int ngrp = a.nb < kGroups ? a.nb : kGroups;
    const int per = (a.nb + ngrp - 1) / ngrp;
    const int c0 = a.b0 + grp * per;
    int nc = a.b0 + a.nb - c0;
    nc = nc > per ? per : nc;
    if (grp >= ngrp || nc <= 0) return;   // the whole group leaves

    // this thread's 96 weights: row = (unit, gate) of the slice, chunks 4 j + q of the row
    const int row = tid >> 2, q = tid & 3;
    const int w_row = (row & 3) * kH + sl * kUnits + (row >> 2);
    float4 w[24];
    {
        const float4* wp = (const float4*)(a.w_hh[dir] + (size_t)w_row * kH);
#pragma unroll
        for (int j = 0; j < 24; ++j) w[j] = wp[4 * j + q];
    }
    // cell-update role: one (unit, clip) pair per thread
    const int cu_u = tid % kUnits, cu_b = tid / kUnits;
    const bool cu_on = cu_b < nc;
    const int unit = sl * kUnits + cu_u;
    float c = 0.f;
    if (tid == 0) sh_fail = 0;
    u64* xbase = a.xch + (size_t)((grp * 2 + dir) * 2) * kGroupClips * kH;
    const int T = a.T;

    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s;
        float p_i = 0.f, p_f = 0.f, p_g = 0.f, p_o = 0.f;
        if (cu_on) {   // requested before the wait for h
            const float* pp = a.pre + ((size_t)(c0 + cu_b) * T + t) * (2 * kG4) + dir * kG4 + unit;
            p_i = pp[0];
            p_f = pp[kH];
            p_g = pp[2 * kH];
            p_o = pp[3 * kH];
        }
        if (s > 0) {   // h of step s - 1, column tid of every clip of the group
            const u64* src = xbase + (size_t)((s - 1) & 1) * kGroupClips * kH + tid;
            const unsigned tag = (unsigned)s;
            for (int b = 0; b < nc; ++b) {
                unsigned spins = 0;
                for (;;) {
                    const u64 g = __hip_atomic_load(src + (size_t)b * kH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(g >> 32) == tag) {
                        sh_h[b][tid] = __uint_as_float((unsigned)g);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                    ++spins;
                    if (spins > (1u << 20) ||
                        ((spins & 1023u) == 0 && (__hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u))) {
                        atomicOr(a.err, 2u);   // bounded: a block that is not resident would otherwise hang the device
                        sh_fail = 1;
                        break;
                    }
                }
            }
        }
        __syncthreads();
        if (sh_fail) return;
        if (s > 0) {
            for (int b = 0; b < nc; ++b) {
                const float4* hp = (const float4*)sh_h[b];
                float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
                for (int j = 0; j < 24; j += 2) {
                    acc0 = dot4(w[j], hp[4 * j + q], acc0);
                    acc1 = dot4(w[j + 1], hp[4 * j + 4 + q], acc1);
                }
                float acc = acc0 + acc1;
                acc += __shfl_xor(acc, 1);
                acc += __shfl_xor(acc, 2);
                if (q == 0) sh_g[b][row] = acc;
            }
        }
        __syncthreads();
        if (cu_on) {
            if (s > 0) {
                const float* gp = &sh_g[cu_b][cu_u * 4];
                p_i += gp[0];
                p_f += gp[1];
                p_g += gp[2];
                p_o += gp[3];
            }
            const float gi = sigmoid_f(p_i), gf = sigmoid_f(p_f), gg = tanhf(p_g), go = sigmoid_f(p_o);
            c = gf * c + gi * gg;
            const float tc = tanhf(c);
            const float h = go * tc;
            a.y[((size_t)(c0 + cu_b) * T + t) * (2 * kH) + dir * kH + unit] = h;
            lstm_save<kSave>(a, (size_t)(c0 + cu_b) * T + t, dir, unit, gi, gf, gg, go, c, tc);
            if (s + 1 < T)
                __hip_atomic_store(xbase + ((size_t)(s & 1) * kGroupClips + cu_b) * kH + unit,
                                   ((u64)(unsigned)(s + 1) << 32) | __float_as_uint(h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool kSave>
__global__ __launch_bounds__(kSafeThreads) void lstm_safe_kernel(const LstmArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_h[kSafeClips][kH];
    __shared__ float sh_g[kSafeClips][kG4];
    const int tid = threadIdx.x;
    const int dir = blockIdx.x & 1, c0 = (blockIdx.x >> 1) * kSafeClips;
    int nc = a.B - c0;
    nc = nc > kSafeClips ? kSafeClips : nc;
    const int T = a.T;
    const float4* wt = a.w_hh_t + (size_t)dir * (kH / 4) * kG4;
    float c[3] = {0.f, 0.f, 0.f};
    for (int i = tid; i < kSafeClips * kH; i += kSafeThreads) (&sh_h[0][0])[i] = 0.f;

    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s;
        __syncthreads();
        if (s > 0) {
            float acc[3][kSafeClips];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int b = 0; b < kSafeClips; ++b) acc[r][b] = 0.f;
            for (int k4 = 0; k4 < kH / 4; ++k4) {
                float4 wv[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) wv[r] = wt[(size_t)k4 * kG4 + tid + r * kSafeThreads];
#pragma unroll
                for (int b = 0; b < kSafeClips; ++b) {
                    const float4 hv = ((const float4*)sh_h[b])[k4];
#pragma unroll
                    for (int r = 0; r < 3; ++r) acc[r][b] = dot4(wv[r], hv, acc[r][b]);
                }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int b = 0; b < kSafeClips; ++b) sh_g[b][tid + r * kSafeThreads] = acc[r][b];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int p = tid + i * kSafeThreads, b = p / kH, u = p - b * kH;
            if (b >= nc) continue;
            const float* pp = a.pre + ((size_t)(c0 + b) * T + t) * (2 * kG4) + dir * kG4 + u;
            float p_i = pp[0], p_f = pp[kH], p_g = pp[2 * kH], p_o = pp[3 * kH];
            if (s > 0) {
                p_i += sh_g[b][u];
                p_f += sh_g[b][kH + u];
                p_g += sh_g[b][2 * kH + u];
                p_o += sh_g[b][3 * kH + u];
            }
            const float gi = sigmoid_f(p_i), gf = sigmoid_f(p_f), gg = tanhf(p_g), go = sigmoid_f(p_o);
            c[i] = gf * c[i] + gi * gg;
            const float tc = tanhf(c[i]);
            const float h = go * tc;
            a.y[((size_t)(c0 + b) * T + t) * (2 * kH) + dir * kH + u] = h;
            lstm_save<kSave>(a, (size_t)(c0 + b) * T + t, dir, u, gi, gf, gg, go, c[i], tc);
            sh_h[b][u] = h;   // read by the next step's products, behind its first barrier
        }
    }
}

// W_ih of both directions stacked and K-padded: wcat [2 * 4H][Kp], bias [2 * 4H] = b_ih + b_hh
__global__ void lstm_pack_ih_kernel(const float* w0, const float* w1, const float* bi0, const float* bi1, const float* bh0,
                                    const float* bh1, int In, int Kp, float* wcat, float* bias) {
    const long total = (long)2 * kG4 * Kp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / Kp), k = (int)(i - (long)n * Kp);
        const int d = n / kG4, r = n - d * kG4;
        wcat[i] = k < In ? (d ? w1 : w0)[(size_t)r * In + k] : 0.f;
        if (k == 0) bias[n] = (d ? bi1 : bi0)[r] + (d ? bh1 : bh0)[r];
    }
}

__global__ void lstm_pack_hh_t_kernel(const float* w0, const float* w1, float4* wt) {
    const int total = 2 * (kH / 4) * kG4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int d = i / ((kH / 4) * kG4), rem = i - d * (kH / 4) * kG4;
        const int k4 = rem / kG4, r = rem - k4 * kG4;
        wt[i] = *(const float4*)((d ? w1 : w0) + (size_t)r * kH + 4 * k4);
    }
}

struct Plan {
    size_t off_err, off_xch, off_wcat, off_bias, off_xpad, off_pre, off_wt, total;
    int Kp;
};

Plan plan_scratch(int B, int T, int In) {
    Plan p;
    const size_t M = (size_t)B * T;
    p.Kp = (In + 31) / 32 * 32;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    p.off_err = take(kErrBytes);
    p.off_xch = take(kXchGranules * 8);
    p.off_wcat = take((size_t)2 * kG4 * p.Kp * 4);
    p.off_bias = take((size_t)2 * kG4 * 4);
    p.off_xpad = take(p.Kp != In ? M * p.Kp * 4 : 0);
    p.off_pre = take(M * 2 * kG4 * 4);
    p.off_wt = take((size_t)2 * kH * kG4 * 4);
    p.total = o;
    return p;
}

}  // namespace

size_t lstm_scratch_bytes(int B, int T, int In) { return plan_scratch(B, T, In).total; }

// One layer.  x [B*T][In] f32, weights as torch.nn.LSTM keeps them (w_ih [4H][In], w_hh [4H][H], biases [4H]; index 0
// forward, 1 reverse), y [B][T][2H].  flags bit 0: safe path.  On the group path the call WAITS for the layer (it reads
// the fault word); *fault_count is incremented when the layer had to be rerun on the safe path.  save (optional): the
// training forward -- the same kernels also store [B*T][2][kLstmSave][H] for the adjoint; y is what it is without.
int lstm_layer_run(const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                   const float* const* b_ih, const float* const* b_hh, float* y, void* scratch, size_t scratch_bytes, int flags,
                   int cu_count, int* fault_count, hipStream_t st, float* save) {
    DIMX_REQUIRE(H == kH, DIMX_ERR_ARG, "lstm: only hidden size %d is built (H=%d)", kH, H);
    DIMX_REQUIRE(x && y && scratch && w_ih && w_hh && b_ih && b_hh && B >= 1 && T >= 1 && In >= 4 && In % 4 == 0, DIMX_ERR_ARG,
                 "lstm: null argument or bad shape (B=%d T=%d In=%d)", B, T, In);
    for (int d = 0; d < 2; ++d)
        DIMX_REQUIRE(w_ih[d] && w_hh[d] && b_ih[d] && b_hh[d] && ((uintptr_t)w_hh[d] % 16) == 0, DIMX_ERR_ARG,
                     "lstm: null or misaligned weight (direction %d)", d);
    const Plan p = plan_scratch(B, T, In);
    DIMX_REQUIRE(scratch_bytes >= p.total && ((uintptr_t)scratch % 256) == 0, DIMX_ERR_WORKSPACE, "lstm: scratch %zu < %zu", scratch_bytes,
                 p.total);
    unsigned char* sb = (unsigned char*)scratch;
    unsigned* err = (unsigned*)(sb + p.off_err);
    float* wcat = (float*)(sb + p.off_wcat);
    float* bias = (float*)(sb + p.off_bias);
    float* pre = (float*)(sb + p.off_pre);
    const int M = B * T;

    hipLaunchKernelGGL(lstm_pack_ih_kernel, dim3(512), dim3(256), 0, st, w_ih[0], w_ih[1], b_ih[0], b_ih[1], b_hh[0], b_hh[1], In, p.Kp,
                       wcat, bias);
    DIMX_HIP(hipGetLastError());
    const float* A = x;
    int lda = In;
    if (p.Kp != In) {
        DIMX_TRY(launch_cast_pad(DIMX_F32, x, In, nullptr, sb + p.off_xpad, p.Kp, M, In, st));
        A = (const float*)(sb + p.off_xpad);
        lda = p.Kp;
    }
    GemmArgs g;
    gemm_args_init(g);
    g.in_dtype = DIMX_F32;
    g.out_dtype = DIMX_F32;
    g.A = A;
    g.lda = lda;
    g.W = wcat;
    g.ldw = p.Kp;
    g.M = M;
    g.N = 2 * kG4;
    g.K = p.Kp;
    g.bias = bias;
    gemm_set_plain_out(g, pre, 2 * kG4);
    DIMX_TRY(launch_gemm(g, st));

    LstmArgs a;
    a.pre = pre;
    a.w_hh[0] = w_hh[0];
    a.w_hh[1] = w_hh[1];
    a.w_hh_t = (const float4*)(sb + p.off_wt);
    a.y = y;
    a.B = B;
    a.T = T;
    a.xch = (u64*)(sb + p.off_xch);
    a.err = err;
    a.save = save;
    bool safe = (flags & 1) != 0 || cu_count != kGridBlocks;
    if (!safe) {
        DIMX_HIP(hipMemsetAsync(err, 0, kErrBytes, st));
        for (int b0 = 0; b0 < B; b0 += kGroups * kGroupClips) {
            a.b0 = b0;
            a.nb = B - b0 < kGroups * kGroupClips ? B - b0 : kGroups * kGroupClips;
            DIMX_HIP(hipMemsetAsync(a.xch, 0, kXchGranules * 8, st));
            if (save) hipLaunchKernelGGL(lstm_group_kernel<true>, dim3(kGridBlocks), dim3(kGroupThreads), 0, st, a);
            else hipLaunchKernelGGL(lstm_group_kernel<false>, dim3(kGridBlocks), dim3(kGroupThreads), 0, st, a);
            DIMX_HIP(hipGetLastError());
        }
        unsigned host_err = 0;
        DIMX_HIP(hipMemcpyAsync(&host_err, err, 4, hipMemcpyDeviceToHost, st));
        DIMX_HIP(hipStreamSynchronize(st));
        if (host_err) {   // a poll timed out (the 256 blocks were not co-resident): the layer is recomputed below
            if (fault_count) ++*fault_count;
            safe = true;
        }
    }
    if (safe) {
        hipLaunchKernelGGL(lstm_pack_hh_t_kernel, dim3(512), dim3(256), 0, st, w_hh[0], w_hh[1], (float4*)(sb + p.off_wt));
        DIMX_HIP(hipGetLastError());
        a.b0 = 0;
        a.nb = B;
        if (save) hipLaunchKernelGGL(lstm_safe_kernel<true>, dim3(2 * ceil_div(B, kSafeClips)), dim3(kSafeThreads), 0, st, a);
        else hipLaunchKernelGGL(lstm_safe_kernel<false>, dim3(2 * ceil_div(B, kSafeClips)), dim3(kSafeThreads), 0, st, a);
        DIMX_HIP(hipGetLastError());
    }
    return DIMX_OK;
}

}  // namespace dimx
