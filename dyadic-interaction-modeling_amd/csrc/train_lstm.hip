// train_lstm.hip -- the adjoint of lstm.hip's recurrence (back-propagation through time of one bidirectional LSTM(384) layer)
// and the small kernels of the DIM-Speaker converter's training step (EmocaConverter, code/seq2seq_pretrain.py:759-842; the
// loop of code/train_converter.py:17-96): the mesh loss with its gradient, the shifted hidden states of dW_hh, the slab sum of
// the split-K input adjoint of the V-wide Linear.
//
// The training forward is lstm.hip's own kernels with their save switch: per (clip, frame, direction) the post-activation
// gates i, f, g, o, c_t and tanh c_t ([B*T][2][kLstmSave][H]).  The adjoint walks the forward order in reverse:
//     dh = dy_t + dh_rec;  do = dh tanh(c_t) o (1 - o);  dc += dh o (1 - tanh^2 c_t);
//     di = dc g i (1 - i);  df = dc c_prev f (1 - f);  dg = dc i (1 - g^2);  dc <- dc f;  dh_rec = W_hh^T dgates
// all f32, zero initial state, no per-clip lengths (padded frames take part exactly as in the forward).  It writes
// dgates [B*T][2][4H]; the weight and input gradients are GEMMs over it (train.hip).
//
//   This file carries the no-communication path only (the forward has a weight-stationary group kernel beside it; its mirror for
//   the adjoint -- a 1536 x 24 slice of W_hh^T in registers per block, the 1536 gate gradients per clip exchanged as tagged
//   granules -- is not in the tree: DESIGN.md section 12).
//   safe path (lstm_bwd_safe_kernel): one block of 768 threads per (4 clips, direction), no communication between blocks.
//     W_hh, regrouped once per call as [direction][4H / 4][H] float4 (four gate rows of one hidden unit per element), is re-read
//     from L2 every step: thread (half, u) adds 768 of the 1536 gate rows of column u for the four clips, the two halves are
//     added in a fixed order by the cell update.  What the next step needs of the saved forward is requested before the
//     products of this one.
//
// No float atomics: a rerun is bit-identical.
#include "common.hpp"
#include "train.hpp"

namespace dimx {

namespace {

constexpr int kH = 384;
constexpr int kG4 = 4 * kH;
constexpr int kSafeClips = 4;
constexpr int kBwdSafeThreads = 2 * kH;   // thread = (half of the gate rows, hidden unit)
constexpr int kBwdCells = kSafeClips * kH / kBwdSafeThreads;   // 2 cell updates per thread
constexpr int kHalfR4 = kG4 / 4 / 2;      // 192 float4 groups of gate rows per half

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

struct LstmBwdArgs {
    const float* dy;       // [B][T][2H]
    const float* save;     // [B*T][2][kLstmSave][H]
    const float4* w_bt;    // [2][4H / 4][H] float4: element (d, r4, u) = W_hh[d][4 r4 .. 4 r4 + 3][u]
    float* dgates;         // [B*T][2][4H]
    int B, T;
};

struct CellIn {
    float gi, gf, gg, go, tc, cp, dy;
};

__global__ __launch_bounds__(kBwdSafeThreads) void lstm_bwd_safe_kernel(const LstmBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_dg[kSafeClips][kG4];
    __shared__ float sh_dh[2][kSafeClips][kH];
    const int tid = threadIdx.x;
    const int dir = blockIdx.x & 1, c0 = (blockIdx.x >> 1) * kSafeClips;
    int nc = a.B - c0;
    nc = nc > kSafeClips ? kSafeClips : nc;
    const int T = a.T;
    const int half = tid / kH, mu = tid - half * kH;
    const float4* wp = a.w_bt + ((size_t)dir * (kG4 / 4) + (size_t)half * kHalfR4) * kH + mu;
    float dc[kBwdCells];
    CellIn in[kBwdCells];
#pragma unroll
    for (int i = 0; i < kBwdCells; ++i) dc[i] = 0.f;
    for (int i = tid; i < 2 * kSafeClips * kH; i += kBwdSafeThreads) (&sh_dh[0][0][0])[i] = 0.f;

    // the saved forward of step s (forward order), cell (b, u) = tid + i * threads
    auto fetch = [&](int s) {
        const int t = dir ? T - 1 - s : s;
#pragma unroll
        for (int i = 0; i < kBwdCells; ++i) {
            const int p = tid + i * kBwdSafeThreads, b = p / kH, u = p - b * kH;
            if (b >= nc) continue;
            const size_t row = (size_t)(c0 + b) * T + t;
            const float* sp = a.save + (row * 2 + dir) * (size_t)(kLstmSave * kH) + u;
            in[i].gi = sp[0];
            in[i].gf = sp[kH];
            in[i].gg = sp[2 * kH];
            in[i].go = sp[3 * kH];
            in[i].tc = sp[5 * kH];
            in[i].cp = 0.f;
            if (s > 0) {   // c of the step before in the direction's walk
                const size_t rowp = dir ? row + 1 : row - 1;
                in[i].cp = a.save[(rowp * 2 + dir) * (size_t)(kLstmSave * kH) + 4 * kH + u];
            }
            in[i].dy = a.dy[row * (2 * kH) + dir * kH + u];
        }
    };
    fetch(T - 1);

    for (int s = T - 1; s >= 0; --s) {
        const int t = dir ? T - 1 - s : s;
        __syncthreads();   // sh_dh of step s + 1 is complete
#pragma unroll
        for (int i = 0; i < kBwdCells; ++i) {
            const int p = tid + i * kBwdSafeThreads, b = p / kH, u = p - b * kH;
            float d_i = 0.f, d_f = 0.f, d_g = 0.f, d_o = 0.f;
            if (b < nc) {
                const CellIn& c = in[i];
                const float dh = c.dy + (sh_dh[0][b][u] + sh_dh[1][b][u]);
                d_o = dh * c.tc * c.go * (1.f - c.go);
                const float dcv = dc[i] + dh * c.go * (1.f - c.tc * c.tc);
                d_i = dcv * c.gg * c.gi * (1.f - c.gi);
                d_f = dcv * c.cp * c.gf * (1.f - c.gf);
                d_g = dcv * c.gi * (1.f - c.gg * c.gg);
                dc[i] = dcv * c.gf;
                float* gp = a.dgates + (((size_t)(c0 + b) * T + t) * 2 + dir) * kG4 + u;
                gp[0] = d_i;
                gp[kH] = d_f;
                gp[2 * kH] = d_g;
                gp[3 * kH] = d_o;
            }
            sh_dg[b][u] = d_i;
            sh_dg[b][kH + u] = d_f;
            sh_dg[b][2 * kH + u] = d_g;
            sh_dg[b][3 * kH + u] = d_o;
        }
        if (s == 0) break;
        fetch(s - 1);      // in flight during the products below
        __syncthreads();
        float acc[kSafeClips];
#pragma unroll
        for (int b = 0; b < kSafeClips; ++b) acc[b] = 0.f;
#pragma unroll 4
        for (int r4 = 0; r4 < kHalfR4; ++r4) {
            const float4 wv = wp[(size_t)r4 * kH];
#pragma unroll
            for (int b = 0; b < kSafeClips; ++b) acc[b] = dot4(wv, ((const float4*)sh_dg[b])[half * kHalfR4 + r4], acc[b]);
        }
#pragma unroll
        for (int b = 0; b < kSafeClips; ++b) sh_dh[half][b][mu] = acc[b];
    }
}

__global__ void lstm_bwd_pack_kernel(const float* w0, const float* w1, float4* wt) {
    const int total = 2 * (kG4 / 4) * kH;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int d = i / ((kG4 / 4) * kH), rem = i - d * (kG4 / 4) * kH;
        const int r4 = rem / kH, u = rem - r4 * kH;
        const float* w = (d ? w1 : w0) + (size_t)(4 * r4) * kH + u;
        wt[i] = make_float4(w[0], w[kH], w[2 * kH], w[3 * kH]);
    }
}

// hp[b][t][d * H + u] = y[b][t -/+ 1][d * H + u]: the hidden state that entered the cell update of frame t (zero at the start of
// each direction's walk) -- the right operand of dW_hh = dG^T . H_prev
__global__ void lstm_hprev_kernel(const float* __restrict__ y, float* __restrict__ hp, int B, int T) {
    const long total = (long)B * T * 2 * kH;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % (2 * kH));
        const long row = i / (2 * kH);
        const int t = (int)(row % T);
        const int tp = col < kH ? t - 1 : t + 1;
        hp[i] = (tp >= 0 && tp < T) ? y[(row + (tp - t)) * (2 * kH) + col] : 0.f;
    }
}

// loss = mse(xp, xv) + 5 mse(xp[.., map, :], xv[.., map, :]) with the mouth term as a per-vertex weight (multiplicity of the
// vertex in the map).  part[2 * block] = sum d^2, part[2 * block + 1] = sum w_v d^2; dY [M][Vp] (pad columns zero) optional.
__global__ __launch_bounds__(256) void mesh_loss_kernel(const float* __restrict__ xp, const float* __restrict__ xv, const float* __restrict__ vw,
                                                        int M, int V, int Vp, float c_full, float c_mouth, float* __restrict__ dY,
                                                        float* __restrict__ part) {
    __shared__ float sm[2][256];
    const long total = (long)M * Vp;
    float s0 = 0.f, s1 = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / Vp;
        const int col = (int)(i - row * Vp);
        float g = 0.f;
        if (col < V) {
            const float d = xp[row * V + col] - xv[row * V + col];
            const float w = vw ? vw[col / 3] : 0.f;
            s0 += d * d;
            s1 += w * d * d;
            g = (c_full + c_mouth * w) * d;
        }
        if (dY) dY[i] = g;
    }
    sm[0][threadIdx.x] = s0;
    sm[1][threadIdx.x] = s1;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            sm[0][threadIdx.x] += sm[0][threadIdx.x + k];
            sm[1][threadIdx.x] += sm[1][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sm[0][0];
        part[2 * blockIdx.x + 1] = sm[1][0];
    }
}

// out3 = {total, full-mesh mse, mouth mse}: the partials are added in a fixed order (f64: they are few)
__global__ __launch_bounds__(256) void mesh_loss_finish_kernel(const float* __restrict__ part, int n, double inv_full, double inv_mouth,
                                                               float* __restrict__ out3) {
    __shared__ double sm[2][256];
    double s0 = 0., s1 = 0.;
    for (int i = threadIdx.x; i < n; i += 256) {
        s0 += (double)part[2 * i];
        s1 += (double)part[2 * i + 1];
    }
    sm[0][threadIdx.x] = s0;
    sm[1][threadIdx.x] = s1;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            sm[0][threadIdx.x] += sm[0][threadIdx.x + k];
            sm[1][threadIdx.x] += sm[1][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mse = sm[0][0] * inv_full, mouth = sm[1][0] * inv_mouth;
        out3[0] = (float)(mse + 5.0 * mouth);
        out3[1] = (float)mse;
        out3[2] = (float)mouth;
    }
}

__global__ void sum_slabs_kernel(const float* __restrict__ slabs, int n, long stride, float* __restrict__ out, long count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
        float s = slabs[i];
        for (int k = 1; k < n; ++k) s += slabs[(size_t)k * stride + i];
        out[i] = s;
    }
}

struct BwdPlan {
    size_t off_wt, total;
};
BwdPlan plan_bwd(int B, int T) {
    BwdPlan p;
    p.off_wt = 0;
    p.total = align_up((size_t)2 * kG4 * kH * 4, 256);
    return p;
}

inline int ew_blocks(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

size_t lstm_bwd_scratch_bytes(int B, int T) { return plan_bwd(B, T).total; }

// The no-communication path is the only one: flags, cu_count and fault_count are accepted for the forward's calling convention
// (flags bit 0 and the default select the same kernel) and no fault can arise here.
int lstm_bwd_run(const float* dy, const float* save, const float* const* w_hh, int B, int T, float* dgates, void* scratch,
                 size_t scratch_bytes, int flags, int cu_count, int* fault_count, hipStream_t st) {
    DIMX_REQUIRE(dy && save && w_hh && w_hh[0] && w_hh[1] && dgates && scratch && B >= 1 && T >= 1, DIMX_ERR_ARG,
                 "lstm_bwd: null argument or bad shape (B=%d T=%d)", B, T);
    const BwdPlan p = plan_bwd(B, T);
    DIMX_REQUIRE(scratch_bytes >= p.total && ((uintptr_t)scratch % 256) == 0, DIMX_ERR_WORKSPACE, "lstm_bwd: scratch %zu < %zu", scratch_bytes,
                 p.total);
    (void)flags;
    (void)cu_count;
    (void)fault_count;
    float4* wt = (float4*)((unsigned char*)scratch + p.off_wt);
    hipLaunchKernelGGL(lstm_bwd_pack_kernel, dim3(512), dim3(256), 0, st, w_hh[0], w_hh[1], wt);
    DIMX_HIP(hipGetLastError());
    LstmBwdArgs a;
    a.dy = dy;
    a.save = save;
    a.w_bt = wt;
    a.dgates = dgates;
    a.B = B;
    a.T = T;
    hipLaunchKernelGGL(lstm_bwd_safe_kernel, dim3(2 * ceil_div(B, kSafeClips)), dim3(kBwdSafeThreads), 0, st, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int tr_lstm_hprev(const float* y, float* hp, int B, int T, hipStream_t s) {
    hipLaunchKernelGGL(lstm_hprev_kernel, dim3(ew_blocks((long)B * T * 2 * kH)), dim3(256), 0, s, y, hp, B, T);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int tr_mesh_loss_parts(int M, int Vp) { return ew_blocks((long)M * Vp); }

int tr_mesh_loss(const float* mesh, const float* target, const float* vert_w, int n_mouth, int M, int V, int Vp, float* dY, float* part,
                 float* loss_out, hipStream_t s) {
    DIMX_REQUIRE(mesh && target && part && loss_out && M >= 1 && V >= 3 && V % 3 == 0 && Vp >= V && (!vert_w || n_mouth >= 1), DIMX_ERR_ARG,
                 "mesh_loss: bad arguments (M=%d V=%d n_mouth=%d)", M, V, n_mouth);
    const double inv_full = 1.0 / ((double)M * V);
    const double inv_mouth = vert_w ? 1.0 / ((double)M * 3.0 * n_mouth) : 0.0;
    const int blocks = tr_mesh_loss_parts(M, Vp);
    hipLaunchKernelGGL(mesh_loss_kernel, dim3(blocks), dim3(256), 0, s, mesh, target, vert_w, M, V, Vp, (float)(2.0 * inv_full),
                       (float)(10.0 * inv_mouth), dY, part);
    hipLaunchKernelGGL(mesh_loss_finish_kernel, dim3(1), dim3(256), 0, s, part, blocks, inv_full, inv_mouth, loss_out);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int tr_sum_slabs(const float* slabs, int n, long stride, float* out, long count, hipStream_t s) {
    hipLaunchKernelGGL(sum_slabs_kernel, dim3(ew_blocks(count)), dim3(256), 0, s, slabs, n, stride, out, count);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
