// seq_score.hip -- sequence log-likelihoods over dumped logits, and the best-of-S pick by them.
//
// The model's own verdict on a sampled sequence: sum over the scored columns of logits[tok] - logsumexp(logits), the float64 value
// of that formula on the f32 logits (the definition is dimx/scoring.py).  Two launches, one per entry point, no atomics, no host
// synchronisation, every sum in a fixed order:
//   seq_logprob_kernel (one block per row): wave w takes the columns first + w, first + w + 4, ...; lane l holds entries l + 64 c,
//                      c = 0..7 (the sampler's map: 256 contiguous bytes per load instruction).  Exact f32 row maximum, exp of the
//                      double difference, double wave sum (xor 32, 16, ... 1), double log; lane 0 carries the wave's partial, the
//                      four partials meet in LDS and are added in wave order.
//   score_pick_kernel  (one block per clip): first maximum of the row (NaN counts as -inf), ok flag, gather of the winner.
#include "common.hpp"
#include "pick_gather.hpp"

namespace dimx {
namespace {

constexpr int kVocab = 512;        // the sampler's vocabulary: 8 entries per lane of a wave
constexpr int kSeqThreads = 256;
constexpr int kSeqWaves = kSeqThreads / 64;
constexpr int kPickThreads = 256;

struct SeqArgs {
    const float* logits;
    long row_stride, step_stride;
    const int32_t* tokens;
    long tok_rs;
    const int32_t* first;
    const int32_t* last;
    int rpc, n;
    double* tok_lp;
    double* score;
    int32_t* count;
};

__device__ __forceinline__ int clamp_col(int c, int n) { return c < 0 ? 0 : (c > n ? n : c); }

__global__ __launch_bounds__(kSeqThreads) void seq_logprob_kernel(SeqArgs a) {
    __shared__ double sh_sum[kSeqWaves];
    __shared__ int sh_cnt[kSeqWaves];
    const int r = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int clip = r / a.rpc, n = a.n;
    const int c0 = clamp_col(a.first ? a.first[clip] : 0, n), c1 = clamp_col(a.last ? a.last[clip] : n, n);
    const float* row = a.logits + (size_t)r * a.row_stride;
    const int32_t* trow = a.tokens + (size_t)r * a.tok_rs;
    double* lprow = a.tok_lp ? a.tok_lp + (size_t)r * n : nullptr;
    if (lprow)
        for (int c = threadIdx.x; c < n; c += kSeqThreads)
            if (c < c0 || c >= c1) lprow[c] = 0.0;
    double acc = 0.0;
    int cnt = 0;
    for (int c = c0 + w; c < c1; c += kSeqWaves) {   // wave-uniform: every lane of the wave walks the same columns
        const int tok = __builtin_amdgcn_readfirstlane(trow[c]);
        if ((unsigned)tok >= (unsigned)kVocab) {     // the -100 padding of forward_vq and anything else outside the vocabulary
            if (lprow && lane == 0) lprow[c] = 0.0;
            continue;
        }
        const float* p = row + (size_t)c * a.step_stride;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[lane + 64 * k];
        float m = v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) m = fmaxf(m, v[k]);
        m = wave_max(m);
        const double md = (double)m;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += exp((double)v[k] - md);
        s = wave_sum_f64(s);
        const double lp = ((double)p[tok] - md) - log(s);
        acc += lp;
        ++cnt;
        if (lprow && lane == 0) lprow[c] = lp;
    }
    if (lane == 0) {
        sh_sum[w] = acc;
        sh_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh_sum[0];
        int k = sh_cnt[0];
        for (int i = 1; i < kSeqWaves; ++i) {
            t += sh_sum[i];
            k += sh_cnt[i];
        }
        a.score[r] = t;
        a.count[r] = k;
    }
}

struct PickArgs {
    const double* score;
    const float* yp;
    long yp_cs, yp_ss, yp_fs;
    const int32_t* lens;
    const int32_t* tokens;
    long tok_rs;
    int S, L, W, n;
    int32_t* win;
    uint8_t* ok;
    float* best;
    int32_t* best_tokens;
};

__global__ __launch_bounds__(kPickThreads) void score_pick_kernel(PickArgs a) {
    __shared__ int sh_win, sh_ok;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) {
        const double inf = __builtin_inf();
        double cur = -inf;
        int w = 0, fin = 0;
        for (int s = 0; s < a.S; ++s) {
            double d = a.score[(size_t)j * a.S + s];
            if (d != d) d = -inf;
            if (d > -inf && d < inf) fin = 1;
            if (d > cur) {
                cur = d;
                w = s;
            }
        }
        a.win[j] = w;
        a.ok[j] = (uint8_t)fin;
        sh_win = w;
        sh_ok = fin;
    }
    __syncthreads();
    if (a.best) {
        int n = 0;
        if (sh_ok) {
            n = a.lens[j];
            n = n < 0 ? 0 : (n > a.L ? a.L : n);
        }
        gather_winner_rows<kPickThreads>(a.yp + (size_t)j * a.yp_cs + (size_t)sh_win * a.yp_ss, a.yp_fs,
                                         a.best + (size_t)j * a.L * a.W, a.L, a.W, n);
    }
    if (a.best_tokens) {
        const int32_t* src = a.tokens + ((size_t)j * a.S + sh_win) * a.tok_rs;
        int32_t* dst = a.best_tokens + (size_t)j * a.n;
        for (int c = threadIdx.x; c < a.n; c += kPickThreads) dst[c] = sh_ok ? src[c] : -100;
    }
}

}  // namespace
}  // namespace dimx

using namespace dimx;

int dimx_op_seq_logprob(const float* logits, long row_stride, long step_stride, const int32_t* tokens, long tok_row_stride,
                        const int32_t* first, const int32_t* last, int rows_per_clip, int R, int n, double* tok_logprob, double* score,
                        int32_t* count, void* stream) {
    DIMX_REQUIRE(logits && tokens && score && count, DIMX_ERR_ARG, "seq_logprob: null operand");
    DIMX_REQUIRE(R >= 0 && n >= 1 && rows_per_clip >= 1, DIMX_ERR_ARG, "seq_logprob: R=%d n=%d rows_per_clip=%d out of range", R, n,
                 rows_per_clip);
    DIMX_REQUIRE(R % rows_per_clip == 0, DIMX_ERR_ARG, "seq_logprob: R=%d is not a multiple of rows_per_clip=%d", R, rows_per_clip);
    DIMX_REQUIRE(step_stride >= kVocab, DIMX_ERR_ARG, "seq_logprob: step stride %ld below the %d entries of a column", step_stride, kVocab);
    DIMX_REQUIRE(row_stride >= 0 && tok_row_stride >= 0, DIMX_ERR_ARG, "seq_logprob: negative stride");
    if (R == 0) return DIMX_OK;
    SeqArgs a;
    a.logits = logits, a.row_stride = row_stride, a.step_stride = step_stride;
    a.tokens = tokens, a.tok_rs = tok_row_stride;
    a.first = first, a.last = last, a.rpc = rows_per_clip, a.n = n;
    a.tok_lp = tok_logprob, a.score = score, a.count = count;
    hipLaunchKernelGGL(seq_logprob_kernel, dim3(R), dim3(kSeqThreads), 0, (hipStream_t)stream, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int dimx_op_score_select(const double* score, const float* y_pred, long yp_clip_stride, long yp_sample_stride, long yp_frame_stride,
                         const int32_t* lens, const int32_t* tokens, long tok_row_stride, int B, int S, int L, int W, int n,
                         int32_t* win, uint8_t* ok, float* best, int32_t* best_tokens, void* stream) {
    DIMX_REQUIRE(score && win && ok, DIMX_ERR_ARG, "score_select: null operand");
    DIMX_REQUIRE(B >= 1 && S >= 1, DIMX_ERR_ARG, "score_select: B=%d S=%d must be positive", B, S);
    DIMX_REQUIRE(!best || (y_pred && lens && L >= 1 && W >= 1), DIMX_ERR_ARG,
                 "score_select: best needs y_pred, lens and L=%d, W=%d positive", L, W);
    DIMX_REQUIRE(!best_tokens || (tokens && n >= 1), DIMX_ERR_ARG, "score_select: best_tokens needs tokens and n=%d positive", n);
    DIMX_REQUIRE(yp_clip_stride >= 0 && yp_sample_stride >= 0 && yp_frame_stride >= 0 && tok_row_stride >= 0, DIMX_ERR_ARG,
                 "score_select: negative stride");
    PickArgs a;
    a.score = score, a.yp = y_pred, a.yp_cs = yp_clip_stride, a.yp_ss = yp_sample_stride, a.yp_fs = yp_frame_stride;
    a.lens = lens, a.tokens = tokens, a.tok_rs = tok_row_stride;
    a.S = S, a.L = L, a.W = W, a.n = n;
    a.win = win, a.ok = ok, a.best = best, a.best_tokens = best_tokens;
    hipLaunchKernelGGL(score_pick_kernel, dim3(B), dim3(kPickThreads), 0, (hipStream_t)stream, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
