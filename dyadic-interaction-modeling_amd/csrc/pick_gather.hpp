// pick_gather.hpp -- the gather half of a best-of-S pick, shared by fd_pick_kernel (fd_select.hip) and score_pick_kernel
// (seq_score.hip): the winning try's rows [L, W] f32 out of y_pred [B, S, L, W], zero for t >= n.
#pragma once
#include "common.hpp"

namespace dimx {

// src = the winner's first frame (frames fs elements apart, feature stride 1), dst = the clip's dense [L, W] rows; the whole
// block takes part, THREADS = its size.  Frames t >= n are never read.
template <int THREADS>
__device__ __forceinline__ void gather_winner_rows(const float* src, long fs, float* dst, int L, int W, int n) {
    const int total = L * W;
    for (int e = threadIdx.x; e < total; e += THREADS) {
        const int t = e / W, c = e - t * W;
        dst[e] = t < n ? src[(size_t)t * fs + c] : 0.f;
    }
}

}  // namespace dimx
