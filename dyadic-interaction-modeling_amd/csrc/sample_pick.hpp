// sample_pick.hpp -- the arithmetic of the top-k sampler as device functions: one wave per row of 512 logits, element lane + 64 c
// in slot c of a lane.  In a header because two kernels run it: sample_kernel (elementwise.hip, which has the full description)
// and the sampling head of the first decoder layer's launch (chain.hip, xcd_layer_kernel HEAD).  One body, so the two routes
// share the lane <-> element map, the reductions and the noise addressing: the same token from the same logits.
#pragma once
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kSampleVocab = 512;   // rows of the logits / embedding table the sampler is written for (8 x 64 lanes)

__device__ __forceinline__ uint32_t f32_order_key(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t splitmix(uint64_t key, uint64_t ctr) {
    uint64_t z = key + (ctr + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the row's logits, split-K slabs added in slab order, and the lane's running maximum (first index wins a tie)
__device__ __forceinline__ void sample_load_row(const float* __restrict__ lr, int nslab, long slab_stride, int lane, float (&v)[8],
                                                float& mx, int& mi) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = lr[lane + 64 * c];
        for (int sidx = 1; sidx < nslab; ++sidx) v[c] += lr[(size_t)sidx * slab_stride + lane + 64 * c];  // split-K slabs
        if (v[c] > mx) {
            mx = v[c];
            mi = lane + 64 * c;
        }
    }
}

// the k-th largest key: a 32-step bitwise search on the order-preserving integer image of the floats, counting with ballots
// (0 = keep everything: top_k outside 1 .. 511)
__device__ __forceinline__ uint32_t sample_topk_threshold(const uint32_t (&key)[8], int top_k) {
    uint32_t thr = 0;
    if (top_k > 0 && top_k < 512) {
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = thr | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) cnt += __popcll(__ballot(key[c] >= cand));
            if (cnt >= top_k) {
                thr = cand;
                // exactly k keys at or above the candidate: that IS the top-k set (every key >= its minimum is
                // already counted), the remaining bits could only tighten the threshold onto that minimum
                if (cnt == top_k) break;
            }
        }
    }
    return thr;
}

// where a row's noise comes from: the injected tensor [steps, rows_total, 512], or the counter-based generator keyed by
// (step, GLOBAL sequence row, code)
struct SampleNoise {
    const float* noise;
    uint64_t seed, step;
    int rows_total, row0, row, rng_tot, rng_off;
};

// softmax(T) over the survivors (key >= thr), divided by the noise, arg-max.  Only the <= top_k (+ ties) survivors need a
// probability and a noise draw: they are compacted to one per lane through cv / ci (128 entries each, this wave's own; 2 rounds
// cover up to 128 survivors; more than that -- massive ties -- falls back to the per-element loop).
__device__ __forceinline__ int sample_survivor(const float (&v)[8], const uint32_t (&key)[8], uint32_t thr, float mx, float temperature,
                                               const SampleNoise& nz, float* cv, int* ci, int lane) {
    const float inv_t = 1.0f / temperature;
    int nsurv_lane = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) nsurv_lane += key[c] >= thr ? 1 : 0;
    int incl = nsurv_lane;  // inclusive prefix over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const int total = __shfl(incl, 63);
    float best = -1.f;
    int bi = 0x7fffffff;
    auto score = [&](float pv, float zs, int i) {
        float q;
        if (nz.noise) {
            q = nz.noise[((size_t)nz.step * nz.rows_total + nz.row0 + nz.row) * 512 + i];
        } else {
            const uint64_t r = splitmix(nz.seed, ((uint64_t)nz.step * nz.rng_tot + nz.rng_off + nz.row0 + nz.row) * 512 + i);
            const float u = (float)(r >> 40) * (1.0f / 16777216.0f);
            q = fmaxf(-log1pf(-u), 9.313225746154785e-10f);
        }
        const float sc = (pv / zs) / q;
        if (sc > best || (sc == best && i < bi)) {
            best = sc;
            bi = i;
        }
    };
    if (total <= 128) {
        int pos = incl - nsurv_lane;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (key[c] >= thr) {
                cv[pos] = v[c];
                ci[pos] = lane + 64 * c;
                ++pos;
            }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float pv[2] = {0.f, 0.f};
        int pi[2] = {0, 0};
        float zsum = 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int k = lane + 64 * r;
            if (k < total) {
                pv[r] = expf((cv[k] - mx) * inv_t);
                pi[r] = ci[k];
                zsum += pv[r];
            }
        }
        zsum = wave_sum(zsum);
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (lane + 64 * r < total) score(pv[r], zsum, pi[r]);
    } else {
        float p[8];
        float zsum = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            p[c] = key[c] >= thr ? expf((v[c] - mx) * inv_t) : 0.f;
            zsum += p[c];
        }
        zsum = wave_sum(zsum);
#pragma unroll
        for (int c = 0; c < 8; ++c) score(p[c], zsum, lane + 64 * c);
    }
    wave_argmax(best, bi);
    return bi;
}

// What the sampling head of the first layer's launch does for row `row` (SampleHeadArgs, common.hpp): sample_kernel's top-k route
// at step `step` -- the logits' slab sum, the optional dump, arg-max, threshold, survivors -- then the token column and the next
// position of the token history.  temperature / seed / row window come from the call's parameter block, as in sample_kernel.
__device__ __forceinline__ int sample_head_row(const SampleHeadArgs& hd, int row, int step, float* cv, int* ci, int lane) {
    const int32_t* dp = hd.params + 2;
    const float temperature = __builtin_bit_cast(float, dp[0]);
    const uint64_t seed = *(const uint64_t*)(dp + 2);
    const int rng_off = dp[4];
    const int rng_tot = dp[5] > 0 ? dp[5] : hd.rows_total;
    float v[8];
    float mx = -3.0e38f;
    int mi = 0;
    sample_load_row(hd.logits + (size_t)row * hd.ld_logits, hd.nslab, hd.slab_stride, lane, v, mx, mi);
    if (hd.logits_out) {
        float* lo = hd.logits_out + ((size_t)row * hd.logits_out_ld + step) * 512;
#pragma unroll
        for (int c = 0; c < 8; ++c) lo[lane + 64 * c] = v[c];
    }
    wave_argmax(mx, mi);
    const bool greedy = temperature <= 0.f || (hd.noise == nullptr && seed == 0);
    int tok = mi;
    if (!greedy) {
        uint32_t key[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) key[c] = f32_order_key(v[c]);
        const uint32_t thr = sample_topk_threshold(key, hd.top_k);
        const SampleNoise nz = {hd.noise, seed, (uint64_t)step, hd.rows_total, hd.row0, row, rng_tot, rng_off};
        tok = sample_survivor(v, key, thr, mx, temperature, nz, cv, ci, lane);
    }
    if (lane == 0) {
        hd.tokens[(size_t)row * hd.tok_ld + step] = tok;
        if (step + 1 < hd.hist_ld) hd.hist[(size_t)row * hd.hist_ld + step + 1] = tok < 0 ? 0 : (tok >= kSampleVocab ? kSampleVocab - 1 : tok);
    }
    return tok;
}

}  // namespace
}  // namespace dimx
