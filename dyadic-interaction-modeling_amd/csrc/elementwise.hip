// elementwise.hip -- the small HBM-bound kernels that glue the dense stages together: input cast/pad,
// embedding gathers, context assembly, token bookkeeping, cross-entropy/argmax over the 512-entry
// vocabulary and the top-k / softmax / noise-argmax sampler of the autoregressive loop.
#include "common.hpp"
#include "sample_pick.hpp"

namespace dimx {
namespace {

// y[m, 0:ldy) = x[m, 0:K) (+ coladd) zero-padded; x is f32 [M, ldx]
template <typename OutT>
__global__ void cast_pad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ coladd,
                                OutT* __restrict__ y, int ldy, int M, int K, const uint8_t* __restrict__ zero_rows) {
    const long total = (long)M * ldy;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / ldy), k = (int)(i - (long)m * ldy);
        float v = 0.f;
        if (k < K && !(zero_rows && zero_rows[m])) {  // zero_rows: SLM's masked frames (seq2seq_pretrain.py:211-212)
            v = x[(size_t)m * ldx + k];
            if (coladd) v += coladd[k];
        }
        store_from_f32<OutT>(y + i, v);
    }
}

// y[m, :] = table[idx[m], :]   (codebook lookup = the one-hot matmul of
// code/seq2seq_pretrain.py:457-459; token embedding of the teacher-forced decoder)
template <typename OutT>
__global__ void gather_rows_kernel(const float* __restrict__ table, int ld_table, int rows,
                                   const int32_t* __restrict__ idx, OutT* __restrict__ y, int ldy, int M, int C) {
    const long total = (long)M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / C), c = (int)(i - (long)m * C);
        int r = idx[m];
        r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
        store_from_f32<OutT>(y + (size_t)m * ldy + c, table[(size_t)r * ld_table + c]);
    }
}

// ctx[m] = cat(x_s[m] + patch_embed_dec_s, audio[m])   (code/seq2seq_pretrain.py:445-446)
template <typename OutT>
__global__ void context_concat_kernel(const float* __restrict__ x_s, const float* __restrict__ patch,
                                      const float* __restrict__ audio, OutT* __restrict__ ctx, int M, int dim,
                                      int dim_a) {
    const int W = dim + dim_a;
    const long total = (long)M * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / W), c = (int)(i - (long)m * W);
        const float v = c < dim ? x_s[(size_t)m * dim + c] + patch[c] : audio[(size_t)m * dim_a + (c - dim)];
        store_from_f32<OutT>(ctx + i, v);
    }
}

// fqn codes per frame (1 for the listener / SLMFT VQ-VAEs, 8 for the legacy speaker VQ-VAE)
__global__ void finalize_idx_kernel(int32_t* idx, const int32_t* lens, int B, int T, int fqn, int32_t pad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T * fqn) return;
    const int b = i / (T * fqn), t = (i - b * T * fqn) / fqn;
    if (lens && t >= lens[b]) idx[i] = pad;
}

// AutoregressiveWrapper.forward: inp = z[:, :-1] with ignore_index -> pad_value 0, target = z[:, 1:]
__global__ void shift_tokens_kernel(const int32_t* z, int32_t* inp, int32_t* tgt, int B, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = T - 1;
    if (i >= B * n) return;
    const int b = i / n, t = i - b * n;
    const int32_t v = z[b * T + t];
    inp[i] = v == -100 ? 0 : v;
    tgt[i] = z[b * T + t + 1];
}

// one wave per row of V = 512 logits: cross entropy against target (0 where target < 0) and argmax
__global__ __launch_bounds__(256) void ce_argmax_kernel(const float* __restrict__ logits,
                                                        const int32_t* __restrict__ target,
                                                        float* __restrict__ row_loss,
                                                        int32_t* __restrict__ argmax_tok, int R) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const float* lr = logits + (size_t)row * 512;
    float v[8];
    float mx = -3.0e38f;
    int mi = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = lr[lane + 64 * c];
        if (v[c] > mx) {
            mx = v[c];
            mi = lane + 64 * c;
        }
    }
    wave_argmax(mx, mi);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) se += expf(v[c] - mx);
    se = wave_sum(se);
    if (lane == 0) {
        if (argmax_tok) argmax_tok[row] = mi;
        if (row_loss) {
            const int t = target ? target[row] : -100;
            row_loss[row] = (t >= 0 && t < 512) ? (mx + logf(se)) - lr[t] : 0.f;
        }
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    uint32_t o;
    o = (uint32_t)xor_lane_i32<32>((int)v); v = o < v ? o : v;
    o = (uint32_t)xor_lane_i32<16>((int)v); v = o < v ? o : v;
    o = (uint32_t)xor_lane_i32<8>((int)v);  v = o < v ? o : v;
    o = (uint32_t)xor_lane_i32<4>((int)v);  v = o < v ? o : v;
    o = (uint32_t)xor_lane_i32<2>((int)v);  v = o < v ? o : v;
    o = (uint32_t)xor_lane_i32<1>((int)v);  v = o < v ? o : v;
    return v;
}

// Sampler of AutoregressiveWrapper.generate: top-k filter (k = 52), softmax(T), multinomial.
// torch.multinomial(p, 1) == argmax(p / q), q ~ Exp(1) (tests/golden/sampler_multinomial.npz), so the
// noise is an input: injected (parity) or drawn from a counter-based splitmix64 stream (production).
// One wave per row; the k-th largest logit is found by a 32-step bitwise search on the order-preserving
// integer image of the floats, counting with ballots.
//
// KIND selects the filter (DIMX_FILTER_*).  KIND 0 is the top-k search above, untouched.  The other three kept sets are
// thresholds on the same integer keys, so they only replace the search and hand `thr` to the same survivor code:
//   top_p  keep i iff mass(l_j > l_i) <= thres * Z: the smallest key c* with mass(key > c*) <= thres * Z, found by the same
//          32-step bitwise search with a masked wave sum for the ballots.  The masked sum always adds the same 512 slots in the
//          same order (zeros for the excluded ones), so it is non-increasing in c in float32 too and the search is exact for it.
//   min_p  keep i iff e_i >= min_p, e_i = exp(l_i - max) (e_max = 1, no partition sum)
//   top_a  keep i iff e_i >= ratio * Z^(1 - pow)
// thres >= 1 and min_p <= 0 keep everything; the arg-max is always kept.  fa / fb come from the parameter block (words
// 9 / 10 behind dev_params) when there is one: the captured step graph does not depend on them.
//
// GUIDED (sample_guided_kernel, classifier-free guidance; the definition is dimx/guidance.py): the row sampled is
// g = c + (s - 1) * (c - u) in f32, three roundings and that of s - 1, c = row `row` of `logits` and u = row `row` of `logits_u`,
// each summed over its slabs in the order above.  Everything after that -- filter, temperature, noise, arg-max, forced token --
// is the code of the plain sampler on g, with the noise row and the generator counter of row `row` of an R-row launch.  What the
// plain sampler writes for its row is written twice, for row `row` and for row `row + R` (the unconditional half of a 2R-row
// step); tokens_u [R, tok_ld] takes the second copy of the token (optional).  s is word 11 of the parameter block when there is one.
// logits_out takes g; branch_out [2, R, logits_out_ld, 512] takes c and u (optional).
template <int KIND, bool GUIDED>
__device__ __forceinline__ void sample_body(const float* __restrict__ logits, int ld, int R, int top_k,
                                            float temperature, const float* __restrict__ noise,
                                            uint64_t seed, const int32_t* __restrict__ step_dev,
                                            uint64_t step_host, int32_t* __restrict__ tokens, int tok_ld,
                                            int tok_col_from_step, int nslab, long slab_stride,
                                            float* __restrict__ logits_out, int logits_out_ld, int row0,
                                            int rows_total,
                                            const float* __restrict__ emb_table, int emb_C,
                                            float* __restrict__ x_next, int32_t* __restrict__ step_rw,
                                            unsigned* __restrict__ done_ctr,
                                            const float* __restrict__ pos_table, float pos_scale,
                                            int pos_rows, const int32_t* __restrict__ dev_params,
                                            void* __restrict__ y_next, const float* __restrict__ y_gamma,
                                            int y_bf16, const float* __restrict__ qkv0_table,
                                            float* __restrict__ qkv0_out, int qkv0_N,
                                            const int32_t* __restrict__ prompt, int prompt_ld, int prompt_max,
                                            const int32_t* __restrict__ prompt_len, int prompt_div,
                                            int32_t* __restrict__ epoch_rw, float fa, float fb,
                                            uint8_t* __restrict__ keep_out, int32_t* __restrict__ hist, int hist_ld,
                                            const float* __restrict__ logits_u, float scale,
                                            float* __restrict__ branch_out, int32_t* __restrict__ tokens_u) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t step = step_dev ? (uint64_t)*step_dev : step_host;
    if (dev_params) {  // generate(): temperature / seed live in device memory so that the captured step graph
                       // does not depend on them (a new seed per batch must not force a re-capture)
        temperature = __builtin_bit_cast(float, dev_params[0]);
        seed = *(const uint64_t*)(dev_params + 2);
        if constexpr (KIND != DIMX_FILTER_TOP_K) {
            fa = __builtin_bit_cast(float, dev_params[9]);
            fb = __builtin_bit_cast(float, dev_params[10]);
        }
    }
    // counter of the on-device generator: (step, GLOBAL sequence row, code) -- a rank that generates rows
    // [off, off + R) of a sharded batch of `tot` sequences draws what the single-process batch would draw
    const int rng_off = dev_params ? dev_params[4] : 0;
    const int rng_tot = dev_params && dev_params[5] > 0 ? dev_params[5] : rows_total;
    if (row < R) {
    const float* lr = logits + (size_t)row * ld;
    // the fused pre-norm's weight does not depend on the token: its loads go out with the logits' (behind the token's embedding
    // row they were one more exposed L2 round trip at the tail of every decode step)
    float2 gam[16];
    const bool fast_embed = x_next && emb_C / 2 <= 16 * 64;
    if (y_next && fast_embed) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = lane + 64 * k;
            gam[k] = ((const float2*)y_gamma)[i < emb_C / 2 ? i : emb_C / 2 - 1];
        }
    }
    float v[8];
    float mx = -3.0e38f;
    int mi = 0;
    if constexpr (!GUIDED) {
        sample_load_row(lr, nslab, slab_stride, lane, v, mx, mi);
    } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = lr[lane + 64 * c];
        for (int sidx = 1; sidx < nslab; ++sidx) v[c] += lr[(size_t)sidx * slab_stride + lane + 64 * c];  // split-K slabs
        if constexpr (GUIDED) {
            const float* ur = logits_u + (size_t)row * ld;
            float u = ur[lane + 64 * c];
            for (int sidx = 1; sidx < nslab; ++sidx) u += ur[(size_t)sidx * slab_stride + lane + 64 * c];
            if (branch_out) {   // both raw rows: [2, R, steps, 512]
                const size_t at = ((size_t)row * logits_out_ld + (tok_col_from_step ? step : 0)) * 512 + lane + 64 * c;
                branch_out[at] = v[c];
                branch_out[(size_t)R * logits_out_ld * 512 + at] = u;
            }
            // s - 1 == 0 returns c itself (no c + 0 * inf, no -0 + 0); otherwise three separate roundings, never an fma
            const float sm1 = __fsub_rn(dev_params ? __builtin_bit_cast(float, dev_params[11]) : scale, 1.0f);
            if (sm1 != 0.f) v[c] = __fadd_rn(v[c], __fmul_rn(sm1, __fsub_rn(v[c], u)));
        }
        if (v[c] > mx) {
            mx = v[c];
            mi = lane + 64 * c;
        }
    }
    }
    if (logits_out) {  // per-step dump of the raw logits: [rows, steps, 512]
        float* lo = logits_out + ((size_t)row * logits_out_ld + (GUIDED && !tok_col_from_step ? 0 : step)) * 512;
#pragma unroll
        for (int c = 0; c < 8; ++c) lo[lane + 64 * c] = v[c];
    }
    // Prompted generation (dimx_generate_prompted): while the next position still lies inside this clip's prompt the row
    // takes the prompt's token instead of a sampled one -- before the token, the embedding row, the pre-norm and the q/k/v
    // table row below are written.  plen = clamp(prompt_len, P0, Pmax), P0 - 1 = dev_params[8] (word 10 of the parameter block: the call's first step).
    // One wave per row: the branch is wave-uniform, and a forced row skips the arg-max, top-k, softmax and noise work.
    bool forced = false;
    int tok = 0;
    if (prompt) {
        const int clip = row / prompt_div;
        int plen = prompt_len ? prompt_len[clip] : prompt_max;
        const int p0 = dev_params ? dev_params[8] + 1 : 1;
        plen = plen < p0 ? p0 : (plen > prompt_max ? prompt_max : plen);
        if ((int)step + 1 < plen) {
            forced = true;
            tok = prompt[(size_t)clip * prompt_ld + step + 1];
            tok = tok < 0 ? 0 : (tok >= kSampleVocab ? kSampleVocab - 1 : tok);   // the clamp of embed_step_kernel
        }
    }
    if (!forced) {
    wave_argmax(mx, mi);
    const bool greedy = temperature <= 0.f || (noise == nullptr && seed == 0);
    tok = mi;
    if (!greedy || keep_out) {
        uint32_t key[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) key[c] = f32_order_key(KIND == DIMX_FILTER_TOP_K ? v[c] : v[c] + 0.f);   // + 0: -0 ties with +0
        uint32_t thr = 0;
        if constexpr (KIND != DIMX_FILTER_TOP_K) {
            float e[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) e[c] = expf(v[c] - mx);
            // mass of the keys above cnd: slot c of lane l always enters at the same place of the same sum
            auto mass_above = [&](uint32_t cnd) {
                float m = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) m += key[c] > cnd ? e[c] : 0.f;
                return wave_sum(m);
            };
            if constexpr (KIND == DIMX_FILTER_TOP_P) {
                if (fa < 1.0f) {
                    const float lim = fa * mass_above(0u);   // no finite float has key 0: this is Z
                    uint32_t lo = 0;                         // the largest c whose mass above still exceeds the limit
                    for (int bit = 31; bit >= 0; --bit) {
                        const uint32_t cand = lo | (1u << bit);
                        if (mass_above(cand) > lim) lo = cand;
                    }
                    thr = lo + 1u;   // mass above the largest key is 0 <= lim, so lo < 2^32 - 1
                }
            } else {
                float lim = fa;
                if constexpr (KIND == DIMX_FILTER_TOP_A) lim = fb * powf(mass_above(0u), 1.0f - fa);
                uint32_t kmin = f32_order_key(mx + 0.f);   // the arg-max stays, whatever the limit
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (e[c] >= lim && key[c] < kmin) kmin = key[c];
                thr = wave_min_u32(kmin);
            }
        } else {
            thr = sample_topk_threshold(key, top_k);
        }
        if (keep_out) {   // dimx_op_sample_filtered: the kept set as this launch decided it
#pragma unroll
            for (int c = 0; c < 8; ++c) keep_out[(size_t)row * 512 + lane + 64 * c] = key[c] >= thr ? 1 : 0;
        }
        if (!greedy) {
            __shared__ float cand_v[4][128];
            __shared__ int cand_i[4][128];
            const SampleNoise nz = {noise, seed, step, rows_total, row0, row, rng_tot, rng_off};
            tok = sample_survivor(v, key, thr, mx, temperature, nz, cand_v[threadIdx.x >> 6], cand_i[threadIdx.x >> 6], lane);
        }  // !greedy
    }
    }  // !forced
    if (lane == 0) tokens[(size_t)row * tok_ld + (tok_col_from_step ? (int)step : 0)] = tok;
    if constexpr (GUIDED)
        if (tokens_u && lane == 0) tokens_u[(size_t)row * tok_ld + (tok_col_from_step ? (int)step : 0)] = tok;
    // the first layer's token history (its self attention in the table form, decode_attn_body.hpp): the next position's input
    if (hist && lane == 0 && (int)step + 1 < hist_ld)
        hist[(size_t)row * hist_ld + step + 1] = tok < 0 ? 0 : (tok >= kSampleVocab ? kSampleVocab - 1 : tok);
    if constexpr (GUIDED)
        if (hist && lane == 0 && (int)step + 1 < hist_ld)
            hist[(size_t)(row + R) * hist_ld + step + 1] = tok < 0 ? 0 : (tok >= kSampleVocab ? kSampleVocab - 1 : tok);
    if (x_next) {  // next step's decoder input: token embedding row (fused embed_step)
        // Non-finite logits (a chain fault's garbage, before the call that suffered it regenerates the batch) leave no survivor to win
        // the arg-max and tok = 0x7fffffff: the token column keeps it, but no table is addressed with it
        const int tk = tok < 0 ? 0 : (tok >= kSampleVocab ? kSampleVocab - 1 : tok);
        const float2* src = (const float2*)(emb_table + (size_t)tk * emb_C);
        float2* dst = (float2*)(x_next + (size_t)row * emb_C);
        const bool with_pos = pos_table && (int)step + 1 < pos_rows;   // legacy decoder: + pos_emb[next position] * dim^-0.5
        const float2* pr = with_pos ? (const float2*)(pos_table + (size_t)(step + 1) * emb_C) : nullptr;
        // all of the row's loads in flight together, then the stores (a plain copy loop keeps load -> store order: up to
        // 9 dependent L2 round trips at the tail of every decode step)
        const int nv = emb_C / 2;
        if (nv <= 16 * 64) {
            float2 v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = lane + 64 * k;
                v[k] = src[i < nv ? i : nv - 1];
            }
            if (qkv0_table) {
                // the first layer's q/k/v of this token is a row of a table (no positional term in this decoder: the layer's
                // input depends on the token alone).  Its loads go out with the embedding row's, behind the same dependent
                // hop on the token, and land in slab 0 of the step's q/k/v buffer (the launcher checks qkv0_N <= 12 * 256).
                const float4* qs = (const float4*)(qkv0_table + (size_t)tk * qkv0_N);
                float4* qd = (float4*)(qkv0_out + (size_t)row * qkv0_N);
                const int nq = qkv0_N / 4;
                float4 w[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const int i = lane + 64 * k;
                    w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (i < nq) w[k] = qs[i];
                }
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const int i = lane + 64 * k;
                    if (i < nq) qd[i] = w[k];
                }
                if constexpr (GUIDED) {
                    float4* qd2 = (float4*)(qkv0_out + (size_t)(row + R) * qkv0_N);
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        const int i = lane + 64 * k;
                        if (i < nq) qd2[i] = w[k];
                    }
                }
            }
            if (with_pos) {
                float2 q[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = lane + 64 * k;
                    q[k] = pr[i < nv ? i : nv - 1];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    v[k] = make_float2(__fadd_rn(v[k].x, __fmul_rn(q[k].x, pos_scale)), __fadd_rn(v[k].y, __fmul_rn(q[k].y, pos_scale)));
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = lane + 64 * k;
                if (i < nv) dst[i] = v[k];
            }
            if constexpr (GUIDED) {
                float2* dst2 = (float2*)(x_next + (size_t)(row + R) * emb_C);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = lane + 64 * k;
                    if (i < nv) dst2[i] = v[k];
                }
            }
            if (y_next) {
                // round 4: the first decoder layer's pre-norm of this row rides along (y = LayerNorm(x) * gamma, no bias) -- one
                // launch less per decode step.  Same lane <-> element map, summation order and wave reductions as
                // add_slabs_layernorm_kernel (norm.hip), so the f32 parity mode's bits do not change.
                float sm = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (lane + 64 * k < nv) sm += v[k].x + v[k].y;
                const float inv_c = 1.0f / (float)emb_C;
                const float mean = (y_bf16 ? wave_sum_sel<true>(sm) : wave_sum_sel<false>(sm)) * inv_c;
                float qs = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (lane + 64 * k < nv) {
                        const float a0 = v[k].x - mean, b0 = v[k].y - mean;
                        qs += a0 * a0 + b0 * b0;
                    }
                const float rstd = rsqrtf((y_bf16 ? wave_sum_sel<true>(qs) : wave_sum_sel<false>(qs)) * inv_c + 1e-5f);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = lane + 64 * k;
                    if (i < nv) {
                        const float2 g = gam[k];
                        const float o0 = (v[k].x - mean) * rstd * g.x, o1 = (v[k].y - mean) * rstd * g.y;
                        if (y_bf16)
                            *(uint32_t*)((bf16*)y_next + (size_t)row * emb_C + 2 * i) = pack_bf16x2(o0, o1);
                        else
                            *(float2*)((float*)y_next + (size_t)row * emb_C + 2 * i) = make_float2(o0, o1);
                        if constexpr (GUIDED) {
                            if (y_bf16)
                                *(uint32_t*)((bf16*)y_next + (size_t)(row + R) * emb_C + 2 * i) = pack_bf16x2(o0, o1);
                            else
                                *(float2*)((float*)y_next + (size_t)(row + R) * emb_C + 2 * i) = make_float2(o0, o1);
                        }
                    }
                }
            }
        } else {
            for (int i = lane; i < nv; i += 64) {
                float2 e = src[i];
                if (with_pos) {
                    const float2 q = pr[i];
                    e = make_float2(__fadd_rn(e.x, __fmul_rn(q.x, pos_scale)), __fadd_rn(e.y, __fmul_rn(q.y, pos_scale)));
                }
                dst[i] = e;
                if constexpr (GUIDED) ((float2*)(x_next + (size_t)(row + R) * emb_C))[i] = e;
            }
        }
    }
    }  // row < R
    // the block that finishes last advances the device step counter (every block has read it by then)
    if (step_rw) {
        __syncthreads();
        if (threadIdx.x == 0) {  // no fence needed: only the READ of the step counter must precede the arrival
            const unsigned prev = atomicAdd(done_ctr, 1u);
            if (prev == gridDim.x - 1) {
                *done_ctr = 0u;
                *step_rw = (int32_t)step + 1;
                if (epoch_rw) *epoch_rw += 1;   // steps done in this call: the chain kernels' counter epoch
            }
        }
    }
}

#define DIMX_SAMPLE_PARAMS                                                                                                             \
    const float *__restrict__ logits, int ld, int R, int top_k, float temperature, const float *__restrict__ noise, uint64_t seed,     \
        const int32_t *__restrict__ step_dev, uint64_t step_host, int32_t *__restrict__ tokens, int tok_ld, int tok_col_from_step,     \
        int nslab, long slab_stride, float *__restrict__ logits_out, int logits_out_ld, int row0, int rows_total,                      \
        const float *__restrict__ emb_table, int emb_C, float *__restrict__ x_next, int32_t *__restrict__ step_rw,                     \
        unsigned *__restrict__ done_ctr, const float *__restrict__ pos_table, float pos_scale, int pos_rows,                           \
        const int32_t *__restrict__ dev_params, void *__restrict__ y_next, const float *__restrict__ y_gamma, int y_bf16,              \
        const float *__restrict__ qkv0_table, float *__restrict__ qkv0_out, int qkv0_N, const int32_t *__restrict__ prompt,            \
        int prompt_ld, int prompt_max, const int32_t *__restrict__ prompt_len, int prompt_div, int32_t *__restrict__ epoch_rw,         \
        float fa, float fb, uint8_t *__restrict__ keep_out, int32_t *__restrict__ hist, int hist_ld
#define DIMX_SAMPLE_ARGS                                                                                                               \
    logits, ld, R, top_k, temperature, noise, seed, step_dev, step_host, tokens, tok_ld, tok_col_from_step, nslab, slab_stride,        \
        logits_out, logits_out_ld, row0, rows_total, emb_table, emb_C, x_next, step_rw, done_ctr, pos_table, pos_scale, pos_rows,      \
        dev_params, y_next, y_gamma, y_bf16, qkv0_table, qkv0_out, qkv0_N, prompt, prompt_ld, prompt_max, prompt_len, prompt_div,      \
        epoch_rw, fa, fb, keep_out, hist, hist_ld

template <int KIND>
__global__ __launch_bounds__(256) void sample_kernel(DIMX_SAMPLE_PARAMS) {
    sample_body<KIND, false>(DIMX_SAMPLE_ARGS, nullptr, 1.0f, nullptr, nullptr);
}

// the guided sampler: one wave per CLIP, rows b (conditional) and b + R (unconditional) of a 2R-row decode step
template <int KIND>
__global__ __launch_bounds__(256) void sample_guided_kernel(DIMX_SAMPLE_PARAMS, const float* __restrict__ logits_u, float scale,
                                                            float* __restrict__ branch_out, int32_t* __restrict__ tokens_u) {
    sample_body<KIND, true>(DIMX_SAMPLE_ARGS, logits_u, scale, branch_out, tokens_u);
}

// x[b, :] = token_emb[tok_b], tok_b = start[b] (row stride start_ld) at the call's first step (start_step: 0, or P0 - 1 of a
// prompted generation) else the token sampled at the previous step
__global__ __launch_bounds__(256) void embed_step_kernel(const float* __restrict__ table, int C,
                                                         const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ tokens, int tok_ld,
                                                         const int32_t* __restrict__ step_dev, float* __restrict__ x,
                                                         int rows, int start_div,
                                                         const float* __restrict__ pos_table, float pos_scale, int start_ld,
                                                         int start_step) {
    const int b = blockIdx.x;
    const int step = *step_dev;
    int tok = step == start_step ? start[(size_t)(b / start_div) * start_ld] : tokens[(size_t)b * tok_ld + step - 1];
    tok = tok < 0 ? 0 : (tok >= rows ? rows - 1 : tok);
    const float4* src = (const float4*)(table + (size_t)tok * C);
    float4* dst = (float4*)(x + (size_t)b * C);
    if (pos_table) {
        const float4* pr = (const float4*)(pos_table + (size_t)step * C);
        for (int i = threadIdx.x; i < C / 4; i += blockDim.x) {
            const float4 e = src[i], q = pr[i];
            dst[i] = make_float4(__fadd_rn(e.x, __fmul_rn(q.x, pos_scale)), __fadd_rn(e.y, __fmul_rn(q.y, pos_scale)),
                                 __fadd_rn(e.z, __fmul_rn(q.z, pos_scale)), __fadd_rn(e.w, __fmul_rn(q.w, pos_scale)));
        }
    } else {
        for (int i = threadIdx.x; i < C / 4; i += blockDim.x) dst[i] = src[i];
    }
}

// ids[i] = min(i, rows - 1): the token ids of the q/k/v table's build rounds (the last round repeats the last id)
__global__ void iota_clamp_kernel(int32_t* __restrict__ ids, int n, int rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = i < rows ? i : rows - 1;
}

// table[id0 + m, :] = slab 0 + slab 1 + ... of row m of a split-K projection, added in slab order exactly as the
// projection's consumers add them (load_f32_slabs, decode_attn_body.hpp); rows at or past `rows` (padding) are skipped
__global__ __launch_bounds__(256) void sum_slabs_rows_kernel(const float* __restrict__ slabs, int nslab, long slab_stride,
                                                             float* __restrict__ table, int id0, int rows, int M, int N) {
    const int m = blockIdx.x;
    if (m >= M || id0 + m >= rows) return;
    const float4* src = (const float4*)(slabs + (size_t)m * N);
    float4* dst = (float4*)(table + (size_t)(id0 + m) * N);
    for (int i = threadIdx.x; i < N / 4; i += blockDim.x) {
        float4 v = src[i];
        for (int s = 1; s < nslab; ++s) {
            const float4 t = *(const float4*)(slabs + (size_t)s * slab_stride + (size_t)m * N + 4 * i);
            v.x = __fadd_rn(v.x, t.x); v.y = __fadd_rn(v.y, t.y); v.z = __fadd_rn(v.z, t.z); v.w = __fadd_rn(v.w, t.w);
        }
        dst[i] = v;
    }
}

// out[b, :] = table[clamp(start[b / start_div]), :]: step 0's first-layer q/k/v (the clamp of embed_step_kernel)
__global__ __launch_bounds__(256) void gather_start_rows_kernel(const float* __restrict__ table, int N, int rows,
                                                                const int32_t* __restrict__ start, int start_div,
                                                                float* __restrict__ out, int start_ld,
                                                                int32_t* __restrict__ hist, int hist_ld) {
    const int b = blockIdx.x;
    int tok = start[(size_t)(b / start_div) * start_ld];
    tok = tok < 0 ? 0 : (tok >= rows ? rows - 1 : tok);
    if (hist && threadIdx.x == 0) hist[(size_t)b * hist_ld] = tok;   // position 0 of the row's token history
    const float4* src = (const float4*)(table + (size_t)tok * N);
    float4* dst = (float4*)(out + (size_t)b * N);
    for (int i = threadIdx.x; i < N / 4; i += blockDim.x) dst[i] = src[i];
}

// image[r, :] = bf16(table[r, col0 : col0 + W]): the K / V columns of the first layer's q/k/v table in the operand type, rounded
// as the cache append rounds them (store_chunk<bf16>: pack_bf16x2), so a row holds the bits the cache would hold
__global__ __launch_bounds__(256) void kv0_image_kernel(const float* __restrict__ table, int ld, int col0, int W,
                                                        uint32_t* __restrict__ image) {
    const float2* src = (const float2*)(table + (size_t)blockIdx.x * ld + col0);
    uint32_t* dst = image + (size_t)blockIdx.x * (W / 2);
    for (int i = threadIdx.x; i < W / 2; i += blockDim.x) {
        const float2 v = src[i];
        dst[i] = pack_bf16x2(v.x, v.y);
    }
}

// x[b*n + t, :] += pos[t, :] * scale   (TransformerWrapper abs. positional embedding of the legacy decoder,
// code/seq2seq.py:39 -> x-transformers AbsolutePositionalEmbedding: emb(arange(n)) * dim^-0.5)
__global__ void add_pos_rows_kernel(float* __restrict__ x, const float* __restrict__ pos, int M, int n, int C,
                                    float scale) {
    const long total = (long)M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / C), c = (int)(i - (long)m * C);
        x[i] = __fadd_rn(x[i], __fmul_rn(pos[(size_t)(m % n) * C + c], scale));
    }
}

// lens[b] = number of set entries of mask[b, :]  (the reference indexes v_speaker[i][mask[i]], code/seq2seq.py:228)
__global__ __launch_bounds__(64) void mask_lens_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ lens,
                                                       int T) {
    const int b = blockIdx.x;
    int n = 0;
    for (int t = threadIdx.x; t < T; t += 64) n += mask[(size_t)b * T + t] ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) n += __shfl_xor(n, o);
    if (threadIdx.x == 0) lens[b] = n;
}

// ListenerGenerator's x_speaker (code/seq2seq.py:224-241): the per-clip code vectors live channel-major as
// [zdim, len*fqn], are zero-padded along the LAST axis to T*fqn, and that memory is then re-read through
// .view(B,-1,fqn,zdim).view(B,-1,fqn*zdim) -- a reinterpretation, not a transpose.  Output element f of clip b is
// therefore channel c = f / (T*fqn), position p = f % (T*fqn) of the padded tensor.
template <typename OutT>
__global__ void legacy_scramble_kernel(const float* __restrict__ E, const int32_t* __restrict__ idx,
                                       const int32_t* __restrict__ lens, OutT* __restrict__ out, int B, int T, int fqn,
                                       int zdim, int n_embed) {
    const long per = (long)T * fqn * zdim, total = (long)B * per;
    const int P = T * fqn;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per);
        const long f = i - (long)b * per;
        const int c = (int)(f / P), p = (int)(f - (long)c * P);
        float v = 0.f;
        if (p < lens[b] * fqn) {
            int r = idx[(size_t)b * P + p];
            r = r < 0 ? 0 : (r >= n_embed ? n_embed - 1 : r);
            v = E[(size_t)r * zdim + c];
        }
        store_from_f32<OutT>(out + i, v);
    }
}

__global__ void step_inc_kernel(int32_t* step) { *step += 1; }

// per clip group: [0] step counter = step0 (0, or P0 - 1 of a prompted generation), [8] done counter = 0, [2] temperature
// bits, [4..5] seed, [6] global row offset and [7] global row count of the sampler's counter-based generator (generate()),
// [9] steps done in this call = 0 (the chain kernels' counter epoch), [10] step0 again, constant over the call (the sampler's
// clamp of the prompt lengths), [11] / [12] the sampler filter's real-valued parameters (thres | min_p | min_p_pow, min_p_ratio)
// [13] the guidance scale of a guided generation (sample_guided_kernel; 1 otherwise)
__global__ void gen_params_kernel(int32_t* base, int groups, float temperature, uint64_t seed, int row_off,
                                  int rows_total, int step0, float filter_a, float filter_b, float guidance) {
    const int g = threadIdx.x;
    if (g >= groups) return;
    int32_t* p = base + 16 * g;
    p[0] = step0;
    p[8] = 0;
    p[9] = 0;
    p[10] = step0;
    p[2] = __builtin_bit_cast(int32_t, temperature);
    *(uint64_t*)(p + 4) = seed;
    p[6] = row_off;
    p[7] = rows_total;
    p[11] = __builtin_bit_cast(int32_t, filter_a);
    p[12] = __builtin_bit_cast(int32_t, filter_b);
    p[13] = __builtin_bit_cast(int32_t, guidance);
    p[14] = 1;   // no step of this call has run yet: the sampling head of the first layer's launch (chain.hip) clears it
}

// dst[b, step, :] = src[b, :]  (optional per-step logits dump of generate)
__global__ void copy_rows_step_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int V, int n,
                                      const int32_t* __restrict__ step_dev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * V) return;
    const int b = i / V, c = i - b * V;
    dst[((size_t)b * n + *step_dev) * V + c] = src[i];
}

__global__ void mask_and_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t va = a ? a[i] : 1, vb = b ? b[i] : 1;
    out[i] = (va && vb) ? 1 : 0;
}

inline int ew_blocks(long total) {
    long b = (total + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace

int launch_cast_pad(int out_dtype, const float* x, int ldx, const float* coladd, void* y, int ldy, int M, int K,
                    hipStream_t s, const uint8_t* zero_rows) {
    DIMX_REQUIRE(x && y && M > 0 && K > 0 && ldy >= K, DIMX_ERR_ARG, "cast_pad: bad arguments");
    const int g = ew_blocks((long)M * ldy);
    if (out_dtype == DIMX_BF16)
        hipLaunchKernelGGL(cast_pad_kernel<bf16>, dim3(g), dim3(256), 0, s, x, ldx, coladd, (bf16*)y, ldy, M, K, zero_rows);
    else
        hipLaunchKernelGGL(cast_pad_kernel<float>, dim3(g), dim3(256), 0, s, x, ldx, coladd, (float*)y, ldy, M, K, zero_rows);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_gather_rows(int out_dtype, const float* table, int ld_table, int rows, const int32_t* idx, void* y,
                       int ldy, int M, int C, hipStream_t s) {
    DIMX_REQUIRE(table && idx && y && M > 0 && C > 0, DIMX_ERR_ARG, "gather_rows: bad arguments");
    const int g = ew_blocks((long)M * C);
    if (out_dtype == DIMX_BF16)
        hipLaunchKernelGGL(gather_rows_kernel<bf16>, dim3(g), dim3(256), 0, s, table, ld_table, rows, idx, (bf16*)y,
                           ldy, M, C);
    else
        hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(g), dim3(256), 0, s, table, ld_table, rows, idx,
                           (float*)y, ldy, M, C);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_context_concat(int out_dtype, const float* x_s, const float* patch, const float* audio, void* ctx, int M,
                          int dim, int dim_a, hipStream_t s) {
    DIMX_REQUIRE(x_s && patch && audio && ctx && M > 0, DIMX_ERR_ARG, "context_concat: bad arguments");
    const int g = ew_blocks((long)M * (dim + dim_a));
    if (out_dtype == DIMX_BF16)
        hipLaunchKernelGGL(context_concat_kernel<bf16>, dim3(g), dim3(256), 0, s, x_s, patch, audio, (bf16*)ctx, M,
                           dim, dim_a);
    else
        hipLaunchKernelGGL(context_concat_kernel<float>, dim3(g), dim3(256), 0, s, x_s, patch, audio, (float*)ctx, M,
                           dim, dim_a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_finalize_idx(int32_t* idx, const int32_t* lens, int B, int T, int32_t pad_value, hipStream_t s, int fqn) {
    if (!lens) return DIMX_OK;
    hipLaunchKernelGGL(finalize_idx_kernel, dim3(ceil_div(B * T * fqn, 256)), dim3(256), 0, s, idx, lens, B, T, fqn,
                       pad_value);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_shift_tokens(const int32_t* z, int32_t* inp, int32_t* tgt, int B, int T, hipStream_t s) {
    hipLaunchKernelGGL(shift_tokens_kernel, dim3(ceil_div(B * (T - 1), 256)), dim3(256), 0, s, z, inp, tgt, B, T);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_ce_argmax(const float* logits, const int32_t* target, float* row_loss, int32_t* argmax_tok, int R, int V,
                     hipStream_t s) {
    DIMX_REQUIRE(V == 512, DIMX_ERR_ARG, "ce_argmax: vocabulary %d != 512", V);
    hipLaunchKernelGGL(ce_argmax_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, s, logits, target, row_loss, argmax_tok,
                       R);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

static int check_sample(const SampleArgs& a) {
    const SampleFilter& filt = a.filt;
    DIMX_REQUIRE(a.logits && a.tokens && a.R > 0, DIMX_ERR_ARG, "sample: bad arguments");
    DIMX_REQUIRE(filt.kind >= DIMX_FILTER_TOP_K && filt.kind <= DIMX_FILTER_TOP_A, DIMX_ERR_ARG, "sample: unknown filter kind %d", filt.kind);
    DIMX_REQUIRE(!filt.keep_out || !a.prompt, DIMX_ERR_ARG, "sample: keep_out is not written for prompted rows");
    DIMX_REQUIRE(!a.prompt || (a.step_dev && a.tok_col_from_step && a.prompt_max >= 1 && a.prompt_ld >= a.prompt_max && a.prompt_div >= 1),
                 DIMX_ERR_ARG, "sample: a prompt needs the device step counter, 1 <= prompt_max <= prompt_ld and rows per clip >= 1");
    DIMX_REQUIRE(!a.qkv0_table || (a.x_next && a.qkv0_out && !a.pos_table && a.emb_C / 2 <= 16 * 64 && a.qkv0_N % 4 == 0 && a.qkv0_N > 0 &&
                                   a.qkv0_N <= 12 * 256),
                 DIMX_ERR_ARG, "sample: the q/k/v table rides on the fused embedding (no positional table) and holds rows of k * 4 <= 3072");
    DIMX_REQUIRE(!a.hist || (a.step_dev && a.hist_ld >= 1), DIMX_ERR_ARG, "sample: the token history needs the device step counter");
    DIMX_REQUIRE(!a.y_next || (a.x_next && a.y_gamma && a.emb_C % 128 == 0 && a.emb_C <= 2048), DIMX_ERR_ARG,
                 "sample: the fused pre-norm needs the fused embedding and a width of k * 128 <= 2048");
    return DIMX_OK;
}

// the kernels' common arguments, in DIMX_SAMPLE_PARAMS' order
#define DIMX_SAMPLE_LAUNCH_ARGS(sa)                                                                                                      \
    sa.logits, sa.ld_logits, sa.R, sa.top_k, sa.temperature, sa.noise, sa.seed, sa.step_dev, sa.step_host, sa.tokens, sa.tok_ld, sa.tok_col_from_step, \
        sa.nslab < 1 ? 1 : sa.nslab, sa.slab_stride, sa.logits_out, sa.logits_out_ld, sa.row0, sa.rows_total, sa.emb_table, sa.emb_C, sa.x_next,  \
        sa.step_rw, sa.done_ctr, sa.pos_table, sa.pos_scale, sa.pos_rows, sa.dev_params, sa.y_next, sa.y_gamma, sa.y_dtype == DIMX_BF16 ? 1 : 0, \
        sa.qkv0_table, sa.qkv0_out, sa.qkv0_N, sa.prompt, sa.prompt_ld, sa.prompt_max, sa.prompt_len, sa.prompt_div < 1 ? 1 : sa.prompt_div,     \
        sa.epoch_rw, sa.filt.a, sa.filt.b, sa.filt.keep_out, sa.hist, sa.hist_ld

int launch_sample(const SampleArgs& a, hipStream_t s) {
    const SampleFilter& filt = a.filt;
    DIMX_TRY(check_sample(a));
    const int wpb = a.R <= 1024 ? 1 : 4;  // one row per block for decode-sized batches: all CUs busy
    auto kern = filt.kind == DIMX_FILTER_TOP_P   ? sample_kernel<DIMX_FILTER_TOP_P>
                : filt.kind == DIMX_FILTER_MIN_P ? sample_kernel<DIMX_FILTER_MIN_P>
                : filt.kind == DIMX_FILTER_TOP_A ? sample_kernel<DIMX_FILTER_TOP_A>
                                                 : sample_kernel<DIMX_FILTER_TOP_K>;
    hipLaunchKernelGGL(kern, dim3(ceil_div(a.R, wpb)), dim3(64 * wpb), 0, s, DIMX_SAMPLE_LAUNCH_ARGS(a));
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

// a.R clips: rows [0, R) of a.logits are sampled against rows [0, R) of g.logits_u, and every per-row output of the sampler is
// written for rows r and r + R (the caller's buffers hold 2R rows); a.rows_total counts clips (the noise rows of an R-row launch)
int launch_sample_guided(const SampleArgs& a, const GuidedArgs& g, hipStream_t s) {
    const SampleFilter& filt = a.filt;
    DIMX_TRY(check_sample(a));
    DIMX_REQUIRE(g.logits_u && !filt.keep_out, DIMX_ERR_ARG, "sample_guided: no unconditional logits, or keep_out (not written here)");
    DIMX_REQUIRE(a.dev_params || g.scale - g.scale == 0.f, DIMX_ERR_ARG, "sample_guided: the scale is NaN or infinite");
    DIMX_REQUIRE(!g.branch_out || a.logits_out_ld >= 1, DIMX_ERR_ARG, "sample_guided: the branch dump needs its step count (logits_out_ld)");
    const int wpb = a.R <= 1024 ? 1 : 4;
    auto kern = filt.kind == DIMX_FILTER_TOP_P   ? sample_guided_kernel<DIMX_FILTER_TOP_P>
                : filt.kind == DIMX_FILTER_MIN_P ? sample_guided_kernel<DIMX_FILTER_MIN_P>
                : filt.kind == DIMX_FILTER_TOP_A ? sample_guided_kernel<DIMX_FILTER_TOP_A>
                                                 : sample_guided_kernel<DIMX_FILTER_TOP_K>;
    hipLaunchKernelGGL(kern, dim3(ceil_div(a.R, wpb)), dim3(64 * wpb), 0, s, DIMX_SAMPLE_LAUNCH_ARGS(a), g.logits_u, g.scale, g.branch_out,
                       g.tokens_u);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_gen_params(int32_t* base, int groups, float temperature, uint64_t seed, int row_off, int rows_total,
                      hipStream_t s, int step0, float filter_a, float filter_b, float guidance) {
    DIMX_REQUIRE(step0 >= 0, DIMX_ERR_ARG, "gen_params: negative first step");
    hipLaunchKernelGGL(gen_params_kernel, dim3(1), dim3(64), 0, s, base, groups, temperature, seed, row_off, rows_total, step0,
                       filter_a, filter_b, guidance);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_embed_step(const float* table, int C, int rows, const int32_t* start, const int32_t* tokens, int tok_ld,
                      const int32_t* step_dev, float* x, int B, int start_div, hipStream_t s, const float* pos_table,
                      float pos_scale, int start_ld, int start_step) {
    DIMX_REQUIRE(C % 4 == 0 && start_ld >= 1 && start_step >= 0, DIMX_ERR_ARG, "embed_step: C %% 4, start stride or step");
    hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(256), 0, s, table, C, start, tokens, tok_ld, step_dev, x,
                       rows, start_div < 1 ? 1 : start_div, pos_table, pos_scale, start_ld, start_step);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_iota_clamp(int32_t* ids, int n, int rows, hipStream_t s) {
    DIMX_REQUIRE(ids && n > 0 && rows > 0, DIMX_ERR_ARG, "iota_clamp: bad arguments");
    hipLaunchKernelGGL(iota_clamp_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, ids, n, rows);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_sum_slabs_rows(const float* slabs, int nslab, long slab_stride, float* table, int id0, int rows, int M, int N,
                          hipStream_t s) {
    DIMX_REQUIRE(slabs && table && nslab >= 1 && M > 0 && N > 0 && N % 4 == 0 && slab_stride % 4 == 0 && id0 >= 0, DIMX_ERR_ARG,
                 "sum_slabs_rows: bad arguments");
    hipLaunchKernelGGL(sum_slabs_rows_kernel, dim3(M), dim3(256), 0, s, slabs, nslab, slab_stride, table, id0, rows, M, N);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_gather_start_rows(const float* table, int N, int rows, const int32_t* start, int start_div, float* out, int B,
                             hipStream_t s, int start_ld, int32_t* hist, int hist_ld) {
    DIMX_REQUIRE(table && start && out && B > 0 && N > 0 && N % 4 == 0 && rows > 0 && start_ld >= 1 && (!hist || hist_ld >= 1), DIMX_ERR_ARG,
                 "gather_start_rows: bad arguments");
    hipLaunchKernelGGL(gather_start_rows_kernel, dim3(B), dim3(256), 0, s, table, N, rows, start, start_div < 1 ? 1 : start_div, out,
                       start_ld, hist, hist_ld);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_kv0_image(const float* table, int ld, int rows, int col0, int W, void* image, hipStream_t s) {
    DIMX_REQUIRE(table && image && rows > 0 && W > 0 && W % 2 == 0 && col0 >= 0 && col0 % 2 == 0 && ld % 2 == 0 && col0 + W <= ld, DIMX_ERR_ARG,
                 "kv0_image: bad arguments");
    hipLaunchKernelGGL(kv0_image_kernel, dim3(rows), dim3(256), 0, s, table, ld, col0, W, (uint32_t*)image);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_add_pos_rows(float* x, const float* pos, int M, int n, int C, float scale, hipStream_t s) {
    DIMX_REQUIRE(x && pos && M > 0 && n > 0, DIMX_ERR_ARG, "add_pos_rows: bad arguments");
    const long total = (long)M * C;
    const int blocks = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
    hipLaunchKernelGGL(add_pos_rows_kernel, dim3(blocks), dim3(256), 0, s, x, pos, M, n, C, scale);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_mask_lens(const uint8_t* mask, int32_t* lens, int B, int T, hipStream_t s) {
    DIMX_REQUIRE(mask && lens && B > 0 && T > 0, DIMX_ERR_ARG, "mask_lens: bad arguments");
    hipLaunchKernelGGL(mask_lens_kernel, dim3(B), dim3(64), 0, s, mask, lens, T);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_legacy_scramble(int out_dtype, const float* E, const int32_t* idx, const int32_t* lens, void* out, int B,
                           int T, int fqn, int zdim, int n_embed, hipStream_t s) {
    DIMX_REQUIRE(E && idx && lens && out && B > 0 && T > 0, DIMX_ERR_ARG, "legacy_scramble: bad arguments");
    const long total = (long)B * T * fqn * zdim;
    const int blocks = (int)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192);
    if (out_dtype == DIMX_BF16)
        hipLaunchKernelGGL((legacy_scramble_kernel<bf16>), dim3(blocks), dim3(256), 0, s, E, idx, lens, (bf16*)out, B,
                           T, fqn, zdim, n_embed);
    else
        hipLaunchKernelGGL((legacy_scramble_kernel<float>), dim3(blocks), dim3(256), 0, s, E, idx, lens, (float*)out,
                           B, T, fqn, zdim, n_embed);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_step_inc(int32_t* step_dev, hipStream_t s) {
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step_dev);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_copy_rows_step(const float* src, float* dst, int B, int V, int n, const int32_t* step_dev, hipStream_t s) {
    hipLaunchKernelGGL(copy_rows_step_kernel, dim3(ceil_div(B * V, 256)), dim3(256), 0, s, src, dst, B, V, n, step_dev);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_mask_and(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(mask_and_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, a, b, out, n);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
