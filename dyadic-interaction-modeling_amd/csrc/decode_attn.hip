// decode_attn.hip -- one-query attention of the autoregressive decoder step (KV-cached
// AutoregressiveWrapper.generate, call site reference code/seq2seq_pretrain.py:450): for every
// (clip, head) a single 64-d query attends over the cached keys.  Self-attention additionally appends
// this step's key/value to the cache; cross-attention reads the context K/V projected once per clip and
// honours the context (padding) mask.
//
// M = 1 per (clip, head): no matrix-core work, the kernel is a pure HBM stream of the K/V caches
// ([B,H,Tmax,64], 128 B (bf16) / 256 B (f32) per key).  One wave per (clip, head); 8 (bf16) or 16 (f32)
// lanes cooperate on one key so that every wave-wide load instruction covers 1 KiB of contiguous
// cache, scores go through LDS (one float per key), and the P.V pass re-streams V the same way.
#include "common.hpp"
#include "decode_attn_body.hpp"

namespace dimx {
namespace {

// TAB: the first layer's table form (decode_attn_body.hpp) -- K / V rows from the table over the token ids, no cache
// WIN: the windowed cross form (decode_attn_body.hpp) -- the step counter bounds the keys
template <typename T, bool SELF, bool QF32, int NSPLIT, bool TAB = false, bool WIN = false>
__global__ __launch_bounds__(256) void decode_attn_kernel(const DecodeAttnArgs a) {
    constexpr int PPB = 4 / NSPLIT;  // (clip, head) pairs per block
    __shared__ float sc[PPB][kMaxKeys];
    __shared__ float red_m[4], red_l[4];
    __shared__ float red_acc[4][64];
    decode_attn_body<T, SELF, QF32, NSPLIT, 4, false, TAB, WIN>(a, blockIdx.x, &sc[0][0], kMaxKeys, red_m, red_l, &red_acc[0][0]);
}

// Multi-sample cross attention: SQ query rows (independent samples of the same clip) share one pass over
// the clip's K/V cache -- the reference's best-of-10 protocol (code/x_engine_pt.py:257) re-reads the same
// context ten times; here the cache is streamed once per (clip, head) and every key is scored against all SQ
// queries.  q/out rows of clip b are b*SQ .. b*SQ+SQ-1; scores live in LDS as [SQ][n].
// WIN: the windowed form, as in decode_attn_body -- n below is what the step may see; the launcher sizes the LDS for n_keys.
template <typename T, int SQ, bool QF32, bool WIN = false>
__global__ __launch_bounds__(256) void decode_attn_multi_kernel(const DecodeAttnArgs a) {
    constexpr int EPC = 16 / sizeof(T);
    constexpr int LPK = 64 / EPC;
    constexpr int KPI = 64 / LPK;
    constexpr int U = 4;
    constexpr int KB = U * KPI;
    extern __shared__ __attribute__((aligned(16))) float dyn_sc[];  // [4 waves][SQ][npad]

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + wave;
    const bool active = pair < a.B * a.H;
    const int b = active ? pair / a.H : 0, h = active ? pair % a.H : 0;   // b = clip
    const int sub = lane / LPK, ch = lane % LPK;
    int n = a.n_keys;
    if constexpr (WIN) n = win_keys(*a.step, a.lookahead, a.n_keys);
    const int npad = (n + 3) & ~3;
    const float scale2 = a.scale * 1.4426950408889634f;
    const T* kc = (const T*)a.kcache + ((size_t)(b * a.H + h) * a.Tmax) * 64 + ch * EPC;
    const T* vc = (const T*)a.vcache + ((size_t)(b * a.H + h) * a.Tmax) * 64 + ch * EPC;
    float* s = dyn_sc + (size_t)wave * SQ * npad;
    const bool masked = a.kmask != nullptr;

    auto load_batch = [&](const T* base, int j0, uint4 (&r)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            r[u] = ld_stream(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };
    uint4 cur[U], nxt[U];
    load_batch(kc, 0, cur);
    float qv[SQ][EPC];
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
        const size_t row = (size_t)b * SQ + q;
        if (QF32)
            load_f32_slabs<EPC>((const float*)a.q + row * a.q_ld + h * 64 + ch * EPC, a.nslab, a.slab_stride, qv[q]);
        else
            load_chunk<T, EPC>((const T*)a.q + row * a.q_ld + h * 64 + ch * EPC, qv[q]);
    }
    float mx[SQ];
#pragma unroll
    for (int q = 0; q < SQ; ++q) mx[q] = kNegD;
    for (int j0 = 0; j0 < n; j0 += KB) {
        if (j0 + KB < n) load_batch(kc, j0 + KB, nxt);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float kv[EPC];
            cvt_chunk<T, EPC>(cur[u], kv);
            const bool dead = masked && j < n && a.kmask[(size_t)b * a.kmask_ld + j] == 0;
#pragma unroll
            for (int q = 0; q < SQ; ++q) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < EPC; ++e) d = fmaf(qv[q][e], kv[e], d);
                d = LPK == 8 ? group8_sum(d) : row16_sum(d);
                if (j < n) {
                    const float sv = dead ? kNegD : d * scale2;
                    if (ch == 0) s[q * npad + j] = sv;
                    mx[q] = fmaxf(mx[q], sv);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    load_batch(vc, 0, cur);
#pragma unroll
    for (int q = 0; q < SQ; ++q) mx[q] = wave_max(mx[q]);
    __syncthreads();
    float lsum[SQ];
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
        float l = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float p = exp2f(s[q * npad + j] - mx[q]);
            s[q * npad + j] = p;
            l += p;
        }
        lsum[q] = wave_sum_sel<sizeof(T) == 2>(l);
    }
    __syncthreads();
    float acc[SQ][EPC];
#pragma unroll
    for (int q = 0; q < SQ; ++q)
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[q][e] = 0.f;
    for (int j0 = 0; j0 < n; j0 += KB) {
        if (j0 + KB < n) load_batch(vc, j0 + KB, nxt);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float vv[EPC];
            cvt_chunk<T, EPC>(cur[u], vv);
#pragma unroll
            for (int q = 0; q < SQ; ++q) {
                const float p = j < n ? s[q * npad + j] : 0.f;
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[q][e] = fmaf(p, vv[e], acc[q][e]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            if (LPK <= 8) acc[q][e] += xor_lane_f32<8>(acc[q][e]);
            acc[q][e] += xor_lane_f32<16>(acc[q][e]);
            acc[q][e] += xor_lane_f32<32>(acc[q][e]);
        }
        if (active && sub == 0) {
            const float inv = lsum[q] > 0.f ? 1.0f / lsum[q] : 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[q][e] *= inv;
            store_chunk<T, EPC>((T*)a.out + ((size_t)b * SQ + q) * a.o_ld + h * 64 + ch * EPC, acc[q]);
        }
    }
}

}  // namespace

int launch_decode_attn(const DecodeAttnArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.kcache && a.vcache && a.out, DIMX_ERR_ARG, "decode_attn: null operand");
    DIMX_REQUIRE((a.knew == nullptr) == (a.vnew == nullptr), DIMX_ERR_ARG, "decode_attn: knew/vnew mismatch");
    DIMX_REQUIRE(a.knew == nullptr || a.step != nullptr, DIMX_ERR_ARG, "decode_attn: self attention needs a step counter");
    DIMX_REQUIRE(a.Tmax <= kMaxKeys && a.n_keys <= kMaxKeys, DIMX_ERR_ARG, "decode_attn: more than %d keys", kMaxKeys);
    DIMX_REQUIRE(a.knew != nullptr || a.n_keys >= 1, DIMX_ERR_ARG, "decode_attn: cross attention over %d keys", a.n_keys);
    if (a.tab) {
        const int epc = a.dtype == DIMX_BF16 ? 8 : 4;
        DIMX_REQUIRE(a.knew && a.q_f32 && a.hist && a.hist_ld >= a.Tmax && a.Tmax >= 1 && a.tab_rows >= 1, DIMX_ERR_ARG,
                     "decode_attn: the table form is self attention on f32 slabs with a token history of at least Tmax entries per row");
        DIMX_REQUIRE(a.tab_ld % epc == 0 && a.tab_koff % epc == 0 && a.tab_voff % epc == 0 && a.tab_koff >= 0 && a.tab_voff >= 0 &&
                         a.tab_koff + a.H * 64 <= a.tab_ld && a.tab_voff + a.H * 64 <= a.tab_ld && (uintptr_t)a.tab % 16 == 0,
                     DIMX_ERR_ARG, "decode_attn: table rows of %d with K at %d and V at %d", a.tab_ld, a.tab_koff, a.tab_voff);
    }
    DIMX_REQUIRE(!a.win || (a.knew == nullptr && a.step != nullptr && !a.tab), DIMX_ERR_ARG,
                 "decode_attn: the windowed form is cross attention with a step counter");
    if (a.rows_per_clip > 1) {
        // multi-sample cross attention: a.B = clips, rows = B * rows_per_clip
        DIMX_REQUIRE(a.knew == nullptr, DIMX_ERR_ARG, "decode_attn: rows_per_clip applies to cross attention only");
        const int S = a.rows_per_clip;
        const int npad = (a.n_keys + 3) & ~3;
        const size_t lds = (size_t)4 * S * npad * sizeof(float);
        DIMX_REQUIRE(lds <= 150 * 1024, DIMX_ERR_ARG, "decode_attn: %d samples x %d keys do not fit the LDS score buffer", S,
                     a.n_keys);
        dim3 grid(ceil_div(a.B * a.H, 4)), block(256);
#define DM_W(TT, SS, QQ, WW)                                                                                    \
    do {                                                                                                        \
        (void)hipFuncSetAttribute((const void*)decode_attn_multi_kernel<TT, SS, QQ, WW>,                        \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
        hipLaunchKernelGGL((decode_attn_multi_kernel<TT, SS, QQ, WW>), grid, block, lds, s, a);                 \
    } while (0)
#define DM(TT, SS, QQ)                        \
    do {                                      \
        if (a.win) DM_W(TT, SS, QQ, true);    \
        else DM_W(TT, SS, QQ, false);         \
    } while (0)
#define DM_S(TT, QQ)                         \
    do {                                     \
        switch (S) {                         \
            case 2: DM(TT, 2, QQ); break;    \
            case 4: DM(TT, 4, QQ); break;    \
            case 5: DM(TT, 5, QQ); break;    \
            case 8: DM(TT, 8, QQ); break;    \
            case 10: DM(TT, 10, QQ); break;  \
            default:                         \
                set_error("decode_attn: rows_per_clip %d not in {2,4,5,8,10}", S); \
                return DIMX_ERR_ARG;         \
        }                                    \
    } while (0)
        if (a.dtype == DIMX_BF16) { if (a.q_f32) DM_S(bf16, true); else DM_S(bf16, false); }
        else { if (a.q_f32) DM_S(float, true); else DM_S(float, false); }
#undef DM_S
#undef DM
#undef DM_W
        DIMX_HIP(hipGetLastError());
        return DIMX_OK;
    }
    // waves per (clip, head): enough waves to cover the chip (~12 per CU) without splitting large batches
    const int pairs = a.B * a.H;
    int nsplit = 1;
    if (pairs * 2 <= 3072) nsplit = 2;
    if (pairs * 4 <= 3072) nsplit = 4;
    // f32 parity mode: the wave count decides the summation order, and a rank's shard of a batch must reproduce the rows of the
    // whole batch bit for bit -- so it may depend on the cache length only, never on the batch (round 4; until then
    // a 128-clip shard ran 2 waves per pair, the 256-clip batch 1, and equal tokens were a matter of no near-tie being hit)
    if (a.dtype != DIMX_BF16) nsplit = a.Tmax >= 1024 ? 4 : (a.Tmax >= 512 ? 2 : 1);
    if (a.force_nsplit == 1 || a.force_nsplit == 2 || a.force_nsplit == 4) nsplit = a.force_nsplit;
    dim3 grid(ceil_div(pairs, 4 / nsplit)), block(256);
    const bool self = a.knew != nullptr;
#define DA_LAUNCH(TT, SS, QQ, NS) hipLaunchKernelGGL((decode_attn_kernel<TT, SS, QQ, NS>), grid, block, 0, s, a)
#define DA_NS(TT, SS, QQ)                          \
    do {                                           \
        if (nsplit == 4) DA_LAUNCH(TT, SS, QQ, 4); \
        else if (nsplit == 2) DA_LAUNCH(TT, SS, QQ, 2); \
        else DA_LAUNCH(TT, SS, QQ, 1);             \
    } while (0)
#define DA_TAB(TT)                                                                                  \
    do {                                                                                            \
        if (nsplit == 4) hipLaunchKernelGGL((decode_attn_kernel<TT, true, true, 4, true>), grid, block, 0, s, a);      \
        else if (nsplit == 2) hipLaunchKernelGGL((decode_attn_kernel<TT, true, true, 2, true>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((decode_attn_kernel<TT, true, true, 1, true>), grid, block, 0, s, a);                  \
    } while (0)
#define DA_WIN(TT, QQ)                                                                              \
    do {                                                                                            \
        if (nsplit == 4) hipLaunchKernelGGL((decode_attn_kernel<TT, false, QQ, 4, false, true>), grid, block, 0, s, a);      \
        else if (nsplit == 2) hipLaunchKernelGGL((decode_attn_kernel<TT, false, QQ, 2, false, true>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((decode_attn_kernel<TT, false, QQ, 1, false, true>), grid, block, 0, s, a);                  \
    } while (0)
    if (a.tab) {
        if (a.dtype == DIMX_BF16) DA_TAB(bf16); else DA_TAB(float);
    } else if (a.win) {
        if (a.dtype == DIMX_BF16) { if (a.q_f32) DA_WIN(bf16, true); else DA_WIN(bf16, false); }
        else { if (a.q_f32) DA_WIN(float, true); else DA_WIN(float, false); }
    } else if (a.dtype == DIMX_BF16) {
        if (a.q_f32) { if (self) DA_NS(bf16, true, true); else DA_NS(bf16, false, true); }
        else { if (self) DA_NS(bf16, true, false); else DA_NS(bf16, false, false); }
    } else {
        if (a.q_f32) { if (self) DA_NS(float, true, true); else DA_NS(float, false, true); }
        else { if (self) DA_NS(float, true, false); else DA_NS(float, false, false); }
    }
#undef DA_WIN
#undef DA_TAB
#undef DA_NS
#undef DA_LAUNCH
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
