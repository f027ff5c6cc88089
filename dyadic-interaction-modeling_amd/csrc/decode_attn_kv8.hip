// decode_attn_kv8.hip -- the decode step's cross attention over an FP8 copy of the context K/V (dimx/kv8.py is the definition).
//
// The cross K/V cache of a generation is written once per clip and streamed by every decode step; it is the step's one large HBM
// stream (decode_attn.hip).  kv8_quant_kernel turns a layer's cache [B, H, Tp, 64] (bf16 / f32) into OCP e4m3fn codes
// [B, H, Tp, 64] uint8 plus one f32 scale per (clip, head, key) [B, H, Tp], once per generation (kv8_append_kernel: the rows a
// streaming session's push appended, K and V of every layer in one launch -- a row's codes depend on that row alone); decode_attn_kv8_kernel is the
// one-query cross attention over those codes: decode_attn_body's shape with 16 elements per 16-byte lane load --
//   4 lanes per key, 16 keys (1 KiB contiguous) per wave-wide load, 4 loads = 64 keys per batch, the next batch in flight while
//   the current one is consumed, codes unpacked by the hardware convert (v_cvt_pk_f32_fp8).
// A batch is 64 keys and a wave has 64 lanes, so the scales stay off the key loops: the score loop stores the raw q . codes dots
// of its batch to the LDS score row, then lane i scales the dot of key j0 + i by kscale (loaded one batch ahead, coalesced) and the
// softmax scale and applies the mask; the value loop's lane i turns that score into p and stores p * vscale for the batch's
// fmas while summing the unscaled p.  A wave only ever touches the scores of the batches it scored itself, so the waves of a
// (clip, head) meet at the three fixed-order reductions (max, sum, output) and nowhere else.  No atomics; repeats are bit-identical.
// decode_attn_mq_kv8_kernel (further down) is the multi-query form for best-of-N generation: the S queries of a clip against that
// clip's codes on the matrix cores, one wave per (clip, head), the codes read once for all S (dimx/kv8.py attention_rows).
#include "common.hpp"
#include "decode_attn_body.hpp"

namespace dimx {
namespace {

typedef float f32x2_cv __attribute__((ext_vector_type(2)));

// 16 e4m3fn codes (one 16-byte load) -> 16 floats, element e = byte e
__device__ __forceinline__ void unpack_fp8x16(const uint4& u, float (&v)[16]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2_cv lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const f32x2_cv hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        v[4 * i] = lo.x; v[4 * i + 1] = lo.y; v[4 * i + 2] = hi.x; v[4 * i + 3] = hi.y;
    }
}

__device__ __forceinline__ float group4_sum(float v) {  // the xor 1, 2 butterfly over a key's four lanes
    v += dpp_f32<DPP_XOR1>(v);
    v += dpp_f32<DPP_XOR2>(v);
    return v;
}
__device__ __forceinline__ float group4_max(float v) {
    v = fmaxf(v, dpp_f32<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f32<DPP_XOR2>(v));
    return v;
}

template <typename T> __device__ __forceinline__ void load_row16(const T* p, float (&v)[16]);
template <> __device__ __forceinline__ void load_row16<float>(const float* p, float (&v)[16]) { load_f32_chunk<16>(p, v); }
template <> __device__ __forceinline__ void load_row16<bf16>(const bf16* p, float (&v)[16]) {
    float a[8], b[8];
    load_chunk<bf16, 8>(p, a);
    load_chunk<bf16, 8>(p + 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = a[e]; v[8 + e] = b[e]; }
}

// One row of 64 floats held by four neighbouring lanes, 16 elements each -> the lane's 16 codes and the row's scale (dimx/kv8.py
// quantize).  Every lane of the four must be active (the butterfly).  The one quantiser of this file: kv8_quant_kernel and the self
// form's append both call it, so their bits cannot differ.
__device__ __forceinline__ float quant_row16(const float (&x)[16], uint4& codes) {
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
    amax = group4_max(amax);
    const bool zero = amax < 0x1p-60f;
    const float scale = zero ? 0.f : __fdiv_rn(amax, 448.f);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fminf(fmaxf(__fdiv_rn(x[4 * i + e], zero ? 1.f : scale), -448.f), 448.f);
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
        w[i] = zero ? 0u : (uint32_t)p;
    }
    codes = make_uint4(w[0], w[1], w[2], w[3]);
    return scale;
}

// Rows 0 .. T - 1 of every (clip, head) of one cache [BH, Tp, 64] -> codes / scales (dimx/kv8.py quantize): four lanes per row,
// 16 elements each.  Rows at or past T are neither read nor written.
// Tc: the cache's rows per (clip, head) where they differ from the codes' (the generation's self caches are [R, H, T, 64]).
template <typename T>
__global__ __launch_bounds__(256) void kv8_quant_kernel(const T* cache, long rows, int Tc, int Tp, int Tn, uint8_t* codes, float* scales) {
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = tid >> 2;
    const int ch = (int)(tid & 3);
    const bool live = row < rows;
    const long r = live ? row : rows - 1;   // every lane of the wave stays active for the butterfly
    const long at = (r / Tn) * Tp + r % Tn;
    float x[16];
    load_row16<T>(cache + ((r / Tn) * Tc + r % Tn) * 64 + ch * 16, x);
    uint4 w;
    const float scale = quant_row16(x, w);
    if (live) {
        *(uint4*)(codes + at * 64 + ch * 16) = w;
        if (ch == 0) scales[at] = scale;
    }
}

// Rows [n0, n0 + c) of every (clip, head) of the K and V caches of every layer -> codes / scales, one launch (a streaming
// session's push: stream.hip).  blockIdx.y picks the cache (2 l: layer l's K, 2 l + 1: its V), so the pointer loads are
// scalar; blockIdx.x covers that cache's B * H * c rows, four lanes per row as above.  Rows outside the range are neither read nor
// written; a wave with fewer live rows than lanes recomputes the last row and stores nothing (the butterfly needs every lane).
template <typename T>
__global__ __launch_bounds__(256) void kv8_append_kernel(const Kv8AppendArgs a) {
    const int which = blockIdx.y;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long rows = (long)a.B * a.H * a.c;
    const long row = tid >> 2;
    const int ch = (int)(tid & 3);
    const bool live = row < rows;
    const long r = live ? row : rows - 1;
    const long pair = r / a.c;
    const int j = a.n0 + (int)(r % a.c);
    float x[16];
    load_row16<T>((const T*)a.cache[which] + (pair * a.Tc + j) * 64 + ch * 16, x);
    uint4 w;
    const float scale = quant_row16(x, w);
    if (live) {
        const long at = pair * a.Tp + j;
        *(uint4*)(a.codes[which] + at * 64 + ch * 16) = w;
        if (ch == 0) a.scales[which][at] = scale;
    }
}

template <typename TO> __device__ __forceinline__ void store_out16(TO* p, const float (&v)[16]);
template <> __device__ __forceinline__ void store_out16<float>(float* p, const float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(p + 4 * i) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}
template <> __device__ __forceinline__ void store_out16<bf16>(bf16* p, const float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
        *(uint4*)(p + 8 * i) = make_uint4(pack_bf16x2(v[8 * i], v[8 * i + 1]), pack_bf16x2(v[8 * i + 2], v[8 * i + 3]),
                                          pack_bf16x2(v[8 * i + 4], v[8 * i + 5]), pack_bf16x2(v[8 * i + 6], v[8 * i + 7]));
}

// TO: the type of out (the handle's operand type).  NSPLIT (1, 2, 4): waves per (clip, head), batches dealt round-robin, partial
// (max, sum, output) combined through LDS in wave order.  WIN: the key count is win_keys(*step, lookahead, n_keys); everything
// below runs on that n as the plain form would with n_keys = n, so the bits are those of the plain form called with n_keys = n.
// Codes and scales at or past n are never read: loads past it are redirected to row n - 1.
template <typename TO, int NSPLIT, bool WIN>
__global__ __launch_bounds__(256) void decode_attn_kv8_kernel(const Kv8AttnArgs a) {
    constexpr int EPC = 16;          // codes per 16-byte lane load
    constexpr int LPK = 4;           // lanes per key
    constexpr int KPI = 16;          // keys per wave-wide load
    constexpr int U = 4;             // loads per batch
    constexpr int KB = U * KPI;      // keys per batch == lanes of a wave
    constexpr int PPB = 4 / NSPLIT;  // (clip, head) pairs per block
    static_assert(KB == 64, "a batch is one key per lane");
    __shared__ float sc[PPB][kMaxKeys];
    __shared__ float red_m[4], red_l[4];
    __shared__ float red_acc[4][64];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pib = wave / NSPLIT, part = wave % NSPLIT;
    const int pair = blockIdx.x * PPB + pib;
    const bool active = pair < a.B * a.H;
    const int b = active ? pair / a.H : 0, h = active ? pair % a.H : 0;
    const int sub = lane / LPK, ch = lane % LPK;
    const int jfirst = part * KB, jstep = NSPLIT * KB;  // this wave's key batches: jfirst, jfirst + jstep, ...

    float qv[EPC];
    load_f32_slabs<EPC>(a.q + (size_t)b * a.q_ld + h * 64 + ch * EPC, a.nslab, a.slab_stride, qv);
    int n = a.n_keys;
    if constexpr (WIN) n = win_keys(*a.step, a.lookahead, a.n_keys);
    const float scale2 = a.scale * 1.4426950408889634f;

    const size_t row0 = (size_t)(b * a.H + h) * a.Tmax;
    const uint8_t* kc = a.kcodes + row0 * 64 + ch * EPC;
    const uint8_t* vc = a.vcodes + row0 * 64 + ch * EPC;
    const float* ks = a.kscale + row0;
    const float* vs = a.vscale + row0;
    const uint8_t* km = a.kmask ? a.kmask + (size_t)b * a.kmask_ld : nullptr;
    float* s = &sc[pib][0];

    auto load_batch = [&](const uint8_t* base, int j0, uint4 (&r)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            r[u] = ld_stream(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };
    auto own = [&](int j0) { return j0 + lane < n ? j0 + lane : n - 1; };   // the key whose score this lane scales in batch j0

    uint4 cur[U] = {}, nxt[U] = {}, vfirst[U] = {};
    float kcur = 0.f, knxt = 0.f, vcur = 0.f, vnxt = 0.f;
    bool dcur = false, dnxt = false;   // the lane's own key is masked
    if (jfirst < n) {
        load_batch(kc, jfirst, cur);
        load_batch(vc, jfirst, vfirst);  // the first V batch rides along: short contexts are one latency hop shorter
        kcur = ks[own(jfirst)];
        vcur = vs[own(jfirst)];
        if (km) dcur = km[own(jfirst)] == 0;
    }

    // ---- scores: raw dots of the batch, then one key per lane scaled and masked
    float mx = kNegD;
    for (int j0 = jfirst; j0 < n; j0 += jstep) {
        if (j0 + jstep < n) {
            load_batch(kc, j0 + jstep, nxt);
            knxt = ks[own(j0 + jstep)];
            if (km) dnxt = km[own(j0 + jstep)] == 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float kv[EPC];
            unpack_fp8x16(cur[u], kv);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) d = fmaf(qv[e], kv[e], d);
            d = group4_sum(d);
            if (ch == 0 && j < n) s[j] = d;
        }
        if (j0 + lane < n) {
            float sv = (s[j0 + lane] * kcur) * scale2;
            if (dcur) sv = kNegD;
            s[j0 + lane] = sv;
            mx = fmaxf(mx, sv);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        kcur = knxt;
        dcur = dnxt;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = vfirst[u];
    mx = wave_max(mx);
    if (NSPLIT > 1) {
        if (lane == 0) red_m[wave] = mx;
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NSPLIT; ++p) mx = fmaxf(mx, red_m[pib * NSPLIT + p]);
    }

    // ---- o = sum_j p_j vscale_j codes_j, row sum of the unscaled p_j
    float lsum = 0.f;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    for (int j0 = jfirst; j0 < n; j0 += jstep) {
        if (j0 + jstep < n) {
            load_batch(vc, j0 + jstep, nxt);
            vnxt = vs[own(j0 + jstep)];
        }
        if (j0 + lane < n) {
            const float p = exp2f(s[j0 + lane] - mx);
            lsum += p;
            s[j0 + lane] = p * vcur;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float vv[EPC];
            unpack_fp8x16(cur[u], vv);
            const float p = j < n ? s[j] : 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(p, vv[e], acc[e]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        vcur = vnxt;
    }
    lsum = wave_sum_sel<sizeof(TO) == 2>(lsum);
    if (NSPLIT > 1) {
        if (lane == 0) red_l[wave] = lsum;
        __syncthreads();
        lsum = 0.f;
#pragma unroll
        for (int p = 0; p < NSPLIT; ++p) lsum += red_l[pib * NSPLIT + p];
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) {  // xor 4 .. 32 butterfly over the key sub-groups
        acc[e] += xor_lane_f32<4>(acc[e]);
        acc[e] += xor_lane_f32<8>(acc[e]);
        acc[e] += xor_lane_f32<16>(acc[e]);
        acc[e] += xor_lane_f32<32>(acc[e]);
    }
    if (NSPLIT > 1) {  // combine the partial outputs of the pair's waves in wave order
        if (sub == 0) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) red_acc[wave][ch * EPC + e] = acc[e];
        }
        __syncthreads();
        if (part == 0 && sub == 0) {
#pragma unroll
            for (int p = 1; p < NSPLIT; ++p)
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += red_acc[pib * NSPLIT + p][ch * EPC + e];
        }
    }
    if (active && part == 0 && sub == 0) {
        const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] *= inv;
        store_out16<TO>((TO*)a.out + (size_t)b * a.o_ld + h * 64 + ch * EPC, acc);
    }
}

// The self form over FP8 self caches (dimx/kv8.py self_step): the kernel above with decode_attn_body's SELF duties.  q and this
// step's k / v come from the projection's f32 slabs; n = *step rows are cached and the keys are the positions 0 .. n.  Every wave
// of a (row, head) quantises the new k / v row in registers (quant_row16: each key group of four lanes holds the whole row), so
// the new row's codes are a uint4 per lane like a loaded one and its scales a float like a loaded one: the batch that contains
// position n swaps them in where it consumes that key, and the loops below are the cross form's over n + 1 keys.  One wave stores
// codes and scales at position n; loads are clamped to n - 1 (none at all at n = 0), so no load depends on that store and rows
// past n are neither read nor written.  n itself is clamped to n_max < Tmax.
// Four blocks per CU asked for: the new row's registers would otherwise lift the kernel past 128 VGPRs and cost it the fourth wave
// per SIMD the cross form has (118 .. 122 VGPRs, no scratch, with the bound; 130 .. 136 without).
template <typename TO, int NSPLIT>
__global__ __launch_bounds__(256, 4) void decode_attn_self_kv8_kernel(const Kv8SelfArgs a) {
    constexpr int EPC = 16;          // codes per 16-byte lane load
    constexpr int LPK = 4;           // lanes per key
    constexpr int KPI = 16;          // keys per wave-wide load
    constexpr int U = 4;             // loads per batch
    constexpr int KB = U * KPI;      // keys per batch == lanes of a wave
    constexpr int PPB = 4 / NSPLIT;  // (row, head) pairs per block
    static_assert(KB == 64, "a batch is one key per lane");
    __shared__ float sc[PPB][kMaxKeys];
    __shared__ float red_m[4], red_l[4];
    __shared__ float red_acc[4][64];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pib = wave / NSPLIT, part = wave % NSPLIT;
    const int pair = blockIdx.x * PPB + pib;
    const bool active = pair < a.B * a.H;
    const int b = active ? pair / a.H : 0, h = active ? pair % a.H : 0;
    const int sub = lane / LPK, ch = lane % LPK;
    const int jfirst = part * KB, jstep = NSPLIT * KB;  // this wave's key batches: jfirst, jfirst + jstep, ...

    float qv[EPC], knv[EPC], vnv[EPC];
    const size_t at = (size_t)b * a.ld + h * 64 + ch * EPC;
    load_f32_slabs<EPC>(a.q + at, a.nslab, a.slab_stride, qv);
    load_f32_slabs<EPC>(a.knew + at, a.nslab, a.slab_stride, knv);
    load_f32_slabs<EPC>(a.vnew + at, a.nslab, a.slab_stride, vnv);
    int n = a.step ? *a.step : a.n_max;  // rows already cached
    n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
    const int tot = n + 1;
    const float scale2 = a.scale * 1.4426950408889634f;

    const size_t row0 = (size_t)(b * a.H + h) * a.Tmax;
    const uint8_t* kc = a.kcodes + row0 * 64 + ch * EPC;
    const uint8_t* vc = a.vcodes + row0 * 64 + ch * EPC;
    const float* ks = a.kscale + row0;
    const float* vs = a.vscale + row0;
    float* s = &sc[pib][0];

    auto load_batch = [&](const uint8_t* base, int j0, uint4 (&r)[U]) {
        if (n == 0) return;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            r[u] = ld_stream(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };
    // the scale of the key whose score this lane scales in batch j0 (position n: the register one, swapped in at the use)
    auto load_scale = [&](const float* base, int j0) { return n == 0 ? 0.f : base[j0 + lane < n ? j0 + lane : n - 1]; };

    uint4 cur[U] = {}, nxt[U] = {}, vfirst[U] = {};
    float kcur = 0.f, knxt = 0.f, vcur = 0.f, vnxt = 0.f;
    if (jfirst < tot) {
        load_batch(kc, jfirst, cur);
        load_batch(vc, jfirst, vfirst);
        kcur = load_scale(ks, jfirst);
        vcur = load_scale(vs, jfirst);
    }

    // ---- this step's row: codes and scales in registers, one store by the pair's first wave
    uint4 kn8, vn8;
    const float ksn = quant_row16(knv, kn8);
    const float vsn = quant_row16(vnv, vn8);
    if (active && part == 0 && sub == 0) {
        *(uint4*)(a.kcodes + (row0 + n) * 64 + ch * EPC) = kn8;
        *(uint4*)(a.vcodes + (row0 + n) * 64 + ch * EPC) = vn8;
        if (ch == 0) {
            a.kscale[row0 + n] = ksn;
            a.vscale[row0 + n] = vsn;
        }
    }

    // ---- scores: raw dots of the batch, then one key per lane scaled
    float mx = kNegD;
    for (int j0 = jfirst; j0 < tot; j0 += jstep) {
        if (j0 + jstep < tot) {
            load_batch(kc, j0 + jstep, nxt);
            knxt = load_scale(ks, j0 + jstep);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float kv[EPC];
            unpack_fp8x16(j == n ? kn8 : cur[u], kv);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) d = fmaf(qv[e], kv[e], d);
            d = group4_sum(d);
            if (ch == 0 && j < tot) s[j] = d;
        }
        if (j0 + lane < tot) {
            const float sv = (s[j0 + lane] * (j0 + lane == n ? ksn : kcur)) * scale2;
            s[j0 + lane] = sv;
            mx = fmaxf(mx, sv);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        kcur = knxt;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = vfirst[u];
    mx = wave_max(mx);
    if (NSPLIT > 1) {
        if (lane == 0) red_m[wave] = mx;
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NSPLIT; ++p) mx = fmaxf(mx, red_m[pib * NSPLIT + p]);
    }

    // ---- o = sum_j p_j vscale_j codes_j, row sum of the unscaled p_j
    float lsum = 0.f;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    for (int j0 = jfirst; j0 < tot; j0 += jstep) {
        if (j0 + jstep < tot) {
            load_batch(vc, j0 + jstep, nxt);
            vnxt = load_scale(vs, j0 + jstep);
        }
        if (j0 + lane < tot) {
            const float p = exp2f(s[j0 + lane] - mx);
            lsum += p;
            s[j0 + lane] = p * (j0 + lane == n ? vsn : vcur);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            float vv[EPC];
            unpack_fp8x16(j == n ? vn8 : cur[u], vv);
            const float p = j < tot ? s[j] : 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(p, vv[e], acc[e]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        vcur = vnxt;
    }
    lsum = wave_sum_sel<sizeof(TO) == 2>(lsum);
    if (NSPLIT > 1) {
        if (lane == 0) red_l[wave] = lsum;
        __syncthreads();
        lsum = 0.f;
#pragma unroll
        for (int p = 0; p < NSPLIT; ++p) lsum += red_l[pib * NSPLIT + p];
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) {  // xor 4 .. 32 butterfly over the key sub-groups
        acc[e] += xor_lane_f32<4>(acc[e]);
        acc[e] += xor_lane_f32<8>(acc[e]);
        acc[e] += xor_lane_f32<16>(acc[e]);
        acc[e] += xor_lane_f32<32>(acc[e]);
    }
    if (NSPLIT > 1) {  // combine the partial outputs of the pair's waves in wave order
        if (sub == 0) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) red_acc[wave][ch * EPC + e] = acc[e];
        }
        __syncthreads();
        if (part == 0 && sub == 0) {
#pragma unroll
            for (int p = 1; p < NSPLIT; ++p)
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += red_acc[pib * NSPLIT + p][ch * EPC + e];
        }
    }
    if (active && part == 0 && sub == 0) {
        const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] *= inv;
        store_out16<TO>((TO*)a.out + (size_t)b * a.o_ld + h * 64 + ch * EPC, acc);
    }
}

// ---- the multi-query form (dimx/kv8.py attention_rows): the S <= 16 queries of a clip against that clip's codes on the matrix cores,
// one wave per (clip, head), the codes read once for all S.  v_mfma_f32_16x16x32_bf16 throughout; a tile is 32 keys:
//   * load shape: lane (g = lane >> 4, i = lane & 15) loads the 16 codes [16 g, 16 g + 16) of key j0 + 16 t + i (t = 0, 1) -- still 16 keys
//     x 64 B = 1 KiB per wave-wide load -- and converts them to bf16 in registers (every e4m3fn value is a bf16 value: exact);
//   * scores transposed, S^T = K . Q^T: the K fragment of k-step s is the lane's codes 8 s .. 8 s + 7, the Q fragment the same
//     elements of query i's row (rows i >= S are zero), so both operands contract in the same permuted order.  The tile's result has
//     the query on the lane (column i) and the keys j0 + 16 t + 4 g + r in its registers: kscale, the softmax scale and the mask are
//     applied to it in f32 (one scale per key, never folded into an operand), the softmax is online over tiles, and the row sum is
//     accumulated from the unrounded f32 p;
//   * p * vscale, rounded once to bf16, is ALREADY the B operand of O^T = V^T . P^T with k-slot 8 g + 4 t + r <-> key j0 + 16 t + 4 g + r
//     (the accumulator-as-operand idiom); V^T's fragment wants one d and eight keys per lane while the codes lie key-major, so the
//     wave stores its bf16 V tile [32 keys][64 d] to its own LDS rows and reads it back with ds_read_b64_tr_b16 (attention_tr.hip has
//     the lane map): group g's read t addresses keys 16 t + 4 g .. + 3 of the 16 d of block c and hands lane i column i of them;
//   * NP = 3 (the exact form): q and p * vscale enter as three bf16 planes each (x = x0 + x1 + x2 exactly, the gemm_x3.hip idea);
//     a bf16 plane times an exact bf16 code is exact in f32, so the result is the f32 one up to accumulation order.
// Loads are clamped to row n - 1 and slots at or past n get p = 0, so nothing at or past the bound is read; padded query rows are
// never stored.  One wave per pair whatever the batch: a slice of clips has the whole batch's bits.  No atomics, no block barrier.
typedef uint32_t u32x4_mq __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_mq __attribute__((ext_vector_type(2)));
constexpr int kMqVld = 144;   // bytes per key row of a wave's V tile in LDS: 64 bf16 and 16 bytes of padding

__device__ __forceinline__ void codes_to_bf16x16(const uint4& u, u32x4_mq (&f)[2]) {
    float v[16];
    unpack_fp8x16(u, v);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        f[i] = u32x4_mq{pack_bf16x2(v[8 * i], v[8 * i + 1]), pack_bf16x2(v[8 * i + 2], v[8 * i + 3]), pack_bf16x2(v[8 * i + 4], v[8 * i + 5]),
                        pack_bf16x2(v[8 * i + 6], v[8 * i + 7])};
}
// the eight transposing reads of a V tile: t[2 c + tt] = column (lane & 15) of the [4 keys][16 d] block at keys 16 tt + 4 g .., d 16 c ..
__device__ __forceinline__ void lds_read_v_tr16(uint32_t addr, u32x2_mq (&t)[8]) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %8\n\t"
        "ds_read_b64_tr_b16 %1, %8 offset:2304\n\t"
        "ds_read_b64_tr_b16 %2, %8 offset:32\n\t"
        "ds_read_b64_tr_b16 %3, %8 offset:2336\n\t"
        "ds_read_b64_tr_b16 %4, %8 offset:64\n\t"
        "ds_read_b64_tr_b16 %5, %8 offset:2368\n\t"
        "ds_read_b64_tr_b16 %6, %8 offset:96\n\t"
        "ds_read_b64_tr_b16 %7, %8 offset:2400\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])
        : "v"(addr)
        : "memory");
}
static_assert(16 * kMqVld == 2304, "lds_read_v_tr16's offsets are 16 key rows apart");

// NP bf16 planes of eight floats, plane p in f[p]: x = f[0] + f[1] + .. exactly while the remainders are representable
template <int NP> __device__ __forceinline__ void bf16_planes8(float (&x)[8], u32x4_mq (&f)[NP]) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t word = pack_bf16x2(x[2 * w], x[2 * w + 1]);
            f[p][w] = word;
            if (p + 1 < NP) {
                x[2 * w] -= bf16_to_f32((uint16_t)(word & 0xffffu));
                x[2 * w + 1] -= bf16_to_f32((uint16_t)(word >> 16));
            }
        }
}

template <typename TO, int NP>
__global__ __launch_bounds__(256) void decode_attn_mq_kv8_kernel(const Kv8AttnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char vt[4][32 * kMqVld];
    __shared__ __attribute__((aligned(16))) float sl[4][64];   // the tile's K scales | V scales, one per key
    __shared__ __attribute__((aligned(16))) float sk[4][32];   // the tile's key states: 0 a key, 1 masked, 2 at or past the bound
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= a.B * a.H) return;   // whole waves leave; nothing below meets another wave
    const int b = pair / a.H, h = pair % a.H;
    const int S = a.rows_per_clip;
    const int qi = lane & 15, g = lane >> 4;
    const bool qlive = qi < S;
    const size_t qrow = (size_t)b * S + (qlive ? qi : 0);

    u32x4_mq qf[NP][2];
    {
        float qv[16];
        if (a.q_bf16) load_row16<bf16>((const bf16*)(const void*)a.q + qrow * a.q_ld + h * 64 + g * 16, qv);
        else load_f32_slabs<16>(a.q + qrow * a.q_ld + h * 64 + g * 16, a.nslab, a.slab_stride, qv);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float x[8];
            u32x4_mq f[NP];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = qlive ? qv[8 * i + e] : 0.f;
            bf16_planes8<NP>(x, f);
#pragma unroll
            for (int p = 0; p < NP; ++p) qf[p][i] = f[p];
        }
    }
    int n = a.n_keys;
    if (a.win) n = win_keys(*a.step, a.lookahead, a.n_keys);
    const float scale2 = a.scale * 1.4426950408889634f;

    const size_t row0 = (size_t)(b * a.H + h) * a.Tmax;
    const uint8_t* kc = a.kcodes + row0 * 64 + g * 16;
    const uint8_t* vc = a.vcodes + row0 * 64 + g * 16;
    const float* ks = a.kscale + row0;
    const float* vs = a.vscale + row0;
    const uint8_t* km = a.kmask ? a.kmask + (size_t)b * a.kmask_ld : nullptr;
    unsigned char* vrow = &vt[wave][0];
    const uint32_t vaddr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)vrow + (4 * g + (qi >> 2)) * kMqVld + (qi & 3) * 8;

    auto load_tile = [&](const uint8_t* base, int j0, uint4 (&r)[2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = j0 + 16 * t + qi;
            r[t] = ld_stream(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };
    // lanes 0 .. 31: K scale and state of key j0 + lane; lanes 32 .. 63: V scale of key j0 + lane - 32
    auto load_side = [&](int j0, float& sc, float& st) {
        const int j = j0 + (lane & 31), jc = j < n ? j : n - 1;
        sc = lane < 32 ? ks[jc] : vs[jc];
        st = j >= n ? 2.f : ((km && lane < 32 && km[jc] == 0) ? 1.f : 0.f);
    };

    uint4 kcur[2] = {}, vcur[2] = {}, knxt[2] = {}, vnxt[2] = {};
    float scc = 0.f, scn = 0.f, stc = 2.f, stn = 2.f;
    load_tile(kc, 0, kcur);
    load_tile(vc, 0, vcur);
    load_side(0, scc, stc);

    float m_run = kNegD, lsum = 0.f;
    f32x4_t o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < n; j0 += 32) {
        if (j0 + 32 < n) {
            load_tile(kc, j0 + 32, knxt);
            load_tile(vc, j0 + 32, vnxt);
            load_side(j0 + 32, scn, stn);
        }
        sl[wave][lane] = scc;
        if (lane < 32) sk[wave][lane] = stc;
#pragma unroll
        for (int t = 0; t < 2; ++t) {   // the V tile, bf16, key-major
            u32x4_mq f[2];
            codes_to_bf16x16(vcur[t], f);
            unsigned char* p = vrow + (16 * t + qi) * kMqVld + g * 32;
            *(u32x4_mq*)p = f[0];
            *(u32x4_mq*)(p + 16) = f[1];
        }
        // ---- scores of the tile: S^T[key][query]
        f32x4_t sacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            u32x4_mq kf[2];
            codes_to_bf16x16(kcur[t], kf);
            sacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = NP - 1; p >= 0; --p)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[s]), __builtin_bit_cast(bf16x8_t, qf[p][s]),
                                                                      sacc[t], 0, 0, 0);
        }
        float sv[8], vsc[8];
        bool live[8];
        float tmax = kNegD;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float4 k4 = *(const float4*)&sl[wave][16 * t + 4 * g];
            const float4 v4 = *(const float4*)&sl[wave][32 + 16 * t + 4 * g];
            const float4 s4 = *(const float4*)&sk[wave][16 * t + 4 * g];
            const float kk[4] = {k4.x, k4.y, k4.z, k4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = (sacc[t][r] * kk[r]) * scale2;
                if (ss[r] == 1.f) x = kNegD;
                live[4 * t + r] = ss[r] < 2.f;
                sv[4 * t + r] = x;
                vsc[4 * t + r] = vv[r];
                if (live[4 * t + r]) tmax = fmaxf(tmax, x);
            }
        }
        tmax = fmaxf(tmax, xor_lane_f32<16>(tmax));
        tmax = fmaxf(tmax, xor_lane_f32<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        lsum *= alpha;
        float pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = live[e] ? exp2f(sv[e] - m_new) : 0.f;
            lsum += p;
            pv[e] = live[e] ? p * vsc[e] : 0.f;
        }
        u32x4_mq pf[NP];
        bf16_planes8<NP>(pv, pf);
        // ---- O^T[d][query] += V^T . P^T
        u32x2_mq tv[8];
        lds_read_v_tr16(vaddr, tv);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x4_mq vf = {tv[2 * c][0], tv[2 * c][1], tv[2 * c + 1][0], tv[2 * c + 1][1]};
            o[c] *= alpha;
#pragma unroll
            for (int p = NP - 1; p >= 0; --p)
                o[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf), __builtin_bit_cast(bf16x8_t, pf[p]), o[c], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) { kcur[t] = knxt[t]; vcur[t] = vnxt[t]; }
        scc = scn;
        stc = stn;
    }
    lsum += xor_lane_f32<16>(lsum);
    lsum += xor_lane_f32<32>(lsum);
    const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
    if (qlive) {   // lane: query qi, d 16 c + 4 g .. + 3
        TO* op = (TO*)a.out + qrow * a.o_ld + h * 64 + 4 * g;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float r0 = o[c][0] * inv, r1 = o[c][1] * inv, r2 = o[c][2] * inv, r3 = o[c][3] * inv;
            if constexpr (sizeof(TO) == 2) *(uint2*)(op + 16 * c) = make_uint2(pack_bf16x2(r0, r1), pack_bf16x2(r2, r3));
            else *(float4*)(op + 16 * c) = make_float4(r0, r1, r2, r3);
        }
    }
}

}  // namespace

int launch_decode_attn_mq_kv8(const Kv8AttnArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.kcodes && a.kscale && a.vcodes && a.vscale && a.out, DIMX_ERR_ARG, "decode_attn_kv8_multi: null operand");
    DIMX_REQUIRE(a.out_dtype == DIMX_BF16 || a.out_dtype == DIMX_F32, DIMX_ERR_ARG, "decode_attn_kv8_multi: out_dtype %d", a.out_dtype);
    const int S = a.rows_per_clip;
    DIMX_REQUIRE(S == 2 || S == 4 || S == 5 || S == 8 || S == 10, DIMX_ERR_ARG, "decode_attn_kv8_multi: rows_per_clip %d not in {2,4,5,8,10}", S);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.Tmax >= 1, DIMX_ERR_ARG, "decode_attn_kv8_multi: empty shape");
    DIMX_REQUIRE(a.n_keys >= 1 && a.n_keys <= a.Tmax && a.n_keys <= kMaxKeys, DIMX_ERR_ARG,
                 "decode_attn_kv8_multi: n_keys %d outside 1 .. min(Tmax = %d, %d)", a.n_keys, a.Tmax, kMaxKeys);
    const long rows = (long)a.B * S;
    if (a.q_bf16)
        DIMX_REQUIRE(a.nslab == 1 && a.q_ld % 8 == 0, DIMX_ERR_ARG, "decode_attn_kv8_multi: bf16 q is one row array (nslab = %d) with q_ld = %d a multiple of 8",
                     a.nslab, a.q_ld);
    else
        DIMX_REQUIRE(a.nslab >= 1 && a.nslab <= 8 && (a.nslab == 1 || a.slab_stride >= rows * a.q_ld) && a.q_ld % 4 == 0 && a.slab_stride % 4 == 0,
                     DIMX_ERR_ARG, "decode_attn_kv8_multi: nslab=%d (1..8) with slabs %ld apart, q_ld=%d (16-byte multiples)", a.nslab, a.slab_stride, a.q_ld);
    const int oal = a.out_dtype == DIMX_BF16 ? 8 : 4;
    DIMX_REQUIRE(a.q_ld >= a.H * 64 && a.o_ld >= a.H * 64 && a.o_ld % oal == 0, DIMX_ERR_ARG,
                 "decode_attn_kv8_multi: q_ld=%d o_ld=%d (rows of at least H*64, o_ld a 16-byte multiple)", a.q_ld, a.o_ld);
    DIMX_REQUIRE((uintptr_t)a.q % 16 == 0 && (uintptr_t)a.kcodes % 16 == 0 && (uintptr_t)a.vcodes % 16 == 0 && (uintptr_t)a.out % 16 == 0 &&
                     (uintptr_t)a.kscale % 4 == 0 && (uintptr_t)a.vscale % 4 == 0,
                 DIMX_ERR_ARG, "decode_attn_kv8_multi: misaligned operand (q / codes / out 16 bytes, scales 4)");
    DIMX_REQUIRE(a.kmask == nullptr || a.kmask_ld >= a.n_keys, DIMX_ERR_ARG, "decode_attn_kv8_multi: kmask_ld=%d < n_keys=%d", a.kmask_ld, a.n_keys);
    DIMX_REQUIRE(!a.win || a.step != nullptr, DIMX_ERR_ARG, "decode_attn_kv8_multi: the windowed form needs a step counter");
    const long pairs = (long)a.B * a.H;
    DIMX_REQUIRE(pairs <= 0x7fffffffL && rows * a.q_ld <= 0x7fffffffffL, DIMX_ERR_ARG, "decode_attn_kv8_multi: %ld (clip, head) pairs", pairs);
    // one wave per (clip, head) in both forms, whatever the batch: a slice of clips reproduces the whole batch's rows bit for bit
    dim3 grid((unsigned)((pairs + 3) / 4)), block(256);
#define KV8_MQ(TT)                                                                                    \
    do {                                                                                              \
        if (a.exact) hipLaunchKernelGGL((decode_attn_mq_kv8_kernel<TT, 3>), grid, block, 0, s, a);    \
        else hipLaunchKernelGGL((decode_attn_mq_kv8_kernel<TT, 1>), grid, block, 0, s, a);            \
    } while (0)
    if (a.out_dtype == DIMX_BF16) KV8_MQ(bf16);
    else KV8_MQ(float);
#undef KV8_MQ
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_kv8_quant(int dtype, const void* cache, int B, int H, int Tp, int T, uint8_t* codes, float* scales, hipStream_t s, int cache_T) {
    DIMX_REQUIRE(dtype == DIMX_BF16 || dtype == DIMX_F32, DIMX_ERR_ARG, "kv8_quantize: dtype %d", dtype);
    DIMX_REQUIRE(cache && codes && scales, DIMX_ERR_ARG, "kv8_quantize: null operand");
    DIMX_REQUIRE((uintptr_t)cache % 16 == 0 && (uintptr_t)codes % 16 == 0 && (uintptr_t)scales % 4 == 0, DIMX_ERR_ARG,
                 "kv8_quantize: misaligned operand (cache / codes 16 bytes, scales 4)");
    DIMX_REQUIRE(B >= 1 && H >= 1 && T >= 1 && T <= Tp, DIMX_ERR_ARG, "kv8_quantize: B=%d H=%d T=%d Tp=%d (need 1 <= T <= Tp)", B, H, T, Tp);
    const int Tc = cache_T > 0 ? cache_T : Tp;
    DIMX_REQUIRE(T <= Tc, DIMX_ERR_ARG, "kv8_quantize: T=%d rows of a cache that holds %d per (clip, head)", T, Tc);
    const long rows = (long)B * H * T;
    const long blocks = (rows * 4 + 255) / 256;
    DIMX_REQUIRE(blocks <= 0x7fffffffL, DIMX_ERR_ARG, "kv8_quantize: %ld rows", rows);
    if (dtype == DIMX_BF16)
        hipLaunchKernelGGL((kv8_quant_kernel<bf16>), dim3((unsigned)blocks), dim3(256), 0, s, (const bf16*)cache, rows, Tc, Tp, T, codes, scales);
    else
        hipLaunchKernelGGL((kv8_quant_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)cache, rows, Tc, Tp, T, codes, scales);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_kv8_append(const Kv8AppendArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.dtype == DIMX_BF16 || a.dtype == DIMX_F32, DIMX_ERR_ARG, "kv8_append: dtype %d", a.dtype);
    DIMX_REQUIRE(a.depth >= 1 && a.depth <= 8, DIMX_ERR_ARG, "kv8_append: depth %d outside 1 .. 8", a.depth);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.c >= 1 && a.n0 >= 0, DIMX_ERR_ARG, "kv8_append: B=%d H=%d n0=%d c=%d (need B, H, c >= 1 and n0 >= 0)", a.B,
                 a.H, a.n0, a.c);
    DIMX_REQUIRE(a.Tp >= 1 && a.Tp <= kMaxKeys && a.Tc >= 1, DIMX_ERR_ARG, "kv8_append: Tp=%d outside 1 .. %d or Tc=%d < 1", a.Tp, kMaxKeys, a.Tc);
    DIMX_REQUIRE((long)a.n0 + a.c <= a.Tc && (long)a.n0 + a.c <= a.Tp, DIMX_ERR_ARG,
                 "kv8_append: rows %d .. %ld of caches that hold %d and code planes that hold %d per (clip, head)", a.n0, (long)a.n0 + a.c - 1, a.Tc,
                 a.Tp);
    for (int i = 0; i < 2 * a.depth; ++i) {
        DIMX_REQUIRE(a.cache[i] && a.codes[i] && a.scales[i], DIMX_ERR_ARG, "kv8_append: null operand (layer %d %s)", i / 2, i % 2 ? "V" : "K");
        DIMX_REQUIRE((uintptr_t)a.cache[i] % 16 == 0 && (uintptr_t)a.codes[i] % 16 == 0 && (uintptr_t)a.scales[i] % 4 == 0, DIMX_ERR_ARG,
                     "kv8_append: misaligned operand (layer %d %s; cache / codes 16 bytes, scales 4)", i / 2, i % 2 ? "V" : "K");
    }
    const long rows = (long)a.B * a.H * a.c;
    const long blocks = (rows * 4 + 255) / 256;
    DIMX_REQUIRE(blocks <= 0x7fffffffL, DIMX_ERR_ARG, "kv8_append: %ld rows per cache", rows);
    const dim3 grid((unsigned)blocks, (unsigned)(2 * a.depth)), block(256);
    if (a.dtype == DIMX_BF16) hipLaunchKernelGGL((kv8_append_kernel<bf16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((kv8_append_kernel<float>), grid, block, 0, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_decode_attn_self_kv8(const Kv8SelfArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.knew && a.vnew && a.kcodes && a.kscale && a.vcodes && a.vscale && a.out, DIMX_ERR_ARG, "decode_attn_self_kv8: null operand");
    DIMX_REQUIRE(a.out_dtype == DIMX_BF16 || a.out_dtype == DIMX_F32, DIMX_ERR_ARG, "decode_attn_self_kv8: out_dtype %d", a.out_dtype);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.Tmax >= 1, DIMX_ERR_ARG, "decode_attn_self_kv8: empty shape");
    DIMX_REQUIRE(a.n_max >= 0 && a.n_max < a.Tmax && a.n_max < kMaxKeys, DIMX_ERR_ARG,
                 "decode_attn_self_kv8: %d cached rows outside 0 .. min(Tmax = %d, %d) - 1", a.n_max, a.Tmax, kMaxKeys);
    DIMX_REQUIRE(a.nslab >= 1 && a.nslab <= 8 && (a.nslab == 1 || a.slab_stride >= (long)a.B * a.ld), DIMX_ERR_ARG,
                 "decode_attn_self_kv8: nslab=%d (1..8) with slabs %ld apart", a.nslab, a.slab_stride);
    const int oal = a.out_dtype == DIMX_BF16 ? 8 : 4;
    DIMX_REQUIRE(a.ld >= a.H * 64 && a.o_ld >= a.H * 64 && a.ld % 4 == 0 && a.slab_stride % 4 == 0 && a.o_ld % oal == 0, DIMX_ERR_ARG,
                 "decode_attn_self_kv8: ld=%d o_ld=%d slab_stride=%ld (rows of at least H*64, 16-byte multiples)", a.ld, a.o_ld, a.slab_stride);
    DIMX_REQUIRE((uintptr_t)a.q % 16 == 0 && (uintptr_t)a.knew % 16 == 0 && (uintptr_t)a.vnew % 16 == 0 && (uintptr_t)a.kcodes % 16 == 0 &&
                     (uintptr_t)a.vcodes % 16 == 0 && (uintptr_t)a.out % 16 == 0 && (uintptr_t)a.kscale % 4 == 0 && (uintptr_t)a.vscale % 4 == 0,
                 DIMX_ERR_ARG, "decode_attn_self_kv8: misaligned operand (q / k / v / codes / out 16 bytes, scales 4)");
    // waves per (row, head): launch_decode_attn's rule -- on an f32 handle a function of the cache length only
    const int pairs = a.B * a.H;
    int nsplit = 1;
    if (pairs * 2 <= 3072) nsplit = 2;
    if (pairs * 4 <= 3072) nsplit = 4;
    if (a.out_dtype != DIMX_BF16) nsplit = a.Tmax >= 1024 ? 4 : (a.Tmax >= 512 ? 2 : 1);
    if (a.force_nsplit == 1 || a.force_nsplit == 2 || a.force_nsplit == 4) nsplit = a.force_nsplit;
    dim3 grid(ceil_div(pairs, 4 / nsplit)), block(256);
#define KV8S_NS(TT)                                                                                                       \
    do {                                                                                                                  \
        if (nsplit == 4) hipLaunchKernelGGL((decode_attn_self_kv8_kernel<TT, 4>), grid, block, 0, s, a);                  \
        else if (nsplit == 2) hipLaunchKernelGGL((decode_attn_self_kv8_kernel<TT, 2>), grid, block, 0, s, a);             \
        else hipLaunchKernelGGL((decode_attn_self_kv8_kernel<TT, 1>), grid, block, 0, s, a);                              \
    } while (0)
    if (a.out_dtype == DIMX_BF16) KV8S_NS(bf16);
    else KV8S_NS(float);
#undef KV8S_NS
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int launch_decode_attn_kv8(const Kv8AttnArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.kcodes && a.kscale && a.vcodes && a.vscale && a.out, DIMX_ERR_ARG, "decode_attn_kv8: null operand");
    DIMX_REQUIRE(a.out_dtype == DIMX_BF16 || a.out_dtype == DIMX_F32, DIMX_ERR_ARG, "decode_attn_kv8: out_dtype %d", a.out_dtype);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.Tmax >= 1, DIMX_ERR_ARG, "decode_attn_kv8: empty shape");
    DIMX_REQUIRE(a.n_keys >= 1 && a.n_keys <= a.Tmax && a.n_keys <= kMaxKeys, DIMX_ERR_ARG,
                 "decode_attn_kv8: n_keys %d outside 1 .. min(Tmax = %d, %d)", a.n_keys, a.Tmax, kMaxKeys);
    DIMX_REQUIRE(a.nslab >= 1 && a.nslab <= 8 && (a.nslab == 1 || a.slab_stride >= (long)a.B * a.q_ld), DIMX_ERR_ARG,
                 "decode_attn_kv8: nslab=%d (1..8) with slabs %ld apart", a.nslab, a.slab_stride);
    const int oal = a.out_dtype == DIMX_BF16 ? 8 : 4;
    DIMX_REQUIRE(a.q_ld >= a.H * 64 && a.o_ld >= a.H * 64 && a.q_ld % 4 == 0 && a.slab_stride % 4 == 0 && a.o_ld % oal == 0, DIMX_ERR_ARG,
                 "decode_attn_kv8: q_ld=%d o_ld=%d slab_stride=%ld (rows of at least H*64, 16-byte multiples)", a.q_ld, a.o_ld, a.slab_stride);
    DIMX_REQUIRE((uintptr_t)a.q % 16 == 0 && (uintptr_t)a.kcodes % 16 == 0 && (uintptr_t)a.vcodes % 16 == 0 && (uintptr_t)a.out % 16 == 0 &&
                     (uintptr_t)a.kscale % 4 == 0 && (uintptr_t)a.vscale % 4 == 0,
                 DIMX_ERR_ARG, "decode_attn_kv8: misaligned operand (q / codes / out 16 bytes, scales 4)");
    DIMX_REQUIRE(a.kmask == nullptr || a.kmask_ld >= a.n_keys, DIMX_ERR_ARG, "decode_attn_kv8: kmask_ld=%d < n_keys=%d", a.kmask_ld, a.n_keys);
    DIMX_REQUIRE(!a.win || a.step != nullptr, DIMX_ERR_ARG, "decode_attn_kv8: the windowed form needs a step counter");
    // waves per (clip, head): launch_decode_attn's rule -- on an f32 handle a function of the cache length only, so a shard of a
    // batch reproduces the whole batch's rows bit for bit
    const int pairs = a.B * a.H;
    int nsplit = 1;
    if (pairs * 2 <= 3072) nsplit = 2;
    if (pairs * 4 <= 3072) nsplit = 4;
    if (a.out_dtype != DIMX_BF16) nsplit = a.Tmax >= 1024 ? 4 : (a.Tmax >= 512 ? 2 : 1);
    if (a.force_nsplit == 1 || a.force_nsplit == 2 || a.force_nsplit == 4) nsplit = a.force_nsplit;
    dim3 grid(ceil_div(pairs, 4 / nsplit)), block(256);
#define KV8_LAUNCH(TT, NS, WW) hipLaunchKernelGGL((decode_attn_kv8_kernel<TT, NS, WW>), grid, block, 0, s, a)
#define KV8_NS(TT, WW)                              \
    do {                                            \
        if (nsplit == 4) KV8_LAUNCH(TT, 4, WW);     \
        else if (nsplit == 2) KV8_LAUNCH(TT, 2, WW); \
        else KV8_LAUNCH(TT, 1, WW);                 \
    } while (0)
    if (a.out_dtype == DIMX_BF16) { if (a.win) KV8_NS(bf16, true); else KV8_NS(bf16, false); }
    else { if (a.win) KV8_NS(float, true); else KV8_NS(float, false); }
#undef KV8_NS
#undef KV8_LAUNCH
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
