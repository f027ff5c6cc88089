// stream_attn.hip -- append attention: the self attention of one encoder sublayer for the c new rows of every clip of a
// streaming session (stream.hip) over that layer's growing K / V cache.
//
// Per (clip, head): the c new k / v rows (f32, as the q/k/v projection wrote them) are rounded to the cache type and stored as
// cache rows [n0, n0 + c); then query i (0 <= i < c) attends over the cache rows 0 .. n0 + i, the new ones as the cache holds
// them -- a row sees the K / V every later row will see.  One pass over the cache serves all c queries: a key batch is loaded
// once and every query that may see it consumes it from registers (cdna_hip_programming.md, attention decode: up to 16 query
// rows per K/V pass; the kernel is a stream of the cache, the arithmetic rides along).
//
// Shape, after decode_attn_body.hpp: one wave per (clip, head), 4 per block; a key row is 16 bytes per lane over 8 (bf16) / 16
// (f32) lanes, U = 4 wave-wide loads make a batch of 32 / 16 keys, the next batch's K and V loads are in flight while the
// current one is consumed; fixed orders, no atomics.  The softmax runs online, batch by batch (running maximum, rescaled sum
// and accumulator per query), because c score rows of up to 2048 keys do not fit the LDS.
//
// Two properties the session rests on (tests/test_gpu_stream.py):
//   * a row is a function of its own inputs.  Key batches start at multiples of the batch size counted from key 0, never from
//     n0; query i walks the batches 0 .. (n0 + i) / KB and inside a batch only the keys j <= n0 + i enter its maximum, sum and
//     accumulator (selects, not multiplications by zero).  That is the operation sequence the row would run alone (c = 1), in
//     any chunk and at any place in it: same bits.  The instantiations for 1 / 4 / 16 queries share one per-query body.
//   * no read past the frontier.  A load of key j >= n0 + c is redirected to row n0 + c - 1, and what a lane holds of a key
//     j > n0 + i never reaches query i.
#include "online_softmax_body.hpp"   // QState, query_batch: the per-query body, shared with win_attn.hip
#include "stages.hpp"

namespace dimx {
namespace {

// QM: the most queries per (clip, head) this instantiation holds state for (c <= QM)
template <typename T, int QM> __global__ __launch_bounds__(256) void append_attn_kernel(const AppendAttnArgs a) {
    constexpr int EPC = 16 / sizeof(T);
    constexpr int LPK = 64 / EPC;   // lanes per key: 8 (bf16) / 16 (f32)
    constexpr int KPI = 64 / LPK;   // keys per wave-wide load: 8 / 4
    constexpr int U = 4;
    constexpr int KB = U * KPI;     // keys per batch: 32 / 16
    __shared__ float qs[4][QM][64];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + wave;
    const bool active = pair < a.B * a.H;
    const int b = active ? pair / a.H : 0, h = active ? pair % a.H : 0;
    const int sub = lane / LPK, ch = lane % LPK;
    const int c = a.c, n0 = a.n0, n = n0 + c;
    T* kc = (T*)a.kcache + ((size_t)(b * a.H + h) * a.Tmax) * 64 + ch * EPC;
    T* vc = (T*)a.vcache + ((size_t)(b * a.H + h) * a.Tmax) * 64 + ch * EPC;

    // ---- the new rows: k / v rounded into the cache, q into the LDS (f32)
    for (int i = sub; i < c; i += KPI) {
        const size_t row = ((size_t)b * c + i) * a.ld + h * 64 + ch * EPC;
        float t[EPC];
        load_f32_chunk<EPC>(a.q + row, t);
#pragma unroll
        for (int e = 0; e < EPC; ++e) qs[wave][i][ch * EPC + e] = t[e];
        if (active) {
            load_f32_chunk<EPC>(a.k + row, t);
            store_chunk<T, EPC>(kc + (size_t)(n0 + i) * 64, t);
            load_f32_chunk<EPC>(a.v + row, t);
            store_chunk<T, EPC>(vc + (size_t)(n0 + i) * 64, t);
        }
    }
    // the block's cache stores and LDS rows are visible to the block from here (the loads below read rows this wave stored
    // through other lanes; a workgroup's waves share one CU and its write-through L1)
    __syncthreads();

    auto load_batch = [&](const T* base, int j0, uint4 (&r)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            r[u] = *(const uint4*)(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };

    QState<EPC> st[QM];
#pragma unroll
    for (int i = 0; i < QM; ++i) {
        st[i].m = kNegD;
        st[i].l = 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) st[i].acc[e] = 0.f;
    }
    const float scale2 = a.scale * 1.4426950408889634f;

    uint4 kcur[U], vcur[U], knxt[U], vnxt[U];
    load_batch(kc, 0, kcur);
    load_batch(vc, 0, vcur);
    for (int j0 = 0; j0 < n; j0 += KB) {
        if (j0 + KB < n) {
            load_batch(kc, j0 + KB, knxt);
            load_batch(vc, j0 + KB, vnxt);
        }
#pragma unroll
        for (int i = 0; i < QM; ++i) {
            if (i < c && j0 <= n0 + i)   // wave-uniform
                query_batch<T, EPC, LPK, KPI, U>(st[i], &qs[wave][i][ch * EPC], kcur, vcur, j0, sub, n0 + i, scale2);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kcur[u] = knxt[u];
            vcur[u] = vnxt[u];
        }
    }

    // ---- per query: the key sub-groups' partial sums and accumulators, xor LPK .. 32 butterfly, then the row
#pragma unroll
    for (int i = 0; i < QM; ++i) {
        if (i < c) {
            float l = st[i].l;
            if (LPK <= 8) l += xor_lane_f32<8>(l);
            l += xor_lane_f32<16>(l);
            l += xor_lane_f32<32>(l);
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                float v = st[i].acc[e];
                if (LPK <= 8) v += xor_lane_f32<8>(v);
                v += xor_lane_f32<16>(v);
                v += xor_lane_f32<32>(v);
                acc[e] = v;
            }
            if (active && sub == 0) {
                const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] *= inv;
                store_chunk<T, EPC>((T*)a.out + ((size_t)b * c + i) * a.o_ld + h * 64 + ch * EPC, acc);
            }
        }
    }
}

}  // namespace

int launch_append_attn(const AppendAttnArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.k && a.v && a.kcache && a.vcache && a.out, DIMX_ERR_ARG, "append_attn: null operand");
    DIMX_REQUIRE(a.dtype == DIMX_F32 || a.dtype == DIMX_BF16, DIMX_ERR_ARG, "append_attn: unknown cache type %d", a.dtype);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.c >= 1 && a.c <= kAppendMaxRows, DIMX_ERR_ARG, "append_attn: B=%d H=%d c=%d (1 <= c <= %d)", a.B, a.H,
                 a.c, kAppendMaxRows);
    DIMX_REQUIRE(a.n0 >= 0 && a.Tmax <= kMaxKeys && a.n0 + a.c <= a.Tmax, DIMX_ERR_ARG,
                 "append_attn: rows [%d, %d) do not fit a cache of %d rows (at most %d)", a.n0, a.n0 + a.c, a.Tmax, kMaxKeys);
    DIMX_REQUIRE(a.ld >= a.H * 64 && a.ld % 4 == 0 && a.o_ld >= a.H * 64 && a.o_ld % 8 == 0, DIMX_ERR_ARG,
                 "append_attn: row strides %d / %d for %d heads", a.ld, a.o_ld, a.H);
    DIMX_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.kcache | (uintptr_t)a.vcache | (uintptr_t)a.out) % 16 == 0,
                 DIMX_ERR_ARG, "append_attn: operands must be 16-byte aligned");
    dim3 grid(ceil_div(a.B * a.H, 4)), block(256);
#define AA(TT)                                                                                  \
    do {                                                                                        \
        if (a.c == 1) hipLaunchKernelGGL((append_attn_kernel<TT, 1>), grid, block, 0, s, a);       \
        else if (a.c <= 4) hipLaunchKernelGGL((append_attn_kernel<TT, 4>), grid, block, 0, s, a);  \
        else hipLaunchKernelGGL((append_attn_kernel<TT, 16>), grid, block, 0, s, a);               \
    } while (0)
    if (a.dtype == DIMX_BF16) AA(bf16); else AA(float);
#undef AA
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
