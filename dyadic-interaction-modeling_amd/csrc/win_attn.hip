// win_attn.hip -- windowed cross attention for many queries: the cross attention of a teacher-forced decoder pass under the
// online bound (dimx/online.py), over the generation-layout K / V caches [B, H, Tp, 64] that dimx_encode_ctx(for_generate = 1)
// and a session's K / V append write.
//
// Query row i of a clip has position t = t0 + i and keeps key j iff j < win_keys(t, lookahead, n_keys) and the clip's keep-mask
// keeps j: what decode step t reads under WIN (decode_attn_body.hpp).  Nothing is appended to the cache.
//
// Shape, after stream_attn.hip, whose per-query body (online_softmax_body.hpp) it shares: one wave per (clip, head, tile of up to
// QM queries), 4 per block; a key batch (32 keys in bf16, 16 in f32) is loaded once into registers and every query of the tile
// that may see it consumes it, the next batch's K, V and mask bytes in flight; online softmax per query in f32; selects, not
// products with zero; fixed orders, no atomics, no LDS score rows.  A tile walks the batches below the bound of its LAST query
// only -- at lookahead 0 about half the key tiles of the launch.
//
// The properties of append_attn_kernel, for a bound that is no longer n0 + i (tests/test_gpu_win_prefill.py):
//   * a row is a function of its own inputs.  Key batches start at multiples of the batch size counted from key 0; query i walks
//     the batches below its own bound and inside a batch only its visible, kept keys enter maximum, sum and accumulator.  The
//     bits of a row do not depend on Lq, on t0 versus i for a fixed t0 + i, on its place in a tile or on the instantiation.
//   * no read past the bound of the tile's last query: a load of key j >= that bound is redirected to the last visible row, and
//     what a lane holds of a key outside query i's window never reaches query i.
//   * a row with no kept key gives zeros.
#include "online_softmax_body.hpp"
#include "stages.hpp"

namespace dimx {
namespace {

// QM: the queries of a tile
template <typename T, int QM> __global__ __launch_bounds__(256) void win_attn_kernel(const WinAttnArgs a) {
    constexpr int EPC = 16 / sizeof(T);
    constexpr int LPK = 64 / EPC;   // lanes per key: 8 (bf16) / 16 (f32)
    constexpr int KPI = 64 / LPK;   // keys per wave-wide load: 8 / 4
    constexpr int U = 4;
    constexpr int KB = U * KPI;     // keys per batch: 32 / 16
    __shared__ float qs[4][QM][64];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles = (a.Lq + QM - 1) / QM;
    const long item = (long)blockIdx.x * 4 + wave;   // the tiles of a (clip, head) are neighbours: they read the same K / V rows
    const bool active = item < (long)a.B * a.H * tiles;
    const int pair = active ? (int)(item / tiles) : 0, tile = active ? (int)(item % tiles) : 0;
    const int b = pair / a.H, h = pair % a.H;
    const int sub = lane / LPK, ch = lane % LPK;
    const int i0 = tile * QM;
    const int cq = a.Lq - i0 < QM ? a.Lq - i0 : QM;
    const T* kc = (const T*)a.kcache + ((size_t)(b * a.H + h) * a.Tp) * 64 + ch * EPC;
    const T* vc = (const T*)a.vcache + ((size_t)(b * a.H + h) * a.Tp) * 64 + ch * EPC;
    const uint8_t* km = a.kmask ? a.kmask + (size_t)b * a.kmask_ld : nullptr;

    for (int i = sub; i < cq; i += KPI) {
        float t[EPC];
        load_f32_chunk<EPC>(a.q + ((size_t)b * a.Lq + i0 + i) * a.ld + h * 64 + ch * EPC, t);
#pragma unroll
        for (int e = 0; e < EPC; ++e) qs[wave][i][ch * EPC + e] = t[e];
    }
    __syncthreads();

    // the keys query i of the tile may see; n: those of its last query, the tile's read bound (the bound grows with the position)
    auto bound = [&](int i) { return win_keys(a.t0 + i0 + i, a.lookahead, a.n_keys); };
    const int n = bound(cq - 1);

    auto load_batch = [&](const T* base, int j0, uint4 (&r)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            r[u] = *(const uint4*)(base + (size_t)(j < n ? j : n - 1) * 64);
        }
    };
    // bit u: the clip's mask keeps key j0 + u * KPI + sub
    auto load_keep = [&](int j0) -> unsigned {
        if (!km) return ~0u;
        unsigned keep = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPI + sub;
            keep |= (km[j < n ? j : n - 1] ? 1u : 0u) << u;
        }
        return keep;
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
    unsigned keep_cur, keep_nxt = ~0u;
    load_batch(kc, 0, kcur);
    load_batch(vc, 0, vcur);
    keep_cur = load_keep(0);
    for (int j0 = 0; j0 < n; j0 += KB) {
        if (j0 + KB < n) {
            load_batch(kc, j0 + KB, knxt);
            load_batch(vc, j0 + KB, vnxt);
            keep_nxt = load_keep(j0 + KB);
        }
#pragma unroll
        for (int i = 0; i < QM; ++i) {
            if (i < cq) {   // wave-uniform
                const int bi = bound(i);
                if (j0 < bi) query_batch<T, EPC, LPK, KPI, U>(st[i], &qs[wave][i][ch * EPC], kcur, vcur, j0, sub, bi - 1, scale2, keep_cur);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kcur[u] = knxt[u];
            vcur[u] = vnxt[u];
        }
        keep_cur = keep_nxt;
    }

#pragma unroll
    for (int i = 0; i < QM; ++i) {
        if (i < cq) {
            float acc[EPC];
            query_finish<EPC, LPK>(st[i], acc);
            if (active && sub == 0) store_chunk<T, EPC>((T*)a.out + ((size_t)b * a.Lq + i0 + i) * a.o_ld + h * 64 + ch * EPC, acc);
        }
    }
}

}  // namespace

int launch_win_attn(const WinAttnArgs& a, hipStream_t s) {
    DIMX_REQUIRE(a.q && a.kcache && a.vcache && a.out, DIMX_ERR_ARG, "win_attn: null operand");
    DIMX_REQUIRE(a.dtype == DIMX_F32 || a.dtype == DIMX_BF16, DIMX_ERR_ARG, "win_attn: unknown cache type %d", a.dtype);
    DIMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.Lq >= 1 && a.t0 >= 0 && a.t0 <= (1 << 30) && a.Lq <= (1 << 30), DIMX_ERR_ARG,
                 "win_attn: B=%d H=%d Lq=%d t0=%d", a.B, a.H, a.Lq, a.t0);
    DIMX_REQUIRE(a.n_keys >= 1 && a.n_keys <= a.Tp && a.n_keys <= kMaxKeys, DIMX_ERR_ARG, "win_attn: %d keys in a cache of %d rows (at most %d)",
                 a.n_keys, a.Tp, kMaxKeys);
    DIMX_REQUIRE(a.ld >= a.H * 64 && a.ld % 4 == 0 && a.o_ld >= a.H * 64 && a.o_ld % 8 == 0, DIMX_ERR_ARG,
                 "win_attn: row strides %d / %d for %d heads", a.ld, a.o_ld, a.H);
    DIMX_REQUIRE(!a.kmask || a.kmask_ld >= a.n_keys, DIMX_ERR_ARG, "win_attn: kmask_ld=%d < n_keys=%d", a.kmask_ld, a.n_keys);
    DIMX_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.kcache | (uintptr_t)a.vcache | (uintptr_t)a.out) % 16 == 0, DIMX_ERR_ARG,
                 "win_attn: operands must be 16-byte aligned");
    const int QM = a.Lq == 1 ? 1 : (a.Lq <= 4 ? 4 : 16);
    const long items = (long)a.B * a.H * ceil_div(a.Lq, QM);
    DIMX_REQUIRE(items <= (1L << 30), DIMX_ERR_ARG, "win_attn: %ld (clip, head, tile) items", items);
    dim3 grid((unsigned)((items + 3) / 4)), block(256);
#define WA(TT)                                                                               \
    do {                                                                                     \
        if (QM == 1) hipLaunchKernelGGL((win_attn_kernel<TT, 1>), grid, block, 0, s, a);       \
        else if (QM == 4) hipLaunchKernelGGL((win_attn_kernel<TT, 4>), grid, block, 0, s, a);  \
        else hipLaunchKernelGGL((win_attn_kernel<TT, 16>), grid, block, 0, s, a);              \
    } while (0)
    if (a.dtype == DIMX_BF16) WA(bf16); else WA(float);
#undef WA
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

}  // namespace dimx
