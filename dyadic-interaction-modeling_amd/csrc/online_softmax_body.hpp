// online_softmax_body.hpp -- one query against one key batch held in registers, with the running state of an online softmax.
// In a header because two kernels run it: append_attn_kernel (stream_attn.hip, the encoder increments of a streaming session)
// and win_attn_kernel (win_attn.hip, the windowed cross attention of many queries).  Both rest on the same property: the
// operation sequence of a query depends on its own limit and on the batch grid counted from key 0, on nothing else.
#pragma once
#include "decode_attn_body.hpp"

namespace dimx {
namespace {

// per-query running state of the online softmax
template <int EPC> struct QState {
    float m, l;
    float acc[EPC];
};

// Query `qrow` (f32 row in LDS, this lane's chunk at qrow + ch * EPC) against one key batch held in registers.  lim = the last
// key the query may see; keys of the batch past it are left out of everything, and so is key u of this lane's sub-group when
// bit u of `keep` is clear (a key mask; all ones without one).  The caller guarantees j0 <= lim.  A batch without a visible kept
// key leaves the state as it was: the new maximum is the old one and alpha = 1.
template <typename T, int EPC, int LPK, int KPI, int U>
__device__ __forceinline__ void query_batch(QState<EPC>& st, const float* qrow, const uint4 (&kb)[U], const uint4 (&vb)[U], int j0, int sub,
                                            int lim, float scale2, unsigned keep = ~0u) {
    float qv[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) qv[e] = qrow[e];
    float sv[U];
    float bm = kNegD;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float kv[EPC];
        cvt_chunk<T, EPC>(kb[u], kv);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) d = fmaf(qv[e], kv[e], d);
        d = LPK == 8 ? group8_sum(d) : row16_sum(d);
        const int j = j0 + u * KPI + sub;
        sv[u] = (j <= lim && (keep >> u & 1u)) ? d * scale2 : kNegD;
        bm = fmaxf(bm, sv[u]);
    }
    bm = wave_max(bm);
    const float mn = fmaxf(st.m, bm);
    const float alpha = exp2f(st.m - mn);   // first batch: st.m = kNegD -> 0, and l / acc are 0 anyway
    st.m = mn;
    st.l *= alpha;
#pragma unroll
    for (int e = 0; e < EPC; ++e) st.acc[e] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = j0 + u * KPI + sub;
        if (j <= lim && (keep >> u & 1u)) {
            float vv[EPC];
            cvt_chunk<T, EPC>(vb[u], vv);
            const float p = exp2f(sv[u] - mn);
            st.l += p;
#pragma unroll
            for (int e = 0; e < EPC; ++e) st.acc[e] = fmaf(p, vv[e], st.acc[e]);
        }
    }
}

// the key sub-groups' partial sums and accumulators of one query, xor LPK .. 32 butterfly; acc leaves normalised (a row without a
// kept key: zeros)
template <int EPC, int LPK> __device__ __forceinline__ void query_finish(const QState<EPC>& st, float (&acc)[EPC]) {
    float l = st.l;
    if (LPK <= 8) l += xor_lane_f32<8>(l);
    l += xor_lane_f32<16>(l);
    l += xor_lane_f32<32>(l);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        float v = st.acc[e];
        if (LPK <= 8) v += xor_lane_f32<8>(v);
        v += xor_lane_f32<16>(v);
        v += xor_lane_f32<32>(v);
        acc[e] = v;
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] *= inv;
}

}  // namespace
}  // namespace dimx
