// common.hpp -- shared host/device helpers for libdimx_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>

#include "../../include/dimx.h"

namespace dimx {

// ---------------------------------------------------------------- error plumbing
void set_error(const char* fmt, ...);
const char* get_error();

#define DIMX_HIP(expr)                                                                       \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            dimx::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return DIMX_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

#define DIMX_REQUIRE(cond, code, ...)       \
    do {                                    \
        if (!(cond)) {                      \
            dimx::set_error(__VA_ARGS__);   \
            return (code);                  \
        }                                   \
    } while (0)

#define DIMX_TRY(expr)            \
    do {                          \
        int _s = (expr);          \
        if (_s != DIMX_OK) return _s; \
    } while (0)

// ---------------------------------------------------------------- element types
struct bf16 {
    uint16_t x;
};

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int kPerChunk = 4;  // elements per 16-byte chunk
    static constexpr int kId = DIMX_F32;
};
template <> struct Elem<bf16> {
    static constexpr int kPerChunk = 8;
    static constexpr int kId = DIMX_BF16;
};

inline size_t dtype_size(int dt) { return dt == DIMX_BF16 ? 2 : 4; }

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

__device__ __forceinline__ float bf16_to_f32(uint16_t u) {
    return __builtin_bit_cast(float, (uint32_t)u << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {  // round-to-nearest-even (v_cvt_pk_bf16_f32)
    __bf16 h = (__bf16)f;
    return __builtin_bit_cast(uint16_t, h);
}
// one v_cvt_pk_bf16_f32 (round-to-nearest-even, both halves); the scalar form above costs cvt + shift + or per pair
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const f32x2_t f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
}
inline uint16_t host_f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

template <typename T> __device__ __forceinline__ float load_as_f32(const T* p);
template <> __device__ __forceinline__ float load_as_f32<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load_as_f32<bf16>(const bf16* p) { return bf16_to_f32(p->x); }

template <typename T> __device__ __forceinline__ void store_from_f32(T* p, float v);
template <> __device__ __forceinline__ void store_from_f32<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_from_f32<bf16>(bf16* p, float v) { p->x = f32_to_bf16(v); }

// ---------------------------------------------------------------- activations
enum { ACT_NONE = 0, ACT_LEAKY = 1, ACT_GELU_TANH = 2, ACT_GELU_ERF = 3 };

__device__ __forceinline__ float apply_act(float x, int act) {
    switch (act) {
        case ACT_LEAKY: return x > 0.f ? x : 0.2f * x;
        case ACT_GELU_TANH: {
            // reference code/utils/base_model_util.py:81-94
            const float c = 0.7978845608028654f;
            float inner = c * (x + 0.044715f * (x * x * x));
            return x * (0.5f * (1.0f + tanhf(inner)));
        }
        case ACT_GELU_ERF: return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f));
        default: return x;
    }
}

// Wave-wide reductions on the DPP / readlane paths instead of __shfl_xor (which hipcc lowers to ds_bpermute_b32: an LDS
// round trip of ~100 cycles per step, six dependent steps per reduction -- the tail of every LayerNorm, softmax and
// sampler launch of the decode step).  Bit-identical to the ASCENDING xor butterfly (xor 1, 2, 4, ...): quad_perm IS
// xor 1 / xor 2; after those steps a quad holds one value, so the half-row and row mirrors deliver exactly the partner
// group's partial sum (a + b == b + a), and the four row totals are combined as (t0 + t1) + (t2 + t3) like the butterfly
// does in every lane (verified bit for bit by tools/ubench/dpp_check.hip).  All 64 lanes must be active.
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
__device__ __forceinline__ float lane_f32(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// v of lane (l ^ O) for O in {1, 2, 4, 8, 16, 32}, entirely on the vector ALU (what __shfl_xor means, without the
// ds_bpermute round trip): quad_perm for 1 / 2, two bank-masked row shifts for 4, row_ror:8 for 8, the gfx950 lane-swap
// instructions v_permlane16_swap / v_permlane32_swap for 16 / 32 (forms verified against __shfl_xor on the GPU:
// tools/ubench/dpp_check.hip).  All 64 lanes must be active.
__device__ __forceinline__ int wave_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
template <int O> __device__ __forceinline__ int xor_lane_i32(int v) {
    static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "xor distance");
    if constexpr (O == 1) {
        return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
    } else if constexpr (O == 2) {
        return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
    } else if constexpr (O == 4) {  // quads 0, 2 read lane + 4 (row_shl:4), quads 1, 3 read lane - 4 (row_shr:4)
        const int r = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xF, 0x5, false);
        return __builtin_amdgcn_update_dpp(r, v, 0x114, 0xF, 0xA, false);
    } else if constexpr (O == 8) {
        return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
    } else if constexpr (O == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        return ((wave_lane() >> 4) & 1) ? (int)r[0] : (int)r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        return wave_lane() >= 32 ? (int)r[0] : (int)r[1];
    }
}
template <int O> __device__ __forceinline__ float xor_lane_f32(float v) {
    return __builtin_bit_cast(float, xor_lane_i32<O>(__builtin_bit_cast(int, v)));
}

// sum over aligned groups of 8 (16) lanes, every lane of the group gets it; == the xor-1,2,4(,8) butterfly bit for bit
// when the operation is commutative, which + and max are
__device__ __forceinline__ float group8_sum(float v) {
    v += dpp_f32<DPP_XOR1>(v);
    v += dpp_f32<DPP_XOR2>(v);
    v += dpp_f32<DPP_HALF_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v = group8_sum(v);
    v += dpp_f32<DPP_ROW_MIRROR>(v);
    return v;
}
// (value, index) of the wave's maximum, ties to the smaller index, in every lane: four in-row steps on DPP, the two
// cross-row steps on the lane-swap instructions (no LDS round trip left)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#define DIMX_ARGMAX_STEP(OV, OI)                          \
    do {                                                  \
        const float ov_ = (OV);                           \
        const int oi_ = (OI);                             \
        if (ov_ > v || (ov_ == v && oi_ < i)) {           \
            v = ov_;                                      \
            i = oi_;                                      \
        }                                                 \
    } while (0)
    DIMX_ARGMAX_STEP(dpp_f32<DPP_XOR1>(v), dpp_i32<DPP_XOR1>(i));
    DIMX_ARGMAX_STEP(dpp_f32<DPP_XOR2>(v), dpp_i32<DPP_XOR2>(i));
    DIMX_ARGMAX_STEP(dpp_f32<DPP_HALF_MIRROR>(v), dpp_i32<DPP_HALF_MIRROR>(i));
    DIMX_ARGMAX_STEP(dpp_f32<DPP_ROW_MIRROR>(v), dpp_i32<DPP_ROW_MIRROR>(i));
    DIMX_ARGMAX_STEP(xor_lane_f32<16>(v), xor_lane_i32<16>(i));
    DIMX_ARGMAX_STEP(xor_lane_f32<32>(v), xor_lane_i32<32>(i));
#undef DIMX_ARGMAX_STEP
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_f32<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f32<DPP_XOR2>(v));
    v = fmaxf(v, dpp_f32<DPP_HALF_MIRROR>(v));
    v = fmaxf(v, dpp_f32<DPP_ROW_MIRROR>(v));
    return fmaxf(fmaxf(lane_f32(v, 0), lane_f32(v, 16)), fmaxf(lane_f32(v, 32), lane_f32(v, 48)));
}
// The wave sum of the f32 parity mode and of the VQ search keeps its historical association (xor 32, 16, ... 1: the order
// oracle/vq_argmin.c restates); the bf16 perf mode takes the DPP form, which associates as xor 1, 2, ... 32 -- the two
// differ in the last bit for about a third of all inputs (tools/ubench/dpp_check.hip).
__device__ __forceinline__ float wave_sum(float v) {  // the xor 32, 16, ... 1 butterfly, step for step
    v += xor_lane_f32<32>(v);
    v += xor_lane_f32<16>(v);
    v += xor_lane_f32<8>(v);
    v += xor_lane_f32<4>(v);
    v += xor_lane_f32<2>(v);
    v += xor_lane_f32<1>(v);
    return v;
}
__device__ __forceinline__ float wave_sum_fast(float v) {
    v = row16_sum(v);
    return (lane_f32(v, 0) + lane_f32(v, 16)) + (lane_f32(v, 32) + lane_f32(v, 48));
}
template <bool FAST> __device__ __forceinline__ float wave_sum_sel(float v) { return FAST ? wave_sum_fast(v) : wave_sum(v); }
template <int O> __device__ __forceinline__ double xor_lane_f64(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)xor_lane_i32<O>((int)(unsigned)u), hi = (unsigned)xor_lane_i32<O>((int)(unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// the xor 32, 16, ... 1 butterfly in double: every lane ends with the same bits.  All 64 lanes must be active.
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += xor_lane_f64<32>(v);
    v += xor_lane_f64<16>(v);
    v += xor_lane_f64<8>(v);
    v += xor_lane_f64<4>(v);
    v += xor_lane_f64<2>(v);
    v += xor_lane_f64<1>(v);
    return v;
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// split-K count that leaves no split empty: the kernels give split i the k-tiles [i*per, (i+1)*per) with per = ceil(nk / sp), so a
// count whose last split starts past nk (nk = 49, sp = 8: per = 7, 7 splits cover it) is lowered to the count that per really needs --
// the same per, the same partition, and no slab the kernel would leave unwritten
inline int splitk_nonempty(int nk, int sp) {
    if (nk < 1 || sp < 1) return 1;
    if (sp > nk) sp = nk;
    return ceil_div(nk, ceil_div(nk, sp));
}

// ---------------------------------------------------------------- GEMM launcher
struct OutSeg {
    void* ptr;
    long sb, sh, st, sd;  // element strides for (batch row, head, time, channel)
    int D;                // channels per head inside the segment
};

struct GemmArgs {
    int in_dtype, out_dtype;
    const void* A;
    int lda;
    const void* W;
    int ldw;  // row stride of W (elements), >= the k extent the loop runs over
    int kloop;  // k extent of the main loop (multiple of the k-tile; 0 = ldw).  ldw > kloop lets the caller pad the
                // row stride so that consecutive rows do not camp on the same L2 channels
    int M, N, K;
    // temporal k=5 convolution gather on A (conv_T > 0)
    int conv_T;
    const int32_t* conv_lens;
    int conv_C;
    // epilogue
    const float* bias;
    int act;
    const float* residual;
    int ldr;
    const float* rowadd;  // [rows, ld_rowadd] table added after the activation
    int rowadd_mode;      // 0 none, 1 row t, 2 row b + rowadd_off, 3 fixed row rowadd_off
    float rowadd_scale;
    int rowadd_off, ld_rowadd;
    int rowadd_div;       // mode 2: table row = b / rowadd_div + rowadd_off (several samples per clip share a row)
    // rows decompose as m = b*rowT + t (rowT = 1 -> b = m, t = 0); used by rowadd and the output map
    int rowT;
    // output: N columns split into nseg equal segments of seg_width columns; element (m, n) of
    // segment s goes to seg[s].ptr + b*sb + t*st + (nn / D)*sh + (nn % D)*sd, nn = n - s*seg_width
    OutSeg seg[3];
    int nseg, seg_width;
    // scheduling knobs
    int allow_splitk;  // perf mode: split K with f32 atomics when the grid is small (in-place residual only)
    int splitk;        // set by the launcher
    int force_simple;  // tests: force the register-staged kernel
    int cfg;           // tile/stage configuration id of the LDS-DMA kernel (0 = automatic)
    int force_splitk;  // tuning: requested split count (0 = automatic)
    int out_slabs;     // split-K partial sums go to f32 slabs C + split*slab_stride (plain stores, fixed order
                       // reduction by the consumer kernel); requires act none, no residual/rowadd, plain output
    long slab_stride;  // elements between slabs
    int stage_out;     // set by the launcher: large-M outputs leave through LDS as 8/16-byte row-contiguous pieces
    // deferred LayerNorm of the A operand (gemm_ws_kernel only; see ChainArgs.defer): A holds bf16(x) un-normalised, W the
    // gamma-scaled weights; acc <- rstd[m] * (acc - mean[m] * ln_colsum[n]) before bias / activation.  ln_stats =
    // [M / 32][32][32][2] per-slice {sum x, sum (x - slice mean)^2}, 32 equal column slices of ln_C columns.
    const float* ln_stats;
    const float* ln_colsum;
    int ln_C;
    unsigned* ln_err;  // optional: bit 2 is set when a row's |mean| exceeds 8 standard deviations (deferred form too coarse)
    int w_tiled;       // W is stored as [N/8][ldw/BK] blocks of 8 rows x 128 B (1 KiB, contiguous): an LDS-DMA piece then reads one
                       // contiguous KiB instead of 8 row segments (tools/ubench/cu_load_rate.hip: 122-143 vs 70-78 GB/s per CU).
                       // gemm_ws_kernel only.  Measured: -0.2 us per decode GEMM, nothing end to end (1467 vs 1467 clips/s) -- the
                       // model keeps row-major weights; the switch stays for tools/gemm_ab.py and the kernel test.
    const void* w3;    // round 6, f32 parity mode: W as three bf16 planes [3][N][ldw] whose sum is W exactly (split_x3); with it a
    long w3_plane;     // GEMM of the DECODE STEP (x3_decode) runs on the bf16 matrix cores, f32-equivalent (gemm_x3_kernel).  Elements between planes.
    int x3_decode;     // set by the decode step (dimx_generate) and by dimx_op_gemm_x3 only: the kernel choice must not depend on M -- a
                       // rank's shard of a batch reproduces the rows of the whole batch bit for bit whatever the batch size
    int vt_pack4;      // set by the launcher: transposed (time-contiguous) segments take 4 packed rows per store
};

void gemm_args_init(GemmArgs& a);
// plain row-major output helper
void gemm_set_plain_out(GemmArgs& a, void* C, int ldc);
int launch_gemm(const GemmArgs& a, hipStream_t s);
// what launch_gemm would run for `a`, from the launcher's own decision code, without launching (dimx_op_gemm_route): *route =
// kernel (cfg id 1/3/4/14/34/35/72, 256 = gemm256, 1064 / 1128 = register-staged gemm_kernel 64x64 / 128x128, 2000 = gemm_x3)
// | stage_out << 16 | vt_pack4 << 17; the launcher's argument errors are returned as they are
int gemm_route(const GemmArgs& a, int* route);
// the 256 x 256 phase-pipelined prefill kernel (gemm256.hip): taken by launch_gemm when eligible
bool gemm256_eligible(const GemmArgs& a);
int launch_gemm256(const GemmArgs& a, hipStream_t s);
int launch_gemm256_segs(const GemmArgs& a, const OutSeg* segs, int nseg, int seg_width, hipStream_t s);
// the split-bf16 decode GEMM of the f32 parity mode (gemm_x3.hip): eligibility, tile / split plan (functions of N, K and the
// slab flag only), launch
bool gemm_use_x3(const GemmArgs& a);
bool gemm_x3_plan(const GemmArgs& a, int* bn_out, int* sp_out);
int launch_gemm_x3(const GemmArgs& a, hipStream_t s);
// W [N][ldw] f32 -> three bf16 planes [3][N][ldw] with plane0 + plane1 + plane2 == W exactly
int launch_split_x3(const float* w, void* planes, size_t n, hipStream_t s);
// number of K splits launch_gemm will use for an out_slabs GEMM (the consumer needs it)
int gemm_plan_splits(const GemmArgs& a);

// ---------------------------------------------------------------- other launchers
int launch_layernorm(int out_dtype, const float* x, void* y, const float* gamma, const float* beta, int M,
                     int C, hipStream_t s);
// x[row] += sum_s slabs[s][row] (fixed order), then y = LayerNorm(x); decode-step residual + pre-norm
int launch_add_slabs_layernorm(int out_dtype, float* x, const float* slabs, int nslab, long slab_stride, void* y,
                               const float* gamma, int M, int C, hipStream_t s);
int launch_instnorm(int out_dtype, const float* x, void* y, const int32_t* lens, int B, int T, int C,
                    hipStream_t s);

struct AttnArgs {
    int dtype;
    const void *q, *k, *vt;
    void* o;
    long q_sb, q_st, q_sh;  // q element (b,i,h,d) at q + b*q_sb + i*q_st + h*q_sh + d
    long k_sb, k_st, k_sh;
    long v_sb, v_sh, v_sd;  // vt element (b,h,d,j) at vt + b*v_sb + h*v_sh + d*v_sd + j
    int v_rows;             // 1: `vt` is V itself, row-major like k: element (b,j,h,d) at vt + b*v_sb + j*v_st + h*v_sh + d (bf16, D <= 64)
    long v_st;
    long o_sb, o_st, o_sh;
    int B, H, Lq, Lk, D;
    float scale;
    int causal;
    const int32_t* lens;   // [B] optional
    const uint8_t* kmask;  // [B, kmask_ld] optional
    int kmask_ld;
    // attention_tr.hip with a key mask: scratch for the packed 64-bit validity words, B * ceil(Lk / 64) of them, owned by the
    // CALLER (its workspace arena: one buffer per handle and call, so launches on other streams / devices never share it and
    // nothing is allocated inside a launch or a stream capture -- ADVICE round 4)
    unsigned long long* kwords;
    size_t kwords_cap;     // in words
    int kwords_ready;      // the words in `kwords` are already packed for this kmask (launch_pack_key_words): no pack launch -- the decode
                           // loop packs its context mask once per generation, not once per step and layer
};
// key validity words of attention_tr.hip: word[b][t] bit j <-> key 64 t + j of clip b is a key; words [B][ceil(Lk / 64)]
int launch_pack_key_words(const uint8_t* kmask, int kmask_ld, const int32_t* lens, int B, int Lk, unsigned long long* words, size_t cap,
                          hipStream_t s);
int launch_attention(const AttnArgs& a, hipStream_t s);
int launch_attention_tr(const AttnArgs& a, hipStream_t s);
// mlp_fused.hip: x <- x + W2 . gelu(W1 . LayerNorm(x) + b1) + b2 in one launch (bf16 operands, C = 384); the weights are packed once
// on the host into the kernel's LDS chunk images
size_t mlp_fused_packed_bytes(int C, int F);
int mlp_fused_pack(const float* w1, const float* b1, const float* w2, int C, int F, uint16_t* out);
int launch_mlp_fused(float* x, const void* packed, const float* b2, const float* ln_g, const float* ln_b, int M, int C, int F, int act,
                     hipStream_t s);  // attention_tr.hip: bf16, D 48 / 64, q / k / v row-major

struct DecodeAttnArgs {
    int dtype;             // storage type of q / caches / out
    const void* q;         // [B, q_ld] : head h at h*64
    int q_ld;
    int q_f32;             // q / knew / vnew are f32 split-K slabs [nslab][B, ld]: summed in slab order on load
    int nslab;
    long slab_stride;      // elements between slabs
    int force_nsplit;      // tests: waves per (clip, head) (0 = automatic)
    int rows_per_clip;     // cross attention with several query rows per clip (multi-sample generation):
                           // rows r*S .. r*S+S-1 of q/out share clip r's K/V cache and mask (0/1 = one row)
    const void* knew;      // self-attn: this step's k/v rows [B, *] (nullptr for cross attention)
    const void* vnew;
    int kv_ld;
    void* kcache;          // [B,H,Tmax,64]
    void* vcache;
    int Tmax;
    void* out;             // [B, o_ld]
    int o_ld;
    int B, H;
    const int32_t* step;   // device scalar: self -> number of cached keys before this step
    int n_keys;            // cross: number of keys (T); self: ignored
    const uint8_t* kmask;  // cross: [B, kmask_ld] optional
    int kmask_ld;
    float scale;
    // self attention of the first decoder layer in its table form (tab != nullptr; decode_attn_body.hpp, TAB): the K / V row of
    // position j is a row of a table over the token ids, picked by the row's token history, and no cache is read or written
    const void* tab;       // [tab_rows, tab_ld] in the storage type: K of head h at tab_koff + h*64, V at tab_voff + h*64
    int tab_ld, tab_koff, tab_voff, tab_rows;
    const int32_t* hist;   // [B, hist_ld] the layer's input token of every position so far (hist_ld >= Tmax)
    int hist_ld;
    // cross attention in its windowed (online) form (win != 0; decode_attn_body.hpp, WIN): the query of decode step t = *step sees
    // the keys j < clamp(t + 2 + lookahead, 1, n_keys) only -- the speaker frames that exist when frame t + 1 is produced
    int win, lookahead;
};
int launch_decode_attn(const DecodeAttnArgs& a, hipStream_t s);

// The cross form over an FP8 copy of the context K/V (decode_attn_kv8.hip; dimx/kv8.py): one query row per clip
struct Kv8AttnArgs {
    const float* q;        // f32 split-K slabs [nslab][B, q_ld], head h at h*64, summed in slab order
    int q_ld, nslab;
    long slab_stride;      // elements between slabs
    const uint8_t* kcodes; // [B,H,Tmax,64] e4m3fn codes
    const float* kscale;   // [B,H,Tmax]
    const uint8_t* vcodes;
    const float* vscale;
    int Tmax;
    void* out;             // [B, o_ld] of out_dtype
    int out_dtype, o_ld;
    int B, H;
    int n_keys;
    const uint8_t* kmask;  // [B, kmask_ld] optional
    int kmask_ld;
    float scale;
    int force_nsplit;      // tests: waves per (clip, head) (0 = automatic)
    int win, lookahead;    // the windowed form: keys j < clamp(*step + 2 + lookahead, 1, n_keys)
    const int32_t* step;
    // the multi-query form only (launch_decode_attn_mq_kv8): rows b*S .. b*S+S-1 of q / out share clip b's codes, scales and mask row
    int rows_per_clip;     // S in {2, 4, 5, 8, 10}; B counts clips
    int q_bf16;            // q is one bf16 row array [B*S, q_ld] (a plain projection's output), nslab = 1
    int exact;             // 0: matrix-core form (q and p * vscale rounded to bf16), 1: exact form (three bf16 planes of each)
};
int launch_decode_attn_kv8(const Kv8AttnArgs& a, hipStream_t s);
// S queries of a clip against that clip's FP8 codes on the matrix cores, the codes read once for all S (dimx/kv8.py attention_rows)
int launch_decode_attn_mq_kv8(const Kv8AttnArgs& a, hipStream_t s);
// rows 0 .. T - 1 of every (clip, head) of one cache [B,H,Tp,64] (dtype) -> codes [B,H,Tp,64] / scales [B,H,Tp]; cache_T > 0: the
// cache is [B,H,cache_T,64] (a generation's self caches)
int launch_kv8_quant(int dtype, const void* cache, int B, int H, int Tp, int T, uint8_t* codes, float* scales, hipStream_t s, int cache_T = 0);
// rows [n0, n0 + c) of every (clip, head) of the K and V caches of `depth` layers -> their codes / scales, one launch (dimx/kv8.py
// append; what a streaming session's push issues after it appended the rows).  Rows outside the range are neither read nor written.
struct Kv8AppendArgs {
    const void* cache[16];   // [2 l] layer l's K cache, [2 l + 1] its V cache: [B, H, Tc, 64] in dtype
    uint8_t* codes[16];      // ... their code planes [B, H, Tp, 64]
    float* scales[16];       // ... and scale planes [B, H, Tp]
    int dtype, depth;        // DIMX_F32 / DIMX_BF16; 1 .. 8 layers
    int B, H, Tc, Tp;
    int n0, c;               // 0 <= n0, 1 <= c, n0 + c <= min(Tc, Tp), Tp <= 2048
};
int launch_kv8_append(const Kv8AppendArgs& a, hipStream_t s);
// The self form over FP8 self-attention caches (decode_attn_kv8.hip; dimx/kv8.py self_step): one launch quantises this step's k / v
// row, stores it at position n and attends over the rows 0 .. n, the own row taken from registers
struct Kv8SelfArgs {
    const float* q;        // f32 split-K slabs [nslab][B, ld]: q | new k | new v of head h at q / knew / vnew + h*64, summed in slab order
    const float* knew;
    const float* vnew;
    int ld, nslab;
    long slab_stride;      // elements between slabs
    uint8_t* kcodes;       // [B,H,Tmax,64] e4m3fn codes: rows 0 .. n - 1 are read, row n is written
    float* kscale;         // [B,H,Tmax]
    uint8_t* vcodes;
    float* vscale;
    int Tmax;
    void* out;             // [B, o_ld] of out_dtype
    int out_dtype, o_ld;
    int B, H;
    const int32_t* step;   // device scalar: n, the rows already cached; nullptr = n_max
    int n_max;             // n is clamped to 0 .. n_max (< Tmax): no row at or past Tmax can be addressed whatever *step holds
    float scale;
    int force_nsplit;      // tests: waves per (row, head) (0 = automatic)
};
int launch_decode_attn_self_kv8(const Kv8SelfArgs& a, hipStream_t s);

int launch_vq_argmin(const float* z, int N, const float* Et /*[128][512]*/, const float* ee /*[512]*/,
                     int32_t* idx, float* best_d, float* margin, hipStream_t s);

// ---------------------------------------------------------------- XCD-local chain kernels (chain.hip)
struct ChainGemmDesc {
    const void* W;  // [N][ldw] bf16, rows = output columns
    int N, K, ldw;
    int cols, rows_pad, ncb, nkt;  // filled by the planner: columns per CU, 8-row padded, 32-column blocks, k-tiles
};
struct ChainArgs {
    int B;  // rows (clips), <= 256: group g = rows [32g, 32g + 32) lives on XCD g
    // first projection (optional, g1.W != nullptr): A1 [B, lda1] bf16 . W1^T -> xr [B, C] f32 (C = g1.N)
    ChainGemmDesc g1;
    const void* A1;
    int lda1;
    float* xr;
    // row phase: x [B, C] f32 += xr (+ slabs[0..nslab) of a preceding chip-wide split-K GEMM); y = LayerNorm(x) * gamma
    float* x;
    int C;
    const float* slabs;
    int nslab;
    long slab_stride;
    void* y;  // bf16 [B, C]
    const float* gamma;
    // second projection (optional): y . W2^T -> out2 [B, ld_out2] f32 (K = C)
    ChainGemmDesc g2;
    float* out2;
    int ld_out2;
    // synchronisation: this launch site's per-XCD arrival counters [8][16] (zeroed once per generate call), the
    // device step counter (epoch of the monotonic counters), error flags (bit 0 placement, bit 1 barrier timeout)
    unsigned* counters;
    unsigned* seen;  // [8][32] this launch site's (XCD, CU slot) claim stamps (zeroed with the counters)
    const int32_t* step;
    unsigned* err;
    // Deferred LayerNorm (defer = 1, needs g1): the CU that owns a column slice of the first projection adds the residual
    // itself, writes x (f32) and y = bf16(x) UN-normalised plus the partial row sums {sum x, sum x^2} of its columns into
    // stats[group][CU][row][2]; the consumer of y multiplies with gamma-scaled weights W' = gamma o W and corrects its
    // result: LN(x) . W^T = rstd * (x . W'^T - mean * colsum(W')).  No row phase and no second group barrier; with no
    // second projection the kernel has no group barrier at all (the next launch -- ff1 -- is the consumer).
    int defer;
    float* stats;            // [8][32][32][2] f32
    const float* colsum2;    // [g2.N] f32: row sums of the gamma-scaled second projection (defer && g2)
    int nbar;                                                // set by the launcher
    int fault;  // test hook (dimx_debug_chain_fault): the blocks of XCD 2i+1 claim XCD 2i's slots -- a non-bijective placement
    int offA1, offW1, offRed1, offA2, offW2, offRed2;        // LDS plan, set by the launcher
};
// The sampling head of the first layer's launch (chain.hip, xcd_layer_kernel HEAD; needs the table form of its self attention).
// Layer 0's input is a function of the sampled token alone, and the CU that owns clip b is the consumer of row b's token: one of
// its waves runs sample_kernel's top-k route (sample_pick.hpp) on the logits the previous step left, and the attention waves take
// q / new k / new v from row qkv0[token] of the f32 table -- no sampler launch, no copy of that row into slab 0.
// `params` is the call's parameter block (gen_params_kernel): word 0 the step word, 2.. the sampler's dev_params, 8 the arrival
// counter, 9 the chain epoch, 14 the first-step flag.  Every block reads words 0 / 9 / 14 once at entry.  Flag set: no logits yet,
// the head is skipped, the token is hist[b][step], and x is what the start-token launches wrote.  Flag clear: the head samples
// step `word`, the launch runs position word + 1 at epoch + 1, and the block that arrives last advances both words -- after
// every block has read them; the step's later launches see the advanced values across the kernel boundary.
struct SampleHeadArgs {
    int on;                     // 0 = a launch without the head
    const float* logits;        // [B, ld_logits] x nslab slabs, added in slab order
    int ld_logits, nslab;
    long slab_stride;
    int top_k;
    const float* noise;         // [steps, rows_total, 512] or nullptr (the counter-based generator)
    int row0, rows_total;
    int32_t* tokens;            // [B, tok_ld], column = the step sampled
    int tok_ld;
    float* logits_out;          // [B, logits_out_ld, 512] or nullptr
    int logits_out_ld;
    const float* emb_table;     // [512][C] -> x[b, :]
    const float* qkv0;          // [512][qkv0_N] f32: q | k | v of a token
    int qkv0_N;
    int32_t* hist;              // == sa.hist, written at position step + 1
    int hist_ld;
    int32_t* params;
};
// The attention half of a decoder layer as ONE launch (chain.hip, xcd_layer_kernel; round 5): self attention -> out-projection +
// residual -> (deferred LayerNorm) cross-q projection -> cross attention -> out-projection + residual.  Clip i of group g is CU
// slot i of XCD g for both attentions and all three projections split their columns over the XCD's 32 CUs, so every hand-off
// stays inside the XCD (four group barriers); the projections' weight slices are requested while the attentions stream.
struct LayerChainArgs {
    int B, C;                       // clips (<= 256), model dim
    DecodeAttnArgs sa, ca;          // self / cross attention, one query row per (clip, head); out = o (bf16 [B, ld_o]); ca.q = qc
    ChainGemmDesc g_so, g_cq, g_co; // self out-projection [C][inner], cross q (gamma-scaled) [inner][C], cross out-projection [C][inner]
    const void* o;                  // attention output rows = A operand of the two out-projections
    int ld_o;
    float* x;                       // [B, C] f32 residual stream
    void* y;                        // [B, C] bf16(x), un-normalised
    float* stats;                   // [8][32][32][2] partial row sums (deferred LayerNorm)
    const float* colsum_cq;         // [inner] row sums of the gamma-scaled q projection
    float* qc;                      // [B, ld_qc] f32 cross-attention queries
    int ld_qc;
    unsigned* counters;             // this launch site's per-XCD arrival counters [8][16] + claim stamps [8][32]
    unsigned* seen;
    const int32_t* step;            // epoch of the monotonic counters: launches on one counter set must see 0, 1, 2, ... (the decode
    int epoch_add;                  // step counter in dimx_generate; nullptr + epoch_add = the call index in dimx_op_layer_chain)
    unsigned* err;
    int fault;
    unsigned long long* prof;       // tuning only: [256][16] phase stamps
    SampleHeadArgs head;            // head.on: the sampler of the previous step's logits is this launch's first stage
    int sc_stride;                // floats per (clip, head) score row in LDS
    int off_base, off_A1, off_W1, off_A2, off_W2, off_W3, off_A3;  // LDS plan (bytes), set by the launcher
};
bool layer_chain_supported(const LayerChainArgs& a, int cu_count);
int launch_layer_chain(const LayerChainArgs& a, hipStream_t s);
size_t chain_plan(ChainArgs& a);
bool chain_supported(const ChainArgs& a, int cu_count);
int launch_chain(const ChainArgs& a, hipStream_t s);

// elementwise helpers (elementwise.hip)
int launch_cast_pad(int out_dtype, const float* x, int ldx, const float* coladd, void* y, int ldy, int M, int K,
                    hipStream_t s, const uint8_t* zero_rows = nullptr);
int launch_gather_rows(int out_dtype, const float* table, int ld_table, int rows, const int32_t* idx, void* y,
                       int ldy, int M, int C, hipStream_t s);
// One bidirectional LSTM layer, hidden 384, f32 (lstm.hip).  Weights as torch.nn.LSTM keeps them, index 0 forward / 1 reverse;
// scratch: lstm_scratch_bytes(B, T, In) bytes, 256-byte aligned.  flags bit 0 = the safe path; cu_count != 256 takes it too.
// The group path waits for the layer on the host (it reads the fault word) and on a fault reruns it on the safe path and
// increments *fault_count.  save (training forward): [B*T][2][kLstmSave][H] f32 = the post-activation gates i, f, g, o, c_t and
// tanh c_t of every cell update, stored by the same kernels; y does not depend on it.
constexpr int kLstmSave = 6;
size_t lstm_scratch_bytes(int B, int T, int In);
int lstm_layer_run(const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                   const float* const* b_ih, const float* const* b_hh, float* y, void* scratch, size_t scratch_bytes, int flags,
                   int cu_count, int* fault_count, hipStream_t st, float* save = nullptr);
// The adjoint of that recurrence (train_lstm.hip): dy [B][T][2H], save as above, w_hh [2] -> dgates [B*T][2][4H] (the gradient
// of the gate pre-activations, i f g o).  The forward's calling convention; only the no-communication path is built.
size_t lstm_bwd_scratch_bytes(int B, int T);
int lstm_bwd_run(const float* dy, const float* save, const float* const* w_hh, int B, int T, float* dgates, void* scratch,
                 size_t scratch_bytes, int flags, int cu_count, int* fault_count, hipStream_t st);
int launch_context_concat(int out_dtype, const float* x_s, const float* patch, const float* audio, void* ctx,
                          int M, int dim, int dim_a, hipStream_t s);
int launch_finalize_idx(int32_t* idx, const int32_t* lens, int B, int T, int32_t pad_value, hipStream_t s,
                        int fqn = 1);
int launch_shift_tokens(const int32_t* z, int32_t* inp, int32_t* tgt, int B, int T, hipStream_t s);
int launch_ce_argmax(const float* logits, const int32_t* target, float* row_loss, int32_t* argmax_tok, int R,
                     int V, hipStream_t s);
// sampler filter of a launch (DIMX_FILTER_*): kind 0 = the launch's top_k.  a / b are read from the launch only when there
// is no device parameter block (dimx_op_sample_filtered); keep_out [R, 512]: the kept set the launch used (optional)
struct SampleFilter {
    int kind = 0;
    float a = 0.f, b = 0.f;
    uint8_t* keep_out = nullptr;
};
// one sampler launch (sample_kernel's arguments, in its order); a caller names the fields it sets
struct SampleArgs {
    const float* logits = nullptr;
    int ld_logits = 0, R = 0, top_k = 0;
    float temperature = 0.f;
    const float* noise = nullptr;
    uint64_t seed = 0;
    const int32_t* step_dev = nullptr;
    uint64_t step_host = 0;
    int32_t* tokens = nullptr;
    int tok_ld = 0, tok_col_from_step = 0, nslab = 0;
    long slab_stride = 0;
    float* logits_out = nullptr;
    int logits_out_ld = 0, row0 = 0, rows_total = 0;
    const float* emb_table = nullptr;
    int emb_C = 0;
    float* x_next = nullptr;
    int32_t* step_rw = nullptr;
    unsigned* done_ctr = nullptr;
    const float* pos_table = nullptr;
    float pos_scale = 0.f;
    int pos_rows = 0;
    const int32_t* dev_params = nullptr;
    void* y_next = nullptr;
    const float* y_gamma = nullptr;
    int y_dtype = DIMX_F32;
    const float* qkv0_table = nullptr;
    float* qkv0_out = nullptr;
    int qkv0_N = 0;
    // prompted generation: rows whose next position lies inside their clip's prompt [clips, prompt_ld] take its token
    // (clip = row / prompt_div; length clamp(prompt_len, dev_params[8] + 1, prompt_max), NULL = prompt_max);
    // epoch_rw: a second counter advanced with the step counter (steps done in this call)
    const int32_t* prompt = nullptr;
    int prompt_ld = 0, prompt_max = 0;
    const int32_t* prompt_len = nullptr;
    int prompt_div = 1;
    int32_t* epoch_rw = nullptr;
    SampleFilter filt;
    // the first layer's token history [R, hist_ld]: position step + 1 takes the (clamped) token of this launch (needs step_dev)
    int32_t* hist = nullptr;
    int hist_ld = 0;
};
int launch_sample(const SampleArgs& a, hipStream_t s);
// Classifier-free guidance (sample_guided_kernel; the definition is dimx/guidance.py): what the guided sampler takes beside a
// SampleArgs of R = clips rows.  The row sampled is c + (scale - 1) * (c - u), c / u = row r of a.logits / logits_u (same leading
// dimension, slab count and slab stride); every per-row output is written for rows r and r + R.  The scale is read from word 11
// behind a.dev_params when there is a parameter block.  a.logits_out takes the guided rows.
struct GuidedArgs {
    const float* logits_u = nullptr;
    float scale = 1.f;
    float* branch_out = nullptr;    // [2, R, a.logits_out_ld, 512]: c and u as summed (optional)
    int32_t* tokens_u = nullptr;    // [R, a.tok_ld]: the token once more, for the unconditional rows (optional)
};
int launch_sample_guided(const SampleArgs& a, const GuidedArgs& g, hipStream_t s);
// Beam search (beam.hip; the definition is dimx/beam.py).  One selection launch: rows clip * W + w of `logits` (split-K slabs, added
// in slab order like the sampler) are the W beams of a clip; column c = *step_dev (or step_host).  The mode of a clip is
// forced while c + 1 < clamp(prompt_len, dev_params[8] + 1, prompt_max) (the sampler's rule), frozen when c >= lens[clip] - len_off,
// live otherwise -- or mode[clip] (0 live, 1 forced with forced_tok[clip], 2 frozen) when `mode` is given (dimx_op_beam_step).
// cum_in / cum_out may be the same buffer.  step_rw / done_ctr / epoch_rw advance the step word as the sampler does.
struct BeamSelectArgs {
    const float* logits = nullptr;
    int nslab = 1;
    long slab_stride = 0;
    int nclip = 0, W = 0;
    const int32_t* step_dev = nullptr;
    int step_host = 0;
    int32_t* step_rw = nullptr;
    unsigned* done_ctr = nullptr;
    int32_t* epoch_rw = nullptr;
    const int32_t* dev_params = nullptr;
    const int32_t* prompt = nullptr;
    int prompt_ld = 0, prompt_max = 0;
    const int32_t* prompt_len = nullptr;
    const int32_t* lens = nullptr;
    int len_off = 0;
    const int32_t* mode = nullptr;
    const int32_t* forced_tok = nullptr;
    const double* cum_in = nullptr;
    double* cum_out = nullptr;
    int32_t* parent = nullptr;
    int32_t* tokens = nullptr;     // [R, tok_ld], column c (column 0 without step_dev)
    int32_t* backptr = nullptr;    // [R, tok_ld] or nullptr
    int tok_ld = 1;
    float* logits_out = nullptr;   // [R, tok_ld, 512] or nullptr
    const float* emb_table = nullptr;   // next step's input row x_next[row] = emb_table[token] (emb_C % 4 == 0) or nullptr
    int emb_C = 0;
    float* x_next = nullptr;
    const float* qkv0_table = nullptr;  // and the first layer's q/k/v table row into qkv0_out[row] (qkv0_N % 4 == 0) or nullptr
    float* qkv0_out = nullptr;
    int qkv0_N = 0;
};
bool beam_width_supported(int W);   // {1, 2, 4, 5, 8, 10}: the rows per clip generate_impl accepts
int launch_beam_select(const BeamSelectArgs& a, hipStream_t s);
// In-place permutation of nbuf caches [nclip * W, H, T, 64] (element size es) by parent beam, positions 0 .. c, and of the token /
// back-pointer columns 0 .. c - 1; c = *step_dev - step_back (the selection has advanced the word already) or c_host.
struct BeamReorderArgs {
    void* buf[16] = {};
    int nbuf = 0, es = 4, nclip = 0, W = 0, H = 0, T = 0;
    const int32_t* parent = nullptr;
    const int32_t* step_dev = nullptr;
    int step_back = 0, c_host = 0;
    int32_t* tokens = nullptr;
    int32_t* backptr = nullptr;
    int tok_ld = 0;
};
int launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s);
// The same permutation over FP8 self caches (dimx_set_self_kv8 under dimx_set_beam_kv8; the definition is dimx/kv8.py reorder): nbuf
// pairs of a code plane [nclip * W, H, Tp, 64] uint8 and its scale plane [nclip * W, H, Tp] f32 -- the K and the V pair of every
// layer (stages.hpp kv8_layer_of) -- positions 0 .. c, codes and scale of a position together; the position stride is Tp, not T.
// Tokens / back-pointers and c as in BeamReorderArgs.  One launch of at most 8 pairs (a decoder of depth 4): 16 pointers, the plain
// kernel's argument block -- with 32 the W = 8 and W = 10 instantiations run out of scalar registers.
constexpr int kBeamKv8Pairs = 8;
struct BeamReorderKv8Args {
    uint8_t* codes[kBeamKv8Pairs] = {};
    float* scale[kBeamKv8Pairs] = {};
    int nbuf = 0, nclip = 0, W = 0, H = 0, Tp = 0;
    const int32_t* parent = nullptr;
    const int32_t* step_dev = nullptr;
    int step_back = 0, c_host = 0;
    int32_t* tokens = nullptr;
    int32_t* backptr = nullptr;
    int tok_ld = 0;
};
int launch_beam_reorder_kv8(const BeamReorderKv8Args& a, hipStream_t s);
// cum[r] = 0 for beam 0 of a clip, -inf for the others; parent[r] = r % W
int launch_beam_init(double* cum, int32_t* parent, int R, int W, hipStream_t s);
// the first decoder layer's q/k/v as a table over the token ids (generate.hip qkv0_table_build): id list of the build rounds,
// slab-order sum of a round's projection into the table rows, and step 0's rows by start token
int launch_iota_clamp(int32_t* ids, int n, int rows, hipStream_t s);
int launch_sum_slabs_rows(const float* slabs, int nslab, long slab_stride, float* table, int id0, int rows, int M, int N,
                          hipStream_t s);
int launch_gather_start_rows(const float* table, int N, int rows, const int32_t* start, int start_div, float* out, int B,
                             hipStream_t s, int start_ld = 1, int32_t* hist = nullptr, int hist_ld = 0);
// the K / V columns [col0, col0 + W) of that table as a bf16 image [rows][W] (the bits the decode cache append would store)
int launch_kv0_image(const float* table, int ld, int rows, int col0, int W, void* image, hipStream_t s);
// generate(): the per-group step counters = step0, done counters = 0, and temperature + seed next to them (read by the sampler)
int launch_gen_params(int32_t* base, int groups, float temperature, uint64_t seed, int row_off, int rows_total,
                      hipStream_t s, int step0 = 0, float filter_a = 0.f, float filter_b = 0.f, float guidance = 1.f);
int launch_embed_step(const float* table, int C, int rows, const int32_t* start, const int32_t* tokens, int tok_ld,
                      const int32_t* step_dev, float* x, int B, int start_div, hipStream_t s,
                      const float* pos_table = nullptr, float pos_scale = 0.f, int start_ld = 1, int start_step = 0);
// prompted generation's prefill (kv_prefill.hip): head rows [B, n, H*64] -> the generation cache [B*S, H, T, 64] (clip rows
// broadcast to the S samples; positions >= n untouched); the f32 mode's V^T [B*H, 64, ld_t] -> the same cache; a
// channel-contiguous V [B*H, ld_rows, 64] -> V^T [B*H, 64, ld_t] (positions n .. ld_t written as 0); the prompt's input ids of
// the prefilled positions + its own tokens into the output columns < n0
int launch_kv_rows_to_cache(int dtype, const void* src, void* cache, int B, int n, int H, int T, int S, hipStream_t st);
int launch_kv_vt_to_cache(const float* vt, int ld_t, float* cache, int B, int n, int H, int T, int S, hipStream_t st);
int launch_kv_rows_to_vt(const float* v_rows, int ld_rows, float* vt, int ld_t, int B, int n, int H, hipStream_t st);
int launch_prompt_rows(const int32_t* prompt, int ld, int B, int n0, int V, int S, int32_t* inp, int32_t* tokens, int tok_ld,
                       hipStream_t st);
int launch_add_pos_rows(float* x, const float* pos, int M, int n, int C, float scale, hipStream_t s);
int launch_mask_lens(const uint8_t* mask, int32_t* lens, int B, int T, hipStream_t s);
int launch_legacy_scramble(int out_dtype, const float* E, const int32_t* idx, const int32_t* lens, void* out, int B,
                           int T, int fqn, int zdim, int n_embed, hipStream_t s);
int launch_step_inc(int32_t* step_dev, hipStream_t s);
int launch_copy_rows_step(const float* src, float* dst, int B, int V, int n, const int32_t* step_dev, hipStream_t s);
int launch_mask_and(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, hipStream_t s);

}  // namespace dimx
