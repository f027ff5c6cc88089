// kmeans_sid.hip -- the SID diversity metric (calcuate_sid): a float64 KMeans fit on the ground-truth frames, then the
// assignment of frames to its centres, their histogram and its entropy.
//
// Reference: code/metrics/eval_utils.py:51-83, KMeans(k, random_state=0, n_init='auto').fit(gt).predict(pred) and
// -sum h log2(h + 1e-6).  The definition of every number here is dimx.mymetrics.kmeans_fit_f64 / kmeans_assign_f64 / sid_entropy:
// scikit-learn's k-means++ and lloyd path on float64 inputs with the random numbers drawn on the host (kmeans_draws: they do not
// depend on the data).  Distances are sum_c (x_c - c_c)^2 in column order, in float64.
//
// Fit, everything enqueued at once on one stream (stream order is the only grid-wide synchronisation; no block waits for another):
//   km_colsum / km_mean / km_center / km_tol    column means, Xc = x - mean (f64, workspace), tol * mean(var)
//   km_update(0)                                centre 0 = Xc[first], closest = its distances
//   per further centre s:  km_scan, km_bscan    inclusive scan of closest in blocks of 1024, offsets of the blocks, the potential
//                          km_cand              the trials' candidates (lower bound of U * pot in the scan, clipped to N - 1), per
//                                               block the partial potentials sum_i min(closest_i, d(x_i, candidate))
//                          km_update(s)         the partials in block order, first minimum, centre s, closest
//   per Lloyd iteration:   km_assign            nearest centre per point (first index on ties), "a label changed", and the partial
//                                               centre sums: a wave walks 32 consecutive points in order, one lane per column, into
//                                               acc[label][column] in LDS; a block keeps its sums over the tiles it owns
//                          km_combine           block k: the partials of centre k in block order, the new centre, its shift
//                          km_final             strict convergence (no label changed), sum shift^2 <= tol, an empty cluster or the
//                                               last iteration set the device word `done`; centres + mean go out
// Every launch after `done` is set returns at once.  No floating-point atomics anywhere: two calls on the same inputs are
// bit-identical.  The tile of an assign block lies in LDS next to the centres (K * F <= 2048 doubles) and four copies of acc.
// Assign (SID): the same nearest-centre search on (double) f32 rows, an int64 histogram with integer atomics, the entropy.
// Frames beyond N (M) are never read.  All address arithmetic is 64-bit.
#include "common.hpp"

namespace dimx {
namespace {

constexpr int kKmTile = 128;        // points of one tile
constexpr int kKmThreads = 256;     // assign / colsum / center blocks: 4 waves
constexpr int kKmMaxF = 64;
constexpr int kKmMaxKF = 2048;      // centres in LDS: 16 KB
constexpr int kKmMaxTrials = 16;
constexpr int kKmScan = 1024;       // elements of one scan block (256 threads x 4)
constexpr int kKmMaxGrid = 256;     // blocks of km_assign: a function of N only, so the partition is the same on every device
// state words (int32) at the head of the workspace
enum { KM_DONE = 0, KM_CHANGED = 1, KM_NITER = 2, KM_STATUS = 3, KM_STATE_WORDS = 16 };

__host__ __device__ inline int km_ldx(int F) { return F | 1; }

struct KmWs {
    int32_t* state;     // [KM_STATE_WORDS]
    int32_t* cand;      // [kKmMaxTrials]
    double* scal;       // [0] potential, [1] tol
    double* mean;       // [64]
    double* colpart;    // [ntiles][64]
    double* Xc;         // [N][F]
    double* closest;    // [N]
    double* scan;       // [N] inclusive inside a scan block
    double* bincl;      // [nscan] inclusive block totals
    double* ppot;       // [ntiles][kKmMaxTrials]
    double* cen;        // [2][KF]
    double* part;       // [grid][KF]
    int32_t* pcnt;      // [grid][K]
    double* shift;      // [K]
    int32_t* cnt;       // [K]
    int32_t* labels;    // [N]
};

struct KmArgs {
    const float* x;     // first column of the window of row 0
    long fs;
    int N, F, K, trials, ntiles, nscan, grid, max_iter;
    int first;
    const double* U;    // [(K - 1)][trials], device
    double tol;
    double* centers;    // out [K][F]
    int32_t* n_iter;    // out
    int32_t* status;    // out
    int32_t* labels;    // the labels the fit works on ([N]; the caller's array or the workspace's)
    KmWs w;
};

// rows of the tile that starts at row r0 of n
__device__ __forceinline__ int km_rows(int n, long r0) {
    const long left = (long)n - r0;
    return left < (long)kKmTile ? (int)left : kKmTile;
}

__device__ __forceinline__ bool km_done(const KmArgs& a) { return *(volatile const int32_t*)(a.w.state + KM_DONE) != 0; }

// rows [r0, r0 + rows) of the dense f64 matrix src [., F] -> tile[r][c] (row stride ldx)
__device__ __forceinline__ void km_load_tile(const double* src, long r0, int rows, int F, int ldx, double* tile) {
    const double* p = src + (size_t)r0 * F;
    for (int e = threadIdx.x; e < rows * F; e += blockDim.x) {
        const int r = e / F, c = e - r * F;
        tile[r * ldx + c] = p[e];
    }
}

// ------------------------------------------------------------------------------------------------ mean, centring, tolerance
// per tile the column sums: wave w walks rows 32 w .. 32 w + 31 in order, lane c owns column c; CENTER: of (x - mean)^2, and Xc
template <bool CENTER>
__global__ __launch_bounds__(kKmThreads) void km_colsum_kernel(KmArgs a) {
    __shared__ double red[4][kKmMaxF];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63;
    const long r0 = (long)blockIdx.x * kKmTile + 32 * wv;
    double s = 0.0;
    if (c < a.F) {
        const double mu = CENTER ? a.w.mean[c] : 0.0;
        for (int i = 0; i < 32; ++i) {
            const long r = r0 + i;
            if (r >= a.N) break;
            const double v = (double)a.x[(size_t)r * a.fs + c] - mu;
            if (CENTER) {
                a.w.Xc[(size_t)r * a.F + c] = v;
                s += v * v;
            } else {
                s += v;
            }
        }
    }
    red[wv][c] = s;
    __syncthreads();
    if (threadIdx.x < kKmMaxF) a.w.colpart[(size_t)blockIdx.x * kKmMaxF + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    if (CENTER && threadIdx.x < kKmTile) {
        const long r = (long)blockIdx.x * kKmTile + threadIdx.x;
        if (r < a.N) a.labels[r] = -1;
    }
}

// one block of 64: the tiles' partial sums in tile order.  TOL = false: mean[c];  TOL = true: tol * mean_c var_c
template <bool TOL>
__global__ __launch_bounds__(64) void km_mean_kernel(KmArgs a) {
    __shared__ double var[kKmMaxF];
    const int c = threadIdx.x;
    double s = 0.0;
    if (c < a.F)
        for (int b = 0; b < a.ntiles; ++b) s += a.w.colpart[(size_t)b * kKmMaxF + c];
    if (!TOL) {
        if (c < a.F) a.w.mean[c] = s / (double)a.N;
        return;
    }
    var[c] = s / (double)a.N;
    __syncthreads();
    if (c == 0) {
        double t = 0.0;
        for (int j = 0; j < a.F; ++j) t += var[j];
        a.w.scal[1] = a.tol * (t / (double)a.F);
    }
}

// ------------------------------------------------------------------------------------------------ k-means++
// inclusive scan of closest inside blocks of 1024: a thread scans its 4 elements, the 256 thread totals are scanned in LDS
__global__ __launch_bounds__(256) void km_scan_kernel(KmArgs a) {
    __shared__ double buf[2][256];
    const long i0 = (long)blockIdx.x * kKmScan + 4 * (long)threadIdx.x;
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + j < a.N ? a.w.closest[i0 + j] : 0.0;
    v[1] += v[0], v[2] += v[1], v[3] += v[2];
    buf[0][threadIdx.x] = v[3];
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {
        const double t = buf[cur][threadIdx.x] + (threadIdx.x >= o ? buf[cur][threadIdx.x - o] : 0.0);
        buf[cur ^ 1][threadIdx.x] = t;
        cur ^= 1;
        __syncthreads();
    }
    const double off = threadIdx.x ? buf[cur][threadIdx.x - 1] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < a.N) a.w.scan[i0 + j] = off + v[j];
    if (threadIdx.x == 255) a.w.bincl[blockIdx.x] = buf[cur][255];
}

// the scan blocks' totals -> inclusive, in block order; the potential
__global__ __launch_bounds__(64) void km_bscan_kernel(KmArgs a) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < a.nscan; ++b) {
        s += a.w.bincl[b];
        a.w.bincl[b] = s;
    }
    a.w.scal[0] = s;
}

// first index i with S(i) >= r, S(i) = (total of the scan blocks before i's) + scan[i]; N - 1 when there is none
__device__ int km_lower_bound(const KmArgs& a, double r) {
    int lo = 0, hi = a.nscan;                       // first block whose inclusive total reaches r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.w.bincl[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= a.nscan) return a.N - 1;
    const double off = lo ? a.w.bincl[lo - 1] : 0.0;
    const long b0 = (long)lo * kKmScan;
    const long left = (long)a.N - b0;
    const int n = left < (long)kKmScan ? (int)left : kKmScan;
    int l = 0, h = n;
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (off + a.w.scan[b0 + mid] < r) l = mid + 1;
        else h = mid;
    }
    return (int)(b0 + min(l, n - 1));
}

// per tile and trial the partial potential sum_i min(closest_i, d(x_i, candidate_t)); block 0 leaves the candidates' indices
__global__ __launch_bounds__(kKmTile) void km_cand_kernel(KmArgs a, int step) {
    extern __shared__ double km_dyn[];
    __shared__ int cid[kKmMaxTrials];
    const int F = a.F, ldx = km_ldx(F), T = a.trials;
    double* tile = km_dyn;                          // kKmTile x ldx
    double* crow = tile + kKmTile * ldx;            // T x F
    double* red = crow + kKmMaxTrials * kKmMaxF;    // T x kKmTile
    if (threadIdx.x < T) {
        const int id = km_lower_bound(a, a.U[(size_t)(step - 1) * T + threadIdx.x] * a.w.scal[0]);
        cid[threadIdx.x] = id;
        if (blockIdx.x == 0) a.w.cand[threadIdx.x] = id;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * F; e += kKmTile) {
        const int t = e / F, c = e - t * F;
        crow[t * kKmMaxF + c] = a.w.Xc[(size_t)cid[t] * F + c];
    }
    const long r0 = (long)blockIdx.x * kKmTile;
    const int rows = km_rows(a.N, r0);
    km_load_tile(a.w.Xc, r0, rows, F, ldx, tile);
    __syncthreads();
    const int p = threadIdx.x;
    const double cl = p < rows ? a.w.closest[r0 + p] : 0.0;
    for (int t = 0; t < T; ++t) {
        double d = 0.0;
        if (p < rows) {
            for (int c = 0; c < F; ++c) {
                const double e = tile[p * ldx + c] - crow[t * kKmMaxF + c];
                d = fma(e, e, d);
            }
            d = fmin(cl, d);
        }
        red[t * kKmTile + p] = d;
    }
    __syncthreads();
    if (threadIdx.x < T) {
        double s = 0.0;
        for (int q = 0; q < kKmTile; ++q) s += red[threadIdx.x * kKmTile + q];
        a.w.ppot[(size_t)blockIdx.x * kKmMaxTrials + threadIdx.x] = s;
    }
}

// centre `step` = the candidate with the smallest potential (step 0: the host's first index); closest <- min(closest, its distances)
__global__ __launch_bounds__(kKmTile) void km_update_kernel(KmArgs a, int step) {
    extern __shared__ double km_dyn[];
    __shared__ double pot[kKmMaxTrials];
    __shared__ int pick;
    const int F = a.F, ldx = km_ldx(F);
    double* tile = km_dyn;
    double* crow = tile + kKmTile * ldx;
    if (step > 0 && threadIdx.x < a.trials) {
        double s = 0.0;
        for (int b = 0; b < a.ntiles; ++b) s += a.w.ppot[(size_t)b * kKmMaxTrials + threadIdx.x];
        pot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int id = a.first;
        if (step > 0) {
            int best = 0;
            for (int t = 1; t < a.trials; ++t)
                if (pot[t] < pot[best]) best = t;
            id = a.w.cand[best];
        }
        pick = min(max(id, 0), a.N - 1);
    }
    __syncthreads();
    if (threadIdx.x < F) {
        const double v = a.w.Xc[(size_t)pick * F + threadIdx.x];
        crow[threadIdx.x] = v;
        if (blockIdx.x == 0) a.w.cen[(size_t)step * F + threadIdx.x] = v;
    }
    const long r0 = (long)blockIdx.x * kKmTile;
    const int rows = km_rows(a.N, r0);
    km_load_tile(a.w.Xc, r0, rows, F, ldx, tile);
    __syncthreads();
    const int p = threadIdx.x;
    if (p < rows) {
        double d = 0.0;
        for (int c = 0; c < F; ++c) {
            const double e = tile[p * ldx + c] - crow[c];
            d = fma(e, e, d);
        }
        a.w.closest[r0 + p] = step > 0 ? fmin(a.w.closest[r0 + p], d) : d;
    }
}

// ------------------------------------------------------------------------------------------------ nearest centre
// 256 threads, 128 points in tile: thread 2 p + h searches half h of the centres for point p; both lanes of the pair return the label.
// The first index wins ties (np.argmin): strict < inside a half, the lower half on equal distances.
__device__ __forceinline__ int km_nearest(const double* tile, int ldx, const double* cen, int K, int F) {
    const int p = threadIdx.x >> 1, h = threadIdx.x & 1, Kh = (K + 1) >> 1;
    const int k0 = h ? Kh : 0, k1 = h ? K : Kh;
    double best = __builtin_inf();
    int bk = k0 < K ? k0 : 0;
    for (int k = k0; k < k1; ++k) {
        double d = 0.0;
        for (int c = 0; c < F; ++c) {
            const double e = tile[p * ldx + c] - cen[k * F + c];
            d = fma(e, e, d);
        }
        if (d < best) best = d, bk = k;
    }
    const double ob = __shfl_xor(best, 1);
    const int ok = __shfl_xor(bk, 1);
    if (ob < best || (ob == best && ok < bk)) bk = ok;
    return bk;
}

// ------------------------------------------------------------------------------------------------ Lloyd
__global__ __launch_bounds__(kKmThreads) void km_assign_kernel(KmArgs a, int it) {
    extern __shared__ double km_dyn[];
    __shared__ int lab[kKmTile];
    __shared__ int changed;
    if (km_done(a)) return;
    const int F = a.F, K = a.K, KF = K * F, ldx = km_ldx(F);
    double* cen = km_dyn;                           // KF
    double* tile = cen + KF;                        // kKmTile x ldx
    double* acc = tile + kKmTile * ldx;             // 4 x KF
    int* cnt = (int*)(acc + 4 * KF);                // 4 x K
    const double* cur = a.w.cen + (size_t)(it & 1) * KF;
    for (int e = threadIdx.x; e < KF; e += kKmThreads) cen[e] = cur[e];
    for (int e = threadIdx.x; e < 4 * KF; e += kKmThreads) acc[e] = 0.0;
    for (int e = threadIdx.x; e < 4 * K; e += kKmThreads) cnt[e] = 0;
    if (threadIdx.x == 0) changed = 0;
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63;
    for (int tl = blockIdx.x; tl < a.ntiles; tl += a.grid) {
        const long r0 = (long)tl * kKmTile;
        const int rows = km_rows(a.N, r0);
        __syncthreads();                            // the previous tile's readers are done; the first pass orders the zeroing
        km_load_tile(a.w.Xc, r0, rows, F, ldx, tile);
        __syncthreads();
        const int p = threadIdx.x >> 1;
        int k = 0;
        if (p < rows) k = km_nearest(tile, ldx, cen, K, F);
        if (p < rows && (threadIdx.x & 1) == 0) {
            lab[p] = k;
            if (a.labels[r0 + p] != k) {
                a.labels[r0 + p] = k;
                changed = 1;
            }
        }
        __syncthreads();
        const int pe = min(32 * wv + 32, rows);
        for (int q = 32 * wv; q < pe; ++q) {        // in point order: the sum's order is fixed
            const int l = lab[q];
            if (c < F) acc[(size_t)wv * KF + l * F + c] += tile[q * ldx + c];
            if (c == 63) cnt[wv * K + l] += 1;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < KF; e += kKmThreads)
        a.w.part[(size_t)blockIdx.x * KF + e] = ((acc[e] + acc[KF + e]) + acc[2 * KF + e]) + acc[3 * KF + e];
    for (int e = threadIdx.x; e < K; e += kKmThreads)
        a.w.pcnt[(size_t)blockIdx.x * K + e] = cnt[e] + cnt[K + e] + cnt[2 * K + e] + cnt[3 * K + e];
    if (threadIdx.x == 0 && changed) atomicOr(a.w.state + KM_CHANGED, 1);
}

// block k: the new centre k = (the blocks' partial sums in block order) * (1 / count), its shift against the old one
__global__ __launch_bounds__(64) void km_combine_kernel(KmArgs a, int it) {
    __shared__ double sq[kKmMaxF];
    if (km_done(a)) return;
    const int F = a.F, K = a.K, KF = K * F, k = blockIdx.x, c = threadIdx.x;
    int n = 0;
    for (int b = 0; b < a.grid; ++b) n += a.w.pcnt[(size_t)b * K + k];
    double d2 = 0.0;
    if (c < F) {
        double s = 0.0;
        for (int b = 0; b < a.grid; ++b) s += a.w.part[(size_t)b * KF + k * F + c];
        const double old = a.w.cen[(size_t)(it & 1) * KF + k * F + c];
        const double nw = n > 0 ? s * (1.0 / (double)n) : old;
        a.w.cen[(size_t)((it + 1) & 1) * KF + k * F + c] = nw;
        d2 = (nw - old) * (nw - old);
    }
    sq[c] = d2;
    __syncthreads();
    if (c == 0) {
        double s = 0.0;
        for (int j = 0; j < F; ++j) s += sq[j];
        a.w.shift[k] = sqrt(s);
        a.w.cnt[k] = n;
    }
}

__global__ __launch_bounds__(256) void km_final_kernel(KmArgs a, int it) {
    __shared__ int stop;
    const bool was_done = km_done(a);
    __syncthreads();                                // every thread has read the word before thread 0 may set it
    if (was_done) return;
    if (threadIdx.x == 0) {
        double tot = 0.0;
        int empty = 0;
        for (int k = 0; k < a.K; ++k) {
            tot += a.w.shift[k] * a.w.shift[k];
            empty |= a.w.cnt[k] == 0 ? 1 : 0;
        }
        const int ch = a.w.state[KM_CHANGED];
        a.w.state[KM_CHANGED] = 0;
        stop = (empty || !ch || tot <= a.w.scal[1] || it == a.max_iter - 1) ? 1 : 0;
        if (stop) {
            a.w.state[KM_NITER] = it + 1;
            a.w.state[KM_STATUS] = empty ? it + 1 : 0;
            *a.n_iter = it + 1;
            *a.status = empty ? it + 1 : 0;
        }
    }
    __syncthreads();
    if (!stop) return;
    const int KF = a.K * a.F;
    const double* cen = a.w.cen + (size_t)((it + 1) & 1) * KF;
    for (int e = threadIdx.x; e < KF; e += 256) a.centers[e] = cen[e] + a.w.mean[e % a.F];
    __syncthreads();
    if (threadIdx.x == 0) a.w.state[KM_DONE] = 1;
}

// ------------------------------------------------------------------------------------------------ SID: assign, histogram, entropy
struct SidArgs {
    const float* x;     // first column of the window of row 0
    long fs;
    int M, F, K, ntiles, grid;
    const double* centers;
    unsigned long long* hist;   // [K]
    double* sid;
    int32_t* labels;    // [M] or null
};

__global__ __launch_bounds__(kKmThreads) void km_sid_assign_kernel(SidArgs a) {
    extern __shared__ double km_dyn[];
    __shared__ int hist[kKmMaxKF];
    const int F = a.F, K = a.K, KF = K * F, ldx = km_ldx(F);
    double* cen = km_dyn;
    double* tile = cen + KF;
    for (int e = threadIdx.x; e < KF; e += kKmThreads) cen[e] = a.centers[e];
    for (int e = threadIdx.x; e < K; e += kKmThreads) hist[e] = 0;
    for (int tl = blockIdx.x; tl < a.ntiles; tl += a.grid) {
        const long r0 = (long)tl * kKmTile;
        const int rows = km_rows(a.M, r0);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * F; e += kKmThreads) {
            const int r = e / F, c = e - r * F;
            tile[r * ldx + c] = (double)a.x[(size_t)(r0 + r) * a.fs + c];
        }
        __syncthreads();
        const int p = threadIdx.x >> 1;
        if (p < rows) {
            const int k = km_nearest(tile, ldx, cen, K, F);
            if ((threadIdx.x & 1) == 0) {
                atomicAdd(&hist[k], 1);
                if (a.labels) a.labels[r0 + p] = k;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < K; e += kKmThreads)
        if (hist[e]) atomicAdd(a.hist + e, (unsigned long long)hist[e]);
}

__global__ __launch_bounds__(64) void km_entropy_kernel(SidArgs a) {
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int k = 0; k < a.K; ++k) tot += (double)a.hist[k];
    double s = 0.0;
    for (int k = 0; k < a.K; ++k) {
        const double h = (double)a.hist[k] / tot;
        s += h * log2(h + 1e-6);
    }
    *a.sid = -s;
}

// the workspace plan; returns the bytes
size_t km_plan(int N, int K, int F, KmWs* w, char* base) {
    const size_t ntiles = ((size_t)N + kKmTile - 1) / kKmTile, nscan = ((size_t)N + kKmScan - 1) / kKmScan;
    const size_t grid = ntiles < (size_t)kKmMaxGrid ? ntiles : (size_t)kKmMaxGrid, KF = (size_t)K * F;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    KmWs t;
    t.state = (int32_t*)take(KM_STATE_WORDS * sizeof(int32_t));
    t.cand = (int32_t*)take(kKmMaxTrials * sizeof(int32_t));
    t.scal = (double*)take(2 * sizeof(double));
    t.mean = (double*)take(kKmMaxF * sizeof(double));
    t.colpart = (double*)take(ntiles * kKmMaxF * sizeof(double));
    t.Xc = (double*)take((size_t)N * F * sizeof(double));
    t.closest = (double*)take((size_t)N * sizeof(double));
    t.scan = (double*)take((size_t)N * sizeof(double));
    t.bincl = (double*)take(nscan * sizeof(double));
    t.ppot = (double*)take(ntiles * kKmMaxTrials * sizeof(double));
    t.cen = (double*)take(2 * KF * sizeof(double));
    t.part = (double*)take(grid * KF * sizeof(double));
    t.pcnt = (int32_t*)take(grid * K * sizeof(int32_t));
    t.shift = (double*)take((size_t)K * sizeof(double));
    t.cnt = (int32_t*)take((size_t)K * sizeof(int32_t));
    t.labels = (int32_t*)take((size_t)N * sizeof(int32_t));
    if (w) *w = t;
    return off;
}

bool km_shape_ok(int K, int F) { return K >= 1 && F >= 1 && F <= kKmMaxF && (long long)K * F <= kKmMaxKF; }

size_t km_assign_lds(int K, int F, bool with_acc) {
    return ((size_t)K * F * (with_acc ? 5 : 1) + (size_t)kKmTile * km_ldx(F)) * sizeof(double) + (with_acc ? (size_t)4 * K * sizeof(int) : 0);
}

}  // namespace
}  // namespace dimx

using namespace dimx;

size_t dimx_op_kmeans_fit_ws_bytes(int N, int K, int F) {
    if (N < 1 || !km_shape_ok(K, F)) return 0;
    return km_plan(N, K, F, nullptr, nullptr);
}

int dimx_op_kmeans_fit(const float* frames, long frame_stride, int N, int W, int c0, int F, int K, int first_index, const double* U,
                       int trials, double tol, int max_iter, double* centers, int32_t* n_iter, int32_t* status, int32_t* labels,
                       void* workspace, size_t workspace_bytes, void* stream) {
    DIMX_REQUIRE(frames && centers && n_iter && status && workspace, DIMX_ERR_ARG, "kmeans_fit: null operand");
    DIMX_REQUIRE(N >= 1 && K >= 1 && F >= 1, DIMX_ERR_ARG, "kmeans_fit: N=%d K=%d F=%d must be positive", N, K, F);
    DIMX_REQUIRE(km_shape_ok(K, F), DIMX_ERR_ARG, "kmeans_fit: K=%d x F=%d centres leave the LDS plan (F <= %d, K * F <= %d)", K, F,
                 kKmMaxF, kKmMaxKF);
    DIMX_REQUIRE(N >= K, DIMX_ERR_ARG, "kmeans_fit: N=%d frames for K=%d clusters", N, K);
    DIMX_REQUIRE(c0 >= 0 && W >= 1 && c0 <= W - F, DIMX_ERR_ARG, "kmeans_fit: columns [%d, %d) leave the row of %d", c0, c0 + F, W);
    DIMX_REQUIRE(frame_stride >= W, DIMX_ERR_ARG, "kmeans_fit: frame stride %ld below the row of %d", frame_stride, W);
    DIMX_REQUIRE(first_index >= 0 && first_index < N, DIMX_ERR_ARG, "kmeans_fit: first_index=%d outside [0, %d)", first_index, N);
    DIMX_REQUIRE(K == 1 || (U && trials >= 1 && trials <= kKmMaxTrials), DIMX_ERR_ARG, "kmeans_fit: trials=%d outside 1..%d or no draws",
                 trials, kKmMaxTrials);
    DIMX_REQUIRE(max_iter >= 1 && max_iter <= 100000 && tol >= 0.0, DIMX_ERR_ARG, "kmeans_fit: max_iter=%d tol=%g", max_iter, tol);
    DIMX_REQUIRE(((uintptr_t)workspace & 255) == 0, DIMX_ERR_ARG, "kmeans_fit: workspace not 256-byte aligned");
    const size_t need = dimx_op_kmeans_fit_ws_bytes(N, K, F);
    DIMX_REQUIRE(workspace_bytes >= need, DIMX_ERR_ARG, "kmeans_fit: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    KmArgs a;
    km_plan(N, K, F, &a.w, (char*)workspace);
    a.x = frames + c0, a.fs = frame_stride;
    a.N = N, a.F = F, a.K = K, a.trials = K > 1 ? trials : 1, a.max_iter = max_iter;
    a.ntiles = (N + kKmTile - 1) / kKmTile, a.nscan = (N + kKmScan - 1) / kKmScan;
    a.grid = a.ntiles < kKmMaxGrid ? a.ntiles : kKmMaxGrid;
    a.first = first_index, a.U = U, a.tol = tol;
    a.centers = centers, a.n_iter = n_iter, a.status = status;
    a.labels = labels ? labels : a.w.labels;
    hipStream_t s = (hipStream_t)stream;
    const int ldx = km_ldx(F);
    const size_t lds_pp = ((size_t)kKmTile * ldx + (size_t)kKmMaxTrials * kKmMaxF + (size_t)kKmMaxTrials * kKmTile) * sizeof(double);
    const size_t lds_as = km_assign_lds(K, F, true);
    // the attributes belong to (function, device): always the largest plan, never this call's own (calls from several host threads)
    const size_t lds_pp_max = ((size_t)kKmTile * km_ldx(kKmMaxF) + (size_t)kKmMaxTrials * kKmMaxF + (size_t)kKmMaxTrials * kKmTile) * sizeof(double);
    const size_t lds_wide = km_assign_lds(kKmMaxKF / kKmMaxF, kKmMaxF, true), lds_many = km_assign_lds(kKmMaxKF, 1, true);
    const size_t lds_as_max = lds_wide > lds_many ? lds_wide : lds_many;   // tile + counters over F at K * F = 2048: largest at an end
    DIMX_HIP(hipFuncSetAttribute((const void*)km_cand_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pp_max));
    DIMX_HIP(hipFuncSetAttribute((const void*)km_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pp_max));
    DIMX_HIP(hipFuncSetAttribute((const void*)km_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_as_max));
    DIMX_HIP(hipMemsetAsync(a.w.state, 0, KM_STATE_WORDS * sizeof(int32_t), s));
    hipLaunchKernelGGL(km_colsum_kernel<false>, dim3(a.ntiles), dim3(kKmThreads), 0, s, a);
    hipLaunchKernelGGL(km_mean_kernel<false>, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(km_colsum_kernel<true>, dim3(a.ntiles), dim3(kKmThreads), 0, s, a);
    hipLaunchKernelGGL(km_mean_kernel<true>, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(km_update_kernel, dim3(a.ntiles), dim3(kKmTile), lds_pp, s, a, 0);
    DIMX_HIP(hipGetLastError());
    for (int st = 1; st < K; ++st) {
        hipLaunchKernelGGL(km_scan_kernel, dim3(a.nscan), dim3(256), 0, s, a);
        hipLaunchKernelGGL(km_bscan_kernel, dim3(1), dim3(64), 0, s, a);
        hipLaunchKernelGGL(km_cand_kernel, dim3(a.ntiles), dim3(kKmTile), lds_pp, s, a, st);
        hipLaunchKernelGGL(km_update_kernel, dim3(a.ntiles), dim3(kKmTile), lds_pp, s, a, st);
    }
    DIMX_HIP(hipGetLastError());
    for (int it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(km_assign_kernel, dim3(a.grid), dim3(kKmThreads), lds_as, s, a, it);
        hipLaunchKernelGGL(km_combine_kernel, dim3(K), dim3(64), 0, s, a, it);
        hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(256), 0, s, a, it);
    }
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}

int dimx_op_sid_assign(const float* frames, long frame_stride, int M, int W, int c0, int F, const double* centers, int K, int64_t* hist,
                       double* sid, int32_t* labels, void* stream) {
    DIMX_REQUIRE(frames && centers && hist && sid, DIMX_ERR_ARG, "sid_assign: null operand");
    DIMX_REQUIRE(M >= 1 && K >= 1 && F >= 1, DIMX_ERR_ARG, "sid_assign: M=%d K=%d F=%d must be positive", M, K, F);
    DIMX_REQUIRE(km_shape_ok(K, F), DIMX_ERR_ARG, "sid_assign: K=%d x F=%d centres leave the LDS plan (F <= %d, K * F <= %d)", K, F,
                 kKmMaxF, kKmMaxKF);
    DIMX_REQUIRE(c0 >= 0 && W >= 1 && c0 <= W - F, DIMX_ERR_ARG, "sid_assign: columns [%d, %d) leave the row of %d", c0, c0 + F, W);
    DIMX_REQUIRE(frame_stride >= W, DIMX_ERR_ARG, "sid_assign: frame stride %ld below the row of %d", frame_stride, W);
    SidArgs a;
    a.x = frames + c0, a.fs = frame_stride, a.M = M, a.F = F, a.K = K;
    a.ntiles = (M + kKmTile - 1) / kKmTile;
    a.grid = a.ntiles < kKmMaxGrid ? a.ntiles : kKmMaxGrid;
    a.centers = centers, a.hist = (unsigned long long*)hist, a.sid = sid, a.labels = labels;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds_max = ((size_t)kKmMaxKF + (size_t)kKmTile * km_ldx(kKmMaxF)) * sizeof(double);
    DIMX_HIP(hipFuncSetAttribute((const void*)km_sid_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    DIMX_HIP(hipMemsetAsync(hist, 0, (size_t)K * sizeof(int64_t), s));
    hipLaunchKernelGGL(km_sid_assign_kernel, dim3(a.grid), dim3(kKmThreads), km_assign_lds(K, F, false), s, a);
    hipLaunchKernelGGL(km_entropy_kernel, dim3(1), dim3(64), 0, s, a);
    DIMX_HIP(hipGetLastError());
    return DIMX_OK;
}
