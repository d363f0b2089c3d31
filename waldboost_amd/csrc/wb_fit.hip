// Split search of the FPGA flavour's weak learner on the device (wb_fit_level_launch, wb_fit_route_launch): what
// reference fpga/training.py:15-57 (H, _fit_threshold, _find_split) computes for every open node of one tree level, and
// the routing of :133-138.  tests/fit_reference.py is the NumPy statement.
//
// Semantics, per open node with sample set S and per entry f of the ordered feature list A:
//   * candidates are the integers t = xmin .. xmax + 1, xmin / xmax over ALL samples of S (both classes, any weight);
//   * L_c(t) = sum of the class-c weights of S with x_f < t, T_c = L_c(xmax + 1), R_c = T_c - L_c;
//   * M(f, t) = H(T0, T1) - ((L0 + L1) / (T0 + T1) * H(L0 + 1e-4, L1 + 1e-4) + (R0 + R1) / (T0 + T1) * H(R0 + 1e-4, R1 + 1e-4)),
//     H(a, b) = -(a / (a + b) * log2(a / (a + b)) + b / (a + b) * log2(b / (a + b))), float64, every operation rounded on
//     its own (this file is built with -ffp-contract=off);
//   * the smallest t with the largest M wins per feature, the first entry of A with the largest M per node; a NaN is the
//     largest value (np.argmax), so a node without weight in one class answers (A[0], its xmin).
//
// Weights are 64-bit integers q = rint(w' * 2^62) (w' sums to 0.5 per class, so a class's sum is about 2^61): every sum is
// an integer add, hence independent of the order of samples, lanes, waves and runs; a sum converts back as
// double(sum) * 2^-62.
//
// Kernels:
//   fit_hist_kernel   one workgroup per entry of A, all open nodes of the level (at most WB_FIT_MAX_OPEN) at once.  Phase 1
//                     walks the feature's column (feature-major samples: 256 contiguous bytes per step) and adds q into
//                     hist[node][class][value] in LDS with 64-bit LDS atomics.  Value 0 -- most of a grad_hist_4_u1 sample
//                     -- would serialise a wave on one address, so it goes to a lane-private copy zero[node][class][lane]
//                     instead (lane = thread % 64: the 64 lanes of a wave add to 64 different addresses; the workgroup's
//                     four waves share the copy, so an address is contended four ways at the most, across waves, and
//                     the adds stay atomic) that is folded into bin 0 afterwards.  xmin / xmax
//                     are kept per thread in registers and merged once with LDS min / max.  Phase 2 turns every histogram
//                     into its inclusive prefix sum in place, phase 3 rates the 257 candidates (thread j rates t = j,
//                     thread 0 also t = 256) and reduces them to one record (metric, t) per (node, entry of A).
//   fit_pick_kernel   one workgroup per open node: the first best record over A -> WbFitSplit.  Both argmaxes end in
//                     wb_best_reduce (wb_best_reduce.h, shared with wb_cart.hip) under FitBest's order.
//   fit_route_kernel  one thread per sample: a sample of an open node moves to the node's left child when
//                     x[feature] <= t, to the right child otherwise.
// No accumulation crosses workgroups; no kernel uses scratch memory.
#include "wb_best_reduce.h"
#include "wb_common.h"

#define WB_FIT_THREADS 256
#define WB_FIT_SCALE 0x1p-62

namespace {

struct FitLevel {                   // the level's nodes: tree ids level_base .. level_base + n_level - 1
    int32_t level_base, n_level, n_open;
    int8_t slot[WB_FIT_MAX_OPEN];   // open slot (0 .. n_open - 1) of the level's j-th node, -1 for a leaf
};

__device__ inline int fit_slot(const FitLevel &lv, int32_t node) {
    const int32_t rel = node - lv.level_base;
    int s = -1;
#pragma unroll
    for (int j = 0; j < WB_FIT_MAX_OPEN; ++j) s = (rel == j && j < lv.n_level) ? (int)lv.slot[j] : s;
    return s;
}

// One candidate of an argmax in np.argmax's order: rank 2 = NaN (beats every number), 1 = a number, 0 = no candidate;
// among equals the smaller index.
struct FitBest {
    double m;
    int32_t idx, rank;
    __device__ static bool better(const FitBest &a, const FitBest &b) {
        if (a.rank != b.rank) return a.rank > b.rank;
        if (a.rank == 1 && a.m != b.m) return a.m > b.m;
        return a.idx < b.idx;
    }
};
static_assert(sizeof(FitBest) == 16, "FitBest is 4 dwords, no padding");

__device__ inline FitBest fit_make(double m, int32_t idx) {
    FitBest c;
    c.m = m;
    c.idx = idx;
    c.rank = m != m ? 2 : 1;
    return c;
}

__device__ inline double fit_entropy(double a, double b) {
    const double tot = a + b;
    const double pa = a / tot, pb = b / tot;
    return -(pa * log2(pa) + pb * log2(pb));
}

__global__ __launch_bounds__(WB_FIT_THREADS) void fit_hist_kernel(
        const uint8_t *__restrict__ xt, int64_t n_samples, int64_t n_features, const unsigned long long *__restrict__ q,
        const uint8_t *__restrict__ cls, const int32_t *__restrict__ node, FitLevel lv, const int32_t *__restrict__ allowed,
        int n_allowed, double *__restrict__ rec_metric, int32_t *__restrict__ rec_t, double *__restrict__ totals) {
    extern __shared__ unsigned long long fit_lds[];
    const int n_open = lv.n_open;
    unsigned long long *hist = fit_lds;                                    // [n_open][2][256]
    unsigned long long *zero = hist + (size_t)n_open * 512;                // [n_open][2][64]
    __shared__ int smin[WB_FIT_MAX_OPEN], smax[WB_FIT_MAX_OPEN];
    __shared__ FitBest part[WB_FIT_THREADS / WB_WAVE];
    const int tid = threadIdx.x, lane = tid % WB_WAVE;
    const int a = blockIdx.x;
    const int64_t f = allowed[a];

    for (int i = tid; i < n_open * 640; i += WB_FIT_THREADS) fit_lds[i] = 0ull;
    if (tid < WB_FIT_MAX_OPEN) {
        smin[tid] = 256;
        smax[tid] = -1;
    }
    __syncthreads();

    const bool f_ok = f >= 0 && f < n_features;                            // (the caller checks; never read outside)
    int mn[WB_FIT_MAX_OPEN], mx[WB_FIT_MAX_OPEN];
#pragma unroll
    for (int k = 0; k < WB_FIT_MAX_OPEN; ++k) {
        mn[k] = 256;
        mx[k] = -1;
    }
    if (f_ok) {
        const uint8_t *col = xt + (size_t)f * (size_t)n_samples;
        for (int64_t i = tid; i < n_samples; i += WB_FIT_THREADS) {
            const int s = fit_slot(lv, node[i]);
            if (s < 0) continue;
            const int x = col[i];
            const int sc = s * 2 + (cls[i] != 0 ? 1 : 0);
            const unsigned long long w = q[i];
#pragma unroll
            for (int k = 0; k < WB_FIT_MAX_OPEN; ++k) {
                mn[k] = (s == k && x < mn[k]) ? x : mn[k];
                mx[k] = (s == k && x > mx[k]) ? x : mx[k];
            }
            if (w != 0ull) atomicAdd(&fit_lds[x == 0 ? n_open * 512 + sc * WB_WAVE + lane : sc * 256 + x], w);
        }
    }
#pragma unroll
    for (int k = 0; k < WB_FIT_MAX_OPEN; ++k) {
        if (mx[k] >= 0) {
            atomicMin(&smin[k], mn[k]);
            atomicMax(&smax[k], mx[k]);
        }
    }
    __syncthreads();
    if (tid < n_open * 2) {
        unsigned long long z = 0ull;
        for (int l = 0; l < WB_WAVE; ++l) z += zero[tid * WB_WAVE + l];
        hist[tid * 256] += z;
    }
    __syncthreads();

    // inclusive prefix sums over the 256 bins of every histogram, in place (thread j owns bin j)
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long add[2 * WB_FIT_MAX_OPEN];
#pragma unroll
        for (int h = 0; h < 2 * WB_FIT_MAX_OPEN; ++h) add[h] = (h < n_open * 2 && tid >= off) ? hist[h * 256 + tid - off] : 0ull;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2 * WB_FIT_MAX_OPEN; ++h)
            if (h < n_open * 2) hist[h * 256 + tid] += add[h];
        __syncthreads();
    }

    for (int k = 0; k < n_open; ++k) {
        const unsigned long long *h0 = hist + (size_t)k * 512, *h1 = h0 + 256;
        const int xmin = smin[k], xmax = smax[k];
        const double t0 = (double)h0[255] * WB_FIT_SCALE, t1 = (double)h1[255] * WB_FIT_SCALE;
        const double tsum = t0 + t1;
        const double h_all = fit_entropy(t0, t1);
        FitBest best;
        best.m = 0.0;
        best.idx = 0x7fffffff;
        best.rank = 0;
        for (int t = tid; t <= 256; t += WB_FIT_THREADS) {
            if (t < xmin || t > xmax + 1) continue;
            const double l0 = t == 0 ? 0.0 : (double)h0[t - 1] * WB_FIT_SCALE;
            const double l1 = t == 0 ? 0.0 : (double)h1[t - 1] * WB_FIT_SCALE;
            const double r0 = t0 - l0, r1 = t1 - l1;
            const double lw = (l0 + l1) / tsum, rw = (r0 + r1) / tsum;
            const double m = h_all - (lw * fit_entropy(l0 + 1e-4, l1 + 1e-4) + rw * fit_entropy(r0 + 1e-4, r1 + 1e-4));
            const FitBest c = fit_make(m, t);
            if (FitBest::better(c, best)) best = c;
        }
        best = wb_best_reduce<WB_FIT_THREADS / WB_WAVE>(best, part);
        if (tid == 0) {
            const bool ok = f_ok && best.rank != 0;                         // (an open node holds samples, so rank != 0)
            rec_metric[(size_t)k * n_allowed + a] = ok ? best.m : -__builtin_inf();
            rec_t[(size_t)k * n_allowed + a] = ok ? best.idx : 0;
            if (a == 0) {
                totals[2 * k] = t0;
                totals[2 * k + 1] = t1;
            }
        }
    }
}

__global__ __launch_bounds__(WB_FIT_THREADS) void fit_pick_kernel(const double *__restrict__ rec_metric,
                                                                  const int32_t *__restrict__ rec_t,
                                                                  const double *__restrict__ totals,
                                                                  const int32_t *__restrict__ allowed, int n_allowed,
                                                                  WbFitSplit *__restrict__ out) {
    __shared__ FitBest part[WB_FIT_THREADS / WB_WAVE];
    const int k = blockIdx.x;
    FitBest best;
    best.m = 0.0;
    best.idx = 0x7fffffff;
    best.rank = 0;
    for (int a = threadIdx.x; a < n_allowed; a += WB_FIT_THREADS) {
        const FitBest c = fit_make(rec_metric[(size_t)k * n_allowed + a], a);
        if (FitBest::better(c, best)) best = c;
    }
    best = wb_best_reduce<WB_FIT_THREADS / WB_WAVE>(best, part);
    if (threadIdx.x == 0) {
        WbFitSplit s;
        s.feature = allowed[best.idx];
        s.threshold = rec_t[(size_t)k * n_allowed + best.idx];
        s.metric = best.m;
        s.t0 = totals[2 * k];
        s.t1 = totals[2 * k + 1];
        out[k] = s;
    }
}

__global__ __launch_bounds__(WB_FIT_THREADS) void fit_route_kernel(const uint8_t *__restrict__ xt, int64_t n_samples,
                                                                   int64_t n_features, int32_t *__restrict__ node, FitLevel lv,
                                                                   const WbFitSplit *__restrict__ splits, int32_t child_base) {
    const int64_t i = (int64_t)blockIdx.x * WB_FIT_THREADS + threadIdx.x;
    if (i >= n_samples) return;
    const int s = fit_slot(lv, node[i]);
    if (s < 0) return;
    const int64_t f = splits[s].feature;
    if (f < 0 || f >= n_features) return;
    const int x = xt[(size_t)f * (size_t)n_samples + (size_t)i];
    node[i] = child_base + 2 * s + (x <= splits[s].threshold ? 0 : 1);
}

size_t fit_records_bytes(int n_allowed, int n_open) {
    return ((size_t)n_open * (size_t)n_allowed * 8 + 15) / 16 * 16;
}

int fit_level(const char *who, int level_base, int n_level, const int8_t *slot, int n_open, FitLevel *lv) {
    WB_REQUIRE(slot != nullptr, "%s: null pointer", who);
    WB_REQUIRE(n_level >= 1 && n_level <= WB_FIT_MAX_OPEN && level_base >= 0, "%s: a level has 1 .. %d nodes", who, WB_FIT_MAX_OPEN);
    WB_REQUIRE(n_open >= 1 && n_open <= n_level, "%s: 1 .. n_level open nodes", who);
    lv->level_base = level_base;
    lv->n_level = n_level;
    lv->n_open = n_open;
    int seen = 0;
    for (int j = 0; j < WB_FIT_MAX_OPEN; ++j) {
        lv->slot[j] = j < n_level ? slot[j] : (int8_t)-1;
        if (j < n_level) {
            WB_REQUIRE(slot[j] >= -1 && slot[j] < n_open, "%s: slot[%d] = %d outside -1 .. n_open - 1", who, j, (int)slot[j]);
            if (slot[j] >= 0) {
                WB_REQUIRE(!(seen >> slot[j] & 1), "%s: slot %d given twice", who, (int)slot[j]);
                seen |= 1 << slot[j];
            }
        }
    }
    WB_REQUIRE(seen == (1 << n_open) - 1, "%s: every slot 0 .. n_open - 1 must belong to one node", who);
    return WB_OK;
}

}  // namespace

extern "C" int wb_fit_scratch_bytes(int n_allowed, int n_open, size_t *bytes) {
    WB_REQUIRE(bytes != nullptr, "wb_fit_scratch_bytes: null pointer");
    WB_REQUIRE(n_allowed >= 1 && n_open >= 1 && n_open <= WB_FIT_MAX_OPEN, "wb_fit_scratch_bytes: n_allowed >= 1, n_open 1 .. %d",
               WB_FIT_MAX_OPEN);
    // float64 metric and (behind them) int32 threshold per (open node, entry), then float64 T0, T1 per open node
    *bytes = fit_records_bytes(n_allowed, n_open) + fit_records_bytes(n_allowed, n_open) / 2 + (size_t)WB_FIT_MAX_OPEN * 16;
    return WB_OK;
}

extern "C" int wb_fit_level_launch(void *stream, const uint8_t *xt, int64_t n_samples, int64_t n_features, const uint64_t *q,
                                   const uint8_t *cls, const int32_t *node, int level_base, int n_level, const int8_t *slot,
                                   int n_open, const int32_t *allowed, int n_allowed, void *scratch, size_t scratch_bytes,
                                   WbFitSplit *splits) {
    FitLevel lv;
    if (int rc = fit_level("wb_fit_level_launch", level_base, n_level, slot, n_open, &lv)) return rc;
    WB_REQUIRE(xt && q && cls && node && allowed && scratch && splits, "wb_fit_level_launch: null pointer");
    WB_REQUIRE(n_samples >= 1 && n_features >= 1 && n_allowed >= 1, "wb_fit_level_launch: empty problem");
    WB_REQUIRE(n_samples <= 0x7fffffff, "wb_fit_level_launch: at most 2^31 - 1 samples");
    WB_REQUIRE(wb_aligned(q, 8) && wb_aligned(node, 4) &&
               wb_aligned(allowed, 4) && wb_aligned(scratch, 16) &&
               wb_aligned(splits, 8), "wb_fit_level_launch: misaligned pointer");
    size_t need = 0;
    if (int rc = wb_fit_scratch_bytes(n_allowed, n_open, &need)) return rc;
    WB_REQUIRE(scratch_bytes >= need, "wb_fit_level_launch: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    uint8_t *s = static_cast<uint8_t *>(scratch);
    double *rec_metric = reinterpret_cast<double *>(s);
    int32_t *rec_t = reinterpret_cast<int32_t *>(s + fit_records_bytes(n_allowed, n_open));
    double *totals = reinterpret_cast<double *>(s + fit_records_bytes(n_allowed, n_open) + fit_records_bytes(n_allowed, n_open) / 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)n_open * 640 * 8;        // hist 4 KiB + zero-bin copies 1 KiB per open node
    hipLaunchKernelGGL(fit_hist_kernel, dim3(n_allowed), dim3(WB_FIT_THREADS), lds, st, xt, n_samples, n_features,
                       reinterpret_cast<const unsigned long long *>(q), cls, node, lv, allowed, n_allowed, rec_metric, rec_t, totals);
    WB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fit_pick_kernel, dim3(n_open), dim3(WB_FIT_THREADS), 0, st, rec_metric, rec_t, totals, allowed, n_allowed, splits);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_fit_route_launch(void *stream, const uint8_t *xt, int64_t n_samples, int64_t n_features, int32_t *node,
                                   int level_base, int n_level, const int8_t *slot, int n_open, const WbFitSplit *splits,
                                   int child_base) {
    FitLevel lv;
    if (int rc = fit_level("wb_fit_route_launch", level_base, n_level, slot, n_open, &lv)) return rc;
    WB_REQUIRE(xt && node && splits, "wb_fit_route_launch: null pointer");
    WB_REQUIRE(n_samples >= 1 && n_samples <= 0x7fffffff && n_features >= 1, "wb_fit_route_launch: 1 .. 2^31 - 1 samples");
    WB_REQUIRE(child_base >= level_base + n_level, "wb_fit_route_launch: children are numbered behind their level");
    WB_REQUIRE(wb_aligned(node, 4) && wb_aligned(splits, 8),
               "wb_fit_route_launch: misaligned pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n_samples + WB_FIT_THREADS - 1) / WB_FIT_THREADS);
    hipLaunchKernelGGL(fit_route_kernel, dim3(blocks), dim3(WB_FIT_THREADS), 0, st, xt, n_samples, n_features, node, lv, splits,
                       (int32_t)child_base);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
