// Split search of the base weak learner on float32 samples (wb_cart_sort_launch, wb_cart_level_launch): what
// scikit-learn's DecisionTreeClassifier(class_weight="balanced"), gini criterion, best splitter -- the learner behind
// reference training.py:33-50 -- computes for the open nodes of one tree level.  tests/cart_reference.py is the NumPy
// statement.
//
// Semantics, per open node with n samples, integer class totals T0, T1, and per feature f:
//   * the node's samples sorted by the float32 value x_f (-0.0 equal to +0.0) are xs[0 .. n-1]; the feature is constant,
//     and skipped, when xs[n-1] <= xs[0] + 1e-7f (float32 add);
//   * position p = 1 .. n-1 is a candidate when xs[p] > xs[p-1] + 1e-7f (float32 add, the node's own neighbours) and
//     p >= min_samples_leaf and n - p >= min_samples_leaf;
//   * L_c = class-c sum of the first p sorted samples, R_c = T_c - L_c (64-bit integer operations), each converted to
//     float64 once and scaled by `scale` (a power of two: exact); proxy = (l0*l0 + l1*l1)/(l0+l1) + (r0*r0 + r1*r1)/(r0+r1),
//     float64, every operation rounded on its own (this file is built with -ffp-contract=off); a NaN proxy never wins;
//   * the largest proxy wins; among equal proxies the smallest feature index, then the smallest p;
//   * the node routes a sample left when double(x_f) <= threshold, threshold = xs[p-1]/2.0 + xs[p]/2.0 in float64,
//     replaced by xs[p-1] if it equals xs[p] or is infinite.
//
// Weights are 64-bit integers, so every sum is an integer add and does not depend on the order of equal values, of lanes,
// of waves or on the run.
//
// Kernels:
//   cart_sort_kernel  once per fit, one workgroup per feature column: order[f] = the sample indices sorted by
//                     (key(x_f), index), key the order-preserving uint32 image of the float with -0.0 folded onto +0.0.
//                     A bitonic network with all comparators ascending (so that positions past n, virtual +inf, never
//                     move): chunks of WB_CART_SORT_CHUNK elements are sorted in LDS, the strides that span chunks
//                     compare in global memory (the column belongs to this workgroup alone), the strides below a chunk
//                     run in LDS again.
//   cart_scan_kernel  one workgroup per feature.  order[f] is kept partitioned by node (cart_part_kernel), so an open node
//                     is the segment begin .. end of every column and a sample's predecessor within the node is its
//                     neighbour.  The workgroup walks the segment 256 positions at a time with an exclusive scan of the
//                     two class sums (wave shuffles, then the four wave totals through LDS, a running carry across
//                     steps), rates its candidates and reduces them to one record per (node, feature).
//   cart_best_kernel  one workgroup per open node: the first best record over the features -> WbCartSplit.  Both
//                     reductions are wb_best_reduce (wb_best_reduce.h, shared with wb_fit.hip) under CartBest's order.
//   cart_move_kernel  one thread per position of the open segments: the sample there moves to the node's left or right
//                     child (node[sample] = child_base + 2 * slot + side).
//   cart_part_kernel  one workgroup per feature: the stable partition of every split segment into left | right.
// No accumulation crosses workgroups, no floating-point atomics; no kernel uses scratch memory.
#include "wb_best_reduce.h"
#include "wb_common.h"

#define WB_CART_THREADS 256
#define WB_CART_WAVES (WB_CART_THREADS / WB_WAVE)
#define WB_CART_SORT_THREADS 512
#define WB_CART_SORT_CHUNK 4096
#define WB_CART_FEATURE_THRESHOLD 1e-7f

namespace {

struct CartLevel {
    int32_t n_open, min_leaf, child_base, pad;
    int32_t begin[WB_FIT_MAX_OPEN], end[WB_FIT_MAX_OPEN];
    unsigned long long t0[WB_FIT_MAX_OPEN], t1[WB_FIT_MAX_OPEN];
    double scale;
};

__device__ inline uint32_t cart_key(float x) {
    uint32_t b = __float_as_uint(x);
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (key, index) a sorts behind (key, index) b
__device__ inline bool cart_behind(uint32_t ka, uint32_t ia, uint32_t kb, uint32_t ib) { return ka > kb || (ka == kb && ia > ib); }

__device__ inline double cart_threshold(float lo, float hi) {
    double t = (double)lo / 2.0 + (double)hi / 2.0;
    if (t == (double)hi || t == __builtin_inf() || t == -__builtin_inf()) t = (double)lo;
    return t;
}

// ---- sort
__device__ inline void cart_lds_exchange(uint32_t *skey, uint32_t *sidx, int i, int l) {
    const uint32_t ki = skey[i], kl = skey[l], ii = sidx[i], il = sidx[l];
    if (cart_behind(ki, ii, kl, il)) {
        skey[i] = kl;
        skey[l] = ki;
        sidx[i] = il;
        sidx[l] = ii;
    }
}

// the half-cleaners of strides j0, j0 / 2 .. 1 over the `len` elements in LDS
__device__ inline void cart_lds_strides(uint32_t *skey, uint32_t *sidx, int len, int j0) {
    for (int j = j0; j >= 1; j >>= 1) {
        for (int t = threadIdx.x; t < len / 2; t += WB_CART_SORT_THREADS) {
            const int i = (t / j) * 2 * j + t % j;
            cart_lds_exchange(skey, sidx, i, i + j);
        }
        __syncthreads();
    }
}

__device__ inline void cart_global_exchange(const float *col, int32_t *ord, int n, int i, int l) {
    if (l >= n) return;                                     // (a virtual +inf: stays where it is)
    const uint32_t oi = (uint32_t)ord[i], ol = (uint32_t)ord[l];
    if (cart_behind(cart_key(col[oi]), oi, cart_key(col[ol]), ol)) {
        ord[i] = (int32_t)ol;
        ord[l] = (int32_t)oi;
    }
}

__global__ __launch_bounds__(WB_CART_SORT_THREADS) void cart_sort_kernel(const float *xt, int n, int32_t *order) {
    __shared__ uint32_t skey[WB_CART_SORT_CHUNK], sidx[WB_CART_SORT_CHUNK];
    const float *col = xt + (size_t)blockIdx.x * (size_t)n;
    int32_t *ord = order + (size_t)blockIdx.x * (size_t)n;
    const int tid = threadIdx.x;
    int P = 2;                                              // the network's size: a power of two >= n
    while (P < n) P <<= 1;
    const int len = P < WB_CART_SORT_CHUNK ? P : WB_CART_SORT_CHUNK;

    // every chunk sorted on its own
    for (int base = 0; base < n; base += len) {
        for (int t = tid; t < len; t += WB_CART_SORT_THREADS) {
            const int i = base + t;
            skey[t] = i < n ? cart_key(col[i]) : 0xffffffffu;
            sidx[t] = i < n ? (uint32_t)i : 0xffffffffu;
        }
        __syncthreads();
        for (int k = 2; k <= len; k <<= 1) {
            for (int t = tid; t < len / 2; t += WB_CART_SORT_THREADS) {
                const int blk = t / (k / 2), low = t % (k / 2);
                cart_lds_exchange(skey, sidx, blk * k + low, blk * k + k - 1 - low);
            }
            __syncthreads();
            cart_lds_strides(skey, sidx, len, k >> 2);
        }
        for (int t = tid; t < len; t += WB_CART_SORT_THREADS)
            if (base + t < n) ord[base + t] = (int32_t)sidx[t];
        __syncthreads();
    }

    // merges of sorted runs longer than a chunk
    for (int k = 2 * WB_CART_SORT_CHUNK; k <= P; k <<= 1) {
        for (int t = tid; t < P / 2; t += WB_CART_SORT_THREADS) {
            const int blk = t / (k / 2), low = t % (k / 2);
            cart_global_exchange(col, ord, n, blk * k + low, blk * k + k - 1 - low);
        }
        __syncthreads();
        for (int j = k >> 2; j >= WB_CART_SORT_CHUNK; j >>= 1) {
            for (int t = tid; t < P / 2; t += WB_CART_SORT_THREADS) {
                const int i = (t / j) * 2 * j + t % j;
                cart_global_exchange(col, ord, n, i, i + j);
            }
            __syncthreads();
        }
        for (int base = 0; base < n; base += WB_CART_SORT_CHUNK) {
            for (int t = tid; t < WB_CART_SORT_CHUNK; t += WB_CART_SORT_THREADS) {
                const int i = base + t;
                const uint32_t o = i < n ? (uint32_t)ord[i] : 0xffffffffu;
                skey[t] = i < n ? cart_key(col[o]) : 0xffffffffu;
                sidx[t] = o;
            }
            __syncthreads();
            cart_lds_strides(skey, sidx, WB_CART_SORT_CHUNK, WB_CART_SORT_CHUNK / 2);
            for (int t = tid; t < WB_CART_SORT_CHUNK; t += WB_CART_SORT_THREADS)
                if (base + t < n) ord[base + t] = (int32_t)sidx[t];
            __syncthreads();
        }
    }
}

// ---- split search
// One candidate: ok = 0 is "none"; the larger proxy wins, among equals the smaller idx (a position, or a feature).
struct CartBest {
    double m;
    int32_t idx, ok;
    float lo, hi;
    __device__ static bool better(const CartBest &a, const CartBest &b) {
        if (a.ok != b.ok) return a.ok > b.ok;
        if (!a.ok) return false;
        if (a.m != b.m) return a.m > b.m;
        return a.idx < b.idx;
    }
};
static_assert(sizeof(CartBest) == 24, "CartBest is 6 dwords, no padding");

__device__ inline CartBest cart_none() {
    CartBest c;
    c.m = -__builtin_inf();
    c.idx = 0x7fffffff;
    c.ok = 0;
    c.lo = 0.0f;
    c.hi = 0.0f;
    return c;
}

__device__ inline double cart_half_proxy(double a, double b) { return (a * a + b * b) / (a + b); }

__global__ __launch_bounds__(WB_CART_THREADS) void cart_scan_kernel(
        const float *__restrict__ xt, int n_samples, int n_features, const unsigned long long *__restrict__ q,
        const uint8_t *__restrict__ cls, const int32_t *__restrict__ order, CartLevel lv, double *__restrict__ rec_proxy,
        int32_t *__restrict__ rec_p, float *__restrict__ rec_lo, float *__restrict__ rec_hi) {
    __shared__ unsigned long long wsum[2][WB_CART_WAVES];
    __shared__ CartBest part[WB_CART_WAVES];
    const int tid = threadIdx.x, lane = tid % WB_WAVE, wave = tid / WB_WAVE;
    const int f = blockIdx.x;
    const float *col = xt + (size_t)f * (size_t)n_samples;
    const int32_t *ord = order + (size_t)f * (size_t)n_samples;

    for (int k = 0; k < lv.n_open; ++k) {
        const int b = lv.begin[k], e = lv.end[k], n = e - b;
        const unsigned long long T0 = lv.t0[k], T1 = lv.t1[k];
        CartBest best = cart_none();
        const float x_first = col[ord[b]], x_last = col[ord[e - 1]];
        if (!(x_last <= x_first + WB_CART_FEATURE_THRESHOLD)) {       // (the same for every thread)
            unsigned long long c0 = 0ull, c1 = 0ull;                   // class sums of the positions before `base`
            for (int base = b; base < e; base += WB_CART_THREADS) {
                const int i = base + tid;
                const bool valid = i < e;
                const int s = valid ? ord[i] : 0;
                const float x = valid ? col[s] : 0.0f;
                const unsigned long long w = valid ? q[s] : 0ull;
                const bool one = valid && cls[s] != 0;
                const unsigned long long a0 = one ? 0ull : w, a1 = one ? w : 0ull;
                unsigned long long v0 = a0, v1 = a1;                   // inclusive sums within the wave
#pragma unroll
                for (int off = 1; off < WB_WAVE; off <<= 1) {
                    const unsigned long long u0 = __shfl_up(v0, off), u1 = __shfl_up(v1, off);
                    if (lane >= off) {
                        v0 += u0;
                        v1 += u1;
                    }
                }
                if (lane == WB_WAVE - 1) {
                    wsum[0][wave] = v0;
                    wsum[1][wave] = v1;
                }
                __syncthreads();
                unsigned long long L0 = c0 + v0 - a0, L1 = c1 + v1 - a1;   // sums of the positions before i
#pragma unroll
                for (int w2 = 0; w2 < WB_CART_WAVES; ++w2) {
                    L0 += w2 < wave ? wsum[0][w2] : 0ull;
                    L1 += w2 < wave ? wsum[1][w2] : 0ull;
                    c0 += wsum[0][w2];
                    c1 += wsum[1][w2];
                }
                __syncthreads();                                        // (wsum is written again in the next step)
                const int p = i - b;
                if (valid && p >= 1 && p >= lv.min_leaf && n - p >= lv.min_leaf) {
                    const float x_prev = col[ord[i - 1]];
                    if (x > x_prev + WB_CART_FEATURE_THRESHOLD) {
                        const double l0 = (double)L0 * lv.scale, l1 = (double)L1 * lv.scale;
                        const double r0 = (double)(T0 - L0) * lv.scale, r1 = (double)(T1 - L1) * lv.scale;
                        const double m = cart_half_proxy(l0, l1) + cart_half_proxy(r0, r1);
                        CartBest c;
                        c.m = m;
                        c.idx = p;
                        c.ok = m == m ? 1 : 0;
                        c.lo = x_prev;
                        c.hi = x;
                        if (CartBest::better(c, best)) best = c;
                    }
                }
            }
        }
        best = wb_best_reduce<WB_CART_WAVES>(best, part);
        if (tid == 0) {
            const size_t r = (size_t)k * (size_t)n_features + (size_t)f;
            rec_proxy[r] = best.ok ? best.m : -__builtin_inf();
            rec_p[r] = best.ok ? best.idx : 0;
            rec_lo[r] = best.lo;
            rec_hi[r] = best.hi;
        }
    }
}

__global__ __launch_bounds__(WB_CART_THREADS) void cart_best_kernel(const double *__restrict__ rec_proxy,
                                                                    const int32_t *__restrict__ rec_p,
                                                                    const float *__restrict__ rec_lo,
                                                                    const float *__restrict__ rec_hi, int n_features,
                                                                    CartLevel lv, WbCartSplit *__restrict__ out) {
    __shared__ CartBest part[WB_CART_WAVES];
    const int k = blockIdx.x;
    const size_t row = (size_t)k * (size_t)n_features;
    CartBest best = cart_none();
    for (int f = threadIdx.x; f < n_features; f += WB_CART_THREADS) {
        CartBest c;
        c.m = rec_proxy[row + f];
        c.idx = f;
        c.ok = rec_p[row + f] > 0 ? 1 : 0;
        c.lo = 0.0f;
        c.hi = 0.0f;
        if (CartBest::better(c, best)) best = c;
    }
    best = wb_best_reduce<WB_CART_WAVES>(best, part);
    if (threadIdx.x == 0) {
        WbCartSplit s;
        s.feature = best.ok ? best.idx : -1;
        s.n_left = best.ok ? rec_p[row + best.idx] : 0;
        s.lo = best.ok ? rec_lo[row + best.idx] : 0.0f;
        s.hi = best.ok ? rec_hi[row + best.idx] : 0.0f;
        s.proxy = best.ok ? best.m : -__builtin_inf();
        s.t0 = (double)lv.t0[k] * lv.scale;
        s.t1 = (double)lv.t1[k] * lv.scale;
        out[k] = s;
    }
}

__device__ inline int cart_slot(const CartLevel &lv, int i) {
    int s = -1;
#pragma unroll
    for (int k = 0; k < WB_FIT_MAX_OPEN; ++k) s = (k < lv.n_open && i >= lv.begin[k] && i < lv.end[k]) ? k : s;
    return s;
}

__global__ __launch_bounds__(WB_CART_THREADS) void cart_move_kernel(const float *__restrict__ xt, int n_samples,
                                                                    const int32_t *__restrict__ order, CartLevel lv,
                                                                    const WbCartSplit *__restrict__ splits,
                                                                    int32_t *__restrict__ node) {
    const int i = blockIdx.x * WB_CART_THREADS + threadIdx.x;          // a position of column 0's order
    if (i >= n_samples) return;
    const int k = cart_slot(lv, i);
    if (k < 0) return;
    const WbCartSplit sp = splits[k];
    if (sp.feature < 0) return;                                         // (no valid candidate: the node stays a leaf)
    const int s = order[i];
    const float x = xt[(size_t)sp.feature * (size_t)n_samples + (size_t)s];
    node[s] = lv.child_base + 2 * k + ((double)x <= cart_threshold(sp.lo, sp.hi) ? 0 : 1);
}

__global__ __launch_bounds__(WB_CART_THREADS) void cart_part_kernel(int n_samples, const int32_t *__restrict__ order_in,
                                                                    int32_t *__restrict__ order_out, CartLevel lv,
                                                                    const WbCartSplit *__restrict__ splits,
                                                                    const int32_t *__restrict__ node) {
    __shared__ int wcount[WB_CART_WAVES];
    const int tid = threadIdx.x, lane = tid % WB_WAVE, wave = tid / WB_WAVE;
    const int32_t *in = order_in + (size_t)blockIdx.x * (size_t)n_samples;
    int32_t *out = order_out + (size_t)blockIdx.x * (size_t)n_samples;
    for (int k = 0; k < lv.n_open; ++k) {
        if (splits[k].feature < 0) continue;                            // (the same for every thread)
        const int b = lv.begin[k], e = lv.end[k], n_left = splits[k].n_left;
        const int left_id = lv.child_base + 2 * k;
        int carry = 0;                                                  // left-going samples before `base`
        for (int base = b; base < e; base += WB_CART_THREADS) {
            const int i = base + tid;
            const bool valid = i < e;
            const int s = valid ? in[i] : 0;
            const bool left = valid && node[s] == left_id;
            const unsigned long long mask = __ballot(left);
            if (lane == 0) wcount[wave] = __popcll(mask);
            __syncthreads();
            int rank = carry + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
            for (int w2 = 0; w2 < WB_CART_WAVES; ++w2) {
                rank += w2 < wave ? wcount[w2] : 0;
                carry += wcount[w2];
            }
            __syncthreads();                                            // (wcount is written again in the next step)
            const int dest = left ? b + rank : b + n_left + (i - b - rank);
            if (valid && dest >= b && dest < e) out[dest] = s;
        }
    }
}

size_t cart_records(int64_t n_features, int n_open) { return ((size_t)n_open * (size_t)n_features + 1) / 2 * 2; }

}  // namespace

extern "C" int wb_cart_sort_launch(void *stream, const float *xt, int64_t n_samples, int64_t n_features, int32_t *order) {
    WB_REQUIRE(xt && order, "wb_cart_sort_launch: null pointer");
    WB_REQUIRE(n_samples >= 1 && n_features >= 1, "wb_cart_sort_launch: empty problem");
    if (n_samples > WB_CART_MAX_SAMPLES || n_features > WB_CART_MAX_FEATURES) {
        wb_set_error("wb_cart_sort_launch: at most %d samples and %d features", WB_CART_MAX_SAMPLES, WB_CART_MAX_FEATURES);
        return WB_ERR_UNSUPPORTED;
    }
    WB_REQUIRE(wb_aligned(xt, 4) && wb_aligned(order, 4),
               "wb_cart_sort_launch: misaligned pointer");
    hipLaunchKernelGGL(cart_sort_kernel, dim3((unsigned)n_features), dim3(WB_CART_SORT_THREADS), 0,
                       static_cast<hipStream_t>(stream), xt, (int)n_samples, order);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_cart_scratch_bytes(int64_t n_features, int n_open, size_t *bytes) {
    WB_REQUIRE(bytes != nullptr, "wb_cart_scratch_bytes: null pointer");
    WB_REQUIRE(n_features >= 1 && n_features <= WB_CART_MAX_FEATURES && n_open >= 1 && n_open <= WB_FIT_MAX_OPEN,
               "wb_cart_scratch_bytes: n_features 1 .. %d, n_open 1 .. %d", WB_CART_MAX_FEATURES, WB_FIT_MAX_OPEN);
    // per (open node, feature) a float64 proxy, then an int32 position, then float32 lo and hi
    *bytes = cart_records(n_features, n_open) * 20;
    return WB_OK;
}

extern "C" int wb_cart_level_launch(void *stream, const float *xt, int64_t n_samples, int64_t n_features, const uint64_t *q,
                                    const uint8_t *cls, const int32_t *order_in, int32_t *order_out, int32_t *node,
                                    int n_open, const int32_t *begin, const int32_t *end, const uint64_t *t0,
                                    const uint64_t *t1, double scale, int min_samples_leaf, int child_base, void *scratch,
                                    size_t scratch_bytes, WbCartSplit *splits) {
    const char *who = "wb_cart_level_launch";
    WB_REQUIRE(begin && end && t0 && t1, "%s: null pointer", who);
    WB_REQUIRE(n_open >= 1 && n_open <= WB_FIT_MAX_OPEN, "%s: a level has 1 .. %d open nodes", who, WB_FIT_MAX_OPEN);
    WB_REQUIRE(n_samples >= 1 && n_samples <= WB_CART_MAX_SAMPLES && n_features >= 1 && n_features <= WB_CART_MAX_FEATURES,
               "%s: 1 .. %d samples, 1 .. %d features", who, WB_CART_MAX_SAMPLES, WB_CART_MAX_FEATURES);
    CartLevel lv;
    lv.n_open = n_open;
    lv.min_leaf = min_samples_leaf;
    lv.child_base = child_base;
    lv.pad = 0;
    lv.scale = scale;
    for (int k = 0; k < WB_FIT_MAX_OPEN; ++k) {
        lv.begin[k] = lv.end[k] = 0;
        lv.t0[k] = lv.t1[k] = 0ull;
        if (k >= n_open) continue;
        WB_REQUIRE(begin[k] >= 0 && begin[k] < end[k] && end[k] <= n_samples, "%s: segment %d = [%d, %d) outside 0 .. n_samples",
                   who, k, (int)begin[k], (int)end[k]);
        WB_REQUIRE(k == 0 || begin[k] >= end[k - 1], "%s: segment %d overlaps its predecessor (segments ascend)", who, k);
        WB_REQUIRE(t0[k] < (1ull << 62) && t1[k] < (1ull << 62), "%s: class totals must stay below 2^62", who);
        lv.begin[k] = begin[k];
        lv.end[k] = end[k];
        lv.t0[k] = t0[k];
        lv.t1[k] = t1[k];
    }
    WB_REQUIRE(min_samples_leaf >= 1 && child_base >= 0 && child_base <= 0x7fffffff - 2 * WB_FIT_MAX_OPEN,
               "%s: min_samples_leaf >= 1, child_base >= 0", who);
    WB_REQUIRE(scale > 0.0 && scale < __builtin_inf(), "%s: scale must be positive and finite", who);
    WB_REQUIRE(xt && q && cls && order_in && order_out && node && scratch && splits && order_in != order_out, "%s: null pointer", who);
    WB_REQUIRE(wb_aligned(xt, 4) && wb_aligned(q, 8) &&
               wb_aligned(order_in, 4) && wb_aligned(order_out, 4) &&
               wb_aligned(node, 4) && wb_aligned(scratch, 16) &&
               wb_aligned(splits, 8), "%s: misaligned pointer", who);
    size_t need = 0;
    if (int rc = wb_cart_scratch_bytes(n_features, n_open, &need)) return rc;
    WB_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes, %zu needed", who, scratch_bytes, need);
    const size_t recs = cart_records(n_features, n_open);
    uint8_t *s = static_cast<uint8_t *>(scratch);
    double *rec_proxy = reinterpret_cast<double *>(s);
    int32_t *rec_p = reinterpret_cast<int32_t *>(s + recs * 8);
    float *rec_lo = reinterpret_cast<float *>(s + recs * 12);
    float *rec_hi = reinterpret_cast<float *>(s + recs * 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_samples, F = (int)n_features;
    hipLaunchKernelGGL(cart_scan_kernel, dim3(F), dim3(WB_CART_THREADS), 0, st, xt, N, F,
                       reinterpret_cast<const unsigned long long *>(q), cls, order_in, lv, rec_proxy, rec_p, rec_lo, rec_hi);
    WB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cart_best_kernel, dim3(n_open), dim3(WB_CART_THREADS), 0, st, rec_proxy, rec_p, rec_lo, rec_hi, F, lv, splits);
    WB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cart_move_kernel, dim3((N + WB_CART_THREADS - 1) / WB_CART_THREADS), dim3(WB_CART_THREADS), 0, st, xt, N,
                       order_in, lv, splits, node);
    WB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cart_part_kernel, dim3(F), dim3(WB_CART_THREADS), 0, st, N, order_in, order_out, lv, splits, node);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
