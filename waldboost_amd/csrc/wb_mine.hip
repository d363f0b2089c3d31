// Hard-negative mining on the device: label every detection record of a batch against its image's ground truth, choose at
// most max_tp / max_fp of the hits per (image, level) group, and crop the chosen windows out of the channel pyramid
// (wb_mine_select_launch, wb_mine_gather_launch) -- the step between two fits of the training loop (reference
// samples.py:46-216: label_boxes, select_candidates, gather_samples), for a whole batch without a trip to the host.
//
// The rule (tests/mine_reference.py states it in NumPy, tests/mine_designs.py proves designed answers):
//   * record (image, level, r, c): image and level clamped into [0, n_images) and [0, n_levels); its box is float32
//     [c, r, c + n, r + m] * inv_scale[level] (wb_match_iou.h: window_box);
//   * best / owner: the float64 IoU over gt[gt_off[image] .. gt_off[image + 1]), first argmax; no candidates: best 0,
//     owner -1 (wb_match_iou.h: match_iou, match_argmax);
//   * FP hit: best < max_fp_iou, or no candidates at all;  TP hit: candidates, best > min_tp_iou and gt_ignore[owner] == 0;
//   * key = fmix32(((r << 16) | c) ^ g),  g = fmix32(fmix32(seed ^ fmix32(serial[image] + 0x9E3779B9)) ^ (level * 0x9E3779B1));
//     fmix32 is a bijection and (r, c) unique inside a group, so the keys of a group never tie;
//   * per group and class the min(H, cap) hits with the smallest keys are chosen; a window chosen for both is FP.
//
// Selection never sorts: an 8-bit digit-histogram select over the 32-bit keys, most significant digit first.
//   mine_label_kernel    one thread per record: label, key, hits; keys[] and a packed (group, hits) word go to scratch; the
//                        hits count into hist[group][class][key >> 24] (integer atomics in global memory: the keys are
//                        hashes, so a group's adds spread evenly over its 256 counters)
//   mine_scan_kernel     one workgroup per (group, class): a 256-wide prefix sum finds the digit in which the cap-th smallest
//                        key lies, fixes it in the group's prefix, lowers the cap by the hits below it, and clears the counters
//   mine_digit_kernel    one thread per record: a hit whose key still matches its group's prefix counts its next digit
//   ... digits 2, 1, 0 alike: after the fourth scan the prefix IS the cap-th smallest key and limit = that key + 1;
//       H <= cap settles in the first scan (limit 2^32: every hit), cap 0 likewise (limit 0)
//   mine_emit_kernel     one thread per record: chosen = hit and key < limit; a chosen record takes the next output row
//                        (one integer atomic), recomputes its best / owner and writes its 32-byte row with two 16-byte stores
// Nine launches and one memset whatever the number of groups; scratch: 6 bytes per record and 2 KiB + 32 bytes per group.
// The rows come out in arrival order: the caller orders them by (image, level, r, c) (a sort of the few chosen rows).
//
// Nothing outside the buffers is read or written whatever the records hold: image, level and the candidate range are
// clamped, an output row is written only below out_capacity, and the gather checks every window against its level and
// every level against the image stride before it reads (a window that fails is written as zeros and flagged).
#include "wb_match_iou.h"   // the window's box, the IoU and its argmax, the output row, the limits of a batch

#define WB_MINE_PENDING 0xFFFFFFFFFFFFFFFFull

namespace {

struct MineState {       // per (group, class)
    uint32_t prefix;     // the digits fixed so far of the cap-th smallest key
    uint32_t krem;       // how many of the hits that match the prefix are still to choose
    uint64_t limit;      // chosen: key < limit;  WB_MINE_PENDING while the select runs
};

struct MineArgs {
    const float *inv_scale;
    const double *gt;
    const int32_t *gt_off;
    const uint8_t *gt_ignore;
    const uint32_t *serial;
    int64_t n_gt;
    int n_images, n_levels, m, n;
    double min_tp_iou, max_fp_iou;
    uint32_t want, seed;          // want: bit 0 TP, bit 1 FP
};

struct MineMatch {
    double best;
    int32_t owner;
    uint32_t hits;                // bit 0 TP hit, bit 1 FP hit (before `want`)
};

__device__ inline uint32_t mine_fmix32(uint32_t x) {
    x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
    return x;
}

__device__ inline int32_t mine_clamp(int32_t v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__device__ inline uint32_t mine_key(const MineArgs &a, int32_t image, int32_t level, uint32_t r, uint32_t c) {
    const uint32_t g = mine_fmix32(mine_fmix32(a.seed ^ mine_fmix32(a.serial[image] + 0x9E3779B9u)) ^ ((uint32_t)level * 0x9E3779B1u));
    return mine_fmix32(((r << 16) | c) ^ g);
}

// label_boxes for one record (image and level already clamped)
__device__ inline MineMatch mine_match(const MineArgs &a, int32_t image, int32_t level, uint32_t r, uint32_t c) {
    const MatchBox box = match_box(window_box(a.inv_scale[level], r, c, a.m, a.n));
    const MatchRange rg = match_range(a.gt_off, image, a.n_gt);
    double bestv = -1.0;
    int32_t own = -1;
    match_argmax(bestv, own, box, a.gt, rg.lo, rg.hi, 0);
    MineMatch out;
    out.best = own < 0 ? 0.0 : bestv;
    out.owner = own;
    const bool fp = own < 0 || out.best < a.max_fp_iou;
    const bool tp = own >= 0 && out.best > a.min_tp_iou && a.gt_ignore[rg.lo + own] == 0;
    out.hits = (tp ? 1u : 0u) | (fp ? 2u : 0u);
    return out;
}

__global__ __launch_bounds__(256) void mine_label_kernel(const WbDet *det, int64_t n_det, MineArgs a, uint32_t *keys, uint16_t *gf,
                                                         uint32_t *hist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_det) return;
    const WbDet d = det[i];
    const int32_t image = mine_clamp(d.image, a.n_images), level = mine_clamp(d.level, a.n_levels);
    const uint32_t g = (uint32_t)image * (uint32_t)a.n_levels + (uint32_t)level;
    const uint32_t hits = mine_match(a, image, level, d.r, d.c).hits & a.want;
    const uint32_t key = mine_key(a, image, level, d.r, d.c);
    keys[i] = key;
    gf[i] = (uint16_t)((g << 2) | hits);
    if (hits & 1u) atomicAdd(&hist[(size_t)(2 * g) * 256 + (key >> 24)], 1u);
    if (hits & 2u) atomicAdd(&hist[(size_t)(2 * g + 1) * 256 + (key >> 24)], 1u);
}

// digit `pass` (1 .. 3) of the hits whose key still matches its group's prefix
__global__ __launch_bounds__(256) void mine_digit_kernel(int64_t n_det, const uint32_t *keys, const uint16_t *gf, const MineState *state,
                                                         uint32_t *hist, int pass) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_det) return;
    const uint32_t w = gf[i];
    if ((w & 3u) == 0) return;
    const uint32_t key = keys[i], shift = 24u - 8u * (uint32_t)pass;
#pragma unroll
    for (uint32_t cls = 0; cls < 2; ++cls) {
        if (!(w & (1u << cls))) continue;
        const uint32_t gc = 2 * (w >> 2) + cls;
        const MineState st = state[gc];
        if (st.limit == WB_MINE_PENDING && (key >> (shift + 8)) == (st.prefix >> (shift + 8)))
            atomicAdd(&hist[(size_t)gc * 256 + ((key >> shift) & 255u)], 1u);
    }
}

// one workgroup per (group, class): fix digit `pass` of the cap-th smallest key, clear the counters
__global__ __launch_bounds__(256) void mine_scan_kernel(uint32_t *hist, MineState *state, int pass, uint32_t k_tp, uint32_t k_fp,
                                                        uint32_t *n_rows) {
    __shared__ uint32_t s[256];
    const uint32_t t = threadIdx.x, gc = blockIdx.x;
    uint32_t *h = hist + (size_t)gc * 256;
    const uint32_t cnt = h[t];
    h[t] = 0;
    s[t] = cnt;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const uint32_t incl = s[t], below = incl - cnt, total = s[255];
    MineState st;
    if (pass == 0) {
        st.prefix = 0;
        st.krem = (gc & 1u) ? k_fp : k_tp;
        st.limit = WB_MINE_PENDING;
        if (gc == 0 && t == 0) *n_rows = 0;                // (the emit kernel counts from here)
    } else {
        st = state[gc];
    }
    __syncthreads();                                       // everyone has read the state before one thread writes it
    if (st.limit != WB_MINE_PENDING) return;               // (workgroup-uniform)
    if (pass == 0 && (st.krem == 0 || total <= st.krem)) { // nothing to choose, or every hit
        if (t == 0) {
            st.limit = st.krem == 0 ? 0ull : 0x100000000ull;
            state[gc] = st;
        }
        return;
    }
    // total > krem > 0 in pass 0, total >= krem > 0 afterwards: exactly one digit holds the krem-th smallest key
    if (below < st.krem && st.krem <= incl) {
        st.prefix |= t << (24u - 8u * (uint32_t)pass);
        st.krem -= below;
        if (pass == 3) st.limit = (uint64_t)st.prefix + 1;
        state[gc] = st;
    }
}

__global__ __launch_bounds__(256) void mine_emit_kernel(const WbDet *det, int64_t n_det, MineArgs a, const uint32_t *keys,
                                                        const uint16_t *gf, const MineState *state, MineRow *rows,
                                                        int64_t out_capacity, uint32_t *n_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_det) return;
    const uint32_t w = gf[i];
    if ((w & 3u) == 0) return;
    const uint32_t key = keys[i], g = w >> 2;
    bool chosen[2];
#pragma unroll
    for (uint32_t cls = 0; cls < 2; ++cls) {
        const uint64_t lim = state[2 * g + cls].limit;
        chosen[cls] = (w & (1u << cls)) && lim != WB_MINE_PENDING && (uint64_t)key < lim;
    }
    const int32_t label = chosen[1] ? -1 : (chosen[0] ? 1 : 0);      // TP first, then FP: FP wins
    if (label == 0) return;
    uint32_t at;
    if (!row_take(n_rows, out_capacity, at)) return;       // (the launcher refuses a capacity the rule could exceed)
    const WbDet d = det[i];
    const MineMatch mt = mine_match(a, mine_clamp(d.image, a.n_images), mine_clamp(d.level, a.n_levels), d.r, d.c);
    row_store(rows, at, d, mt.best, mt.owner, label);
}

// crops of the chosen rows: one workgroup per row, element by element (a crop is m * n * C elements, rows of n * C contiguous
// ones; the chosen rows are few, so the launch is small next to the scan)
template <typename E>
__global__ __launch_bounds__(256) void mine_gather_kernel(const E *buf, int64_t img_stride, int n_images, const WbMineLevel *levels,
                                                          int n_levels, int C, const MineRow *rows, int m, int n, E *out,
                                                          uint32_t *err) {
    const WbDet d = rows[blockIdx.x].det;
    bool ok = d.image >= 0 && d.image < n_images && d.level >= 0 && d.level < n_levels;
    int64_t base = 0;
    int v = 0;
    if (ok) {
        const WbMineLevel lv = levels[d.level];
        v = lv.v;
        ok = lv.u >= 0 && lv.v >= 0 && (int)d.r + m <= lv.u && (int)d.c + n <= lv.v && lv.chn_off >= 0 &&
             lv.chn_off + (int64_t)lv.u * lv.v * C <= img_stride;
        base = (int64_t)d.image * img_stride + lv.chn_off;
    }
    const int rowlen = n * C, elems = m * rowlen;
    E *dst = out + (size_t)blockIdx.x * elems;
    for (int e = threadIdx.x; e < elems; e += 256) {
        const int i = e / rowlen, j = e - i * rowlen;
        dst[e] = ok ? buf[base + ((int64_t)((int)d.r + i) * v + d.c) * C + j] : (E)0;
    }
    if (!ok && threadIdx.x == 0) atomicOr(err, 1u);
}

struct MineLayout {
    size_t state, hist, keys, gf, total;
};

inline MineLayout mine_layout(int64_t n_det, int n_images, int n_levels) {
    const size_t G = (size_t)n_images * (size_t)n_levels;
    MineLayout l;
    l.state = 0;
    l.hist = l.state + G * 2 * sizeof(MineState);
    l.keys = l.hist + G * 2 * 256 * sizeof(uint32_t);
    l.gf = l.keys + (size_t)n_det * 4;
    l.total = (l.gf + (size_t)n_det * 2 + 255) / 256 * 256;
    return l;
}

}  // namespace

static_assert(sizeof(MineState) == 16 && sizeof(WbMineLevel) == 16, "wb_mine layouts");

extern "C" int wb_mine_scratch_bytes(int64_t n_det, int n_images, int n_levels, size_t *bytes) {
    WB_REQUIRE(bytes, "wb_mine_scratch_bytes: null pointer");
    const int rc = label_sizes_ok("wb_mine_scratch_bytes", n_det, n_images, n_levels);
    if (rc != WB_OK) return rc;
    *bytes = mine_layout(n_det, n_images, n_levels).total;
    return WB_OK;
}

extern "C" int wb_mine_select_launch(void *stream, const WbDet *det, int64_t n_det, const float *inv_scale, int n_levels, int m, int n,
                                     const double *gt, const int32_t *gt_off, const uint8_t *gt_ignore, int64_t n_gt,
                                     const uint32_t *serial, int n_images, double min_tp_iou, double max_fp_iou, int64_t max_tp,
                                     int64_t max_fp, int want_tp, int want_fp, uint32_t seed, void *scratch, size_t scratch_bytes,
                                     void *rows, int64_t out_capacity, uint32_t *n_rows) {
    const int rc = label_sizes_ok("wb_mine_select_launch", n_det, n_images, n_levels);
    if (rc != WB_OK) return rc;
    WB_REQUIRE(n_gt >= 0 && max_tp >= 0 && max_fp >= 0 && out_capacity >= 0 && m >= 1 && n >= 1 && m <= 65536 && n <= 65536,
               "wb_mine_select_launch: n_gt = %lld, max_tp = %lld, max_fp = %lld, out_capacity = %lld, m = %d, n = %d", (long long)n_gt,
               (long long)max_tp, (long long)max_fp, (long long)out_capacity, m, n);
    if (n_det == 0) return WB_OK;
    WB_REQUIRE(det && inv_scale && gt_off && serial && scratch && rows && n_rows && ((gt && gt_ignore) || n_gt == 0),
               "wb_mine_select_launch: null pointer");
    WB_REQUIRE(n_images >= 1 && n_levels >= 1, "wb_mine_select_launch: %lld records of no image or level", (long long)n_det);
    WB_REQUIRE(wb_aligned(det, 16) && wb_aligned(rows, 16) && wb_aligned(scratch, 16),
               "wb_mine_select_launch: det, rows and scratch must be 16-byte aligned");
    WB_REQUIRE(wb_aligned(gt, 8), "wb_mine_select_launch: gt must be 8-byte aligned");
    WB_REQUIRE(wb_aligned(inv_scale, 4) && wb_aligned(gt_off, 4) && wb_aligned(serial, 4) && wb_aligned(n_rows, 4),
               "wb_mine_select_launch: inv_scale, gt_off, serial and n_rows must be 4-byte aligned");
    const MineLayout l = mine_layout(n_det, n_images, n_levels);
    WB_REQUIRE(scratch_bytes >= l.total, "wb_mine_select_launch: scratch of %zu bytes, %zu needed", scratch_bytes, l.total);
    const uint32_t k_tp = want_tp ? (uint32_t)(max_tp < n_det ? max_tp : n_det) : 0u;
    const uint32_t k_fp = want_fp ? (uint32_t)(max_fp < n_det ? max_fp : n_det) : 0u;
    const int64_t G = (int64_t)n_images * n_levels;
    const int64_t most = G * ((int64_t)k_tp + k_fp) < n_det ? G * ((int64_t)k_tp + k_fp) : n_det;
    WB_REQUIRE(out_capacity >= most, "wb_mine_select_launch: room for %lld rows, up to %lld can be chosen", (long long)out_capacity,
               (long long)most);
    char *base = static_cast<char *>(scratch);
    MineState *state = reinterpret_cast<MineState *>(base + l.state);
    uint32_t *hist = reinterpret_cast<uint32_t *>(base + l.hist);
    uint32_t *keys = reinterpret_cast<uint32_t *>(base + l.keys);
    uint16_t *gf = reinterpret_cast<uint16_t *>(base + l.gf);
    MineArgs a;
    a.inv_scale = inv_scale, a.gt = gt, a.gt_off = gt_off, a.gt_ignore = gt_ignore, a.serial = serial;
    a.n_gt = n_gt, a.n_images = n_images, a.n_levels = n_levels, a.m = m, a.n = n;
    a.min_tp_iou = min_tp_iou, a.max_fp_iou = max_fp_iou;
    a.want = (want_tp ? 1u : 0u) | (want_fp ? 2u : 0u), a.seed = seed;
    hipStream_t st = (hipStream_t)stream;
    const dim3 per_det((uint32_t)((n_det + 255) / 256)), per_group((uint32_t)(2 * G)), wg(256);
    WB_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)G * 2 * 256 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(mine_label_kernel, per_det, wg, 0, st, det, n_det, a, keys, gf, hist);
    hipLaunchKernelGGL(mine_scan_kernel, per_group, wg, 0, st, hist, state, 0, k_tp, k_fp, n_rows);
    for (int pass = 1; pass < 4; ++pass) {
        hipLaunchKernelGGL(mine_digit_kernel, per_det, wg, 0, st, n_det, keys, gf, state, hist, pass);
        hipLaunchKernelGGL(mine_scan_kernel, per_group, wg, 0, st, hist, state, pass, k_tp, k_fp, n_rows);
    }
    hipLaunchKernelGGL(mine_emit_kernel, per_det, wg, 0, st, det, n_det, a, keys, gf, state, static_cast<MineRow *>(rows), out_capacity,
                       n_rows);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_mine_gather_launch(void *stream, const void *buf, int dtype, int64_t img_stride, int n_images, const WbMineLevel *levels,
                                     int n_levels, int C, const void *rows, int64_t n_rows, int m, int n, void *out, uint32_t *err) {
    WB_REQUIRE(n_rows >= 0 && img_stride >= 0 && n_images >= 0 && n_levels >= 0,
               "wb_mine_gather_launch: n_rows = %lld, img_stride = %lld, n_images = %d, n_levels = %d: negative", (long long)n_rows,
               (long long)img_stride, n_images, n_levels);
    WB_REQUIRE(m >= 1 && n >= 1 && C >= 1 && (int64_t)m * n * C < (1ll << 31), "wb_mine_gather_launch: window %d x %d x %d", m, n, C);
    if (dtype != WB_DTYPE_F32 && dtype != WB_DTYPE_U8) {
        wb_set_error("wb_mine_gather_launch: dtype %d (float32 and uint8 channels have crops)", dtype);
        return WB_ERR_UNSUPPORTED;
    }
    if (n_rows > WB_LABEL_MAX_DET) {
        wb_set_error("wb_mine_gather_launch: %lld rows (at most %d in one call)", (long long)n_rows, WB_LABEL_MAX_DET);
        return WB_ERR_UNSUPPORTED;
    }
    WB_REQUIRE(err, "wb_mine_gather_launch: null pointer");
    WB_REQUIRE(wb_aligned(err, 4), "wb_mine_gather_launch: err must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    WB_HIP_CHECK(hipMemsetAsync(err, 0, 4, st));
    if (n_rows == 0) return WB_OK;
    WB_REQUIRE(buf && levels && rows && out, "wb_mine_gather_launch: null pointer");
    WB_REQUIRE(wb_aligned(rows, 16) && wb_aligned(levels, 8) && (dtype == WB_DTYPE_U8 || (wb_aligned(buf, 4) && wb_aligned(out, 4))),
               "wb_mine_gather_launch: rows 16-byte, levels 8-byte, float buffers 4-byte aligned");
    const dim3 grid((uint32_t)n_rows), wg(256);
    if (dtype == WB_DTYPE_F32)
        hipLaunchKernelGGL((mine_gather_kernel<float>), grid, wg, 0, st, static_cast<const float *>(buf), img_stride, n_images, levels,
                           n_levels, C, static_cast<const MineRow *>(rows), m, n, static_cast<float *>(out), err);
    else
        hipLaunchKernelGGL((mine_gather_kernel<uint8_t>), grid, wg, 0, st, static_cast<const uint8_t *>(buf), img_stride, n_images, levels,
                           n_levels, C, static_cast<const MineRow *>(rows), m, n, static_cast<uint8_t *>(out), err);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
