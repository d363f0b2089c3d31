// Multiple-instance pruning (Zhang & Viola 2007) of a finished cascade: the dense labelling of a pyramid's window grids
// against ground truth (wb_mip_windows_launch) and the stage-sequential prune over bags of windows (wb_mip_prune_launch).
//
// The rule (tests/mip_reference.py states it in NumPy, tests/mip_designs.py proves designed answers):
//   * the windows of level l (u x v channels, window m x n) are those the scan visits: r in [0, u - m), c in [0, v - n);
//     the box of a window is float32 [c, r, c + n, r + m] * inv_scale[l] (wb_match_iou.h: window_box);
//   * best / owner: the float64 IoU over the image's ground truth, first argmax (wb_match_iou.h: match_iou, match_argmax);
//   * a window is ACCEPTABLE when its image has ground truth, best > min_iou (strict, float64) and gt_ignore[owner] == 0:
//     the miner's TP rule without caps; it belongs to the bag of its owner only;
//   * prune: a window is retained at the start when its final score trace[T - 1][i] >= floor; for t = 0 .. T - 1, in
//     order, theta[t] = min over the bags that still have a retained window of the max of trace[t][i] over the bag's
//     retained windows, and then every retained window with `not (trace[t][i] >= theta[t])` stops being retained
//     (removed_at[i] = t); removed_at is -1 for a window never retained and T for one that survives every stage.
//
// mip_windows_kernel   one thread per window of one (image, level) grid, one launch per level that has windows (grid.y:
//                      the image); the image's ground truth passes through LDS in chunks of 256 boxes (8 KiB + 256
//                      flags), every thread of the workgroup walking the chunk; a hit takes the next output row with one
//                      integer atomic and leaves as a 32-byte row (wb_match_iou.h: MineRow, two 16-byte stores) while there is room
// mip_start_kernel     one thread per window: removed_at = T (retained) or -1
// mip_window_kernel    stage t, one thread per window: a retained window is first tested against theta[t - 1] (t > 0), and if
//                      it stays, its key goes into bag_max[bag] (atomicMax); t == T only tests and counts the survivors
// mip_bag_kernel       stage t, one thread per bag: takes bag_max[b] and clears it for the next stage; the wave's smallest
//                      key of the non-empty bags goes into theta[t] (atomicMin); stage 0 counts the non-empty bags
// wb_keys_to_floats_launch   theta's keys back to floats in place (all ones -- no bag -- becomes +inf; wb_common.h)
// A stage depends on the one before it through theta[t - 1] alone, and that dependency is carried by the order of the
// launches on the stream: 2 T + 3 small launches and three memsets, enqueued back to back with no host wait between
// them.  No workgroup waits for another.  Maxima, minima and counts are integer atomics on order-preserving keys
// (wb_f32_key), so the result depends neither on the order of the windows nor on the run.
#include "wb_match_iou.h"   // the window's box, the IoU and its argmax, the output row, the limits of a batch

#define WB_MIP_CHUNK 256                // ground-truth boxes staged in LDS at a time

namespace {

struct MipWinArgs {
    const double *gt;
    const int32_t *gt_off;
    const uint8_t *gt_ignore;
    int64_t n_gt;
    int level, nr, nc, m, n;          // nr x nc windows: (u - m) x (v - n)
    float inv_scale;
    double min_iou;
    MineRow *rows;
    int64_t out_capacity;
    uint32_t *n_rows;
};

__global__ __launch_bounds__(256) void mip_windows_kernel(MipWinArgs a) {
    __shared__ double s_gt[WB_MIP_CHUNK * 4];
    __shared__ uint8_t s_ign[WB_MIP_CHUNK];
    const int32_t image = (int32_t)blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x, n_win = (int64_t)a.nr * a.nc;
    const bool live = w < n_win;                           // (nobody leaves early: the whole workgroup stages every chunk)
    const int r = live ? (int)(w / a.nc) : 0, c = live ? (int)(w - (int64_t)r * a.nc) : 0;
    const MatchBox box = match_box(window_box(a.inv_scale, (uint32_t)r, (uint32_t)c, a.m, a.n));
    const MatchRange rg = match_range(a.gt_off, image, a.n_gt);
    double bestv = -1.0;
    int32_t own = -1;
    uint32_t own_ign = 0;
    for (int64_t k0 = rg.lo; k0 < rg.hi; k0 += WB_MIP_CHUNK) {
        const int cnt = (int)(rg.hi - k0 < WB_MIP_CHUNK ? rg.hi - k0 : WB_MIP_CHUNK);
        __syncthreads();                                   // the chunk before is read out
        for (int e = threadIdx.x; e < 4 * cnt; e += 256) s_gt[e] = a.gt[4 * k0 + e];
        if ((int)threadIdx.x < cnt) s_ign[threadIdx.x] = a.gt_ignore[k0 + threadIdx.x];
        __syncthreads();
        const int32_t first = (int32_t)(k0 - rg.lo);
        match_argmax(bestv, own, box, s_gt, 0, cnt, first);
        if (own >= first) own_ign = s_ign[own - first];   // the owner lies in this chunk: its flag, while it is staged
    }
    if (!live || own < 0 || !(bestv > a.min_iou) || own_ign != 0) return;
    uint32_t at;
    if (!row_take(a.n_rows, a.out_capacity, at)) return;
    WbDet d;
    d.image = image, d.level = a.level, d.r = (uint16_t)r, d.c = (uint16_t)c, d.score = 0.f;
    row_store(a.rows, at, d, bestv, own, 1);
}

struct MipArgs {
    const float *trace;      // [T][stride]
    const int32_t *bag;      // [N]
    int64_t N, stride;
    int T, n_bags;
    float floor;
    uint32_t *theta;         // [T]: keys while the chain runs, floats after wb_keys_to_floats_launch
    int32_t *removed_at;     // [N]: T while a window is retained
    uint32_t *counts;        // retained bags, surviving windows
    uint32_t *bag_max;       // [n_bags]: 0 = no retained window (no finite score has the key 0)
};

__global__ __launch_bounds__(256) void mip_start_kernel(MipArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int32_t b = a.bag[i];
    const bool in = b >= 0 && b < a.n_bags && a.trace[(int64_t)(a.T - 1) * a.stride + i] >= a.floor;
    a.removed_at[i] = in ? a.T : -1;
}

__global__ __launch_bounds__(256) void mip_window_kernel(MipArgs a, int t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool in = i < a.N && a.removed_at[i] == a.T;
    if (in && t > 0) {
        const uint32_t k = a.theta[t - 1];
        const float th = k == 0xFFFFFFFFu ? INFINITY : wb_key_f32(k);
        if (!(a.trace[(int64_t)(t - 1) * a.stride + i] >= th)) {       // the cascade's test
            a.removed_at[i] = t - 1;
            in = false;
        }
    }
    if (t < a.T) {
        if (in) atomicMax(&a.bag_max[a.bag[i]], wb_f32_key(a.trace[(int64_t)t * a.stride + i]));
    } else {                                               // behind the last stage: the survivors, one add per wave
        const uint64_t alive = __ballot(in);
        if ((threadIdx.x & (WB_WAVE - 1)) == 0 && alive) atomicAdd(&a.counts[1], (uint32_t)__popcll(alive));
    }
}

__global__ __launch_bounds__(256) void mip_bag_kernel(MipArgs a, int t) {
    const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
    uint32_t k = 0;
    if (b < a.n_bags) {
        k = a.bag_max[b];
        a.bag_max[b] = 0;                                  // the next stage starts from nothing
    }
    const uint32_t mn = wb_wave_min_u32(k ? k : 0xFFFFFFFFu);
    const uint64_t full = __ballot(k != 0);
    if ((threadIdx.x & (WB_WAVE - 1)) == 0 && full) {
        atomicMin(&a.theta[t], mn);
        if (t == 0) atomicAdd(&a.counts[0], (uint32_t)__popcll(full));
    }
}

inline size_t mip_scratch(int64_t n_bags) { return ((size_t)n_bags * 4 + 255) / 256 * 256; }

}  // namespace

extern "C" int wb_mip_windows_launch(void *stream, const WbMineLevel *levels_host, const float *inv_scale_host, int n_levels, int m,
                                     int n, const double *gt, const int32_t *gt_off, const uint8_t *gt_ignore, int64_t n_gt,
                                     int n_images, double min_iou, void *rows, int64_t out_capacity, uint32_t *n_rows) {
    const int rc = label_sizes_ok("wb_mip_windows_launch", 0, n_images, n_levels);
    if (rc != WB_OK) return rc;
    WB_REQUIRE(n_gt >= 0 && out_capacity >= 0 && m >= 1 && n >= 1 && m <= 65536 && n <= 65536,
               "wb_mip_windows_launch: n_gt = %lld, out_capacity = %lld, m = %d, n = %d", (long long)n_gt, (long long)out_capacity, m, n);
    WB_REQUIRE(n_rows && ((levels_host && inv_scale_host) || n_levels == 0), "wb_mip_windows_launch: null pointer");
    WB_REQUIRE(wb_aligned(n_rows, 4), "wb_mip_windows_launch: n_rows must be 4-byte aligned");
    int64_t total = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int u = levels_host[l].u, v = levels_host[l].v;
        WB_REQUIRE(u >= 0 && v >= 0 && u <= 65536 && v <= 65536, "wb_mip_windows_launch: level %d is %d x %d (0 .. 65536)", l, u, v);
        if (u > m && v > n) total += (int64_t)(u - m) * (v - n);
    }
    total *= n_images;
    if (total >= (1ll << 32)) {
        wb_set_error("wb_mip_windows_launch: %lld windows (fewer than 2^32 in one call)", (long long)total);
        return WB_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    WB_HIP_CHECK(hipMemsetAsync(n_rows, 0, 4, st));
    if (total == 0 || n_gt == 0) return WB_OK;             // no window, or no image with ground truth: no hit
    WB_REQUIRE(gt && gt_off && gt_ignore && (rows || out_capacity == 0), "wb_mip_windows_launch: null pointer");
    WB_REQUIRE(wb_aligned(rows, 16) && wb_aligned(gt, 8) && wb_aligned(gt_off, 4),
               "wb_mip_windows_launch: rows must be 16-byte, gt 8-byte, gt_off 4-byte aligned");
    MipWinArgs a;
    a.gt = gt, a.gt_off = gt_off, a.gt_ignore = gt_ignore, a.n_gt = n_gt, a.m = m, a.n = n, a.min_iou = min_iou;
    a.rows = static_cast<MineRow *>(rows), a.out_capacity = out_capacity, a.n_rows = n_rows;
    for (int l = 0; l < n_levels; ++l) {
        const int u = levels_host[l].u, v = levels_host[l].v;
        if (u <= m || v <= n) continue;
        a.level = l, a.nr = u - m, a.nc = v - n, a.inv_scale = inv_scale_host[l];
        const int64_t blocks = ((int64_t)a.nr * a.nc + 255) / 256;
        hipLaunchKernelGGL(mip_windows_kernel, dim3((uint32_t)blocks, (uint32_t)n_images), dim3(256), 0, st, a);
    }
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_mip_scratch_bytes(int64_t n_bags, size_t *bytes) {
    WB_REQUIRE(bytes, "wb_mip_scratch_bytes: null pointer");
    WB_REQUIRE(n_bags >= 0 && n_bags < (1ll << 31), "wb_mip_scratch_bytes: %lld bags (0 .. 2^31 - 1)", (long long)n_bags);
    *bytes = mip_scratch(n_bags);
    return WB_OK;
}

extern "C" int wb_mip_prune_launch(void *stream, const float *trace, int64_t stride, int n_stages, int64_t n_windows, const int32_t *bag,
                                   int64_t n_bags, float floor, void *scratch, size_t scratch_bytes, float *theta, int32_t *removed_at,
                                   uint32_t *counts) {
    const int64_t N = n_windows;
    const int T = n_stages;
    WB_REQUIRE(N >= 0 && T >= 0 && stride >= N && n_bags >= 0 && n_bags < (1ll << 31),
               "wb_mip_prune_launch: n_windows = %lld, stride = %lld, n_stages = %d, n_bags = %lld", (long long)N, (long long)stride, T,
               (long long)n_bags);
    WB_REQUIRE(counts && (theta || T == 0), "wb_mip_prune_launch: null pointer");
    WB_REQUIRE(wb_aligned(theta, 4) && wb_aligned(counts, 4), "wb_mip_prune_launch: theta and counts must be 4-byte aligned");
    WB_REQUIRE(T == 0 || ((int64_t)T - 1) * stride + N < (1ll << 31), "wb_mip_prune_launch: a trace of %lld x %d entries (fewer than 2^31)",
               (long long)stride, T);
    hipStream_t st = (hipStream_t)stream;
    WB_HIP_CHECK(hipMemsetAsync(counts, 0, 8, st));
    const bool empty = N == 0 || T == 0 || n_bags == 0;
    if (T > 0) WB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)theta, empty ? 0x7F800000 : -1, (size_t)T, st));   // +inf, or the keys' start
    if (empty) {                                           // no window is retained: +inf and zeros, nobody's removed_at is T
        if (N > 0) {
            WB_REQUIRE(removed_at && wb_aligned(removed_at, 4), "wb_mip_prune_launch: removed_at null or not 4-byte aligned");
            WB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)removed_at, -1, (size_t)N, st));
        }
        return WB_OK;
    }
    WB_REQUIRE(trace && bag && scratch && removed_at, "wb_mip_prune_launch: null pointer");
    WB_REQUIRE(wb_aligned(trace, 4) && wb_aligned(bag, 4) && wb_aligned(scratch, 4) && wb_aligned(removed_at, 4),
               "wb_mip_prune_launch: trace, bag, scratch and removed_at must be 4-byte aligned");
    WB_REQUIRE(scratch_bytes >= mip_scratch(n_bags), "wb_mip_prune_launch: scratch of %zu bytes, %zu needed", scratch_bytes,
               mip_scratch(n_bags));
    MipArgs a;
    a.trace = trace, a.bag = bag, a.N = N, a.stride = stride, a.T = T, a.n_bags = (int)n_bags, a.floor = floor;
    a.theta = reinterpret_cast<uint32_t *>(theta), a.removed_at = removed_at, a.counts = counts;
    a.bag_max = static_cast<uint32_t *>(scratch);
    WB_HIP_CHECK(hipMemsetAsync(a.bag_max, 0, (size_t)n_bags * 4, st));
    const dim3 per_window((uint32_t)((N + 255) / 256)), per_bag((uint32_t)((n_bags + 255) / 256)), wg(256);
    hipLaunchKernelGGL(mip_start_kernel, per_window, wg, 0, st, a);
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(mip_window_kernel, per_window, wg, 0, st, a, t);
        hipLaunchKernelGGL(mip_bag_kernel, per_bag, wg, 0, st, a, t);
    }
    hipLaunchKernelGGL(mip_window_kernel, per_window, wg, 0, st, a, T);
    WB_HIP_CHECK(hipGetLastError());
    return wb_keys_to_floats_launch(st, a.theta, T);
}
