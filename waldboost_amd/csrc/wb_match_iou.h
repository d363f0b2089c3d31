// Labelling a window against ground truth: the one statement of the window's box, the float64 IoU of boxes.iou, the
// first-argmax rule, the 32-byte output row and the limits of a labelled batch.  The matcher (wb_match.hip), the miner
// (wb_mine.hip), the dense window labelling (wb_mip.hip) and get_boxes (wb_det.hip) all compute through these, operation
// by operation (the files are built with -ffp-contract=off).
#pragma once
#include "wb_common.h"

#define WB_LABEL_MAX_DET (1 << 26)      // most records or detections of one call (what one scan can return)
#define WB_LABEL_MAX_IMAGES 1024
#define WB_LABEL_MAX_LEVELS 256
#define WB_LABEL_MAX_GROUPS 16384       // (image, level) groups: a group index and two hit bits share 16 bits of the miner's scratch

namespace {

// ---- the box of window (r, c) of a level: Model.get_boxes (reference model.py:136-147), [c, r, c+n, r+m] as fp32, times sc = fp32(1/scale)
__device__ inline float4 window_box(float sc, uint32_t r, uint32_t c, int m, int n) {
    return make_float4((float)c * sc, (float)r * sc, (float)((int)c + n) * sc, (float)((int)r + m) * sc);
}

// a box in float64 with its area: what the IoU takes as `a`
struct MatchBox {
    double x1, y1, x2, y2, area;
};
__device__ inline MatchBox match_box(double x1, double y1, double x2, double y2) { return {x1, y1, x2, y2, (x2 - x1) * (y2 - y1)}; }
__device__ inline MatchBox match_box(float4 b) { return match_box((double)b.x, (double)b.y, (double)b.z, (double)b.w); }

// ---- an image's candidates gt[lo .. hi), clamped into [0, n_gt] whatever gt_off holds
struct MatchRange {
    int64_t lo, hi;
};

__device__ inline MatchRange match_range(const int32_t *gt_off, int32_t b, int64_t n_gt) {
    int64_t lo = gt_off[b], hi = gt_off[b + 1];
    lo = lo < 0 ? 0 : (lo > n_gt ? n_gt : lo);
    hi = hi < 0 ? 0 : (hi > n_gt ? n_gt : hi);
    if (hi < lo) hi = lo;
    return {lo, hi};
}

// boxes.iou, operation by operation
__device__ inline double match_iou(const MatchBox &a, double bx1, double by1, double bx2, double by2) {
    double iw = (a.x2 < bx2 ? a.x2 : bx2) - (a.x1 > bx1 ? a.x1 : bx1);
    double ih = (a.y2 < by2 ? a.y2 : by2) - (a.y1 > by1 ? a.y1 : by1);
    iw = iw < 0.0 ? 0.0 : iw;
    ih = ih < 0.0 ? 0.0 : ih;
    const double inter = iw * ih;
    const double area_b = (bx2 - bx1) * (by2 - by1);
    const double uni = a.area + area_b - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// ---- best IoU and its owner (np.argmax: the FIRST candidate that reaches the largest IoU).  A search starts from
//      bestv = -1, own = -1: an IoU is never negative and never NaN, so the first candidate takes it; own stays -1 (and
//      best is 0) without candidates.  One step walks the candidates cand[lo .. hi) of four doubles each, in LDS or in
//      global memory, whose owner indices start at `first`.  (The range comes by reference so that the LDS chunk loop
//      of match_kernel keeps the code it had with the walk written out in it, as tools/kernel_text.py checks.)
template <typename I>
__device__ inline void match_argmax(double &bestv, int32_t &own, const MatchBox &a, const double *cand, const I &lo, const I &hi,
                                    int32_t first) {
    double b = bestv;                                      // (the walk in registers of its own: one copy of the running best)
    int32_t o = own;
    for (I k = lo; k < hi; ++k) {
        const double v = match_iou(a, cand[4 * k], cand[4 * k + 1], cand[4 * k + 2], cand[4 * k + 3]);
        if (v > b) {
            b = v;
            o = first + (int32_t)(k - lo);
        }
    }
    bestv = b, own = o;
}

// ---- one labelled window: the 32-byte row of wb_mine_select_launch and wb_mip_windows_launch, read by wb_mine_gather_launch
struct MineRow {
    WbDet det;
    double best;
    int32_t owner;
    int32_t label;
};
static_assert(sizeof(MineRow) == 32, "the labelled row");

// the next output row: *n_rows counts every taker, whatever the room (the full count); false: no room, nothing is written
__device__ inline bool row_take(uint32_t *n_rows, int64_t out_capacity, uint32_t &at) {
    at = atomicAdd(n_rows, 1u);
    return (int64_t)at < out_capacity;
}
// two 16-byte stores
__device__ inline void row_store(MineRow *rows, uint32_t at, const WbDet &d, double best, int32_t owner, int32_t label) {
    uint4 lo, hi;
    __builtin_memcpy(&lo, &d, 16);
    __builtin_memcpy(&hi.x, &best, 8);
    hi.z = (uint32_t)owner;
    hi.w = (uint32_t)label;
    uint4 *dst = reinterpret_cast<uint4 *>(rows + at);
    dst[0] = lo;
    dst[1] = hi;
}

// ---- the limits of a labelled batch and their refusal (n_det = 0: a call that takes no records)
inline int label_sizes_ok(const char *who, int64_t n_det, int n_images, int n_levels) {
    WB_REQUIRE(n_det >= 0 && n_images >= 0 && n_levels >= 0, "%s: n_det = %lld, n_images = %d, n_levels = %d: negative", who,
               (long long)n_det, n_images, n_levels);
    if (n_det > WB_LABEL_MAX_DET || n_images > WB_LABEL_MAX_IMAGES || n_levels > WB_LABEL_MAX_LEVELS ||
        (int64_t)n_images * n_levels > WB_LABEL_MAX_GROUPS) {
        wb_set_error("%s: %lld records, %d images, %d levels (at most %d records, %d images, %d levels, %d images * levels)", who,
                     (long long)n_det, n_images, n_levels, WB_LABEL_MAX_DET, WB_LABEL_MAX_IMAGES, WB_LABEL_MAX_LEVELS, WB_LABEL_MAX_GROUPS);
        return WB_ERR_UNSUPPORTED;
    }
    return WB_OK;
}

}  // namespace
