// The float64 IoU of boxes.iou and an image's clamped candidate range: what match_kernel (wb_match.hip) and the miner's
// labelling (wb_mine.hip) both compute, operation by operation (both files are built with -ffp-contract=off).
#pragma once
#include <stdint.h>

namespace {

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
__device__ inline double match_iou(double ax1, double ay1, double ax2, double ay2, double area_a, double bx1, double by1,
                                   double bx2, double by2) {
    double iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1);
    double ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
    iw = iw < 0.0 ? 0.0 : iw;
    ih = ih < 0.0 ? 0.0 : ih;
    const double inter = iw * ih;
    const double area_b = (bx2 - bx1) * (by2 - by1);
    const double uni = area_a + area_b - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

}  // namespace
