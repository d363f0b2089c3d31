// Box matching on the device (wb_match_launch): for every detection its best IoU over the ground-truth boxes of its image
// and the box that gives it -- the step of the reference's Evaluator.evaluate between NMS and the precision / recall curve
// (reference testing.py:53-58 iou.argmax / iou.max), and the miner's samples._match_ground_truth.
//
// Semantics (tests/match_designs.py proves the expected answers in exact arithmetic):
//   * detection i belongs to image b = dt_image[i]; its candidates are gt[gt_off[b] .. gt_off[b + 1]);
//   * iou is boxes.iou's float64 arithmetic, operation by operation (wb_match_iou.h; this file is built with
//     -ffp-contract=off: no fused multiply-add; the float64 divide is the correctly rounded one);
//   * best[i] is the largest iou, owner[i] the FIRST candidate that reaches it, counted inside the image's own list
//     (np.argmax; wb_match_iou.h: match_argmax): a detection that overlaps nothing is owned by candidate 0;  no candidates:
//     best 0, owner -1.
//
// One kernel, one thread per detection, 256 per workgroup.  A workgroup whose detections all belong to one image stages
// that image's candidates through LDS, WB_MATCH_CHUNK = 64 boxes at a time: 64 boxes are 256 doubles, ONE coalesced 8-byte
// load per thread, and every thread then reads the same box at the same time, which the LDS serves as a broadcast (no bank
// conflict whatever the chunk size).  2 KiB per workgroup is never what limits the workgroups of a CU (160 KiB of LDS
// against at most 8 workgroups of 256), so a larger chunk would only save barriers: an image seldom has more than 64
// ground-truth boxes, which makes it one load, two barriers.  A workgroup that straddles images reads its candidates from
// global memory, every thread its own range (neighbouring threads mostly the same addresses).
//
// Whatever dt_image and gt_off hold, nothing outside the buffers is read: the image is clamped to [0, n_images), both ends
// of a range to [0, n_gt], and an end in front of its start gives an empty range.  Every loop is bounded by n_gt.
#include "wb_match_iou.h"   // the IoU, the candidate range and the argmax step

#define WB_MATCH_CHUNK 64           // candidates staged in LDS at a time: 4 * 64 doubles = one per thread

namespace {

__global__ __launch_bounds__(256) void match_kernel(const double *dt, const int32_t *dt_image, const double *gt,
                                                    const int32_t *gt_off, int64_t n_dt, int64_t n_gt, int n_images,
                                                    double *best, int32_t *owner) {
    __shared__ double sg[4 * WB_MATCH_CHUNK];
    __shared__ int32_t s_first, s_mixed;
    const uint32_t tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool live = i < n_dt;
    const int64_t ii = live ? i : n_dt - 1;                    // (threads behind the last detection walk with it)
    int32_t b = dt_image[ii];
    b = b < 0 ? 0 : (b >= n_images ? n_images - 1 : b);
    if (tid == 0) {
        s_first = b;
        s_mixed = 0;
    }
    __syncthreads();
    if (b != s_first) s_mixed = 1;                             // (every writer writes the same value)
    __syncthreads();
    const bool one_image = s_mixed == 0;                       // (workgroup-uniform)
    const MatchRange r = match_range(gt_off, b, n_gt);
    const MatchBox box = match_box(dt[4 * ii], dt[4 * ii + 1], dt[4 * ii + 2], dt[4 * ii + 3]);
    double bestv = -1.0;
    int32_t own = -1;
    if (one_image) {
        for (int64_t c0 = r.lo; c0 < r.hi; c0 += WB_MATCH_CHUNK) {     // (r is the same in every thread)
            const uint32_t m = r.hi - c0 < WB_MATCH_CHUNK ? (uint32_t)(r.hi - c0) : (uint32_t)WB_MATCH_CHUNK;
            __syncthreads();                                   // the last chunk has been read by everyone
            if (tid < 4u * m) sg[tid] = gt[4 * c0 + tid];
            __syncthreads();
            match_argmax(bestv, own, box, sg, 0u, m, (int32_t)(c0 - r.lo));
        }
    } else {
        match_argmax(bestv, own, box, gt, r.lo, r.hi, 0);
    }
    if (live) {
        best[i] = own < 0 ? 0.0 : bestv;
        owner[i] = own;
    }
}

}  // namespace

extern "C" int wb_match_launch(void *stream, const double *dt, const int32_t *dt_image, const double *gt, const int32_t *gt_off,
                               int64_t n_dt, int64_t n_gt, int n_images, double *best, int32_t *owner) {
    WB_REQUIRE(n_dt >= 0 && n_gt >= 0 && n_images >= 0, "wb_match_launch: n_dt = %lld, n_gt = %lld, n_images = %d: negative",
               (long long)n_dt, (long long)n_gt, n_images);
    if (n_dt == 0) return WB_OK;
    WB_REQUIRE(dt && dt_image && gt_off && best && owner && (gt || n_gt == 0), "wb_match_launch: null pointer");
    WB_REQUIRE(n_images >= 1, "wb_match_launch: %lld detections of no image", (long long)n_dt);
    WB_REQUIRE(wb_aligned(dt, 8) && wb_aligned(gt, 8) && wb_aligned(best, 8), "wb_match_launch: dt, gt and best must be 8-byte aligned");
    WB_REQUIRE(wb_aligned(dt_image, 4) && wb_aligned(gt_off, 4) && wb_aligned(owner, 4),
               "wb_match_launch: dt_image, gt_off and owner must be 4-byte aligned");
    if (n_dt > WB_LABEL_MAX_DET) {
        wb_set_error("wb_match_launch: %lld detections (at most %d in one call)", (long long)n_dt, WB_LABEL_MAX_DET);
        return WB_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(match_kernel, dim3((uint32_t)((n_dt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dt, dt_image, gt,
                       gt_off, n_dt, n_gt, n_images, best, owner);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
