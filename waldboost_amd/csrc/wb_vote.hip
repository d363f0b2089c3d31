// Box voting on the device (wb_vote_launch): every box that non-maximum suppression kept is replaced by the weighted mean
// of the boxes of its cluster, and the size of the cluster is counted -- Viola-Jones's merge of overlapping detections, the
// "box voting" of later detectors, OpenCV's minNeighbors.  DESIGN.md 4.16; tests/vote_reference.py states the rule in NumPy.
//
// The rule:
//   * a box is LIVE unless the score threshold is in use and `not (score >= score_threshold)` (what NMS dropped first);
//   * for a kept box k, box j is a VOTER when j == k (always: a box of no area, whose IoU with itself is 0, still votes
//     for itself), or when j is live, group[j] == group[k] and iou(box_k, box_j) >= vote_iou;
//   * iou is boxes.iou's float64 arithmetic, operation by operation (wb_match_iou.h; this file is built with
//     -ffp-contract=off: no fused multiply-add; the float64 divide is the correctly rounded one);
//   * weights: WB_VOTE_UNIFORM w_j = 1.0;  WB_VOTE_SCORE w_j = float64(score_j) - float64(score_threshold), >= 0 for every
//     live box (the mode needs a threshold; a box that is not live votes for nobody but itself);
//   * the order of the sums is part of the contract: lane l of 64 visits the candidates j = l, l + 64, l + 128, ... ascending
//     and adds, for a voter, sw = sw + w and sc[i] = sc[i] + (w * float64(x_ji)) for the four coordinates -- the product
//     rounded, then the sum; the 64 partials of the five doubles and of the vote count are then combined by a butterfly:
//     for s = 1, 2, 4, 8, 16, 32: p = p + p[lane ^ s].  Nothing of it depends on the grid, the chunk size or the run;
//   * merged_k[i] = float32(sc[i] / sw) when sw > 0 (a correctly rounded divide, a round-to-nearest-even cast); otherwise
//     (every voter exactly at the threshold) box k's own coordinates;  votes_k = the number of voters, >= 1;
//   * the row of a box that is not kept holds its own box and votes = 0.
// Cost: K * n IoU tests for K kept boxes (ceil(n / 64) per lane and kept box).
//
// One kernel, one launch, no atomics, no scratch, no host synchronisation.  One wave per box, four waves per workgroup: a
// wave whose box is not kept writes its row and has nothing to sum -- nobody has to count or compact the kept boxes on the
// host -- and a workgroup without any kept box leaves at once.  In the other workgroups all 256 threads stage the
// candidates through LDS, WB_VOTE_CHUNK = 256 at a time (box, weight, group: 28 bytes each, 7 KiB in all), and each wave
// with a kept box walks the chunk 64 candidates at a time: one global read of a candidate serves up to four kept boxes.
// Lane l reads the 16 bytes of box l of its 64: consecutive lanes read consecutive 16-byte slots, the layout
// ds_read_b128 serves without a bank conflict; the weight (8 bytes) and the group (4 bytes) lie in arrays of their own for
// the same reason.  Liveness is folded into the staged weight: -1 marks a candidate that is not live or lies behind the
// last box (a live weight is never negative).  The fp64 work per candidate is some twenty operations and one divide.
#include "wb_match_iou.h"   // the float64 IoU

#define WB_VOTE_WAVES 4
#define WB_VOTE_CHUNK 256           // candidates staged at a time: one per thread, a multiple of 64

namespace {

__device__ inline double vote_weight(int weights, float score, float score_threshold) {
    return weights == WB_VOTE_SCORE ? __dsub_rn((double)score, (double)score_threshold) : 1.0;
}

__global__ __launch_bounds__(64 * WB_VOTE_WAVES) void vote_kernel(const float4 *boxes, const float *scores, const int32_t *group,
                                                                  const uint8_t *keep, int64_t n, double vote_iou, int weights,
                                                                  int use_score_threshold, float score_threshold, float4 *merged,
                                                                  int32_t *votes) {
    __shared__ float4 s_box[WB_VOTE_CHUNK];
    __shared__ double s_w[WB_VOTE_CHUNK];
    __shared__ int32_t s_group[WB_VOTE_CHUNK];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int64_t k = (int64_t)blockIdx.x * WB_VOTE_WAVES + (tid >> 6);
    const bool mine = k < n;
    const int64_t kk = mine ? k : n - 1;                       // (waves behind the last box stage with everyone else)
    const float4 bk = boxes[kk];
    const bool kept = mine && keep[kk] != 0;                   // (wave-uniform)
    if (mine && !kept && lane == 0) {
        merged[k] = bk;
        votes[k] = 0;
    }
    if (!__syncthreads_or(kept)) return;                       // (workgroup-uniform)

    const MatchBox a = match_box(bk);
    const int32_t gk = group ? group[kk] : 0;
    const double wk = vote_weight(weights, scores[kk], score_threshold);
    double sw = 0.0, sc[4] = {0.0, 0.0, 0.0, 0.0};
    int32_t cnt = 0;
    for (int64_t c0 = 0; c0 < n; c0 += WB_VOTE_CHUNK) {
        __syncthreads();                                       // the last chunk has been read by everyone
        const int64_t j = c0 + tid;
        if (j < n) {
            const float s = scores[j];
            const bool live = !use_score_threshold || s >= score_threshold;
            s_box[tid] = boxes[j];
            s_w[tid] = live ? vote_weight(weights, s, score_threshold) : -1.0;
            s_group[tid] = group ? group[j] : 0;
        } else {
            s_box[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
            s_w[tid] = -1.0;
            s_group[tid] = 0;
        }
        __syncthreads();
        if (!kept) continue;
        for (uint32_t t0 = 0; t0 < WB_VOTE_CHUNK && c0 + t0 < n; t0 += 64) {
            const uint32_t t = t0 + lane;
            const float4 b = s_box[t];
            double w = s_w[t];
            const bool self = c0 + t == k;
            const double v = match_iou(a, (double)b.x, (double)b.y, (double)b.z, (double)b.w);
            const bool voter = self || (w >= 0.0 && s_group[t] == gk && v >= vote_iou);
            if (self) w = wk;
            if (voter) {
                sw = __dadd_rn(sw, w);
                sc[0] = __dadd_rn(sc[0], __dmul_rn(w, (double)b.x));
                sc[1] = __dadd_rn(sc[1], __dmul_rn(w, (double)b.y));
                sc[2] = __dadd_rn(sc[2], __dmul_rn(w, (double)b.z));
                sc[3] = __dadd_rn(sc[3], __dmul_rn(w, (double)b.w));
                ++cnt;
            }
        }
    }
    if (!kept) return;
    for (int s = 1; s < WB_WAVE; s <<= 1) {                    // the butterfly, on the two halves of each double
        sw = __dadd_rn(sw, __shfl_xor(sw, s, WB_WAVE));
        for (int i = 0; i < 4; ++i) sc[i] = __dadd_rn(sc[i], __shfl_xor(sc[i], s, WB_WAVE));
        cnt += __shfl_xor(cnt, s, WB_WAVE);
    }
    if (lane == 0) {
        merged[k] = sw > 0.0 ? make_float4((float)(sc[0] / sw), (float)(sc[1] / sw), (float)(sc[2] / sw), (float)(sc[3] / sw)) : bk;
        votes[k] = cnt;
    }
}

}  // namespace

extern "C" int wb_vote_launch(void *stream, const float *boxes, const float *scores, const int32_t *group, const uint8_t *keep,
                              int64_t n, double vote_iou, int weights, int use_score_threshold, float score_threshold,
                              float *merged, int32_t *votes) {
    WB_REQUIRE(n >= 0, "wb_vote_launch: n = %lld: negative", (long long)n);
    WB_REQUIRE(vote_iou >= 0.0, "wb_vote_launch: vote_iou must be a number >= 0");
    WB_REQUIRE(weights == WB_VOTE_UNIFORM || weights == WB_VOTE_SCORE, "wb_vote_launch: weights = %d (WB_VOTE_UNIFORM or WB_VOTE_SCORE)",
               weights);
    WB_REQUIRE(weights != WB_VOTE_SCORE || use_score_threshold, "wb_vote_launch: WB_VOTE_SCORE weights need a score threshold");
    WB_REQUIRE(!use_score_threshold || score_threshold == score_threshold, "wb_vote_launch: score_threshold is NaN");
    if (n == 0) return WB_OK;
    WB_REQUIRE(boxes && scores && keep && merged && votes, "wb_vote_launch: null pointer");
    WB_REQUIRE(wb_aligned(boxes, 16) && wb_aligned(merged, 16), "wb_vote_launch: boxes and merged must be 16-byte aligned");
    WB_REQUIRE(wb_aligned(scores, 4) && wb_aligned(group, 4) && wb_aligned(votes, 4),
               "wb_vote_launch: scores, group and votes must be 4-byte aligned");
    if (n > WB_LABEL_MAX_DET) {
        wb_set_error("wb_vote_launch: %lld boxes (at most %d in one call)", (long long)n, WB_LABEL_MAX_DET);
        return WB_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(vote_kernel, dim3((uint32_t)((n + WB_VOTE_WAVES - 1) / WB_VOTE_WAVES)), dim3(64 * WB_VOTE_WAVES), 0,
                       (hipStream_t)stream, reinterpret_cast<const float4 *>(boxes), scores, group, keep, n, vote_iou, weights,
                       use_score_threshold, score_threshold, reinterpret_cast<float4 *>(merged), votes);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
