"""Diagnostic: what box voting costs on top of non-maximum suppression (iou_threshold 0.3, vote_iou 0.5).

    python tools/vote_timing.py           per box set: boxes in / kept, non_max_suppression alone and merge_detections (warm,
                                          median of repeated calls), for both weight modes
    python tools/vote_timing.py --trace   a few warm merge_detections calls on the first set and nothing else: the body of
                                          `rocprofv3 --kernel-trace --stats -- python tools/vote_timing.py --trace`

The box sets: the detections of the bench image and model (1080p, cfg2_d2_T128: what tools/nms_timing.py times, some 3 000
boxes) and 2^16 detector-like boxes (tests/nms_reference.py detector_like_boxes, the largest set wb_nms_launch orders itself).
The yardstick is non_max_suppression on the same set: both calls upload the boxes and read their result back, so the
difference is the vote kernel (K * N IoU tests for K kept boxes) and the larger read-back (20 bytes per box more)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import waldboost_amd as wb
from nms_reference import detector_like_boxes
from waldboost_amd.synth import synth_image

T, V = 0.3, 0.5


def median_ms(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.sort(ts)
    return float(np.median(ts)), float(ts[0]), float(ts[-1])


def box_sets():
    M = wb.load(os.path.join(ROOT, "tests/golden/models/cfg2_d2_T128.pb"))
    yield "bench image 1080p seed 0, model cfg2_d2_T128", M.detect(synth_image(1080, 1920, 0))
    boxes, scores = detector_like_boxes(1 << 16, 7)
    yield "2^16 detector-like boxes", wb.Boxes(boxes, scores=scores)


if "--trace" in sys.argv:
    name, bx = next(box_sets())
    for _ in range(10):
        out = wb.merge_detections(bx, T, vote_iou=V)
    torch.cuda.synchronize()
    print(name, "kept", len(out))
    sys.exit(0)

fmt = lambda r: f"median {r[0]:.3f} ms (min {r[1]:.3f}, max {r[2]:.3f}; 30 calls)"
for name, bx in box_sets():
    kept = wb.non_max_suppression(bx, T)
    merged = wb.merge_detections(bx, T, vote_iou=V)
    votes = merged.get_field("votes")
    assert len(merged) == len(kept)
    print(f"{name}: {len(bx)} boxes in, {len(kept)} kept at iou_threshold {T}; vote_iou {V}: {int(votes.sum())} votes, "
          f"mean {votes.mean():.2f}, most {int(votes.max())}, {int((votes == 1).sum())} kept boxes alone")
    s = float(np.median(bx.get_field("scores")))
    print("  non_max_suppression alone                     ", fmt(median_ms(lambda: wb.non_max_suppression(bx, T))))
    print("  merge_detections, uniform weights             ", fmt(median_ms(lambda: wb.merge_detections(bx, T, vote_iou=V))))
    print("  non_max_suppression, score_threshold = median ", fmt(median_ms(lambda: wb.non_max_suppression(bx, T, s))))
    print("  merge_detections, score weights, the same     ", fmt(median_ms(lambda: wb.merge_detections(bx, T, s, vote_iou=V, weights="score"))))
