"""Diagnostic: what non-maximum suppression costs on the bench image and model (1080p, cfg2_d2_T128, iou_threshold 0.3).

    python tools/nms_timing.py            detections in / kept, Model.detect and Model.detect_stream with and without
                                          the threshold (warm, median of repeated calls), non_max_suppression alone, the
                                          NumPy yardstick on the same boxes on the host
    python tools/nms_timing.py --trace    a few warm Model.detect(iou_threshold=0.3) calls and nothing else: the body of
                                          `rocprofv3 --kernel-trace --stats -- python tools/nms_timing.py --trace`
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import waldboost_amd as wb
from waldboost_amd.synth import synth_image

T = 0.3
M = wb.load(os.path.join(ROOT, "tests/golden/models/cfg2_d2_T128.pb"))
img = synth_image(1080, 1920, 0)


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


if "--trace" in sys.argv:
    for _ in range(10):
        kept = M.detect(img, iou_threshold=T)
    torch.cuda.synchronize()
    print("kept", len(kept))
    sys.exit(0)

from nms_reference import nms_keep
plain = M.detect(img)
kept = M.detect(img, iou_threshold=T)
print(f"image 1080p seed 0, model cfg2_d2_T128, iou_threshold {T}: {len(plain)} detections in, {len(kept)} kept")
t0 = time.perf_counter()
want = nms_keep(plain.get(), plain.get_field("scores"), T)
host = (time.perf_counter() - t0) * 1e3
assert np.array_equal(kept.get(), plain.get()[want])
print(f"yardstick (NumPy, one IoU row per kept box) on the host: {host:.2f} ms")
fmt = lambda r: f"median {r[0]:.3f} ms (min {r[1]:.3f}, max {r[2]:.3f}; 30 calls)"
print("Model.detect(img)                      ", fmt(median_ms(lambda: M.detect(img))))
print("Model.detect(img, iou_threshold=0.3)   ", fmt(median_ms(lambda: M.detect(img, iou_threshold=T))))
print("non_max_suppression(plain, 0.3) alone  ", fmt(median_ms(lambda: wb.non_max_suppression(plain, T))), "(upload, three launches, read-back)")
pinned = [torch.from_numpy(synth_image(1080, 1920, s)).pin_memory().numpy() for s in range(8)]
for batch in (1, 4):
    for kw in ({}, dict(iou_threshold=T)):
        rs = []
        for _ in range(5):
            list(M.detect_stream(pinned, lanes=3, batch=batch, **kw))          # (warm: lanes, graphs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(len(b) for b in M.detect_stream(pinned * 8, lanes=3, batch=batch, **kw))
            rs.append((time.perf_counter() - t0) * 1e3 / (len(pinned) * 8))
        print(f"Model.detect_stream(lanes=3, batch={batch}{', iou_threshold=0.3' if kw else ''}): median {np.median(rs):.3f} ms per image "
              f"(min {min(rs):.3f}, max {max(rs):.3f}; 5 runs of 64 images, {n} boxes returned)")
