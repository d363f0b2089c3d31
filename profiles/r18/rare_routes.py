"""One-off timing of the two rare routes whose launches change: python rare_routes.py ROOT (the tree to import from)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
import torch
import waldboost_amd as wb
import waldboost_amd.model as wm
from waldboost_amd import engine as E
from waldboost_amd.synth import synth_image

assert os.path.dirname(os.path.abspath(wb.__file__)) == os.path.join(ROOT, "waldboost_amd")
M = wb.load(os.path.join(ROOT, "tests/golden/models/cfg2_d2_T128.pb"))


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        per.append(time.perf_counter() - t0)
    return {"ms_median": float(np.median(per)) * 1e3, "ms_min": float(np.min(per)) * 1e3, "ms_mean": float(np.mean(per)) * 1e3}


out = {"root": ROOT}
# 1. detect_batch with the ordered batch form switched off
wm._ORDER_BATCH = False
for name, (h, w, b) in {"batch8_1080p": (1080, 1920, 8), "batch5_210x290": (210, 290, 5)}.items():
    imgs = np.stack([synth_image(h, w, 600 + i) for i in range(b)])
    n_det = sum(len(x) for x in M.detect_batch(imgs))
    out[name] = dict(timed(lambda: M.detect_batch(imgs), 30), detections=n_det)
    if hasattr(wm, "_ORDER_BATCH_MAX"):                      # (this build: the host route lies in front; also time the device route)
        keep = wm._HOST_POST_BATCH
        wm._HOST_POST_BATCH = 0
        out[name + "_device_route"] = dict(timed(lambda: M.detect_batch(imgs), 30), detections=n_det)
        wm._HOST_POST_BATCH = keep
wm._ORDER_BATCH = True
# 2. one image, more detections than the one read-back holds, ordered on the device
E._ENGINES.clear()
E.PyramidEngine._FETCH_ROWS = 64
wm._HOST_POST_MAX = 0
for name, (h, w) in {"one_1080p": (1080, 1920), "one_240x320": (240, 320)}.items():
    im = synth_image(h, w, 950)
    n_det = len(M.detect(im))
    out[name] = dict(timed(lambda: M.detect(im), 40), detections=n_det)
print(json.dumps(out))
