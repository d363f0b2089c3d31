"""Per-launch time of the octave kernels (PyramidEngine.launch_octaves): HIP events around 50 launches, the best of 3, one
JSON line per workload.  To compare two builds of the library, run this once per build in a fresh process each, alternating
(WB_NATIVE_LIB names the library a process loads):
    python tools/oct_time.py;  WB_NATIVE_LIB=/path/to/other/libwaldboost_hip.so python tools/oct_time.py;  ... """
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd.engine import PyramidEngine  # noqa: E402
from waldboost_amd.synth import synth_image  # noqa: E402

# (H, W, dtype, batch): the benchmark's image at batch 1 and 64, the float64-held chain, an image with a tail octave
WORKLOADS = [(1080, 1920, "uint8", 1), (1080, 1920, "float32", 1), (1080, 1920, "uint8", 64), (1080, 1920, "float32", 64),
             (1080, 1920, "int16", 1), (2048, 2064, "uint8", 1)]


def image(H, W, dtype, seed):
    if dtype == "int16":
        return (synth_image(H, W, seed, np.float32) * 60000.0 - 30000.0).astype(np.int16)
    return synth_image(H, W, seed, np.dtype(dtype))


for H, W, dtype, B in WORKLOADS:
    e = PyramidEngine(H, W, np.dtype(dtype), 2, 8, 1, batch=B)
    e.load_images(np.stack([image(H, W, dtype, s) for s in range(B)]))
    for _ in range(3):
        e.launch_octaves()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            e.launch_octaves()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / 50)
    print(json.dumps({"lib": nat.LIB_PATH, "H": H, "W": W, "dtype": dtype, "batch": B, "us_per_launch": round(min(best) * 1e3, 3),
                      "us_per_image": round(min(best) * 1e3 / B, 3), "rounds_us": [round(t * 1e3, 3) for t in best]}), flush=True)
    del e
