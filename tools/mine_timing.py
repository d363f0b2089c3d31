#!/usr/bin/env python3
"""Time of one pool update -- hard-negative mining of a list of images -- with the host pool (samples.SamplePool: one image
per scan, labels and choice in NumPy, crops copied to the host) against the device pool (samples.DeviceSamplePool at batch 1
and 8: wb_mine_select_launch, wb_mine_gather_launch, samples resident), on the same machine and inputs:

  * tests/golden/models/cfg2_d2_T128.pb truncated to 0, 8 and 128 stages (0: every window of the pyramid is a record);
  * `--images` synthetic 1080p images with planted ground truth (four boxes each), quotas nothing fills, so that every
    update mines every image; default caps (100 per level, image and class);
  * a host clock around `update` on a fresh pool, the device synchronised before the clock stops; the pools alternate
    inside a round; the first round of every setting is the warm-up and is not counted.

The two pools choose by different rules (np.random.choice against the keyed select), so the samples differ; their numbers
are printed.  Needs a GPU; prints one line per setting.
    python tools/mine_timing.py [--images 8] [--rounds 3] [--stages 128,8,0]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import waldboost_amd as wb  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd.samples import DeviceSamplePool, SamplePool  # noqa: E402
from waldboost_amd.synth import synth_image  # noqa: E402


def items_for(count, H=1080, W=1920):
    out = []
    for k in range(count):
        rng = np.random.default_rng(500 + k)
        img = synth_image(H, W, 500 + k).astype(np.int32)
        gt = []
        for _ in range(4):
            side = int(rng.integers(48, 200))
            x, y = int(rng.integers(0, W - side)), int(rng.integers(0, H - side))
            img[y:y + side, x:x + side] += 60
            gt.append([x, y, x + side, y + side])
        out.append(dict(image=np.clip(img, 0, 255).astype(np.uint8), groundtruth_boxes=wb.Boxes(np.array(gt, "f"))))
    return out


def truncated(M, T):
    K = wb.Model(M.shape, M.channel_opts)
    for weak, theta in list(M)[:T]:
        K.append(weak, theta)
    return K


def one_update(make, model, items):
    pool = make()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pool.update(model, items)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, pool.pool_stats()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stages", default="128,8,0")
    a = ap.parse_args()
    nat.require_gpu()
    M = wb.load(os.path.join(ROOT, "tests", "golden", "models", "cfg2_d2_T128.pb"))
    items = items_for(a.images)
    never = dict(min_tp=10 ** 9, min_fp=10 ** 9)
    pools = [("host", lambda: SamplePool(**never)), ("device batch 1", lambda: DeviceSamplePool(batch=1, **never)),
             ("device batch 8", lambda: DeviceSamplePool(batch=8, **never))]
    for T in (int(t) for t in a.stages.split(",")):
        K = truncated(M, T)
        times, stats = {name: [] for name, _ in pools}, {}
        np.random.seed(0)
        for rnd in range(a.rounds + 1):
            for name, make in pools:
                dt, stats[name] = one_update(make, K, items)
                print(f"  stages={T} round {rnd} {name}: {dt * 1e3:.1f} ms", file=sys.stderr, flush=True)
                if rnd:
                    times[name].append(dt)
        ms = lambda name: f"{min(times[name]) * 1e3:.1f} ms (median {float(np.median(times[name])) * 1e3:.1f})"
        host = min(times["host"])
        print(f"stages={T} images={a.images}: " + "; ".join(
            f"{name} {ms(name)}, {stats[name]['num_tp']} tp + {stats[name]['num_fp']} fp" + ("" if name == "host" else f", x{host / min(times[name]):.2f}")
            for name, _ in pools), flush=True)


if __name__ == "__main__":
    main()
