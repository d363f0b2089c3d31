#!/usr/bin/env python3
"""Time of threshold calibration on the GPU against its NumPy statement on the host, on the same machine and inputs:

  * tests/golden/models/cfg2_d2_T128.pb (the 128-stage bench model) with every theta at -inf;
  * a pool of `--samples` random float32 samples of the model's window shape (12, 12, 4), resident on the device;
  * calibration.calibrate (recall 0.99: wb_samples_trace_launch for the final scores, a device sort for the floor,
    wb_calib_min_launch, two small read-backs), Model.stage_scores with the trace left on the device and with the
    (N, T) read-back, calibration.stage_survival; and tests/calib_reference.py (trace + prune) in NumPy;
  * a host clock around each call, the device synchronised before the clock starts and before it stops; `--warmup`
    calls are not counted; median, minimum and maximum of `--runs` calls (the statement: of `--host-runs`).

The results are compared before anything is timed.  Needs a GPU; prints one line per measurement.
    python tools/calib_timing.py [--samples 20000] [--runs 30] [--warmup 5] [--host-runs 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import calib_reference as ref  # noqa: E402
import waldboost_amd as wb  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd import calibration  # noqa: E402
from util import oracle_model  # noqa: E402


def timed(f, runs, warmup, sync=True):
    out = []
    for k in range(warmup + runs):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        if sync:
            torch.cuda.synchronize()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    return np.array(out)


def line(what, t):
    print(f"{what}: median {np.median(t) * 1e3:.3f} ms, min {t.min() * 1e3:.3f}, max {t.max() * 1e3:.3f} ({t.size} runs)", flush=True)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    nat.require_gpu()
    M = wb.load(os.path.join(ROOT, "tests", "golden", "models", "cfg2_d2_T128.pb"))
    M.theta = [float("-inf")] * len(M)
    rng = np.random.default_rng(0)
    lo, hi = (float(f(np.concatenate([w.threshold[w.left >= 0] for w in M.classifier]))) for f in (np.min, np.max))
    Xh = rng.uniform(lo, hi, (a.samples,) + tuple(M.shape)).astype(np.float32)      # values across the model's thresholds
    Xd = torch.from_numpy(Xh).cuda()
    trees = oracle_model(M)[2]
    print(f"model: {len(M)} stages, window {tuple(M.shape)}; {a.samples} float32 samples", flush=True)

    # the same answers first
    tr = ref.trace(trees, Xh)
    want = ref.prune(tr, 0.99)
    res = wb.calibrate(M, Xd, recall=0.99, inplace=False)
    assert np.all(res.theta == want["theta"]) and res.retained == want["retained"].sum()
    assert np.array_equal(M.stage_scores(Xd).view(np.uint32), tr.view(np.uint32))

    g_cal = line("calibrate (device pool)", timed(lambda: wb.calibrate(M, Xd, recall=0.99, inplace=False), a.runs, a.warmup))
    g_dev = line("stage_scores, trace left on the device", timed(lambda: M.stage_scores(Xd, device=True), a.runs, a.warmup))
    line("stage_scores with the (N, T) read-back", timed(lambda: M.stage_scores(Xd), a.runs, a.warmup))
    line("stage_survival", timed(lambda: calibration.stage_survival(M, Xd), a.runs, a.warmup))
    h_tr = line("NumPy statement: trace", timed(lambda: ref.trace(trees, Xh), a.host_runs, 1, sync=False))
    h_pr = line("NumPy statement: prune", timed(lambda: ref.prune(tr, 0.99), a.host_runs, 1, sync=False))
    print(f"calibrate: x{(h_tr + h_pr) / g_cal:.0f} against trace + prune on the host; stage_scores on the device: "
          f"x{h_tr / g_dev:.0f} against the host trace", flush=True)


if __name__ == "__main__":
    main()
