#!/usr/bin/env python3
"""Time of fitting the box regressor on the GPU against its NumPy statement on the host (tests/regress_reference.py), on the
same machine and windows:

  * regression.fit on the six planted-square training images of the mining tests (96 x 128, window (8, 8, 4), an empty
    model, min_iou 0.5, uncapped: 1313 windows, D = 256) -- pyramid, scan, mining, targets, the Gram update, the one
    download and the host solve;
  * its parts on the resident crops: Accumulator.add (wb_gram_launch: two launches) alone, and the host solve alone;
  * the statement on the SAME crops and targets, already on the host as float64: A^T A in NumPy (BLAS) and the solve;
  * wb_regress_predict_launch on the 1313 crops against the statement's predict;
  * a host clock around each call, the device synchronised before the clock starts and before it stops; `--warmup` calls
    are not counted; median, minimum and maximum of `--runs` calls.

The results are compared before anything is timed.  Needs a GPU; prints one line per measurement.
    python tools/regress_timing.py [--flavour float|fpga] [--runs 20] [--warmup 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import regress_reference as rr  # noqa: E402
import waldboost_amd as wb  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd import fpga, regression  # noqa: E402
from waldboost_amd.samples import mine_batch  # noqa: E402

HUGE = 10 ** 9


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
    ap.add_argument("--flavour", choices=["float", "fpga"], default="float")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    nat.require_gpu()
    shape = (8, 8, 4)
    chn = wb.channels.grad_hist if a.flavour == "float" else fpga.grad_hist_4_u1
    dtype = np.float32 if a.flavour == "float" else np.uint8
    M = wb.Model(shape, dict(shrink=2, n_per_oct=8, smooth=1, channels=chn))
    items = [dict(image=it["image"], groundtruth_boxes=wb.Boxes(it["gt"].astype("f"))) for it in rr.planted_images(range(6))]
    gts = [it["groundtruth_boxes"] for it in items]

    # the windows, once: the same crops and targets for both sides
    mined = mine_batch(M, np.stack([it["image"] for it in items]), gts, tp=True, fp=False, min_tp_iou=0.5, max_tp_candidates=HUGE)
    scales = M.detect_raw(items[0]["image"])["scales"]
    T_dev = regression.targets(mined, gts, scales)
    X_host, T_host = rr.features(mined.samples.cpu().numpy()), T_dev.cpu().numpy()
    N, D = X_host.shape
    acc = regression.Accumulator(shape, dtype)
    acc.add(mined.samples, T_dev)
    S = acc.state()
    S_ref = rr.gram(X_host, T_host)
    reg = regression.fit(M, items, max_candidates=HUGE)
    W, b, _, _ = rr.solve(S, 1e-2)
    assert N == reg.n_samples and np.array_equal(reg.W, W) and np.array_equal(reg.b, b)
    rel = np.abs(S - S_ref).max() / np.abs(S_ref).max()
    W_ref, b_ref, _, _ = rr.solve(S_ref, 1e-2)
    pred = reg.predict(mined.samples)
    assert np.array_equal(pred.view(np.uint64), rr.predict(X_host, W, b).view(np.uint64))
    print(f"{a.flavour}: {N} windows, D = {D}; max |S - S_numpy| / max |S| = {rel:.3g}; max |W - W_numpy| = {np.abs(W - W_ref).max():.3g}", flush=True)

    g_fit = line("regression.fit (six images: pyramid, scan, mining, targets, Gram, download, solve)",
                 timed(lambda: regression.fit(M, items, max_candidates=HUGE), a.runs, a.warmup))

    def gram_only():
        fresh.S.zero_()
        fresh.add(mined.samples, T_dev)
    fresh = regression.Accumulator(shape, dtype)
    g_gram = line("Accumulator.add on the resident crops (wb_gram_launch, two launches)", timed(gram_only, a.runs, a.warmup))
    g_solve = line("the host solve (BoxRegressor.from_state)", timed(lambda: regression.BoxRegressor.from_state(shape, S, 1e-2), a.runs, a.warmup, sync=False))
    h_gram = line("NumPy statement: A^T A on the same crops (float64, on the host already)", timed(lambda: rr.gram(X_host, T_host), a.runs, a.warmup, sync=False))
    h_all = line("NumPy statement: A^T A and the solve", timed(lambda: rr.solve(rr.gram(X_host, T_host), 1e-2), a.runs, a.warmup, sync=False))
    g_pred = line("BoxRegressor.predict_device on the resident crops", timed(lambda: reg.predict_device(mined.samples), a.runs, a.warmup))
    h_pred = line("NumPy statement: predict", timed(lambda: rr.predict(X_host, W, b), a.runs, a.warmup, sync=False))
    print(f"fit: {g_fit * 1e3:.2f} ms for the whole call, of which the Gram update {g_gram * 1e3:.3f} ms and the solve {g_solve * 1e3:.2f} ms; "
          f"the statement's Gram and solve on crops already in host memory: {h_all * 1e3:.2f} ms (Gram {h_gram * 1e3:.2f} ms); "
          f"predict x{h_pred / g_pred:.0f} against the statement", flush=True)


if __name__ == "__main__":
    main()
