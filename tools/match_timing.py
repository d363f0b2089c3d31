#!/usr/bin/env python3
"""Time of boxes.match_boxes (wb_match_launch) against the host's samples._match_ground_truth, at 2^20 detections against 16
ground-truth boxes and at 4096 against 64 (one image each):

  * match_boxes as a caller sees it: conversion, ONE upload, the launch, ONE read-back -- a host clock around the call, which
    ends in the read-back's synchronise;
  * the bare launch: device events around `reps` launches on resident buffers;
  * samples._match_ground_truth on the same boxes: the dense NumPy form, seven (N x G) float64 temporaries.

The results of the two are compared first (owner exactly, best IoU bit for bit).  Needs a GPU; prints one line per size.
    python tools/match_timing.py [--reps 200] [--rounds 5]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import waldboost_amd as wb  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd.boxes import Boxes  # noqa: E402
from waldboost_amd.samples import _match_ground_truth  # noqa: E402


def boxes_for(n, g, seed, H=1080, W=1920):
    """g ground-truth boxes of 30 .. 200 pixels in an H x W image; n float32 detections, half of them near a box."""
    rng = np.random.default_rng(seed)
    size = rng.uniform(30, 200, (g, 2))
    xy = rng.uniform(0, 1, (g, 2)) * ([W, H] - size)
    gt = np.concatenate([xy, xy + size], 1)
    near = gt[rng.integers(0, g, n)] + rng.normal(0, 8, (n, 4))
    s = rng.uniform(24, 180, (n, 1))
    p = rng.uniform(0, 1, (n, 2)) * ([W, H] - s)
    anywhere = np.concatenate([p, p + s], 1)
    dt = np.where(rng.random((n, 1)) < 0.5, near, anywhere).astype(np.float32)
    return Boxes(dt), Boxes(gt, ignore=np.zeros(g))


def best_of(fn, rounds):
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times), float(np.median(times))


def launch_time(dt, gt, reps, rounds):
    lib, dev = nat.load(), nat.require_gpu()
    n, g = len(dt), len(gt)
    d_dt = torch.from_numpy(np.asarray(dt.get(), np.float64)).to(dev)
    d_gt = torch.from_numpy(np.asarray(gt.get(), np.float64)).to(dev)
    d_img = torch.zeros(n, dtype=torch.int32, device=dev)
    d_off = torch.tensor([0, g], dtype=torch.int32, device=dev)
    best = torch.empty(n, dtype=torch.float64, device=dev)
    owner = torch.empty(n, dtype=torch.int32, device=dev)

    def go():
        nat.check(lib.wb_match_launch(nat.stream_ptr(), nat.ptr(d_dt), nat.ptr(d_img), nat.ptr(d_gt), nat.ptr(d_off), n, g, 1,
                                      nat.ptr(best), nat.ptr(owner)), "wb_match_launch")
    for _ in range(10):
        go()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            go()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e-3)
    return min(out), float(np.median(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    nat.require_gpu()
    for n, g in ((1 << 20, 16), (4096, 64)):
        dt, gt = boxes_for(n, g, n + g)
        best, owner = wb.match_boxes(dt, gt)                   # (also the warm-up)
        h_best, h_owner, _ = _match_ground_truth(dt, gt)
        assert np.array_equal(owner, h_owner) and np.array_equal(best.view(np.uint64), h_best.view(np.uint64)), "results differ"
        for _ in range(2):
            wb.match_boxes(dt, gt)
        surface = best_of(lambda: wb.match_boxes(dt, gt), a.rounds)
        host = best_of(lambda: _match_ground_truth(dt, gt), max(a.rounds // 2, 2))
        bare = launch_time(dt, gt, a.reps if n > 100000 else 10 * a.reps, a.rounds)
        ms = lambda t: f"{t[0] * 1e3:.3f} ms (median {t[1] * 1e3:.3f})"
        print(f"n_dt={n} n_gt={g}: match_boxes with upload and read-back {ms(surface)}; bare launch {ms(bare)}; "
              f"host _match_ground_truth {ms(host)}; matched {int((best > 0.5).sum())} above 0.5", flush=True)


if __name__ == "__main__":
    main()
