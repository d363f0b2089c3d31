#!/usr/bin/env python3
"""Time fpga.DTree.fit at the training workload's shape -- 10 000 samples of (12, 12, 4) uint8 features, depth 2 --
against the NumPy yardstick (tests/fit_reference.py) on the host.  Samples are mostly zero, like grad_hist_4_u1 crops.

    python tools/fit_timing.py [--samples 10000] [--depth 2] [--repeat 5]

Prints the median wall time of a fit (host arrays in, tree out: upload, transpose, one launch group and one read-back per
tree level, node predictions on the host), the time of the yardstick, and their ratio; the trees must be equal.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch
    import fit_reference as fr
    from waldboost_amd import fpga

    rng = np.random.default_rng(0)
    shape = (12, 12, 4)
    n0 = args.samples // 2
    n1 = args.samples - n0
    F = int(np.prod(shape))
    X0, X1 = rng.integers(0, 256, (n0, F)), rng.integers(0, 256, (n1, F))
    for f, d in ((7, 40), (200, -30), (411, 25)):
        X1[:, f] = np.clip(X1[:, f] + d, 0, 255)
    X0[rng.random((n0, F)) < 0.7] = 0
    X1[rng.random((n1, F)) < 0.7] = 0
    X0, X1 = X0.astype(np.uint8).reshape((n0,) + shape), X1.astype(np.uint8).reshape((n1,) + shape)
    W0, W1 = np.exp(rng.normal(0, 1, n0)), np.exp(rng.normal(0, 1, n1))

    tree = fpga.DTree.fit(X0, W0, X1, W1, max_depth=args.depth)          # (first call: library load, allocator warm-up)
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        tree = fpga.DTree.fit(X0, W0, X1, W1, max_depth=args.depth)
        times.append(time.perf_counter() - t)
    gpu = float(np.median(times))
    D0, D1 = torch.from_numpy(X0).cuda(), torch.from_numpy(X1).cuda()
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fpga.DTree.fit(D0, W0, D1, W1, max_depth=args.depth)
        times.append(time.perf_counter() - t)
    resident = float(np.median(times))
    t = time.perf_counter()
    ref, nodes = fr.fit(X0, W0, X1, W1, max_depth=args.depth)
    host = time.perf_counter() - t
    same = bytes(ref.content()) == bytes(tree.content())
    gaps = [n["gap"] for n in nodes if n["left"] >= 0]
    print(f"samples {args.samples} x {shape}, depth {args.depth}, {tree.left.size} nodes")
    print(f"fpga.DTree.fit        {gpu * 1e3:9.2f} ms  (median of {args.repeat}; samples already on the device: {resident * 1e3:.2f} ms)")
    print(f"tests/fit_reference   {host * 1e3:9.2f} ms  (host, NumPy)")
    print(f"ratio                 {host / gpu:9.1f} x")
    print(f"trees equal: {same}; smallest gap of the yardstick's splits: {np.nanmin(gaps):.3g}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
