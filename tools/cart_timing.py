#!/usr/bin/env python3
"""Time training.DTree.fit -- one depth-2 tree on float32 samples of shape (12, 12, 4), 2000 and 24000 of them -- against
scikit-learn's own fit of the same data on the host (DecisionTreeClassifier(class_weight="balanced", max_depth=2), what
the reference's training.DTree.fit runs).

    python tools/cart_timing.py [--samples 2000 24000] [--depth 2] [--repeat 7]

Per size it prints the median and the spread (min .. max) of the wall time of a fit -- host arrays in, tree out: upload,
transpose, the sort, one launch group and one read-back per tree level, node predictions on the host --, the same with
the samples already on the device, the time of the sort kernel alone (device events), scikit-learn's time, and whether
the two trees are equal.  The first fit (library load, allocator warm-up) is not timed.  scikit-learn is needed for the
comparison only; without it the GPU times are printed alone.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def data(n, shape, seed=0):
    rng = np.random.default_rng(seed)
    n0 = n // 2
    n1 = n - n0
    F = int(np.prod(shape))
    X0, X1 = rng.random((n0, F), dtype=np.float32), rng.random((n1, F), dtype=np.float32)
    for f, e in ((7, 0.6), (200, 1.5), (411, 0.8)):            # class 1 skewed within 0 .. 1: informative, no pure region
        X1[:, f] **= np.float32(e)
    X0[rng.random((n0, F)) < 0.5] = 0                           # half of a grad_hist sample carries no gradient
    X1[rng.random((n1, F)) < 0.5] = 0
    return X0.reshape((n0,) + shape), np.exp(rng.normal(0, 1, n0)), X1.reshape((n1,) + shape), np.exp(rng.normal(0, 1, n1))


def wall(fn, repeat):
    import torch
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return np.array(times) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[2000, 24000])
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    import torch
    from waldboost_amd import _native as nat
    from waldboost_amd import training
    try:
        from sklearn.tree import DecisionTreeClassifier
    except ImportError:
        DecisionTreeClassifier = None

    shape = (12, 12, 4)
    ok = True
    fmt = lambda t: f"{np.median(t):9.2f} ms  ({t.min():.2f} .. {t.max():.2f}, n = {t.size})"
    for n in args.samples:
        X0, W0, X1, W1 = data(n, shape)
        tree = training.DTree.fit(X0, W0, X1, W1, max_depth=args.depth)          # (not timed)
        host_in = wall(lambda: training.DTree.fit(X0, W0, X1, W1, max_depth=args.depth), args.repeat)
        D0, D1 = torch.from_numpy(X0).cuda(), torch.from_numpy(X1).cuda()
        resident = wall(lambda: training.DTree.fit(D0, W0, D1, W1, max_depth=args.depth), args.repeat)
        # the sort alone, by device events
        lib = nat.load()
        F = int(np.prod(shape))
        xt = torch.cat([D0.reshape(-1, F), D1.reshape(-1, F)]).t().contiguous()
        order = torch.empty((F, n), dtype=torch.int32, device=xt.device)
        sort_ms = []
        for _ in range(args.repeat + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            nat.check(lib.wb_cart_sort_launch(nat.stream_ptr(), nat.ptr(xt), n, F, nat.ptr(order)), "wb_cart_sort_launch")
            b.record()
            torch.cuda.synchronize()
            sort_ms.append(a.elapsed_time(b))
        sort_ms = np.array(sort_ms[1:])
        print(f"samples {n} x {shape} float32, depth {args.depth}, {tree.left.size} nodes")
        print(f"  training.DTree.fit, host arrays    {fmt(host_in)}")
        print(f"  training.DTree.fit, device tensors {fmt(resident)}")
        print(f"  of which cart_sort_kernel          {fmt(sort_ms)}")
        if DecisionTreeClassifier is not None:
            X = np.concatenate([X0.reshape(-1, F), X1.reshape(-1, F)])
            Y = np.array([0] * X0.shape[0] + [1] * X1.shape[0])
            W = np.concatenate([W0, W1])
            times = []
            for _ in range(max(3, args.repeat // 2)):
                t = time.perf_counter()
                T = DecisionTreeClassifier(class_weight="balanced", max_depth=args.depth, random_state=0).fit(X, Y, sample_weight=W)
                times.append(time.perf_counter() - t)
            times = np.array(times) * 1e3
            shape_of = lambda f: np.unravel_index(f, shape) if f >= 0 else (0, 0, 0)
            same = (np.array_equal(T.tree_.children_left, tree.left) and np.array_equal(T.tree_.threshold.astype(np.float32), tree.threshold)
                    and np.array_equal(np.array([shape_of(f) for f in T.tree_.feature]), tree.feature))
            ok = ok and same
            print(f"  scikit-learn on the host           {fmt(times)}")
            print(f"  ratio (host arrays)                {np.median(times) / np.median(host_in):9.1f} x;  trees equal: {same}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
