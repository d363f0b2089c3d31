"""The NumPy statement of threshold calibration (waldboost_amd/calibration.py; csrc/wb_cascade.hip:
wb_samples_trace_launch, wb_calib_min_launch).

Trees are the oracle's plain dicts (oracle.wb_oracle.make_tree); a sample walks a tree with ``X[i, r, c, ch] <=
threshold`` (oracle.tree_apply) and the running score is a float32 ``+=`` in stage order, from 0.

  trace(trees, X)                  (N, T) float32: the running score after every stage, no rejection
  trace_rejecting(trees, thetas, X) ((N, T) float32, alive int64 (T + 1,)): the thetas applied as Model.predict applies
                                   them (``H >= theta``, -inf never rejects); -inf from the rejecting stage on;
                                   alive[t] = samples entering stage t, alive[T] = samples passing every stage
  prune(trace, recall, margin)     the pruning rule on an unrejected trace
"""
import math

import numpy as np

from oracle import wb_oracle as orc


def trace(trees, X):
    N = X.shape[0]
    out = np.zeros((N, len(trees)), np.float32)
    h = np.zeros(N, np.float32)
    for t, tree in enumerate(trees):
        h += tree["prediction"][orc.tree_apply(tree, X)]
        out[:, t] = h
    return out


def trace_rejecting(trees, thetas, X):
    N, T = X.shape[0], len(trees)
    out = np.full((N, T), -np.inf, np.float32)
    alive = np.zeros(T + 1, np.int64)
    h = np.zeros(N, np.float32)
    mask = np.ones(N, bool)
    for t, (tree, theta) in enumerate(zip(trees, thetas)):
        alive[t] = mask.sum()
        h[mask] += tree["prediction"][orc.tree_apply(tree, X[mask, ...])]
        if theta != -np.inf:
            mask = np.logical_and(mask, h >= theta)
        out[mask, t] = h[mask]
    alive[T] = mask.sum()
    return out, alive


def keep_count(recall, n):
    return min(n, max(1, math.ceil(recall * n)))


def prune(tr, recall, margin=0.0):
    """The rule on an unrejected trace tr (N, T): dict(keep, floor, retained (N,) bool, theta float32 (T,))."""
    N, T = tr.shape
    F = tr[:, -1]
    keep = keep_count(recall, N)
    floor = np.sort(F)[::-1][keep - 1]
    retained = F >= floor
    theta = tr[retained].min(axis=0).astype(np.float32) - np.float32(margin)
    return dict(keep=keep, floor=np.float32(floor), retained=retained, theta=theta.astype(np.float32))
