"""The rule of multiple-instance pruning (calibration.instance_windows / prune_instances; csrc/wb_mip.hip:
wb_mip_windows_launch, wb_mip_prune_launch), stated in NumPy.  No GPU, no torch.

  windows(levels, inv_scale, m, n, gts, ignores, min_iou)   the acceptable windows of the window grids of a batch of pyramids
  f32_key(x) / key_f32(k)                                    wb_f32_key: uint32 keys whose unsigned order is float order
  bag_floor(F, bag, n_bags, recall)                          the floor: the keep-th largest bag maximum of the final scores
  prune(trace, bag, n_bags, floor, margin)                   the stage-sequential prune
"""
import math

import numpy as np

import mine_reference as mref

ROW = mref.ROW


def window_grid(u, v, m, n):
    """(rows, cols) of the windows the scan visits on a u x v level: r in [0, u - m), c in [0, v - n)."""
    return max(int(u) - int(m), 0), max(int(v) - int(n), 0)


def windows(levels, inv_scale, m, n, gts, ignores, min_iou=0.7):
    """levels: [(u, v)] per pyramid level; gts[b]: image b's float64 [G, 4] (None / empty: no ground truth); ignores[b]:
    its flags.  Returns dict(rows: the acceptable windows as ROW records in (image, level, r, c) order -- score 0, label 1,
    best and owner as wb_match_launch gives them; reachable / unreachable: int64 [K, 2] (image, index) of the non-ignored
    ground-truth boxes that own an acceptable window / own none, in (image, index) order)."""
    inv_scale = np.asarray(inv_scale, np.float32)
    out, reach, unreach = [], [], []
    for b, g in enumerate(gts):
        if g is None or len(g) == 0:
            continue
        g = np.asarray(g, np.float64).reshape(-1, 4)
        ign = np.asarray(ignores[b]) != 0
        owned = np.zeros(len(g), bool)
        for l, (u, v) in enumerate(levels):
            nr, nc = window_grid(u, v, m, n)
            if nr == 0 or nc == 0:
                continue
            r, c = (x.reshape(-1) for x in np.indices((nr, nc)))
            boxes = mref.record_boxes(np.full(r.size, l), r, c, inv_scale, m, n)
            t = mref.iou_table(boxes, g)
            owner = np.argmax(t, axis=1)                                    # the first candidate that reaches the maximum
            best = t[np.arange(r.size), owner]
            ok = np.flatnonzero((best > float(min_iou)) & ~ign[owner])
            rows = np.zeros(ok.size, ROW)
            rows["image"], rows["level"], rows["r"], rows["c"] = b, l, r[ok], c[ok]
            rows["best"], rows["owner"], rows["label"] = best[ok], owner[ok], 1
            out.append(rows)
            owned[owner[ok]] = True
        reach += [(b, k) for k in np.flatnonzero(owned)]
        unreach += [(b, k) for k in np.flatnonzero(~owned & ~ign)]
    pairs = lambda x: np.array(x, np.int64).reshape(-1, 2)
    return dict(rows=np.concatenate(out) if out else np.zeros(0, ROW), reachable=pairs(reach), unreachable=pairs(unreach))


def bags_of(rows, reachable):
    """The bag of every row: the position of (image, owner) in `reachable`."""
    index = {(int(b), int(k)): i for i, (b, k) in enumerate(reachable)}
    return np.array([index[(int(w["image"]), int(w["owner"]))] for w in rows], np.int32).reshape(-1)


def f32_key(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_f32(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & 0x80000000, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def keep_count(recall, n):
    return min(n, max(1, math.ceil(recall * n)))


def bag_maxima(F, bag, n_bags):
    """(keys uint32 [n_bags] of the largest F of every bag, 0 for a bag without windows; the bags that have windows)."""
    G = np.zeros(n_bags, np.uint32)
    np.maximum.at(G, np.asarray(bag, np.int64), f32_key(F))
    present = np.zeros(n_bags, bool)
    present[np.asarray(bag, np.int64)] = True
    return G, present


def bag_floor(F, bag, n_bags, recall):
    """(floor float32, keep): the keep-th largest of the bags' maxima of F, keep = keep_count(recall, bags that have
    windows); bag ids without windows contribute nothing."""
    G, present = bag_maxima(F, bag, n_bags)
    G = np.sort(G[present])[::-1]
    keep = keep_count(recall, G.size)
    return key_f32(G[keep - 1:keep])[0], keep


def prune(tr, bag, n_bags, floor, margin=0.0):
    """The rule on an unrejected trace tr (N, T) float32 (no NaN), bag (N,) in [0, n_bags): dict(theta float32 (T,),
    removed_at int32 (N,), initial (N,) bool, retained_bags, surviving)."""
    tr = np.asarray(tr, np.float32)
    N, T = tr.shape
    bag = np.asarray(bag, np.int64)
    theta = np.full(T, np.inf, np.float32)
    removed_at = np.full(N, -1, np.int32)
    if N == 0 or T == 0:
        return dict(theta=theta, removed_at=removed_at, initial=np.zeros(N, bool), retained_bags=0, surviving=0)
    initial = tr[:, -1] >= np.float32(floor)
    live = initial.copy()
    removed_at[live] = T
    for t in range(T):
        if not live.any():
            break
        G = np.zeros(n_bags, np.uint32)                                    # key 0: a bag without retained windows
        np.maximum.at(G, bag[live], f32_key(tr[live, t]))
        theta[t] = key_f32(G[G != 0].min(keepdims=True))[0]
        gone = live & ~(tr[:, t] >= theta[t])                              # the cascade's test
        removed_at[gone] = t
        live &= ~gone
    with np.errstate(over="ignore"):
        out = (theta - np.float32(margin)).astype(np.float32)
    return dict(theta=out, removed_at=removed_at, initial=initial, retained_bags=int(np.unique(bag[initial]).size),
                surviving=int((removed_at == T).sum()))


def backward(tr, keep_rows):
    """calibrate(recall=1.0) on the rows keep_rows of the trace: the minimum of every stage over them (on keys)."""
    tr = np.asarray(tr, np.float32)
    return key_f32(f32_key(tr[keep_rows]).min(axis=0))
