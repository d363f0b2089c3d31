"""The NumPy statement of ``waldboost_amd.fpga.DTree.fit`` -- the yardstick of the fit tests (the reference's
fpga/training.py:15-171 with NumPy 1.x semantics for uint8 samples, stated without its per-feature Python loop).

Inputs: X0, X1 (N, m, n, C) samples of class 0 / 1, W0, W1 weights.  X is the two sets concatenated and flattened to
(N, F) features, Y their class.  Split weights w' = W with each class divided by twice its sum, once over all samples.

Nodes are numbered breadth first (a FIFO); a node is a leaf when depth == max_depth or it holds fewer than
min_samples_leaf samples (empty leaves occur and are kept).  A split node with sample set S and ordered feature list A
(allowed_features[depth], or all features) rates, for every f in A, the integer thresholds t = xmin .. xmax + 1 (xmin,
xmax over S, both classes; 256 is a legal threshold):

    L_c(t) = sum of w' over the class-c samples of S with x_f < t,  T_c = L_c(xmax + 1),  R_c = T_c - L_c
    M(f, t) = H(T0, T1) - ((L0 + L1) / (T0 + T1) * H(L0 + 1e-4, L1 + 1e-4) + (R0 + R1) / (T0 + T1) * H(R0 + 1e-4, R1 + 1e-4))
    H(a, b) = -(a / (a + b) * log2(a / (a + b)) + b / (a + b) * log2(b / (a + b)))

in float64.  Per feature the smallest t with the largest M wins, over features the first entry of A with the largest M
(np.argmax both times: a NaN is the largest value, so a node in which one class is absent or weightless -- every M is
NaN there -- answers (A[0], its xmin)).  The node stores (f, t) and routes with x_f <= t (the metric rated x_f < t:
the reference's own difference).  Every node, leaf or not, predicts log((sum W[y==1] + 1e-3) / (sum W[y==0] + 1e-3)) / 2
from the unnormalised W, stored as float32, clipped to +-clip, then round(quantizer * pred) / quantizer.

``fit`` returns the tree and, per node, its sample set and (for split nodes) the whole metric table.
"""
from collections import deque

import numpy as np

from waldboost_amd.training import DTree

NO_CANDIDATE = -np.inf          # entry of a metric table at a (feature, t) that is no candidate of the node


def entropy(a, b):
    tot = a + b
    return -((a / tot) * np.log2(a / tot) + (b / tot) * np.log2(b / tot))


def metric_table(X, Y, w, S, A):
    """M[(entry of A), t] for t = 0 .. 256 over the samples S (indices into X, Y, w); NO_CANDIDATE outside xmin .. xmax + 1."""
    A = np.asarray(A)
    xs = X[np.ix_(S, A)].astype(np.int64)                    # (|S|, |A|)
    nA = A.size
    L = np.zeros((2, nA, 257))
    for c in (0, 1):
        rows = Y[S] == c
        flat = (xs[rows] + 256 * np.arange(nA)[None, :]).ravel()
        hist = np.bincount(flat, weights=np.repeat(w[S][rows].astype(np.float64), nA), minlength=256 * nA).reshape(nA, 256)
        L[c, :, 1:] = np.cumsum(hist, axis=1)
    xmin, xmax = xs.min(axis=0), xs.max(axis=0)
    t = np.arange(257)[None, :]
    cand = (t >= xmin[:, None]) & (t <= xmax[:, None] + 1)
    T = np.take_along_axis(L, np.broadcast_to((xmax + 1)[None, :, None], (2, nA, 1)), axis=2)       # (2, nA, 1)
    R = T - L
    with np.errstate(all="ignore"):
        tsum = T[0] + T[1]
        M = entropy(T[0], T[1]) - ((L[0] + L[1]) / tsum * entropy(L[0] + 1e-4, L[1] + 1e-4) +
                                   (R[0] + R[1]) / tsum * entropy(R[0] + 1e-4, R[1] + 1e-4))
    return np.where(cand, M, NO_CANDIDATE)


def best_split(M):
    """(entry of A, t, metric) of a metric table: np.argmax per feature, then over features."""
    t = np.argmax(M, axis=1)
    m = M[np.arange(M.shape[0]), t]
    k = int(np.argmax(m))
    return k, int(t[k]), m[k]


def table_gap(M):
    """The best metric minus the largest strictly smaller value of the table (NaN tables: NaN)."""
    v = M[M != NO_CANDIDATE]
    if np.isnan(v).any():
        return np.nan
    best = v.max()
    rest = v[v < best]
    return best - rest.max() if rest.size else np.inf


def split_weights(W, Y):
    """w': W with each class divided by twice its sum, in W's dtype (the reference's expression; the contract is stated on
    float64 weights -- fpga.DTree.fit widens any other float type to float64 first)."""
    w = W.copy()
    with np.errstate(all="ignore"):
        w[Y == 0] /= w[Y == 0].sum() * 2
        w[Y == 1] /= w[Y == 1].sum() * 2
    return w


def fit(X0, W0, X1, W1, max_depth=2, min_samples_leaf=10, allowed_features=None, clip=3, quantizer=32):
    """-> (tree, nodes): a waldboost_amd.training.DTree and per node a dict with 'samples', 'depth', and for split
    nodes 'A', 'table' (metric_table), 'feature' (flat index), 'threshold', 'metric', 'gap', 'left', 'right'."""
    shape = X0.shape[1:]
    F = int(np.prod(shape))
    X = np.concatenate([np.asarray(X0).reshape(-1, F), np.asarray(X1).reshape(-1, F)])
    Y = np.array([0] * X0.shape[0] + [1] * X1.shape[0])
    W = np.concatenate([W0, W1])
    w = split_weights(W, Y)
    nodes = []
    todo = deque([(np.arange(W.size), 0, 0)])
    n_ids = 1
    while todo:
        S, depth, nid = todo.popleft()
        node = dict(samples=S, depth=depth, feature=-1, threshold=-1, left=-1, right=-1)
        if depth != max_depth and not S.size < min_samples_leaf:
            A = np.arange(F) if allowed_features is None else np.asarray(allowed_features[depth])
            M = metric_table(X, Y, w, S, A)
            k, t, m = best_split(M)
            f = int(A[k])
            goes_left = X[S, f] <= t
            node.update(A=A, table=M, feature=f, threshold=t, metric=m, gap=table_gap(M), left=n_ids, right=n_ids + 1)
            todo.append((S[goes_left], depth + 1, n_ids))
            todo.append((S[~goes_left], depth + 1, n_ids + 1))
            n_ids += 2
        assert nid == len(nodes)
        nodes.append(node)
    pred = np.empty(len(nodes), "f")
    for i, node in enumerate(nodes):
        y, ws = Y[node["samples"]], W[node["samples"]]
        pred[i] = np.log((ws[y == 1].sum() + 1e-3) / (ws[y == 0].sum() + 1e-3)) / 2
    if clip is not None:
        pred = np.clip(pred, -clip, clip)
    if quantizer is not None:
        pred = np.round(quantizer * pred) / quantizer
    feature = [np.unravel_index(n["feature"], shape) if n["feature"] >= 0 else None for n in nodes]
    tree = DTree(feature, np.array([n["threshold"] for n in nodes], np.float64), [n["left"] for n in nodes],
                 [n["right"] for n in nodes], pred)
    return tree, nodes


def node_prediction(W, Y, samples, clip=3, quantizer=32):
    """The prediction of a node with the given sample set, as `fit` computes it."""
    pred = np.empty(1, "f")
    y, ws = Y[samples], W[samples]
    pred[0] = np.log((ws[y == 1].sum() + 1e-3) / (ws[y == 0].sum() + 1e-3)) / 2
    if clip is not None:
        pred = np.clip(pred, -clip, clip)
    if quantizer is not None:
        pred = np.round(quantizer * pred) / quantizer
    return pred[0]
