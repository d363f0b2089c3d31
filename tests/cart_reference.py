"""The NumPy statement of ``waldboost_amd.training.DTree.fit`` -- the yardstick of the CART tests: scikit-learn's
``DecisionTreeClassifier(class_weight="balanced")``, gini criterion, best splitter (the learner behind the reference's
training.py:33-50), with integer weights and a fixed rule for exact ties.

Inputs: X0, X1 (N, m, n, C) float32 or uint8 samples of class 0 / 1, W0, W1 weights.  X is the two sets concatenated,
flattened to (N, F) and widened to float32, Y their class.

    sw_i = W_i * (N / (2 * count(Y == Y_i)))            float64; the balanced class weight counts samples, not weight
    q_i  = rint(sw_i * 2^k)                             integers; k = min(61 - e, 1000), fsum(sw) = m * 2^e, 0.5 <= m < 1

Every weight sum and difference below is an integer operation; a sum converts to float64 once, times 2^-k (exact).

A node with sample set S, n = |S|, class totals T0, T1 is a leaf when depth == max_depth, n < min_samples_split,
n < 2 * min_samples_leaf, 1 - (t0^2 + t1^2) / (t0 + t1)^2 <= DBL_EPSILON, or no feature has a valid candidate.  Else,
per feature f with xs the float32 values of S sorted (-0.0 equal to +0.0):

    the feature is constant, and skipped, when xs[n-1] <= xs[0] + 1e-7f                 (float32 add)
    p in 1 .. n-1 is a candidate when xs[p] > xs[p-1] + 1e-7f (float32 add) and p >= min_samples_leaf and
        n - p >= min_samples_leaf
    L = class sums of the first p sorted samples, R = T - L
    proxy = (l0*l0 + l1*l1) / (l0 + l1) + (r0*r0 + r1*r1) / (r0 + r1)                   float64; a NaN never wins

The largest proxy wins; among equal proxies the smallest flat feature index, then the smallest p (sklearn's pick among
exact ties depends on random_state: this rule is the build's own).  threshold = xs[p-1] / 2.0 + xs[p] / 2.0 in float64,
replaced by xs[p-1] if it equals xs[p] or is infinite; samples with double(x_f) <= threshold go left.  Nodes are numbered
in pre-order, left first.  Node n predicts log(w1 / w0) / 2 with w_c = (W * (leaf == n) * (Y == c)).sum() + 1e-3 (the
reference's expression: 0 on internal nodes); the tree stores thresholds as float32, -2 on leaves.
"""
import math

import numpy as np

from waldboost_amd.training import DTree

FEATURE_THRESHOLD = np.float32(1e-7)


def split_weights(W, Y):
    """(q, k): uint64 integer weights and the power of two they are scaled by."""
    N = Y.size
    counts = np.bincount(Y, minlength=2)
    sw = np.asarray(W, np.float64) * (N / (2.0 * counts))[Y]
    k = min(61 - math.frexp(math.fsum(sw))[1], 1000)
    return np.rint(np.ldexp(sw, k)).astype(np.uint64), k


def half_proxy(a, b):
    return (a * a + b * b) / (a + b)


def proxy_table(X, Y, q, S, scale, min_samples_leaf):
    """(proxy[p-1, f] for p = 1 .. n-1 -- -inf where p is no candidate or the proxy is NaN --, xs[n, F] the sorted
    columns) over the samples S."""
    n = S.size
    x = X[S] + np.float32(0.0)                                  # (-0.0 + 0.0 = +0.0)
    o = np.argsort(x, axis=0, kind="stable")
    xs = np.take_along_axis(x, o, axis=0)
    with np.errstate(all="ignore"):
        constant = xs[-1] <= xs[0] + FEATURE_THRESHOLD
        cand = xs[1:] > xs[:-1] + FEATURE_THRESHOLD
    p = np.arange(1, n)[:, None]
    cand &= (p >= min_samples_leaf) & (n - p >= min_samples_leaf) & ~constant[None, :]
    q0 = np.where(Y[S] == 0, q[S], np.uint64(0)).astype(np.uint64)
    q1 = np.where(Y[S] == 1, q[S], np.uint64(0)).astype(np.uint64)
    T0, T1 = q0.sum(dtype=np.uint64), q1.sum(dtype=np.uint64)
    L0 = np.cumsum(q0[o], axis=0, dtype=np.uint64)[:-1]
    L1 = np.cumsum(q1[o], axis=0, dtype=np.uint64)[:-1]
    with np.errstate(all="ignore"):
        l0, l1 = L0.astype(np.float64) * scale, L1.astype(np.float64) * scale
        r0, r1 = (T0 - L0).astype(np.float64) * scale, (T1 - L1).astype(np.float64) * scale
        proxy = half_proxy(l0, l1) + half_proxy(r0, r1)
    proxy = np.where(cand & ~np.isnan(proxy), proxy, -np.inf)
    return proxy, xs


def pick(proxy):
    """(f, p) of the winner: the largest proxy, then the smallest feature, then the smallest p; None without candidates."""
    if proxy.size == 0 or not np.any(proxy > -np.inf):
        return None
    best = proxy.max()
    per_feature = proxy.max(axis=0)
    f = int(np.flatnonzero(per_feature == best)[0])
    p = int(np.flatnonzero(proxy[:, f] == best)[0]) + 1
    return f, p


def threshold_of(lo, hi):
    with np.errstate(all="ignore"):
        t = np.float64(lo) / 2.0 + np.float64(hi) / 2.0
    if t == np.float64(hi) or np.isinf(t):
        t = np.float64(lo)
    return t


def table_gap(proxy):
    """Relative lead of the best proxy over the largest strictly smaller one, and the number of features that reach the
    best."""
    v = proxy[proxy > -np.inf]
    best = v.max()
    rest = v[v < best]
    gap = (best - rest.max()) / abs(best) if rest.size else np.inf
    return gap, int((proxy.max(axis=0) == best).sum())


def fit(X0, W0, X1, W1, max_depth, min_samples_leaf=1, min_samples_split=2, **ignored):
    """-> (tree, nodes): a waldboost_amd.training.DTree and per pre-order node a dict with 'samples' (ascending), 'depth',
    'T0', 'T1' (ints), 't0', 't1', and for searched nodes 'table' (proxy_table), for split nodes also 'feature' (flat),
    'p', 'lo', 'hi', 'proxy', 'threshold' (float64), 'left', 'right', 'gap', 'winners'."""
    shape = X0.shape[1:]
    F = int(np.prod(shape))
    X = np.concatenate([np.asarray(X0).reshape(-1, F), np.asarray(X1).reshape(-1, F)]).astype(np.float32)
    Y = np.array([0] * X0.shape[0] + [1] * X1.shape[0])
    W = np.concatenate([W0, W1])
    q, k = split_weights(W, Y)
    scale = math.ldexp(1.0, -k)
    nodes = []

    def grow(S, depth):
        T0, T1 = int(q[S[Y[S] == 0]].sum()), int(q[S[Y[S] == 1]].sum())
        t0, t1 = np.float64(float(T0) * scale), np.float64(float(T1) * scale)
        node = dict(samples=S, depth=depth, T0=T0, T1=T1, t0=t0, t1=t1, feature=-1, left=-1, right=-1)
        nid = len(nodes)
        nodes.append(node)
        n = S.size
        with np.errstate(all="ignore"):
            impurity = 1.0 - (t0 * t0 + t1 * t1) / ((t0 + t1) * (t0 + t1))
        if depth == max_depth or n < min_samples_split or n < 2 * min_samples_leaf or impurity <= np.finfo(np.float64).eps:
            return nid
        table, xs = proxy_table(X, Y, q, S, scale, min_samples_leaf)
        node["table"] = table
        win = pick(table)
        if win is None:
            return nid
        f, p = win
        lo, hi = xs[p - 1, f], xs[p, f]
        thr = threshold_of(lo, hi)
        gap, winners = table_gap(table)
        goes_left = X[S, f].astype(np.float64) <= thr
        assert int(goes_left.sum()) == p
        node.update(feature=f, p=p, lo=lo, hi=hi, proxy=table[p - 1, f], threshold=thr, gap=gap, winners=winners)
        node["left"] = grow(S[goes_left], depth + 1)
        node["right"] = grow(S[~goes_left], depth + 1)
        return nid

    grow(np.arange(Y.size), 0)
    leaf = np.empty(Y.size, np.int64)
    for i, node in enumerate(nodes):
        if node["left"] < 0:
            leaf[node["samples"]] = i
    pred = np.empty(len(nodes))
    for n in range(len(nodes)):
        mask = leaf == n
        w0 = (W * mask * (Y == 0)).sum() + 1e-3
        w1 = (W * mask * (Y == 1)).sum() + 1e-3
        pred[n] = np.log(w1 / w0) / 2
    feature = [np.unravel_index(n["feature"], shape) if n["feature"] >= 0 else None for n in nodes]
    tree = DTree(feature, np.array([n.get("threshold", -2.0) for n in nodes], np.float64), [n["left"] for n in nodes],
                 [n["right"] for n in nodes], pred)
    return tree, nodes
