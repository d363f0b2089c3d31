"""Designed inputs of the CART level kernels (csrc/wb_cart.hip) whose winner is planted, and emulations of kernels that
get a rule wrong.

A design is one tree level: X (N, F) float32, Y (N,) classes, q (N,) integer weights (scale 1), the open nodes as lists of
sample indices, min_samples_leaf, and per node the planted answer ``(feature, p, lo, hi)`` or ``None`` (no candidate).
``exact_winner`` derives the answer from exact rational arithmetic on the integers, so a planted answer is proved, not
observed: tests/test_cart_designs_host.py holds the planted answer, the rational one and the float64 statement
(tests/cart_reference.py) against each other; tests/test_gpu_cart_designs.py holds the kernels against them.
"""
from fractions import Fraction

import numpy as np

import cart_reference as cr

ULP = np.float32(2.0 ** -24)            # the spacing of float32 in 0.5 .. 1
F32 = np.float32
EPS = np.float32(1e-7)


def _design(name, X, Y, q, nodes, expect, min_leaf=1):
    X = np.ascontiguousarray(np.asarray(X, np.float32))
    return dict(name=name, X=X, Y=np.asarray(Y, np.int64), q=np.asarray(q, np.uint64), nodes=[np.asarray(s, np.int64) for s in nodes],
                expect=expect, min_leaf=min_leaf)


def sorted_node(X, S, f):
    """The node's samples sorted by (value with -0.0 == +0.0, index)."""
    x = X[S, f] + F32(0.0)
    return S[np.lexsort((S, x))]


def candidates(xs, n, min_leaf, ge=False, f64_add=False):
    """The positions p = 1 .. n-1 the rule admits on the sorted values xs (ge / f64_add: the rule got wrong)."""
    if f64_add:
        bound_all, bound = xs[0].astype(np.float64) + 1e-7, xs[:-1].astype(np.float64) + 1e-7
    else:
        bound_all, bound = xs[0] + EPS, xs[:-1] + EPS
    if (xs[-1] < bound_all) if ge else (xs[-1] <= bound_all):
        return []
    step = (xs[1:] >= bound) if ge else (xs[1:] > bound)
    return [p for p in range(1, n) if step[p - 1] and p >= min_leaf and n - p >= min_leaf]


def exact_winner(d, k):
    """(feature, p, lo, hi) of node k by exact rational arithmetic, None without candidates: the largest proxy, then the
    smallest feature, then the smallest p; a 0 / 0 (a NaN in floats) never wins."""
    X, Y, q, S = d["X"], d["Y"], d["q"], d["nodes"][k]
    n = S.size
    best = None
    for f in range(X.shape[1]):
        o = sorted_node(X, S, f)
        xs = X[o, f]
        T = [sum(int(q[i]) for i in o if Y[i] == c) for c in (0, 1)]
        for p in candidates(xs, n, d["min_leaf"]):
            L = [sum(int(q[i]) for i in o[:p] if Y[i] == c) for c in (0, 1)]
            R = [T[0] - L[0], T[1] - L[1]]
            if L[0] + L[1] == 0 or R[0] + R[1] == 0:
                continue
            proxy = Fraction(L[0] ** 2 + L[1] ** 2, L[0] + L[1]) + Fraction(R[0] ** 2 + R[1] ** 2, R[0] + R[1])
            if best is None or proxy > best[0]:
                best = (proxy, f, p, xs[p - 1], xs[p])
    return None if best is None else best[1:]


def statement_winner(d, k):
    """(feature, p, lo, hi, proxy) of node k by the float64 statement, None without candidates."""
    table, xs = cr.proxy_table(d["X"], d["Y"], d["q"], d["nodes"][k], 1.0, d["min_leaf"])
    win = cr.pick(table)
    if win is None:
        return None
    f, p = win
    return f, p, xs[p - 1, f], xs[p, f], table[p - 1, f]


def emulated_winner(d, k, ge=False, global_pred=False, f64_add=False, last_f=False, last_p=False):
    """The winner of a kernel that gets the 1e-7 rule wrong: `>=` for `>`, the predecessor in the whole column instead
    of in the node, or the add in float64; or of a reduction that prefers the larger feature or the larger position among
    equal proxies."""
    X, Y, q, S = d["X"], d["Y"], d["q"], d["nodes"][k]
    n = S.size
    everyone = np.concatenate(d["nodes"])
    best = None
    for f in range(X.shape[1]):
        o = sorted_node(X, S, f)
        xs = X[o, f]
        cand = candidates(xs, n, d["min_leaf"], ge=ge, f64_add=f64_add)
        if global_pred:
            col = np.sort(X[everyone, f])
            cand = [p for p in cand if xs[p] > col[np.searchsorted(col, xs[p], side="left") - 1] + EPS]
        q0 = np.where(Y[o] == 0, q[o], 0).astype(np.uint64)
        q1 = np.where(Y[o] == 1, q[o], 0).astype(np.uint64)
        for p in cand:
            with np.errstate(all="ignore"):
                l0, l1 = np.float64(q0[:p].sum()), np.float64(q1[:p].sum())
                r0, r1 = np.float64(q0[p:].sum()), np.float64(q1[p:].sum())
                m = cr.half_proxy(l0, l1) + cr.half_proxy(r0, r1)
            key = (m, f if last_f else -f, p if last_p else -p)
            if not np.isnan(m) and (best is None or key > best[0]):
                best = (key, f, p, xs[p - 1], xs[p])
    return None if best is None else best[1:]


def float_sum_proxies(X, Y, w, S, f):
    """The proxies of a kernel that adds float64 weights along the sorted column in the given order of S (a stable sort:
    equal values keep the order of S) -- what an order-dependent accumulation computes."""
    x = X[S, f] + F32(0.0)
    o = S[np.argsort(x, kind="stable")]
    w0, w1 = np.where(Y[o] == 0, w[o], 0.0), np.where(Y[o] == 1, w[o], 0.0)
    L0, L1 = np.cumsum(w0)[:-1], np.cumsum(w1)[:-1]
    T0, T1 = np.cumsum(w0)[-1], np.cumsum(w1)[-1]
    with np.errstate(all="ignore"):
        return cr.half_proxy(L0, L1) + cr.half_proxy(T0 - L0, T1 - L1)


def designs():
    out = []
    rng = np.random.default_rng(12)

    # a column that separates the classes, copied, and once more as different values with the same partition: the proxy of
    # a pure split is T0 + T1, which no impure split reaches, and the three columns tie exactly -> the lowest index
    n = 40
    Y = np.array([0, 1] * (n // 2))
    X = rng.random((n, 6)).astype(np.float32)
    sep = np.where(Y == 0, rng.uniform(0.1, 0.4, n), rng.uniform(0.6, 0.9, n)).astype(np.float32)
    X[:, 2] = sep
    X[:, 4] = sep
    X[:, 5] = sep * F32(3.0) + F32(1.0)
    lo, hi = sep[Y == 0].max(), sep[Y == 1].min()
    out.append(_design("duplicated_columns", X, Y, rng.integers(1, 1000, n), [np.arange(n)], [(2, n // 2, lo, hi)]))

    # classes 0 1 0 along one column, equal weights: p = 1 and p = 2 give 4 + 4 and 4 + 4 -> the lowest p
    out.append(_design("equal_positions", [[0.1], [0.2], [0.3]], [0, 1, 0], [4, 4, 4], [[0, 1, 2]], [(0, 1, F32(0.1), F32(0.2))]))

    # a chain 0.5, 0.5 + 2 ulp, ... : every step is 1.19e-7, but 0.5 + 1e-7f rounds to 0.5 + 2 ulp in float32, so no step is a
    # candidate although the chain spans 8 ulp = 4.8e-7 (the column is not constant); column 1 has one ordinary, worse, step
    chain = (F32(0.5) + np.arange(5, dtype=np.float32) * 2 * ULP).astype(np.float32)
    X = np.stack([chain, np.array([0.1, 0.1, 0.1, 0.9, 0.9], np.float32)], axis=1)
    out.append(_design("chain_float32_add", X, [0, 0, 1, 1, 1], [8, 8, 8, 8, 8], [np.arange(5)], [(1, 3, F32(0.1), F32(0.9))]))

    # the same chain alone: a column that is not constant and has no candidate -> no split
    out.append(_design("chain_only", chain[:, None], [0, 0, 1, 1, 1], [8, 8, 8, 8, 8], [np.arange(5)], [None]))

    # steps of exactly 1e-7f from 0: `>` refuses them (the column is constant by the rule), `>=` would take the pure split.
    # Column 1 sorts the classes 1 0 0 1: p = 1 and p = 3 tie (5 + 125 / 15 both ways, the same two float64 terms), p = 2 is worse
    X = np.stack([np.array([0.0, 0.0, 1e-7, 1e-7], np.float32), np.array([0.2, 0.7, 0.1, 0.8], np.float32)], axis=1)
    out.append(_design("exact_step", X, [0, 0, 1, 1], [5, 5, 5, 5], [np.arange(4)], [(1, 1, F32(0.1), F32(0.2))]))

    # two nodes share a column: node 0 holds 0.5 and 0.5 + 3 ulp (a step of 1.8e-7: a candidate), node 1 holds
    # 0.5 + 2 ulp between them and 0.9 -- the predecessor in the whole column is 1 ulp away
    X = np.array([[0.5], [0.5 + 3 * 2.0 ** -24], [0.5 + 2 * 2.0 ** -24], [0.9]], np.float32)
    out.append(_design("per_node_predecessor", X, [0, 1, 0, 1], [3, 3, 3, 3], [[0, 1], [2, 3]],
                       [(0, 1, X[0, 0], X[1, 0]), (0, 1, X[2, 0], X[3, 0])]))

    # -0.0 and +0.0 are one value: no step between them; the split is at 0 | 1
    X = np.array([[-0.0], [0.0], [-0.0], [1.0], [0.0], [1.0]], np.float32)
    out.append(_design("signed_zero", X, [0, 0, 0, 1, 0, 1], [2, 3, 4, 5, 6, 7], [np.arange(6)], [(0, 4, F32(0.0), F32(1.0))]))

    # lo = 2 + 1 ulp, hi = 2 + 2 ulp (ulp 2.4e-7 > 1e-7): the float64 midpoint lies strictly between, a float32 midpoint
    # rounds to even = hi and would send hi's samples left
    two = np.float32(2.0)
    a = np.nextafter(two, F32(3.0))
    b = np.nextafter(a, F32(3.0))
    out.append(_design("midpoint_rounds", [[a], [a], [b], [b]], [0, 0, 1, 1], [1, 2, 3, 4], [np.arange(4)], [(0, 2, a, b)]))

    # min_samples_leaf = 3 on ten samples: the pure split at p = 2 (and at n - p = 2) is not allowed; the best allowed ones
    # are exactly p = 3 and n - p = 3
    x = np.linspace(0.05, 0.95, 10).astype(np.float32)[:, None]
    out.append(_design("min_leaf_left", x, [0, 0, 1, 1, 1, 1, 1, 1, 1, 1], [6] * 10, [np.arange(10)], [(0, 3, x[2, 0], x[3, 0])], min_leaf=3))
    out.append(_design("min_leaf_right", x, [1, 1, 1, 1, 1, 1, 1, 1, 0, 0], [6] * 10, [np.arange(10)], [(0, 7, x[6, 0], x[7, 0])], min_leaf=3))

    # a node of two samples next to one of three
    X = np.array([[0.3, 0.5], [0.6, 0.5], [0.1, 0.2], [0.2, 0.4], [0.3, 0.1]], np.float32)
    out.append(_design("two_samples", X, [1, 0, 0, 1, 1], [7, 9, 2, 2, 2], [[0, 1], [2, 3, 4]],
                       [(0, 1, F32(0.3), F32(0.6)), (0, 1, F32(0.1), F32(0.2))]))

    # the first sorted sample has weight 0: p = 1 leaves an empty-weight child, 0 / 0, which never wins; p = 2 does
    out.append(_design("zero_weight_child", [[0.1], [0.2], [0.3]], [0, 0, 1], [0, 5, 5], [[0, 1, 2]], [(0, 2, F32(0.2), F32(0.3))]))
    # ... and when that is the only candidate the node has no split
    out.append(_design("zero_weight_only", [[0.1], [0.2]], [0, 1], [0, 5], [[0, 1]], [None]))

    # several workgroup steps and more than one wave: 700 samples in three nodes with duplicates (values on a grid of 64)
    n = 700
    Y = rng.integers(0, 2, n)
    X = (rng.integers(0, 64, (n, 5)) / 64.0).astype(np.float32)
    X[:, 3] = np.where(Y == 0, X[:, 3] * 0.5, 0.5 + X[:, 3] * 0.5).astype(np.float32) * (rng.random(n) < 0.9) + X[:, 3] * (rng.random(n) >= 0.9)
    perm = rng.permutation(n)
    d = _design("three_nodes", X, Y, rng.integers(1, 1 << 40, n), [np.sort(perm[:300]), np.sort(perm[300:301 + 256]), np.sort(perm[557:])],
                [None, None, None], min_leaf=2)
    d["expect"] = [exact_winner(d, k) for k in range(3)]
    out.append(d)

    # an exact tie the workgroup reduction has to break: two nodes of 300 and 200 samples, columns 10, 200 and 290 count
    # 0, 1, 2, ... within each node, class 1 (weight 7) sits on a node's first and last sample, class 0 (weight 3) between.
    # p = 1 and p = n - 1 mirror L and R -- the same two float64 terms, added in the other order -- so six candidates per
    # node share the best proxy: in the scan the rival position lies in another 256-position step (n = 300) or in wave 3 of
    # the same step (n = 200), in the pick the rival features lie in wave 3 (200) and in the second turn of the strided
    # feature loop (290).  Column 100 varies too and is worse; every other column is constant.
    sizes, F = (300, 200), 300
    within = np.concatenate([np.arange(n) for n in sizes])
    X = np.full((within.size, F), 0.5, np.float32)
    X[:, [10, 200, 290]] = within[:, None]
    X[:, 100] = np.concatenate([(np.arange(n) * 7 + 3) % n for n in sizes])          # (7 is coprime to both sizes)
    Y = np.concatenate([np.r_[1, np.zeros(n - 2, np.int64), 1] for n in sizes])
    out.append(_design("tie_across_waves_steps_features", X, Y, np.where(Y == 1, 7, 3), [np.arange(300), np.arange(300, 500)],
                       [(10, 1, F32(0.0), F32(1.0))] * 2))
    return out


def level_order(d):
    """(order (F, N) int32, begin, end): every column sorted within each node's segment, the nodes one after the other
    (samples outside every node fill the tail)."""
    X = d["X"]
    N, F = X.shape
    rest = np.setdiff1d(np.arange(N), np.concatenate(d["nodes"]))
    order = np.empty((F, N), np.int32)
    begin, end, at = [], [], 0
    for S in d["nodes"]:
        begin.append(at)
        at += S.size
        end.append(at)
    for f in range(F):
        order[f] = np.concatenate([sorted_node(X, S, f) for S in d["nodes"]] + [rest])
    return order, np.array(begin, np.int32), np.array(end, np.int32)
