"""CPU tests of the CART designs (tests/cart_designs.py): every planted winner is the one exact rational arithmetic
gives and the one the float64 statement gives, and emulated kernels that get one rule wrong answer differently on the
design made for that rule -- so the GPU tests on the same designs can tell such a kernel from a right one."""
import numpy as np
import pytest

import cart_designs as cd
import cart_reference as cr
from tree_fixture import cart_case as case

DESIGNS = {d["name"]: d for d in cd.designs()}


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a[0] == b[0] and a[1] == b[1] and np.float32(a[2]) == np.float32(b[2]) and np.float32(a[3]) == np.float32(b[3])


@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_planted_winner_is_the_exact_and_the_stated_one(name):
    d = DESIGNS[name]
    for k in range(len(d["nodes"])):
        exact = cd.exact_winner(d, k)
        stated = cd.statement_winner(d, k)
        assert same(exact, d["expect"][k]), (name, k, exact, d["expect"][k])
        assert same(stated, exact), (name, k, stated, exact)
        if exact is not None:
            # the split the threshold makes is the split the position names
            f, p, lo, hi = exact
            thr = cr.threshold_of(lo, hi)
            assert np.float64(lo) <= thr < np.float64(hi)
            assert int((d["X"][d["nodes"][k], f].astype(np.float64) <= thr).sum()) == p
            # emulations with every rule right agree
            assert same(cd.emulated_winner(d, k), exact)


def test_designs_cover_what_they_are_named_for():
    d = DESIGNS["duplicated_columns"]
    table, _ = cr.proxy_table(d["X"], d["Y"], d["q"], d["nodes"][0], 1.0, 1)
    best = table.max()
    assert np.flatnonzero(table.max(axis=0) == best).tolist() == [2, 4, 5]          # three columns tie exactly
    assert best == float(sum(int(v) for v in d["q"]))                                # a pure split: T0 + T1
    assert not np.array_equal(d["X"][:, 5], d["X"][:, 2])
    d = DESIGNS["equal_positions"]
    table, _ = cr.proxy_table(d["X"], d["Y"], d["q"], d["nodes"][0], 1.0, 1)
    assert table[0, 0] == table[1, 0] == 8.0
    d = DESIGNS["chain_only"]
    x = d["X"][:, 0]
    assert np.all(np.diff(x.astype(np.float64)) > 1e-7) and x[-1] - x[0] > 4e-7     # every step exceeds 1e-7 in float64 ...
    assert np.all(x[1:] == x[:-1] + np.float32(1e-7))                               # ... and equals it after the float32 add
    d = DESIGNS["signed_zero"]
    assert np.signbit(d["X"][:, 0]).any() and (~np.signbit(d["X"][d["X"][:, 0] == 0, 0])).any()
    d = DESIGNS["zero_weight_child"]
    with np.errstate(all="ignore"):
        assert np.isnan(cr.half_proxy(np.float64(0.0), np.float64(0.0)))
    assert cd.exact_winner(DESIGNS["zero_weight_only"], 0) is None
    d = DESIGNS["three_nodes"]
    assert [s.size for s in d["nodes"]] == [300, 257, 143] and all(e is not None for e in d["expect"])
    for name in ("min_leaf_left", "min_leaf_right"):
        d = DESIGNS[name]
        f, p, lo, hi = d["expect"][0]
        assert p == d["min_leaf"] or d["nodes"][0].size - p == d["min_leaf"]
        free = dict(d, min_leaf=1)
        assert cd.exact_winner(free, 0)[1] in (2, 8)                                  # without the limit the pure split wins


def test_a_reduction_that_breaks_ties_the_other_way_shows():
    d = DESIGNS["tie_across_waves_steps_features"]
    for k, n in enumerate((300, 200)):
        table, _ = cr.proxy_table(d["X"], d["Y"], d["q"], d["nodes"][k], 1.0, 1)
        best = table.max()
        p, f = np.nonzero(table == best)                                                # (row p - 1 of the table is position p)
        assert sorted(zip((p + 1).tolist(), f.tolist())) == [(1, 10), (1, 200), (1, 290), (n - 1, 10), (n - 1, 200), (n - 1, 290)]
        assert n - 1 >= 256 or (n - 1) // 64 == 3                                     # another step, or wave 3 of the same one
        assert table[:, 100].max() < best and np.isfinite(table[:, 100].max())          # an ordinary column, worse
        assert np.flatnonzero(np.isfinite(table).any(axis=0)).tolist() == [10, 100, 200, 290]
        assert same(cd.emulated_winner(d, k), d["expect"][k])
        assert cd.emulated_winner(d, k, last_p=True)[:2] == (10, n - 1)
        assert cd.emulated_winner(d, k, last_f=True)[:2] == (290, 1)
    table, _ = cr.proxy_table(d["X"], d["Y"], d["q"], d["nodes"][0], 1.0, 1)
    assert abs(table.max() - 894.108768035516) < 1e-9 and np.sort(table[:, 10])[-3] < 890


def test_a_wrong_comparison_in_the_step_rule_shows():
    d = DESIGNS["exact_step"]
    assert cd.emulated_winner(d, 0, ge=True)[0] == 0 and d["expect"][0][0] == 1
    d = DESIGNS["chain_float32_add"]
    assert cd.emulated_winner(d, 0, f64_add=True)[0] == 0 and d["expect"][0][0] == 1
    assert cd.emulated_winner(DESIGNS["chain_only"], 0, f64_add=True) is not None


def test_a_predecessor_taken_from_the_whole_column_shows():
    d = DESIGNS["per_node_predecessor"]
    assert cd.emulated_winner(d, 0, global_pred=True) is None and d["expect"][0] is not None
    assert same(cd.emulated_winner(d, 1, global_pred=True), d["expect"][1])


def test_a_float32_threshold_shows():
    d = DESIGNS["midpoint_rounds"]
    f, p, lo, hi = d["expect"][0]
    wrong = np.float32(lo) / np.float32(2.0) + np.float32(hi) / np.float32(2.0)
    assert wrong == hi                                                                 # rounds to even: onto xs[p]
    assert int((d["X"][:, f] <= wrong).sum()) == 4 != p
    thr = cr.threshold_of(lo, hi)
    assert np.float64(lo) < thr < np.float64(hi) and np.float32(thr) in (lo, hi)       # no float32 lies between


def test_order_dependent_float_sums_show():
    """Duplicated values with weights over many orders of magnitude: float64 running sums depend on the order in which
    equal values arrive, the integer sums of the statement do not."""
    rng = np.random.default_rng(5)
    n = 400
    X = (rng.integers(0, 8, (n, 1)) / 8.0).astype(np.float32)
    Y = rng.integers(0, 2, n)
    W = 10.0 ** rng.uniform(-16, 0, n)
    S = np.arange(n)
    P = rng.permutation(n)
    a, b = cd.float_sum_proxies(X, Y, W, S, 0), cd.float_sum_proxies(X, Y, W, P, 0)
    steps = np.flatnonzero(np.diff(np.sort(X[:, 0])) > 0)                             # the candidates: the same in any order
    assert np.any(a[steps] != b[steps])
    q, k = cr.split_weights(W, Y)
    ta, _ = cr.proxy_table(X, Y, q, S, 2.0 ** -k, 1)
    tb, _ = cr.proxy_table(X, Y, q, P, 2.0 ** -k, 1)
    assert np.array_equal(ta, tb)


def test_breadth_first_numbering_shows():
    X0, W0, X1, W1, kw, want = case("pure_d3")
    tree, nodes = cr.fit(X0, W0, X1, W1, **kw)
    order, todo = [], [0]
    while todo:                                                                         # breadth first
        n = todo.pop(0)
        order.append(n)
        if nodes[n]["left"] >= 0:
            todo += [nodes[n]["left"], nodes[n]["right"]]
    index = {n: i for i, n in enumerate(order)}
    left = [index.get(nodes[n]["left"], -1) for n in order]
    assert left != want["left"].tolist() and np.array_equal(tree.left, want["left"])
