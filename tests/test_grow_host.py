"""CPU tests of the host half of both tree learners -- the growth loop (waldboost_amd/_grow.py) with each learner's leaf
rules, child numbering, final numbering, prediction expressions and clip / quantise -- with the level search, the only
step that needs the GPU, replaced by a NumPy stand-in built from the statements (tests/cart_reference.py,
tests/fit_reference.py).  Every golden tree (tests/golden/cart_trees.npz, fit_trees.npz) must come out bit for bit and
node by node; two scripted searches hold the numbering where a correct search does not lead."""
import numpy as np
import pytest

import cart_reference as cr
import fit_reference as fr
import tree_fixture
from waldboost_amd import _native as nat
from waldboost_amd import training
from waldboost_amd.fpga import training as fpga_training


def cart_search(X0, X1, F, Y, q, scale, min_leaf):
    """training._level_search from the statement's proxy_table, pick and threshold_of."""
    X = np.concatenate([np.asarray(X0).reshape(-1, F), np.asarray(X1).reshape(-1, F)]).astype(np.float32)
    where = np.zeros(Y.size, np.int32)

    def search(depth, level, opened, child_base):
        rec = np.zeros(len(opened), nat.CART_SPLIT_DTYPE)
        for j, nd in enumerate(opened):
            S = nd["samples"]
            table, xs = cr.proxy_table(X, Y, q, S, scale, min_leaf)
            win = cr.pick(table)
            rec[j]["t0"], rec[j]["t1"] = float(nd["T0"]) * scale, float(nd["T1"]) * scale
            rec[j]["feature"], rec[j]["proxy"] = -1, -np.inf
            if win is not None:
                f, p = win
                lo, hi = xs[p - 1, f], xs[p, f]
                right = ~(X[S, f].astype(np.float64) <= cr.threshold_of(lo, hi))
                where[S] = child_base + 2 * j + right
                rec[j]["feature"], rec[j]["n_left"], rec[j]["lo"], rec[j]["hi"], rec[j]["proxy"] = f, p, lo, hi, table[p - 1, f]
        return rec, where.copy()
    return search


def fit_search(X0, X1, F, Y, q, allowed):
    """fpga.training._level_search from the statement's metric_table and best_split."""
    X = np.concatenate([np.asarray(X0).reshape(-1, F), np.asarray(X1).reshape(-1, F)])
    w = np.ldexp(q.astype(np.float64), -62)
    where = np.zeros(Y.size, np.int32)

    def search(depth, level, opened, child_base):
        rec = np.zeros(len(opened), nat.FIT_SPLIT_DTYPE)
        slot = fpga_training._slots(level, opened)
        assert [level[j]["id"] for j in np.flatnonzero(slot >= 0)] == [nd["id"] for nd in opened]
        for j, nd in enumerate(opened):
            S, A = nd["samples"], allowed[depth]
            k, t, m = fr.best_split(fr.metric_table(X, Y, w, S, A))
            where[S] = child_base + 2 * j + ~(X[S, A[k]] <= t)
            rec[j]["feature"], rec[j]["threshold"], rec[j]["metric"] = A[k], t, m
            rec[j]["t0"], rec[j]["t1"] = w[S][Y[S] == 0].sum(), w[S][Y[S] == 1].sum()
        return rec, where.copy()
    return search


def assert_nodes_equal(info, nodes):
    assert len(info["samples"]) == len(nodes)
    for i, n in enumerate(nodes):
        assert np.array_equal(info["samples"][i], n["samples"]) and info["depth"][i] == n["depth"], i


@pytest.mark.parametrize("name", tree_fixture.case_names("cart"))
def test_cart_host_half_gives_every_reference_tree(name, monkeypatch):
    monkeypatch.setattr(training, "_level_search", cart_search)
    X0, W0, X1, W1, kw, want = tree_fixture.cart_case(name)
    tree, info = training.fit_detail(X0, W0, X1, W1, **kw)
    tree_fixture.assert_tree_equal(tree, want, name)
    stated, nodes = cr.fit(X0, W0, X1, W1, **kw)
    assert_nodes_equal(info, nodes)
    assert info["T0"] == [n["T0"] for n in nodes] and info["flat_feature"].tolist() == [n["feature"] for n in nodes]
    assert info["searched"].tolist() == ["table" in n for n in nodes]


@pytest.mark.parametrize("name", tree_fixture.case_names("fit"))
def test_fit_host_half_gives_every_reference_tree(name, monkeypatch):
    monkeypatch.setattr(fpga_training, "_level_search", fit_search)
    X0, W0, X1, W1, kw, want = tree_fixture.fit_case(name)
    tree, info = fpga_training.fit_detail(X0, W0, X1, W1, **kw)
    tree_fixture.assert_tree_equal(tree, want, name)
    stated, nodes = fr.fit(X0, W0, X1, W1, **kw)
    assert_nodes_equal(info, nodes)
    assert info["flat_feature"].tolist() == [n["feature"] for n in nodes]


def scripted(dtype, script, seen):
    """A search that splits every open node by the script: with m = script[node id], every m-th of the node's samples goes
    right (so both classes reach both children); None is a CART node without a candidate."""
    def factory(X0, X1, F, Y, q, *rest):
        where = np.zeros(Y.size, np.int32)

        def search(depth, level, opened, child_base):
            seen.append(([nd["id"] for nd in level], [nd["id"] for nd in opened], child_base))
            rec = np.zeros(len(opened), dtype)
            for j, nd in enumerate(opened):
                m = script[nd["id"]]
                rec[j]["feature"] = -1 if m is None else 0
                if m is not None:
                    right = np.arange(nd["samples"].size) % m == m - 1
                    where[nd["samples"]] = child_base + 2 * j + right
                    if "n_left" in dtype.names:
                        rec[j]["n_left"], rec[j]["lo"], rec[j]["hi"] = (~right).sum(), 1.0, 2.0
            return rec, where.copy()
        return search
    return factory


@pytest.mark.parametrize("stuck", [1, 2])
def test_cart_preorder_survives_a_hole_in_the_level_order_ids(stuck, monkeypatch):
    """One child of the root has no candidate (feature -1) while its sibling splits: the sibling's children keep the ids
    their slot gives them, so the level-order ids have a hole (3, 4 or 5, 6 are never made) and the depth below still
    has to find its nodes."""
    script = {0: 2, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 2, stuck: None}
    seen = []
    monkeypatch.setattr(training, "_level_search", scripted(nat.CART_SPLIT_DTYPE, script, seen))
    X = np.arange(40 * 4, dtype=np.float32).reshape(40, 2, 2, 1)
    tree, info = training.fit_detail(X[:20], np.ones(20), X[20:], np.ones(20), max_depth=3)
    kids = [5, 6] if stuck == 1 else [3, 4]
    assert seen == [([0], [0], 1), ([1, 2], [1, 2], 3), (kids, kids, 7)]
    want_left = [1, -1, 3, 4, -1, -1, 7, -1, -1] if stuck == 1 else [1, 2, 3, -1, -1, 6, -1, -1, -1]
    want_right = [2, -1, 6, 5, -1, -1, 8, -1, -1] if stuck == 1 else [8, 5, 4, -1, -1, 7, -1, -1, -1]
    assert tree.left.tolist() == want_left and tree.right.tolist() == want_right
    for i, (l, r) in enumerate(zip(tree.left, tree.right)):
        assert (l, r) == (-1, -1) or (l == i + 1 and r > l)                          # parent < left < right, left follows
        if l >= 0:
            S = info["samples"][i]
            assert np.array_equal(np.sort(np.concatenate([info["samples"][l], info["samples"][r]])), S)
            assert info["samples"][l].size == info["n_left"][i] and info["depth"][l] == info["depth"][r] == info["depth"][i] + 1
    stuck_at = 1 if stuck == 1 else 8                                                 # (pre-order index of the stuck node)
    assert info["searched"][stuck_at] and info["flat_feature"][stuck_at] == -1 and info["samples"][stuck_at].size == 20
    assert np.array_equal(tree.threshold == -2, tree.left < 0) and set(tree.threshold[tree.left >= 0]) == {1.5}


def test_fit_children_are_numbered_by_slot_not_by_position_in_the_level(monkeypatch):
    """Level 2 holds open, leaf, open, leaf (nodes 4 and 6 are below min_samples_leaf): the children of node 5, slot 1, are
    9 and 10 -- by its position in the level they would be 11 and 12."""
    script = {0: 2, 1: 3, 2: 3, 3: 2, 5: 2}
    seen = []
    monkeypatch.setattr(fpga_training, "_level_search", scripted(nat.FIT_SPLIT_DTYPE, script, seen))
    X = np.zeros((40, 2, 2, 1), np.uint8)
    tree, info = fpga_training.fit_detail(X[:25], np.ones(25), X[25:], np.ones(15), max_depth=3, min_samples_leaf=10)
    assert seen == [([0], [0], 1), ([1, 2], [1, 2], 3), ([3, 4, 5, 6], [3, 5], 7)]
    level, opened = ([dict(id=i) for i in ids] for ids in seen[2][:2])
    assert fpga_training._slots(level, opened).tolist() == [0, -1, 1, -1]
    assert tree.left.tolist() == [1, 3, 5, 7, -1, 9, -1, -1, -1, -1, -1] and tree.right.tolist() == [2, 4, 6, 8, -1, 10, -1, -1, -1, -1, -1]
    assert [s.size for s in info["samples"]] == [40, 20, 20, 14, 6, 14, 6, 7, 7, 7, 7]
    assert np.array_equal(np.sort(np.concatenate([info["samples"][9], info["samples"][10]])), info["samples"][5])
    assert info["depth"].tolist() == [0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3]
    assert np.array_equal(tree.threshold == -1, tree.left < 0)
