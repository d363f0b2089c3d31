"""GPU tests of the training side: fpga.DTree.fit (csrc/wb_fit.hip) against the reference's trees
(tests/golden/fit_trees.npz) and against the NumPy yardstick (tests/fit_reference.py) node by node, its independence of
the sample order, Learner.fit_stage against the reference's values, and fpga.train end to end."""
import os
from functools import partial

import numpy as np
import pytest

import fit_designs as fd
import fit_reference as fr
import waldboost_amd as wb
import tree_fixture
from waldboost_amd import fpga, training
from waldboost_amd.fpga.training import fit_detail
from waldboost_amd.synth import synth_image

pytestmark = pytest.mark.gpu
assert_tree_equal, case = tree_fixture.assert_tree_equal, tree_fixture.fit_case
case_names, fixture = partial(tree_fixture.case_names, "fit"), partial(tree_fixture.fixture, "fit")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------ the reference's trees, exactly
@pytest.mark.parametrize("name", case_names())
def test_fit_equals_the_reference_tree(name):
    X0, W0, X1, W1, kw, want = case(name)
    assert_tree_equal(fpga.DTree.fit(X0, W0, X1, W1, **kw), want, name)


def test_fit_takes_device_tensors():
    import torch
    X0, W0, X1, W1, kw, want = case("base_d3")
    tree = fpga.DTree.fit(torch.from_numpy(X0).cuda(), W0, torch.from_numpy(X1).cuda(), W1, **kw)
    assert_tree_equal(tree, want)


# ------------------------------------------------------------------------------ random cases, every node
def _random_case(seed, n0, n1, shape, zero_share):
    rng = np.random.default_rng(seed)
    F = int(np.prod(shape))
    X0, X1 = rng.integers(0, 256, (n0, F)), rng.integers(0, 256, (n1, F))
    for f, d in ((3, 50), (F // 2, -35), (F - 1, 20)):
        X1[:, f] = np.clip(X1[:, f] + d, 0, 255)
    if zero_share:                                                     # mostly-zero columns, as grad_hist_4_u1 samples are
        X0[rng.random((n0, F)) < zero_share] = 0
        X1[rng.random((n1, F)) < zero_share] = 0
    W0, W1 = np.exp(rng.normal(0, 1, n0)), np.exp(rng.normal(0, 1, n1))
    return X0.astype(np.uint8).reshape((n0,) + shape), W0, X1.astype(np.uint8).reshape((n1,) + shape), W1


def _banks(shape, depth):
    B = fpga.PixelBanks(shape, (2, 2))
    return [B.bank_pixels(b) for b in fpga.BankScheduler(4).schedule(depth)]


RANDOM_CASES = {
    "n2000_d3": (dict(seed=11, n0=1200, n1=800, shape=(6, 6, 2), zero_share=0), dict(max_depth=3)),
    "zeros_d4": (dict(seed=12, n0=700, n1=650, shape=(8, 8, 4), zero_share=0.8), dict(max_depth=4, min_samples_leaf=20)),
    "banks_d2": (dict(seed=13, n0=150, n1=90, shape=(5, 7, 3), zero_share=0.3), dict(max_depth=2, min_samples_leaf=5, banks=True)),
    "raw_d1": (dict(seed=14, n0=257, n1=63, shape=(3, 3, 1), zero_share=0), dict(max_depth=1, clip=None, quantizer=None)),
}


@pytest.mark.parametrize("name", sorted(RANDOM_CASES))
def test_every_node_of_a_random_tree_holds_against_the_yardstick(name):
    """At every split node, on the node's sample set as the GPU routed it: the yardstick's metric of the GPU's (f, t) is
    within 1e-10 of the yardstick's maximum -- the two sides differ by float64 rounding of cumulative sums (at most
    N * 2^-53 * 0.5, 1e-13 at N = 2000), amplified by the entropy's slope near the 1e-4 regulariser (at most
    log2(1e4) = 13), plus a few ulp of log2: 1e-12 at the worst; 1e-10 is 100 times that -- and where (f, t) is the
    yardstick's argmax the node equals the yardstick's.  Children, leaf rule and predictions are exact at every node."""
    data, kw = RANDOM_CASES[name]
    kw = dict(kw)
    X0, W0, X1, W1 = _random_case(**data)
    shape = X0.shape[1:]
    if kw.pop("banks", False):
        kw["allowed_features"] = _banks(shape, kw["max_depth"])
    tree, info = fit_detail(X0, W0, X1, W1, **kw)
    F = int(np.prod(shape))
    X = np.concatenate([X0.reshape(-1, F), X1.reshape(-1, F)])
    Y = np.array([0] * X0.shape[0] + [1] * X1.shape[0])
    W = np.concatenate([W0, W1])
    w = fr.split_weights(W, Y)
    msl = kw.get("min_samples_leaf", 10)
    assert np.array_equal(info["samples"][0], np.arange(W.size))
    n_split = n_tied = 0
    for i in range(tree.left.size):
        S, depth = info["samples"][i], int(info["depth"][i])
        pred = fr.node_prediction(W, Y, S, kw.get("clip", 3), kw.get("quantizer", 32))
        assert bits(tree.prediction[i:i + 1])[0] == bits(np.array([pred], np.float32))[0], (i, tree.prediction[i], pred)
        is_leaf = depth == kw["max_depth"] or S.size < msl
        assert (tree.left[i] < 0) == is_leaf and (tree.right[i] < 0) == is_leaf
        if is_leaf:
            assert tree.threshold[i] == -1 and tree.feature[i].tolist() == [0, 0, 0]
            continue
        n_split += 1
        A = kw["allowed_features"][depth] if "allowed_features" in kw else np.arange(F)
        M = fr.metric_table(X, Y, w, S, A)
        f, t = int(info["flat_feature"][i]), int(tree.threshold[i])
        assert tree.feature[i].tolist() == list(np.unravel_index(f, shape)) and f in A
        k, t_best, m_best = fr.best_split(M)
        if np.isnan(m_best):
            assert (f, t) == (int(A[0]), int(X[S, A[0]].min())) and np.isnan(info["metric"][i])
        else:
            mine = M[np.flatnonzero(A == f), t].max()
            print(f"{name} node {i}: |S| {S.size} gpu ({f}, {t}) yardstick ({int(A[k])}, {t_best}) metric {mine:.17g} "
                  f"best {m_best:.17g} gpu's {info['metric'][i]:.17g} gap {fr.table_gap(M):.3g}")
            assert mine >= m_best - 1e-10
            assert abs(info["metric"][i] - mine) <= 1e-10
            if fr.table_gap(M) >= 1e-8:
                assert (f, t) == (int(A[k]), t_best)
                n_tied += int((M == m_best).sum() >= 2)           # ... where the yardstick's best was an exact tie
        goes_left = X[S, f] <= t
        assert np.array_equal(info["samples"][tree.left[i]], S[goes_left])
        assert np.array_equal(info["samples"][tree.right[i]], S[~goes_left])
        assert info["depth"][tree.left[i]] == info["depth"][tree.right[i]] == depth + 1
    assert n_split >= 1
    print(f"{name}: {n_tied} of {n_split} split nodes had an exact tie at the best and were held to the first argmax")
    if name == "banks_d2":                                  # 240 samples leave gaps in 0 .. 255: runs of thresholds tie
        assert n_tied >= 1
    # the whole tree against the yardstick's, when every split of it is clear
    ref_tree, nodes = fr.fit(X0, W0, X1, W1, **kw)
    gaps = np.array([n["gap"] for n in nodes if n["left"] >= 0])
    if np.all(np.isnan(gaps) | (gaps >= 1e-8)):
        assert_tree_equal(tree, {a: getattr(ref_tree, a) for a in ("feature", "threshold", "left", "right", "prediction")}, name)


# ------------------------------------------------------------------------------ a designed tree
def _designed_tree_case():
    """Depth 3 from the planted generator of tests/fit_designs.py: the root's column f* = 10 has a copy, feature 4, earlier
    in allowed_features[0]; class 0 keeps to the low side of t* and 25 class-1 samples stray there, so the root's right
    child is pure -- the NaN rule, (A[0], xmin) -- and is split again all the same.  Integer weights with a class total of
    2^17: the split weights and every sum of them are exact on both sides, so ties are ties."""
    rng = np.random.default_rng(21)
    shape, n0, n1, f_star, f_dup, t_star = (3, 3, 2), 150, 170, 10, 4, 120
    F = int(np.prod(shape))
    cls = np.array([0] * n0 + [1] * n1, np.uint8)
    X = fd._noise(rng, n0 + n1, F)
    col = fd._planted_values(rng, cls, t_star, flip=0.0)
    col[n0 + rng.permutation(n1)[:25]] = rng.integers(30, t_star - 29, 25)
    X[:, f_star] = X[:, f_dup] = col
    W = []
    for n in (n0, n1):
        k = rng.integers(256, 1024, n)
        rest = 2 ** 17 - int(k.sum())                           # a class total of 2^17: w' = W / 2^18 is exact
        k += rest // n
        k[:rest % n] += 1
        assert k.sum() == 2 ** 17 and k.min() > 0
        W.append(k.astype(np.float64))
    allowed = [np.array([13, 4, 2, 10, 7, 0, 16]), np.array([9, 1, 15, 3, 12]), np.array([17, 5, 11, 8, 6, 14])]
    kw = dict(max_depth=3, min_samples_leaf=10, allowed_features=allowed)
    return X[:n0].reshape((n0,) + shape), W[0], X[n0:].reshape((n1,) + shape), W[1], kw, (f_star, f_dup)


def test_designed_tree_with_a_feature_tie_and_a_pure_child():
    X0, W0, X1, W1, kw, (f_star, f_dup) = _designed_tree_case()
    tree, info = fit_detail(X0, W0, X1, W1, **kw)
    ref_tree, nodes = fr.fit(X0, W0, X1, W1, **kw)
    assert_tree_equal(tree, {a: getattr(ref_tree, a) for a in ("feature", "threshold", "left", "right", "prediction")})
    # the yardstick's tree is a fair judge: every rated split of it leads by a margin
    gaps = np.array([n["gap"] for n in nodes if n["left"] >= 0])
    assert np.all(np.isnan(gaps) | (gaps >= 1e-6)) and tree.depth() == 3
    # the cross-feature tie occurred: the copy's row of the root's table equals f*'s bit for bit, the best is in both and
    # in several thresholds of each, and the earlier entry of A and its first best threshold were taken
    root = nodes[0]
    A, M = root["A"].tolist(), root["table"]
    ka, kb = A.index(f_dup), A.index(f_star)
    tied = M == root["metric"]
    assert ka < kb and np.array_equal(M[ka].view(np.uint64), M[kb].view(np.uint64))
    assert tied[ka].sum() >= 2 and np.flatnonzero(tied.any(axis=1)).tolist() == [ka, kb]
    assert info["flat_feature"][0] == f_dup and tree.threshold[0] == np.flatnonzero(tied[ka])[0]
    # the pure child occurred: one class, at least min_samples_leaf samples, a NaN metric, (A[0], xmin), and children
    pure = int(tree.right[0])
    S = info["samples"][pure]
    assert S.size >= kw["min_samples_leaf"] and S.min() >= X0.shape[0] and info["depth"][pure] == 1
    assert np.isnan(info["metric"][pure]) and np.isnan(nodes[pure]["metric"]) and info["t0"][pure] == 0 and info["t1"][pure] > 0
    first = int(kw["allowed_features"][1][0])
    xs = np.concatenate([X0, X1]).reshape(-1, X0[0].size)[S, first]
    assert (int(info["flat_feature"][pure]), int(tree.threshold[pure])) == (first, int(xs.min()))
    assert tree.left[pure] > 0 and tree.right[pure] > 0
    assert np.array_equal(info["samples"][tree.left[pure]], S[xs == xs.min()])
    assert np.isfinite(info["metric"][tree.left[0]])                        # ... beside a rated node in the same launch


# ------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize("name", ["n2000_d3", "zeros_d4"])
def test_fit_does_not_depend_on_sample_order_or_run(name):
    data, kw = RANDOM_CASES[name]
    X0, W0, X1, W1 = _random_case(**data)
    tree, info = fit_detail(X0, W0, X1, W1, **kw)
    again, info2 = fit_detail(X0, W0, X1, W1, **kw)
    rng = np.random.default_rng(5)
    p0, p1 = rng.permutation(W0.size), rng.permutation(W1.size)
    perm, info3 = fit_detail(X0[p0], W0[p0], X1[p1], W1[p1], **kw)
    assert np.isfinite(info["metric"]).sum() >= 3
    for other, oinfo in ((again, info2), (perm, info3)):
        assert bytes(other.content()) == bytes(tree.content())
        for key in ("metric", "t0", "t1"):
            assert np.array_equal(bits(oinfo[key]), bits(info[key])), key
    # the same samples reach every node
    where = np.concatenate([p0, W0.size + p1])
    for a, b in zip(info["samples"], info3["samples"]):
        assert np.array_equal(a, np.sort(where[b]))


# ------------------------------------------------------------------------------ Learner.fit_stage
def test_learner_fit_stage_equals_the_reference():
    z = fixture()
    X0, W0, X1, W1, _, _ = case("base_d2")
    L = training.Learner(alpha=float(z["stage/alpha"]), wh=fpga.DTree, max_depth=2)
    M = wb.Model((6, 6, 2), {})
    for s in range(2):
        H0, H1 = z[f"stage/{s}/H0"], z[f"stage/{s}/H1"]
        loss, fpr, tpr = L.fit_stage(M, X0, H0, X1, H1, theta=None)
        assert len(M) == len(L) == s + 1
        assert_tree_equal(M.classifier[-1], {a: z[f"stage/{s}/{a}"] for a in ("feature", "threshold", "left", "right", "prediction")})
        theta = M.theta[-1]
        assert np.isfinite(theta)
        assert bits(np.array([theta], np.float32))[0] == bits(z[f"stage/{s}/theta"].astype(np.float32).reshape(1))[0]
        assert L.p0[-1] == z[f"stage/{s}/p0"] and L.p1[-1] == z[f"stage/{s}/p1"]
        assert loss == z[f"stage/{s}/loss"]
        assert fpr == z[f"stage/{s}/fpr"] and tpr == z[f"stage/{s}/tpr"]
        # the next stage's scores are the reference's
        if s == 0:
            assert np.array_equal(H0 + M.classifier[-1].predict(X0), z["stage/1/H0"])
            assert np.array_equal(H1 + M.classifier[-1].predict(X1), z["stage/1/H1"])


# ------------------------------------------------------------------------------ fpga.train end to end
def _training_images():
    items = []
    for seed in range(8):
        img = synth_image(128, 160, 100 + seed).astype(np.int32)
        rng = np.random.default_rng(seed)
        gt = []
        for size, x_lo in ((24, 4), (32, 84)):
            x, y = x_lo + int(rng.integers(0, 40)), 4 + int(rng.integers(0, 128 - size - 8))
            img[y:y + size, x:x + size] += 90
            gt.append([x, y, x + size, y + size])
        items.append(dict(image=np.clip(img, 0, 255).astype(np.uint8), groundtruth_boxes=wb.Boxes(np.array(gt, "f"))))
    return items


def test_fpga_train_end_to_end(tmp_path):
    np.random.seed(0)                                       # (select_candidates draws from np.random)
    items = _training_images()
    M = wb.Model((8, 8, 4), dict(shrink=2, n_per_oct=8, smooth=1, channels=fpga.grad_hist_4_u1))
    pool = wb.SamplePool(min_tp=40, min_fp=200, min_tp_iou=0.5, max_fp_iou=0.3)
    seen = []

    def capture(model, learner, stage):
        X0, H0 = pool.get_false_positives()
        X1, H1 = pool.get_true_positives()
        seen.append((stage, len(model), len(learner), X0, H0, X1, H1))

    L = fpga.train(M, items, pool=pool, length=4, max_depth=2, callbacks=[capture])
    assert len(M) == 4 and len(L) == 4 and L.wh is fpga.DTree and [s[0] for s in seen] == [0, 1, 2, 3]
    banks, sched = fpga.PixelBanks(M.shape, (2, 2)), fpga.BankScheduler(4)
    for (stage, n_model, n_learner, X0, H0, X1, H1), weak in zip(seen, M.classifier):
        assert n_model == n_learner == stage + 1 and X0.dtype == np.uint8 and X0.shape[0] > 0 and X1.shape[0] > 0
        ftrs = [banks.bank_pixels(b) for b in sched.schedule(2)]
        again = fpga.DTree.fit(X0, training.weights(H0), X1, training.weights(-H1), max_depth=2, allowed_features=ftrs)
        assert bytes(again.content()) == bytes(weak.content()), stage
        assert weak.depth() >= 1
    assert fpga.train(M, items, learner=L, pool=pool, length=4) is None        # long enough already
    path = str(tmp_path / "trained.pb")
    M.save(path)
    K = wb.load(path)
    assert len(K) == 4
    for it in items[:2]:
        a, b = M.detect_raw(it["image"]), K.detect_raw(it["image"])
        assert np.array_equal(a["boxes"], b["boxes"]) and np.array_equal(bits(a["scores"]), bits(b["scores"]))
        assert np.array_equal(a["level"], b["level"]) and a["scores"].size > 0


# ------------------------------------------------------------------------------ errors
def test_fit_errors():
    X = np.zeros((12, 2, 2, 1), np.uint8)
    W = np.ones(12)
    with pytest.raises(NotImplementedError):
        fpga.DTree.fit(X.astype(np.float32), W, X, W)
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, W[:5], X, W)
    bad = W.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, W, X, bad)
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, W, X, W, allowed_features=[np.array([0, 4])] * 2)       # feature 4 of 4
    # constant samples: every candidate ties, the first wins; weightless classes: every metric is NaN
    tree = fpga.DTree.fit(X, W, X, W, max_depth=1)
    assert tree.left.tolist() == [1, -1, -1] and tree.threshold[0] == 0 and tree.feature[0].tolist() == [0, 0, 0]
    tree = fpga.DTree.fit(X, np.zeros(12), X, W, max_depth=1)
    assert tree.left.tolist() == [1, -1, -1] and tree.threshold[0] == 0
