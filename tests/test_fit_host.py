"""CPU tests of the training side: the NumPy yardstick of fpga.DTree.fit against the reference's trees, the host
arithmetic of the stage learner (rejection threshold, schedule, banks, weights, loss, Learner bookkeeping) against
values the reference computed (tests/golden/fit_trees.npz), and the resource metadata of the split-search kernels."""
import logging
import pickle
from functools import partial

import numpy as np
import pytest

import fit_reference as fr
import waldboost_amd as wb
import tree_fixture
from test_host import _kernel_scratch_sizes
from waldboost_amd import _native as nat
from waldboost_amd import fpga, training

assert_tree_equal, case = tree_fixture.assert_tree_equal, tree_fixture.fit_case
case_names, fixture = partial(tree_fixture.case_names, "fit"), partial(tree_fixture.fixture, "fit")


@pytest.mark.parametrize("name", case_names())
def test_numpy_yardstick_reproduces_every_reference_tree(name):
    X0, W0, X1, W1, kw, want = case(name)
    tree, nodes = fr.fit(X0, W0, X1, W1, **kw)
    assert_tree_equal(tree, want, name)
    # the fixture's promise: every split that has a metric leads by at least 1e-8
    gaps = np.array([n.get("gap", np.nan) for n in nodes])
    assert np.array_equal(np.isnan(gaps), np.isnan(want["gap"]))
    assert np.all(gaps[~np.isnan(gaps)] >= 1e-8)


def test_fixture_holds_the_designed_cases():
    """Pure children answer (A[0], xmin), a constant first feature leaves an empty child, small children become leaves,
    a duplicated column resolves to the lower index, and neither class of the odd case counts a multiple of 64."""
    X0, W0, X1, W1, kw, want = case("pure_d2")
    assert want["feature"][0].tolist() == [0, 0, 0] and np.isnan(want["gap"][1]) and np.isnan(want["gap"][2])
    f = X0.reshape(X0.shape[0], -1)[:, 0]
    left0 = f[f <= want["threshold"][0]]
    assert want["feature"][1].tolist() == [0, 0, 0] and want["threshold"][1] == left0.min()
    X0, W0, X1, W1, kw, want = case("pure_empty")
    _, nodes = fr.fit(X0, W0, X1, W1, **kw)
    assert any(n["samples"].size == 0 for n in nodes) and want["feature"][1].tolist() == [0, 1, 0]      # flat index 2
    X0, W0, X1, W1, kw, want = case("odd_small_child")
    _, nodes = fr.fit(X0, W0, X1, W1, **kw)
    assert any(0 < n["samples"].size < kw["min_samples_leaf"] and n["depth"] < kw["max_depth"] for n in nodes)
    assert X0.shape[0] % 64 and X1.shape[0] % 64
    X0, W0, X1, W1, kw, want = case("const_dup_d2")
    F = np.concatenate([X0, X1]).reshape(X0.shape[0] + X1.shape[0], -1)
    assert np.all(F[:, 3] == 0) and np.all(F[:, 8] == 255) and np.array_equal(F[:, 5], F[:, 40])
    assert want["feature"][0].tolist() == list(np.unravel_index(5, X0.shape[1:]))
    X0, W0, X1, W1, kw, want = case("wide_d2")
    assert min(W0.min(), W1.min()) <= 1e-29 and max(W0.max(), W1.max()) == 1.0


@pytest.mark.parametrize("name", ["normal", "normal_f32", "separated", "two_values", "no_ratio"])
def test_fit_rejection_threshold_equals_the_reference(name, caplog):
    z = fixture()
    H0, H1 = z[f"theta/{name}/H0"], z[f"theta/{name}/H1"]
    P0, P1, alpha = z[f"theta/{name}/args"]
    with caplog.at_level(15, logger="waldboost_amd.training"):
        theta = training.fit_rejection_threshold(H0, P0, H1, P1, alpha)
    want = z[f"theta/{name}/theta"]
    assert np.float64(theta) == want
    if name.startswith("normal"):
        assert np.isfinite(theta) and type(theta) == H0.dtype.type
        # the reference's loop, for the vectorised form to be held against
        ts = np.unique(np.concatenate([H0, H1]))[1:]
        R = np.array([(P0 * ((H0 < t).sum() / H0.size) + (1 - P0) + 1e-6) / (P1 * ((H1 < t).sum() / H1.size) + (1 - P1) + 1e-6)
                      for t in ts]).astype(ts.dtype)
        assert theta == ts[np.flatnonzero(R > 1 / alpha).max()]
    elif name == "separated":
        assert theta == H1.min()
    else:
        assert theta == -np.inf
    assert caplog.records and all(r.levelno == 15 for r in caplog.records)
    expect = {"separated": "non-overlapping", "two_values": "Not enough unique", "no_ratio": "No suitable theta"}
    if name in expect:
        assert any(expect[name] in r.getMessage() for r in caplog.records)


def test_rejection_schedule_equals_the_reference():
    z = fixture()
    for row, want in zip(z["schedule/ctor"], z["schedule/result"]):
        s0, s1, target, is_none = row
        iv = None if is_none else (None if np.isnan(s0) else int(s0), None if np.isnan(s1) else int(s1))
        S = training.BasicRejectionSchedule(iv, target)
        for (stage, p0), w in zip(z["schedule/probe"], want):
            got = S(int(stage), p0)
            assert (got is None and np.isnan(w)) or got == w
    assert training.BasicRejectionSchedule()(0, 1.0) is None and training.BasicRejectionSchedule()(3, 1e-6) == -np.inf


def test_pixel_banks_and_scheduler_equal_the_reference():
    z = fixture()
    for shape, block in (((6, 6, 2), (2, 2)), ((5, 7), (2, 3)), ((8, 8, 4), (2, 2))):
        tag = "x".join(map(str, shape)) + "_" + "x".join(map(str, block))
        B = fpga.PixelBanks(shape, block)
        assert np.array_equal(B.pattern, z[f"banks/{tag}/pattern"]) and B.pattern.shape == z[f"banks/{tag}/pattern"].shape
        assert np.array_equal(B.bank_pixels([1]), z[f"banks/{tag}/pixels"])
        assert np.array_equal(B.bank_pixels([int(np.prod(block)) - 1, 0]), z[f"banks/{tag}/pixels2"])
    S = fpga.BankScheduler(4)
    assert np.array_equal(np.array([S.schedule(2), S.schedule(2), S.schedule(2)]), z["banks/schedule"])
    S = fpga.BankScheduler()
    assert np.array_equal(np.array([S.schedule(3), S.schedule(3), S.schedule(3)]), z["banks/schedule_default"])


def test_weights_loss_and_as_features_equal_the_reference():
    z = fixture()
    for h, w in (("weights/H", "weights/W"), ("weights/H32", "weights/W32")):
        got = training.weights(z[h])
        assert got.dtype == z[w].dtype and np.array_equal(got, z[w])
    assert np.float64(training.loss(z["loss/H0"], z["loss/H1"])) == z["loss/value"]
    X = np.arange(2 * 3 * 4 * 5, dtype=np.uint8).reshape(2, 3, 4, 5)
    assert np.array_equal(training.as_features(X), X.reshape(2, 60))


def test_learner_bookkeeping_and_pickle_round_trip(tmp_path):
    L = training.Learner(alpha=0.2, wh=fpga.DTree, max_depth=2, clip=2)
    assert len(L) == 0 and bool(L) and L.loss is None and L.false_positive_rate == 1.0 and L.true_positive_rate == 1.0
    L.p0, L.p1, L.losses = [0.5, 0.25], [1.0, 0.9], [0.4, 0.3]
    assert len(L) == 2 and L.loss == 0.3 and L.false_positive_rate == 0.125 and L.true_positive_rate == 0.9
    st = L.get_stats()
    assert np.array_equal(st["false_positive_rate"], [0.5, 0.125]) and np.array_equal(st["loss"], [0.4, 0.3])
    path = str(tmp_path / "learner.pkl")
    L.save(path)
    K = training.Learner.load(path)
    assert K.wh is fpga.DTree and K.alpha == 0.2 and K.wh_args == dict(max_depth=2, clip=2)
    assert K.p0 == L.p0 and K.p1 == L.p1 and K.losses == L.losses
    assert pickle.load(open(path, "rb")).keys() == {"alpha", "wh", "wh_args", "p0", "p1", "losses"}
    with pytest.raises(ValueError):
        training.Learner.from_dict(dict(alpha=0.1, wh=fpga.DTree, wh_args={}, p0=[0.5], p1=[], losses=[0.1]))
    # the default weak learner stays the sklearn one, which has no kernel here; the package re-exports as the reference does
    assert training.Learner().wh is training.DTree and fpga.Learner is training.Learner
    assert fpga.BasicRejectionSchedule is training.BasicRejectionSchedule
    with pytest.raises(NotImplementedError):
        training.DTree.fit(None, None, None, None)


def test_fit_argument_errors_need_no_gpu():
    X = np.zeros((4, 2, 2, 1), np.uint8)
    W = np.ones(4)
    with pytest.raises(NotImplementedError):
        fpga.DTree.fit(X.astype(np.float32), W, X, W)
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, np.ones(3), X, W)
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, np.array([1.0, np.nan, 1.0, 1.0]), X, W)
    with pytest.raises(ValueError):
        fpga.DTree.fit(X, W, X, -W)
    with pytest.raises(NotImplementedError):
        fpga.DTree.fit(X, W, X, W, max_depth=9)
    with pytest.raises(ValueError):
        fpga.train(wb.Model((8, 8, 4), {}), [], learner=training.Learner())        # wh must be fpga.DTree


def test_split_search_kernels_use_no_scratch_memory_and_exports_are_declared():
    nat.load()
    sizes = _kernel_scratch_sizes(open(nat.LIB_PATH, "rb").read())
    fit = {k: v for k, v in sizes.items() if "fit_hist_kernel" in k or "fit_pick_kernel" in k or "fit_route_kernel" in k}
    assert len(fit) == 3, sorted(fit)
    assert set(fit.values()) == {0}, fit
    assert not any("cascade" in k for k in fit)
    for name in ("wb_fit_scratch_bytes", "wb_fit_level_launch", "wb_fit_route_launch"):
        assert name in nat.SYMBOLS
    assert nat.WB_ABI_VERSION == 8 and nat.FIT_SPLIT_DTYPE.itemsize == 32


def test_fit_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    lib = nat.load()
    n = C.c_size_t()
    assert lib.wb_fit_scratch_bytes(72, 4, C.byref(n)) == 0 and n.value >= 72 * 4 * 12 + 4 * 16
    assert lib.wb_fit_scratch_bytes(72, 9, C.byref(n)) == nat.WB_ERR_INVALID
    slot = np.array([0, -1], np.int8)
    p = slot.ctypes.data_as(C.c_void_p)
    # null device pointers and malformed levels are refused before any HIP call
    assert lib.wb_fit_level_launch(None, None, 10, 4, None, None, None, 1, 2, p, 1, None, 4, None, 0, None) == nat.WB_ERR_INVALID
    assert lib.wb_fit_level_launch(None, None, 10, 4, None, None, None, 1, 2, p, 2, None, 4, None, 0, None) == nat.WB_ERR_INVALID
    assert b"slot" in lib.wb_last_error()
    assert lib.wb_fit_route_launch(None, None, 10, 4, None, 1, 2, p, 1, None, 3) == nat.WB_ERR_INVALID
