"""CPU tests of training.DTree.fit: the NumPy statement (tests/cart_reference.py) against the trees the reference's own
fit gave (tests/golden/cart_trees.npz), the argument and dtype errors, the package's exports and the resource metadata of
the CART kernels."""
from functools import partial

import numpy as np
import pytest

import cart_reference as cr
import waldboost_amd as wb
import tree_fixture
from test_host import _kernel_scratch_sizes
from waldboost_amd import _native as nat
from waldboost_amd import training

assert_tree_equal, case = tree_fixture.assert_tree_equal, tree_fixture.cart_case
case_names, fixture = partial(tree_fixture.case_names, "cart"), partial(tree_fixture.fixture, "cart")
KERNELS = ("cart_sort_kernel", "cart_scan_kernel", "cart_best_kernel", "cart_move_kernel", "cart_part_kernel")


@pytest.mark.parametrize("name", case_names())
def test_statement_reproduces_every_reference_tree(name):
    X0, W0, X1, W1, kw, want = case(name)
    tree, nodes = cr.fit(X0, W0, X1, W1, **kw)
    assert_tree_equal(tree, want, name)
    # the fixture's promise: every split leads by at least 1e-9 relative and is reached by one feature only
    splits = [n for n in nodes if n["left"] >= 0]
    assert all(n["gap"] >= 1e-9 and n["winners"] == 1 for n in splits)
    assert np.array_equal(np.isnan(want["gap"]), [n["left"] < 0 for n in nodes])
    # pre-order: a parent's index is below its children's, the left child follows its parent
    for i, n in enumerate(nodes):
        assert n["left"] in (-1, i + 1) and (n["left"] < 0) == (n["right"] < 0) and (n["right"] < 0 or n["right"] > n["left"])


def test_fixture_holds_the_designed_cases():
    z = fixture()
    names = case_names()
    assert {int(z[f"case/{n}/args"][0]) for n in names} == {1, 2, 3, 4}
    X0, W0, X1, W1, kw, want = case("u8_d2")
    assert X0.dtype == np.uint8 and X1.dtype == np.uint8
    assert case("base_d2")[0].dtype == np.float32 and case("base_d2")[0].shape[1:] == (6, 6, 2)
    # min_samples_leaf forbids the children of the root's children; min_samples_split stops nodes that may split otherwise
    X0, W0, X1, W1, kw, want = case("base_no_children")
    _, nodes = cr.fit(X0, W0, X1, W1, **kw)
    assert any(n["left"] < 0 and n["depth"] < kw["max_depth"] and kw["min_samples_leaf"] <= n["samples"].size < 2 * kw["min_samples_leaf"]
               for n in nodes)
    X0, W0, X1, W1, kw, want = case("base_split")
    _, nodes = cr.fit(X0, W0, X1, W1, **kw)
    assert any(n["left"] < 0 and n["depth"] < kw["max_depth"] and 2 * kw["min_samples_leaf"] <= n["samples"].size < kw["min_samples_split"]
               for n in nodes)
    # constant columns: 0, a value, and one that varies by less than 1e-7
    X0, W0, X1, W1, kw, want = case("const_d2")
    F = np.concatenate([X0, X1]).reshape(X0.shape[0] + X1.shape[0], -1)
    assert np.all(F[:, 3] == 0) and np.all(F[:, 8] == 0.75) and 0 < np.ptp(F[:, 5]) < 1e-7
    # a pure left child of the root while the right one goes on: left != breadth-first numbering
    X0, W0, X1, W1, kw, want = case("pure_d3")
    assert want["left"][1] == -1 and want["left"][2] > 0
    X0, W0, X1, W1, kw, want = case("sep_d3")
    assert want["left"].tolist() == [1, -1, -1]
    X0, W0, X1, W1, kw, want = case("wide_d2")
    assert min(W0.min(), W1.min()) <= 1e-29 and max(W0.max(), W1.max()) == 1.0
    X0, W0, X1, W1, kw, want = case("unequal_d2")
    assert X0.shape[0] > 30 * X1.shape[0]
    X0, W0, X1, W1, kw, want = case("tiny_d3")
    F = np.concatenate([X0, X1])
    assert (np.abs(F) < 1e-7).mean() > 0.4 and np.all(np.abs(F.reshape(F.shape[0], -1)[:, 11]) < 1e-7)
    X0, W0, X1, W1, kw, want = case("big_d3")
    assert X0.shape[0] + X1.shape[0] > 4096                   # above the sort's chunk
    assert X0.shape[0] % 64 and case("odd_d2")[0].shape[0] % 64


def test_integer_weights_keep_their_total_below_2_62():
    for W in (np.full(24000, 1e300), np.full(10, 1e-200), np.exp(np.random.default_rng(0).normal(0, 3, 777))):
        Y = (np.arange(W.size) % 3 == 0).astype(np.int64)
        q, k = cr.split_weights(W, Y)
        q2, k2 = training.cart_split_weights(W, Y)
        assert k == k2 and np.array_equal(q, q2)
        total = sum(int(v) for v in q)
        assert 2 ** 59 <= total < 2 ** 62


def test_fit_argument_errors_need_no_gpu():
    X = np.zeros((4, 2, 2, 1), np.float32)
    X[:2] = 1
    W = np.ones(4)
    fit = training.DTree.fit
    for bad in (None, [[1.0]], X.astype(np.float64), X.astype(np.int32), X.astype(np.float16)):
        with pytest.raises(NotImplementedError):
            fit(bad, W, X, W, max_depth=2)
        with pytest.raises(NotImplementedError):
            fit(X, W, bad, W, max_depth=2)
    with pytest.raises(NotImplementedError):
        fit(None, None, None, None)
    with pytest.raises(NotImplementedError, match=r"Learner\(max_depth=2\)"):
        fit(X, W, X, W)
    for kw in (dict(max_depth=None), dict(max_depth=5), dict(max_depth=0), dict(max_depth=2.0), dict(max_depth=2, min_samples_leaf=0.1),
               dict(max_depth=2, min_samples_split=0.5), dict(max_depth=2, max_features=3), dict(max_depth=2, criterion="entropy"),
               dict(max_depth=2, splitter="random"), dict(max_depth=2, class_weight=None)):
        with pytest.raises(NotImplementedError):
            fit(X, W, X, W, **kw)
    with pytest.raises(ValueError):
        fit(X, W, X, W, max_depth=2, min_samples_leaf=0)
    with pytest.raises(ValueError):
        fit(X, W, X, W, max_depth=2, min_samples_split=1)
    with pytest.raises(ValueError):
        fit(X, np.ones(3), X, W, max_depth=2)
    with pytest.raises(ValueError):
        fit(X, np.array([1.0, np.nan, 1.0, 1.0]), X, W, max_depth=2)
    with pytest.raises(ValueError):
        fit(X, W, X, -W, max_depth=2)
    with pytest.raises(ValueError):
        fit(X, W, X, np.zeros(4), max_depth=2)              # a class without weight
    with pytest.raises(ValueError):
        fit(X, W, X[:, :1], W, max_depth=2)
    Xn = X.copy()
    Xn[1, 0, 0, 0] = np.inf
    with pytest.raises(ValueError):
        fit(X, W, Xn, W, max_depth=2)
    Xn[1, 0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        fit(Xn, W, X, W, max_depth=2)
    big = np.zeros((nat.WB_CART_MAX_SAMPLES, 1, 1, 1), np.uint8)
    with pytest.raises(NotImplementedError, match="at most"):
        fit(big, np.ones(big.shape[0]), X[:, :1, :1], W, max_depth=1)
    # the accepted spellings get as far as the GPU
    if not __import__("torch").cuda.is_available():
        with pytest.raises(nat.NativeError):
            fit(X, W, X.astype(np.uint8), W, max_depth=2, criterion="gini", splitter="best", random_state=3, min_samples_leaf=1,
                min_samples_split=2)


def test_train_and_the_learner_are_exported():
    for name in ("train", "Learner", "BasicRejectionSchedule"):
        assert name in wb.__all__ and hasattr(wb, name)
    assert wb.Learner is training.Learner and wb.BasicRejectionSchedule is training.BasicRejectionSchedule
    assert not hasattr(wb, "train_softcascade")
    M = wb.Model((8, 8, 4), {})
    with pytest.raises(RuntimeError):
        L = training.Learner(max_depth=2)
        L.p0, L.p1, L.losses = [1.0], [1.0], [0.5]
        wb.train(M, [], learner=L, length=2)                  # the learner is one stage ahead of the model
    assert wb.train(M, [], length=0) is None
    assert "out of scope" not in (training.__doc__ + wb.__doc__)


def test_cart_kernels_use_no_scratch_memory_and_exports_are_declared():
    nat.load()
    sizes = _kernel_scratch_sizes(open(nat.LIB_PATH, "rb").read())
    cart = {k: v for k, v in sizes.items() if any(name in k for name in KERNELS)}
    assert len(cart) == len(KERNELS), sorted(cart)
    assert set(cart.values()) == {0}, cart
    assert not any(bad in k for k in cart for bad in ("cascade", "fit_hist_kernel", "fit_pick_kernel", "fit_route_kernel"))
    for name in ("wb_cart_sort_launch", "wb_cart_scratch_bytes", "wb_cart_level_launch"):
        assert name in nat.SYMBOLS
    assert nat.WB_ABI_VERSION == 8 and nat.CART_SPLIT_DTYPE.itemsize == 40


def test_cart_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    lib = nat.load()
    n = C.c_size_t()
    assert lib.wb_cart_scratch_bytes(72, 4, C.byref(n)) == 0 and n.value >= 72 * 4 * 20
    assert lib.wb_cart_scratch_bytes(72, 9, C.byref(n)) == nat.WB_ERR_INVALID
    assert lib.wb_cart_scratch_bytes(72, 4, None) == nat.WB_ERR_INVALID
    assert lib.wb_cart_sort_launch(None, None, 10, 4, None) == nat.WB_ERR_INVALID
    fake = C.c_void_p(4096)                                   # (never dereferenced: refused before any HIP call)
    assert lib.wb_cart_sort_launch(None, fake, nat.WB_CART_MAX_SAMPLES + 1, 4, fake) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_cart_sort_launch(None, fake, 0, 4, fake) == nat.WB_ERR_INVALID
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    t = np.array([5, 5], np.uint64)

    def level(begin, end, n_open=2, scale=1.0, min_leaf=1, dev=None, t0=t):
        b, e = np.array(begin, np.int32), np.array(end, np.int32)
        return lib.wb_cart_level_launch(None, dev, 10, 4, dev, dev, dev, dev, dev, n_open, hp(b), hp(e), hp(t0), hp(t), scale, min_leaf, 1,
                                        dev, 0, dev)
    assert level([0, 5], [5, 10]) == nat.WB_ERR_INVALID and b"null" in lib.wb_last_error()
    assert level([0, 4], [5, 10], dev=fake) == nat.WB_ERR_INVALID and b"overlaps" in lib.wb_last_error()
    assert level([0, 5], [5, 11], dev=fake) == nat.WB_ERR_INVALID and b"segment" in lib.wb_last_error()
    assert level([0, 5], [0, 10], dev=fake) == nat.WB_ERR_INVALID                      # an empty segment
    assert level([0, 5], [5, 10], n_open=9, dev=fake) == nat.WB_ERR_INVALID
    assert level([0, 5], [5, 10], scale=0.0, dev=fake) == nat.WB_ERR_INVALID
    assert level([0, 5], [5, 10], min_leaf=0, dev=fake) == nat.WB_ERR_INVALID
    assert level([0, 5], [5, 10], dev=fake, t0=np.array([1 << 62, 5], np.uint64)) == nat.WB_ERR_INVALID
