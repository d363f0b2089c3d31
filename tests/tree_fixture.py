"""Reader of the golden trees of both learners for the fit tests: tests/golden/fit_trees.npz (fpga.DTree.fit, written by
tests/golden/make_golden_fit.py) and tests/golden/cart_trees.npz (training.DTree.fit, tests/golden/make_golden_cart.py).
``name`` is "fit" or "cart"."""
import os

import numpy as np

from util import GOLDEN

_Z = {}
ARRAYS = ("feature", "threshold", "left", "right", "prediction")


def fixture(name):
    if name not in _Z:
        _Z[name] = np.load(os.path.join(GOLDEN, f"{name}_trees.npz"))
    return _Z[name]


def case_names(name):
    return sorted({k.split("/")[1] for k in fixture(name).files if k.startswith("case/")})


def _case(z, name):
    d = str(z[f"case/{name}/data"])
    return tuple(z[f"data/{d}/{k}"] for k in ("X0", "W0", "X1", "W1")), z[f"case/{name}/args"], \
        {k: z[f"case/{name}/{k}"] for k in ARRAYS + ("gap",)}


def _opt(v):
    return None if np.isnan(v) else (int(v) if float(v).is_integer() else float(v))


def fit_case(name):
    """(X0, W0, X1, W1, keyword arguments of fpga.DTree.fit, expected arrays) of a case of fit_trees.npz."""
    z = fixture("fit")
    data, a, want = _case(z, name)
    kw = dict(max_depth=int(a[0]), min_samples_leaf=int(a[1]), clip=_opt(a[2]), quantizer=_opt(a[3]))
    if f"case/{name}/allowed" in z.files:
        kw["allowed_features"] = [row[row >= 0] for row in z[f"case/{name}/allowed"]]
    return data + (kw, want)


def cart_case(name):
    """(X0, W0, X1, W1, keyword arguments of training.DTree.fit, expected arrays) of a case of cart_trees.npz."""
    data, a, want = _case(fixture("cart"), name)
    return data + (dict(max_depth=int(a[0]), min_samples_leaf=int(a[1]), min_samples_split=int(a[2])), want)


def assert_tree_equal(tree, want, what=""):
    """feature, left, right equal; threshold and prediction equal in their float32 bits."""
    assert np.array_equal(tree.left, want["left"]) and np.array_equal(tree.right, want["right"]), (what, tree.left, want["left"])
    assert np.array_equal(tree.feature, np.asarray(want["feature"]).reshape(-1, 3)), (what, tree.feature, want["feature"])
    assert tree.threshold.dtype == np.float32 and tree.prediction.dtype == np.float32
    for a in ("threshold", "prediction"):
        assert np.array_equal(getattr(tree, a).view(np.uint32), np.asarray(want[a], np.float32).view(np.uint32)), \
            (what, a, getattr(tree, a), want[a])
