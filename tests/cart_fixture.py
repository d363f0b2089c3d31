"""Reader of tests/golden/cart_trees.npz (written by tests/golden/make_golden_cart.py) for the CART tests."""
import os

import numpy as np

from util import GOLDEN

_Z = []
ARRAYS = ("feature", "threshold", "left", "right", "prediction")


def fixture():
    if not _Z:
        _Z.append(np.load(os.path.join(GOLDEN, "cart_trees.npz")))
    return _Z[0]


def case_names():
    return sorted({k.split("/")[1] for k in fixture().files if k.startswith("case/")})


def case(name):
    """(X0, W0, X1, W1, keyword arguments, expected arrays) of a fixture case."""
    z = fixture()
    d = str(z[f"case/{name}/data"])
    X0, W0, X1, W1 = (z[f"data/{d}/{k}"] for k in ("X0", "W0", "X1", "W1"))
    a = z[f"case/{name}/args"]
    kw = dict(max_depth=int(a[0]), min_samples_leaf=int(a[1]), min_samples_split=int(a[2]))
    want = {k: z[f"case/{name}/{k}"] for k in ARRAYS + ("gap",)}
    return X0, W0, X1, W1, kw, want


def assert_tree_equal(tree, want, what=""):
    """feature, left, right equal; threshold and prediction equal in their float32 bits."""
    assert np.array_equal(tree.left, want["left"]) and np.array_equal(tree.right, want["right"]), (what, tree.left, want["left"])
    assert np.array_equal(tree.feature, np.asarray(want["feature"]).reshape(-1, 3)), (what, tree.feature, want["feature"])
    assert tree.threshold.dtype == np.float32 and tree.prediction.dtype == np.float32
    for a in ("threshold", "prediction"):
        assert np.array_equal(getattr(tree, a).view(np.uint32), np.asarray(want[a], np.float32).view(np.uint32)), \
            (what, a, getattr(tree, a), want[a])
