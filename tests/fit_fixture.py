"""Reader of tests/golden/fit_trees.npz (written by tests/golden/make_golden_fit.py) for the fit tests."""
import os

import numpy as np

from util import GOLDEN

_Z = []


def fixture():
    if not _Z:
        _Z.append(np.load(os.path.join(GOLDEN, "fit_trees.npz")))
    return _Z[0]


def case_names():
    return sorted({k.split("/")[1] for k in fixture().files if k.startswith("case/")})


def _opt(v):
    return None if np.isnan(v) else (int(v) if float(v).is_integer() else float(v))


def case(name):
    """(X0, W0, X1, W1, keyword arguments, expected arrays) of a fixture case."""
    z = fixture()
    d = str(z[f"case/{name}/data"])
    X0, W0, X1, W1 = (z[f"data/{d}/{k}"] for k in ("X0", "W0", "X1", "W1"))
    a = z[f"case/{name}/args"]
    kw = dict(max_depth=int(a[0]), min_samples_leaf=int(a[1]), clip=_opt(a[2]), quantizer=_opt(a[3]))
    if f"case/{name}/allowed" in z.files:
        kw["allowed_features"] = [row[row >= 0] for row in z[f"case/{name}/allowed"]]
    want = {k: z[f"case/{name}/{k}"] for k in ("feature", "threshold", "left", "right", "prediction", "gap")}
    return X0, W0, X1, W1, kw, want


def assert_tree_equal(tree, want, what=""):
    """feature, left, right equal; threshold and prediction equal in their float32 bits."""
    assert np.array_equal(tree.left, want["left"]) and np.array_equal(tree.right, want["right"]), (what, tree.left, want["left"])
    assert np.array_equal(tree.feature, want["feature"]), (what, tree.feature, want["feature"])
    assert tree.threshold.dtype == np.float32 and tree.prediction.dtype == np.float32
    assert np.array_equal(tree.threshold.view(np.uint32), np.asarray(want["threshold"], np.float32).view(np.uint32)), \
        (what, tree.threshold, want["threshold"])
    assert np.array_equal(tree.prediction.view(np.uint32), np.asarray(want["prediction"], np.float32).view(np.uint32)), \
        (what, tree.prediction, want["prediction"])
