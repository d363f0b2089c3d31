#!/usr/bin/env python3
"""Golden fixtures for ``training.DTree.fit``: the reference's own ``training.DTree.fit`` (reference training.py:33-50,
scikit-learn's DecisionTreeClassifier(class_weight="balanced")) run on small designed inputs.  Same method and stand-ins
as make_golden.py; build container only (it needs the reference tree and scikit-learn).  Writes
tests/golden/cart_trees.npz: inputs, arguments and the reference's tree arrays.

sklearn visits the features in a random permutation and keeps the first strict improvement, so among exactly tied
candidates its pick depends on ``random_state``; the build's rule (lowest feature, then lowest position) is its own.  A
fixture case must therefore not depend on either.  For every case this generator asserts:

* the reference's tree is identical for random_state 0 .. 7;
* in every split node the best proxy (tests/cart_reference.py) leads the largest strictly smaller proxy of any candidate
  by at least 1e-9 relative, so that no float64 rounding difference -- sklearn accumulates float64 sums, the build
  integer ones -- can change the winner;
* no two different features reach the best proxy.

Small nodes of deep trees tie easily (several features separate three samples equally well).  Each data set is drawn
from the first seed, counted up from its base seed, at which all of its cases satisfy the three conditions; the seed
found is printed and stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

MIN_GAP = 1e-9


def lognormal_weights(rng, n):
    return np.exp(rng.normal(0.0, 1.0, n))


def float_data(seed, n0, n1, shape, shifts=((5, 0.25), (17, -0.2), (9, 0.12)), grid=None):
    """Uniform float32 samples in 0 .. 1; class 1 has the features `shifts` moved, so that some splits are informative.
    grid: values are multiples of 1 / grid (fewer mantissa bits: the file compresses)."""
    rng = np.random.default_rng(seed)
    F = int(np.prod(shape))
    X0, X1 = rng.random((n0, F)), rng.random((n1, F))
    for f, d in shifts:
        X1[:, f] += d
    if grid:
        X0, X1 = np.round(X0 * grid) / grid, np.round(X1 * grid) / grid
    return dict(X0=X0.astype(np.float32).reshape((n0,) + shape), X1=X1.astype(np.float32).reshape((n1,) + shape),
                W0=lognormal_weights(rng, n0), W1=lognormal_weights(rng, n1))


def make_base(seed):
    return float_data(seed, 300, 200, (6, 6, 2))


def make_odd(seed):
    return float_data(seed, 37, 26, (4, 4, 2))


def make_u8(seed):
    rng = np.random.default_rng(seed)
    X0, X1 = rng.integers(0, 256, (300, 32)), rng.integers(0, 256, (200, 32))
    for f, d in ((5, 60), (17, -45), (9, 30)):
        X1[:, f] = np.clip(X1[:, f] + d, 0, 255)
    return dict(X0=X0.astype(np.uint8).reshape(300, 4, 4, 2), X1=X1.astype(np.uint8).reshape(200, 4, 4, 2),
                W0=lognormal_weights(rng, 300), W1=lognormal_weights(rng, 200))


def make_const(seed):
    """Columns that are constant: 0, a value, and one that varies by less than 1e-7 in all."""
    d = float_data(seed, 300, 200, (4, 4, 2))
    rng = np.random.default_rng(seed + 1000)
    for X in (d["X0"], d["X1"]):
        f = X.reshape(X.shape[0], -1)
        f[:, 3] = 0.0
        f[:, 8] = 0.75
        f[:, 5] = np.float32(0.5) + rng.integers(0, 2, X.shape[0]).astype(np.float32) * np.float32(5.9604645e-08)
    return d


def make_pure(seed):
    """Feature 0 separates most of class 0 from everything else: the root's left child is pure, a leaf, and the right
    child goes on splitting -- an unbalanced tree in pre-order."""
    d = float_data(seed, 300, 200, (4, 4, 2), shifts=((17, -0.2), (9, 0.12)))
    rng = np.random.default_rng(seed + 1000)
    f0 = d["X0"].reshape(300, -1)
    f0[:, 0] = np.where(np.arange(300) < 220, rng.uniform(0.0, 0.4, 300), rng.uniform(0.6, 1.0, 300)).astype(np.float32)
    d["X1"].reshape(200, -1)[:, 0] = rng.uniform(0.6, 1.0, 200).astype(np.float32)
    return d


def make_sep(seed):
    """Feature 2 separates the classes: both children of the root are pure."""
    d = float_data(seed, 80, 60, (4, 4, 2))
    rng = np.random.default_rng(seed + 1000)
    d["X0"].reshape(80, -1)[:, 2] = rng.uniform(0.0, 0.4, 80).astype(np.float32)
    d["X1"].reshape(60, -1)[:, 2] = rng.uniform(0.6, 1.0, 60).astype(np.float32)
    return d


def make_wide(seed):
    d = float_data(seed, 300, 200, (4, 4, 2))
    rng = np.random.default_rng(seed + 1000)
    d["W0"], d["W1"] = 10.0 ** rng.uniform(-30, 0, 300), 10.0 ** rng.uniform(-30, 0, 200)
    d["W0"][0], d["W1"][0], d["W0"][1], d["W1"][1] = 1.0, 1.0, 1e-30, 1e-30
    return d


def make_unequal(seed):
    return float_data(seed, 2000, 60, (4, 4, 2), grid=4096)


def make_tiny(seed):
    """Most values of the uninformative columns are residues below 1e-7 in size (as a grad_hist channel's projection
    leaves where there is no gradient), drawn alike for both classes, the rest ordinary: runs of sorted values that the
    1e-7 rule holds together, then a step.  Column 11 holds residues only: constant by the rule.  The informative columns
    5, 17 and 9 keep ordinary values, so the best split of a node lies at an ordinary step.  (That matters: scikit-learn
    1.7.2 as built compares with a threshold of 0 where its source says 1e-7 -- it splits two values 1e-9 apart --, so it
    would accept a winning split inside a run of residues, which the stated rule does not rate.)"""
    d = float_data(seed, 300, 200, (4, 4, 2))
    rng = np.random.default_rng(seed + 1000)
    for X in (d["X0"], d["X1"]):
        f = X.reshape(X.shape[0], -1)
        residue = (10.0 ** rng.uniform(-12, -7.3, f.shape) * rng.choice([-1.0, 1.0], f.shape)).astype(np.float32)
        keep = rng.random(f.shape) >= 0.6
        keep[:, [5, 17, 9]] = True
        keep[:, 11] = False
        f[...] = np.where(keep, f, residue)
    return d


def make_big(seed):
    return float_data(seed, 2500, 1700, (4, 4, 2), shifts=((5, -0.2), (17, -0.15), (9, 0.1)), grid=4096)


DATA = {"base": (make_base, 1), "odd": (make_odd, 20), "u8": (make_u8, 30), "const": (make_const, 40), "pure": (make_pure, 50),
        "sep": (make_sep, 55), "wide": (make_wide, 60), "unequal": (make_unequal, 70), "tiny": (make_tiny, 80), "big": (make_big, 90)}

d = dict
CASES = {
    "base_d1": d(data="base", max_depth=1),
    "base_d2": d(data="base", max_depth=2),
    "base_d3": d(data="base", max_depth=3, min_samples_leaf=5),
    "base_d4": d(data="base", max_depth=4, min_samples_leaf=10),
    "base_leaf10": d(data="base", max_depth=3, min_samples_leaf=10),
    "base_no_children": d(data="base", max_depth=3, min_samples_leaf=130),     # 2 * 130 exceeds every child of the root
    "base_split": d(data="base", max_depth=4, min_samples_leaf=5, min_samples_split=120),
    "odd_d2": d(data="odd", max_depth=2, min_samples_leaf=4),
    "u8_d2": d(data="u8", max_depth=2),
    "u8_d3": d(data="u8", max_depth=3, min_samples_leaf=10),
    "const_d2": d(data="const", max_depth=2),
    "pure_d3": d(data="pure", max_depth=3, min_samples_leaf=10),
    "sep_d3": d(data="sep", max_depth=3),
    "wide_d2": d(data="wide", max_depth=2),
    "unequal_d2": d(data="unequal", max_depth=2, min_samples_leaf=5),
    "tiny_d2": d(data="tiny", max_depth=2),
    "tiny_d3": d(data="tiny", max_depth=3, min_samples_leaf=10),
    "big_d3": d(data="big", max_depth=3),
}
ARRAYS = ("feature", "threshold", "left", "right", "prediction")


def arg_record(kw):
    return np.array([kw["max_depth"], kw.get("min_samples_leaf", 1), kw.get("min_samples_split", 2)], np.int64)


def run_case(rt, cr, data, kw):
    """The reference's tree arrays, or None when the case does not satisfy the generator's conditions."""
    args = {k: v for k, v in kw.items() if k != "data"}
    trees = [rt.DTree.fit(data["X0"], data["W0"], data["X1"], data["W1"], random_state=rs, **args) for rs in range(8)]
    first = {a: getattr(trees[0], a) for a in ARRAYS}
    for T in trees[1:]:
        if any(not np.array_equal(getattr(T, a), first[a], equal_nan=True) for a in ARRAYS):
            return None
    _, nodes = cr.fit(data["X0"], data["W0"], data["X1"], data["W1"], **args)
    for n in nodes:
        if n["left"] >= 0 and (not n["gap"] >= MIN_GAP or n["winners"] != 1):
            return None
    first["gap"] = np.array([n.get("gap", np.nan) for n in nodes])
    return first


def main():
    if not hasattr(np, "bool"):
        np.bool = bool
    mg.import_reference()
    from waldboost import training as rt
    import cart_reference as cr

    out = {}
    for name, (make, seed0) in DATA.items():
        mine = {c: kw for c, kw in CASES.items() if kw["data"] == name}
        for seed in range(seed0, seed0 + 40):
            data = make(seed)
            res = {c: run_case(rt, cr, data, kw) for c, kw in mine.items()}
            if all(r is not None for r in res.values()):
                break
        else:
            raise SystemExit(f"no seed for {name}")
        for k, v in data.items():
            out[f"data/{name}/{k}"] = v
        out[f"data/{name}/seed"] = np.int64(seed)
        for c, r in res.items():
            out[f"case/{c}/data"] = np.array(name)
            out[f"case/{c}/args"] = arg_record(mine[c])
            for a in ARRAYS + ("gap",):
                out[f"case/{c}/{a}"] = r[a]
            print(f"{c:18s} seed {seed:3d} nodes {r['left'].size:2d} splits {int((r['left'] >= 0).sum()):2d} "
                  f"min gap {np.nanmin(r['gap']) if np.isfinite(r['gap']).any() else np.nan:.3g}")
    path = os.path.join(HERE, "cart_trees.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print(f"cart golden fixtures written: {size} bytes")


if __name__ == "__main__":
    main()
