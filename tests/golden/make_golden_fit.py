#!/usr/bin/env python3
"""Golden fixtures for the training side: the reference's own ``fpga.DTree.fit`` (reference fpga/training.py:15-171),
``Learner.fit_stage``, ``fit_rejection_threshold``, ``BasicRejectionSchedule``, ``weights`` / ``loss`` (training.py) and
``PixelBanks`` / ``BankScheduler`` (fpga/banks.py) run on small designed inputs.  Same method and stand-ins as
make_golden.py; build container only.  Writes tests/golden/fit_trees.npz: inputs, arguments and expected arrays.

Under NumPy 2 the reference's ``np.arange(xmin-1, xmax+2)`` wraps for uint8 scalars and raises whenever a feature's
minimum is 0; on the same values widened to int64 it computes what NumPy 1.x computed for uint8.  That is the
definition adopted: the reference is fed ``X.astype(np.int64)``.

For every split node of every tree the whole metric table is computed (tests/fit_reference.py) and `gap` -- the best
metric minus the largest strictly smaller value over all (f, t) -- is recorded and asserted to be at least 1e-8, so that
no float64 rounding difference can change an argmax.  (Nodes in which one class is absent have no metric: every value is
NaN and the answer is (A[0], xmin); their gap is recorded as NaN.)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

NONE = np.nan            # how a None argument / result is stored


def lognormal_weights(rng, n):
    return np.exp(rng.normal(0.0, 1.0, n))


def random_data(seed, n0, n1, shape, shifts=((5, 60), (17, -45))):
    """Uniform uint8 samples; class 1 has the features `shifts` moved, so that some splits are informative."""
    rng = np.random.default_rng(seed)
    F = int(np.prod(shape))
    X0 = rng.integers(0, 256, (n0, F))
    X1 = rng.integers(0, 256, (n1, F))
    for f, d in shifts:
        X1[:, f] = np.clip(X1[:, f] + d, 0, 255)
    return dict(X0=X0.astype(np.uint8).reshape((n0,) + shape), X1=X1.astype(np.uint8).reshape((n1,) + shape),
                W0=lognormal_weights(rng, n0), W1=lognormal_weights(rng, n1))


def designed_data():
    shape = (6, 6, 2)
    data = {"base": random_data(1, 300, 200, shape), "odd": random_data(20, 67, 61, shape),      # (a seed whose small nodes have no near-tied splits)
            "big": random_data(3, 3000, 2000, (4, 4, 2), shifts=((5, -40), (17, -30), (9, -25)))}
    # a column that is all 0, one that is all 255, and a duplicated informative column (the lower index must win)
    d = random_data(4, 300, 200, shape)
    for X in (d["X0"], d["X1"]):
        f = X.reshape(X.shape[0], -1)
        f[:, 3] = 0
        f[:, 8] = 255
        f[:, 40] = f[:, 5]
    data["const_dup"] = d
    # feature 0 separates the classes: both children of the root are pure
    d = random_data(5, 300, 200, shape)
    rng = np.random.default_rng(55)
    d["X0"].reshape(300, -1)[:, 0] = rng.integers(0, 100, 300)
    d["X1"].reshape(200, -1)[:, 0] = rng.integers(150, 256, 200)
    d["X0"].reshape(300, -1)[:, 2] = 7
    d["X1"].reshape(200, -1)[:, 2] = 7
    data["pure"] = d
    # weights from 1e-30 to 1
    d = random_data(6, 300, 200, shape)
    rng = np.random.default_rng(66)
    d["W0"], d["W1"] = 10.0 ** rng.uniform(-30, 0, 300), 10.0 ** rng.uniform(-30, 0, 200)
    d["W0"][0], d["W1"][0], d["W0"][1], d["W1"][1] = 1.0, 1.0, 1e-30, 1e-30
    data["wide"] = d
    return data


def cases(PixelBanks, BankScheduler):
    banks = PixelBanks((6, 6, 2), (2, 2))
    sched = BankScheduler(4)
    sched.schedule(2)                                       # (the first stage's banks 0, 1 are skipped: start at 2, 3)
    bank_lists = [banks.bank_pixels(b) for b in sched.schedule(3)]
    d = dict
    return {
        "base_d2": d(data="base"),
        "base_d1": d(data="base", max_depth=1),
        "base_d3": d(data="base", max_depth=3),
        "base_d4": d(data="base", max_depth=4, min_samples_leaf=5),
        "base_noclip": d(data="base", clip=None),
        "base_noquant": d(data="base", quantizer=None),
        "base_raw": d(data="base", clip=None, quantizer=None, max_depth=3),
        "base_banks": d(data="base", max_depth=3, allowed_features=bank_lists),
        "odd_d3": d(data="odd", max_depth=3, min_samples_leaf=4),
        "odd_small_child": d(data="odd", max_depth=3, min_samples_leaf=40),       # children below min_samples_leaf
        "big_d3": d(data="big", max_depth=3),
        "const_dup_d2": d(data="const_dup"),
        "const_only": d(data="const_dup", allowed_features=[np.array([8, 3, 5]), np.array([8, 3])]),   # 255 / 0 columns only
        "pure_d2": d(data="pure"),                                                # pure children answer (A[0], xmin)
        "pure_empty": d(data="pure", max_depth=3,
                        allowed_features=[np.arange(72), np.array([2, 0]), np.arange(72)]),   # a constant A[0]: an empty child
        "wide_d2": d(data="wide"),
    }


def arg_record(kw):
    out = dict(max_depth=kw.get("max_depth", 2), min_samples_leaf=kw.get("min_samples_leaf", 10),
               clip=NONE if kw.get("clip", 3) is None else kw.get("clip", 3),
               quantizer=NONE if kw.get("quantizer", 32) is None else kw.get("quantizer", 32))
    return np.array([out["max_depth"], out["min_samples_leaf"], out["clip"], out["quantizer"]], np.float64)


def main():
    if not hasattr(np, "bool"):
        np.bool = bool
    mg.import_reference()
    from waldboost import training as rt
    from waldboost.fpga import training as rf
    from waldboost.fpga.banks import BankScheduler, PixelBanks
    import fit_reference as fr

    out = {}
    data = designed_data()
    for name, d in data.items():
        for k, v in d.items():
            out[f"data/{name}/{k}"] = v
    gaps_seen = []
    for name, kw in cases(PixelBanks, BankScheduler).items():
        d = data[kw["data"]]
        args = {k: v for k, v in kw.items() if k != "data"}
        T = rf.DTree.fit(d["X0"].astype(np.int64), d["W0"], d["X1"].astype(np.int64), d["W1"], **args)
        tree, nodes = fr.fit(d["X0"], d["W0"], d["X1"], d["W1"], **args)
        gaps = np.array([n.get("gap", np.nan) for n in nodes])
        splits = np.array([n["left"] >= 0 for n in nodes])
        finite = splits & ~np.isnan(gaps)
        assert np.all(gaps[finite] >= 1e-8), (name, gaps)
        gaps_seen.extend(gaps[finite & np.isfinite(gaps)])
        out[f"case/{name}/data"] = np.array(kw["data"])
        out[f"case/{name}/args"] = arg_record(kw)
        if "allowed_features" in kw:
            A = kw["allowed_features"]
            pad = np.full((len(A), max(len(a) for a in A)), -1, np.int32)
            for i, a in enumerate(A):
                pad[i, :len(a)] = a
            out[f"case/{name}/allowed"] = pad
        out[f"case/{name}/feature"] = T.feature
        out[f"case/{name}/threshold"] = T.threshold
        out[f"case/{name}/left"] = T.left
        out[f"case/{name}/right"] = T.right
        out[f"case/{name}/prediction"] = T.prediction
        out[f"case/{name}/gap"] = gaps
        print(f"{name:16s} nodes {T.left.size:2d} splits {int(splits.sum()):2d} pure {int((splits & np.isnan(gaps)).sum())} "
              f"empty {sum(n['samples'].size == 0 for n in nodes)} min gap {np.nanmin(np.where(finite, gaps, np.nan)) if finite.any() else np.nan:.3g}")
    print(f"gaps {min(gaps_seen):.3g} .. {max(gaps_seen):.3g}")

    # ---- Learner.fit_stage: two stages on the base data (float64 scores), the weak learner fed widened samples
    class Widened:
        @staticmethod
        def fit(X0, W0, X1, W1, **kw):
            return rf.DTree.fit(X0.astype(np.int64), W0, X1.astype(np.int64), W1, **kw)

    class Stages(list):
        def append(self, weak, theta):
            list.append(self, (weak, theta))

    d = data["base"]
    rng = np.random.default_rng(7)
    H0, H1 = rng.normal(-0.3, 0.5, 300), rng.normal(0.3, 0.5, 200)
    L = rt.Learner(alpha=0.2, wh=Widened, max_depth=2)
    M = Stages()
    for s in range(2):
        out[f"stage/{s}/H0"], out[f"stage/{s}/H1"] = H0, H1
        loss, fpr, tpr = L.fit_stage(M, d["X0"], H0, d["X1"], H1, theta=None)
        weak, theta = M[-1]
        for a in ("feature", "threshold", "left", "right", "prediction"):
            out[f"stage/{s}/{a}"] = getattr(weak, a)
        out[f"stage/{s}/theta"] = np.float64(theta)
        out[f"stage/{s}/p0"], out[f"stage/{s}/p1"], out[f"stage/{s}/loss"] = np.float64(L.p0[-1]), np.float64(L.p1[-1]), np.float64(loss)
        out[f"stage/{s}/fpr"], out[f"stage/{s}/tpr"] = np.float64(fpr), np.float64(tpr)
        H0, H1 = H0 + weak.predict(d["X0"]), H1 + weak.predict(d["X1"])
        print(f"stage {s}: theta {theta:.4f} p0 {L.p0[-1]:.4f} p1 {L.p1[-1]:.4f} loss {loss:.5f}")
    out["stage/alpha"] = np.float64(0.2)

    # ---- fit_rejection_threshold: the normal case and the three early returns
    rng = np.random.default_rng(8)
    q = lambda a: np.round(a * 8) / 8                       # (repeated responses, as quantised trees give)
    theta_cases = {
        "normal": (q(rng.normal(-1, 1, 400)), 0.5, q(rng.normal(1.5, 0.7, 300)), 0.98, 0.1),
        "normal_f32": (q(rng.normal(-1, 1, 400)).astype(np.float32), 0.9, q(rng.normal(1, 0.7, 300)).astype(np.float32), 1.0, 0.2),
        "separated": (rng.uniform(-2, -1, 50), 1.0, rng.uniform(0.5, 2, 40), 1.0, 0.1),         # max0 < min1 -> min1
        "two_values": (np.array([0.5, 0.25, 0.5]), 1.0, np.array([0.25, 0.5]), 1.0, 0.1),       # < 3 unique -> -inf
        "no_ratio": (rng.normal(0, 1, 200), 1.0, rng.normal(-0.5, 1, 250) - 3.0 * (np.arange(250) == 0), 1.0, 0.01),   # no R > 1/alpha -> -inf
    }
    for name, (h0, p0, h1, p1, alpha) in theta_cases.items():
        out[f"theta/{name}/H0"], out[f"theta/{name}/H1"] = h0, h1
        out[f"theta/{name}/args"] = np.array([p0, p1, alpha])
        th = rt.fit_rejection_threshold(h0, p0, h1, p1, alpha)
        out[f"theta/{name}/theta"] = np.float64(th)
        print(f"theta/{name}: {th}")
    assert np.isfinite(out["theta/normal/theta"]) and np.isfinite(out["theta/normal_f32/theta"])
    assert out["theta/separated/theta"] == theta_cases["separated"][2].min()
    assert out["theta/two_values/theta"] == -np.inf and out["theta/no_ratio/theta"] == -np.inf

    # ---- schedule, banks, weights, loss
    sch = [((0, None), 1e-5), ((2, 5), 1e-3), (None, 1e-5), ((None, 3), 0.5)]
    probe = [(0, 1.0), (1, 1.0), (2, 0.6), (3, 1e-4), (5, 0.4), (6, 1.0), (40, 1e-6)]
    res = np.empty((len(sch), len(probe)))
    for i, (iv, tp) in enumerate(sch):
        S = rt.BasicRejectionSchedule(iv, tp)
        for j, (stage, p0) in enumerate(probe):
            r = S(stage, p0)
            res[i, j] = NONE if r is None else r
    out["schedule/ctor"] = np.array([[NONE if iv is None or iv[0] is None else iv[0], NONE if iv is None or iv[1] is None else iv[1], tp,
                                      1.0 if iv is None else 0.0] for iv, tp in sch])
    out["schedule/probe"], out["schedule/result"] = np.array(probe), res
    for shape, block in (((6, 6, 2), (2, 2)), ((5, 7), (2, 3)), ((8, 8, 4), (2, 2))):
        tag = "x".join(map(str, shape)) + "_" + "x".join(map(str, block))
        B = PixelBanks(shape, block)
        out[f"banks/{tag}/pattern"] = B.pattern
        out[f"banks/{tag}/pixels"] = B.bank_pixels([1])
        out[f"banks/{tag}/pixels2"] = B.bank_pixels([int(np.prod(block)) - 1, 0])
    S = BankScheduler(4)
    out["banks/schedule"] = np.array([S.schedule(2), S.schedule(2), S.schedule(2)])
    S = BankScheduler()
    out["banks/schedule_default"] = np.array([S.schedule(3), S.schedule(3), S.schedule(3)])
    h = rng.normal(0, 1, 37)
    out["weights/H"], out["weights/W"] = h, rt.weights(h)
    out["weights/H32"], out["weights/W32"] = h.astype(np.float32), rt.weights(h.astype(np.float32))
    out["loss/H0"], out["loss/H1"] = h[:20], h[20:]
    out["loss/value"] = np.float64(rt.loss(h[:20], h[20:]))

    path = os.path.join(HERE, "fit_trees.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print(f"fit golden fixtures written: {size} bytes")


if __name__ == "__main__":
    main()
