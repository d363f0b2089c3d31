#!/usr/bin/env python3
"""Golden fixtures for the precision / recall curve of ``waldboost_amd.testing.Evaluator.evaluate``: scikit-learn 0.24.2's
``sklearn.metrics.precision_recall_curve`` and ``auc`` (what reference testing.py:72-76 calls) run on small (y_true, scores)
inputs.  Needs scikit-learn 0.24.2 and nothing else: it reads nothing from the reference.  Later releases no longer cut
the curve at full recall and answer the no-positive case differently, so any other version is refused.
Writes tests/golden/eval_curves.npz: per case y_true, scores, precision, recall, thresholds, auc (NaNs as they come)."""
import os
import warnings

import numpy as np
import sklearn
import sklearn.metrics

HERE = os.path.dirname(os.path.abspath(__file__))
VERSION = "0.24.2"


def cases():
    rng = np.random.default_rng(20240)
    b = lambda *v: np.array(v, bool)
    yield "doc-example", b(0, 0, 1, 1), np.array([0.1, 0.4, 0.35, 0.8])
    yield "heavy-ties", rng.random(64) < 0.4, np.round(rng.normal(0, 1, 64) * 2) / 2
    yield "all-tied", rng.random(20) < 0.5, np.full(20, 1.5)
    yield "all-positive", np.ones(12, bool), rng.normal(0, 1, 12)
    yield "all-positive-ties", np.ones(9, bool), np.array([1, 1, 2, 2, 2, 3, 0, 0, 0], np.float64)
    yield "single-positive", b(1), np.array([0.25])
    yield "single-negative", b(0), np.array([0.25])
    yield "positives-lowest", np.arange(30) < 6, np.arange(30, dtype=np.float64)
    yield "positives-highest", np.arange(30) >= 24, np.arange(30, dtype=np.float64)
    yield "float32-scores", rng.random(48) < 0.5, (np.round(rng.normal(0, 2, 48) * 8) / 8).astype(np.float32)
    yield "float32-general", rng.random(40) < 0.3, rng.normal(0, 1, 40).astype(np.float32)
    yield "no-positive", np.zeros(10, bool), rng.normal(0, 1, 10)
    yield "no-positive-ties", np.zeros(6, bool), np.array([1, 1, 0, 0, 2, 2], np.float64)
    yield "one-positive-last", np.arange(17) == 0, np.arange(17, dtype=np.float64)
    yield "negative-scores-and-zeros", rng.random(33) < 0.5, np.array([-0.0, 0.0, -1.5, 2.0] * 8 + [0.0])


def main():
    assert sklearn.__version__ == VERSION, f"scikit-learn {VERSION} is the yardstick, this is {sklearn.__version__}"
    out = {"sklearn_version": np.array(VERSION), "names": []}
    for name, y, s in cases():
        assert y.size <= 64
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            p, r, t = sklearn.metrics.precision_recall_curve(y, s)
            a = sklearn.metrics.auc(r, p)
        out["names"].append(name)
        for k, v in (("y_true", y), ("scores", s), ("precision", p), ("recall", r), ("thresholds", t), ("auc", np.float64(a))):
            out[f"{name}/{k}"] = np.asarray(v)
        print(f"{name}: {y.size} samples, {t.size} thresholds, auc {a!r}")
    out["names"] = np.array(out["names"])
    np.savez(os.path.join(HERE, "eval_curves.npz"), **out)


if __name__ == "__main__":
    main()
