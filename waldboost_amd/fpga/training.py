"""The FPGA flavour's weak learner and training loop (reference fpga/training.py): ``DTree.fit`` grows one
decision tree by information gain over weighted 256-bin histograms, ``train`` is the stage loop around it.

What runs where:

* the split search -- per open node and feature two weighted histograms, their prefix sums, the metric of every
  threshold and the two argmaxes -- and the routing of samples to child nodes are HIP kernels (csrc/wb_fit.hip,
  ``wb_fit_level_launch`` / ``wb_fit_route_launch``), one launch group per tree level, launched by ``_level_search``;
* the weight normalisation (float64, the class sums correctly rounded so that they do not depend on the sample order),
  the leaf/split decision per node and the node predictions -- the reference's own NumPy expressions over the node
  membership the GPU returns, so they are bit-equal -- run on the host, around the growth loop shared with
  ``training.DTree.fit`` (``waldboost_amd/_grow.py``: ``grow``, ``check_weights``, ``stage``, ``MAX_DEPTH``);
* ``SamplePool.update``, ``weak.predict`` and ``model.append`` run on the GPU as before.

tests/fit_reference.py is the NumPy statement of what ``DTree.fit`` computes.
"""
import ctypes as C
import logging
import math

import numpy as np

from .. import _native as nat
from .._grow import MAX_DEPTH, check_weights, grow, stage
from ..samples import SamplePool
from ..training import BasicRejectionSchedule
from ..training import DTree as BaseDTree
from ..training import Learner
from .banks import BankScheduler, PixelBanks

def _check_samples(X, name):
    """(N, sample shape) of an ndarray or tensor (N, m, n, C) of uint8."""
    dt = nat.dtype_name(X)
    if dt != "uint8":
        raise NotImplementedError(f"fpga.DTree.fit: no kernel for {dt} samples ({name}); the split search is built on "
                                  "256-bin histograms of uint8 channels")
    if len(X.shape) != 4:
        raise ValueError(f"{name} must have shape (N, m, n, C), got {tuple(X.shape)}")
    return int(X.shape[0]), tuple(int(s) for s in X.shape[1:])


def fit_detail(X0, W0, X1, W1, max_depth=2, min_samples_leaf=10, allowed_features=None, clip=3, quantizer=32):
    """``DTree.fit`` with its working: returns (tree, info), info a dict with per node (breadth-first id) ``samples``
    (indices into the concatenated class-0, class-1 samples, ascending), ``depth``, and for split nodes ``metric``,
    ``t0``, ``t1`` (the best metric and the node's normalised class weights as the kernel saw them; NaN on leaves)."""
    if not 1 <= int(max_depth) <= MAX_DEPTH:
        raise NotImplementedError(f"fpga.DTree.fit: max_depth must be 1 .. {MAX_DEPTH} (a level of at most "
                                  f"{nat.WB_FIT_MAX_OPEN} nodes per launch), got {max_depth}")
    max_depth = int(max_depth)
    n0, shape = _check_samples(X0, "X0")
    n1, shape1 = _check_samples(X1, "X1")
    if shape != shape1:
        raise ValueError(f"X0 and X1 hold samples of different shapes: {shape}, {shape1}")
    W = np.concatenate([check_weights(W0, n0, "W0"), check_weights(W1, n1, "W1")])
    N, F = n0 + n1, int(np.prod(shape))
    Y = np.array([0] * n0 + [1] * n1)
    if allowed_features is not None:
        if len(allowed_features) < max_depth:
            raise ValueError("allowed_features needs one feature list per tree depth")
        allowed = [np.asarray(a).reshape(-1).astype(np.int64) for a in allowed_features[:max_depth]]
        if any(a.size == 0 or a.min() < 0 or a.max() >= F for a in allowed):
            raise ValueError(f"allowed_features must be non-empty lists of feature indices 0 .. {F - 1}")
    else:
        allowed = [np.arange(F)] * max_depth

    # split weights: each class divided by twice its sum, once over all samples, in float64 (reference
    # fpga/training.py:105-107), then to integers of 2^-62: exact, a power-of-two scale of a float of at most 0.5.  The
    # class sum is the correctly rounded one (math.fsum) where the reference takes np.sum: it differs from that by an ulp
    # at the most and does not depend on the order of the samples, which np.sum's pairwise adds do.  (A class whose weights
    # are all 0 divides 0 by 0 in the reference; it has no weight in any node either way: every metric is NaN.)
    wq = W.astype(np.float64)
    for c in (0, 1):
        total = math.fsum(wq[Y == c])
        wq[Y == c] = wq[Y == c] / (total * 2) if total > 0 else 0.0
    q = np.rint(np.ldexp(wq, 62)).astype(np.uint64)

    def opens(nd):
        if nd["depth"] == max_depth or nd["samples"].size < min_samples_leaf:
            return False
        if nd["samples"].size == 0:
            raise ValueError("fpga.DTree.fit: cannot split an empty node (min_samples_leaf must be at least 1)")
        return True

    def split(nd, s):                   # every open node splits
        nd.update(feature=int(s["feature"]), threshold=int(s["threshold"]), metric=float(s["metric"]), t0=float(s["t0"]), t1=float(s["t1"]))
        return {}, {}

    nodes = grow(N, lambda samples, depth: dict(samples=samples, depth=depth, feature=-1, threshold=-1), opens,
                 _level_search(X0, X1, F, Y, q, allowed), split)

    # the tree and the node predictions: the reference's expressions (fpga/training.py:144-171)
    n_nodes = len(nodes)
    feature = [None] * n_nodes
    threshold = np.empty(n_nodes)
    left = np.empty(n_nodes, "i")
    right = np.empty(n_nodes, "i")
    pred = np.empty(n_nodes, "f")
    for nid, nd in nodes.items():
        f = nd["feature"]
        feature[nid] = np.unravel_index(f, shape) if f >= 0 else None
        threshold[nid] = nd["threshold"]
        left[nid] = nd["left"]
        right[nid] = nd["right"]
        y, w = Y[nd["samples"]], W[nd["samples"]]
        w0 = w[y == 0].sum() + 1e-3
        w1 = w[y == 1].sum() + 1e-3
        pred[nid] = np.log(w1 / w0) / 2
    if clip is not None:
        pred = np.clip(pred, -clip, clip)
    if quantizer is not None:
        pred = np.round(quantizer * pred) / quantizer
    col = lambda key: np.array([nodes[i].get(key, np.nan) for i in range(n_nodes)])
    info = dict(samples=[nodes[i]["samples"] for i in range(n_nodes)], depth=np.array([nodes[i]["depth"] for i in range(n_nodes)]),
                flat_feature=np.array([nodes[i]["feature"] for i in range(n_nodes)]), metric=col("metric"), t0=col("t0"), t1=col("t1"))
    return BaseDTree(feature, threshold, left, right, pred), info


def _slots(level, opened):
    """slot[j]: the index among the open nodes of the level's j-th node, -1 for a leaf (a level's ids are consecutive:
    every open node of the level before it split)."""
    slot = np.full(len(level), -1, np.int8)
    for j, nd in enumerate(opened):
        slot[nd["id"] - level[0]["id"]] = j
    return slot


def _level_search(X0, X1, F, Y, q, allowed):
    """The level search of ``fit_detail`` on the GPU (csrc/wb_fit.hip), for ``_grow.grow``: stages the samples and per level
    launches the histograms, the pick over ``allowed[depth]`` and the routing."""
    import torch
    dev = nat.require_gpu()
    N = Y.size
    xt, q_d, cls_d, node_d = stage(X0, X1, F, torch.uint8, q, Y, dev)
    allowed_d = {}

    def search(depth, level, opened, child_base):
        n_open, base = len(opened), level[0]["id"]
        slot = _slots(level, opened)
        A = allowed[depth]
        key = id(A)
        if key not in allowed_d:
            allowed_d[key] = torch.from_numpy(A.astype(np.int32)).to(dev)
        scratch = torch.empty(nat.query("wb_fit_scratch_bytes", A.size, n_open), dtype=torch.uint8, device=dev)
        splits_d = torch.empty(n_open * nat.FIT_SPLIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        slot_p = slot.ctypes.data_as(C.c_void_p)
        nat.launch("wb_fit_level_launch", xt, N, F, q_d, cls_d, node_d, base, len(level), slot_p, n_open, allowed_d[key], A.size,
                   scratch, scratch.numel(), splits_d)
        nat.launch("wb_fit_route_launch", xt, N, F, node_d, base, len(level), slot_p, n_open, splits_d, child_base)
        return splits_d.cpu().numpy().view(nat.FIT_SPLIT_DTYPE), node_d.cpu().numpy()
    return search


class DTree:
    """Decision tree training algorithm of the FPGA flavour (reference fpga/training.py:60-171).  Unlike the sklearn
    learner, the features a split may test can be restricted per node depth (``allowed_features``), which the FPGA needs
    to evaluate trees in parallel without bank collisions."""

    @staticmethod
    def fit(X0, W0, X1, W1, max_depth=2, min_samples_leaf=10, allowed_features=None, clip=3, quantizer=32):
        """Train a decision tree on the GPU.

        X0, X1 : uint8 ndarrays or device tensors (N, m, n, C): samples of class 0 and class 1.  Other dtypes raise
            NotImplementedError (there is no kernel for them), as the channel functions do.
        W0, W1 : sample weights; must be finite and non-negative (ValueError otherwise).
        max_depth : 1 .. 4.  A tree level is one launch over at most 8 nodes; a larger depth raises NotImplementedError.
        min_samples_leaf : a node with fewer samples becomes a leaf.
        allowed_features : None, or per depth the ordered list of flat feature indices a split may test.
        clip, quantizer : node predictions are clipped to +-clip and rounded to multiples of 1/quantizer (None: skip).

        Returns an initialised ``waldboost_amd.training.DTree``: nodes in breadth-first order, `feature` as (r, c, ch),
        a split routes with ``x <= threshold``; leaves carry threshold -1.  The tree equals the reference's on the
        same values (NumPy 1.x semantics for uint8 samples; under NumPy 2 the reference needs them widened to int64)
        whenever the best split of every node leads by more than float64 rounding -- for float64 weights: weights of
        another float type are widened to float64 first, where the reference normalises and accumulates its histograms
        in the weights' own type (float32 weights give it float32 rounding, which this fit does not imitate); weights
        below 2^-63 of their class's total count as 0 in the split search.  The result does not depend on the order of the samples or on the run.
        """
        return fit_detail(X0, W0, X1, W1, max_depth, min_samples_leaf, allowed_features, clip, quantizer)[0]


def train(model, training_images, learner=None, pool=None, length=64, max_depth=2, theta_schedule=BasicRejectionSchedule(),
          bank_pattern_shape=(2, 2), clip=3, quantizer=32, callbacks=[], logger=None):
    """Train a model with FPGA friendly feature access patterns (reference fpga/training.py:174-264): stages are
    appended to `model` until it has `length` of them.

    training_images : iterable of dicts with 'image' and 'groundtruth_boxes' (what SamplePool.update scans).
    learner, pool : continue with these (their lengths must agree with the model's); new ones otherwise.
    theta_schedule : callable (stage, false positive rate) -> -inf or None (estimate the rejection threshold).
    bank_pattern_shape : block of the bank pattern, e.g. (2, 2) for 4 banks; tree depth d of a stage may only test the
        features of the bank scheduled for it.  None: no restriction.
    clip, quantizer : accepted as in the reference, which does not hand them on either: the trees get DTree.fit's
        defaults (3, 32) unless the learner's wh_args say otherwise.
    callbacks : called as cb(model, learner, stage) after every stage.

    Returns the learner (None when the model is long enough already).
    """
    logger = logger or logging.getLogger("WaldBoost/FPGA")
    if len(model) >= length:
        return
    learner = learner or Learner(wh=DTree)
    if learner.wh is not DTree:
        raise ValueError("Learner.wh should be waldboost_amd.fpga.DTree")
    if len(model) != len(learner):
        raise RuntimeError("Model length and learner length are not consistent")
    if learner.wh_args.get("max_depth") != max_depth:
        learner.wh_args["max_depth"] = max_depth
    if len(model) > 0:
        logger.info(f"{len(model)} stages are already present, continuing")
    if bank_pattern_shape is not None:
        banks = PixelBanks(model.shape, bank_pattern_shape)
        scheduler = BankScheduler(np.prod(bank_pattern_shape))
    pool = pool or SamplePool()
    for stage in range(len(model), length):
        logger.info(f"Training stage {stage}")
        pool.update(model, training_images)
        X0, H0 = pool.get_false_positives()
        X1, H1 = pool.get_true_positives()
        if bank_pattern_shape is not None:
            ftrs = [banks.bank_pixels(b) for b in scheduler.schedule(max_depth)]
        else:
            ftrs = None
        loss, p0, p1 = learner.fit_stage(model, X0, H0, X1, H1, allowed_features=ftrs,
                                         theta=theta_schedule(stage, learner.false_positive_rate))
        logger.log(15, f"Stage {stage}: loss: {loss:g}, fpr: {p0:g}, tpr: {p1:g}")
        for cb in callbacks:
            cb(model, learner, stage)
    return learner
