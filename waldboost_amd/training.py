"""``DTree`` -- the weak classifier of the cascade (reference training.py:23-96) -- and the stage
learner around it (reference training.py:14-20, 99-253).

Same constructor, attributes, proto I/O and ``predict_on_image``/``apply``/``predict``
signatures as the reference so that ``from waldboost_amd.training import DTree`` is a drop-in;
the evaluation runs in a HIP kernel (csrc/wb_cascade.hip: tree_eval_kernel).  ``DTree.fit``
(reference training.py:33-50: scikit-learn's ``DecisionTreeClassifier(class_weight="balanced")``,
gini criterion, best splitter) trains on the GPU: the sort of every feature column and the split
search, routing and re-partitioning of each tree level are HIP kernels (csrc/wb_cart.hip, launched
by ``_level_search``); the class weights, the leaf decisions, the pre-order numbering and the node
predictions -- the reference's own NumPy expressions -- run on the host, around the growth loop
this learner shares with the FPGA flavour's (``_grow.grow``; ``check_weights``,
``stage`` and ``MAX_DEPTH`` live there too).  tests/cart_reference.py is the NumPy statement of
what it computes.  ``waldboost_amd.fpga.DTree`` (csrc/wb_fit.hip) is the FPGA
flavour's learner on uint8 samples.

``Learner``, ``fit_rejection_threshold``, ``BasicRejectionSchedule``, ``weights``, ``loss`` and
``as_features`` are the reference's host arithmetic on a pool's scores; ``Learner.fit_stage`` calls
``wh.fit`` and ``weak.predict``, which run on the GPU.
"""
import ctypes as C
import logging
import math
import pickle

import numpy as np

from . import _native as nat
from ._grow import MAX_DEPTH, check_weights, grow, stage
from .compare import channel_tensor

logger = logging.getLogger(__name__)


def weights(H):
    """Sample weights of the scores H (reference training.py:14-15)."""
    return np.exp(H) / H.size / 2


def as_features(X):
    """(N, m, n, C) samples as (N, m*n*C) feature rows (reference training.py:18-20)."""
    n, *shape = X.shape
    return X.reshape((n, int(np.prod(shape))))


_ARRAYS = ("threshold", "prediction", "feature", "left", "right")
_REBINDS = [0]          # bumped whenever an array attribute of any DTree is rebound (Model.device_cascade's cache watches it)


class DTree:
    def __init__(self, feature, threshold, left, right, prediction):
        # reference training.py:24-31.  The five arrays are views into ONE private block of bytes per tree, so that
        # `content()` -- what Model.device_cascade compares against the copy on the GPU -- is one buffer per tree;
        # they stay writable (the reference's are) and an in-place edit shows up in that buffer.
        feature = np.array([f if f is not None else [0, 0, 0] for f in feature], np.uint8).reshape(-1, 3)
        threshold = np.array(threshold, np.float32)
        left = np.array(left, np.int8)
        right = np.array(right, np.int8)
        prediction = np.array(prediction, np.float32)
        k = left.size
        if not (feature.shape[0] == threshold.size == right.size == prediction.size == k) or threshold.ndim != 1 \
                or left.ndim != 1 or right.ndim != 1 or prediction.ndim != 1:
            raise ValueError("DTree arrays must have one entry per node")
        blob = np.empty(13 * k, np.uint8)
        views = dict(threshold=blob[:4 * k].view(np.float32), prediction=blob[4 * k:8 * k].view(np.float32),
                     feature=blob[8 * k:11 * k].reshape(k, 3), left=blob[11 * k:12 * k].view(np.int8),
                     right=blob[12 * k:].view(np.int8))
        for name, src in (("threshold", threshold), ("prediction", prediction), ("feature", feature), ("left", left),
                          ("right", right)):
            views[name][...] = src
            object.__setattr__(self, name, views[name])
        object.__setattr__(self, "_blob", blob)
        self.node = self.left >= 0
        self.node_idx = np.flatnonzero(self.node)

    def __setattr__(self, name, value):
        # rebinding one of the arrays (w.threshold = other) detaches the tree from its block: content() then reads
        # the five arrays one by one
        if name in _ARRAYS:
            object.__setattr__(self, "_blob", None)
            _REBINDS[0] += 1
        object.__setattr__(self, name, value)

    # copy.copy / copy.deepcopy / pickle: NumPy copies (or unpickles) every view on its own, which would leave a tree whose
    # `_blob` no longer shares memory with `threshold`, `feature`, ...: an in-place edit of the copy would then never reach
    # content(), and Model.device_cascade would keep scanning with the stale GPU cascade.  So the state that travels is the
    # five arrays (plus whatever else a caller hung on the tree), and the restored tree gets a block and views of its own.
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k not in ("_blob", "_dev", "node", "node_idx") and k not in _ARRAYS}
        state["_arrays"] = {a: np.array(getattr(self, a)) for a in _ARRAYS}
        return state

    def __setstate__(self, state):
        state = dict(state)
        arrays = state.pop("_arrays", None)
        if arrays is None:              # (a pickle written before this protocol existed: plain attribute dict)
            arrays = {a: state.pop(a) for a in _ARRAYS}
            for k in ("_blob", "_dev", "node", "node_idx"):
                state.pop(k, None)
        DTree.__init__(self, arrays["feature"], arrays["threshold"], arrays["left"], arrays["right"], arrays["prediction"])
        for k, v in state.items():
            object.__setattr__(self, k, v)

    def content(self):
        """The tree's current arrays as one bytes-like object (cheap: the private block itself unless an array
        was rebound)."""
        if self._blob is not None:
            return self._blob
        return b"".join([np.ascontiguousarray(getattr(self, a)).tobytes() + b"|" for a in _ARRAYS])

    @staticmethod
    def fit(X0, W0, X1, W1, **kwargs):
        """Train a decision tree on the GPU as the reference does with scikit-learn's
        ``DecisionTreeClassifier(class_weight="balanced", **kwargs)`` (reference training.py:33-50).

        X0, X1 : float32 or uint8 ndarrays or device tensors (N, m, n, C): samples of class 0 and class 1 (uint8 is
            widened to float32, as sklearn does).  Anything else raises NotImplementedError; non-finite values raise
            ValueError.  At most 65536 samples and 65536 features (NotImplementedError beyond).
        W0, W1 : sample weights, finite and non-negative with a positive total per class (ValueError otherwise).
        max_depth : required, an int 1 .. 4 (a tree level is one launch group over at most 8 open nodes); None or a larger
            value raises NotImplementedError.
        min_samples_leaf (default 1), min_samples_split (default 2) : ints, as in sklearn; fractions raise
            NotImplementedError.
        criterion="gini", splitter="best" are accepted, random_state is accepted and ignored; any other keyword raises
            NotImplementedError.

        Returns a ``DTree`` with sklearn's arrays: nodes in pre-order (left first), float32 thresholds (a node routes with
        ``x <= threshold``), leaves with threshold -2 and children -1, and the reference's node predictions.

        Stated deviations from sklearn.  (1) Ties: among candidates of exactly equal proxy the smallest flat feature index
        wins, then the smallest position; sklearn visits the features in a random permutation and keeps the first strict
        improvement, so its pick among exact ties depends on ``random_state``.  (2) The balanced sample weights are turned
        into integers of 2^-k (k chosen so that their total stays below 2^62) and every sum of the split search is an
        integer sum, where sklearn accumulates float64: the result does not depend on the order of the samples or on the
        run, and equals sklearn's whenever the best split of every node leads by more than float64 rounding.
        """
        return fit_detail(X0, W0, X1, W1, **kwargs)[0]

    # ---- wire format (reference training.py:51-72, model.proto DTree)
    @staticmethod
    def from_proto(proto):
        ftr = np.array(proto.feature).reshape((-1, 3))
        ftr = [tuple(x) if x[0] >= 0 else None for x in ftr]
        return DTree(ftr, np.array(proto.threshold), np.array(proto.left), np.array(proto.right),
                     np.array(proto.prediction))

    def as_proto(self, proto):
        proto.Clear()
        # the reference tests `f is not None` on rows of a uint8 array, which is always true, so
        # leaves are written as 0,0,0 (never -1,-1,-1); kept for byte-compatible files
        proto.feature.extend(int(x) for x in self.feature.reshape(-1))
        proto.threshold.extend(float(x) for x in self.threshold)
        proto.left.extend(int(x) for x in self.left)
        proto.right.extend(int(x) for x in self.right)
        proto.prediction.extend(float(x) for x in self.prediction)

    # ---- evaluation
    def _device_arrays(self, dev):
        import torch
        key = (str(dev), bytes(self.content()))          # (an edited tree is uploaded again)
        cache = self.__dict__.setdefault("_dev", {})
        if key not in cache:
            cache.clear()
            cache[key] = tuple(torch.from_numpy(np.array(a)).to(dev) for a in
                               (self.feature, self.threshold, self.left, self.right, self.prediction))
        return cache[key]

    def predict_on_image(self, X, rs, cs) -> np.ndarray:
        """Leaf prediction for the windows with origins (rs[i], cs[i]) of channel image
        X[u,v,C] (reference training.py:84-96)."""
        import torch
        dev = nat.require_gpu()
        rs = np.asarray(rs)
        cs = np.asarray(cs)
        if rs.size == 0:
            return np.empty(0, np.float32)
        u, v, C = X.shape
        fmax = self.feature[self.node].max(axis=0) if self.node.any() else np.zeros(3, np.int64)
        if rs.min() < 0 or cs.min() < 0 or rs.max() + int(fmax[0]) >= u or cs.max() + int(fmax[1]) >= v or int(fmax[2]) >= C:
            raise IndexError("window feature outside the channel image")
        Xd, wb_dt = channel_tensor(X, dev)        # any dtype, compared as NumPy would (compare.py)
        rd = torch.from_numpy(rs.astype(np.int32)).to(dev)
        cd = torch.from_numpy(cs.astype(np.int32)).to(dev)
        out = torch.empty(rs.size, dtype=torch.float32, device=dev)
        f, t, l, r, p = self._device_arrays(dev)
        nat.launch("wb_tree_eval_launch", Xd, wb_dt, u, v, C, rd, cd, rs.size, f, t, l, r, p, self.left.size, out)
        return out.cpu().numpy()

    def apply(self, X):
        """Index of the leaf each sample X[i] (shape (m,n,C)) reaches (reference training.py:73-81)."""
        import torch
        dev = nat.require_gpu()
        N, m, n, C = X.shape
        if N == 0:
            return np.zeros(0, "i")
        fmax = self.feature[self.node].max(axis=0) if self.node.any() else np.zeros(3, np.int64)
        if int(fmax[0]) >= m or int(fmax[1]) >= n or int(fmax[2]) >= C:
            raise IndexError("tree feature outside the sample")
        Xd, wb_dt = channel_tensor(X, dev)
        out = torch.empty(N, dtype=torch.int32, device=dev)
        f, t, l, r, p = self._device_arrays(dev)
        nat.launch("wb_tree_apply_launch", Xd, wb_dt, N, m, n, C, f, t, l, r, self.left.size, out)
        return out.cpu().numpy().astype("i")

    def predict(self, X):
        """prediction[apply(X)] (reference training.py:82-83)."""
        return self.prediction[self.apply(X)]

    def depth(self):
        def d(n):
            return 0 if self.left[n] < 0 else 1 + max(d(int(self.left[n])), d(int(self.right[n])))
        return d(0)


_FIT_KEYS = ("max_depth", "min_samples_leaf", "min_samples_split", "criterion", "splitter", "random_state")


def _cart_check_samples(X, name):
    if not (isinstance(X, np.ndarray) or nat.is_tensor(X)) or nat.window_codes(X) is None:
        what = nat.dtype_name(X) if hasattr(X, "dtype") else type(X).__name__
        raise NotImplementedError(f"training.DTree.fit: no kernel for {what} samples ({name}); float32 or uint8 ndarrays or "
                                  "device tensors (N, m, n, C) are accepted")


def _cart_int(kwargs, key, default, least):
    v = kwargs.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise NotImplementedError(f"training.DTree.fit: {key} must be an int (fractions of the sample count are not built), got {v!r}")
    if v < least:
        raise ValueError(f"training.DTree.fit: {key} must be at least {least}, got {v}")
    return int(v)


def _cart_args(kwargs):
    unknown = sorted(set(kwargs) - set(_FIT_KEYS))
    if unknown:
        raise NotImplementedError(f"training.DTree.fit: no kernel for the arguments {unknown}; accepted: {list(_FIT_KEYS)}")
    if kwargs.get("criterion", "gini") != "gini" or kwargs.get("splitter", "best") != "best":
        raise NotImplementedError('training.DTree.fit: only criterion="gini" and splitter="best" are built')
    d = kwargs.get("max_depth")
    if d is None or isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= d <= MAX_DEPTH:
        raise NotImplementedError(f"training.DTree.fit: max_depth must be an int 1 .. {MAX_DEPTH} (a level of at most "
                                  f"{nat.WB_FIT_MAX_OPEN} open nodes per launch), got {d!r}; e.g. Learner(max_depth=2)")
    return int(d), _cart_int(kwargs, "min_samples_leaf", 1, 1), _cart_int(kwargs, "min_samples_split", 2, 2)


def cart_split_weights(W, Y):
    """(q, k): the balanced sample weights sw = W * (N / (2 * count(Y == y))) (sklearn's, on unweighted counts) as
    integers q = rint(sw * 2^k), uint64, k the power that keeps their total below 2^62."""
    N = Y.size
    counts = np.bincount(Y, minlength=2)
    with np.errstate(all="ignore"):
        sw = W.astype(np.float64) * (N / (2.0 * counts))[Y]
        total = math.fsum(sw) if np.all(np.isfinite(sw)) else np.inf
    if not np.isfinite(total) or total <= 0:
        raise ValueError("training.DTree.fit: the weights must have a finite positive total")
    k = min(61 - math.frexp(total)[1], 1000)
    q = np.rint(np.ldexp(sw, k)).astype(np.uint64)
    for c in (0, 1):
        if not int(q[Y == c].sum()) > 0:
            raise ValueError(f"training.DTree.fit: the weights of class {c} must have a positive total")
    return q, k


def fit_detail(X0, W0, X1, W1, **kwargs):
    """``DTree.fit`` with its working: returns (tree, info), info a dict with per node (pre-order id) ``samples`` (indices
    into the concatenated class-0, class-1 samples, ascending), ``depth``, ``T0``/``T1`` (the integer class totals),
    ``t0``/``t1`` (the same as float64), ``k`` (weights are integers of 2^-k), and for the nodes the GPU searched
    ``flat_feature`` (-1: a leaf), ``proxy``, ``p``, ``n_left``, ``lo``, ``hi`` as the kernel wrote them (NaN / 0 / -1
    for the others) and the float64 ``threshold``."""
    _cart_check_samples(X0, "X0")
    _cart_check_samples(X1, "X1")
    max_depth, min_leaf, min_split = _cart_args(kwargs)
    if len(X0.shape) != 4 or len(X1.shape) != 4:
        raise ValueError(f"X0 and X1 must have shape (N, m, n, C), got {tuple(X0.shape)}, {tuple(X1.shape)}")
    shape = tuple(int(s) for s in X0.shape[1:])
    if shape != tuple(int(s) for s in X1.shape[1:]):
        raise ValueError(f"X0 and X1 hold samples of different shapes: {shape}, {tuple(X1.shape[1:])}")
    n0, n1 = int(X0.shape[0]), int(X1.shape[0])
    N, F = n0 + n1, int(np.prod(shape))
    if n0 < 1 or n1 < 1 or F < 1:
        raise ValueError("training.DTree.fit: both classes need at least one sample")
    W = np.concatenate([check_weights(W0, n0, "W0"), check_weights(W1, n1, "W1")])
    Y = np.array([0] * n0 + [1] * n1)
    q, k = cart_split_weights(W, Y)
    scale = math.ldexp(1.0, -k)
    for X in (X0, X1):
        if isinstance(X, np.ndarray) and X.dtype.kind == "f" and not np.all(np.isfinite(X)):
            raise ValueError("training.DTree.fit: the samples must be finite")
    if N > nat.WB_CART_MAX_SAMPLES or F > nat.WB_CART_MAX_FEATURES:
        raise NotImplementedError(f"training.DTree.fit: at most {nat.WB_CART_MAX_SAMPLES} samples and {nat.WB_CART_MAX_FEATURES} "
                                  f"features, got {N} and {F}")

    def new_node(samples, depth, begin=0):
        y = Y[samples]
        T0, T1 = int(q[samples[y == 0]].sum()), int(q[samples[y == 1]].sum())
        return dict(samples=samples, depth=depth, begin=begin, T0=T0, T1=T1, t0=float(T0) * scale, t1=float(T1) * scale, feature=-1)

    def opens(nd):
        n, t0, t1 = nd["samples"].size, nd["t0"], nd["t1"]
        if nd["depth"] == max_depth:
            return False
        with np.errstate(all="ignore"):
            impurity = np.float64(1.0) - (np.float64(t0) * t0 + np.float64(t1) * t1) / ((np.float64(t0) + t1) * (np.float64(t0) + t1))
        return not (n < min_split or n < 2 * min_leaf or impurity <= np.finfo(np.float64).eps)

    def split(nd, s):
        nd.update(searched=True, proxy=float(s["proxy"]), p=int(s["n_left"]), n_left=int(s["n_left"]), lo=float(s["lo"]),
                  hi=float(s["hi"]), k_t0=float(s["t0"]), k_t1=float(s["t1"]))
        if s["feature"] < 0:
            return None
        lo, hi = np.float64(s["lo"]), np.float64(s["hi"])
        thr = lo / 2.0 + hi / 2.0
        if thr == hi or np.isinf(thr):
            thr = lo
        nd.update(feature=int(s["feature"]), threshold=float(thr))
        return dict(begin=nd["begin"]), dict(begin=nd["begin"] + int(s["n_left"]))

    nodes = grow(N, new_node, opens, _level_search(X0, X1, F, Y, q, scale, min_leaf), split)      # by the GPU's ids: level by level

    # sklearn's numbering: pre-order, left first (a parent's index is below its children's)
    pre = []

    def walk(g):
        pre.append(g)
        if nodes[g]["left"] >= 0:
            walk(nodes[g]["left"])
            walk(nodes[g]["right"])
    walk(0)
    index = {g: i for i, g in enumerate(pre)}
    n_nodes = len(pre)
    feature = [np.unravel_index(nodes[g]["feature"], shape) if nodes[g]["feature"] >= 0 else None for g in pre]
    threshold = np.array([nodes[g].get("threshold", -2.0) for g in pre], np.float64)
    left = np.array([index.get(nodes[g]["left"], -1) for g in pre])
    right = np.array([index.get(nodes[g]["right"], -1) for g in pre])
    # the node predictions: the reference's expressions (training.py:43-49) on the leaf each sample reached
    leaf = np.empty(N, np.int64)
    for g in pre:
        if nodes[g]["left"] < 0:
            leaf[nodes[g]["samples"]] = index[g]
    pred = np.empty(n_nodes)
    for n in range(n_nodes):
        mask = leaf == n
        w0 = (W * mask * (Y == 0)).sum() + 1e-3
        w1 = (W * mask * (Y == 1)).sum() + 1e-3
        pred[n] = np.log(w1 / w0) / 2
    col = lambda key, default, dt: np.array([nodes[g].get(key, default) for g in pre], dt)
    info = dict(samples=[nodes[g]["samples"] for g in pre], depth=col("depth", 0, np.int64), k=k,
                T0=[nodes[g]["T0"] for g in pre], T1=[nodes[g]["T1"] for g in pre],
                t0=col("t0", np.nan, np.float64), t1=col("t1", np.nan, np.float64),
                kernel_t0=col("k_t0", np.nan, np.float64), kernel_t1=col("k_t1", np.nan, np.float64),
                searched=col("searched", False, bool), flat_feature=col("feature", -1, np.int64),
                proxy=col("proxy", np.nan, np.float64), p=col("p", 0, np.int64), n_left=col("n_left", 0, np.int64),
                lo=col("lo", np.nan, np.float32), hi=col("hi", np.nan, np.float32), threshold=threshold)
    return DTree(feature, threshold, left, right, pred), info


def _level_search(X0, X1, F, Y, q, scale, min_leaf):
    """The level search of ``fit_detail`` on the GPU (csrc/wb_cart.hip), for ``_grow.grow``: stages the samples, sorts every
    column once, and per level launches the scan, the pick, the routing and the re-partitioning of the sorted columns."""
    import torch
    dev = nat.require_gpu()
    N = Y.size
    xt, q_d, cls_d, node_d = stage(X0, X1, F, torch.float32, q, Y, dev)
    if not bool(torch.isfinite(xt).all()):
        raise ValueError("training.DTree.fit: the samples must be finite")
    orders = [torch.empty((F, N), dtype=torch.int32, device=dev) for _ in range(2)]        # sorted by value within each node: in, out
    nat.launch("wb_cart_sort_launch", xt, N, F, orders[0])
    hp = lambda values, dt: np.array(values, dt).ctypes.data_as(C.c_void_p)

    def search(depth, level, opened, child_base):
        n_open = len(opened)
        scratch = torch.empty(nat.query("wb_cart_scratch_bytes", F, n_open), dtype=torch.uint8, device=dev)
        splits_d = torch.empty(n_open * nat.CART_SPLIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        nat.launch("wb_cart_level_launch", xt, N, F, q_d, cls_d, orders[0], orders[1], node_d, n_open,
                   hp([nd["begin"] for nd in opened], np.int32), hp([nd["begin"] + nd["samples"].size for nd in opened], np.int32),
                   hp([nd["T0"] for nd in opened], np.uint64), hp([nd["T1"] for nd in opened], np.uint64), scale, min_leaf, child_base,
                   scratch, scratch.numel(), splits_d)
        orders.reverse()
        return splits_d.cpu().numpy().view(nat.CART_SPLIT_DTYPE), node_d.cpu().numpy()
    return search


def loss(H0, H1):
    """Exponential loss of the two score sets (reference training.py:99-102)."""
    W0 = weights(H0)
    W1 = weights(-H1)
    return W0.mean() + W1.mean()


class Learner:
    """Training algorithm (reference training.py:105-188): fits one weak classifier and one rejection threshold per
    stage and keeps the per-stage pass rates and losses.  The default ``wh`` is ``training.DTree``, whose ``fit`` needs a
    ``max_depth`` of 1 .. 4 among the ``wh_args`` (``Learner(max_depth=2)``); ``fpga.train`` passes ``fpga.DTree``."""

    def __init__(self, alpha=0.1, wh=DTree, **wh_args):
        self.alpha = alpha
        self.wh = wh
        self.wh_args = wh_args
        self.p0 = []
        self.p1 = []
        self.losses = []

    @staticmethod
    def from_dict(d):
        L = Learner(alpha=d["alpha"], wh=d["wh"], **d["wh_args"])
        L.p0 = d["p0"]
        L.p1 = d["p1"]
        L.losses = d["losses"]
        if len(L.p0) != len(L.losses) or len(L.p1) != len(L.losses):
            raise ValueError("Wrong values for p0, p1 or loss")
        return L

    def save(self, filename):
        with open(filename, "wb") as f:
            pickle.dump(self.__dict__, f)

    @staticmethod
    def load(filename):
        with open(filename, "rb") as f:
            return Learner.from_dict(pickle.load(f))

    @property
    def false_positive_rate(self):
        return np.prod(self.p0)

    @property
    def true_positive_rate(self):
        return np.prod(self.p1)

    @property
    def loss(self):
        return self.losses[-1] if self.losses else None

    def __len__(self):
        return len(self.losses)

    def __bool__(self):
        return True

    def get_stats(self):
        return {
            "false_positive_rate": np.cumprod(self.p0),
            "true_positive_rate": np.cumprod(self.p1),
            "loss": np.array(self.losses),
        }

    def fit_stage(self, model, X0, H0, X1, H1, theta=None, **wh_args):
        """Append a new stage to the model: returns (loss, false positive rate, true positive rate)."""
        W0 = weights(H0)
        W1 = weights(-H1)
        weak = self.wh.fit(X0, W0, X1, W1, **{**self.wh_args, **wh_args})
        H0 = H0 + weak.predict(X0)
        H1 = H1 + weak.predict(X1)
        if not theta:       # (None -- and 0.0, as in the reference -- means: estimate it)
            theta = fit_rejection_threshold(H0, self.false_positive_rate, H1, self.true_positive_rate, self.alpha)
        p0 = (H0 >= theta).sum() / H0.size
        p1 = (H1 >= theta).sum() / H1.size
        self.p0.append(p0)
        self.p1.append(p1)
        self.losses.append(loss(H0, H1))
        model.append(weak, theta)
        return self.loss, self.false_positive_rate, self.true_positive_rate


def fit_rejection_threshold(H0, P0, H1, P1, alpha):
    """Rejection threshold by the SPRT (reference training.py:191-220): the largest candidate t (a response that
    occurs, the smallest excepted) whose likelihood ratio R(t) exceeds 1/alpha.  The reference's loop over candidates
    is two ``searchsorted`` calls here: the counts `(H < t).sum()` are integers, so R is the same float for float."""
    max0 = np.max(H0)
    min1 = np.min(H1)
    if max0 < min1:
        logger.log(15, f"H0 and H1 are non-overlapping H0 < {max0}, H1 > {min1}")
        return min1
    ts = np.unique(np.concatenate([H0.flatten(), H1.flatten()]))
    if ts.size < 3:
        logger.log(15, f"Not enough unique responses to estimate theta (forcing to {-np.inf})")
        return -np.inf
    ts = ts[1:]
    logger.log(15, f"Testing {ts.size} thresholds on interval <{min(ts):.2f},{max(ts):.2f}>")
    p0 = np.searchsorted(np.sort(H0.flatten()), ts, side="left") / H0.size
    p1 = np.searchsorted(np.sort(H1.flatten()), ts, side="left") / H1.size
    R = ((P0 * p0 + (1 - P0) + 1e-6) / (P1 * p1 + (1 - P1) + 1e-6)).astype(ts.dtype)   # (the reference fills an empty_like(ts))
    A = 1 / alpha
    logger.log(15, f"R: <{min(R):.2f},{max(R):.2f}>; need R > {A}")
    idx = np.nonzero(R > A)[0]
    if idx.size == 0:
        logger.log(15, "No suitable theta found")
        theta = -np.inf
    else:
        theta = ts[np.max(idx)]
    logger.log(15, f"theta = {theta:.4f}")
    return theta


class BasicRejectionSchedule:
    """Which stages learn a rejection threshold (reference training.py:223-253): called with (stage, p0) it returns
    -inf outside ``rejection_interval`` = (first, last) stage or once the false positive rate p0 has fallen below
    ``target_p0``, and None (estimate theta from the data) otherwise."""

    def __init__(self, rejection_interval=(0, None), target_p0=1e-5):
        if rejection_interval is None:
            rejection_interval = (None, None)
        self.s0 = rejection_interval[0] or 0
        self.s1 = rejection_interval[1] or np.inf
        self.target_p0 = target_p0

    def __call__(self, stage, p0):
        if stage < self.s0 or stage > self.s1 or p0 < self.target_p0:
            return -np.inf
        return None
