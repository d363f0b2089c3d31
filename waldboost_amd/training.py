"""``DTree`` -- the weak classifier of the cascade (reference training.py:23-96) -- and the stage
learner around it (reference training.py:14-20, 99-253).

Same constructor, attributes, proto I/O and ``predict_on_image``/``apply``/``predict``
signatures as the reference so that ``from waldboost_amd.training import DTree`` is a drop-in;
the evaluation runs in a HIP kernel (csrc/wb_cascade.hip: tree_eval_kernel).  ``DTree.fit``
(sklearn training, reference training.py:33-50) is out of scope of this build: the weak learner
that trains here is ``waldboost_amd.fpga.DTree`` (csrc/wb_fit.hip).

``Learner``, ``fit_rejection_threshold``, ``BasicRejectionSchedule``, ``weights``, ``loss`` and
``as_features`` are the reference's host arithmetic on a pool's scores; ``Learner.fit_stage`` calls
``wh.fit`` and ``weak.predict``, which run on the GPU.
"""
import logging
import pickle

import numpy as np

from . import _native as nat
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
    def fit(*args, **kwargs):
        raise NotImplementedError("training.DTree.fit (the sklearn learner) has no kernel in this build; "
                                  "waldboost_amd.fpga.DTree.fit trains on the GPU")

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
        lib = nat.load()
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
        nat.check(lib.wb_tree_eval_launch(nat.stream_ptr(), nat.ptr(Xd), wb_dt, u, v, C, nat.ptr(rd), nat.ptr(cd), rs.size,
                                          nat.ptr(f), nat.ptr(t), nat.ptr(l), nat.ptr(r), nat.ptr(p),
                                          self.left.size, nat.ptr(out)), "wb_tree_eval_launch")
        return out.cpu().numpy()

    def apply(self, X):
        """Index of the leaf each sample X[i] (shape (m,n,C)) reaches (reference training.py:73-81)."""
        import torch
        lib = nat.load()
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
        nat.check(lib.wb_tree_apply_launch(nat.stream_ptr(), nat.ptr(Xd), wb_dt, N, m, n, C, nat.ptr(f), nat.ptr(t),
                                           nat.ptr(l), nat.ptr(r), self.left.size, nat.ptr(out)), "wb_tree_apply_launch")
        return out.cpu().numpy().astype("i")

    def predict(self, X):
        """prediction[apply(X)] (reference training.py:82-83)."""
        return self.prediction[self.apply(X)]

    def depth(self):
        def d(n):
            return 0 if self.left[n] < 0 else 1 + max(d(int(self.left[n])), d(int(self.right[n])))
        return d(0)


def loss(H0, H1):
    """Exponential loss of the two score sets (reference training.py:99-102)."""
    W0 = weights(H0)
    W1 = weights(-H1)
    return W0.mean() + W1.mean()


class Learner:
    """Training algorithm (reference training.py:105-188): fits one weak classifier and one rejection threshold per
    stage and keeps the per-stage pass rates and losses.  The default ``wh`` is ``training.DTree``, whose ``fit`` is not
    part of this build; ``fpga.train`` passes ``fpga.DTree``."""

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
