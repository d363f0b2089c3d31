"""Minimal stand-in for the third-party ``bbx.Boxes`` container the reference returns
(call sites: reference model.py:139,147,177,179 and __init__.py:126-130).

``bbx`` is not vendored upstream and is absent here; only the members those call sites (and
the docstring example at model.py:166-171) use are provided.  Parity at this boundary is
unpinned upstream.
"""
from typing import NamedTuple

import numpy as np


class Boxes:
    def __init__(self, coords, **fields):
        self._c = np.asarray(coords).reshape(-1, 4)
        self._fields = {k: np.asarray(v) for k, v in fields.items()}

    def get(self):
        """(N,4) array of [xmin, ymin, xmax, ymax]."""
        return self._c

    def set_field(self, name, value):
        value = np.asarray(value)
        if value.shape[0] != len(self):
            raise ValueError(f"field {name!r} has {value.shape[0]} rows, boxes have {len(self)}")
        self._fields[name] = value

    def add_field(self, name, value):
        """As set_field (bbx exposes both; reference samples.py:157 adds 'regression_target' with it)."""
        self.set_field(name, value)

    def get_field(self, name):
        return self._fields[name]

    def has_field(self, name):
        return name in self._fields

    def fields(self):
        return list(self._fields)

    def normalized(self, scale=1.0):
        return Boxes((self._c * np.float32(scale)).astype(self._c.dtype), **self._fields)

    def area(self):
        """(x2 - x1) * (y2 - y1) per box, float64 (stand-in for ``bbx.Boxes.area``, reference testing.py:42; bbx is absent here
        and this boundary is unpinned upstream)."""
        c = np.asarray(self._c, np.float64)
        return (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])

    def __len__(self):
        return self._c.shape[0]

    def __getitem__(self, idx):
        if isinstance(idx, (int, np.integer)):
            idx = [idx]
        return Boxes(self._c[idx], **{k: v[idx] for k, v in self._fields.items()})

    def __repr__(self):
        return f"Boxes(n={len(self)}, fields={self.fields()})"


def concatenate(boxes, fields=None):
    boxes = list(boxes)
    if not boxes:
        return Boxes(np.empty((0, 4), "f"))
    names = list(boxes[0].fields()) if fields is None else list(fields)
    out = Boxes(np.concatenate([b.get() for b in boxes]))
    for n in names:
        out._fields[n] = np.concatenate([b.get_field(n) for b in boxes])
    return out


def iou(a, b):
    """Pairwise intersection-over-union of two box lists -> (len(a), len(b)) float array
    (stand-in for ``bbx.iou``, reference samples.py:133; areas are (x2-x1)*(y2-y1))."""
    A = np.asarray(a.get(), np.float64).reshape(-1, 4)
    B = np.asarray(b.get(), np.float64).reshape(-1, 4)
    iw = np.clip(np.minimum(A[:, None, 2], B[None, :, 2]) - np.maximum(A[:, None, 0], B[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(A[:, None, 3], B[None, :, 3]) - np.maximum(A[:, None, 1], B[None, :, 1]), 0, None)
    inter = iw * ih
    area_a = ((A[:, 2] - A[:, 0]) * (A[:, 3] - A[:, 1]))[:, None]
    area_b = ((B[:, 2] - B[:, 0]) * (B[:, 3] - B[:, 1]))[None, :]
    union = area_a + area_b - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


def boxes_in_window(boxes, window, min_overlap=1):
    """bool [N]: the part of each box inside the single box `window` is at least `min_overlap` of the box's own area --
    ``inter >= min_overlap * area``, inter the clipped intersection, float64 host arithmetic (so a box that exactly fills the
    window passes at 1, and so does a box of no area).  Stand-in for ``bbx.boxes_in_window`` (reference testing.py:43); bbx is
    absent here and this boundary is unpinned upstream."""
    w = np.asarray(window.get() if isinstance(window, Boxes) else window, np.float64).reshape(-1)
    if w.size != 4:
        raise ValueError("boxes_in_window takes ONE window box")
    c = np.asarray(boxes.get(), np.float64).reshape(-1, 4)
    iw = np.clip(np.minimum(c[:, 2], w[2]) - np.maximum(c[:, 0], w[0]), 0, None)
    ih = np.clip(np.minimum(c[:, 3], w[3]) - np.maximum(c[:, 1], w[1]), 0, None)
    return iw * ih >= min_overlap * boxes.area()


def set_aspect_ratio(boxes, ar):
    """Boxes of the same centres and areas whose width / height is `ar`: ``w' = sqrt(area * ar)``, ``h' = sqrt(area / ar)``,
    float64 host arithmetic; every field is carried over.  Stand-in for ``bbx.set_aspect_ratio`` (reference testing.py:50-51);
    bbx is absent here and this boundary is unpinned upstream."""
    ar = float(ar)
    if not ar > 0 or not np.isfinite(ar):
        raise ValueError("aspect ratio must be a positive number")
    c = np.asarray(boxes.get(), np.float64).reshape(-1, 4)
    cx, cy = (c[:, 0] + c[:, 2]) / 2, (c[:, 1] + c[:, 3]) / 2
    area = boxes.area()
    w, h = np.sqrt(area * ar), np.sqrt(area / ar)
    return Boxes(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), **{k: boxes.get_field(k) for k in boxes.fields()})


_MATCH_COORD_MAX = 2.0 ** 500   # coordinates below it: no difference, product or sum of match_boxes' arithmetic overflows


def _match_coords(b, what):
    c = np.ascontiguousarray(np.asarray(b.get(), np.float64).reshape(-1, 4))
    if not (np.abs(c) < _MATCH_COORD_MAX).all():               # (a NaN fails the comparison too)
        raise ValueError(f"match_boxes: {what} coordinates must be finite and below 2**500 in magnitude")
    return c


def match_boxes(dt_boxes, gt_boxes_per_image, dt_image=None):
    """(best float64 [N], owner int32 [N]): for every detection the largest ``iou`` over the ground-truth boxes of its image
    and the index, inside that image's list, of the FIRST box that reaches it (``np.argmax``: a detection that overlaps nothing
    is owned by box 0); an image without ground truth gives best 0, owner -1.

    dt_boxes, gt_boxes_per_image: one pair of Boxes -- or the detections of a whole data set in one Boxes, ``dt_image`` the
    image ordinal of each, and a list with every image's ground-truth Boxes.  Coordinates are converted to float64 as `iou`
    does (ground truth need not hold float32 values); all of them must be finite and below 2**500 in magnitude, so that no
    product can overflow into a NaN (ValueError).

    Runs on the GPU (wb_match_launch): one upload, one launch, one read-back; like everything in this package it has no CPU
    fallback and raises NativeError without a GPU.  No detections: empty arrays, without touching the device."""
    if isinstance(gt_boxes_per_image, Boxes):
        if dt_image is not None:
            raise ValueError("match_boxes: dt_image goes with a LIST of ground-truth Boxes")
        gts = [gt_boxes_per_image]
        image = np.zeros(len(dt_boxes), np.int32)
    else:
        gts = list(gt_boxes_per_image)
        if dt_image is None:
            raise ValueError("match_boxes: a list of ground-truth Boxes needs dt_image")
        image = np.asarray(dt_image).reshape(-1)
        if image.size != len(dt_boxes):
            raise ValueError(f"match_boxes: {image.size} dt_image entries, {len(dt_boxes)} detections")
        if image.size and (image.dtype.kind not in "iu" or image.min() < 0 or image.max() >= len(gts)):
            raise ValueError(f"match_boxes: dt_image must hold integers in [0, {len(gts)})")
        image = image.astype(np.int32)
    dt = _match_coords(dt_boxes, "detection")
    gt = [_match_coords(g, "ground-truth") for g in gts]
    n = dt.shape[0]
    if n == 0:
        return np.zeros(0, np.float64), np.zeros(0, np.int32)
    off = np.zeros(len(gt) + 1, np.int64)
    np.cumsum([g.shape[0] for g in gt], out=off[1:])
    n_gt = int(off[-1])
    if n_gt >= 1 << 31:
        raise ValueError("match_boxes: at most 2**31 - 1 ground-truth boxes")
    from . import _native as nat
    dev = nat.require_gpu()
    inp = nat.Block.upload(dev, dt=dt, gt=np.concatenate(gt), image=image, gt_off=off.astype(np.int32))
    out = nat.Block.empty(dev, best=(n, np.float64), owner=(n, np.int32))
    nat.launch("wb_match_launch", inp.ptr["dt"], inp.ptr["image"], inp.ptr["gt"], inp.ptr["gt_off"], n, n_gt, len(gt), out.ptr["best"],
               out.ptr["owner"])
    h = out.host()
    return h["best"].copy(), h["owner"].copy()


_NMS_RANK_MAX = 1 << 16      # most boxes wb_nms_launch orders itself (a quadratic pass); above: torch.sort + wb_nms_ordered_launch
VOTE_WEIGHTS = ("uniform", "score")      # WB_VOTE_UNIFORM, WB_VOTE_SCORE


class Suppression(NamedTuple):
    """The checked scalar arguments of non-maximum suppression and box voting; `suppression` makes it."""
    iou_threshold: float
    score_threshold: float = None        # a float32 value as a Python float; None: no box is dropped by its score
    vote: tuple = None                   # (vote_iou, index into VOTE_WEIGHTS, min_votes); None: no box voting

    @property
    def threshold_args(self):
        """(use_score_threshold, score_threshold) as the launch functions take them."""
        return (0, 0.0) if self.score_threshold is None else (1, self.score_threshold)


def suppression(iou_threshold, score_threshold=None, vote_iou=None, weights="uniform", min_votes=1):
    """The Suppression of these arguments -- every rule about them is here and nowhere else -- or None for iou_threshold
    None: the plain detect call, which takes neither of the other thresholds.  vote_iou None: no voting (`weights` and
    `min_votes` are not looked at then).  ValueError for anything else that is not a suppression."""
    if iou_threshold is None:
        if score_threshold is not None:
            raise ValueError("score_threshold is part of non-maximum suppression: give an iou_threshold too (1.0 suppresses nothing)")
        if vote_iou is not None:
            raise ValueError("vote_iou merges what non-maximum suppression keeps: give an iou_threshold too")
        return None
    iou_threshold = float(iou_threshold)
    if not iou_threshold >= 0.0:
        raise ValueError("iou_threshold must be a number >= 0")
    if score_threshold is not None:
        score_threshold = float(np.float32(score_threshold))
        if score_threshold != score_threshold:
            raise ValueError("score_threshold is NaN")
    if vote_iou is None:
        return Suppression(iou_threshold, score_threshold)
    vote_iou = float(vote_iou)
    if not vote_iou >= 0.0:
        raise ValueError("vote_iou must be a number >= 0")
    if weights not in VOTE_WEIGHTS:
        raise ValueError(f"vote weights must be one of {VOTE_WEIGHTS}, not {weights!r}")
    if weights == "score" and score_threshold is None:
        raise ValueError('"score" vote weights are measured from the score threshold: give a score_threshold')
    if int(min_votes) != min_votes or min_votes < 0:
        raise ValueError("min_votes must be an integer >= 0")
    return Suppression(iou_threshold, score_threshold, (vote_iou, VOTE_WEIGHTS.index(weights), int(min_votes)))


def _checked_arrays(boxes, scores, group, voting=False):
    """The checked arrays of a suppression: (boxes float32 [n][4], scores float32 [n], group int32 [n] or None)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    n = scores.size
    if boxes.shape[0] != n:
        raise ValueError(f"{boxes.shape[0]} boxes, {n} scores")
    if group is not None:
        group = np.asarray(group).reshape(-1)
        if group.size != n:
            raise ValueError(f"{group.size} group entries, {n} boxes")
        group = np.unique(group, return_inverse=True)[1].astype(np.int32).reshape(-1)     # (any dtype: equality is all that counts)
    if voting and not np.isfinite(boxes).all():
        raise ValueError("box voting: coordinates must be finite")
    if voting and np.isnan(scores).any():
        raise ValueError("box voting: scores must not be NaN")
    return boxes, scores, group


class _DeviceBoxes:
    """n > 0 checked boxes on the device -- ONE upload of boxes | scores | group | keep, the absent ones left out -- with the
    launches that work on them and the ONE block their results come back in: merged | votes with `vote`, then n_keep | keep
    unless the keep flags were given."""

    def __init__(self, boxes, scores, group, keep=None, vote=False):
        from . import _native as nat
        self.dev, self.n, n = nat.require_gpu(), scores.size, scores.size
        given = dict(boxes=boxes, scores=scores, group=group, keep=keep)
        self.inp = nat.Block.upload(self.dev, **{k: v for k, v in given.items() if v is not None})
        specs = dict(merged=((n, 4), np.float32), votes=(n, np.int32)) if vote else {}
        if keep is None:
            specs.update(n_keep=(1, np.uint32), keep=(n, np.uint8))
        self.out = nat.Block.empty(self.dev, **specs)

    def nms(self, how):
        """Greedy NMS into out's n_keep and keep, enqueued on the current stream."""
        import torch
        from . import _native as nat
        at, n = self.inp.ptr, self.n
        scratch = torch.empty(nat.query("wb_nms_scratch_bytes", n), dtype=torch.uint8, device=self.dev)
        tail = (n, how.iou_threshold, *how.threshold_args, scratch, scratch.numel(), self.out.ptr["keep"], self.out.ptr["n_keep"])
        if n <= _NMS_RANK_MAX:
            nat.launch("wb_nms_launch", at["boxes"], at["scores"], at.get("group"), *tail)
        else:
            # descending, the two zeros one value (-(s + 0) is -0.0 for both), equal scores in input order
            order = torch.sort(-(self.inp.tensor("scores") + 0.0), stable=True).indices.to(torch.int32)
            nat.launch("wb_nms_ordered_launch", at["boxes"], at["scores"], at.get("group"), order, *tail)

    def vote(self, how):
        """wb_vote_launch into out's merged and votes, on the keep flags that were given or that nms left, on the current stream."""
        from . import _native as nat
        at, out, (vote_iou, code, _) = self.inp.ptr, self.out.ptr, how.vote
        nat.launch("wb_vote_launch", at["boxes"], at["scores"], at.get("group"), at.get("keep", out.get("keep")), self.n, vote_iou, code,
                   *how.threshold_args, out["merged"], out["votes"])

    def flags(self, h):
        """The keep flags (bool [n]) of the read-back `h` of out."""
        keep = h["keep"].astype(bool)
        assert int(h["n_keep"][0]) == int(keep.sum())
        return keep


def _keep_mask(boxes, scores, how, group=None):
    """nms_keep_mask of a Suppression."""
    boxes, scores, group = _checked_arrays(boxes, scores, group)
    if scores.size == 0:
        return np.zeros(0, bool)
    d = _DeviceBoxes(boxes, scores, group)
    d.nms(how)
    return d.flags(d.out.host())


def nms_keep_mask(boxes, scores, iou_threshold=0.5, score_threshold=None, group=None):
    """Keep flags (bool [N], input order) of greedy non-maximum suppression, computed on the GPU (wb_nms_launch): the
    arrays go up in one upload, the flags come back in one read-back.  See non_max_suppression for the semantics.  More than
    2**16 boxes are put in visiting order by a stable torch.sort on the device and go through wb_nms_ordered_launch: every N
    a detect call can return (2**26) is accepted; the cost grows with N * N (include/waldboost_hip.h has the figures)."""
    return _keep_mask(boxes, scores, suppression(float(iou_threshold), score_threshold), group)


def finish(boxes, how, group=None):
    """The tail of every detect call and the body of non_max_suppression and merge_detections: the Boxes `boxes` (with
    'scores') after the Suppression `how` -- None: `boxes` itself; without a vote: what non_max_suppression returns; with
    one: what merge_detections returns.  One upload, the launches on the same device arrays, one read-back."""
    if how is None:
        return boxes
    if not boxes.has_field("scores"):
        raise ValueError("suppression needs a 'scores' field")
    voting = how.vote is not None
    b, s, g = _checked_arrays(boxes.get(), boxes.get_field("scores"), group, voting)
    if s.size == 0:
        out = boxes[np.zeros(0, np.intp)]
        if voting:
            out.set_field("votes", np.zeros(0, np.int32))
        return out
    d = _DeviceBoxes(b, s, g, vote=voting)
    d.nms(how)
    if not voting:
        return boxes[np.flatnonzero(d.flags(d.out.host()))]
    d.vote(how)
    h = d.out.host()
    idx = np.flatnonzero(d.flags(h) & (h["votes"] >= how.vote[-1]))             # (min_votes)
    kept = boxes[idx]
    out = Boxes(h["merged"][idx], **{k: kept.get_field(k) for k in kept.fields()})
    out.set_field("votes", h["votes"][idx])
    return out


def non_max_suppression(boxes, iou_threshold=0.5, score_threshold=None, group=None):
    """Greedy non-maximum suppression of a Boxes with a 'scores' field (stand-in for ``bbx.non_max_suppression``,
    reference testing.py:46; the detection script asks for it as detect(..., iou_threshold=, score_threshold=)).

    Boxes with ``not (score >= float32(score_threshold))`` are dropped first.  The rest is visited by score, highest
    first (-0.0 equals +0.0; of equal scores the one EARLIER in the input goes first: ``np.argsort(-scores,
    kind="stable")``); a box is kept unless an already kept box of the same group (``group``: one integer per box;
    None: one group) overlaps it with ``iou(...) > iou_threshold`` -- strict, `iou` being this module's float64
    function.  Returns the kept boxes in their input order, every field sliced.  Scores must not be NaN.

    Runs on the GPU (wb_nms_launch; above 2**16 boxes torch.sort + wb_nms_ordered_launch); like everything in this package it has no CPU fallback and
    raises NativeError without a GPU.  An empty Boxes is returned as an empty Boxes without touching the device."""
    return finish(boxes, suppression(float(iou_threshold), score_threshold), group)


def vote_boxes(boxes, scores, keep, vote_iou=0.5, weights="uniform", score_threshold=None, group=None):
    """Box voting: (merged float32 [N][4], votes int32 [N]).  Every box that `keep` (uint8 / bool [N], as nms_keep_mask
    answers) marks becomes the weighted mean of its VOTERS and `votes` counts them; a row that is not kept holds its own box
    and 0 votes.

    A box is live unless ``not (score >= float32(score_threshold))`` -- the boxes NMS dropped first.  Box j votes for the
    kept box k when j is k itself (always), or when j is live, of k's group and ``iou(box_k, box_j) >= vote_iou`` (`iou`
    being this module's float64 function).  weights: "uniform", every voter counts 1; "score", a voter counts
    ``float64(score) - float64(float32(score_threshold))`` (needs a score_threshold).  The sums are float64 in a fixed order
    (include/waldboost_hip.h, wb_vote_launch; tests/vote_reference.py states the whole rule in NumPy), so the result is the
    same bits on every run.  When the weights sum to 0 (every voter exactly at the threshold) a kept box stays as it is.

    Runs on the GPU (wb_vote_launch: K * N IoU tests for K kept boxes): one upload, one launch, one read-back; no CPU
    fallback.  Coordinates must be finite, scores not NaN (ValueError, like every bad argument, before the device is
    touched).  An empty input returns empty arrays without touching the device."""
    how = suppression(0.0, score_threshold, vote_iou, weights)
    boxes, scores, group = _checked_arrays(boxes, scores, group, voting=True)
    keep = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, np.uint8)
    if keep.size != scores.size:
        raise ValueError(f"{keep.size} keep flags, {scores.size} boxes")
    if scores.size == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int32)
    d = _DeviceBoxes(boxes, scores, group, keep, vote=True)
    d.vote(how)
    h = d.out.host()
    return h["merged"].copy(), h["votes"].copy()


def merge_detections(boxes, iou_threshold=0.5, score_threshold=None, group=None, vote_iou=0.5, weights="uniform", min_votes=1):
    """Greedy non-maximum suppression of a Boxes with a 'scores' field, exactly as non_max_suppression does it, and then box
    voting (vote_boxes has the rule): every kept box is replaced by the weighted mean of the boxes of its cluster -- itself
    and the live boxes of its group with ``iou >= vote_iou`` to it -- so the suppressed windows still say where the object is.

    Returns the kept boxes in input order, every field sliced; the coordinates are the merged ones; 'scores' is unchanged (it
    is the score of the cluster's mode); a new int32 field 'votes' counts each box's voters (>= 1).  Kept boxes with
    ``votes < min_votes`` are left out (an isolated firing is more often a false alarm than a cluster is); NMS is NOT run
    again after that, so a box such a kept box had suppressed does not come back.

    Runs on the GPU: one upload, the NMS launches and wb_vote_launch on the same device arrays, one read-back of flags, boxes
    and votes out of one block; no CPU fallback.  Bad arguments raise ValueError before the device is touched.  An empty Boxes
    is returned as an empty Boxes (with a 'votes' field) without touching the device."""
    return finish(boxes, suppression(float(iou_threshold), score_threshold, vote_iou, weights, min_votes), group)
