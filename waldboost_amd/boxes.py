"""Minimal stand-in for the third-party ``bbx.Boxes`` container the reference returns
(call sites: reference model.py:139,147,177,179 and __init__.py:126-130).

``bbx`` is not vendored upstream and is absent here; only the members those call sites (and
the docstring example at model.py:166-171) use are provided.  Parity at this boundary is
unpinned upstream.
"""
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
    import ctypes as C
    import torch
    from . import _native as nat
    lib = nat.load()
    dev = nat.require_gpu()
    # one upload: detections | ground truth | dt_image | gt_off (the doubles first: everything stays aligned)
    parts = [dt.reshape(-1).view(np.uint8)] + [g.reshape(-1).view(np.uint8) for g in gt]
    parts += [image.view(np.uint8), off.astype(np.int32).view(np.uint8)]
    d_in = torch.from_numpy(np.concatenate(parts)).to(dev)
    d_out = torch.empty(12 * n, dtype=torch.uint8, device=dev)         # best | owner: one read-back
    at = lambda t, o: C.c_void_p(t.data_ptr() + o)
    o_gt, o_img = 32 * n, 32 * (n + n_gt)
    nat.check(lib.wb_match_launch(nat.stream_ptr(), at(d_in, 0), at(d_in, o_img), at(d_in, o_gt), at(d_in, o_img + 4 * n), n, n_gt,
                                  len(gt), at(d_out, 0), at(d_out, 8 * n)), "wb_match_launch")
    h = d_out.cpu().numpy()
    return h[:8 * n].view(np.float64).copy(), h[8 * n:].view(np.int32).copy()


_NMS_RANK_MAX = 1 << 16      # most boxes wb_nms_launch orders itself (a quadratic pass); above: torch.sort + wb_nms_ordered_launch


def _nms_inputs(boxes, scores, iou_threshold, score_threshold, group):
    """The checked arguments of an NMS call: (boxes float32 [n][4], scores float32 [n], iou_threshold, group int32 [n] or None)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    n = scores.size
    if boxes.shape[0] != n:
        raise ValueError(f"{boxes.shape[0]} boxes, {n} scores")
    iou_threshold = float(iou_threshold)
    if not iou_threshold >= 0.0:
        raise ValueError("iou_threshold must be a number >= 0")
    if score_threshold is not None and np.isnan(np.float32(score_threshold)):
        raise ValueError("score_threshold is NaN")
    if group is not None:
        group = np.asarray(group).reshape(-1)
        if group.size != n:
            raise ValueError(f"{group.size} group entries, {n} boxes")
        group = np.unique(group, return_inverse=True)[1].astype(np.int32).reshape(-1)     # (any dtype: equality is all that counts)
    return boxes, scores, iou_threshold, group


def _nms_enqueue(lib, dev, p_boxes, d_scores, p_group, n, iou_threshold, score_threshold):
    """Greedy NMS of n > 0 boxes that lie on the device already (p_boxes, p_group: device pointers, the group's may be
    null; d_scores: a float32 tensor), enqueued on the current stream: the device bytes n_keep (uint32) | keep flags [n]."""
    import ctypes as C
    import torch
    from . import _native as nat
    need = C.c_size_t()
    nat.check(lib.wb_nms_scratch_bytes(n, C.byref(need)), "wb_nms_scratch_bytes")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.empty(4 + n, dtype=torch.uint8, device=dev)           # n_keep | keep flags: one read-back
    tail = (n, iou_threshold, 0 if score_threshold is None else 1, 0.0 if score_threshold is None else float(np.float32(score_threshold)),
            nat.ptr(scratch), scratch.numel(), C.c_void_p(out.data_ptr() + 4), nat.ptr(out))
    if n <= _NMS_RANK_MAX:
        nat.check(lib.wb_nms_launch(nat.stream_ptr(), p_boxes, nat.ptr(d_scores), p_group, *tail), "wb_nms_launch")
    else:
        # descending, the two zeros one value (-(s + 0) is -0.0 for both), equal scores in input order
        order = torch.sort(-(d_scores + 0.0), stable=True).indices.to(torch.int32)
        nat.check(lib.wb_nms_ordered_launch(nat.stream_ptr(), p_boxes, nat.ptr(d_scores), p_group, nat.ptr(order), *tail),
                  "wb_nms_ordered_launch")
    return out


def nms_keep_mask(boxes, scores, iou_threshold=0.5, score_threshold=None, group=None):
    """Keep flags (bool [N], input order) of greedy non-maximum suppression, computed on the GPU (wb_nms_launch): the
    arrays are uploaded, the flags read back.  See non_max_suppression for the semantics.  More than 2**16 boxes are put
    in visiting order by a stable torch.sort on the device and go through wb_nms_ordered_launch: every N a detect call
    can return (2**26) is accepted; the cost grows with N * N (include/waldboost_hip.h has the figures)."""
    from . import _native as nat
    boxes, scores, iou_threshold, group = _nms_inputs(boxes, scores, iou_threshold, score_threshold, group)
    n = scores.size
    if n == 0:
        return np.zeros(0, bool)
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    d_boxes = torch.from_numpy(boxes).to(dev)
    d_scores = torch.from_numpy(scores).to(dev)
    d_group = torch.from_numpy(group).to(dev) if group is not None else None
    h = _nms_enqueue(lib, dev, nat.ptr(d_boxes), d_scores, nat.ptr(d_group), n, iou_threshold, score_threshold).cpu().numpy()
    keep = h[4:].astype(bool)
    assert int(h[:4].view(np.uint32)[0]) == int(keep.sum())
    return keep


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
    if not boxes.has_field("scores"):
        raise ValueError("non_max_suppression needs a 'scores' field")
    if len(boxes) == 0:
        return boxes[np.zeros(0, np.intp)]
    keep = nms_keep_mask(boxes.get(), boxes.get_field("scores"), iou_threshold, score_threshold, group)
    return boxes[np.flatnonzero(keep)]


VOTE_WEIGHTS = ("uniform", "score")      # WB_VOTE_UNIFORM, WB_VOTE_SCORE


def _vote_inputs(boxes, scores, vote_iou, weights, score_threshold, min_votes=1):
    """The checked arguments of a voting call: (vote_iou, weights code, float32 score_threshold or None, min_votes)."""
    vote_iou = float(vote_iou)
    if not vote_iou >= 0.0:
        raise ValueError("vote_iou must be a number >= 0")
    if weights not in VOTE_WEIGHTS:
        raise ValueError(f"weights must be one of {VOTE_WEIGHTS}, not {weights!r}")
    if score_threshold is not None:
        score_threshold = float(np.float32(score_threshold))
        if score_threshold != score_threshold:
            raise ValueError("score_threshold is NaN")
    elif weights == "score":
        raise ValueError('"score" weights are measured from the score threshold: give a score_threshold')
    if not np.isfinite(boxes).all():
        raise ValueError("box voting: coordinates must be finite")
    if np.isnan(scores).any():
        raise ValueError("box voting: scores must not be NaN")
    if int(min_votes) != min_votes or min_votes < 0:
        raise ValueError("min_votes must be an integer >= 0")
    return vote_iou, VOTE_WEIGHTS.index(weights), score_threshold, int(min_votes)


def _vote_enqueue(lib, d_boxes, d_scores, d_group, d_keep, n, vote_iou, code, score_threshold, d_merged, d_votes):
    """wb_vote_launch on device pointers (ctypes), on the current stream."""
    from . import _native as nat
    nat.check(lib.wb_vote_launch(nat.stream_ptr(), d_boxes, d_scores, d_group, d_keep, n, vote_iou, code, 0 if score_threshold is None else 1,
                                 0.0 if score_threshold is None else score_threshold, d_merged, d_votes), "wb_vote_launch")


def _upload_boxes(dev, boxes, scores, group, keep=None):
    """One upload of boxes | scores | group | keep (the absent ones left out): (the device bytes, ctypes pointers by name)."""
    import ctypes as C
    import torch
    parts = dict(boxes=boxes.reshape(-1), scores=scores)
    if group is not None:
        parts["group"] = group
    if keep is not None:
        parts["keep"] = keep
    blob = torch.from_numpy(np.concatenate([p.view(np.uint8) for p in parts.values()])).to(dev)
    offs = np.cumsum([0] + [p.nbytes for p in parts.values()])
    at = {k: C.c_void_p(blob.data_ptr() + int(o)) for k, o in zip(parts, offs)}
    at.setdefault("group", C.c_void_p(0))
    return blob, at, {k: int(o) for k, o in zip(parts, offs)}


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
    from . import _native as nat
    boxes, scores, _, group = _nms_inputs(boxes, scores, 0.0, score_threshold, group)
    n = scores.size
    keep = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, np.uint8)
    if keep.size != n:
        raise ValueError(f"{keep.size} keep flags, {n} boxes")
    vote_iou, code, score_threshold, _ = _vote_inputs(boxes, scores, vote_iou, weights, score_threshold)
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int32)
    import ctypes as C
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    blob, at, _ = _upload_boxes(dev, boxes, scores, group, keep)
    out = torch.empty(20 * n, dtype=torch.uint8, device=dev)          # merged | votes: one read-back
    _vote_enqueue(lib, at["boxes"], at["scores"], at["group"], at["keep"], n, vote_iou, code, score_threshold, nat.ptr(out),
                  C.c_void_p(out.data_ptr() + 16 * n))
    h = out.cpu().numpy()
    return h[:16 * n].view(np.float32).reshape(n, 4).copy(), h[16 * n:].view(np.int32).copy()


def merge_detections(boxes, iou_threshold=0.5, score_threshold=None, group=None, vote_iou=0.5, weights="uniform", min_votes=1):
    """Greedy non-maximum suppression of a Boxes with a 'scores' field, exactly as non_max_suppression does it, and then box
    voting (vote_boxes has the rule): every kept box is replaced by the weighted mean of the boxes of its cluster -- itself
    and the live boxes of its group with ``iou >= vote_iou`` to it -- so the suppressed windows still say where the object is.

    Returns the kept boxes in input order, every field sliced; the coordinates are the merged ones; 'scores' is unchanged (it
    is the score of the cluster's mode); a new int32 field 'votes' counts each box's voters (>= 1).  Kept boxes with
    ``votes < min_votes`` are left out (an isolated firing is more often a false alarm than a cluster is); NMS is NOT run
    again after that, so a box such a kept box had suppressed does not come back.

    Runs on the GPU: one upload, the NMS launches and wb_vote_launch on the same device arrays, one read-back; no CPU
    fallback.  Bad arguments raise ValueError before the device is touched.  An empty Boxes is returned as an empty Boxes
    (with a 'votes' field) without touching the device."""
    from . import _native as nat
    if not boxes.has_field("scores"):
        raise ValueError("merge_detections needs a 'scores' field")
    b, s, iou_threshold, g = _nms_inputs(boxes.get(), boxes.get_field("scores"), iou_threshold, score_threshold, group)
    vote_iou, code, score_threshold, min_votes = _vote_inputs(b, s, vote_iou, weights, score_threshold, min_votes)
    n = s.size
    if n == 0:
        out = boxes[np.zeros(0, np.intp)]
        out.set_field("votes", np.zeros(0, np.int32))
        return out
    import ctypes as C
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    blob, at, offs = _upload_boxes(dev, b, s, g)
    d_scores = blob[offs["scores"]:offs["scores"] + 4 * n].view(torch.float32)            # (what the sort of the long path reads)
    flags = _nms_enqueue(lib, dev, at["boxes"], d_scores, at["group"], n, iou_threshold, score_threshold)
    out = torch.empty(20 * n, dtype=torch.uint8, device=dev)
    _vote_enqueue(lib, at["boxes"], at["scores"], at["group"], C.c_void_p(flags.data_ptr() + 4), n, vote_iou, code, score_threshold,
                  nat.ptr(out), C.c_void_p(out.data_ptr() + 16 * n))
    h = torch.cat([out, flags[4:]]).cpu().numpy()                     # merged | votes | keep flags: one read-back
    merged, votes, keep = h[:16 * n].view(np.float32).reshape(n, 4), h[16 * n:20 * n].view(np.int32), h[20 * n:].astype(bool)
    idx = np.flatnonzero(keep & (votes >= min_votes))
    res = boxes[idx]
    res = Boxes(merged[idx].copy(), **{k: res.get_field(k) for k in res.fields()})
    res.set_field("votes", votes[idx].copy())
    return res
