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


_NMS_RANK_MAX = 1 << 16      # most boxes wb_nms_launch orders itself (a quadratic pass); above: torch.sort + wb_nms_ordered_launch


def nms_keep_mask(boxes, scores, iou_threshold=0.5, score_threshold=None, group=None):
    """Keep flags (bool [N], input order) of greedy non-maximum suppression, computed on the GPU (wb_nms_launch): the
    arrays are uploaded, the flags read back.  See non_max_suppression for the semantics.  More than 2**16 boxes are put
    in visiting order by a stable torch.sort on the device and go through wb_nms_ordered_launch: every N a detect call
    can return (2**26) is accepted; the cost grows with N * N (include/waldboost_hip.h has the figures)."""
    from . import _native as nat
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
    if n == 0:
        return np.zeros(0, bool)
    import ctypes as C
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    need = C.c_size_t()
    nat.check(lib.wb_nms_scratch_bytes(n, C.byref(need)), "wb_nms_scratch_bytes")
    d_boxes = torch.from_numpy(boxes).to(dev)
    d_scores = torch.from_numpy(scores).to(dev)
    d_group = torch.from_numpy(group).to(dev) if group is not None else None
    scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.empty(4 + n, dtype=torch.uint8, device=dev)           # n_keep | keep flags: one read-back
    tail = (n, iou_threshold, 0 if score_threshold is None else 1, 0.0 if score_threshold is None else float(np.float32(score_threshold)),
            nat.ptr(scratch), scratch.numel(), C.c_void_p(out.data_ptr() + 4), nat.ptr(out))
    if n <= _NMS_RANK_MAX:
        nat.check(lib.wb_nms_launch(nat.stream_ptr(), nat.ptr(d_boxes), nat.ptr(d_scores), nat.ptr(d_group), *tail), "wb_nms_launch")
    else:
        # descending, the two zeros one value (-(s + 0) is -0.0 for both), equal scores in input order
        order = torch.sort(-(d_scores + 0.0), stable=True).indices.to(torch.int32)
        nat.check(lib.wb_nms_ordered_launch(nat.stream_ptr(), nat.ptr(d_boxes), nat.ptr(d_scores), nat.ptr(d_group), nat.ptr(order), *tail),
                  "wb_nms_ordered_launch")
    h = out.cpu().numpy()
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
