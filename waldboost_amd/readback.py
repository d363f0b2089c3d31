"""A scan's results on their way from the device to ``Boxes``: the byte layout of a finish block, the sort key's bit
fields, the host's own ordering and box arithmetic, what the engine's read-back methods return, and the one form --
Detections -- that every one of them is turned into.  NumPy only.

A finish block of `rows` records, as wb_det_finish_sorted_launch (one image) and wb_det_order_batch_launch (one block
per image, back to back behind a 16-byte prefix) write it:  16-byte header | 8 * rows keys | 16 * rows boxes | 4 * rows
scores.  header: int32 [4] -- [0] the detections, [1] the fullest shard's count (above the shard capacity: records were
dropped, grow the buffer and scan again; in a batch's block: the image's detections again, above `rows` they did not fit
-- the fullest shard is word 1 of the prefix), [3] 1 when the sections are in key order.  keys: uint64, boxes: float32
[rows, 4] (XYXY), scores: float32.  wb_det_finish_sorted_launch copies alive[B, L, T] behind the block.
A key is level << 54 | r << 40 | c << 26 | position: 10 / 14 / 14 bits of the window and, in the low 26, the row of the
block's boxes and scores that is the window's.  Keys are unique; ascending, they are the reference's order (level, r, c).
"""
from typing import NamedTuple, Optional

import numpy as np

from ._native import DET_DTYPE

# PyramidEngine.fetch_final, ONE image -- keys: uint64 [n]; boxes: float32 [rows, 4]; scores: float32 [rows]; alive: int64
# [B, L, T]; ordered: keys ascending and boxes[i] / scores[i] the i-th detection, else keys unsorted and boxes / scores
# indexed by key_positions; keep: bool [n] by position, the flags non-maximum suppression left on the device, None when
# none ran or it left none (the caller then suppresses the complete result).  Views of the page-locked read-back buffer
# (here and in ImageResult): copy what is kept
Finished = NamedTuple("Finished", [("keys", np.ndarray), ("boxes", np.ndarray), ("scores", np.ndarray), ("alive", np.ndarray),
                                   ("ordered", bool), ("keep", Optional[np.ndarray])])
# one image of PyramidEngine.fetch_ordered_batch, in the reference's order: keys [n], boxes [n, 4], scores [n], keep
ImageResult = NamedTuple("ImageResult", [("keys", np.ndarray), ("boxes", np.ndarray), ("scores", np.ndarray),
                                         ("keep", Optional[np.ndarray])])
# PyramidEngine.fetch -- total: detections; records: int32 [total, 4] in shard order, None when `limit` left them on the
# device; alive: int64 [B, L, T]
Packed = NamedTuple("Packed", [("total", int), ("records", Optional[np.ndarray]), ("alive", np.ndarray)])


class FinishBlock:
    """Layout of one finish block of `rows` records."""

    def __init__(self, rows):
        self.rows = int(rows)
        self.nbytes = 16 + 28 * self.rows

    def views(self, host_bytes, offset=0):
        """(header int32 [4], keys uint64 [rows], boxes float32 [rows, 4], scores float32 [rows]) of the block `offset`
        bytes into the uint8 array `host_bytes`: views, not copies."""
        P = self.rows
        h = host_bytes[offset:offset + self.nbytes]
        return (h[:16].view(np.int32), h[16:16 + 8 * P].view(np.uint64),
                h[16 + 8 * P:16 + 24 * P].view(np.float32).reshape(P, 4), h[16 + 24 * P:].view(np.float32))


def key_fits(n_levels, max_u, max_v):
    """Whether a pyramid of `n_levels` levels of at most max_u x max_v channel pixels fits the sort key's fields."""
    return 0 < n_levels <= 1024 and max_u <= 16384 and max_v <= 16384


def split_keys(keys):
    """(level int32, r int64, c int64) of sort keys."""
    f = np.uint64(0x3fff)
    return ((keys >> np.uint64(54)).astype(np.int32), ((keys >> np.uint64(40)) & f).astype(np.int64),
            ((keys >> np.uint64(26)) & f).astype(np.int64))


def key_positions(keys):
    """The rows (intp) of the finish block's boxes and scores that belong to the keys."""
    return (keys & np.uint64((1 << 26) - 1)).astype(np.intp)


def host_boxes(records, m, n, inv_scales, with_image=False):
    """WbDet records in any order (DET_DTYPE, or the int32 [k, 4] they are read back as) -> (image int64 -- None without
    with_image --, level int32, r int64, c int64, boxes float32 [k, 4], scores float32 [k]) in the reference's order,
    (image,) level, r, c, for an m x n window; inv_scales: float32(1.0 / scale) per level.  The float32 arithmetic of
    boxes_kernel and Model.get_boxes, bit for bit."""
    d = records.view(DET_DTYPE).reshape(-1)
    level, r, c = d["level"].astype(np.int64), d["r"].astype(np.int64), d["c"].astype(np.int64)
    key = (level << 32) | (r << 16) | c
    if with_image:
        key |= d["image"].astype(np.int64) << 48
    order = np.argsort(key)                               # unique keys: any sort kind
    level, r, c = level[order], r[order], c[order]
    inv = inv_scales[level] if d.size else np.zeros(0, "f")
    boxes = np.empty((d.size, 4), np.float32)
    np.multiply(c.astype(np.float32), inv, out=boxes[:, 0])
    np.multiply(r.astype(np.float32), inv, out=boxes[:, 1])
    np.multiply((c + n).astype(np.float32), inv, out=boxes[:, 2])
    np.multiply((r + m).astype(np.float32), inv, out=boxes[:, 3])
    return (d["image"][order].astype(np.int64) if with_image else None, level.astype(np.int32), r, c, boxes,
            d["score"][order])


class Detections:
    """One image's detections in the reference's order (level, r, c): boxes float32 [n, 4] (XYXY), scores float32 [n],
    keep: the flags non-maximum suppression left on the device (bool [n]) or None.  The windows stay as they came -- sort
    keys or (level, r, c) -- and are split on demand; a converter told windows=False leaves them out altogether (Model.detect
    never asks: it pays neither the split nor the copy of the keys).  Owns its arrays: what the converters below take from
    a page-locked read-back buffer, they copy."""
    __slots__ = ("boxes", "scores", "keep", "_keys", "_windows")

    def __init__(self, boxes, scores, keep=None, keys=None, windows=None):
        self.boxes, self.scores, self.keep, self._keys, self._windows = boxes, scores, keep, keys, windows

    @classmethod
    def none(cls):
        return cls(np.empty((0, 4), np.float32), np.empty(0, np.float32), keys=np.empty(0, np.uint64))

    def windows(self):
        """(level int32 [n], r int64 [n], c int64 [n])"""
        if self._windows is None:
            if self._keys is None:
                raise ValueError("these detections were converted without their windows")
            self._windows = split_keys(self._keys)
        return self._windows

    def take(self, at):
        """The detections at rows `at`."""
        return Detections(self.boxes[at], self.scores[at], None, None if self._keys is None else self._keys[at],
                          None if self._windows is None else tuple(a[at] for a in self._windows))


def from_finished(fin, windows=True):
    """A Finished: slice copies when the device ordered it; otherwise the keys sorted here -- unique, so any sort kind
    gives the reference's order -- and boxes, scores and keep gathered by the keys' positions."""
    ks, keep = fin.keys, fin.keep
    if fin.ordered:
        return Detections(fin.boxes[:ks.size].copy(), fin.scores[:ks.size].copy(), None if keep is None else keep.copy(),
                          ks.copy() if windows else None)
    ks = np.sort(ks)
    at = key_positions(ks)
    return Detections(fin.boxes[at], fin.scores[at], keep[at] if keep is not None else None, ks if windows else None)


def from_image_result(item, windows=True):
    """An ImageResult (in order already)."""
    return Detections(item.boxes.copy(), item.scores.copy(), None if item.keep is None else item.keep.copy(),
                      item.keys.copy() if windows else None)


def _cut(count, image, level, r, c, boxes, scores):
    """Arrays ordered by (image, level, r, c) -> [Detections of image b for b < count]."""
    cuts = np.searchsorted(image, np.arange(count + 1))
    return [Detections(boxes[a:b], scores[a:b], windows=(level[a:b], r[a:b], c[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]


def from_packed(records, count, m, n, inv_scales, one_slot=False):
    """Packed records in shard order (Packed.records) -> [Detections per image < count], ordered and their boxes formed
    on the host (host_boxes); records of a slot >= count -- an earlier batch's -- are dropped.  one_slot: the engine
    holds one image, every record is its (no image column to sort by or to cut at)."""
    if one_slot:
        _, level, r, c, boxes, scores = host_boxes(records, m, n, inv_scales)
        return [Detections(boxes, scores, windows=(level, r, c))]
    d = records.view(DET_DTYPE).reshape(-1)
    return _cut(count, *host_boxes(d[d["image"] < count], m, n, inv_scales, with_image=True))


def from_ordered(records, boxes, scores, count):
    """Records the device put in order (by image, level, r, c: int32 [k, 4]) with their boxes and scores, as host arrays
    of their own -> [Detections per image < count]."""
    d = records.view(DET_DTYPE).reshape(-1)
    return _cut(count, d["image"], d["level"].astype(np.int32), d["r"].astype(np.int64), d["c"].astype(np.int64), boxes, scores)
