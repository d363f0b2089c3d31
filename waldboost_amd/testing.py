"""Detector testing (reference testing.py): ``detect_on_images`` streams a data set through the hot path, ``evaluate_model``
collects its results in an ``Evaluator``, and ``Evaluator.evaluate`` turns them into a precision / recall curve and its AUC.

The evaluation's device work is batched over the data set, not looped over images: non-maximum suppression of all images'
detections with the image as the group (``boxes.nms_keep_mask``, whole images in chunks of at most 4096 boxes -- one band of
the NMS kernels, three launches a call) and ONE ``boxes.match_boxes`` call (wb_match_launch) for every detection's best IoU
and owning ground-truth box.  Flags, thresholds and the curve are host arithmetic on what comes back.  The curve is a NumPy
restatement of scikit-learn 0.24.2's ``precision_recall_curve`` and ``auc`` (the package does not import sklearn).
DESIGN section 4.9 has the argument and the reference's quirks that are kept."""
import collections
import logging
import random
from itertools import cycle, islice

import numpy as np

from .boxes import Boxes, boxes_in_window, match_boxes, nms_keep_mask, set_aspect_ratio

_NMS_CHUNK = 4096       # one band of the NMS kernels (WB_NMS_BAND): up to here a call is three launches


def _nms_chunks(counts, limit=_NMS_CHUNK):
    """Ranges (first image, one past the last) of consecutive images whose detections go into one NMS call: as many whole
    images as hold at most `limit` boxes together; an image with more than `limit` gets a call of its own.  A pure
    function of the per-image counts; ranges without a box are left out (all images empty: no call at all)."""
    chunks, lo, total = [], 0, 0
    for k, c in enumerate(counts):
        c = int(c)
        if c < 0:
            raise ValueError("negative count")
        if total > 0 and total + c > limit:
            chunks.append((lo, k))
            lo, total = k, 0
        total += c
    if total > 0:
        chunks.append((lo, len(counts)))
    return chunks


def _precision_recall_curve(y_true, scores):
    """(precision, recall, thresholds) as scikit-learn 0.24.2's ``sklearn.metrics.precision_recall_curve(y_true, scores)``
    returns them for boolean `y_true`, restated in NumPy, bit for bit: descending order by a stable mergesort reversed,
    one point per distinct score, cumulative counts (integers, so exact), precision = tps / (tps + fps) with NaN set to 0,
    recall = tps / tps[-1], the curve cut at the FIRST point of full recall, reversed, and (1, 0) appended.  (Releases from
    1.1 on no longer cut the curve; 0.24.2 is the version the reference was used with and the yardstick of the tests.)
    No sample at all: ValueError.  No positive sample: recall is 0 / 0 = NaN, as that release returns it."""
    y_true = np.asarray(y_true).reshape(-1).astype(bool)
    scores = np.asarray(scores).reshape(-1)
    if y_true.size != scores.size:
        raise ValueError(f"{y_true.size} labels, {scores.size} scores")
    if y_true.size == 0:
        raise ValueError("no evaluated detections: there is no precision / recall curve of nothing")
    if not np.isfinite(scores).all():
        raise ValueError("scores must be finite")
    order = np.argsort(scores, kind="mergesort")[::-1]
    scores, y_true = scores[order], y_true[order]
    idx = np.r_[np.where(np.diff(scores))[0], y_true.size - 1]
    tps = np.cumsum(y_true.astype(np.int64))[idx].astype(np.float64)
    fps = 1 + idx - tps
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = tps / (tps + fps)
        precision[np.isnan(precision)] = 0
        recall = tps / tps[-1]
    sl = slice(int(tps.searchsorted(tps[-1])), None, -1)
    return np.r_[precision[sl], 1], np.r_[recall[sl], 0], scores[idx][sl]


def _auc(x, y):
    """scikit-learn 0.24.2's ``sklearn.metrics.auc(x, y)``: the trapezoid rule, signed by the direction of x."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    if x.shape[0] < 2:
        raise ValueError(f"At least 2 points are needed to compute area under curve, but x.shape = {x.shape}")
    dx = np.diff(x)
    direction = 1
    if np.any(dx < 0):
        if not np.all(dx <= 0):
            raise ValueError(f"x is neither increasing nor decreasing : {x}.")
        direction = -1
    return direction * (dx * (y[1:] + y[:-1]) / 2.0).sum()      # (np.trapz, written out)


class Evaluator:
    """Collects per-image ground truth and detections and evaluates them (reference testing.py:18-81)."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.eval_data = dict()

    def add_ground_truth(self, idx, boxes: Boxes, shape):
        if idx not in self.eval_data:
            self.eval_data[idx] = dict()
        self.eval_data[idx].update(gt=boxes, shape=shape)

    def add_detections(self, idx, boxes: Boxes):
        if idx not in self.eval_data:
            self.eval_data[idx] = dict()
        self.eval_data[idx].update(dt=boxes)

    def evaluate(self, match_iou_threshold=0.5, dt_iou_threshold=0.5, min_gt_area=0, min_gt_area_in_image=1, normalize_ar=None):
        """dict(precision, recall, threshold: lists; auc; iou_threshold; n_eval, n_ign: ground-truth boxes evaluated / ignored).

        Per image: a ground-truth box is ignored when its 'ignore' field is not 0 (no such field: nothing is), its area is
        under `min_gt_area`, or less than `min_gt_area_in_image` of it lies inside the image; the detections go through
        non-maximum suppression at `dt_iou_threshold` (on float32 coordinates and scores, as ``non_max_suppression``);
        `normalize_ar` then gives detections and ground truth that aspect ratio; every detection is owned by the
        ground-truth box of largest IoU and is a true positive when that IoU is ``> match_iou_threshold`` (strict).

        The reference's quirks, kept: several detections may match one ground-truth box and ALL count as true positives; a
        detection is dropped when the box that owns it is ignored, and the owner is the first argmax -- box 0 for a
        detection that overlaps nothing; recall is relative to the number of true-positive detections, not of
        ground-truth boxes; an image without ground truth contributes only false positives.  An image with detections
        but no ground-truth entry, or the reverse, raises KeyError.  (The reference's ``np.bool`` is ``bool``.)

        On the device: one NMS call per chunk of whole images (`_nms_chunks`) with the image as the group -- which equals
        per-image NMS bit for bit --, and one `match_boxes` call for the whole data set."""
        images = list(self.eval_data.values())
        gts = [d["gt"] for d in images]
        dts = [d["dt"] for d in images]
        shapes = [d["shape"] for d in images]
        gt_ignore = []
        for gt, (h, w) in zip(gts, shapes):
            flags = gt.get_field("ignore") if gt.has_field("ignore") else np.zeros(len(gt))
            gt_ignore.append(np.logical_or.reduce([
                np.asarray(flags).reshape(-1) != 0,
                gt.area() < min_gt_area,
                ~boxes_in_window(gt, Boxes([0, 0, w, h]), min_overlap=min_gt_area_in_image)]))
        # non-maximum suppression: whole images per call, the image ordinal as the group
        counts = [len(b) for b in dts]
        keep = [np.zeros(c, bool) for c in counts]
        for lo, hi in _nms_chunks(counts):
            at = [k for k in range(lo, hi) if counts[k]]
            mask = nms_keep_mask(np.concatenate([dts[k].get() for k in at]), np.concatenate([dts[k].get_field("scores") for k in at]),
                                 dt_iou_threshold, group=np.repeat(at, [counts[k] for k in at]))
            for k, part in zip(at, np.split(mask, np.cumsum([counts[k] for k in at])[:-1])):
                keep[k] = part
        dts = [b[np.flatnonzero(m)] for b, m in zip(dts, keep)]
        dt_scores = [b.get_field("scores") for b in dts]
        if normalize_ar is not None:
            dts = [set_aspect_ratio(b, normalize_ar) for b in dts]
            gts = [set_aspect_ratio(b, normalize_ar) for b in gts]
        # one matching call for the whole data set
        n_kept = [len(b) for b in dts]
        all_dt = Boxes(np.concatenate([np.asarray(b.get(), np.float64).reshape(-1, 4) for b in dts]) if dts else np.empty((0, 4)))
        best, owner = match_boxes(all_dt, gts, np.repeat(np.arange(len(dts)), n_kept))
        labels, scores = [], []
        cuts = np.cumsum(n_kept)[:-1] if dts else []
        for gt_ign, sc, b, o in zip(gt_ignore, dt_scores, np.split(best, cuts), np.split(owner, cuts)):
            if gt_ign.size > 0:
                ign = gt_ign[o]
                labels.append((b > match_iou_threshold)[~ign])
                scores.append(sc[~ign])
            else:
                labels.append(np.zeros(len(sc), bool))
                scores.append(sc)
        if not labels:
            raise ValueError("no evaluated detections: the evaluator holds no image")
        y_true = np.concatenate(labels)
        scores = np.concatenate(scores)
        ignored = np.concatenate(gt_ignore)
        p, r, t = _precision_recall_curve(y_true, scores)
        return dict(precision=p.tolist(), recall=r.tolist(), threshold=t.tolist(), auc=_auc(r, p), iou_threshold=match_iou_threshold,
                    n_eval=(ignored == 0).sum(), n_ign=(ignored != 0).sum())


def random_iterator(seq, maxlen=None):
    """Iterate over the elements of an indexable sequence in a random order, again and again in that order (reference
    testing.py:84-96, with its missing ``cycle`` import); stops after ``maxlen + 1`` elements, as the reference's
    ``i > maxlen`` does."""
    if not hasattr(seq, "__len__") or not hasattr(seq, "__getitem__"):
        raise TypeError("Sequence must be indexable")
    order = list(range(len(seq)))
    random.shuffle(order)
    for i, j in enumerate(cycle(order)):
        if maxlen is not None and i > maxlen:
            return
        yield seq[j]


def evaluate_model(testing_images, *model, num_images=None, shuffle=False, lanes=1, batch=1):
    """Run `model` on `num_images` of `testing_images` (all of them when they have a length) and return the Evaluator that
    holds every image's ground truth and detections (reference testing.py:99-124).  lanes / batch: passed to
    `detect_on_images` (an extension).  No image at all: an empty Evaluator and the reference's warning (the reference
    itself dies there on an unbound name)."""
    if num_images is None:
        if hasattr(testing_images, "__len__"):
            num_images = len(testing_images)
        else:
            raise ValueError("Require num_images with infinite dataset")
    if shuffle:
        testing_images = random_iterator(testing_images)
    imgs = islice(testing_images, num_images)
    E = Evaluator()
    logging.info(f"Running model on {num_images} images")
    idx = 0
    for idx, (gt, dt, shape) in enumerate(detect_on_images(imgs, *model, lanes=lanes, batch=batch), start=1):
        E.add_ground_truth(idx, gt, shape)
        E.add_detections(idx, dt)
        if idx % 20 == 0:
            logging.info(f"{idx}")
    if num_images != idx:
        logging.warning(f"Requested test on {num_images} but only {idx} images were given in dataset.")
    return E


def detect_on_images(images, *model, gt_key="groundtruth_boxes", lanes=1, batch=1):
    """Yield (gt_boxes, dt_boxes, image.shape[:2]) for every dict of `images` (keys 'image' and
    `gt_key`), detections from ``waldboost_amd.detect(image, *model)``.
    lanes / batch (an extension; one model only): more than one of either runs the images through
    ``Model.detect_stream`` -- same tuples in the same order, but up to lanes * batch - 1 dicts are taken from `images`
    ahead of the tuple being yielded."""
    from . import detect
    empty_boxes = Boxes(np.empty((0, 4)), ignore=np.empty(0))
    if (lanes > 1 or batch > 1) and len(model) == 1:
        meta = collections.deque()

        def source():
            for data_dict in images:
                image = data_dict.get("image")
                meta.append((data_dict.get(gt_key, empty_boxes), image.shape[:2]))
                yield image

        for dt_boxes in model[0].detect_stream(source(), lanes=lanes, batch=batch):
            gt_boxes, shape = meta.popleft()
            dt_boxes.set_field("label", np.zeros(len(dt_boxes), np.int64))      # (what detect() adds for its one model)
            yield gt_boxes, dt_boxes, shape
        return
    for data_dict in images:
        image = data_dict.get("image")
        gt_boxes = data_dict.get(gt_key, empty_boxes)
        dt_boxes = detect(image, *model)
        yield gt_boxes, dt_boxes, image.shape[:2]
