"""The NumPy statement of greedy non-maximum suppression as waldboost_amd defines it -- the yardstick of the NMS tests.

Boxes with `not (score >= float32(score_threshold))` are dropped; the rest is visited in stable descending score order
(-0.0 and +0.0 tie; equal scores in input order); a box is kept unless an already kept box of its group has
`waldboost_amd.boxes.iou(...) > iou_threshold` with it (strict, float64).  The result is a mask over the input order.
One IoU row per kept box: no N x N matrix."""
import numpy as np

from waldboost_amd.boxes import Boxes, iou


def nms_keep(boxes, scores, iou_threshold, group=None, score_threshold=None):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32).reshape(-1)
    n = scores.size
    group = None if group is None else np.asarray(group).reshape(-1)
    dead = np.zeros(n, bool) if score_threshold is None else ~(scores >= np.float32(score_threshold))
    keep = np.zeros(n, bool)
    everything = Boxes(boxes)
    for i in np.argsort(-(scores + np.float32(0)), kind="stable"):      # (+0: -0.0 and +0.0 tie)
        if dead[i]:
            continue
        keep[i] = True
        hit = iou(Boxes(boxes[i:i + 1]), everything)[0] > iou_threshold
        if group is not None:
            hit &= group == group[i]
        dead |= hit
        dead[i] = True
    return keep


def nms_boxes(bx, iou_threshold, group=None, score_threshold=None):
    """The yardstick on a Boxes with a 'scores' field: the kept boxes, every field sliced, input order."""
    return bx[np.flatnonzero(nms_keep(bx.get(), bx.get_field("scores"), iou_threshold, group, score_threshold))]


def detector_like_boxes(n, seed, H=1080, W=1920, m=12, n_cols=12, levels=24):
    """Boxes as Model.get_boxes forms them: integer (r, c) windows of random pyramid levels times float32(1/scale);
    scores quantised to 1/8, so that ties dominate."""
    rng = np.random.default_rng(seed)
    scales = 0.5 * 2.0 ** (-np.arange(levels) / 8)
    lv = rng.integers(0, levels, n)
    inv = (1.0 / scales[lv]).astype(np.float32)
    u, v = (H * scales[lv]).astype(int), (W * scales[lv]).astype(int)
    r = (rng.random(n) * np.maximum(u - m, 1)).astype(int)
    c = (rng.random(n) * np.maximum(v - n_cols, 1)).astype(int)
    f = lambda a: a.astype(np.float32) * inv
    boxes = np.stack([f(c), f(r), f(c + n_cols), f(r + m)], 1)
    scores = (np.round(rng.normal(0, 2, n) * 8) / 8).astype(np.float32)
    return boxes, scores


# (name, boxes, scores, iou_threshold, group, score_threshold, expected keep flags): answers written by hand
def hand_cases():
    f = lambda *rows: np.array(rows, np.float32)
    A = [0, 0, 10, 10]
    yield "identical: the earlier wins", f(A, A), np.array([1, 1], "f"), 0.5, None, None, [1, 0]
    yield "identical, later scores higher", f(A, A), np.array([1, 2], "f"), 0.5, None, None, [0, 1]
    # chain: iou(A,B) = 60/140, iou(B,C) = 60/140, iou(A,C) = 20/180; A > B > C in score
    yield ("chain: C survives because B is gone", f(A, [4, 0, 14, 10], [8, 0, 18, 10]), np.array([3, 2, 1], "f"), 0.3, None, None,
           [1, 0, 1])
    # iou = 50 / 150 = 1/3 (x overlap 5 of 10): the threshold is that very double -- strict > keeps both
    yield "iou equals the threshold: kept", f(A, [5, 0, 15, 10]), np.array([2, 1], "f"), 50.0 / 150.0, None, None, [1, 1]
    yield ("just below it: suppressed", f(A, [5, 0, 15, 10]), np.array([2, 1], "f"), float(np.nextafter(50.0 / 150.0, 0)), None, None,
           [1, 0])
    yield "threshold 0, touching boxes (iou 0): kept", f(A, [10, 0, 20, 10]), np.array([2, 1], "f"), 0.0, None, None, [1, 1]
    yield "threshold 0, one pixel of overlap", f(A, [9, 0, 19, 10]), np.array([2, 1], "f"), 0.0, None, None, [1, 0]
    yield "-0.0 ties with +0.0: the earlier wins", f(A, A), np.array([-0.0, 0.0], "f"), 0.5, None, None, [1, 0]
    yield "+0.0 then -0.0", f(A, A), np.array([0.0, -0.0], "f"), 0.5, None, None, [1, 0]
    yield "groups do not suppress each other", f(A, A, A), np.array([3, 2, 1], "f"), 0.5, [0, 1, 0], None, [1, 1, 0]
    yield ("score_threshold drops first (equality passes)", f(A, A, [50, 50, 60, 60]), np.array([-1, -2, -3], "f"), 0.5,
           None, -2.0, [1, 0, 0])
    yield "score_threshold keeps equality", f(A, [50, 50, 60, 60]), np.array([0.5, 0.25], "f"), 0.5, None, 0.25, [1, 1]
    yield "degenerate boxes (union 0): iou 0", f([3, 3, 3, 3], [3, 3, 3, 3]), np.array([1, 1], "f"), 0.0, None, None, [1, 1]
    yield "threshold 1: nothing is suppressed", f(A, A), np.array([1, 1], "f"), 1.0, None, None, [1, 1]
