"""The NumPy statement of waldboost_amd.testing.Evaluator.evaluate -- the yardstick of the evaluation tests: the reference's
own loop over images (reference testing.py:31-81) with nms_reference.nms_keep for the suppression, boxes.iou with argmax and
max for the matching, and the package's restatement of scikit-learn 0.24.2's curve (which tests/test_eval_host.py holds
against recorded sklearn output).  No GPU."""
import numpy as np

from nms_reference import nms_keep
from waldboost_amd.boxes import Boxes, boxes_in_window, iou, set_aspect_ratio
from waldboost_amd.testing import _auc, _precision_recall_curve


def evaluate_images(images, match_iou_threshold=0.5, dt_iou_threshold=0.5, min_gt_area=0, min_gt_area_in_image=1, normalize_ar=None,
                    details=None):
    """images: (gt Boxes, dt Boxes, (h, w)) per image.  details: a dict that receives the counts the tests assert on."""
    labels, scores, ignored = [], [], []
    n_suppressed = n_dropped = 0
    for gt_boxes, dt_all, (h, w) in images:
        flags = gt_boxes.get_field("ignore") if gt_boxes.has_field("ignore") else np.zeros(len(gt_boxes))
        gt_ignore = np.logical_or.reduce([flags != 0, gt_boxes.area() < min_gt_area,
                                          ~boxes_in_window(gt_boxes, Boxes([0, 0, w, h]), min_overlap=min_gt_area_in_image)])
        keep = nms_keep(dt_all.get(), dt_all.get_field("scores"), dt_iou_threshold)
        n_suppressed += int((~keep).sum())
        dt_boxes = dt_all[np.flatnonzero(keep)]
        dt_scores = dt_boxes.get_field("scores")
        if normalize_ar is not None:
            dt_boxes = set_aspect_ratio(dt_boxes, normalize_ar)
            gt_boxes = set_aspect_ratio(gt_boxes, normalize_ar)
        table = iou(gt_boxes, dt_boxes)
        if table.shape[0] > 0:
            ign = gt_ignore[table.argmax(axis=0)]
            tp = (table.max(axis=0) > match_iou_threshold)[~ign]
            score = dt_scores[~ign]
            n_dropped += int(ign.sum())
        else:
            tp = np.zeros(len(dt_boxes), bool)
            score = dt_scores
        ignored.append(gt_ignore)
        labels.append(tp)
        scores.append(score)
    y_true, scores, ignored = np.concatenate(labels), np.concatenate(scores), np.concatenate(ignored)
    if details is not None:
        details.update(tp=int(y_true.sum()), fp=int((~y_true).sum()), dropped=n_dropped, suppressed=n_suppressed)
    p, r, t = _precision_recall_curve(y_true, scores)
    return dict(precision=p.tolist(), recall=r.tolist(), threshold=t.tolist(), auc=_auc(r, p), iou_threshold=match_iou_threshold,
                n_eval=(ignored == 0).sum(), n_ign=(ignored != 0).sum())


def same_dict(a, b):
    """Equal keys; lists and numbers bit for bit (NaNs in place)."""
    bits = lambda x: np.asarray(x, np.float64).view(np.uint64)
    if set(a) != set(b):
        return False
    for k in ("precision", "recall", "threshold"):
        if len(a[k]) != len(b[k]) or not np.array_equal(bits(a[k]), bits(b[k])):
            return False
    return bool(bits(a["auc"]) == bits(b["auc"]) and a["iou_threshold"] == b["iou_threshold"] and int(a["n_eval"]) == int(b["n_eval"])
                and int(a["n_ign"]) == int(b["n_ign"]))
