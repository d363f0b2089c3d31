"""The NumPy statement of box voting as waldboost_amd defines it -- the yardstick of the voting tests (wb_vote_launch,
boxes.vote_boxes, boxes.merge_detections and the vote_iou= keyword of the detect calls).

Inputs: boxes float32 [n][4] XYXY, scores float32 [n] (no NaN), group int32 [n] or None, keep uint8 [n] as NMS wrote it,
vote_iou a double >= 0, weights "uniform" or "score", the optional score_threshold NMS used.

* A box is LIVE unless the score threshold is in use and `not (score >= float32(score_threshold))`.
* For a kept box k, box j is a VOTER when j == k (always, even for a zero-area box whose IoU with itself is 0), or when j is
  live, in k's group, and `waldboost_amd.boxes.iou(box_k, box_j) >= vote_iou` (float64, every operation rounded on its own).
* Weights: "uniform" w_j = 1.0; "score" w_j = float64(score_j) - float64(float32(score_threshold)), >= 0 for every live box
  (the mode needs a threshold; a box that is not live never votes except for itself).
* Order: lane l of 64 visits j = l, l + 64, l + 128, ... ascending; for each voter sw = sw + w and, per coordinate,
  sc[i] = sc[i] + (w * float64(x_ji)), the product rounded first, then the sum (no fused multiply-add).  The 64 partials of the
  five doubles and of the integer vote count are combined by a butterfly: for s in 1, 2, 4, 8, 16, 32: p = p + p[lane ^ s].
* merged_k[i] = float32(sc[i] / sw) when sw > 0; otherwise box k's own coordinates.  votes_k = the number of voters, >= 1.
* Rows of boxes that are not kept hold their own box and votes = 0.

(A lane's sums start from +0.0 and a sum that starts there never becomes -0.0, so adding +0.0 for a candidate that does not
vote leaves every bit as it is: the statement adds `where(voter, term, 0.0)`.)"""
import numpy as np

from waldboost_amd.boxes import Boxes, iou

WEIGHTS = ("uniform", "score")
LANES = 64
KEPT_AT_A_TIME = 64          # kept boxes summed together (bounds the [K][n] tables)


def live_mask(scores, score_threshold):
    scores = np.asarray(scores, np.float32).reshape(-1)
    return np.ones(scores.size, bool) if score_threshold is None else scores >= np.float32(score_threshold)


def vote_weights(scores, weights, score_threshold):
    """w_j of every box as if it voted, float64 [n]."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    if weights == "uniform":
        return np.ones(scores.size, np.float64)
    if weights != "score":
        raise ValueError(f"weights must be one of {WEIGHTS}")
    if score_threshold is None:
        raise ValueError('"score" weights need a score_threshold')
    return scores.astype(np.float64) - np.float64(np.float32(score_threshold))


def voters(boxes, scores, keep, vote_iou, score_threshold=None, group=None):
    """(kept indices [K], voter table bool [K][n])."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = boxes.shape[0]
    kept = np.flatnonzero(np.asarray(keep).reshape(-1) != 0)
    v = iou(Boxes(boxes[kept]), Boxes(boxes)) >= vote_iou
    v &= live_mask(scores, score_threshold)[None, :]
    if group is not None:
        group = np.asarray(group).reshape(-1)
        v &= group[kept][:, None] == group[None, :]
    v[np.arange(kept.size), kept] = True
    return kept, v.reshape(kept.size, n)


def lane_sums(terms):
    """terms float64 / int [K][n][F] -> [K][F]: 64 lanes, each adding its candidates in ascending order, then the butterfly."""
    K, n, F = terms.shape
    rows = -(-n // LANES)
    padded = np.zeros((K, rows * LANES, F), terms.dtype)
    padded[:, :n] = terms
    padded = padded.reshape(K, rows, LANES, F)
    p = np.zeros((K, LANES, F), terms.dtype)
    for r in range(rows):
        p = p + padded[:, r]
    lane = np.arange(LANES)
    for s in (1, 2, 4, 8, 16, 32):
        p = p + p[:, lane ^ s]
    return p[:, 0]


def vote(boxes, scores, keep, vote_iou=0.5, weights="uniform", score_threshold=None, group=None):
    """(merged float32 [n][4], votes int32 [n])."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    n = scores.size
    w_all = vote_weights(scores, weights, score_threshold)
    merged, votes = boxes.copy(), np.zeros(n, np.int32)
    if n == 0:
        return merged, votes
    keep = np.asarray(keep).reshape(-1) != 0
    kept_all = np.flatnonzero(keep)
    x = boxes.astype(np.float64)
    for at in range(0, kept_all.size, KEPT_AT_A_TIME):
        part = np.zeros(n, bool)
        part[kept_all[at:at + KEPT_AT_A_TIME]] = True
        kept, v = voters(boxes, scores, part, vote_iou, score_threshold, group)
        w = np.where(v, w_all[None, :], 0.0)                                        # [K][n]
        terms = np.concatenate([w[:, :, None], np.where(v[:, :, None], w_all[None, :, None] * x[None, :, :], 0.0)], 2)
        sums = lane_sums(terms)
        sw, sc = sums[:, 0], sums[:, 1:]
        votes[kept] = lane_sums(v[:, :, None].astype(np.int32))[:, 0]
        ok = sw > 0
        with np.errstate(all="ignore"):
            merged[kept[ok]] = (sc[ok] / sw[ok, None]).astype(np.float32)
    return merged, votes


def merge(bx, iou_threshold=0.5, score_threshold=None, group=None, vote_iou=0.5, weights="uniform", min_votes=1):
    """The yardstick of merge_detections on a Boxes with a 'scores' field: nms_reference.nms_keep, then vote; the kept boxes
    with at least min_votes voters, input order, every field sliced, the coordinates merged and a 'votes' field added."""
    from nms_reference import nms_keep
    scores = bx.get_field("scores")
    keep = nms_keep(bx.get(), scores, iou_threshold, group, score_threshold)
    merged, votes = vote(bx.get(), scores, keep, vote_iou, weights, score_threshold, group)
    idx = np.flatnonzero(keep & (votes >= min_votes))
    out = Boxes(merged[idx], **{k: bx.get_field(k)[idx] for k in bx.fields()})
    out.set_field("votes", votes[idx])
    return out
