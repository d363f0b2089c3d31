"""Box voting behind the detect calls: the vote_iou= / vote_weights= / min_votes= keywords of Model.detect, waldboost_amd.detect
and regression.detect_and_refine against the NumPy statement (tests/vote_reference.py) applied to the same call's complete,
unsuppressed result -- boxes, scores and vote counts bit-identical and in the same order -- and the calls without the
keyword exactly as they were.  The mean IoU to the planted squares before and after merging is printed, not gated."""
import os

import numpy as np
import pytest

import regress_designs as rd
import regress_reference as rr
import vote_reference as vr
import waldboost_amd as wb
from nms_reference import nms_boxes
from test_gpu_regress import fitted
from waldboost_amd import regression
from waldboost_amd.synth import synth_image
from util import GOLDEN

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
MODES = [("uniform", 0.5), ("score", 0.5), ("uniform", 0.3), ("score", 0.7)]


def same(got, want, fields=("scores", "votes")):
    assert len(got) == len(want), (len(got), len(want))
    assert got.get().dtype == np.float32 and np.array_equal(bits(got.get()), bits(want.get()))
    for k in fields:
        assert got.get_field(k).dtype == want.get_field(k).dtype and np.array_equal(got.get_field(k), want.get_field(k)), k
    return True


def same_plain(a, b):
    return len(a) == len(b) and np.array_equal(bits(a.get()), bits(b.get())) and np.array_equal(bits(a.get_field("scores")), bits(b.get_field("scores")))


def test_model_detect_with_vote_iou_is_the_statement_on_its_plain_result():
    M = wb.load(os.path.join(GOLDEN, "models", "cfg2_d2_T128.pb"))
    seen = clusters = 0
    for image in (synth_image(480, 640, 0), synth_image(480, 640, 1), synth_image(1080, 1920, 0)):
        plain = M.detect(image)
        if len(plain) == 0:
            continue
        s = float(np.median(plain.get_field("scores")))
        for weights, v in (MODES if image.shape[0] < 1080 else MODES[:2]):            # (the statement takes its time on the large one)
            got = M.detect(image, iou_threshold=0.3, score_threshold=s, vote_iou=v, vote_weights=weights)
            want = vr.merge(plain, 0.3, s, None, v, weights)
            assert same(got, want)
            seen += len(plain)
            clusters += int((want.get_field("votes") >= 2).sum())
            assert np.any(bits(got.get()) != bits(nms_boxes(plain, 0.3, score_threshold=s).get())) or not (want.get_field("votes") >= 2).any()
        assert same(M.detect(image, iou_threshold=0.5, vote_iou=0.5), vr.merge(plain, 0.5))             # no score threshold
        few = M.detect(image, iou_threshold=0.3, vote_iou=0.5, min_votes=3)
        assert same(few, vr.merge(plain, 0.3, vote_iou=0.5, min_votes=3)) and (few.get_field("votes") >= 3).all()
        # without the keyword: today's results, no 'votes' field
        assert same_plain(M.detect(image, vote_iou=None), plain) and not M.detect(image).has_field("votes")
        kept = M.detect(image, iou_threshold=0.3, score_threshold=s, vote_iou=None, vote_weights="score", min_votes=5)
        assert same_plain(kept, nms_boxes(plain, 0.3, score_threshold=s)) and not kept.has_field("votes")
    print(f"{seen} detections went through voting, {clusters} kept boxes had more than their own vote")
    assert seen >= 200 and clusters >= 1


@pytest.mark.parametrize("rank_max", [None, 0], ids=["ranked", "ordered"])
def test_merge_detections_is_nms_keep_mask_then_vote_boxes_then_min_votes(rank_max, monkeypatch):
    """The three public functions share one device body: merging is the two steps and the filter, bit for bit and field for
    field -- also when the boxes go through torch.sort + wb_nms_ordered_launch (_NMS_RANK_MAX 0)."""
    import vote_designs as vd
    from waldboost_amd import boxes as B
    if rank_max is not None:
        monkeypatch.setattr(B, "_NMS_RANK_MAX", rank_max)
    d = next(x for x in vd.all_designs() if x.name == "sprinkle-n129-score-thr-groups")   # 44 kept, 30 with a second vote
    bx = wb.Boxes(d.boxes, scores=d.scores, label=d.group.astype(np.int64), index=np.arange(d.n))
    for min_votes in (1, 2):
        got = B.merge_detections(bx, d.nms_t, d.score_t, d.group, d.vote_iou, d.weights, min_votes)
        keep = B.nms_keep_mask(d.boxes, d.scores, d.nms_t, d.score_t, d.group)
        assert keep.dtype == bool and np.array_equal(keep, d.keep != 0)
        merged, votes = B.vote_boxes(d.boxes, d.scores, keep, d.vote_iou, d.weights, d.score_t, d.group)
        idx = np.flatnonzero(keep & (votes >= min_votes))
        assert 0 < idx.size and (min_votes == 1 or idx.size < keep.sum())
        assert got.fields() == ["scores", "label", "index", "votes"] and np.array_equal(got.get_field("index"), idx)
        assert same(got, wb.Boxes(merged[idx], scores=d.scores[idx], label=bx.get_field("label")[idx], votes=votes[idx]), ("scores", "label", "votes"))


def test_multi_model_detect_votes_inside_the_label_when_separate():
    A = wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    B = wb.load(os.path.join(GOLDEN, "models", "cfg2_d2_T128.pb"))
    img = synth_image(240, 320, 3)
    scale = [1.0, 0.5]
    plain = wb.detect(img, A, B, response_scale=scale)
    labels = plain.get_field("label")
    assert len(plain) >= 50 and 0 < (labels == 0).sum() < len(plain)
    s = float(np.median(plain.get_field("scores")))
    for weights, v in MODES[:2]:
        kw = dict(iou_threshold=0.2, score_threshold=s, vote_iou=v, vote_weights=weights)
        one = wb.detect(img, A, B, response_scale=scale, **kw)
        sep = wb.detect(img, A, B, response_scale=scale, separate=True, **kw)
        w_one, w_sep = vr.merge(plain, 0.2, s, None, v, weights), vr.merge(plain, 0.2, s, labels, v, weights)
        assert same(one, w_one, ("scores", "label", "votes")) and same(sep, w_sep, ("scores", "label", "votes"))
        assert 0 < len(w_one) <= len(w_sep) < len(plain)
    again = wb.detect(img, A, B, response_scale=scale, vote_iou=None)
    assert same_plain(again, plain) and not again.has_field("votes")
    t = wb.detect(img, A, B, response_scale=scale, iou_threshold=0.2, separate=True)
    assert same_plain(t, nms_boxes(plain, 0.2, group=labels)) and not t.has_field("votes")


def planted_iou(boxes, gt):
    """Per box the largest IoU over the planted squares `gt` and the square that gives it."""
    table = np.stack([rr.iou_rows(boxes, np.broadcast_to(g, boxes.shape)) for g in gt], 1)
    owner = table.argmax(1)
    return table[np.arange(owner.size), owner], owner


@pytest.mark.parametrize("flavour", ["float", "fpga"])
def test_detect_and_refine_votes_on_the_refined_boxes(flavour):
    """On the held-out planted-square images: detect_and_refine(..., vote_iou=) is the statement applied to the refined boxes.
    Reported, not gated: the mean IoU to the planted squares of the kept boxes that belong to one (IoU > 0.5 before merging),
    after plain NMS and after merging."""
    M, acc, reg = fitted(flavour)
    before, after, votes, raw_before, raw_after = [], [], [], [], []
    for it in rr.planted_images(range(6, 12)):
        raw_kept, raw_merged = M.detect(it["image"], iou_threshold=0.3), M.detect(it["image"], iou_threshold=0.3, vote_iou=0.5)
        assert same(raw_merged, vr.merge(M.detect(it["image"]), 0.3))
        best, owner = planted_iou(raw_kept.get(), it["gt"])
        raw_before.append(best[best > 0.5])
        raw_after.append(rr.iou_rows(raw_merged.get()[best > 0.5], it["gt"][owner[best > 0.5]]))
        refined = regression.detect_and_refine(it["image"], M, reg)
        assert not refined.has_field("votes")
        for weights, s in (("uniform", None), ("score", 0.0)):
            got = regression.detect_and_refine(it["image"], M, reg, iou_threshold=0.3, score_threshold=s, vote_iou=0.5, vote_weights=weights)
            assert same(got, vr.merge(refined, 0.3, s, None, 0.5, weights))
        kept = regression.detect_and_refine(it["image"], M, reg, iou_threshold=0.3)
        assert same_plain(kept, nms_boxes(refined, 0.3)) and not kept.has_field("votes")
        merged = regression.detect_and_refine(it["image"], M, reg, iou_threshold=0.3, vote_iou=0.5)
        assert len(merged) == len(kept)
        best, owner = planted_iou(kept.get(), it["gt"])
        sel = np.flatnonzero(best > 0.5)
        before.append(best[sel])
        after.append(rr.iou_rows(merged.get()[sel], it["gt"][owner[sel]]))
        votes.append(merged.get_field("votes")[sel])
    before, after, votes = np.concatenate(before), np.concatenate(after), np.concatenate(votes)
    print(f"{flavour}: {before.size} kept boxes on planted squares, mean votes {votes.mean():.1f}: mean IoU after NMS {before.mean():.3f} -> "
          f"after merging {after.mean():.3f}, {(after > before).mean():.1%} improved")
    raw_before, raw_after = np.concatenate(raw_before), np.concatenate(raw_after)
    print(f"{flavour}: without regression, {raw_before.size} kept boxes on planted squares: mean IoU after NMS {raw_before.mean():.3f} -> "
          f"after merging {raw_after.mean():.3f}, {(raw_after > raw_before).mean():.1%} improved")
    assert before.size >= 3 and raw_before.size >= 1


def test_detect_and_refine_with_a_trained_cascade_votes_by_score():
    M = wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    W, b = rd.random_weights(M.shape, seed=4)
    reg = regression.BoxRegressor(M.shape, W * 0.05, b)
    image = synth_image(200, 264, 41)
    refined = regression.detect_and_refine(image, M, reg)
    assert len(refined) >= 3
    s = float(np.median(refined.get_field("scores")))
    for weights, v in MODES:
        got = regression.detect_and_refine(image, M, reg, iou_threshold=0.3, score_threshold=s, vote_iou=v, vote_weights=weights, min_votes=1)
        assert same(got, vr.merge(refined, 0.3, s, None, v, weights))
    tiny = regression.detect_and_refine(np.zeros((8, 8), np.uint8), M, reg, iou_threshold=0.3, vote_iou=0.5)
    assert len(tiny) == 0 and tiny.has_field("votes")
