"""The voting kernel on the designed box sets of tests/vote_designs.py (proved on the host by test_vote_designs_host.py):
planted voter sets in exact integer arithmetic, the order design, voters at and a rounding below the threshold, zero-area
boxes, coinciding groups, boxes that are not live, sw == 0, -0.0 scores.  Everything goes through the C ABI (wb_vote_launch)
into output buffers pre-filled with garbage, and through boxes.vote_boxes / boxes.merge_detections; boxes, vote counts and
guard bytes are compared bit for bit with the statement (tests/vote_reference.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import vote_designs as vd
import vote_reference as vr
import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.boxes import Boxes, merge_detections, vote_boxes

pytestmark = pytest.mark.gpu

DESIGNS = vd.all_designs()
name = lambda d: d.name
GUARD = 64
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def statement(d):
    return d.want if d.want is not None else vr.vote(d.boxes, d.scores, d.keep, **d.args())


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def launch(d, fill):
    """One wb_vote_launch of design d into merged / votes buffers pre-filled with the byte `fill`, guard bytes around both."""
    import torch
    lib, n = nat.load(), d.n
    d_boxes, d_scores, d_keep = dev(d.boxes.reshape(-1)), dev(d.scores), dev(d.keep)
    d_group = dev(d.group) if d.group is not None else None
    merged = torch.full((GUARD + 16 * n + GUARD,), fill, dtype=torch.uint8, device="cuda")
    votes = torch.full((GUARD + 4 * n + GUARD,), fill, dtype=torch.uint8, device="cuda")
    nat.check(lib.wb_vote_launch(nat.stream_ptr(), nat.ptr(d_boxes), nat.ptr(d_scores), nat.ptr(d_group), nat.ptr(d_keep), n, d.vote_iou,
                                 vr.WEIGHTS.index(d.weights), 0 if d.score_t is None else 1, 0.0 if d.score_t is None else float(np.float32(d.score_t)),
                                 C.c_void_p(merged.data_ptr() + GUARD), C.c_void_p(votes.data_ptr() + GUARD)), "wb_vote_launch")
    hm, hv = merged.cpu().numpy(), votes.cpu().numpy()
    for h in (hm, hv):
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), f"{d.name}: bytes around an output were written"
    return hm[GUARD:-GUARD].view(np.float32).reshape(n, 4).copy(), hv[GUARD:-GUARD].view(np.int32).copy()


def describe(d, got, want):
    bad = np.flatnonzero((bits(got[0]) != bits(want[0])).any(1) | (got[1] != want[1]))
    if bad.size == 0:
        return f"{d.name}: equal"
    i = int(bad[0])
    return (f"{d.name}: {bad.size} rows differ, first at {i} (keep {d.keep[i]}, lane {i % 64}, chunk {i // vd.CHUNK}): box {got[0][i]} votes {got[1][i]}, "
            f"expected {want[0][i]} votes {want[1][i]}" + (f", planted voters {d.planted[i]}" if d.planted and i in d.planted else ""))


@pytest.mark.parametrize("d", DESIGNS, ids=name)
def test_the_c_abi_gives_the_statement_whatever_the_buffers_held(d):
    want = statement(d)
    first = launch(d, 0xA5)
    assert np.array_equal(bits(first[0]), bits(want[0])) and np.array_equal(first[1], want[1]), describe(d, first, want)
    # rows of boxes that are not kept are written: their own box, 0 votes
    off = d.keep == 0
    assert np.array_equal(bits(first[0][off]), bits(d.boxes[off])) and (first[1][off] == 0).all() and (first[1][~off] >= 1).all()
    # other garbage, another run: the same bits
    second = launch(d, 0xFF)
    assert np.array_equal(bits(second[0]), bits(first[0])) and np.array_equal(second[1], first[1]), describe(d, second, first)


@pytest.mark.parametrize("d", DESIGNS, ids=name)
def test_vote_boxes_and_merge_detections_give_the_statement(d):
    want = statement(d)
    got = vote_boxes(d.boxes, d.scores, d.keep, **d.args())
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), describe(d, got, want)
    # the design's keep flags are greedy NMS's at d.nms_t: merge_detections runs both
    bx = Boxes(d.boxes, scores=d.scores, index=np.arange(d.n))
    kw = dict(iou_threshold=d.nms_t, score_threshold=d.score_t, group=d.group, vote_iou=d.vote_iou, weights=d.weights)
    out = merge_detections(bx, **kw)
    kept = np.flatnonzero(d.keep)
    assert np.array_equal(out.get_field("index"), kept), f"{d.name}: merge_detections kept other boxes than the design"
    assert np.array_equal(bits(out.get()), bits(want[0][kept])) and np.array_equal(out.get_field("votes"), want[1][kept])
    assert out.get_field("votes").dtype == np.int32 and np.array_equal(bits(out.get_field("scores")), bits(d.scores[kept]))
    assert np.array_equal(bits(bx.get()), bits(d.boxes))                       # the input is left as it was


def test_merge_detections_is_the_statement_with_every_field_sliced():
    d = next(x for x in DESIGNS if x.name == "coinciding-groups-n70")
    bx = Boxes(d.boxes, scores=d.scores, label=d.group.astype(np.int64), tag=np.arange(d.n)[::-1].copy())
    kw = dict(iou_threshold=d.nms_t, score_threshold=d.score_t, group=d.group, vote_iou=d.vote_iou, weights=d.weights)
    got, want = wb.merge_detections(bx, **kw), vr.merge(bx, **kw)
    assert set(got.fields()) == {"scores", "label", "tag", "votes"} and len(got) == len(want) == d.n_keep
    assert np.array_equal(bits(got.get()), bits(want.get()))
    for k in got.fields():
        assert np.array_equal(got.get_field(k), want.get_field(k)) and got.get_field(k).dtype == want.get_field(k).dtype, k


def test_min_votes_filters_at_below_and_above_a_planted_count():
    d = next(x for x in DESIGNS if x.name == "positions-n600")
    assert d.want[1][0] == 6 and d.want[1][256] == 6 and d.want[1][599] == 3 and d.want[1][511] == 3     # the planted counts
    bx = Boxes(d.boxes, scores=d.scores, index=np.arange(d.n))
    kept = np.flatnonzero(d.keep)
    for min_votes, survivors in ((0, kept), (1, kept), (2, [0, 256, 511, 599]), (3, [0, 256, 511, 599]), (4, [0, 256]), (6, [0, 256]), (7, [])):
        out = merge_detections(bx, iou_threshold=d.nms_t, vote_iou=d.vote_iou, min_votes=min_votes)
        assert out.get_field("index").tolist() == list(survivors), min_votes
        assert np.array_equal(bits(out.get()), bits(d.want[0][list(survivors)].reshape(-1, 4)))
        assert np.array_equal(out.get_field("votes"), d.want[1][list(survivors)])
    # a suppressed box does not come back when its suppressor is filtered: NMS is not run again
    assert 597 not in merge_detections(bx, iou_threshold=d.nms_t, vote_iou=d.vote_iou, min_votes=4).get_field("index")
