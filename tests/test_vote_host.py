"""CPU tests of box voting's host side: the argument checks of vote_boxes / merge_detections and of the vote_iou= keywords
(all before the device is touched), the empty input, the export's refusals with fake pointers, the header's declaration and
the binding, the kernel's resource metadata, and the statement's own small cases."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import vote_reference as vr
import waldboost_amd as wb
from test_host import _kernel_scratch_sizes
from waldboost_amd import _native as nat
from waldboost_amd import boxes as wbb
from waldboost_amd import regression

A = [0, 0, 10, 10]
f = lambda *rows: np.array(rows, np.float32)


def test_statement_by_hand():
    b = f(A, [2, 0, 12, 10], [8, 0, 18, 10], [50, 50, 60, 60])                 # IoU with A: 80/120, 20/180, 0
    s = np.array([4, 3, 2, 1], np.float32)
    keep = [1, 0, 0, 1]
    m, v = vr.vote(b, s, keep, 0.5)
    assert v.tolist() == [2, 0, 0, 1] and m.dtype == np.float32 and v.dtype == np.int32
    assert m.tolist() == [[1, 0, 11, 10], [2, 0, 12, 10], [8, 0, 18, 10], [50, 50, 60, 60]]
    m, v = vr.vote(b, s, keep, 0.1, "score", 1.0)                               # weights 3, 2, 1 (and 0 for the last)
    assert v.tolist() == [3, 0, 0, 1] and np.array_equal(m[3], b[3])            # sw == 0: its own box
    assert np.array_equal(m[0], np.array([(3 * 0 + 2 * 2 + 8) / 6, 0, (30 + 24 + 18) / 6, 10], np.float32))
    m, v = vr.vote(b, s, keep, 0.1, "uniform", 2.5)                             # the third box is not live
    assert v.tolist() == [2, 0, 0, 1]
    m, v = vr.vote(b, s, keep, 0.1, group=[0, 1, 0, 0])
    assert v.tolist() == [2, 0, 0, 1] and m[0].tolist() == [4, 0, 14, 10]
    m, v = vr.vote(f([3, 3, 3, 3]), [1.0], [1])                                 # no area: iou 0 with itself, its own voter
    assert v.tolist() == [1] and m.tolist() == [[3, 3, 3, 3]]
    bx = wb.Boxes(b, scores=s, tag=np.arange(4))
    out = vr.merge(bx, 0.1, vote_iou=0.5)
    assert out.get_field("votes").tolist() == [2, 1] and out.get_field("tag").tolist() == [0, 3] and out.get_field("scores").tolist() == [4, 1]
    assert len(vr.merge(bx, 0.1, vote_iou=0.5, min_votes=2)) == 1 and len(vr.merge(bx, 0.1, vote_iou=0.5, min_votes=3)) == 0


def test_vote_boxes_and_merge_detections_check_their_arguments_before_the_device():
    b, s, k = f(A, A), np.array([1, 2], "f"), [0, 1]
    bad = [dict(vote_iou=-0.1), dict(vote_iou=float("nan")), dict(weights="scores"), dict(weights="score"), dict(weights=1),
           dict(score_threshold=float("nan")), dict(group=[0]), dict(group=[0, 1, 2])]
    for kw in bad:
        with pytest.raises(ValueError):
            wbb.vote_boxes(b, s, k, **kw)
        with pytest.raises(ValueError):
            wbb.merge_detections(wb.Boxes(b, scores=s), **kw)
    for args in ((b, s[:1], k), (b, s, [1]), (b, s, [1, 0, 1]), (f([0, 0, np.inf, 1], A), s, k), (f([0, np.nan, 1, 1], A), s, k),
                 (b, np.array([np.nan, 1], "f"), k)):
        with pytest.raises(ValueError):
            wbb.vote_boxes(*args)
    bx = wb.Boxes(b, scores=s)
    for kw in (dict(iou_threshold=-1), dict(min_votes=-1), dict(min_votes=1.5)):
        with pytest.raises(ValueError):
            wbb.merge_detections(bx, **kw)
    with pytest.raises(ValueError):
        wbb.merge_detections(wb.Boxes(b))                                       # no scores
    with pytest.raises(ValueError):
        wbb.merge_detections(wb.Boxes(f([0, 0, np.inf, 1], A), scores=s))


def _suppression_entry_points():
    """name -> (the call, taking boxes.suppression's keyword names, and which of them it takes)."""
    image = np.zeros((64, 64), np.uint8)
    M = wb.Model((8, 8, 4), wb.default_channel_opts)
    reg = regression.BoxRegressor((8, 8, 4), np.zeros((256, 4)), np.zeros(4))
    b, s, k = f(A, A), np.array([1, 2], "f"), [0, 1]
    bx = wb.Boxes(b, scores=s)
    nms = {"iou_threshold", "score_threshold"}
    voting = nms | {"vote_iou", "weights", "min_votes"}
    detect_kw = lambda kw: {"vote_weights" if key == "weights" else key: v for key, v in kw.items()}
    return {"non_max_suppression": (lambda **kw: wbb.non_max_suppression(bx, **kw), nms),
            "nms_keep_mask": (lambda **kw: wbb.nms_keep_mask(b, s, **kw), nms),
            "vote_boxes": (lambda **kw: wbb.vote_boxes(b, s, k, **kw), {"score_threshold", "vote_iou", "weights"}),
            "merge_detections": (lambda **kw: wbb.merge_detections(bx, **kw), voting),
            "Model.detect": (lambda **kw: M.detect(image, **detect_kw(kw)), voting),
            "Model.detect_batch": (lambda **kw: M.detect_batch(image[None], **kw), nms),
            "Model.detect_stream": (lambda **kw: next(M.detect_stream([image], **kw)), nms),
            "waldboost_amd.detect": (lambda **kw: wb.detect(image, M, **detect_kw(kw)), voting),
            "detect_and_refine": (lambda **kw: regression.detect_and_refine(image, M, reg, **detect_kw(kw)), voting)}


@pytest.mark.parametrize("key,value,takers", [("iou_threshold", -1.0, 8), ("iou_threshold", float("nan"), 8), ("score_threshold", float("nan"), 9),
                                              ("vote_iou", -0.5, 5), ("weights", "best", 5), ("min_votes", 1.5, 4)])
def test_every_entry_point_refuses_a_bad_scalar_in_the_same_words(key, value, takers):
    """One statement of the suppression arguments (boxes.suppression): whichever call is given the bad value says the same,
    and says it before the device is touched (this test needs no GPU)."""
    said = {}
    for name, (call, takes) in _suppression_entry_points().items():
        if key not in takes:
            continue
        kw = dict(iou_threshold=0.3, vote_iou=0.5) if key in ("weights", "min_votes") else dict(iou_threshold=0.3)
        kw[key] = value
        with pytest.raises(ValueError) as e:
            call(**{k: v for k, v in kw.items() if k in takes})
        said[name] = str(e.value)
    assert len(said) == takers and len(set(said.values())) == 1, said
    with pytest.raises(ValueError) as e:
        wbb.suppression(**dict(dict(iou_threshold=0.3, vote_iou=0.5), **{key: value}))
    assert str(e.value) in said.values()


def test_an_empty_input_never_touches_the_device():
    m, v = wbb.vote_boxes(np.zeros((0, 4), "f"), np.zeros(0, "f"), np.zeros(0, np.uint8), weights="score", score_threshold=0.0)
    assert m.shape == (0, 4) and m.dtype == np.float32 and v.shape == (0,) and v.dtype == np.int32
    out = wbb.merge_detections(wb.Boxes(np.zeros((0, 4), "f"), scores=np.zeros(0, "f"), label=np.zeros(0, np.int64)), group=np.zeros(0, int))
    assert len(out) == 0 and set(out.fields()) == {"scores", "label", "votes"} and out.get_field("votes").dtype == np.int32


def test_the_package_exports_merge_detections_and_needs_a_gpu_to_compute():
    assert "merge_detections" in wb.__all__ and wb.merge_detections is wbb.merge_detections
    assert "NOT run" in wbb.merge_detections.__doc__                            # min_votes does not run NMS again, and says so
    if not __import__("torch").cuda.is_available():
        with pytest.raises(nat.NativeError):
            wbb.vote_boxes(f(A), [1.0], [1])
        with pytest.raises(nat.NativeError):
            wb.merge_detections(wb.Boxes(f(A), scores=np.ones(1, "f")))


def test_the_header_declares_the_symbol_and_the_binding_follows():
    header = open(os.path.join(os.path.dirname(nat.__file__), "..", "include", "waldboost_hip.h")).read()
    assert "int wb_vote_launch(void *stream," in header and "#define WB_ABI_VERSION 8" in header
    assert "#define WB_VOTE_UNIFORM 0" in header and "#define WB_VOTE_SCORE 1" in header
    decl = header[header.index("int wb_vote_launch("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == 12
    res, args = nat.SYMBOLS["wb_vote_launch"]
    P = C.c_void_p
    assert res is C.c_int and args == [P, P, P, P, P, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_float, P, P]
    assert (nat.WB_VOTE_UNIFORM, nat.WB_VOTE_SCORE) == (0, 1) and wbb.VOTE_WEIGHTS == ("uniform", "score") and nat.WB_ABI_VERSION == 8
    assert hasattr(nat.load(), "wb_vote_launch")
    comment = header[:header.index("int wb_vote_launch(")][-4000:]
    for phrase in ("K * n", "j == k", "lane ^ s", "sw > 0", "votes = 0"):       # the rule and the cost stand in the header
        assert phrase in comment, phrase


def test_the_vote_kernel_uses_no_scratch_memory():
    nat.load()
    sizes = _kernel_scratch_sizes(open(nat.LIB_PATH, "rb").read())
    mine = {k: v for k, v in sizes.items() if "vote_kernel" in k}
    assert len(mine) == 1 and set(mine.values()) == {0}, mine


def test_the_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = nat.load()
    fake, odd, eight = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4104)    # (never dereferenced: refused before any HIP call)

    def vote(boxes=fake, scores=fake, group=fake, keep=fake, n=5, t=0.5, weights=0, use=0, thr=0.0, merged=fake, votes=fake):
        return lib.wb_vote_launch(None, boxes, scores, group, keep, n, t, weights, use, thr, merged, votes)
    assert vote(n=0, boxes=None, scores=None, group=None, keep=None, merged=None, votes=None) == 0          # nothing to do: no launch
    for kw in (dict(boxes=None), dict(scores=None), dict(keep=None), dict(merged=None), dict(votes=None), dict(boxes=eight), dict(merged=eight),
               dict(scores=odd), dict(group=odd), dict(votes=odd), dict(n=-1), dict(t=-0.5), dict(t=float("nan")), dict(weights=2),
               dict(weights=-1), dict(weights=1), dict(use=1, thr=float("nan")), dict(n=0, t=float("nan")), dict(n=0, weights=1)):
        assert vote(**kw) == nat.WB_ERR_INVALID, kw
        assert b"wb_vote_launch" in lib.wb_last_error()
    assert vote(n=(1 << 26) + 1) == nat.WB_ERR_UNSUPPORTED
    assert vote(n=(1 << 26) + 1, boxes=None) == nat.WB_ERR_INVALID


def test_the_detect_calls_have_the_keywords_with_off_defaults():
    for fn in (wb.Model.detect, wb.detect, regression.detect_and_refine):
        p = inspect.signature(fn).parameters
        assert (p["vote_iou"].default, p["vote_weights"].default, p["min_votes"].default) == (None, "uniform", 1), fn
        assert "round trip" in fn.__doc__, fn
    for fn in (wb.Model.detect_stream, wb.Model.detect_batch):
        assert "vote_iou" not in inspect.signature(fn).parameters
    p = inspect.signature(wbb.vote_boxes).parameters
    assert [p[k].default for k in ("vote_iou", "weights", "score_threshold", "group")] == [0.5, "uniform", None, None]
    p = inspect.signature(wbb.merge_detections).parameters
    assert [p[k].default for k in ("iou_threshold", "score_threshold", "group", "vote_iou", "weights", "min_votes")] == [0.5, None, None, 0.5, "uniform", 1]


def test_vote_iou_without_an_iou_threshold_raises_before_anything_runs():
    image = np.zeros((64, 64), np.uint8)
    M = wb.Model((8, 8, 4), wb.default_channel_opts)
    reg = regression.BoxRegressor((8, 8, 4), np.zeros((256, 4)), np.zeros(4))
    calls = (lambda **kw: M.detect(image, **kw), lambda **kw: wb.detect(image, M, **kw), lambda **kw: regression.detect_and_refine(image, M, reg, **kw))
    for call in calls:
        for kw in (dict(vote_iou=0.5), dict(vote_iou=0.5, score_threshold=None, vote_weights="score"), dict(iou_threshold=0.3, vote_iou=-1.0),
                   dict(iou_threshold=0.3, vote_iou=float("nan")), dict(iou_threshold=0.3, vote_iou=0.5, vote_weights="score"),
                   dict(iou_threshold=0.3, vote_iou=0.5, vote_weights="best"), dict(iou_threshold=0.3, vote_iou=0.5, min_votes=-2)):
            with pytest.raises(ValueError):
                call(**kw)
