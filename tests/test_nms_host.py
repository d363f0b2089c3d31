"""Non-maximum suppression, the parts that need no GPU: the NumPy yardstick against answers written by hand, the
argument checks and scratch sizes of the new exports, and the Python surface's signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.boxes import Boxes
from nms_reference import detector_like_boxes, hand_cases, nms_boxes, nms_keep

HAND = list(hand_cases())


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_yardstick_against_hand_written_answers(case):
    _, boxes, scores, t, group, st, expected = case
    assert nms_keep(boxes, scores, t, group, st).astype(int).tolist() == expected


def test_yardstick_equals_the_full_matrix_form_on_detector_like_boxes():
    from waldboost_amd.boxes import iou
    boxes, scores = detector_like_boxes(300, 4)
    _, counts = np.unique(scores, return_counts=True)
    assert counts[counts > 1].sum() > 0.9 * scores.size            # ties dominate
    full = iou(Boxes(boxes), Boxes(boxes))
    for t in (0.0, 0.2, 0.5):
        keep = np.zeros(300, bool)
        dead = np.zeros(300, bool)
        for i in np.argsort(-scores, kind="stable"):
            if not dead[i]:
                keep[i] = True
                dead |= full[i] > t
        got = nms_keep(boxes, scores, t)
        assert np.array_equal(got, keep) and 0 < got.sum() < 300


def test_nms_exports_reject_bad_arguments_without_a_device():
    lib = nat.load()
    assert lib.wb_abi_version() == 8
    buf = (C.c_uint8 * 4096)()
    a = C.addressof(buf)
    a += (-a) % 16                                                  # a 16-byte aligned host address: never dereferenced
    big = 1 << 30
    ok = dict(stream=None, boxes=a, scores=a, group=None, n=8, t=0.5, use=0, st=0.0, scratch=a, nbytes=big, keep=a, n_keep=a)

    def launch(**kw):
        p = dict(ok, **kw)
        return lib.wb_nms_launch(p["stream"], p["boxes"], p["scores"], p["group"], p["n"], p["t"], p["use"], p["st"], p["scratch"],
                                 p["nbytes"], p["keep"], p["n_keep"])

    for bad in (dict(boxes=None), dict(scores=None), dict(keep=None), dict(n_keep=None), dict(scratch=None), dict(n=-1),
                dict(t=float("nan")), dict(t=-0.1), dict(nbytes=64), dict(boxes=a + 4), dict(scratch=a + 8), dict(scores=a + 2),
                dict(use=1, st=float("nan"))):
        assert launch(**bad) == nat.WB_ERR_INVALID, bad
        assert lib.wb_last_error().startswith(b"wb_nms_launch"), (bad, lib.wb_last_error())
    assert launch(n=(1 << 16) + 1) == nat.WB_ERR_UNSUPPORTED       # (the quadratic rank pass: wb_nms_ordered_launch above)

    def ordered(**kw):
        p = dict(dict(ok, order=a), **kw)
        return lib.wb_nms_ordered_launch(p["stream"], p["boxes"], p["scores"], p["group"], p["order"], p["n"], p["t"], p["use"], p["st"],
                                         p["scratch"], p["nbytes"], p["keep"], p["n_keep"])

    for bad in (dict(order=None), dict(order=a + 2), dict(boxes=None), dict(n=-1), dict(t=float("nan")), dict(nbytes=64), dict(scratch=None)):
        assert ordered(**bad) == nat.WB_ERR_INVALID, bad
        assert lib.wb_last_error().startswith(b"wb_nms_ordered_launch"), (bad, lib.wb_last_error())
    assert ordered(n=(1 << 26) + 1) == nat.WB_ERR_UNSUPPORTED

    okf = dict(fin=a, cap=64, images=1, t=0.5, use=0, st=0.0, scratch=a, nbytes=big, result=a)

    def finish(**kw):
        p = dict(okf, **kw)
        return lib.wb_nms_finish_launch(None, p["fin"], p["cap"], p["images"], p["t"], p["use"], p["st"], p["scratch"], p["nbytes"],
                                        p["result"])

    for bad in (dict(fin=None), dict(result=None), dict(scratch=None), dict(cap=62), dict(cap=0), dict(images=0), dict(t=float("nan")),
                dict(t=-1.0), dict(nbytes=1024), dict(fin=a + 8), dict(result=a + 2)):
        assert finish(**bad) == nat.WB_ERR_INVALID, bad
        assert lib.wb_last_error().startswith(b"wb_nms_finish_launch"), (bad, lib.wb_last_error())
    need = C.c_size_t()
    assert lib.wb_nms_scratch_bytes(-1, C.byref(need)) == nat.WB_ERR_INVALID
    assert lib.wb_nms_scratch_bytes(8, None) == nat.WB_ERR_INVALID
    assert lib.wb_nms_finish_scratch_bytes(64, 0, C.byref(need)) == nat.WB_ERR_INVALID


def test_nms_scratch_sizes():
    """wb_nms_scratch_bytes is monotone in n and at least the documented layout: 25 bytes per box and 16 per 64 boxes, 16
    of counters, then 64 rows of ceil(n / 64) words; up to 4096 boxes the whole matrix (n64 rows)."""
    lib = nat.load()
    need = C.c_size_t()
    last = 0
    for n in list(range(0, 200)) + [1000, 4095, 4096, 4097, 20000, 65536, 100000, 1 << 20, 1 << 26]:
        assert lib.wb_nms_scratch_bytes(n, C.byref(need)) == 0
        n64 = max((n + 63) // 64 * 64, 64)
        W = n64 // 64
        fixed = 25 * n64 + 16 * W + 16
        assert need.value >= fixed + 64 * W * 8, n
        if n <= 4096:
            assert need.value >= fixed + n64 * W * 8, n
        assert need.value >= last, n
        last = need.value
    assert last < (1 << 26) * 25 + (16 << 20) + 512 + (1 << 29) + 1    # (the matrix is banded -- 64 rows of 8 MiB there --, not n x n / 8 bytes)
    assert lib.wb_nms_scratch_bytes((1 << 26) + 1, C.byref(need)) == nat.WB_ERR_UNSUPPORTED
    one, four = C.c_size_t(), C.c_size_t()
    assert lib.wb_nms_finish_scratch_bytes(4096, 1, C.byref(one)) == 0 and lib.wb_nms_finish_scratch_bytes(4096, 4, C.byref(four)) == 0
    assert four.value == 4 * one.value and one.value >= 25 * 4096 + 4096 * 64 * 8


def test_non_max_suppression_of_nothing_is_nothing():
    assert "non_max_suppression" in wb.__all__ and wb.non_max_suppression is wb.boxes.non_max_suppression
    empty = Boxes(np.empty((0, 4), "f"), scores=np.empty(0, "f"), label=np.empty(0, np.int64))
    out = wb.non_max_suppression(empty, iou_threshold=0.2)
    assert isinstance(out, Boxes) and len(out) == 0 and set(out.fields()) == {"scores", "label"}
    with pytest.raises(ValueError):
        wb.non_max_suppression(Boxes(np.zeros((1, 4), "f")))        # no scores


def test_non_max_suppression_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    boxes, scores = detector_like_boxes(10, 0)
    with pytest.raises(nat.NativeError):
        wb.non_max_suppression(Boxes(boxes, scores=scores), 0.2)


def test_detect_entry_points_take_the_nms_keywords():
    for fn in (wb.Model.detect, wb.Model.detect_stream, wb.Model.detect_batch, wb.detect):
        p = inspect.signature(fn).parameters
        assert p["iou_threshold"].default is None and p["score_threshold"].default is None, fn
    assert inspect.signature(wb.detect).parameters["separate"].default is False
    p = inspect.signature(wb.non_max_suppression).parameters
    assert list(p) == ["boxes", "iou_threshold", "score_threshold", "group"]
    assert p["iou_threshold"].default == 0.5 and p["score_threshold"].default is None and p["group"].default is None
    M = wb.Model((4, 4, 4), dict(wb.default_channel_opts))
    with pytest.raises(ValueError):
        M.detect(np.zeros((64, 64), np.uint8), score_threshold=0.0)  # a score threshold alone is not a suppression
    with pytest.raises(ValueError):
        M.detect(np.zeros((64, 64), np.uint8), iou_threshold=float("nan"))


def test_yardstick_on_the_recorded_reference_detections():
    """The counts the fixtures' reference detections give (and that every GPU comparison starts from)."""
    import os
    from util import GOLDEN
    want = {"cfg1_640x480": (855, 85, 198, 366), "mixed_200x264": (275, 18, 51, 114)}
    for name, (n, k0, k2, k5) in want.items():
        d = np.load(os.path.join(GOLDEN, name + ".npz"))["det"]
        bx = Boxes(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], 1), scores=d["score"])
        assert len(bx) == n
        assert [len(nms_boxes(bx, t)) for t in (0.0, 0.2, 0.5)] == [k0, k2, k5]
