"""The evaluation surface, the parts that need no GPU: the NumPy restatement of scikit-learn 0.24.2's precision / recall curve
and AUC against the recorded sklearn output (tests/golden/eval_curves.npz, written by make_golden_eval.py), the NMS chunk
planner, the three bbx stand-ins on answers computed by hand, the Evaluator's bookkeeping and argument errors,
random_iterator, and wb_match_launch's refusals at the C ABI."""
import ctypes as C
import inspect
import logging
import os
import warnings

import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd import testing as wt
from waldboost_amd.boxes import Boxes, boxes_in_window, set_aspect_ratio
from util import GOLDEN

CURVES = np.load(os.path.join(GOLDEN, "eval_curves.npz"))
NAMES = [str(n) for n in CURVES["names"]]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_curve_restatement_equals_recorded_sklearn_bit_for_bit(name):
    assert str(CURVES["sklearn_version"]) == "0.24.2" and "0.24.2" in wt._precision_recall_curve.__doc__
    y, s = CURVES[f"{name}/y_true"], CURVES[f"{name}/scores"]
    assert y.size <= 64
    p, r, t = wt._precision_recall_curve(y, s)
    assert same(p, CURVES[f"{name}/precision"]) and same(r, CURVES[f"{name}/recall"]) and same(t, CURVES[f"{name}/thresholds"])
    assert same(np.float64(wt._auc(r, p)), CURVES[f"{name}/auc"])
    try:
        import sklearn
        import sklearn.metrics
    except ImportError:
        return
    if sklearn.__version__ == "0.24.2":                        # the yardstick itself, live (later releases do not cut the curve)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            lp, lr, lt = sklearn.metrics.precision_recall_curve(y, s)
            la = sklearn.metrics.auc(lr, lp)
        assert same(p, lp) and same(r, lr) and same(t, lt) and same(np.float64(wt._auc(r, p)), np.float64(la))


def test_the_fixture_holds_the_cases_asked_for():
    y = lambda n: CURVES[f"{n}/y_true"]
    s = lambda n: CURVES[f"{n}/scores"]
    assert len(NAMES) >= 12
    assert len(np.unique(s("heavy-ties"))) < 16 and y("heavy-ties").size == 64
    assert y("all-positive").all() and y("single-positive").size == 1
    assert y("positives-lowest")[np.argsort(s("positives-lowest"))[:6]].all() and y("positives-lowest").sum() == 6
    assert s("float32-scores").dtype == np.float32 and CURVES["float32-scores/thresholds"].dtype == np.float32
    assert not y("no-positive").any() and np.isnan(CURVES["no-positive/recall"][0]) and np.isnan(CURVES["no-positive/auc"])
    # full recall cuts the curve: fewer points than distinct scores
    assert CURVES["positives-highest/thresholds"].size == 6 < len(np.unique(s("positives-highest")))


def test_curve_argument_errors():
    with pytest.raises(ValueError):
        wt._precision_recall_curve(np.zeros(0, bool), np.zeros(0))
    with pytest.raises(ValueError):
        wt._precision_recall_curve(np.ones(3, bool), np.zeros(2))
    with pytest.raises(ValueError):
        wt._precision_recall_curve(np.ones(2, bool), np.array([0.0, np.nan]))
    with pytest.raises(ValueError):
        wt._auc(np.array([1.0]), np.array([1.0]))
    with pytest.raises(ValueError):
        wt._auc(np.array([0.0, 1.0, 0.5]), np.array([1.0, 1.0, 1.0]))
    assert wt._auc(np.array([1.0, 0.5, 0.0]), np.array([0.5, 0.5, 1.0])) == 0.25 + 0.375


def test_nms_chunks_on_hand_cases():
    f = wt._nms_chunks
    assert inspect.signature(f).parameters["limit"].default == 4096
    assert f([4000, 96]) == [(0, 2)]                           # the total fits exactly
    assert f([4000, 97]) == [(0, 1), (1, 2)]
    assert f([10, 5000, 10]) == [(0, 1), (1, 2), (2, 3)]       # one image over the limit: a call of its own
    assert f([5000]) == [(0, 1)]
    assert f([0, 3, 0, 0, 4, 0], limit=6) == [(0, 4), (4, 6)]  # empty images ride along
    assert f([3, 0, 0], limit=3) == [(0, 3)]
    assert f([3, 3, 0, 0], limit=3) == [(0, 1), (1, 4)]
    assert f([0, 0, 0]) == [] and f([]) == []                  # nothing to suppress: no call
    assert f([2, 2, 2, 2, 2], limit=4) == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(ValueError):
        f([1, -1])
    # every image with boxes is in exactly one range, in order
    rng = np.random.default_rng(0)
    for _ in range(50):
        counts = rng.integers(0, 9, rng.integers(1, 12)).tolist()
        ch = f(counts, limit=10)
        seen = [k for lo, hi in ch for k in range(lo, hi)]
        assert seen == sorted(set(seen)) and {k for k, c in enumerate(counts) if c} <= set(seen)
        assert all(sum(counts[lo:hi]) <= 10 for lo, hi in ch) and all(sum(counts[lo:hi]) > 0 for lo, hi in ch)


def test_bbx_stand_ins_on_hand_computed_cases():
    b = Boxes(np.array([[0, 0, 4, 2], [1, 1, 1, 5], [-2, 0, 2, 4], [10, 10, 20, 30]], np.float32), tag=np.arange(4))
    assert b.area().dtype == np.float64 and b.area().tolist() == [8.0, 0.0, 16.0, 200.0]
    win = Boxes([0, 0, 20, 30])
    # inside; no area (0 >= 0); half outside; exactly filling the window's corner
    assert boxes_in_window(b, win).tolist() == [True, True, False, True]
    assert boxes_in_window(b, win, min_overlap=0.5).tolist() == [True, True, True, True]
    assert boxes_in_window(b, win, min_overlap=0.51).tolist() == [True, True, False, True]
    full = Boxes(np.array([[0, 0, 20, 30], [0, 0, 20.5, 30]]))
    assert boxes_in_window(full, win, min_overlap=1).tolist() == [True, False]      # a box exactly filling the window passes at 1
    assert boxes_in_window(Boxes(np.array([[30, 40, 50, 60]])), win, min_overlap=0).tolist() == [True]
    with pytest.raises(ValueError):
        boxes_in_window(b, Boxes(np.zeros((2, 4))))
    s = set_aspect_ratio(b, 4.0)                               # area 8 -> 5.65.. x 1.41..; area 16 -> 8 x 2; area 200 -> 28.28.. x 7.07..
    c = s.get()
    assert c.dtype == np.float64 and s.fields() == ["tag"] and s.get_field("tag").tolist() == [0, 1, 2, 3]
    assert c[2].tolist() == [-4.0, 1.0, 4.0, 3.0]              # centre (0, 2), 8 x 2
    assert c[1].tolist() == [1.0, 3.0, 1.0, 3.0]               # no area: its centre
    w, h = np.sqrt(8.0 * 4.0), np.sqrt(8.0 / 4.0)
    assert c[0].tolist() == [2 - w / 2, 1 - h / 2, 2 + w / 2, 1 + h / 2]
    sq = set_aspect_ratio(b, 1.0).get()
    assert sq[2].tolist() == [-2.0, 0.0, 2.0, 4.0] and sq[3].tolist() == [15 - np.sqrt(200.0) / 2, 20 - np.sqrt(200.0) / 2, 15 + np.sqrt(200.0) / 2,
                                                                         20 + np.sqrt(200.0) / 2]
    with pytest.raises(ValueError):
        set_aspect_ratio(b, 0.0)
    for fn in (Boxes.area, boxes_in_window, set_aspect_ratio):
        assert "unpinned upstream" in fn.__doc__


def test_evaluator_bookkeeping_and_argument_errors():
    E = wt.Evaluator()
    assert E.eval_data == {}
    gt = Boxes(np.array([[0, 0, 10, 10]]), ignore=np.zeros(1))
    dt = Boxes(np.empty((0, 4), "f"), scores=np.empty(0, "f"))
    E.add_ground_truth("a", gt, (20, 30))
    E.add_detections("a", dt)
    E.add_detections("b", dt)
    assert list(E.eval_data) == ["a", "b"] and E.eval_data["a"]["gt"] is gt and E.eval_data["a"]["shape"] == (20, 30)
    assert E.eval_data["a"]["dt"] is dt and set(E.eval_data["b"]) == {"dt"}
    with pytest.raises(KeyError):
        E.evaluate()                                           # image "b": detections but no ground truth entry
    E.clear()
    E.add_ground_truth(1, gt, (20, 30))
    with pytest.raises(KeyError):
        E.evaluate()                                           # the reverse
    E.add_detections(1, dt)
    with pytest.raises(ValueError):
        E.evaluate()                                           # no evaluated detections at all (and no device needed to say so)
    E.clear()
    assert E.eval_data == {}
    with pytest.raises(ValueError):
        E.evaluate()
    p = inspect.signature(wt.Evaluator.evaluate).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("match_iou_threshold", 0.5), ("dt_iou_threshold", 0.5), ("min_gt_area", 0),
                                                          ("min_gt_area_in_image", 1), ("normalize_ar", None)]
    p = inspect.signature(wt.evaluate_model).parameters
    assert [k for k in p] == ["testing_images", "model", "num_images", "shuffle", "lanes", "batch"]
    assert p["num_images"].default is None and p["shuffle"].default is False and p["lanes"].default == 1 and p["batch"].default == 1


def test_evaluate_model_without_images(caplog):
    with caplog.at_level(logging.WARNING):
        E = wt.evaluate_model([], num_images=3)
    assert isinstance(E, wt.Evaluator) and E.eval_data == {}
    assert "Requested test on 3 but only 0 images" in caplog.text
    with pytest.raises(ValueError):
        wt.evaluate_model(iter([]))                            # no length, no num_images


def test_random_iterator():
    seq = list(range(10, 17))
    it = wt.random_iterator(seq)
    first = [next(it) for _ in range(7)]
    again = [next(it) for _ in range(7)]
    assert sorted(first) == seq and again == first             # every element once per cycle, the cycles alike
    assert len(list(wt.random_iterator(seq, maxlen=3))) == 4   # (the reference's `i > maxlen`)
    assert list(wt.random_iterator([])) == []
    for bad in (iter(seq), (x for x in seq), 5):
        with pytest.raises(TypeError):
            next(wt.random_iterator(bad))


def test_match_boxes_surface_without_a_device():
    assert "match_boxes" in wb.__all__ and wb.match_boxes is wb.boxes.match_boxes
    assert list(inspect.signature(wb.match_boxes).parameters) == ["dt_boxes", "gt_boxes_per_image", "dt_image"]
    gt = Boxes(np.array([[0, 0, 10, 10.5]]))
    best, owner = wb.match_boxes(Boxes(np.empty((0, 4))), gt)  # no detections: no device
    assert best.shape == owner.shape == (0,) and best.dtype == np.float64 and owner.dtype == np.int32
    best, owner = wb.match_boxes(Boxes(np.empty((0, 4))), [gt, gt], np.zeros(0, np.int64))
    assert best.size == 0
    one = Boxes(np.array([[0, 0, 1, 1]]))
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 500, -2.0 ** 500):
        with pytest.raises(ValueError):
            wb.match_boxes(Boxes(np.array([[0, 0, 1, bad]])), gt)
        with pytest.raises(ValueError):
            wb.match_boxes(one, Boxes(np.array([[bad, 0, 1, 1]])))
    with pytest.raises(ValueError):
        wb.match_boxes(one, [gt])                              # a list needs dt_image
    with pytest.raises(ValueError):
        wb.match_boxes(one, gt, [0])                           # one pair takes none
    for bad in ([1], [-1], [0, 0], [0.0]):
        with pytest.raises(ValueError):
            wb.match_boxes(one, [gt], bad)


def test_match_boxes_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return                                                 # (tests/test_gpu_match_designs.py has the GPU's side)
    with pytest.raises(nat.NativeError):
        wb.match_boxes(Boxes(np.array([[0, 0, 1, 1]])), Boxes(np.array([[0, 0, 1, 1]])))


def test_match_export_rejects_bad_arguments_without_a_launch():
    lib = nat.load()
    assert lib.wb_abi_version() == 8
    buf = (C.c_uint8 * 256)()
    a = C.addressof(buf)
    a += (-a) % 16                                             # an aligned host address: never dereferenced
    ok = dict(dt=a, dt_image=a, gt=a, gt_off=a, n_dt=8, n_gt=4, n_images=2, best=a, owner=a)

    def launch(**kw):
        p = dict(ok, **kw)
        return lib.wb_match_launch(None, p["dt"], p["dt_image"], p["gt"], p["gt_off"], p["n_dt"], p["n_gt"], p["n_images"], p["best"], p["owner"])

    for bad in (dict(dt=None), dict(dt_image=None), dict(gt=None), dict(gt_off=None), dict(best=None), dict(owner=None), dict(n_dt=-1),
                dict(n_gt=-1), dict(n_images=-1), dict(n_images=0), dict(dt=a + 4), dict(gt=a + 4), dict(best=a + 4), dict(dt_image=a + 2),
                dict(gt_off=a + 2), dict(owner=a + 2), dict(n_dt=0, n_gt=-1)):
        assert launch(**bad) == nat.WB_ERR_INVALID, bad
        assert lib.wb_last_error().startswith(b"wb_match_launch"), (bad, lib.wb_last_error())
    assert launch(n_dt=(1 << 26) + 1) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_last_error().startswith(b"wb_match_launch")
    # no detections: success, nothing launched, pointers not looked at
    assert launch(n_dt=0) == 0 and launch(n_dt=0, dt=None, dt_image=None, gt=None, gt_off=None, best=None, owner=None, n_images=0) == 0
