"""Evaluator.evaluate and evaluate_model on the GPU against tests/eval_reference.py, the per-image NumPy statement: planted data
fed through add_detections / add_ground_truth (detector-like boxes, ground truth copied from some of them with jitter, some
of it ignored, one image without ground truth, one without detections), the same with one image beyond the NMS chunk limit,
and a model run end to end.  The dicts must be equal, lists bit for bit."""
import functools
import os

import numpy as np
import pytest

import waldboost_amd as wb
from eval_reference import evaluate_images, same_dict
from nms_reference import detector_like_boxes
from util import GOLDEN
from waldboost_amd.boxes import Boxes
from waldboost_amd.synth import synth_image
from waldboost_amd.testing import Evaluator, _nms_chunks, detect_on_images, evaluate_model

pytestmark = pytest.mark.gpu

SHAPE = (1080, 1920)
SETTINGS = {"default": {}, "normalize_ar": dict(normalize_ar=1.0), "min_gt_area": dict(min_gt_area=2500.0),
            "thresholds": dict(match_iou_threshold=0.3, dt_iou_threshold=0.2, min_gt_area_in_image=0.9)}


def planted_image(k, n):
    """n detector-like detections; ground truth: every 9th detection moved and stretched by a few pixels (doubles that are no
    float32 values), every 4th of those ignored; box 0 of odd images ignored as well (it owns what overlaps nothing)."""
    rng = np.random.default_rng(1000 + k)
    boxes, scores = detector_like_boxes(n, 50 + k)
    dt = Boxes(boxes, scores=scores)
    src = boxes[::9].astype(np.float64)
    gt = src + rng.uniform(-3, 3, src.shape) * (src[:, 2:3] - src[:, 0:1]) / 24
    ignore = (np.arange(len(gt)) % 4 == 3).astype(np.float64)
    if k % 2:
        ignore[0] = 1
    return Boxes(gt, ignore=ignore), dt, SHAPE


@functools.lru_cache(None)
def planted_images(big=False):
    out = [planted_image(k, 250 + 20 * k) for k in range(12)]
    out[4] = (Boxes(np.empty((0, 4)), ignore=np.empty(0)), out[4][1], SHAPE)                          # no ground truth
    out[7] = (out[7][0], Boxes(np.empty((0, 4), "f"), scores=np.empty(0, "f")), SHAPE)                # no detections
    if big:
        out = out[:3] + [planted_image(20, 5000)] + out[3:6]
    return tuple(out)


@functools.lru_cache(None)
def reference(big, setting):
    details = {}
    return evaluate_images(planted_images(big), details=details, **SETTINGS[setting]), details


def evaluator_of(images):
    E = Evaluator()
    for idx, (gt, dt, shape) in enumerate(images):
        E.add_detections(idx, dt)                              # (either order of the two calls)
        E.add_ground_truth(idx, gt, shape)
    return E


def show(ref, got):
    return {k: (ref[k], got[k]) for k in ("auc", "n_eval", "n_ign")} | {"points": (len(ref["precision"]), len(got["precision"]))}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_evaluate_equals_the_per_image_statement(setting):
    ref, details = reference(False, setting)
    # not vacuous, on the reference's own output
    assert details["tp"] >= 1 and details["fp"] >= 1 and details["dropped"] >= 1 and details["suppressed"] >= 1, details
    assert 0 < ref["auc"] < 1 and ref["n_ign"] >= 1 and ref["n_eval"] >= 1 and len(ref["threshold"]) > 5
    if setting == "min_gt_area":
        assert ref["n_ign"] > reference(False, "default")[0]["n_ign"]
    got = evaluator_of(planted_images()).evaluate(**SETTINGS[setting])
    assert same_dict(ref, got), show(ref, got)
    assert isinstance(got["precision"], list) and isinstance(got["recall"], list) and isinstance(got["threshold"], list)
    assert got["iou_threshold"] == SETTINGS[setting].get("match_iou_threshold", 0.5)


def test_evaluate_with_an_image_beyond_the_nms_chunk_limit():
    images = planted_images(True)
    counts = [len(dt) for _, dt, _ in images]
    chunks = _nms_chunks(counts)
    assert max(counts) == 5000 and (3, 4) in chunks and len(chunks) >= 3       # the big image alone, others together
    ref, details = reference(True, "default")
    assert details["tp"] >= 1 and details["fp"] >= 1 and details["dropped"] >= 1 and details["suppressed"] >= 1, details
    got = evaluator_of(images).evaluate()
    assert same_dict(ref, got), show(ref, got)


def test_evaluate_model_end_to_end():
    """cfg1_d1_T32.pb on three 200 x 264 images; ground truth from the model's own strongest detections, moved a little, the
    last of each image ignored.  lanes / batch change nothing, and the result is the per-image statement's on
    detect_on_images' own tuples."""
    M, N = wb.load(os.path.join(GOLDEN, "cfg1_d1_T32.pb")), wb.load(os.path.join(GOLDEN, "cfg1_d1_T32.pb"))
    ims = [synth_image(200, 264, 40 + i) for i in range(3)]
    dicts = []
    for i, im in enumerate(ims):
        d = M.detect(im)
        top = np.argsort(-d.get_field("scores"), kind="stable")[:4]
        gt = d.get()[top].astype(np.float64) + np.array([1.25, -0.75, 2.5, 0.5]) * (1 + i)
        dicts.append({"image": im, "groundtruth_boxes": Boxes(gt, ignore=(np.arange(len(gt)) == len(gt) - 1).astype(np.float64))})
    tuples = list(detect_on_images(dicts, M))
    assert all(len(dt) > 0 for _, dt, _ in tuples)
    details = {}
    ref = evaluate_images(tuples, details=details)
    assert details["tp"] >= 1 and details["fp"] >= 1 and details["suppressed"] >= 1, details
    E1 = evaluate_model(dicts, M)
    E2 = evaluate_model(dicts, N, lanes=2, batch=2)
    assert list(E1.eval_data) == list(E2.eval_data) == [1, 2, 3] and E1.eval_data[2]["shape"] == (200, 264)
    got1, got2 = E1.evaluate(), E2.evaluate()
    assert same_dict(got1, got2), show(got1, got2)
    assert same_dict(ref, got1), show(ref, got1)
    assert len(evaluate_model(dicts, M, num_images=2).eval_data) == 2
