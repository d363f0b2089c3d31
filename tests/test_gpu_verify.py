"""Verifier.predict and detect_and_verify on the GPU against the NumPy contract (tests/verify_reference.py): seeded random
weights with non-trivial batch-normalisation statistics, random float32 and uint8 crops, equal as float32 values (-0 and
+0 alike); chunked and unchunked predict equal; detect_and_verify returns Model.detect's boxes and the contract's scores
on the crops gather_samples cuts for the same detections."""
import os

import numpy as np
import pytest
import torch

import verify_reference as ref
import waldboost_amd as wb
from waldboost_amd import verification as ver
from waldboost_amd.samples import gather_samples
from util import GOLDEN

pytestmark = pytest.mark.gpu

N = 300


def random_verifier(shape, seed):
    """model_cnn(seed) with non-trivial biases and batch-normalisation statistics (gammas of both signs)."""
    rng = np.random.default_rng(seed)
    arrays = ver.model_cnn(shape, seed=seed).get_weights()
    for k in range(4):
        cout = arrays[6 * k + 1].size
        arrays[6 * k + 1] = (rng.standard_normal(cout) * 0.1).astype("f")
        arrays[6 * k + 2] = rng.uniform(0.5, 1.5, cout).astype("f") * rng.choice([-1, 1], cout, p=[0.25, 0.75]).astype("f")
        arrays[6 * k + 3] = (rng.standard_normal(cout) * 0.2).astype("f")
        arrays[6 * k + 4] = (rng.standard_normal(cout) * 0.3).astype("f")
        arrays[6 * k + 5] = rng.uniform(0.2, 2.0, cout).astype("f")
    arrays[25] = (rng.standard_normal(128) * 0.1).astype("f")
    arrays[27] = np.array([0.25], "f")
    return ver.Verifier.from_keras_weights(shape, arrays, epsilon=1e-3)


def contract(V, X, H):
    return ref.predict(V.get_weights(), V.epsilon, X, H)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape", [(12, 12, 4), (14, 14, 1), (13, 15, 3), (32, 32, 16)], ids=str)
def test_predict_equals_the_contract(shape, dtype):
    rng = np.random.default_rng(sum(shape))
    V = random_verifier(shape, seed=shape[0] + shape[2])
    if dtype == np.uint8:
        X = rng.integers(0, 256, (N,) + shape).astype(np.uint8)
    else:
        X = (rng.standard_normal((N,) + shape) * rng.choice([0.01, 1.0, 30.0], (N, 1, 1, 1))).astype(np.float32)
        X[rng.random(X.shape) < 0.05] = 0.0
    H = (rng.standard_normal(N) * 3).astype(np.float32)
    want = contract(V, X, H)
    assert np.isfinite(want).all() and np.unique(want).size > N // 2
    got = V.predict([X, H])
    assert got.shape == (N, 1) and got.dtype == np.float32
    assert np.array_equal(got[:, 0], want), np.flatnonzero(got[:, 0] != want)
    # chunked and unchunked, host arrays and device tensors, (N,) and (N, 1) scores: the same bits
    base = got.view(np.uint32)
    for batch in (1, 64, 100, 299):
        again = V.predict([torch.from_numpy(X).cuda(), H.reshape(-1, 1)], batch_size=batch)
        assert np.array_equal(again.view(np.uint32), base), batch
    dev = V.predict_device([X, torch.from_numpy(H).cuda()])
    assert dev.is_cuda and dev.shape == (N, 1) and np.array_equal(dev.cpu().numpy().view(np.uint32), base)
    assert V.predict([X[:0], H[:0]]).shape == (0, 1)


def _check_detect_and_verify(M, img):
    V = random_verifier(tuple(M.shape), seed=11)
    M.reset()
    bbs, scores = ver.detect_and_verify(img, M, V)
    n_loc, n_weak = M.n_loc, M.n_weak
    M.reset()
    res = M.detect_raw(img)
    assert (n_loc, n_weak) == (M.n_loc, M.n_weak) and n_loc > 0          # the statistics advance as in a scan
    assert res["scores"].size > 0
    assert bbs.dtype == np.float32 and bbs.shape == (res["scores"].size, 4) and np.array_equal(bbs, res["boxes"])
    assert scores.dtype == np.float32 and scores.shape == res["scores"].shape
    levels = list(M.channels(img))
    X = np.concatenate([gather_samples(levels[lv][0], res["r"][res["level"] == lv], res["c"][res["level"] == lv], M.shape)
                        for lv in np.unique(res["level"])])
    want = contract(V, X, res["scores"])
    assert np.array_equal(scores, want), np.flatnonzero(scores != want)
    return X.dtype


def test_detect_and_verify_on_float_channels():
    M = wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    img = np.load(os.path.join(GOLDEN, "mixed_200x264.npz"))["image"]
    assert _check_detect_and_verify(M, img) == np.float32


def test_detect_and_verify_on_uint8_channels():
    M = wb.load(os.path.join(GOLDEN, "grad_hist_4_u1_d2_T24.pb"))
    img = np.load(os.path.join(GOLDEN, "grad_hist_4_u1_200x264.npz"))["image"]
    assert _check_detect_and_verify(M, img) == np.uint8


@pytest.mark.parametrize("name", ["mixed", "grad_hist_4_u1"])
def test_the_three_calls_behind_one_scan_front_report_the_same_detections(name):
    """detect_and_verify, detect_and_refine (a regressor of zero weights moves no box; no NMS) and get_samples_from_image
    (no ground truth, uncapped: every window is yielded) scan through Model.scan_resident: the same boxes and scores, bit
    for bit and in one order, the same n_loc / n_weak; an image too small for any level is each call's empty value."""
    from waldboost_amd import regression
    from waldboost_amd.samples import get_samples_from_image
    M = wb.load(os.path.join(GOLDEN, name + "_d2_T24.pb"))
    img = np.load(os.path.join(GOLDEN, name + "_200x264.npz"))["image"]
    reg = regression.BoxRegressor(M.shape, np.zeros((int(np.prod(M.shape)), 4)), np.zeros(4))
    calls = {"verify": lambda im: ver.detect_and_verify(im, M, random_verifier(tuple(M.shape), seed=11))[0],
             "refine": lambda im: regression.detect_and_refine(im, M, reg),
             "samples": lambda im: wb.concatenate(list(get_samples_from_image(M, im, None, max_fp_candidates=10 ** 9)), ["scores"])}
    M.reset()
    want = M.detect_raw(img)
    counts = (M.n_loc, M.n_weak)
    assert want["scores"].size >= 3 and counts[0] > 0
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for what, call in calls.items():
        M.reset()
        got = call(img)
        assert (M.n_loc, M.n_weak) == counts, what
        boxes = got if what == "verify" else got.get()
        assert boxes.dtype == np.float32 and np.array_equal(u32(boxes), u32(want["boxes"])), what
        if what != "verify":                                                    # (the verifier's scores are its own)
            assert np.array_equal(u32(got.get_field("scores")), u32(want["scores"])), what
        M.reset()
        tiny = call(np.zeros((8, 8), np.uint8))
        assert len(tiny) == 0 and (M.n_loc, M.n_weak) == (0, 0), what
    assert calls["refine"](np.zeros((8, 8), np.uint8)).fields() == ["scores"]
    assert list(get_samples_from_image(M, np.zeros((8, 8), np.uint8), None)) == []


def test_detect_and_verify_without_detections_and_with_the_wrong_shape():
    M = wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    img = np.load(os.path.join(GOLDEN, "mixed_200x264.npz"))["image"]
    V = random_verifier(tuple(M.shape), seed=11)
    # an image too small for any level
    assert ver.detect_and_verify(np.zeros((8, 8), np.uint8), M, V) == ([], [])
    # a model that rejects everything
    g = np.load(os.path.join(GOLDEN, "reject_200x264.npz"))
    R = wb.Model(M.shape, M.channel_opts)
    for w, t in zip(M.classifier, g["theta"]):
        R.append(w, float(t))
    assert ver.detect_and_verify(img, R, V) == ([], [])
    assert R.n_loc == int(g["n_loc"]) and R.n_weak == int(g["n_weak"])
    # the verifier is for another window
    m, n, Cc = M.shape
    with pytest.raises(ValueError):
        ver.detect_and_verify(img, M, random_verifier((m, n + 1, Cc), seed=1))
    with pytest.raises(ValueError):
        ver.detect_and_verify(img, M, random_verifier((m, n, Cc + 1), seed=1))
