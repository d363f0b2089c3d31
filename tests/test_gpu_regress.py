"""Box regression end to end on the GPU (waldboost_amd.regression) against the statement of tests/regress_reference.py:
targets, fit on the planted-square training images of the mining tests, detect_and_refine, the held-out improvement,
save / load, the errors, mixed image shapes and the accumulator's reuse."""
import functools
import os

import numpy as np
import pytest
import torch

import regress_designs as rd
import regress_reference as rr
import waldboost_amd as wb
from oracle import wb_oracle as orc
from test_gpu_mine import _training_images
from waldboost_amd import fpga, regression
from waldboost_amd.samples import mine_batch
from waldboost_amd.synth import synth_image
from util import GOLDEN

pytestmark = pytest.mark.gpu

HUGE = 10 ** 9
SHAPE = (8, 8, 4)
FLAVOURS = ["float", "fpga"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def empty_model(flavour):
    chn = wb.channels.grad_hist if flavour == "float" else fpga.grad_hist_4_u1
    return wb.Model(SHAPE, dict(shrink=2, n_per_oct=8, smooth=1, channels=chn))


@functools.lru_cache(None)
def statement_sets(flavour):
    """The CPU statement's windows (oracle pyramid) of the training and the held-out images."""
    opts = dict(shrink=2, n_per_oct=8, smooth=1, channels=orc.grad_hist if flavour == "float" else orc.grad_hist_4_u1)
    pyramid_of = lambda image: list(orc.channel_pyramid(image, opts))
    return (rr.image_set(rr.planted_images(range(6)), pyramid_of, SHAPE), rr.image_set(rr.planted_images(range(6, 12)), pyramid_of, SHAPE))


@functools.lru_cache(None)
def mined_training(flavour):
    """The six training images through one mine_batch, uncapped, and its host copies."""
    M = empty_model(flavour)
    items = _training_images()
    gts = [it["groundtruth_boxes"] for it in items]
    images = np.stack([it["image"] for it in items])
    mined = mine_batch(M, images, gts, tp=True, fp=False, min_tp_iou=0.5, max_tp_candidates=HUGE)
    scales = M.detect_raw(items[0]["image"])["scales"]
    return M, items, gts, mined, scales


@functools.lru_cache(None)
def fitted(flavour):
    M = empty_model(flavour)
    acc = regression.Accumulator(SHAPE, np.float32 if flavour == "float" else np.uint8)
    reg = regression.fit(M, _training_images(), max_candidates=HUGE, accumulator=acc)
    return M, acc, reg


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_targets_are_the_statement(flavour):
    M, items, gts, mined, scales = mined_training(flavour)
    assert len(mined) == 1313
    T = regression.targets(mined, gts, scales)
    assert T.is_cuda and T.dtype == torch.float64 and tuple(T.shape) == (1313, 4)
    h = lambda k: getattr(mined, k).cpu().numpy()
    off = np.cumsum([0] + [len(g) for g in gts])
    want = rr.targets(h("boxes"), np.concatenate([np.asarray(g.get(), np.float64) for g in gts]), off[h("image")] + h("instance_id"),
                      np.array(scales, np.float64)[h("level")])
    assert np.array_equal(bits(T.cpu().numpy()), bits(want))
    # the mined windows are the CPU statement's windows: same crops, boxes and targets, in the same order
    train = statement_sets(flavour)[0]
    assert np.array_equal(rr.features(h("samples")), train["X"]) and np.array_equal(bits(h("boxes")), bits(train["boxes"]))
    assert np.array_equal(bits(want), bits(train["T"]))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_fit_accumulates_the_statement_gram(flavour):
    """N == 1313 for the empty model; for uint8 channels the [X | 1] block of S is the integer Gram exactly; everything lies
    within (N + 8) * 2^-52 * (|A|^T |A|) of the exact Gram (the reference here is an 80-bit product sum, whose own error
    (N + 1) * 2^-63 * (|A|^T |A|) is taken off the bound)."""
    M, acc, reg = fitted(flavour)
    train = statement_sets(flavour)[0]
    N, D = train["X"].shape
    S = acc.state()
    assert acc.n == N == 1313 and S[D, D] == N and reg.n_samples == N and reg.input_shape == SHAPE
    assert np.array_equal(bits(S), bits(S.T))
    A = rr.design(train["X"], train["T"])
    if flavour == "fpga":
        Ai = A[:, :D + 1].astype(np.int64)
        assert np.array_equal(S[:D + 1, :D + 1], (Ai.T @ Ai).astype(np.float64))
    Al = A.astype(np.longdouble)
    exact = Al.T @ Al
    absgram = np.abs(A).T @ np.abs(A)
    err = np.abs(S.astype(np.longdouble) - exact).astype(np.float64)
    bound = ((N + 8) * 2.0 ** -52 - (N + 1) * 2.0 ** -63) * absgram
    print(f"{flavour}: largest |S - exact| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    # the solve is the statement's on the same S; against the statement's own float64 Gram the regressors differ by rounding
    W, b, rss, tss = rr.solve(S, 1e-2)
    assert np.array_equal(bits(reg.W), bits(W)) and np.array_equal(bits(reg.b), bits(b)) and (reg.rss <= reg.tss).all()
    W2, b2, _, _ = rr.solve(rr.gram(train["X"], train["T"]), 1e-2)
    held = statement_sets(flavour)[1]
    ours = rr.refine(held["boxes"], rr.predict(held["X"], W, b), 1.0 / held["scale"])
    theirs = rr.refine(held["boxes"], rr.predict(held["X"], W2, b2), 1.0 / held["scale"])
    print(f"{flavour}: largest difference between boxes refined by the GPU-fitted and the statement-fitted regressor: "
          f"{np.abs(ours.astype(np.float64) - theirs).max():.3g} pixels")
    # fitting again gives the same bits
    again = regression.fit(empty_model(flavour), _training_images(), max_candidates=HUGE)
    assert np.array_equal(bits(again.W), bits(reg.W)) and np.array_equal(bits(again.b), bits(reg.b))


def windows_of(M, image):
    """(raw result, crops (N, m, n, C)) of M's detections on image, the crops read from the pyramid the scan left resident."""
    from test_gpu_mine import engine_of
    res = M.detect_raw(image)
    eng = engine_of(M, image[None])
    eng.load_images(image)                                    # (whatever form of the pyramid the scan used: the channels themselves)
    eng.run_channels()
    m, n, C = M.shape
    levels = {}
    crops = np.zeros((res["scores"].size, m, n, C), np.dtype(str(eng.chn.dtype).replace("torch.", "")))
    for i, (l, r, c) in enumerate(zip(res["level"], res["r"], res["c"])):
        if int(l) not in levels:
            levels[int(l)] = eng.read_level(0, int(l))
        crops[i] = levels[int(l)][int(r):int(r) + m, int(c):int(c) + n]
    return res, crops


def statement_refine(M, image, reg):
    res, crops = windows_of(M, image)
    inv64 = np.array([1.0 / float(s) for s in res["scales"]])[res["level"]]
    return res, rr.refine(res["boxes"], rr.predict(rr.features(crops), reg.W, reg.b), inv64)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_detect_and_refine_is_the_statement_and_improves_held_out_boxes(flavour):
    """Boxes bit-equal to the statement's refine of Model.detect's boxes under the fitted W; scores and order untouched; on the
    held-out images (seeds 6 .. 11) the windows with IoU > 0.5 to a ground-truth box are better on average and for more
    than half of them."""
    M, acc, reg = fitted(flavour)
    raw_iou, ref_iou = [], []
    for it in rr.planted_images(range(6, 12)):
        plain = M.detect(it["image"])
        got = regression.detect_and_refine(it["image"], M, reg)
        res, want = statement_refine(M, it["image"], reg)
        assert np.array_equal(bits(plain.get()), bits(res["boxes"]))
        assert got.get().dtype == np.float32 and np.array_equal(bits(got.get()), bits(want))
        assert np.array_equal(bits(got.get_field("scores")), bits(plain.get_field("scores")))
        table = np.stack([rr.iou_rows(res["boxes"], np.broadcast_to(g, res["boxes"].shape)) for g in it["gt"]], 1)
        owner = table.argmax(1)
        keep = np.flatnonzero(table[np.arange(owner.size), owner] > 0.5)
        raw_iou.append(table[keep, owner[keep]])
        ref_iou.append(rr.iou_rows(got.get()[keep], it["gt"][owner[keep]]))
    raw_iou, ref_iou = np.concatenate(raw_iou), np.concatenate(ref_iou)
    print(f"{flavour}: held-out ({raw_iou.size} windows) mean IoU {raw_iou.mean():.3f} -> {ref_iou.mean():.3f}, "
          f"{(ref_iou > raw_iou).mean():.1%} improved")
    assert raw_iou.size == 1266
    assert ref_iou.mean() > raw_iou.mean() and (ref_iou > raw_iou).mean() > 0.5


@pytest.mark.parametrize("name", ["mixed_d2_T24.pb", "grad_hist_4_u1_d2_T24.pb"])
def test_detect_and_refine_with_a_trained_cascade_and_nms(name, tmp_path):
    """A golden cascade (window (12, 12, 4)) and a regressor of random weights: the statement's boxes in Model.detect's order,
    scores untouched; with thresholds, non_max_suppression of those refined boxes; the same after save / load."""
    M = wb.load(os.path.join(GOLDEN, name))
    W, b = rd.random_weights(M.shape, seed=4)
    reg = regression.BoxRegressor(M.shape, W * 0.05, b)
    image = synth_image(200, 264, 41)
    plain = M.detect(image)
    assert len(plain) >= 3
    got = regression.detect_and_refine(image, M, reg)
    res, want = statement_refine(M, image, reg)
    assert np.array_equal(bits(got.get()), bits(want)) and np.any(got.get() != plain.get())
    assert np.array_equal(bits(got.get_field("scores")), bits(plain.get_field("scores")))
    refined = wb.Boxes(want, scores=res["scores"])
    for kw in (dict(iou_threshold=0.3), dict(iou_threshold=0.5, score_threshold=float(np.median(res["scores"])))):
        a, e = regression.detect_and_refine(image, M, reg, **kw), wb.non_max_suppression(refined, kw["iou_threshold"], kw.get("score_threshold"))
        assert 0 < len(a) < len(plain)
        assert np.array_equal(bits(a.get()), bits(e.get())) and np.array_equal(bits(a.get_field("scores")), bits(e.get_field("scores")))
    path = str(tmp_path / "reg.npz")
    reg.save(path)
    back = regression.BoxRegressor.load(path)
    assert np.array_equal(bits(regression.detect_and_refine(image, M, back).get()), bits(want))
    _, crops = windows_of(M, image)
    assert np.array_equal(bits(back.predict(crops)), bits(rr.predict(rr.features(crops), reg.W, reg.b)))
    assert np.array_equal(bits(back.predict_device(torch.from_numpy(crops).cuda()).cpu().numpy()), bits(reg.predict(crops)))
    tiny = regression.detect_and_refine(np.zeros((8, 8), np.uint8), M, reg)
    assert len(tiny) == 0 and tiny.has_field("scores")


def test_errors():
    M, acc, reg = fitted("fpga")
    image = _training_images()[0]["image"]
    with pytest.raises(ValueError):
        regression.detect_and_refine(image, empty_model("float"), reg)                            # channel dtypes differ
    with pytest.raises(ValueError):
        regression.detect_and_refine(image, wb.load(os.path.join(GOLDEN, "grad_hist_4_u1_d2_T24.pb")), reg)     # window shapes differ
    with pytest.raises(ValueError):
        regression.detect_and_refine(image, M, reg, score_threshold=0.0)                          # a score threshold without NMS
    with pytest.raises(ValueError):
        regression.fit(M, [dict(image=image, groundtruth_boxes=None)])                            # no positives at all
    with pytest.raises(ValueError):
        regression.fit(empty_model("float"), _training_images(), accumulator=acc)                # the accumulator is uint8's
    a = regression.Accumulator(SHAPE, np.uint8)
    X, T = torch.zeros((3, 8, 8, 4), dtype=torch.uint8, device="cuda"), torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    for badX, badT in ((X.float(), T), (X[:, :7], T), (X, T.float()), (X, T[:2])):
        with pytest.raises(ValueError):
            a.add(badX, badT)
    with pytest.raises(TypeError):
        a.add(X.cpu().numpy(), T)
    a.add(X[:0], T[:0])
    assert a.n == 0
    with pytest.raises(ValueError):
        a.solve()                                                                                 # N < 2
    a.add(X, T)
    with pytest.raises(ValueError):
        a.solve()                                                                                 # the features do not vary


def test_mixed_image_shapes_and_accumulator_reuse():
    """fit over images of two shapes (batches are cut at a shape change) equals the same mine_batch / add_mined sequence by
    hand, bit for bit; a second l2 is solved from the same accumulator without another pass."""
    M = empty_model("fpga")
    items = _training_images()[:3]
    small = _training_images((80, 160))[:2]
    mixed = items[:2] + small + items[2:]
    acc = regression.Accumulator(SHAPE, np.uint8)
    reg = regression.fit(M, mixed, max_candidates=4, batch=2, seed=5, accumulator=acc)
    by_hand = regression.Accumulator(SHAPE, np.uint8)
    serial = 0
    for group in (mixed[:2], mixed[2:4], mixed[4:]):
        images = np.stack([it["image"] for it in group])
        gts = [it["groundtruth_boxes"] for it in group]
        mined = mine_batch(M, images, gts, tp=True, fp=False, min_tp_iou=0.5, max_tp_candidates=4, seed=5, serial0=serial)
        serial += len(group)
        assert len(mined) > 0
        by_hand.add_mined(mined, gts, M.detect_raw(group[0]["image"])["scales"])
    S = acc.state()
    assert acc.n == by_hand.n == int(S[-5, -5]) and np.array_equal(bits(S), bits(by_hand.state()))
    assert 0 < acc.n < 1313
    other = acc.solve(1e-1)
    W, b, rss, tss = rr.solve(S, 1e-1)
    assert other.l2 == 1e-1 and np.array_equal(bits(other.W), bits(W)) and np.array_equal(bits(other.b), bits(b))
    assert not np.array_equal(other.W, reg.W)
    assert np.array_equal(bits(regression.BoxRegressor.from_state(SHAPE, S, 1e-2).W), bits(reg.W))
