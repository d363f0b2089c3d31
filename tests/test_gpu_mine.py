"""Mining on the device through the engine (samples.mine_batch, DeviceSamplePool) with the golden models on small images:
against the statement of tests/mine_reference.py applied to the scan's own records and the pyramid's own levels, against
today's get_samples_from_image / SamplePool where no choice happens (caps of 10**9), and through train / fpga.train."""
import functools
import os

import numpy as np
import pytest

import mine_reference as ref
import waldboost_amd as wb
from waldboost_amd import engine as _engine
from waldboost_amd import channels as _channels
from waldboost_amd import fpga, samples
from waldboost_amd.samples import DeviceSamplePool, SampleLabel, SamplePool, get_samples_from_image, mine_batch
from waldboost_amd.synth import synth_batch, synth_image
from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = {"f32": "mixed_d2_T24.pb", "u8": "grad_hist_4_u1_d2_T24.pb"}
HUGE = 10 ** 9
FIELDS = ("scores", "row", "col", "instance_id", "tp_label", "samples")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def setup(tag):
    """(model, images [3, 200, 264], ground truth per image): the ground truth is planted on boxes a first detect found --
    the first and the middle one as they are (their windows are true positives), the last one flagged 'ignore' -- and image 2
    has none."""
    M = wb.load(os.path.join(GOLDEN, CASES[tag]))
    images = synth_batch(3, 200, 264, seed0=40)
    gts = []
    for b in range(2):
        found = M.detect(images[b]).get()
        assert len(found) >= 3
        gt = wb.Boxes(found[[0, len(found) // 2, len(found) - 1]].astype(np.float32))
        gt.set_field("ignore", np.array([0, 0, 1]))
        gts.append(gt)
    gts.append(None)
    return M, images, gts


def truncated(M, T):
    K = wb.Model(M.shape, M.channel_opts)
    for weak, theta in list(M)[:T]:
        K.append(weak, theta)
    return K


def engine_of(M, images):
    shrink, n_per_oct, smooth, spec = _channels.read_opts(M.channel_opts)
    B, H, W = images.shape
    return _engine.get_engine(H, W, images.dtype, shrink, n_per_oct, smooth, B, channels=spec)


def statement(M, images, gts, serial0=0, **params):
    """(rows, crops) the statement gives for the scan's records (detect_batch_raw) and the pyramid's levels (eng.read_level,
    after a mine_batch of the same images left the pyramid resident)."""
    res = M.detect_batch_raw(images)
    det = np.zeros(res["image"].size, ref.DET)
    det["image"], det["level"], det["r"], det["c"], det["score"] = res["image"], res["level"], res["r"], res["c"], res["scores"]
    inv_scale = np.array([np.float32(1.0 / s) for s in res["scales"]], np.float32)
    m, n, C = M.shape
    g = [np.asarray(b.get(), np.float64) if b is not None else None for b in gts]
    ign = [np.asarray(b.get_field("ignore")) if b is not None and b.has_field("ignore") else np.zeros(0 if b is None else len(b)) for b in gts]
    serial = (serial0 + np.arange(len(gts))).astype(np.uint32)
    rows = ref.mine(det[np.random.default_rng(1).permutation(det.size)], inv_scale, m, n, g, ign, serial, **params)["rows"]
    return rows, res


def crops_of(M, images, rows):
    eng = engine_of(M, images)
    m, n, C = M.shape
    levels = {}
    out = np.zeros((len(rows), m, n, C), np.dtype(str(eng.chn.dtype).replace("torch.", "")))
    for i, w in enumerate(rows):
        key = (int(w["image"]), int(w["level"]))
        if key not in levels:
            levels[key] = eng.read_level(*key)
        out[i] = levels[key][int(w["r"]):int(w["r"]) + m, int(w["c"]):int(w["c"]) + n]
    return out


def assert_rows(got, rows, crops=None):
    """A MinedSamples against ref.ROW records, bit for bit."""
    assert len(got) == len(rows)
    h = lambda k: getattr(got, k).cpu().numpy()
    for k, f in (("image", "image"), ("level", "level"), ("row", "r"), ("col", "c"), ("instance_id", "owner"), ("tp_label", "label")):
        assert np.array_equal(h(k), rows[f]), k
    assert np.array_equal(bits(h("scores")), bits(rows["score"]))
    assert np.array_equal(h("best").view(np.uint64), rows["best"].view(np.uint64))
    if crops is not None:
        assert h("samples").dtype == crops.dtype and np.array_equal(h("samples"), crops)


@pytest.mark.parametrize("tag", list(CASES))
def test_mine_batch_is_the_statement(tag):
    """(a) and (f): batch 3, 2 and 1 against the statement; the same seed twice gives the same bits, another seed another choice."""
    M, images, gts = setup(tag)
    params = dict(max_tp=3, max_fp=5, seed=9)
    kw = dict(max_tp_candidates=3, max_fp_candidates=5, seed=9)
    want, res = statement(M, images, gts, serial0=10, **params)
    got = mine_batch(M, images, gts, serial0=10, **kw)
    labels = set(want["label"].tolist())
    assert labels == {ref.TP, ref.FP} and len(want) < res["image"].size           # TP, FP and ignored windows all occur
    assert_rows(got, want, crops_of(M, images, want))
    boxes = ref.record_boxes(want["level"], want["r"], want["c"], [np.float32(1.0 / s) for s in res["scales"]], M.shape[0], M.shape[1])
    assert np.array_equal(got.boxes.cpu().numpy(), boxes)
    again = mine_batch(M, images, gts, serial0=10, **kw)
    assert_rows(again, want)
    assert np.array_equal(again.samples.cpu().numpy(), got.samples.cpu().numpy())
    other = mine_batch(M, images, gts, serial0=10, **{**kw, "seed": 10})
    assert len(other) == len(want) and not np.array_equal(other.row.cpu().numpy(), want["r"])
    # an image's part does not depend on the batch it sat in
    pair = mine_batch(M, images[1:], gts[1:], serial0=11, **kw)
    part = want[want["image"] >= 1].copy()
    part["image"] -= 1
    assert_rows(pair, part, crops_of(M, images[1:], part))
    for b in range(3):
        one = mine_batch(M, images[b], gts[b], serial0=10 + b, **kw)
        part = want[want["image"] == b].copy()
        part["image"] = 0
        assert_rows(one, part, crops_of(M, images[b:b + 1], part))


def test_scan_statistics_advance_as_in_a_scan():
    M, images, gts = setup("f32")
    M.reset()
    M.detect_batch_raw(images)
    want = (M.n_loc, M.n_weak)
    M.reset()
    mine_batch(M, images, gts)
    assert (M.n_loc, M.n_weak) == want and want[0] > 0


@pytest.mark.parametrize("tag", list(CASES))
def test_without_choice_it_is_get_samples_from_image(tag):
    """(b) caps of 10**9: to_boxes() of each image equals the concatenated yields of get_samples_from_image, field for field."""
    M, images, gts = setup(tag)
    kw = dict(max_tp_candidates=HUGE, max_fp_candidates=HUGE)
    got = mine_batch(M, images, gts, **kw).to_boxes()
    for b in range(3):
        want = wb.concatenate(list(get_samples_from_image(M, images[b], gts[b], **kw)))
        part = got[np.flatnonzero(got.get_field("image") == b)]
        assert len(part) == len(want) > 0
        assert np.array_equal(part.get(), want.get())
        for k in FIELDS:
            a, w = part.get_field(k), want.get_field(k)
            assert a.shape == w.shape and np.array_equal(a, w), (b, k)
        assert np.array_equal(bits(part.get_field("scores")), bits(want.get_field("scores")))
    for flags, lab in ((dict(tp=False), SampleLabel.FALSE_POSITIVE), (dict(fp=False), SampleLabel.TRUE_POSITIVE)):
        only = mine_batch(M, images, gts, **kw, **flags).to_boxes()
        assert len(only) > 0 and (only.get_field("tp_label") == lab).all()


def test_a_model_without_stages_returns_every_window_thinned_to_the_caps():
    """(c) length 0, batch 2, 40 x 56 images: every window is a detection; per (image, level) and class at most the cap."""
    M = truncated(setup("f32")[0], 0)
    images = synth_batch(2, 40, 56, seed0=3)
    gt = wb.Boxes(np.array([[8, 8, 32, 32]], "f"))
    M.reset()
    want, res = statement(M, images, [gt, None], max_tp=2, max_fp=6, min_tp_iou=0.5)
    assert res["image"].size == M.n_loc > 0                                       # every window of both pyramids
    got = mine_batch(M, images, [gt, None], max_tp_candidates=2, max_fp_candidates=6, min_tp_iou=0.5)
    assert_rows(got, want, crops_of(M, images, want))
    for l in np.unique(res["level"]):
        H = int(((res["image"] == 1) & (res["level"] == l)).sum())                 # image 1 has no ground truth: every window an FP hit
        assert int(((want["image"] == 1) & (want["level"] == l)).sum()) == min(6, H)
        at = (want["image"] == 0) & (want["level"] == l)
        assert (want["label"][at] == ref.TP).sum() <= 2 and (want["label"][at] == ref.FP).sum() <= 6
    assert (want["label"][want["image"] == 1] == ref.FP).all() and (want["label"] == ref.TP).any()
    # images too small for any level: an empty result
    none = mine_batch(M, synth_batch(2, 8, 8), [None, None])
    assert len(none) == 0 and tuple(none.samples.shape) == (0,) + tuple(M.shape)


def test_ground_truth_is_validated():
    M, images, gts = setup("f32")
    bad = wb.Boxes(np.array([[0, 0, np.nan, 5]], "f"))
    with pytest.raises(ValueError, match="finite"):
        mine_batch(M, images, [bad, None, None])
    flags = wb.Boxes(np.array([[0, 0, 5, 5]], "f"))
    flags.set_field("ignore", np.zeros((1, 1)))
    with pytest.raises(ValueError, match="single dimension"):
        mine_batch(M, images, [flags, None, None])
    with pytest.raises(ValueError):
        mine_batch(M, images, gts[:2])


def _items(tag):
    M, images, gts = setup(tag)
    extra = synth_batch(3, 200, 264, seed0=70)
    return [dict(image=im, groundtruth_boxes=g) for im, g in zip(list(images) + list(extra), gts + gts)]


def assert_same_pool(dev_pool, host_pool):
    a, b = dev_pool.to_host(), host_pool.samples
    assert (a is None) == (b is None)
    if a is None:
        return
    assert len(a) == len(b) and np.array_equal(a.get(), b.get())
    for k in FIELDS:
        assert np.array_equal(a.get_field(k), b.get_field(k)), k
    assert np.array_equal(bits(a.get_field("scores")), bits(b.get_field("scores")))
    assert dev_pool.pool_stats() == host_pool.pool_stats()


@pytest.mark.parametrize("tag", list(CASES))
def test_device_pool_is_the_host_pool_without_choice(tag):
    """(d) caps of 10**9, batch 1, three updates with a growing model: contents and order identical."""
    M = setup(tag)[0]
    items = _items(tag)
    kw = dict(max_tp_candidates=HUGE, max_fp_candidates=HUGE)
    dp, hp = DeviceSamplePool(batch=1, **kw), SamplePool(**kw)
    for T, min_tp, min_fp in ((6, 1, 50), (12, 3, 10 ** 6), (24, 4, 200)):
        dp.min_tp = hp.min_tp = min_tp
        dp.min_fp = hp.min_fp = min_fp
        K = truncated(M, T)
        dp.update(K, iter(items))
        hp.update(K, iter(items))
        assert_same_pool(dp, hp)
        for label in (SampleLabel.TRUE_POSITIVE, SampleLabel.FALSE_POSITIVE):
            (X, H), (Xh, Hh) = dp.get_samples(label), hp.get_samples(label)
            assert X.is_cuda and H.dtype == np.float32 and np.array_equal(X.cpu().numpy(), Xh) and np.array_equal(bits(H), bits(Hh))
    assert len(dp.samples) > 0


def test_quotas_and_batches():
    """(g) an update that needs only FP returns no TP; batches of equal shape, flushed on a shape change; the stop after the
    first batch that fills both quotas."""
    M = setup("f32")[0]
    items = _items("f32")
    pool = DeviceSamplePool(min_tp=0, min_fp=5, batch=2)
    pool.update(M, items)
    assert pool.pool_stats()["num_tp"] == 0 and pool.pool_stats()["num_fp"] >= 5
    assert pool.images_seen == 2                                              # one batch was enough
    small = dict(image=synth_image(120, 136, 5), groundtruth_boxes=None)
    pool = DeviceSamplePool(min_tp=0, min_fp=10 ** 6, batch=4)
    seen = []
    real = samples.mine_batch
    try:
        samples.mine_batch = lambda model, images, gt, **kw: seen.append((tuple(images.shape), kw["serial0"])) or real(model, images, gt, **kw)
        pool.update(M, items[:3] + [small, small] + items[3:])
    finally:
        samples.mine_batch = real
    assert seen == [((3, 200, 264), 0), ((2, 120, 136), 3), ((3, 200, 264), 5)] and pool.images_seen == 8
    assert (pool.samples.tp_label == SampleLabel.FALSE_POSITIVE).all()


def _training_images(size=(96, 128)):
    items = []
    for seed in range(6):
        img = synth_image(size[0], size[1], 100 + seed).astype(np.int32)
        rng = np.random.default_rng(seed)
        gt = []
        for side, x_lo in ((24, 4), (32, 60)):
            x, y = x_lo + int(rng.integers(0, 30)), 4 + int(rng.integers(0, size[0] - side - 8))
            img[y:y + side, x:x + side] += 90
            gt.append([x, y, x + side, y + side])
        items.append(dict(image=np.clip(img, 0, 255).astype(np.uint8), groundtruth_boxes=wb.Boxes(np.array(gt, "f"))))
    return items


@pytest.mark.parametrize("flavour", ["float", "fpga"])
def test_train_with_either_pool_gives_the_same_model(flavour, tmp_path):
    """(e) length 3, depth 2, caps of 10**9 and batch 1: byte-identical saved models; the device pool's samples stay on the GPU."""
    items = _training_images()
    kw = dict(min_tp=10, min_fp=100, min_tp_iou=0.5, max_fp_iou=0.3, max_tp_candidates=HUGE, max_fp_candidates=HUGE)
    saved = []
    for pool in (SamplePool(**kw), DeviceSamplePool(batch=1, **kw)):
        if flavour == "float":
            M = wb.Model((8, 8, 4), wb.default_channel_opts)
            L = wb.train(M, items, learner=wb.Learner(max_depth=2), pool=pool, length=3)
        else:
            M = wb.Model((8, 8, 4), dict(shrink=2, n_per_oct=8, smooth=1, channels=fpga.grad_hist_4_u1))
            L = fpga.train(M, items, pool=pool, length=3, max_depth=2)
        assert len(M) == 3 and len(L) == 3
        path = str(tmp_path / f"{type(pool).__name__}.pb")
        M.save(path)
        with open(path, "rb") as f:
            saved.append(f.read())
    assert pool.samples.samples.is_cuda and len(pool.samples) > 0
    assert saved[0] == saved[1]
