"""Multiple-instance pruning end to end on the committed models with their thetas set to -inf, on the scene of
tests/mip_cases.py (two 120 x 136 images; ground truth planted on windows of the open model's scan; an ignored and an
oversized box), against the statement (tests/mip_reference.py on the oracle's pyramid and trees): instance_windows field
for field, the thresholds, floor and counts of prune_instances, what the pruned model detects, the guarantees against
calibrate(recall=1.0), a .pb round trip and the refusals.  tests/test_mip_host.py proves on the host that the scene is not
empty and that its thresholds lie above backward pruning's."""
import numpy as np
import pytest

import mip_cases as mc
import mip_reference as ref
import waldboost_amd as wb
from waldboost_amd import calibration

pytestmark = pytest.mark.gpu

T = 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def items(tag):
    s = mc.scene(tag)
    return [dict(image=s["images"][b], groundtruth_boxes=s["boxes"][b]) for b in range(2)]


def keys_of(res):
    return set(zip(res["level"].astype(int).tolist(), res["r"].astype(int).tolist(), res["c"].astype(int).tolist()))


def assert_rows(got, rows, crops):
    h = lambda k: getattr(got, k).cpu().numpy()
    assert len(got) == len(rows)
    for k, f in (("image", "image"), ("level", "level"), ("row", "r"), ("col", "c"), ("instance_id", "owner"), ("tp_label", "label")):
        assert np.array_equal(h(k), rows[f]), k
    assert np.array_equal(h("best").view(np.uint64), rows["best"].view(np.uint64)) and (h("scores") == 0).all()
    assert h("samples").dtype == crops.dtype and np.array_equal(h("samples"), crops)


@pytest.mark.parametrize("tag", list(mc.CASES))
def test_instance_windows_is_the_statement(tag):
    s, st = mc.scene(tag), mc.statement(tag)
    M = mc.open_model(tag)
    m, n = s["shape"]
    # the planted boxes are windows of the open model's own scan
    for b in range(2):
        assert set(s["planted"][b]) <= keys_of(M.detect_raw(s["images"][b]))
    got, bag, reach, unreach = calibration.instance_windows(M, s["images"], s["boxes"], min_iou=mc.MIN_IOU)
    assert_rows(got, st["rows"], st["crops"])
    assert np.array_equal(bag.cpu().numpy(), st["bag"]) and bag.dtype == __import__("torch").int32
    assert np.array_equal(reach, st["reachable"]) and np.array_equal(unreach, st["unreachable"])
    boxes = ref.mref.record_boxes(st["rows"]["level"], st["rows"]["r"], st["rows"]["c"], s["inv_scale"], m, n)
    assert np.array_equal(bits(got.boxes.cpu().numpy()), bits(boxes))
    # an image's part does not depend on the batch it sat in; one image may come as [H, W] with its Boxes
    for b in range(2):
        one, bag1, reach1, unreach1 = calibration.instance_windows(M, s["images"][b], s["boxes"][b], min_iou=mc.MIN_IOU)
        at = st["rows"]["image"] == b
        part = st["rows"][at].copy()
        part["image"] = 0
        assert_rows(one, part, st["crops"][at])
        assert np.array_equal(bag1.cpu().numpy(), st["bag"][at] - st["bag"][at].min())
        assert np.array_equal(reach1[:, 1], st["reachable"][st["reachable"][:, 0] == b][:, 1]) and (reach1[:, 0] == 0).all()
        assert np.array_equal(unreach1[:, 1], st["unreachable"][st["unreachable"][:, 0] == b][:, 1])
    # no ground truth at all: nothing is acceptable, nothing is unreachable
    none, bag0, reach0, unreach0 = calibration.instance_windows(M, s["images"], [None, None])
    assert len(none) == 0 and bag0.numel() == 0 and reach0.shape == (0, 2) and unreach0.shape == (0, 2)


@pytest.mark.parametrize("recall", [1.0, 0.5])
@pytest.mark.parametrize("tag", list(mc.CASES))
def test_prune_instances_is_the_statement_and_keeps_its_promises(tag, recall, tmp_path):
    s, st = mc.scene(tag), mc.statement(tag)
    p = mc.pruned(tag, recall)
    M = mc.open_model(tag)
    res = wb.prune_instances(M, items(tag), recall=recall, min_iou=mc.MIN_IOU)
    print(f"{tag} recall {recall}: {res}")
    assert res.theta.dtype == np.float32 and np.array_equal(bits(res.theta), bits(p["theta"]))
    assert bits([res.floor])[0] == bits([p["floor"]])[0]
    assert (res.n_bags, res.retained, res.n_windows, res.surviving) == (p["n_bags"], p["retained_bags"], len(st["rows"]), p["surviving"])
    assert res.recall == res.retained / res.n_bags and res.retained >= p["keep"] == calibration.keep_count(recall, res.n_bags)
    assert np.array_equal(res.unreachable, st["unreachable"]) and res.old_theta == [float("-inf")] * T
    assert all(type(t) is float for t in M.theta) and np.array_equal(np.array(M.theta, np.float64), p["theta"].astype(np.float64))
    # batches of one image give the same bits; inplace=False leaves the model alone; a margin lowers every theta
    K = mc.open_model(tag)
    res1 = wb.prune_instances(K, items(tag), recall=recall, min_iou=mc.MIN_IOU, batch=1, margin=0.375, inplace=False)
    assert np.array_equal(bits(res1.theta), bits(p["theta"] - np.float32(0.375))) and K.theta == [float("-inf")] * T
    assert (res1.floor, res1.retained, res1.surviving) == (res.floor, res.retained, res.surviving)
    assert np.array_equal(res1.unreachable, st["unreachable"])
    # what the pruned model detects: of the acceptable windows exactly the statement's survivors, image by image
    rows = st["rows"]
    alive = p["removed_at"] == T
    for b in range(2):
        found = keys_of(M.detect_raw(s["images"][b]))
        at = rows["image"] == b
        acceptable = list(zip(rows["level"][at].tolist(), rows["r"][at].tolist(), rows["c"][at].tolist()))
        survivors = {k for k, a in zip(acceptable, alive[at]) if a}
        assert found & set(acceptable) == survivors, (tag, recall, b)
    # every retained box has a detection that it owns with an IoU above min_iou
    for k in np.unique(st["bag"][p["initial"]]):
        mine = alive & (st["bag"] == k)
        assert mine.any() and (rows["best"][mine] > mc.MIN_IOU).all()
        b, owner = st["reachable"][k]
        assert (rows["image"][mine] == b).all() and (rows["owner"][mine] == owner).all()
    # never below backward pruning on the windows retained at the start, and no dearer on any sample set
    crops = st["crops"][p["initial"]]
    B = mc.open_model(tag)
    back = wb.calibrate(B, crops, recall=1.0)
    assert np.array_equal(bits(back.theta), bits(ref.backward(st["trace"], p["initial"])))
    assert (res.theta >= back.theta).all()
    if recall == 1.0:
        assert (res.theta > back.theta).any()                                  # (shown possible on the host: test_mip_host.py)
    rng = np.random.default_rng(5)
    level0 = mc.level0(tag)
    m, n = s["shape"]
    rs, cs = rng.integers(0, level0.shape[0] - m, 300), rng.integers(0, level0.shape[1] - n, 300)
    random_crops = np.stack([level0[r:r + m, c:c + n] for r, c in zip(rs, cs)])
    cost, cost_back = calibration.expected_cost(M, random_crops), calibration.expected_cost(B, random_crops)
    print(f"{tag} recall {recall}: expected cost {cost} under multiple-instance pruning, {cost_back} under backward pruning")
    assert cost <= cost_back
    # a .pb round trip keeps the thresholds
    path = str(tmp_path / "pruned.pb")
    M.save(path)
    assert np.array_equal(np.array(wb.load(path).theta, np.float64), res.theta.astype(np.float64))


def test_refusals():
    tag = "u8"
    M = mc.open_model(tag)
    it = items(tag)
    for bad in (dict(recall=0.0), dict(recall=1.5), dict(recall=float("nan")), dict(margin=-1.0), dict(margin=float("nan")),
                dict(min_iou=1.0), dict(min_iou=-0.1)):
        with pytest.raises(ValueError):
            wb.prune_instances(M, it, **bad)
    with pytest.raises(ValueError, match="at least one stage"):
        wb.prune_instances(wb.Model(M.shape, dict(M.channel_opts)), it)
    K = mc.open_model(tag)
    K.classifier[2].prediction[np.flatnonzero(np.asarray(K.classifier[2].left) < 0)[0]] = float("inf")
    with pytest.raises(ValueError, match="stage 2 has a non-finite prediction"):
        wb.prune_instances(K, it)
    # no reachable ground truth: none at all, only an ignored box, only a box no window reaches
    s = mc.scene(tag)
    huge = wb.Boxes(np.array([[-2 * mc.W, -2 * mc.H, 3 * mc.W, 3 * mc.H]], np.float32))
    ignored = wb.Boxes(s["boxes"][0].get()[:1])
    ignored.set_field("ignore", np.array([1]))
    for gt in (None, ignored, huge):
        with pytest.raises(ValueError, match="reachable"):
            wb.prune_instances(M, [dict(image=s["images"][0], groundtruth_boxes=gt)])
    with pytest.raises(ValueError, match="min_iou"):
        calibration.instance_windows(M, s["images"], s["boxes"], min_iou=1.0)
    with pytest.raises(ValueError):
        calibration.instance_windows(M, s["images"], s["boxes"][:1])
    assert M.theta == [float("-inf")] * T                                      # a refused call leaves the model alone
