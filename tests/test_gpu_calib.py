"""Threshold calibration end to end on the committed models with their thetas set to -inf: positives mined from a small
image against planted boxes (samples.mine_batch) and a few hundred random crops of a pyramid level, against the statement
(tests/calib_reference.py on the oracle's trees); the guarantees of calibration.calibrate, Model.stage_scores against
Model.predict, stage_survival / expected_cost, a .pb round trip and what a calibrated model detects."""
import functools
import os

import numpy as np
import pytest

import calib_reference as ref
import waldboost_amd as wb
from waldboost_amd import calibration
from waldboost_amd.samples import gather_samples, mine_batch
from waldboost_amd.synth import synth_image
from util import GOLDEN, oracle_model

pytestmark = pytest.mark.gpu

CASES = {"f32": "mixed_d2_T24.pb", "u8": "grad_hist_4_u1_d2_T24.pb"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_model(tag):
    """The committed model with every theta at -inf."""
    M = wb.load(os.path.join(GOLDEN, CASES[tag]))
    M.theta = [float("-inf")] * len(M)
    return M


@functools.lru_cache(None)
def setup(tag):
    """(mined positives: device tensor, random crops: ndarray, {set: unrejected statement trace}): the positives are the
    true-positive windows mine_batch finds on a 120 x 136 image for three boxes planted on windows of the open model's own
    scan; the crops are 300 random windows of the image's first pyramid level."""
    M = open_model(tag)
    img = synth_image(120, 136, 11)
    found = M.detect(img).get()
    gt = wb.Boxes(found[[len(found) // 5, len(found) // 2, len(found) - 7]].astype(np.float32))
    mined = mine_batch(M, img, gt, fp=False, min_tp_iou=0.5, max_tp_candidates=60)
    assert 20 <= len(mined) <= 1000
    chns, _ = next(iter(M.channels(img)))
    rng = np.random.default_rng(5)
    m, n, _ = M.shape
    rs, cs = rng.integers(0, chns.shape[0] - m, 300), rng.integers(0, chns.shape[1] - n, 300)
    crops = gather_samples(chns, rs, cs, M.shape)
    trees = oracle_model(M)[2]
    return mined.samples, crops, {"mined": ref.trace(trees, mined.samples.cpu().numpy()), "crops": ref.trace(trees, crops)}


def samples_of(tag, which):
    mined, crops, traces = setup(tag)
    return (mined if which == "mined" else crops), traces[which]


@pytest.mark.parametrize("which", ["mined", "crops"])
@pytest.mark.parametrize("tag", list(CASES))
def test_calibrate_keeps_exactly_the_retained_with_their_scores_and_is_tight(tag, which):
    X, tr = samples_of(tag, which)
    for recall in (0.9, 1.0, 0.5):
        M = open_model(tag)
        p = ref.prune(tr, recall)
        res = wb.calibrate(M, X, recall=recall)
        assert np.all(res.theta == p["theta"]) and res.retained == p["retained"].sum() and res.floor == float(p["floor"])
        assert res.retained >= p["keep"] and res.recall == res.retained / len(tr)
        assert all(type(t) is float for t in M.theta) and np.all(np.array(M.theta) == p["theta"].astype(np.float64))
        H, mask = M.predict(X)
        assert np.array_equal(mask, p["retained"])                                     # True exactly on the retained
        assert np.array_equal(bits(H[mask]), bits(tr[mask, -1]))                       # with their unrejected scores
        assert (tr[p["retained"]] == p["theta"][None, :]).any(axis=0).all()            # every threshold is met: tight


@pytest.mark.parametrize("tag", list(CASES))
def test_stage_scores_survival_and_cost_follow_the_statement(tag):
    X, tr = samples_of(tag, "crops")
    M = open_model(tag)
    assert np.array_equal(bits(M.stage_scores(X)), bits(tr))
    wb.calibrate(M, samples_of(tag, "mined")[0], recall=0.9)
    trees, thetas = oracle_model(M)[2:]
    rt, alive = ref.trace_rejecting(trees, thetas, X)
    got = M.stage_scores(X, reject=True)
    assert np.array_equal(bits(got), bits(rt))
    H, mask = M.predict(X)
    assert np.array_equal(bits(got[:, -1]), bits(H))
    surv = calibration.stage_survival(M, X)
    T = len(M)
    entering = np.concatenate([np.ones((len(X), 1), bool), ~np.isneginf(rt[:, :-1])], axis=1)      # sample i enters stage t
    assert np.array_equal(surv, alive) and surv[:T].sum() == entering.sum() and surv[T] == mask.sum()
    assert calibration.expected_cost(M, X) == entering.sum() / len(X)
    assert 1 <= calibration.expected_cost(M, X) <= T                                   # everybody enters stage 0, nobody more than T


@pytest.mark.parametrize("tag", list(CASES))
def test_a_calibrated_model_survives_a_pb_round_trip(tag, tmp_path):
    X, _ = samples_of(tag, "mined")
    M = open_model(tag)
    res = wb.calibrate(M, X, recall=0.95)
    path = str(tmp_path / "calibrated.pb")
    M.save(path)
    L = wb.load(path)
    assert np.array_equal(np.array(L.theta, np.float64), res.theta.astype(np.float64))
    crops, _ = samples_of(tag, "crops")
    a, b = M.predict(crops), L.predict(crops)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("tag", list(CASES))
def test_a_calibrated_model_detects_a_subset_with_the_same_scores_and_no_more_work(tag):
    X, _ = samples_of(tag, "mined")
    M = open_model(tag)
    img = synth_image(240, 320, 3)
    before = M.detect_raw(img)
    weak_before, M.n_weak = M.n_weak, 0
    wb.calibrate(M, X, recall=0.9)
    after = M.detect_raw(img)
    key = lambda r: (r["level"].astype(np.int64) << 40) | (r["r"].astype(np.int64) << 20) | r["c"].astype(np.int64)
    kb, ka = key(before), key(after)
    print(f"{tag}: {kb.size} detections before, {ka.size} after; n_weak {weak_before} -> {M.n_weak}")
    assert ka.size <= kb.size and np.isin(ka, kb).all()
    at = np.searchsorted(kb, ka)                                                        # (keys ascend: level, row, col order)
    assert np.array_equal(kb[at], ka) and np.array_equal(bits(before["scores"][at]), bits(after["scores"]))
    assert M.n_weak <= weak_before


@pytest.mark.parametrize("tag", list(CASES))
def test_a_device_pool_hands_in_its_true_positives_where_they_lie(tag):
    from waldboost_amd.samples import DeviceSamplePool, SampleLabel
    import torch
    M = open_model(tag)
    img = synth_image(120, 136, 11)
    found = M.detect(img).get()
    gt = wb.Boxes(found[[len(found) // 5, len(found) // 2, len(found) - 7]].astype(np.float32))
    both = mine_batch(M, img, gt, min_tp_iou=0.5, max_tp_candidates=60, max_fp_candidates=5)
    pool = DeviceSamplePool()
    pool.samples = both
    X = pool.get_true_positives()[0]
    assert isinstance(X, torch.Tensor) and X.is_cuda and 0 < len(X) < len(both)
    assert len(X) == int((both.tp_label == SampleLabel.TRUE_POSITIVE).sum())
    want = wb.calibrate(open_model(tag), X, recall=0.9)
    got = wb.calibrate(M, pool, recall=0.9)
    assert (got.n, got.retained, got.floor) == (want.n, want.retained, want.floor) and np.array_equal(bits(got.theta), bits(want.theta))
    assert np.array_equal(M.predict(X)[1].sum(), got.retained)
