"""Host proofs for the end-to-end scene of tests/test_gpu_mip.py (tests/mip_cases.py; CPU): from the plan alone it has at
least 4 bags and between 20 and 5000 acceptable windows, and for the statement alone (the oracle's pyramid and trees) some
theta lies strictly above backward pruning's -- so the comparisons of the GPU test can fail."""
import numpy as np
import pytest

import mip_cases as mc
import mip_reference as ref
import waldboost_amd as wb


@pytest.mark.parametrize("tag", list(mc.CASES))
def test_the_scene_is_not_empty_by_the_plan_alone(tag):
    s = mc.scene(tag)
    m, n = s["shape"]
    win = ref.windows(s["levels"], s["inv_scale"], m, n, s["gts"], s["ignores"], mc.MIN_IOU)
    rows = win["rows"]
    assert len(win["reachable"]) >= 4 and 20 <= rows.size <= 5000
    # every planted window is a row with IoU 1, owned by its own box (unless a box in front of it is its twin); the ignored
    # box and the oversized one own no row; the oversized one is unreachable
    index = {(int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])): w for w in rows}
    for b, ws in enumerate(s["planted"]):
        for k, (l, r, c) in enumerate(ws):
            if s["ignores"][b][k]:
                assert (b, l, r, c) not in index
            else:
                assert index[(b, l, r, c)]["best"] == 1.0 and index[(b, l, r, c)]["owner"] == k
    assert [tuple(x) for x in win["unreachable"]] == [(1, 3)]
    assert {tuple(x) for x in win["reachable"]} == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)}
    assert len(set(rows["image"])) == 2 and len(set(rows["level"])) >= 4


@pytest.mark.parametrize("tag", list(mc.CASES))
def test_the_statement_prunes_above_backward_pruning(tag):
    st = mc.statement(tag)
    tr = st["trace"]
    assert np.isfinite(tr).all() and tr.shape == (st["rows"].size, 24)
    for recall in (1.0, 0.5):
        p = mc.pruned(tag, recall)
        back = ref.backward(tr, p["initial"])
        assert (p["theta"] >= back).all(), (tag, recall)
        if recall == 1.0:                                                        # the operating point the GPU test compares at
            assert (p["theta"] > back).any(), tag
        assert p["retained_bags"] >= p["keep"] and p["surviving"] >= p["retained_bags"]
        alive = p["removed_at"] == tr.shape[1]
        assert set(st["bag"][alive]) == set(st["bag"][p["initial"]]) and (tr[alive, -1] >= p["floor"]).all()
    assert mc.pruned(tag, 0.5)["keep"] == 3 and mc.pruned(tag, 1.0)["retained_bags"] == 5


def test_bad_arguments_are_refused_before_any_image_is_looked_at():
    M = mc.open_model("u8")

    def images():
        raise AssertionError("the images were looked at")
        yield

    for bad, word in ((dict(recall=0.0), "recall"), (dict(recall=1.0000001), "recall"), (dict(recall=float("nan")), "recall"),
                      (dict(margin=-1e-9), "margin"), (dict(margin=float("inf")), "margin"), (dict(min_iou=1.0), "min_iou"),
                      (dict(min_iou=-0.1), "min_iou"), (dict(min_iou=float("nan")), "min_iou")):
        with pytest.raises(ValueError, match=word):
            wb.prune_instances(M, images(), **bad)
    with pytest.raises(ValueError, match="at least one stage"):
        wb.prune_instances(wb.Model(M.shape, dict(M.channel_opts)), images())
    M.classifier[2].prediction[np.flatnonzero(np.asarray(M.classifier[2].left) < 0)[0]] = float("nan")
    with pytest.raises(ValueError, match="stage 2 has a non-finite prediction"):
        wb.prune_instances(M, images())
    assert "prune_instances" in wb.__all__ and wb.prune_instances is wb.calibration.prune_instances
