"""The designs of match_designs.py, proved on the host (no GPU): for every detection the planted owner is the first candidate
of largest IoU and the expected best is that IoU, with every IoU either proved 0 from the coordinates (the boxes share no
interior) or computed in exact rational arithmetic, one rounding per operation; the sizes and boundaries are the ones the
kernel's two paths need; and each emulated wrong kernel differs from the proof on a design named here."""
import numpy as np
import pytest

import match_designs as md
from waldboost_amd.boxes import Boxes, iou

S = md.scene()
IMAGES = md.images()
BY = {g.name: (b, g) for b, g in enumerate(IMAGES)}


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("g", IMAGES, ids=lambda g: g.name)
def test_planted_owners_follow_from_exact_arithmetic(g):
    want = g.want_owner
    b = BY[g.name][0]
    first = int(np.searchsorted(S.dt_image, b))
    n_exact = 0
    for j in range(len(g.dt)):
        vals = []
        for k in range(len(g.gt)):
            if md.disjoint(g.dt[j], g.gt[k]):
                vals.append(0.0)
            else:
                vals.append(md.iou_exact(g.dt[j], g.gt[k]))
                n_exact += 1
        if not vals:
            assert want[j] == -1 and S.want_best[first + j] == 0.0
            continue
        top = max(vals)
        assert vals.index(top) == want[j], (g.name, j, vals.index(top), want[j])
        assert bits(top) == bits(S.want_best[first + j]), (g.name, j)
        if g.plant[j] == md.NONE:
            assert top == 0.0 and want[j] == 0
        else:
            assert top > 0.0
    if len(g.gt) and len(g.dt):
        table = iou(Boxes(g.dt), Boxes(g.gt))                  # the contract's own function agrees
        assert np.array_equal(table.argmax(1), want)
        assert np.array_equal(bits(table.max(1)), bits(S.want_best[first:first + len(g.dt)]))
        assert n_exact >= 1 or g.name == "no-ground-truth"


def test_the_scene_holds_the_sizes_and_boundaries_asked_for():
    C, W = md.CHUNK, md.WG
    assert S.n_images <= 40 and S.n_dt <= 2048 and S.n_gt <= 300 and S.n_dt % W != 0
    starts = [int(np.searchsorted(S.dt_image, b)) for b in range(S.n_images)]
    assert starts[1] == 64 and starts[2] == 256                # image boundaries at detections 63 | 64 and 255 | 256
    uniform = [len(set(S.dt_image[w:w + W].tolist())) == 1 for w in range(0, S.n_dt, W)]
    assert uniform == [False, True, True, True, True, False, False, True]
    lds_counts = {len(IMAGES[S.dt_image[w]].gt) for w, u in zip(range(0, S.n_dt, W), uniform) if u}
    assert {1, C, C + 1, 2 * C + 1} <= lds_counts
    inside = [s for s in starts[6:] if s % W]                  # boundaries inside a workgroup
    assert len(inside) >= 3
    assert len(BY["no-ground-truth"][1].gt) == 0 and len(BY["no-ground-truth"][1].dt) > 0
    assert len(BY["no-detections"][1].dt) == 0 and len(BY["no-detections"][1].gt) > 0
    assert (S.want_owner[S.dt_image == BY["no-ground-truth"][0]] == -1).all()
    # winners at candidate 0 and at the last candidate, on both paths; ties that go to the lower index
    for name in ("two-chunks-plus-1", "chunk-plus-1", "three-candidates-twin-192-dets", "tail-109-dets"):
        b, g = BY[name]
        own = g.want_owner[g.plant != md.NONE]
        assert own.min() <= 1 and own.max() >= len(g.gt) - 2, name
    b, g = BY["two-chunks-plus-1"]
    assert (g.want_owner == 2 * C).any() and (g.want_owner == C - 1).any() and np.array_equal(g.gt[C - 1], g.gt[C])
    b, g = BY["chunk-plus-1"]
    assert (g.want_owner == 0).any() and np.array_equal(g.gt[0], g.gt[C - 1]) and not (g.want_owner == C - 1).any() and (g.want_owner == C).any()
    # none-detections: owner 0, best 0
    none = np.concatenate([g.plant == md.NONE for g in IMAGES])
    assert none.sum() > 50 and (S.want_best[none] == 0).all() and set(S.want_owner[none].tolist()) == {0, -1}
    # degenerate boxes: a union of exactly 0
    b, g = BY["degenerate"]
    assert ((g.gt[:, 2] - g.gt[:, 0]) * (g.gt[:, 3] - g.gt[:, 1]) == 0).sum() == 2 and (g.dt[0] == g.gt[0]).all()
    # coordinates that are no float32 values
    for name in ("fractions-not-float32", "general-float64"):
        g = BY[name][1]
        assert (g.gt.astype(np.float32).astype(np.float64) != g.gt).any(1).all(), name


def test_the_emulated_kernel_gives_the_expected_answers():
    best, owner = md.emulate(S)
    assert np.array_equal(owner, S.want_owner) and np.array_equal(bits(best), bits(S.want_best)), md.describe_mismatch(S, best, owner)


# fault -> an image on which the emulated wrong kernel must differ from the proof
EXPOSED_ON = {"last_max": "chunk-plus-1", "ge": "three-candidates-twin-192-dets", "f32": "fractions-not-float32", "fused": "general-float64",
              "shift_image": "one-candidate-64-dets", "stale_chunk": "two-chunks-plus-1", "owner_global": "one-chunk"}


@pytest.mark.parametrize("fault", md.FAULTS)
def test_each_emulated_wrong_kernel_differs_on_a_named_design(fault):
    best, owner = md.emulate(S, (fault,))
    b = BY[EXPOSED_ON[fault]][0]
    at = S.dt_image == b
    wrong = (owner != S.want_owner) | (bits(best) != bits(S.want_best))
    assert wrong[at].any(), fault
    print(md.describe_mismatch(S, best, owner))
    if fault in ("f32", "fused"):                              # the owner is right: only the value's bits tell
        assert np.array_equal(owner[at], S.want_owner[at])
    if fault == "fused":                                       # the exact-arithmetic fused form says the same
        i = int(np.flatnonzero(wrong & at)[0])
        g = IMAGES[b]
        j = i - int(np.searchsorted(S.dt_image, b))
        assert md.iou_exact(g.dt[j], g.gt[g.want_owner[j]], fused=True) == best[i] != S.want_best[i]
    if fault == "stale_chunk":                                 # only whole workgroups of an image with more than one chunk notice
        names = {IMAGES[k].name for k in set(S.dt_image[wrong].tolist())}
        assert names == {"two-chunks-plus-1", "chunk-plus-1"}
    if fault in ("last_max", "ge"):                            # twins and detections that overlap nothing
        b2, g = BY["chunk-plus-1"]
        w = wrong[S.dt_image == b2]
        assert w[(g.plant == 0) | (g.plant == md.NONE)].all() and not w[(g.plant != 0) & (g.plant != md.NONE)].any()


def test_mismatch_message_names_the_detection():
    best, owner = S.want_best.copy(), S.want_owner.copy()
    owner[300] += 1
    msg = md.describe_mismatch(S, best, owner)
    assert "1 detections differ" in msg and "workgroup 1, thread 44" in msg and "two-chunks-plus-1" in msg
