"""The matching kernel on the designed scene of tests/match_designs.py (proved on the host by test_match_designs_host.py): at the
C ABI (wb_match_launch) and through waldboost_amd.match_boxes; `best` is compared as bits, `owner` exactly, and every entry
of both outputs must have been written over its sentinel."""
import ctypes as C

import numpy as np
import pytest

import match_designs as md
import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.boxes import Boxes

pytestmark = pytest.mark.gpu

S = md.scene()
GUARD = 64
BEST_FILL, OWNER_FILL = -7.0, -7


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(4, a.dtype)).cuda()


def launch(dt, dt_image, gt, gt_off, n_images):
    """One wb_match_launch -> (best, owner) of outputs pre-filled with the sentinels, guard entries on both sides checked."""
    import torch
    lib, n = nat.load(), len(dt)
    d_dt, d_img, d_gt, d_off = dev(dt.reshape(-1)), dev(dt_image.astype(np.int32)), dev(gt.reshape(-1)), dev(gt_off.astype(np.int32))
    best = torch.full((GUARD + n + GUARD,), BEST_FILL, dtype=torch.float64, device="cuda")
    owner = torch.full((GUARD + n + GUARD,), OWNER_FILL, dtype=torch.int32, device="cuda")
    nat.check(lib.wb_match_launch(nat.stream_ptr(), nat.ptr(d_dt), nat.ptr(d_img), nat.ptr(d_gt), nat.ptr(d_off), n, len(gt), n_images,
                                  C.c_void_p(best.data_ptr() + 8 * GUARD), C.c_void_p(owner.data_ptr() + 4 * GUARD)), "wb_match_launch")
    hb, ho = best.cpu().numpy(), owner.cpu().numpy()
    for h, fill in ((hb, BEST_FILL), (ho, OWNER_FILL)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), "entries around the outputs were written"
    return hb[GUARD:GUARD + n], ho[GUARD:GUARD + n]


def check(best, owner):
    assert np.array_equal(owner, S.want_owner) and np.array_equal(bits(best), bits(S.want_best)), md.describe_mismatch(S, best, owner)


def test_the_designed_scene_at_the_c_abi():
    best, owner = launch(S.dt, S.dt_image, S.gt, S.gt_off, S.n_images)
    # every entry was written over its sentinel (no expected answer is a sentinel)
    assert not (S.want_best == BEST_FILL).any() and not (S.want_owner == OWNER_FILL).any()
    assert not (best == BEST_FILL).any() and not (owner == OWNER_FILL).any()
    check(best, owner)


def test_the_designed_scene_through_match_boxes():
    best, owner = wb.match_boxes(Boxes(S.dt), [Boxes(g.gt) for g in S.images], S.dt_image)
    assert best.dtype == np.float64 and owner.dtype == np.int32
    check(best, owner)


@pytest.mark.parametrize("g", [g for g in S.images if len(g.dt)], ids=lambda g: g.name)
def test_each_image_as_one_pair(g):
    """The one-pair form: every image alone (sizes 64 .. 256: both paths are the LDS path of one or one partial workgroup)."""
    best, owner = wb.match_boxes(Boxes(g.dt), Boxes(g.gt))
    at = S.dt_image == S.images.index(g)
    assert np.array_equal(owner, S.want_owner[at]) and np.array_equal(bits(best), bits(S.want_best[at])), g.name


def test_offsets_and_images_out_of_range_read_nothing_outside():
    """dt_image below 0 and beyond the last image are clamped, offsets beyond n_gt and negative ones as well, an end in front
    of its start is an empty range: the answers are those of the clamped call."""
    img = S.dt_image.copy()
    first, last = img == 0, img == S.n_images - 1
    img[first], img[last] = -5, S.n_images + 1000
    best, owner = launch(S.dt, img, S.gt, S.gt_off, S.n_images)
    check(best, owner)
    off = S.gt_off.copy()
    off[0], off[-1] = -3, S.n_gt + 100                         # clamped to 0 and n_gt: the same ranges
    best, owner = launch(S.dt, S.dt_image, S.gt, off, S.n_images)
    check(best, owner)
    off = S.gt_off.copy()
    off[3] = off[4] + 5                                        # image 3 ends in front of its start: no candidates
    best, owner = launch(S.dt, S.dt_image, S.gt, off, S.n_images)
    at = S.dt_image == 3
    assert (owner[at] == -1).all() and (best[at] == 0).all()
    keep = ~at & (S.dt_image != 2)                             # (image 2's range grew by that: its answers are another matter)
    assert np.array_equal(owner[keep], S.want_owner[keep]) and np.array_equal(bits(best[keep]), bits(S.want_best[keep]))


def test_no_detections_touch_nothing():
    best, owner = wb.match_boxes(Boxes(np.empty((0, 4))), Boxes(S.gt))
    assert best.shape == (0,) and owner.shape == (0,) and best.dtype == np.float64 and owner.dtype == np.int32
    assert nat.load().wb_match_launch(None, None, None, None, None, 0, 5, 1, None, None) == 0
