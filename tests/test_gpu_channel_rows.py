"""Step 2 of the detection-path channel kernel (uint8 images, shrink 2, smoothed, canonical grad_hist) hands a wave a run
of contiguous shrunk rows and carries half of every pixel's patch -- as column differences and horizontal [1,2,1] sums --
down the run.  These tests walk every split of a bottom tile's rows over the four waves (waves without a row included),
with one and with two tile columns, on noise and on content whose gradients sit at the ends of their range or vanish,
and compare the pyramid bit for bit with the oracle; the rank bytes written from the same tiles are covered by small
cascades through Model.detect_raw."""
import numpy as np
import pytest

import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd.synth import random_tree_arrays, synth_image
from util import oracle_detect

pytestmark = pytest.mark.gpu

# level 0 of an image of 2u rows holds u output rows: 16 in the top tile and u - 16 = 1 .. 16 in the bottom one, which
# then forms u - 14 = 3 .. 18 shrunk rows (the smooth's halo included)
HEIGHTS = [2 * u for u in range(17, 33)]
# 40 output columns: one tile column whose lanes 42.. lie past the level; 70: two tile columns, the first with the two
# columns beyond the 64th lane live
WIDTHS = [80, 140]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (((y + x) & 1) * 255).astype(np.uint8)                # gradients of +-1020 and 0


def flat_blocks(H, W, seed):
    """Large flat blocks that meet in steps one pixel wide, some of them one grey level high: pooled zeros beside a
    gradient (the exact redo of a block, the odd values the smooth is told about)."""
    rng = np.random.default_rng(seed)
    bh, bw = 11, 13                                              # edges on even and on odd rows / columns
    lv = rng.choice(np.array([0, 1, 2, 127, 128, 255], np.uint8), (-(-H // bh), -(-W // bw)))
    return np.ascontiguousarray(np.kron(lv, np.ones((bh, bw), np.uint8))[:H, :W])


def image(kind, H, W):
    if kind == "noise":
        return synth_image(H, W, H + W)
    if kind == "checkerboard":
        return checkerboard(H, W)
    return flat_blocks(H, W, H + W)


def check_pyramid(img):
    got = list(wb.channels.channel_pyramid(img, dict(wb.default_channel_opts)))
    ref = list(orc.channel_pyramid(img, dict(wb.default_channel_opts, channels=orc.grad_hist)))
    assert len(got) == len(ref)
    for (c, s), (rc, rs) in zip(got, ref):
        assert s == rs and c.shape == rc.shape
        assert np.array_equal(bits(c), bits(rc)), (img.shape, c.shape)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", HEIGHTS)
def test_every_split_of_the_bottom_tile_rows(H, W):
    check_pyramid(image("noise", H, W))


def check_cell_pyramid(img, shrink, smooth):
    opts = dict(shrink=shrink, n_per_oct=4, smooth=smooth)
    got = list(wb.channels.channel_pyramid(img, dict(opts, channels=wb.channels.grad_hist)))
    ref = list(orc.channel_pyramid(img, dict(opts, channels=orc.grad_hist)))
    assert len(got) == len(ref)
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.shape == rc.shape
        assert np.array_equal(bits(c), bits(rc)), (img.shape, shrink, smooth, l, c.shape)


@pytest.mark.parametrize("shrink,smooth", [(1, 0), (1, 1), (2, 0), (4, 0), (4, 1)])
def test_every_bottom_tile_height_in_the_other_grad_hist_cells(shrink, smooth):
    """channels_kernel is the only kernel that trims a bottom tile's rows to its level, so every grad_hist cell splits the
    rows of step 1 over its waves in its own way (its own tile height, halo and strip length).  The tests above walk the
    cell of the detection path; this one walks the other five: a full top tile and a bottom tile of 1 .. TU output rows --
    every u mod TU, with the tile shape the library reports -- at one narrow width and at one of two tile columns."""
    from waldboost_amd import _native as nat
    from waldboost_amd.plan import chan_tile
    tu, tv = chan_tile(nat.WB_CHN_GRAD_HIST, shrink)
    for u in range(tu + 1, 2 * tu + 1):
        for v in (tv // 2 + 8, tv + 6):
            H, W = shrink * u, shrink * v
            check_cell_pyramid(synth_image(H, W, H + W), shrink, smooth)


@pytest.mark.parametrize("kind", ["noise", "checkerboard", "flat_blocks"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", [36, 64])
def test_content_fed_from_carried_values(H, W, kind):
    check_pyramid(image(kind, H, W))


@pytest.mark.parametrize("H,W,kind", [(36, 80, "noise"), (64, 140, "flat_blocks"), (46, 140, "noise")])
def test_rank_path_records_and_alive(H, W, kind):
    img = image(kind, H, W)
    rng = np.random.default_rng(H * W)
    shape = (8, 8, 4)
    M = wb.Model(shape, dict(wb.default_channel_opts))
    for t in range(8):                                           # a small depth-2 cascade that rejects some windows at most stages
        f, th, l, r, p = random_tree_arrays(rng, shape, 2, 2.0, 60.0)
        M.append(wb.DTree(f, th, l, r, p), float("-inf") if t < 2 else float(np.float32(-0.1 * t)))
    ref = oracle_detect(M, img)
    res = M.detect_raw(img)
    assert np.array_equal(res["alive"], ref["alive"])
    assert np.array_equal(res["level"], ref["level"]) and np.array_equal(res["r"], ref["r"]) and np.array_equal(res["c"], ref["c"])
    assert np.array_equal(bits(res["scores"]), bits(ref["scores"]))
    assert np.array_equal(bits(res["boxes"]), bits(ref["boxes"]))
    assert 0 < ref["alive"][0][-1] < ref["alive"][0][0]          # (the cascade rejected some windows of level 0, not all)
