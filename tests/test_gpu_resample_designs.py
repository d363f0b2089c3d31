"""Step 1 of the channel tile kernels (resample_tile, csrc/wb_chan_tile.h) on designed levels: images on which thousands
of resized pixels are decided by the order of the fp64 operations or by the clip to the octave's (min, max) -- counted, and
shown to reach the channels, by test_resample_designs_host.py -- through every cell of the kernels' dispatch table
(function x image dtype x shrink x smooth), through a batch of two images with different minima, and through the route
without the host's patch table.  Every comparison is bit for bit with the oracle's pyramid: bytes, shapes and scales.

uint8 images take the staged / fast-path / exact-redo code the designs aim at.  float32 and int16 images take the kernel's
direct path and ride along on the same pixels: for float32 nothing is designed (no truncation), for int16 the truncation
toward zero on both sides of zero (ratio_levels: the image minus 160) and the clip to the MAXIMUM of an all-negative
octave (plateaus: the image minus 300) are."""
import numpy as np
import pytest

import resample_designs as rd
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd.chanfunc import SPECS
from waldboost_amd.engine import PyramidEngine

pytestmark = pytest.mark.gpu

FUNCS = {"grad_hist": wb.channels.grad_hist, "grad_mag": wb.channels.grad_mag, "grad_hist_4_u1": wb.fpga.grad_hist_4_u1,
         "grad_mag_u1": wb.fpga.grad_mag_u1}


def oracle_pyramid(img, func, shrink, n_per_oct, smooth):
    return list(orc.channel_pyramid(img, dict(shrink=shrink, n_per_oct=n_per_oct, smooth=smooth, channels=func)))


def engine_pyramids(imgs, func, shrink, n_per_oct, smooth, table):
    """The pyramids of a batch [B, H, W] in ONE launch of a freshly built engine (the patch table is computed in the
    constructor: `table` says whether it must be there): per image the list of (channels, scale)."""
    B, H, W = imgs.shape
    eng = PyramidEngine(H, W, imgs.dtype, shrink, n_per_oct, smooth, batch=B, channels=SPECS[func])
    assert (eng.chan_patches is not None) == (table and func != "grad_mag" and imgs.dtype == np.uint8)
    eng.load_images(imgs)
    eng.run_channels()
    return [[(eng.read_level(b, l), eng.plan.scales[l]) for l in range(eng.plan.n_levels)] for b in range(B)]


def same_pyramid(got, ref, what, func, shrink, n_per_oct, smooth, shape, masks=None):
    assert len(got) == len(ref), what
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.dtype == rc.dtype and c.shape == rc.shape, (what, l)
        if not np.array_equal(np.ascontiguousarray(c).view(np.uint8), np.ascontiguousarray(rc).view(np.uint8)):
            plan = rd.make_plan(shape[0], shape[1], func, shrink, n_per_oct, smooth)
            pytest.fail(f"{what}: " + rd.describe_mismatch(c, rc, l, func, shrink, smooth, plan, masks))


def masks_of(design, shrink, dtype, slot=1):
    return rd.design_masks(design, shrink, "uint8" if dtype == "float32" else dtype, slot)


@pytest.mark.parametrize("case", rd.CASES, ids=rd.case_id)
def test_designed_levels_through_every_cell(case, monkeypatch):
    design, func, dtype, shrink, smooth = case
    img, opts, _ = rd.design_image(design, shrink, dtype)
    npo = opts["n_per_oct"]
    ref = oracle_pyramid(img, func, shrink, npo, smooth)
    masks = masks_of(design, shrink, dtype)
    args = (func, shrink, npo, smooth, img.shape, masks)
    got = list(wb.channels.channel_pyramid(img, dict(shrink=shrink, n_per_oct=npo, smooth=smooth, channels=FUNCS[func])))
    same_pyramid(got, ref, "level by level, patch table", *args)
    if dtype == "uint8":
        # once more without the host's table: every workgroup computes its patch extent itself
        monkeypatch.setenv("WB_NO_TILE_PATCHES", "1")
        bare = engine_pyramids(img[None], func, shrink, npo, smooth, table=False)[0]
        same_pyramid(bare, ref, "one launch, no patch table", *args)
        same_pyramid(bare, got, "no patch table against patch table", *args)


@pytest.mark.parametrize("smooth", rd.SMOOTHS)
@pytest.mark.parametrize("shrink", rd.SHRINKS)
@pytest.mark.parametrize("func,dtype", [c for c in rd.CELL_INPUTS if c[1] != "float32"], ids=str)
def test_plateaus_batch_of_two_keeps_each_image_to_its_own_range(func, dtype, shrink, smooth):
    """Slot 0 has the smaller minimum (12), slot 1 the larger (37): image 1 clipped to image 0's range keeps the 36s the
    truncation leaves on its plateaus, and, the images swapped, image 1 clipped to image 0's range has its 12s raised.
    int16 (all negative: the maximum is the live bound): the maxima are -240 and -237, wrong for each other likewise."""
    imgs, opts, _ = rd.plateaus(shrink, dtype)
    npo = opts["n_per_oct"]
    refs = [oracle_pyramid(im, func, shrink, npo, smooth) for im in imgs]
    for order in ((0, 1), (1, 0)):
        got = engine_pyramids(np.ascontiguousarray(imgs[list(order)]), func, shrink, npo, smooth, table=True)
        for b, slot in enumerate(order):
            same_pyramid(got[b], refs[slot], f"batch slot {b} (design image {slot})", func, shrink, npo, smooth, imgs.shape[1:],
                         masks_of("plateaus", shrink, dtype, slot))


@pytest.mark.parametrize("cell", rd.PATH_CELLS, ids=rd.case_id)
def test_every_path_of_a_cell_with_and_without_the_patch_table(cell, monkeypatch):
    func, shrink, smooth = cell
    for H, W, npo in rd.path_levels(func, shrink, smooth)[0]:
        img = rd.path_image(H, W)
        ref = oracle_pyramid(img, func, shrink, npo, smooth)
        args = (func, shrink, npo, smooth, img.shape)
        with_table = engine_pyramids(img[None], func, shrink, npo, smooth, table=True)[0]
        same_pyramid(with_table, ref, f"{H}x{W}/{npo}, patch table", *args)
        with monkeypatch.context() as m:
            m.setenv("WB_NO_TILE_PATCHES", "1")
            bare = engine_pyramids(img[None], func, shrink, npo, smooth, table=False)[0]
        same_pyramid(bare, ref, f"{H}x{W}/{npo}, no patch table", *args)
        same_pyramid(bare, with_table, f"{H}x{W}/{npo}, no patch table against patch table", *args)
