"""channels_gm_kernel (csrc/wb_chan_gm.hip) on the designed inputs of gradmag_designs.py, bit for bit against the oracle:
every design through the six cells (shrink 1, 2, 4 x smooth 0, 1) at n_per_oct = 1 (side4: 4), the uint8 designs once more
as float32 images of the same integers, and batches of two designs in one launch and in either order, for both image
dtypes.  test_gradmag_designs_host.py proves what the designs hold and that a wrong kernel would show."""
import numpy as np
import pytest

import gradmag_designs as gm
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd.chanfunc import SPECS
from waldboost_amd.engine import PyramidEngine

pytestmark = pytest.mark.gpu

CELLS = [(d, s, sm) for d in gm.DESIGNS for s in gm.SHRINKS for sm in gm.SMOOTHS]


def ident(c):
    return "-".join(str(x) for x in c)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def oracle_pyramid(img, shrink, smooth, n_per_oct=1):
    with np.errstate(under="ignore"):
        return list(orc.channel_pyramid(img, dict(shrink=shrink, n_per_oct=n_per_oct, smooth=smooth, channels="grad_mag")))


def same_pyramid(got, ref, what, img, name, shrink, smooth):
    assert len(got) == len(ref) > 0, what
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.dtype == rc.dtype == np.float32 and c.shape == rc.shape, (what, l)
        if not np.array_equal(bits(c), bits(rc)):
            pytest.fail(f"{what}: " + gm.describe_mismatch(c, rc, img, name, shrink, smooth, l))


@pytest.mark.parametrize("cell", CELLS, ids=ident)
def test_designs_through_the_cells(cell):
    name, shrink, smooth = cell
    npo = gm.N_PER_OCT.get(name, 1)
    for design, index, img in gm.cases(shrink):
        if design != name:
            continue
        got = list(wb.channels.channel_pyramid(img, dict(shrink=shrink, n_per_oct=npo, smooth=smooth, channels=wb.channels.grad_mag)))
        same_pyramid(got, oracle_pyramid(img, shrink, smooth, npo), f"{img.dtype} {name}[{index}]", img, name, shrink, smooth)


def engine_pyramids(imgs, shrink, smooth):
    B, H, W = imgs.shape
    eng = PyramidEngine(H, W, imgs.dtype, shrink, 1, smooth, batch=B, channels=SPECS["grad_mag"])
    eng.load_images(imgs)
    eng.run_channels()
    return [[(eng.read_level(b, l), eng.plan.scales[l]) for l in range(eng.plan.n_levels)] for b in range(B)]


@pytest.mark.parametrize("smooth", gm.SMOOTHS)
@pytest.mark.parametrize("shrink", gm.SHRINKS)
@pytest.mark.parametrize("pair", [("squares", "seams"), ("unit", "tiny")], ids=ident)
def test_batch_of_two_designs_in_one_launch(pair, shrink, smooth):
    """uint8: the squares noise beside the seams texture; float32: noise in [0, 1] beside the subnormal squares.  Workgroup
    (tile, image) reads its own image's pixels, halo and clip range."""
    imgs2 = [gm.design_images(name, shrink)[0] for name in pair]
    assert imgs2[0].shape == imgs2[1].shape and imgs2[0].dtype == imgs2[1].dtype and not np.array_equal(*imgs2)
    refs = [oracle_pyramid(im, shrink, smooth) for im in imgs2]
    for order in ((0, 1), (1, 0)):
        imgs = np.ascontiguousarray(np.stack(imgs2)[list(order)])
        got = engine_pyramids(imgs, shrink, smooth)
        for b, slot in enumerate(order):
            same_pyramid(got[b], refs[slot], f"batch slot {b} ({pair[slot]})", imgs[b], pair[slot], shrink, smooth)
