"""Step 2 and step 3 of channels_kernel (csrc/wb_channels.hip) on the designed gradients of gradient_designs.py, bit for
bit against the oracle: every design through the six uint8 grad_hist cells (shrink 1, 2, 4 x smooth 0, 1) at
n_per_oct = 1, the same pixels as float32 images (channels_kernel<float, ..., FAST = false>: project_f64 and the smooth's
chain on every tile), a batch of two in one launch (the per-workgroup flag must neither leak to nor be lost from a
batch-mate), and the rank bytes through a small cascade whose thresholds tell an exact 0 from a residue from an ordinary
value.  test_gradient_designs_host.py proves what the designs hold and that a wrong kernel would show.

grad_mag, grad_hist_4_u1 and grad_mag_u1 ride along on the same images at their cells: these images are not designed for
them (no projection, no residues, no flag), they are simply further inputs with many zero and extreme gradients.  Their own
designs are u1_designs.py (test_gpu_u1_designs.py) and gradmag_designs.py (test_gpu_gradmag_designs.py)."""
import numpy as np
import pytest

import gradient_designs as gd
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd.chanfunc import SPECS
from waldboost_amd.engine import PyramidEngine
from util import oracle_detect

pytestmark = pytest.mark.gpu

FUNCS = {"grad_hist": wb.channels.grad_hist, "grad_mag": wb.channels.grad_mag, "grad_hist_4_u1": wb.fpga.grad_hist_4_u1,
         "grad_mag_u1": wb.fpga.grad_mag_u1}
CELLS = [(d, i, s, sm) for d, i in gd.CASES for s in gd.SHRINKS for sm in gd.SMOOTHS]
SHAPE = (12, 12, 4)


def ident(c):
    return "-".join(str(x) for x in c)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def oracle_pyramid(img, func, shrink, smooth):
    return list(orc.channel_pyramid(img, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=func)))


def same_pyramid(got, ref, what, img, shrink, smooth, designed=True):
    assert len(got) == len(ref) > 0, what
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.dtype == rc.dtype and c.shape == rc.shape, (what, l)
        if not np.array_equal(bits(c), bits(rc)):
            if designed:
                pytest.fail(f"{what}: " + gd.describe_mismatch(c, rc, img, shrink, smooth, l))
            pytest.fail(f"{what}: level {l}, {int((bits(c) != bits(rc)).sum())} bytes differ")


@pytest.mark.parametrize("cell", CELLS, ids=ident)
def test_designs_through_the_uint8_cells(cell):
    name, index, shrink, smooth = cell
    img = gd.design_images(name, shrink)[index]
    got = list(wb.channels.channel_pyramid(img, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=wb.channels.grad_hist)))
    same_pyramid(got, oracle_pyramid(img, "grad_hist", shrink, smooth), "uint8", img, shrink, smooth)


@pytest.mark.parametrize("cell", CELLS, ids=ident)
def test_designs_as_float_images(cell):
    """The general route: the same integers as float32 pixels -- fp64 projection per pixel, the nine-term chain per output."""
    name, index, shrink, smooth = cell
    img = gd.design_images(name, shrink)[index]
    imf = img.astype(np.float32)
    got = list(wb.channels.channel_pyramid(imf, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=wb.channels.grad_hist)))
    same_pyramid(got, oracle_pyramid(imf, "grad_hist", shrink, smooth), "float32", img, shrink, smooth)


def engine_pyramids(imgs, shrink, smooth):
    B, H, W = imgs.shape
    eng = PyramidEngine(H, W, imgs.dtype, shrink, 1, smooth, batch=B, channels=SPECS["grad_hist"])
    eng.load_images(imgs)
    eng.run_channels()
    return [[(eng.read_level(b, l), eng.plan.scales[l]) for l in range(eng.plan.n_levels)] for b in range(B)]


@pytest.mark.parametrize("variant", ["all", "wave3", "lanes", "bottom2"])
@pytest.mark.parametrize("shrink", gd.SHRINKS)
def test_batch_mates_keep_their_own_flag(shrink, variant):
    """One launch, two images, either order: the smooth_windows design (tiles that must take the chain) beside the plain
    image of the same shape (no odd value: every tile takes the fast smooth).  Workgroup (tile, image) owns its flag."""
    design = gd.window_image(shrink, variant)
    plain = gd.flat_image(shrink, variant)
    refs = [oracle_pyramid(im, "grad_hist", shrink, 1) for im in (design, plain)]
    for order in ((0, 1), (1, 0)):
        imgs = np.ascontiguousarray(np.stack([design, plain])[list(order)])
        got = engine_pyramids(imgs, shrink, 1)
        for b, slot in enumerate(order):
            same_pyramid(got[b], refs[slot], f"batch slot {b} ({'design' if slot == 0 else 'plain'} image)", imgs[b], shrink, 1)


def class_cascade(values, seed):
    """Depth-2 trees over channels 1 .. 3 whose thresholds are 0, a residue value of the design and that value's next float32
    below: `v <= 0` is true for Z alone, `v <= below(r)` for Z and smaller residues, `v <= r` up to r itself."""
    rng = np.random.default_rng(seed)
    M = wb.Model(SHAPE, dict(shrink=2, n_per_oct=1, smooth=values["smooth"], channels=wb.channels.grad_hist))
    left, right = np.array([1, 3, 5, -1, -1, -1, -1], np.int8), np.array([2, 4, 6, -1, -1, -1, -1], np.int8)
    for t in range(9):
        k = 1 + t % 3
        r = np.float32(values[k])
        thr = np.array([0.0, r, np.nextafter(r, np.float32(-np.inf)), 0, 0, 0, 0], np.float32)
        thr[:3] = thr[:3][rng.permutation(3)]
        feat = np.zeros((7, 3), np.uint8)
        feat[:3] = np.stack([rng.integers(0, SHAPE[0], 3), rng.integers(0, SHAPE[1], 3), [k, 1 + (t + 1) % 3, 1 + (t + 2) % 3]], 1)
        pred = np.zeros(7, np.float32)
        pred[3:] = (rng.uniform(0.2, 1.0, 4) * rng.choice([-1.0, 1.0], 4)).astype(np.float32)
        theta = float("-inf") if t % 4 == 3 else float(np.float32(-0.1 - 0.05 * t))
        M.append(wb.DTree(feat, thr, left, right, pred), theta)
    return M


@pytest.mark.parametrize("smooth", gd.SMOOTHS)
@pytest.mark.parametrize("case", [("words", 1), ("order", 0), ("zeros", 0), ("smooth_windows", gd.WINDOW_VARIANTS.index("all"))], ids=ident)
def test_rank_bytes_tell_zero_from_residue_from_ordinary(case, smooth):
    name, index = case
    img = gd.design_images(name, 2)[index]
    lv = gd.oracle_level0(name, index, 2, smooth)
    values = dict(smooth=smooth)
    for k in (1, 2, 3):
        res = lv[..., k][(lv[..., k] > 0) & (lv[..., k] < 1e-6)]
        if res.size == 0:                                   # (smooth_windows: residues in channel 2 alone)
            res = lv[..., 2][(lv[..., 2] > 0) & (lv[..., 2] < 1e-6)]
        vals, n = np.unique(res, return_counts=True)
        values[k] = vals[np.argmax(n)]                      # the commonest residue: pixels ON the threshold
    # (an x-only image decides column by column: seeds whose cascade keeps some columns and drops others)
    M = class_cascade(values, {("smooth_windows", 0): 108, ("smooth_windows", 1): 116}.get((name, smooth), 10 * index + smooth))
    ref = oracle_detect(M, img)
    res = M.detect_raw(img)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(res["alive"], ref["alive"])
    assert np.array_equal(res["level"], ref["level"]) and np.array_equal(res["r"], ref["r"]) and np.array_equal(res["c"], ref["c"])
    assert np.array_equal(f32(res["scores"]), f32(ref["scores"])) and np.array_equal(f32(res["boxes"]), f32(ref["boxes"]))
    n_win = ref["alive"][0, 0]
    kept = int((ref["level"] == 0).sum())
    assert n_win == (lv.shape[0] - SHAPE[0]) * (lv.shape[1] - SHAPE[1]) and 0 < kept < n_win, (kept, n_win)
    assert (ref["alive"][0] < n_win).any()


@pytest.mark.parametrize("smooth", gd.SMOOTHS)
@pytest.mark.parametrize("shrink", gd.SHRINKS)
@pytest.mark.parametrize("func", ["grad_mag", "grad_hist_4_u1", "grad_mag_u1"])
def test_other_channel_functions_ride_along(func, shrink, smooth):
    for name, index in gd.CASES:
        img = gd.design_images(name, shrink)[index]
        got = list(wb.channels.channel_pyramid(img, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=FUNCS[func])))
        same_pyramid(got, oracle_pyramid(img, func, shrink, smooth), f"{func} on {name}[{index}]", img, shrink, smooth, designed=False)
