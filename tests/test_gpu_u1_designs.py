"""Step 2 and step 3 of channels_u1_kernel (csrc/wb_chan_u1.hip) on the designed inputs of u1_designs.py, byte for byte
against the oracle: every design through the six cells (shrink 1, 2, 4 x smooth 0, 1) of both integer functions at
n_per_oct = 1, a batch of two designs in one launch and in either order, and the wrap and border designs through a small
cascade whose thresholds sit on the pooled values on either side of a wrap.  test_u1_designs_host.py proves what the designs
hold and that a wrong kernel would show."""
import numpy as np
import pytest

import u1_designs as ud
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd.chanfunc import SPECS
from waldboost_amd.engine import PyramidEngine
from util import oracle_detect

pytestmark = pytest.mark.gpu

FUNCS = {"grad_hist_4_u1": wb.fpga.grad_hist_4_u1, "grad_mag_u1": wb.fpga.grad_mag_u1}
CELLS = [(f, d, s, sm) for f in FUNCS for d in ud.DESIGNS for s in ud.SHRINKS for sm in ud.SMOOTHS]


def ident(c):
    return "-".join(str(x) for x in c)


def oracle_pyramid(img, func, shrink, smooth):
    return list(orc.channel_pyramid(img, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=func)))


def same_pyramid(got, ref, what, img, func, shrink, smooth):
    assert len(got) == len(ref) > 0, what
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.dtype == rc.dtype == np.uint8 and c.shape == rc.shape, (what, l)
        if not np.array_equal(c, rc):
            pytest.fail(f"{what}: " + ud.describe_mismatch(c, rc, img, func, shrink, smooth, l))


@pytest.mark.parametrize("cell", CELLS, ids=ident)
def test_designs_through_the_cells(cell):
    func, name, shrink, smooth = cell
    for index, img in enumerate(ud.design_images(name, shrink)):
        got = list(wb.channels.channel_pyramid(img, dict(shrink=shrink, n_per_oct=1, smooth=smooth, channels=FUNCS[func])))
        same_pyramid(got, oracle_pyramid(img, func, shrink, smooth), f"{func} on {name}[{index}]", img, func, shrink, smooth)


def engine_pyramids(imgs, func, shrink, smooth):
    B, H, W = imgs.shape
    eng = PyramidEngine(H, W, imgs.dtype, shrink, 1, smooth, batch=B, channels=SPECS[func])
    eng.load_images(imgs)
    eng.run_channels()
    return [[(eng.read_level(b, l), eng.plan.scales[l]) for l in range(eng.plan.n_levels)] for b in range(B)]


@pytest.mark.parametrize("smooth", ud.SMOOTHS)
@pytest.mark.parametrize("shrink", ud.SHRINKS)
@pytest.mark.parametrize("func", sorted(FUNCS))
def test_batch_of_two_designs_in_one_launch(func, shrink, smooth):
    """The wrap mosaic beside the seams texture (equal shapes, nothing in common), either order: workgroup (tile, image)
    reads its own image's pixels and halo."""
    pair = [ud.design_images("wrap", shrink)[0], ud.design_images("seams", shrink)[0]]
    assert pair[0].shape == pair[1].shape and not np.array_equal(*pair)
    refs = [oracle_pyramid(im, func, shrink, smooth) for im in pair]
    for order in ((0, 1), (1, 0)):
        imgs = np.ascontiguousarray(np.stack(pair)[list(order)])
        got = engine_pyramids(imgs, func, shrink, smooth)
        for b, slot in enumerate(order):
            same_pyramid(got[b], refs[slot], f"batch slot {b} ({('wrap', 'seams')[slot]})", imgs[b], func, shrink, smooth)


SHAPE = (6, 12)


def wrap_cascade(func, smooth, values, seed):
    """Depth-2 trees whose thresholds are a pooled value v that a wrapped block of the design holds, v - 1 and the value the
    block would hold without the wrap (v + 64, 128 or 192): `x <= t` decides differently on either side of the wrap."""
    rng = np.random.default_rng(seed)
    nch = len(values)
    shape = SHAPE + (nch,)
    M = wb.Model(shape, dict(shrink=2, n_per_oct=1, smooth=smooth, channels=FUNCS[func]))
    left, right = np.array([1, 3, 5, -1, -1, -1, -1], np.int8), np.array([2, 4, 6, -1, -1, -1, -1], np.int8)
    for t in range(9):
        k = t % nch
        v, unwrapped = values[k]
        thr = np.array([v, max(v - 1, 0), unwrapped - 1, 0, 0, 0, 0], np.float32)
        thr[:3] = thr[:3][rng.permutation(3)]
        feat = np.zeros((7, 3), np.uint8)
        feat[:3] = np.stack([rng.integers(0, shape[0], 3), rng.integers(0, shape[1], 3), [k, (t + 1) % nch, (t + 2) % nch]], 1)
        pred = np.zeros(7, np.float32)
        pred[3:] = (rng.uniform(0.2, 1.0, 4) * rng.choice([-1.0, 1.0], 4)).astype(np.float32)
        theta = float("-inf") if t % 4 == 3 else float(np.float32(-0.1 - 0.05 * t))
        M.append(wb.DTree(feat, thr, left, right, pred), theta)
    return M


def wrapped_values(img, func):
    """Per channel (v, w): the commonest pooled value v among the blocks of level 0 whose sum wrapped, and the value w the
    commonest such block would hold without the wrap."""
    m = ud.intermediates(img, func, 2)
    out = []
    for k in range(m["level"].shape[-1]):
        wrapped = m["sums"][..., k] >= 256
        assert wrapped.any()
        wrapped &= (m["level"][..., k] > 0) | ~(wrapped & (m["level"][..., k] > 0)).any()       # (a value above 0 where there is one)
        vals, n = np.unique(m["level"][..., k][wrapped], return_counts=True)
        v = int(vals[np.argmax(n)])
        s = m["sums"][..., k][wrapped & (m["level"][..., k] == v)]
        out.append((v, int(s[0] >> 2)))
    return out


# (the wrap design's waves image: the mosaic is flat between its patches, and no cascade of this family splits its windows)
CASCADE_CASES = [("wrap", 1), ("border", 1), ("border", 3)]
# seeds whose cascade keeps some windows of level 0 and drops others (found on the CPU with the oracle)
CASCADE_SEEDS = {("grad_hist_4_u1", "wrap", 1, 0): 2, ("grad_hist_4_u1", "wrap", 1, 1): 2, ("grad_hist_4_u1", "border", 1, 0): 3,
                 ("grad_hist_4_u1", "border", 1, 1): 3, ("grad_hist_4_u1", "border", 3, 0): 14, ("grad_hist_4_u1", "border", 3, 1): 14,
                 ("grad_mag_u1", "wrap", 1, 0): 0, ("grad_mag_u1", "wrap", 1, 1): 2, ("grad_mag_u1", "border", 1, 0): 220,
                 ("grad_mag_u1", "border", 1, 1): 15, ("grad_mag_u1", "border", 3, 0): 220, ("grad_mag_u1", "border", 3, 1): 15}


@pytest.mark.parametrize("smooth", ud.SMOOTHS)
@pytest.mark.parametrize("case", CASCADE_CASES, ids=ident)
@pytest.mark.parametrize("func", sorted(FUNCS))
def test_cascade_thresholds_on_either_side_of_a_wrap(func, case, smooth):
    name, index = case
    img = ud.design_images(name, 2)[index]
    M = wrap_cascade(func, smooth, wrapped_values(img, func), CASCADE_SEEDS[func, name, index, smooth])
    ref = oracle_detect(M, img)
    res = M.detect_raw(img)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(res["alive"], ref["alive"])
    assert np.array_equal(res["level"], ref["level"]) and np.array_equal(res["r"], ref["r"]) and np.array_equal(res["c"], ref["c"])
    assert np.array_equal(f32(res["scores"]), f32(ref["scores"])) and np.array_equal(f32(res["boxes"]), f32(ref["boxes"]))
    u, v = img.shape[0] // 2, img.shape[1] // 2
    n_win = ref["alive"][0, 0]
    kept = int((ref["level"] == 0).sum())
    assert n_win == (u - SHAPE[0]) * (v - SHAPE[1]) and 0 < kept < n_win, (kept, n_win)
    assert (ref["alive"][0] < n_win).any()
