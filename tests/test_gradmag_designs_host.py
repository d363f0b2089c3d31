"""CPU proofs for gradmag_designs.py (no GPU): the kernel restated in NumPy -- pixels mirrored into a 6-pixel halo, the
triangle passes over the haloed magnitudes -- gives the oracle's bits on every level of every design, the designs hold what
they were built to hold (with the counts found), no float design meets an inf or a NaN anywhere in the oracle's pipeline,
every wrong kernel of gm.WRONG_KERNELS differs from the oracle by the asserted number of output pixels in every cell it
applies to, and the findings of the module docstring hold.  Every count asserted here is one the oracle produced on the
CPU; `python tests/test_gradmag_designs_host.py` prints the table."""
import functools

import numpy as np
import pytest

import gradmag_designs as gm
from oracle import wb_oracle as orc

CELLS = [(s, sm) for s in gm.SHRINKS for sm in gm.SMOOTHS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def all_levels(shrink):
    """((design, index, level, pixels), ...) over every design, both dtypes and every level of the pyramid."""
    out = []
    for name, index, img in gm.cases(shrink):
        for l, px in enumerate(gm.levels_of(img, shrink, gm.N_PER_OCT.get(name, 1))):
            out.append((name, index, l, px))
    return tuple(out)


@functools.lru_cache(None)
def oracle_levels(shrink, smooth):
    return tuple(gm.oracle_level(px, shrink, smooth) for _, _, _, px in all_levels(shrink))


def n_wrong(shrink, smooth, wrong, designs=gm.DESIGNS):
    n = 0
    for (name, index, l, px), ref in zip(all_levels(shrink), oracle_levels(shrink, smooth)):
        if name in designs:
            n += int((bits(gm.emulate(px, shrink, smooth, wrong)) != bits(ref)).sum())
    return n


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_restated_kernel_gives_the_oracle_bits(cell):
    """Mirrored pixels under the gradient passes against the oracle's mirrored magnitudes, levels with a side of 4 included."""
    shrink, smooth = cell
    n_deeper = 0
    for (name, index, l, px), ref in zip(all_levels(shrink), oracle_levels(shrink, smooth)):
        got = gm.emulate(px, shrink, smooth)
        assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), (name, index, l)
        n_deeper += l > 0
    assert n_deeper >= 10


def test_designs_stay_within_two_tiles_by_two_and_are_identity_levels():
    for shrink in gm.SHRINKS:
        g = gm.tile_geom(shrink)
        for name, index, img in gm.cases(shrink):
            h, w = img.shape
            assert h <= 70 and w <= 260 and -(-h // (shrink * g["TU"])) <= 2 and -(-w // (shrink * g["TV"])) <= 2
            if name not in gm.N_PER_OCT:
                assert h % shrink == 0 and w % shrink == 0 and gm.is_identity(img, shrink, 0)
                assert np.array_equal(gm.levels_of(img, shrink)[0], img)


def test_a_mismatch_is_described_with_its_intermediates():
    for shrink, smooth in CELLS:
        img = gm.design_images("seams", shrink)[0]
        ref = gm.oracle_level(img, shrink, smooth)
        got = ref.copy()
        got[3, 5, 0] = np.nextafter(got[3, 5, 0], np.float32(9))
        msg = gm.describe_mismatch(got, ref, img, "seams", shrink, smooth)
        assert "1 output pixels differ, first at (3, 5)" in msg and "tile (0, 0)" in msg and "triangle [[" in msg


def test_float_designs_are_finite_in_every_intermediate():
    n = 0
    for shrink in gm.SHRINKS:
        for name, index, l, px in all_levels(shrink):
            if px.dtype != np.float32:
                continue
            with np.errstate(under="ignore"):
                gx, gy = orc.gradients(px)
                mag = np.sqrt(gx ** 2 + gy ** 2)
                first = orc._conv_sym(mag, gm.TRI, 0)
                nrm = orc._conv_sym(first, gm.TRI, 1)
            for a in (px, gx, gy, mag, first, nrm, nrm + gm.EPS) + tuple(gm.oracle_level(px, shrink, sm) for sm in gm.SMOOTHS):
                assert np.isfinite(a).all(), (name, index, l)
            assert (nrm + gm.EPS > 0).all()
            n += 1
    assert n >= 60


# ------------------------------------------------------------------------------ the designs' conditions
def test_reflect_sizes_and_asymmetry():
    for shrink in gm.SHRINKS:
        g = gm.tile_geom(shrink)
        for d, img in zip(gm.BORDER_DELTAS, gm.design_images("reflect", shrink)):
            assert img.shape == (shrink * (g["TU"] + d), shrink * (g["TV"] + d))
            # no border is a mirror line: the six rows (columns) inside it differ from their reflection about any nearby axis
            for a in (img, img[::-1], img.T, img.T[::-1]):
                for k in range(1, 7):
                    assert not np.array_equal(a[:k], a[k:2 * k][::-1])
        for sm in gm.SMOOTHS:
            for wrong in ("clamped_halo", "mirror_of_magnitudes"):
                assert n_wrong(shrink, sm, wrong, ("reflect",)) > 0


def test_side4_levels_have_a_side_of_exactly_four():
    """Rows only, columns only, both -- and the level is the last of its octave, resampled from 8 pixels."""
    for shrink in gm.SHRINKS:
        shapes = []
        for img in gm.design_images("side4", shrink):
            plan = orc.level_plan(img.shape[0], img.shape[1], shrink, 4)
            four = [(lv["nh"], lv["nw"]) for lv in plan if 4 in (lv["nh"], lv["nw"])]
            assert four and all(lv["oct"] == 0 for lv in plan)
            shapes.append(four[-1])
        print("shrink", shrink, "levels with a side of 4:", shapes)
        assert shapes[0][0] == 4 < shapes[0][1] and shapes[1][1] == 4 < shapes[1][0] and shapes[2] == (4, 4)
        assert n_wrong(shrink, 0, "mirror_then_clamp", ("side4",)) > 0


ZERO_FACTS = {1: (1904, 336, 238, 43), 2: (1628, 612, 1136, 320), 4: (260, 348, 1392, 340)}


def test_zero_design_gives_exact_positive_zeros_beside_eps():
    """Per shrink (smooth 0, level 0 of the uint8 image): outputs that are +0, outputs above 0, resized pixels whose
    normaliser is 0, and pixels whose normaliser lies in (0, 8 eps)."""
    found = {}
    for shrink in gm.SHRINKS:
        img = gm.design_images("zero", shrink)[0]
        out = gm.oracle_level(img, shrink, 0)
        assert not np.isnan(out).any() and not (bits(out) == 0x80000000).any()
        _, mag, nrm = gm.normalised(img, parts=True)
        found[shrink] = (int((bits(out) == 0).sum()), int((out > 0).sum()), int((nrm == 0).sum()), int(((nrm > 0) & (nrm < 8 * gm.EPS)).sum()))
        assert ((nrm == 0) <= (mag == 0)).all()
    print("zero design:", found)
    assert found == ZERO_FACTS and all(min(v) > 0 for v in found.values())


UNIT_FACTS = (2240, 428)


def test_unit_design_has_normalisers_of_the_order_of_eps():
    """Level 0 at shrink 1: pixels of the [0, 2^-8] image with a normaliser below 8 eps, and below eps."""
    a, b = gm.design_images("unit", 1)
    assert a.dtype == b.dtype == np.float32 and 0 <= a.min() and a.max() <= 1 and 0 <= b.min() and b.max() <= 2.0 ** -8
    na, nb = gm.normalised(a, parts=True)[2], gm.normalised(b, parts=True)[2]
    found = (int((nb < 8 * gm.EPS).sum()), int((nb < gm.EPS).sum()))
    assert na.min() > 100 * gm.EPS                              # (the [0, 1] image: eps is small beside the normaliser)
    print("unit design:", found)
    assert found == UNIT_FACTS and found[0] == nb.size and found[1] > 100
    # eps is not negligible: dropping it changes every output bit pattern of the small image
    assert (bits(gm.normalised(b)) != bits(gm.normalised(b, parts=True)[1] / nb)).mean() > 0.99


TINY_FACTS = (2235, 5, 2235)


def test_tiny_design_lands_in_the_subnormal_range():
    for shrink in gm.SHRINKS:
        small, smaller = gm.design_images("tiny", shrink)
        with np.errstate(under="ignore"):
            gx, gy = orc.gradients(small)
            sq = gx * gx + gy * gy
            assert (sq < gm.FLT_MIN).all() and np.isfinite(sq).all()
            gx, gy = orc.gradients(smaller)
            assert (gx != 0).any() and not (gx * gx + gy * gy).any()
        for sm in gm.SMOOTHS:
            assert not bits(gm.oracle_level(smaller, shrink, sm)).any()           # +0 everywhere
        if shrink == 1:
            found = (int((sq > 0).sum()), int((sq == 0).sum()), int((gm.oracle_level(small, 1, 0) > 0).sum()))
            print("tiny design, level 0 at shrink 1: subnormal squares, squares of 0, outputs above 0:", found)
            assert found == TINY_FACTS and found[0] > 1000
        assert n_wrong(shrink, 0, "squares_flushed", ("tiny",)) > 0


SQUARES_REACHED = 7448


def test_squares_reached_and_exact():
    sums = set()
    for shrink in gm.SHRINKS:
        for name, index, l, px in all_levels(shrink):
            if px.dtype == np.uint8:
                gx, gy = orc.gradients(px.astype(np.float32))
                s = gx.astype(np.int64) ** 2 + gy.astype(np.int64) ** 2
                assert s.max() <= 2 * 1020 ** 2 < 2 ** 24 and np.array_equal((gx * gx + gy * gy).astype(np.int64), s)
                if name == "squares":
                    sums |= set(np.unique(s).tolist())
    print("distinct gx^2 + gy^2 in the squares design:", len(sums))
    assert len(sums) == SQUARES_REACHED >= 5000


def test_order_profiles_separate_the_two_orders():
    from fractions import Fraction
    assert len(gm.ORDER_PROFILES) == len(gm.design_images("order", 1)) >= 4
    c = gm.ORDER_CENTRE
    for img in gm.design_images("order", 1):
        ref, mag, _ = gm.normalised(img, parts=True)
        assert bits(ref)[c, 4] != bits(gm.normalised(img, "plain_order"))[c, 4]
        B, a, b = float(mag[c, 0]), float(mag[c + 2, 0]), float(mag[c - 4, 0])
        assert mag[c - 2, 0] == B and mag[c + 4, 0] == a and B > 2 ** 19 * a and a > 2 ** 19 * b > 0       # widely different exponents
        assert np.count_nonzero(mag[:, 0]) == 6 and np.array_equal(mag[:, 0], np.abs(orc.gradients(img)[1][:, 0]))
        # the exact sum of the centre window lies within 2^-60 (relative) of the midpoint between two neighbouring fp32 numbers
        w = [Fraction(float(v)) for v in gm.TRI]
        exact = sum(Fraction(float(mag[c + j, 0])) * w[5 + j] for j in range(-5, 6))
        lo = np.float32(float(exact))
        lo, hi = (lo, np.nextafter(lo, np.float32(np.inf))) if Fraction(float(lo)) <= exact else (np.nextafter(lo, np.float32(0)), lo)
        mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
        assert abs(exact - mid) < exact * Fraction(1, 2 ** 60)


# ------------------------------------------------------------------------------ wrong kernels
# keys: (shrink, smooth)
WRONG_COUNTS = {'clamped_halo': {(1, 0): 17524, (1, 1): 15699, (2, 0): 11768, (2, 1): 10414, (4, 0): 3787, (4, 1): 2835},
 'mirror_then_clamp': {(1, 0): 176, (1, 1): 144, (2, 0): 176, (2, 1): 0, (4, 0): 66, (4, 1): 0},
 'mirror_of_magnitudes': {(1, 0): 17812, (1, 1): 16000, (2, 0): 11812, (2, 1): 10452, (4, 0): 3811, (4, 1): 2853},
 'fp64_between_passes': {(1, 0): 2458, (1, 1): 2415, (2, 0): 3319, (2, 1): 3410, (4, 0): 993, (4, 1): 964},
 'other_axis_order': {(1, 0): 3353, (1, 1): 3050, (2, 0): 3743, (2, 1): 4018, (4, 0): 1057, (4, 1): 885},
 'plain_order': {(1, 0): 48, (1, 1): 84, (2, 0): 48, (2, 1): 72, (4, 0): 48, (4, 1): 96},
 'eps_in_fp64': {(1, 0): 8277, (1, 1): 8286, (2, 0): 6800, (2, 1): 6430, (4, 0): 1930, (4, 1): 1656},
 'reciprocal': {(1, 0): 7505, (1, 1): 4445, (2, 0): 6489, (2, 1): 4387, (4, 0): 1708, (4, 1): 1172},
 'sqrt_of_fp64_sum': {(1, 0): 7006, (1, 1): 5998, (2, 0): 7041, (2, 1): 5903, (4, 0): 1914, (4, 1): 1428},
 'pool_pairs': {(2, 0): 8630, (2, 1): 4560, (4, 0): 2839, (4, 1): 1385},
 'smooth_border_at_tile_edge': {(1, 1): 1794, (2, 1): 1818, (4, 1): 994},
 'squares_flushed': {(1, 0): 2930, (1, 1): 2592, (2, 0): 2968, (2, 1): 2604, (4, 0): 804, (4, 1): 620}}
# cells in which a wrong kernel cannot show (findings): a level with a side of 4 has 2 or 1 pooled rows at shrink 2 and 4,
# where the smooth leaves all zeros
ZERO_CELLS = {"mirror_then_clamp": ((2, 1), (4, 1))}


@pytest.mark.parametrize("wrong", gm.WRONG_KERNELS)
def test_wrong_kernels_are_caught_in_every_cell(wrong):
    """Output pixels (over all designs, both dtypes, all levels) a wrong kernel gets wrong, per (shrink, smooth)."""
    found = {c: n_wrong(*c, wrong) for c in CELLS if gm.applies(wrong, *c)}
    print(wrong, found)
    assert found == WRONG_COUNTS[wrong]
    assert {c for c, n in found.items() if n == 0} == set(ZERO_CELLS.get(wrong, ()))


def test_each_design_catches_what_it_was_built_for():
    for shrink, smooth in CELLS:
        for design, wrongs in (("reflect", ("clamped_halo", "mirror_of_magnitudes", "fp64_between_passes", "other_axis_order")),
                               ("unit", ("eps_in_fp64", "reciprocal", "sqrt_of_fp64_sum")), ("zero", ("eps_in_fp64",)),
                               ("squares", ("reciprocal",)), ("order", ("plain_order",)), ("tiny", ("squares_flushed",)),
                               ("seams", ("pool_pairs", "smooth_border_at_tile_edge"))):
            for wrong in wrongs:
                if gm.applies(wrong, shrink, smooth):
                    assert n_wrong(shrink, smooth, wrong, (design,)) > 0, (design, wrong, shrink, smooth)


# ------------------------------------------------------------------------------ findings
def test_one_mirror_then_clamp_is_right_from_a_side_of_five_and_plain_order_outside_its_design():
    others = tuple(d for d in gm.DESIGNS if d != "side4")
    no_order = tuple(d for d in gm.DESIGNS if d != "order")
    for shrink, smooth in CELLS:
        assert n_wrong(shrink, smooth, "mirror_then_clamp", others) == 0
        assert n_wrong(shrink, smooth, "plain_order", no_order) == 0
    for n in range(4, 12):
        same = np.array_equal(gm.halo_index(n, "reflect"), gm.halo_index(n, "mirror_then_clamp"))
        assert same == (n >= 5)


def test_sqrt_of_a_square_is_the_magnitude():
    rng = np.random.default_rng(3)
    x = (rng.uniform(1, 2, 200000) * 2.0 ** rng.integers(-40, 40, 200000)).astype(np.float32)
    assert np.array_equal(np.sqrt(x * x), x)


def test_double_rounding_of_the_fp64_square_root_shows_on_integer_gradients():
    """The sums of squares are exact on uint8 images, yet sqrt in fp64 followed by a rounding to fp32 is not the fp32 sqrt."""
    assert n_wrong(1, 0, "sqrt_of_fp64_sum", ("reflect", "seams", "zero")) > 0


if __name__ == "__main__":
    table = {w: {c: n_wrong(*c, w) for c in CELLS if gm.applies(w, *c)} for w in gm.WRONG_KERNELS}
    print("WRONG_COUNTS = {")
    for w, t in table.items():
        print(f"    {w!r}: {t},")
    print("}")
