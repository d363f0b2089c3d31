"""CPU proofs for u1_designs.py (no GPU): step 2 and step 3 of channels_u1_kernel restated in int64 give the oracle's bytes
on every identity level of every design, the designs hold what they were built to hold (with the counts found), every wrong
kernel of ud.WRONG_KERNELS differs from the oracle by the asserted number of output pixels in every cell it applies to, and
the findings of the module docstring hold.  Every count asserted here is one the oracle produced on the CPU;
`python tests/test_u1_designs_host.py` prints the tables."""
import functools

import numpy as np
import pytest

import u1_designs as ud
from oracle import wb_oracle as orc

FUNCS = tuple(ud.FUNCS)
CELLS = [(f, s, sm) for f in FUNCS for s in ud.SHRINKS for sm in ud.SMOOTHS]
ident = lambda c: "-".join(map(str, c))


@functools.lru_cache(None)
def levels(name, index, shrink):
    return tuple(ud.levels_of(ud.design_images(name, shrink)[index], shrink))


def all_levels(shrink, designs=ud.DESIGNS):
    for name, index in ud.cases(shrink):
        if name in designs:
            for l, px in enumerate(levels(name, index, shrink)):
                yield name, index, l, px


@functools.lru_cache(None)
def oracle_level(name, index, l, func, shrink, smooth):
    return ud.oracle_level(levels(name, index, shrink)[l], func, shrink, smooth)


def n_wrong(func, shrink, smooth, wrong, designs=ud.DESIGNS):
    n = 0
    for name, index, l, px in all_levels(shrink, designs):
        got = ud.emulate(px, func, shrink, smooth, wrong)
        n += int((got != oracle_level(name, index, l, func, shrink, smooth)).any(-1).sum())
    return n


@pytest.mark.parametrize("cell", CELLS, ids=ident)
def test_restated_kernel_gives_the_oracle_bytes(cell):
    func, shrink, smooth = cell
    assert ud.same_tiles()
    n_deeper = 0
    for name, index, l, px in all_levels(shrink):
        got, ref = ud.emulate(px, func, shrink, smooth), oracle_level(name, index, l, func, shrink, smooth)
        assert got.dtype == ref.dtype == np.uint8 and got.shape == ref.shape and np.array_equal(got, ref), (name, index, l)
        n_deeper += l > 0
    assert n_deeper >= 10                                  # the deeper octaves are reached ...
    # ... and their bases come from a pool that wrapped
    img = ud.design_images("smooth", shrink)[0].astype(np.int64)
    assert (ud.block_sums(img) >= 256).any() and np.array_equal(levels("smooth", 0, shrink)[1], (ud.block_sums(img) & 255) >> 2)


def test_designs_stay_within_two_tiles_by_two():
    for shrink in ud.SHRINKS:
        g = ud.tile_geom("grad_hist_4_u1", shrink)
        for name, index in ud.cases(shrink):
            h, w = ud.design_images(name, shrink)[index].shape
            assert h % shrink == 0 and w % shrink == 0
            assert h <= 70 and w <= 260 and -(-h // (shrink * g["TU"])) <= 2 and -(-w // (shrink * g["TV"])) <= 2


def test_a_mismatch_is_described_with_its_intermediates():
    for func, shrink, smooth in CELLS:
        img = ud.design_images("wrap", shrink)[1]
        ref = oracle_level("wrap", 1, 0, func, shrink, smooth)
        got = ref.copy()
        got[3, 5, -1] ^= 1
        msg = ud.describe_mismatch(got, ref, img, func, shrink, smooth)
        assert "1 output pixels differ, first at (3, 5)" in msg and "tile (0, 0)" in msg and "dx [[" in msg
        assert ("window sum" in msg) == bool(smooth) and ("first-stage sums" in msg) == (shrink > 1)


# ------------------------------------------------------------------------------ the designs' conditions
def quotient_facts(shrink=2):
    pairs, vals = set(), [set(), set(), set(), set()]
    for img in ud.design_images("values", shrink):
        dx, dy = ud.sobel_ring(img)
        pairs |= set(zip(dx.ravel().tolist(), dy.ravel().tolist()))
        for k, v in enumerate((np.abs(dx), np.abs(dx - dy), np.abs(dy), np.abs(dx + dy))):
            vals[k] |= set(np.unique(v).tolist())
    div = (4, 8, 4, 8)
    sides = tuple(sum(1 for m in range(1, 256) if div[k] * m in vals[k] and div[k] * m - 1 in vals[k]) for k in range(4))
    both = tuple(sum(1 for m in range(1, 256) if div[k] * m in vals[k] and (div[k] * m - 1 in vals[k] or div[k] * m - 2 in vals[k]))
                 for k in range(4))
    return len(pairs), sides, both, tuple(max(v) // div[k] for k, v in enumerate(vals))


PAIRS_REACHED = 14794
QUOTIENT_SIDES = (219, 0, 222, 0)
QUOTIENT_SIDES_EVEN = (232, 165, 233, 171)


def test_values_reach_both_sides_of_the_quotients():
    """|dx| and |dy| take 4 m - 1 and 4 m for QUOTIENT_SIDES[0 / 2] values of m; |dx -+ dy| is even (finding 1), so its two
    sides of a multiple of 8 are 8 m - 2 and 8 m: QUOTIENT_SIDES_EVEN counts those.  The maxima are the attainable ones."""
    n_pairs, sides, both, top = quotient_facts()
    print("distinct (dx, dy):", n_pairs, "multiples with both sides:", sides, "with the even side:", both, "largest quotients:", top)
    assert (n_pairs, sides, both) == (PAIRS_REACHED, QUOTIENT_SIDES, QUOTIENT_SIDES_EVEN)
    assert top == (255, 191, 255, 191) and sides[1] == sides[3] == 0 and min(sides[0], sides[2], both[1], both[3]) >= 100


def wrap_facts():
    """{(shrink, channel key): {target: blocks of level 0 of the wrap design whose first-stage sum is exactly the target}};
    channel key 4 is grad_mag_u1's."""
    out = {}
    for shrink in (2, 4):
        for k in range(5):
            func = "grad_mag_u1" if k == 4 else "grad_hist_4_u1"
            n = dict.fromkeys(ud.WRAP_TARGETS, 0)
            for img in ud.design_images("wrap", shrink):
                s = ud.intermediates(img, func, shrink)["sums"][..., k % 4]
                for t in ud.WRAP_TARGETS:
                    n[t] += int((s == t).sum())
            out[shrink, k] = tuple(n.values())
    return out


WRAP_COUNTS = {(2, 0): (3, 155, 8, 3, 3, 1, 1, 61),
 (2, 1): (6, 37, 4, 1, 1, 0, 0, 0),
 (2, 2): (2, 167, 4, 4, 3, 2, 2, 2),
 (2, 3): (5, 51, 1, 1, 1, 0, 0, 0),
 (2, 4): (4, 243, 2, 5, 6, 2, 3, 63),
 (4, 0): (4, 172, 8, 4, 3, 1, 1, 61),
 (4, 1): (6, 40, 3, 1, 1, 0, 0, 0),
 (4, 2): (2, 179, 4, 4, 3, 2, 2, 2),
 (4, 3): (6, 56, 1, 1, 1, 0, 0, 0),
 (4, 4): (4, 266, 2, 7, 6, 2, 3, 63)}
WRAP_BLOCKS_4 = (207, 41, 188, 83, 319)  # per channel; the last is grad_mag_u1's


def test_wrap_blocks_hold_the_exact_sums():
    """Every searched patch spells its sum at its slot of the mosaic; every target the search reached is there in every
    channel, at both shrinks; at shrink 4 there are 4 x 4 blocks made of four 2 x 2 blocks that all wrap."""
    assert sorted(ud.WRAP_MISSING) == sorted(f"{k}:{t}" for k in range(5) for t in ud.WRAP_TARGETS if f"{k}:{t}" not in ud.WRAP_PATCHES)
    assert all(int(m.split(":")[0]) in (1, 3) and int(m.split(":")[1]) > 764 for m in ud.WRAP_MISSING)
    for shrink in (2, 4):
        mosaic = ud.design_images("wrap", shrink)[0]
        sums = {k: ud.intermediates(mosaic, "grad_mag_u1" if k == 4 else "grad_hist_4_u1", shrink)["sums"][..., k % 4] for k in range(5)}
        for key, (r, c) in ud.mosaic_slots(*mosaic.shape).items():
            k, t = (int(v) for v in key.split(":"))
            assert sums[k][r, c] == t, (shrink, key)
    facts = wrap_facts()
    print("blocks per target", ud.WRAP_TARGETS, facts)
    assert facts == WRAP_COUNTS
    for (shrink, k), n in facts.items():
        assert all(c > 0 or f"{k}:{t}" in ud.WRAP_MISSING for t, c in zip(ud.WRAP_TARGETS, n)), (shrink, k)
    four = []
    for k in range(5):
        func = "grad_mag_u1" if k == 4 else "grad_hist_4_u1"
        w = sum((ud.block_sums((ud.intermediates(img, func, 4)["sums"][..., k % 4] >= 256).astype(np.int64)) == 4).sum()
                for img in ud.design_images("wrap", 4))
        four.append(int(w))
    print("4 x 4 blocks of four wrapping blocks, per channel:", four)
    assert tuple(four) == WRAP_BLOCKS_4 and min(four) > 0


BORDER_BLOCKS = {1: (632, 543), 2: (632, 612), 4: (312, 307)}


def test_border_ring_changes_every_block_that_straddles_it():
    """(blocks on the ring, blocks among them whose pooled value the ring changes) per shrink, grad_hist_4_u1, over the four
    level sizes; the sizes are TU S + d by TV S + d, so the last tile row and column hold 0 (an exact tile), 1 and 2 outputs."""
    found = {}
    for shrink in ud.SHRINKS:
        g = ud.tile_geom("grad_hist_4_u1", shrink)
        n_ring = n_changed = 0
        for d, img in zip(ud.BORDER_DELTAS, ud.design_images("border", shrink)):
            assert img.shape == (shrink * (g["TU"] + d), shrink * (g["TV"] + d))
            ref = ud.emulate(img, "grad_hist_4_u1", shrink, 0)
            got = ud.emulate(img, "grad_hist_4_u1", shrink, 0, "no_ring")
            ring = ud.ring_mask(ref.shape[:2])
            n_ring += int(ring.sum())
            n_changed += int(((got != ref).any(-1) & ring).sum())
            assert not ((got != ref).any(-1) & ~ring).any()
        found[shrink] = (n_ring, n_changed)
    print("ring blocks, changed by the ring:", found)
    # (the texture is random: a ring pixel whose own gradient is zero, or a block whose change is shifted out, stays)
    assert found == BORDER_BLOCKS and all(c >= (0.85 if s == 1 else 0.95) * n for s, (n, c) in found.items())


SMOOTH_SIDES = {1: (386, 5779, 492, 8765, 4080, 2171), 2: (409, 6837, 387, 8413, 1008, 1943), 4: (103, 1586, 98, 2041, 1008, 510)}


def test_smooth_windows_sit_on_both_sides_of_the_multiples():
    """Per shrink: windows of the smooth design (all four channels) with a sum of 16 k - 1, 16 k, 16 k + 1 (k >= 1), the
    windows above 255, the largest sum, and windows whose four channels hold four different sums."""
    found = {}
    for shrink in ud.SHRINKS:
        n = [0, 0, 0, 0, 0, 0]
        for img in ud.design_images("smooth", shrink):
            w = ud.intermediates(img, "grad_hist_4_u1", shrink)["windows"]
            big = w >= 15
            n[0] += int((big & (w % 16 == 15)).sum())
            n[1] += int((big & (w % 16 == 0)).sum())
            n[2] += int((big & (w % 16 == 1)).sum())
            n[3] += int((w > 255).sum())
            n[4] = max(n[4], int(w.max()))
            n[5] += int((np.sort(w, -1)[..., 1:] != np.sort(w, -1)[..., :-1]).all(-1).sum())
        found[shrink] = tuple(n)
    print("smooth windows:", found)
    assert found == SMOOTH_SIDES
    assert found[1][4] == 4080 and found[2][4] <= 1008 and found[4][4] <= 1008 and all(min(v) > 0 for v in found.values())


def test_tiny_levels():
    for shrink in ud.SHRINKS:
        sides = {min(im.shape) for im in ud.design_images("tiny", shrink)}
        assert sides == {n for n in (8, 9, 10) if n % shrink == 0}
        for name, index, l, px in all_levels(shrink):
            assert min(px.shape) >= 8                        # n_per_oct = 1: no level below 8 pixels a side
            rows = min(px.shape) // shrink
            ref = oracle_level(name, index, l, "grad_hist_4_u1", shrink, 1)
            if rows < 3:
                assert shrink == 4 and not ref.any()
        flat = [oracle_level("tiny", i, 0, "grad_hist_4_u1", 4, 1) for i in range(2)]
        assert [f.shape[:2] for f in flat] == [(2, 38), (16, 2)] and not any(f.any() for f in flat)
        assert all(oracle_level("tiny", i, 0, "grad_hist_4_u1", 4, 0).any() for i in range(2))


# ------------------------------------------------------------------------------ wrong kernels
# keys: h / m for grad_hist_4_u1 / grad_mag_u1, then shrink and smooth
WRONG_COUNTS = {'no_ring': {'h10': 3895,
             'h11': 3792,
             'h20': 3280,
             'h21': 3121,
             'h40': 1570,
             'h41': 1282,
             'm10': 3895,
             'm11': 3787,
             'm20': 3151,
             'm21': 2883,
             'm40': 1454,
             'm41': 1059},
 'ring_at_tile_edge': {'h10': 2723,
                       'h11': 4225,
                       'h20': 2300,
                       'h21': 3375,
                       'h40': 1114,
                       'h41': 1533,
                       'm10': 2723,
                       'm11': 4224,
                       'm20': 2221,
                       'm21': 3105,
                       'm40': 1042,
                       'm41': 1281},
 'ring_off_by_one': {'h10': 1832,
                     'h11': 1843,
                     'h20': 1593,
                     'h21': 1502,
                     'h40': 761,
                     'h41': 619,
                     'm10': 1832,
                     'm11': 1839,
                     'm20': 1522,
                     'm21': 1385,
                     'm40': 711,
                     'm41': 513},
 'dx_zeroed_only': {'h10': 3289,
                    'h11': 3295,
                    'h20': 3013,
                    'h21': 2840,
                    'h40': 1426,
                    'h41': 1105,
                    'm10': 3289,
                    'm11': 3278,
                    'm20': 2927,
                    'm21': 2628,
                    'm40': 1359,
                    'm41': 904},
 'pool_no_wrap': {'h20': 9275, 'h21': 12435, 'h40': 3282, 'h41': 3157, 'm20': 9975, 'm21': 12587, 'm40': 3394, 'm41': 3177},
 'pool_rounded': {'h20': 18069, 'h21': 14306, 'h40': 5908, 'h41': 4480, 'm20': 10661, 'm21': 7800, 'm40': 5350, 'm41': 3966},
 'pool4_once': {'h40': 5762, 'h41': 4990, 'm40': 5325, 'm41': 4890},
 'smooth_rounded': {'h11': 19882, 'h21': 15913, 'h41': 4050, 'm11': 11374, 'm21': 9001, 'm41': 2201},
 'smooth_packed': {'h11': 25033, 'h21': 21337, 'h41': 5118},
 'smooth_border_at_tile_edge': {'h11': 2712, 'h21': 2370, 'h41': 1098, 'm11': 2724, 'm21': 2375, 'm41': 1109},
 'smooth_border_without_smooth': {'h10': 0, 'h20': 3398, 'h40': 1672, 'm10': 0, 'm20': 3378, 'm40': 1674},
 'gm_half_sum': {'m10': 21001, 'm11': 23527, 'm20': 19760, 'm21': 17731, 'm40': 5339, 'm41': 4305},
 'gm_min': {'m10': 21441, 'm11': 23704, 'm20': 21949, 'm21': 19925, 'm40': 5938, 'm41': 4753}}


@pytest.mark.parametrize("wrong", ud.WRONG_KERNELS)
def test_wrong_kernels_are_caught_in_every_cell(wrong):
    """Output pixels (over all designs and identity levels) a wrong kernel gets wrong, per (function, shrink, smooth)."""
    found = {cell_key(c): n_wrong(*c, wrong) for c in CELLS if ud.applies(wrong, *c)}
    print(wrong, found)
    assert found == WRONG_COUNTS[wrong]
    assert {c for c, n in found.items() if n == 0} == set(ZERO_CELLS.get(wrong, ()))


# cells in which a wrong kernel cannot show (a finding): at shrink 1 the level's border IS the gradients' zero ring, so a
# smooth border applied with the smooth off changes nothing there
ZERO_CELLS = {"smooth_border_without_smooth": ("h10", "m10")}


def cell_key(c):
    return f"{'h' if c[0] == 'grad_hist_4_u1' else 'm'}{c[1]}{c[2]}"


def test_each_design_catches_what_it_was_built_for():
    for func, shrink, smooth in CELLS:
        for design, wrongs in (("wrap", ("pool_no_wrap", "pool_rounded", "pool4_once")),
                               ("border", ("no_ring", "ring_at_tile_edge", "ring_off_by_one", "dx_zeroed_only", "smooth_border_at_tile_edge")),
                               ("seams", ("ring_at_tile_edge", "smooth_border_at_tile_edge")),
                               ("smooth", ("smooth_rounded", "smooth_packed")),
                               ("values", ("gm_half_sum", "gm_min"))):
            for wrong in wrongs:
                if ud.applies(wrong, func, shrink, smooth) and cell_key((func, shrink, smooth)) not in ZERO_CELLS.get(wrong, ()):
                    assert n_wrong(func, shrink, smooth, wrong, (design,)) > 0, (design, wrong, func, shrink, smooth)


# ------------------------------------------------------------------------------ findings
def test_diagonal_differences_are_even_and_the_clamp_never_acts():
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    ky = kx.T
    for k in (kx - ky, kx + ky):
        assert (k % 2 == 0).all() and k[k > 0].sum() == 6 and k.sum() == 0          # 2 x (three pixels - three pixels): <= 1530
    assert (kx - ky).tolist() == [[0, 2, 2], [-2, 0, 2], [-2, -2, 0]]
    assert 255 * kx[kx > 0].sum() == 1020 and 1020 >> 2 == 255 and 1530 >> 3 == 191 and 4 * 191 == 764
    top = np.zeros(4, np.int64)
    for shrink in ud.SHRINKS:
        for name, index, l, px in all_levels(shrink):
            dx, dy = orc._sobel_int(px)
            assert ((dx - dy) % 2 == 0).all() and ((dx + dy) % 2 == 0).all()
            assert np.array_equal(np.trunc(0.5 * dx - 0.5 * dy), np.sign(dx - dy) * (np.abs(dx - dy) // 2))
            top = np.maximum(top, ud.channel_values(dx, dy, "grad_hist_4_u1").max(axis=(0, 1)))
    assert top.tolist() == [255, 191, 255, 191]                # attained, and never above: the clamp is dead code
    rng = np.random.default_rng(0)
    s = ud.centre_sums(np.where(rng.random((400000, 4, 4)) < 0.3, rng.integers(0, 256, (400000, 4, 4)), 255 * rng.integers(0, 2, (400000, 4, 4))))
    assert s[:, 1].max() <= ud.WRAP_MAX_13 and s[:, 3].max() <= ud.WRAP_MAX_13 <= 764


def test_second_pooling_stage_never_wraps():
    top = 0
    for func in FUNCS:
        for name, index, l, px in all_levels(4):
            first = ud.pool2(ud.intermediates(px, func, 4)["ch"])
            assert first.max() <= 63
            top = max(top, int(ud.block_sums(first).max()))
    assert 4 * 63 == 252 and 200 <= top <= 252                 # (and the designs come close to the bound)


def test_bottom_ring_is_the_last_pixel_of_its_block():
    """Level sides are multiples of the shrink; the ring row nh - 1 is the first pixel row of a tile only at shrink 1."""
    for shrink in ud.SHRINKS:
        g = ud.tile_geom("grad_hist_4_u1", shrink)
        first = []
        for name, index, l, px in all_levels(shrink):
            assert px.shape[0] % shrink == 0 and px.shape[1] % shrink == 0
            assert (px.shape[0] - 1) % shrink == shrink - 1
            first.append((px.shape[0] - 1) % (shrink * g["TU"]) == 0 or (px.shape[1] - 1) % (shrink * g["TV"]) == 0)
        assert any(first) == (shrink == 1)
        last = [(px.shape[0] % (shrink * g["TU"]) == 0, px.shape[1] % (shrink * g["TV"]) == 0) for _, _, _, px in all_levels(shrink)]
        assert any(a for a, _ in last) and any(b for _, b in last)


def test_min_is_right_on_pure_diagonals():
    img = ud.design_images("wrap", 2)[1]
    q = img.shape[0] // 4
    band = np.s_[2 * q + 2:3 * q - 2, 2:img.shape[1] - 10]
    dx, dy = ud.sobel_ring(img)
    same = (np.abs(dx) >> 2) == (np.abs(dy) >> 2)
    assert same[band].mean() > 0.9
    got, ref = ud.channel_values(dx, dy, "grad_mag_u1", "gm_min"), ud.channel_values(dx, dy, "grad_mag_u1")
    assert np.array_equal(got[same], ref[same]) and not np.array_equal(got, ref)


if __name__ == "__main__":
    print("PAIRS_REACHED, QUOTIENT_SIDES, QUOTIENT_SIDES_EVEN =", quotient_facts()[:3])
    print("WRAP_COUNTS =", wrap_facts())
    table = {w: {c: n_wrong(*c, w) for c in CELLS if ud.applies(w, *c)} for w in ud.WRONG_KERNELS}
    print("WRONG_COUNTS = {")
    for w, t in table.items():
        print(f"    {w!r}: {t},")
    print("}")
