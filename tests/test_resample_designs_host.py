"""The designed levels of resample_designs.py, proved on the host (no GPU): that the oracle's resize is the classifier's own
trunc(clip(t)) and, away from the decided pixels, the truncation of the exact value; that every design holds the decided
pixels it was built for, in staged tiles and -- at the ordinary rate -- in the tiles beyond the LDS budget; that a kernel deciding one of them the other way changes the bytes
of the channels; that the path designs reach every path their cell has; and that the classifier's staged / beyond-budget
split is the one the tile geometry implies.  Parametrised over the list the GPU module runs (resample_designs.CASES)."""
import functools

import numpy as np
import pytest

import resample_designs as rd
from oracle import wb_oracle as orc
from waldboost_amd.plan import PyramidPlan

N_SAMPLE = 300


@functools.lru_cache(None)
def _octaves(design, shrink, dtype, slot=1):
    if design == "ratio_levels":
        img, opts, _ = rd.ratio_levels(shrink, dtype)
    else:
        imgs, opts, _ = rd.plateaus(shrink, dtype)
        img = imgs[slot]
    return img, opts, rd.octaves_of(img)


def _levels(design, shrink, dtype, slot=1):
    img, opts, octs = _octaves(design, shrink, dtype, slot)
    plan = orc.level_plan(img.shape[0], img.shape[1], shrink, opts["n_per_oct"])
    return img, opts, octs, plan


@functools.lru_cache(None)
def _oracle_ties_to_exact(design, shrink, dtype):
    """Item 1, once per (design, shrink, dtype): the image and the levels do not depend on the function or the smooth."""
    img, opts, octs, plan = _levels(design, shrink, dtype)
    masks = rd.design_masks(design, shrink, dtype)
    assert len(masks) >= 2
    n_exact = 0
    for l, m in masks.items():
        lv = plan[l]
        base = octs[lv["oct"]]
        got = orc.resize_bilinear(base, lv["nh"], lv["nw"])
        assert got.dtype == img.dtype and np.array_equal(got.astype(np.int64), m["out"]), (design, shrink, dtype, l)
        if "trunc_exact" in m:
            away = ~rd.decided(m)
            clipped = np.clip(m["trunc_exact"], int(base.min()), int(base.max()))
            assert np.array_equal(m["out"][away], clipped[away]), (design, shrink, dtype, l)
            if base.min() >= 0:
                assert np.array_equal(m["trunc_exact"], m["floor_exact"])
            # |t - exact| stays far below the `near` band: four products and three sums of values below 2^9
            n_exact += int(away.sum())
    return n_exact


def _tiles_holding(mask, func, shrink, smooth, paths):
    """The set of paths of the tiles that compute the output pixels under the resized pixels of `mask`."""
    g = rd.tile_geom(func, shrink, smooth)
    ys, xs = np.nonzero(mask)
    ty = np.minimum(ys // shrink // g["TU"], paths.shape[0] - 1)
    tx = np.minimum(xs // shrink // g["TV"], paths.shape[1] - 1)
    return set(paths[ty, tx].tolist())


def _population(masks, kinds):
    """The designed pixels a wrong kernel can get wrong: (level, y, x, wrong value) of the pixels in one of `kinds` whose
    other side is another value (the clip holds both sides of a few)."""
    ls, ys, xs, wr = [], [], [], []
    for l, m in masks.items():
        sel = np.logical_or.reduce([m[k] for k in kinds]) & (m["wrong"] != m["out"])
        y, x = np.nonzero(sel)
        ls.append(np.full(y.size, l)); ys.append(y); xs.append(x); wr.append(m["wrong"][sel])
    return tuple(np.concatenate(a) for a in (ls, ys, xs, wr))


def _visible_estimate(masks, kinds, func, dtype, shrink, smooth):
    ls, ys, xs, wr = _population(masks, kinds)
    n = ls.size
    pick = np.random.default_rng(5).choice(n, min(n, N_SAMPLE), replace=False)
    seen = 0
    for l in np.unique(ls[pick]):
        p = pick[ls[pick] == l]
        resized = masks[l]["out"].astype(dtype)
        share, k = rd.visible_share(resized, ys[p], xs[p], wr[p], func, shrink, smooth, N_SAMPLE)
        seen += round(share * k)
    return n, seen / len(pick), n * seen / len(pick)


@pytest.mark.parametrize("case", rd.CASES, ids=rd.case_id)
def test_design_holds_what_it_was_built_for(case):
    design, func, dtype, shrink, smooth = case
    img, opts, octs, levels = _levels(design, shrink, dtype)
    assert max(img.shape) <= 400 and min(rd.level0_tiles(img.shape[0], img.shape[1], shrink)) >= 3
    if dtype == "float32":
        # float32 images ride along on the same pixels (the kernel's direct path, no truncation: nothing is designed for
        # them); what the oracle computes is the same t, rounded once and clipped
        u8, _, u8_octs, _ = _levels(design, shrink, "uint8")
        assert img.dtype == np.float32 and np.array_equal(img, u8)
        lv = levels[rd.ratio_level_indices(img.shape[0], img.shape[1], shrink, opts["n_per_oct"])[0]]
        base = octs[lv["oct"]]
        t = rd.level_t(base, lv["nh"], lv["nw"])
        assert np.array_equal(orc.resize_bilinear(base, lv["nh"], lv["nw"]), np.clip(t.astype(np.float32), base.min(), base.max()))
        return
    # 1. the oracle against the classifier's own t and against exact arithmetic
    n_exact = _oracle_ties_to_exact(design, shrink, dtype)
    masks = rd.design_masks(design, shrink, dtype)
    plan = rd.make_plan(img.shape[0], img.shape[1], func, shrink, opts["n_per_oct"], smooth)
    tiles = rd.classify_tiles(plan, func)
    strict = "downscale" if func == "grad_mag" else "staged"
    if design == "ratio_levels":
        assert n_exact > 10000
        # 2. coverage: counts of decided pixels, on at least two strict down-scale levels of small-fraction ratios ...
        assert set(masks) <= set(rd.ratio_level_indices(img.shape[0], img.shape[1], shrink, opts["n_per_oct"])) and len(masks) >= 2      # (octaves 0 .. 2)
        n_decided = sum(int((m["tie"] | m["near"]).sum()) for m in masks.values())
        n_landed = sum(int(m["landed"].sum()) for m in masks.values())
        n_near = sum(int(m["near"].sum()) for m in masks.values())
        n_rd = sum(int(m["rounding_decided"].sum()) for m in masks.values())
        assert n_decided >= 500 and n_rd >= 100 and n_near >= 100, (n_decided, n_rd, n_near, n_landed)
        if dtype == "int16":
            assert sum(int((m["near"] & (m["t"] < 0)).sum()) for m in masks.values()) >= 30      # both sides of zero
            assert sum(int((m["near"] & (m["t"] > 0)).sum()) for m in masks.values()) >= 30
        # ... in tiles of the strict down-scale path.  A tile of an identity level cannot hold a decided pixel (weights 1 and
        # 0: t is the pixel itself, whatever the order, and lies in the octave's range), so the second path with decided
        # pixels is the one beyond the LDS budget, in the cells that have it: item 2b below
        held = set()
        for l, m in masks.items():
            held |= _tiles_holding(rd.decided(m), func, shrink, smooth, tiles[l])
        assert strict in held
        assert levels[0]["nh"] == img.shape[0] and levels[0]["nw"] == img.shape[1]
        assert np.array_equal(rd.level_t(img, img.shape[0], img.shape[1]), img.astype(np.float64))
        kinds = ("tie", "near", "landed")
    else:
        # 2. coverage, for both images of the batch: pixels the clip decides, in at least two octaves, and pixels on the
        # plateaus at interior values where nothing rescues the truncation
        both = rd.plateaus(shrink, dtype)[0]                  # (each image's range is wrong for the other at both ends)
        assert both[0].min() < both[1].min() and both[0].max() < both[1].max()
        for slot in (0, 1):
            sm = rd.design_masks(design, shrink, dtype, slot)
            per_oct = {}
            for m in sm.values():
                per_oct[m["oct"]] = per_oct.get(m["oct"], 0) + int(m["clip_decided"].sum())
            assert sum(per_oct.values()) >= 200 and sum(v >= 20 for v in per_oct.values()) >= 2, per_oct
            off = 300 if dtype == "int16" else 0
            lost = 0
            for v in np.array(_interior_values(slot), np.int64) - off:
                for m in sm.values():
                    on = np.abs(m["t"] - v) < rd.NEAR                      # (a flat 2 x 2 source patch of value v)
                    short = on & (np.trunc(m["t"]) != v)
                    assert not (short & m["clip_decided"]).any()
                    lost += int(short.sum())
            assert lost >= 200, lost
            # the live bound: the minimum for uint8, the maximum for the all-negative int16 form
            bound = _octaves(design, shrink, dtype, slot)[0].max() if dtype == "int16" else _octaves(design, shrink, dtype, slot)[0].min()
            for m in sm.values():
                assert (m["out"][m["clip_decided"]] == bound).all()
        assert strict in {p for l in masks for p in _tiles_holding(masks[l]["clip_decided"], func, shrink, smooth, tiles[l])}
        kinds = ("clip_decided",)
    # 2b. the tiles beyond the LDS budget (direct loads, the fast path and the redo on them) lie on the levels of the largest
    # zoom, none of which is a ratio level: over every level of octaves 0 .. 2 they must hold at least a hundred pixels of
    # the design's own class -- `near` (fp64 masks) or clip_decided -- in every cell whose plan has such tiles
    # (uint8 images only: the other dtypes stage no patch and take direct loads in every tile)
    if dtype != "uint8":
        pass
    elif "direct_budget" in rd.paths_of(func) and any(p is not None and (p == "direct_budget").any() for p in tiles):
        every = rd.all_level_masks(design, shrink, dtype)
        n_direct = rd.count_in_path(every, "near" if design == "ratio_levels" else "clip_decided", "direct_budget", func, shrink, smooth, tiles)
        assert shrink == 2 and n_direct >= 100, n_direct
    else:
        assert shrink != 2 or func == "grad_mag"
    # 3. visibility: the resized image is never written out, so a decided pixel must show in the channels
    n, share, est = _visible_estimate(masks, kinds, func, dtype, shrink, smooth)
    assert est >= 100, (n, share, est)


def _interior_values(slot):
    return rd.PLATEAU_VALUES["interior"] if slot == 1 else (rd.PLATEAU_VALUES["min"], rd.PLATEAU_VALUES["interior"][0])


@pytest.mark.parametrize("shrink", rd.SHRINKS)
def test_ratio_shapes_meet_their_criteria(shrink):
    """The shapes were chosen by hand (resample_designs.RATIO_SHAPES); what they were chosen for is checked here."""
    assert rd.ratio_shape_ok(*rd.RATIO_SHAPES[shrink][:2], shrink, rd.RATIO_SHAPES[shrink][2])
    assert not rd.ratio_shape_ok(75, 150, shrink, 2)                    # (a shape of the suite's other tests does not)


@pytest.mark.parametrize("shrink", rd.SHRINKS)
@pytest.mark.parametrize("dtype", ["uint8", "int16"])
def test_a_kernel_without_the_clip_or_with_another_order_is_caught(shrink, dtype, monkeypatch):
    """The designs bite: the oracle's own resize with its clip replaced by a no-op differs from the unmodified one in at
    least the counted clip_decided pixels, and the same four terms summed in another association move at least a hundred
    of the decided pixels of the ratio levels to the other side."""
    class NoClip:                                   # numpy as the oracle sees it, but for np.clip
        clip = staticmethod(lambda a, lo, hi: a)

        def __getattr__(self, name):
            return getattr(np, name)
    for slot in (0, 1):
        img, opts, octs, levels = _levels("plateaus", shrink, dtype, slot)
        masks = rd.design_masks("plateaus", shrink, dtype, slot)
        want = {l: orc.resize_bilinear(octs[levels[l]["oct"]], levels[l]["nh"], levels[l]["nw"]) for l in masks}
        with monkeypatch.context() as mp:
            mp.setattr(orc, "np", NoClip())
            bare = {l: orc.resize_bilinear(octs[levels[l]["oct"]], levels[l]["nh"], levels[l]["nw"]) for l in masks}
        n_diff = sum(int((bare[l] != want[l]).sum()) for l in masks)
        n_clip = sum(int(m["clip_decided"].sum()) for m in masks.values())
        assert n_diff >= n_clip >= 200, (n_diff, n_clip)
        assert all(np.array_equal(bare[l] != want[l], masks[l]["clip_decided"]) for l in masks)
    img, opts, octs, levels = _levels("ratio_levels", shrink, dtype)
    moved = outside = 0
    for l, m in rd.design_masks("ratio_levels", shrink, dtype).items():
        base = octs[levels[l]["oct"]]
        other = np.trunc(np.clip(rd.level_t_other_order(base, levels[l]["nh"], levels[l]["nw"]), base.min(), base.max())).astype(np.int64)
        diff = other != m["out"]
        moved += int((diff & rd.decided(m)).sum())
        outside += int((diff & ~rd.decided(m)).sum())
        assert np.array_equal(other[diff], m["wrong"][diff])
    assert moved >= 100 and outside == 0, (moved, outside)


# ------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("cell", rd.PATH_CELLS, ids=rd.case_id)
def test_path_designs_reach_every_path_of_their_cell(cell):
    func, shrink, smooth = cell
    shapes, impossible = rd.path_levels(func, shrink, smooth)
    found = set()
    for H, W, npo in shapes:
        n = rd.path_counts(rd.make_plan(H, W, func, shrink, npo, smooth), func)
        found |= {p for p, k in n.items() if k}
    assert found | impossible == set(rd.paths_of(func)) and not found & impossible, (found, impossible)
    # ... and the impossible ones stay away over a sweep of other shapes and octave lengths
    for H, W, npo in [(64, 97, 3), (99, 131, 5), (131, 97, 8), (150, 211, 12), (203, 277, 16), (58, 260, 7)]:
        n = rd.path_counts(rd.make_plan(H, W, func, shrink, npo, smooth), func)
        assert not any(n[p] for p in impossible), (H, W, npo, n)


def _patch_budget(g):
    """TileGeom::PROWS / PPITCH (csrc/wb_chan_tile.h), restated: the rows and the bytes per row of the staged source patch.
    A change of the LDS budget there has to be made here too:
      PROWS  = S == 2 ? (TU == 16 ? 74 : 2 * RH - 8) : 2 * RH + 4
      PPITCH = S == 4 ? 2 * RW + 12 : (S == 2 && TU != 16) ? 256 : ((SU * SV * 16) / PROWS) & ~3"""
    S, su, sv = g["S"], g["TU"] + 2 * g["HS"], g["TV"] + 2 * g["HS"]
    prows = (74 if g["TU"] == 16 else 2 * g["RH"] - 8) if S == 2 else 2 * g["RH"] + 4
    ppitch = 2 * g["RW"] + 12 if S == 4 else 256 if (S == 2 and g["TU"] != 16) else ((su * sv * 16) // prows) & ~3
    return prows, ppitch


@pytest.mark.parametrize("cell", [c for c in rd.PATH_CELLS if c[0] != "grad_mag"], ids=rd.case_id)
def test_staged_and_beyond_budget_split_is_the_geometry(cell):
    """The classifier reads the split from the library's patch table; the taps of the tile's pixels (the geometry of
    test_tile_patch_table_covers_every_tap_of_its_tile) and the LDS budget must give the same answer for every tile."""
    func, shrink, smooth = cell
    g = rd.tile_geom(func, shrink, smooth)
    prows, ppitch = _patch_budget(g)
    n = dict(staged=0, direct_budget=0)
    for H, W, npo in rd.path_levels(func, shrink, smooth)[0]:
        plan = rd.make_plan(H, W, func, shrink, npo, smooth)
        for l, paths in enumerate(rd.classify_tiles(plan, func)):
            lv = plan.levels[l]
            if paths is None or not (lv["h"] > lv["nh"] and lv["w"] > lv["nw"]):
                continue
            ty_taps, tx_taps = PyramidPlan.axis_taps(lv["h"], lv["nh"]), PyramidPlan.axis_taps(lv["w"], lv["nw"])
            for ty in range(paths.shape[0]):
                for tx in range(paths.shape[1]):
                    u0, v0 = ty * g["TU"], tx * g["TV"]
                    vrows = min(lv["u"] - u0, g["TU"]) if func == "grad_hist" else g["TU"]      # (channels_kernel trims the rows)
                    ry0, rx0 = shrink * (u0 - g["HS"]) - 1, shrink * (v0 - g["HS"]) - 1
                    rh = shrink * (vrows + 2 * g["HS"]) + 2
                    ys = np.clip(np.arange(ry0, ry0 + rh), 0, lv["nh"] - 1)
                    xs = np.clip(np.arange(rx0, rx0 + g["RW"]), 0, lv["nw"] - 1)
                    nrow = int(ty_taps["i1"][ys].max() - ty_taps["i0"][ys].min()) + 1
                    nbyte = int(tx_taps["i1"][xs].max() - tx_taps["i0"][xs].min()) + 1
                    want = "staged" if nrow + 1 <= prows and nbyte + 8 <= ppitch else "direct_budget"
                    assert paths[ty, tx] == want, (H, W, npo, l, ty, tx, nrow, nbyte, prows, ppitch)
                    n[want] += 1
    assert n["staged"] > 0 and (n["direct_budget"] > 0) == (shrink == 2), n


def test_mismatch_message_names_level_pixel_tile_path_and_design():
    """The GPU module's failure message, on a mismatch planted under a decided pixel of a ratio level."""
    func, shrink, smooth = "grad_hist_4_u1", 2, 1
    img, opts, octs, levels = _levels("ratio_levels", shrink, "uint8")
    masks = rd.design_masks("ratio_levels", shrink, "uint8")
    l = max(masks, key=lambda k: int(masks[k]["rounding_decided"].sum()))
    y, x = (int(v) for v in np.argwhere(masks[l]["rounding_decided"])[0])
    ref = rd.chain(masks[l]["out"].astype(np.uint8), func, shrink, smooth)
    got = ref.copy()
    got[y // shrink, x // shrink, 0] ^= 1
    plan = rd.make_plan(img.shape[0], img.shape[1], func, shrink, opts["n_per_oct"], smooth)
    msg = rd.describe_mismatch(got, ref, l, func, shrink, smooth, plan, masks)
    ty, tx = rd.tile_of(func, shrink, smooth, y // shrink, x // shrink)
    assert f"level {l}: 1 output pixels differ, first at ({y // shrink}, {x // shrink})" in msg and f"tile ({ty}, {tx}) path staged" in msg
    assert "rounding_decided" in msg
    assert "not a designed level" in rd.describe_mismatch(got, ref, l, func, shrink, smooth, plan, {})
