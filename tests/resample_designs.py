"""Designed levels for step 1 of the channel tile kernels (NumPy and the library's host-only entry points: no GPU, no torch).

Step 1 (resample_tile, csrc/wb_chan_tile.h) resizes a tile bilinearly and casts it back to the image dtype.  For uint8
images -- and for integer images held as float64 -- a resized pixel is trunc(clip(t)), t the oracle's fp64 four-term sum.
A kernel with the right taps is wrong only where t lies so close to an integer that the order of the fp64 operations, or
the clip to the octave's (min, max), decides the truncation.  On noise at an ordinary level that is one pixel in five
hundred, and the clip never decides where the octave's minimum is 0 (0 * w is exact).  Here the test decides: it picks
levels and pixels on which those cases are many, counts them (test_resample_designs_host.py, no GPU), and
test_gpu_resample_designs.py runs them through every cell of the kernels' dispatch table.

What is provided
  classify_tiles    the path every tile of every level of a plan takes through step 1 (PATHS / GM_PATHS), from the level
                    geometry, the tile shape the library reports (wb_channels_tile) and its own per-tile patch table
                    (wb_channels_tile_patches: rows == 0 on a strict down-scale = the direct loads beyond the LDS budget).
  classify_pixels   per level: the oracle's t, the same sum in exact integer arithmetic on the fp64 weights (every fp64
                    weight is m * 2^-k: Python integers at a common power of two per axis), and the masks
                      tie               the exact value is an integer
                      rounding_decided  ... and trunc(t) differs from it (t came out on the other side)
                      near              0 < |t - rint(t)| < 1e-9
                      landed            t is an integer and the exact value is not (fp64 rounding put t ON the integer: the
                                        class the three above leave out -- a third of the decided pixels of a 3/4 level)
                      clip_decided      trunc(t) != trunc(clip(t, min, max)) for the level's own octave
                    with, per pixel, the `wrong` neighbour value a kernel would write that decided the other way.
  ratio_levels      noise from the upper half of the byte range on a shape whose plan holds strict down-scale levels
                    with nh/h and nw/w fractions of denominator <= 8 (RATIO_SHAPES: chosen by hand, held to
                    ratio_shape_ok by the host test).  The lower half of the image is the same noise in 2 x 2, 4 x 4 and 8 x 8 blocks:
                    `rounding_decided` asks for an exact integer, which needs a flat 2 x 2 source patch -- on pixel noise
                    of 128 values one patch in two million -- so the flat patches of the blocks carry that class at
                    octaves 0, 1 and 2, and the pixel noise carries `near`.
  plateaus          noise of [40, 62] (2x2 pooling never wraps, every octave keeps the structure) with flat rectangles
                    and bars at the octave minimum (37; 12 in the second image of the batch), at interior values (50,
                    58) and at the maximum (63; 60 in the second image, whose noise ends at 59); int16: the image minus
                    300, all negative, where truncation toward zero makes the MAXIMUM the live bound (-237 and -240).
  path_levels       per (function, shrink, smooth) cell, shapes whose tiles take every path that exists for the cell,
                    and the paths that cannot occur there.

Findings (host arithmetic, asserted by the host test).
  * `upscale` cannot occur in a PyramidPlan in any cell: nh = int(h * s / shrink) * shrink <= h for s <= 1.  The kernel
    keeps the branch for level tables handed in through the C ABI.
  * `direct_budget` occurs at shrink 2 only, with AND without smooth: a 16 x 64 tile's patch rows are 256 bytes wide
    with smooth (134 resized columns: a zoom above 1.83) but 220 bytes wide without (130 columns: a zoom above 1.61), so
    n_per_oct >= 4 already reaches it at smooth 0, while smooth 1 needs the last level of an octave of >= 8.  At shrink 1
    and 4 the patch holds any zoom below 2.
  * `mixed_axis` cannot occur at shrink 1 (level 0 is the identity on both axes, every other level a strict down-scale
    on both); at shrink 2 and 4 it is level 0 of an octave with exactly one side a multiple of the shrink.
  * grad_mag takes no patch table (its kernel computes the extents): its strict down-scales are one class, `downscale`.
  * Paths reached by the designs, per cell (tiles; ratio shape + path shapes): every function at shrink 1: ident_inner,
    ident_edge, staged (grad_mag: downscale); at shrink 2: those, mixed_axis and -- not grad_mag -- direct_budget (16
    tiles of the 288 x 384 / 12 plan at smooth 0, 5 at smooth 1; 9 and 3 of 150 x 300 / 12); at shrink 4: ident_inner,
    ident_edge, staged / downscale, mixed_axis (76 x 150).

Counts the host test measures (octaves 0 .. 2 of every design; uint8 / int16)
  ratio_levels   shrink 1, 280 x 392 / 9 per octave, levels 2, 11, 20 (ratio 6/7): tie | near 26666 / 26738,
                   rounding_decided 254 / 198, near 2571 / 2551, landed 59 / 11
                 shrink 2, 288 x 384 / 12, levels 7, 8, 15, 19, 20, 27, 31 (2/3, 5/8, 5/6): tie | near 42399 / 42378,
                   rounding_decided 237 / 316, near 1990 / 1991, landed 62 / 29
                 shrink 4, 384 x 384 / 12, 13 levels (5/6, 2/3, 5/8, 7/8, 3/4, ...): tie | near 99281 / 99383,
                   rounding_decided 682 / 877, near 6541 / 6757, landed 241 / 91
                 summed in another association (level_t_other_order) at least 100 of them change sides, and no other pixel
  plateaus       clip_decided in octaves 0, 1, 2 -- uint8, slot 0 (minimum 12): 2901 381 44 / 2806 374 68 / 4173 598 73
                 at shrink 1 / 2 / 4; slot 1 (minimum 37): 2615 427 89 / 2559 466 88 / 4080 463 103; int16, slot 0 (maximum
                 -240): 441 102 32 / 401 139 46 / 574 166 27; slot 1 (maximum -237): 1505 346 68 / 1956 430 102 / 2981 666
                 141.  Pixels of the interior plateaus that come out one off with no clip to restore them: 1452 .. 4191 per
                 image.
  beyond budget  The ratio levels' decided pixels all lie in staged tiles (grad_mag: downscale): the tiles beyond the LDS
                 budget sit on the levels of the largest zoom (levels 9 .. 11 of an octave of 12 without smooth, level 11
                 with it), none of them a ratio level, and a tile of an identity level cannot hold a decided pixel (t is
                 the pixel).  Over every level of octaves 0 .. 2 the shrink-2 uint8 designs hold, inside direct_budget
                 tiles: ratio_levels 949 (smooth 0) / 186 (smooth 1) `near` pixels, plateaus 342 / 131 clip_decided ones
                 -- the same for the three functions with a patch table; the host test asks for 100.
  visibility     share of a sample of 300 decided pixels whose flip changes the channel bytes, x population = estimate
                 grad_hist, grad_mag (any dtype): every flip visible at every shrink and smooth (estimate = population:
                   ratio_levels 26512 .. 98965, plateaus 1919 .. 4646)
                 grad_hist_4_u1   ratio_levels 88 / 87 % (shrink 1, smooth 0 / 1), 72 / 58 % (2), 33 / 22 % (4): >= 22090
                                  plateaus     61 / 59 %, 40 / 31 %, 14 / 8 %: >= 387
                 grad_mag_u1      ratio_levels 80 / 69 %, 37 / 23 %, 12 / 6 %: >= 5934
                                  plateaus     53 / 44 %, 22 / 15 %, 4.7 / 3.0 %: >= 139 (shrink 4 with smooth; 188 over a
                                  sample of 2000) -- an integer channel shows a flipped pixel only beside a gradient, which
                                  is why the plateaus are mostly narrow bars
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

from oracle import wb_oracle as orc
from waldboost_amd import _native as nat
from waldboost_amd.plan import PyramidPlan

FUNC_IDS = {"grad_hist": nat.WB_CHN_GRAD_HIST, "grad_hist_4_u1": nat.WB_CHN_GRAD_HIST_4_U1,
            "grad_mag_u1": nat.WB_CHN_GRAD_MAG_U1, "grad_mag": nat.WB_CHN_GRAD_MAG}
PATHS = ("ident_inner", "ident_edge", "staged", "direct_budget", "mixed_axis", "upscale")
GM_PATHS = ("ident_inner", "ident_edge", "downscale", "mixed_axis", "upscale")
NEAR = 1e-9

# the cells of test_every_cell_of_the_channel_dispatch_vs_oracle: function x image dtype, x shrink x smooth
CELL_INPUTS = [("grad_hist", "uint8"), ("grad_hist", "float32"), ("grad_hist", "int16"), ("grad_hist_4_u1", "uint8"),
               ("grad_mag_u1", "uint8"), ("grad_mag", "uint8"), ("grad_mag", "float32")]
SHRINKS = (1, 2, 4)
SMOOTHS = (0, 1)
# the ONE list both test modules are parametrised over: (design, function, image dtype, shrink, smooth)
CASES = [(d, fn, dt, sh, sm) for d in ("ratio_levels", "plateaus") for fn, dt in CELL_INPUTS for sh in SHRINKS for sm in SMOOTHS]
PATH_CELLS = [(fn, sh, sm) for fn in FUNC_IDS for sh in SHRINKS for sm in SMOOTHS]


def case_id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------ tiles
def paths_of(func):
    return GM_PATHS if func == "grad_mag" else PATHS


@functools.lru_cache(None)
def tile_geom(func, shrink, smooth):
    """The resized tile of a cell: output tile (TU, TV) as the library reports it, smooth halo HS, grad_mag's triangle halo
    NH (GmGeom::NH), and RH x RW = S * (T + 2 HS) + 2 NH + 2 (TileGeom / GmTile)."""
    tu, tv = C.c_int(), C.c_int()
    assert nat.load().wb_channels_tile(FUNC_IDS[func], shrink, C.byref(tu), C.byref(tv)) == 0
    hs, nh = (1 if smooth else 0), (5 if func == "grad_mag" else 0)
    return dict(S=shrink, TU=tu.value, TV=tv.value, HS=hs, NH=nh, RH=shrink * (tu.value + 2 * hs) + 2 * nh + 2,
                RW=shrink * (tv.value + 2 * hs) + 2 * nh + 2)


def make_plan(H, W, func, shrink, n_per_oct, smooth):
    return PyramidPlan(H, W, shrink, n_per_oct, smooth, chan_func=FUNC_IDS[func])


def natural_tiles(plan, g):
    """(level, ty, tx) of every tile, level by level, row-major."""
    parts = []
    for l, lv in enumerate(plan.levels):
        ny, nx = -(-lv["u"] // g["TU"]), -(-lv["v"] // g["TV"])
        if ny <= 0 or nx <= 0:
            continue
        a = np.zeros(ny * nx, nat.TILE_DTYPE)
        a["level"] = l
        a["ty"], a["tx"] = np.divmod(np.arange(ny * nx), nx)
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, nat.TILE_DTYPE)


def patch_table(plan, func, tiles):
    """The library's WbTilePatch per tile (wb_channels_tile_patches; grad_mag has none: None)."""
    if func == "grad_mag" or not tiles.size:
        return None
    table, _ = plan.level_table()
    out = np.zeros(tiles.size, nat.PATCH_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    tiles = np.ascontiguousarray(tiles)
    rc = nat.load().wb_channels_tile_patches(FUNC_IDS[func], plan.shrink, plan.smooth, vp(table), plan.n_levels, vp(tiles), tiles.size, vp(out))
    assert rc == 0, nat.load().wb_last_error()
    return out


def classify_tiles(plan, func):
    """Per level of the plan a [ny, nx] object array: the path of every tile through step 1 (None for a level without tiles)."""
    g = tile_geom(func, plan.shrink, plan.smooth)
    tiles = natural_tiles(plan, g)
    patches = patch_table(plan, func, tiles)
    out = [None] * plan.n_levels
    S, RH, RW = g["S"], g["RH"], g["RW"]
    for i, t in enumerate(tiles):
        l = int(t["level"])
        lv = plan.levels[l]
        if out[l] is None:
            out[l] = np.empty((-(-lv["u"] // g["TU"]), -(-lv["v"] // g["TV"])), object)
        ry0 = S * (int(t["ty"]) * g["TU"] - g["HS"]) - g["NH"] - 1
        rx0 = S * (int(t["tx"]) * g["TV"] - g["HS"]) - g["NH"] - 1
        idy, idx = lv["h"] == lv["nh"], lv["w"] == lv["nw"]
        if idy and idx:
            # the kernel's own condition for the dword copy (resample_tile: `ident && ry0 >= 0 && ...`)
            inner = ry0 >= 0 and ry0 + RH <= lv["nh"] and rx0 >= 0 and rx0 + 4 * (-(-RW // 4)) <= lv["nw"]
            path = "ident_inner" if inner else "ident_edge"
        elif lv["h"] > lv["nh"] and lv["w"] > lv["nw"]:
            path = "downscale" if patches is None else ("staged" if patches[i]["rows"] else "direct_budget")
        elif lv["h"] < lv["nh"] or lv["w"] < lv["nw"]:
            path = "upscale"
        else:
            path = "mixed_axis"
        if patches is not None and path not in ("staged", "direct_budget"):
            assert patches[i]["rows"] == 0 and patches[i]["bytes"] == 0      # (only a strict down-scale stages a patch)
        out[l][int(t["ty"]), int(t["tx"])] = path
    return out


def path_counts(plan, func):
    n = dict.fromkeys(paths_of(func), 0)
    for m in classify_tiles(plan, func):
        if m is not None:
            for p in m.ravel():
                n[p] += 1
    return n


def tile_of(func, shrink, smooth, r, c):
    """(ty, tx) of the tile that computes output pixel (r, c) of a level."""
    g = tile_geom(func, shrink, smooth)
    return r // g["TU"], c // g["TV"]


# ------------------------------------------------------------------------------ pixels
def _pow2_ints(w):
    """fp64 weights -> (object array of Python integers a, k) with w == a / 2**k exactly."""
    fr = [Fraction(float(x)) for x in w]
    k = max(f.denominator.bit_length() - 1 for f in fr)
    return np.array([f.numerator * ((1 << k) // f.denominator) for f in fr], object), k


def level_t(base, nh, nw):
    """The oracle's fp64 t of a level: its taps, its four-term sum (resize_bilinear before clip and cast)."""
    r0, r1, wr0, wr1 = orc._axis_taps(base.shape[0], nh)
    c0, c1, wc0, wc1 = orc._axis_taps(base.shape[1], nw)
    v = base.astype(np.float64)
    wr0 = wr0[:, None]; wr1 = wr1[:, None]
    wc0 = wc0[None, :]; wc1 = wc1[None, :]
    t = (v[r0][:, c0] * wr0) * wc0
    t = t + (v[r0][:, c1] * wr0) * wc1
    t = t + (v[r1][:, c0] * wr1) * wc0
    t = t + (v[r1][:, c1] * wr1) * wc1
    return t


def level_t_other_order(base, nh, nw):
    """The same four terms in another association: columns first inside each product, the sum from the last term to the
    first -- what a kernel that did not keep scipy's order would compute (the host test's check that the designs bite)."""
    r0, r1, wr0, wr1 = orc._axis_taps(base.shape[0], nh)
    c0, c1, wc0, wc1 = orc._axis_taps(base.shape[1], nw)
    v = base.astype(np.float64)
    wr0 = wr0[:, None]; wr1 = wr1[:, None]
    wc0 = wc0[None, :]; wc1 = wc1[None, :]
    a = v[r0][:, c0] * (wr0 * wc0)
    b = v[r0][:, c1] * (wr0 * wc1)
    c = v[r1][:, c0] * (wr1 * wc0)
    d = v[r1][:, c1] * (wr1 * wc1)
    return a + (b + (c + d))


def level_exact(base, nh, nw):
    """The four-term sum in exact arithmetic: (N, k), object array of Python integers with value N / 2**k."""
    r0, r1, wr0, wr1 = orc._axis_taps(base.shape[0], nh)
    c0, c1, wc0, wc1 = orc._axis_taps(base.shape[1], nw)
    ar, kr = _pow2_ints(np.concatenate([wr0, wr1]))
    ac, kc = _pow2_ints(np.concatenate([wc0, wc1]))
    ar0, ar1, ac0, ac1 = ar[:nh, None], ar[nh:, None], ac[None, :nw], ac[None, nw:]
    v = base.astype(np.int64).astype(object)
    n = v[r0][:, c0] * ar0 * ac0 + v[r0][:, c1] * ar0 * ac1 + v[r1][:, c0] * ar1 * ac0 + v[r1][:, c1] * ar1 * ac1
    return n, kr + kc


def _trunc_i(t):
    return np.trunc(t).astype(np.int64)


def classify_pixels(base, nh, nw, exact=True):
    """The designed-pixel masks of one level resized from the octave image `base` (uint8 or an integer dtype), see the
    module docstring.  Returns a dict: t, out (= the oracle's pixel: trunc(clip(t))), tie, rounding_decided, near,
    landed, clip_decided, floor_exact (int64; exact=True only) and wrong (int64: the value on the side that rounding or the clip
    decided against; == out where nothing was decided)."""
    assert base.dtype.kind in "iu"
    t = level_t(base, nh, nw)
    mn, mx = np.float64(base.min()), np.float64(base.max())
    out = _trunc_i(np.clip(t, mn, mx))
    raw = _trunc_i(t)
    res = dict(t=t, out=out, clip_decided=raw != out)
    d = np.abs(t - np.rint(t))
    res["near"] = (d > 0) & (d < NEAR)
    if exact:
        n, k = level_exact(base, nh, nw)
        tie = np.asarray((n & ((1 << k) - 1)) == 0, bool)
        fl = (n >> k).astype(np.int64)
        res["tie"] = tie
        res["floor_exact"] = fl
        res["trunc_exact"] = np.where((fl < 0) & ~tie, fl + 1, fl)
        res["rounding_decided"] = res["tie"] & (raw != fl)
        res["landed"] = (d == 0) & ~tie
    else:
        res["tie"] = np.zeros(t.shape, bool)
        res["rounding_decided"] = np.zeros(t.shape, bool)
        res["landed"] = np.zeros(t.shape, bool)
    # the wrong neighbour: where the clip decided, the unclipped truncation; where the integer n = rint(t) is (almost)
    # hit, the truncation from n's other side, clipped like the oracle's -- equal to `out` when the clip holds both sides
    n_int = np.rint(t)
    below = _trunc_i(np.clip(n_int - 0.5, mn, mx))
    above = _trunc_i(np.clip(n_int + 0.5, mn, mx))
    other = np.where(below != out, below, above)
    res["wrong"] = np.where(res["clip_decided"], raw, np.where(decided(res), other, out))
    return res


def decided(m):
    """The pixels of a level whose truncation the order of the fp64 operations decides."""
    return m["tie"] | m["near"] | m["landed"]


def octaves_of(image):
    return list(orc.image_octaves(image))


def designed_levels(image, shrink, n_per_oct, which="all", max_oct=3):
    """classify_pixels of the levels of a design: which = "ratio" (strict down-scales whose two ratios have a denominator
    <= 8: exact arithmetic), or "all" levels of the first max_oct octaves (fp64 masks only).  {level index: masks}."""
    H, W = image.shape
    octs = octaves_of(image)
    out = {}
    for l, lv in enumerate(orc.level_plan(H, W, shrink, n_per_oct)):
        if lv["nh"] < 1 or lv["nw"] < 1 or lv["oct"] >= max_oct:
            continue
        if which == "ratio" and not is_ratio_level(lv):
            continue
        out[l] = classify_pixels(octs[lv["oct"]], lv["nh"], lv["nw"], exact=which == "ratio")
        out[l]["oct"] = lv["oct"]
    return out


def is_ratio_level(lv, max_den=8):
    return (lv["nh"] < lv["h"] and lv["nw"] < lv["w"] and lv["nh"] > 0 and lv["nw"] > 0
            and Fraction(lv["nh"], lv["h"]).denominator <= max_den and Fraction(lv["nw"], lv["w"]).denominator <= max_den)


# ------------------------------------------------------------------------------ the channels a resized pixel reaches
def chain(resized, func, shrink, smooth):
    """The oracle's own chain behind the resize: channel function, pools, smooth (channel_pyramid's loop body)."""
    chns = orc.CHANNEL_FUNCS[func](resized)
    if shrink >= 2:
        chns = orc.avg_pool_2(chns)
    if shrink == 4:
        chns = orc.avg_pool_2(chns)
    if smooth == 1:
        chns = orc.smooth_image_3d(chns)
    return np.ascontiguousarray(np.atleast_3d(chns))


CROP = 24        # >= the reach of one resized pixel into the output and back: 4 (smooth at shrink 4) + 3 (pools) + 6 + 6 (grad_mag)


def visible_share(resized, ys, xs, wrong, func, shrink, smooth, n_sample, seed=0):
    """Of a sample of at most n_sample designed pixels (ys, xs), the share whose replacement by `wrong` changes the bytes
    of the channels.  Each flip is pushed through `chain` on a crop of the level around it: the crop starts on a multiple of
    4 (the pools keep their phase), reaches CROP pixels or the level's own border, and any difference lies in outputs
    whose whole input is inside the crop.  Returns (share, sampled)."""
    n = len(ys)
    if n == 0:
        return 0.0, 0
    pick = np.arange(n) if n <= n_sample else np.random.default_rng(seed).choice(n, n_sample, replace=False)
    seen = 0
    for i in pick:
        y, x = int(ys[i]), int(xs[i])
        y0, x0 = max(0, (y - CROP) & ~3), max(0, (x - CROP) & ~3)
        crop = resized[y0:y + CROP + 1, x0:x + CROP + 1]
        flip = crop.copy()
        flip[y - y0, x - x0] = wrong[i]
        a, b = chain(crop, func, shrink, smooth), chain(flip, func, shrink, smooth)
        seen += not np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return seen / len(pick), len(pick)


# ------------------------------------------------------------------------------ design builders
# (H, W, n_per_oct) per shrink.  Chosen by hand from a listing of every shape up to 400 x 400 (steps of 4 * shrink) and
# n_per_oct 3 .. 12 that meets ratio_shape_ok, for the ratio levels with the most pixels whose zoom is NOT a dyadic
# fraction (6/7, 5/8, 5/6: inexact fp64 weights; a 2/3 or 4/5 level has exact weights and t is never off its exact value)
# and for an octave-0 level among them.  The host test holds them to ratio_shape_ok; nothing searches at test time.
RATIO_SHAPES = {1: (280, 392, 9), 2: (288, 384, 12), 4: (384, 384, 12)}


def ratio_level_indices(H, W, shrink, n_per_oct):
    """Levels that qualify: strict down-scale, both ratios of denominator <= 8, more than one tile in every cell."""
    out = []
    for l, lv in enumerate(orc.level_plan(H, W, shrink, n_per_oct)):
        if not is_ratio_level(lv):
            continue
        u, v = lv["nh"] // shrink, lv["nw"] // shrink
        if all(-(-u // tile_geom(fn, shrink, 0)["TU"]) * -(-v // tile_geom(fn, shrink, 0)["TV"]) > 1 for fn in FUNC_IDS):
            out.append(l)
    return out


def level0_tiles(H, W, shrink):
    """The smallest tile grid level 0 has over the functions: (rows of tiles, columns of tiles)."""
    lv = orc.level_plan(H, W, shrink, 1)[0]
    u, v = lv["nh"] // shrink, lv["nw"] // shrink
    return (min(-(-u // tile_geom(fn, shrink, 0)["TU"]) for fn in FUNC_IDS), min(-(-v // tile_geom(fn, shrink, 0)["TV"]) for fn in FUNC_IDS))


def ratio_shape_ok(H, W, shrink, n_per_oct):
    """What a ratio_levels shape has to offer: sides of at most 400, a level 0 of at least 3 x 3 tiles in every cell with a
    tile inside it (ident_inner) for every function and smooth, and at least two qualifying levels in octaves 0 .. 2, one
    of them with a zoom that is no dyadic fraction on either axis."""
    plan = orc.level_plan(H, W, shrink, n_per_oct)
    idx = [l for l in ratio_level_indices(H, W, shrink, n_per_oct) if plan[l]["oct"] < 3]
    dyadic = lambda n, d: (Fraction(d, n).denominator & (Fraction(d, n).denominator - 1)) == 0
    inexact = [l for l in idx if not dyadic(plan[l]["nh"], plan[l]["h"]) and not dyadic(plan[l]["nw"], plan[l]["w"])]
    inner = all(path_counts(make_plan(H, W, fn, shrink, n_per_oct, sm), fn)["ident_inner"] > 0 for fn in FUNC_IDS for sm in SMOOTHS)
    return max(H, W) <= 400 and min(level0_tiles(H, W, shrink)) >= 3 and inner and len(idx) >= 2 and len(inexact) >= 1


def _block_noise(rng, H, W, k, lo, hi):
    a = rng.integers(lo, hi, (-(-H // k), -(-W // k)), dtype=np.uint8)
    return np.kron(a, np.ones((k, k), np.uint8))[:H, :W]


def _as_dtype(img_u8, dtype, offset):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return img_u8
    if dtype == np.float32:
        return img_u8.astype(np.float32)
    assert dtype == np.int16
    return (img_u8.astype(np.int16) - offset).astype(np.int16)


def ratio_levels(shrink, dtype="uint8"):
    """(image, channel_opts without the function, notes): see the module docstring.  int16: the image minus 160, near-integer
    values on both sides of zero; float32: the same pixels as floats (the kernel's direct path, nothing designed)."""
    H, W, npo = RATIO_SHAPES[shrink]
    rng = np.random.default_rng(1000 + shrink)
    img = rng.integers(128, 256, (H, W), dtype=np.uint8)
    top = H // 2
    third = -(-W // 3)
    for j, k in enumerate((2, 4, 8)):                         # flat 2 x 2 source patches at octave 0, 1 and 2
        img[top:, j * third:(j + 1) * third] = _block_noise(rng, H - top, min(third, W - j * third), k, 128, 256)
    opts = dict(shrink=shrink, n_per_oct=npo, smooth=None)
    notes = dict(kind="ratio_levels", levels=ratio_level_indices(H, W, shrink, npo), which="ratio")
    return _as_dtype(img, dtype, 160), opts, notes


PLATEAU_VALUES = dict(min=37, interior=(50, 58), max=63, second_min=12, second_max=60)


def _plateau_image(H, W, seed, vmin, interior, vmax):
    """Noise of [40, vmax - 1] with flat rectangles -- wide ones that survive three octaves, and bars 3 and 5 pixels wide for
    their perimeter (an integer channel function shows a flipped pixel only beside a gradient) -- whose edges sit on odd
    and on even coordinates."""
    rng = np.random.default_rng(seed)
    img = rng.integers(40, vmax, (H, W), dtype=np.uint8)
    vals = [vmin, interior[0], vmax, vmin, interior[1], vmin]
    # six wide rectangles on a 2 x 3 grid, half a cell each way, origins alternately odd and even
    ch, cw = H // 2, W // 3
    for i, v in enumerate(vals):
        gy, gx = divmod(i, 3)
        y0, x0 = gy * ch + 3 + (i & 1), gx * cw + 4 + ((i >> 1) & 1)
        img[y0:y0 + ch // 2 + (i & 1), x0:x0 + cw // 2] = v
    # bars in what the rectangles leave free of every cell: horizontal ones under them, vertical ones beside them
    for i in range(6):
        gy, gx = divmod(i, 3)
        y0 = gy * ch + 3 + ch // 2 + 4
        for j, y in enumerate(range(y0, (gy + 1) * ch - 8, 8)):
            v = vals[(i + 3) % 6] if j % 3 == 2 else vmin
            img[y + (j & 1):y + (j & 1) + (3 if j % 2 else 5), gx * cw + 3:gx * cw + cw // 2] = v
        x0 = gx * cw + 4 + cw // 2 + 4
        for j, x in enumerate(range(x0, (gx + 1) * cw - 8, 8)):
            v = vals[(i + 3) % 6] if j % 3 == 2 else vmin
            img[gy * ch + 2:(gy + 1) * ch - 3, x + (j & 1):x + (j & 1) + (5 if j % 2 else 3)] = v
    return img


def plateaus(shrink, dtype="uint8"):
    """(images [2, H, W], channel_opts without the function, notes).  Slot 0 has the minimum 12, slot 1 the minimum 37 (the
    larger minimum in slot 1: a kernel that clipped image 1 to image 0's range would leave its 36s standing); both hold
    plateaus at 37, at interior values and at their maximum: 60 in slot 0, 63 in slot 1.  int16: minus 300 -- every value
    negative, so the fp64 sum over a plateau falls short TOWARD zero, the truncation gives v + 1, and the clip to the
    MAXIMUM decides: -240 in slot 0, -237 in slot 1, so the range of the wrong image is wrong here too."""
    H, W, npo = RATIO_SHAPES[shrink]
    a = _plateau_image(H, W, 2000 + shrink, PLATEAU_VALUES["min"], PLATEAU_VALUES["interior"], PLATEAU_VALUES["max"])
    b = _plateau_image(H, W, 3000 + shrink, PLATEAU_VALUES["second_min"], (PLATEAU_VALUES["min"], PLATEAU_VALUES["interior"][0]),
                       PLATEAU_VALUES["second_max"])
    imgs = np.stack([_as_dtype(b, dtype, 300), _as_dtype(a, dtype, 300)])
    opts = dict(shrink=shrink, n_per_oct=npo, smooth=None)
    notes = dict(kind="plateaus", which="all", minima=(12, 37), maxima=(60, 63), interior=((37, 50), (50, 58)))
    return imgs, opts, notes


def design_image(design, shrink, dtype):
    """(2-D image, opts, notes) of a case of CASES; plateaus: the image of slot 1 (minimum 37)."""
    if design == "ratio_levels":
        return ratio_levels(shrink, dtype)
    imgs, opts, notes = plateaus(shrink, dtype)
    return imgs[1], opts, notes


@functools.lru_cache(None)
def design_masks(design, shrink, dtype, slot=1):
    """{level: masks} of a design's image (plateaus: of batch slot `slot`): shared by every cell of that shrink and dtype."""
    if design == "ratio_levels":
        img, opts, notes = ratio_levels(shrink, dtype)
    else:
        imgs, opts, notes = plateaus(shrink, dtype)
        img = imgs[slot]
    return designed_levels(img, shrink, opts["n_per_oct"], which=notes["which"])


@functools.lru_cache(None)
def all_level_masks(design, shrink, dtype, slot=1):
    """fp64 masks (near, clip_decided) of EVERY level of octaves 0 .. 2 of a design, the ratio levels included."""
    if design == "ratio_levels":
        img, opts, _ = ratio_levels(shrink, dtype)
    else:
        imgs, opts, _ = plateaus(shrink, dtype)
        img = imgs[slot]
    return designed_levels(img, shrink, opts["n_per_oct"], which="all")


def count_in_path(masks, kind, path, func, shrink, smooth, tiles):
    """How many pixels of mask `kind` lie under output pixels computed by tiles of `path` (tiles: classify_tiles of the plan)."""
    g = tile_geom(func, shrink, smooth)
    n = 0
    for l, m in masks.items():
        if tiles[l] is None:
            continue
        ys, xs = np.nonzero(m[kind])
        ty = np.minimum(ys // shrink // g["TU"], tiles[l].shape[0] - 1)
        tx = np.minimum(xs // shrink // g["TV"], tiles[l].shape[1] - 1)
        n += int((tiles[l][ty, tx] == path).sum())
    return n


def path_levels(func, shrink, smooth):
    """(shapes, impossible): shapes [(H, W, n_per_oct)] for uint8 noise images whose plans hold, together, every path that
    exists in the cell; `impossible`: the paths that cannot occur there (module docstring: Findings)."""
    impossible = {"upscale"}
    if func != "grad_mag" and shrink != 2:
        impossible.add("direct_budget")
    if shrink == 1:
        impossible.add("mixed_axis")
    # the ratio shape holds the inner and edge identity tiles and the staged ones (at shrink 2 also tiles beyond the
    # budget); 75 x 150 (shrink 2) and 76 x 150 (shrink 4) have a level 0 that is the identity on one axis only
    shapes = [RATIO_SHAPES[shrink]]
    if shrink == 2:
        shapes.append((75, 150, 2))
        if func != "grad_mag":
            shapes.append((150, 300, 12))                     # the last levels of an octave of 12: zoom 1.68 .. 1.89
    if shrink == 4:
        shapes.append((76, 150, 2))
    return shapes, impossible


def path_image(H, W):
    return np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W), dtype=np.uint8)


# ------------------------------------------------------------------------------ failure messages
def describe_mismatch(got, ref, level, func, shrink, smooth, plan, masks=None):
    """Names the first differing output pixel of a level, its tile, the tile's path and whether a designed pixel lies in the
    3 x 3 (x shrink) footprint of that output pixel."""
    diff = np.argwhere((np.ascontiguousarray(got).view(np.uint8).reshape(got.shape[0], got.shape[1], -1)
                        != np.ascontiguousarray(ref).view(np.uint8).reshape(ref.shape[0], ref.shape[1], -1)).any(-1))
    r, c = (int(x) for x in diff[0])
    ty, tx = tile_of(func, shrink, smooth, r, c)
    tiles = classify_tiles(plan, func)[level]
    msg = (f"level {level}: {len(diff)} output pixels differ, first at ({r}, {c}) = {got[r, c].tolist()} against {ref[r, c].tolist()}, "
           f"tile ({ty}, {tx}) path {tiles[ty, tx]}")
    if masks is not None and level in masks:
        m = masks[level]
        rad = shrink * (1 + (1 if smooth else 0)) + (6 if func == "grad_mag" else 1)
        ys = slice(max(r * shrink - rad, 0), r * shrink + shrink + rad)
        xs = slice(max(c * shrink - rad, 0), c * shrink + shrink + rad)
        kinds = [k for k in ("tie", "near", "landed", "rounding_decided", "clip_decided") if m[k][ys, xs].any()]
        msg += f", designed pixels in its footprint: {kinds or 'none'}"
    else:
        msg += ", not a designed level"
    return msg
