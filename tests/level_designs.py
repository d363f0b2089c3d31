"""Designed inputs for the level kernels of csrc/wb_chan_levels.hip and for the cast-back of the float64-held image dtypes
(NumPy and the library's host-only entry points: no GPU, no torch).

Two pieces of pyramid code are held here on purpose:

  * the cast of a resized level back to the image dtype -- Src<double>::finish (csrc/wb_chan_tile.h, the channel tile
    kernels) and the sizeof(T) == 8 branch of resize_level_kernel (its own copy of the clip and the WB_CAST_* switch, the
    result a double) -- for every image dtype held as float64.  wb_resize_level_launch hands back the resized and cast
    image itself: every wrong pixel is visible.
  * the pyramid around a caller's own channel function: resize_level_kernel, pool2_kernel and smooth_kernel
    (wb_pool_smooth_launch), on arrays [H][W][C] of uint8 and float32.

What is provided
  CAST_DESIGNS, cast_design     one design per cast mode and purpose: images, n_per_oct, the designed levels, the classes it
                                claims and the emulated wrong kernels (CAST_FAULTS) it is meant to catch
  level_masks                   per level: the oracle's fp64 t, the oracle's pixel (as float64) and the masks of the classes
  emulate_level                 the level a kernel with one fault of CAST_FAULTS would return
  round_f16_exact, bool_exact   exact arithmetic the host test holds the oracle's float16 and bool casts to
  POOL_CASES, pool_case         the arrays of the pool and smooth designs; oracle_pool_smooth, pool_wrong, smooth_wrong
  same_values, describe_level_mismatch, describe_array_mismatch

Classes (per level; the TRUNC ones are resample_designs.classify_pixels's, with exact integer arithmetic)
  TRUNC   tie_or_near, rounding_decided, landed, clip_decided; negative_fraction: t in (-1, 0) on its way to the integer 0
          (trunc gives -0.0 in fp64, the integer types have one zero); beyond_f32: the pixel is no float32
  F16     tie_down / tie_up: clip(t) is exactly the midpoint of two float16 neighbours and the even rule sends it down / up
          (for even integers of [2048, 4094]: an odd integer 1 / 3 mod 4); through_f32: rounding through float32 first
          gives another float16; subnormal: the pixel is a non-zero float16 below 2^-14; at_max: the pixel is 65504
  BOOL    partial: 0 < t < 1 (True under != 0, False under >= 0.5 for the lower half of them, False under truncation);
          beside: t == 0 exactly although a tap of weight 0 meets a True
  NONE    wide: the pixel has more than 24 significant bits; clip_decided: t != clip(t); near: the other association of
          the four-term sum (resample_designs.level_t_other_order) gives another double
  NaN     all_nan: every pixel of a level of the octave that holds the NaN; untouched: the levels of the other octaves

Findings (host arithmetic, asserted by test_level_designs_host.py)
  * `clip_after_cast` is no fault: every cast here is monotone and the clip bounds are values of the image dtype, so the
    clip and the cast commute.  The host test asserts that this emulated kernel equals the oracle on every design; no
    design is meant to catch it.
  * a float16 level cannot overflow: t is a convex combination of pixels up to fp64 rounding and 65504 rounds to inf only
    from 65520 on.  The `max` image (maximum 65504) therefore holds the pixels that must come out as 65504, not as inf;
    `no_clip` differs on no float16 pixel and is asked of the TRUNC and NONE plateaus only.
  * an output element count of 257 is prime: it needs a side of 257 (a 2 x 514 array pooled, a 1 x 257 array copied) --
    longer than the 96 columns of the other arrays, 1028 elements in all.
  * for uint8 arrays `fp32_accumulate` and `separable` are exact (sums up to 4080): they are asked of the float32 `cancel`
    array only.
  * found on the GPU by the `zero` designs through wb_resize_level_launch (first wrong pixel: class negative_fraction;
    plateaus-int8 and, in octave 4, top-int64 hold such pixels too): a pixel with -1 < clip(t) < 0 of an integer image was
    stored as trunc = -0.0, another bit pattern than the integer's one zero.  resize_level_kernel now adds + 0.0 after the
    truncation, as pool_f64_kernel does, and so does the same expression in Src<double>::finish -- where grad_hist's
    absolute value hid the sign and no test could show it.

Counts the host test measures (its assertions are the floors of 100 per class and per wrong kernel; these are the values,
summed over a design's levels; pytest -s prints them)
  zero      levels 2, 11, 20 of 280 x 392 / 9.  int16 / int32 / int64: tie_or_near 26738, rounding_decided 198,
            negative_fraction 621; differing pixels: floor 8696, round 40947, other_order 652, negative_zero (trunc without
            the + 0.0) 621.  int8 (32 of the 128 values below zero): 26728, 200, 1285; 19060, 40769, 645, 1285
  top       the same levels.  uint16: tie_or_near 24902, rounding_decided 1377; round 41314, other_order 3311.  int32 / uint32:
            tie_or_near 25029 / 24572, rounding_decided 1901 / 1955, beyond_f32 80522 / 105167 (of 105840 pixels); round 41807 /
            41830, other_order 3498 / 3739, through_float32 as many as beyond_f32.  int64 / uint64 (+-2^50 in column bands /
            2^50; the fp64 spacing there is 1/4): landed 12646, beyond_f32 105534; round 36474 / 36457, other_order 8306 / 8281
  plateaus  clip_decided in the 27 levels of octaves 0 .. 2, slot 0 / slot 1 (no_clip differs in as many): int8 346 / 1020, int16
            575 / 1919, uint16 18119 / 14036, int32 16302 / 13708, uint32 19783 / 12781, int64 355 / 330, uint64 10507 / 16592
  float16   ties (112 x 168 / 9, levels 2, 6, 11, 15: 96 x 144 and 70 x 105, and 48 x 72 and 35 x 52 of octave 1): tie_down 345, tie_up 358,
            through_f32 247; f16_through_f32 differs in 247 pixels, f16_truncate in 9923.  subnormal (40 x 56 / 3, levels 1, 2,
            4, 5): 2768 subnormal pixels, f16_flush differs in as many, f16_truncate in 1326.  max (15 x 180 / 3, one octave: a
            float16 quad of such values overflows in avg_pool_2): at_max 1078
  bool      bars / inverse (64 x 96 / 4, octaves 0 and 1): partial 1618 / 1114, beside 730 / 157; bool_half differs in 1263 / 173,
            bool_trunc in 1618 / 1087
  float64   wide (112 x 168 / 9, octaves 0 and 1): wide 122478, clip_decided 3773, near 42503; through_float32 differs in 122478,
            no_clip in 3773, other_order in 37633
  NaN       float16 / float64, 41 x 57 / 3: all_nan 4652 (every pixel of the 3 levels of octave 0), untouched 1359 (octaves 1, 2)
  pool      uint8 quads: every sum 0 .. 1020 in each of the four arrays (C = 1, 2, 3, 5); nowrap differs in 1165 of 1536, 768 of
            1024, 3091 of 4371 and 823 of 1100 elements, and in 198 .. 396 of the 255 .. 513 of the count arrays.  float32
            quads: rowfirst differs in 261 / 189 / 746 / 201 elements, pairwise in 355 / 228 / 1046 / 247; +-inf in the oracle's
            order and finite rows first in 16 (C = 3: 33) quads, the other way round in as many, finite pairwise in as many
  smooth    cancel (10 x 14 x 3, 288 interior elements): fp32_accumulate differs in 52, separable in 48; border_copied in 72 of
            198 (all255), 93 of 702 (ramps), 132 of 420 (cancel), 36 of 99 (nonfinite) elements
"""
import functools
from fractions import Fraction

import numpy as np

import octave_designs as od
import resample_designs as rd
from oracle import wb_oracle as orc
from waldboost_amd.plan import PyramidPlan

CAST_MODE = {"int8": "TRUNC", "int16": "TRUNC", "uint16": "TRUNC", "int32": "TRUNC", "uint32": "TRUNC", "int64": "TRUNC",
             "uint64": "TRUNC", "bool": "BOOL", "float16": "F16", "float64": "NONE"}
HELD = tuple(CAST_MODE)
CAST_FAULTS = ("floor", "round", "through_float32", "f16_through_f32", "f16_truncate", "f16_flush", "bool_half", "bool_trunc",
               "no_clip", "clip_after_cast", "other_order", "negative_zero")
SIGNED = ("int8", "int16", "int32", "int64")
FLOOR = 100                               # designed pixels per claimed class, and differing pixels per fault (the issue's floor)
RATIO_H, RATIO_W, RATIO_NPO = rd.RATIO_SHAPES[1]
F16_SHAPE = (112, 168, 9)

# (design, dtype): the list both test modules are parametrised over
CAST_DESIGNS = ([("zero", d) for d in SIGNED] + [("top", d) for d in ("uint16", "int32", "uint32", "int64", "uint64")]
                + [("plateaus", d) for d in HELD if CAST_MODE[d] == "TRUNC"]
                + [("ties", "float16"), ("subnormal", "float16"), ("max", "float16")]
                + [("bars", "bool"), ("inverse", "bool"), ("all_false", "bool"), ("all_true", "bool")]
                + [("wide", "float64"), ("nan", "float16"), ("nan", "float64")])
# the existing uint8 / float32 images of resample_designs, for wb_resize_level_launch's own two kernels
PLAIN_DESIGNS = [(d, t) for d in ("ratio_levels", "plateaus") for t in ("uint8", "float32")]


def case_id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------ bits
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def differing(got, ref):
    """Boolean array: where got and ref differ -- bit for bit, except that any NaN equals any NaN (the payload and sign of
    a generated NaN are the hardware's)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    d = bits(got) != bits(ref)
    if got.dtype.kind == "f":
        d &= ~(np.isnan(got) & np.isnan(ref))
    return d


def same_values(got, ref):
    return not differing(got, ref).any()


# ------------------------------------------------------------------------------ cast designs: images
def _signs(shape, band=56):
    """+1 / -1 in column bands of `band` pixels (a multiple of 8: the bands survive three octaves)."""
    return np.where((np.arange(shape[1]) // band) % 2 == 1, -1, 1)[None, :] * np.ones(shape, np.int64)


def _top_offset(dtype):
    """What lifts a byte image to the top of the dtype's range (64-bit types: to 2^50, exact in float64)."""
    dt = np.dtype(dtype)
    return (1 << 50) if dt.itemsize == 8 else int(np.iinfo(dt).max)


@functools.lru_cache(None)
def _u8_ratio():
    return rd.ratio_levels(1, "uint8")[0]


@functools.lru_cache(None)
def _u8_plateaus():
    return rd.plateaus(1, "uint8")[0]


def _f16_blocks(rng, H, W, lo, hi, step):
    """Multiples of `step` in [lo, hi]: pixel noise in the upper half, flat 2 x 2, 4 x 4 and 8 x 8 blocks in the lower."""
    n = (hi - lo) // step + 1
    img = lo + step * rng.integers(0, n, (H, W))
    top, third = H // 2, -(-W // 3)
    for j, k in enumerate((2, 4, 8)):
        w = min(third, W - j * third)
        a = lo + step * rng.integers(0, n, (-(-(H - top) // k), -(-w // k)))
        img[top:, j * third:j * third + w] = np.kron(a, np.ones((k, k), np.int64))[:H - top, :w]
    return img


def _bool_bars(H, W):
    """False ground with isolated True pixels (every 7th row, 9th column) and short bars, horizontal and vertical, whose
    ends sit on odd and on even coordinates."""
    img = np.zeros((H, W), np.bool_)
    img[3::7, 4::9] = True
    for i, y in enumerate(range(5, H - 2, 11)):
        x = 2 + 13 * (i % 5)
        img[y, x:x + 3 + (i % 4)] = True
    for i, x in enumerate(range(7, W - 2, 10)):
        y = 1 + 9 * (i % 5)
        img[y:y + 2 + (i % 5), x] = True
    return img


@functools.lru_cache(None)
def cast_design(name, dtype):
    """dict(images [n, H, W] (read-only), n_per_oct, levels (the designed ones), claims {class: slot or None}, faults)."""
    dt = np.dtype(dtype)
    mode = CAST_MODE.get(dtype)
    H, W, npo = RATIO_H, RATIO_W, RATIO_NPO
    ratio_lv = rd.ratio_level_indices(H, W, 1, npo)[:3]
    if name == "zero":
        imgs = (_u8_ratio().astype(np.int64) - 160).astype(dt)[None]
        d = dict(levels=ratio_lv, claims=("tie_or_near", "rounding_decided", "negative_fraction"),
                 faults=("floor", "round", "other_order", "negative_zero"))
    elif name == "top":
        v = _u8_ratio().astype(np.int64) + (_top_offset(dtype) - 255)
        if dtype == "int64":
            v = v * _signs(v.shape)
        imgs = v.astype(dt)[None]
        wide = dt.itemsize >= 4
        claims = ("landed",) if dt.itemsize == 8 else ("tie_or_near", "rounding_decided")
        d = dict(levels=ratio_lv, claims=claims + (("beyond_f32",) if wide else ()),
                 faults=("round", "other_order") + (("through_float32",) if wide else ()))
    elif name == "plateaus":
        p = _u8_plateaus().astype(np.int64)
        off = {"int8": -100, "int16": -300, "int64": -63 - (1 << 50)}.get(dtype)
        if off is None:
            off = _top_offset(dtype) - 63
        imgs = (p + off).astype(dt)
        d = dict(levels=[l for l in range(3 * npo)], claims=("clip_decided",), faults=("no_clip",), exact=False)
    elif name == "ties":
        H, W, npo = F16_SHAPE
        imgs = _f16_blocks(np.random.default_rng(4100), H, W, 2048, 4094, 2).astype(dt)[None]
        d = dict(levels=[2, 6, npo + 2, npo + 6], claims=("tie_down", "tie_up", "through_f32"), faults=("f16_through_f32", "f16_truncate"))
    elif name == "subnormal":
        H, W, npo = 40, 56, 3
        rng = np.random.default_rng(4200)
        v = rng.integers(1, 1024, (H, W)) * rng.choice([-1, 1], (H, W))
        imgs = (v * 2.0 ** -24).astype(dt)[None]
        d = dict(levels=[1, 2, 4, 5], claims=("subnormal",), faults=("f16_flush", "f16_truncate"))
    elif name == "max":
        # one octave only (15 rows): a float16 quad of such values overflows in avg_pool_2, which is not the point here
        H, W, npo = 15, 180, 3
        rng = np.random.default_rng(4300)
        v = 32768 + 32 * rng.integers(0, 1023, (H, W))
        v[2:13, 10:120] = 65504
        v[4:12, 130:170] = 32768
        imgs = v.astype(dt)[None]
        d = dict(levels=[1, 2], claims=("at_max",), faults=())
    elif name in ("bars", "inverse"):
        H, W, npo = 64, 96, 4
        b = _bool_bars(H, W)
        imgs = (b if name == "bars" else ~b)[None]
        d = dict(levels=list(range(2 * npo)), claims=("partial", "beside"), faults=("bool_half", "bool_trunc"))
    elif name in ("all_false", "all_true"):
        H, W, npo = 64, 96, 4
        imgs = np.full((1, H, W), name == "all_true", np.bool_)
        d = dict(levels=list(range(2 * npo)), claims=(), faults=())
    elif name == "wide":
        H, W, npo = F16_SHAPE
        rng = np.random.default_rng(4400)
        v = 300.0 + 400.0 * rng.random((H, W))
        v[H // 2:, :] = np.kron(300.0 + 400.0 * rng.random((H // 8, W // 4)), np.ones((4, 4)))[:H - H // 2, :W]
        lo, hi = 100.0 + 1.0 / 3.0, 900.0 + 2.0 / 7.0               # the octaves' bounds: away from 0, 53 significant bits
        for i, (y, x) in enumerate(((4, 6), (4, 90), (60, 20), (60, 110), (30, 50), (84, 70))):
            v[y:y + 18 + (i & 1), x:x + 40 + (i >> 1)] = hi if i % 2 else lo
        imgs = v[None]
        d = dict(levels=list(range(2 * npo)), claims=("wide", "clip_decided", "near"), faults=("through_float32", "no_clip", "other_order"))
    elif name == "nan":
        H, W, npo = 41, 57, 3
        rng = np.random.default_rng(4500)
        v = np.round(rng.standard_normal((H, W)) * 64.0) / 8.0
        v[H - 3:, W - 3:] = 2.5
        imgs = v.astype(dt)[None]
        imgs[0, H - 1, W - 1] = np.nan                                # the odd last row and column: octave 0 only
        d = dict(levels=list(range(3 * npo)), claims=("all_nan", "untouched"), faults=())
    else:
        raise KeyError(name)
    assert imgs.dtype == dt and (mode is not None)
    imgs.setflags(write=False)
    d.update(name=name, dtype=dtype, images=imgs, n_per_oct=npo, shape=(H, W), exact=d.get("exact", True))
    return d


def plain_design(name, dtype):
    """The uint8 / float32 images of resample_designs at shrink 1: (images [n, H, W], n_per_oct)."""
    if name == "ratio_levels":
        img, opts, _ = rd.ratio_levels(1, dtype)
        return img[None], opts["n_per_oct"]
    imgs, opts, _ = rd.plateaus(1, dtype)
    return imgs, opts["n_per_oct"]


@functools.lru_cache(None)
def octaves_of(name, dtype, slot=0):
    imgs = cast_design(name, dtype)["images"] if (name, dtype) in CAST_DESIGNS else plain_design(name, dtype)[0]
    with np.errstate(all="ignore"):
        return list(orc.image_octaves(imgs[slot]))


def plan_levels(H, W, shrink, n_per_oct):
    return orc.level_plan(H, W, shrink, n_per_oct)


@functools.lru_cache(None)
def oracle_level(name, dtype, slot, l):
    """The oracle's level l of a design's image (shrink 1), in the image dtype; shared, read-only."""
    d_npo = cast_design(name, dtype)["n_per_oct"] if (name, dtype) in CAST_DESIGNS else plain_design(name, dtype)[1]
    octs = octaves_of(name, dtype, slot)
    H, W = octs[0].shape
    lv = plan_levels(H, W, 1, d_npo)[l]
    with np.errstate(all="ignore"):
        out = orc.resize_bilinear(octs[lv["oct"]], lv["nh"], lv["nw"])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------ cast designs: classes
def _clip(t, base):
    mn, mx = np.float64(base.min()), np.float64(base.max())
    with np.errstate(invalid="ignore"):
        return np.clip(t, mn, mx)


def _f16_neighbours(v):
    """(lo, hi) float16 neighbours of the doubles v with lo <= v <= hi, as float64 (equal where v is a float16)."""
    with np.errstate(over="ignore"):
        r = v.astype(np.float16)
        r64 = r.astype(np.float64)
        up = np.nextafter(r, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(r, np.float16(-np.inf)).astype(np.float64)
    lo = np.where(r64 <= v, r64, dn)
    hi = np.where(r64 >= v, r64, up)
    return lo, hi


def level_masks(base, nh, nw, exact=True):
    """The classes of one level resized from the octave image `base` (a held dtype): dict with t, out (the oracle's pixel as
    float64) and one boolean mask per class of the dtype's cast mode (module docstring)."""
    mode = CAST_MODE[str(base.dtype)]
    with np.errstate(all="ignore"):
        ref = orc.resize_bilinear(base, nh, nw)
    out = ref.astype(np.float64)
    if mode == "TRUNC":
        m = rd.classify_pixels(base, nh, nw, exact=exact)
        t = m["t"]
        if base.dtype.itemsize == 8:
            # NumPy's float -> integer cast is undefined outside the target's range: no fp64 value comes near it
            assert np.abs(t).max() < 2.0 ** 52 and (base.dtype.kind == "i" or t.min() >= 0.0)
        v = _clip(t, base)
        res = dict(t=t, out=out, tie_or_near=m["tie"] | m["near"], rounding_decided=m["rounding_decided"], landed=m["landed"],
                   near=m["near"], clip_decided=m["clip_decided"], negative_fraction=(v < 0) & (v > -1),
                   beyond_f32=out.astype(np.float32).astype(np.float64) != out)
        assert np.array_equal(m["out"], ref.astype(np.int64))
        if exact:
            res.update(tie=m["tie"], trunc_exact=m["trunc_exact"])
        return res
    t = rd.level_t(base, nh, nw)
    v = _clip(t, base)
    res = dict(t=t, out=out)
    if mode == "F16":
        lo, hi = _f16_neighbours(v)
        tie = (lo != hi) & (v - lo == hi - v)                       # (exact: Sterbenz, the neighbours are within a factor 2)
        res["tie_down"] = tie & (out == lo)
        res["tie_up"] = tie & (out == hi)
        with np.errstate(over="ignore"):
            res["through_f32"] = bits(v.astype(np.float32).astype(np.float16)) != bits(v.astype(np.float16))
        res["subnormal"] = (out != 0) & (np.abs(out) < 2.0 ** -14)
        res["at_max"] = out == 65504.0
        res["all_nan"] = np.isnan(out)
    elif mode == "BOOL":
        res["partial"] = (t > 0) & (t < 1)
        res["beside"] = (t == 0) & _bool_any_tap(base, nh, nw, nonzero_only=False)
    else:
        res["wide"] = out.astype(np.float32).astype(np.float64) != out
        res["clip_decided"] = bits(t) != bits(v)
        res["near"] = bits(rd.level_t_other_order(base, nh, nw)) != bits(t)
        res["all_nan"] = np.isnan(out)
    return res


def _bool_any_tap(base, nh, nw, nonzero_only=True):
    """Whether any of the four taps of an output pixel (nonzero_only: any tap whose fp64 weight product is not 0) is True."""
    r0, r1, wr0, wr1 = orc._axis_taps(base.shape[0], nh)
    c0, c1, wc0, wc1 = orc._axis_taps(base.shape[1], nw)
    hit = np.zeros((nh, nw), bool)
    for r, wr in ((r0, wr0), (r1, wr1)):
        for c, wc in ((c0, wc0), (c1, wc1)):
            live = np.ones((nh, nw), bool) if not nonzero_only else ((wr != 0)[:, None] & (wc != 0)[None, :])
            hit |= base[r][:, c] & live
    return hit


def bool_exact(base, nh, nw):
    """What a bool level must be: True where a tap of non-zero weight meets a True (a weight is an fp64 number m * 2^-k
    with |m * 2^-k| >= 2^-53 or 0, so no product of two of them underflows and no sum of non-negative terms cancels) --
    unless the octave is all True, where the clip to [1, 1] lifts every pixel."""
    if base.all():
        return np.ones((nh, nw), bool)
    return _bool_any_tap(base, nh, nw)


def round_f16_exact(x):
    """One double rounded to binary16, nearest even, by integer arithmetic; the result as a float."""
    x = float(x)
    if x != x or x in (float("inf"), float("-inf")) or x == 0.0:
        return x
    a = Fraction(abs(x))
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -14) - 10)                            # the spacing of float16 at |x|
    u = a / q
    n = u.numerator // u.denominator
    rem = u - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = float(n * q)
    if r >= 65520.0:
        r = float("inf")
    return -r if x < 0 else (r if r != 0.0 else 0.0)


def emulate_level(base, nh, nw, fault=None):
    """The level (as float64) a kernel with `fault` (CAST_FAULTS; None: the right kernel) would hand back."""
    mode = CAST_MODE[str(base.dtype)]
    t = rd.level_t_other_order(base, nh, nw) if fault == "other_order" else rd.level_t(base, nh, nw)
    mn, mx = np.float64(base.min()), np.float64(base.max())
    with np.errstate(all="ignore"):
        if mn != mn or mx != mx:
            return np.full(t.shape, np.nan)
        v = t if fault in ("no_clip", "clip_after_cast") else np.clip(t, mn, mx)
        if mode == "TRUNC":
            v = np.floor(v) if fault == "floor" else np.rint(v) if fault == "round" else np.trunc(v)
            if fault != "negative_zero":
                v = v + 0.0
        elif mode == "BOOL":
            hit = v >= 0.5 if fault == "bool_half" else np.trunc(v) != 0 if fault == "bool_trunc" else v != 0
            v = hit.astype(np.float64)
        elif mode == "F16":
            if fault == "f16_through_f32":
                r = v.astype(np.float32).astype(np.float16)
            elif fault == "f16_truncate":
                lo, hi = _f16_neighbours(v)
                r = np.where(v >= 0, lo, hi).astype(np.float16)
            else:
                r = v.astype(np.float16)
            v = r.astype(np.float64)
            if fault == "f16_flush":
                v = np.where(np.abs(v) < 2.0 ** -14, np.copysign(0.0, v), v)
        if fault == "through_float32":
            v = v.astype(np.float32).astype(np.float64)
        if fault == "clip_after_cast":
            v = np.clip(v, mn, mx)
    return v


@functools.lru_cache(None)
def design_masks(name, dtype, slot=0):
    """{level: masks} of the designed levels of a cast design's image `slot`."""
    d = cast_design(name, dtype)
    octs = octaves_of(name, dtype, slot)
    H, W = d["shape"]
    plan = plan_levels(H, W, 1, d["n_per_oct"])
    out = {}
    for l in d["levels"]:
        lv = plan[l]
        out[l] = level_masks(octs[lv["oct"]], lv["nh"], lv["nw"], exact=d["exact"])
        out[l]["oct"] = lv["oct"]
        if d["name"] == "nan":
            out[l]["untouched"] = ~np.isnan(out[l]["out"]) & (lv["oct"] > 0)
    return out


CLASS_NAMES = ("tie", "tie_or_near", "rounding_decided", "landed", "clip_decided", "negative_fraction", "beyond_f32", "tie_down", "tie_up",
               "through_f32", "subnormal", "at_max", "partial", "beside", "wide", "near", "all_nan", "untouched")


def describe_level_mismatch(got, ref, level, masks=None):
    """Names the first wrong pixel of a level and the designed classes it belongs to."""
    diff = np.argwhere(differing(got, ref))
    r, c = (int(x) for x in diff[0])
    msg = f"level {level}: {len(diff)} of {got.size} pixels differ, first at ({r}, {c}) = {got[r, c]!r} ({int(bits(got)[r, c]):#x}) against {ref[r, c]!r} ({int(bits(ref)[r, c]):#x})"
    if masks is not None and level in masks:
        m = masks[level]
        kinds = [k for k in CLASS_NAMES if k in m and m[k][r, c]]
        msg += f", t = {m['t'][r, c]!r}, classes: {kinds or 'none'}"
    else:
        msg += ", not a designed level"
    return msg


# ------------------------------------------------------------------------------ pool and smooth designs
def _place(quads, H, W, C, fill):
    """Quads laid over the 2 x 2 cells of an [H][W][C] array: channel c of cell p (row-major) holds quad p * C + c, so no two
    channels of a cell hold the same quad; a = (0, 0), b = (1, 0), c = (0, 1), d = (1, 1) as (row, column); the odd last row
    and column hold `fill`."""
    oh, ow = H // 2, W // 2
    arr = np.full((H, W, C), fill, quads.dtype)
    q = quads[np.arange(oh * ow * C) % len(quads)].reshape(oh, ow, C, 4)
    arr[0:2 * oh:2, 0:2 * ow:2] = q[..., 0]
    arr[1:2 * oh:2, 0:2 * ow:2] = q[..., 1]
    arr[0:2 * oh:2, 1:2 * ow:2] = q[..., 2]
    arr[1:2 * oh:2, 1:2 * ow:2] = q[..., 3]
    return arr


@functools.lru_cache(None)
def u8_quads():
    """octave_designs.quad_list with one quad of every sum 0 .. 1020 first: the first 1021 cells of an array hold every
    residue of the sum mod 256 at every wrap count (0, 256, 512, 768 taken off)."""
    ql = od.quad_list()
    _, first = np.unique(ql.astype(np.int64).sum(1), return_index=True)
    rest = np.setdiff1d(np.arange(len(ql)), first)
    return ql[np.concatenate([first, rest])]


@functools.lru_cache(None)
def f32_quads():
    """octave_designs.float_quad_list: the overflowing quads (+inf and -inf, by the first two values alone or only by the
    whole sum), those near FLT_MAX / 4, the subnormal ones, then the mixed magnitudes."""
    mixed, big, near, sub = od.float_quad_list()
    fmax = float(np.finfo(np.float32).max)
    one = []                              # overflow in one order only: (t, t, -t, small) is +-inf in the oracle's order and finite
    for sign in (1.0, -1.0):              # rows first; (t, -.2 t, .8 t, -t) +-inf but finite pairwise; (t, -.9 t, .8 t, .05 t) finite
        for i in range(8):                # in the oracle's order and +-inf rows first
            t = sign * fmax * (0.7 + 0.01 * i)
            one += [[t, t, -t, sign * 1e30 * (i + 1)], [t, -0.2 * t, 0.8 * t, -t], [t, -0.9 * t, 0.8 * t, 0.05 * t]]
    return np.concatenate([np.array(one, np.float32), big, near, sub, mixed]).astype(np.float32)


def _cancel(H, W, C):
    """float32 values of magnitude 2^60 and 2^30 next to 1.0 and 3.0, signs mixed: the nine-term fp64 sum cancels exactly
    where an fp32 accumulation has long lost the small terms, and in another order where rows are summed first."""
    assert C == 3
    rng = np.random.default_rng(4600)
    pal = np.array([2.0 ** 60, -2.0 ** 60, 2.0 ** 59, -2.0 ** 59, 2.0 ** 30, -2.0 ** 30, 2.0 ** 29, -2.0 ** 29, 1.0, -1.0, 3.0, 0.5,
                    1.0 + 2.0 ** -20], np.float32)
    a = pal[rng.integers(0, len(pal), (H, W, C))]                    # channel 2: the palette at random
    a[..., :2] = rng.integers(1, 8, (H, W, 2)).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W]
    # channel 0: +-2^30 in every other column, signs alternating: around an odd column the two cancel inside each row and
    # fp64 keeps the small terms between them (2^30 + 2 is exact), fp32 has lost them (its spacing at 2^30 is 128)
    a[..., 0] = np.where(x % 2 == 0, np.where(x % 4 == 0, 2.0 ** 30, -(2.0 ** 30)), a[..., 0])
    # channel 1: +-2^60 on the even rows and columns, the sign alternating along the row: in source order every small term
    # summed before a 2^60 is lost in fp64 too (its spacing there is 256), so the result holds only what came after the last
    # cancellation -- a row pass first keeps the rows without a 2^60 whole
    a[..., 1] = np.where((x % 2 == 0) & (y % 2 == 0), np.where(x % 4 == 0, 2.0 ** 60, -(2.0 ** 60)), a[..., 1])
    return a.astype(np.float32)


def _ramps(H, W):
    """uint8 [H][W][3]: a row ramp, a column ramp (steps that are no multiple of 16: the weights show in the low bits) and
    single bright pixels on 0 (one per 4 x 4 cell, at every phase)."""
    a = np.zeros((H, W, 3), np.uint8)
    a[..., 0] = (np.arange(H) * 19 % 256)[:, None]
    a[..., 1] = (np.arange(W) * 13 % 256)[None, :] + (np.arange(H) % 3)[:, None]
    for i, (y, x) in enumerate((y, x) for y in range(1, H - 2, 4) for x in range(1, W - 2, 4)):
        a[y + i % 2, x + (i // 2) % 2, 2] = 255 - 7 * (i % 9)
    return a


def _nonfinite(H, W):
    rng = np.random.default_rng(4700)
    a = rng.standard_normal((H, W, 1)).astype(np.float32) * np.float32(8)
    a[1, 1, 0] = np.nan
    a[1, W - 2, 0] = np.inf
    a[H - 2, 1, 0] = -np.inf
    return a


# name -> (dtype, builder).  The shapes: C = 1, 2, 3, 5; odd H and odd W (the last row and column hold 255 / 7.0e37: read
# into a result they show); H = 1 and W = 1 (pooled: empty); output element counts of 255, 256, 257 and 513 pooled (n...p)
# and unpooled (n...s); H < 3 and W < 3 (smoothed: all zeros); a pooled size of odd x odd (tmp_odd: both steps).
_POOL = {
    "quads_c1": ("uint8", lambda: _place(u8_quads(), 64, 96, 1, 255)),
    "quads_c2": ("uint8", lambda: _place(u8_quads(), 33, 65, 2, 255)),
    "quads_c3": ("uint8", lambda: _place(u8_quads(), 63, 95, 3, 255)),
    "quads_c5": ("uint8", lambda: _place(u8_quads(), 23, 41, 5, 255)),
    "fquads_c1": ("float32", lambda: _place(f32_quads(), 64, 96, 1, 7.0e37)),
    "fquads_c2": ("float32", lambda: _place(f32_quads(), 33, 65, 2, 7.0e37)),
    "fquads_c3": ("float32", lambda: _place(f32_quads(), 63, 95, 3, 7.0e37)),
    "fquads_c5": ("float32", lambda: _place(f32_quads(), 23, 41, 5, 7.0e37)),
    "all255": ("uint8", lambda: np.full((9, 11, 2), 255, np.uint8)),
    "ramps": ("uint8", lambda: _ramps(13, 18)),
    "cancel": ("float32", lambda: _cancel(10, 14, 3)),
    "nonfinite": ("float32", lambda: _nonfinite(9, 11)),
    "tmp_odd": ("uint8", lambda: _place(u8_quads()[::3], 30, 46, 3, 255)),
    "ftmp_odd": ("float32", lambda: _place(f32_quads()[136::2], 31, 47, 3, 7.0e37)),
}
for _dt, _q, _f in (("uint8", u8_quads, 255), ("float32", f32_quads, 7.0e37)):
    _p = "" if _dt == "uint8" else "f"
    for _n, (_h, _w) in {"n255p": (31, 35), "n256p": (32, 32), "n257p": (2, 514), "n513p": (38, 54), "n255s": (15, 17), "n256s": (16, 16),
                         "n257s": (1, 257), "n513s": (19, 27), "h1": (1, 40), "w1": (40, 1), "h2": (2, 7), "w2": (7, 2)}.items():
        _c = 2 if _n in ("h1", "w1") else 1
        if _h >= 2 and _w >= 2:
            _POOL[_p + _n] = (_dt, lambda q=_q, h=_h, w=_w, c=_c, f=_f: _place(q()[5::7], h, w, c, f))
        else:
            _POOL[_p + _n] = (_dt, lambda q=_q, h=_h, w=_w, c=_c: np.ascontiguousarray(q()[5::7].reshape(-1)[:h * w * c].reshape(h, w, c)))
POOL_CASES = list(_POOL)
CELLS = [(shrink, smooth) for shrink in (1, 2) for smooth in (0, 1)]
# the emulated wrong kernels and the arrays meant to catch each (cell: the (shrink, smooth) it is asked in)
POOL_FAULTS = {"nowrap": ((2, 0), ["quads_c1", "quads_c2", "quads_c3", "quads_c5", "tmp_odd", "n255p", "n256p", "n257p", "n513p"]),
               "rowfirst": ((2, 0), ["fquads_c1", "fquads_c2", "fquads_c3", "fquads_c5", "ftmp_odd"]),
               "pairwise": ((2, 0), ["fquads_c1", "fquads_c2", "fquads_c3", "fquads_c5", "ftmp_odd"]),
               "fp32_accumulate": ((1, 1), ["cancel"]),
               "separable": ((1, 1), ["cancel"]),
               "border_copied": ((1, 1), ["all255", "ramps", "cancel", "nonfinite", "quads_c3", "fquads_c3"])}


@functools.lru_cache(None)
def pool_case(name):
    """The array [H][W][C] of a case, read-only and shared."""
    dtype, build = _POOL[name]
    a = np.ascontiguousarray(build())
    assert a.dtype == np.dtype(dtype) and a.ndim == 3
    a.setflags(write=False)
    return a


def out_shape(arr, shrink):
    H, W, C = arr.shape
    return (H // 2, W // 2, C) if shrink == 2 else (H, W, C)


@functools.lru_cache(None)
def oracle_pool_smooth(name, shrink, smooth):
    """The oracle's avg_pool_2 (shrink 2) and smooth_image_3d (smooth 1) of a case; computed once."""
    x = pool_case(name)
    with np.errstate(all="ignore"):
        if shrink == 2:
            x = orc.avg_pool_2(x)
        if smooth:
            x = orc.smooth_image_3d(x)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def pool_wrong(arr, fault):
    """avg_pool_2 as a kernel with `fault` would compute it: nowrap (uint8: the sum is not taken mod 256), rowfirst
    ((a + c) + b) + d, pairwise (a + b) + (c + d)."""
    h, w = arr.shape[0] // 2, arr.shape[1] // 2
    a, b, c, d = arr[0:2 * h:2, 0:2 * w:2], arr[1:2 * h:2, 0:2 * w:2], arr[0:2 * h:2, 1:2 * w:2], arr[1:2 * h:2, 1:2 * w:2]
    if arr.dtype == np.uint8:
        assert fault == "nowrap"
        return ((a.astype(np.uint32) + b + c + d) >> 2).astype(np.uint8)
    with np.errstate(all="ignore"):
        s = ((a + c) + b) + d if fault == "rowfirst" else (a + b) + (c + d)
        return (s / 4).astype(arr.dtype)


def smooth_wrong(arr, fault):
    """smooth_image_3d as a kernel with `fault` would compute it: fp32_accumulate (the oracle's order in float32),
    separable (fp64: the 1-2-1 row pass, then the 1-2-1 column pass), border_copied (the border keeps the input)."""
    with np.errstate(all="ignore"):
        ref = orc.smooth_image_3d(arr)
        u, v = arr.shape[:2]
        if fault == "border_copied":
            out = arr.copy()
            if u >= 3 and v >= 3:
                out[1:u - 1, 1:v - 1] = ref[1:u - 1, 1:v - 1]
            return out
        out = np.zeros_like(arr)
        if u < 3 or v < 3:
            return out
        if fault == "separable":
            a = arr.astype(np.float64)
            rows = (a[:, :-2] + 2 * a[:, 1:-1]) + a[:, 2:]
            acc = (rows[:-2] + 2 * rows[1:-1]) + rows[2:]
        else:
            a = arr.astype(np.float32)
            two, four = np.float32(2), np.float32(4)
            sh = lambda dr, dc: a[1 + dr:u - 1 + dr, 1 + dc:v - 1 + dc]
            acc = sh(-1, -1) + two * sh(-1, 0)
            acc = acc + sh(-1, 1)
            acc = acc + two * sh(0, -1)
            acc = acc + four * sh(0, 0)
            acc = acc + two * sh(0, 1)
            acc = acc + sh(1, -1)
            acc = acc + two * sh(1, 0)
            acc = acc + sh(1, 1)
            assert acc.dtype == np.float32
        out[1:u - 1, 1:v - 1] = (acc / 16).astype(arr.dtype)
        return out


def describe_array_mismatch(got, ref, what):
    diff = np.argwhere(differing(got, ref))
    y, x, c = (int(i) for i in diff[0])
    return (f"{what}: {len(diff)} of {got.size} elements differ, first at (row {y}, column {x}, channel {c}) = {got[y, x, c]!r} against "
            f"{ref[y, x, c]!r}" + (" (border)" if y in (0, got.shape[0] - 1) or x in (0, got.shape[1] - 1) else ""))


def level_record(H, W, n_per_oct, l):
    """(WbLevel record [1], the plan) of level l of the shrink-1 plan of an H x W image, as PyramidPlan lays it out."""
    plan = PyramidPlan(H, W, 1, n_per_oct, 0)
    table, _ = plan.level_table()
    return np.ascontiguousarray(table[l:l + 1]), plan
