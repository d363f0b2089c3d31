"""Designed inputs for channels_gm_kernel (csrc/wb_chan_gm.hip: grad_mag on uint8 and float32 images): NumPy, the oracle and
the library's host-only entry points, no GPU, no torch.

With n_per_oct = 1 every level is the identity level of its octave (asserted through the oracle's own resize: levels_of),
so the steps after the resample see exactly the chosen pixels; the deeper octaves' bases are the oracle's pool of the
design (wrapping for uint8, fp32 for float32 images).  The one exception is `side4` (n_per_oct = 4), see below.  emulate()
restates the kernel: the pixels with a 6-pixel halo taken at the REFLECTED coordinate, the gradients and fp32 magnitudes
of the haloed tile (the oracle's own passes), the 11-tap triangle filter without borders over them -- fp64, scipy's
symmetric order, one fp32 rounding per pass, rows' axis first --, mag / (fp32(t) + eps) in fp32, the fp32 pool ((a + b) + c)
+ d, the oracle's smooth.  That the mirrored PIXELS give the mirrored magnitudes is the kernel's claim; the host test holds
it to the oracle, which mirrors the magnitudes.  WRONG_KERNELS are the mistakes a kernel could make, emulated the same way;
test_gradmag_designs_host.py asserts how many output pixels each gets wrong and test_gpu_gradmag_designs.py runs the designs
through the kernel bit for bit.

Designs (design_images(name, shrink): a tuple of images of at most two tile rows by two tile columns of the cell; the
tile comes from wb_channels_tile).  uint8 designs also run as float32 images of the same integers (BOTH_DTYPES)
  reflect  a ramp along x + y with another texture in each of the first and last six rows and columns, at TU S + d by
           TV S + d pixels, d = -S, 0, S, 2 S: an exact tile, bottom and right tiles of one and two output rows and columns
  side4    8 x 32, 32 x 8 and 8 x 8 pixels at n_per_oct = 4: the last level of the first octave has a side of exactly 4
           (rows only, columns only, both), the one size at which the 6-pixel halo is reflected more than once
  zero     flat fields with single pixels dented by one grey level, some further than the 11-tap window apart: mag = 0 and
           normaliser = 0 give exactly +0, and beside a dent the normaliser is of the order of eps
  unit     float32 noise in [0, 1], and blocky noise in [0, 2^-8] that fades to 0 towards the left
  tiny     float32 noise scaled by 2^-70 (every square gx^2 + gy^2 is subnormal or 0) and by 2^-80 (every square underflows
           to 0: the output is +0 everywhere)
  squares  uint8 noise of five contrasts: 7448 distinct sums gx^2 + gy^2 (the host test's SQUARES_REACHED)
  order    float32 images, constant along x, whose profile along y was searched (ORDER_PROFILES, search_order_profiles, not
           run at test time) so that the first triangle pass, summed in plain left-to-right order, rounds to another fp32
           than in scipy's symmetric order
  seams    noise whose contrast and grain differ in every quadrant around the tile seam, in both directions

Findings (asserted by the host test)
  * On uint8 images gx^2 + gy^2 <= 2 x 1020^2 < 2^24: every square and every sum is exact in fp32, so each output bit hangs
    on the square root and the division being correctly rounded.  `sqrt of an fp64 sum of squares` still differs there:
    the fp64 root rounded to fp32 is rounded twice.
  * For a level side n >= 5 one mirror followed by a clamp gives the pixels of the full reflection (the halo is 6 wide:
    at n = 5 coordinate -6 mirrors to 5 and clamps to 4, which is the reflection's own pixel); the count of
    `mirror_then_clamp` is 0 outside side4, and inside it at shrink 2 and 4 with the smooth on, where a level of 4 pixels
    pools to fewer than 3 rows and the smooth leaves all zeros.
  * The plain-order triangle sum changes no output pixel of any design but `order`, in any cell:
    the fp64 sums differ in their last bits, 29 bits below the fp32 rounding.
  * sqrt(fl(x x)) = |x| in fp32 when x x neither overflows nor falls into the subnormal range; images that are constant
    along one axis therefore have mag = |g| exactly, which is what lets the `order` search place fp32 magnitudes at will.
"""
import ctypes as C
import functools

import numpy as np

import u1_designs as ud
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat

SHRINKS = (1, 2, 4)
SMOOTHS = (0, 1)
DESIGNS = ("reflect", "side4", "zero", "unit", "tiny", "squares", "order", "seams")
BOTH_DTYPES = ("reflect", "side4", "zero", "seams")
N_PER_OCT = {"side4": 4}
NH = 5
EPS = np.float32(1e-3)
TRI = orc.triangle_kernel(NH)
BORDER_DELTAS = (-1, 0, 1, 2)
FLT_MIN = np.float32(2.0 ** -126)


@functools.lru_cache(None)
def tile_geom(shrink):
    tu, tv = C.c_int(), C.c_int()
    assert nat.load().wb_channels_tile(nat.WB_CHN_GRAD_MAG, shrink, C.byref(tu), C.byref(tv)) == 0
    return dict(S=shrink, TU=tu.value, TV=tv.value)


def levels_of(img, shrink, n_per_oct=1):
    """The resized pixels of every level, by the oracle's own plan and resize; at n_per_oct = 1 each is asserted to be its
    octave's image itself as long as the octave's sides are multiples of the shrink."""
    out = []
    plan = orc.level_plan(img.shape[0], img.shape[1], shrink, n_per_oct)
    bases = list(orc.image_octaves(img))
    for lv in plan:
        base = bases[lv["oct"]]
        px = orc.resize_bilinear(base, lv["nh"], lv["nw"])
        if n_per_oct == 1 and (lv["nh"], lv["nw"]) == base.shape:
            assert np.array_equal(px, base)
        out.append(px)
    return out


def is_identity(img, shrink, level):
    lv = orc.level_plan(img.shape[0], img.shape[1], shrink, 1)[level]
    return (lv["nh"], lv["nw"]) == (lv["h"], lv["w"])


# ------------------------------------------------------------------------------ the kernel, restated
def halo_index(n, mode, pad=NH + 1):
    """Level coordinate each tile coordinate -pad .. n + pad - 1 stands for."""
    i = np.arange(-pad, n + pad)
    if mode == "reflect":                        # scipy 'reflect': (d c b a | a b c d | d c b a), any number of times
        j = np.mod(i, 2 * n)
        return np.where(j >= n, 2 * n - 1 - j, j)
    if mode == "clamp":
        return np.clip(i, 0, n - 1)
    assert mode == "mirror_then_clamp"
    j = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
    return np.clip(j, 0, n - 1)


def magnitudes(px32, wrong=None, parts=False):
    gx, gy = orc.gradients(px32)
    if wrong == "sqrt_of_fp64_sum":
        mag = np.sqrt(gx.astype(np.float64) ** 2 + gy.astype(np.float64) ** 2).astype(np.float32)
    else:
        sx, sy = gx * gx, gy * gy
        if wrong == "squares_flushed":
            sx, sy = np.where(sx < FLT_MIN, np.float32(0), sx), np.where(sy < FLT_MIN, np.float32(0), sy)
        s = sx + sy
        if wrong == "squares_flushed":
            s = np.where(s < FLT_MIN, np.float32(0), s)
        mag = np.sqrt(s)
    return (mag, gx, gy) if parts else mag


def tri_pass(a, axis, order="symmetric"):
    """The 11-tap triangle filter over the inside of `a` along `axis` (10 shorter), fp64 result."""
    w = TRI.astype(np.float64)
    x = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n = x.shape[0] - 2 * NH
    if order == "symmetric":
        t = x[NH:NH + n] * w[NH]
        for jj in range(-NH, 0):
            t = t + (x[NH + jj:NH + jj + n] + x[NH - jj:NH - jj + n]) * w[NH + jj]
    else:
        t = x[0:n] * w[0]
        for j in range(1, 2 * NH + 1):
            t = t + x[j:j + n] * w[j]
    return np.moveaxis(t, 0, axis)


def normalised(px, wrong=None, parts=False):
    """mag / (triangle(mag) + eps) of one level, float32 [nh, nw]."""
    px32 = px.astype(np.float32)
    nh, nw = px32.shape
    if wrong == "mirror_of_magnitudes":
        # the level's own magnitudes, mirrored about the edge sample (d c b | a b c d | c b a): one off
        mg = np.pad(magnitudes(px32), NH, mode="reflect")
    else:
        mode = {"clamped_halo": "clamp", "mirror_then_clamp": "mirror_then_clamp"}.get(wrong, "reflect")
        halo = px32[halo_index(nh, mode)][:, halo_index(nw, mode)]
        mg = magnitudes(halo, wrong)[1:-1, 1:-1]                 # (the outermost ring has no neighbour: the kernel never forms it)
    order = "plain" if wrong == "plain_order" else "symmetric"
    first, second = (1, 0) if wrong == "other_axis_order" else (0, 1)
    t = tri_pass(mg, first, order)
    if wrong != "fp64_between_passes":
        t = t.astype(np.float32)
    t = tri_pass(t, second, order)
    mag = mg[NH:-NH, NH:-NH]
    with np.errstate(under="ignore"):
        if wrong == "eps_in_fp64":
            den = (t + np.float64(EPS)).astype(np.float32)
        else:
            den = t.astype(np.float32) + EPS
        out = mag * (np.float32(1) / den) if wrong == "reciprocal" else mag / den
    out = out.astype(np.float32)
    return (out, mag, t.astype(np.float32)) if parts else out


def pool2(ch, wrong=None):
    u, v = ch.shape[0] // 2 * 2, ch.shape[1] // 2 * 2
    a, b, c, d = ch[0:u:2, 0:v:2], ch[1:u:2, 0:v:2], ch[0:u:2, 1:v:2], ch[1:u:2, 1:v:2]
    with np.errstate(under="ignore"):
        s = (a + c) + (b + d) if wrong == "pool_pairs" else ((a + b) + c) + d
        return (s * np.float32(0.25)).astype(np.float32)


WRONG_KERNELS = ("clamped_halo", "mirror_then_clamp", "mirror_of_magnitudes", "fp64_between_passes", "other_axis_order", "plain_order",
                 "eps_in_fp64", "reciprocal", "sqrt_of_fp64_sum", "pool_pairs", "smooth_border_at_tile_edge", "squares_flushed")


def applies(wrong, shrink, smooth_on):
    if wrong == "pool_pairs":
        return shrink > 1
    if wrong == "smooth_border_at_tile_edge":
        return smooth_on == 1
    return True


def emulate(px, shrink, smooth_on, wrong=None):
    """One level of resized pixels `px` as the kernel (or a wrong kernel) computes it: float32 [u, v, 1]."""
    lv = normalised(px, wrong)
    for _ in range({1: 0, 2: 1, 4: 2}[shrink]):
        lv = pool2(lv, wrong)
    lv = lv[..., None]
    if smooth_on:
        with np.errstate(under="ignore"):
            lv = orc.smooth_image_3d(lv)
        if wrong == "smooth_border_at_tile_edge":
            # (the seams between tiles alone: what such a kernel stores on the level's own border depends on its halo)
            g = tile_geom(shrink)
            y, x = np.indices(lv.shape[:2])
            edge = (y % g["TU"] == 0) | (y % g["TU"] == g["TU"] - 1) | (x % g["TV"] == 0) | (x % g["TV"] == g["TV"] - 1)
            lv = np.where(edge[..., None], np.float32(0), lv)
    return lv


def oracle_level(px, shrink, smooth_on):
    with np.errstate(under="ignore"):
        lv = orc.grad_mag(px)
        for _ in range({1: 0, 2: 1, 4: 2}[shrink]):
            lv = orc.avg_pool_2(lv)
        return orc.smooth_image_3d(lv) if smooth_on else lv


# ------------------------------------------------------------------------------ designs
def _clip8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def base_shape(shrink):
    g = tile_geom(shrink)
    return shrink * 2 * g["TU"], shrink * (g["TV"] + 6)


def reflect_image(H, W, seed):
    """A ramp along x + y (no symmetry about any border) with noise of another contrast in each of the first and last six
    rows and columns."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = (40 + 3 * x + 5 * y) % 211
    for k in range(6):
        amp = 25 * (k + 1)
        img[k, :] = rng.integers(0, amp + 1, W) + 5 * k
        img[H - 1 - k, :] = 255 - rng.integers(0, amp + 1, W)
    for k in range(6):
        amp = 20 * (6 - k)
        img[6:H - 6, k] = rng.integers(0, amp + 1, max(H - 12, 0)) + 100
        img[6:H - 6, W - 1 - k] = 130 - rng.integers(0, amp + 1, max(H - 12, 0))
    return _clip8(img)


def reflect_images(shrink):
    g = tile_geom(shrink)
    return tuple(reflect_image(shrink * (g["TU"] + d), shrink * (g["TV"] + d), 80 + d) for d in BORDER_DELTAS)


def side4_images():
    return tuple(ud.noise_image(h, w, 90 + h + w, (255, 90)) for h, w in ((8, 32), (32, 8), (8, 8)))


def zero_image(H, W):
    """Flat at 100 (left) and 7 (right); dents of one grey level, densely in the upper half, 16 apart in the lower."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.where(x < W // 2, 100, 7)
    img[(y < H // 2) & (y % 5 == 2) & (x % 7 == 3)] -= 1
    img[(y >= H // 2) & (y % 16 == 8) & (x % 16 == 8)] += 1
    return _clip8(img)


def unit_images(H, W):
    rng = np.random.default_rng(101)
    a = rng.random((H, W), np.float32)
    b = (np.kron(rng.random((-(-H // 3), -(-W // 3)), np.float32), np.ones((3, 3), np.float32))[:H, :W] * np.float32(2.0 ** -8)).astype(np.float32)
    # (fading to 0 towards the left: normalisers from 8 eps down to below eps)
    b = (b * (np.arange(W, dtype=np.float32) / np.float32(W))[None, :]).astype(np.float32)
    return a, b


def tiny_images(H, W):
    rng = np.random.default_rng(102)
    a = rng.random((H, W), np.float32)
    return a * np.float32(2.0 ** -70), a * np.float32(2.0 ** -80)


def squares_image(H, W):
    return ud.noise_image(H, W, 103, (255, 100, 30, 8, 2))


# float32 bit patterns of f(c - 5), f(c - 1), f(c + 3) of the first profiles search_order_profiles found: 216 hits in 2000
# trials (seed 0); every other row of a profile is 0
ORDER_PROFILES = ("2b370b16 4068193d 369fc4df", "2aa353b1 40cec4f0 3618ec4e", "2bd504e0 4139a4b8 370fe5fe",
                  "29328b48 3e43c080 340f87a5", "27c27588 3f71e969 358f9714", "26a603d2 3ef6ece3 320a964c")


ORDER_ROWS, ORDER_CENTRE = 24, 12


def order_profile(B, up, a=None, b=None):
    """f(y), float32 [ORDER_ROWS]: three lone samples, so that |gy| (= mag: the image is constant along x) is B at rows
    c - 2 and c, a at c + 2 and c + 4, b at c - 6 and c - 4, and 0 elsewhere.  The window centred on c then sums
    B (w5 + w3) + a (w3 + w1) + b w1; a and b are solved in exact arithmetic so that this lies within 2^-70 of the midpoint
    between two fp32 numbers `up` halves of an ulp above B (w5 + w3): B, a and b are 2^23 and 2^47 apart, the fp64 sums are
    inexact, and whether the fp64 result falls on, above or below the midpoint is a matter of the order."""
    from fractions import Fraction
    w = [Fraction(float(v)) for v in TRI]
    c = ORDER_CENTRE
    if a is None:
        M = Fraction(float(B)) * (w[5] + w[3])
        lo = np.float32(float(M))
        lo = lo if Fraction(float(lo)) <= M else np.nextafter(lo, np.float32(0))
        ulp = Fraction(float(np.nextafter(lo, np.float32(np.inf)))) - Fraction(float(lo))
        T = Fraction(float(lo)) + ulp * (2 * up + 1) / 2
        a = np.float32(float((T - M) / (w[3] + w[1])))
        a = a if Fraction(float(a)) * (w[3] + w[1]) <= T - M else np.nextafter(a, np.float32(0))
        b = np.float32(float((T - M - Fraction(float(a)) * (w[3] + w[1])) / w[1]))
    f = np.zeros(ORDER_ROWS, np.float32)
    f[c - 1], f[c + 3], f[c - 5] = np.float32(B) / 4, np.float32(a) / 4, np.float32(b) / 4
    return f


def search_order_profiles(n_trials=2000, seed=0, want=6):
    """Profiles of order_profile's family on which the plain-order first pass changes the output at the centre row (not run
    at test time).  Returns (hex strings, hits, trials)."""
    rng = np.random.default_rng(seed)
    found, hits = [], 0
    for _ in range(n_trials):
        B = np.float32(rng.uniform(1, 2) * 2.0 ** int(rng.integers(-2, 6)))
        f = order_profile(B, int(rng.integers(0, 8)))
        img = np.repeat(f[:, None], 8, 1)
        ref, got = normalised(img), normalised(img, "plain_order")
        if ref[ORDER_CENTRE, 4].view(np.uint32) != got[ORDER_CENTRE, 4].view(np.uint32):
            hits += 1
            if len(found) < want:
                found.append(" ".join(f"{v:08x}" for v in f.view(np.uint32)[[ORDER_CENTRE - 5, ORDER_CENTRE - 1, ORDER_CENTRE + 3]]))
    return found, hits, n_trials


def order_images(W):
    out = []
    for p in ORDER_PROFILES:
        f = np.zeros(ORDER_ROWS, np.float32)
        f[[ORDER_CENTRE - 5, ORDER_CENTRE - 1, ORDER_CENTRE + 3]] = np.array([int(h, 16) for h in p.split()], np.uint32).view(np.float32)
        out.append(np.repeat(f[:, None], W, 1))
    return tuple(out)


@functools.lru_cache(None)
def design_images(name, shrink):
    H, W = base_shape(shrink)
    if name == "reflect":
        return reflect_images(shrink)
    if name == "side4":
        return side4_images()
    if name == "zero":
        return (zero_image(H, W),)
    if name == "unit":
        return unit_images(H, W)
    if name == "tiny":
        return tiny_images(H, W)
    if name == "squares":
        return (squares_image(H, W),)
    if name == "order":
        return order_images(8 * shrink)
    assert tile_geom(shrink) == ud.tile_geom("grad_hist_4_u1", shrink)
    return (ud.seams_image(H, W, shrink),)


def cases(shrink):
    """(design, index, image) with the uint8 designs of BOTH_DTYPES once more as float32 images."""
    out = []
    for d in DESIGNS:
        for i, img in enumerate(design_images(d, shrink)):
            out.append((d, i, img))
            if d in BOTH_DTYPES:
                out.append((d, f"{i}f", img.astype(np.float32)))
    return out


# ------------------------------------------------------------------------------ failure messages
def describe_mismatch(got, ref, img, name, shrink, smooth_on, level=0):
    """Names the first differing output pixel, its tile, and the restated magnitudes and normalisers of its block."""
    diff = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
    r, c = (int(v) for v in diff[0])
    g = tile_geom(shrink)
    msg = (f"level {level}: {len(diff)} output pixels differ, first at ({r}, {c}) channel 0: {got[r, c, 0]!r} against {ref[r, c, 0]!r}, "
           f"tile ({r // g['TU']}, {c // g['TV']}), row {r % g['TU']} column {c % g['TV']} of it")
    px = levels_of(img, shrink, N_PER_OCT.get(name, 1))[level]
    out, mag, nrm = normalised(px, parts=True)
    blk = np.s_[shrink * r:shrink * (r + 1), shrink * c:shrink * (c + 1)]
    return msg + (f"; level of {px.shape[0]} x {px.shape[1]} pixels; of its own block: mag {mag[blk].tolist()}, triangle {nrm[blk].tolist()}, "
                  f"mag / (triangle + eps) {out[blk].tolist()}")
