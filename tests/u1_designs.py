"""Designed inputs for step 2 and step 3 of channels_u1_kernel (csrc/wb_chan_u1.hip: grad_hist_4_u1, NCH = 4, and
grad_mag_u1, NCH = 1): NumPy, the oracle and the library's host-only entry points, no GPU, no torch.

With n_per_oct = 1 every level is the identity level of its octave (gradient_designs.identity_levels asserts it through
the oracle), so the steps after the resample see exactly the chosen pixels; the deeper octaves' bases are the oracle's
wrapping uint8 pool of the design.  Step 2 and step 3 are restated in int64: the two Sobel stencils with numba's zero
ring, the channel values |dx| >> 2, |dx - dy| >> 3, |dy| >> 2, |dx + dy| >> 3 (or max(|dx|, |dy|) >> 2), the pool
((a + b + c + d) & 255) >> 2 once or twice, the smooth (nine-term sum) >> 4 with its zero border.  WRONG_KERNELS are the
mistakes a kernel could make, emulated the same way; test_u1_designs_host.py asserts how many output pixels each gets
wrong on every design and cell it applies to, and test_gpu_u1_designs.py runs the designs through the kernels bit for bit.

Designs (design_images(name, shrink): a tuple of uint8 images of at most two tile rows by two tile columns of the cell;
the tile comes from wb_channels_tile)
  values   0 / 255 steps, stripes and corners; ramps whose slope (0 .. 40) changes every column, every row and every
           diagonal; seeded noise of four contrasts; 0 / 255 noise with three pixels in ten drawn afresh.  Every quotient gets both sides (4 m - 1 and 4 m, 8 m - 1 and 8 m) of
           the multiples the host test counts (QUOTIENT_SIDES), up to the attained maxima 255 / 191, and 14794 distinct (dx, dy)
  wrap     a mosaic of 4 x 4 patches (WRAP_PATCHES, found by search_wrap_patches, not run at test time) whose centre 2 x 2
           block has a channel sum of exactly 255, 256, 257, 511, 512, 767, 768 or 1020, and bands of triangle waves of
           slope 32 / 64 / 96 along x, y, x + y and x - y, where whole runs of neighbouring blocks sum to 256, 512 and 768:
           the 4 x 4 blocks of shrink 4 made of four wrapping 2 x 2 blocks (the host test's WRAP_BLOCKS_4; a patch of the
           mosaic is one 2 x 2 block of its 4 x 4 block)
  border   0 / 255 texture in the outermost two rows and columns of a level of TU S + d by TV S + d pixels, d = -S, 0, S,
           2 S: an exact tile, bottom and right tiles of one and two output rows and columns, a last tile row cut short
  seams    noise whose contrast and grain differ in every quadrant around the tile seam, in both directions
  smooth   period-4 square waves of 0 / 255 along x, y and the diagonals (channel values of 255 in whole windows: nine-term
           sums of 4080 at shrink 1) beside ramps and noise: windows with sums of 16 k - 1, 16 k and 16 k + 1
           (the host test's SMOOTH_SIDES), neighbouring channels with different values and sums above 255
  tiny     levels of 8, 9 and 10 pixels on one axis (those that are a multiple of the shrink) and wide on the other

Findings (asserted by the host test)
  * dx - dy = 2 (p01 + p02 + p12 - p10 - p20 - p21) and dx + dy likewise: both are even and at most 1530, so trunc and
    floor of the half never differ, channels 1 and 3 never exceed 191 and the clamp to 255 never acts (|dx|, |dy| <= 1020
    gives 255 at most in channels 0 and 2 as well).
  * A block sum of channel 1 or 3 is at most 764: those channels wrap at most twice and never reach 767, 768 or 1020.
    The search found no block of channel 1 or 3 summing to more than WRAP_MAX_13; WRAP_MISSING lists what it did not reach.
  * The second pooling stage of shrink 4 never wraps: first-stage values are at most 63, the sum at most 252.
  * A level side is a multiple of the shrink, so the bottom and right ring is always the LAST pixel of its block, and the
    first pixel of a tile only at shrink 1 (side TU + 1).  A ring off by one at the bottom therefore shows at every shrink,
    but only in the last block row.
  * With n_per_oct = 1 a level has at least 8 pixels a side, so a level with fewer than 3 pooled rows -- where the smooth
    leaves all zeros -- exists at shrink 4 alone (8 pixels: 2 rows).
  * At shrink 2 and 4 the smooth's nine-term sum is at most 16 * 63 = 1008; sums above 255 per channel -- a carry from
    byte to byte of a packed sum -- exist at every shrink.
  * At shrink 1 the level's border is the gradients' zero ring itself: a smooth border applied with the smooth off changes
    nothing there (it shows at shrink 2 and 4, where a border block pools pixels inside the ring).
  * grad_mag_u1 as min(|dx|, |dy|) is right wherever |dx| >> 2 == |dy| >> 2: the designs' pure diagonals do not show it.
"""
import ctypes as C
import functools

import numpy as np

import gradient_designs as gd
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat

FUNCS = {"grad_hist_4_u1": nat.WB_CHN_GRAD_HIST_4_U1, "grad_mag_u1": nat.WB_CHN_GRAD_MAG_U1}
SHRINKS = (1, 2, 4)
SMOOTHS = (0, 1)
DESIGNS = ("values", "wrap", "border", "seams", "smooth", "tiny")
WRAP_TARGETS = (255, 256, 257, 511, 512, 767, 768, 1020)
BORDER_DELTAS = (-1, 0, 1, 2)                      # in units of the shrink


@functools.lru_cache(None)
def tile_geom(func, shrink):
    tu, tv = C.c_int(), C.c_int()
    assert nat.load().wb_channels_tile(FUNCS[func], shrink, C.byref(tu), C.byref(tv)) == 0
    return dict(S=shrink, TU=tu.value, TV=tv.value)


def same_tiles():
    """Both integer functions share one tile per shrink (the designs are built once for both)."""
    return all(tile_geom("grad_hist_4_u1", s) == tile_geom("grad_mag_u1", s) for s in SHRINKS)


# ------------------------------------------------------------------------------ step 2, restated
def sobel_open(img):
    """(dx, dy) in int64 at EVERY pixel, the coordinates outside the level clamped as step 1 of the kernel clamps them."""
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    hv = p[:-2, :] + 2 * p[1:-1, :] + p[2:, :]
    hh = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    return hv[:, 2:] - hv[:, :-2], hh[2:, :] - hh[:-2, :]


def ring_mask(shape, bottom=1):
    """True on numba's 1-pixel ring; bottom=0: the bottom row and right column left out (`>= nh` for `>= nh - 1`)."""
    m = np.zeros(shape, bool)
    m[0, :] = m[:, 0] = True
    if bottom:
        m[-1, :] = m[:, -1] = True
    return m


def sobel_ring(img, wrong=None, geom=None):
    """The gradients as the kernel forms them (asserted equal to the oracle's stencils), or as a wrong kernel would."""
    dx, dy = sobel_open(img)
    ring = ring_mask(img.shape)
    if wrong is None:
        dx, dy = np.where(ring, 0, dx), np.where(ring, 0, dy)
        ox, oy = orc._sobel_int(img)
        assert np.array_equal(dx, ox) and np.array_equal(dy, oy)
        return dx, dy
    if wrong == "no_ring":
        return dx, dy
    if wrong == "ring_at_tile_edge":
        y, x = np.indices(img.shape)
        ph, pw = geom["S"] * geom["TU"], geom["S"] * geom["TV"]
        ring = (y % ph == 0) | (y % ph == ph - 1) | (x % pw == 0) | (x % pw == pw - 1)
    elif wrong == "ring_off_by_one":
        ring = ring_mask(img.shape, bottom=0)
    elif wrong == "dx_zeroed_only":
        return np.where(ring, 0, dx), dy
    return np.where(ring, 0, dx), np.where(ring, 0, dy)


def channel_values(dx, dy, func, wrong=None):
    """int64 [H, W, NCH]."""
    ax, ay = np.abs(dx), np.abs(dy)
    if func == "grad_mag_u1":
        m = {"gm_half_sum": (ax + ay) // 2, "gm_min": np.minimum(ax, ay)}.get(wrong, np.maximum(ax, ay))
        return (m >> 2)[..., None]
    return np.stack([ax >> 2, np.abs(dx - dy) >> 3, ay >> 2, np.abs(dx + dy) >> 3], -1)


def block_sums(ch):
    u, v = ch.shape[0] // 2 * 2, ch.shape[1] // 2 * 2
    return ch[0:u:2, 0:v:2] + ch[1:u:2, 0:v:2] + ch[0:u:2, 1:v:2] + ch[1:u:2, 1:v:2]


def pool2(ch, wrong=None):
    s = block_sums(ch)
    if wrong == "pool_no_wrap":
        return s >> 2
    if wrong == "pool_rounded":
        return ((s & 255) + 2) >> 2
    return (s & 255) >> 2


def pool(ch, shrink, wrong=None):
    if shrink == 4 and wrong == "pool4_once":
        u, v = ch.shape[0] // 4, ch.shape[1] // 4
        s = ch[:4 * u, :4 * v].reshape(u, 4, v, 4, -1).sum(axis=(1, 3))
        return (s & 255) >> 4
    for _ in range({1: 0, 2: 1, 4: 2}[shrink]):
        ch = pool2(ch, wrong)
    return ch


# ------------------------------------------------------------------------------ step 3, restated
def window_sums(lv):
    """Nine-term sums of the interior windows, int64 [u - 2, v - 2, NCH]."""
    u, v = lv.shape[:2]
    sh = lambda r, c: lv[1 + r:u - 1 + r, 1 + c:v - 1 + c]
    return (sh(-1, -1) + 2 * sh(-1, 0) + sh(-1, 1) + 2 * sh(0, -1) + 4 * sh(0, 0) + 2 * sh(0, 1) + sh(1, -1) + 2 * sh(1, 0) + sh(1, 1))


def smooth(lv, wrong=None, geom=None):
    u, v, nch = lv.shape
    out = np.zeros_like(lv)
    if wrong == "smooth_border_at_tile_edge":
        # (outside the level the kernel's halo holds zeros: those blocks lie on or beyond the ring)
        full = window_sums(np.pad(lv, ((1, 1), (1, 1), (0, 0)))) >> 4
        y, x = np.indices((u, v))
        edge = (y % geom["TU"] == 0) | (y % geom["TU"] == geom["TU"] - 1) | (x % geom["TV"] == 0) | (x % geom["TV"] == geom["TV"] - 1)
        return np.where(edge[..., None], 0, full)
    if u < 3 or v < 3:
        return out
    s = window_sums(lv)
    if wrong == "smooth_rounded":
        o = (s + 8) >> 4
    elif wrong == "smooth_packed" and nch == 4:
        # the nine words summed as 32-bit integers, every channel cut out of the packed sum: the lower bytes' carries ride along
        packed = sum(s[..., k] << (8 * k) for k in range(4)) & 0xFFFFFFFF
        o = np.stack([(packed >> (8 * k + 4)) & 255 for k in range(4)], -1)
    else:
        o = s >> 4
    out[1:-1, 1:-1] = o
    return out


WRONG_KERNELS = ("no_ring", "ring_at_tile_edge", "ring_off_by_one", "dx_zeroed_only", "pool_no_wrap", "pool_rounded", "pool4_once",
                 "smooth_rounded", "smooth_packed", "smooth_border_at_tile_edge", "smooth_border_without_smooth", "gm_half_sum", "gm_min")


def applies(wrong, func, shrink, smooth_on):
    if wrong in ("pool_no_wrap", "pool_rounded"):
        return shrink > 1
    if wrong == "pool4_once":
        return shrink == 4
    if wrong in ("smooth_rounded", "smooth_border_at_tile_edge"):
        return smooth_on == 1
    if wrong == "smooth_packed":
        return smooth_on == 1 and func == "grad_hist_4_u1"
    if wrong == "smooth_border_without_smooth":
        return smooth_on == 0
    if wrong.startswith("gm_"):
        return func == "grad_mag_u1"
    return True


def emulate(img, func, shrink, smooth_on, wrong=None):
    """One level of pixels `img` as the kernel (or a wrong kernel) computes it: uint8 [u, v, NCH]."""
    g = tile_geom(func, shrink)
    dx, dy = sobel_ring(img, wrong if wrong in ("no_ring", "ring_at_tile_edge", "ring_off_by_one", "dx_zeroed_only") else None, g)
    lv = pool(channel_values(dx, dy, func, wrong), shrink, wrong)
    if smooth_on:
        lv = smooth(lv, wrong, g)
    elif wrong == "smooth_border_without_smooth":
        lv = np.where(ring_mask(lv.shape[:2])[..., None], 0, lv)
    assert lv.min() >= 0 and lv.max() <= 255
    return lv.astype(np.uint8)


def oracle_level(img, func, shrink, smooth_on):
    lv = orc.CHANNEL_FUNCS[func](img)
    for _ in range({1: 0, 2: 1, 4: 2}[shrink]):
        lv = orc.avg_pool_2(lv)
    return orc.smooth_image_3d(lv) if smooth_on else lv


def intermediates(img, func, shrink):
    """What a failure message and the host test ask about a level: gradients, channel values, first-stage block sums,
    the shrunk level and its window sums."""
    dx, dy = sobel_ring(img)
    ch = channel_values(dx, dy, func)
    lv = pool(ch, shrink)
    return dict(dx=dx, dy=dy, ch=ch, sums=block_sums(ch) if shrink > 1 else None, level=lv,
                windows=window_sums(lv) if min(lv.shape[:2]) >= 3 else None)


# ------------------------------------------------------------------------------ designs
def _clip8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def base_shape(shrink):
    """(H, W) of two tile rows by two tile columns (the second column 6 outputs wide)."""
    g = tile_geom("grad_hist_4_u1", shrink)
    return shrink * 2 * g["TU"], shrink * (g["TV"] + 6)


def _fold(f):
    f = f % 510
    return np.where(f > 255, 510 - f, f)


def _varying(n, rng, hi):
    return _fold(np.cumsum(rng.integers(0, hi + 1, n)))


def noise_image(H, W, seed, contrasts=(255, 60, 12, 3)):
    """Vertical bands of seeded noise, one per contrast, each around its own grey level."""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W), np.int64)
    q = -(-W // len(contrasts))
    for i, c in enumerate(contrasts):
        lo = int(rng.integers(0, 256 - c))
        img[:, i * q:(i + 1) * q] = lo + rng.integers(0, c + 1, (H, min(q, W - i * q)))
    return _clip8(img)


def values_images(H, W):
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(21)
    f, g, d = _varying(W, rng, 40), _varying(H, rng, 40), _varying(H + W + 1, rng, 40)
    ramps = np.where(x < W // 3, f[x] // 2 + g[y] // 2, np.where(x < 2 * W // 3, d[x + y], d[x - y + H]))
    hard = np.where(rng.random((H, W)) < 0.3, rng.integers(0, 256, (H, W)), 255 * rng.integers(0, 2, (H, W)))
    return gd.extremes_image(H, W), _clip8(ramps), noise_image(H, W, 22), _clip8(hard)


# 4 x 4 pixel patches (two hex digits per pixel, row-major) whose centre 2 x 2 block has a channel sum of exactly the
# target, keyed "channel:target" (channel 4 stands for grad_mag_u1's only channel): the first patch search_wrap_patches found
WRAP_PATCHES = dict(p.split("=") for p in (
    "0:1020=ff0000ffff0000ffff0000ffff0000ff 0:255=c7d3f248d73c777ad61a0b145a7f50d8 0:256=00584b1c9f00ffffff0000000064ffff "
    "0:257=6ec1962c0470c1975e006ebfb8610471 0:511=92af440292b3420293b0420094b34103 0:512=5cc0ddf7045cc3dd03035fc01f00065d "
    "0:767=ffffa900ffff0000ffcc000053ffffff 0:768=07ffff000000ffff0000ffb1000000ff 1:255=92af440292b3420293b0420094b34103 "
    "1:256=00ff4400eeff4e36ffff9a00ff000000 1:257=6ec1962c0470c1975e006ebfb8610471 1:511=7dc2ffff137cc5ff02117fc47400117d "
    "1:512=98280025ed982900d5ec9826ffd7ec98 2:1020=ffffffffffffffff0000000000000000 2:255=b7f197ecef96ee9496f09322ed912100 "
    "2:256=140010350011366110365f76376272be 2:257=6ec1962c0470c1975e006ebfb8610471 2:511=ffffff5500008d07ee00ffff5cfffff7 "
    "2:512=002d00ff6c00ffff00ffffffffffff00 2:767=f2feed0000000000ff33000000ffffed 2:768=ceffff00ff00000000004d00fff3ff52 "
    "3:255=ffbcff00008f00ff0000000000ff0000 3:256=430d02830e0081640384668381628089 3:257=9cb4418eb3458c13438b11178e121500 "
    "3:511=ffffff99ffff9a5bff9c5b039b58002b 3:512=003a2a843b2a82f32d83f6ff82f6feff 4:1020=ffffffffffffffff0000000000000000 "
    "4:255=ffa5ff00830000ffff22ff005900fb00 4:256=00584b1c9f00ffffff0000000064ffff 4:257=ec16f423a6feb230e95ababe1f46a2de "
    "4:511=92af440292b3420293b0420094b34103 4:512=5cc0ddf7045cc3dd03035fc01f00065d 4:767=f2feed0000000000ff33000000ffffed "
    "4:768=ceffff00ff00000000004d00fff3ff52 "
).split())
WRAP_MISSING = ("1:767", "1:768", "1:1020", "3:767", "3:768", "3:1020")
WRAP_MAX_13 = 637                                 # (30 rounds of 200000 patches)


def patch_array(s):
    return np.array([int(s[i:i + 2], 16) for i in range(0, 32, 2)], np.int64).reshape(4, 4)


def centre_sums(p):
    """p int64 [n, 4, 4] -> block sums of the centre 2 x 2 block, [n, 5]: grad_hist_4_u1's channels, then grad_mag_u1's."""
    hv = p[:, :-2, :] + 2 * p[:, 1:-1, :] + p[:, 2:, :]
    hh = p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:]
    dx, dy = hv[:, :, 2:] - hv[:, :, :-2], hh[:, 2:, :] - hh[:, :-2, :]
    ch = np.concatenate([channel_values(dx, dy, "grad_hist_4_u1"), channel_values(dx, dy, "grad_mag_u1")], -1)
    return ch.sum(axis=(1, 2))


def search_wrap_patches(rounds=40, n=200000):
    """{"channel:target": patch}, the largest sums seen in channels 1 and 3 (not run at test time).  Families: uniform
    noise; 0 / 255 with some pixels drawn afresh; a column, row or diagonal profile plus noise of +-2."""
    found, top = {}, 0
    y, x = np.mgrid[0:4, 0:4]
    axes = np.stack([x, y, x + y, x - y + 3])
    for rnd in range(rounds):
        rng = np.random.default_rng(rnd)
        kind = rng.integers(0, 3, n)[:, None, None]
        uni = rng.integers(0, 256, (n, 4, 4))
        binary = np.where(rng.random((n, 4, 4)) < 0.25, uni, 255 * rng.integers(0, 2, (n, 4, 4)))
        prof = np.cumsum(rng.integers(-128, 129, (n, 7)), 1)
        prof = np.take_along_axis(prof, axes[rng.integers(0, 4, n)].reshape(n, 16), 1).reshape(n, 4, 4) + rng.integers(-2, 3, (n, 4, 4))
        prof -= prof.min(axis=(1, 2), keepdims=True)
        p = np.clip(np.where(kind == 0, uni, np.where(kind == 1, binary, prof)), 0, 255)
        s = centre_sums(p)
        top = max(top, int(s[:, 1].max()), int(s[:, 3].max()))
        for k in range(5):
            for t in WRAP_TARGETS:
                hit = np.nonzero(s[:, k] == t)[0]
                if hit.size:
                    found.setdefault(f"{k}:{t}", "".join(f"{v:02x}" for v in p[hit[0]].ravel()))
    return found, top


def mosaic_image(H, W):
    """The patches on a grid of stride 4, each with its centre block on even coordinates, over mid grey."""
    img = np.full((H, W), 128, np.int64)
    slots = [(r, c) for r in range(1, H - 4, 4) for c in range(1, W - 4, 4)]
    assert len(slots) >= len(WRAP_PATCHES)
    for (r, c), key in zip(slots, sorted(WRAP_PATCHES)):
        img[r:r + 4, c:c + 4] = patch_array(WRAP_PATCHES[key])
    return _clip8(img)


def mosaic_slots(H, W):
    """{key: (block row, block column)} of the 2 x 2 blocks that hold the patches' centres."""
    slots = [(r, c) for r in range(1, H - 4, 4) for c in range(1, W - 4, 4)]
    return {key: ((r + 1) // 2, (c + 1) // 2) for (r, c), key in zip(slots, sorted(WRAP_PATCHES))}


def waves_image(H, W):
    """Four bands of triangle waves of slope 32, 64 and 96 per pixel (a third of the width each) along x, y, x + y and
    x - y: block sums of 8 x slope = 256, 512, 768 in channel 0 (2, 3 and 1) away from the waves' turning points, and a
    0 / 255 step every 2 pixels in the last columns (1020)."""
    y, x = np.mgrid[0:H, 0:W]
    slope = np.select([x < W // 3, x < 2 * W // 3], [32, 64], 96)
    q = H // 4
    t = np.select([y < q, y < 2 * q, y < 3 * q], [x, y, x + y], x - y + H)
    img = _fold(slope * t)
    img[:, W - 8:] = np.where((x[:, W - 8:] // 2) % 2 == 0, 255, 0)
    return _clip8(img)


def wrap_images(H, W):
    return mosaic_image(H, W), waves_image(H, W)


def border_image(H, W, seed):
    """A gentle ramp with 0 / 255 texture (grain 1 and 2) in the outermost two rows and columns."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = (60 + 2 * x + 3 * y) % 200
    tex = 255 * np.kron(rng.integers(0, 2, (-(-H // 2), -(-W // 2))), np.ones((2, 2), np.int64))[:H, :W]
    tex ^= 255 * ((x + y) % 2) * (rng.integers(0, 2, (H, W)))
    edge = (y < 2) | (x < 2) | (y >= H - 2) | (x >= W - 2)
    return _clip8(np.where(edge, tex, img))


def border_images(shrink):
    g = tile_geom("grad_hist_4_u1", shrink)
    return tuple(border_image(shrink * (g["TU"] + d), shrink * (g["TV"] + d), 30 + d) for d in BORDER_DELTAS)


def seams_image(H, W, shrink):
    """Noise of another contrast and grain in each quadrant around the seam of tile (0, 0) with its neighbours."""
    g = tile_geom("grad_hist_4_u1", shrink)
    rng = np.random.default_rng(41)
    y, x = np.mgrid[0:H, 0:W]
    quad = 2 * (y >= shrink * g["TU"]) + (x >= shrink * g["TV"])
    img = np.zeros((H, W), np.int64)
    for qd, (c, grain) in enumerate(((255, 1), (90, 2), (200, 3), (30, 1))):
        t = np.kron(rng.integers(0, c + 1, (-(-H // grain), -(-W // grain))), np.ones((grain, grain), np.int64))[:H, :W]
        img = np.where(quad == qd, t + 10 * qd, img)
    return _clip8(img)


def smooth_images(H, W):
    y, x = np.mgrid[0:H, 0:W]
    sq = lambda t: np.where((t // 2) % 2 == 0, 255, 0)
    q = W // 4
    waves = np.select([x < q, x < 2 * q, x < 3 * q], [sq(x), sq(y), sq(x + y)], sq(x - y + H))
    rng = np.random.default_rng(51)
    mixed = np.where(y < H // 2, _varying(W, rng, 25)[x] // 2 + _varying(H, rng, 25)[y] // 2, noise_image(H, W, 52, (255, 120, 40, 9)))
    return _clip8(waves), _clip8(mixed)


def tiny_sides(shrink):
    return tuple(n for n in (8, 9, 10) if n % shrink == 0)


def tiny_images(shrink):
    H, W = base_shape(shrink)
    out = []
    for n in tiny_sides(shrink):
        out += [noise_image(n, W, 60 + n, (255, 40)), noise_image(H, n, 70 + n, (255,))]
    return tuple(out)


@functools.lru_cache(None)
def design_images(name, shrink):
    H, W = base_shape(shrink)
    if name == "values":
        return values_images(H, W)
    if name == "wrap":
        return wrap_images(H, W)
    if name == "border":
        return border_images(shrink)
    if name == "seams":
        return (seams_image(H, W, shrink),)
    if name == "smooth":
        return smooth_images(H, W)
    return tiny_images(shrink)


def cases(shrink):
    return [(d, i) for d in DESIGNS for i in range(len(design_images(d, shrink)))]


def levels_of(img, shrink):
    """The identity levels of a design (the image and the deeper octaves that are whole multiples of the shrink)."""
    return gd.identity_levels(img, shrink)


# ------------------------------------------------------------------------------ failure messages
def describe_mismatch(got, ref, img, func, shrink, smooth_on, level=0):
    """Names the first differing output pixel, its tile and channel, and -- on an identity level -- the restated values under it."""
    diff = np.argwhere(got != ref)
    r, c, k = (int(v) for v in diff[0])
    g = tile_geom(func, shrink)
    msg = (f"level {level}: {len(np.unique(diff[:, :2], axis=0))} output pixels differ, first at ({r}, {c}) channel {k}: {int(got[r, c, k])} "
           f"against {int(ref[r, c, k])}, tile ({r // g['TU']}, {c // g['TV']}), row {r % g['TU']} column {c % g['TV']} of it")
    lv = levels_of(img, shrink)
    if level < len(lv):
        m = intermediates(lv[level], func, shrink)
        h = 1 if smooth_on else 0
        u, v = m["level"].shape[:2]
        win = np.s_[max(r - h, 0):min(r + h + 1, u), max(c - h, 0):min(c + h + 1, v)]
        msg += f"; shrunk values of the channel under it {m['level'][win][..., k].tolist()}"
        if smooth_on and m["windows"] is not None and 0 < r < u - 1 and 0 < c < v - 1:
            msg += f", window sum {int(m['windows'][r - 1, c - 1, k])}"
        px = np.s_[shrink * r:shrink * (r + 1), shrink * c:shrink * (c + 1)]
        msg += f"; dx {m['dx'][px].tolist()}, dy {m['dy'][px].tolist()} of its own block"
        if shrink > 1:
            s2 = np.s_[(shrink // 2) * r:(shrink // 2) * (r + 1), (shrink // 2) * c:(shrink // 2) * (c + 1)]
            msg += f", first-stage sums {m['sums'][s2][..., k].tolist()}"
    return msg
