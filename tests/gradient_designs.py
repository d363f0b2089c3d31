"""Designed gradients for step 2 and step 3 of channels_kernel (csrc/wb_channels.hip): NumPy and the library's host-only
entry points, no GPU, no torch.

With n_per_oct = 1 every level is the identity level of its octave (asserted through the oracle: identity_levels), so
step 2 sees exactly the pixels the test chose.  On uint8 pixels the Sobel gradients are integers; from (gx, gy) alone
every pixel has, per channel k = 1, 2, 3, one of three classes

  Z  the oracle's value is exactly 0
  R  a residue of the fp64 projection: 1e-16 .. 2e-13 (channel 1: gx == gy != 0 and RN64(gx c1) != RN64(gx s1); channel 3
     the same with gx == -gy; channel 2: gy == 0 != gx, the value fp32(|gx| cos(pi/2)))
  O  an ordinary value: an integer, or fp32(d sin(pi/4)) >= 0.7071

and a 2 x 2 block read in pooling order a, b, c, d = (0,0), (1,0), (0,1), (1,1) is a word of {Z,R,O}^4.  classify()
derives the classes in int64 arithmetic, restates project_int / project_ordinary / the redo condition / the pool / both
forms of the smooth in NumPy (every fp32 fma emulated through fp64 with a check that the double rounding cannot show),
and per tile says whether the workgroup flag `odd_values` is raised and whether the two forms of the smooth differ in an
output pixel of that tile (`separating`).  WRONG_KERNELS are the mistakes a kernel could make, emulated the same way;
test_gradient_designs_host.py asserts how many output pixels each of them gets wrong on the designs, and
test_gpu_gradient_designs.py runs the designs through the kernels bit for bit.

Designs (design_images(name, shrink): a tuple of uint8 images of about two tile rows by two tile columns of the cell)
  words           a mosaic of 4 x 4 patches, each found by a search to spell one block word in its centre block
                  (WORD_PATCHES), and two seeded compositions of one family (ramps of slope
                  0 .. 3 along x, y, x + y, x - y or a random profile, point perturbations of +-3, random cells) that add the
                  words the mosaic lacks (WORD_SEEDS).  Neither search runs at test time.  At shrink 2 level 0 holds 73 / 77 /
                  73 of the 81 words in channels 1 / 2 / 3 (WORDS_REACHED); WORDS_MISSING names the others, all of them
                  mixtures of R and Z without an O: channel 2 lacks exactly the four words of one R beside three Z
  order           x / x + y / x - y ramps whose slope changes every column (every diagonal): residue-only blocks with two
                  different residues.  Only channel 2 can be sensitive to the order of the pool: a residue of channel 1 or
                  3 is 0 or ONE ulp of an fp64 product below 1020 -- a power of two between 2^-53 and 2^-43 --, and four
                  of those sum exactly in fp32 in any order (asserted over all 1020 magnitudes by the host test)
  absorb          a 0 / 255 square wave of period 4 along x (|gx| = 1020, gy == 0) with single pixels dented by one grey
                  level: three of the largest channel-2 residues (1.87e-13 together) beside the smallest ordinary value there
                  is, 1; ramps of slope 3 along x + y and x - y with the same dents for channels 1 and 3 (3.4e-13 beside
                  fp32(2 sin(pi/4)), the smallest ordinary value of those channels: d is even, see extremes)
  zeros           sawteeth of slope 23 along the diagonals (gx == +-gy == +-184: the two fp64 products round alike, class Z
                  inside blocks the kernel redoes), a ramp along y alone (gx == 0 throughout, gy != 0: no redo), a zigzag
                  along x (both signs of gx)
  extremes        steps, stripes and corners of 0 / 255: |gx| = |gy| = 1020.  d = |gx -+ gy| is EVEN and at most 1530, not
                  1 .. 2040: gx - gy is the stencil [[0,-2,-2],[2,0,-2],[2,2,0]].  So the kernel's bound d <= 2040 is not
                  attained, the largest value is fp32(1530 sin(pi/4)) = 1081.87 and the smallest ordinary pooled values at
                  shrink 2 are 0.25 (channels 0, 2) and 0.35355 (channels 1, 3): single pixels of 1 in a field of 0 give them
  smooth_windows  f(x) + g(y): f a zigzag whose slope changes every column (channel-2 residues of different sizes, tuned by
                  window_profile to put separating windows beside the tile edge and the level's borders), g a sawtooth of
                  slope 7 (|gy| >= 28 > |gx|: ordinary values in every channel) that is flat in a band of rows.  Variants:
                  the band is the run of rows of wave 0, 1, 2, 3 of step 2 at shrink 2 and ends before lane 61 (that wave's
                  rows alone raise the flag of tile (0, 0)); g == 0 (`all`: every window, all four tile edges, lanes 64 and
                  65 in the window of output column 63); f flat up to lane 64's column (`lanes`: the stand-alone lanes alone
                  raise the first tile column's flag); bottom tiles of 1 and 2 output rows (3 and 4 shrunk rows: waves
                  1, 1, 1, 0 and 1, 1, 1, 1 -- a bottom tile of one output row is all border, so nothing of it can differ;
                  the split 1, 1, 0, 0 belongs to smooth 0, where there is no flag)
  plain           no residue anywhere: every tile takes the fast smooth, with ordinary values down to 2^-4 at shrink 4

Findings (asserted by the host test with their counts)
  * A redo the kernel did not need cannot change a bit (project_int is exact everywhere), so dropping `o[0] != 0` from the
    condition is slower, not wrong: no design can expose it.
  * A kernel whose flag is raised only by the rows of waves 0 .. 2 is wrong only at shrink 2 (runs of rows); at shrink 1
    the waves' rows interleave and any 3-row window holds a row of waves 0 .. 2.
  * The two forms of the smooth differ in channel 2 alone, and only in windows of residues without an ordinary value:
    630 of the 2040 interior outputs of the x-only image; 0 in channels 1 and 3, also where every value is a residue.
  * No tile of the designs, and none of the 4552 separating tiles of 4000 random images of the word family (64-wide cells,
    shrink 1 and 2), is separating with its odd values in the halo ring alone, or in the stand-alone lanes 64 / 65 alone.
    An output's window is centred on a pixel of the tile, so the tile's own pixels under it must be exact zeros in channel
    2 (gx == gy == 0 on whole blocks) while the ring beside them holds two DIFFERENT residues and no ordinary value; a region
    with gy == 0 that meets a flat one has the form c + (-1)^x (a + b x), whose |gx| is constant, so the ring's residues
    come out equal and their sum is exact in fp32 as well.  That argument is borne out by the search, not proven for every
    image: a flag lost from a halo thread alone has not been made to show in the bits, and no test is claimed for it.
  * At shrink 4 an ordinary value can lie below the flag's 0.125 (one pixel of |gx| = 1 pools to 2^-4).  The kernel looks at
    redone blocks only, so such a tile stays on the fast smooth -- rightly: multiples of 2^-4 (2^-27 in channels 1, 3) below
    2^11 still sum exactly.  odd_pixels restates that; the `plain` design holds 12 such values.
"""
import ctypes as C
import functools
import itertools
from fractions import Fraction

import numpy as np

from oracle import wb_oracle as orc
from waldboost_amd import _native as nat

Z, R, O = 0, 1, 2
LETTERS = "ZRO"
CS, SN = orc.orientation_table()
C1, S1, C2 = float(CS[1]), float(SN[1]), float(CS[2])
CHI = np.float32(S1)
CLO = np.float32(S1 - float(CHI))
C2HI = np.float32(C2)
C2LO = np.float32(C2 - float(C2HI))
ODD_BELOW = np.float32(0.125)
SHRINKS = (1, 2, 4)
SMOOTHS = (0, 1)
DESIGNS = ("words", "order", "absorb", "zeros", "extremes", "smooth_windows", "plain")
WINDOW_VARIANTS = ("wave0", "wave1", "wave2", "wave3", "all", "lanes", "bottom1", "bottom2")


@functools.lru_cache(None)
def tile_geom(shrink, smooth):
    tu, tv = C.c_int(), C.c_int()
    assert nat.load().wb_channels_tile(nat.WB_CHN_GRAD_HIST, shrink, C.byref(tu), C.byref(tv)) == 0
    return dict(S=shrink, TU=tu.value, TV=tv.value, HS=1 if smooth else 0)


def identity_levels(img, shrink):
    """The octave images of a design whose (only) level is the identity: the oracle's resize asserted to return the octave
    image itself.  Level 0 always is (the designs' sides are multiples of the shrink); a later octave with a side that is
    no multiple of the shrink is cut to one and resampled, and ends the list."""
    out = []
    plan = orc.level_plan(img.shape[0], img.shape[1], shrink, 1)
    for base, lv in zip(orc.image_octaves(img), plan):
        if (lv["nh"], lv["nw"]) != base.shape:
            break
        assert np.array_equal(orc.resize_bilinear(base, lv["nh"], lv["nw"]), base)
        out.append(base)
    assert out, "level 0 of a design is not the image"
    return out


# ------------------------------------------------------------------------------ step 2, restated
def sobel_int(img):
    """(gx, gy) in int64: the [1,2,1] x [-1,0,1] passes with the edge pixel duplicated; asserted equal to orc.gradients."""
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    hv = p[:-2, :] + 2 * p[1:-1, :] + p[2:, :]
    hh = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    gx, gy = hv[:, :-2] - hv[:, 2:], hh[:-2, :] - hh[2:, :]
    ox, oy = orc.gradients(img.astype(np.float32))
    assert np.array_equal(gx, ox.astype(np.int64)) and np.array_equal(gy, oy.astype(np.int64))
    return gx, gy


def classes_of(gx, gy):
    """int8 [H, W, 4]: Z / R / O per channel, from the integers and the fp64 constants alone."""
    g = gx.astype(np.float64)
    leftover = (g * C1) != (g * S1)
    cl = np.full(gx.shape + (4,), O, np.int8)
    cl[..., 0][gx == 0] = Z
    for k, diag in ((1, gx == gy), (3, gx == -gy)):
        cl[..., k][diag] = np.where(leftover & (gx != 0), R, Z)[diag]
    cl[..., 2][gy == 0] = np.where(gx != 0, R, Z)[gy == 0]
    return cl


def fmaf(a, b, c):
    """fp32 fma(a, b, c) through fp64: a * b is exact there; where the fp64 sum is not, the two fp64 neighbours of the sum
    must round to the same fp32 (the true value lies between them), so the double rounding cannot show."""
    p = a.astype(np.float64) * np.float64(b)
    c = np.asarray(c, np.float64)
    t = p + c
    r = t.astype(np.float32)
    bv = t - p
    inexact = ((p - (t - bv)) + (c - bv)) != 0
    if inexact.any():
        ti = t[inexact]
        lo, hi = np.nextafter(ti, -np.inf).astype(np.float32), np.nextafter(ti, np.inf).astype(np.float32)
        assert np.array_equal(lo, hi), "fp32 fma emulation: a sum on a rounding boundary"
    return r


def split_sin(d):
    """fp32(d sin(pi/4)) as the kernel forms it: fma(d, chi, d * clo)."""
    d = np.abs(d).astype(np.float32)
    return fmaf(d, CHI, d * CLO)


def project_int(gx, gy, tiny=True, c2_split=True):
    """project_int of the kernel, float32 [H, W, 4].  tiny=False: the d == 0 residue dropped; c2_split=False: the
    cos(pi/2) residue from the fp32 constant alone."""
    g = gx.astype(np.float64)
    t = np.abs((g * C1 - g * S1).astype(np.float32)) if tiny else np.zeros(gx.shape, np.float32)
    ax = np.abs(gx).astype(np.float32)
    out = np.empty(gx.shape + (4,), np.float32)
    out[..., 0] = ax
    out[..., 1] = np.where(gx == gy, t, split_sin(gx - gy))
    out[..., 2] = np.where(gy == 0, fmaf(ax, C2HI, ax * C2LO) if c2_split else ax * C2HI, np.abs(gy).astype(np.float32))
    out[..., 3] = np.where(gx == -gy, t, split_sin(gx + gy))
    return out


def project_ordinary(gx, gy):
    out = np.empty(gx.shape + (4,), np.float32)
    out[..., 0] = np.abs(gx)
    out[..., 1] = split_sin(gx - gy)
    out[..., 2] = np.abs(gy)
    out[..., 3] = split_sin(gx + gy)
    return out


def project_contracted(gx, gy):
    """The float route with the projection contracted to fma(gx, c, -(gy * s)) in fp64, in exact rational arithmetic per
    distinct (gx, gy) (Fraction -> float is correctly rounded)."""
    pairs, inv = np.unique(np.stack([gx.ravel(), gy.ravel()], 1), axis=0, return_inverse=True)
    tab = np.empty((len(pairs), 4), np.float32)
    cf = [Fraction(float(c)) for c in CS]
    for i, (x, y) in enumerate(pairs.tolist()):
        for k in range(4):
            tab[i, k] = abs(np.float32(float(x * cf[k] - Fraction(float(y) * float(SN[k])))))
    return tab[inv.ravel()].reshape(gx.shape + (4,))


POOL_ORDERS = {"kernel": "abcd", "reversed": "dcba", "pairs": "ac|bd"}


def pool2(ch, order="kernel"):
    u, v = ch.shape[0] // 2 * 2, ch.shape[1] // 2 * 2
    q = dict(a=ch[0:u:2, 0:v:2], b=ch[1:u:2, 0:v:2], c=ch[0:u:2, 1:v:2], d=ch[1:u:2, 1:v:2])
    o = POOL_ORDERS[order]
    if "|" in o:
        s = (q[o[0]] + q[o[1]]) + (q[o[3]] + q[o[4]])
    else:
        s = ((q[o[0]] + q[o[1]]) + q[o[2]]) + q[o[3]]
    return (s * np.float32(0.25)).astype(np.float32)


def pool(ch, shrink, order="kernel"):
    for _ in range({1: 0, 2: 1, 4: 2}[shrink]):
        ch = pool2(ch, order)
    return ch


def block_any(mask, shrink):
    u, v = mask.shape[0] // shrink, mask.shape[1] // shrink
    return mask[:u * shrink, :v * shrink].reshape(u, shrink, v, shrink, *mask.shape[2:]).any(axis=(1, 3))


def step2(gx, gy, shrink, wrong=None):
    """The shrunk level as channels_kernel<uint8, FAST> forms it (wrong=None), or as one of WRONG_KERNELS would.
    Returns (level float32 [u, v, 4], redo bool [u, v])."""
    kw = dict(tiny=wrong != "no_tiny", c2_split=wrong != "c2_fp32_constant")
    order = wrong[5:] if wrong and wrong.startswith("pool_") else "kernel"
    exact = pool(project_int(gx, gy, **kw), shrink, order)          # (pool_*: the redone blocks -- the residues -- in another order)
    if shrink == 1:
        return exact, np.zeros(gx.shape, bool)
    first = pool(project_ordinary(gx, gy), shrink)
    ks = [k for k in (1, 2, 3) if wrong != f"redo_without_channel_{k}"]
    redo = first[..., ks].min(-1) == 0
    if wrong != "redo_without_gx_term":
        redo &= first[..., 0] != 0
    if wrong == "no_redo":
        redo[:] = False
    return np.where(redo[..., None], exact, first), redo


def words_of(cl):
    """uint8 [u, v, 4]: per 2 x 2 block and channel the word a + 3 b + 9 c + 27 d of the classes."""
    u, v = cl.shape[0] // 2 * 2, cl.shape[1] // 2 * 2
    c = cl.astype(np.uint8)
    return c[0:u:2, 0:v:2] + 3 * c[1:u:2, 0:v:2] + 9 * c[0:u:2, 1:v:2] + 27 * c[1:u:2, 1:v:2]


def word_name(w):
    return "".join(LETTERS[(int(w) // 3 ** i) % 3] for i in range(4))


# ------------------------------------------------------------------------------ step 3, restated
def smooth_fast(lv, fp32_channels=(0, 2)):
    """The separable smooth of the kernel over a whole level: fma(2, a1, a0) + a2 along rows, the same form over rows, in
    fp32 for `fp32_channels` and fp64 for the others; border zeroed."""
    out = np.zeros_like(lv)
    u, v = lv.shape[:2]
    if u < 3 or v < 3:
        return out
    for k in range(4):
        a = lv[..., k]
        if k in fp32_channels:
            s = fmaf(a[:, 1:-1], np.float32(2), a[:, :-2]) + a[:, 2:]
            o = (fmaf(s[1:-1], np.float32(2), s[:-2]) + s[2:]) * np.float32(0.0625)
        else:
            a = a.astype(np.float64)
            s = (2.0 * a[:, 1:-1] + a[:, :-2]) + a[:, 2:]
            o = (((2.0 * s[1:-1] + s[:-2]) + s[2:]) * 0.0625).astype(np.float32)
        out[1:-1, 1:-1, k] = o
    return out


def wave_rows(su_need, shrink):
    """Owner wave of every shrunk row of a 64-wide tile in step 2: at shrink 2 wave w of 4 owns the
    run i_w = w q + min(w, rem), n_w = q + (w < rem); at shrink 1 row i belongs to wave i % 4."""
    if shrink == 1:
        return np.arange(su_need) % 4
    q, rem = divmod(su_need, 4)
    own = np.empty(su_need, np.int64)
    for w in range(4):
        i = w * q + min(w, rem)
        own[i:i + q + (w < rem)] = w
    return own


def odd_pixels(lv, redo, shrink):
    """Shrunk pixels whose thread raises the flag: a value in (0, 0.125) -- under a shrink only a redone block is looked at
    (the first pass writes 0 for a residue; an ordinary value below 0.125 exists only at shrink 4: one pixel of |gx| = 1
    pools to 2^-4, still inside the fast smooth's exact range, and the host test holds the fast smooth to the oracle there)."""
    odd = ((lv > 0) & (lv < ODD_BELOW)).any(-1)
    return odd if shrink == 1 else odd & redo


def odd_ring(img, shrink, wrong=None):
    """bool [u + 2, v + 2]: odd_pixels of level 0 and of the ring of shrunk pixels around it, which the tiles on the level's
    border compute as their smooth halo.  Step 1 clamps coordinates outside the level, so the ring is the level of the image
    padded with its edge pixels: above and below the level gy == 0 and gx is four times the first (last) row's difference
    -- a channel-2 residue, so a border tile's flag is almost always up --, left and right of it gx == 0 (no residue)."""
    gx, gy = sobel_int(np.pad(img, shrink, mode="edge"))
    lv, redo = step2(gx, gy, shrink, wrong)
    return odd_pixels(lv, redo, shrink)


def tile_report(lv, ring, ref_smooth, shrink, waves=(0, 1, 2, 3), lanes=True):
    """Per tile of a smoothed level (lv: the shrunk level, ring: odd_ring of its image, ref_smooth: the oracle's smooth of
    lv): dict of [ny, nx] arrays odd (an odd value in the tile or its halo ring, computed by a wave of `waves`; lanes=False:
    not by the stand-alone lanes 64 and 65), odd_inner (... in the tile itself), separating (the fast smooth differs from
    the oracle in an output pixel of the tile) and n_sep."""
    g = tile_geom(shrink, 1)
    u, v = lv.shape[:2]
    ny, nx = -(-u // g["TU"]), -(-v // g["TV"])
    assert ring.shape == (u + 2, v + 2)
    diff = (smooth_fast(lv).view(np.uint32) != ref_smooth.view(np.uint32)).any(-1)
    rep = dict(odd=np.zeros((ny, nx), bool), odd_inner=np.zeros((ny, nx), bool), n_sep=np.zeros((ny, nx), np.int64))
    for ty, tx in itertools.product(range(ny), range(nx)):
        u0, v0 = ty * g["TU"], tx * g["TV"]
        vrows = min(u - u0, g["TU"])
        own = wave_rows(vrows + 2, shrink) if g["TV"] == 64 else np.zeros(vrows + 2, np.int64)
        for i in range(vrows + 2):
            row = ring[u0 + i]                                # (ring coordinates: level row u0 - 1 + i, level column + 1)
            cols = row[v0:v0 + g["TV"] + 2]
            # (lanes 64 and 65 of a 64-wide tile are stand-alone pixels of the LAST wave)
            first64 = row[v0:v0 + 64].any()
            extra = row[v0 + 64:v0 + 66].any() if g["TV"] == 64 else False
            hit = cols.any() if g["TV"] != 64 else ((first64 and own[i] in waves) or (extra and lanes and 3 in waves))
            rep["odd"][ty, tx] |= bool(hit)
        rep["odd_inner"][ty, tx] = ring[1:-1, 1:-1][u0:u0 + vrows, v0:v0 + g["TV"]].any()
        rep["n_sep"][ty, tx] = diff[u0:u0 + vrows, v0:v0 + g["TV"]].sum()
    rep["separating"] = rep["n_sep"] > 0
    rep["diff"] = diff
    return rep


def smooth_kernel(lv, ring, ref_smooth, shrink, wrong=None):
    """The smoothed level as the kernel gives it: per tile the fast form, or (flag raised) the oracle's chain."""
    if wrong == "smooth_all_fp32":
        fast = smooth_fast(lv, (0, 1, 2, 3))
    else:
        fast = smooth_fast(lv)
    lost = int(wrong[-1]) if wrong and wrong.startswith("flag_without_wave_") else None
    rep = tile_report(lv, ring, ref_smooth, shrink, waves=tuple(w for w in range(4) if w != lost), lanes=wrong != "flag_without_lanes_64_65")
    g = tile_geom(shrink, 1)
    out = fast.copy()
    if wrong != "flag_ignored":
        for ty, tx in zip(*np.nonzero(rep["odd"])):
            sl = np.s_[ty * g["TU"]:(ty + 1) * g["TU"], tx * g["TV"]:(tx + 1) * g["TV"]]
            out[sl] = ref_smooth[sl]
    return out, rep


WRONG_KERNELS = ("no_redo", "redo_without_gx_term", "redo_without_channel_1", "redo_without_channel_2", "redo_without_channel_3",
                 "pool_reversed", "pool_pairs", "c2_fp32_constant", "no_tiny", "flag_ignored", "flag_without_wave_0",
                 "flag_without_wave_1", "flag_without_wave_2", "flag_without_wave_3", "flag_without_lanes_64_65", "smooth_all_fp32",
                 "float_contracted")
SMOOTH_WRONG = tuple(w for w in WRONG_KERNELS if w.startswith("flag_") or w == "smooth_all_fp32")


def applies(wrong, shrink, smooth):
    if wrong in ("flag_ignored", "smooth_all_fp32"):
        return smooth == 1
    if wrong.startswith("flag_without_wave_"):
        return smooth == 1 and shrink == 2
    if wrong == "flag_without_lanes_64_65":
        return smooth == 1 and shrink in (1, 2)
    if wrong.startswith("redo") or wrong == "no_redo" or wrong.startswith("pool_"):
        return shrink > 1
    return True


def emulate(img, shrink, smooth, wrong=None):
    """Level 0 of the design as the kernel (or a wrong kernel) computes it, float32 [u, v, 4]."""
    gx, gy = sobel_int(img)
    if wrong == "float_contracted":
        lv = pool(project_contracted(gx, gy), shrink)
    else:
        lv, redo = step2(gx, gy, shrink, wrong)
    if not smooth:
        return lv
    ref_lv = pool(orc.grad_hist(img), shrink)
    if wrong in SMOOTH_WRONG:
        return smooth_kernel(lv, odd_ring(img, shrink), orc.smooth_image_3d(ref_lv), shrink, wrong)[0]
    return orc.smooth_image_3d(lv)


@functools.lru_cache(None)
def oracle_level0(name, index, shrink, smooth):
    img = design_images(name, shrink)[index]
    lv = pool(orc.grad_hist(img), shrink)
    return orc.smooth_image_3d(lv) if smooth else lv


def classify(img, shrink):
    """Everything the tests ask about level 0 of a design: gradients, classes (asserted against orc.grad_hist), the
    oracle's and the restated kernel's shrunk level, redo, words (2 x 2 blocks of level 0's pixels), residue_only."""
    gx, gy = sobel_int(img)
    cl = classes_of(gx, gy)
    ref = orc.grad_hist(img)
    ocl = np.where(ref == 0, Z, np.where(ref < 1e-6, R, O))
    assert np.array_equal(cl, ocl), "classes from the integers against the oracle's values"
    lv, redo = step2(gx, gy, shrink)
    has = lambda c: block_any(cl == c, shrink) if shrink > 1 else (cl == c)
    ring = odd_ring(img, shrink)
    assert np.array_equal(ring[1:-1, 1:-1], odd_pixels(lv, redo, shrink))
    return dict(gx=gx, gy=gy, cls=cl, pixels=ref, level=lv, ref_level=pool(ref, shrink), redo=redo, words=words_of(cl),
                residue_only=has(R) & ~has(O), ring=ring)


# ------------------------------------------------------------------------------ designs
def base_shape(shrink, rows=None):
    """(H, W) of two tile rows by two tile columns (the second column 6 outputs wide); rows: output rows instead."""
    g = tile_geom(shrink, 1)
    return shrink * (rows or 2 * g["TU"]), shrink * (g["TV"] + 6)


def _clip8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def word_image(seed, H, W):
    """One image of the family the word search draws from."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    kind = int(rng.integers(0, 8))
    slope = int(rng.integers(0, 4))
    t = [np.zeros_like(x), x, y, x + y, x - y + H][kind % 5]
    if kind < 5:
        img = 20 + (slope * t) % 200
    else:                       # a profile along x, x + y or x - y whose slope (-3 .. 3, often 0) changes at random
        steps = rng.integers(-3, 4, H + W + 1) * (rng.random(H + W + 1) < 0.6)
        img = 100 + np.cumsum(steps)[t]
    if rng.random() < 0.5:
        k = int(rng.integers(2, 6))
        cells = rng.integers(0, 2, (-(-H // k), -(-W // k))) * int(rng.integers(1, 60))
        sel = np.kron(rng.integers(0, 2, (-(-H // 16), -(-W // 16))), np.ones((16, 16), np.int64))[:H, :W]
        img = np.where(sel == 1, 20 + np.kron(cells, np.ones((k, k), np.int64))[:H, :W], img)
    n = int(rng.integers(0, 201))
    img[rng.integers(0, H, n), rng.integers(0, W, n)] += rng.integers(-3, 4, n)
    return _clip8(img)


# 4 x 4 pixel patches (one base-36 digit per pixel, row-major) whose centre 2 x 2 block spells a word in channel 1, 2 or 3:
# the first patch found per (channel, word) by search_word_patches -- a block's gradients depend on nothing else
WORD_PATCHES = (
    "0000000000000000 0000000000000001 0000000000030030 0000000010000000 0000000100000010 0000020000000000 "
    "0000100000000010 0000200100000100 0000200200000200 0001000000000000 0002000000002000 0010100000000000 "
    "0020020000000000 0030000000001000 0030000200000000 0030000300000000 0033000030010000 0100000000000000 "
    "0100100000000000 0111110111111111 0112111111111114 0120012301230123 0132123423453486 0133313333315133 "
    "0200000020000000 0212022130222122 0220000002000000 0222012301230123 0223222222022224 02450485496a87ac "
    "0246023602460246 0246024702460246 02460468468a68aa 0300000000002000 0300000300000000 0331333333333333 "
    "0333333303333330 0333333333333303 0333333333335333 0363333533333335 0369036903690369 0369369b69bf9cfi "
    "0369369c69cf9cfi 0369379c69bf9cfi 036a265b579e4cbd 042624684689689c 0448124602560246 0548025513661246 "
    "058b58be8behbefk 0636332333633240 069c79cf9cficfil 1000000000000000 1000000000000001 1000000010000000 "
    "1002000000100000 1011242232635414 1110111411112411 1110121441101213 1111011111111111 1111101111111110 "
    "1111111110111101 1111111111011111 1111111111100111 1111111111101111 1111111111110111 1111111111110121 "
    "1111111111111011 1111111311110121 1111121011111111 1111441111011313 1113111111111110 1204234534564567 "
    "1330033333333333 2000000002000000 2022222202202222 2022222222122222 2022232220213212 2023022222022222 "
    "2033332040534233 2101111111111111 2101111411141424 2111011111111101 2202222222222222 2202222522223222 "
    "2220222222202222 2222022242222221 2222121222220220 2222212222222200 2222220222222220 2222220222222224 "
    "2222222022222204 2222222202222422 2222222222222202 2222222242222220 2222222242225220 2222222322252220 "
    "2222250122223252 2222321202235223 2222423022222222 2224202222222422 2230222322222222 2277227802852467 "
    "2345234533350345 2363360223563321 2522222222223420 3000000000020000 3033333333303333 3034333333303333 "
    "3036333333333333 3063330143512305 3133033333333333 3231063331240336 3232022222422222 3233533304233333 "
    "3250333333333333 3318254606765345 3330333324362506 3332333323330333 3333031333332333 3333033336636332 "
    "3333233333333303 3333233363330341 3333303334323033 3333333033333333 3333333303633333 3333333331033333 "
    "3333333333303313 3333333333333036 3333333333333063 3333333333350533 3333333533033633 3333633333333330 "
    "3335333133330336 3336333333333033 3351303343433033 3360333363333333 3363330033333606 3410333433333333 "
    "3433033335352333 3433033631333033 3453534510340153 3456264512330323 3533033333332333 3613343353135330 "
    "4075062523343432 4456234512340123 5336260313366003 5503333333333333 56a8456a37562044 5beg58be258b0258 "
    "6333333233333330 68aa468a24680546 68ac468a24680249 8dbh58be258b0258 8egg69cf369c0469 9cfh69cf369c0369 "
    "9cfi69cf369c0369 9cfi69cf369c066c 9cfi69cf469c0289 9cfi69cg469c0369 abfi69cf369c0369"
).split()
# seeds of word_image that add words the mosaic of patches does not hold (search_word_seeds over 40000 seeds, greedy order)
WORD_SEEDS = (232, 301)
# distinct words of channels 1, 2, 3 over level 0 of the shrink-2 images, and the words neither search reached
WORDS_REACHED = (73, 77, 73)
WORDS_MISSING = {1: "RRZR RRZZ RZRR RZRZ ZRZR ZRZZ ZZRR ZZRZ".split(), 2: "RZZZ ZRZZ ZZRZ ZZZR".split(),
                 3: "RRRZ RRZZ RZRZ RZZZ ZRRR ZRZR ZZRR ZZZR".split()}


def mosaic_image(H, W):
    """The patches on a grid of stride 4, each with its centre block on even coordinates (rows 4 i + 2, 4 i + 3)."""
    img = np.zeros((H, W), np.int64)
    slots = [(r, c) for r in range(1, H - 4, 4) for c in range(1, W - 4, 4)]
    for (r, c), p in zip(slots, WORD_PATCHES):
        img[r:r + 4, c:c + 4] = np.array([int(ch, 36) for ch in p]).reshape(4, 4)
    return _clip8(img)


def search_word_patches(rounds=15, n=200000):
    """{(channel, word): patch string}: random 4 x 4 patches -- a ramp of slope 0 .. 3 along x, y, x + y or x - y plus
    perturbations of +-3 on 10, 30 or 60 % of the pixels -- classified at their centre block (not run at test time)."""
    found = {}
    y, x = np.mgrid[0:4, 0:4]
    ramps = np.stack([0 * x, x, y, x + y, x - y + 3])
    for rnd in range(rounds):
        rng = np.random.default_rng(rnd)
        base = ramps[rng.integers(0, 5, n)] * rng.integers(0, 4, n)[:, None, None]
        p = base + rng.integers(-3, 4, (n, 4, 4)) * (rng.random((n, 4, 4)) < rng.choice([0.1, 0.3, 0.6], n)[:, None, None])
        p -= p.min(axis=(1, 2), keepdims=True)
        ok = p.max(axis=(1, 2)) < 36
        hv = p[:, :-2, :] + 2 * p[:, 1:-1, :] + p[:, 2:, :]
        hh = p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:]
        gx, gy = hv[:, :, :-2] - hv[:, :, 2:], hh[:, :-2, :] - hh[:, 2:, :]
        cl = classes_of(gx.reshape(n * 2, 2), gy.reshape(n * 2, 2)).reshape(n, 2, 2, 4).astype(np.int64)
        w = cl[:, 0, 0] + 3 * cl[:, 1, 0] + 9 * cl[:, 0, 1] + 27 * cl[:, 1, 1]
        for k in (1, 2, 3):
            vals, idx = np.unique(np.where(ok, w[:, k], -1), return_index=True)
            for v, i in zip(vals.tolist(), idx.tolist()):
                if v >= 0:
                    found.setdefault((k, v), "".join("0123456789abcdefghijklmnopqrstuvwxyz"[t] for t in p[i].ravel()))
    return found


def search_word_seeds(n_seeds, H=64, W=140):
    """Greedy cover of the block words of channels 1 .. 3 by images of the family (not run at test time)."""
    seen, picked = [set(), set(), set()], []
    for seed in range(n_seeds):
        img = word_image(seed, H, W)
        gx, gy = sobel_int(img)
        w = words_of(classes_of(gx, gy))
        new = [set(np.unique(w[..., k]).tolist()) - seen[k - 1] for k in (1, 2, 3)]
        if any(new):
            picked.append(seed)
            for k in range(3):
                seen[k] |= new[k]
    # second pass: the picked images in greedy order of what they add, the useless ones dropped
    sets = {}
    for seed in picked:
        gx, gy = sobel_int(word_image(seed, H, W))
        w = words_of(classes_of(gx, gy))
        sets[seed] = {(k, x) for k in (1, 2, 3) for x in np.unique(w[..., k]).tolist()}
    have, order = set(), []
    while True:
        best = max(sets, key=lambda s: len(sets[s] - have))
        if not sets[best] - have:
            break
        order.append(best)
        have |= sets[best]
    return order, seen


def _ramp_varying(n, rng, lo=0, hi=3):
    """Integer profile of n samples whose slope (lo .. hi) changes at every sample, folded into 0 .. 230."""
    s = rng.integers(lo, hi + 1, n)
    f = np.cumsum(s)
    period = 2 * 230
    f = f % period
    return np.where(f > 230, period - f, f)


def order_image(H, W, seed=5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    f = _ramp_varying(H + W + 1, rng)
    img = np.empty((H, W), np.int64)
    third = H // 3
    img[:third] = f[x[:third]]
    img[third:2 * third] = f[(x + y)[third:2 * third]]
    img[2 * third:] = f[(x - y + H)[2 * third:]]
    return _clip8(img + 10)


def absorb_image(H, W, seed=6):
    """Top third: 0 / 255 square wave of period 4 along x (|gx| = 1020, gy == 0) with dents of one grey level; below it
    ramps of slope 3 along x + y and x - y with the same dents."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    third = H // 3
    img = np.where((x // 2) % 2 == 0, 255, 0).astype(np.int64)
    img[third:2 * third] = (3 * (x + y) % 240)[third:2 * third]
    img[2 * third:] = (3 * (x - y + H) % 240)[2 * third:]
    n = H * W // 40
    ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
    img[ys, xs] += np.where(img[ys, xs] > 128, -1, 1)
    return _clip8(img)


def zeros_image(H, W, seed=7):
    """Six vertical strips: sawteeth of slope 23 along x + y and x - y, rising and falling -- gx == +-gy == +-184, one of the 84
    magnitudes up to 1020 whose two fp64 products round alike: class Z with a gradient --, a ramp along y alone (gx == 0,
    gy != 0: no redo) and a zigzag along x (both signs of gx, gy == 0)."""
    y, x = np.mgrid[0:H, 0:W]
    q = -(-W // 6)
    saw = lambda t: (23 * t) % 230
    strips = [saw(x + y), 230 - saw(x + y), saw(x - y + H), 230 - saw(x - y + H), 3 * y % 250,
              np.where(x % 16 < 8, x % 8 * 5, 35 - x % 8 * 5)]
    img = np.empty((H, W), np.int64)
    for i, st in enumerate(strips):
        img[:, i * q:(i + 1) * q] = st[:, i * q:(i + 1) * q]
    return _clip8(img)


def extremes_image(H, W):
    """0 / 255 in stripes, steps and corners; single pixels of 1 in a flat region of 0 (the smallest ordinary values)."""
    y, x = np.mgrid[0:H, 0:W]
    q = W // 4
    img = np.zeros((H, W), np.int64)
    img[:, :q] = np.where((x[:, :q] // 3) % 2 == 0, 255, 0)
    img[:, q:2 * q] = np.where((y[:, q:2 * q] // 3) % 2 == 0, 255, 0)
    img[:, 2 * q:3 * q] = np.where(((x + y)[:, 2 * q:3 * q] // 4) % 2 == 0, 255, 0)
    img[:, 3 * q:] = np.where(((x // 5 + y // 3)[:, 3 * q:]) % 2 == 0, 255, 0)
    img[H // 2:, 3 * q + 4:] = 0
    for dy, dx in ((6, 6), (6, 11), (11, 6), (11, 11)):          # every parity: each corner pixel of a dot alone in a block
        img[H // 2 + dy, 3 * q + dx] = 1
    return _clip8(img)


def _fold(slopes):
    f = np.cumsum(slopes) + 1000
    return np.abs(f % 200 - 100)


def _x_only_separating(f, shrink):
    """Per level column: does the fast smooth differ from the chain on an image of eight level rows that is f(x) in every row."""
    img = _clip8(np.repeat(f[None, :], 8 * shrink, 0))
    lv = pool(orc.grad_hist(img), shrink)
    return (smooth_fast(lv).view(np.uint32) != orc.smooth_image_3d(lv).view(np.uint32)).any(-1)[3]


@functools.lru_cache(None)
def window_profile(shrink, seed=8):
    """f(x): slopes of -3 .. 3 that change every column, folded into 0 .. 100, then re-drawn locally (seeded, at most 3000
    draws per place) until the x-only image has a separating output in the columns on both sides of the tile edge -- the first
    tile column's last output has lanes 64 and 65 in its window -- and beside both borders of the level."""
    g = tile_geom(shrink, 1)
    W = base_shape(shrink)[1]
    v = W // shrink
    groups = [[1], [g["TV"] - 1, g["TV"]], [v - 2]]
    rng = np.random.default_rng(seed)
    slopes = rng.integers(-3, 4, W)
    done = []
    for grp in groups:
        lo, hi = max(shrink * (grp[0] - 2), 0), min(shrink * (grp[-1] + 3), W)
        for _ in range(3000):
            sep = _x_only_separating(_fold(slopes), shrink)
            if sep[done + grp].all():
                break
            slopes[lo:hi] = rng.integers(-3, 4, hi - lo)
        done += grp
    have = _x_only_separating(_fold(slopes), shrink)[done]
    assert have.all(), "window_profile: no profile found"
    return _fold(slopes)


def window_image(shrink, variant, seed=8):
    """f(x) + g(y), see the module docstring."""
    g = tile_geom(shrink, 1)
    rows = dict(bottom1=g["TU"] + 1, bottom2=g["TU"] + 2).get(variant)
    H, W = base_shape(shrink, rows)
    f = window_profile(shrink, seed)
    if variant == "lanes":
        # flat up to the column of lane 64, then a slope that grows by one every column: the first tile column's only odd
        # values are the two stand-alone pixels of its last wave
        edge = shrink * (g["TV"] - 1)
        f = np.concatenate([np.full(edge + 1, 10), 10 + np.cumsum(1 + np.arange(W - edge - 1) % 5)])
    slope = np.full(H, 7, np.int64)
    u = H // shrink
    if variant in ("all", "lanes", "bottom1", "bottom2"):
        band = (g["TU"] - 3, u - 1) if variant.startswith("bottom") else (0, u - 1)
    else:
        own = wave_rows(g["TU"] + 2, 2)
        rows_w = np.nonzero(own == int(variant[-1]))[0] - 1           # level rows of the wave's run in tile row 0
        band = (max(int(rows_w[0]), 0), int(rows_w[-1]))
    slope[max(shrink * band[0] - 1, 0):shrink * band[1] + shrink + 1] = 0    # gy == 0 on every pixel of the band's blocks
    # (a sawtooth: |gy| >= 28 > |gx| on every row outside the band, the wrap included, so no channel there holds a residue)
    gcol = (np.cumsum(slope) - slope[0]) % 140
    img = f[None, :] + gcol[:, None]
    if variant.startswith("wave"):
        # the band ends before lane 61's column: the stand-alone lanes 64 and 65 (the LAST wave's in every row) see ordinary
        # values, so in tile (0, 0) the rows of wave w alone raise the flag
        steep = (7 * np.arange(H)) % 140
        x0 = shrink * (g["TV"] - 4)
        img[:, x0:] = (f[None, :] + steep[:, None])[:, x0:]
        # (constant first and last rows: the ring above and below the level holds exact zeros, see odd_ring)
        img[0] = img[-1] = 0
    return _clip8(img)


@functools.lru_cache(None)
def design_images(name, shrink):
    H, W = base_shape(shrink)
    if name == "words":
        return (mosaic_image(H, W),) + tuple(word_image(s, H, W) for s in WORD_SEEDS)
    if name == "smooth_windows":
        return tuple(window_image(shrink, v) for v in WINDOW_VARIANTS)
    return ({"order": order_image, "absorb": absorb_image, "zeros": zeros_image, "extremes": extremes_image,
             "plain": plain_image}[name](H, W),)


CASES = [(d, i) for d in DESIGNS for i in range({"smooth_windows": len(WINDOW_VARIANTS), "words": 1 + len(WORD_SEEDS)}.get(d, 1))]


def plain_image(H, W):
    """No residue anywhere (no tile raises the flag): a ramp along x + 2 y on the left, on the right a ramp of slope 2 along y
    with single pixels one grey level up -- |gx| of 1 and 2 in a field of gx == 0, the ordinary values that pool to 2^-4 and
    fp32(2 sin(pi/4)) / 16 at shrink 4, below the flag's 0.125."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.where(x < W // 2, (x + 2 * y) % 251, (2 * y) % 250)
    img[(x >= W // 2 + 4) & (x < W - 4) & (y % 9 == 4) & (x % 11 == 5)] += 1
    img[0] = img[-1] = 0                                      # (no residue in the ring around the level either: odd_ring)
    return _clip8(img)


def flat_image(shrink, variant="all"):
    """The plain design at the shape of a smooth_windows variant: the batch-mate without any odd value."""
    return plain_image(*window_image(shrink, variant).shape)


# ------------------------------------------------------------------------------ failure messages
def describe_mismatch(got, ref, img, shrink, smooth, level=0):
    """Names the first differing output pixel of level 0, its tile, the wave that owns its row in step 2 and the words of
    the blocks under its window."""
    diff = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
    r, c = (int(x) for x in diff[0])
    g = tile_geom(shrink, smooth)
    ty, tx = r // g["TU"], c // g["TV"]
    msg = (f"level {level}: {len(diff)} output pixels differ, first at ({r}, {c}) = {got[r, c].tolist()} against {ref[r, c].tolist()}, "
           f"tile ({ty}, {tx})")
    if level == 0:
        m = classify(img, shrink)
        vrows = min(m["level"].shape[0] - ty * g["TU"], g["TU"])
        if g["TV"] == 64:
            msg += f", shrunk row {r - ty * g['TU'] + g['HS']} of wave {wave_rows(vrows + 2 * g['HS'], shrink)[r - ty * g['TU'] + g['HS']]}"
        if shrink == 2:
            h = g["HS"]
            w = m["words"][max(r - h, 0):r + h + 1, max(c - h, 0):c + h + 1]
            msg += ", block words (channels 1, 2, 3) under its window: " + "; ".join(
                "/".join(word_name(x) for x in row[1:]) for row in w.reshape(-1, 4))
        msg += f", redo {bool(m['redo'][r, c])}, residue_only {m['residue_only'][r, c].tolist()}"
    return msg
