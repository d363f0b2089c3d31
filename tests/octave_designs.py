"""Designed images for step 0 of every timed step: the octave kernels of csrc/wb_octaves.hip (NumPy only: no GPU, no torch,
nothing of the library).

octaves_block_kernel pools a 128 x 128 (uint8) or 64 x 64 (float32) block of the image down to one pixel in LDS and keeps,
per octave, a (min, max) pair that leaves the workgroup with one atomic per value; octaves_tail_kernel walks the octaves
beyond a block's reach; the dtypes held as float64 take one plain launch per octave (pool_f64_kernel).  Noise covers the
arithmetic of the pooling well (every 2 x 2 quad of a +70 uint8 image wraps, 17 .. 31 % of float32 quads are order
sensitive) but not three other things, which the designs here hold on purpose:

  * the (min, max) reduction.  On noise every extreme occurs in many lanes, waves and workgroups, so a kernel that drops
    one wave's partial, one octave's slot or a batch-mate's words still reports the right keys.  `extremes` puts each
    extreme into ONE pixel of one octave, whose owner -- workgroup, wave, lane, kernel -- is chosen by position.
  * the byte load path (regs / dword / scalar), an accident of shape and alignment: `load_path` restates the kernel's
    conditions, and the cases name the path every image of a batch takes (72 x 80: regs / dword / regs).
  * the float64-held dtypes' semantics (`held_quads`): sums on and beside every wrap boundary, negative sums of every
    residue mod 4, bool patterns, float16 double rounding, float64 order.

What is provided
  load_path, batch_paths    the kernel's choice of load path, from shape and alignment
  owner_map                 workgroup, wave, lane and kernel of every pixel of an octave
  walk_octaves, tail_octaves
  pool4                     the 2 x 2 pooling of every dtype restated (and, by `fault`, the wrong kernels' versions)
  hier_octaves              the pooling block by block with zero padding of partial blocks, then the tail's floor chain
  packed_octave1            the regs path's packed 16-bit lane arithmetic on dwords, bit for bit
  extremes, tail_bait, quads, float_quads, held_quads      the designs; CASES lists every run of the GPU module
  emulated_keys             the (min, max) a kernel with one fault of KEY_FAULTS in its reduction would report

Findings (host arithmetic, asserted by test_octave_designs_host.py)
  * hier_octaves equals orc.image_octaves bit for bit on every case: a padded pixel never reaches a stored one, because a
    stored pixel (y, x) of octave k needs y < floor(H / 2^k), and its 2^k x 2^k footprint then ends at (y + 1) * 2^k <= H.
  * no uint8 octave at or above 2 can wrap: octave-1 values are at most 63 (((s & 255) >> 2), so a quad of them sums to at
    most 252.  A "wrap in octave 2" therefore needs no design; the host test asserts the bound on every uint8 case.
  * the last (partial) workgroup of 129 x 144, 131 x 260, 65 x 80 and 67 x 132 owns too few pixels of octaves >= 1 for
    four waves; the wave sweep of its partials runs on 200 x 208, 201 x 213, 200 x 212 and 100 x 108.
  * the wave-0 walk exists for float32 too (octaves 3 .. 6 of a 64 x 64 block); the sweep covers it.
  * found by held_quads on the GPU and fixed in pool_f64_kernel: an integer quad whose wrapped sum is -1 .. -3 was stored
    as trunc(s / 4.0) = -0.0 (12 pixels of octave 1 of the int8 image), another bit pattern and another key than the
    integer's one zero; the kernel now adds + 0.0 in the integer branches.

Counts the host test measures (its assertions are the inequalities; these are the values)
  quads 131 x 272        4084 quads, every sum 3 .. 1017 in at least 3 splits: 3060 wrap, 2034 with a + b alone at or above
                         256, 1634 with a byte of 255; of the image's 8840 cells 6635 wrap, 801 .. 864 at each of the 8 cell
                         columns of a 16-pixel group, 47 .. 52 in each column beside a 128-pixel seam, 101 and 111 in the two
                         rows beside it.  Pixels of octaves >= 1 that differ: without the wrap 9486, with the high lane's
                         mask dropped 5469 (72 x 80 x 3, where only images 0 and 2 pack: 1769)
  float_quads 67 x 132   of the 2178 pixels of octave 1: 24 are +inf, 24 -inf, 64 subnormal, 24 above FLT_MAX / 8; over all
                         octaves row-first changes 569 pixels, pairwise 812, reversed 1131 (65 x 80: 365 / 488 / 684)
  held_quads 37 x 50     no wrap: int8 284, int16 295, uint16 523, int32 287, uint32 527 pixels; floor instead of trunc:
                         int8 256, int16 272, int32 254, int64 271; one float16 rounding 269; float64 row-first 103,
                         pairwise 147, reversed 212 (batch 1; three times that at batch 3)
  key faults             cases (of the 214 `extremes` and `tail_bait` ones) with a changed key: wave 0 / 1 / 2 / 3 dropped
                         214 / 109 / 115 / 65 (wave 0 owns the background's first pixel too), lane 0 only 208, image 1 or 2
                         written to image 0's words 52 each, padding admitted 126, odd tails admitted 30; a dropped octave
                         slot shows in every case that has the octave (slot 8: the 2048 x 2064 and 2048 x 8208 ones)
  tail waves             TAIL_WAVE_SHAPES, 8 cases each (of the 254 in all): the tail octave is 8 x 32, wave w owns rows 2 w and
                         2 w + 1; a tail kernel that drops wave w's partial changes that octave's key on the 4 cases with
                         an extreme in wave w, for every w (every other tail octave of the cases holds 64 pixels, wave 0's)

Not exposed by any design: none of KEY_FAULTS / PIXEL_FAULTS.  Outside that list, and not designed for: the 48 KiB
dynamic-LDS branch of the tail launch (it needs a float32 image of 160 MB: 1024 x 39424; left out).
"""
import functools

import numpy as np

from oracle import wb_oracle as orc

BLOCK = {"uint8": (128, 7), "float32": (64, 6)}          # block side at octave 0, octaves derived inside the block
# the smallest shapes whose tail octave (float32: 7, uint8: 8) is 8 x 32 = 256 pixels: one per thread of octaves_tail_kernel,
# 64 per wave (a tail octave of 64 pixels is wave 0's alone)
TAIL_WAVE_SHAPES = (("float32", 1024, 4112), ("uint8", 2048, 8208))
HELD = ("int8", "int16", "uint16", "int32", "uint32", "int64", "bool", "float16", "float64")
PIXEL_FAULTS = ("nowrap", "lane_carry", "rowfirst", "pairwise", "reversed", "floor", "single_f16")
KEY_FAULTS = ([("wave", w) for w in range(4)] + [("slot", j) for j in range(9)] + [("lane0",), ("image", 1), ("image", 2),
              ("padding",), ("odd_tails",)])


# ------------------------------------------------------------------------------ geometry
def octave_dims(H, W):
    return orc.octave_shapes(H, W)


def oct_offsets(H, W):
    """(element offset of octave k in an image's octave buffer -- octave 0 is the image itself --, elements per image),
    as PyramidPlan lays them out."""
    off, acc = [], 0
    for k, (h, w) in enumerate(octave_dims(H, W)):
        off.append(acc if k else 0)
        if k:
            acc += h * w
    return off, max(acc, 1)


def load_path(H, W, img_offset_bytes, img_stride, oct1_offset_bytes):
    """The byte load path of octaves_block_kernel<uint8_t>: offsets are those of the batch's image pointer and of THIS
    image's octave-1 pointer from a 16-byte aligned address, img_stride the elements between two images."""
    n_oct = len(octave_dims(H, W))
    if (n_oct > 1 and W % 16 == 0 and img_stride % 16 == 0 and img_offset_bytes % 16 == 0 and (W >> 1) % 4 == 0
            and oct1_offset_bytes % 4 == 0):
        return "regs"
    if W % 4 == 0 and img_stride % 4 == 0 and img_offset_bytes % 4 == 0:
        return "dword"
    return "scalar"


def batch_paths(dtype, H, W, B):
    """The path of every image of a batch laid out as the engine does (aligned buffers, stride H * W and oct_total)."""
    if str(dtype) != "uint8":
        return ["scalar"] * B
    off, total = oct_offsets(H, W)
    return [load_path(H, W, 0, H * W, b * total + (off[1] if len(off) > 1 else 0)) for b in range(B)]


def walk_octaves(dtype, n_oct):
    """Octaves wave 0 walks alone: the block's share is at most 64 pixels."""
    OB, LV = BLOCK[dtype]
    return [k for k in range(1, min(LV, n_oct - 1) + 1) if (OB >> k) ** 2 <= 64]


def tail_octaves(dtype, n_oct):
    return list(range(BLOCK[dtype][1] + 1, n_oct))


def owner_map(dtype, H, W, k, path="scalar"):
    """Who produces pixel (y, x) of octave k (and reduces its key): dict of arrays [h_k, w_k] wg, wave, lane, and kernel
    ("block" | "tail" | "held") and walk (the wave-0 walk)."""
    dtype = str(dtype)
    h, w = H >> k, W >> k
    y, x = np.mgrid[0:h, 0:w]
    if dtype not in BLOCK:                              # minmax_f64_kernel / pool_f64_kernel: thread = pixel
        i = y * w + x
        return dict(kernel="held", walk=False, wg=i // 256, wave=(i % 256) >> 6, lane=i & 63)
    OB, LV = BLOCK[dtype]
    if k > LV:
        tid = (y * w + x) % 256
        return dict(kernel="tail", walk=False, wg=np.zeros_like(y), wave=tid >> 6, lane=tid & 63)
    ns = OB >> k
    by, bx = y // ns, x // ns
    r, c = y - by * ns, x - bx * ns
    walk = False
    if dtype == "float32":
        path = "scalar"
    if k == 0:
        it = (r // 2) * (OB // 16) + c // 16 if path == "regs" else r * (OB // 4) + c // 4 if path == "dword" else r * OB + c
        tid = it % 256
    elif k == 1 and path == "regs":
        tid = (r * (OB // 16) + c // 8) % 256
    elif ns * ns > 64:
        tid = (r * ns + c) % 256
    else:
        tid, walk = r * ns + c, True
    return dict(kernel="block", walk=walk, wg=by * (-(-W // OB)) + bx, wave=tid >> 6, lane=tid & 63)


def n_workgroups(dtype, H, W):
    OB = BLOCK[str(dtype)][0]
    return -(-H // OB) * -(-W // OB)


# ------------------------------------------------------------------------------ pooling
def pool4(a, b, c, d, fault=None):
    """One pooled pixel from a = [2r, 2c], b = [2r + 1, 2c], c = [2r, 2c + 1], d = [2r + 1, 2c + 1], in the arrays' dtype,
    as the kernels compute it; `fault` (PIXEL_FAULTS) gives what a wrong kernel would."""
    dt = a.dtype
    if dt == np.bool_:
        return a | b | c | d
    if dt.kind in "iu":
        bits = dt.itemsize * 8
        s = a.astype(np.int64) + b.astype(np.int64) + c.astype(np.int64) + d.astype(np.int64)
        if bits < 64 and fault != "nowrap":
            s = s & ((1 << bits) - 1)
            if dt.kind == "i":
                s = np.where(s >= (1 << (bits - 1)), s - (1 << bits), s)
        q = s >> 2 if fault == "floor" else np.where(s >= 0, s >> 2, -((-s) >> 2))
        return q.astype(dt)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if dt == np.float16:
            if fault == "single_f16":
                return ((a.astype(np.float64) + b + c + d) / 4).astype(np.float16)
            return (((a + b) + c) + d) / np.float16(4)
        if fault == "rowfirst":
            s = ((a + c) + b) + d
        elif fault == "pairwise":
            s = (a + b) + (c + d)
        elif fault == "reversed":
            s = ((d + c) + b) + a
        else:
            s = ((a + b) + c) + d
        return s * dt.type(0.25)


def pool_floor(arr, fault=None):
    """Octave k + 1 of octave k: floor dimensions, the odd last row and column dropped."""
    h, w = arr.shape[0] // 2, arr.shape[1] // 2
    return pool4(arr[0:2 * h:2, 0:2 * w:2], arr[1:2 * h:2, 0:2 * w:2], arr[0:2 * h:2, 1:2 * w:2], arr[1:2 * h:2, 1:2 * w:2], fault)


def hier_octaves(img, fault=None):
    """The octaves as the kernels derive them: (stored, padded).  uint8 / float32: every OB x OB block of the zero-padded
    image is pooled down on its own, octave k of the block is cropped to the (H >> k, W >> k) pixels that exist, and the
    octaves beyond the block's reach follow from the last of them by floor pooling (the tail kernel).  padded[k] is the
    whole grid of block shares, the pixels a kernel that let padding into its keys would see.  Held dtypes: the plain floor
    chain (padded is stored)."""
    H, W = img.shape
    dims = octave_dims(H, W)
    n_oct = len(dims)
    name = str(img.dtype)
    if name not in BLOCK:
        out = [img]
        for _ in range(1, n_oct):
            out.append(pool_floor(out[-1], fault))
        return out, out
    OB, LV = BLOCK[name]
    nby, nbx = -(-H // OB), -(-W // OB)
    top = min(LV, n_oct - 1)
    full = np.zeros((nby * OB, nbx * OB), img.dtype)
    full[:H, :W] = img
    padded = [full] + [np.zeros((nby * (OB >> k), nbx * (OB >> k)), img.dtype) for k in range(1, top + 1)]
    for by in range(nby):
        for bx in range(nbx):
            cur = full[by * OB:(by + 1) * OB, bx * OB:(bx + 1) * OB]
            for k in range(1, top + 1):
                cur = pool_floor(cur, fault)
                ns = OB >> k
                padded[k][by * ns:(by + 1) * ns, bx * ns:(bx + 1) * ns] = cur
    stored = [img] + [padded[k][:dims[k][0], :dims[k][1]] for k in range(1, top + 1)]
    for k in range(top + 1, n_oct):
        stored.append(pool_floor(stored[-1], fault))
        padded.append(stored[-1])
    return stored, padded


def packed_octave1(img, high_mask=0x3f):
    """Octave 1 of a uint8 image with W % 8 == 0 by the regs path's arithmetic: the byte pairs of two rows summed in the
    16-bit lanes of a dword, ((sum >> 2) & 0x3f) | (((sum >> 18) & high_mask) << 8) two pixels at a time."""
    H, W = img.shape
    assert img.dtype == np.uint8 and W % 8 == 0
    h = H // 2
    a = np.ascontiguousarray(img[0:2 * h:2]).view("<u4").astype(np.uint64)
    b = np.ascontiguousarray(img[1:2 * h:2]).view("<u4").astype(np.uint64)
    m = np.uint64(0x00ff00ff)
    e = np.uint64(8)
    s = (a & m) + ((a >> e) & m) + (b & m) + ((b >> e) & m)
    o = ((s >> np.uint64(2)) & np.uint64(0x3f)) | (((s >> np.uint64(18)) & np.uint64(high_mask)) << e)
    return np.ascontiguousarray(o.astype("<u2")).view(np.uint8).reshape(h, W // 2)


def wrong_octaves(img, fault):
    """The stored octaves a kernel with a PIXEL_FAULT would write (octave 0 is the image)."""
    if fault == "lane_carry":
        octs = [img, packed_octave1(img, 0xffffffff)]
        for _ in range(2, len(octave_dims(*img.shape))):
            octs.append(pool_floor(octs[-1]))
        return octs
    return hier_octaves(img, fault)[0]


# ------------------------------------------------------------------------------ keys
def key32(v):
    """The 32-bit order-preserving key of a uint8 or float32 pixel (PixKey)."""
    if isinstance(v, (np.uint8, int, np.integer)):
        return np.uint32(v)
    b = np.array([v], np.float32).view(np.uint32)[0]
    return np.uint32(~b) if b & np.uint32(0x80000000) else np.uint32(b | np.uint32(0x80000000))


def key64(v):
    """The 64-bit key of a held dtype's pixel, a float64 on the device (f64_key)."""
    b = np.array([v], np.float64).view(np.uint64)[0]
    return np.uint64(~b) if b >> np.uint64(63) else np.uint64(b | np.uint64(1 << 63))


def true_keys(octs):
    return [(o.min(), o.max()) for o in octs]


def emulated_keys(dtype, images, paths, fault, only=None):
    """[image][octave] -> (min, max) or None (the words stay zero), as a kernel with `fault` (KEY_FAULTS) in its reduction
    would report them: a wave's partial dropped, an octave's slot dropped, only lane 0's value kept, image b's keys
    written to image 0's words, padded pixels or the odd tails admitted.  `only`: the octaves the fault acts in (the
    others keep their true keys)."""
    dtype = str(dtype)
    B, H, W = images.shape
    out = []
    for b in range(B):
        stored, padded = hier_octaves(images[b])
        keys = []
        for k, o in enumerate(stored):
            vals = o
            if only is not None and k not in only:
                pass
            elif fault[0] == "wave" or fault[0] == "lane0":
                own = owner_map(dtype, H, W, k, paths[b])
                vals = o[own["wave"] != fault[1]] if fault[0] == "wave" else o[own["lane"] == 0]
            elif fault[0] == "padding":
                vals = padded[k]
            elif fault[0] == "odd_tails" and k == 1:
                z = np.zeros((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), o.dtype)
                z[:H, :W] = images[b]
                vals = pool_floor(z)
            keys.append((vals.min(), vals.max()) if vals.size and not (fault[0] == "slot" and k == fault[1]) else None)
        out.append(keys)
    if fault[0] == "image" and fault[1] < B:
        src = out[fault[1]]
        out[0] = [(min(p[0], q[0]), max(p[1], q[1])) for p, q in zip(out[0], src)]
        out[fault[1]] = [None] * len(src)
    return out


# ------------------------------------------------------------------------------ designs
EXTREME_VALUES = {"uint8": (32, 60, 5), "float32": (32.0, 4128.0, -4064.0), "int16": (-100, 700, -900),
                  "float64": (0.5, 4096.5, -4095.5)}          # background m, the higher and the lower plateau


def extremes(dtype, H, W, B, k, hi, lo):
    """Images [B, H, W] flat at m with, in image hi[0], a 2^k aligned square of the higher value over pixel hi[1:] of octave
    k, and in image lo[0] one of the lower value over lo[1:].  uint8 constants stay below 64 (((4 c) & 255) >> 2 == c), the
    float values are small integers (+ 0.5): a plateau survives pooling unchanged down to octave k, where it is ONE pixel."""
    m, vh, vl = EXTREME_VALUES[str(dtype)]
    imgs = np.full((B, H, W), m, np.dtype(dtype))
    for (b, y, x), v in ((hi, vh), (lo, vl)):
        assert (y + 1) << k <= H and (x + 1) << k <= W
        imgs[b, y << k:(y + 1) << k, x << k:(x + 1) << k] = v
    return imgs


def extremes_closed_form(dtype, H, W, B, k, hi, lo):
    """[image][octave] -> (background, squares [(y0, x0, side, value)]): the plateaus shrink to a pixel at octave k; above
    it each pixel is blended with three background pixels (or with the other plateau's, where they share a quad)."""
    dt = np.dtype(dtype)
    m, vh, vl = EXTREME_VALUES[str(dtype)]
    dims = octave_dims(H, W)
    out = []
    for b in range(B):
        mine = {(y, x): v for (bb, y, x), v in ((hi, vh), (lo, vl)) if bb == b}
        per = []
        for j, (h, w) in enumerate(dims):
            if j <= k:
                sq = [(y << (k - j), x << (k - j), 1 << (k - j), v) for (y, x), v in mine.items()]
            else:
                nxt = {}
                for (y, x) in mine:
                    py, px = y >> 1, x >> 1
                    if py < h and px < w and (py, px) not in nxt:
                        q = [np.array([mine.get((2 * py + dy, 2 * px + dx), m)], dt) for dx in (0, 1) for dy in (0, 1)]
                        nxt[(py, px)] = pool4(*q)[0]
                mine = nxt
                sq = [(y, x, 1, v) for (y, x), v in mine.items()]
            per.append((dt.type(m), sq))
        out.append(per)
    return out


def render(shape, form):
    m, squares = form
    o = np.full(shape, m, m.dtype)
    for y0, x0, s, v in squares:
        o[y0:y0 + s, x0:x0 + s] = v
    return o


def pick_owner(dtype, H, W, path, k, wg, wave, nth=0):
    """A pixel (y, x) of octave k owned by workgroup `wg` ("first" | "last" | "any") and wave `wave` (None: any), in a lane
    other than 0 where the owner has one; None if the owner holds no pixel of that octave."""
    own = owner_map(dtype, H, W, k, path)
    sel = np.ones(own["wave"].shape, bool)
    if wg != "any":
        sel &= own["wg"] == (0 if wg == "first" else own["wg"].max())     # (the last workgroup that holds a pixel of the octave)
    if wave is not None:
        sel &= own["wave"] == wave
    if (sel & (own["lane"] != 0)).any():
        sel &= own["lane"] != 0
    at = np.argwhere(sel)
    if not len(at):
        return None
    return tuple(int(v) for v in at[min(nth, len(at) - 1)])


BAIT_VALUES = {"uint8": (20, 0, 255, 200), "float32": (1.0, -3.0e38, 3.0e38, 1000.0)}       # m, lowest, highest, bright


def tail_bait(dtype, H, W, B, variant):
    """Flat images of odd H and / or W.  "corner": the odd last row holds the image's only lowest value, the odd last column
    (the last row again where W is even) its only highest: they belong to octave 0's keys and to nothing else.  "pairs":
    vertical pairs of a bright value in the odd last column and horizontal pairs in the odd last row, next to the padding:
    a kernel that let the padded quad into its keys would report half of it as octave 1's maximum."""
    m, vlo, vhi, bright = BAIT_VALUES[str(dtype)]
    imgs = np.full((B, H, W), m, np.dtype(dtype))
    assert H % 2 or W % 2
    for b in range(B):
        if variant == "corner":
            if H % 2:
                imgs[b, H - 1, 5 + 3 * b] = vlo
            else:
                imgs[b, 4 + 2 * b, W - 1] = vlo
            if W % 2:
                imgs[b, 6 + 2 * b, W - 1] = vhi
            else:
                imgs[b, H - 1, W - 3 - 2 * b] = vhi
        else:
            if W % 2:
                imgs[b, 2 + 2 * b:H - 1 - (H % 2):6, W - 1] = bright
                imgs[b, 3 + 2 * b:H - (H % 2):6, W - 1] = bright
            if H % 2:
                imgs[b, H - 1, 2 + 2 * b:W - 1 - (W % 2):6] = bright
                imgs[b, H - 1, 3 + 2 * b:W - (W % 2):6] = bright
    return imgs


@functools.lru_cache(None)
def quad_list():
    """uint8 quads (a, b, c, d): every sum 0 .. 1020 in four splits -- even, greedy from a (a and a + b saturate first: bytes
    of 255, a + b alone at or above 256), greedy from d, and random."""
    rng = np.random.default_rng(77)
    out = []
    for s in range(1021):
        q, r = divmod(s, 4)
        even = [q + (i < r) for i in range(4)]
        g, rest = [], s
        for _ in range(4):
            g.append(min(rest, 255))
            rest -= g[-1]
        rnd, rest = [], s
        for left in (3, 2, 1, 0):                              # each value within what the others can still make up
            rnd.append(int(rng.integers(max(0, rest - 255 * left), min(255, rest) + 1)))
            rest -= rnd[-1]
        rnd = [rnd[i] for i in rng.permutation(4)]
        out += [even, g, g[::-1], rnd]
    return np.array(out, np.uint8)[rng.permutation(len(out))]          # (no sum tied to a row or column of the image)


def _fill_quads(H, W, B, quads, fill, step):
    """Quads laid row-major over the 2 x 2 cells of [B, H, W] images, cyclically, image b starting `step` * b quads into
    the list (the same quad then sits at another column, lane and block in each image); odd tails hold `fill`."""
    h, w = H // 2, W // 2
    imgs = np.full((B, H, W), fill, quads.dtype)
    for b in range(B):
        q = quads[(np.arange(h * w) + step * b) % len(quads)].reshape(h, w, 4)
        imgs[b, 0:2 * h:2, 0:2 * w:2] = q[..., 0]
        imgs[b, 1:2 * h:2, 0:2 * w:2] = q[..., 1]
        imgs[b, 0:2 * h:2, 1:2 * w:2] = q[..., 2]
        imgs[b, 1:2 * h:2, 1:2 * w:2] = q[..., 3]
    return imgs


def quads(H, W, B):
    """quad_list over the image: 136 cells to a row at W = 272 and 4084 quads, so every quad lands on several column
    positions of a 16-pixel group and on both sides of the 128-pixel seams."""
    return _fill_quads(H, W, B, quad_list(), np.uint8(77), 1531)


@functools.lru_cache(None)
def float_quad_list():
    """float32 quads: values of mixed magnitude (order-sensitive sums), then quads that overflow to +inf and to -inf (the
    first two alone, or only the whole sum), values near FLT_MAX / 4 whose sum stays finite, and subnormals whose quarter
    is subnormal (a multiply by 0.25 that flushed them would show).  Finite, no zero, no NaN."""
    rng = np.random.default_rng(78)
    n = 2000
    mixed = (rng.standard_normal((n, 4)) * np.exp2(rng.integers(-8, 9, (n, 4)))).astype(np.float32)
    mixed[mixed == 0] = np.float32(1.0)
    fmax = np.finfo(np.float32).max
    big = []
    for sign in (1.0, -1.0):
        for i in range(24):
            t = np.float32(fmax * (0.55 + 0.015 * i))
            q = [t, t, np.float32(1e30 * (i + 1)), np.float32(3e29)] if i % 2 else [np.float32(fmax * 0.3), np.float32(fmax * 0.3), t, np.float32(1e36)]
            big.append([np.float32(sign) * v for v in q])
    near = [[np.float32(fmax * f) for f in (0.2499 - 1e-4 * i, 0.2499, 0.2499 - 2e-4 * i, 0.2501)] for i in range(24)]
    tiny = np.float32(2.0 ** -149)
    sub = [[tiny * np.float32(8 + (3 * i + j) % 23) for j in range(4)] for i in range(64)]
    return mixed, np.array(big, np.float32), np.array(near, np.float32), np.array(sub, np.float32)


def float_quads(H, W, B):
    """Mixed-magnitude quads everywhere; where the image has room (H >= 32, W >= 128) the +inf quads fill the cells of columns
    0 .. 3 and rows 0 .. 5, the -inf quads cells half an image to the right (a pixel of the last octave spans less than a
    quarter of the width, so +inf and -inf never meet in a quad: the host test asserts no NaN in any octave), the
    near-FLT_MAX / 4 quads the cells of columns 16 .. 19, and the subnormal quads those of columns 24 .. 31, rows 0 .. 7."""
    mixed, big, near, sub = float_quad_list()
    imgs = _fill_quads(H, W, B, mixed, np.float32(0.75), 517)
    if H >= 32 and W >= 128:
        far = max(32, (W // 4) & ~7)                  # the -inf cells: half an image away from the +inf ones
        for b in range(B):
            def put(q, r0, c0, nr, nc):
                q = q[(np.arange(nr * nc) + b) % len(q)].reshape(nr, nc, 4)
                blk = imgs[b, 2 * r0:2 * (r0 + nr), 2 * c0:2 * (c0 + nc)]
                blk[0::2, 0::2], blk[1::2, 0::2], blk[0::2, 1::2], blk[1::2, 1::2] = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
            put(big[:24], 0, 0, 6, 4)
            put(big[24:], 0, far, 6, 4)
            put(near, 0, 16, 6, 4)
            put(sub, 0, 24, 8, 8)
    return imgs


def _split4(s, lo, hi, rng, greedy):
    """Four integers of [lo, hi] that sum to s: near-even, or saturating from the first."""
    if greedy:
        out, rest = [], s
        for i in range(4):
            left = 3 - i
            v = min(hi, max(lo, rest - (lo * left if s >= 0 else hi * left)))
            v = min(hi, max(lo, v))
            # keep the remainder reachable by the values still to come
            v = max(v, rest - hi * left)
            v = min(v, rest - lo * left)
            out.append(v)
            rest -= v
        assert rest == 0
        return out
    q, r = divmod(s, 4)
    out = [q + (i < r) for i in range(4)]
    if all(lo < v < hi for v in out):
        j = int(rng.integers(1, 1 + min(1000, hi - max(out), min(out) - lo)))
        out[0] += j
        out[3] -= j
    return out


@functools.lru_cache(None)
def held_quad_list(dtype):
    """Quads of a held dtype, see held_quads."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(79 + sum(dtype.encode()))
    if dt == np.bool_:
        return np.array([[(p >> i) & 1 for i in range(4)] for p in range(16)], np.bool_)
    if dt == np.float16:
        n = 300
        q = (rng.standard_normal((n, 4)) * np.exp2(rng.integers(-4, 8, (n, 4)))).astype(np.float16)
        q[::5] = np.array([2048, 1, 1, 1], np.float16) * np.exp2(rng.integers(-6, 3, (len(q[::5]), 1))).astype(np.float16)
        return q
    if dt == np.float64:
        return rng.standard_normal((300, 4)) * np.exp2(rng.integers(-20, 21, (300, 4)))
    bits = dt.itemsize * 8
    lo, hi = (-(1 << 50), 1 << 50) if bits == 64 else (int(np.iinfo(dt).min), int(np.iinfo(dt).max))
    sums = []
    if bits < 64:
        half = 1 << (bits - 1)
        bounds = [half, 3 * half, -half, -3 * half] if dt.kind == "i" else [2 * half, 4 * half, 6 * half]
        sums += [bd + e for bd in bounds for e in range(-5, 6)]
    if dt.kind == "i":
        sums += list(range(-16, 1)) + [-(1 << (bits - 2 if bits < 64 else 48)) - e for e in range(8)]
    if bits == 64:
        sums += [4 * hi - e for e in range(8)] + [4 * lo + e for e in range(8)] + [(1 << 50) + e for e in range(8)]
    sums = [s for s in sums if 4 * lo <= s <= 4 * hi]
    out = [_split4(s, lo, hi, rng, g) for s in sums for g in (False, True)]
    full = rng.integers(lo, hi, (200, 4), dtype=np.int64, endpoint=True)
    return np.concatenate([np.array(out, np.int64), full]).astype(dt)


def held_quads(dtype, H, W, B):
    """The integer types: sums on and beside every wrap boundary of the type from both sides (odd multiples of 2^(bits-1)
    for the signed, multiples of 2^bits for the unsigned), negative sums of every residue mod 4, values of the whole range;
    int64: values up to 2^50, no wrap.  bool: the 16 patterns.  float16: quads whose sum rounds differently after each add
    than once (2048 + 1 + 1 + 1).  float64: mixed magnitudes."""
    q = held_quad_list(dtype)
    fill = q.dtype.type(1) if q.dtype != np.bool_ else np.bool_(False)
    return _fill_quads(H, W, B, q, fill, 97)


# ------------------------------------------------------------------------------ the cases
def _case(design, dtype, H, W, B, **args):
    tag = "-".join(f"{k}{v}" for k, v in args.items() if k not in ("hi", "lo"))
    pos = "".join(f"-{n}{'.'.join(map(str, args[n]))}" for n in ("hi", "lo") if n in args)
    return dict(id=f"{design}-{dtype}-{H}x{W}x{B}" + (f"-{tag}" if tag else "") + pos, design=design, dtype=dtype, H=H, W=W, B=B, args=args)


def _extreme_cases():
    """The ownership sweep.  Per (dtype, shape, k): extremes in wave w of the first workgroup and wave w + 1 of the last, and
    the other way round, for every wave the two workgroups have at that octave; the wave-0 walk and tail octaves with one
    extreme in the first and one in the last workgroup; waves w and w + 1 of the tail kernel; batches of 3 with the maximum alone in image b and the minimum
    alone in image b + 1."""
    out = []

    def add(dtype, H, W, B, k, hi_want, lo_want, slots=(0, 0)):
        paths = batch_paths(dtype, H, W, B)
        hi = pick_owner(dtype, H, W, paths[slots[0]], k, *hi_want)
        lo = pick_owner(dtype, H, W, paths[slots[1]], k, *lo_want, nth=3)
        if hi is None or lo is None:
            return
        if slots[0] == slots[1] and hi == lo:
            lo = pick_owner(dtype, H, W, paths[slots[1]], k, *lo_want, nth=7)
        if slots[0] != slots[1] or hi != lo:
            out.append(_case("extremes", dtype, H, W, B, k=k, hi=(slots[0],) + hi, lo=(slots[1],) + lo))

    sweeps = [("uint8", 200, 208, (0, 1)), ("uint8", 201, 213, (0, 1, 2)), ("uint8", 200, 212, (0,)), ("float32", 100, 108, (0, 1, 2))]
    for dtype, H, W, ks in sweeps:
        for k in ks:
            for w in range(4):
                add(dtype, H, W, 1, k, ("first", w), ("last", (w + 1) % 4))
                add(dtype, H, W, 1, k, ("last", w), ("first", (w + 1) % 4))
    # the issue's seam shapes: one extreme on each side of a block seam
    for dtype, H, W in (("uint8", 129, 144), ("uint8", 131, 260), ("float32", 65, 80), ("float32", 67, 132)):
        for k in (0, 1):
            add(dtype, H, W, 1, k, ("first", None), ("last", None))
    # the wave-0 walk (uint8: octaves 4 .. 7, float32: 3 .. 6) and the tail kernel's octaves
    for dtype, H, W in (("uint8", 200, 208), ("uint8", 1024, 1040), ("uint8", 2048, 2064), ("float32", 100, 108), ("float32", 1024, 1040)):
        n_oct = len(octave_dims(H, W))
        for k in walk_octaves(dtype, n_oct) + tail_octaves(dtype, n_oct):
            if (H, W) == (2048, 2064) and k < 8:
                continue                                      # (1024 x 1040 holds the walk)
            add(dtype, H, W, 1, k, ("first", None), ("last", None))
            add(dtype, H, W, 1, k, ("last", None), ("first", None))
    # the tail kernel's four waves: extremes in wave w and wave w + 1 of its one workgroup, both ways round
    for dtype, H, W in TAIL_WAVE_SHAPES:
        k = tail_octaves(dtype, len(octave_dims(H, W)))[-1]
        for w in range(4):
            add(dtype, H, W, 1, k, ("any", w), ("any", (w + 1) % 4))
            add(dtype, H, W, 1, k, ("any", (w + 1) % 4), ("any", w))
    # batches of 3: 200 x 208 and 72 x 80 / 73 x 80 (image 1 leaves the regs path), float32, and two held dtypes
    for dtype, H, W, ks in (("uint8", 200, 208, (0, 1, 4)), ("uint8", 72, 80, (0, 1, 3)), ("uint8", 73, 80, (1,)), ("float32", 100, 108, (0, 1, 3)),
                            ("int16", 40, 76, (0, 1, 2)), ("float64", 40, 76, (0, 1, 2))):
        for k in ks:
            for b in range(3):
                add(dtype, H, W, 3, k, ("any", 1 if k < 2 else None), ("any", 2 if k < 2 else None), slots=(b, (b + 1) % 3))
    for dtype in ("int16", "float64"):                            # (one atomic per wave: each wave of the first and last workgroup)
        for k in (0, 1):
            for w in range(4):
                add(dtype, 40, 76, 1, k, ("first", w), ("last", (w + 1) % 4))
                add(dtype, 40, 76, 1, k, ("last", w), ("first", (w + 1) % 4))
        add(dtype, 40, 76, 1, 2, ("first", 1), ("last", None))
    seen = set()
    return [c for c in out if not (c["id"] in seen or seen.add(c["id"]))]


def _all_cases():
    out = _extreme_cases()
    for dtype, H, W, B in (("uint8", 131, 133, 1), ("uint8", 131, 133, 3), ("uint8", 131, 144, 1), ("uint8", 129, 145, 1), ("uint8", 2049, 2065, 1),
                           ("float32", 67, 133, 1), ("float32", 67, 133, 3), ("float32", 65, 80, 1)):
        for variant in ("corner", "pairs"):
            out.append(_case("tail_bait", dtype, H, W, B, variant=variant))
    for H, W, B in ((131, 272, 1), (131, 272, 3), (72, 80, 3), (73, 80, 3), (131, 132, 1), (131, 132, 3), (131, 133, 1), (131, 133, 3),
                    (129, 144, 1), (131, 260, 1), (8, 8, 1), (8, 16, 1), (9, 23, 3), (1024, 1040, 1), (2048, 2064, 1)):
        out.append(_case("quads", "uint8", H, W, B))
    for H, W, B in ((67, 132, 1), (67, 132, 3), (65, 80, 1), (8, 8, 1), (8, 16, 1), (9, 23, 3), (1024, 1040, 1)):
        out.append(_case("float_quads", "float32", H, W, B))
    for dtype in HELD:
        for B in (1, 3):
            out.append(_case("held_quads", dtype, 37, 50, B))
    return out


CASES = _all_cases()
# what the GPU module claims for the path of every image of the uint8 batches where the path is the point
PATH_CLAIMS = {(72, 80, 3): ["regs", "dword", "regs"], (73, 80, 3): ["regs", "dword", "regs"], (131, 132, 1): ["dword"],
               (131, 132, 3): ["dword"] * 3, (131, 133, 1): ["scalar"], (131, 133, 3): ["scalar"] * 3, (131, 272, 1): ["regs"],
               (131, 272, 3): ["regs"] * 3, (200, 208, 3): ["regs", "dword", "regs"], (200, 208, 1): ["regs"], (200, 212, 1): ["dword"],
               (201, 213, 1): ["scalar"]}
# the C ABI runs of one 131 x 272 image: (bytes the image pointer is off a 16-byte boundary, elements added to every octave
# offset) -> the path load_path must give
CABI_RUNS = [((0, 0), "regs"), ((0, 2), "dword"), ((4, 0), "dword"), ((4, 2), "dword"), ((1, 0), "scalar"), ((1, 2), "scalar")]
CABI_SHAPE = (131, 272)


def case_id(c):
    return c["id"]


@functools.lru_cache(None)
def _images(cid):
    c = next(c for c in CASES if c["id"] == cid)
    fn = {"extremes": extremes, "tail_bait": tail_bait, "quads": lambda dt, *a: quads(*a), "float_quads": lambda dt, *a: float_quads(*a),
          "held_quads": held_quads}[c["design"]]
    imgs = fn(c["dtype"], c["H"], c["W"], c["B"], **c["args"])
    imgs.setflags(write=False)
    return imgs


def images(case):
    """The case's batch [B, H, W], read-only and shared."""
    return _images(case["id"])


@functools.lru_cache(None)
def _reference(cid):
    imgs = _images(cid)
    return [list(orc.image_octaves(im)) for im in imgs]


def reference(case):
    """[image][octave] -> the oracle's octave (orc.image_octaves), computed once per case."""
    return _reference(case["id"])


def cabi_images():
    """The two images of the C ABI differential: quads, and extremes with one extreme on each side of the block seam."""
    H, W = CABI_SHAPE
    return {"quads": quads(H, W, 1)[0], "extremes": extremes("uint8", H, W, 1, 1, (0, 5, 9), (0, 64, 130))[0]}


def describe_mismatch(case, b, k, got, ref):
    """Names the first differing pixel of an octave and its owner."""
    diff = np.argwhere(~(np.ascontiguousarray(got).view(np.uint8).reshape(got.shape + (-1,))
                         == np.ascontiguousarray(ref).view(np.uint8).reshape(ref.shape + (-1,))).all(-1))
    y, x = (int(v) for v in diff[0])
    path = batch_paths(case["dtype"], case["H"], case["W"], case["B"])[b]
    own = owner_map(case["dtype"], case["H"], case["W"], k, path)
    return (f"{case['id']}: image {b} (path {path}) octave {k}: {len(diff)} pixels differ, first at ({y}, {x}) = {got[y, x]!r} against "
            f"{ref[y, x]!r}, {own['kernel']} kernel workgroup {int(own['wg'][y, x])} wave {int(own['wave'][y, x])} lane {int(own['lane'][y, x])}"
            + (" (wave-0 walk)" if own["walk"] else ""))
