"""Designed detection / ground-truth sets for the matching kernel (wb_match.hip), where the test decides which candidate owns
every detection, and a NumPy emulation of the kernel with a switch for each way a rewrite could go wrong.  No GPU, no torch.

* Every ground-truth box sits in a cell of its own (cells are CELL apart), a detection inside the cell of the box it is
  planted on: it overlaps that box, the box's twins (identical boxes at other indices: the LOWER index must win) and its decoy
  (a box in the same cell that overlaps less) and nothing else.  `none` detections sit in a cell without any box: IoU 0
  with every candidate, so candidate 0 owns them.
* images(): the images in detection order.  Their sizes put image boundaries at detections 63 | 64 and 255 | 256 and inside
  a workgroup (the straddling path), whole workgroups on one image with 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 1 candidates (the
  LDS path), an image without ground truth, one without detections, degenerate boxes, coordinates that are no float32
  values, and general float64 boxes whose IoU a float32 or a fused computation gets wrong.
* iou_exact(): the contract's operation sequence, every operation done in exact rational arithmetic and rounded once.
* emulate(): the kernel's two paths in NumPy; FAULTS names its switches.
tests/test_match_designs_host.py proves all of it on the CPU; tests/test_gpu_match_designs.py runs it."""
import functools
from fractions import Fraction

import numpy as np

CHUNK = 64               # WB_MATCH_CHUNK
WG = 256                 # detections per workgroup
CELL = 32
CELLS_X = 512
NONE = -2                # a detection planted on no box


def cell_origin(c):
    return float(CELL * (c % CELLS_X)), float(CELL * (c // CELLS_X))


class Image:
    """One image: gt [G, 4] float64, dt [n, 4] float64, plant [n]: the index the construction says owns each detection
    (NONE: overlaps nothing -> 0, or -1 without ground truth)."""

    def __init__(self, name, gt, dt, plant):
        self.name = name
        self.gt = np.asarray(gt, np.float64).reshape(-1, 4)
        self.dt = np.asarray(dt, np.float64).reshape(-1, 4)
        self.plant = np.asarray(plant, np.int64).reshape(-1)
        assert self.plant.size == self.dt.shape[0]

    @property
    def want_owner(self):
        none = -1 if len(self.gt) == 0 else 0
        return np.where(self.plant == NONE, none, self.plant).astype(np.int32)


_next_cell = [0]


def _cells(n):
    c = _next_cell[0]
    _next_cell[0] += n
    return c


def planted_image(name, G, n, seed, twins=(), decoys=(), first=()):
    """G boxes of 10 x 10 at integer coordinates, one per cell; twins: (k1, k2) box k2 becomes a copy of box k1 (k1 < k2);
    decoys: (k, at) box `at` becomes box k moved by 8 in x.  Detection j is planted on first[j] while that lasts, then on a
    seeded choice among the boxes that are not decoys or later twins; every 17th overlaps nothing.  A detection on box k is
    box k moved by 1, 2 or 3 in x: IoU 90/110, 80/120 or 70/130 with it, at most 50/150 with its decoy."""
    rng = np.random.default_rng(seed)
    base = _cells(G + 1)
    gt = np.zeros((G, 4))
    for k in range(G):
        ox, oy = cell_origin(base + k)
        gt[k] = [ox, oy, ox + 10, oy + 10]
    taken = set()
    for k1, k2 in twins:
        assert k1 < k2 < G and k2 not in taken
        gt[k2] = gt[k1]
        taken.add(k2)
    for k, at in decoys:
        assert at < G and at not in taken and k != at
        gt[at] = gt[k] + [8, 0, 8, 0]
        taken.add(at)
    free = [k for k in range(G) if k not in taken]
    ex, ey = cell_origin(base + G)                             # the cell without a box
    dt, plant = np.zeros((n, 4)), np.zeros(n, np.int64)
    for j in range(n):
        if G == 0 or (j % 17 == 16 and j >= len(first)):
            dt[j], plant[j] = [ex + j % 5, ey, ex + j % 5 + 10, ey + 10], NONE
            continue
        k = first[j] if j < len(first) else free[int(rng.integers(0, len(free)))]
        assert k in free
        s = 1 + j % 3
        dt[j], plant[j] = gt[k] + [s, 0, s, 0], k
    return Image(name, gt, dt, plant)


def degenerate_image(name, n):
    """Box 0 is a point, box 1 an ordinary box around it, box 2 a line inside box 1, box 3 a copy of box 1.  Point and line
    detections have union 0 with their like and intersection 0 with everything: owner 0, best 0."""
    base = _cells(1)
    ox, oy = cell_origin(base)
    gt = np.array([[ox + 3, oy + 3, ox + 3, oy + 3], [ox, oy, ox + 10, oy + 10], [ox + 5, oy + 1, ox + 5, oy + 9], [ox, oy, ox + 10, oy + 10]])
    kinds = [(gt[0], NONE), (gt[2], NONE), (gt[1] + [2, 0, 2, 0], 1), (gt[1], 1), ([ox + 5, oy + 5, ox + 5, oy + 5], NONE)]
    dt = np.array([kinds[j % 5][0] for j in range(n)], np.float64)
    return Image(name, gt, dt, [kinds[j % 5][1] for j in range(n)])


def general_image(name, G, n, seed, fractions_only=False):
    """Boxes with coordinates that are no float32 values.  fractions_only: the planted geometry plus 0.1 and 0.3; otherwise
    general doubles: a box of 8 .. 20 a side inside its cell, the detection that box with every corner moved by up to 2."""
    rng = np.random.default_rng(seed)
    base = _cells(G)
    gt = np.zeros((G, 4))
    for k in range(G):
        ox, oy = cell_origin(base + k)
        if fractions_only:
            gt[k] = [ox + 0.1, oy + 0.3, ox + 10.1, oy + 10.3]
        else:
            x, y = ox + rng.uniform(3, 6), oy + rng.uniform(3, 6)
            gt[k] = [x, y, x + rng.uniform(8, 20), y + rng.uniform(8, 20)]
    plant = rng.integers(0, G, n)
    plant[:G] = np.arange(G)[:n]
    if fractions_only:
        dt = gt[plant] + np.array([0.7, 0.2, 0.7, 0.2]) * (1 + np.arange(n) % 3)[:, None]
    else:
        dt = gt[plant] + rng.uniform(-2, 2, (n, 4))
    return Image(name, gt, dt, plant)


@functools.lru_cache(None)
def images():
    _next_cell[0] = 0
    C = CHUNK
    out = [
        # workgroup 0 straddles: the boundary at detections 63 | 64, the next at 255 | 256
        planted_image("one-candidate-64-dets", 1, 64, 1),
        planted_image("three-candidates-twin-192-dets", 3, 192, 2, twins=[(0, 2)], first=[0, 1, 0]),
        # whole workgroups on one image: the LDS path
        planted_image("two-chunks-plus-1", 2 * C + 1, WG, 3, twins=[(C - 1, C), (5, 2 * C - 1)], decoys=[(2 * C, 0), (1, C + 7), (C + 1, 2)],
                      first=[2 * C, 1, C - 1, C + 1, 5, C - 2, 2 * C - 2, 3]),
        planted_image("chunk-plus-1", C + 1, WG, 4, twins=[(0, C - 1)], decoys=[(C, 1)], first=[C, 0, C - 2, 2]),
        planted_image("one-chunk", C, WG, 5, twins=[(7, C - 1)], decoys=[(0, C - 2)], first=[0, 7, C - 3]),
        planted_image("one-candidate-256-dets", 1, WG, 6),
        # workgroup 5 on: boundaries inside workgroups
        planted_image("no-ground-truth", 0, 100, 7),
        planted_image("no-detections", 5, 0, 8),
        general_image("fractions-not-float32", 6, 121, 9, fractions_only=True),
        degenerate_image("degenerate", 100),
        general_image("general-float64", 12, 191, 10),
        # the last workgroup is not full and is all one image
        planted_image("tail-109-dets", 8, 109, 11, twins=[(2, 6)], decoys=[(7, 0)], first=[7, 2, 1]),
    ]
    return out


class Scene:
    """The call's arrays for a list of images."""

    def __init__(self, imgs):
        self.images = list(imgs)
        self.dt = np.ascontiguousarray(np.concatenate([g.dt for g in imgs]))
        self.gt = np.ascontiguousarray(np.concatenate([g.gt for g in imgs]))
        self.dt_image = np.repeat(np.arange(len(imgs)), [len(g.dt) for g in imgs]).astype(np.int32)
        self.gt_off = np.concatenate([[0], np.cumsum([len(g.gt) for g in imgs])]).astype(np.int32)
        self.want_owner = np.concatenate([g.want_owner for g in imgs]).astype(np.int32)
        self.want_best = np.array([iou_float(self.dt[i], self.gt[self.gt_off[b] + o]) if o >= 0 else 0.0
                                   for i, (b, o) in enumerate(zip(self.dt_image, self.want_owner))], np.float64)
        self.n_dt, self.n_gt, self.n_images = len(self.dt), len(self.gt), len(imgs)

    def name_of(self, i):
        b = int(self.dt_image[i])
        return f"detection {i} (workgroup {i // WG}, thread {i % WG}; image {b} '{self.images[b].name}', its detection {i - int(np.searchsorted(self.dt_image, b))})"


@functools.lru_cache(None)
def scene():
    return Scene(images())


def describe_mismatch(s, best, owner):
    bad = np.flatnonzero((np.asarray(owner) != s.want_owner) | (np.asarray(best, np.float64).view(np.uint64) != s.want_best.view(np.uint64)))
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return (f"{bad.size} detections differ, first {s.name_of(i)}: owner {owner[i]} (want {s.want_owner[i]}), "
            f"best {float(best[i])!r} (want {float(s.want_best[i])!r})")


# ------------------------------------------------------------------------------ the contract's arithmetic
def iou_float(a, b):
    """boxes.iou's operation sequence on Python floats (IEEE doubles: every operation rounded once)."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    uni = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / uni if uni > 0 else 0.0


def iou_exact(a, b, fused=False):
    """The same with every operation done exactly (Fraction) and rounded once to a double; fused: the union as ONE
    rounding of area_a + area_b - iw * ih's last step, fma(-iw, ih, area_a + area_b)."""
    F = lambda v: Fraction(float(v))
    op = lambda x: F(float(x))                                  # (Fraction -> double is correctly rounded)
    a, b = [F(v) for v in a], [F(v) for v in b]
    iw = op(max(min(a[2], b[2]) - max(a[0], b[0]), 0))
    ih = op(max(min(a[3], b[3]) - max(a[1], b[1]), 0))
    inter = op(iw * ih)
    s = op(op(op(a[2] - a[0]) * op(a[3] - a[1])) + op(op(b[2] - b[0]) * op(b[3] - b[1])))
    uni = op(s - iw * ih) if fused else op(s - inter)
    return float(inter / uni) if uni > 0 else 0.0


def disjoint(a, b):
    """Proved from the coordinates alone: the boxes share no interior, so iw or ih is exactly 0."""
    return bool(min(a[2], b[2]) <= max(a[0], b[0]) or min(a[3], b[3]) <= max(a[1], b[1]))


# ------------------------------------------------------------------------------ the kernel in NumPy
FAULTS = ("last_max", "ge", "f32", "fused", "shift_image", "stale_chunk", "owner_global")


def iou_table(dt, gt, faults=()):
    """match_iou for every (detection, candidate) pair, operation by operation."""
    T = np.float32 if "f32" in faults else np.float64
    A, B, zero = dt.astype(T), gt.astype(T), T(0)
    ax1, ay1, ax2, ay2 = (A[:, None, k] for k in range(4))
    bx1, by1, bx2, by2 = (B[None, :, k] for k in range(4))
    iw = np.where(ax2 < bx2, ax2, bx2) - np.where(ax1 > bx1, ax1, bx1)
    ih = np.where(ay2 < by2, ay2, by2) - np.where(ay1 > by1, ay1, by1)
    iw, ih = np.where(iw < 0, zero, iw), np.where(ih < 0, zero, ih)
    inter = iw * ih
    s = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)
    uni = s - inter
    if "fused" in faults:
        uni = uni.copy()
        for r, c in zip(*np.nonzero(inter > 0)):
            uni[r, c] = float(Fraction(float(s[r, c])) - Fraction(float(iw[r, c])) * Fraction(float(ih[r, c])))
    return np.where(uni > 0, inter / np.where(uni > 0, uni, 1), zero).astype(np.float64)


def emulate(s, faults=(), prefill=(-7.0, -7)):
    """(best, owner) as match_kernel computes them, workgroup by workgroup, with `faults`."""
    faults = tuple(faults)
    assert all(f in FAULTS for f in faults), faults
    best, owner = np.full(s.n_dt, prefill[0], np.float64), np.full(s.n_dt, prefill[1], np.int32)
    clamp = lambda v: min(max(int(v), 0), s.n_gt)
    for w0 in range(0, s.n_dt, WG):
        idx = np.arange(w0, min(w0 + WG, s.n_dt))
        imgs = np.clip(s.dt_image[idx], 0, s.n_images - 1)
        one_image = len(set(imgs.tolist())) == 1
        for b in sorted(set(imgs.tolist())):
            at = idx[imgs == b]
            bb = b + 1 if "shift_image" in faults else b
            lo, hi = (clamp(s.gt_off[bb]), clamp(s.gt_off[bb + 1])) if bb + 1 <= s.n_images else (0, 0)
            hi = max(hi, lo)
            G = hi - lo
            if G == 0:
                best[at], owner[at] = 0.0, -1
                continue
            cand = np.arange(lo, hi)
            if one_image and "stale_chunk" in faults:          # the LDS still holds the first chunk
                cand = lo + (cand - lo) % CHUNK
            t = iou_table(s.dt[at], s.gt[cand], faults)
            if "last_max" in faults or "ge" in faults:         # (a `>=` update walks on to the last maximum)
                o = G - 1 - np.argmax(t[:, ::-1], axis=1)
            else:
                o = np.argmax(t, axis=1)
            best[at] = t[np.arange(len(at)), o]
            owner[at] = o + (lo if "owner_global" in faults else 0)
    return best, owner
