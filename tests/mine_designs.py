"""Designed record sets for the mining kernels (wb_mine.hip), where the construction decides which windows are chosen and
how they are labelled, and NumPy emulations of the kernels with a switch for each way a rewrite could go wrong.  No GPU,
no torch.

* Label scenes: 10 x 10 windows at integer positions on level 0 (scale 1), every ground-truth box in a cell of its own
  (cells are CELL apart); a window moved by s = 1, 2, 3 columns off its box has IoU 90/110, 80/120, 70/130 with it and 0 with
  everything else.  The thresholds sit on double(80/120), one double below and one above it.
* Select scenes: the winners are planted through the inverse of fmix32 -- the test picks the KEYS of a group's windows
  and derives their (r, c): keys 0 .. K-1 win whatever else the group holds.
* Gather scenes: a pyramid buffer whose every element encodes (image, level, row, col, channel).
* emulate_select(): the kernel's digit-histogram select in NumPy; emulate_gather(); FAULTS names their switches.
tests/test_mine_designs_host.py proves all of it on the CPU; tests/test_gpu_mine_designs.py runs it."""
import functools

import numpy as np

import mine_reference as ref

CELL = 32
M = N = 10
TP, FP = ref.TP, ref.FP
DEFAULTS = dict(min_tp_iou=0.7, max_fp_iou=0.3, max_tp=100, max_fp=100, want_tp=True, want_fp=True, seed=0)
V2 = 80.0 / 120.0            # the IoU of a window two columns off its box (test_mine_designs_host proves it from Fractions)


class Scene:
    """One call: det (ref.DET, shuffled), inv_scale, (m, n), gts / ignores per image, serial per image, params, and
    expect = {(image, level, r, c): (label, owner)} of the windows the construction says are chosen."""

    def __init__(self, name, det, gts, ignores, serial, expect, inv_scale=(1.0,), m=M, n=N, shuffle=1, **params):
        assert set(params) <= set(DEFAULTS), params
        self.name, self.m, self.n = name, m, n
        det = np.asarray(det, ref.DET).reshape(-1)
        self.det = det[np.random.default_rng(shuffle).permutation(det.size)] if shuffle else det
        self.inv_scale = np.asarray(inv_scale, np.float32)
        self.gts = [np.asarray(g, np.float64).reshape(-1, 4) if g is not None else None for g in gts]
        self.ignores = [np.asarray(f, np.uint8).reshape(-1) for f in ignores]
        self.serial = np.asarray(serial, np.uint32)
        self.params = {**DEFAULTS, **params}
        self.expect = dict(expect)
        keys = set(zip(det["image"].tolist(), det["level"].tolist(), det["r"].tolist(), det["c"].tolist()))
        assert len(keys) == det.size, f"{name}: (image, level, r, c) not unique"
        assert set(self.expect) <= keys

    @property
    def n_images(self):
        return len(self.gts)

    def reference(self):
        return ref.mine(self.det, self.inv_scale, self.m, self.n, self.gts, self.ignores, self.serial, **self.params)


def chosen_of(rows):
    """{(image, level, r, c): (label, owner)} of ref.ROW records."""
    return {(int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])): (int(w["label"]), int(w["owner"])) for w in rows}


def records(image, level, r, c, first_score=0.0):
    r = np.asarray(r).reshape(-1)
    det = np.zeros(r.size, ref.DET)
    det["image"], det["level"], det["r"], det["c"] = image, level, r, np.asarray(c).reshape(-1)
    det["score"] = first_score + 0.25 * np.arange(r.size)                    # (every record carries a score of its own)
    return det


# ------------------------------------------------------------------------------ label scenes
def cell_box(k):
    x, y = CELL * (k % 64), CELL * (k // 64)
    return [x, y, x + N, y + M]


def off_box(k, s):
    """(r, c) of the window s columns off box k."""
    x, y, _, _ = cell_box(k)
    return y, x + s


def threshold_scene(which):
    """30 boxes, window k is 1 + k % 3 columns off box k.  The thresholds (both) sit on V2 ('on'), one double below it
    ('below') or one above ('above'): the s = 2 windows are neither (both comparisons are strict), TP, or FP."""
    thr = dict(on=V2, below=np.nextafter(V2, 0.0), above=np.nextafter(V2, 1.0))[which]
    G = 30
    pos = [off_box(k, 1 + k % 3) for k in range(G)]
    det = records(0, 0, [p[0] for p in pos], [p[1] for p in pos])
    expect = {}
    for k, (r, c) in enumerate(pos):
        s = 1 + k % 3
        lab = TP if s == 1 else FP if s == 3 else dict(on=None, below=TP, above=FP)[which]
        if lab is not None:
            expect[(0, 0, r, c)] = (lab, k)
    return Scene(f"threshold-{which}", det, [[cell_box(k) for k in range(G)]], [np.zeros(G)], [3], expect, min_tp_iou=thr, max_fp_iou=thr)


def owners_scene(want_tp=True, want_fp=True, both=False):
    """Image 0: box 1 is a twin of box 0 and ignored (the FIRST argmax owns: TP, owner 0), box 2 is ignored (its window is
    neither), box 3 plain, box 5 a twin of box 4 with box 4 the ignored one (owner 4: neither).  Image 1: no ground
    truth (None), image 2: an empty list: every window FP, owner -1.  Image 3: all boxes ignored: windows on them are
    neither, windows that overlap nothing are FP with owner 0.  both: max_fp_iou 0.9 > min_tp_iou 0.5, so the windows
    one column off a plain box are hit for both classes and end up FP (TP when FP is not wanted)."""
    g0 = [cell_box(0), cell_box(0), cell_box(2), cell_box(3), cell_box(4), cell_box(4)]
    i0 = [0, 1, 1, 0, 1, 0]
    w0 = [off_box(0, 1), off_box(2, 1), off_box(3, 1), off_box(4, 1), off_box(9, 0)]            # (box 9 does not exist: IoU 0)
    g3 = [cell_box(k) for k in range(3)]
    w3 = [off_box(0, 1), off_box(1, 1), off_box(7, 0), off_box(8, 3)]
    w1 = [off_box(k, 0) for k in range(4)]
    det = np.concatenate([records(0, 0, *zip(*w0)), records(1, 0, *zip(*w1), first_score=10), records(2, 0, *zip(*w1), first_score=20),
                          records(3, 0, *zip(*w3), first_score=30)])
    near = FP if (both and want_fp) else TP                                     # what a window one column off a plain box gets
    expect = {}
    if want_tp or (both and want_fp):
        expect[(0, 0) + w0[0]] = (near, 0)
        expect[(0, 0) + w0[2]] = (near, 3)
    if both and want_fp:                                                        # (0.818 < 0.9: FP hits whoever owns them)
        expect[(0, 0) + w0[1]] = (FP, 2)
        expect[(0, 0) + w0[3]] = (FP, 4)
        expect[(3, 0) + w3[0]] = (FP, 0)
        expect[(3, 0) + w3[1]] = (FP, 1)
    if want_fp:
        expect[(0, 0) + w0[4]] = (FP, 0)
        for w in w1:
            expect[(1, 0) + w] = (FP, -1)
            expect[(2, 0) + w] = (FP, -1)
        expect[(3, 0) + w3[2]] = (FP, 0)
        expect[(3, 0) + w3[3]] = (FP, 0)
    params = dict(min_tp_iou=0.5, max_fp_iou=0.9) if both else {}
    name = "owners" + ("-both" if both else "") + ("" if want_tp else "-no-tp") + ("" if want_fp else "-no-fp")
    return Scene(name, det, [g0, None, [], g3], [i0, [], [], [1, 1, 1]], [11, 12, 13, 14], expect, want_tp=want_tp, want_fp=want_fp, **params)


# ------------------------------------------------------------------------------ select scenes
def planted_group(image, serial, level, seed, keys, first_score=0.0):
    """Records of group (image, level) whose windows carry exactly `keys`."""
    r, c = ref.window_of_key(seed, serial, level, np.asarray(keys, np.uint64))
    return records(image, level, r, c, first_score)


def losers(rng, count, lo=1 << 20):
    """`count` distinct keys, all of them >= lo."""
    out = set()
    while len(out) < count:
        out.add(int(rng.integers(lo, 1 << 32)))
    return sorted(out)


def select_scene(cls, K, seed=77):
    """Groups over 2 images x 4 levels with planted keys; class `cls` alone is wanted and capped at K.  FP: no ground
    truth, every window a hit.  TP: one box per image and min_tp_iou = -1, every window a hit owned by box 0."""
    rng = np.random.default_rng(1000 + K)
    serial = [5, 9]
    low = list(range(K))
    top = 0xFFFFFFFF
    groups = {                                  # (image, level): (winning keys, losing keys)
        (0, 0): ([], []),                                                        # H = 0
        (0, 1): (low[:K - 1], []),                                               # H = K - 1
        (0, 2): (low, []),                                                       # H = K
        (0, 3): ([0xABCDEF00 + j for j in range(K)], [0xABCDEF00 + K]),          # H = K + 1, keys differ in the last digit only
        (1, 0): ([0] + [0x7FFFFF00 + j for j in range(K - 1)], [top, top - 1, 0x7FFFFF00 + K - 1, 0x80000000]),   # keys at 0 and 2^32 - 1
        (1, 1): (low, losers(rng, 40)),
        (1, 2): (low, losers(rng, 300)),                                         # (more than one workgroup's worth)
        (1, 3): ([0x00010000 + 256 * j for j in range(K)], [0x00010000 + 256 * K + j for j in range(5)]),          # decided in digit 1
    }
    det, expect = [], {}
    for (b, l), (win, lose) in groups.items():
        d = planted_group(b, serial[b], l, seed, win + lose, first_score=100 * b + 10 * l)
        det.append(d)
        for w in d[:len(win)]:
            expect[(b, l, int(w["r"]), int(w["c"]))] = (cls, -1 if cls == FP else 0)
    # the same windows at two levels of one image and at one level of two serials, other winners in each: every group
    # holds the windows that carry keys 0 .. K-1 in ITS OWN group (they win there) and in the other two (they lose there)
    trio = [(2, 6, 0), (2, 6, 1), (3, 2, 1)]                                    # (image, serial, level)
    pos = [ref.window_of_key(seed, s, l, np.arange(K, dtype=np.uint64)) for _, s, l in trio]
    for i, (b, s, l) in enumerate(trio):
        r, c = np.concatenate([p[0] for p in pos]), np.concatenate([p[1] for p in pos])
        det.append(records(b, l, r, c, first_score=500 + 50 * i))
        for j in range(K):
            expect[(b, l, int(pos[i][0][j]), int(pos[i][1][j]))] = (cls, -1 if cls == FP else 0)
    serial = serial + [6, 2]
    box = [[0, 0, N, M]]
    gts = [None] * 4 if cls == FP else [box] * 4
    ign = [[]] * 4 if cls == FP else [[0]] * 4
    params = dict(want_tp=False, max_fp=K, max_fp_iou=2.0) if cls == FP else dict(want_fp=False, max_tp=K, min_tp_iou=-1.0)
    return Scene(f"select-{'fp' if cls == FP else 'tp'}-K{K}", np.concatenate(det), gts, ign, serial, expect, inv_scale=(1.0, 0.5, 2.0, 1.5),
                 seed=seed, **params)


def all_scene():
    """K >= H everywhere: every hit is chosen."""
    s = select_scene(FP, 3)
    expect = {(int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])): (FP, -1) for w in s.det}
    return Scene("select-all", s.det, s.gts, s.ignores, s.serial, expect, inv_scale=s.inv_scale, seed=77, want_tp=False, max_fp=10 ** 9,
                 max_fp_iou=2.0)


SIZES = (0, 1, 63, 64, 65, 257, 1025)


def sized_scene(n_det, K=7, seed=5):
    """n_det records dealt over 2 images x 2 levels and shuffled, so that a group's records lie spread over wave and
    workgroup boundaries; per group keys 0 .. K-1 win."""
    rng = np.random.default_rng(n_det)
    serial = [40, 41]
    det, expect = [], {}
    for g in range(4):
        b, l = g // 2, g % 2
        size = (n_det - g + 3) // 4
        keys = list(range(min(K, size))) + losers(rng, max(size - K, 0))
        d = planted_group(b, serial[b], l, seed, keys, first_score=1000 * g)
        det.append(d)
        for w in d[:min(K, size)]:
            expect[(b, l, int(w["r"]), int(w["c"]))] = (FP, -1)
    return Scene(f"sized-{n_det}", np.concatenate(det), [None, None], [[], []], serial, expect, inv_scale=(1.0, 0.75), seed=seed,
                 shuffle=n_det + 1, want_tp=False, max_fp=K)


@functools.lru_cache(None)
def scenes():
    out = [threshold_scene(w) for w in ("on", "below", "above")]
    out += [owners_scene(), owners_scene(both=True), owners_scene(want_tp=False), owners_scene(want_fp=False),
            owners_scene(want_fp=False, both=True), owners_scene(want_tp=False, want_fp=False)]
    out += [select_scene(FP, 4), select_scene(TP, 4), select_scene(FP, 1), select_scene(TP, 1), all_scene()]
    out += [sized_scene(n) for n in SIZES]
    return {s.name: s for s in out}


# ------------------------------------------------------------------------------ the select kernels in NumPy
SELECT_FAULTS = ("le", "tp_last", "no_ignore", "last_argmax", "k_plus_1", "per_image", "no_serial", "no_level", "append_order",
                 "swap_rc_box")
# the scene that catches each
CAUGHT_BY = dict(le="threshold-on", tp_last="owners-both", no_ignore="owners", last_argmax="owners", k_plus_1="select-fp-K4",
                 per_image="select-fp-K4", no_serial="select-fp-K4", no_level="select-tp-K4", append_order="sized-257",
                 swap_rc_box="threshold-on")


def digit_select(keys, K):
    """The limit (chosen: key < limit) of wb_mine's four 8-bit passes over the distinct uint32 `keys`."""
    keys = np.asarray(keys, np.uint64)
    prefix, krem = 0, int(K)
    for p in range(4):
        shift = 24 - 8 * p
        live = keys[(keys >> (shift + 8)) == (prefix >> (shift + 8))] if p else keys
        hist = np.bincount(((live >> shift) & 255).astype(np.int64), minlength=256)
        if p == 0 and (krem == 0 or hist.sum() <= krem):
            return 0 if krem == 0 else 1 << 32
        incl = np.cumsum(hist)
        t = int(np.flatnonzero((incl - hist < krem) & (krem <= incl))[0])
        prefix |= t << shift
        krem -= int(incl[t] - hist[t])
    return prefix + 1


def emulate_select(s, faults=()):
    """The rows wb_mine_select_launch + the caller's ordering give for scene `s`, with `faults`."""
    faults = tuple(faults)
    assert all(f in SELECT_FAULTS for f in faults), faults
    p, det = s.params, s.det
    L = len(s.inv_scale)
    r, c = (det["c"], det["r"]) if "swap_rc_box" in faults else (det["r"], det["c"])
    boxes = ref.record_boxes(det["level"], r, c, s.inv_scale, s.m, s.n)
    best, owner = np.zeros(det.size), np.full(det.size, -1, np.int32)
    hits = np.zeros((2, det.size), bool)
    for i in range(det.size):
        b = int(det["image"][i])
        g = s.gts[b]
        if g is None or len(g) == 0:
            hits[1, i] = True
            continue
        t = ref.iou_table(boxes[i], g)[0]
        o = len(t) - 1 - int(np.argmax(t[::-1])) if "last_argmax" in faults else int(np.argmax(t))
        best[i], owner[i] = t[o], o
        ign = False if "no_ignore" in faults else bool(s.ignores[b][o])
        if "le" in faults:
            hits[0, i], hits[1, i] = best[i] >= p["min_tp_iou"] and not ign, best[i] <= p["max_fp_iou"]
        else:
            hits[0, i], hits[1, i] = best[i] > p["min_tp_iou"] and not ign, best[i] < p["max_fp_iou"]
    hits[0] &= bool(p["want_tp"])
    hits[1] &= bool(p["want_fp"])
    serial = np.zeros_like(s.serial) if "no_serial" in faults else s.serial
    level = np.zeros_like(det["level"]) if "no_level" in faults else det["level"]
    keys = ref.window_keys(p["seed"], serial[det["image"]] if det.size else serial[:0], level, det["r"], det["c"])
    group = det["image"].astype(np.int64) * (1 if "per_image" in faults else L) + (0 if "per_image" in faults else det["level"])
    chosen = np.zeros((2, det.size), bool)
    for cls, cap in ((0, p["max_tp"]), (1, p["max_fp"])):
        K = min(int(cap), det.size) + (1 if "k_plus_1" in faults else 0)
        for g in np.unique(group[hits[cls]]):
            at = np.flatnonzero(hits[cls] & (group == g))
            chosen[cls, at] = keys[at].astype(np.uint64) < digit_select(keys[at], K)
    if "tp_last" in faults:
        label = np.where(chosen[0], TP, np.where(chosen[1], FP, 0))
    else:
        label = np.where(chosen[1], FP, np.where(chosen[0], TP, 0))
    at = np.flatnonzero(label)
    rows = np.zeros(at.size, ref.ROW)
    for k in ref.DET.names:
        rows[k] = det[k][at]
    rows["best"], rows["owner"], rows["label"] = best[at], owner[at], label[at]
    return rows if "append_order" in faults else ref.ordered(rows)


# ------------------------------------------------------------------------------ gather scenes
GATHER_FAULTS = ("swap_rc_crop", "wrong_stride", "neighbour_level")
SHAPES = ((2, 2, 1), (3, 5, 2), (14, 14, 4))
LEVEL_DIMS = ((20, 24), (16, 18), (14, 15))
N_IMAGES = 2
PAD = 8                     # elements between two images' pyramids


class GatherScene:
    """A pyramid buffer of N_IMAGES images x 3 levels whose element (image, level, row, col, channel) holds a code of its
    own place; windows at the four corners of every level (r + m == u, c + n == v among them), one in the middle, and
    -- last -- one row too low in its level: written as zeros, err set."""

    def __init__(self, shape, dtype):
        self.m, self.n, self.C = shape
        self.dtype = np.dtype(dtype)
        self.name = f"gather-{self.m}x{self.n}x{self.C}-{self.dtype.name}"
        C = self.C
        self.levels = np.zeros(len(LEVEL_DIMS), ref.LEVEL)
        off = 0
        for l, (u, v) in enumerate(LEVEL_DIMS):
            self.levels[l] = (off, u, v)
            off += u * v * C
        self.stride = off + PAD
        buf = np.zeros(N_IMAGES * self.stride, np.int64)
        for b in range(N_IMAGES):
            for l, (u, v) in enumerate(LEVEL_DIMS):
                rr, cc, ch = np.meshgrid(np.arange(u), np.arange(v), np.arange(C), indexing="ij")
                code = ((((b * 3 + l) * 32 + rr) * 32 + cc) * 4 + ch) + 1                  # < 2^24: exact in float32
                o = b * self.stride + int(self.levels[l]["chn_off"])
                buf[o:o + u * v * C] = code.reshape(-1)
        self.codes = buf
        self.buf = (buf % 251).astype(np.uint8) if self.dtype == np.uint8 else buf.astype(np.float32)
        rows = []
        for b in range(N_IMAGES):
            for l, (u, v) in enumerate(LEVEL_DIMS):
                for r, c in ((0, 0), (0, v - self.n), (u - self.m, 0), (u - self.m, v - self.n), ((u - self.m) // 2, (v - self.n) // 2)):
                    rows.append((b, l, r, c))
        rows = sorted(set(rows))
        rows.append((1, 1, LEVEL_DIMS[1][0] - self.m + 1, 0))                               # just outside its level
        self.rows = np.zeros(len(rows), ref.ROW)
        for i, (b, l, r, c) in enumerate(rows):
            self.rows[i] = (b, l, r, c, 0.5 * i, 0.0, -1, FP)

    def expect(self):
        """The crops, from the codes: out[i, y, x, ch] = code(image, level, r + y, c + x, ch); the last row zeros."""
        out = np.zeros((len(self.rows), self.m, self.n, self.C), np.int64)
        for i, w in enumerate(self.rows[:-1]):
            yy, xx, ch = np.meshgrid(np.arange(self.m), np.arange(self.n), np.arange(self.C), indexing="ij")
            out[i] = ((((int(w["image"]) * 3 + int(w["level"])) * 32 + int(w["r"]) + yy) * 32 + int(w["c"]) + xx) * 4 + ch) + 1
        out = (out % 251).astype(np.uint8) if self.dtype == np.uint8 else out.astype(np.float32)
        out[-1] = 0
        return out, 1


@functools.lru_cache(None)
def gather_scenes():
    out = [GatherScene(shape, dt) for shape in SHAPES for dt in (np.float32, np.uint8)]
    return {g.name: g for g in out}


def emulate_gather(g, faults=()):
    """(out, err) as mine_gather_kernel computes them, with `faults`."""
    faults = tuple(faults)
    assert all(f in GATHER_FAULTS for f in faults), faults
    m, n, C = g.m, g.n, g.C
    out = np.zeros((len(g.rows), m, n, C), g.buf.dtype)
    err = 0
    stride = g.stride - PAD if "wrong_stride" in faults else g.stride
    for i, w in enumerate(g.rows):
        b, l, r, c = int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])
        lv = g.levels[l]
        if r + m > lv["u"] or c + n > lv["v"]:
            err = 1
            continue
        off = int(g.levels[(l + 1) % len(g.levels)]["chn_off"] if "neighbour_level" in faults else lv["chn_off"])
        if "swap_rc_crop" in faults:
            r, c = c, r
        v = int(lv["v"])
        for y in range(m):
            at = b * stride + off + ((r + y) * v + c) * C
            seg = g.buf[at:at + n * C]
            out[i, y].reshape(-1)[:seg.size] = seg                                           # (the emulation may run off the end)
    return out, err
