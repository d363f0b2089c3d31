"""Designed box sets for the NMS kernels (wb_nms.hip), where the test decides the answer, and a NumPy emulation of the
device algorithm with a switch for each way a rewrite could go wrong.  No GPU, no torch.

* PLANTED: every box sits in a cell of its own or in a cluster (pair K->R, chain K->R~>S, star); cells are CELL apart and all
  coordinates are small integers, so IoUs between cells are exactly 0 and those inside a cell are 1, 60/140 or 20/180.  Each
  removed box has ONE kept suppressor, at a visiting position the design chooses: `classify` maps such an edge to the
  (band, row chunk, kept ordinal, column word, bit) at which nms_scan_kernel or nms_spread_kernel has to read its matrix word.
* rounding_cases(): pairs of general float32 boxes whose IoU by the contract's operation sequence differs from a fused,
  a float32, a reciprocal, a multiplied-out or a truncated one, each run at the thresholds one rounding apart.
* ORDERS: two identical boxes at neighbouring ranks of a visiting order the design knows; the earlier one survives.
* finish_batches(): wb_nms_finish_launch inputs built from planted images.
* emulate(): rank by counting, matrix words, band scan with the four-at-a-time loop, spread; FAULTS names its switches.
tests/test_nms_designs_host.py proves all of it on the CPU; tests/test_gpu_nms_designs.py runs it."""
import functools
from fractions import Fraction

import numpy as np

BAND = 4096              # WB_NMS_BAND
FINISH_MAX = 4096        # WB_NMS_FINISH_MAX
CELL = 32                # cell pitch (a power of two); a cluster is at most 30 wide
CELLS_X = 512
T_PLANT = 0.3            # in (20/180, 60/140): neighbours of a chain overlap above it, next-but-one neighbours below
UNTOUCHED = -1           # expected flag of a box no position visits


# ------------------------------------------------------------------------------ layout (nms_layout, nms_plain)
def layout(n):
    n64 = max((n + 63) // 64 * 64, 64)
    W = n64 // 64
    return n64, W, (25 * n64 + 16 * W + 16 + 255) // 256 * 256


def scratch_bytes(n, rows=None):
    """Bytes of a scratch that gives n boxes bands of `rows` rows (None: the whole matrix, at most BAND rows)."""
    n64, W, fixed = layout(n)
    return fixed + (min(n64, BAND) if rows is None else rows) * W * 8


def band_rows(n, rows=None):
    n64 = max((n + 63) // 64 * 64, 64)
    return min(n64, BAND) if rows is None else min(rows, n64, BAND)


def finish_block(P, keys, boxes, scores, header):
    """One image's finish block of capacity P: int32 header[4] | uint64 keys[P] | float32 boxes[P][4] | float32 scores[P]."""
    blk = np.zeros(16 + 28 * P, np.uint8)
    blk[:16].view(np.int32)[:] = header
    n = len(keys)
    blk[16:16 + 8 * P].view(np.uint64)[:n] = keys
    blk[16 + 8 * P:16 + 24 * P].view(np.float32).reshape(P, 4)[:n] = boxes
    blk[16 + 24 * P:].view(np.float32)[:n] = scores
    return blk


# ------------------------------------------------------------------------------ designs
class Design:
    """boxes, scores, group: the call's arrays (input order).  order[p]: the input index position p visits (>= n: none).
    want[i]: 1 kept, 0 not, UNTOUCHED.  forms: the entries it runs through ("rank", "ordered", "surface", "by_key")."""

    def __init__(self, name, boxes, scores, order, want, iou_t, group=None, score_t=None, rows=None, keys=None,
                 forms=("rank", "ordered", "surface"), edges=(), stats=None):
        self.name, self.n = name, len(scores)
        self.boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        self.scores = np.ascontiguousarray(scores, np.float32)
        self.group = None if group is None else np.ascontiguousarray(group, np.int32)
        self.order = np.asarray(order, np.int64)
        self.want = np.asarray(want, np.int8)
        self.iou_t, self.score_t, self.rows, self.keys = float(iou_t), score_t, rows, keys
        self.forms, self.edges, self.stats = tuple(forms), list(edges), stats or {}

    @property
    def n_keep(self):
        return int((self.want == 1).sum())

    @property
    def R(self):
        return band_rows(self.n, self.rows)

    def position_of(self):
        pos = np.full(self.n, -1, np.int64)
        ok = self.order < self.n
        pos[self.order[ok]] = np.flatnonzero(ok)
        return pos

    def __repr__(self):
        return self.name


def cell_origin(c):
    return CELL * (c % CELLS_X), CELL * (c // CELLS_X)


class Plant:
    """A planted design under construction, in POSITION space (p = place in the visiting order)."""

    def __init__(self, name, n, seed, rows=None, score_t=None, forms=("rank", "ordered", "surface")):
        self.name, self.n, self.seed, self.rows, self.score_t, self.forms = name, n, seed, rows, score_t, forms
        self.off = np.full(n, -1)
        self.cell = np.full(n, -1)
        self.want = np.ones(n, np.int8)
        self.role = ["F"] * n
        self.group = np.zeros(n, np.int64)
        self.score = None                # None: n - p, strictly decreasing
        self.edges = []                  # (kind, label, suppressor position, target position)
        self.n_cells = 0
        self.use_groups = False
        self.under = np.zeros(n, bool)   # positions the score threshold drops (their flag is 0 whatever the geometry says)

    def put(self, p, cell, off, role, want, group=0):
        assert 0 <= p < self.n and self.off[p] < 0, (self.name, p)
        assert off + 10 <= CELL - 2
        self.off[p], self.cell[p], self.role[p], self.want[p], self.group[p] = off, cell, role, want, group
        if group != 0:
            self.use_groups = True

    def new_cell(self):
        self.n_cells += 1
        return self.n_cells - 1

    def pair(self, label, k, r, group=0):
        return self.star(label, k, [r], group)

    def star(self, label, k, rs, group=0):
        c = self.new_cell()
        self.put(k, c, 0, "K", 1, group)
        for r in rs:
            assert r > k
            self.put(r, c, 4, "R", 0, group)
            self.edges.append(("suppress", f"{label}: K@{k} -> R@{r}", k, r))
        return self

    def chain(self, label, ps, group=0):
        """K -> R ~> S -> R' ~> S' ...: box i at x offset 4 i; the even ones are kept, the odd ones removed."""
        assert list(ps) == sorted(ps) and 3 <= len(ps) <= 5
        c = self.new_cell()
        for i, p in enumerate(ps):
            self.put(p, c, 4 * i, "KR"[i % 2] if i < 2 else "SR"[i % 2], 1 - i % 2, group)
        for i in range(1, len(ps)):
            if i % 2:
                self.edges.append(("suppress", f"{label}: K@{ps[i - 1]} -> R@{ps[i]}", ps[i - 1], ps[i]))
            else:
                self.edges.append(("nospread", f"{label}: removed R@{ps[i - 1]} ~> S@{ps[i]}", ps[i - 1], ps[i]))
        return self

    def build(self, iou_t=T_PLANT, by_key=False):
        n = self.n
        for p in range(n):
            if self.off[p] < 0:
                self.put(p, self.new_cell(), 0, "F", 1, self.group[p])
        self.want[self.under] = 0
        ox, oy = cell_origin(self.cell)
        x1 = ox + self.off
        pos_boxes = np.stack([x1, oy, x1 + 10, oy + 10], 1).astype(np.float32)
        rng = np.random.default_rng(self.seed)
        order = rng.permutation(n)                             # position p is input index order[p]
        boxes = np.empty((n, 4), np.float32)
        boxes[order] = pos_boxes
        pos_scores = np.arange(n, 0, -1).astype(np.float32) if self.score is None else np.asarray(self.score, np.float32)
        keys = None
        if by_key:                                             # equal scores: the key decides, and it says "position"
            pos_scores = np.ones(n, np.float32)
            keys = np.empty(n, np.uint64)
            keys[order] = (np.arange(n, dtype=np.uint64) << np.uint64(26)) | rng.integers(0, 1 << 26, n).astype(np.uint64)
        scores = np.empty(n, np.float32)
        scores[order] = pos_scores
        want = np.empty(n, np.int8)
        want[order] = self.want
        group = None
        if self.use_groups:
            group = np.empty(n, np.int32)
            group[order] = self.group
        stats = dict(kept=int((self.want == 1).sum()), removed=sum(r == "R" for r in self.role), chain_s=sum(r == "S" for r in self.role),
                     roles="".join(self.role))
        return Design(self.name, boxes, scores, order, want, iou_t, group, self.score_t, self.rows, keys,
                      ("by_key",) if by_key else self.forms, self.edges, stats)


def classify(d, edge):
    """Where the device has to read the matrix word that carries `edge`: a dict of coordinates for the design's band size."""
    _, _, k, r = edge
    R = d.R
    pos = d.position_of()
    kept_at = np.zeros(max((d.n + 63) // 64 * 64, 64), bool)
    kept_at[pos[(d.want == 1) & (pos >= 0)]] = True
    chunk0 = k // 64 * 64
    out = dict(band=k // R, chunk=(k % R) // 64, row_bit=k % 64, ordinal=int(kept_at[chunk0:k].sum()) + 1, word=r // 64, bit=r % 64,
               target_band=r // R, adjacent=r == k + 1, last_row=r == d.n - 1, last_word=r // 64 == (d.n - 1) // 64)
    if r // 64 == k // 64:
        out["where"] = "diagonal"
    elif out["target_band"] == out["band"]:
        out["where"] = "scan"
        out["u"], out["round"] = (out["ordinal"] - 1) % 4, (out["ordinal"] - 1) // 4
        Rw = min(R, (d.n + 63) // 64 * 64 - out["band"] * R) // 64
        out["last_lane"] = (r % R) // 64 == Rw - 1
    else:
        out["where"] = "spread"
        first_behind = (out["band"] + 1) * R // 64
        out["block_x"], out["lane"] = (r // 64 - first_behind) // 64, (r // 64 - first_behind) % 64
        out["block_y"], out["wave"] = out["chunk"] // 4, out["chunk"] % 4
        out["first_word_behind"] = r // 64 == first_behind
    return out


def describe_mismatch(d, got):
    """Names the design, the first differing box and the planted edges that touch it, with their coordinates."""
    got = np.asarray(got).astype(np.int64)
    bad = np.flatnonzero(got != d.want)
    if bad.size == 0:
        return f"{d.name}: flags equal"
    pos = d.position_of()
    i = int(bad[0])
    p = int(pos[i])
    msg = f"{d.name}: {bad.size} flags differ, first at input index {i} (position {p}: word {p // 64} bit {p % 64}): want {d.want[i]}, got {got[i]}"
    for e in d.edges:
        if p in (e[2], e[3]):
            msg += f"; {e[0]} edge '{e[1]}' {classify(d, e)}"
    return msg


# ---- A. planted suppressions
def _diag():
    p = Plant("diag-n385", 385, 1)
    combos = [[(0, 1), (31, 32), (62, 63)], [(0, 31), (32, 63)], [(0, 32), (31, 63)], [(0, 63), (32, 33)]]
    for c, cs in enumerate(combos):
        for a, b in cs:
            p.pair(f"diagonal chunk {c} row bit {a} col bit {b}", 64 * c + a, 64 * c + b)
    p.pair("row bit 63 -> bit 0 of the next chunk", 64 * 4 + 63, 64 * 5)
    p.chain("chain inside a diagonal block", [64 * 4 + 3, 64 * 4 + 4, 64 * 4 + 5, 64 * 4 + 40, 64 * 4 + 41])
    return p.build()


def _ordinal(k):
    """The suppressor is the k-th kept row of chunk 1, behind three rows that chunk 0 removed: ordinal k, bit k + 2."""
    p = Plant(f"scan-ordinal{k}-n256", 256, 10 + k)
    p.star("in front of the suppressor", 0, [64, 65, 66])
    p.pair(f"kept row {k} of its chunk (x[{(k - 1) % 4}], round {(k - 1) // 4})", 64 + 2 + k, 128 + 17 + k)
    return p.build()


def _ordinals_together():
    p = Plant("scan-ordinals-together-n256", 256, 19)
    p.star("in front of the suppressors", 0, [64, 65, 66])
    for k in (1, 2, 3, 4, 5, 8):
        p.star(f"kept row {k}", 64 + 2 + k, [128 + 3 * k, 192 + 5 * k])
    return p.build()


def _last_word(n):
    p = Plant(f"scan-lastword-n{n}", n, n)
    last = (n - 1) // 64 * 64
    p.pair("first chunk -> bit 0 of the band's last word", 7, last)
    if n - 1 > last:
        p.pair("second chunk -> the last row before the padding", 64 + 9, n - 1)
        p.chain("chain into the last word", [130, 131, n - 2])
    else:
        p.chain("chain through chunks 1 and 2", [70, 71, 140])
    return p.build()


def _bands(rows, n):
    p = Plant(f"bands-rows{rows}-n{n}", n, rows + n, rows=rows)
    R = rows
    p.pair("band 0 -> band 1, the first word behind the band", R - 2, R + 5)
    p.pair("band 0 -> band 3", 3, 3 * R + 33)
    p.chain("R in band 0, S in band 1", [10, 20, R + 40])
    p.pair("band 1 -> band 4 (b + 3)", R + 1, 4 * R + 63 if 4 * R + 63 < n - 1 else 4 * R)
    p.pair("band 2 -> the last word of all, last row", 2 * R + 31, n - 1)
    p.chain("a longer chain over four bands", [12, R + 12, 2 * R + 12, 3 * R + 12, 3 * R + 13])
    if rows > 64:
        p.pair("chunk to chunk inside band 1", R + 70, R + 64 * (rows // 64 - 1) + 9)
    return p.build()


BIG_N = 8300


def _big(variant):
    n = BIG_N
    p = Plant(f"big-{variant}-n{n}", n, 83, forms=("rank", "ordered"))
    if variant == "a":
        p.star("row 0", 0, [4096, 8191, 8192, n - 1])
        p.star("chunk 3", 3 * 64 + 5, [5000, 8200])
        p.star("chunk 4", 4 * 64 + 6, [4100, 8250])
        p.star("chunk 63", 63 * 64 + 7, [6000, 8298])
        p.chain("R in band 0, S in band 2", [100, 4000, 8260])
    elif variant == "b":
        p.star("row 4095", 4095, [4096, 8191, 8192, n - 1])
    else:
        p.star("row 4096", 4096, [8191, 8192, n - 1])
        p.chain("R in band 1, S in band 2", [4200, 8000, 8270])
    return p.build()


I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _groups():
    p = Plant("groups-n200", 200, 5)
    labels = [I32_MIN, -1, 0, I32_MAX]
    for p_ in range(200):
        p.group[p_] = labels[p_ % 4]
    p.use_groups = True
    k = 0
    for ga in labels:                                          # K and R in different groups: both kept; in the same: R goes
        for gb in labels:
            c = p.new_cell()
            a, b = 3 * k, 3 * k + 70
            p.put(a, c, 0, "K", 1, ga)
            p.put(b, c, 4, "R" if ga == gb else "K", 1 if ga != gb else 0, gb)
            if ga == gb:
                p.edges.append(("suppress", f"groups {ga} / {gb}: K@{a} -> R@{b}", a, b))
            k += 1
    c = p.new_cell()                                           # a star whose targets alternate groups
    p.put(50, c, 0, "K", 1, -1)
    for j, r in enumerate(range(130, 190, 5)):
        mine = j % 2 == 0
        p.put(r, c, 4 if mine else 8, "R" if mine else "K", 0 if mine else 1, -1 if mine else I32_MAX)
        if mine:
            p.edges.append(("suppress", f"star over groups: K@50 -> R@{r}", 50, r))
    # (the other group's boxes of that star are identical: the first of them is kept, the rest it removes)
    first = True
    for j, r in enumerate(range(130, 190, 5)):
        if j % 2:
            if not first:
                p.want[r], p.role[r] = 0, "R"
                p.edges.append(("suppress", f"star over groups, other group: K@135 -> R@{r}", 135, r))
            first = False
    return p.build()


def _score_threshold(kind):
    n = 130
    if kind in ("equal", "negzero", "poszero"):
        p = Plant(f"score-threshold-{kind}-n{n}", n, 40)
        q = 70                                                 # the last position that passes
        if kind == "equal":
            p.score = np.arange(n, 0, -1).astype(np.float32)
            p.score_t = float(p.score[q])
        else:
            z = np.float32(-0.0 if kind == "poszero" else 0.0)                # the score; the threshold is the other zero
            p.score = np.concatenate([np.arange(q, 0, -1), [z], -np.arange(1, n - q)]).astype(np.float32)
            p.score_t = -float(z)
        p.pair("passes -> passes", 5, 60)
        p.pair("the box AT the threshold suppresses nothing that passes", q, 100)
        p.chain("S is under the threshold", [20, 30, 90])
        p.under[q + 1:] = True
        return p.build()
    # K is under the threshold although it comes early: only a caller's order can say that
    p = Plant(f"score-threshold-ordered-n{n}", n, 41, forms=("ordered",))
    p.score = np.arange(n, 0, -1).astype(np.float32)
    p.score_t = 50.0
    for k in (4, 64, 100):
        p.score[k] = 49.0
    p.pair("K dropped: R is kept", 4, 9)
    p.chain("K dropped: R kept, S removed", [64, 66, 75])
    p.pair("K dropped, R under the threshold as well", 100, 120)
    p.want[[4, 64, 100]] = 0
    p.want[9] = 1
    p.want[[66, 75]] = [1, 0]
    p.under[:] = p.score < 50.0
    p.edges = [("suppress", "R kept (its K is dropped) -> S removed", 66, 75)]
    return p.build()


def sprinkle(n, seed, by_key=False, name=None):
    """A planted design of any n: pairs, chains and stars at seeded positions among filler."""
    p = Plant(name or f"sprinkle-n{n}-{'key' if by_key else 'scores'}", n, seed, forms=("rank", "ordered", "surface"))
    rng = np.random.default_rng(seed + 7)
    free = sorted(rng.permutation(n)[:n // 2].tolist())
    j = 0
    while j < len(free):
        kind = int(rng.integers(0, 3))
        take = (2, 3, 4)[kind]
        ps = free[j:j + take]
        j += take
        if len(ps) < 2:
            break
        if len(ps) == 2 or kind == 0:
            p.star("pair", ps[0], ps[1:2])
            j -= len(ps) - 2
        elif kind == 1:
            p.chain("chain", ps[:3])
        else:
            p.star("star", ps[0], ps[1:])
    return p.build(by_key=by_key)


@functools.lru_cache(None)
def planted():
    out = [_diag(), _ordinals_together()] + [_ordinal(k) for k in (1, 2, 3, 4, 5, 8)]
    out += [_last_word(n) for n in (193, 255)]
    out += [_bands(64, 385), _bands(192, 831), _bands(192, 1025)]
    out += [_groups()] + [_score_threshold(k) for k in ("equal", "negzero", "poszero", "ordered")]
    out += [sprinkle(65, 3), sprinkle(1, 4), sprinkle(1100, 5)]
    out += [_big(v) for v in "abc"]
    return out


def by_name(name):
    return next(d for d in planted() + orders() if d.name == name)


def coverage():
    """The coordinates the planted edges hit, as a set of tags (test_nms_designs_host.py holds REQUIRED against it)."""
    tags = set()
    for d in planted():
        big = d.n == BIG_N
        for e in d.edges:
            c = classify(d, e)
            kind, k, r = e[0], e[2], e[3]
            if kind == "nospread":
                tags.add(("nospread", "same band" if c["band"] == c["target_band"] else f"band +{c['target_band'] - c['band']}"))
                continue
            if c["where"] == "diagonal":
                tags |= {("diagonal row bit", c["row_bit"]), ("diagonal col bit", c["bit"])}
                if c["adjacent"]:
                    tags.add(("diagonal adjacent", c["row_bit"]))
            elif c["where"] == "scan":
                if c["ordinal"] != c["row_bit"] + 1:
                    tags.add(("scan ordinal behind removed rows", c["ordinal"]))
                tags.add(("scan x[u] round", c["u"], c["round"]))
                if c["adjacent"]:
                    tags.add(("scan adjacent", c["row_bit"], c["bit"]))
                if c["last_lane"]:
                    tags.add(("scan last word", d.n % 64, "last row" if c["last_row"] else "bit %d" % c["bit"]))
                if big:
                    tags.add(("big scan", k, r))
            else:
                gap = c["target_band"] - c["band"]
                if big:
                    tags |= {("big spread", k, r), ("big spread chunk", c["chunk"], c["block_y"], c["wave"]), ("big spread block_x", c["block_x"])}
                else:
                    tags.add(("spread", d.rows, f"band +{gap}"))
                    if c["first_word_behind"]:
                        tags.add(("spread", d.rows, "first word behind"))
                    if c["last_word"]:
                        tags.add(("spread", d.rows, "last word of all"))
    return tags


def required_coverage():
    n = BIG_N
    req = {("diagonal row bit", b) for b in (0, 31, 32)} | {("diagonal col bit", b) for b in (31, 32, 63)}
    req |= {("diagonal adjacent", 0), ("diagonal adjacent", 31), ("scan adjacent", 63, 0)}       # (row bit 63 / col bit 0: the next chunk)
    req |= {("scan ordinal behind removed rows", k) for k in (1, 2, 3, 4, 5, 8)}
    req |= {("scan x[u] round", u, 0) for u in range(4)} | {("scan x[u] round", 0, 1), ("scan x[u] round", 3, 1)}
    req |= {("scan last word", 1, "last row"), ("scan last word", 63, "last row"), ("scan last word", 63, "bit 0")}
    for rows in (64, 192):
        req |= {("spread", rows, t) for t in ("band +1", "band +3", "first word behind", "last word of all")}
    req |= {("nospread", "same band"), ("nospread", "band +1")}
    req |= {("big spread", k, r) for k in (0, 4095) for r in (4096, 8191, 8192, n - 1)}
    req |= {("big scan", 4096, 8191), ("big spread", 4096, 8192), ("big spread", 4096, n - 1)}
    req |= {("big spread chunk", c, c // 4, c % 4) for c in (0, 3, 4, 63)} | {("big spread block_x", 0), ("big spread block_x", 1)}
    return req


# ---- B. one rounding from the threshold
def _f(x):
    return Fraction(float(x))


def iou_forms(a, b):
    """The contract IoU `u` of two float32 boxes (each operation rounded once, in float64) and the wrong forms' values:
    fused (union = fma(-iw, ih, area_a + area_b)), f32 (all in float32), recip (inter * (1 / union)), trunc (the exact
    quotient rounded toward zero); `inter`, `uni` for the multiply form.  None when the boxes do not overlap."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    iw = max(min(a64[2], b64[2]) - max(a64[0], b64[0]), 0.0)
    ih = max(min(a64[3], b64[3]) - max(a64[1], b64[1]), 0.0)
    inter = iw * ih
    if not inter > 0:
        return None
    s = (a64[2] - a64[0]) * (a64[3] - a64[1]) + (b64[2] - b64[0]) * (b64[3] - b64[1])
    uni = s - inter
    u = inter / uni
    fused_uni = float(_f(s) - _f(iw) * _f(ih))
    exact = _f(inter) / _f(uni)
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    iw32 = max(min(a32[2], b32[2]) - max(a32[0], b32[0]), np.float32(0))
    ih32 = max(min(a32[3], b32[3]) - max(a32[1], b32[1]), np.float32(0))
    i32 = iw32 * ih32
    u32 = (a32[2] - a32[0]) * (a32[3] - a32[1]) + (b32[2] - b32[0]) * (b32[3] - b32[1]) - i32
    return dict(u=float(u), inter=float(inter), uni=float(uni), fused=float(inter / fused_uni), f32=float(i32 / u32),
                recip=float(inter * (1.0 / uni)), trunc=float(u) if _f(u) <= exact else float(np.nextafter(u, 0.0)))


def multiply_decides(forms, t):
    return forms["inter"] > t * forms["uni"]


ROUNDING_FORMS = ("fused", "f32", "recip", "multiply", "trunc")
ROUNDING_SEED, ROUNDING_PER_FORM = 2024, 8
PLACES = [(0, 1), (5, 37), (31, 32), (0, 63), (63, 64), (3, 81), (40, 127), (64, 129), (70, 100), (127, 128), (33, 95), (62, 126)]
ROUNDING_N = 130


def general_pair(rng):
    """Two overlapping general float32 boxes: every corner rounded to float32 on its own, the near corners on binades
    2^-2 .. 2^10 and the far ones 20 to 220 further (so a width is the difference of floats of different binades)."""
    f = np.float32
    a1 = (rng.uniform(1, 2, 2) * 2.0 ** rng.integers(-2, 10, 2)).astype(f)
    wa, wb = rng.uniform(20, 220, 2), rng.uniform(20, 220, 2)
    b1 = np.abs(a1 + rng.uniform(-0.6, 0.6, 2) * wa).astype(f)
    return np.concatenate([a1, (a1 + wa).astype(f)]).astype(f), np.concatenate([b1, (b1 + wb).astype(f)]).astype(f)


def splitting_threshold(form, fm):
    """The threshold at which the contract and the wrong `form` decide differently on a pair with forms `fm`, or None."""
    u = fm["u"]
    if form == "multiply":
        below = float(np.nextafter(u, 0.0))
        return u if multiply_decides(fm, u) else below if not multiply_decides(fm, below) else None
    return min(u, fm[form]) if fm[form] != u else None


@functools.lru_cache(None)
def search_rounding_pairs():
    """The seeded search: per wrong form the first ROUNDING_PER_FORM pairs that expose it (about a second; the result is
    kept in ROUNDING_BITS and test_nms_designs_host.py derives it again)."""
    rng = np.random.default_rng(ROUNDING_SEED)
    found = {k: [] for k in ROUNDING_FORMS}
    tries = 0
    while any(len(v) < ROUNDING_PER_FORM for v in found.values()):
        tries += 1
        assert tries < 200000
        a, b = general_pair(rng)
        fm = iou_forms(a, b)
        if fm is None:
            continue
        for k in ROUNDING_FORMS:
            if len(found[k]) < ROUNDING_PER_FORM and splitting_threshold(k, fm) is not None:
                found[k].append((k, a, b))
    return [x for k in ROUNDING_FORMS for x in found[k]]


ROUNDING_BITS = [
    ("fused", [0x4150681c, 0x3f056333, 0x42972d9a, 0x42806a44, 0x411e2668, 0x3e925c51, 0x42ee30c6, 0x43517180]),
    ("fused", [0x4005aff3, 0x3ea1cdcf, 0x426c1eba, 0x42ba3c78, 0x3ff2c3c0, 0x40af34a4, 0x430c6eb2, 0x434ede7f]),
    ("fused", [0x40b13961, 0x4001d696, 0x4337aef7, 0x42944bb0, 0x3e965e39, 0x40004af0, 0x43383036, 0x4304ed7a]),
    ("fused", [0x419789af, 0x3f94ecf2, 0x43224626, 0x42cc30f0, 0x41a3ba49, 0x401594fa, 0x434a0de3, 0x434f37d0]),
    ("fused", [0x405a810e, 0x405fc5f5, 0x42df9243, 0x434b16b2, 0x40b80f09, 0x41286add, 0x42941647, 0x43136690]),
    ("fused", [0x40ae571a, 0x3fef0903, 0x430cc25c, 0x42a0c664, 0x427f3421, 0x3ec46ca6, 0x434e2ee2, 0x4306c95f]),
    ("fused", [0x3f2c33ef, 0x3e83fddf, 0x42db5299, 0x42debec8, 0x420b1b67, 0x3c15e866, 0x43408e0f, 0x432d8157]),
    ("fused", [0x40352c02, 0x4156f7e3, 0x434faa4a, 0x4312af4c, 0x403688db, 0x421c3611, 0x42f06b53, 0x434713d8]),
    ("f32", [0x405681a4, 0x401b6ef1, 0x43373eb1, 0x435d96cd, 0x42831957, 0x4209eec4, 0x42e3fde1, 0x428c74e1]),
    ("f32", [0x4315b615, 0x424b5c77, 0x433ec9d4, 0x4337fc8c, 0x432d27e9, 0x42c55cfc, 0x434214f3, 0x4353b498]),
    ("f32", [0x3f4c64ad, 0x3fa9a50f, 0x42daafe2, 0x4299de05, 0x41e4db5d, 0x41e9914f, 0x435f9943, 0x42b7a7a4]),
    ("f32", [0x3f2259cc, 0x3ea24fe2, 0x42e426e2, 0x429250f3, 0x42179bc2, 0x3f4c4350, 0x436bb0c6, 0x429c1f85]),
    ("f32", [0x3fbbe80c, 0x43fb82d5, 0x4215197b, 0x440f0408, 0x4071fd54, 0x43f631d1, 0x4272f43a, 0x442d5efd]),
    ("f32", [0x416abd23, 0x42aca494, 0x42a0aebe, 0x42de311a, 0x400e0ced, 0x429f508e, 0x4321717e, 0x43270724]),
    ("f32", [0x44202c08, 0x40c8f938, 0x443a73af, 0x42855530, 0x441da89a, 0x3f3753cb, 0x443beaa5, 0x4309cb27]),
    ("f32", [0x40f8d31e, 0x40062bd3, 0x43038fe2, 0x430dc98a, 0x4269bf0a, 0x42a0d827, 0x42adca8a, 0x4314ac6d]),
    ("recip", [0x4315b615, 0x424b5c77, 0x433ec9d4, 0x4337fc8c, 0x432d27e9, 0x42c55cfc, 0x434214f3, 0x4353b498]),
    ("recip", [0x3f2259cc, 0x3ea24fe2, 0x42e426e2, 0x429250f3, 0x42179bc2, 0x3f4c4350, 0x436bb0c6, 0x429c1f85]),
    ("recip", [0x3fbbe80c, 0x43fb82d5, 0x4215197b, 0x440f0408, 0x4071fd54, 0x43f631d1, 0x4272f43a, 0x442d5efd]),
    ("recip", [0x416abd23, 0x42aca494, 0x42a0aebe, 0x42de311a, 0x400e0ced, 0x429f508e, 0x4321717e, 0x43270724]),
    ("recip", [0x3ea93a80, 0x43b41889, 0x41b834df, 0x4402dc15, 0x4114cb8b, 0x43d1ac16, 0x42f1617b, 0x440b4a34]),
    ("recip", [0x42c80a10, 0x411a1b3a, 0x43464ce8, 0x425ecc3f, 0x424066ec, 0x406cd737, 0x433a8ccd, 0x42085975]),
    ("recip", [0x415e662a, 0x438f557c, 0x428b020d, 0x43a05e59, 0x40ebd94c, 0x4385e635, 0x43224f77, 0x43c37f0a]),
    ("recip", [0x442456ec, 0x40eedd39, 0x444fe450, 0x4360ee6f, 0x44239b04, 0x42fa81d4, 0x44513ccd, 0x43ab53aa]),
    ("multiply", [0x3fbbe80c, 0x43fb82d5, 0x4215197b, 0x440f0408, 0x4071fd54, 0x43f631d1, 0x4272f43a, 0x442d5efd]),
    ("multiply", [0x3ea93a80, 0x43b41889, 0x41b834df, 0x4402dc15, 0x4114cb8b, 0x43d1ac16, 0x42f1617b, 0x440b4a34]),
    ("multiply", [0x3ff3d97c, 0x3f413d33, 0x4316003b, 0x4313a3dd, 0x4240d373, 0x429a005d, 0x4364385a, 0x42f49e49]),
    ("multiply", [0x400797f2, 0x431b6d6b, 0x43060bf3, 0x43ab699f, 0x41712d5f, 0x433caa4c, 0x42de5eb5, 0x435771eb]),
    ("multiply", [0x3f04706e, 0x41be06c6, 0x429e4c81, 0x42c45a75, 0x420b49ec, 0x40876122, 0x4332f05a, 0x4230be3d]),
    ("multiply", [0x43c8e1b7, 0x401bb29a, 0x44107594, 0x43484b67, 0x43b2a20c, 0x42de451b, 0x43d4042f, 0x43298db7]),
    ("multiply", [0x40634f3e, 0x3f846be1, 0x431a8583, 0x425ec6f3, 0x426783e9, 0x4120481f, 0x43784926, 0x433c4692]),
    ("multiply", [0x4212b044, 0x40d77923, 0x435280b7, 0x431541ef, 0x42567304, 0x42457a54, 0x431b4847, 0x43286549]),
    ("trunc", [0x4315b615, 0x424b5c77, 0x433ec9d4, 0x4337fc8c, 0x432d27e9, 0x42c55cfc, 0x434214f3, 0x4353b498]),
    ("trunc", [0x3fbbe80c, 0x43fb82d5, 0x4215197b, 0x440f0408, 0x4071fd54, 0x43f631d1, 0x4272f43a, 0x442d5efd]),
    ("trunc", [0x40f8d31e, 0x40062bd3, 0x43038fe2, 0x430dc98a, 0x4269bf0a, 0x42a0d827, 0x42adca8a, 0x4314ac6d]),
    ("trunc", [0x43308cff, 0x41b474d7, 0x4378b1a8, 0x4301d428, 0x430df879, 0x40ba6462, 0x433cef33, 0x4326672a]),
    ("trunc", [0x411f97f8, 0x3f3e2e34, 0x42d55c12, 0x43313562, 0x41b9b463, 0x41e887c2, 0x42b615d7, 0x4359f9f3]),
    ("trunc", [0x3ff3d97c, 0x3f413d33, 0x4316003b, 0x4313a3dd, 0x4240d373, 0x429a005d, 0x4364385a, 0x42f49e49]),
    ("trunc", [0x44795d10, 0x3f6fd29d, 0x4492afbc, 0x41b1f307, 0x4471dabe, 0x40c28ed7, 0x448c06a2, 0x42b136f7]),
    ("trunc", [0x4347f2fe, 0x43771718, 0x43bf80d1, 0x43b8aaba, 0x4363cc62, 0x4398165a, 0x43dd4b9c, 0x43f604f6]),
]


@functools.lru_cache(None)
def rounding_pairs():
    """(form, a, b, forms dict, t at which the form decides differently) of the pairs kept in ROUNDING_BITS."""
    out = []
    for form, bits in ROUNDING_BITS:
        ab = np.array(bits, np.uint32).view(np.float32)
        fm = iou_forms(ab[:4], ab[4:])
        out.append((form, ab[:4].copy(), ab[4:].copy(), fm, splitting_threshold(form, fm)))
    return out


def _among_filler(name, pair, places, t, second_kept, n=ROUNDING_N, seed=0):
    pa, pb = places
    pos_boxes = np.empty((n, 4), np.float32)
    ox, oy = cell_origin(np.arange(n))
    pos_boxes[:] = np.stack([16384 + ox, oy, 16384 + ox + 10, oy + 10], 1)
    pos_boxes[pa], pos_boxes[pb] = pair
    order = np.random.default_rng(seed).permutation(n)
    boxes, scores, want = np.empty((n, 4), np.float32), np.empty(n, np.float32), np.ones(n, np.int8)
    boxes[order] = pos_boxes
    scores[order] = np.arange(n, 0, -1)
    want[order[pb]] = 1 if second_kept else 0
    return Design(name, boxes, scores, order, want, t, forms=("rank",), edges=[("suppress", f"the pair: @{pa} -> @{pb}", pa, pb)])


@functools.lru_cache(None)
def rounding_cases():
    """One call per (pair, threshold): t = u (strict: both kept), t = nextafter(u, 0) (the second removed) and the t at
    which the pair's wrong form decides differently.  Each carries .target = (form, forms dict) for the last kind."""
    out = []
    for j, (form, a, b, fm, t_form) in enumerate(rounding_pairs()):
        u = fm["u"]
        ts = [("t=u", u, None), ("t=below-u", float(np.nextafter(u, 0.0)), None)]
        if t_form not in (ts[0][1], ts[1][1]):
            ts.append((f"t=min(u,{form})", t_form, form))
        else:
            k = 0 if t_form == u else 1
            ts[k] = (ts[k][0] + f"-splits-{form}", t_form, form)
        for i, (label, t, target) in enumerate(ts):
            d = _among_filler(f"rounding-{j:02d}-{form}-{label}", (a, b), PLACES[(j + 5 * i) % len(PLACES)], t, not u > t, seed=j)
            d.target, d.forms_of_pair, d.pair = target, fm, (a, b)
            out.append(d)
    return out


def odd_boxes():
    """The fixed set of non-ordinary boxes (the expectation is nms_keep's): (boxes, scores)."""
    inf, nan, d, big = np.inf, np.nan, 1e-40, 3e38
    rows = [[0, 0, 10, 10], [4, 0, 14, 10], [10, 0, 0, 10], [10, 10, 0, 0], [10, 10, 0, 0], [14, 10, 4, 0], [3, 3, 3, 3], [3, 3, 3, 3], [0, 0, 0, 10],
            [0, 0, inf, 10], [5, 0, inf, 10], [-inf, -inf, inf, inf], [-inf, -inf, inf, inf], [inf, 0, inf, 10], [-inf, 0, 5, 10], [-inf, 0, 6, 10],
            [nan, 0, 10, 10], [0, 0, 10, nan], [0, 0, 10, 10], [nan, nan, nan, nan],
            [0, 0, d, d], [0, 0, d, d], [0, 0, d, 10], [d, 0, 3 * d, 10], [0, 0, 2 * d, 10], [0, 0, 2 * d, 2 * d],
            [-big, -big, big, big], [-big, -big, big, big], [1e38, 1e38, big, big], [-big, 0, big, 10], [-big, 0, big, 8], [2.9e38, 0, 3e38, 10],
            [2.95e38, 0, 3.05e38, 10]]
    with np.errstate(all="ignore"):
        boxes = np.array(rows, np.float64).astype(np.float32)
    n = len(boxes)
    scores = np.empty(n, np.float32)
    scores[np.random.default_rng(12).permutation(n)] = np.arange(n, 0, -1)
    return boxes, scores


ODD_THRESHOLDS = (0.0, 0.3, 0.75)


# ---- C. the visiting order made visible
def score_word(s, negzero_first=False):
    """nms_score_word: descending score as an ascending word; the two zeros are one value."""
    s = np.asarray(s, np.float32)
    b = (s + np.float32(0)).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    w = (~key).astype(np.uint64)
    if negzero_first:
        w = w * np.uint64(2) + np.where((s == 0) & np.signbit(s), 0, 1).astype(np.uint64)
    return w


def adjacent_rank_pairs(name, scores, parity, keys=None, visit=None):
    """n boxes whose visiting order is known: ranks 2k + parity and 2k + parity + 1 are two identical boxes in a cell of
    their own, so exactly the earlier visited survives; a swap of two neighbours in the order flips two flags."""
    scores = np.asarray(scores, np.float32)
    n = scores.size
    idx = np.arange(n)
    if visit is not None:
        order, form = np.asarray(visit, np.int64), "ordered"
    elif keys is not None:
        order, form = np.lexsort((idx, keys, score_word(scores))), "by_key"
    else:
        order, form = np.argsort(-(scores + np.float32(0)), kind="stable"), "rank"
    valid = order < n
    cell = np.arange(n)                                        # cell of the box at position p
    want_pos = np.ones(n, np.int8)
    edges = []
    for p in range(parity, n - 1, 2):
        if valid[p] and valid[p + 1]:
            cell[p + 1] = cell[p]
            want_pos[p + 1] = 0
            edges.append(("suppress", f"ranks {p} and {p + 1}", p, p + 1))
    boxes = np.zeros((n, 4), np.float32)
    want = np.full(n, UNTOUCHED, np.int8)
    ox, oy = cell_origin(cell)
    boxes[order[valid]] = np.stack([ox, oy, ox + 10, oy + 10], 1)[valid]
    want[order[valid]] = want_pos[valid]
    unvisited = np.flatnonzero(want == UNTOUCHED)              # (boxes no position names: out of everyone's way)
    for j, i in enumerate(unvisited):
        boxes[i] = [40000 + 32 * j, 0, 40010 + 32 * j, 10]
    return Design(f"{name}-parity{parity}", boxes, scores, order, want, 0.5, keys=keys, edges=edges,
                  forms=(form,) if form != "rank" else ("rank", "surface"))


def _tiny_ladder():
    d = np.array([1, 2, 3], np.uint32)
    pos, neg = d.view(np.float32), (d | np.uint32(0x80000000)).view(np.float32)
    vals = np.concatenate([neg[::-1], np.array([-0.0, 0.0], np.float32), pos])
    return vals


@functools.lru_cache(None)
def orders():
    rng = np.random.default_rng(77)
    sets = [(f"order-equal-n{n}", np.full(n, 2.5, np.float32), None, None) for n in (255, 256, 257, 513)]
    runs = np.repeat(np.arange(5), [200, 100, 250, 30, 20]).astype(np.float32)                  # run 1 straddles 256, run 2 512
    sets.append(("order-runs-contiguous-n600", -runs, None, None))
    sets.append(("order-runs-scattered-n600", -runs[rng.permutation(600)], None, None))
    ladder = np.tile(_tiny_ladder(), 9)[rng.permutation(72)]
    sets.append(("order-zero-ladder-n72", ladder, None, None))
    sets.append(("order-zeros-n66", np.where(rng.random(66) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32), None, None))
    wide = np.array([np.inf, -np.inf, -1e38, -3e38, -1e-38, -1e-30, -1.0, -1.0000001, 1e38, 3.4e38, 3.3999999e38, 1e-45, -1e-45, 0.0], np.float32)
    sets.append(("order-inf-and-wide-n70", np.tile(wide, 5)[rng.permutation(70)], None, None))
    keys = rng.permutation(300).astype(np.uint64) << np.uint64(26)
    sets.append(("order-keys-random-n300", np.full(300, 1.0, np.float32), keys, None))
    keys2 = keys.copy()
    keys2[40:120] = np.repeat(keys[40:120:2], 2)[rng.permutation(80)]                            # every key twice: the index decides
    sets.append(("order-keys-equal-block-n300", np.full(300, 1.0, np.float32), keys2, None))
    keys3 = keys2.copy()
    sets.append(("order-keys-and-score-runs-n300", -np.repeat(np.arange(3), 100).astype(np.float32)[rng.permutation(300)], keys3, None))
    perm = rng.permutation(200)
    sc = rng.normal(0, 1, 200).astype(np.float32)
    sets.append(("order-callers-permutation-n200", sc, None, perm))
    bad = perm.copy().astype(np.int64)
    bad[[0, 63, 64, 131, 199]] = [200, 205, 0xFFFFFFFF, 1 << 31, 200]
    sets.append(("order-callers-entries-beyond-n-n200", sc, None, bad))
    return [adjacent_rank_pairs(name, s, parity, k, v) for name, s, k, v in sets for parity in (0, 1)]


# ---- D. finish batches
def finish_batches():
    """[(cap, [image, ...])]: image = dict(total, by_key, design or None, done).  Sizes 0, 1, 64, 65, cap, 4096, 4097."""
    def im(total, by_key, cap, seed):
        done = total <= cap and total <= FINISH_MAX
        held = min(total, cap)
        d = sprinkle(held, seed, by_key, name=f"finish-cap{cap}-image{seed - 100}-n{total}-{'key' if by_key else 'scores'}") if held else None
        return dict(total=total, by_key=by_key, design=d, done=done, held=held)
    out = []
    k, s = True, False
    for cap, sizes in ((64, [(64, k), (0, s), (64, k), (1, s), (65, k), (63, s)]),
                       (4096, [(4096, k), (0, s), (4096, k), (1, s), (64, k), (65, s), (4097, k), (1000, s)]),
                       (8192, [(5000, k), (4096, k), (0, s), (4096, s), (4097, k), (65, k)])):
        out.append((cap, [im(t, by_key, cap, 100 + j) for j, (t, by_key) in enumerate(sizes)]))
    return out


def finish_arrays(cap, images, fill=0x5A):
    """The batch's input bytes, and the result bytes expected in a buffer pre-filled with `fill`."""
    blocks, want = [], np.full((len(images), 16 + cap), fill, np.uint8)
    for b, g in enumerate(images):
        d = g["design"]
        hdr = [g["total"], g["total"], g["held"], 0 if g["by_key"] else 1]
        if d is None:
            blocks.append(finish_block(cap, np.zeros(0, np.uint64), np.zeros((0, 4), "f"), np.zeros(0, "f"), hdr))
        else:
            keys = d.keys if d.keys is not None else np.arange(d.n, dtype=np.uint64) << np.uint64(26)
            blocks.append(finish_block(cap, keys, d.boxes, d.scores, hdr))
        if g["done"]:
            want[b, :16].view(np.uint32)[:] = [d.n_keep if d is not None else 0, g["total"], 1, 0]
            if d is not None:
                want[b, 16:16 + d.n] = d.want
        else:
            want[b, :16] = 0
    return np.concatenate(blocks), want


# ------------------------------------------------------------------------------ the reference with an explicit order
def keep_by_order(d):
    """Greedy NMS of design d along d.order with boxes.iou (what nms_keep does, for an order that is not the score order)."""
    from waldboost_amd.boxes import Boxes, iou
    n = d.n
    dead = np.zeros(n, bool) if d.score_t is None else ~(d.scores >= np.float32(d.score_t))
    keep = np.full(n, UNTOUCHED, np.int8)
    everything = Boxes(d.boxes)
    for i in d.order:
        if i >= n:
            continue
        keep[i] = 0
        if dead[i]:
            continue
        keep[i] = 1
        with np.errstate(all="ignore"):
            hit = iou(Boxes(d.boxes[i:i + 1]), everything)[0] > d.iou_t
        if d.group is not None:
            hit &= d.group == d.group[i]
        dead |= hit
    return keep


# ------------------------------------------------------------------------------ the device algorithm in NumPy
FAULTS = ("or_removed_rows", "first_round_only", "last_lane_stale", "no_carry", "spread_first_block", "spread_chunks_lt4", "low_half",
          "padding_alive", "ge", "iou_fused", "iou_f32", "iou_recip", "iou_multiply", "ties_desc_index", "negzero_first", "index_before_key",
          "score_gt", "no_groups", "no_first_reset", "iou_trunc")
M64 = (1 << 64) - 1


def rank_by_counting(hi, lo, faults=(), by_key=False):
    """nms_rank_kernel: p(i) = number of (hi, lo, index) triples smaller than i's, 256 at a time."""
    n = len(hi)
    idx = np.arange(n, dtype=np.uint64)
    smaller = np.zeros(n, np.int64)
    H, L, I = hi[:, None], lo[:, None], idx[:, None]
    for t0 in range(0, n, 256):
        hj, lj, ij = hi[None, t0:t0 + 256], lo[None, t0:t0 + 256], idx[None, t0:t0 + 256]
        lt_lo, lt_i = lj < L, ij < I
        if "ties_desc_index" in faults:
            lt_lo, lt_i = lj > L, ij > I
        second = lt_i if ("index_before_key" in faults and by_key) else lt_lo | ((lj == L) & lt_i)
        smaller += ((hj < H) | ((hj == H) & second)).sum(1)
    return smaller


def hits(a, b, thr, faults=()):
    """nms_matrix_kernel's `iou > thr` for row boxes a [m, 4] against column boxes b [k, 4] (float32), operation by operation."""
    if "iou_f32" in faults:
        A, B, zero = a.astype(np.float32), b.astype(np.float32), np.float32(0)
    else:
        A, B, zero = a.astype(np.float64), b.astype(np.float64), 0.0
    ax1, ay1, ax2, ay2 = (A[:, None, k] for k in range(4))
    bx1, by1, bx2, by2 = (B[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        iw = np.where(ax2 < bx2, ax2, bx2) - np.where(ax1 > bx1, ax1, bx1)
        ih = np.where(ay2 < by2, ay2, by2) - np.where(ay1 > by1, ay1, by1)
        iw, ih = np.where(iw < 0, zero, iw), np.where(ih < 0, zero, ih)
        inter = iw * ih
        s = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)
        uni = s - inter
        pos = np.isfinite(inter) & (inter > 0) & np.isfinite(s)
        if "iou_fused" in faults:
            uni = uni.copy()
            for r, c in zip(*np.nonzero(pos)):
                uni[r, c] = float(_f(s[r, c]) - _f(iw[r, c]) * _f(ih[r, c]))
        safe = np.where(uni > 0, uni, 1)
        if "iou_multiply" in faults:
            return (uni > 0) & (inter > thr * uni)
        q = inter * (1.0 / safe) if "iou_recip" in faults else inter / safe
        if "iou_trunc" in faults:
            q = q.copy()
            for r, c in zip(*np.nonzero(pos & (uni > 0) & np.isfinite(uni))):
                if _f(q[r, c]) > _f(inter[r, c]) / _f(uni[r, c]):
                    q[r, c] = np.nextafter(q[r, c], 0.0)
        iou = np.where(uni > 0, q, zero).astype(np.float64)
        return iou >= thr if "ge" in faults else iou > thr


def _bits(word):
    word, out = int(word), []
    while word:
        low = word & -word
        out.append(low.bit_length() - 1)
        word ^= low
    return out


def _ballot(flags):
    return int(np.packbits(np.asarray(flags, bool), bitorder="little").view("<u8")[0])


def fresh_scratch(n_words=(BIG_N + 63) // 64, fill=0):
    """What the scan reads of a scratch before writing it: removed[] and cnt[0]."""
    return dict(removed=np.full(n_words, M64 if fill else 0, np.uint64), cnt=0xFFFFFFFF if fill else 0)


_matrix_cache = {}


def emulate(d, faults=(), form=None, scratch=None, prefill=UNTOUCHED):
    """(keep flags int8 [n] in a buffer pre-filled with `prefill`, count) as the five kernels compute them, with `faults`."""
    faults = tuple(faults)
    assert all(f in FAULTS for f in faults), faults
    form = form or d.forms[0]
    if form == "surface":
        form = "rank"
    n = d.n
    n64 = (n + 63) // 64 * 64
    Wn = n64 // 64
    R = d.R if form != "by_key" else max(n64, 64)
    scratch = fresh_scratch(max(Wn, 1)) if scratch is None else scratch
    removed = scratch["removed"]
    keep = np.full(n, prefill, np.int8)
    # ---- order
    under = np.zeros(n, bool)
    if d.score_t is not None:
        st = np.float32(d.score_t)
        under = ~(d.scores > st) if "score_gt" in faults else ~(d.scores >= st)
    group = np.zeros(n, np.int64) if d.group is None or "no_groups" in faults else d.group.astype(np.int64)
    order = np.full(max(n64, 1), 0xFFFFFFFF, np.int64)
    sbox, sgroup, sdead = np.zeros((n64, 4), np.float32), np.zeros(n64, np.int64), np.ones(n64, bool)
    if n:
        if form == "ordered":
            visit = d.order
            ok = visit < n
            ii = np.where(ok, visit, 0)
            order[:n] = np.where(ok, visit, 0xFFFFFFFF)
            sbox[:n], sgroup[:n], sdead[:n] = d.boxes[ii], group[ii], ~ok | under[ii]
        else:
            by_key = form == "by_key"
            lo = d.keys.astype(np.uint64) if by_key else np.arange(n, dtype=np.uint64)
            p = rank_by_counting(score_word(d.scores, "negzero_first" in faults), lo, faults, by_key)
            assert sorted(p.tolist()) == list(range(n))
            order[p] = np.arange(n)
            sbox[p], sgroup[p], sdead[p] = d.boxes, group, under
    # ---- matrix (every band's rows at once: row p, word j / 64)
    iou_faults = tuple(f for f in faults if f.startswith("iou_") or f == "ge")
    cache_key = None if set(faults) & {"ties_desc_index", "negzero_first", "index_before_key"} else (d.name, form, iou_faults, "no_groups" in faults)
    if cache_key in _matrix_cache:
        M = _matrix_cache[cache_key]
    else:
        M = np.zeros((max(n64, 64), max(Wn, 1)), np.uint64)
        col = np.arange(n64)
        for rc in range(Wn):
            rows = np.arange(64 * rc, 64 * rc + 64)
            cb = sbox[np.minimum(col[64 * rc:], n - 1)]
            h = hits(sbox[np.minimum(rows, n - 1)], cb, d.iou_t, iou_faults)
            h &= (sgroup[np.minimum(rows, n - 1)][:, None] == sgroup[np.minimum(col[64 * rc:], n - 1)][None, :])
            h &= (col[None, 64 * rc:] > rows[:, None]) & (col[None, 64 * rc:] < n)
            M[64 * rc:64 * rc + 64, rc:Wn] = np.packbits(h, axis=1, bitorder="little").view("<u8")
        if cache_key is not None:
            _matrix_cache[cache_key] = M
    # ---- bands
    r0, total = 0, 0
    while True:
        rows = min(n64 - r0, R)
        last, first = r0 + rows >= n64, r0 == 0 and "no_first_reset" not in faults
        w0, Rw = r0 // 64, rows // 64
        win, dead0 = np.full(64, M64, np.uint64), []
        for c in range(Rw):
            p = r0 + 64 * c + np.arange(64)
            alive_pad = "padding_alive" in faults
            dead = np.where(p < n, sdead[np.minimum(p, n64 - 1)], not alive_pad)
            m = _ballot(dead)
            dead0.append(m)
            if not first and "no_carry" not in faults:
                m |= int(removed[w0 + c])
            win[c] = np.uint64(m)
        if first:
            removed[w0 + Rw:Wn] = 0
        total = 0 if first else int(scratch["cnt"]) & 0xFFFFFFFF
        keptw, spread_rows = [0] * 64, []
        for c in range(Rw):
            D = M[r0 + 64 * c:r0 + 64 * c + 64, w0 + c].tolist()
            rem, kept = int(win[c]), 0
            for r in range(64):
                bit = 1 << r
                if not rem & bit:
                    kept |= bit
                    rem |= D[r]
                elif "or_removed_rows" in faults and not dead0[c] & bit:
                    rem |= D[r]
            keptw[c] = kept
            total += bin(kept).count("1")
            rs = _bits(kept if "or_removed_rows" not in faults else ~dead0[c] & M64)
            spread_rows.append(rs)
            if "first_round_only" in faults:
                rs = rs[:4]
            hi = Rw - 1 if "last_lane_stale" in faults else Rw
            if rs and hi > c + 1:
                for q in range(0, len(rs), 4):                             # four rows in flight
                    x = M[[r0 + 64 * c + r for r in rs[q:q + 4]], w0 + c + 1:w0 + hi]
                    win[c + 1:hi] |= np.bitwise_or.reduce(x, axis=0)
        for c in range(Rw):
            for lane in range(64):
                p = r0 + 64 * c + lane
                if p < n and order[p] < n:
                    sh = lane & 31 if ("low_half" in faults and lane >= 32) else lane
                    keep[order[p]] = (keptw[c] >> sh) & 1
        scratch["cnt"] = total & 0xFFFFFFFF
        if not last:
            behind = Wn - (w0 + Rw)
            nbx = 1 if "spread_first_block" in faults else (behind + 63) // 64
            lo_w, hi_w = w0 + Rw, min(w0 + Rw + 64 * nbx, Wn)
            for c in range(Rw if "spread_chunks_lt4" not in faults else min(Rw, 4)):
                if spread_rows[c]:
                    removed[lo_w:hi_w] |= np.bitwise_or.reduce(M[[r0 + 64 * c + r for r in spread_rows[c]], lo_w:hi_w], axis=0)
        r0 += rows
        if r0 >= n64:
            break
    return keep, scratch["cnt"]
