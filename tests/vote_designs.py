"""Designed box sets for the voting kernel (wb_vote.hip), where the test decides the answer, and a NumPy emulation of the
kernel with a switch for each way a rewrite could go wrong.  No GPU, no torch.

* PLANTED (exact integer designs): every box sits in a cell of its own or in a cluster around a kept box K = [0, 0, 10, 10] of
  its cell, shifted by dx along x: dx = 0 (a twin), 1, 2 overlap K by 1, 90/110, 80/120 -- voters at vote_iou = 0.5 --, dx = 4,
  8 by 60/140, 20/180 -- suppressed by K at the NMS threshold 0.1, but no voters.  Members of another group (identical boxes
  at dx = 1, the first of them kept) and members under the score threshold lie on top of the voters and must not vote.  Cells
  are CELL apart, coordinates, scores and the threshold are small integers: every weight is an integer, every sum is exact in
  any order, so a wrong voter set shows as a wrong value whatever the order.  The design states its voter sets (`planted`) and
  the merged boxes that follow from them by rational arithmetic (`want`); its keep flags are what greedy NMS answers.
* order_design(): float32 coordinates and score weights found by a seeded search such that the prescribed order of the sums,
  one sequential sum over j, a butterfly that starts at s = 32, a fused multiply-add and a float32 accumulation all give
  different float32 boxes: pairs of voters of equal weight 2^40 .. 2^90 at mirrored x1 / y1 cancel, and what is left of the
  small ones depends on when the large ones met.
* edge_designs(): a voter exactly at vote_iou and one a rounding below it (nms_designs' rounding pairs), a zero-area kept box,
  every voter at the score threshold (sw == 0), -0.0 scores, voters at the first and the last candidate.
* emulate(): the kernel in NumPy; FAULTS names its switches.
tests/test_vote_designs_host.py proves all of it on the CPU; tests/test_gpu_vote_designs.py runs it."""
import functools
from fractions import Fraction

import numpy as np

import nms_designs as nd
from waldboost_amd.boxes import Boxes, iou

CELL, CELLS_X = 32, 512
CHUNK = 256              # WB_VOTE_CHUNK
VOTE_T, NMS_T = 0.5, 0.1
THR = 10                 # the planted designs' score threshold
SIZES = (1, 63, 64, 65, 129, CHUNK - 1, CHUNK, CHUNK + 1)
BIG_N = 4097             # one more than an NMS band


class Design:
    """boxes, scores, group, keep: the call's arrays.  vote_iou, weights, score_t: its scalars; nms_t: the NMS threshold under
    which `keep` is what greedy NMS answers.  planted: {kept index: sorted voter indices} or None; want: (merged, votes) that
    follow from `planted` in exact arithmetic, or None (the statement decides)."""

    def __init__(self, name, boxes, scores, keep, group=None, vote_iou=VOTE_T, weights="uniform", score_t=None, nms_t=NMS_T, planted=None):
        self.name, self.n = name, len(scores)
        self.boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        self.scores = np.ascontiguousarray(scores, np.float32)
        self.group = None if group is None else np.ascontiguousarray(group, np.int32)
        self.keep = np.ascontiguousarray(keep, np.uint8)
        self.vote_iou, self.weights, self.score_t, self.nms_t = float(vote_iou), weights, score_t, nms_t
        self.planted = planted
        self.want = None if planted is None else exact_result(self)

    @property
    def n_keep(self):
        return int((self.keep != 0).sum())

    def args(self):
        """The keywords of vote_reference.vote / boxes.vote_boxes behind (boxes, scores, keep)."""
        return dict(vote_iou=self.vote_iou, weights=self.weights, score_threshold=self.score_t, group=self.group)

    def __repr__(self):
        return self.name


def weight_of(d, j):
    """w_j as an exact rational."""
    return Fraction(1) if d.weights == "uniform" else Fraction(float(d.scores[j])) - Fraction(float(np.float32(d.score_t)))


def exact_result(d):
    """(merged float32 [n][4], votes int32 [n]) from d.planted by rational arithmetic: the sums exactly, ONE rounding of the
    quotient to float64 (what a correctly rounded divide of two exactly summed doubles gives), then the cast."""
    merged, votes = d.boxes.copy(), np.zeros(d.n, np.int32)
    for k, js in d.planted.items():
        ws = [weight_of(d, j) for j in js]
        sw = sum(ws)
        votes[k] = len(js)
        if sw > 0:
            for i in range(4):
                sc = sum(w * Fraction(float(d.boxes[j, i])) for w, j in zip(ws, js))
                assert abs(sc.numerator) < 2 ** 53 and sc.denominator == 1 and sw.denominator == 1 and sw < 2 ** 53      # exact in float64
                merged[k, i] = np.float32(float(sc / sw))
    return merged, votes


def cell_origin(c):
    return CELL * (c % CELLS_X), CELL * (c // CELLS_X)


# ------------------------------------------------------------------------------ planted designs
class Plant:
    """A planted design under construction.  cluster(k, ...) puts K at input index k and its members at the given indices."""

    def __init__(self, name, n, weights="uniform", score_t=None):
        self.name, self.n, self.weights, self.score_t = name, n, weights, score_t
        self.box = np.zeros((n, 4), np.int64)
        self.score = np.zeros(n, np.float64)
        self.group = np.zeros(n, np.int64)
        self.keep = np.zeros(n, np.uint8)
        self.used = np.zeros(n, bool)
        self.planted = {}
        self.cells = 0
        self.use_groups = False

    def _put(self, j, cell, dx, score, group=0, keep=0, size=10):
        assert not self.used[j], (self.name, j)
        ox, oy = cell_origin(cell)
        self.box[j] = [ox + dx, oy, ox + dx + size, oy + size]
        self.score[j], self.group[j], self.keep[j], self.used[j] = score, group, keep, True
        if group:
            self.use_groups = True

    def cluster(self, k, voters=(), near=(), other=(), dead=(), k_score=None):
        """voters: [(index, dx in 0 1 2)], near: [(index, dx in 4 8)], other: indices of another group's twins at dx = 1 (the
        first is kept, the rest vote for it), dead: indices under the score threshold at dx = 1.  K's score is the cell's
        highest (of equal scores K comes first in the input); members' scores are THR + (index % 5)."""
        c = self.cells
        self.cells += 1
        self._put(k, c, 0, 100 + k % 21 if k_score is None else k_score, keep=1)
        mine = [k]
        for j, dx in voters:
            assert dx in (0, 1, 2)
            self._put(j, c, dx, min(THR + j % 5, self.score[k]))
            assert self.score[j] < self.score[k] or j > k
            mine.append(j)
        for j, dx in near:
            assert dx in (4, 8)
            self._put(j, c, dx, THR + j % 5)
        for j in dead:
            assert self.score_t is not None
            self._put(j, c, 1, THR - 1 - j % 3)
        theirs = []
        for q, j in enumerate(other):
            self._put(j, c, 1, 90 if q == 0 else THR + j % 5, group=1, keep=1 if q == 0 else 0)
            theirs.append(j)
        self.planted[k] = sorted(mine)
        if theirs:
            self.planted[theirs[0]] = sorted(theirs)
        return self

    def zero_area(self, j, cell=None):
        """A kept box of no area (twins of it share `cell`: their IoU is 0, each is kept and votes for itself alone)."""
        if cell is None:
            cell = self.cells
            self.cells += 1
        self._put(j, cell, 3, 50 + j % 11, keep=1, size=0)
        self.planted[j] = [j]
        return cell

    def build(self, vote_iou=VOTE_T):
        for j in np.flatnonzero(~self.used):                   # filler: a cell of its own, kept, its own only voter
            self._put(j, self.cells, 0, 50 + j % 11, keep=1)
            self.planted[int(j)] = [int(j)]
            self.cells += 1
        assert self.cells <= CELLS_X * CELLS_X
        return Design(self.name, self.box, self.score, self.keep, self.group if self.use_groups else None, vote_iou, self.weights,
                      self.score_t, NMS_T, dict(sorted(self.planted.items())))


def sprinkle(n, seed, weights="uniform", score_t=None, groups=False, mean_cluster=4, name=None):
    """A planted design of any n: clusters of seeded sizes at seeded input indices, the rest filler."""
    p = Plant(name or f"sprinkle-n{n}-{weights}{'-thr' if score_t is not None else ''}{'-groups' if groups else ''}", n, weights, score_t)
    rng = np.random.default_rng(seed)
    free = rng.permutation(n).tolist()
    if n >= 3:                                                 # a cluster whose voters are the first and the last candidate
        k = free.pop(next(i for i, j in enumerate(free) if j not in (0, n - 1)))
        free = [j for j in free if j not in (0, n - 1)]
        p.cluster(k, voters=[(0, 1), (n - 1, 2)], k_score=200)
    while free:
        size = int(min(len(free), rng.integers(1, 2 * mean_cluster)))
        ks, free = free[:size], free[size:]
        if size == 1:
            continue                                           # filler
        k = min(ks)                                            # (of equal scores the earlier index goes first)
        kinds = ["voter", "near"] + (["other"] if groups else []) + (["dead"] if score_t is not None else [])
        parts = dict(voter=[], near=[], other=[], dead=[])
        for j in ks:
            if j != k:
                kind = kinds[int(rng.integers(0, len(kinds)))] if rng.random() < 0.6 else "voter"
                parts[kind].append(j)
        p.cluster(k, voters=[(j, int(rng.integers(0, 3))) for j in parts["voter"]], near=[(j, (4, 8)[int(rng.integers(0, 2))]) for j in parts["near"]],
                  other=parts["other"], dead=parts["dead"])
    return p.build()


@functools.lru_cache(None)
def planted():
    out = []
    for n in SIZES:
        out.append(sprinkle(n, n))
        out.append(sprinkle(n, 1000 + n, "score", THR, groups=True))
    out.append(sprinkle(129, 7, "uniform", THR, groups=True))
    out.append(sprinkle(BIG_N, 41, "score", THR, groups=True, mean_cluster=10))
    out.append(sprinkle(BIG_N, 42, "uniform", mean_cluster=10))
    # K in every chunk position class, its voters in other chunks and lanes
    p = Plant("positions-n600", 600)
    p.cluster(0, voters=[(63, 1), (64, 2), (255, 0), (257, 1), (598, 2)], near=[(1, 4), (258, 8)])
    p.cluster(599, voters=[(597, 1), (2, 2)], k_score=300)
    p.cluster(256, voters=[(320, 0), (384, 1), (448, 2), (512, 1), (576, 2)], near=[(65, 4)])       # every voter in K's lane
    p.cluster(511, voters=[(3, 1), (510, 2)], k_score=301)
    out.append(p.build())
    # groups whose boxes coincide: twins of both groups on top of each other
    p = Plant("coinciding-groups-n70", 70, "score", THR)
    p.cluster(5, voters=[(6, 0), (40, 0), (69, 1)], other=[7, 8, 41, 68], dead=[9, 42])
    p.cluster(30, voters=[(31, 0)], other=[0], dead=[64])
    out.append(p.build())
    # a box that is not live on top of a kept one, uniform weights (liveness is not a matter of the weights)
    p = Plant("not-live-uniform-n66", 66, "uniform", THR)
    p.cluster(10, voters=[(11, 1), (65, 2)], dead=[0, 12, 64])
    out.append(p.build())
    # zero-area kept boxes, alone and as twins
    p = Plant("zero-area-n67", 67)
    c = p.zero_area(3)
    p.zero_area(66, c)
    p.zero_area(0)
    p.cluster(20, voters=[(21, 1)])
    out.append(p.build())
    # every voter exactly at the threshold under "score": sw == 0, the kept box stays
    p = Plant("all-at-threshold-n130", 130, "score", THR)
    p.cluster(4, voters=[(70, 1), (129, 2), (64, 0)], k_score=THR)
    p.cluster(5, voters=[(6, 1)], k_score=THR + 3)             # (next to it a cluster whose kept box alone has weight)
    for j in (70, 129, 64, 6):
        p.score[j] = THR
    out.append(p.build())
    return out


# ------------------------------------------------------------------------------ edge designs (the statement decides)
def _among_filler(name, rows, scores, n, at, **kw):
    """`rows` at the input indices `at`, filler boxes (cells of their own, far away) everywhere else; keep = greedy NMS."""
    from nms_reference import nms_keep
    boxes = np.empty((n, 4), np.float32)
    ox, oy = cell_origin(np.arange(n))
    boxes[:] = np.stack([16384 + ox, oy, 16384 + ox + 10, oy + 10], 1)
    sc = (3 + np.arange(n) % 7).astype(np.float32)
    boxes[list(at)], sc[list(at)] = rows, scores
    keep = nms_keep(boxes, sc, kw.get("nms_t", NMS_T), kw.get("group"), kw.get("score_t"))
    return Design(name, boxes, sc, keep, **kw)


@functools.lru_cache(None)
def edge_designs():
    out = []
    seen = set()
    for form, a, b, fm, _ in nd.rounding_pairs():             # general float32 pairs whose IoU the wrong forms round differently
        if form in seen:
            continue
        seen.add(form)
        u = fm["u"]
        for label, t in (("at", u), ("a-rounding-above", float(np.nextafter(u, 1.0)))):
            d = _among_filler(f"threshold-{form}-{label}", [a, b], [900, 800], 130, (17, 100), vote_iou=t, nms_t=u / 2)
            d.expect_votes = {17: 2 if t == u else 1}
            out.append(d)
    f = lambda *r: np.array(r, np.float32)
    # 80/120 as a double, and the next double above it
    u = 80.0 / 120.0
    for label, t in (("at", u), ("a-rounding-above", float(np.nextafter(u, 1.0)))):
        d = _among_filler(f"threshold-two-thirds-{label}", f([0, 0, 10, 10], [2, 0, 12, 10]), [900, 800], 65, (64, 0), vote_iou=t)
        d.expect_votes = {64: 2 if t == u else 1}
        out.append(d)
    # -0.0 scores: live at a threshold of either zero, weight 0 under "score" and 1 under "uniform"
    for weights in ("uniform", "score"):
        for thr in (0.0, -0.0):
            d = _among_filler(f"negative-zero-{weights}-thr{thr}", f([0, 0, 10, 10], [1, 0, 11, 10], [2, 0, 12, 10], [1, 0, 11, 10]),
                              [5, -0.0, 0.0, -1.0], 70, (3, 0, 69, 33), weights=weights, score_t=thr)
            d.expect_votes = {3: 3}
            out.append(d)
    # vote_iou = 0: every live box of the group votes for every kept box
    d = _among_filler("vote-iou-zero-n20", f([0, 0, 10, 10], [1, 0, 11, 10]), [900, 800], 20, (4, 9), vote_iou=0.0)
    d.expect_votes = {4: 20}
    out.append(d)
    return out


# ------------------------------------------------------------------------------ the order design
ORDER_N, ORDER_PAIRS, ORDER_SEED = 300, 100, 0
ORDER_THR = -1.2345678 * 2.0 ** 64       # (a weight score - threshold then has up to 53 bits, and its product with a coordinate rounds)


def order_family(seed):
    """One kept box [0, 0, 10, 10] of score 2^100 at a seeded index and ORDER_PAIRS pairs of voters: the two of a pair have one
    score m * 2^e (e in 40 .. 90) and mirrored x1 = +-a, y1 = +-b; the rest is filler.  "score" weights from the threshold
    ORDER_THR, which lies under every score."""
    rng = np.random.default_rng(seed)
    n = ORDER_N
    at = rng.permutation(n)[:1 + 2 * ORDER_PAIRS]
    rows, scores = np.zeros((at.size, 4), np.float32), np.zeros(at.size, np.float32)
    rows[0], scores[0] = [0, 0, 10, 10], 2.0 ** 100
    for q in range(ORDER_PAIRS):
        a, b = rng.uniform(0.01, 0.5, 2).astype(np.float32)
        far = (10 + rng.uniform(-0.5, 0.5, 4)).astype(np.float32)
        s = np.float32(rng.uniform(1, 2) * 2.0 ** rng.integers(40, 91))
        rows[1 + 2 * q], rows[2 + 2 * q] = [a, b, far[0], far[1]], [-a, -b, far[2], far[3]]
        scores[1 + 2 * q] = scores[2 + 2 * q] = s
    d = _among_filler(f"order-seed{seed}", rows, scores, n, at, weights="score", score_t=ORDER_THR, nms_t=0.3)
    d.kept_box = int(at[0])
    return d


def separates(d):
    """The float32 box of d's kept box under the prescribed order and under each wrong one; True when all differ from it."""
    k = d.kept_box
    right = emulate(d)[0][k]
    wrong = {f: emulate(d, (f,))[0][k] for f in ("sequential", "butterfly_from_32", "fma", "f32_acc")}
    return all(not np.array_equal(right.view(np.uint32), w.view(np.uint32)) for w in wrong.values()), right, wrong


def search_order_seed(limit=64):
    return next(seed for seed in range(limit) if separates(order_family(seed))[0])


@functools.lru_cache(None)
def order_design():
    return order_family(ORDER_SEED)


def all_designs():
    return planted() + edge_designs() + [order_design()]


# ------------------------------------------------------------------------------ the kernel in NumPy
FAULTS = ("gt", "no_self", "no_groups", "dead_vote", "fma", "f32_acc", "sequential", "skip_partial_chunk", "kept_weight", "divide_zero",
          "votes_lane0", "butterfly_from_32")
SLOW_FAULTS = ("fma",)       # scalar loops with rational arithmetic: small designs only


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _sum_lanes(w, x, v, faults):
    """(sw, sc[4], votes) of one kept box: w float64 [n], x float64 [n][4], v bool [n]."""
    n = w.size
    ft = np.float32 if "f32_acc" in faults else np.float64
    w, x = w.astype(ft), x.astype(ft)
    terms = np.concatenate([w[:, None], w[:, None] * x], 1)
    terms = np.where(v[:, None], terms, ft(0))
    if "sequential" in faults:
        tot = np.add.accumulate(np.concatenate([np.zeros((1, 5), ft), terms]), 0)[-1]
        return tot[0], tot[1:], int(v.sum())
    rows = -(-n // 64)
    pad = np.zeros((rows * 64, 5), ft)
    pad[:n] = terms
    pad = pad.reshape(rows, 64, 5)
    cnt = np.zeros(rows * 64, np.int64)
    cnt[:n] = v
    cnt = cnt.reshape(rows, 64).sum(0)
    if "fma" in faults:
        p = np.zeros((64, 5))
        for j in np.flatnonzero(v):
            l = j % 64
            p[l, 0] = p[l, 0] + float(w[j])
            for i in range(4):
                p[l, 1 + i] = _fma(float(w[j]), float(x[j, i]), p[l, 1 + i])
    else:
        p = np.zeros((64, 5), ft)
        for r in range(rows):
            p = p + pad[r]
    votes0 = int(cnt[0])
    lane = np.arange(64)
    for s in ((32, 16, 8, 4, 2, 1) if "butterfly_from_32" in faults else (1, 2, 4, 8, 16, 32)):
        p = p + p[lane ^ s]
        cnt = cnt + cnt[lane ^ s]
    return p[0, 0], p[0, 1:], votes0 if "votes_lane0" in faults else int(cnt[0])


def emulate(d, faults=()):
    """(merged float32 [n][4], votes int32 [n]) as the kernel computes them, with `faults`."""
    faults = tuple(faults)
    assert all(f in FAULTS for f in faults), faults
    n = d.n
    merged, votes = d.boxes.copy(), np.zeros(n, np.int32)
    x = d.boxes.astype(np.float64)
    thr = None if d.score_t is None else np.float32(d.score_t)
    live = np.ones(n, bool) if thr is None or "dead_vote" in faults else d.scores >= thr
    w_all = np.ones(n) if d.weights == "uniform" else d.scores.astype(np.float64) - np.float64(thr)
    kept = np.flatnonzero(d.keep != 0)
    seen = n // CHUNK * CHUNK if "skip_partial_chunk" in faults else n
    for k0 in range(0, kept.size, 128):
        ks = kept[k0:k0 + 128]
        table = iou(Boxes(d.boxes[ks]), Boxes(d.boxes))
        for k, row in zip(ks, table):
            v = (row > d.vote_iou if "gt" in faults else row >= d.vote_iou) & live
            if d.group is not None and "no_groups" not in faults:
                v &= d.group == d.group[k]
            if "no_self" not in faults:
                v[k] = True
            v[seen:] = False
            w = np.full(n, w_all[k]) if "kept_weight" in faults else w_all
            sw, sc, votes[k] = _sum_lanes(w, x, v, faults)
            with np.errstate(all="ignore"):
                if sw > 0 or ("divide_zero" in faults and sw == 0):
                    merged[k] = (sc / sw).astype(np.float32)
    return merged, votes
