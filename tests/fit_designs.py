"""Designed inputs for the split-search kernels (csrc/wb_fit.hip) at the C ABI, and an exact reference (NumPy only: no GPU,
no torch).

A random tree leaves to chance whether two thresholds or two features tie, how large a node is, which lane holds a zero
and whether a weightless sample bounds a column.  Here the test plants which (feature, threshold) wins in every open node
and by what margin, and knows the answer before any kernel runs.

Why it can be exact.  The weights q are integers.  In designs 1-6 they are small integers k shifted left by one common
power of two (at least 2^12) so that the larger class sums to just under 2^61: every partial sum then has fewer than 50
significant bits, `double(sum) * 2^-62` is exact, and the float64 cumulative sums of tests/fit_reference.py are the same
numbers as the kernel's integer sums.  Two candidates with the same integer (L0, L1, T0, T1) get bit-identical metrics on
every side: a tie is exact, and the contract's rule -- the smallest t, then the first entry of A -- decides it.

A planted node.  Column f* of the node's samples holds 30 .. t*-10 for class 0 and t* .. 255 for class 1, with the class
of one sample in ten flipped; the other columns are noise, half of it zeros.  The best threshold is any t with the low
group on its left: the run (largest value below t*) + 1 .. (smallest value from t* on), at least ten wide, all tied; the
expected t is its first.  A copy of the column under another feature index ties across A; the expected feature is
whichever comes first in A.

`exact_tables` is the high-precision reference: integer histograms, `float(int) * 2^-62`, then the contract's metric in
its operation order in extended precision (np.longdouble with a 64-bit significand; mpmath at 80 bits of working
precision where the platform's long double is no wider than a double).  `fit_reference.metric_table` stays the float64
yardstick, and `yardstick_deviation()` measures how far the two are apart.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import fit_reference as fr

NAN_NODE = "nan"                 # want[s] of a node without weight in one class: (A[0], xmin of A[0]'s column), NaN metric
NO_CANDIDATE = -np.inf
SCALE = 2.0 ** -62
EXTENDED = np.finfo(np.longdouble).nmant >= 63
if not EXTENDED:
    import mpmath                # (asserted here, at import: there is an extended format either way)
    mpmath.mp.prec = 80
assert EXTENDED or mpmath.mp.prec >= 64

PLANTED_N = (63, 64, 65, 255, 256, 257, 700)         # below, at, over one wave / one pass of the 256-thread column walk
EIGHT_SIZES = (1, 63, 64, 65, 255, 256, 257, 700)
EIGHT_SLOTS = (5, 2, 7, 0, 1, 6, 4, 3)
BETWEEN_SLOTS = (-1, 2, -1, 0, 1, -1, -1, 3)


@dataclass
class Design:
    name: str
    xt: np.ndarray               # uint8 [F][N], feature-major
    q: np.ndarray                # uint64 [N]
    cls: np.ndarray              # uint8 [N]
    node: np.ndarray             # int32 [N]
    level_base: int
    n_level: int
    slot: np.ndarray             # int8 [n_level]
    n_open: int
    A: np.ndarray                # int32 [n_allowed]
    want: list                   # per open slot (feature, threshold) or NAN_NODE
    tie_t: list = field(default_factory=list)        # per open slot: an exact tie over >= 2 thresholds is claimed
    tie_A: list = field(default_factory=list)        # per open slot: ... and over >= 2 entries of A
    exact_sums: bool = True      # every partial sum is a float64 (designs 1-6)

    def node_of(self, s):
        return self.level_base + int(np.flatnonzero(self.slot == s)[0])

    def samples(self, s):
        return np.flatnonzero(self.node == self.node_of(s))

    def expected(self, s):
        """(feature, threshold, metric is NaN) of open slot s."""
        if self.want[s] == NAN_NODE:
            return int(self.A[0]), int(self.xt[self.A[0], self.samples(s)].min()), True
        return int(self.want[s][0]), int(self.want[s][1]), False

    def permuted(self, perm):
        return Design(self.name + "/permuted", np.ascontiguousarray(self.xt[:, perm]), self.q[perm].copy(), self.cls[perm].copy(),
                      self.node[perm].copy(), self.level_base, self.n_level, self.slot, self.n_open, self.A, self.want, self.tie_t,
                      self.tie_A, self.exact_sums)


# ------------------------------------------------------------------------------ building blocks
def _scaled(k):
    """Small integer weights -> q: one power-of-two factor (>= 2^12) that brings the sum of all of them under 2^61, so a
    class's sum is about 2^61 at the most and any partial sum is a float64."""
    k = np.asarray(k, np.uint64)
    total = int(k.sum(dtype=np.uint64))
    shift = 61 - total.bit_length()
    assert shift >= 12 and total.bit_length() + 1 <= 50
    return k << np.uint64(shift)


def _balanced_classes(rng, n):
    return rng.permutation(np.arange(n) % 2).astype(np.uint8)


def _planted_values(rng, cls, tstar, flip=0.1, low=30):
    """Class 0 in low .. tstar-10, class 1 in tstar .. 255, the class of round(flip * n) samples swapped; a swapped sample
    keeps 20 values away from the gap, so that no threshold beside the gap sheds swapped samples only."""
    n = cls.size
    swapped = np.zeros(n, bool)
    swapped[rng.permutation(n)[:int(round(flip * n))]] = True
    side = cls.astype(np.int64) ^ swapped
    lo = np.where(swapped, rng.integers(low, tstar - 29, n), rng.integers(low, tstar - 9, n))
    hi = np.where(swapped, rng.integers(tstar + 20, 256, n), rng.integers(tstar, 256, n))
    return np.where(side == 0, lo, hi).astype(np.uint8)


def _noise(rng, n, F, zero_share=0.5):
    x = rng.integers(0, 256, (n, F))
    x[rng.random((n, F)) < zero_share] = 0
    return x.astype(np.uint8)


def _first_of_run(x, q, tstar):
    """The first threshold of the tied run below tstar: one more than the largest value under tstar that carries weight."""
    below = x[(x < tstar) & (q > 0)]
    return int(below.max()) + 1


def _level(name, rng, F, A, level_base, n_level, slots, open_nodes, other_nodes=(), exact_sums=True, weights=None):
    """A level from node descriptions.  open_nodes: per level position j a planted node dict(n, fstar, dup, tstar), or
    dict(n, kind) for a NaN node: 'one_sample', 'weightless_class1' (class-1 samples present, all with q = 0) or
    'no_class1'.  other_nodes: (node id, n) of leaves and foreign nodes, whose samples weigh the most and hold only 0 and
    255.  Samples of all nodes are interleaved at random.  weights: None for exact-sum weights, or (rng, cls) -> q."""
    ids = []
    for j, d in open_nodes.items():
        ids += [level_base + j] * d["n"]
    for nid, n in other_nodes:
        ids += [nid] * n
    node = rng.permutation(np.array(ids, np.int32))
    N = node.size
    X = _noise(rng, N, F)
    cls = np.zeros(N, np.uint8)
    k = rng.integers(256, 1024, N).astype(np.uint64)
    for nid, n in other_nodes:
        S = np.flatnonzero(node == nid)
        X[S] = rng.choice(np.array([0, 255], np.uint8), (S.size, F))
        cls[S] = _balanced_classes(rng, S.size)
        k[S] = 4095
    slot = np.asarray(slots, np.int8)
    n_open = int((slot >= 0).sum())
    A = np.asarray(A, np.int32)
    want, tie_t, tie_A = [None] * n_open, [False] * n_open, [False] * n_open
    for j, d in open_nodes.items():
        S = np.flatnonzero(node == level_base + j)
        kind = d.get("kind", "planted")
        if kind == "planted":
            cls[S] = _balanced_classes(rng, S.size)
            X[S, d["fstar"]] = _planted_values(rng, cls[S], d["tstar"])
            if d.get("dup") is not None:
                X[S, d["dup"]] = X[S, d["fstar"]]
        elif kind == "one_sample":
            cls[S] = 1
        else:                                   # a node without weight in class 1; a weightless sample holds A[0]'s minimum
            cls[S] = 0 if kind == "no_class1" else _balanced_classes(rng, S.size)
            k[S[cls[S] == 1]] = 0
            X[S, A[0]] = rng.integers(30, 256, S.size)
            light = S[cls[S] == 1][0] if kind == "weightless_class1" else S[0]
            k[light] = 0
            X[light, A[0]] = 3
    q = _scaled(k) if weights is None else weights(rng, cls)
    for j, d in open_nodes.items():
        S = np.flatnonzero(node == level_base + j)
        s = int(slot[j])
        if d.get("kind", "planted") != "planted":
            want[s] = NAN_NODE
            continue
        pos = [int(np.flatnonzero(A == f)[0]) for f in (d["fstar"], d.get("dup")) if f is not None and f in A]
        want[s] = (int(A[min(pos)]), _first_of_run(X[S, d["fstar"]], q[S], d["tstar"]))
        tie_t[s], tie_A[s] = True, len(pos) == 2
    return Design(name, np.ascontiguousarray(X.T), q, cls, node, level_base, n_level, slot, n_open, A, want, tie_t, tie_A, exact_sums)


# ------------------------------------------------------------------------------ the designs
def planted(seed, n, dup_first):
    """1: one open node of n samples, 9 features; the duplicate of f* = 4 is feature 7, before or after it in a
    non-ascending A."""
    rng = np.random.default_rng([1, seed, n, dup_first])
    A = [8, 2, 7, 0, 4, 6, 1, 5, 3] if dup_first else [8, 2, 4, 0, 7, 6, 1, 5, 3]
    return _level(f"planted[{n}-{'dup_first' if dup_first else 'dup_last'}]", rng, 9, A, 0, 1, [0],
                  {0: dict(n=n, fstar=4, dup=7, tstar=int(rng.integers(80, 200)))})


def eight_nodes(seed):
    """2: level 7 .. 14, all open, permuted slots, sizes 1 .. 700 interleaved; node j plants feature j with its copy
    8 + j, the copy first in A for odd j; the one-sample node is a NaN node."""
    rng = np.random.default_rng([2, seed])
    A = [18, 16, 9, 1, 0, 8, 11, 3, 2, 10, 17, 13, 5, 4, 12, 15, 7, 6, 14]
    sizes = rng.permutation(EIGHT_SIZES)
    nodes = {}
    for j, n in enumerate(sizes):
        nodes[j] = dict(n=int(n), kind="one_sample") if n == 1 else dict(n=int(n), fstar=j, dup=8 + j, tstar=70 + 20 * j)
    return _level("eight_nodes", rng, 19, A, 7, 8, EIGHT_SLOTS, nodes)


def leaves_between(seed):
    """3: four open nodes between four leaves, plus samples of nodes outside the level; the bystanders weigh the most and
    hold 0 and 255, and must change nothing."""
    rng = np.random.default_rng([3, seed])
    A = [6, 0, 9, 3, 5, 1, 8, 2, 7, 4]
    nodes = {1: dict(n=100, fstar=0, dup=5, tstar=90), 3: dict(n=65, fstar=1, dup=6, tstar=140),
             4: dict(n=130, fstar=2, dup=7, tstar=200), 7: dict(n=257, fstar=3, dup=8, tstar=120)}
    others = [(7, 40), (9, 40), (12, 40), (13, 40), (0, 30), (3, 30), (6, 30), (15, 30), (16, 30), (22, 30)]
    return _level("leaves_between", rng, 10, A, 7, 8, BETWEEN_SLOTS, nodes, others)


def nan_beside_normal(seed, no_class1):
    """4: a node without class-1 weight (weightless class-1 samples, or none at all) beside a planted node; in the NaN
    node a weightless sample holds the smallest value of A[0]'s column."""
    rng = np.random.default_rng([4, seed, no_class1])
    A = [5, 1, 3, 0, 4, 2]
    nodes = {0: dict(n=90, kind="no_class1" if no_class1 else "weightless_class1"), 1: dict(n=150, fstar=3, dup=2, tstar=110)}
    return _level(f"nan_beside_normal[{'no_class1' if no_class1 else 'weightless'}]", rng, 6, A, 1, 2, [1, 0], nodes)


EDGE_COLUMNS = ("all_0", "all_255", "only_0_and_255", "zeros_in_lane_5", "weightless_0_below_50", "weightless_bounds")


def edge_columns(seed, column):
    """5: one node of 300 samples rated one column at a time (A = [f]).  all_0 is also the column with a zero at every
    index (every lane of the zero-bin copy adds); zeros_in_lane_5 has its zeros at i % 64 == 5 only (one lane carries
    them all); weightless_bounds: every weighted sample holds 50, weightless ones 0 and 255, so all 257 candidates tie.
    want is the first argmax of the exact table (test_fit_designs_host.py states the closed forms it must equal)."""
    rng = np.random.default_rng([5, seed])
    n = 300
    cls = _balanced_classes(rng, n)
    k = rng.integers(256, 1024, n).astype(np.uint64)
    k[[7, 100, 299]] = 0
    X = np.zeros((n, len(EDGE_COLUMNS)), np.uint8)
    X[:, 1] = 255
    X[:, 2] = np.where(_planted_values(rng, cls, 128) < 128, 0, 255)
    X[:, 3] = _planted_values(rng, cls, 150)
    X[np.arange(n) % 64 == 5, 3] = 0
    X[:, 4] = _planted_values(rng, cls, 170, low=50)
    X[7, 4] = 0
    X[:, 5] = 50
    X[100, 5], X[299, 5] = 0, 255
    f = EDGE_COLUMNS.index(column)
    d = Design(f"edge_columns[{column}]", np.ascontiguousarray(X.T), _scaled(k), cls, np.zeros(n, np.int32), 0, 1,
               np.array([0], np.int8), 1, np.array([f], np.int32), [None], [column != "zeros_in_lane_5"], [False])
    _, t, _ = first_argmax(_tables(d)[0]["table"])
    d.want[0] = (f, t)
    return d


WIDE_CASES = {                  # name: (n_allowed, position of f* in A, position of its copy or None)
    "256-late": (256, 200, 255),        # the last thread of fit_pick_kernel's first pass holds the copy
    "257-late": (257, 256, None),       # f* is the one entry of the second pass
    "257-early": (257, 3, 256),         # ... or its copy is, and must not displace the earlier entry
    "600-late": (600, 300, 599),
    "600-early": (600, 599, 3),         # the copy comes first and wins
}


def wide_A(seed, which):
    """6: 640 features, 300 samples, A a shuffle of n_allowed distinct features in which f* and its copy sit at the
    positions of WIDE_CASES."""
    n_allowed, at_f, at_dup = WIDE_CASES[which]
    rng = np.random.default_rng([6, seed, n_allowed, at_f])
    F, fstar, dup = 640, 611, 17
    rest = iter(rng.permutation(np.setdiff1d(np.arange(F), [fstar, dup])).tolist())
    A = [fstar if i == at_f else dup if i == at_dup else next(rest) for i in range(n_allowed)]
    assert len(set(A)) == n_allowed
    return _level(f"wide_A[{which}]", rng, F, A, 0, 1, [0],
                  {0: dict(n=300, fstar=fstar, dup=None if at_dup is None else dup, tstar=int(rng.integers(80, 200)))})


def three_wide(seed):
    """Three open nodes and a leaf over 257 entries of A: the record block of the scratch is no multiple of 16 bytes."""
    rng = np.random.default_rng([8, seed])
    A = rng.permutation(300)[:257].tolist()
    nodes = {0: dict(n=80, fstar=int(A[256]), dup=None, tstar=100), 2: dict(n=70, fstar=int(A[5]), dup=int(A[200]), tstar=150),
             3: dict(n=64, fstar=int(A[100]), dup=int(A[40]), tstar=190)}
    return _level("three_wide", rng, 300, A, 3, 4, [2, -1, 0, 1], nodes, [(4, 20)])


def _lognormal_q(rng, cls):
    W = np.exp(rng.normal(0, 3, cls.size))
    w = W.copy()
    for c in (0, 1):
        w[cls == c] /= w[cls == c].sum() * 2
    q = np.rint(np.ldexp(w, 62)).astype(np.uint64)
    order = rng.permutation(cls.size)
    q[order[:4]] = 1
    q[order[4:8]] = 0
    return q


def full_bits(seed):
    """7: planted, 700 samples, q = rint(w' * 2^62) of log-normal weights (sigma 3): all 62 bits in use, sums that no
    float64 holds; a few q are 1 and a few 0.  The copy of the column still ties exactly."""
    rng = np.random.default_rng([7, seed])
    d = _level("full_bits", rng, 9, [8, 2, 7, 0, 4, 6, 1, 5, 3], 0, 1, [0],
               {0: dict(n=700, fstar=4, dup=7, tstar=int(rng.integers(80, 200)))}, exact_sums=False, weights=_lognormal_q)
    assert int(d.q.max()).bit_length() >= 58 and np.any(d.q & np.uint64(0xfff))
    return d


CASES = {}
for _n in PLANTED_N:
    for _first in (True, False):
        CASES[f"planted[{_n}-{'dup_first' if _first else 'dup_last'}]"] = functools.partial(planted, 0, _n, _first)
CASES["eight_nodes"] = functools.partial(eight_nodes, 0)
CASES["leaves_between"] = functools.partial(leaves_between, 0)
for _v in (False, True):
    CASES[f"nan_beside_normal[{'no_class1' if _v else 'weightless'}]"] = functools.partial(nan_beside_normal, 0, _v)
for _c in EDGE_COLUMNS:
    CASES[f"edge_columns[{_c}]"] = functools.partial(edge_columns, 0, _c)
for _w in WIDE_CASES:
    CASES[f"wide_A[{_w}]"] = functools.partial(wide_A, 0, _w)
CASES["three_wide"] = functools.partial(three_wide, 0)
CASES["full_bits"] = functools.partial(full_bits, 0)


@functools.lru_cache(maxsize=None)
def design(name):
    d = CASES[name]()
    assert d.name == name, (d.name, name)
    for a in (d.xt, d.q, d.cls, d.node):
        a.setflags(write=False)
    return d


# ------------------------------------------------------------------------------ the exact reference
def _entropy(a, b):
    tot = a + b
    pa, pb = a / tot, b / tot
    return -(pa * np.log2(pa) + pb * np.log2(pb))


def _metric_extended(L0, L1, t0, t1):
    """The contract's metric for float64 L0, L1 [nA][257] and totals t0, t1, in extended precision, its operation order."""
    if EXTENDED:
        ld = np.longdouble
        L0, L1, t0, t1, eps = L0.astype(ld), L1.astype(ld), ld(t0), ld(t1), ld(1e-4)
        with np.errstate(all="ignore"):
            tsum = t0 + t1
            R0, R1 = t0 - L0, t1 - L1
            return _entropy(t0, t1) - ((L0 + L1) / tsum * _entropy(L0 + eps, L1 + eps) + (R0 + R1) / tsum * _entropy(R0 + eps, R1 + eps))
    mp = mpmath.mp

    def H(a, b):
        tot = a + b
        pa, pb = a / tot, b / tot
        return -(pa * mp.log(pa, 2) + pb * mp.log(pb, 2))

    out = np.empty(L0.shape, object)
    T0, T1, eps = mp.mpf(float(t0)), mp.mpf(float(t1)), mp.mpf(1e-4)
    for i in np.ndindex(L0.shape):
        if t0 == 0 or t1 == 0:
            out[i] = mp.nan
            continue
        l0, l1 = mp.mpf(float(L0[i])), mp.mpf(float(L1[i]))
        out[i] = H(T0, T1) - ((l0 + l1) / (T0 + T1) * H(l0 + eps, l1 + eps) + (T0 - l0 + T1 - l1) / (T0 + T1) * H(T0 - l0 + eps, T1 - l1 + eps))
    return out


def _tables(d):
    out = []
    nA = d.A.size
    for s in range(d.n_open):
        S = d.samples(s)
        assert S.size >= 1
        xs = d.xt[d.A.astype(np.int64)][:, S].astype(np.int64)                         # [nA][|S|]
        hist = np.zeros((2, nA, 256), np.uint64)
        np.add.at(hist, (d.cls[S].astype(np.int64)[None, :], np.arange(nA)[:, None], xs), d.q[S][None, :])
        ints = [[int(v) for v in hist[c, 0]] for c in (0, 1)]                            # exact: Python integers
        T0i, T1i = sum(ints[0]), sum(ints[1])
        assert T0i + T1i < 2 ** 63
        Li = np.zeros((2, nA, 257), np.uint64)
        Li[:, :, 1:] = np.cumsum(hist, axis=2, dtype=np.uint64)
        assert int(Li[0, 0, 256]) == T0i and int(Li[1, 0, 256]) == T1i
        if d.exact_sums:
            assert np.array_equal(Li.astype(np.float64).astype(np.uint64), Li)           # every partial sum is a float64
        L = Li.astype(np.float64) * SCALE
        t0, t1 = float(T0i) * SCALE, float(T1i) * SCALE
        M = _metric_extended(L[0], L[1], t0, t1)
        xmin, xmax = xs.min(axis=1), xs.max(axis=1)
        t = np.arange(257)[None, :]
        cand = (t >= xmin[:, None]) & (t <= xmax[:, None] + 1)
        if not EXTENDED:
            M = np.array([[float("nan") if mpmath.isnan(v) else v for v in row] for row in M], object)
        table = np.where(cand, M, NO_CANDIDATE)
        out.append(dict(T0i=T0i, T1i=T1i, t0=t0, t1=t1, table=table, cand=cand, samples=S))
    return out


_TABLES = {}


def exact_tables(d):
    """Per open slot: T0i, T1i (the integer class sums), t0, t1 (float(int) * 2^-62), table [n_allowed][257] (the metric in
    extended precision; NO_CANDIDATE outside xmin .. xmax + 1), cand, samples."""
    if d.name not in _TABLES:
        _TABLES[d.name] = _tables(d)
    return _TABLES[d.name]


def first_argmax(table):
    """(entry of A, t, value): the first largest per row, then the first largest row; a NaN is the largest value."""
    if table.dtype == object:
        def better(a, b):
            return (a != a and b == b) or (a == a and b == b and a > b)
        best = None
        for k in range(table.shape[0]):
            row = None
            for t in range(table.shape[1]):
                if row is None or better(table[k, t], table[k, row]):
                    row = t
            if best is None or better(table[k, row], table[best[0], best[1]]):
                best = (k, row)
        return best[0], best[1], table[best]
    t = np.argmax(table, axis=1)
    m = table[np.arange(table.shape[0]), t]
    k = int(np.argmax(m))
    return k, int(t[k]), m[k]


def yardstick_table(d, s):
    """tests/fit_reference.py's float64 table of open slot s."""
    w = d.q.astype(np.float64) * SCALE
    return fr.metric_table(d.xt.T, d.cls, w, d.samples(s), d.A)


def runner_up_margin(table):
    """The best value minus the largest strictly smaller candidate (inf when every candidate ties; NaN tables: NaN)."""
    v = table[table != NO_CANDIDATE]
    if any(x != x for x in v):
        return np.nan
    best = v.max()
    rest = v[v < best]
    return float(best - rest.max()) if rest.size else np.inf


def table_deviation(d):
    """The largest |float64 yardstick - extended reference| over the finite entries of a design's tables."""
    dev = 0.0
    for s, ex in enumerate(exact_tables(d)):
        Y = yardstick_table(d, s)
        E = ex["table"]
        assert np.array_equal(Y == NO_CANDIDATE, E == NO_CANDIDATE)
        fin = np.array([[v == v and v != NO_CANDIDATE for v in row] for row in E]) if E.dtype == object else np.isfinite(E)
        assert np.array_equal(np.isfinite(Y), fin)
        if fin.any():
            dev = max(dev, float(max(abs(y - e) for y, e in zip(Y[fin], E[fin]))))
    return dev


@functools.lru_cache(maxsize=None)
def yardstick_deviation():
    """d: the largest |float64 yardstick - extended reference| over all finite table entries of the exact-sum designs (1-6).
    Computed from the two references alone; the GPU test's metric tolerance is 16 * d."""
    return max(table_deviation(design(name)) for name in CASES if design(name).exact_sums)
