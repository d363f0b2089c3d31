"""The designs of tests/calib_designs.py, proved on the host: what they plant holds in exact rational arithmetic, and each
of ten wrong kernels, emulated in NumPy, differs from the statement (tests/calib_reference.py) on at least one design."""
from fractions import Fraction

import numpy as np
import pytest

import calib_designs as cd
import calib_reference as ref

DESIGNS = cd.designs()


def exact_rows(d):
    """Per distinct row of leaves: the exact prefix sums of the planted increments (Fractions), and the rows' owners."""
    rows, inverse = np.unique(d.leaf, axis=0, return_inverse=True)
    sums = []
    for row in rows:
        acc, out = Fraction(0), []
        for t, leaf in enumerate(row):
            acc += Fraction(float(d.values64[t, leaf]))
            out.append(acc)
        sums.append(out)
    return sums, inverse.reshape(-1)


_statement = {}


def statement(d):
    if d.name not in _statement:
        _statement[d.name] = ref.trace(d.trees, d.X)
    return _statement[d.name]


@pytest.mark.parametrize("name", list(DESIGNS))
def test_every_planted_value_is_a_float32_and_the_walk_finds_it(name):
    d = DESIGNS[name]
    for v in d.values64.reshape(-1):
        assert Fraction(float(v)) == Fraction(float(np.float32(v))), (name, v)
    for th in d.thetas:
        assert th == float("-inf") or Fraction(th) == Fraction(float(np.float32(th))), (name, th)
    # the statement's own walk on (trees, X) lands in the planted leaves: its trace is the fp32 sum, in stage order, of the
    # planted increments
    tr = statement(d)
    h = np.zeros(d.N, np.float32)
    for t in range(d.T):
        h = h + d.increments[:, t]
        assert np.array_equal(h.view(np.uint32), tr[:, t].view(np.uint32)), (name, t)


@pytest.mark.parametrize("name", [n for n, d in DESIGNS.items() if d.exact])
def test_exact_designs_never_round(name):
    d = DESIGNS[name]
    tr = statement(d)
    sums, row_of = exact_rows(d)
    first = {r: int(np.flatnonzero(row_of == r)[0]) for r in range(len(sums))}
    for r, i in first.items():
        assert [Fraction(float(x)) for x in tr[i]] == sums[r], (name, i)
    assert all(np.array_equal(tr[row_of == r], np.broadcast_to(tr[first[r]], tr[row_of == r].shape)) for r in first)


@pytest.mark.parametrize("name", [n for n, d in DESIGNS.items() if d.owners])
def test_every_planted_owner_is_the_unique_minimum(name):
    d = DESIGNS[name]
    sums, row_of = exact_rows(d)
    for recall, owner in d.owners.items():
        retained = ref.prune(statement(d), recall)["retained"]
        assert retained.all()                                              # (the owner designs keep everybody)
        counts = np.bincount(row_of, minlength=len(sums))
        for t in range(d.T):
            low = min(s[t] for s in sums)
            rows = [r for r, s in enumerate(sums) if s[t] == low]
            assert len(rows) == 1 and counts[rows[0]] == 1 and row_of[owner[t]] == rows[0], (name, t)
            assert low < 0                                                 # negative minima: a signed compare of the bits errs
    own = next(iter(d.owners.values()))
    assert d.N == 1 or d.T == 1 or (own[1:] != own[:-1]).all()            # neighbouring stages: different owners
    if d.N > 1 and d.T >= 4:
        assert d.N - 1 in own                                              # the last sample (last lane of a partial wave)
    if d.N > cd.WG and d.T >= 6:
        assert (d.N - 1) // cd.WG * cd.WG in own                           # the first lane of the last workgroup


def test_the_order_design_shows_order_and_precision():
    d = DESIGNS["order-65x6"]
    inc = [float(x) for x in d.increments[0]]
    assert sum(Fraction(x) for x in inc) == 2
    fwd = np.float32(0)
    for x in inc:
        fwd = np.float32(fwd + np.float32(x))
    rev = np.float32(0)
    for x in inc[::-1]:
        rev = np.float32(rev + np.float32(x))
    assert (float(fwd), float(rev), float(np.float32(np.sum(np.array(inc, np.float64))))) == (0.0, 1.0, 2.0)
    assert float(statement(d)[0, -1]) == 0.0


def test_the_ties_design_keeps_whole_groups():
    d = DESIGNS["ties-257x4"]
    tr = statement(d)
    assert set(d.recalls) == set(cd.TIES_KEEP)
    for recall, (keep, retained) in cd.TIES_KEEP.items():
        p = ref.prune(tr, recall)
        assert (p["keep"], int(p["retained"].sum())) == (keep, retained), recall
    assert ref.keep_count(0.249, 257) + 1 == ref.keep_count(0.25, 257)     # either side of a ceil step
    assert any(r > k for k, r in cd.TIES_KEEP.values())                    # retained exceeds keep


def test_the_reject_designs_meet_theta_exactly_and_one_ulp_below():
    for name in ("reject-130x5-uint8", "reject-130x5-float32"):
        d = DESIGNS[name]
        tr = statement(d)
        th = np.array(d.thetas, np.float32)
        assert (tr[:, 0] == th[0]).any() and (tr[:, 4] == th[4]).any()                       # h == theta: passes
        assert (tr[:, 2] == np.nextafter(th[2], np.float32(-np.inf))).any()                  # one ulp below: rejected
        assert np.isneginf(th[1]) and np.isneginf(th[3])                                     # -inf between finite ones
        rt, alive = ref.trace_rejecting(d.trees, d.thetas, d.X)
        assert alive[1] == d.N and alive[3] == 64 and alive[5] == 48
        assert np.array_equal(np.isneginf(rt[:, 0]), np.zeros(d.N, bool))
        at = np.flatnonzero(tr[:, 2] == np.nextafter(th[2], np.float32(-np.inf)))
        assert np.isneginf(rt[at, 2:]).all() and not np.isneginf(rt[at, :2]).any()


# ---- wrong kernels: name -> f(design, recall) -> what the kernel would hand back, comparable with right()
def right(d, recall):
    tr = statement(d)
    rt, alive = ref.trace_rejecting(d.trees, d.thetas, d.X)
    return dict(trace=tr, rtrace=rt, alive=alive, theta=ref.prune(tr, recall)["theta"])


def theta_of(tr, retained):
    if not retained.any():
        return np.full(tr.shape[1], np.inf, np.float32)
    return tr[retained].min(axis=0).astype(np.float32)


def wrong_float64(d, recall):
    tr = np.cumsum(d.increments.astype(np.float64), axis=1).astype(np.float32)
    return dict(trace=tr, theta=ref.prune(tr, recall)["theta"])


def wrong_reversed(d, recall):
    tr = np.zeros((d.N, d.T), np.float32)
    h = np.zeros(d.N, np.float32)
    for t in range(d.T - 1, -1, -1):
        h = h + d.increments[:, t]
        tr[:, t] = h
    return dict(trace=tr)


def wrong_all_samples(d, recall):
    return dict(theta=statement(d).min(axis=0))


def wrong_strict_floor(d, recall):
    tr = statement(d)
    return dict(theta=theta_of(tr, tr[:, -1] > ref.prune(tr, recall)["floor"]))


def wrong_exactly_keep(d, recall):
    tr = statement(d)
    kept = np.zeros(d.N, bool)
    kept[np.argsort(-tr[:, -1], kind="stable")[:ref.keep_count(recall, d.N)]] = True
    return dict(theta=theta_of(tr, kept))


def wrong_thetas_in_trace(d, recall):
    tr = ref.trace_rejecting(d.trees, d.thetas, d.X)[0]
    return dict(trace=tr, theta=ref.prune(tr, recall)["theta"])


def wrong_shifted(d, recall):
    th = ref.prune(statement(d), recall)["theta"]
    return dict(theta=np.concatenate([th[:1], th[:-1]]))


def wrong_partial_wave(d, recall):
    tr = statement(d)
    full = d.N // cd.WAVE * cd.WAVE
    p = ref.prune(tr, recall)
    kept = p["retained"].copy()
    kept[full:] = False
    return dict(theta=theta_of(tr, kept), trace=np.concatenate([tr[:full], np.zeros_like(tr[full:])]))


def wrong_signed_compare(d, recall):
    tr = statement(d)
    kept = ref.prune(tr, recall)["retained"]
    bits = tr[kept].view(np.int32)
    return dict(theta=bits.min(axis=0).astype(np.int32).view(np.float32))


def wrong_strict_reject(d, recall):
    out = np.full((d.N, d.T), -np.inf, np.float32)
    alive = np.zeros(d.T + 1, np.int64)
    tr = statement(d)                                   # (rejection changes no running score, it ends it)
    mask = np.ones(d.N, bool)
    for t, theta in enumerate(d.thetas):
        alive[t] = mask.sum()
        if theta != -np.inf:
            mask &= tr[:, t] > np.float32(theta)
        out[mask, t] = tr[mask, t]
    alive[d.T] = mask.sum()
    return dict(rtrace=out, alive=alive)


WRONG = {
    "float64 accumulation rounded at the end": wrong_float64,
    "reversed stage order": wrong_reversed,
    "minimum over all samples": wrong_all_samples,
    "> instead of >= at the floor": wrong_strict_floor,
    "exactly keep samples retained, ties ignored": wrong_exactly_keep,
    "thetas applied during the unrejected trace": wrong_thetas_in_trace,
    "theta[t] taken from stage t - 1": wrong_shifted,
    "the last partial wave dropped": wrong_partial_wave,
    "minimum by signed compare of the float bits": wrong_signed_compare,
    "rejection with >": wrong_strict_reject,
}


def same(a, b):
    """Equal by value (0.0 == -0.0, inf == inf)."""
    return a.shape == b.shape and bool(np.all(a == b))


@pytest.mark.parametrize("kind", list(WRONG))
def test_a_wrong_kernel_differs_from_the_statement_on_some_design(kind):
    caught = []
    for name, d in DESIGNS.items():
        for recall in d.recalls:
            want, got = right(d, recall), WRONG[kind](d, recall)
            if any(not same(np.asarray(v), np.asarray(want[k])) for k, v in got.items()):
                caught.append((name, recall))
    assert caught, kind
    # the emulation is of a WRONG kernel: the right one, through the same comparison, differs nowhere
    for name, d in DESIGNS.items():
        w = right(d, d.recalls[0])
        assert all(same(v, right(d, d.recalls[0])[k]) for k, v in w.items())
