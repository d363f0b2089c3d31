"""CPU proof of the split-search designs (tests/fit_designs.py), from the two references alone -- the exact tables in
extended precision and the float64 yardstick tests/fit_reference.py -- before any kernel sees them: every design's expected
answer is the first argmax of its exact table, every claimed tie is exact on both sides, every winner leads by a margin,
and the two references agree to within d <= 1e-14 (the GPU tests' metric tolerance is 16 * d)."""
import numpy as np
import pytest

import fit_designs as fd

MARGIN = 1e-6                     # the best distinct runner-up of every rated node trails by at least this


@pytest.mark.parametrize("name", sorted(fd.CASES))
def test_design_answer_ties_and_margin(name):
    d = fd.design(name)
    assert d.n_open == len(d.want) == len(d.tie_t) == len(d.tie_A) and d.xt.dtype == np.uint8 and d.q.dtype == np.uint64
    assert sorted(s for s in d.slot.tolist() if s >= 0) == list(range(d.n_open)) and d.slot.size == d.n_level
    for s, ex in enumerate(fd.exact_tables(d)):
        k, t, best = fd.first_argmax(ex["table"])
        f_want, t_want, is_nan = d.expected(s)
        assert (int(d.A[k]), t) == (f_want, t_want), (name, s)
        assert bool(best != best) == is_nan, (name, s)
        Y = fd.yardstick_table(d, s)
        ky, ty, besty = fd.first_argmax(Y)
        assert (ky, ty) == (k, t) and bool(np.isnan(besty)) == is_nan, (name, s)          # the yardstick agrees
        if is_nan:
            assert min(ex["T0i"], ex["T1i"]) == 0 and (int(d.A[k]), k) == (int(d.A[0]), 0)
            cand = ex["table"][ex["cand"]]
            assert all(v != v for v in cand)                                             # every candidate is NaN
            assert not d.tie_t[s] and not d.tie_A[s]
            continue
        # the first and the last candidate of a row (nothing on one side) are the same number, bit for bit, on both sides:
        # t = xmax + 1 -- and with it t = 256 -- ties with the smaller xmin wherever it is a best, so it never answers
        first, last = ex["cand"].argmax(axis=1), 256 - ex["cand"][:, ::-1].argmax(axis=1)
        rows = np.arange(d.A.size)
        assert np.all(last > first) and np.all(ex["table"][rows, first] == ex["table"][rows, last])
        assert np.array_equal(Y[rows, first].view(np.uint64), Y[rows, last].view(np.uint64))
        margin = fd.runner_up_margin(ex["table"])
        print(f"{name} slot {s}: |S| {ex['samples'].size} answer ({f_want}, {t_want}) margin {margin:.3g}")
        assert margin >= MARGIN, (name, s, margin)
        tied = ex["table"] == best
        if d.tie_t[s]:
            assert tied[k].sum() >= 2, (name, s)
            assert np.unique(Y[tied].view(np.uint64)).size == 1, (name, s)               # bit-equal in float64 too
            assert np.array_equal(tied, Y == besty), (name, s)
        if d.tie_A[s]:
            assert (tied.sum(axis=1) > 0).sum() >= 2, (name, s)
        else:
            assert (tied.sum(axis=1) > 0).sum() == 1, (name, s)


def test_designs_cover_what_they_are_named_for():
    sizes = lambda d: sorted(fd.exact_tables(d)[s]["samples"].size for s in range(d.n_open))
    for n in fd.PLANTED_N:
        for tag in ("dup_first", "dup_last"):
            d = fd.design(f"planted[{n}-{tag}]")
            assert sizes(d) == [n] and d.tie_A == [True] and np.any(np.diff(d.A) < 0)
            assert (d.want[0][0] == 7) == (tag == "dup_first") and np.array_equal(d.xt[4], d.xt[7])
    d = fd.design("eight_nodes")
    assert (d.level_base, d.n_level, d.n_open) == (7, 8, 8) and d.slot.tolist() == list(fd.EIGHT_SLOTS)
    assert sizes(d) == sorted(fd.EIGHT_SIZES) and d.want.count(fd.NAN_NODE) == 1
    assert len({w for w in d.want}) == 8 and np.any(np.diff(d.node) < 0)                # eight answers, interleaved samples
    assert {w[0] >= 8 for w in d.want if w != fd.NAN_NODE} == {True, False}
    d = fd.design("leaves_between")
    assert d.slot.tolist() == list(fd.BETWEEN_SLOTS) and d.n_open == 4
    leaf = np.isin(d.node, d.level_base + np.flatnonzero(d.slot < 0))
    foreign = (d.node < d.level_base) | (d.node >= d.level_base + d.n_level)
    assert leaf.sum() >= 100 and (d.node < d.level_base).sum() >= 30 and (d.node >= d.level_base + 8).sum() >= 30
    by = leaf | foreign
    assert d.q[by].min() > d.q[~by].max() and set(np.unique(d.xt[:, by]).tolist()) == {0, 255}
    for variant in ("weightless", "no_class1"):
        d = fd.design(f"nan_beside_normal[{variant}]")
        s = d.want.index(fd.NAN_NODE)
        S = d.samples(s)
        assert (np.any(d.cls[S] == 1)) == (variant == "weightless") and not np.any(d.q[S][d.cls[S] == 1])
        col = d.xt[d.A[0], S]
        assert d.q[S][np.argmin(col)] == 0 and np.sort(col)[1] > col.min()               # a weightless sample alone fixes xmin
        assert d.expected(s)[:2] == (int(d.A[0]), 3) and d.want[1 - s] != fd.NAN_NODE
    # edge columns: the closed forms
    want = {"all_0": 0, "all_255": 255, "only_0_and_255": 1, "weightless_bounds": 0}
    for column, t in want.items():
        d = fd.design(f"edge_columns[{column}]")
        assert d.A.size == 1 and d.want[0] == (int(d.A[0]), t), column
    d = fd.design("edge_columns[zeros_in_lane_5]")
    col = d.xt[d.A[0]]
    assert np.array_equal(np.flatnonzero(col == 0) % 64, np.full((col == 0).sum(), 5)) and (col == 0).sum() >= 4
    d = fd.design("edge_columns[weightless_0_below_50]")
    col = d.xt[d.A[0]]
    assert col.min() == 0 and d.q[np.argmin(col)] == 0 and np.sort(col)[1] >= 50
    T = fd.exact_tables(d)[0]["table"][0]
    assert np.all(T[1:51] == T[1]) and d.want[0][1] > 50                                 # 1 .. 50 tie; the answer lies above
    d = fd.design("edge_columns[weightless_bounds]")
    col = d.xt[d.A[0]]
    assert set(col[d.q > 0].tolist()) == {50} and col.min() == 0 and col.max() == 255
    for which, (n_allowed, at_f, at_dup) in fd.WIDE_CASES.items():
        d = fd.design(f"wide_A[{which}]")
        assert d.A.size == n_allowed == np.unique(d.A).size and d.xt.shape == (640, 300) and d.A[at_f] == 611
        first = at_f if at_dup is None else min(at_f, at_dup)
        assert d.want[0][0] == d.A[first] and d.tie_A == [at_dup is not None]
        assert at_dup is None or d.A[at_dup] == 17
    assert max(at_f for _, at_f, _ in fd.WIDE_CASES.values()) >= 257
    d = fd.design("three_wide")
    assert (d.A.size, d.n_open) == (257, 3) and (d.n_open * d.A.size * 8) % 16 != 0
    d = fd.design("full_bits")
    assert not d.exact_sums and (d.q == 1).sum() >= 3 and (d.q == 0).sum() >= 3 and int(d.q.max()).bit_length() >= 58
    Li = np.cumsum(d.q[d.cls == 0], dtype=np.uint64)
    assert not np.array_equal(Li.astype(np.float64).astype(np.uint64), Li)               # sums that no float64 holds


def test_exact_sum_designs_are_exact_and_the_yardstick_is_within_d():
    """d, the largest |float64 yardstick - extended reference| over every finite entry of the tables of designs 1-6.  Both
    sides start from the same float64 sums there, so d is the float64 rounding of the metric's own arithmetic: a few ulp
    of values that are at most 1."""
    for name in fd.CASES:
        d = fd.design(name)
        assert d.exact_sums == (name != "full_bits")
        if d.exact_sums:
            assert not np.any(d.q & np.uint64(0xfff)) and int(d.q.sum(dtype=np.uint64)) < 2 ** 61
    dev = fd.yardstick_deviation()
    print(f"d = {dev:.3g}")
    assert 0 < dev <= 1e-14


def test_full_bits_yardstick_rounding_stays_far_below_the_margin():
    d = fd.design("full_bits")
    dev = fd.table_deviation(d)
    margin = fd.runner_up_margin(fd.exact_tables(d)[0]["table"])
    print(f"full_bits: yardstick deviation {dev:.3g}, margin {margin:.3g}")
    assert dev * 1e3 < margin
