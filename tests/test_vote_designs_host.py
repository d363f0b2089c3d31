"""CPU proofs about the designed box sets of tests/vote_designs.py: the planted voter sets and keep flags from exact
arithmetic, the statement (tests/vote_reference.py) on every design, the order design's separation of the summation orders,
and that each emulated wrong kernel differs from the statement on some design."""
from fractions import Fraction

import numpy as np
import pytest

import vote_designs as vd
import vote_reference as vr
from nms_reference import nms_keep

name = lambda d: d.name
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def statement(d):
    return vr.vote(d.boxes, d.scores, d.keep, **d.args())


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def fraction_iou(a, b):
    """IoU of two boxes of integer coordinates as a rational."""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return Fraction(inter, union) if union > 0 else Fraction(0)


@pytest.mark.parametrize("d", vd.planted(), ids=name)
def test_planted_voter_sets_and_keep_flags_follow_from_exact_arithmetic(d):
    c = d.boxes.astype(np.int64)
    assert np.array_equal(c, d.boxes) and np.array_equal(d.scores, np.round(d.scores))          # integers all of them
    live = np.ones(d.n, bool) if d.score_t is None else d.scores >= d.score_t
    kept = np.flatnonzero(d.keep)
    assert sorted(d.planted) == kept.tolist()
    t = Fraction(d.vote_iou)
    assert t > 0
    for k in kept:
        # boxes that do not intersect box k have IoU 0 < vote_iou; the others are decided as rationals
        touch = (np.minimum(c[:, 2], c[k, 2]) > np.maximum(c[:, 0], c[k, 0])) & (np.minimum(c[:, 3], c[k, 3]) > np.maximum(c[:, 1], c[k, 1]))
        mine = {int(k)}
        for j in np.flatnonzero(touch):
            if live[j] and (d.group is None or d.group[j] == d.group[k]) and fraction_iou(c[j].tolist(), c[k].tolist()) >= t:
                mine.add(int(j))
        assert sorted(mine) == d.planted[int(k)], (d.name, int(k))
    assert np.array_equal(nms_keep(d.boxes, d.scores, d.nms_t, d.group, d.score_t), d.keep.astype(bool))
    assert same(statement(d), d.want)
    assert (d.want[1][kept] >= 1).all() and (d.want[1][d.keep == 0] == 0).all()
    assert np.array_equal(bits(d.want[0][d.keep == 0]), bits(d.boxes[d.keep == 0]))


def test_the_designs_cover_the_sizes_and_cases():
    ds = vd.all_designs()
    sizes = {d.n for d in ds}
    assert set(vd.SIZES) | {vd.BIG_N} <= sizes and vd.CHUNK == 256
    assert all(d.n_keep >= 300 for d in ds if d.n == vd.BIG_N)
    for d in vd.planted():
        if d.n >= 3 and d.name.startswith("sprinkle"):                         # voters at the first and the last candidate
            assert any(js[0] == 0 and js[-1] == d.n - 1 and k not in (0, d.n - 1) for k, js in d.planted.items()), d.name
    by = {d.name: d for d in ds}
    z = by["zero-area-n67"]
    assert (z.boxes[3] == z.boxes[66]).all() and z.boxes[3, 0] == z.boxes[3, 2] and z.want[1][3] == z.want[1][66] == 1
    a = by["all-at-threshold-n130"]
    assert a.want[1][4] == 4 and np.array_equal(a.want[0][4], a.boxes[4]) and (a.scores[[4, 70, 129, 64]] == a.score_t).all()
    g = by["coinciding-groups-n70"]
    assert (g.boxes[7] == g.boxes[69]).all() and g.group[7] != g.group[69] and g.want[1][5] == 4 and g.want[1][7] == 4
    assert any(d.weights == "uniform" and d.score_t is not None and d.planted for d in ds)     # a not-live box under uniform weights


@pytest.mark.parametrize("d", vd.edge_designs(), ids=name)
def test_edge_designs_say_what_they_mean(d):
    m, v = statement(d)
    for k, count in d.expect_votes.items():
        assert d.keep[k] and v[k] == count, (d.name, k, v[k])
    assert same(vd.emulate(d), (m, v))
    if d.name.startswith("negative-zero"):
        assert np.signbit(d.scores[0]) and d.scores[0] == 0 and not d.keep[0]
        moved = not np.array_equal(m[3], d.boxes[3])
        assert moved == (d.weights == "uniform")                               # weight 0 under "score": counted, without pull


def test_a_voter_at_the_threshold_and_one_a_rounding_below():
    by = {d.name: d for d in vd.edge_designs()}
    pairs = [(by[n], by[n.replace("-at", "-a-rounding-above")]) for n in by if n.endswith("-at")]
    assert len(pairs) >= 6
    for at, above in pairs:
        assert above.vote_iou == np.nextafter(at.vote_iou, 1.0) and np.array_equal(at.boxes, above.boxes)
        (k, c_at), (_, c_above) = next(iter(at.expect_votes.items())), next(iter(above.expect_votes.items()))
        assert (c_at, c_above) == (2, 1) and statement(at)[1][k] == 2 and statement(above)[1][k] == 1


def test_the_order_design_separates_the_orders():
    d = vd.order_design()
    ok, right, wrong = vd.separates(d)
    print("prescribed", right, {k: v for k, v in wrong.items()})
    assert ok and vd.search_order_seed() == vd.ORDER_SEED
    assert np.array_equal(bits(statement(d)[0][d.kept_box]), bits(right))
    assert statement(d)[1][d.kept_box] == 1 + 2 * vd.ORDER_PAIRS
    # the straight reading of the rule, one kept box, Python floats
    k = d.kept_box
    _, v = vr.voters(d.boxes, d.scores, np.arange(d.n) == k, d.vote_iou, d.score_t, d.group)
    w = d.scores.astype(np.float64) - np.float64(np.float32(d.score_t))
    p = [[0.0] * 5 for _ in range(64)]
    for l in range(64):
        for j in range(l, d.n, 64):
            if v[0, j]:
                p[l][0] = p[l][0] + float(w[j])
                for i in range(4):
                    p[l][1 + i] = p[l][1 + i] + float(w[j]) * float(d.boxes[j, i])
    for s in (1, 2, 4, 8, 16, 32):
        p = [[p[l][i] + p[l ^ s][i] for i in range(5)] for l in range(64)]
    assert np.array_equal(bits(np.array([p[0][1 + i] / p[0][0] for i in range(4)]).astype(np.float32)), bits(right))


def test_the_emulation_is_the_statement_on_every_design():
    for d in vd.all_designs():
        assert same(vd.emulate(d), statement(d)), d.name


@pytest.mark.parametrize("fault", vd.FAULTS)
def test_every_wrong_kernel_differs_from_the_statement_on_some_design(fault):
    assert len(vd.FAULTS) >= 10
    for d in sorted(vd.all_designs(), key=lambda d: d.n):
        if d.n > 700 or (fault in vd.SLOW_FAULTS and d.n > 400):
            continue
        if not same(vd.emulate(d, (fault,)), statement(d)):
            print(f"{fault}: caught by {d.name}")
            return
    raise AssertionError(f"no design tells a kernel with the fault {fault!r} from the statement")
