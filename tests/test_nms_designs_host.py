"""The designs of nms_designs.py, proved on the host (no GPU): the flags each construction predicts are nms_keep's; every
removed box has exactly one kept suppressor and every chain's S a removed overlapper, read off the IoU matrix of its cell; the
planted edges hit the scan and spread coordinates they claim (an assertion over the union of the designs); the rounding pairs
are re-derived in exact rational arithmetic; and each emulated wrong kernel differs from the expectation on a design named
here.  Parametrised over the lists tests/test_gpu_nms_designs.py runs."""
from fractions import Fraction

import numpy as np
import pytest

import nms_designs as nd
from nms_reference import nms_keep
from waldboost_amd.boxes import Boxes, iou

PLANTED, ORDERS, ROUNDING = nd.planted(), nd.orders(), nd.rounding_cases()
FINISH = [g["design"] for _, images in nd.finish_batches() for g in images if g["design"] is not None and g["done"]]
name = lambda d: d.name


def reference_flags(d):
    """nms_keep on the call's arrays; on the by_key form on the arrays in key order (nms_keep's input order is the key order)."""
    with np.errstate(all="ignore"):
        if d.forms == ("ordered",):
            return nd.keep_by_order(d)
        if d.forms == ("by_key",):
            at = np.lexsort((np.arange(d.n), d.keys))
            out = np.empty(d.n, np.int8)
            out[at] = nms_keep(d.boxes[at], d.scores[at], d.iou_t, None, d.score_t)
            return out
        return nms_keep(d.boxes, d.scores, d.iou_t, d.group, d.score_t).astype(np.int8)


def cells_of(d):
    """input indices by cell, after proving from the coordinates that every box lies inside its cell: boxes of different
    cells share no point, so their IoU is exactly 0."""
    b = d.boxes.astype(np.float64)
    assert np.isfinite(b).all() and (b == np.round(b)).all() and (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    cx, cy = np.floor(b[:, 0] / nd.CELL), np.floor(b[:, 1] / nd.CELL)
    assert (b[:, 2] < (cx + 1) * nd.CELL).all() and (b[:, 3] < (cy + 1) * nd.CELL).all() and (b >= 0).all()
    key = (cy * (1 << 20) + cx).astype(np.int64)
    at = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[at])) + 1
    return np.split(at, cuts)


def check_cell_by_cell(d):
    pos = d.position_of()
    under = np.zeros(d.n, bool) if d.score_t is None else ~(d.scores >= np.float32(d.score_t))
    n_multi = 0
    for idx in cells_of(d):
        if len(idx) == 1:
            assert d.want[idx[0]] == (0 if under[idx[0]] else 1), (d.name, idx)
            continue
        n_multi += 1
        idx = idx[np.argsort(pos[idx])]                        # (the cell's boxes in visiting order)
        sub = nd.Design(d.name, d.boxes[idx], d.scores[idx], np.arange(len(idx)), d.want[idx], d.iou_t,
                        None if d.group is None else d.group[idx], d.score_t, forms=("ordered",))
        assert np.array_equal(nd.keep_by_order(sub), d.want[idx]), (d.name, idx, pos[idx])
        # one kept suppressor per removed box, from the cell's whole IoU matrix
        m = iou(Boxes(d.boxes[idx]), Boxes(d.boxes[idx])) > d.iou_t
        if d.group is not None:
            m &= d.group[idx][:, None] == d.group[idx][None, :]
        for j in range(len(idx)):
            if d.want[idx[j]] == 0 and not under[idx[j]]:
                by = [i for i in range(j) if m[i, j] and d.want[idx[i]] == 1]
                assert len(by) == 1, (d.name, "position", pos[idx[j]], "suppressors", pos[idx[by]])
    return n_multi


@pytest.mark.parametrize("d", PLANTED + FINISH, ids=name)
def test_planted_flags_follow_from_the_construction(d):
    n_multi = check_cell_by_cell(d)
    if d.n <= 1100:                                            # (the whole call at once as well)
        assert np.array_equal(reference_flags(d), d.want), nd.describe_mismatch(d, reference_flags(d))
    pos = d.position_of()
    at = np.empty(d.n, np.int64)
    at[pos] = np.arange(d.n)                                   # position -> input index
    t = d.iou_t
    one = lambda a, b: iou(Boxes(d.boxes[at[a]][None]), Boxes(d.boxes[at[b]][None]))[0, 0]
    for kind, label, k, r in d.edges:
        assert k < r and one(k, r) > t, label
        if kind == "suppress":
            assert d.want[at[k]] == 1 and d.want[at[r]] == 0, label
        else:                                                  # a removed box overlaps S from the front and must not count
            assert d.want[at[k]] == 0, label
    roles = d.stats["roles"]
    assert d.stats["kept"] == d.n_keep >= 1 and len(roles) == d.n
    assert d.stats["removed"] == roles.count("R") and d.stats["chain_s"] == roles.count("S")
    if d.n > 1:
        assert d.stats["removed"] >= 1 and n_multi >= 1 and len(d.edges) >= 1
    if any(e[0] == "nospread" for e in d.edges):
        assert d.stats["chain_s"] >= 1
    # the input order is a permutation that is not the visiting order, and the scores say the visiting order
    if d.n > 2:
        assert sorted(d.order.tolist()) == list(range(d.n)) and not np.array_equal(d.order, np.arange(d.n))
    if d.forms != ("ordered",) and d.forms != ("by_key",):
        assert np.array_equal(np.argsort(-(d.scores + np.float32(0)), kind="stable"), d.order)
    if d.forms == ("by_key",):
        assert len(set(d.scores.tolist())) == 1 and np.array_equal(np.lexsort((np.arange(d.n), d.keys)), d.order)


def test_planted_designs_hold_what_they_are_named_for():
    by = {d.name: d for d in PLANTED}
    assert by["bands-rows64-n385"].R == 64 and by["bands-rows192-n831"].R == 192 and by["big-a-n8300"].R == 4096
    n64, W, fixed = nd.layout(1000)
    assert (n64, W, fixed) == (1024, 16, (25 * 1024 + 16 * 16 + 16 + 255) // 256 * 256)       # (test_gpu_nms.py's own figures)
    g = by["groups-n200"]
    assert set(np.unique(g.group).tolist()) == {nd.I32_MIN, -1, 0, nd.I32_MAX}
    assert not np.array_equal(nms_keep(g.boxes, g.scores, g.iou_t), g.want == 1)              # (the groups matter)
    for kind, z in (("negzero", 0.0), ("poszero", -0.0)):
        d = by[f"score-threshold-{kind}-n130"]
        at = np.flatnonzero(d.scores == 0)
        assert at.size == 1 and np.signbit(d.scores[at[0]]) == np.signbit(np.float32(z)) and np.signbit(d.score_t) != np.signbit(np.float32(z))
        assert d.want[at[0]] == 1
    d = by["score-threshold-equal-n130"]
    assert d.want[d.scores == np.float32(d.score_t)].tolist() == [1]
    d = by["score-threshold-ordered-n130"]
    under = d.scores < np.float32(d.score_t)
    assert under[d.order[[4, 64, 100]]].all() and d.want[d.order[[9, 66, 75]]].tolist() == [1, 1, 0]
    assert nd.BIG_N > 8256 and (nd.BIG_N + 63) // 64 - 64 > 64                                  # (a full band, more than 64 words behind)


def test_the_claimed_coordinates_are_the_coordinates_hit():
    got, req = nd.coverage(), nd.required_coverage()
    assert not req - got, sorted(req - got, key=str)
    # the same from the classifier's raw output, for the two cases a reader is most likely to doubt
    d = nd.by_name("scan-ordinal5-n256")
    c = nd.classify(d, next(e for e in d.edges if "kept row 5" in e[1]))
    assert (c["where"], c["chunk"], c["ordinal"], c["row_bit"], c["u"], c["round"], c["word"]) == ("scan", 1, 5, 7, 0, 1, 2)
    d = nd.by_name("big-a-n8300")
    c = nd.classify(d, next(e for e in d.edges if e[2] == 63 * 64 + 7 and e[3] == 8298))
    assert (c["where"], c["band"], c["chunk"], c["block_y"], c["wave"], c["block_x"], c["lane"]) == ("spread", 0, 63, 15, 3, 1, 1)


# ------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("d", PLANTED + ORDERS + FINISH, ids=name)
def test_the_emulated_kernels_give_the_expected_flags(d):
    for form in d.forms:
        if form == "surface" or (form == "ordered" and d.n > 2000):
            continue
        keep, count = nd.emulate(d, (), form)
        assert np.array_equal(keep, d.want), (form, nd.describe_mismatch(d, keep))
        assert count == d.n_keep


def test_the_emulated_kernels_on_the_rounding_cases():
    for d in ROUNDING:
        keep, count = nd.emulate(d)
        assert np.array_equal(keep, d.want) and count == d.n_keep, nd.describe_mismatch(d, keep)


# fault -> the design (and form) on which the emulated wrong kernel differs from the expectation
EXPOSED_ON = {
    "or_removed_rows": ("diag-n385", "rank"),
    "first_round_only": ("scan-ordinal5-n256", "rank"),
    "last_lane_stale": ("scan-lastword-n255", "rank"),
    "no_carry": ("bands-rows64-n385", "rank"),
    "spread_first_block": ("big-a-n8300", "rank"),
    "spread_chunks_lt4": ("big-a-n8300", "rank"),
    "low_half": ("diag-n385", "rank"),
    "padding_alive": ("scan-lastword-n193", "rank"),
    "ge": ("rounding-01-fused-t=u", "rank"),
    "ties_desc_index": ("order-equal-n257-parity0", "rank"),
    "negzero_first": ("order-zero-ladder-n72-parity1", "rank"),
    "index_before_key": ("order-keys-random-n300-parity0", "by_key"),
    "score_gt": ("score-threshold-equal-n130", "rank"),
    "no_groups": ("groups-n200", "rank"),
}
IOU_FAULTS = {"iou_fused": "fused", "iou_f32": "f32", "iou_recip": "recip", "iou_multiply": "multiply", "iou_trunc": "trunc"}


def differs(d, fault, form=None, scratch=None):
    keep, count = nd.emulate(d, (fault,), form, scratch)
    return not np.array_equal(keep, d.want) or count != d.n_keep


@pytest.mark.parametrize("fault", [f for f in nd.FAULTS if f != "no_first_reset"])
def test_each_emulated_wrong_kernel_differs_on_a_named_design(fault):
    if fault in IOU_FAULTS:
        # every case that targets the form: the wrong form decides the other way there
        cases = [d for d in ROUNDING if d.target == IOU_FAULTS[fault]]
        assert len(cases) >= nd.ROUNDING_PER_FORM
        assert all(differs(d, fault) for d in cases), [d.name for d in cases if not differs(d, fault)]
        return
    design, form = EXPOSED_ON[fault]
    d = next(x for x in PLANTED + ORDERS + ROUNDING if x.name == design)
    assert differs(d, fault, form)
    keep, _ = nd.emulate(d, (fault,), form)
    print(nd.describe_mismatch(d, keep))
    if fault == "padding_alive":                               # (the flags are right: only the count tells)
        assert np.array_equal(keep, d.want)
    if fault == "first_round_only":                            # the fifth kept row only: ordinals 1 .. 4 do not notice
        assert not any(differs(nd.by_name(f"scan-ordinal{k}-n256"), fault) for k in (1, 2, 3, 4))
        assert differs(nd.by_name("scan-ordinal8-n256"), fault)
    wrong_at = sorted(d.position_of()[np.flatnonzero(keep != d.want)].tolist())
    if fault == "spread_first_block":                          # every target in words 128 and 129 that no wrongly kept twin removes
        assert wrong_at == [8192, 8200, 8250, 8298]
    if fault == "spread_chunks_lt4":                           # the targets of chunks 4 and 63
        assert wrong_at == [4100, 6000, 8298]


def stale_sequence():
    return [nd.by_name("big-a-n8300"), nd.by_name("sprinkle-n65-scores"), nd.by_name("sprinkle-n1-scores"), nd.sprinkle(0, 1)]


def test_stale_scratch_in_the_emulation():
    """What the `first` branch is for: removed[] and cnt[0] of the last call, or 0xFF bytes, must not reach the next."""
    seq = stale_sequence()
    for fill in (0, 1):
        scratch = nd.fresh_scratch(fill=fill)
        for d in seq + seq[1:2] * 2:
            keep, count = nd.emulate(d, (), "rank", scratch)
            assert np.array_equal(keep, d.want) and count == d.n_keep, (fill, d.name)
    # without the reset: the second of two runs counts on from the first, the empty call reports the last call's count,
    # and on 0xFF bytes nothing is kept
    d = nd.by_name("sprinkle-n65-scores")
    scratch = nd.fresh_scratch()
    assert not differs(d, "no_first_reset", "rank", scratch) and differs(d, "no_first_reset", "rank", scratch)
    assert nd.emulate(nd.sprinkle(0, 1), ("no_first_reset",), "rank", scratch)[1] != 0
    keep, _ = nd.emulate(d, ("no_first_reset",), "rank", nd.fresh_scratch(fill=1))
    assert not keep.any()
    b = nd.by_name("bands-rows64-n385")
    assert differs(b, "no_first_reset", "rank", nd.fresh_scratch(fill=1)) and not differs(b, "no_first_reset", "rank", nd.fresh_scratch())


def test_rank_by_counting_is_the_stable_sort():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 700):
        s = (np.round(rng.normal(0, 1, n) * 2) / 2).astype(np.float32)
        p = nd.rank_by_counting(nd.score_word(s), np.arange(n, dtype=np.uint64))
        order = np.empty(n, np.int64)
        order[p] = np.arange(n)
        assert np.array_equal(order, np.argsort(-(s + np.float32(0)), kind="stable"))
    w = nd.score_word(np.array([np.inf, 3e38, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -3e38, -np.inf], np.float32))
    assert w[4] == w[5] and (np.diff(np.delete(w.astype(np.int64), 5)) > 0).all()


# ------------------------------------------------------------------------------ B. one rounding from the threshold
def rounded(x):
    return float(x)                                            # (Fraction -> double: int / int true division, correctly rounded)


def contract_iou_exactly(a, b):
    """The header's sequence with every operation done exactly and rounded once."""
    F = lambda v: Fraction(float(v))
    op = lambda x: F(rounded(x))
    iw = op(max(min(F(a[2]), F(b[2])) - max(F(a[0]), F(b[0])), 0))
    ih = op(max(min(F(a[3]), F(b[3])) - max(F(a[1]), F(b[1])), 0))
    inter = op(iw * ih)
    area_a = op(op(F(a[2]) - F(a[0])) * op(F(a[3]) - F(a[1])))
    area_b = op(op(F(b[2]) - F(b[0])) * op(F(b[3]) - F(b[1])))
    uni = op(op(area_a + area_b) - inter)
    return rounded(inter / uni), inter, uni, op(area_a + area_b), iw, ih


def test_the_stored_rounding_pairs_are_what_the_search_finds():
    found = nd.search_rounding_pairs()
    assert len(found) == len(nd.ROUNDING_BITS) == nd.ROUNDING_PER_FORM * len(nd.ROUNDING_FORMS)
    for (form, a, b), (form2, bits) in zip(found, nd.ROUNDING_BITS):
        assert form == form2 and np.concatenate([a, b]).view(np.uint32).tolist() == bits
    for form in nd.ROUNDING_FORMS:
        assert sum(f == form for f, _ in nd.ROUNDING_BITS) >= 8


def test_rounding_pairs_in_exact_arithmetic():
    seen = set()
    for form, a, b, fm, t in nd.rounding_pairs():
        u, inter, uni, s, iw, ih = contract_iou_exactly(a, b)
        assert u == fm["u"] == iou(Boxes(a[None]), Boxes(b[None]))[0, 0] and 0 < u < 1
        assert float(inter) == fm["inter"] and float(uni) == fm["uni"]
        assert 20 <= min(a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]) and max(a[2] - a[0], b[3] - b[1]) <= 221
        # the wrong forms, from the same exact ingredients
        assert fm["fused"] == float(np.float64(float(inter)) / np.float64(rounded(s - iw * ih)))
        exact = inter / uni
        assert fm["trunc"] == (u if Fraction(u) <= exact else float(np.nextafter(u, 0.0))) and Fraction(fm["trunc"]) <= exact
        assert fm["recip"] == rounded(inter * Fraction(rounded(1 / uni)))
        assert t is not None and t >= 0
        if form == "multiply":
            assert (fm["inter"] > t * fm["uni"]) != (u > t)
        else:
            assert fm[form] != u and t == min(u, fm[form]) and (fm[form] > t) != (u > t)
        seen.add(form)
    assert seen == set(nd.ROUNDING_FORMS)


@pytest.mark.parametrize("d", ROUNDING, ids=name)
def test_rounding_cases_against_the_yardstick(d):
    assert np.array_equal(reference_flags(d), d.want)
    u = d.forms_of_pair["u"]
    (kind, label, pa, pb), = d.edges
    assert d.want[d.order[pb]] == (0 if u > d.iou_t else 1) and d.n_keep == d.n - int(u > d.iou_t)
    assert d.iou_t in (u, float(np.nextafter(u, 0.0))) or d.target is not None
    # the pair is the only overlap of the call
    m = iou(Boxes(d.boxes), Boxes(d.boxes))
    np.fill_diagonal(m, 0)
    assert int((m > 0).sum()) == 2
    if d.target is not None and d.target != "multiply":
        assert d.forms_of_pair[d.target] != u                  # not vacuous: the targeted form gives another double


def test_rounding_cases_meet_the_matrix_kernel_in_different_places():
    places = {(d.edges[0][2] // 64 == d.edges[0][3] // 64, d.edges[0][2] % 64, d.edges[0][3] % 64) for d in ROUNDING}
    assert {p[0] for p in places} == {True, False} and len({p[1] for p in places}) >= 8 and len({p[2] for p in places}) >= 8
    assert {d.iou_t == d.forms_of_pair["u"] for d in ROUNDING} == {True, False}
    assert len(ROUNDING) <= 130 and all(d.n == nd.ROUNDING_N for d in ROUNDING)


@pytest.mark.parametrize("t", nd.ODD_THRESHOLDS)
def test_non_ordinary_boxes_in_the_emulation(t):
    """Inverted, empty, infinite, NaN, denormal and huge boxes: the kernel's ternaries and NumPy's minimum / clip agree on
    every one of them (a NaN or an inf - inf anywhere reaches the union, which then fails `union > 0`)."""
    boxes, scores = nd.odd_boxes()
    with np.errstate(all="ignore"):
        want = nms_keep(boxes, scores, t)
    d = nd.Design(f"odd-{t}", boxes, scores, np.argsort(-scores, kind="stable"), want.astype(np.int8), t, forms=("rank",))
    keep, count = nd.emulate(d)
    assert np.array_equal(keep, d.want) and count == int(want.sum())
    assert np.isnan(boxes).any() and np.isinf(boxes).any() and (boxes[:, 2] < boxes[:, 0]).any()
    with np.errstate(all="ignore"):
        assert ((boxes[:, 2] - boxes[:, 0] > 0) & (boxes[:, 2] - boxes[:, 0] < 1e-38)).any() and (np.abs(boxes) > 2.9e38).any()
    assert 0 < want.sum() < len(want)                          # something is removed, something is kept


# ------------------------------------------------------------------------------ C. the visiting order
@pytest.mark.parametrize("d", ORDERS, ids=name)
def test_adjacent_rank_pairs_against_the_yardstick(d):
    ref = reference_flags(d)
    assert np.array_equal(ref, d.want), nd.describe_mismatch(d, ref)
    check_cell_by_cell(nd.Design(d.name, d.boxes[d.want >= 0], d.scores[d.want >= 0], np.argsort(d.position_of()[d.want >= 0]),
                                 d.want[d.want >= 0], d.iou_t, forms=("ordered",)))
    assert len(d.edges) >= (d.n - 12) // 2


def test_any_swap_of_neighbours_in_the_order_flips_a_flag():
    for even, odd in zip(ORDERS[::2], ORDERS[1::2]):
        assert even.name[:-1] == odd.name[:-1] and np.array_equal(even.order, odd.order)
        valid = even.order < even.n
        pairs = {e[2] for e in even.edges} | {e[2] for e in odd.edges}
        assert pairs == {p for p in range(even.n - 1) if valid[p] and valid[p + 1]}
        for d in (even, odd):                                  # a swap at an edge's ranks exchanges a 1 and a 0
            for _, _, p, q in d.edges[:: max(len(d.edges) // 5, 1)]:
                swapped = d.order.copy()
                swapped[[p, q]] = swapped[[q, p]]
                s = nd.Design(d.name, d.boxes, d.scores, swapped, d.want, d.iou_t, forms=("ordered",))
                assert int((nd.keep_by_order(s) != d.want).sum()) == 2
    by = {d.name: d for d in ORDERS}
    d = by["order-callers-permutation-n200-parity0"]
    assert sorted(d.order.tolist()) == list(range(200)) and not np.array_equal(d.order, np.argsort(-d.scores, kind="stable"))
    d = by["order-callers-entries-beyond-n-n200-parity0"]
    assert int((d.order >= 200).sum()) == 5 and int((d.want == nd.UNTOUCHED).sum()) >= 4
    d = by["order-keys-equal-block-n300-parity0"]
    assert len(np.unique(d.keys)) == 300 - 40
    for n in (255, 256, 257, 513):
        assert np.array_equal(by[f"order-equal-n{n}-parity0"].order, np.arange(n))
    z = by["order-zero-ladder-n72-parity0"].scores
    assert int((z == 0).sum()) == 18 and int(np.signbit(z[z == 0]).sum()) == 9 and int((np.abs(z[z != 0]) < 1e-44).sum()) == 54


# ------------------------------------------------------------------------------ D. finish batches
def test_finish_batches_hold_the_sizes_and_forms_asked_for():
    seen = set()
    for cap, images in nd.finish_batches():
        fin, want = nd.finish_arrays(cap, images)
        assert fin.size == len(images) * (16 + 28 * cap) and want.shape == (len(images), 16 + cap)
        sizes = [g["total"] for g in images]
        assert {g["by_key"] for g in images if g["done"] and g["total"] > 1} == {True, False}
        assert any(a >= min(cap, 4096) and b == 0 and c >= min(cap, 4096) for a, b, c in zip(sizes, sizes[1:], sizes[2:]))
        for b, g in enumerate(images):
            seen.add((cap, g["total"], g["done"]))
            hdr = fin[b * (16 + 28 * cap):][:16].view(np.int32)
            assert hdr[0] == g["total"] and hdr[3] == (0 if g["by_key"] else 1)
            assert g["done"] == (g["total"] <= cap and g["total"] <= nd.FINISH_MAX)
            info = want[b, :16].view(np.uint32).tolist()
            if g["done"]:
                assert info == [g["design"].n_keep if g["design"] else 0, g["total"], 1, 0] and (want[b, 16 + g["total"]:] == 0x5A).all()
            else:
                assert info == [0, 0, 0, 0] and (want[b, 16:] == 0x5A).all()
    assert {(64, 0, True), (64, 1, True), (64, 64, True), (64, 65, False), (4096, 64, True), (4096, 65, True), (4096, 4096, True),
            (4096, 4097, False), (8192, 4096, True), (8192, 4097, False), (8192, 5000, False)} <= seen


def test_mismatch_message_names_the_design_and_the_edge():
    d = nd.by_name("bands-rows192-n831")
    got = d.want.copy()
    got[d.order[609]] = 1
    msg = nd.describe_mismatch(d, got)
    assert "bands-rows192-n831: 1 flags differ" in msg and "position 609" in msg and "band 0 -> band 3: K@3 -> R@609" in msg
    assert "'where': 'spread'" in msg and "'target_band': 3" in msg
