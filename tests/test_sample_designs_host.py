"""tests/sample_designs.py proven without a GPU: the restated kernels equal the oracle on every design, the designs hold the
edges they claim, and every wrong kernel is separated from the oracle by the designs it is named for, with the exact counts
(sample_designs.RECORDED)."""
import functools

import numpy as np
import pytest

import sample_designs as sd
from oracle import wb_oracle as orc

DTYPES = (np.uint8, np.float32)


# ------------------------------------------------------------------------------ crops
def test_crop_cells_take_the_path_they_are_listed_with():
    for name, dtype, C, x_off, out_off, unit in sd.CROP_CELLS:
        assert sd.crop_path(C, np.dtype(dtype).itemsize, x_off, out_off) == unit, name
        assert sd.crop_path(C, np.dtype(dtype).itemsize) >= unit
    # every listed combination of the issue: three vector cells, six word cells, four byte cells, five fall-backs
    units = [c[5] for c in sd.CROP_CELLS if not (c[3] or c[4]) and c[0] != "u8x43"]
    assert (units.count(16), units.count(4), units.count(1)) == (3, 6, 4) and len(sd.FALLBACK_CELLS) == 5
    assert [sd.CROP_CELL[c][5] for c in sd.FALLBACK_CELLS] == [4, 4, 1, 1, 4]


def test_crop_shapes_cover_the_loop_trip_counts():
    """In cells where a pixel is one element: 1, 63, 64, 65 and 130 elements per crop; 129 in the cell made for it."""
    for cell in ("f32x4", "u8x4", "u8x1", "f32x1"):
        _, dtype, C, _, _, unit = sd.CROP_CELL[cell]
        assert C * np.dtype(dtype).itemsize == unit
    assert [m * n for m, n in sd.CROP_SHAPES[:5]] == [1, 63, 64, 65, 130]
    assert sd.crop_shapes("u8x43") == ((1, 3),) and 1 * 3 * 43 == 129
    assert (1, sd.IMG_W) in sd.CROP_SHAPES and (sd.IMG_H, 1) in sd.CROP_SHAPES and (sd.IMG_H, sd.IMG_W) in sd.CROP_SHAPES
    for m, n in sd.CROP_SHAPES:
        rs, cs = sd.crop_origins(m, n, 300)
        pos = list(zip(rs.tolist(), cs.tolist()))
        assert rs.size == 300 and pos[0] == (sd.IMG_H - m, sd.IMG_W - n) and set(pos[:4]) == {(0, 0), (0, sd.IMG_W - n), (sd.IMG_H - m, 0), pos[0]}
        if (sd.IMG_H - m + 1) * (sd.IMG_W - n + 1) > 1:
            assert len(set(pos)) < 300 and pos != sorted(pos)                       # repeated, unsorted
        assert rs.min() >= 0 and cs.min() >= 0 and rs.max() + m <= sd.IMG_H and cs.max() + n <= sd.IMG_W
        one = sd.crop_origins(m, n, 1)
        assert (int(one[0][0]), int(one[1][0])) == pos[0]


def test_position_codes_tell_any_two_neighbouring_elements_apart():
    f = sd.crop_image(np.float32, 8)
    assert np.array_equal(f.reshape(-1), np.arange(f.size)) and f.reshape(-1)[-1] == f.size - 1 < 1 << 24
    b = sd.crop_image(np.uint8, 5).astype(np.int64)
    for axis in range(3):
        assert (np.diff(b, axis=axis) != 0).all()


@functools.lru_cache(None)
def crop_reference(cell, m, n, N):
    _, dtype, C, _, _, _ = sd.CROP_CELL[cell]
    rs, cs = sd.crop_origins(m, n, N)
    return orc.gather_samples(sd.crop_image(dtype, C), rs, cs, (m, n, C)).view(np.uint8).reshape(-1)


def _crop(cell, m, n, N, wrong=None):
    _, dtype, C, _, _, unit = sd.CROP_CELL[cell]
    rs, cs = sd.crop_origins(m, n, N)
    return sd.crop_kernel(sd.crop_image(dtype, C), rs, cs, m, n, unit, wrong)


@pytest.mark.parametrize("cell", [c[0] for c in sd.CROP_CELLS])
def test_crop_restatement_is_the_oracle(cell):
    for m, n in sd.crop_shapes(cell):
        for N in (1, 300):
            out, front, behind = _crop(cell, m, n, N)
            assert np.array_equal(out, crop_reference(cell, m, n, N)), (cell, m, n, N)
            assert (front == sd.CANARY).all() and (behind == sd.CANARY).all()


def crop_named(wrong, cell, m, n):
    """Is (cell, shape) at N = 300 a design the wrong crop kernel is named for."""
    _, dtype, C, _, _, unit = sd.CROP_CELL[cell]
    px = C * np.dtype(dtype).itemsize
    if wrong == "pitch_n":
        return n < sd.IMG_W
    if wrong == "rows_cols_swapped":
        return (m, n) != (sd.IMG_H, sd.IMG_W)
    if wrong == "cs_unscaled":
        return px // unit > 1 and n < sd.IMG_W
    if wrong == "tail_dropped":
        return (m * n * px // unit) % 64 != 0
    assert wrong == "stride_16"
    return (m * n * px) % 16 != 0


@pytest.mark.parametrize("wrong", sd.WRONG_CROP)
def test_wrong_crop_kernels_are_separated(wrong):
    total = cases = 0
    for cell in (c[0] for c in sd.CROP_CELLS):
        for m, n in sd.crop_shapes(cell):
            out, front, behind = _crop(cell, m, n, 300, wrong)
            ref = crop_reference(cell, m, n, 300)
            bad = int((out != ref).sum()) + int((front != sd.CANARY).sum()) + int((behind != sd.CANARY).sum())
            if crop_named(wrong, cell, m, n):
                assert bad >= 1, (wrong, cell, m, n)
                total += bad
                cases += 1
            else:
                assert bad == 0, (wrong, cell, m, n)          # (the claim is sharp: elsewhere such a kernel IS right)
    print(f"crop/{wrong}: {total} bytes over {cases} designs")
    assert cases >= 10 and sd.RECORDED[f"crop/{wrong}"] == total
    if wrong == "stride_16":                                                    # ... and it writes behind `out`
        assert (_crop("u8x3", 7, 9, 300, wrong)[2] != sd.CANARY).any()


# ------------------------------------------------------------------------------ trees and walks
def test_tree_shapes_are_what_they_are_called():
    w = (5, 4, 3)
    t = {s: sd.noise_tree(s, w, 3) for s in sd.TREE_SHAPES}
    assert t["leaf"]["left"].tolist() == [-1] and sd.tree_depth(t["leaf"]) == 0
    for s in ("right_chain", "left_chain"):
        assert t[s]["left"].size == 127 and (t[s]["left"] >= 0).sum() == 63 and sd.tree_depth(t[s]) == 63
        assert max(t[s]["left"].max(), t[s]["right"].max()) == 126
    assert t["right_chain"]["right"][124] == 126 and t["left_chain"]["left"][124] == 126
    assert np.array_equal(t["right_chain"]["left"], t["left_chain"]["right"])
    assert sd.tree_depth(t["bfs"]) == sd.tree_depth(t["preorder"]) == 2
    # the same tree in two numberings: equal predictions up to the renaming of the leaves
    X = sd.noise_image(200, 20, 3, np.float32, 1).reshape(200, 5, 4, 3)
    a, b = orc.tree_apply(t["bfs"], X), orc.tree_apply(t["preorder"], X)
    assert np.array_equal(np.array(sd.BFS_TO_PREORDER)[a], b) and np.unique(a).size == 4
    u = t["unbalanced"]
    assert u["left"][u["left"][0]] == -1 and sd.tree_depth(u) == 6
    for s in sd.TREE_SHAPES:                      # parent < child: what wb_model_create asks of both numberings
        k = t[s]["left"].size
        for i in np.flatnonzero(t[s]["left"] >= 0):
            assert i < t[s]["left"][i] < k and i < t[s]["right"][i] < k
        if s != "leaf":
            assert tuple(t[s]["feature"][0]) == (4, 3, 2)


def test_big_features_have_bit_7_set_and_fit_their_windows():
    for cell, feats in sd.BIG_FEATURES.items():
        window = sd.WALK_CELL[cell][2]
        assert max(max(f) for f in feats) >= 128 and max(window) <= 256
        for f in feats:
            assert all(a < b for a, b in zip(f, window))
        d = sd.walk_design(cell, "bfs", np.float32)
        assert [tuple(x) for x in d["tree"]["feature"][:3]] == list(feats)
    assert max(max(c[1]) for c in sd.WALK_CELLS if c[1][2] == 1) <= 140 and max(c[3] for c in sd.WALK_CELLS) <= 513
    assert sorted({c[3] for c in sd.WALK_CELLS}) == sorted(sd.COUNTS)


WALK_CASES = [(c[0], s, dt) for c in sd.WALK_CELLS for s in sd.TREE_SHAPES for dt in DTYPES]


@functools.lru_cache(None)
def walk_reference(cell, shape, dtype):
    d = sd.walk_design(cell, shape, dtype)
    return orc.tree_apply(d["tree"], sd.samples(d)), orc.tree_predict_on_image(d["tree"], d["image"], d["rs"], d["cs"])


@pytest.mark.parametrize("cell", [c[0] for c in sd.WALK_CELLS])
def test_walk_restatement_is_the_oracle(cell):
    for shape in sd.TREE_SHAPES:
        for dtype in DTYPES:
            d = sd.walk_design(cell, shape, dtype)
            leaf, pred = walk_reference(cell, shape, dtype)
            assert np.array_equal(sd.tree_apply_kernel(d["tree"], sd.samples(d)), leaf), (cell, shape)
            assert sd.same_floats(sd.tree_eval_kernel(d["tree"], d["image"], d["rs"], d["cs"]), pred), (cell, shape)
            assert np.array_equal(d["tree"]["prediction"][leaf], pred)              # a prediction names its leaf
            u, v, _ = d["image"].shape
            m, n, _ = d["window"]
            assert (int(d["rs"][0]), int(d["cs"][0])) == (u - m, v - n)             # the window that ends on the last element
    # chains: some window leaves at the last leaf, some before the eighth step
    for shape in ("right_chain", "left_chain"):
        if sd.WALK_CELL[cell][3] >= 255:
            leaf = walk_reference(cell, shape, np.float32)[0]
            assert (leaf == 126).any() and (leaf < 14).any(), (cell, shape)


def tie_cases():
    """(dtype, window, threshold) of every tie launch."""
    out = [(np.float32, w, t) for w in sd.TIE_WINDOWS for t in sd.tie_thresholds()]
    return out + [(np.uint8, w, t) for w in sd.TIE_WINDOWS for t in sd.U8_THRESHOLDS]


def test_tie_thresholds_hold_every_value_and_its_neighbours():
    t = sd.tie_thresholds()
    bits = set(t.view(np.uint32).tolist())
    for v in sd.TIE_VALUES[~np.isnan(sd.TIE_VALUES)]:
        for x in (v, sd._up(v), sd._down(v)):
            assert int(np.float32(x).view(np.uint32)) in bits
    assert {0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7f800000, 0xff800000} <= bits and np.isnan(t).sum() == 1
    assert sd.U8_THRESHOLDS.view(np.uint32)[0] == 0x80000001 and sd.U8_THRESHOLDS.view(np.uint32)[1] == 0x80000000


def test_tie_restatement_is_the_oracle_and_the_rules_hold():
    for dtype, w, t in tie_cases():
        X, tree = sd.tie_samples(dtype, w), sd.tie_tree(w, t)
        leaf = orc.tree_apply(tree, X)
        assert np.array_equal(sd.tree_apply_kernel(tree, X), leaf)
        img, rs, cs = sd.as_image(X)
        assert sd.same_floats(sd.tree_eval_kernel(tree, img, rs, cs), orc.tree_predict_on_image(tree, img, rs, cs))
        if np.isnan(t):
            assert (leaf == 2).all()                                        # a NaN threshold sends everything right
        elif dtype == np.float32:
            assert leaf[np.isnan(sd.TIE_VALUES)].tolist() == [2]            # a NaN pixel goes right
    # +-0 are one value, +-1e-40 are not 0
    X = sd.tie_samples(np.float32, (2, 3, 1))
    for t in (0.0, -0.0):
        leaf = orc.tree_apply(sd.tie_tree((2, 3, 1), t), X)
        assert leaf[[3, 4, 5, 6]].tolist() == [1, 1, 2, 1]


def _walk_count(wrong, cases, ties=False, eval_only=False):
    """Windows the wrong walk gets wrong, summed over the named (cell, shape, dtype); every one must show it."""
    total = 0
    for cell, shape, dtype in cases:
        d = sd.walk_design(cell, shape, dtype)
        leaf, pred = walk_reference(cell, shape, dtype)
        if eval_only:
            bad = int((sd.tree_eval_kernel(d["tree"], d["image"], d["rs"], d["cs"], d["window"], wrong).view(np.uint32) != pred.view(np.uint32)).sum())
        else:
            bad = int((sd.tree_apply_kernel(d["tree"], sd.samples(d), wrong) != leaf).sum())
            bad_eval = int((sd.tree_eval_kernel(d["tree"], d["image"], d["rs"], d["cs"], d["window"], wrong).view(np.uint32) != pred.view(np.uint32)).sum())
            if wrong in SAME_READS:
                assert bad_eval == bad, (wrong, cell, shape)                # both kernels share the walk
            else:
                assert bad_eval >= 1 or wrong == "child_unsigned", (wrong, cell, shape)     # (prediction[255 % 1] is the leaf's)
        assert bad >= 1, (wrong, cell, shape, dtype)
        total += bad
    if ties:
        for dtype, w, t in tie_cases():
            X, tree = sd.tie_samples(dtype, w), sd.tie_tree(w, t)
            total += int((sd.tree_apply_kernel(tree, X, wrong) != orc.tree_apply(tree, X)).sum())
    return total


# wrong walks that read the pixels the right one reads
SAME_READS = ("lt_for_le", "nan_goes_left", "flushing_compare", "children_swapped", "cap_3_steps", "cap_7_steps")
FULL = [c for c in WALK_CASES if sd.WALK_CELL[c[0]][3] >= 255]
SPLIT = [c for c in FULL if c[1] != "leaf"]
WALK_NAMED = {
    "lt_for_le": dict(cases=[c for c in SPLIT if c[0] in ("c1", "c3", "c4")], ties=True),
    "nan_goes_left": dict(cases=[], ties=True),
    "flushing_compare": dict(cases=[], ties=True),
    "children_swapped": dict(cases=SPLIT),
    "cap_3_steps": dict(cases=[c for c in FULL if c[1] in ("right_chain", "left_chain", "unbalanced")]),
    "cap_7_steps": dict(cases=[c for c in FULL if c[1] in ("right_chain", "left_chain")]),
    "child_unsigned": dict(cases=FULL),
    "feature_mask_127": dict(cases=[c for c in SPLIT if c[0] in sd.BIG_FEATURES]),
    "feature_row_col_swapped": dict(cases=[c for c in SPLIT if c[0] != "chan200"]),
    "window_pitch_for_image": dict(cases=[c for c in SPLIT if c[0] != "chan200"], eval_only=True),
}


@pytest.mark.parametrize("wrong", sd.WRONG_WALK)
def test_wrong_walks_are_separated(wrong):
    total = _walk_count(wrong, **WALK_NAMED[wrong])
    print(f"walk/{wrong}: {total} windows")
    assert total >= 1 and sd.RECORDED[f"walk/{wrong}"] == total


def test_what_the_tie_designs_alone_separate():
    """Per wrong compare, the tie launches (float32 / uint8) it gets wrong: `<` on every attained threshold, NaN-left on
    the NaN pixel and the NaN threshold, the flushing compare on +-1e-40 against +-0, on +-1e-45 as a threshold, and on
    uint8 0 against -1e-45."""
    def launches(wrong, dtype):
        return sum(bool((sd.tree_apply_kernel(sd.tie_tree(w, t), sd.tie_samples(dt, w), wrong) != orc.tree_apply(sd.tie_tree(w, t), sd.tie_samples(dt, w))).any())
                   for dt, w, t in tie_cases() if dt == dtype and w == sd.TIE_WINDOWS[0])
    got = {w: (launches(w, np.float32), launches(w, np.uint8)) for w in ("lt_for_le", "nan_goes_left", "flushing_compare")}
    print("tie launches separated:", got)
    assert got == sd.RECORDED["tie_launches"]
    assert min(min(v) for k, v in got.items() if k != "nan_goes_left") >= 1 and got["nan_goes_left"][0] >= 2
    # capped walks are right where the finding says
    for cell, shape, dtype in FULL:
        d = sd.walk_design(cell, shape, dtype)
        if sd.tree_depth(d["tree"]) <= 7:
            assert np.array_equal(sd.tree_apply_kernel(d["tree"], sd.samples(d), "cap_7_steps"), walk_reference(cell, shape, dtype)[0])
        if sd.tree_depth(d["tree"]) <= 3:
            assert np.array_equal(sd.tree_apply_kernel(d["tree"], sd.samples(d), "cap_3_steps"), walk_reference(cell, shape, dtype)[0])


# ------------------------------------------------------------------------------ cascades on samples
MODEL_CASES = [(d, c[0]) for d in sd.SCORE_DESIGNS for c in sd.MODEL_CELLS]


@functools.lru_cache(None)
def predict_reference(design, cell):
    d = sd.score_design(design, cell)
    with np.errstate(invalid="ignore", over="ignore"):
        return orc.model_predict(d["window"], d["trees"], list(d["thetas"]), d["X"])


@pytest.mark.parametrize("design", sd.SCORE_DESIGNS)
def test_predict_restatement_is_the_oracle(design):
    for c in sd.MODEL_CELLS:
        d = sd.score_design(design, c[0])
        H, mask = predict_reference(design, c[0])
        gH, gm = sd.predict_kernel(d["window"], d["trees"], d["thetas"], d["X"])
        assert sd.same_floats(gH, H) and np.array_equal(gm.astype(bool), mask), (design, c[0])
        assert (H[~mask] == -np.inf).all() and len(d["trees"]) <= 12 and d["X"].shape[0] in (sd.COUNTS if design != "ties" else (4, 12))
        assert d["X"].dtype == c[2] and max(d["X"].shape) <= 513


def test_score_designs_do_what_they_are_called():
    cell = "w231/f32"
    def paths(design, other=None):
        at = other or next(c[0] for c in sd.MODEL_CELLS if sd.model_count(design, c[0]) > 1)
        d = sd.score_design(design, at)
        H, mask = predict_reference(design, at)
        b = d["X"][:, 0, 0, 0] == 1
        assert b.any() and (~b).any()
        assert np.unique(H[b].view(np.uint32)).size == 1 and np.unique(H[~b].view(np.uint32)).size == 1
        return (H[~b][0], bool(mask[~b][0])), (H[b][0], bool(mask[b][0]))
    assert paths("ge_exact") == ((2.25, True), (-np.inf, False))
    assert paths("ulp_above") == ((-np.inf, False), (1.25, True)) and paths("ulp_below") == ((1.0, True), (-np.inf, False))
    assert paths("absorb") == ((-np.inf, False), (-np.inf, False)) and paths("absorb_kept") == ((1.25, True), (1.0, True))
    assert paths("inf_leaves") == ((np.inf, True), (-np.inf, False))
    a, b = paths("nan_free")
    assert np.isnan(a[0]) and a[1] and b == (2.25, True)
    for design in ("nan_finite_theta", "nan_nan_theta"):
        a, b = paths(design)
        assert a == (-np.inf, False) and b == ((2.25, True) if design == "nan_finite_theta" else (-np.inf, False))
    assert paths("theta_inf") == ((-np.inf, False), (np.inf, True))
    H, mask = predict_reference("empty", cell)
    assert (H == 0).all() and mask.all()
    # the `shapes` cascades: T = 12 with every tree shape, thetas that samples tie with, both outcomes
    for c in sd.MODEL_CELLS:
        d = sd.score_design("shapes", c[0])
        assert len(d["trees"]) == 12 and d["generic"] and max(sd.tree_depth(t) for t in d["trees"]) == 63
        s = sd.score_design("shapes_shallow", c[0])
        assert max(sd.tree_depth(t) for t in s["trees"]) == 2 and s["generic"] == (c[1][2] == 200)
    H, mask = predict_reference("shapes", "w543/f32")
    assert 0 < mask.sum() < mask.size
    assert not sd.REFUSED


PREDICT_NAMED = {"gt_for_ge": ("ge_exact", "shapes", "shapes_shallow", "theta_inf"), "neg_inf_theta_compared": ("nan_free",),
                 "fp64_sum": ("absorb", "absorb_kept"),
                 "rejected_keeps_sum": ("ge_exact", "ulp_above", "ulp_below", "absorb", "nan_finite_theta", "nan_nan_theta", "theta_inf")}


@pytest.mark.parametrize("wrong", sd.WRONG_PREDICT)
def test_wrong_predict_kernels_are_separated(wrong):
    total = 0
    for design in sd.SCORE_DESIGNS:
        for c in sd.MODEL_CELLS:
            d = sd.score_design(design, c[0])
            H, mask = predict_reference(design, c[0])
            gH, gm = sd.predict_kernel(d["window"], d["trees"], d["thetas"], d["X"], wrong)
            nan = np.isnan(gH) & np.isnan(H)
            bad = int(((~nan & (gH.view(np.uint32) != H.view(np.uint32))) | (gm.astype(bool) != mask)).sum())
            if design in PREDICT_NAMED[wrong]:
                assert bad >= 1 or d["X"].shape[0] == 1, (wrong, design, c[0])       # (one sample is one path)
                total += bad
    print(f"predict/{wrong}: {total} samples")
    assert sd.RECORDED[f"predict/{wrong}"] == total
