"""The designed survivor maps (tests/survivor_maps.py) on the CPU: for every parametrisation test_gpu_survivor_maps.py
uses, the closed form equals oracle.cascade_predict_on_image (alive, rows, columns, score bits), and every tile reaches
the regime it is named for -- asserted from its death stages D alone.  This is what keeps the GPU module from passing
vacuously."""
import numpy as np
import pytest

import survivor_maps as sm
from oracle import wb_oracle as orc

OPS = {"==": lambda a, b: a == b, ">": lambda a, b: a > b, "<=": lambda a, b: a <= b}
CASES = sm.scan_cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_specialised_cases_are_scan_cases():
    assert all(c in CASES for c in sm.specialised_cases()) and len(set(CASES)) == len(CASES)
    assert {c[3] for c in CASES if c[0] == (12, 12, 4) and c[4] == 2} == set(sm.LENGTHS)
    assert {c[1] for c in CASES} == {32, 16, 8, 4} and {c[4] for c in CASES} == {1, 2, 3, 4}


@pytest.mark.parametrize("case", CASES, ids=sm.case_id)
def test_closed_form_equals_the_oracle_on_the_composed_map(case):
    casc, tiles, per_row, D, X = sm.build_case(case)
    shape, trees, thetas = casc.oracle()
    alive, rs, cs = sm.closed_form(D, casc.T, casc.free)
    r, c, h, a = orc.cascade_predict_on_image(shape, trees, thetas, X)
    assert np.array_equal(a, alive)
    assert np.array_equal(r, rs) and np.array_equal(c, cs)
    assert np.array_equal(bits(sm.survivor_scores(casc, X, rs, cs)), bits(h))
    # the same decisions from float32 pixels, and the bait is in place: every pixel that is no window's origin never dies
    r, c, h2, a = orc.cascade_predict_on_image(shape, trees, thetas, X.astype(np.float32))
    assert np.array_equal(a, alive) and np.array_equal(r, rs) and np.array_equal(bits(h2), bits(h))
    assert (X[D.shape[0]:, :, 0] == sm.NEVER).all() and (X[:, D.shape[1]:, 0] == sm.NEVER).all()
    # the tree arrays are what the kernels accept: parent < child, the model's depth is the case's
    depth = 0
    for feature, threshold, left, right, prediction in casc.stages:
        inner = np.flatnonzero(left >= 0)
        assert (left[inner] > inner).all() and (right[inner] > inner).all() and tuple(feature[0]) == (0, 0, 0)
        assert (feature[inner[1:], 2] >= 1).all()
        d = lambda n: 0 if left[n] < 0 else 1 + max(d(int(left[n])), d(int(right[n])))
        depth = max(depth, d(0))
    assert depth == case[4]


@pytest.mark.parametrize("case", CASES, ids=sm.case_id)
def test_every_tile_reaches_the_regime_it_is_named_for(case):
    shape, TR, waves, T, depth, free = case
    casc, tiles, per_row, D, X = sm.build_case(case)
    cap, full = sm.queue_cap(TR, waves), TR * sm.TILE_COLS
    names = [t.name for t in tiles]
    assert len(set(names)) == len(names)
    n_claims = 0
    for t in tiles:
        assert t.D.shape == (TR, sm.TILE_COLS) and t.D.dtype == np.uint8
        for stage, op, n in t.claims:
            got = sm.entering(t.D, T, casc.free, stage)
            assert OPS[op](got, n), (t.name, stage, op, n, got)
            n_claims += 1
    assert n_claims >= len(tiles)
    # the sweep behind phase A meets every count it names, in every placement
    if T > sm.PHASE_A:
        by_n = {}
        for t in tiles:
            if t.name.startswith("count["):
                by_n.setdefault(sm.entering(t.D, T, casc.free, sm.PHASE_A), set()).add(t.name.split(",")[1])
        want = {0, 1, 2, 3, sm.SPAR[3], sm.SPAR[1], sm.SPAR_WG - 1, sm.SPAR_WG, sm.SPAR_WG + 1, 63, 64, 65, cap - 1, cap, full - 1, full}
        want |= {cap + 1} if cap < full else set()
        want |= {cap - sm.TILE_COLS * waves + k for k in (-1, 0, 1) if cap - sm.TILE_COLS * waves + k >= 0}
        assert want <= set(by_n), sorted(want - set(by_n))
        assert all(by_n[n] == set(sm.PLACEMENTS) for n in want)
        # placements are what they say: a lone survivor in lane 0 / lane 63, in the first / last row
        one = {t.name.split(",")[1]: np.argwhere(sm.eff_stage(t.D, T, casc.free) >= sm.PHASE_A)[0] for t in tiles
               if t.name.startswith("count[N=1,")}
        assert one["lane0"][1] == 0 and one["lane63"][1] == 63 and one["first_rows"][0] == 0 and one["last_rows"][0] == TR - 1
        assert tuple(one["last_rows"]) == (TR - 1, 63) and one["last_wave"][0] >= TR - max(TR // waves, 1)
    # tiles on the dense continuation: over the queue at stage 8 and 16, at most the queue at 24 -- and the like
    if cap < full and T > 32:
        e = {t.name: [sm.entering(t.D, T, casc.free, s) for s in (8, 16, 24, 32)] for t in tiles if t.name.startswith("staircase[")}
        for r in (16, 24, 32):
            i = (8, 16, 24, 32).index(r)
            for v in (cap + 1, cap, cap - 1):
                hit = [n for n, x in e.items() if f"r={r},v={v}," in n and all(y > cap for y in x[:i]) and x[i] == v]
                assert len(hit) == 2, (r, v, hit)
    if cap < full:
        assert sum(t.name.startswith("dense_to_the_end[") and sm.entering(t.D, T, casc.free, T) > cap for t in tiles) == 2 * len(sm.PLACEMENTS)
    if T > 16:
        seen = {sm.entering(t.D, T, casc.free, 16) for t in tiles if t.name.startswith("second_count[")}
        assert {0, 1, sm.SPAR[3], sm.SPAR[1], sm.SPAR_WG - 1, sm.SPAR_WG, sm.SPAR_WG + 1} <= seen
    # uniform death: one tile per stage, and one for never
    assert [int(t.D[0, 0]) for t in tiles[:T + 2]] == list(range(T + 1)) + [sm.NEVER]
    # the composition puts tile k where which_tile finds it, and the grid ends inside a tile on both sides
    D2, origins = sm.compose(tiles, TR, per_row, 1, 1)
    assert np.array_equal(D2, D) and D.shape[0] % TR == 1 and D.shape[1] % sm.TILE_COLS == 1
    for k in (0, len(tiles) // 2, len(tiles) - 1):
        r0, c0 = origins[k]
        assert np.array_equal(D[r0:r0 + TR, c0:c0 + sm.TILE_COLS], tiles[k].D) and sm.which_tile(r0 + TR - 1, c0 + 63, TR, per_row, tiles) == names[k]


@pytest.mark.parametrize("case", CASES, ids=sm.case_id)
def test_edge_levels_closed_form_equals_the_oracle(case):
    shape, TR, waves, T, depth, free = case
    casc = sm.designed_cascade(shape, T, depth, free)
    _, trees, thetas = casc.oracle()
    grids = sm.edge_grids(TR)
    assert grids[-sm.DENSE_EDGES:] == [(TR, 63), (TR - 1, 64)]
    assert (1, 1) in grids and (1, 200) in grids and (100, 1) in grids and (TR - 1, 64) in grids and (TR, 63) in grids
    assert any(nr % TR == 1 and nc % 64 == 1 and nr > TR for nr, nc in grids) and any(nr * nc == 0 for nr, nc in grids)
    maps = sm.edge_levels(case)
    assert len(maps) >= 2
    for b, per_level in enumerate(maps):
        for l, D in enumerate(per_level):
            assert D.shape == grids[l]
            X = sm.channel_image(D, shape, 100 * b + l)
            alive, rs, cs = sm.closed_form(D, T, casc.free)
            r, c, h, a = orc.cascade_predict_on_image(shape, trees, thetas, X)
            assert np.array_equal(a, alive) and np.array_equal(r, rs) and np.array_equal(c, cs), (b, l)
            assert np.array_equal(bits(sm.survivor_scores(casc, X, rs, cs)), bits(h))
            if l >= len(grids) - sm.DENSE_EDGES:
                # a partial tile on the dense continuation: over the queue behind phase A and at the re-count at 16, to the
                # end for kind "end"; the last valid row and column survive next to the bait
                cap, kind = sm.queue_cap(TR, waves), ("end", "drop")[(b + l) % 2]
                e = sm.eff_stage(D, T, casc.free) == T
                assert e[-1, :].all() and e[:, -1].all()
                assert (X[D.shape[0], :, 0] == sm.NEVER).all() and (X[:, D.shape[1], 0] == sm.NEVER).all()
                if D.size > cap:
                    assert cap + 1 < D.size and (T <= 8 or sm.entering(D, T, casc.free, 8) > cap)
                    assert T <= 16 or sm.entering(D, T, casc.free, 16) > cap
                    assert kind != "end" or rs.size > cap
                    assert kind != "drop" or T <= 24 or rs.size <= cap
                else:
                    assert TR < 32
            elif (b + l) % 3 == 0 and D.size:
                # survivors exactly in the last valid row and column; the bait is the pixel next to each of them
                e = sm.eff_stage(D, T, casc.free) == T
                assert e[-1, :].all() and e[:, -1].all()
                assert (X[D.shape[0], :, 0] == sm.NEVER).all() and (X[:, D.shape[1], 0] == sm.NEVER).all()
    # every image and level has a map of its own
    assert not np.array_equal(maps[0][0], maps[1][0]) and not np.array_equal(maps[0][2], maps[1][2])


@pytest.mark.parametrize("case", [c for c in CASES if c[4] <= 3][::7], ids=sm.case_id)
def test_rank_images_decide_as_the_floats_do(case):
    casc, tiles, per_row, D, X = sm.build_case(case)
    T = casc.T
    S = sm.sorted_thresholds(casc)
    assert np.array_equal(S[0], np.arange(T, dtype=np.float32)) and all(s.size <= 254 for s in S)
    for dtype in (np.uint8, np.uint16):
        R = sm.rank_image(casc, X, dtype)
        assert R.dtype == dtype and R.shape == X.shape
        assert np.array_equal(R[:D.shape[0], :D.shape[1], 0], np.minimum(D, T)) and (R[D.shape[0]:, :, 0] == T).all()
        # a node test `x <= thr` is `rank(x) <= index(thr)` for every pixel and every threshold of its channel
        for c in range(1, 4):
            for i in range(0, S[c].size, 17):
                assert np.array_equal(X[..., c] <= S[c][i], R[..., c] <= i)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_sample_cases_closed_form_equals_the_oracle(depth):
    for N in sm.SAMPLE_COUNTS:
        casc, D, X, rs, cs = sm.sample_case(depth, N)
        shape, trees, thetas = casc.oracle()
        assert rs.size == N and D.size >= N
        want = sm.eff_stage(D[rs, cs], casc.T, casc.free) == casc.T
        for dtype in (np.uint8, np.float32):
            H, mask = orc.model_predict(shape, trees, thetas, orc.gather_samples(X.astype(dtype), rs, cs, shape))
            assert np.array_equal(mask, want) and np.isneginf(H[~mask]).all()
            assert np.array_equal(bits(H[mask]), bits(sm.survivor_scores(casc, X, rs[mask], cs[mask])))
        if N >= 255:
            assert want.any() and not want.all()
