"""CPU proofs for gradient_designs.py (no GPU): the classes derived from the integers are the oracle's, the kernel's step 2
and both forms of its smooth restated in NumPy give the oracle's bits on every design, the designs hold what they were
built to hold (with the counts found), and every wrong kernel of gd.WRONG_KERNELS differs from the oracle somewhere --
or is shown not to be wrong.  Every count asserted here is one the oracle produced on the CPU."""
import functools

import numpy as np
import pytest

import gradient_designs as gd
from oracle import wb_oracle as orc

CASES = [(d, i, s) for d, i in gd.CASES for s in gd.SHRINKS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def n_diff(a, b):
    return int((bits(a) != bits(b)).any(-1).sum())


@functools.lru_cache(None)
def facts(name, index, shrink):
    img = gd.design_images(name, shrink)[index]
    m = gd.classify(img, shrink)
    m["img"] = img
    m["ref_smooth"] = orc.smooth_image_3d(m["ref_level"])
    return m


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_restated_kernel_gives_the_oracle_bits(case):
    """Classes (inside classify), the shrunk level -- first pass, redo condition, exact redo: the absorption claim on every
    block of the design -- and the smooth: the oracle's chain on tiles whose flag is raised, the fast form on all others."""
    name, index, shrink = case
    m = facts(name, index, shrink)
    assert len(gd.identity_levels(m["img"], shrink)) >= 1
    assert np.array_equal(bits(m["level"]), bits(m["ref_level"]))
    got, rep = gd.smooth_kernel(m["level"], m["ring"], m["ref_smooth"], shrink)
    assert np.array_equal(bits(got), bits(m["ref_smooth"])), (rep["odd"], rep["n_sep"])
    # a separating tile always has its flag up, and never from the halo ring alone
    assert not (rep["separating"] & ~rep["odd"]).any() and not (rep["separating"] & ~rep["odd_inner"]).any()


def test_fast_smooth_is_held_to_the_oracle_on_tiles_with_ordinary_values():
    """The exactness claim is not vacuous: tiles whose flag stays down, full of ordinary values (the largest 504 at shrink
    1), the shrink-4 ones with ordinary values below 0.125 included."""
    n_tiles, small = 0, 0
    for name, index, shrink in CASES:
        m = facts(name, index, shrink)
        rep = gd.tile_report(m["level"], m["ring"], m["ref_smooth"], shrink)
        g = gd.tile_geom(shrink, 1)
        for ty, tx in zip(*np.nonzero(~rep["odd"])):
            t = m["level"][ty * g["TU"]:(ty + 1) * g["TU"], tx * g["TV"]:(tx + 1) * g["TV"]]
            n_tiles += int((t >= 0.7).any())
            small += int(((t > 0) & (t < gd.ODD_BELOW)).sum())
    print("tiles on the fast smooth with ordinary values:", n_tiles, "ordinary values below 0.125 among them:", small)
    assert (n_tiles, small) == FAST_TILES


FAST_TILES = (46, 12)


# ------------------------------------------------------------------------------ the designs' conditions
def word_sets(shrink=2):
    out = [set(), set(), set()]
    for i in range(len(gd.design_images("words", shrink))):
        w = facts("words", i, shrink)["words"]
        for k in (1, 2, 3):
            out[k - 1] |= set(np.unique(w[..., k]).tolist())
    return out


def test_words_reached():
    sets = word_sets()
    counts = tuple(len(s) for s in sets)
    print("distinct block words in channels 1, 2, 3:", counts)
    assert counts == gd.WORDS_REACHED and all(c >= f for c, f in zip(counts, (69, 77, 69)))
    for k in (1, 2, 3):
        names = {gd.word_name(w) for w in sets[k - 1]}
        assert sorted(set(map(gd.word_name, range(81))) - names) == sorted(gd.WORDS_MISSING[k])
        for pos in range(4):                                  # one ordinary value beside three residues, in every position
            assert "".join("O" if i == pos else "R" for i in range(4)) in names
        # every residue-only word is there but the ones no search reached (all of them mixtures of R and Z)
        residue_only = {w for w in map(gd.word_name, range(81)) if "O" not in w and "R" in w}
        assert residue_only - names == set(gd.WORDS_MISSING[k]) & residue_only
        assert all("O" not in w for w in gd.WORDS_MISSING[k])


def residue_blocks(m, k):
    """Per 2 x 2 block of level 0's pixels: residue-only in channel k, and the four values [u, v, 4] in pooling order."""
    v = m["pixels"][..., k]
    u, w = v.shape[0] // 2 * 2, v.shape[1] // 2 * 2
    four = np.stack([v[0:u:2, 0:w:2], v[1:u:2, 0:w:2], v[0:u:2, 1:w:2], v[1:u:2, 1:w:2]], -1)
    names = m["words"][..., k]
    only = np.vectorize(lambda x: "O" not in gd.word_name(x) and "R" in gd.word_name(x))(names)
    return only, four


ORDER_COUNTS = {1: (345, 0), 2: (500, 370), 3: (385, 0)}


def test_order_blocks_change_their_bits_in_another_order():
    """Channel 2: residue-only blocks whose pooled bits depend on the order.  Channels 1 and 3: blocks with two magnitudes are
    there, but none can be order-sensitive -- their residues are powers of two within eleven binades (checked here for every
    |gx| <= 1020), whose sums of four are exact in fp32 however they are associated."""
    g = np.arange(1, 1021, dtype=np.float64)
    tiny = np.unique(np.abs(g * gd.C1 - g * gd.S1))
    tiny = tiny[tiny > 0]
    assert (np.frexp(tiny)[0] == 0.5).all() and tiny.max() / tiny.min() == 2.0 ** 10
    m = facts("order", 0, 2)
    found = {}
    for k in (1, 2, 3):
        only, four = residue_blocks(m, k)
        two = only & np.array([[len(set(x[x > 0].tolist())) >= 2 for x in row] for row in four])
        a, b, c, d = (four[..., i] for i in range(4))
        kernel = ((a + b) + c) + d
        other = (bits(((d + c) + b) + a) != bits(kernel)) | (bits((a + c) + (b + d)) != bits(kernel))
        found[k] = (int(two.sum()), int((two & other).sum()))
    print("residue-only blocks with two magnitudes, of them order-sensitive, per channel:", found)
    assert found == ORDER_COUNTS and found[2][1] >= 1 and found[1][0] >= 1 and found[3][0] >= 1
    assert found[1][1] == found[3][1] == 0


ABSORB_EXTREMES = {1: (2.5579538487363607e-13, 1.4142135381698608, 4), 2: (1.8740564655672642e-13, 1.0, 4),
                   3: (3.410605131648481e-13, 1.4142135381698608, 4)}


def test_absorb_three_residues_beside_the_smallest_ordinary_value():
    """The tightest instance of the absorption claim the designs hold: per channel the 3 R + 1 O block with the largest
    sum of residues over its ordinary value -- every position of the O present -- pools to the pool of project_ordinary."""
    m = facts("absorb", 0, 2)
    ordinary = gd.project_ordinary(m["gx"], m["gy"])
    assert np.array_equal(bits(gd.pool2(ordinary)[m["redo"] == 0]), bits(m["ref_level"][m["redo"] == 0]))
    found = {}
    for k in (1, 2, 3):
        _, four = residue_blocks(m, k)
        names = np.vectorize(gd.word_name)(m["words"][..., k])
        best, positions = None, set()
        for pos in range(4):
            sel = names == "".join("O" if i == pos else "R" for i in range(4))
            if not sel.any():
                continue
            positions.add(pos)
            f = four[sel].astype(np.float64)
            o = f[:, pos]
            r = f.sum(-1) - o
            i = int(np.argmax(r / o))
            if best is None or r[i] / o[i] > best[0] / best[1]:
                best = (float(r[i]), float(o[i]))
            # the block's pooled value is the ordinary value's quarter: the residues are absorbed in every position
            assert np.array_equal(bits(m["ref_level"][..., k][sel]), bits((four[sel][:, pos] * np.float32(0.25))))
        print(f"channel {k}: largest residue sum {best[0]:.4g} beside ordinary value {best[1]:.6g}, O in positions {sorted(positions)}")
        found[k] = (best[0], best[1], len(positions))
    assert found == ABSORB_EXTREMES


ZERO_COUNTS = dict(z_pixels_redone=(3930, 1998, 1932), flat_gx_blocks=320, flat_gx_redone=0)


def test_zeros_with_a_gradient():
    m = facts("zeros", 0, 2)
    gx, gy, cl = m["gx"], m["gy"], m["cls"]
    zdiag = ((gx == gy) & (cl[..., 1] == gd.Z) | (gx == -gy) & (cl[..., 3] == gd.Z)) & (gx != 0)
    redo_px = np.kron(m["redo"].astype(np.uint8), np.ones((2, 2), np.uint8)).astype(bool)
    found = (int((zdiag & redo_px).sum()), int((zdiag & redo_px & (gx > 0)).sum()), int((zdiag & redo_px & (gx < 0)).sum()))
    flat = ~gd.block_any(gx != 0, 2) & gd.block_any(gy != 0, 2)
    print("class-Z pixels with gx == +-gy != 0 in redone blocks (all, gx > 0, gx < 0):", found, "blocks with gx == 0 and gy != 0:",
          int(flat.sum()), "redone:", int((flat & m["redo"]).sum()))
    assert found == ZERO_COUNTS["z_pixels_redone"] and min(found) > 0
    assert int(flat.sum()) == ZERO_COUNTS["flat_gx_blocks"] > 0 and int((flat & m["redo"]).sum()) == ZERO_COUNTS["flat_gx_redone"] == 0
    # the redone blocks' Z pixels come out 0: the pooled value of a block of such pixels alone is an exact 0
    allz = ~gd.block_any(~zdiag, 2)
    assert allz.any() and (m["ref_level"][allz][:, [1, 3]].min(-1) == 0).all()


def test_extremes():
    """|gx| and |gy| reach 1020; d = |gx -+ gy| is even (the stencil of gx - gy is [[0,-2,-2],[2,0,-2],[2,2,0]]) and at most
    1530, so the smallest ordinary values are 1 (channels 0, 2) and fp32(2 sin(pi/4)) (channels 1, 3): pooled 0.25 and
    0.35355, and the largest value is fp32(1530 sin(pi/4)) = 1081.87 -- not the 0.7071 / 4 and 1442.5 of d = 1 and 2040."""
    for name, index, shrink in CASES:
        m = facts(name, index, shrink)
        assert not ((m["gx"] - m["gy"]) & 1).any()
    m1, m2 = facts("extremes", 0, 1), facts("extremes", 0, 2)
    gx, gy = m2["gx"], m2["gy"]
    found = (int(np.abs(gx).max()), int(np.abs(gy).max()), int(np.abs(gx - gy).max()), int(np.abs(gx + gy).max()))
    assert found == (1020, 1020, 1530, 1530)
    assert m1["ref_level"].max() == gd.split_sin(np.array([1530]))[0] and abs(float(m1["ref_level"].max()) - 1081.8734) < 1e-3
    lv = m2["ref_level"]
    smallest = [float(lv[..., k][lv[..., k] > 1e-6].min()) for k in range(4)]
    print("smallest ordinary pooled values at shrink 2:", smallest, "largest:", float(lv.max()))
    assert smallest == [0.25, float(np.float32(2 * gd.S1) / 4), 0.25, float(np.float32(2 * gd.S1) / 4)]
    assert float(lv.max()) == 1020.0


WINDOW_COUNTS = {"wave0": 16, "wave1": 48, "wave2": 32, "wave3": 32, "all": 630, "lanes": 60, "bottom1": 42, "bottom2": 63}


def test_smooth_windows_lie_where_they_were_aimed():
    """Shrink 2, the detection cell.  wave<w>: tile (0, 0) is separating and only wave w's rows raise its flag.  all:
    separating outputs on both sides of both tile edges, in lanes 64 / 65's window (output column 63) and beside the level's
    border.  bottom2: the bottom tile's own output row.  bottom1: a bottom tile of one output row is all border (zeros) --
    its three shrunk rows (waves 1, 1, 1, 0) are computed and flagged, and nothing of it can differ."""
    g = gd.tile_geom(2, 1)
    for i, v in enumerate(gd.WINDOW_VARIANTS):
        m = facts("smooth_windows", i, 2)
        rep = gd.tile_report(m["level"], m["ring"], m["ref_smooth"], 2)
        assert int(rep["n_sep"].sum()) == WINDOW_COUNTS[v], (v, rep["n_sep"])
        if v.startswith("wave"):
            w = int(v[-1])
            only = gd.tile_report(m["level"], m["ring"], m["ref_smooth"], 2, waves=(w,))
            rest = gd.tile_report(m["level"], m["ring"], m["ref_smooth"], 2, waves=tuple(x for x in range(4) if x != w))
            assert rep["separating"][0, 0] and only["odd"][0, 0] and not rest["odd"][0, 0]
        if v == "all":
            d = rep["diff"]
            u, vv = d.shape
            assert d[g["TU"] - 1].any() and d[g["TU"]].any() and d[:, g["TV"] - 1].any() and d[:, g["TV"]].any()
            assert d[1].any() and d[u - 2].any() and d[:, 1].any() and d[:, vv - 2].any()
            assert rep["separating"].all()
        if v == "lanes":
            no_lanes = gd.tile_report(m["level"], m["ring"], m["ref_smooth"], 2, lanes=False)
            assert rep["odd"][:, 0].all() and not no_lanes["odd"][:, 0].any() and not rep["separating"][:, 0].any()
        if v == "bottom2":
            assert rep["separating"][1, 0] and m["level"].shape[0] == g["TU"] + 2
        if v == "bottom1":
            assert m["level"].shape[0] == g["TU"] + 1 and rep["odd"][1].all() and not rep["separating"][1].any()
            assert not m["ref_smooth"][g["TU"]:].any()


X_ONLY_RESIDUES = 2208
SMOOTH_FORMS = dict(x=(630, 2040, 0, 0), diag1=(0, 0), diag3=(0, 0))


def test_the_two_forms_of_the_smooth_differ_in_channel_2_alone():
    """on an image that depends on x only every pooled channel-2 value is a residue and the fast smooth (fp32 in
    channel 2) differs from the chain in 630 of 2040 interior outputs; channels 1 and 3 never differ.  On the x + y and
    x - y images every pooled value of channel 1 (3) is a residue or 0 and the fp64 separable sums differ in no output."""
    m = facts("smooth_windows", gd.WINDOW_VARIANTS.index("all"), 2)
    fast = gd.smooth_fast(m["level"])
    d = bits(fast) != bits(m["ref_smooth"])
    u, v = m["level"].shape[:2]
    found = (int(d[..., 2].sum()), (u - 2) * (v - 2), int(d[..., 1].sum()), int(d[..., 3].sum()))
    assert (m["level"][..., 2] < 1e-6).all() and int((m["level"][..., 2] > 0).sum()) == X_ONLY_RESIDUES
    print("x-only image: channel-2 outputs that differ, interior outputs, channel-1 and channel-3 outputs that differ:", found)
    assert found == SMOOTH_FORMS["x"]
    f = gd.window_image(2, "all")[0].astype(np.int64)
    y, x = np.mgrid[0:64, 0:70]
    for k, t in ((1, x + y), (3, x - y + 64)):          # (gx == gy on the x + y image: channel 1)
        img = f[t % f.size].astype(np.uint8)
        lv = gd.pool2(orc.grad_hist(img))
        inner = lv[1:-1, 1:-1, k]
        assert (inner < 1e-6).all() and (inner > 0).sum() > 100 and len(np.unique(inner)) > 3
        dd = bits(gd.smooth_fast(lv)) != bits(orc.smooth_image_3d(lv))
        # (away from the image's own border, where the reflected gradients are ordinary values)
        found = (int(dd[2:-2, 2:-2, k].sum()), int(dd[2:-2, 2:-2, 4 - k].sum()))
        assert found == SMOOTH_FORMS[f"diag{k}"]


# ------------------------------------------------------------------------------ wrong kernels
@functools.lru_cache(None)
def wrong_counts():
    """{wrong kernel: {(shrink, smooth): differing output pixels over all designs}} for the cells it applies to."""
    out = {}
    for w in gd.WRONG_KERNELS:
        out[w] = {}
        for shrink in gd.SHRINKS:
            for smooth in gd.SMOOTHS:
                if not gd.applies(w, shrink, smooth):
                    continue
                n = 0
                for name, index in gd.CASES:
                    m = facts(name, index, shrink)
                    n += n_diff(gd.emulate(m["img"], shrink, smooth, w), m["ref_smooth"] if smooth else m["ref_level"])
                out[w][(shrink, smooth)] = n
    return out


# No design exposes these, and none can:
#   redo_without_gx_term      a redo is exact wherever it runs (project_int is the oracle's projection, pixel by pixel), so a
#                             kernel that redoes MORE blocks is slower, never different
#   flag_without_lanes_64_65  an output of the tile's last column has lane 63 (a row wave's pixel) in its window; for lanes 64
#                             and 65 to hold the tile's only odd values that column must be exact zeros, and a window with two
#                             non-zero columns of an x-only region sums with ONE rounding in either form.  The `lanes` variant
#                             holds such tiles (flag raised by the stand-alone pixels alone) and none is separating; nor was
#                             one among 4000 random images of the word family.
NOT_WRONG = ("redo_without_gx_term", "flag_without_lanes_64_65")
WRONG_COUNTS = {'c2_fp32_constant': {(1, 0): 2527, (1, 1): 1739, (2, 0): 2552, (2, 1): 1545, (4, 0): 561, (4, 1): 405},
                'flag_ignored': {(1, 1): 704, (2, 1): 1080, (4, 1): 261},
                'flag_without_lanes_64_65': {(1, 1): 0, (2, 1): 0},
                'flag_without_wave_0': {(2, 1): 16},
                'flag_without_wave_1': {(2, 1): 48},
                'flag_without_wave_2': {(2, 1): 32},
                'flag_without_wave_3': {(2, 1): 32},
                'float_contracted': {(1, 0): 3472, (1, 1): 2426, (2, 0): 3316, (2, 1): 2307, (4, 0): 665, (4, 1): 285},
                'no_redo': {(2, 0): 10412, (2, 1): 7366, (4, 0): 2527, (4, 1): 1309},
                'no_tiny': {(1, 0): 3908, (1, 1): 2473, (2, 0): 3109, (2, 1): 2477, (4, 0): 685, (4, 1): 313},
                'pool_pairs': {(2, 0): 2069, (2, 1): 1563, (4, 0): 947, (4, 1): 736},
                'pool_reversed': {(2, 0): 3141, (2, 1): 2634, (4, 0): 1553, (4, 1): 1179},
                'redo_without_channel_1': {(2, 0): 1799, (2, 1): 1449, (4, 0): 390, (4, 1): 183},
                'redo_without_channel_2': {(2, 0): 7303, (2, 1): 4889, (4, 0): 1842, (4, 1): 996},
                'redo_without_channel_3': {(2, 0): 1310, (2, 1): 1028, (4, 0): 295, (4, 1): 130},
                'redo_without_gx_term': {(2, 0): 0, (2, 1): 0, (4, 0): 0, (4, 1): 0},
                'smooth_all_fp32': {(1, 1): 1756, (2, 1): 1451, (4, 1): 580}}


def test_every_wrong_kernel_differs_from_the_oracle():
    found = wrong_counts()
    for w, cells in found.items():
        print(w, {f"{s}/{sm}": n for (s, sm), n in cells.items()})
    for w, cells in found.items():
        if w in NOT_WRONG:
            assert all(n == 0 for n in cells.values()), w
        else:
            assert cells and all(n >= 1 for n in cells.values()), (w, cells)
    assert found == WRONG_COUNTS


def test_no_random_image_is_separating_from_its_halo_alone():
    """The halo finding on images that were not designed: 60 of the word family, both 64-wide cells."""
    sep = halo = 0
    for seed in range(60):
        img = gd.word_image(seed, 64, 140)
        for shrink in (1, 2):
            gx, gy = gd.sobel_int(img[:32 * shrink, :70 * shrink])
            lv, _ = gd.step2(gx, gy, shrink)
            rep = gd.tile_report(lv, gd.odd_ring(img[:32 * shrink, :70 * shrink], shrink), orc.smooth_image_3d(lv), shrink)
            sep += int(rep["separating"].sum())
            halo += int((rep["separating"] & ~rep["odd_inner"]).sum())
    assert (sep > 0, halo) == (True, 0)
