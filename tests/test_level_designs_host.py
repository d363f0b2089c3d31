"""The designs of level_designs.py, proved on the host (no GPU): that the oracle's level is the cast the design restates --
in exact arithmetic for the truncation (integers at a common power of two), the float16 rounding (fractions) and the bool
rule (taps of non-zero weight) --; that every cast design holds at least 100 pixels of every class it claims; that every
emulated wrong kernel differs from the oracle in at least 100 pixels of every design meant to catch it (pool and smooth: in
at least one element of every array meant to catch it) and the oracle's own restatement in none; and that the pool and
smooth arrays hold the quads, shapes and element counts they were built for.  Parametrised over the lists the GPU module
runs.  The counts printed here (pytest -s) stand in the docstring of level_designs.py."""
import numpy as np
import pytest

import level_designs as ld
import octave_designs as od
import resample_designs as rd
from oracle import wb_oracle as orc
from waldboost_amd.engine import _IMAGE_CODES

FLOOR = ld.FLOOR


def _levels(name, dtype, slot):
    d = ld.cast_design(name, dtype)
    octs = ld.octaves_of(name, dtype, slot)
    plan = ld.plan_levels(*d["shape"], 1, d["n_per_oct"])
    return d, octs, plan, ld.design_masks(name, dtype, slot)


def test_every_image_dtype_has_a_design():
    designed = {dt for _, dt in ld.CAST_DESIGNS} | {dt for _, dt in ld.PLAIN_DESIGNS}
    assert designed == {str(k) for k in _IMAGE_CODES}
    assert {ld.CAST_MODE[dt] for _, dt in ld.CAST_DESIGNS} == {"TRUNC", "F16", "BOOL", "NONE"}
    for name, dtype in ld.CAST_DESIGNS:
        d = ld.cast_design(name, dtype)
        H, W = d["shape"]
        assert H <= rd.RATIO_SHAPES[1][0] and W <= rd.RATIO_SHAPES[1][1] and d["images"].dtype == np.dtype(dtype)
        octs = {ld.plan_levels(H, W, 1, d["n_per_oct"])[l]["oct"] for l in d["levels"]}
        if name != "max":
            assert 0 in octs and max(octs) >= 1, (name, dtype)          # (source = the image, and source = oct + src_off)


@pytest.mark.parametrize("case", ld.CAST_DESIGNS, ids=ld.case_id)
def test_cast_design_holds_what_it_claims(case):
    name, dtype = case
    mode = ld.CAST_MODE[dtype]
    n_slots = len(ld.cast_design(name, dtype)["images"])
    for slot in range(n_slots):
        d, octs, plan, masks = _levels(name, dtype, slot)
        assert len(masks) >= 2
        count = {k: sum(int(m[k].sum()) for m in masks.values()) for k in d["claims"]}
        wrong = dict.fromkeys(d["faults"] + ("clip_after_cast", None), 0)
        for l, m in masks.items():
            lv = plan[l]
            base = octs[lv["oct"]]
            for f in wrong:
                wrong[f] += int(ld.differing(ld.emulate_level(base, lv["nh"], lv["nw"], f), m["out"]).sum())
            _exact_checks(name, mode, base, lv, m)
        print(f"{name}-{dtype} slot {slot}: classes {count}, differing pixels {wrong}")
        assert all(n >= FLOOR for n in count.values()), count
        assert wrong.pop(None) == 0 and wrong.pop("clip_after_cast") == 0
        assert all(n >= FLOOR for n in wrong.values()), wrong
    if name == "plateaus":
        # two same-shape images with different (min, max): each image's own range decides its plateaus
        a, b = (ld.octaves_of(name, dtype, s)[0] for s in (0, 1))
        assert a.shape == b.shape and (a.min(), a.max()) != (b.min(), b.max())


def _exact_checks(name, mode, base, lv, m):
    t, out = m["t"], m["out"]
    v = ld._clip(t, base)
    if mode == "TRUNC":
        assert np.array_equal(np.trunc(v) + 0.0, out) and not np.signbit(out[out == 0]).any()
        if "trunc_exact" in m:
            # away from the integers by more than the fp64 error of the four-term sum (four products and three sums of
            # values up to max |pixel|: below 8 spacings; at 2^50 the spacing is 1/4 and no pixel is away) the oracle's
            # pixel is the truncation of the exact value, clipped
            bound = max(rd.NEAR, 8 * float(np.spacing(np.abs(base.astype(np.float64)).max())))
            away = np.abs(t - np.rint(t)) > bound
            assert away.sum() > away.size // 2 or base.dtype.itemsize == 8
            clipped = np.clip(m["trunc_exact"], int(base.min()), int(base.max()))
            assert np.array_equal(out[away].astype(np.int64), clipped[away])
        if name == "zero":
            assert base.min() < 0 < base.max() and (out[m["negative_fraction"]] == 0).all()
        if name == "top" and base.dtype.itemsize >= 4 and lv["oct"] == 0:
            assert base.astype(np.float64).max() >= 2.0 ** 31 - 1 and m["beyond_f32"].sum() > out.size // 2
    elif mode == "F16":
        if np.isnan(v).all():
            assert np.isnan(out).all()
            return
        exact = np.array([ld.round_f16_exact(x) for x in v.ravel()]).reshape(v.shape)
        assert ld.same_values(exact, out)
        if name == "ties":
            tie = m["tie_down"] | m["tie_up"]
            assert (v[tie] % 2 == 1).all() and np.array_equal(v[tie] % 4 == 1, m["tie_down"][tie])
            assert base.astype(np.float64).min() >= 2048 and base.astype(np.float64).max() <= 4094 and (base.astype(np.float64) % 2 == 0).all()
        if name == "subnormal" and lv["oct"] == 0:
            assert (np.abs(base.astype(np.float64)) < 2.0 ** -14).all()
        if name == "max":
            assert base.astype(np.float64).max() == 65504.0 and np.isfinite(out).all()
    elif mode == "BOOL":
        assert np.array_equal(out != 0, ld.bool_exact(base, lv["nh"], lv["nw"])) and set(np.unique(out)) <= {0.0, 1.0}
        assert not out[m["beside"]].any()
        if lv["nh"] == lv["h"] and lv["nw"] == lv["w"]:
            assert np.array_equal(out != 0, base)                       # an identity level: weight exactly 0 on the second tap
        if name in ("all_false", "all_true"):
            assert base.min() == base.max() and (out == float(name == "all_true")).all()
    else:
        assert ld.same_values(v, out)
        if name == "wide":
            assert base.min() > 1.0                                     # (the clip bounds are away from the signed zeros)
    if name == "nan":
        assert np.isnan(out).all() == (lv["oct"] == 0) and np.isnan(out).any() == (lv["oct"] == 0)
        assert np.isnan(base).any() == (lv["oct"] == 0)


@pytest.mark.parametrize("case", ld.PLAIN_DESIGNS, ids=ld.case_id)
def test_plain_designs_are_the_resample_images(case):
    name, dtype = case
    imgs, npo = ld.plain_design(name, dtype)
    assert imgs.dtype == np.dtype(dtype) and imgs.shape[1:] == rd.RATIO_SHAPES[1][:2] and npo == rd.RATIO_SHAPES[1][2]
    lv = ld.plan_levels(*imgs.shape[1:], 1, npo)[2]
    assert np.array_equal(ld.oracle_level(name, dtype, 0, 2), orc.resize_bilinear(imgs[0], lv["nh"], lv["nw"]))


# ------------------------------------------------------------------------------ pool and smooth
def _quads_of(arr):
    h, w = arr.shape[0] // 2, arr.shape[1] // 2
    return np.stack([arr[0:2 * h:2, 0:2 * w:2], arr[1:2 * h:2, 0:2 * w:2], arr[0:2 * h:2, 1:2 * w:2], arr[1:2 * h:2, 1:2 * w:2]], -1)


def test_pool_arrays_hold_their_quads_and_shapes():
    for name in ld.POOL_CASES:
        a = ld.pool_case(name)
        H, W, C = a.shape
        assert (H <= 64 and W <= 96 and C <= 5) or a.size <= 1028, name
    for c in (1, 2, 3, 5):
        a = ld.pool_case(f"quads_c{c}")
        q = _quads_of(a).astype(np.int64)
        assert a.shape[2] == c and set(q.sum(-1).ravel().tolist()) == set(range(1021)), c        # every residue at every wrap count
        if c > 1:
            assert (np.diff(q, axis=2) != 0).any(-1).all()                 # the channels of a cell hold different quads
        f = _quads_of(ld.pool_case(f"fquads_c{c}"))
        with np.errstate(all="ignore"):
            ours = np.isinf(((f[..., 0] + f[..., 1]) + f[..., 2]) + f[..., 3])
            rows = np.isinf(((f[..., 0] + f[..., 2]) + f[..., 1]) + f[..., 3])
            pairs = np.isinf((f[..., 0] + f[..., 1]) + (f[..., 2] + f[..., 3]))
        n = [int(x.sum()) for x in (ours & ~rows, ~ours & rows, ours & ~pairs)]
        print(f"fquads_c{c}: +-inf in the oracle's order but not rows first {n[0]}, the other way round {n[1]}, but not pairwise {n[2]}; "
              f"+-inf in every order {int((ours & rows & pairs).sum())}")
        assert min(n) >= 1 and (ours & rows & pairs).any()
    assert {ld.pool_case(n).shape[0] % 2 for n in ("quads_c2", "quads_c3", "quads_c5")} == {1}
    for p in ("", "f"):
        for n, want in (("n255", 255), ("n256", 256), ("n257", 257), ("n513", 513)):
            assert ld.oracle_pool_smooth(p + n + "p", 2, 0).size == want and ld.pool_case(p + n + "s").size == want
        assert ld.oracle_pool_smooth(p + "h1", 2, 0).size == 0 and ld.oracle_pool_smooth(p + "w1", 2, 1).size == 0
        for n in ("h2", "w2"):
            assert not ld.oracle_pool_smooth(p + n, 1, 1).any() and ld.pool_case(p + n).any()
        o = ld.oracle_pool_smooth(p + "tmp_odd", 2, 1)
        assert o.shape[0] % 2 == 1 and o.shape[1] % 2 == 1
    # the odd last row and column never reach a pooled result
    for name in ("quads_c3", "fquads_c3"):
        a = ld.pool_case(name).copy()
        a[-1, :, :] = 1
        a[:, -1, :] = 1
        with np.errstate(all="ignore"):
            assert ld.same_values(orc.avg_pool_2(a), ld.oracle_pool_smooth(name, 2, 0))
    assert (ld.oracle_pool_smooth("all255", 1, 1)[1:-1, 1:-1] == 255).all()
    nf = ld.pool_case("nonfinite")
    assert np.isnan(nf[1, 1, 0]) and np.isinf(nf[1, -2, 0]) and np.isinf(nf[-2, 1, 0])
    for name in ld.POOL_CASES:
        o = ld.oracle_pool_smooth(name, 1, 1)
        border = np.ones(o.shape[:2], bool)
        border[1:-1, 1:-1] = False
        assert not ld.bits(o)[border].any(), name                          # +0.0, the sign bit clear


def _smooth_scalar(arr):
    """smooth_image_3d restated element by element in Python numbers: the nine terms in source order (floats: IEEE fp64;
    uint8: integers), / 16, the cast back."""
    u, v, C = arr.shape
    out = np.zeros_like(arr)
    for y in range(1, u - 1):
        for x in range(1, v - 1):
            for c in range(C):
                g = lambda dy, dx: arr[y + dy, x + dx, c].item()
                s = g(-1, -1) + 2 * g(-1, 0)
                for wgt, dy, dx in ((1, -1, 1), (2, 0, -1), (4, 0, 0), (2, 0, 1), (1, 1, -1), (2, 1, 0), (1, 1, 1)):
                    s = s + wgt * g(dy, dx)
                out[y, x, c] = s // 16 if arr.dtype == np.uint8 else np.float32(s / 16)
    return out


def test_the_oracle_differs_from_its_restatement_nowhere():
    with np.errstate(all="ignore"):
        for name in ld.POOL_CASES:
            a = ld.pool_case(name)
            assert ld.same_values(np.ascontiguousarray(od.pool_floor(a)), ld.oracle_pool_smooth(name, 2, 0)), name
            assert ld.oracle_pool_smooth(name, 1, 0) is not None and ld.same_values(ld.oracle_pool_smooth(name, 1, 0), a)
        for name in ("all255", "ramps", "cancel", "nonfinite", "h2", "fw2", "n255s", "fn255s"):
            assert ld.same_values(_smooth_scalar(ld.pool_case(name)), ld.oracle_pool_smooth(name, 1, 1)), name
        for name in ("tmp_odd", "ftmp_odd"):
            assert ld.same_values(_smooth_scalar(np.ascontiguousarray(od.pool_floor(ld.pool_case(name)))), ld.oracle_pool_smooth(name, 2, 1)), name


@pytest.mark.parametrize("fault", list(ld.POOL_FAULTS))
def test_wrong_pool_and_smooth_kernels_show(fault):
    cell, names = ld.POOL_FAULTS[fault]
    for name in names:
        a = ld.pool_case(name)
        got = ld.pool_wrong(a, fault) if cell == (2, 0) else ld.smooth_wrong(a, fault)
        n = int(ld.differing(np.ascontiguousarray(got), ld.oracle_pool_smooth(name, *cell)).sum())
        print(f"{fault} on {name}: {n} of {got.size} elements differ")
        assert n >= 1, (fault, name)
