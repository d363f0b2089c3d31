"""The designs of octave_designs.py, proved on the host (no GPU): that the block-by-block pooling with zero padding, the
packed 16-bit lane arithmetic and every design's closed form equal the oracle's octaves bit for bit; that load_path gives
the path the GPU module claims for every case; that the ownership sweep of `extremes` reaches every owner a key can be
lost in; and that each emulated wrong kernel changes what the GPU module compares.  Parametrised over the list the GPU
module runs (octave_designs.CASES)."""
import numpy as np
import pytest

import octave_designs as od
from oracle import wb_oracle as orc


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def n_diff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return int((a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))).any(-1).sum())


# ------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("case", od.CASES, ids=od.case_id)
def test_closed_form_equals_the_oracle(case):
    imgs, ref = od.images(case), od.reference(case)
    dtype, H, W, B = case["dtype"], case["H"], case["W"], case["B"]
    dims = od.octave_dims(H, W)
    # (the tail-wave shapes are the smallest with a 256-pixel tail octave: 16.1 MiB; every other image stays within 5 MiB)
    assert imgs.shape == (B, H, W) and imgs.dtype == np.dtype(dtype) and imgs.nbytes <= (17 if (dtype, H, W) in od.TAIL_WAVE_SHAPES else 5) << 20
    for b in range(B):
        assert [o.shape for o in ref[b]] == dims
        # the pooling restated: block by block with zero padding, then the tail's floor chain
        stored, padded = od.hier_octaves(imgs[b])
        assert len(stored) == len(ref[b]) and all(same_bits(s, o) for s, o in zip(stored, ref[b]))
        if dtype == "uint8":
            # octave-1 values are at most 63, a quad of them sums to at most 252: no octave at or above 2 can wrap
            assert all(int(o.max()) <= 63 for o in ref[b][1:])
            if W % 8 == 0 and len(dims) > 1:
                assert same_bits(od.packed_octave1(imgs[b]), ref[b][1])
        if np.dtype(dtype).kind == "f":
            # finite or inf, and every zero of one sign: min() and max() are unambiguous
            for o in ref[b]:
                assert not np.isnan(o).any() and not (np.signbit(o) & (o == 0)).any()
    if dtype == "uint8" and (H, W, B) in od.PATH_CLAIMS:
        assert od.batch_paths(dtype, H, W, B) == od.PATH_CLAIMS[(H, W, B)]
    if case["design"] == "extremes":
        _check_extremes(case, imgs, ref)
    if case["design"] == "tail_bait":
        _check_tail_bait(case, imgs, ref)


def _check_extremes(case, imgs, ref):
    dtype, H, W, B = case["dtype"], case["H"], case["W"], case["B"]
    k, hi, lo = case["args"]["k"], case["args"]["hi"], case["args"]["lo"]
    m, vh, vl = od.EXTREME_VALUES[dtype]
    form = od.extremes_closed_form(dtype, H, W, B, k, hi, lo)
    for b in range(B):
        for j, o in enumerate(ref[b]):
            assert same_bits(od.render(o.shape, form[b][j]), o), (b, j)
            vals = [form[b][j][0]] + [v for *_, v in form[b][j][1]]
            assert (o.min(), o.max()) == (min(vals), max(vals))
            # k and below see the plateau, each image only its own; a batch-mate is flat at m
            if j <= k:
                assert o.max() == (vh if b == hi[0] else m) and o.min() == (vl if b == lo[0] else m)
            if b not in (hi[0], lo[0]):
                assert o.min() == o.max() == m
    # in octave k each extreme is ONE pixel, at the position the case names
    assert int((ref[hi[0]][k] == vh).sum()) == 1 and ref[hi[0]][k][hi[1], hi[2]] == vh
    assert int((ref[lo[0]][k] == vl).sum()) == 1 and ref[lo[0]][k][lo[1], lo[2]] == vl
    if B == 3:
        assert hi[0] != lo[0]


def _check_tail_bait(case, imgs, ref):
    m, vlo, vhi, bright = od.BAIT_VALUES[case["dtype"]]
    dt = np.dtype(case["dtype"]).type
    for b in range(case["B"]):
        if case["args"]["variant"] == "corner":
            assert int((imgs[b] == dt(vlo)).sum()) == 1 and int((imgs[b] == dt(vhi)).sum()) == 1
            assert (ref[b][0].min(), ref[b][0].max()) == (dt(vlo), dt(vhi))
        else:
            assert int((imgs[b] == dt(bright)).sum()) >= 8 and ref[b][0].max() == dt(bright)
        # the odd tails appear in octave 0's keys and in no other octave's keys or pixels
        assert len(ref[b]) >= 3 and all((o == dt(m)).all() for o in ref[b][1:])
    # a kernel that let the padded quads into its keys would raise octave 1's maximum (pairs) / lower its minimum
    wrong = od.emulated_keys(case["dtype"], imgs, od.batch_paths(case["dtype"], case["H"], case["W"], case["B"]), ("odd_tails",))
    for b in range(case["B"]):
        assert wrong[b][1] != (dt(m), dt(m))
        if case["args"]["variant"] == "pairs":
            assert wrong[b][1][1] > dt(m)


# ------------------------------------------------------------------------------ paths
def test_load_path_restates_the_kernel_conditions():
    H, W = od.CABI_SHAPE
    assert H % 2 == 1 and W % 16 == 0
    for (img_off, oct_delta), want in od.CABI_RUNS:
        assert od.load_path(H, W, img_off, H * W, oct_delta) == want
    assert {p for _, p in od.CABI_RUNS} == {"regs", "dword", "scalar"}
    # the batch whose middle image leaves the regs path: oct_total is no multiple of 4
    for H, W in ((72, 80), (73, 80)):
        assert od.oct_offsets(H, W)[1] % 4 == 2 and od.batch_paths("uint8", H, W, 3) == ["regs", "dword", "regs"]
    assert od.load_path(131, 132, 0, 131 * 132, 0) == "dword" and od.load_path(131, 133, 0, 131 * 133, 0) == "scalar"
    assert od.load_path(72, 80, 0, 72 * 80 + 8, 0) == "dword"            # (a stride that breaks the 16-byte rows)
    assert od.load_path(8, 16, 0, 128, 0) == "dword"                      # (one octave: nothing to pool from registers)
    run = {(c["H"], c["W"], c["B"]) for c in od.CASES if c["dtype"] == "uint8"}
    assert set(od.PATH_CLAIMS) <= run
    assert {(72, 80, 3), (73, 80, 3), (131, 132, 1), (131, 133, 1), (129, 144, 1), (131, 260, 1), (8, 8, 1), (8, 16, 1), (9, 23, 3),
            (1024, 1040, 1), (2048, 2064, 1)} <= run
    runf = {(c["H"], c["W"]) for c in od.CASES if c["dtype"] == "float32"}
    assert {(65, 80), (67, 132), (1024, 1040), (8, 8), (8, 16), (9, 23)} <= runf
    # every design runs at batch 1 and at batch 3
    for design in ("extremes", "tail_bait", "quads", "float_quads", "held_quads"):
        assert {c["B"] for c in od.CASES if c["design"] == design} == {1, 3}
    assert {c["dtype"] for c in od.CASES if c["design"] == "held_quads"} == set(od.HELD)
    assert {c["dtype"] for c in od.CASES if c["design"] == "extremes"} == {"uint8", "float32", "int16", "float64"}


# ------------------------------------------------------------------------------ ownership
def _owners(dtype):
    """Per extreme ("hi" | "lo") the owners the sweep's cases give it: (batch, octave, kernel, walk, workgroup kind, wave,
    lane, image)."""
    out = {"hi": [], "lo": []}
    for c in od.CASES:
        if c["design"] != "extremes" or c["dtype"] != dtype:
            continue
        H, W, B, k = c["H"], c["W"], c["B"], c["args"]["k"]
        paths = od.batch_paths(dtype, H, W, B)
        for which in ("hi", "lo"):
            b, y, x = c["args"][which]
            own = od.owner_map(dtype, H, W, k, paths[b])
            wg, last = int(own["wg"][y, x]), int(own["wg"].max())
            kind = "first" if wg == 0 else "last" if wg == last else "inner"
            if own["kernel"] == "block":
                OB = od.BLOCK[dtype][0]
                assert last == od.n_workgroups(dtype, H, W) - 1 or k > 0
                if kind == "last":
                    assert H % OB or W % OB                    # the last workgroup is a partial block
            out[which].append((B, k, own["kernel"], own["walk"], kind, int(own["wave"][y, x]), int(own["lane"][y, x]), b))
    return out


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_ownership_sweep_reaches_every_owner(dtype):
    n_oct_max = 9 if dtype == "uint8" else 8
    walk, tail = od.walk_octaves(dtype, n_oct_max), od.tail_octaves(dtype, n_oct_max)
    assert (walk, tail) == (([4, 5, 6, 7], [8]) if dtype == "uint8" else ([3, 4, 5, 6], [7]))
    for which, owners in _owners(dtype).items():
        block = [o for o in owners if o[2] == "block"]
        for kind in ("first", "last"):
            assert {o[5] for o in block if o[4] == kind and not o[3]} == {0, 1, 2, 3}, (which, kind)
        assert any(o[6] != 0 for o in block)
        assert {o[1] for o in block if o[3]} == set(walk), which
        assert all(o[5] == 0 for o in block if o[3])                     # (the walk is wave 0's)
        assert {o[1] for o in owners if o[2] == "tail"} == set(tail), which
        assert {o[7] for o in owners if o[0] == 3} == {0, 1, 2}, which
        # every path's own octave-0 and octave-1 items (uint8)
    if dtype == "uint8":
        swept = {od.batch_paths("uint8", c["H"], c["W"], 1)[0] for c in od.CASES if c["design"] == "extremes" and c["B"] == 1 and c["args"]["k"] == 0}
        assert swept == {"regs", "dword", "scalar"}


@pytest.mark.parametrize("dtype", ["int16", "float64"])
def test_held_extremes_sit_in_every_octave_and_image(dtype):
    owners = _owners(dtype)
    for which in ("hi", "lo"):
        assert {o[1] for o in owners[which]} == {0, 1, 2} and {o[7] for o in owners[which] if o[0] == 3} == {0, 1, 2}
        for kind in ("first", "last"):                                   # (one atomic per wave: every wave of both ends)
            assert {o[5] for o in owners[which] if o[4] == kind} == {0, 1, 2, 3}
        assert any(o[6] for o in owners[which])


# ------------------------------------------------------------------------------ what the designs hold
def test_quads_hold_every_sum_in_every_position():
    q = od.quad_list().astype(np.int64)
    s = q.sum(1)
    assert np.array_equal(np.unique(s), np.arange(1021))
    for v in range(1021):
        assert len({tuple(r) for r in q[s == v]}) >= (1 if v in (0, 1020) else 2 if v in (1, 2, 1018, 1019) else 3), v
    assert int((q[:, 0] + q[:, 1] >= 256).sum()) >= 500 and int((q == 255).any(1).sum()) >= 500 and int((s >= 256).sum()) >= 2000
    H, W = od.CABI_SHAPE
    img = od.quads(H, W, 1)[0].astype(np.int64)
    h, w = H // 2, W // 2
    cell = img[0:2 * h:2, 0:2 * w:2] + img[1:2 * h:2, 0:2 * w:2] + img[0:2 * h:2, 1:2 * w:2] + img[1:2 * h:2, 1:2 * w:2]
    wraps = cell >= 256
    # a wrapping quad at every column position of a 16-pixel group (cell column mod 8: both byte lanes of each dword), and in
    # the cells on both sides of every 128-pixel seam, in x and in y
    assert all(int(wraps[:, p::8].sum()) >= 100 for p in range(8))
    assert all(wraps[:, c].sum() >= 10 for c in (63, 64, 127, 128)) and all(wraps[r].sum() >= 10 for r in (63, 64))
    assert np.array_equal(np.unique(cell), np.arange(1021))
    assert int(wraps.sum()) >= 5000


def _pixel_fault_counts():
    """fault -> {case id: pixels of octaves >= 1 that differ from the oracle's}, over the cases whose kernel has the fault's
    mechanism."""
    applies = {"nowrap": lambda c: c["design"] in ("quads", "held_quads") and np.dtype(c["dtype"]).kind in "iu" and c["dtype"] != "int64",
               "lane_carry": lambda c: c["design"] == "quads" and c["dtype"] == "uint8",
               "rowfirst": lambda c: c["design"] in ("float_quads", "held_quads") and c["dtype"] in ("float32", "float64"),
               "floor": lambda c: c["design"] == "held_quads" and np.dtype(c["dtype"]).kind == "i",
               "single_f16": lambda c: c["dtype"] == "float16"}
    applies["pairwise"] = applies["reversed"] = applies["rowfirst"]
    out = {}
    for fault in od.PIXEL_FAULTS:
        out[fault] = {}
        for c in od.CASES:
            if not applies[fault](c) or c["H"] > 200:
                continue
            imgs, ref = od.images(c), od.reference(c)
            paths = od.batch_paths(c["dtype"], c["H"], c["W"], c["B"])
            n = 0
            for b in range(c["B"]):
                if fault == "lane_carry" and paths[b] != "regs":
                    continue                                   # (only the regs path packs two pixels into a dword)
                wrong = od.wrong_octaves(imgs[b], fault)
                n += sum(n_diff(wo, o) for wo, o in zip(wrong[1:], ref[b][1:]))
            out[fault][c["id"]] = n
    return out


def test_each_wrong_pooling_is_caught_in_a_hundred_pixels():
    counts = _pixel_fault_counts()
    print({f: max(v.values()) for f, v in counts.items()})
    for fault, per in counts.items():
        assert per and max(per.values()) >= 100, (fault, per)
    # ... in every dtype the fault exists in
    for fault, dtypes in (("nowrap", ("uint8", "int8", "int16", "uint16", "int32", "uint32")), ("floor", ("int8", "int16", "int32", "int64")),
                          ("rowfirst", ("float32", "float64")), ("pairwise", ("float32", "float64")), ("reversed", ("float32", "float64"))):
        for dt in dtypes:
            assert max(n for cid, n in counts[fault].items() if f"-{dt}-" in cid) >= 100, (fault, dt)
    # the regs path's lane carry shows where image 1 of a batch is on another path too (72 x 80: images 0 and 2)
    assert counts["lane_carry"]["quads-uint8-72x80x3"] >= 100 and counts["lane_carry"]["quads-uint8-131x272x1"] >= 1000


def test_float_quads_hold_inf_and_subnormal_quarters():
    c = next(c for c in od.CASES if c["id"] == "float_quads-float32-67x132x1")
    o1 = od.reference(c)[0][1]
    tiny = np.finfo(np.float32).tiny
    assert int(np.isposinf(o1).sum()) >= 20 and int(np.isneginf(o1).sum()) >= 20
    assert int(((o1 > 0) & (o1 < tiny)).sum()) >= 60
    fmax = np.finfo(np.float32).max
    assert int((np.isfinite(o1) & (np.abs(o1) > fmax / 8)).sum()) >= 20
    # the overflow quads are order sensitive as well: a + b alone overflows in half of them
    img = od.images(c)[0]
    with np.errstate(over="ignore"):
        assert int(np.isinf(img[0:12:2, 0:8:2] + img[1:12:2, 0:8:2]).sum()) >= 10


def test_held_quads_sit_on_the_wrap_boundaries():
    for dtype in ("int8", "int16", "uint16", "int32", "uint32"):
        q = od.held_quad_list(dtype).astype(object).sum(1)
        bits = np.dtype(dtype).itemsize * 8
        half = 1 << (bits - 1)
        bounds = [half, 3 * half, -half, -3 * half] if np.dtype(dtype).kind == "i" else [2 * half, 4 * half, 6 * half]
        for bd in bounds:
            for e in (-2, -1, 0, 1):                           # both sides of the boundary, and on it
                assert (q == bd + e).any(), (dtype, bd, e)
    for dtype in ("int8", "int16", "int32", "int64"):
        q = od.held_quad_list(dtype).astype(object).sum(1)
        assert {int(v) % 4 for v in q if -16 <= v < 0} == {0, 1, 2, 3}
    q64 = od.held_quad_list("int64")
    assert int(np.abs(q64).max()) == 1 << 50 and int(np.abs(q64.astype(object).sum(1)).max()) == 1 << 52
    assert len({tuple(r) for r in od.held_quad_list("bool").tolist()}) == 16


# ------------------------------------------------------------------------------ key faults
def _key_cases():
    return sorted((c for c in od.CASES if c["design"] in ("extremes", "tail_bait")), key=lambda c: c["H"] * c["W"] * c["B"])


def _exposed(fault, limit=None):
    """The cases on which a kernel with `fault` in its reduction reports another key than the oracle's."""
    hit = []
    for c in _key_cases():
        n_oct = len(od.octave_dims(c["H"], c["W"]))
        if (fault[0] == "slot" and fault[1] >= n_oct) or (fault[0] == "image" and fault[1] >= c["B"]):
            continue
        if c["H"] > 300 and hit:
            break                                              # (the large shapes only where nothing smaller shows it)
        paths = od.batch_paths(c["dtype"], c["H"], c["W"], c["B"])
        wrong = od.emulated_keys(c["dtype"], od.images(c), paths, fault)
        true = [od.true_keys(o) for o in od.reference(c)]
        if wrong != true:
            hit.append(c["id"])
            if limit and len(hit) >= limit:
                break
    return hit


@pytest.mark.parametrize("fault", od.KEY_FAULTS, ids=lambda f: "-".join(map(str, f)))
def test_each_wrong_reduction_changes_a_key(fault):
    hit = _exposed(fault, limit=None if fault[0] == "wave" else 4)
    assert hit, fault
    if fault[0] == "wave":
        # a dropped wave shows in the block kernel for bytes on every path and for floats, and in the held dtypes' kernels
        assert any("-uint8-200x208x1" in h for h in hit) and any("-uint8-201x213x1" in h for h in hit)
        assert any("-float32-" in h for h in hit) and any("-int16-" in h or "-float64-" in h for h in hit)


@pytest.mark.parametrize("shape", od.TAIL_WAVE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_tail_wave_sweep_exposes_each_wave_of_the_tail_kernel(shape):
    """A tail kernel that drops wave w's partial reports another key for the tail octave on at least one case of the
    sweep, for every w: the octave holds one pixel per thread, 64 per wave, and the extremes sit in single pixels."""
    dtype, H, W = shape
    cases = [c for c in od.CASES if c["design"] == "extremes" and (c["dtype"], c["H"], c["W"]) == shape]
    k = od.tail_octaves(dtype, len(od.octave_dims(H, W)))[-1]
    own = od.owner_map(dtype, H, W, k)
    assert own["kernel"] == "tail" and own["wave"].shape == (8, 32) and all(int((own["wave"] == w).sum()) == 64 for w in range(4))
    assert len(cases) == 8 and all(c["args"]["k"] == k and c["B"] == 1 for c in cases)
    waves = [tuple(int(own["wave"][c["args"][e][1:]]) for e in ("hi", "lo")) for c in cases]
    assert set(waves) == {(w, (w + 1) % 4) for w in range(4)} | {((w + 1) % 4, w) for w in range(4)}

    def changed(c, w):
        wrong = od.emulated_keys(dtype, od.images(c), ["scalar"], ("wave", w), only=(k,))
        true = od.true_keys(od.reference(c)[0])
        assert wrong[0][:k] == true[:k]
        return wrong[0][k] != true[k]
    for w in range(4):
        assert any(changed(c, w) for c in cases), (shape, w)


def test_a_right_reduction_changes_nothing():
    for c in _key_cases()[:40]:
        paths = od.batch_paths(c["dtype"], c["H"], c["W"], c["B"])
        assert od.emulated_keys(c["dtype"], od.images(c), paths, ("none",)) == [od.true_keys(o) for o in od.reference(c)]


def test_mismatch_message_names_image_octave_pixel_and_owner():
    c = next(c for c in od.CASES if c["id"].startswith("quads-uint8-72x80x3"))
    ref = od.reference(c)[1][1]
    got = ref.copy()
    got[5, 9] ^= 1
    msg = od.describe_mismatch(c, 1, 1, got, ref)
    assert "image 1 (path dword) octave 1: 1 pixels differ, first at (5, 9)" in msg and "workgroup 0 wave 1 lane 9" in msg
