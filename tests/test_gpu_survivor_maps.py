"""The cascade kernels on designed survivor maps (tests/survivor_maps.py): the test decides at which stage every window
dies, so alive[], the survivors' (r, c) and the record count are known in closed form, and the score bits from the oracle's
fp32 running sum.  Every comparison is exact.  The maps put chosen numbers of survivors behind stage 8 and 16 into chosen
lanes, rows and waves, sit just under and just over the survivor queue's capacity, walk the dense continuation, and bait
every out-of-grid pixel: test_survivor_maps_host.py proves, without a GPU, the closed form against the oracle and each
map's regime for every parametrisation used here.

Kernel forms: uint8 and float32 tiles through Model.predict_on_image_stats; RANK8 and RANK16 tiles through
wb_cascade_launch on crafted rank buffers (with the grow-and-rescan loop of the detection buffer); each byte form again
after DeviceCascade.specialize; the node-walk kernel through a depth-4 designed tree.  No environment switch of the kernel
is set: the maps are built for the defaults."""

import numpy as np
import pytest

import survivor_maps as sm
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat
from waldboost_amd import engine as _engine
from waldboost_amd.plan import PyramidPlan
from waldboost_amd.samples import gather_samples

pytestmark = pytest.mark.gpu

KIND = {"u8": nat.WB_DTYPE_U8, "f32": nat.WB_DTYPE_F32, "rank8": nat.WB_DTYPE_RANK8, "rank16": nat.WB_DTYPE_RANK16}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def form_array(casc, X, form):
    """The uint8 design X as the tile input of a kernel form."""
    if form == "u8":
        return X
    if form == "f32":
        return X.astype(np.float32)
    return sm.rank_image(casc, X, np.uint8 if form == "rank8" else np.uint16)


def raw_scan(dm, form, images, first_cap=64):
    """wb_cascade_launch on a caller's buffer, the way _SingleLevel.scan calls it, for images[b][l] = [u, v, C] arrays of
    the form's dtype: a level table, chn_stride, the tile list and the detection buffer's grow-and-rescan loop.
    Returns (records sorted by (image, level, r, c), alive[B, L, T])."""
    import torch
    lib, dev = nat.load(), nat.require_gpu()
    B, L, T = len(images), len(images[0]), dm.n_stages
    lv = np.zeros(L, nat.LEVEL_DTYPE)
    off = 0
    for l, a in enumerate(images[0]):
        assert a.shape[2] == dm.C and all(im[l].shape == a.shape for im in images)
        lv[l]["u"], lv[l]["v"], lv[l]["chn_off"] = a.shape[0], a.shape[1], off
        off += (a.size + 3) // 4 * 4                              # every level starts on a multiple of 4 elements
    stride = off + 16                                             # (a byte buffer extends 16 bytes past its last element)
    host = np.zeros((B, stride), images[0][0].dtype)
    for b, im in enumerate(images):
        for l, a in enumerate(im):
            o = int(lv[l]["chn_off"])
            host[b, o:o + a.size] = a.reshape(-1)
    buf = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
    levels = torch.from_numpy(lv.view(np.uint8).copy()).to(dev)
    dims = [(max(a.shape[0] - dm.m, 0), max(a.shape[1] - dm.n, 0)) for a in images[0]]
    tl = PyramidPlan._tiles(dims, dm.tile_rows, dm.tile_cols)
    assert tl.size == sum(-(-r // dm.tile_rows) * -(-c // dm.tile_cols) for r, c in dims)
    tiles = torch.from_numpy(tl.view(np.uint8).copy()).to(dev)
    alive = torch.zeros((B, L, max(T, 1)), dtype=torch.int32, device=dev)
    detb = _engine.DetBuffer(first_cap, dev)
    scans = 0
    while True:
        detb.zero()
        alive.zero_()
        nat.check(lib.wb_cascade_launch(nat.stream_ptr(), dm.handle, nat.ptr(buf), KIND[form], stride, B, nat.ptr(levels), L,
                                        nat.ptr(tiles), int(tl.size), nat.ptr(detb.recs), nat.ptr(detb.counts), detb.cap,
                                        nat.ptr(alive)), "wb_cascade_launch")
        scans += 1
        need = detb.max_count()
        if need <= detb.cap:
            break
        assert scans < 3                                          # (the counts are exact: one re-scan is enough)
        detb = _engine.DetBuffer(int(need * 1.5) + 16, dev)
    d = detb.compact().cpu().numpy().view(nat.DET_DTYPE).reshape(-1)
    d = d[np.lexsort((d["c"], d["r"], d["level"], d["image"]))]
    return d, alive[:, :, :T].cpu().numpy().astype(np.int64)


def expect(casc, maps, Xs):
    """Closed-form alive[B, L, T] and the records (image, level, r, c, score) of maps[b][l] with channel images Xs[b][l]."""
    B, L = len(maps), len(maps[0])
    alive = np.zeros((B, L, casc.T), np.int64)
    cols = [[], [], [], [], []]
    for b in range(B):
        for l in range(L):
            alive[b, l], rs, cs = sm.closed_form(maps[b][l], casc.T, casc.free)
            for k, v in enumerate((np.full(rs.size, b), np.full(rs.size, l), rs, cs, sm.survivor_scores(casc, Xs[b][l], rs, cs))):
                cols[k].append(v)
    return alive, [np.concatenate(c) for c in cols]


def check(what, got, got_alive, want_alive, want, where=lambda b, l, r, c: ""):
    """Exact: alive, record count, (image, level, r, c), score bits.  A failure names the first stray records' tiles."""
    image, level, r, c, score = want
    bad = np.argwhere(got_alive != want_alive)
    assert bad.size == 0, f"{what}: alive[image, level, stage] differs first at {bad[0]}: {got_alive[tuple(bad[0])]} != {want_alive[tuple(bad[0])]}"
    key = lambda i, l, rr, cc: (np.asarray(i, np.int64) << 40) | (np.asarray(l, np.int64) << 32) | (np.asarray(rr, np.int64) << 16) | np.asarray(cc, np.int64)
    kg, kw = key(got["image"], got["level"], got["r"], got["c"]), key(image, level, r, c)
    if kg.size != kw.size or not np.array_equal(kg, kw):
        name = lambda k: (int(k >> 40), int(k >> 32) & 255, int(k >> 16) & 65535, int(k) & 65535)
        extra = [name(k) + (where(*name(k)),) for k in np.setdiff1d(kg, kw)[:5]]
        missing = [name(k) + (where(*name(k)),) for k in np.setdiff1d(kw, kg)[:5]]
        raise AssertionError(f"{what}: {kg.size} records, {kw.size} expected; not expected (image, level, r, c, tile): {extra}; "
                             f"missing: {missing}; duplicates: {kg.size - np.unique(kg).size}")
    diff = np.flatnonzero(bits(got["score"]) != bits(score))
    assert diff.size == 0, (f"{what}: {diff.size} scores differ, first at (image, level, r, c) = "
                            f"{(int(image[diff[0]]), int(level[diff[0]]), int(r[diff[0]]), int(c[diff[0]]))} "
                            f"{where(int(image[diff[0]]), int(level[diff[0]]), int(r[diff[0]]), int(c[diff[0]]))}: "
                            f"{got['score'][diff[0]]!r} != {score[diff[0]]!r}")


def scan_single(M, dm, casc, form, X):
    """One channel image through a kernel form -> (records, alive[1, 1, T])."""
    if form in ("u8", "f32"):
        rs, cs, hs, alive = M.predict_on_image_stats(form_array(casc, X, form))
        d = np.zeros(rs.size, nat.DET_DTYPE)
        d["r"], d["c"], d["score"] = rs, cs, hs
        return d, alive.reshape(1, 1, -1)
    return raw_scan(dm, form, [[form_array(casc, X, form)]])


def forms_of(dm):
    if dm.depth > 3:                                               # the node-walk kernel has no rank form
        return ("u8", "f32")
    assert dm.rank_ok and dm.rank16_ok
    return ("u8", "f32", "rank8", "rank16")


def geometry(case, dm):
    """The tile geometry the maps were built for is the one wb_model_create chose (read back from wb_model_info)."""
    shape, TR, waves, T, depth, free = case
    assert (dm.tile_rows, dm.tile_cols, dm.depth, dm.n_stages) == (TR, sm.TILE_COLS, depth, T)
    assert (dm.m, dm.n, dm.C) == shape
    if depth <= 3:                                                 # (the wave count and the queue capacity, through the LDS size)
        assert dm.lds_bytes == sm.lds_bytes(shape, TR, waves, T, depth)


@pytest.mark.parametrize("case", sm.scan_cases(), ids=sm.case_id)
def test_composed_maps_and_edge_levels(case):
    """Every tile pattern of the case composed into one channel image, through every kernel form; then the edge and partial
    grids as the levels of one launch over two images with maps of their own, through the raw ABI."""
    shape, TR, waves, T, depth, free = case
    casc, tiles, per_row, D, X = sm.build_case(case)
    M = casc.model()
    dm = M.device_cascade()
    geometry(case, dm)
    assert not dm.specialized()
    want_alive, want = expect(casc, [[D]], [[X]])
    where = lambda b, l, r, c: sm.which_tile(r, c, TR, per_row, tiles)
    for form in forms_of(dm):
        got, alive = scan_single(M, dm, casc, form, X)
        check(f"{casc.name} {form}", got, alive, want_alive, want, where)
    maps = sm.edge_levels(case)
    Xs = [[sm.channel_image(Dl, shape, 100 * b + l) for l, Dl in enumerate(per)] for b, per in enumerate(maps)]
    want_alive, want = expect(casc, maps, Xs)
    assert want[0].size and len(set(want[0])) == len(maps)
    for form in forms_of(dm):
        got, alive = raw_scan(dm, form, [[form_array(casc, x, form) for x in per] for per in Xs])
        check(f"{casc.name} {form} edge levels", got, alive, want_alive, want)


@pytest.mark.parametrize("form", ["u8", "rank8", "rank16"])
@pytest.mark.parametrize("case", sm.specialised_cases(), ids=sm.case_id)
def test_composed_maps_on_the_specialised_kernels(case, form):
    """The same maps through the model-specialised build of each byte form, twice."""
    shape, TR, waves, T, depth, free = case
    casc, tiles, per_row, D, X = sm.build_case(case)
    M = casc.model()
    dm = M.device_cascade()
    geometry(case, dm)
    if form == "rank16":
        dm.rank_dtype = nat.WB_DTYPE_RANK16
    built = dm.specialize(KIND[form])
    if depth >= 3 and not built:
        pytest.skip(f"no specialised {form} kernel for {casc.name}: {nat.last_error()}")
    assert built and KIND[form] in dm.specialized(), f"specialize({form}) refused for {casc.name}: {nat.last_error()}"
    want_alive, want = expect(casc, [[D]], [[X]])
    where = lambda b, l, r, c: sm.which_tile(r, c, TR, per_row, tiles)
    maps = sm.edge_levels(case)
    Xs = [[sm.channel_image(Dl, shape, 100 * b + l) for l, Dl in enumerate(per)] for b, per in enumerate(maps)]
    edge_alive, edge_want = expect(casc, maps, Xs)
    edge_in = [[form_array(casc, x, form) for x in per] for per in Xs]
    for run in (1, 2):
        got, alive = scan_single(M, dm, casc, form, X)
        check(f"{casc.name} specialised {form}, run {run}", got, alive, want_alive, want, where)
        got, alive = raw_scan(dm, form, edge_in)
        check(f"{casc.name} specialised {form} edge levels, run {run}", got, alive, edge_alive, edge_want)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_samples_of_a_designed_map(depth, dtype):
    """Model.predict over the windows of a map: mask in closed form, H bit-equal to the oracle's model_predict (-inf
    where rejected); DTree.apply / DTree.predict of single stages on the same samples."""
    for N in sm.SAMPLE_COUNTS:
        casc, D, X, rs, cs = sm.sample_case(depth, N)
        shape, trees, thetas = casc.oracle()
        M = casc.model()
        Xd = X.astype(dtype)
        S = gather_samples(Xd, rs, cs, shape)
        ref = orc.gather_samples(Xd, rs, cs, shape)
        assert S.dtype == ref.dtype and np.array_equal(S, ref)
        H, mask = M.predict(S)
        Hr, mr = orc.model_predict(shape, trees, thetas, ref)
        assert mask.dtype == bool and np.array_equal(mask, sm.eff_stage(D[rs, cs], casc.T, casc.free) == casc.T), N
        assert np.array_equal(mask, mr) and np.array_equal(bits(H), bits(Hr)), N
        assert np.isneginf(H[~mask]).all()
        for t in (0, 7, 16, casc.T - 1):
            w = M.classifier[t]
            leaf = orc.tree_apply(trees[t], ref)
            assert np.array_equal(w.apply(S), leaf), (N, t)
            assert np.array_equal(bits(w.predict(S)), bits(trees[t]["prediction"][leaf])), (N, t)
