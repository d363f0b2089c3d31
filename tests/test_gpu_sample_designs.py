"""The sample kernels of csrc/wb_cascade.hip on designed inputs, straight at the C ABI (wb_gather_samples_launch,
wb_tree_eval_launch, wb_tree_apply_launch, wb_samples_predict_launch through wb_model_create; include/waldboost_hip.h):
tests/sample_designs.py holds the designs, tests/test_sample_designs_host.py proves from the oracle alone what they separate,
and here the kernels must give the oracle's answer exactly -- crops byte for byte with the bytes around `out` untouched, leaf
indices equal, predictions and scores equal by bits (a NaN as NaN).  Then once each through the Python surface."""
import ctypes as C

import numpy as np
import pytest

import sample_designs as sd
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.float32)


def _code(dtype):
    return nat.WB_DTYPE_U8 if np.dtype(dtype) == np.uint8 else nat.WB_DTYPE_F32


def _dev(a):
    """The bytes of `a` on the device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(nat.require_gpu())


def _dev_at(a, offset):
    """The bytes of `a` on the device, `offset` bytes behind a 16-byte boundary -> (the tensor that owns them, pointer)."""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(16 + b.size + 16, dtype=torch.uint8, device=nat.require_gpu())
    assert buf.data_ptr() % 16 == 0 and 0 <= offset < 16
    buf[offset:offset + b.size] = torch.from_numpy(b.copy()).to(buf.device)
    return buf, C.c_void_p(buf.data_ptr() + offset)


# ------------------------------------------------------------------------------ crops
def gather(cell, m, n, N):
    """wb_gather_samples_launch on a cell's image -> (out bytes, the PAD bytes in front of out, the PAD bytes behind)."""
    import torch
    _, dtype, C_, x_off, out_off, unit = sd.CROP_CELL[cell]
    img = sd.crop_image(dtype, C_)
    rs, cs = sd.crop_origins(m, n, N)
    assert rs.min() >= 0 and cs.min() >= 0 and rs.max() + m <= img.shape[0] and cs.max() + n <= img.shape[1]
    nbytes = N * m * n * C_ * img.itemsize
    keep, X = _dev_at(img, x_off)
    buf = torch.full((sd.PAD + out_off + nbytes + sd.PAD,), sd.CANARY, dtype=torch.uint8, device=nat.require_gpu())
    assert buf.data_ptr() % 16 == 0 and sd.PAD % 16 == 0
    out = buf.data_ptr() + sd.PAD + out_off
    assert sd.crop_path(C_, img.itemsize, X.value % 16, out % 16) == unit                   # the path this launch must take
    rd, cd = _dev(rs), _dev(cs)
    nat.check(nat.load().wb_gather_samples_launch(nat.stream_ptr(), X, _code(dtype), img.shape[0], img.shape[1], C_, nat.ptr(rd),
                                                  nat.ptr(cd), N, m, n, C.c_void_p(out)), "wb_gather_samples_launch")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    lo = sd.PAD + out_off
    return h[lo:lo + nbytes], h[:lo], h[lo + nbytes:]


@pytest.mark.parametrize("cell", [c[0] for c in sd.CROP_CELLS])
def test_crops_byte_for_byte_on_every_path(cell):
    _, dtype, C_, _, _, _ = sd.CROP_CELL[cell]
    img = sd.crop_image(dtype, C_)
    for m, n in sd.crop_shapes(cell):
        for N in (1, 300):
            got, front, behind = gather(cell, m, n, N)
            rs, cs = sd.crop_origins(m, n, N)
            ref = orc.gather_samples(img, rs, cs, (m, n, C_)).view(np.uint8).reshape(-1)
            assert np.array_equal(got, ref), (cell, m, n, N, np.flatnonzero(got != ref)[:8])
            assert (front == sd.CANARY).all() and (behind == sd.CANARY).all(), (cell, m, n, N)


# ------------------------------------------------------------------------------ tree walks
SENTINEL = 0x5A


def _tree_dev(tree):
    return [_dev(tree[k]) for k in ("feature", "threshold", "left", "right", "prediction")]


def tree_apply(tree, X):
    import torch
    N, m, n, C_ = X.shape
    for f in tree["feature"][tree["left"] >= 0]:
        assert f[0] < m and f[1] < n and f[2] < C_
    f, t, l, r, _ = _tree_dev(tree)
    Xd = _dev(X)
    out = torch.full((4 * N + 64,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(nat.load().wb_tree_apply_launch(nat.stream_ptr(), nat.ptr(Xd), _code(X.dtype), N, m, n, C_, nat.ptr(f), nat.ptr(t), nat.ptr(l),
                                              nat.ptr(r), tree["left"].size, nat.ptr(out)), "wb_tree_apply_launch")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[4 * N:] == SENTINEL).all()
    return h[:4 * N].view(np.int32)


def tree_eval(tree, image, rs, cs, window):
    import torch
    u, v, C_ = image.shape
    m, n, _ = window
    assert rs.min() >= 0 and cs.min() >= 0 and rs.max() + m <= u and cs.max() + n <= v
    for f in tree["feature"][tree["left"] >= 0]:
        assert f[0] < m and f[1] < n and f[2] < C_
    f, t, l, r, p = _tree_dev(tree)
    Xd, rd, cd = _dev(image), _dev(rs.astype(np.int32)), _dev(cs.astype(np.int32))
    N = rs.size
    out = torch.full((4 * N + 64,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(nat.load().wb_tree_eval_launch(nat.stream_ptr(), nat.ptr(Xd), _code(image.dtype), u, v, C_, nat.ptr(rd), nat.ptr(cd), N,
                                             nat.ptr(f), nat.ptr(t), nat.ptr(l), nat.ptr(r), nat.ptr(p), tree["left"].size, nat.ptr(out)),
              "wb_tree_eval_launch")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[4 * N:] == SENTINEL).all()
    return h[:4 * N].view(np.float32)


@pytest.mark.parametrize("cell", [c[0] for c in sd.WALK_CELLS])
def test_walks_on_every_tree_shape(cell):
    for shape in sd.TREE_SHAPES:
        for dtype in DTYPES:
            d = sd.walk_design(cell, shape, dtype)
            X = sd.samples(d)
            leaf = orc.tree_apply(d["tree"], X)
            got = tree_apply(d["tree"], X)
            assert np.array_equal(got, leaf), (cell, shape, dtype, np.flatnonzero(got != leaf)[:8])
            pred = orc.tree_predict_on_image(d["tree"], d["image"], d["rs"], d["cs"])
            got = tree_eval(d["tree"], d["image"], d["rs"], d["cs"], d["window"])
            assert sd.same_floats(got, pred), (cell, shape, dtype, np.flatnonzero(got != pred)[:8])


@pytest.mark.parametrize("window", sd.TIE_WINDOWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_walks_on_ties_and_special_values(dtype, window):
    X = sd.tie_samples(dtype, window)
    img, rs, cs = sd.as_image(X)
    for t in (sd.U8_THRESHOLDS if dtype == np.uint8 else sd.tie_thresholds()):
        tree = sd.tie_tree(window, t)
        leaf = orc.tree_apply(tree, X)
        got = tree_apply(tree, X)
        assert np.array_equal(got, leaf), (dtype, window, t, t.view(np.uint32), got, leaf)
        got = tree_eval(tree, img, rs, cs, window)
        assert sd.same_floats(got, tree["prediction"][leaf]), (dtype, window, t, got)


# ------------------------------------------------------------------------------ cascades on samples
def create_model(d):
    """wb_model_create on a design's raw arrays -> (return code, handle)."""
    lib = nat.load()
    nat.require_gpu()
    off, f, t, l, r, p = sd.flat_arrays(d["trees"])
    th = np.ascontiguousarray(d["thetas"], np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    h = C.c_void_p()
    m, n, C_ = d["window"]
    rc = lib.wb_model_create(len(d["trees"]), off.ctypes.data_as(C.c_void_p), vp(f), vp(t), vp(l), vp(r), vp(p), vp(th), m, n, C_, C.byref(h))
    return rc, h


def predict(d, handle):
    import torch
    X = d["X"]
    N = X.shape[0]
    Xd = _dev(X)
    H = torch.full((4 * N + 64,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    mask = torch.full((N + 64,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(nat.load().wb_samples_predict_launch(nat.stream_ptr(), handle, nat.ptr(Xd), _code(X.dtype), N, nat.ptr(H), nat.ptr(mask)),
              "wb_samples_predict_launch")
    torch.cuda.synchronize()
    h, k = H.cpu().numpy(), mask.cpu().numpy()
    assert (h[4 * N:] == SENTINEL).all() and (k[N:] == SENTINEL).all()
    return h[:4 * N].view(np.float32), k[:N]


@pytest.mark.parametrize("design", sd.SCORE_DESIGNS)
def test_cascades_on_samples(design):
    lib = nat.load()
    for cell in (c[0] for c in sd.MODEL_CELLS):
        d = sd.score_design(design, cell)
        rc, handle = create_model(d)
        if (design, cell) in sd.REFUSED:
            assert rc != 0 and sd.REFUSED[(design, cell)] in nat.last_error(), (design, cell, rc, nat.last_error())
            continue
        assert rc == 0, (design, cell, nat.last_error())
        try:
            info = nat.WbModelInfo()
            nat.check(lib.wb_model_info(handle, C.byref(info)), "wb_model_info")
            assert info.n_stages == len(d["trees"]) and (info.m, info.n, info.C) == tuple(d["window"])
            # (the node-walk kernel's tile is 4 window rows; a tile kernel's is rows per wave x waves, 8 at the least)
            assert (info.tile_rows == 4) == d["generic"], (design, cell, info.tile_rows, info.depth)
            H, mask = predict(d, handle)
        finally:
            nat.check(lib.wb_model_destroy(handle), "wb_model_destroy")
        with np.errstate(invalid="ignore", over="ignore"):
            rH, rmask = orc.model_predict(d["window"], d["trees"], list(d["thetas"]), d["X"])
        assert set(np.unique(mask).tolist()) <= {0, 1}, (design, cell, np.unique(mask))
        assert np.array_equal(mask.astype(bool), rmask), (design, cell, np.flatnonzero(mask.astype(bool) != rmask)[:8])
        assert sd.same_floats(H, rH), (design, cell, H[:8], rH[:8])
        assert (H[mask == 0].view(np.uint32) == 0xFF800000).all()                       # a rejected sample: -inf


# ------------------------------------------------------------------------------ once through the Python surface
def test_python_surface_holds_the_same_designs():
    import waldboost_amd as wb
    from waldboost_amd.samples import gather_samples
    from waldboost_amd.training import DTree
    # gather_samples: the five-channel float32 cell (words), 65 pixels per crop, 300 unsorted origins
    img = sd.crop_image(np.float32, 5)
    rs, cs = sd.crop_origins(5, 13, 300)
    got = gather_samples(img, rs, cs, (5, 13, 5))
    ref = orc.gather_samples(img, rs, cs, (5, 13, 5))
    assert got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()
    # DTree.predict_on_image / apply: the left chain under features with bit 7 set
    for cell in ("rows130", "chan200"):
        d = sd.walk_design(cell, "left_chain", np.uint8 if cell == "chan200" else np.float32)
        t = d["tree"]
        tree = DTree([tuple(f) for f in t["feature"]], t["threshold"], t["left"], t["right"], t["prediction"])
        X = sd.samples(d)
        assert np.array_equal(tree.apply(X), orc.tree_apply(t, X))
        assert sd.same_floats(tree.predict_on_image(d["image"], d["rs"], d["cs"]), orc.tree_predict_on_image(t, d["image"], d["rs"], d["cs"]))
    # Model.predict: every tree shape on 3 x 7 x 4 float32 samples, and the NaN score that a free stage keeps
    for design in ("shapes", "nan_free"):
        d = sd.score_design(design, "w374/f32")
        M = wb.Model(d["window"], {})
        for t, th in zip(d["trees"], d["thetas"]):
            M.classifier.append(DTree([tuple(f) for f in t["feature"]], t["threshold"], t["left"], t["right"], t["prediction"]))
            M.theta.append(float(th))
        H, mask = M.predict(d["X"])
        with np.errstate(invalid="ignore", over="ignore"):
            rH, rmask = orc.model_predict(d["window"], d["trees"], list(d["thetas"]), d["X"])
        assert mask.dtype == bool and np.array_equal(mask, rmask) and sd.same_floats(H, rH), design
        if design == "nan_free":
            assert np.isnan(H).any() and mask.all()
