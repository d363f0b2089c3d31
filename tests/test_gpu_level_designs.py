"""The level kernels of csrc/wb_chan_levels.hip -- resize_level_kernel, pool2_kernel, smooth_kernel -- and the cast-back of
the float64-held image dtypes in the channel tile kernels (Src<double>::finish) on the designed inputs of level_designs.py:
float16 ties and double roundings, bool pixels under a weight of exactly 0, negative values truncated toward zero, 32 and
64 bit integers no float32 holds, clip-decided pixels, NaN octaves; uint8 quads on every wrap residue, order-sensitive and
overflowing float32 quads, cancelling nine-term sums, borders next to a NaN, arrays of 255, 256, 257 and 513 elements.
What the designs hold, and that a wrong kernel would show, is proved by test_level_designs_host.py.  Every comparison is
bit for bit with the oracle (any NaN equals any NaN: its payload is the hardware's); there are no tolerances.

  1. wb_resize_level_launch at the C ABI: octaves and (min, max) keys from wb_octaves_launch, level records and taps from
     PyramidPlan, a canary behind the output, every level of the plan against orc.resize_bilinear
  2. the same images through the channel kernels (grad_hist; shrink 1 / smooth 0 and shrink 2 / smooth 1)
  3. wb_pool_smooth_launch at the C ABI: every (dtype, shrink, smooth) cell, canaries behind out and tmp, the error returns
  4. through channel_pyramid around a caller's own function, two interleaved generators included"""
import ctypes as C

import numpy as np
import pytest

import level_designs as ld
import resample_designs as rd
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat
from waldboost_amd.engine import image_code
from waldboost_amd.plan import PyramidPlan

pytestmark = pytest.mark.gpu
SPARE = 64                                   # canary elements behind a buffer
POISON = {np.dtype(np.uint8): 0xAB, np.dtype(np.float32): -7.25, np.dtype(np.float64): -7.25}


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _guarded(n, dtype, dev):
    """A device buffer of n elements with SPARE poisoned ones behind it (and the n themselves poisoned)."""
    import torch
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]
    return torch.full((n + SPARE,), POISON[np.dtype(dtype)], dtype=tdt, device=dev)


def _take(buf, n, what):
    h = buf.cpu().numpy()
    assert (h[n:] == h.dtype.type(POISON[h.dtype])).all(), f"{what}: a store behind the buffer"
    return h[:n]


# ------------------------------------------------------------------------------ 1. wb_resize_level_launch
def resized_levels(img, n_per_oct):
    """Every level of the shrink-1 plan of one image through wb_octaves_launch and wb_resize_level_launch: [array [nh, nw] in
    the dtype the image is held in on the device], and the plan."""
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    store, code = image_code(img.dtype)
    store = np.dtype(store)
    H, W = img.shape
    plan = PyramidPlan(H, W, 1, n_per_oct, 0)
    table, _ = plan.level_table()
    taps, _ = plan.tap_table()
    st = nat.stream_ptr()
    img_d = _guarded(H * W, store, dev)
    img_d[:H * W] = torch.from_numpy(np.ascontiguousarray(img.astype(store)).reshape(-1)).to(dev)
    oct_d = _guarded(plan.oct_total, store, dev)
    wide = store == np.float64
    mm_d = torch.zeros((plan.n_oct, 2), dtype=torch.int64 if wide else torch.int32, device=dev)          # the caller zeroes the keys
    off = (C.c_int64 * plan.n_oct)(*[int(x) for x in plan.oct_off])
    rc = lib.wb_octaves_launch(st, nat.ptr(img_d), code, 1, H, W, H * W, nat.ptr(oct_d), plan.oct_total, off, plan.n_oct, nat.ptr(mm_d))
    assert rc == 0, nat.last_error()
    mm = mm_d.cpu().numpy()
    taps_d = torch.from_numpy(taps.view(np.uint8).copy()).to(dev)
    out = []
    for l in range(plan.n_levels):
        rec = np.ascontiguousarray(table[l:l + 1])
        nh, nw = int(rec[0]["nh"]), int(rec[0]["nw"])
        keys = np.ascontiguousarray(mm[int(rec[0]["oct"])])
        buf = _guarded(nh * nw, store, dev)
        rc = lib.wb_resize_level_launch(st, nat.ptr(img_d), nat.ptr(oct_d), code, _vp(rec), _vp(keys), nat.ptr(taps_d), nat.ptr(buf))
        assert rc == 0, nat.last_error()
        out.append(_take(buf, nh * nw, f"level {l}").reshape(nh, nw))
    _take(oct_d, plan.oct_total, "octaves")
    return out, plan


def check_levels(img, n_per_oct, masks, what):
    got, plan = resized_levels(img, n_per_oct)
    with np.errstate(all="ignore"):
        octs = list(orc.image_octaves(img))
        assert plan.n_oct == len(octs) and plan.n_levels >= 3
        for l, lv in enumerate(plan.levels):
            ref = orc.resize_bilinear(octs[lv["oct"]], lv["nh"], lv["nw"])
            assert ref.dtype == img.dtype
            ref = np.ascontiguousarray(ref.astype(got[l].dtype))          # (held dtypes sit on the device as float64: exact)
            if ld.differing(got[l], ref).any():
                if (masks is None or l not in masks) and str(img.dtype) in ld.CAST_MODE:
                    masks = {l: ld.level_masks(octs[lv["oct"]], lv["nh"], lv["nw"], exact=False)}      # (fp64 classes only)
                pytest.fail(f"{what}, octave {lv['oct']}: " + ld.describe_level_mismatch(got[l], ref, l, masks))


@pytest.mark.parametrize("case", ld.CAST_DESIGNS, ids=ld.case_id)
def test_resize_level_casts_back_every_held_dtype(case):
    name, dtype = case
    d = ld.cast_design(name, dtype)
    for slot, img in enumerate(d["images"]):
        check_levels(img, d["n_per_oct"], ld.design_masks(name, dtype, slot), f"{name}-{dtype} image {slot}")


@pytest.mark.parametrize("case", ld.PLAIN_DESIGNS, ids=ld.case_id)
def test_resize_level_of_uint8_and_float32_images(case):
    name, dtype = case
    imgs, npo = ld.plain_design(name, dtype)
    for slot, img in enumerate(imgs):
        masks = rd.design_masks(name, 1, "uint8", slot if name == "plateaus" else 1) if dtype == "uint8" else None
        check_levels(img, npo, masks, f"{name}-{dtype} image {slot}")


def test_resize_level_refuses_bad_arguments_before_any_launch():
    """Both checks return before the kernel is launched (wb_resize_level_launch: the null test is its first statement, a
    dtype code without a kernel falls through to the last else)."""
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    plan = PyramidPlan(16, 24, 1, 2, 0)
    table, _ = plan.level_table()
    taps, _ = plan.tap_table()
    rec = np.ascontiguousarray(table[1:2])
    keys = np.zeros(2, np.uint32)
    img = torch.zeros(16 * 24, dtype=torch.uint8, device=dev)
    taps_d = torch.from_numpy(taps.view(np.uint8).copy()).to(dev)
    buf = _guarded(int(rec[0]["nh"]) * int(rec[0]["nw"]), np.uint8, dev)
    good = [nat.stream_ptr(), nat.ptr(img), None, nat.WB_DTYPE_U8, _vp(rec), _vp(keys), nat.ptr(taps_d), nat.ptr(buf)]
    for i in (1, 4, 5, 6, 7):
        bad = list(good)
        bad[i] = None
        assert lib.wb_resize_level_launch(*bad) == nat.WB_ERR_INVALID and "null pointer" in nat.last_error(), i
    for code in (nat.WB_DTYPE_RANK8, nat.WB_DTYPE_RANK16, 99):
        bad = list(good)
        bad[3] = code
        assert lib.wb_resize_level_launch(*bad) == nat.WB_ERR_UNSUPPORTED and f"dtype code {code}" in nat.last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAB).all()


# ------------------------------------------------------------------------------ 2. the channel kernels
def same_pyramid(got, ref, what):
    assert len(got) == len(ref) > 0, what
    for l, ((c, s), (rc, rs)) in enumerate(zip(got, ref)):
        assert s == rs and c.dtype == rc.dtype and c.shape == rc.shape, (what, l)
        if ld.differing(np.ascontiguousarray(c), np.ascontiguousarray(rc)).any():
            pytest.fail(ld.describe_array_mismatch(np.ascontiguousarray(c), np.ascontiguousarray(rc), f"{what}, level {l}"))


@pytest.mark.parametrize("shrink,smooth", [(1, 0), (2, 1)])
@pytest.mark.parametrize("case", ld.CAST_DESIGNS, ids=ld.case_id)
def test_held_dtypes_through_the_channel_kernels(case, shrink, smooth):
    """Src<double>::finish: the cast designs behind grad_hist, where every flipped pixel shows."""
    name, dtype = case
    d = ld.cast_design(name, dtype)
    img = d["images"][-1].copy()                                         # (plateaus: the image of slot 1)
    opts = dict(shrink=shrink, n_per_oct=d["n_per_oct"], smooth=smooth)
    with np.errstate(all="ignore"):
        ref = list(orc.channel_pyramid(img, dict(opts, channels="grad_hist")))
    got = list(wb.channels.channel_pyramid(img, dict(opts, channels=wb.channels.grad_hist)))
    same_pyramid(got, ref, f"{name}-{dtype} shrink {shrink} smooth {smooth}")


# ------------------------------------------------------------------------------ 3. wb_pool_smooth_launch
def pool_smooth(arr, shrink, smooth):
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    H, W, Cn = arr.shape
    code = nat.WB_DTYPE_U8 if arr.dtype == np.uint8 else nat.WB_DTYPE_F32
    n = int(np.prod(ld.out_shape(arr, shrink)))
    src = torch.from_numpy(arr.copy()).to(dev)
    out = _guarded(n, arr.dtype, dev)
    tmp = _guarded(n, arr.dtype, dev) if shrink == 2 and smooth else None
    rc = lib.wb_pool_smooth_launch(nat.stream_ptr(), nat.ptr(src), code, H, W, Cn, shrink, smooth, nat.ptr(tmp), nat.ptr(out))
    assert rc == 0, nat.last_error()
    if tmp is not None:
        _take(tmp, n, "tmp")
    assert np.array_equal(ld.bits(src.cpu().numpy()), ld.bits(arr)), "the input was written"
    return _take(out, n, "out").reshape(ld.out_shape(arr, shrink))


@pytest.mark.parametrize("shrink,smooth", ld.CELLS)
@pytest.mark.parametrize("name", ld.POOL_CASES)
def test_pool_smooth_cells_on_designed_arrays(name, shrink, smooth):
    arr = ld.pool_case(name)
    ref = ld.oracle_pool_smooth(name, shrink, smooth)
    got = pool_smooth(arr, shrink, smooth)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if ld.differing(got, ref).any():
        pytest.fail(ld.describe_array_mismatch(got, ref, f"{name} {arr.shape} {arr.dtype} shrink {shrink} smooth {smooth}"))


def test_pool_smooth_refuses_bad_arguments_before_any_launch():
    """Every check is a WB_REQUIRE at the head of wb_pool_smooth_launch: nothing is launched, nothing is written."""
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    src = torch.zeros(8 * 8 * 2, dtype=torch.uint8, device=dev)
    out, tmp = _guarded(8 * 8 * 2, np.uint8, dev), _guarded(8 * 8 * 2, np.uint8, dev)
    st = nat.stream_ptr()
    call = lambda i=src, code=nat.WB_DTYPE_U8, shrink=2, smooth=1, t=tmp, o=out: lib.wb_pool_smooth_launch(
        st, nat.ptr(i), code, 8, 8, 2, shrink, smooth, nat.ptr(t), nat.ptr(o))
    assert call(i=None) == nat.WB_ERR_INVALID and "bad argument" in nat.last_error()
    assert call(o=None) == nat.WB_ERR_INVALID and "bad argument" in nat.last_error()
    for code in (nat.WB_DTYPE_F64, nat.WB_DTYPE_RANK8, nat.WB_DTYPE_F16):
        assert call(code=code) == nat.WB_ERR_INVALID and f"channel dtype {code}" in nat.last_error()
    assert call(shrink=4) == nat.WB_ERR_INVALID and "shrink 4" in nat.last_error()
    assert call(t=None) == nat.WB_ERR_INVALID and "tmp buffer" in nat.last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all() and (tmp.cpu().numpy() == 0xAB).all()
    # ... and the same buffers are good arguments: without a tmp where none is needed, and with it
    assert call(smooth=0, t=None) == 0 and call() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 4. the Python surface
def _as_float(im):
    return im.astype("f")[..., None]


def _two_bytes(im):
    """Two uint8 channels: the lowest byte of every pixel (any flipped bit of the cast shows) and the next one."""
    b = np.ascontiguousarray(im).view(np.uint8).reshape(im.shape + (im.dtype.itemsize,))
    return np.ascontiguousarray(np.stack([b[..., 0], b[..., min(1, im.dtype.itemsize - 1)]], -1))


# one held dtype per cast mode (and the NaN octave), each around both functions
CALLABLE_CASES = [("zero", "int8"), ("top", "int32"), ("top", "uint64"), ("ties", "float16"), ("bars", "bool"), ("wide", "float64"), ("nan", "float16")]


@pytest.mark.parametrize("func,shrink,smooth", [(_as_float, 2, 1), (_two_bytes, 1, 0)], ids=["as_float-2-1", "two_bytes-1-0"])
@pytest.mark.parametrize("case", CALLABLE_CASES, ids=ld.case_id)
def test_pyramid_around_a_callable_on_designed_images(case, func, shrink, smooth):
    name, dtype = case
    d = ld.cast_design(name, dtype)
    img = d["images"][0].copy()
    opts = dict(shrink=shrink, n_per_oct=d["n_per_oct"], smooth=smooth, channels=func)
    with np.errstate(all="ignore"):
        ref = list(orc.channel_pyramid(img, opts))
    got = list(wb.channels.channel_pyramid(img, opts))
    same_pyramid(got, ref, f"{name}-{dtype} around {func.__name__}")


@pytest.mark.parametrize("dtype", ["uint8", "int16", "uint32"])
def test_interleaved_callable_pyramids_keep_each_image_to_its_own_range(dtype):
    """Two generators over the plateaus pair -- same shape, different (min, max) -- share the cached engine: each level of
    each must still carry its own clip-decided pixels (PyramidEngine.resize_level reads the keys back once per epoch)."""
    if dtype == "uint32":
        imgs, npo = ld.cast_design("plateaus", dtype)["images"], ld.cast_design("plateaus", dtype)["n_per_oct"]
        masks = [ld.design_masks("plateaus", dtype, b) for b in (0, 1)]
    else:
        imgs, opts, _ = rd.plateaus(1, dtype)
        npo = opts["n_per_oct"]
        masks = [rd.all_level_masks("plateaus", 1, dtype, b) for b in (0, 1)]
    n_levels = 3 * npo                                                # (the octaves the plateaus were counted in)
    for m in masks:
        assert sum(int(m[l]["clip_decided"].sum()) for l in range(n_levels)) >= ld.FLOOR
    opts = dict(shrink=1, n_per_oct=npo, smooth=0, channels=_as_float)
    refs = [list(orc.channel_pyramid(im, opts))[:n_levels] for im in imgs]
    assert (imgs[0].min(), imgs[0].max()) != (imgs[1].min(), imgs[1].max()) and imgs[0].shape == imgs[1].shape
    gens = [wb.channels.channel_pyramid(im.copy(), opts) for im in imgs]
    for l in range(n_levels):
        for b in (0, 1):
            same_pyramid([next(gens[b])], [refs[b][l]], f"generator {b}, level {l}")
    for g in gens:
        g.close()
