"""Step 0 of every timed step -- octaves_block_kernel, octaves_tail_kernel and the pool_f64_kernel chain of
csrc/wb_octaves.hip -- on the designed images of octave_designs.py: single-pixel extremes whose owner (workgroup, wave,
lane, kernel, image of the batch) is chosen by position, odd tails that must stay out of every octave but 0, quads on every
sum and wrap boundary of every dtype, order-sensitive and overflowing float quads; at batch 1 and 3, on the batches whose
middle image leaves the regs load path, and, through the C ABI, one image through all three load paths.  What the designs
hold, and that a wrong kernel would show, is proved by test_octave_designs_host.py.  Every comparison is bit for bit with
the oracle's octaves: pixels and (min, max) keys per image and per octave, no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

import octave_designs as od
from waldboost_amd import _native as nat
from waldboost_amd.engine import PyramidEngine

pytestmark = pytest.mark.gpu
P = C.c_void_p
POISON = {np.dtype(np.uint8): 0xAB, np.dtype(np.float32): -7.25, np.dtype(np.float64): -7.25}


@functools.lru_cache(maxsize=6)
def _engine(H, W, dtype, B):
    return PyramidEngine(H, W, np.dtype(dtype), 2, 8, 1, batch=B)


def run_octaves(case):
    """The case's batch through PyramidEngine.load_images / launch_octaves: (octave buffer [B, oct_total], keys [B, n_oct, 2]
    as unsigned words, engine).  The keys are zeroed and the octave buffer poisoned first: the engine is shared between cases."""
    e = _engine(case["H"], case["W"], case["dtype"], case["B"])
    poison = POISON[e.store_dtype]
    e.ctrl[: e._mm_words].zero_()
    e._oct_flat.fill_(poison)
    e.load_images(od.images(case).copy())
    e.launch_octaves()
    assert e.wide_keys == (case["dtype"] in od.HELD)
    flat = e._oct_flat.cpu().numpy()
    assert (flat[e.batch * e.plan.oct_total:] == flat.dtype.type(poison)).all(), "a store past the last octave of the last image"
    mm = e.minmax.cpu().numpy()
    return e.oct.cpu().numpy(), mm.view(np.uint64 if e.wide_keys else np.uint32), e


def check_octaves(case, buf, mm, off, what=""):
    ref = od.reference(case)
    wide = case["dtype"] in od.HELD
    key = od.key64 if wide else od.key32
    inv = np.uint64(0xFFFFFFFFFFFFFFFF) if wide else np.uint32(0xFFFFFFFF)
    assert mm.shape == (case["B"], len(ref[0]), 2)
    for b in range(case["B"]):
        for k, o in enumerate(ref[b]):
            want = o.astype(buf.dtype)                                   # (held dtypes sit on the device as float64: exact)
            if k:
                got = buf[b, off[k]:off[k] + o.size].reshape(o.shape)
                if not np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)):
                    pytest.fail(what + od.describe_mismatch(case, b, k, got, want))
            lo, hi = inv ^ mm[b, k, 0], mm[b, k, 1]                       # word 0 holds max(~key)
            assert (lo, hi) == (key(want.min()), key(want.max())), (
                f"{what}{case['id']}: image {b} octave {k}: keys ({lo:#x}, {hi:#x}) against ({key(want.min()):#x}, {key(want.max()):#x})")


@pytest.mark.parametrize("case", od.CASES, ids=od.case_id)
def test_designed_octaves_through_the_engine(case):
    buf, mm, e = run_octaves(case)
    assert e.plan.n_oct == len(od.octave_dims(case["H"], case["W"]))
    check_octaves(case, buf, mm, [int(x) for x in e.plan.oct_off])


# ------------------------------------------------------------------------------ the C ABI
def _lib():
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    lib = C.CDLL(nat.LIB_PATH)
    lib.wb_last_error.restype = C.c_char_p
    return lib


def _launch_raw(lib, img, img_off, oct_delta):
    """wb_octaves_launch on one uint8 image that starts img_off bytes into a device buffer, every octave offset moved by
    oct_delta elements: (octaves 1 .., keys)."""
    import torch
    dev = torch.device("cuda")
    H, W = img.shape
    off, total = od.oct_offsets(H, W)
    n_oct = len(off)
    big = torch.zeros(H * W + 64, dtype=torch.uint8, device=dev)
    octb = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0 and octb.data_ptr() % 16 == 0
    big[img_off:img_off + H * W] = torch.from_numpy(img.reshape(-1).copy()).to(dev)
    minmax = torch.zeros((n_oct, 2), dtype=torch.int32, device=dev)              # the caller zeroes the keys
    moved = [0] + [o + oct_delta for o in off[1:]]
    rc = lib.wb_octaves_launch(P(torch.cuda.current_stream().cuda_stream), P(big.data_ptr() + img_off), C.c_int(nat.WB_DTYPE_U8), C.c_int(1),
                               C.c_int(H), C.c_int(W), C.c_int64(H * W), P(octb.data_ptr()), C.c_int64(total), (C.c_int64 * n_oct)(*moved),
                               C.c_int(n_oct), P(minmax.data_ptr()))
    assert rc == 0, lib.wb_last_error().decode()
    torch.cuda.synchronize()
    flat = octb.cpu().numpy()
    assert (flat[:oct_delta] == 0xAB).all() and (flat[total + oct_delta:] == 0xAB).all(), "a store outside the octaves"
    dims = od.octave_dims(H, W)
    octs = [flat[moved[k]:moved[k] + dims[k][0] * dims[k][1]].reshape(dims[k]) for k in range(1, n_oct)]
    return octs, minmax.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("design", ["quads", "extremes"])
def test_one_image_through_the_three_load_paths(design):
    """The same 131 x 272 image from a 16-byte aligned pointer, from 4 bytes in and from 1 byte in, with the octave-1
    pointer 4-byte aligned and not: regs, dword and scalar loads give the same octaves and keys, the oracle's."""
    lib = _lib()
    img = od.cabi_images()[design]
    H, W = img.shape
    ref = list(od.orc.image_octaves(img))
    runs = {}
    for (img_off, oct_delta), path in od.CABI_RUNS:
        assert od.load_path(H, W, img_off, H * W, oct_delta) == path
        octs, mm = _launch_raw(lib, img, img_off, oct_delta)
        for k, o in enumerate(ref):
            if k:
                assert np.array_equal(octs[k - 1], o), (design, path, img_off, oct_delta, k)
            assert (int(np.uint32(~mm[k, 0])), int(mm[k, 1])) == (int(o.min()), int(o.max())), (design, path, img_off, oct_delta, k)
        runs[(img_off, oct_delta)] = (octs, mm)
    assert {p for _, p in od.CABI_RUNS} == {"regs", "dword", "scalar"}
    first = runs[(0, 0)]
    for key, (octs, mm) in runs.items():
        assert all(np.array_equal(a, b) for a, b in zip(octs, first[0])) and np.array_equal(mm, first[1]), key


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = _lib()
    dev = torch.device("cuda")
    img = torch.zeros(72 * 80, dtype=torch.uint8, device=dev)
    octb = torch.zeros(4096, dtype=torch.uint8, device=dev)
    mm = torch.zeros(16, dtype=torch.int32, device=dev)
    off, total = od.oct_offsets(72, 80)
    st = P(torch.cuda.current_stream().cuda_stream)
    args = lambda n_oct: (st, P(img.data_ptr()), C.c_int(nat.WB_DTYPE_U8), C.c_int(1), C.c_int(72), C.c_int(80), C.c_int64(72 * 80),
                          P(octb.data_ptr()), C.c_int64(total), (C.c_int64 * len(off))(*off), C.c_int(n_oct), P(mm.data_ptr()))
    assert lib.wb_octaves_launch(*args(len(off) + 1)) != 0 and b"has 4 octaves" in lib.wb_last_error()
    assert lib.wb_octaves_launch(*args(0)) != 0 and b"out of range" in lib.wb_last_error()
    assert lib.wb_octaves_launch_z(*args(len(off)), None, C.c_int(4)) != 0 and b"zero_words without a pointer" in lib.wb_last_error()
    torch.cuda.synchronize()
    assert int(mm.abs().sum()) == 0 and int(octb.sum()) == 0
