"""engine.checked_input on the CPU: the one check between a caller's image (ndarray or tensor) and an engine's resident
image buffer (PyramidEngine.load_images, load_slot).  Every image dtype with a kernel, both containers, the shapes a
batch and a slot take, the three errors in their order, the 2**51 limit of 64-bit integers on both sides, and what comes
back: the storage dtype, exact values, no copy of an array that needs none."""
import numpy as np
import pytest
import torch

from waldboost_amd.engine import _IMAGE_CODES, checked_input

H, W = 5, 7
DTYPES = sorted(_IMAGE_CODES, key=str)
LIMIT = 1 << 51


def sample(dtype, shape=(H, W)):
    """An image of `dtype` that holds the type's extremes (64-bit integers: the largest magnitudes held exactly)."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    if dtype.kind == "b":
        a = np.arange(n) % 3 == 0
    elif dtype.kind == "f":
        a = np.linspace(-3.0, 250.0, n)
    else:
        info = np.iinfo(dtype)
        lo, hi = max(info.min, -(LIMIT - 1)), min(info.max, LIMIT - 1)
        a = np.array([lo, hi, 0, 1, hi - 1, lo + 1] * n, dtype=object)[:n]
    return np.array(a).astype(dtype).reshape(shape)


def containers(a):
    return [("ndarray", a), ("tensor", torch.from_numpy(a))]


def store(dtype):
    return np.dtype(_IMAGE_CODES[np.dtype(dtype)][0])


def exact_ints(t):
    return [int(x) for x in t.reshape(-1).tolist()]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_image_dtype_in_both_containers_and_every_shape(dtype):
    st = store(dtype)
    a2, a3 = sample(dtype), sample(dtype, (3, H, W))
    for kind, x in containers(a2):
        for want in ((H, W), (1, H, W)):                        # a slot; a batch of one, which a 2-D image fills
            t = checked_input(x, dtype, st, want)
            assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and tuple(t.shape) == want, (kind, want)
            assert t.numpy().dtype == st, kind
            assert np.array_equal(t.numpy().reshape(H, W), a2.astype(st)), kind
        with pytest.raises(ValueError, match=r"expected images of shape \(3, 5, 7\), got \(5, 7\)"):
            checked_input(x, dtype, st, (3, H, W))               # ... but not a larger batch
    for kind, x in containers(a3):
        t = checked_input(x, dtype, st, (3, H, W))
        assert tuple(t.shape) == (3, H, W) and np.array_equal(t.numpy(), a3.astype(st)), kind
        with pytest.raises(ValueError, match="expected images of shape"):
            checked_input(x, dtype, st, (H, W))                  # a slot takes one image
    for kind, x in containers(a3[:1]):
        assert tuple(checked_input(x, dtype, st, (1, H, W)).shape) == (1, H, W), kind
        with pytest.raises(ValueError, match="expected images of shape"):
            checked_input(x, dtype, st, (H, W))


@pytest.mark.parametrize("dtype", [d for d in DTYPES if d.kind in "iub"], ids=str)
def test_integer_types_come_back_as_exact_float64(dtype):
    a = sample(dtype)
    for kind, x in containers(a):
        t = checked_input(x, dtype, store(dtype), (H, W))
        if dtype == np.uint8:
            assert t.dtype == torch.uint8
        else:
            assert t.dtype == torch.float64, kind
        assert exact_ints(t) == [int(v) for v in a.reshape(-1)], kind


@pytest.mark.parametrize("dtype", [np.int64, np.uint64], ids=str)
def test_64_bit_integers_up_to_but_not_at_2_to_the_51(dtype):
    dtype = np.dtype(dtype)
    info, f64 = np.iinfo(dtype), np.dtype(np.float64)
    signed = dtype.kind == "i"
    inside = [LIMIT - 1] + ([-(LIMIT - 1)] if signed else [])
    beyond = [LIMIT, LIMIT + 1, info.max] + ([-LIMIT, -(LIMIT + 1), info.min] if signed else [])
    for v in inside:
        a = sample(dtype)
        a[2, 3] = v
        for kind, x in containers(a):
            assert exact_ints(checked_input(x, dtype, f64, (1, H, W))) == [int(e) for e in a.reshape(-1)], (kind, v)
    for v in beyond:
        a = sample(dtype)
        a[4, 6] = v
        for kind, x in containers(a):
            with pytest.raises(NotImplementedError, match=r"64 bit integer images .* below 2\*\*51"):
                checked_input(x, dtype, f64, (1, H, W))
    # the other integer types have no such limit
    for kind, x in containers(sample(np.uint32)):
        assert float(checked_input(x, np.dtype(np.uint32), np.dtype(np.float64), (H, W)).max()) == float(2 ** 32 - 1)


def test_the_three_errors_and_their_order():
    u8, f32, f64 = np.dtype(np.uint8), np.dtype(np.float32), np.dtype(np.float64)
    i64 = np.dtype(np.int64)
    for kind, x in containers(sample(np.float32)):
        with pytest.raises(TypeError, match=r"engine built for uint8 images, got (torch\.)?float32"):
            checked_input(x, u8, u8, (H, W))
        with pytest.raises(TypeError, match="engine built for uint8 images"):       # wrong dtype AND wrong shape: the dtype
            checked_input(x, u8, u8, (H + 1, W))
        with pytest.raises(ValueError, match=r"expected images of shape \(6, 7\), got \(5, 7\)"):
            checked_input(x, f32, f32, (H + 1, W))
    huge = sample(np.int64)
    huge[0, 0] = LIMIT
    for kind, x in containers(huge):
        with pytest.raises(TypeError, match="engine built for float64 images"):     # wrong dtype AND beyond the range
            checked_input(x, f64, f64, (H, W))
        with pytest.raises(ValueError, match="expected images of shape"):            # wrong shape AND beyond the range
            checked_input(x, i64, f64, (1, H, W + 1))
        with pytest.raises(NotImplementedError, match="2\\*\\*51"):
            checked_input(x, i64, f64, (1, H, W))
    with pytest.raises(NotImplementedError, match="no HIP kernel"):                  # (array_dtype: before anything else)
        checked_input(torch.zeros((H, W), dtype=torch.bfloat16), f32, f32, (H, W))
    with pytest.raises(TypeError, match="engine built for float32 images, got complex64"):
        checked_input(np.zeros((H, W), np.complex64), f32, f32, (H, W))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=str)
def test_an_array_of_the_storage_dtype_is_not_copied_unless_it_has_gaps(dtype):
    dtype = np.dtype(dtype)
    a = sample(dtype)
    for want in ((H, W), (1, H, W)):
        assert checked_input(a, dtype, dtype, want).data_ptr() == a.ctypes.data
        t = torch.from_numpy(a)
        assert checked_input(t, dtype, dtype, want).data_ptr() == t.data_ptr()
    wide = sample(dtype, (H, 2 * W))
    gaps = wide[:, ::2]
    assert not gaps.flags["C_CONTIGUOUS"]
    t = checked_input(gaps, dtype, dtype, (1, H, W))
    assert t.is_contiguous() and np.array_equal(t.numpy()[0], gaps)
    assert not np.shares_memory(t.numpy(), wide)
    # an integer image is converted: a new array, the caller's untouched
    b = sample(np.int16)
    keep = b.copy()
    t = checked_input(b, np.dtype(np.int16), np.dtype(np.float64), (H, W))
    assert not np.shares_memory(t.numpy(), b) and np.array_equal(b, keep)
