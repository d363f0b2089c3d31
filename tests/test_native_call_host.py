"""CPU tests of the binding conventions in waldboost_amd/_native.py: `call` (one name for the call and its error), the
argument conversion behind it, `query` (the size-out entry points), `Scratch` and `window_tensor`.  The library loads
without a GPU; every entry point called here answers before it touches HIP."""
import ctypes as C

import numpy as np
import pytest
import torch

from waldboost_amd import _native as nat

CPU = torch.device("cpu")

# one small argument set per size query of the ABI
QUERIES = {
    "wb_nms_scratch_bytes": (7,),
    "wb_nms_finish_scratch_bytes": (64, 2),
    "wb_mine_scratch_bytes": (100, 2, 3),
    "wb_mip_scratch_bytes": (5,),
    "wb_fit_scratch_bytes": (90, 1),
    "wb_cart_scratch_bytes": (90, 1),
    "wb_verify_weights_floats": (5, 6, 3),
    "wb_verify_scratch_bytes": (5, 6, 3, 8),
    "wb_verify_train_param_floats": (5, 6, 3),
    "wb_verify_train_scratch_bytes": (5, 6, 3, 4),
    "wb_gram_scratch_bytes": (256, 90),
}


def _size_symbols():
    return sorted(name for name in nat.SYMBOLS if name.endswith(("_scratch_bytes", "_floats")))


# ---------------------------------------------------------------------------------------------- call
def test_call_names_the_symbol_it_called_in_a_value_error():
    out = C.c_size_t()
    with pytest.raises(ValueError) as e:
        nat.call("wb_nms_scratch_bytes", -1, C.byref(out))
    assert str(e.value).startswith("wb_nms_scratch_bytes: ")


def test_call_turns_unsupported_into_not_implemented():
    out = C.c_size_t()
    with pytest.raises(NotImplementedError) as e:
        nat.call("wb_nms_scratch_bytes", 1 << 40, C.byref(out))            # more boxes than one call takes
    assert str(e.value).startswith("wb_nms_scratch_bytes: ")


def test_call_returns_nothing_and_fills_the_out_parameter_on_success():
    out = (C.c_int32 * 4)()
    assert nat.call("wb_model_geometry", 8, 2, 8, 8, 4, nat.WB_DTYPE_U8, out) is None
    assert out[1] >= 1 and out[2] >= 1


def test_call_of_an_unknown_name_fails_at_the_call():
    with pytest.raises(AttributeError):
        nat.call("wb_no_such_entry_point", 1)
    with pytest.raises(AttributeError):
        nat.query("wb_no_such_scratch_bytes", 1)
    with pytest.raises(AttributeError):
        nat.call("printf", b"x")                        # in the process, but no symbol of the ABI: it has no argtypes


def test_call_passes_none_as_the_null_pointer():
    with pytest.raises(ValueError) as e:
        nat.call("wb_nms_scratch_bytes", 7, None)
    assert "null pointer" in str(e.value)


# ---------------------------------------------------------------------------------------------- conversion
def test_a_tensor_becomes_its_data_pointer():
    t = torch.arange(10, dtype=torch.float32)
    a = nat.as_arg(t)
    assert isinstance(a, C.c_void_p) and a.value == t.data_ptr()


def test_a_slice_becomes_the_offset_pointer():
    t = torch.arange(10, dtype=torch.float32)
    assert nat.as_arg(t[3:]).value == t.data_ptr() + 3 * 4
    u = torch.zeros((4, 6), dtype=torch.uint8)
    assert nat.as_arg(u[2, 1:]).value == u.data_ptr() + 2 * 6 + 1


def test_none_becomes_null():
    assert nat.as_arg(None) is None                     # what ctypes passes as NULL for every pointer argtype
    assert C.c_void_p(nat.as_arg(None)).value is None


def test_ctypes_values_ints_and_floats_pass_through():
    p, ref, arr = C.c_void_p(1234), C.byref(C.c_int()), (C.c_int64 * 2)(1, 2)
    for a in (p, ref, arr, 7, 0.5, C.c_float(1.5)):
        assert nat.as_arg(a) is a


def test_a_host_array_is_not_converted():
    a = np.zeros(3, np.float32)
    assert nat.as_arg(a) is a                           # the caller passes .ctypes.data_as itself
    with pytest.raises(C.ArgumentError):
        nat.call("wb_nms_scratch_bytes", 7, a)


# ---------------------------------------------------------------------------------------------- query
def test_the_query_table_covers_every_size_symbol():
    assert sorted(QUERIES) == _size_symbols()


def test_every_size_symbol_ends_in_a_pointer_type_query_understands():
    for name in _size_symbols():
        res, args = nat.SYMBOLS[name]
        assert res is C.c_int
        assert args[-1] in (C.POINTER(C.c_size_t), C.POINTER(C.c_int64)), name
        assert args[-1] is C.POINTER(C.c_size_t if name.endswith("_bytes") else C.c_int64), name


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_query_equals_the_hand_written_call(name):
    args = QUERIES[name]
    out = (C.c_size_t if name.endswith("_bytes") else C.c_int64)()
    assert getattr(nat.load(), name)(*args, C.byref(out)) == 0, nat.last_error()
    got = nat.query(name, *args)
    assert type(got) is int and got == out.value and got > 0


def test_query_raises_like_call():
    with pytest.raises(ValueError) as e:
        nat.query("wb_nms_scratch_bytes", -1)
    assert str(e.value).startswith("wb_nms_scratch_bytes: ")


# ---------------------------------------------------------------------------------------------- dtype_name, is_tensor
def test_dtype_name_and_is_tensor():
    assert nat.dtype_name(np.zeros(1, np.uint8)) == "uint8" and nat.dtype_name(torch.zeros(1)) == "float32"
    assert nat.dtype_name(torch.int16) == "int16" and nat.dtype_name(np.dtype(np.float64)) == "float64"
    assert nat.dtype_name([1, 2]) == "None" and nat.dtype_name(None) == "None"
    assert nat.is_tensor(torch.zeros(1)) and not nat.is_tensor(np.zeros(1)) and not nat.is_tensor(None)
    from waldboost_amd import _grow, compare
    assert compare.dtype_name is nat.dtype_name and _grow.is_tensor is nat.is_tensor


# ---------------------------------------------------------------------------------------------- window_tensor
@pytest.mark.parametrize("np_dtype,tdtype,code", [(np.float32, torch.float32, nat.WB_DTYPE_F32), (np.uint8, torch.uint8, nat.WB_DTYPE_U8)])
def test_window_tensor_stages_arrays_and_tensors(np_dtype, tdtype, code):
    rng = np.random.default_rng(3)
    X = (rng.random((4, 5, 6, 3)) * 200).astype(np_dtype)
    assert nat.window_codes(X) == (tdtype, code) and nat.window_codes(torch.from_numpy(X)) == (tdtype, code)
    for given in (X, torch.from_numpy(X.copy())):
        t, c = nat.window_tensor(given, CPU)
        assert c == code and t.dtype == tdtype and t.is_contiguous() and t.device == CPU
        assert np.array_equal(t.numpy(), X)
    # a non-contiguous view comes back contiguous, with the view's values
    for view in (X[:, ::2], torch.from_numpy(X.copy())[:, :, 1:4], X.transpose(0, 2, 1, 3)):
        assert not (view.is_contiguous() if nat.is_tensor(view) else view.flags["C_CONTIGUOUS"])
        t, c = nat.window_tensor(view, CPU)
        assert c == code and t.is_contiguous() and np.array_equal(t.numpy(), np.asarray(view))
    # a tensor that fits already is the result
    fits = torch.from_numpy(X.copy())
    assert nat.window_tensor(fits, CPU)[0] is fits


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.bool_])
def test_window_tensor_refuses_other_dtypes(dtype):
    X = np.zeros((2, 5, 6, 3), dtype)
    assert nat.window_tensor(X, CPU) is None and nat.window_tensor(torch.from_numpy(X), CPU) is None
    assert nat.window_codes(X) is None


# ---------------------------------------------------------------------------------------------- Scratch
def test_scratch_grows_and_never_shrinks():
    s = nat.Scratch()
    big = s.on(CPU, 1000)
    assert big.dtype == torch.uint8 and big.device == CPU and big.numel() >= 1000
    small = s.on(CPU, 10)
    assert small is big and small.data_ptr() == big.data_ptr() and small.numel() >= 1000
    bigger = s.on(CPU, 5000)
    assert bigger.numel() >= 5000 and bigger is not big
    assert s.on(CPU, 5000) is bigger and s.on(CPU, 1) is bigger


def test_scratch_of_nothing_is_sixteen_bytes_and_holders_are_separate():
    s = nat.Scratch()
    assert s.on(CPU, 0).numel() >= 16
    assert nat.Scratch().on(CPU, 0) is not s.on(CPU, 0)
