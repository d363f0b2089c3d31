"""ctypes binding of the C ABI declared in include/waldboost_hip.h.

There is no CPU fallback anywhere in this package: if the HIP library has not been
built (``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C
waldboost_amd/csrc``) every compute entry point raises ``RuntimeError``.

How the package calls the library:

* ``call(name, *args)``: ``SYMBOLS[name]`` called and checked under that one name; ``launch(name, *args)``: the same with
  torch's current stream as the first argument.  A torch tensor is passed as its data pointer, ``None`` as the null
  pointer; ints, floats, ``c_void_p``, ``Block.ptr[...]``, ``C.byref(...)`` and ctypes arrays go to ctypes as they are.
  Host NumPy arrays are not converted: the call site writes ``.ctypes.data_as(...)`` and keeps the array alive.
* ``query(name, *args)``: the int a ``*_scratch_bytes`` / ``*_floats`` function writes through its last pointer.
* ``Scratch``: one grow-only byte buffer per device for the callers that keep a scratch across calls.
* ``window_tensor(X, dev)`` / ``window_codes(x)``: float32 or uint8 channel windows staged for a launch, with their
  ``WB_DTYPE_*`` code; ``dtype_name`` and ``is_tensor`` are the two tests behind them.
* ``check``, ``ptr``, ``stream_ptr``, ``load``, ``last_error``: the pieces, for a site that reads a return code itself and
  for hand-written calls in tests and tools.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WB_NATIVE_LIB: A/B timing of two builds of the same ABI in one session (diagnostic)
LIB_PATH = os.environ.get("WB_NATIVE_LIB") or os.path.join(_HERE, "csrc", "libwaldboost_hip.so")

WB_DTYPE_U8, WB_DTYPE_F32, WB_DTYPE_RANK8 = 0, 1, 2
WB_DTYPE_RANK16 = 13
WB_DTYPE_F64, WB_DTYPE_I8, WB_DTYPE_I16, WB_DTYPE_U16, WB_DTYPE_I32, WB_DTYPE_U32 = 3, 4, 5, 6, 7, 8
WB_ERR_INVALID, WB_ERR_HIP, WB_ERR_UNSUPPORTED = -1, -2, -3
WB_DET_SHARDS = 64
WB_DTYPE_I64, WB_DTYPE_U64, WB_DTYPE_BOOL, WB_DTYPE_F16 = 9, 10, 11, 12
WB_CHN_GRAD_HIST, WB_CHN_GRAD_HIST_4_U1, WB_CHN_GRAD_MAG_U1, WB_CHN_GRAD_MAG = 0, 1, 2, 3
WB_ABI_VERSION = 8

# numpy mirrors of the ABI structs (sizes asserted against the header's comments)
LEVEL_DTYPE = np.dtype([
    ("oct", "<i4"), ("src_h", "<i4"), ("src_w", "<i4"), ("nh", "<i4"), ("nw", "<i4"),
    ("u", "<i4"), ("v", "<i4"), ("tap_off", "<i4"), ("src_off", "<i8"), ("chn_off", "<i8"),
    ("sy", "<f8"), ("sx", "<f8")], align=True)
TAP_DTYPE = np.dtype([("i0", "<i4"), ("i1", "<i4"), ("w0", "<f8"), ("w1", "<f8")], align=True)
TILE_DTYPE = np.dtype([("level", "<i4"), ("ty", "<u2"), ("tx", "<u2")], align=True)
PATCH_DTYPE = np.dtype([("r_lo", "<i4"), ("c_lo", "<i4"), ("rows", "<u2"), ("bytes", "<u2"), ("pad", "<u4")], align=True)   # WbTilePatch
DET_DTYPE = np.dtype([("image", "<i4"), ("level", "<i4"), ("r", "<u2"), ("c", "<u2"), ("score", "<f4")], align=True)
assert LEVEL_DTYPE.itemsize == 64 and TILE_DTYPE.itemsize == 8 and DET_DTYPE.itemsize == 16 and TAP_DTYPE.itemsize == 24
assert PATCH_DTYPE.itemsize == 16
FIT_SPLIT_DTYPE = np.dtype([("feature", "<i4"), ("threshold", "<i4"), ("metric", "<f8"), ("t0", "<f8"), ("t1", "<f8")], align=True)   # WbFitSplit
assert FIT_SPLIT_DTYPE.itemsize == 32
WB_FIT_MAX_OPEN = 8
MINE_ROW_DTYPE = np.dtype([("image", "<i4"), ("level", "<i4"), ("r", "<u2"), ("c", "<u2"), ("score", "<f4"), ("best", "<f8"),
                           ("owner", "<i4"), ("label", "<i4")], align=True)   # wb_mine_select_launch's rows
MINE_LEVEL_DTYPE = np.dtype([("chn_off", "<i8"), ("u", "<i4"), ("v", "<i4")], align=True)   # WbMineLevel
assert MINE_ROW_DTYPE.itemsize == 32 and MINE_LEVEL_DTYPE.itemsize == 16
CART_SPLIT_DTYPE = np.dtype([("feature", "<i4"), ("n_left", "<i4"), ("lo", "<f4"), ("hi", "<f4"), ("proxy", "<f8"), ("t0", "<f8"),
                             ("t1", "<f8")], align=True)   # WbCartSplit
assert CART_SPLIT_DTYPE.itemsize == 40
WB_CART_MAX_SAMPLES = 65536
WB_CART_MAX_FEATURES = 65536
WB_GRAM_CHUNK = 256
WB_GRAM_MAX_P = 2048
WB_VOTE_UNIFORM, WB_VOTE_SCORE = 0, 1


class WbModelInfo(C.Structure):
    _fields_ = [("n_stages", C.c_int32), ("depth", C.c_int32), ("m", C.c_int32), ("n", C.c_int32),
                ("C", C.c_int32), ("tile_rows", C.c_int32), ("tile_cols", C.c_int32), ("lds_bytes", C.c_int32),
                ("rank_ok", C.c_int32), ("specialized", C.c_int32), ("rank16_ok", C.c_int32)]


class WbVerifyTrainHyper(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_epsilon", C.c_double),
                ("momentum", C.c_double), ("bn_epsilon", C.c_double), ("dropout", C.c_double), ("seed", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(WbVerifyTrainHyper) == 64

# every symbol include/waldboost_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "wb_abi_version": (C.c_int, []),
    "wb_last_error": (C.c_char_p, []),
    "wb_channels_tile": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "wb_channel_func_info": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "wb_octaves_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_int, _P]),
    "wb_octaves_launch_z": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64,
                                      C.POINTER(C.c_int64), C.c_int, _P, _P, C.c_int]),
    "wb_channels_launch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int,
                                     _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, C.c_int64,
                                     _P, _P, C.c_int64]),
    "wb_channels_launch_x": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int,
                                       _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, C.c_int64,
                                       _P, _P, C.c_int64, _P, C.c_int]),
    "wb_channels_tile_patches": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P]),
    "wb_resize_level_launch": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "wb_pool_smooth_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "wb_grad_hist_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), _P]),
    "wb_grad_mag_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_double, C.c_int, _P, _P]),
    "wb_model_create": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "wb_model_destroy": (C.c_int, [_P]),
    "wb_model_info": (C.c_int, [_P, C.POINTER(WbModelInfo)]),
    "wb_model_specialize": (C.c_int, [_P, C.c_int]),
    "wb_model_use_specialized": (C.c_int, [_P, C.c_int]),
    "wb_jit_compile_check": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int64)]),
    "wb_jit_compile_check2": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int64)]),
    "wb_jit_compile_check3": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int64)]),
    "wb_model_form_rows": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "wb_model_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "wb_rankgroup_create": (C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "wb_rankgroup_model": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "wb_rankgroup_destroy": (C.c_int, [_P]),
    "wb_cascade_launch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P,
                                    C.c_uint32, _P]),
    "wb_cascade_launch_z": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P,
                                      C.c_uint32, _P, _P, C.c_int]),
    "wb_tree_eval_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int64, _P, _P, _P, _P, _P,
                                      C.c_int, _P]),
    "wb_gather_samples_launch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "wb_samples_predict_launch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, _P]),
    "wb_samples_trace_launch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P]),
    "wb_calib_min_launch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_float, _P, _P]),
    "wb_tree_apply_launch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "wb_boxes_launch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_int, _P, _P]),
    "wb_det_pack_launch": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32]),
    "wb_det_finish_launch": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_uint32]),
    "wb_det_finish_sorted_launch": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_uint32, _P,
                                              C.c_uint32]),
    "wb_det_order_batch_launch": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t,
                                            _P, C.c_uint32]),
    "wb_selftest_projection": (C.c_int, [_P, _P]),
    "wb_nms_scratch_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "wb_nms_launch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_double, C.c_int, C.c_float, _P, C.c_size_t, _P, _P]),
    "wb_nms_ordered_launch": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_double, C.c_int, C.c_float, _P, C.c_size_t, _P, _P]),
    "wb_nms_finish_scratch_bytes": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_size_t)]),
    "wb_nms_finish_launch": (C.c_int, [_P, _P, C.c_uint32, C.c_int, C.c_double, C.c_int, C.c_float, _P, C.c_size_t, _P]),
    "wb_match_launch": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int, _P, _P]),
    "wb_vote_launch": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_float, _P, _P]),
    "wb_mine_scratch_bytes": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "wb_mine_select_launch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P, C.c_int, C.c_double,
                                        C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint32, _P, C.c_size_t, _P, C.c_int64, _P]),
    "wb_mine_gather_launch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    "wb_mip_windows_launch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int64, C.c_int, C.c_double, _P, C.c_int64, _P]),
    "wb_mip_scratch_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "wb_mip_prune_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, C.c_float, _P, C.c_size_t, _P, _P, _P]),
    "wb_fit_scratch_bytes": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "wb_fit_level_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P,
                                      C.c_size_t, _P]),
    "wb_fit_route_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int]),
    "wb_cart_sort_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "wb_cart_scratch_bytes": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    "wb_cart_level_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_double,
                                       C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "wb_verify_weights_floats": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wb_verify_scratch_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t)]),
    "wb_verify_launch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "wb_verify_train_param_floats": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wb_verify_train_scratch_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t)]),
    "wb_verify_train_step": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                       _P, _P, C.c_size_t, _P, _P]),
    "wb_gram_scratch_bytes": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    "wb_gram_launch": (C.c_int, [_P, _P, C.c_int, _P, C.c_int64, C.c_int, _P, _P, C.c_size_t]),
    "wb_regress_predict_launch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P]),
    "wb_regress_apply_launch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int64, C.c_int, C.c_int, _P,
                                          _P, _P, _P, _P, _P]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def load():
    """Load libwaldboost_hip.so (once).  torch is imported first so that the library binds to
    the HIP runtime already in the process (same soname) instead of a second copy."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `make -C waldboost_amd/csrc` or __graft_entry__.build()). "
            "waldboost_amd has no CPU fallback.")
    import torch  # noqa: F401  (loads libamdhip64.so.7 that our library resolves against)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.wb_abi_version() != WB_ABI_VERSION:
        raise NativeError("libwaldboost_hip.so ABI version mismatch")
    _lib = lib
    return lib


def last_error():
    """The thread's last error message of the native library (wb_last_error)."""
    return load().wb_last_error().decode("utf-8", "replace")


def check(rc, what=""):
    if rc == 0:
        return
    msg = load().wb_last_error().decode("utf-8", "replace")
    if rc == WB_ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    if rc == WB_ERR_INVALID:
        raise ValueError(f"{what}: {msg}")
    raise NativeError(f"{what}: {msg} (code {rc})")


def require_gpu():
    """The torch device this process computes on; raises when there is no GPU."""
    import torch
    if not torch.cuda.is_available():
        raise NativeError("waldboost_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                          "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def is_tensor(x):
    return type(x).__module__.startswith("torch")


def dtype_name(x):
    """The dtype of an array or a tensor as NumPy names it ('None' for what has none); a dtype, NumPy's or torch's, names itself."""
    return str(getattr(x, "dtype", x if is_tensor(x) or isinstance(x, np.dtype) else None)).replace("torch.", "")


def as_arg(a):
    """What `call` hands to ctypes for argument `a`: a tensor's data pointer (a view's: where the view starts); anything
    else as it is -- None is ctypes' null pointer.  A host NumPy array is not taken here: the caller passes its pointer
    and answers for its lifetime and contiguity."""
    return C.c_void_p(a.data_ptr()) if is_tensor(a) else a


def _argtypes(name):
    if name not in SYMBOLS:
        raise AttributeError(f"{name} is not a symbol of include/waldboost_hip.h")
    return SYMBOLS[name][1]


def call(name, *args):
    """lib.<name>(*args) with tensors passed as their device pointers (as_arg), checked under that same name."""
    _argtypes(name)
    check(getattr(load(), name)(*map(as_arg, args)), name)


def launch(name, *args):
    """`call` of an entry point whose first parameter is the stream: on torch's current one."""
    call(name, stream_ptr(), *args)


def query(name, *args):
    """The size that `name` writes through its last parameter (*_scratch_bytes: size_t, *_floats: int64), as an int."""
    out = _argtypes(name)[-1]._type_()
    call(name, *args, C.byref(out))
    return int(out.value)


class Scratch:
    """One grow-only byte buffer per device, for launches that are ordered on one stream: on(dev, nbytes) is a uint8
    tensor of at least max(nbytes, 16) bytes -- the one of the call before when that is large enough, whatever it held."""

    def __init__(self):
        self._held = {}

    def on(self, dev, nbytes):
        import torch
        have = self._held.get(dev)
        if have is None or have.numel() < nbytes:
            have = self._held[dev] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        return have


def window_codes(x):
    """(torch dtype, WB_DTYPE_* code) of channel windows `x` (ndarray, tensor or their dtype), which the sample kernels take
    as float32 or uint8; None for any other dtype."""
    import torch
    return {"uint8": (torch.uint8, WB_DTYPE_U8), "float32": (torch.float32, WB_DTYPE_F32)}.get(dtype_name(x))


def window_tensor(X, dev):
    """Channel windows X, a float32 or uint8 ndarray or tensor, staged for a launch: (contiguous tensor on `dev` in X's own
    dtype, WB_DTYPE_* code) -- X itself when it is that already; None for any other dtype.  Shapes and finiteness are
    the caller's to check, and so is the exception that None becomes."""
    import torch
    codes = window_codes(X)
    if codes is None:
        return None
    t = X if is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X))
    return t.to(dev).contiguous(), codes[1]


def _spec(part):
    """(shape, dtype) of a Block part: a NumPy array, or the (shape, dtype) of an output."""
    if isinstance(part, np.ndarray):
        return part.shape, part.dtype
    shape, dtype = part
    return shape if isinstance(shape, tuple) else (int(shape),), np.dtype(dtype)


def block_layout(**parts):
    """({name: byte offset}, total bytes) of arrays packed back to back in the order given -- a Block's layout.  A part is
    a NumPy array (an upload) or a (shape, dtype) spec (an output).  Part `name` must land on a multiple of min(16, the bytes
    of one of its rows), a row being everything behind the first axis: what the kernels' float4 / double / int loads need
    and the launch functions refuse to go without.  Nothing is padded: an order that breaks the rule is an AssertionError
    that names the part.  A part without bytes lies anywhere and moves nothing."""
    offsets, at = {}, 0
    for name, part in parts.items():
        shape, dtype = _spec(part)
        row = math.prod(shape[1:]) * dtype.itemsize
        assert shape[0] * row == 0 or at % min(16, row) == 0, \
            f"block part {name!r} ({dtype} rows of {row} bytes) at byte {at} is not {min(16, row)}-byte aligned: order the parts by row size"
        offsets[name] = at
        at += shape[0] * row
    return offsets, at


class Block:
    """Several typed arrays in ONE device allocation (block_layout), so that they travel in one copy: `upload` sends host
    arrays up, `empty` reserves outputs that `host` brings down together.  ptr[name]: the part's device pointer, a
    ctypes.c_void_p (ptr.get(name) of an absent optional part is None, the null pointer to ctypes); tensor(name): a typed
    torch view into the block; host(): ONE .cpu() -> {name: typed, shaped NumPy view of the copy} (copy what outlives it)."""

    def __init__(self, dev, parts, upload):
        import torch
        self.parts = parts
        self.offsets, self.nbytes = block_layout(**parts)
        if upload:
            flat = [a.reshape(-1) for a in parts.values()]                                  # (a copy where `a` is not contiguous)
            self.blob = torch.from_numpy(np.concatenate([p.view(np.uint8) for p in flat])).to(dev)
        else:
            self.blob = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        base = self.blob.data_ptr()
        self.ptr = {k: C.c_void_p(base + o) for k, o in self.offsets.items()}

    @classmethod
    def upload(cls, dev, **arrays):
        return cls(dev, arrays, True)

    @classmethod
    def empty(cls, dev, **specs):
        return cls(dev, specs, False)

    def _part(self, flat, name):
        """(the bytes of part `name` in `flat`, the blob or a copy of it; its shape; its dtype)"""
        shape, dtype = _spec(self.parts[name])
        at = self.offsets[name]
        return flat[at:at + math.prod(shape) * dtype.itemsize], shape, dtype

    def tensor(self, name):
        """Part `name` as a torch view (a structured dtype: its rows as bytes, uint8 [rows, itemsize])."""
        import torch
        b, shape, dtype = self._part(self.blob, name)
        return b.view(-1, dtype.itemsize) if dtype.names else b.view(getattr(torch, dtype.name)).reshape(shape)

    def host(self):
        h = self.blob.cpu().numpy()
        return {k: b.view(dtype).reshape(shape) for k, (b, shape, dtype) in ((k, self._part(h, k)) for k in self.parts)}
