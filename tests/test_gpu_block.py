"""The packed device block (_native.Block) on the GPU: one upload handed out as pointers and typed views, one allocation of
outputs read back as typed arrays, the null pointer of a part that is not there."""
import ctypes as C

import numpy as np
import pytest
import torch

from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu


def parts():
    rng = np.random.default_rng(3)
    levels = np.zeros(2, nat.LEVEL_DTYPE)
    levels.view(np.uint8)[:] = rng.integers(0, 256, levels.nbytes)
    return dict(doubles=rng.normal(size=(3, 4)), levels=levels, ints=rng.integers(-9, 9, 3).astype(np.int32),
                flags=rng.integers(0, 256, 5).astype(np.uint8))


def test_upload_hands_out_pointers_and_typed_views():
    src = parts()
    blk = nat.Block.upload(nat.require_gpu(), **src)
    offsets, total = nat.block_layout(**src)
    assert blk.blob.is_cuda and blk.blob.dtype == torch.uint8 and blk.blob.numel() == total == 241
    for k, a in src.items():
        assert isinstance(blk.ptr[k], C.c_void_p) and blk.ptr[k].value == blk.blob.data_ptr() + offsets[k]
        t = blk.tensor(k)
        assert t.data_ptr() == blk.ptr[k].value
        if a.dtype.names:                                                        # a struct has no torch dtype: its rows as bytes
            assert tuple(t.shape) == (2, 64) and np.array_equal(t.cpu().numpy(), a.view(np.uint8).reshape(2, 64))
        else:
            assert tuple(t.shape) == a.shape and str(t.dtype) == "torch." + a.dtype.name and np.array_equal(t.cpu().numpy(), a)
    host = blk.host()
    assert list(host) == list(src)
    for k, a in src.items():
        assert host[k].dtype == a.dtype and host[k].shape == a.shape and host[k].tobytes() == a.tobytes()


def test_empty_is_filled_through_its_views_and_read_back_typed():
    src = parts()
    del src["levels"]
    blk = nat.Block.empty(nat.require_gpu(), **{k: (a.shape, a.dtype) for k, a in src.items()})
    assert blk.blob.numel() == nat.block_layout(**src)[1]
    for k, a in src.items():
        blk.tensor(k).copy_(torch.from_numpy(a))
    host = blk.host()
    for k, a in src.items():
        assert host[k].dtype == a.dtype and host[k].shape == a.shape and np.array_equal(host[k], a)


def test_an_absent_optional_part_is_the_null_pointer():
    blk = nat.Block.upload(nat.require_gpu(), boxes=np.zeros((2, 4), np.float32), scores=np.zeros(2, np.float32))
    assert blk.ptr.get("group") is None and C.c_void_p(blk.ptr.get("group")).value is None     # ctypes' NULL
    assert blk.ptr.get("scores").value == blk.blob.data_ptr() + 32
    with pytest.raises(KeyError):
        blk.ptr["group"]
