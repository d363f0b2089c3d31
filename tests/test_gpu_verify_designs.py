"""The verification kernels (csrc/wb_verify.hip) on the designs of tests/verify_designs.py, at the C ABI and through
Verifier.predict: equal to the integer expectation bit for bit, whatever the number of windows, wherever a window sits in
the batch, whatever the scratch held before -- and nothing is written behind `out`."""
import ctypes as C

import numpy as np
import pytest
import torch

import verify_designs as vd
import verify_reference as ref
from waldboost_amd import _native as nat
from waldboost_amd import verification as ver

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1), (3, 5, 2), (12, 12, 4), (14, 14, 1), (32, 32, 16)]
MORE_SHAPES = [(14, 14, 4), (20, 20, 4), (13, 32, 9)]          # the usual windows, and one where only a side is at its limit
COUNTS = [0, 1, 63, 64, 65, 257]
GUARD = 64
# where one and the same window is placed: first and last index, either side of a wave of 64, of the GEMM tile of 64 and
# of every front workgroup's pack (1 .. 8 windows)
SAME = [0, 1, 4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 255, 256]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def packed_weights(design):
    layers = ref.fold(design["arrays"], design["epsilon"])
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in layers[:4]] + [v.reshape(-1) for v in layers[4:]])


def launch(shape, weights, X, scores, scratch=None, fill=None):
    """wb_verify_launch on host arrays; returns (out [N], the guard words in front of and behind it)."""
    lib, dev = nat.load(), nat.require_gpu()
    m, n, Cc = shape
    N = int(X.shape[0])
    count, need = C.c_int64(), C.c_size_t()
    nat.check(lib.wb_verify_weights_floats(m, n, Cc, C.byref(count)), "wb_verify_weights_floats")
    assert count.value == weights.size
    nat.check(lib.wb_verify_scratch_bytes(m, n, Cc, N, C.byref(need)), "wb_verify_scratch_bytes")
    wd = torch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(dev)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev) if N else torch.zeros(16, dtype=torch.uint8, device=dev)
    sd = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(dev) if N else torch.zeros(4, device=dev)
    if scratch is None:
        scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=dev)
    if fill is not None:
        scratch.fill_(fill)
    assert scratch.numel() >= need.value
    buf = torch.full((GUARD + N + GUARD,), -12345.0, dtype=torch.float32, device=dev)
    wdt = nat.WB_DTYPE_U8 if X.dtype == np.uint8 else nat.WB_DTYPE_F32
    nat.check(lib.wb_verify_launch(nat.stream_ptr(), nat.ptr(Xd), wdt, N, m, n, Cc, nat.ptr(wd), nat.ptr(sd), nat.ptr(scratch),
                                   scratch.numel(), nat.ptr(buf[GUARD:])), "wb_verify_launch")
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + N], np.concatenate([host[:GUARD], host[GUARD + N:]]), scratch


@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=str)
def test_every_design_at_the_c_abi_and_through_predict(shape):
    for d in vd.designs(shape):
        want, bound, _ = vd.expected(d)
        assert bound < 2 ** 24
        got, guard, _ = launch(shape, packed_weights(d), d["X"], d["scores"])
        assert np.array_equal(bits(got), bits(want)), (d["name"], got, want)
        assert np.all(guard == np.float32(-12345.0)), d["name"]
        V = ver.Verifier.from_keras_weights(shape, d["arrays"], epsilon=d["epsilon"])
        out = V.predict([d["X"], d["scores"]])
        assert out.shape == (want.size, 1) and out.dtype == np.float32
        assert np.array_equal(bits(out[:, 0]), bits(want)), d["name"]
        out = V.predict([torch.from_numpy(d["X"]).cuda(), d["scores"].reshape(-1, 1)], batch_size=2)
        assert np.array_equal(bits(out[:, 0]), bits(want)), d["name"]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", ["mixed", "batchnorm"])
def test_counts_positions_and_scratch_contents(shape, name):
    d = next(d for d in vd.designs(shape) if d["name"] == name)
    want, _, _ = vd.expected(d)
    K, top = want.size, max(COUNTS)
    pick = np.arange(top) % K
    pick[SAME] = 0
    X, H, expect = d["X"][pick], d["scores"][pick], want[pick]
    weights = packed_weights(d)
    scratch = None
    for N in sorted(COUNTS, reverse=True):                 # (the largest first: its scratch serves the others)
        got, guard, scratch = launch(shape, weights, X[:N], H[:N], scratch)
        assert got.shape == (N,) and np.array_equal(bits(got), bits(expect[:N])), (N, name)
        assert np.all(guard == np.float32(-12345.0)), N
    # one scratch twice, then the same scratch filled with 0xFF (NaN features, had anything been left to read)
    first, _, scratch = launch(shape, weights, X, H, scratch)
    again, _, scratch = launch(shape, weights, X, H, scratch)
    dirty, guard, _ = launch(shape, weights, X, H, scratch, fill=0xFF)
    assert np.array_equal(bits(first), bits(expect)) and np.array_equal(bits(again), bits(expect))
    assert np.array_equal(bits(dirty), bits(expect)) and np.all(guard == np.float32(-12345.0))
    same = bits(first)[SAME]
    assert np.all(same == bits(want[0]))


def test_launch_refuses_bad_arguments_on_the_device():
    lib, dev = nat.load(), nat.require_gpu()
    shape = (12, 12, 4)
    d = vd.designs(shape)[0]
    w = torch.from_numpy(packed_weights(d)).to(dev)
    X = torch.zeros((5,) + shape, device=dev)
    s, out, scratch = torch.zeros(5, device=dev), torch.zeros(8, device=dev), torch.zeros(5 * 576 + 4, device=dev)
    args = lambda **k: [k.get("X", nat.ptr(X)), nat.WB_DTYPE_F32, 5, 12, 12, 4, k.get("w", nat.ptr(w)), nat.ptr(s),
                        k.get("scratch", nat.ptr(scratch)), k.get("nbytes", 5 * 576 * 4), k.get("out", nat.ptr(out))]
    assert lib.wb_verify_launch(nat.stream_ptr(), *args()) == 0
    assert lib.wb_verify_launch(nat.stream_ptr(), *args(out=None)) == nat.WB_ERR_INVALID
    assert lib.wb_verify_launch(nat.stream_ptr(), *args(nbytes=5 * 576 * 4 - 4)) == nat.WB_ERR_INVALID
    assert lib.wb_verify_launch(nat.stream_ptr(), *args(scratch=C.c_void_p(scratch.data_ptr() + 4))) == nat.WB_ERR_INVALID
    assert lib.wb_verify_launch(nat.stream_ptr(), *args(w=C.c_void_p(w.data_ptr() + 4))) == nat.WB_ERR_INVALID
    assert lib.wb_verify_launch(nat.stream_ptr(), *args(out=C.c_void_p(out.data_ptr() + 2))) == nat.WB_ERR_INVALID
    torch.cuda.synchronize()
    V = ver.model_cnn((40, 12, 4), seed=0)
    with pytest.raises(NotImplementedError):
        V.predict([np.zeros((2, 40, 12, 4), "f"), np.zeros(2, "f")])
