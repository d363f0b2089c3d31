"""The CART kernels (csrc/wb_cart.hip) on designed inputs, straight at the C ABI (wb_cart_sort_launch,
wb_cart_level_launch; include/waldboost_hip.h).  The sort must give exactly the permutation by (key, index) -- the
composite key makes it deterministic -- on columns of every size around a wave, a workgroup step, the sort's chunk and
the cap.  The level kernels must give, record by record, the winners tests/cart_designs.py plants and
tests/test_cart_designs_host.py proves, proxies and totals bit-equal to the float64 statement (every weight sum is an
integer, every float64 operation is rounded on its own: there is nothing to tolerate), the routed node ids and the
stable partition of every column."""
import ctypes as C

import numpy as np
import pytest

import cart_designs as cd
import cart_reference as cr
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
PAD = 320
CHUNK = 4096
DESIGNS = {d["name"]: d for d in cd.designs()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(nat.require_gpu())


def sort_key(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def gpu_sort(xt):
    import torch
    lib = nat.load()
    F, N = xt.shape
    x = _dev(xt)
    out = torch.full((PAD + F * N * 4 + PAD,), PATTERN, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(lib.wb_cart_sort_launch(nat.stream_ptr(), nat.ptr(x), N, F, C.c_void_p(out.data_ptr() + PAD)), "wb_cart_sort_launch")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:PAD] == PATTERN) and np.all(o[PAD + F * N * 4:] == PATTERN)         # nothing written around the result
    return o[PAD:PAD + F * N * 4].copy().view(np.int32).reshape(F, N)


def columns(N, F, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (F, N)).astype(np.float32)
    x[0, rng.random(N) < 0.3] = np.float32(-0.0)                                          # both zeros, as one value
    x[0, rng.random(N) < 0.3] = np.float32(0.0)
    if F > 1:
        x[1] = np.float32(-3.25)                                                          # all equal
        x[2] = np.sort(rng.integers(-50, 50, N)).astype(np.float32)[::-1] / 8             # reversed, with duplicates
    return x


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK,
                               2 * CHUNK + 1, 24000, nat.WB_CART_MAX_SAMPLES - 1, nat.WB_CART_MAX_SAMPLES])
def test_sort_gives_the_permutation_by_key_and_index(N):
    for F in (1, 3):
        xt = columns(N, F, N + F)
        order = gpu_sort(xt)
        for f in range(F):
            key = sort_key(xt[f])
            want = np.lexsort((np.arange(N), key))
            assert np.array_equal(np.sort(order[f]), np.arange(N)), (N, F, f)            # a permutation
            assert np.all(np.diff(key[order[f]].astype(np.int64)) >= 0), (N, F, f)       # keys do not decrease
            assert np.array_equal(order[f], want), (N, F, f)                             # equal keys by index


def test_sort_refuses_what_it_does_not_hold():
    import torch
    lib = nat.load()
    x = torch.zeros(16, dtype=torch.float32, device=nat.require_gpu())
    o = torch.zeros(16, dtype=torch.int32, device=nat.require_gpu())
    assert lib.wb_cart_sort_launch(nat.stream_ptr(), nat.ptr(x), nat.WB_CART_MAX_SAMPLES + 1, 1, nat.ptr(o)) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_cart_sort_launch(nat.stream_ptr(), nat.ptr(x), 16, 0, nat.ptr(o)) == nat.WB_ERR_INVALID


def launch_level(d, child_base=1):
    """wb_cart_level_launch on a design -> (splits, node, order_in, order_out, begin, end)."""
    import torch
    lib = nat.load()
    dev = nat.require_gpu()
    X, Y, q = d["X"], d["Y"], d["q"]
    N, F = X.shape
    order, begin, end = cd.level_order(d)
    n_open = len(d["nodes"])
    t0 = np.array([sum(int(q[i]) for i in S if Y[i] == 0) for S in d["nodes"]], np.uint64)
    t1 = np.array([sum(int(q[i]) for i in S if Y[i] == 1) for S in d["nodes"]], np.uint64)
    need = C.c_size_t()
    nat.check(lib.wb_cart_scratch_bytes(F, n_open, C.byref(need)), "wb_cart_scratch_bytes")
    xt, q_d, cls_d, oin = _dev(np.ascontiguousarray(X.T)), _dev(q), _dev(Y.astype(np.uint8)), _dev(order)
    node = torch.zeros(N, dtype=torch.int32, device=dev)
    oout = torch.full((PAD + F * N * 4 + PAD,), PATTERN, dtype=torch.uint8, device=dev)
    scratch = torch.full((need.value + PAD,), PATTERN, dtype=torch.uint8, device=dev)
    rec = n_open * nat.CART_SPLIT_DTYPE.itemsize
    out = torch.full((PAD + rec + PAD,), PATTERN, dtype=torch.uint8, device=dev)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    nat.check(lib.wb_cart_level_launch(nat.stream_ptr(), nat.ptr(xt), N, F, nat.ptr(q_d), nat.ptr(cls_d), nat.ptr(oin),
                                       C.c_void_p(oout.data_ptr() + PAD), nat.ptr(node), n_open, hp(begin), hp(end), hp(t0), hp(t1), 1.0,
                                       d["min_leaf"], child_base, nat.ptr(scratch), need.value, C.c_void_p(out.data_ptr() + PAD)),
              "wb_cart_level_launch")
    torch.cuda.synchronize()
    o, oo = out.cpu().numpy(), oout.cpu().numpy()
    assert np.all(o[:PAD] == PATTERN) and np.all(o[PAD + rec:] == PATTERN) and np.all(scratch.cpu().numpy()[need.value:] == PATTERN)
    assert np.all(oo[:PAD] == PATTERN) and np.all(oo[PAD + F * N * 4:] == PATTERN)
    return (o[PAD:PAD + rec].copy().view(nat.CART_SPLIT_DTYPE), node.cpu().numpy(), order,
            oo[PAD:PAD + F * N * 4].copy().view(np.int32).reshape(F, N), begin, end, t0, t1)


@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_level_kernels_give_the_planted_records(name):
    d = DESIGNS[name]
    child_base = 7
    splits, node, order_in, order_out, begin, end, t0, t1 = launch_level(d, child_base)
    X = d["X"]
    want_node = np.zeros(X.shape[0], np.int32)
    for k, S in enumerate(d["nodes"]):
        s, want = splits[k], d["expect"][k]
        assert s["t0"] == float(t0[k]) and s["t1"] == float(t1[k])
        untouched = np.full(end[k] - begin[k], 0xA5A5A5A5, np.uint32).view(np.int32)           # (the fill pattern)
        if want is None:
            assert s["feature"] == -1 and s["n_left"] == 0 and s["proxy"] == -np.inf, (name, k, s)
            assert np.all(order_out[:, begin[k]:end[k]] == untouched)                    # nothing of a leaf moves
            continue
        f, p, lo, hi = want
        stated = cd.statement_winner(d, k)
        assert (int(s["feature"]), int(s["n_left"])) == (f, p), (name, k, s, want)
        assert s["lo"] == lo and s["hi"] == hi, (name, k, s, want)
        assert np.float64(s["proxy"]).view(np.uint64) == np.float64(stated[4]).view(np.uint64), (name, k, s["proxy"], stated[4])
        left = X[S, f].astype(np.float64) <= cr.threshold_of(lo, hi)
        assert int(left.sum()) == p
        want_node[S] = child_base + 2 * k + (~left)
        for c in range(X.shape[1]):                                                      # the stable partition of every column
            seg = order_in[c, begin[k]:end[k]]
            goes = np.isin(seg, S[left])
            assert np.array_equal(order_out[c, begin[k]:end[k]], np.concatenate([seg[goes], seg[~goes]])), (name, k, c)
    assert np.array_equal(node, want_node), name
