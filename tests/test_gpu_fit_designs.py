"""The split-search kernels (csrc/wb_fit.hip) on designed inputs, straight at the C ABI (wb_fit_level_launch,
wb_fit_route_launch; include/waldboost_hip.h): tests/fit_designs.py plants which (feature, threshold) wins in every open
node, tests/test_fit_designs_host.py proves the designs from the references alone, and here the kernels must give the planted
answer exactly -- the smallest tied threshold, the first tied entry of A, the NaN rule -- with class totals that are
bit-equal to the integer sums and a metric within 16 * d of the extended-precision table (d: fit_designs.yardstick_deviation,
the float64 rounding of the metric's arithmetic as measured between the two references, never taken from the kernel; 16
for the device's log2: up to 2 ulp where the host's is under 1, six calls per metric, every entropy at most 1)."""
import ctypes as C

import numpy as np
import pytest

import fit_designs as fd
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
PAD = 320                          # surplus bytes behind the scratch, and on both sides of the splits


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(nat.require_gpu())


def _slot_p(slot):
    slot = np.ascontiguousarray(slot, np.int8)
    return slot, slot.ctypes.data_as(C.c_void_p)


def launch(d, slot=None, A=None, padded=False):
    """wb_fit_level_launch on a design -> splits (FIT_SPLIT_DTYPE [n_open]); slot / A override the design's.  padded: also
    returns the bytes around the splits and behind the scratch, which were filled with PATTERN."""
    import torch
    lib = nat.load()
    slot, slot_p = _slot_p(d.slot if slot is None else slot)
    A = np.ascontiguousarray(d.A if A is None else A, np.int32)
    n_open = int((slot >= 0).sum())
    F, N = d.xt.shape
    need = C.c_size_t()
    nat.check(lib.wb_fit_scratch_bytes(A.size, n_open, C.byref(need)), "wb_fit_scratch_bytes")
    dev = nat.require_gpu()
    xt, q, cls, node, A_d = _dev(d.xt), _dev(d.q), _dev(d.cls), _dev(d.node), _dev(A)
    scratch = torch.full((need.value + PAD,), PATTERN, dtype=torch.uint8, device=dev)
    rec = n_open * nat.FIT_SPLIT_DTYPE.itemsize
    out = torch.full((PAD + rec + PAD,), PATTERN, dtype=torch.uint8, device=dev)
    assert PAD % 16 == 0 and scratch.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    nat.check(lib.wb_fit_level_launch(nat.stream_ptr(), nat.ptr(xt), N, F, nat.ptr(q), nat.ptr(cls), nat.ptr(node), d.level_base,
                                      slot.size, slot_p, n_open, nat.ptr(A_d), A.size, nat.ptr(scratch), need.value,
                                      C.c_void_p(out.data_ptr() + PAD)), "wb_fit_level_launch")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    splits = o[PAD:PAD + rec].copy().view(nat.FIT_SPLIT_DTYPE)
    if padded:
        return splits, np.concatenate([o[:PAD], o[PAD + rec:]]), scratch.cpu().numpy()[need.value:]
    return splits


def route(d, splits, slot=None):
    """wb_fit_route_launch with child_base = level_base + n_level -> the new node ids."""
    import torch
    lib = nat.load()
    slot, slot_p = _slot_p(d.slot if slot is None else slot)
    F, N = d.xt.shape
    xt, node = _dev(d.xt), _dev(d.node)
    sp = _dev(np.ascontiguousarray(splits))
    nat.check(lib.wb_fit_route_launch(nat.stream_ptr(), nat.ptr(xt), N, F, nat.ptr(node), d.level_base, slot.size, slot_p,
                                      int((slot >= 0).sum()), nat.ptr(sp), d.level_base + slot.size), "wb_fit_route_launch")
    torch.cuda.synchronize()
    return node.cpu().numpy().view(np.int32)


def routed(d, splits):
    """What wb_fit_route_launch must leave in node, in NumPy."""
    want = d.node.copy()
    for s in range(d.n_open):
        S = d.samples(s)
        right = d.xt[int(splits["feature"][s]), S].astype(np.int64) > int(splits["threshold"][s])
        want[S] = d.level_base + d.n_level + 2 * s + right
    return want


def _bits(x):
    return np.array([x], np.float64).view(np.uint64)[0]


_WORST = {}


def check_splits(d, splits):
    """The per-slot assertions of a launch; returns the largest |metric - extended reference|."""
    tol = 16 * fd.yardstick_deviation()
    worst = 0.0
    for s, ex in enumerate(fd.exact_tables(d)):
        f, t, is_nan = d.expected(s)
        got = splits[s]
        assert (int(got["feature"]), int(got["threshold"])) == (f, t), (d.name, s, got, (f, t))
        assert _bits(got["t0"]) == _bits(float(ex["T0i"]) * fd.SCALE), (d.name, s, got["t0"], ex["T0i"])
        assert _bits(got["t1"]) == _bits(float(ex["T1i"]) * fd.SCALE), (d.name, s, got["t1"], ex["T1i"])
        assert bool(np.isnan(got["metric"])) == is_nan, (d.name, s, got["metric"])
        if not is_nan:
            k = int(np.flatnonzero(d.A == f)[0])
            dev = float(abs(got["metric"] - ex["table"][k, t]))
            worst = max(worst, dev)
            assert dev <= tol, (d.name, s, float(got["metric"]), dev, tol)
    return worst


@pytest.mark.parametrize("name", sorted(fd.CASES))
def test_design_gets_its_planted_split(name):
    d = fd.design(name)
    worst = check_splits(d, launch(d))
    _WORST[name] = worst
    print(f"{name}: largest |kernel - extended reference| {worst:.3g} (tolerance {16 * fd.yardstick_deviation():.3g}; "
          f"over the designs so far {max(_WORST.values()):.3g})")


@pytest.mark.parametrize("name", ["eight_nodes", "leaves_between"])
def test_a_node_does_not_depend_on_its_neighbours(name):
    """Every slot's whole record, as bytes, against a launch with that node as the level's only open one."""
    d = fd.design(name)
    full = launch(d)
    for s in range(d.n_open):
        alone = np.full(d.n_level, -1, np.int8)
        alone[np.flatnonzero(d.slot == s)[0]] = 0
        one = launch(d, slot=alone)
        assert one.size == 1 and one.tobytes() == full[s:s + 1].tobytes(), (name, s, one, full[s])


@pytest.mark.parametrize("name", ["eight_nodes", "full_bits"])
def test_records_do_not_depend_on_sample_order_or_run(name):
    d = fd.design(name)
    first = launch(d)
    p = d.permuted(np.random.default_rng(3).permutation(d.q.size))
    assert not np.array_equal(p.node, d.node) or not np.array_equal(p.q, d.q)
    for other in (launch(p), launch(p), launch(d)):
        assert other.tobytes() == first.tobytes(), name


@pytest.mark.parametrize("name", ["eight_nodes", "leaves_between", "nan_beside_normal[weightless]", "planted[257-dup_first]"])
def test_route_moves_open_samples_only(name):
    d = fd.design(name)
    splits = launch(d)
    check_splits(d, splits)
    got, want = route(d, splits), routed(d, splits)
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:10])
    is_open = np.isin(d.node, [d.node_of(s) for s in range(d.n_open)])
    assert np.array_equal(got[~is_open], d.node[~is_open]) and got[is_open].min() >= d.level_base + d.n_level
    for s in range(d.n_open):                                                    # both children of a rated node hold samples
        if d.want[s] != fd.NAN_NODE:
            g = got[d.samples(s)] - (d.level_base + d.n_level + 2 * s)
            assert set(g.tolist()) == {0, 1}, (name, s)


def test_route_on_handwritten_splits():
    """t = 256 sends a node's samples left, t = -1 right, t = a column's xmin exactly the xmin samples left; on permuted
    slots, between leaves and foreign nodes."""
    d = fd.design("leaves_between")
    splits = np.zeros(d.n_open, nat.FIT_SPLIT_DTYPE)
    f_min = 4
    S3 = d.samples(3)
    xmin = int(d.xt[f_min, S3].min())
    splits["feature"] = [2, 9, 0, f_min]
    splits["threshold"] = [256, -1, 255, xmin]
    splits["metric"] = np.nan
    got = route(d, splits)
    assert np.array_equal(got, routed(d, splits))
    base = d.level_base + d.n_level
    assert np.all(got[d.samples(0)] == base) and np.all(got[d.samples(1)] == base + 3) and np.all(got[d.samples(2)] == base + 4)
    left = S3[d.xt[f_min, S3] == xmin]
    assert 1 <= left.size < S3.size and np.array_equal(S3[got[S3] == base + 6], left)
    assert np.array_equal(S3[got[S3] == base + 7], np.setdiff1d(S3, left))        # (22 is also a foreign node's id: untouched)
    by = ~np.isin(d.node, [d.node_of(s) for s in range(d.n_open)])
    assert by.sum() >= 300 and np.array_equal(got[by], d.node[by])
    # the same through eight permuted slots: a slot's children follow the SLOT, not the node's place in the level
    e = fd.design("eight_nodes")
    sp = np.zeros(8, nat.FIT_SPLIT_DTYPE)
    sp["feature"] = np.arange(8)
    sp["threshold"] = [256, -1] * 4
    got = route(e, sp)
    for s in range(8):
        assert np.all(got[e.samples(s)] == 15 + 2 * s + s % 2), s


def test_launch_writes_nothing_beside_its_scratch_and_splits():
    """257 entries of A and 3 open nodes (a record block that is no multiple of 16 bytes): the bytes behind
    wb_fit_scratch_bytes and on both sides of the three split records keep their pattern."""
    d = fd.design("three_wide")
    splits, around, behind = launch(d, padded=True)
    check_splits(d, splits)
    assert around.size == 2 * PAD and np.all(around == PATTERN)
    assert behind.size == PAD and np.all(behind == PATTERN)
