"""The kernels of multiple-instance pruning on the designs of tests/mip_designs.py (proved on the host by
test_mip_designs_host.py): at the C ABI (wb_mip_windows_launch, wb_mip_prune_launch) bit for bit against the statement
(tests/mip_reference.py) -- dirty, guarded outputs and scratch, two consecutive calls, shuffled windows, a padded trace,
a capacity one short of the count -- and through the device plumbing of calibration.prune_instances (bag_floor,
prune_launch, prune_trace)."""
import ctypes as C

import numpy as np
import pytest

import mip_designs as md
import mip_reference as ref
from waldboost_amd import _native as nat
from waldboost_amd import calibration

pytestmark = pytest.mark.gpu

WIN = md.window_designs()
PRUNE = md.prune_designs()
GUARD = 64                        # words on either side of an output
FILL = 0x5A5A5A5A
m = n = md.M


def guarded(words):
    """A device buffer of `words` 32-bit words between guards, all holding FILL; (tensor, pointer to the payload)."""
    import torch
    t = torch.full((words + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
    return t, C.c_void_p(t.data_ptr() + 4 * GUARD)


def payload(t, words):
    h = t.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == FILL).all() and (h[GUARD + words:] == FILL).all(), "words around an output were written"
    return h[GUARD:GUARD + words].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------- windows
def ground_truth(d):
    """(gt float64 [n_gt, 4], gt_off int32 [B + 1], ignore uint8 [n_gt]) of a design, on the device."""
    import torch
    gts = [np.zeros((0, 4)) if g is None else g for g in d.gts]
    off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    return (torch.from_numpy(np.concatenate(gts).astype(np.float64)).cuda(), torch.from_numpy(off).cuda(),
            torch.from_numpy(np.concatenate(d.ignores).astype(np.uint8)).cuda())


def windows_call(d, capacity, **over):
    """One wb_mip_windows_launch into a dirty, guarded row buffer -> (rc, n_rows, the rows written as ref.ROW records)."""
    gt, off, ign = ground_truth(d)
    table = np.zeros(len(d.levels), nat.MINE_LEVEL_DTYPE)
    table["u"], table["v"] = [u for u, _ in d.levels], [v for _, v in d.levels]
    table["chn_off"] = -1                                                       # not looked at: no pyramid is read
    inv = np.ascontiguousarray(d.inv_scale, np.float32)
    rows, pr = guarded(8 * capacity)
    cnt, pc = guarded(1)
    k = dict(levels=table.ctypes.data_as(C.c_void_p), inv=inv.ctypes.data_as(C.c_void_p), L=len(d.levels), m=m, n=n, gt=nat.ptr(gt),
             off=nat.ptr(off), ign=nat.ptr(ign), n_gt=int(gt.shape[0]), B=len(d.gts), min_iou=d.min_iou, rows=pr, cap=capacity, cnt=pc)
    k.update(over)
    rc = nat.load().wb_mip_windows_launch(nat.stream_ptr(), k["levels"], k["inv"], k["L"], k["m"], k["n"], k["gt"], k["off"], k["ign"],
                                          k["n_gt"], k["B"], k["min_iou"], k["rows"], k["cap"], k["cnt"])
    if rc != 0:
        return rc, None, None
    total = int(payload(cnt, 1)[0])
    got = payload(rows, 8 * capacity).view(ref.ROW)
    return rc, total, got[:min(total, capacity)]


@pytest.mark.parametrize("name", list(WIN))
def test_windows_on_the_designs(name):
    d = WIN[name]
    want = ref.windows(d.levels, d.inv_scale, m, n, d.gts, d.ignores, d.min_iou)["rows"]
    rc, total, got = windows_call(d, want.size + 3)
    assert rc == 0, nat.last_error()
    assert total == want.size and ref.mref.ordered(got).tobytes() == want.tobytes(), name      # every field, bit for bit
    rc, total2, again = windows_call(d, want.size)                              # exactly enough room; a second call
    assert rc == 0 and total2 == total and ref.mref.ordered(again).tobytes() == want.tobytes()
    # one row short: the full count, and what was written are rows of the statement, each once
    rc, total3, part = windows_call(d, want.size - 1)
    assert rc == 0 and total3 == want.size and part.size == want.size - 1
    known = {w.tobytes() for w in want}
    assert len({w.tobytes() for w in part}) == part.size and all(w.tobytes() in known for w in part)
    rc, total4, none = windows_call(d, 0)                                       # no room at all: the count alone
    assert rc == 0 and total4 == want.size and none.size == 0


def test_windows_without_ground_truth_or_windows_and_error_returns():
    d = WIN["half"]
    rc, total, _ = windows_call(d, 4, n_gt=0, gt=None, ign=None)                # no ground truth: n_rows = 0 without a launch
    assert rc == 0 and total == 0
    rc, total, _ = windows_call(d, 4, L=0)
    assert rc == 0 and total == 0
    rc, total, _ = windows_call(d, 4, m=40, n=56)                               # the window fills the largest level: no window
    assert rc == 0 and total == 0
    for bad in (dict(cnt=None), dict(levels=None), dict(inv=None), dict(gt=None), dict(off=None), dict(ign=None), dict(rows=None),
                dict(L=-1), dict(B=-1), dict(n_gt=-1), dict(cap=-1), dict(m=0), dict(n=0)):
        assert windows_call(d, 4, **bad)[0] == nat.WB_ERR_INVALID, bad
    assert windows_call(d, 4, B=1025)[0] == nat.WB_ERR_UNSUPPORTED
    assert windows_call(d, 4, L=257)[0] == nat.WB_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------- prune
def prune_call(d, floor, order=None, pad=0, **over):
    """One wb_mip_prune_launch on the design's windows in the order `order`, the trace padded to a stride of N + pad, into
    dirty, guarded outputs and scratch -> (rc, theta float32 (T,), removed_at (N,) in the DESIGN's order, counts (2,))."""
    import torch
    order = np.arange(d.N) if order is None else order
    tr = np.full((d.T, d.N + pad), np.nan, np.float32)
    tr[:, :d.N] = d.trace[order].T
    trace, bag = torch.from_numpy(tr).cuda(), torch.from_numpy(d.bag[order]).cuda()
    need = C.c_size_t()
    assert nat.load().wb_mip_scratch_bytes(d.n_bags, C.byref(need)) == 0 and need.value >= 4 * d.n_bags
    scratch, ps = guarded(need.value // 4)
    theta, pt = guarded(d.T)
    rem, pr = guarded(d.N)
    cnt, pc = guarded(2)
    k = dict(trace=nat.ptr(trace), stride=d.N + pad, T=d.T, N=d.N, bag=nat.ptr(bag), n_bags=d.n_bags, scratch=ps, bytes=need.value,
             theta=pt, rem=pr, cnt=pc)
    k.update(over)
    rc = nat.load().wb_mip_prune_launch(nat.stream_ptr(), k["trace"], k["stride"], k["T"], k["N"], k["bag"], k["n_bags"], C.c_float(floor),
                                        k["scratch"], k["bytes"], k["theta"], k["rem"], k["cnt"])
    if rc != 0:
        return rc, None, None, None
    payload(scratch, need.value // 4)
    back = np.empty(d.N, np.int32)
    back[order] = payload(rem, d.N).view(np.int32)
    return rc, payload(theta, d.T).view(np.float32), back, payload(cnt, 2)


@pytest.mark.parametrize("name", list(PRUNE))
def test_prune_on_the_designs(name):
    d = PRUNE[name]
    rng = np.random.default_rng(3)
    for recall in d.recalls:
        floor, _ = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, recall)
        want = ref.prune(d.trace, d.bag, d.n_bags, floor)
        for order, pad in ((None, 0), (None, 0), (rng.permutation(d.N), 0), (np.arange(d.N)[::-1].copy(), 5)):
            rc, theta, removed, counts = prune_call(d, float(floor), order, pad)
            assert rc == 0, nat.last_error()
            assert np.array_equal(bits(theta), bits(want["theta"])), (name, recall, theta, want["theta"])
            assert np.array_equal(removed, want["removed_at"]), (name, recall, np.flatnonzero(removed != want["removed_at"])[:8])
            assert counts.tolist() == [want["retained_bags"], want["surviving"]], (name, recall)
        if recall in d.theta:
            assert np.array_equal(bits(theta), bits(d.theta[recall]))
    # nobody retained: +inf, -1 and zeros; everybody: the prune at the lowest floor
    for floor in (float("inf"), float("nan")):
        rc, theta, removed, counts = prune_call(d, floor)
        assert rc == 0 and np.isposinf(theta).all() and (removed == -1).all() and counts.tolist() == [0, 0]
    want = ref.prune(d.trace, d.bag, d.n_bags, -np.inf)
    rc, theta, removed, counts = prune_call(d, float("-inf"))
    assert rc == 0 and np.array_equal(bits(theta), bits(want["theta"])) and np.array_equal(removed, want["removed_at"])
    assert counts.tolist() == [want["retained_bags"], want["surviving"]] and counts[0] == np.unique(d.bag).size


def test_prune_edges_and_error_returns():
    d = PRUNE["features-257x6"]
    assert prune_call(d, 20.0)[0] == 0
    # a bag id outside [0, n_bags) is never retained and touches nothing
    import copy
    e = copy.copy(d)
    e.bag = d.bag.copy()
    e.bag[256], e.bag[70] = 4, -1
    rc, theta, removed, counts = prune_call(e, 20.0)
    inside = np.flatnonzero((e.bag >= 0) & (e.bag < 4))
    want = ref.prune(d.trace[inside], d.bag[inside], 4, 20.0)
    assert rc == 0 and np.array_equal(bits(theta), bits(want["theta"])) and np.array_equal(removed[inside], want["removed_at"])
    assert removed[256] == -1 and removed[70] == -1 and counts.tolist() == [want["retained_bags"], want["surviving"]]
    # no windows, no stages or no bags: +inf, -1 and zeros without a kernel, whatever the buffers held
    rc, theta, removed, counts = prune_call(d, 20.0, N=0, stride=0, trace=None, bag=None, rem=None, scratch=None, bytes=0)
    assert rc == 0 and np.isposinf(theta).all() and counts.tolist() == [0, 0] and (removed.view(np.uint32) == FILL).all()
    rc, theta, removed, counts = prune_call(d, 20.0, n_bags=0, scratch=None, bytes=0)
    assert rc == 0 and np.isposinf(theta).all() and counts.tolist() == [0, 0] and (removed == -1).all()
    rc, theta, removed, counts = prune_call(d, 20.0, T=0, theta=None)
    assert rc == 0 and counts.tolist() == [0, 0] and (removed == -1).all() and (theta.view(np.uint32) == FILL).all()
    for bad in (dict(trace=None), dict(bag=None), dict(scratch=None), dict(theta=None), dict(rem=None), dict(cnt=None), dict(N=-1),
                dict(T=-1), dict(n_bags=-1), dict(stride=d.N - 1), dict(bytes=4 * d.n_bags - 1), dict(stride=2 ** 31)):
        assert prune_call(d, 20.0, **bad)[0] == nat.WB_ERR_INVALID, bad
    size = C.c_size_t()
    assert nat.load().wb_mip_scratch_bytes(-1, C.byref(size)) == nat.WB_ERR_INVALID
    assert nat.load().wb_mip_scratch_bytes(5, None) == nat.WB_ERR_INVALID


@pytest.mark.parametrize("name", list(PRUNE))
def test_python_surface_on_the_designs(name):
    import torch
    d = PRUNE[name]
    trace = torch.from_numpy(np.ascontiguousarray(d.trace.T)).cuda()
    bag = torch.from_numpy(d.bag).cuda()
    for recall in d.recalls:
        floor, keep = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, recall)
        got_floor, got_keep = calibration.bag_floor(trace[d.T - 1], bag, d.n_bags, recall)
        assert got_keep == keep and np.array_equal(bits(got_floor.cpu().numpy()), bits([floor]))
        want = ref.prune(d.trace, d.bag, d.n_bags, floor, margin=0.375)
        theta, fl, retained, surviving, removed = calibration.prune_trace(trace, bag, d.n_bags, recall, margin=0.375)
        assert theta.dtype == np.float32 and np.array_equal(bits(theta), bits(want["theta"])) and bits([fl])[0] == bits([floor])[0]
        assert (retained, surviving) == (want["retained_bags"], want["surviving"]) and retained >= keep
        assert np.array_equal(removed.cpu().numpy(), want["removed_at"])
    bad = trace.clone()
    bad[d.T - 1, 0] = float("inf")
    with pytest.raises(ValueError):
        calibration.prune_trace(bad, bag, d.n_bags, 1.0)
