"""The NMS kernels on the designed box sets of tests/nms_designs.py (proved on the host by test_nms_designs_host.py): planted
suppressions whose one matrix word sits at a chosen scan or spread coordinate, IoUs one rounding from the threshold,
neighbouring ranks made visible, finish batches, and scratch that earlier calls or 0xFF bytes left behind.  Everything goes
through the C ABI (wb_nms_launch, wb_nms_ordered_launch, wb_nms_finish_launch) with the design's own scratch size, the
planted designs also through waldboost_amd.non_max_suppression; flags, counts and guard bytes are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import nms_designs as nd
import waldboost_amd as wb
from nms_reference import nms_keep
from waldboost_amd import _native as nat
from waldboost_amd.boxes import Boxes, nms_keep_mask

pytestmark = pytest.mark.gpu

PLANTED, ORDERS, ROUNDING = nd.planted(), nd.orders(), nd.rounding_cases()
name = lambda d: d.name
GUARD, FILL = 16, 0xA5


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(4, a.dtype)).cuda()


def new_scratch(nbytes, fill=0):
    import torch
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def launch(d, form="rank", scratch=None):
    """One wb_nms_launch / wb_nms_ordered_launch of design d on `scratch` (None: fresh zeros of the design's own size; the
    size handed over is the design's in both cases, so the bands are the design's).  -> (flags int8, UNTOUCHED where the
    pre-filled byte is still there; n_keep)."""
    import torch
    lib, n = nat.load(), d.n
    nbytes = nd.scratch_bytes(n, d.rows)
    if scratch is None:
        scratch = new_scratch(nbytes)
    assert scratch.numel() >= nbytes
    d_boxes, d_scores = dev(d.boxes.reshape(-1)), dev(d.scores)
    d_group = dev(d.group) if d.group is not None else None
    out = torch.full((GUARD + 4 + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    tail = (n, d.iou_t, 0 if d.score_t is None else 1, 0.0 if d.score_t is None else d.score_t, nat.ptr(scratch), nbytes,
            C.c_void_p(out.data_ptr() + GUARD + 4), C.c_void_p(out.data_ptr() + GUARD))
    if form == "ordered":
        d_order = dev(d.order.astype(np.uint32).view(np.int32))
        nat.check(lib.wb_nms_ordered_launch(nat.stream_ptr(), nat.ptr(d_boxes), nat.ptr(d_scores), nat.ptr(d_group), nat.ptr(d_order), *tail),
                  "wb_nms_ordered_launch")
    else:
        nat.check(lib.wb_nms_launch(nat.stream_ptr(), nat.ptr(d_boxes), nat.ptr(d_scores), nat.ptr(d_group), *tail), "wb_nms_launch")
    h = out.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + 4 + n:] == FILL).all(), f"{d.name}: bytes around n_keep | keep[{n}] were written"
    flags = h[GUARD + 4:GUARD + 4 + n]
    assert np.isin(flags, (0, 1, FILL)).all(), f"{d.name}: a flag that is neither 0 nor 1"
    return np.where(flags == FILL, nd.UNTOUCHED, flags).astype(np.int8), int(h[GUARD:GUARD + 4].view(np.uint32)[0])


def check(d, got, where):
    flags, count = got
    assert np.array_equal(flags, d.want), f"{where}: {nd.describe_mismatch(d, flags)}"
    assert count == d.n_keep, f"{where}: {d.name}: n_keep {count}, expected {d.n_keep}"


def launch_finish(cap, fin, n_images, iou_t, scratch=None, fill=0x5A):
    """One wb_nms_finish_launch -> the result bytes [n_images, 16 + cap] of a buffer pre-filled with `fill`."""
    import torch
    lib = nat.load()
    need = C.c_size_t()
    nat.check(lib.wb_nms_finish_scratch_bytes(cap, n_images, C.byref(need)), "wb_nms_finish_scratch_bytes")
    if scratch is None:
        scratch = new_scratch(need.value)
    assert scratch.numel() >= need.value and fin.size == n_images * (16 + 28 * cap)
    d_fin = dev(fin)
    res = torch.full((GUARD + n_images * (16 + cap) + GUARD,), fill, dtype=torch.uint8, device="cuda")
    nat.check(lib.wb_nms_finish_launch(nat.stream_ptr(), nat.ptr(d_fin), cap, n_images, iou_t, 0, 0.0, nat.ptr(scratch), need.value,
                                       C.c_void_p(res.data_ptr() + GUARD)), "wb_nms_finish_launch")
    h = res.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), "bytes around the result were written"
    return h[GUARD:-GUARD].reshape(n_images, 16 + cap)


def test_the_scratch_layout_is_the_librarys():
    lib, need = nat.load(), C.c_size_t()
    for n in (0, 1, 64, 65, 1000, 4096, 4097, nd.BIG_N):
        nat.check(lib.wb_nms_scratch_bytes(n, C.byref(need)), "wb_nms_scratch_bytes")
        assert need.value == nd.scratch_bytes(n), n


# ------------------------------------------------------------------------------ A. planted suppressions
@pytest.mark.parametrize("d", [d for d in PLANTED if "rank" in d.forms], ids=name)
def test_planted_designs_through_wb_nms_launch(d):
    """Fresh scratch, the same scratch again, and scratch full of 0xFF: the same flags and count each time."""
    scratch = new_scratch(nd.scratch_bytes(d.n, d.rows))
    check(d, launch(d, "rank", scratch), "fresh scratch")
    check(d, launch(d, "rank", scratch), "the same scratch again")
    check(d, launch(d, "rank", new_scratch(nd.scratch_bytes(d.n, d.rows), 0xFF)), "scratch of 0xFF bytes")


@pytest.mark.parametrize("d", [d for d in PLANTED if "ordered" in d.forms], ids=name)
def test_planted_designs_through_wb_nms_ordered_launch(d):
    scratch = new_scratch(nd.scratch_bytes(d.n, d.rows), 0xFF)
    check(d, launch(d, "ordered", scratch), "scratch of 0xFF bytes")
    check(d, launch(d, "ordered", scratch), "the same scratch again")


@pytest.mark.parametrize("d", [d for d in PLANTED if "surface" in d.forms], ids=name)
def test_planted_designs_through_non_max_suppression(d):
    bx = Boxes(d.boxes, scores=d.scores, tag=np.arange(d.n))
    out = wb.non_max_suppression(bx, iou_threshold=d.iou_t, score_threshold=d.score_t, group=d.group)
    got = np.zeros(d.n, np.int8)
    got[out.get_field("tag")] = 1
    assert np.array_equal(got, d.want), nd.describe_mismatch(d, got)
    kept = np.flatnonzero(d.want == 1)
    assert np.array_equal(out.get_field("tag"), kept)                                       # input order, every field sliced
    assert np.array_equal(out.get().view(np.uint32), d.boxes[kept].view(np.uint32))
    assert np.array_equal(out.get_field("scores").view(np.uint32), d.scores[kept].view(np.uint32))


# ------------------------------------------------------------------------------ B. one rounding from the threshold
@pytest.mark.parametrize("d", ROUNDING, ids=name)
def test_iou_one_rounding_from_the_threshold(d):
    check(d, launch(d), "wb_nms_launch")


@pytest.mark.parametrize("t", nd.ODD_THRESHOLDS)
def test_non_ordinary_boxes(t):
    """Inverted, empty, infinite, NaN, denormal and huge boxes: the kernel decides as boxes.iou does."""
    boxes, scores = nd.odd_boxes()
    with np.errstate(all="ignore"):
        want = nms_keep(boxes, scores, t)
    d = nd.Design(f"non-ordinary-boxes-t{t}", boxes, scores, np.argsort(-scores, kind="stable"), want.astype(np.int8), t, forms=("rank",))
    check(d, launch(d), "wb_nms_launch")
    check(d, launch(d, "ordered"), "wb_nms_ordered_launch")


# ------------------------------------------------------------------------------ C. the visiting order
@pytest.mark.parametrize("d", [d for d in ORDERS if "rank" in d.forms], ids=name)
def test_neighbouring_ranks_through_the_rank_kernel(d):
    check(d, launch(d), "wb_nms_launch")
    got = nms_keep_mask(d.boxes, d.scores, d.iou_t)
    assert np.array_equal(got.astype(np.int8), d.want), nd.describe_mismatch(d, got)


@pytest.mark.parametrize("d", [d for d in ORDERS if d.forms == ("ordered",)], ids=name)
def test_the_callers_order_is_followed(d):
    """A permutation that is not the score order; entries >= n visit nothing: their boxes' flags stay as they were, nothing
    out of range is written, and the count is the kept boxes'."""
    check(d, launch(d, "ordered"), "wb_nms_ordered_launch")


@pytest.mark.parametrize("d", [d for d in ORDERS if d.forms == ("by_key",)], ids=name)
def test_neighbouring_ranks_by_key_on_the_finish_form(d):
    cap = (d.n + 3) // 4 * 4 + 4
    fin = nd.finish_block(cap, d.keys, d.boxes, d.scores, [d.n, d.n, d.n, 0])
    r = launch_finish(cap, fin, 1, d.iou_t)[0]
    assert np.array_equal(r[16:16 + d.n].astype(np.int8), d.want), nd.describe_mismatch(d, r[16:16 + d.n])
    assert r[:16].view(np.uint32).tolist() == [d.n_keep, d.n, 1, 0] and (r[16 + d.n:] == 0x5A).all()


# ------------------------------------------------------------------------------ D. finish form and stale scratch
def check_finish(cap, images, r, want, where):
    for b, g in enumerate(images):
        d, n = g["design"], g["total"] if g["done"] else 0
        assert r[b, :16].view(np.uint32).tolist() == want[b, :16].view(np.uint32).tolist(), f"{where}: cap {cap} image {b} ({g['total']} boxes): info"
        if g["done"] and d is not None:
            assert np.array_equal(r[b, 16:16 + n], want[b, 16:16 + n]), f"{where}: {nd.describe_mismatch(d, r[b, 16:16 + n])}"
        assert np.array_equal(r[b, 16 + n:], want[b, 16 + n:]), f"{where}: cap {cap} image {b}: bytes behind the {n} flags were written"
    assert np.array_equal(r, want)


@pytest.mark.parametrize("batch", nd.finish_batches(), ids=lambda b: f"cap{b[0]}")
def test_finish_batches(batch):
    cap, images = batch
    fin, want = nd.finish_arrays(cap, images)
    lib, need = nat.load(), C.c_size_t()
    nat.check(lib.wb_nms_finish_scratch_bytes(cap, len(images), C.byref(need)), "wb_nms_finish_scratch_bytes")
    scratch = new_scratch(need.value)
    check_finish(cap, images, launch_finish(cap, fin, len(images), nd.T_PLANT, scratch), want, "fresh scratch")
    check_finish(cap, images, launch_finish(cap, fin, len(images), nd.T_PLANT, scratch), want, "the same scratch again")
    # the batch in reverse on what the first two runs left: every image meets another image's scratch
    rev = images[::-1]
    fin_r, want_r = nd.finish_arrays(cap, rev)
    check_finish(cap, rev, launch_finish(cap, fin_r, len(rev), nd.T_PLANT, scratch), want_r, "another batch's scratch")
    check_finish(cap, images, launch_finish(cap, fin, len(images), nd.T_PLANT, new_scratch(need.value, 0xFF)), want, "scratch of 0xFF bytes")


def test_finish_batches_of_every_capacity_on_one_scratch():
    """The engine's case: one allocation, batches of other capacities and sizes one after the other, nothing cleared."""
    batches = nd.finish_batches()
    lib, need, most = nat.load(), C.c_size_t(), 0
    for cap, images in batches:
        nat.check(lib.wb_nms_finish_scratch_bytes(cap, len(images), C.byref(need)), "wb_nms_finish_scratch_bytes")
        most = max(most, need.value)
    scratch = new_scratch(most)
    for cap, images in [batches[1], batches[0], batches[2], batches[0], batches[1]]:
        fin, want = nd.finish_arrays(cap, images)
        check_finish(cap, images, launch_finish(cap, fin, len(images), nd.T_PLANT, scratch), want, f"after the batches before (cap {cap})")


@pytest.mark.parametrize("fill", [0, 0xFF], ids=["zeros", "0xFF"])
@pytest.mark.parametrize("form", ["rank", "ordered"])
def test_smaller_problems_on_the_scratch_a_larger_one_left(form, fill):
    """n = 8300, then 65, 1 and 0 boxes, then 65 twice more, on one allocation with nothing cleared in between."""
    seq = [nd.by_name("big-a-n8300"), nd.by_name("sprinkle-n65-scores"), nd.by_name("sprinkle-n1-scores"), nd.sprinkle(0, 1)]
    scratch = new_scratch(nd.scratch_bytes(nd.BIG_N), fill)
    for k, d in enumerate(seq + [seq[1], seq[1], seq[0]]):
        check(d, launch(d, form, scratch), f"call {k} on the shared scratch")
