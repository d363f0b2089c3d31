"""The mining kernels on the designs of tests/mine_designs.py (proved on the host by test_mine_designs_host.py), at the C ABI
(wb_mine_select_launch, wb_mine_gather_launch): the chosen rows, put in (image, level, r, c) order, bit for bit against the
statement (tests/mine_reference.py); a dirty scratch reused across calls, guard words around the outputs, the error returns."""
import ctypes as C

import numpy as np
import pytest

import mine_designs as md
import mine_reference as ref
from waldboost_amd import _native as nat
from waldboost_amd import samples

pytestmark = pytest.mark.gpu

GUARD = 16                        # rows (select) / crops' worth of bytes (gather) on either side of an output
FILL = 0x5A


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if a.size else np.zeros(16, a.dtype)).view(np.uint8).reshape(-1)).cuda()


_dirty = {}


def dirty_scratch(nbytes):
    """One scratch buffer for all scenes, grown as needed and never cleaned: every call finds what the last one left (the
    first finds 0xFF bytes)."""
    import torch
    if "t" not in _dirty or _dirty["t"].numel() < nbytes:
        _dirty["t"] = torch.full((max(nbytes, 1 << 20),), 0xFF, dtype=torch.uint8, device="cuda")
    return _dirty["t"]


def scene_arrays(s):
    gts = [g if g is not None else np.zeros((0, 4)) for g in s.gts]
    gt = np.concatenate(gts).reshape(-1, 4) if gts else np.zeros((0, 4))
    off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    ign = np.concatenate(s.ignores).astype(np.uint8) if s.ignores else np.zeros(0, np.uint8)
    return gt, off, ign


def select(s, det=None, capacity=None, gt_off=None):
    """One wb_mine_select_launch on scene `s` -> (rc, rows in arrival order or None), guards checked."""
    import torch
    lib, p = nat.load(), s.params
    det = s.det if det is None else det
    n_det, B, L = int(det.size), s.n_images, len(s.inv_scale)
    gt, off, ign = scene_arrays(s)
    off = off if gt_off is None else np.asarray(gt_off, np.int32)
    k = lambda want, cap: min(int(cap), n_det) if want else 0
    room = min(n_det, B * L * (k(p["want_tp"], p["max_tp"]) + k(p["want_fp"], p["max_fp"]))) if capacity is None else capacity
    need = C.c_size_t()
    nat.check(lib.wb_mine_scratch_bytes(n_det, B, L, C.byref(need)), "wb_mine_scratch_bytes")
    scratch = dirty_scratch(need.value)
    d = [dev(x) for x in (det, s.inv_scale, gt, off, ign, s.serial)]
    out = torch.full(((2 * GUARD + room) * 32,), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = lib.wb_mine_select_launch(nat.stream_ptr(), nat.ptr(d[0]), n_det, nat.ptr(d[1]), L, s.m, s.n, nat.ptr(d[2]), nat.ptr(d[3]),
                                   nat.ptr(d[4]), len(gt), nat.ptr(d[5]), B, float(p["min_tp_iou"]), float(p["max_fp_iou"]),
                                   int(p["max_tp"]), int(p["max_fp"]), int(p["want_tp"]), int(p["want_fp"]), int(p["seed"]),
                                   nat.ptr(scratch), need.value, C.c_void_p(out.data_ptr() + 32 * GUARD), room,
                                   C.c_void_p(cnt.data_ptr() + 4))
    if rc != 0:
        return rc, None
    h, hc = out.cpu().numpy(), cnt.cpu().numpy()
    assert hc[0] == hc[2] == 0x5A5A5A5A, "words around the counter were written"
    n = int(hc[1]) if n_det else 0
    assert n <= room
    assert (h[:32 * GUARD] == FILL).all() and (h[32 * (GUARD + n):] == FILL).all(), "rows around the chosen ones were written"
    return rc, h[32 * GUARD: 32 * (GUARD + n)].view(ref.ROW).copy()


def describe(s, got, want):
    a, b = md.chosen_of(got), md.chosen_of(want)
    return (f"{s.name}: {len(got)} rows, want {len(want)}; missing {sorted(set(b) - set(a))[:5]}, unexpected {sorted(set(a) - set(b))[:5]}, "
            f"other label / owner {[(k, a[k], b[k]) for k in sorted(set(a) & set(b)) if a[k] != b[k]][:5]}")


@pytest.mark.parametrize("name", list(md.scenes()))
def test_select_on_the_designs(name):
    s = md.scenes()[name]
    want = s.reference()["rows"]
    rc, got = select(s)
    assert rc == 0, nat.last_error()
    got = ref.ordered(got)
    assert md.chosen_of(got) == s.expect, describe(s, got, want)
    assert got.tobytes() == want.tobytes(), describe(s, got, want)


def test_rows_are_ordered_on_the_device_by_order_rows():
    """The caller's ordering step (samples.order_rows) on the rows of a shuffled scene."""
    import torch
    s = md.scenes()["sized-1025"]
    _, got = select(s)
    rows = torch.from_numpy(got.view(np.int32).reshape(-1, 8).copy()).cuda()
    assert samples.order_rows(rows).cpu().numpy().tobytes() == s.reference()["rows"].tobytes()


def test_the_answer_does_not_depend_on_the_record_order():
    s = md.scenes()["select-fp-K4"]
    want = s.reference()["rows"]
    for order in (np.argsort(s.det, order=("image", "level", "r", "c")), np.arange(s.det.size)[::-1]):
        _, got = select(s, det=s.det[order])
        assert ref.ordered(got).tobytes() == want.tobytes()


def test_images_levels_and_offsets_out_of_range_are_clamped():
    s = md.scenes()["owners"]
    want = s.reference()["rows"]
    det = s.det.copy()
    det["image"][det["image"] == 0] = -4
    det["image"][det["image"] == 3] = 1000
    det["level"][:] = np.where(det["image"] == 1, 77, -1)                   # one level: every level clamps to 0
    _, got = select(s, det=det)
    got = ref.ordered(got)
    fixed = got.copy()
    fixed["image"], fixed["level"] = np.clip(got["image"], 0, 3), 0
    assert ref.ordered(fixed).tobytes() == want.tobytes()
    _, off, _ = scene_arrays(s)
    off[0], off[-1] = -9, off[-1] + 50                                      # clamped to 0 and n_gt: the same ranges
    _, got = select(s, gt_off=off)
    assert ref.ordered(got).tobytes() == want.tobytes()


def test_error_returns():
    import torch
    lib = nat.load()
    s = md.scenes()["owners"]
    n = C.c_size_t()
    assert lib.wb_mine_scratch_bytes(-1, 1, 1, C.byref(n)) == nat.WB_ERR_INVALID
    assert lib.wb_mine_scratch_bytes(10, 1, 1, None) == nat.WB_ERR_INVALID
    assert lib.wb_mine_scratch_bytes(10, 100000, 1, C.byref(n)) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_mine_scratch_bytes(10, 1, 100000, C.byref(n)) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_mine_scratch_bytes((1 << 26) + 1, 1, 1, C.byref(n)) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_mine_scratch_bytes(1000, 4, 8, C.byref(n)) == 0 and n.value >= 6 * 1000 + 32 * (2048 + 32)
    # n_det == 0 launches nothing and looks at no pointer
    assert lib.wb_mine_select_launch(None, None, 0, None, 1, 10, 10, None, None, None, 0, None, 1, 0.7, 0.3, 1, 1, 1, 1, 0, None, 0, None,
                                     0, None) == 0
    rc, _ = select(s, capacity=len(s.expect) - 1)                           # less room than the rule can fill
    assert rc == nat.WB_ERR_INVALID and "room" in nat.last_error()
    gt, off, ign = scene_arrays(s)
    d = [dev(x) for x in (s.det, s.inv_scale, gt, off, ign, s.serial)]
    need = C.c_size_t()
    lib.wb_mine_scratch_bytes(s.det.size, s.n_images, 1, C.byref(need))
    scratch = torch.zeros(need.value + 64, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(32 * (s.det.size + 2), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(det=d[0], n_det=s.det.size, gt_p=d[2], scr=scratch, scr_bytes=need.value, rows_p=rows, max_tp=100, n_gt=len(gt), cnt_p=cnt,
             shift=0):
        at = lambda t: None if t is None else C.c_void_p(t.data_ptr() + shift)
        return lib.wb_mine_select_launch(nat.stream_ptr(), at(det), n_det, nat.ptr(d[1]), 1, s.m, s.n, nat.ptr(gt_p), nat.ptr(d[3]),
                                         nat.ptr(d[4]), n_gt, nat.ptr(d[5]), s.n_images, 0.7, 0.3, max_tp, 100, 1, 1, 0, nat.ptr(scr),
                                         scr_bytes, nat.ptr(rows_p), s.det.size, nat.ptr(cnt_p))
    assert call() == 0
    assert call(det=None) == nat.WB_ERR_INVALID
    assert call(gt_p=None) == nat.WB_ERR_INVALID
    assert call(rows_p=None) == nat.WB_ERR_INVALID
    assert call(cnt_p=None) == nat.WB_ERR_INVALID
    assert call(scr_bytes=need.value - 1) == nat.WB_ERR_INVALID
    assert call(shift=4) == nat.WB_ERR_INVALID                              # det no longer 16-byte aligned
    assert call(n_det=-1) == nat.WB_ERR_INVALID
    assert call(max_tp=-1) == nat.WB_ERR_INVALID
    assert call(n_gt=-1) == nat.WB_ERR_INVALID
    torch.cuda.synchronize()


def gather(g, rows=None, dtype=None):
    """One wb_mine_gather_launch on gather scene `g` -> (rc, out, err), guards checked."""
    import torch
    lib = nat.load()
    rows = g.rows if rows is None else rows
    crop = g.m * g.n * g.C * g.buf.dtype.itemsize
    d_buf, d_lv, d_rows = dev(g.buf), dev(g.levels), dev(rows)
    out = torch.full(((2 * GUARD + len(rows)) * crop,), FILL, dtype=torch.uint8, device="cuda")
    err = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    wdt = (nat.WB_DTYPE_U8 if g.buf.dtype == np.uint8 else nat.WB_DTYPE_F32) if dtype is None else dtype
    rc = lib.wb_mine_gather_launch(nat.stream_ptr(), nat.ptr(d_buf), wdt, g.stride, md.N_IMAGES, nat.ptr(d_lv), len(g.levels), g.C,
                                   nat.ptr(d_rows), len(rows), g.m, g.n, C.c_void_p(out.data_ptr() + GUARD * crop),
                                   C.c_void_p(err.data_ptr() + 4))
    if rc != 0:
        return rc, None, None
    h, he = out.cpu().numpy(), err.cpu().numpy()
    assert he[0] == he[2] == 0x5A5A5A5A, "words around the error word were written"
    assert (h[:GUARD * crop] == FILL).all() and (h[(GUARD + len(rows)) * crop:] == FILL).all(), "bytes around the crops were written"
    return rc, h[GUARD * crop:(GUARD + len(rows)) * crop].view(g.buf.dtype).reshape(len(rows), g.m, g.n, g.C), int(he[1])


@pytest.mark.parametrize("name", list(md.gather_scenes()))
def test_gather_on_the_designs(name):
    g = md.gather_scenes()[name]
    want, want_err = g.expect()
    rc, got, err = gather(g)
    assert rc == 0, nat.last_error()
    assert err == want_err == 1
    assert got.tobytes() == want.tobytes(), f"{name}: crops {np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))} differ"
    rc, got, err = gather(g, rows=g.rows[:-1])                              # without the row outside: no error
    assert rc == 0 and err == 0 and got.tobytes() == want[:-1].tobytes()


def test_gather_rows_out_of_range_are_zeros():
    g = md.gather_scenes()["gather-3x5x2-float32"]
    rows = g.rows[:4].copy()
    rows["image"][0], rows["image"][1], rows["level"][2], rows["level"][3] = -1, md.N_IMAGES, -1, len(g.levels)
    rc, got, err = gather(g, rows=rows)
    assert rc == 0 and err == 1 and not got.any()
    lib = nat.load()
    rc, _, _ = gather(g, dtype=nat.WB_DTYPE_F64)
    assert rc == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_mine_gather_launch(nat.stream_ptr(), None, nat.WB_DTYPE_F32, 10, 1, None, 1, 1, None, 5, 2, 2, None, None) == nat.WB_ERR_INVALID
    assert lib.wb_mine_gather_launch(nat.stream_ptr(), None, nat.WB_DTYPE_F32, 10, 1, None, 1, 1, None, -1, 2, 2, None, None) == nat.WB_ERR_INVALID
