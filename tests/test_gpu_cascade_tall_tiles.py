"""The one-byte forms' tall cascade tile (64 x 64 windows on eight waves, phase A in two passes of four rows per lane) on
designed survivor maps: the map decides at which stage every window dies (tests/survivor_maps.py), so alive[], the
survivors and -- from the oracle's fp32 running sum -- their score bits are known exactly.  Every comparison is exact.

One launch scans all the levels below for two images with maps of their own, on uint8 and on 8-bit rank tiles, with the
generic and with the model-specialised kernel, from a tile table of every 32-row unit (as any caller of the C ABI may
hand over: the kernel leaves at once on the entries that start no tile) and from one of the starting entries only (the
engine's).  Levels, as window grids:
  * 65 x 65: one full tile, a 1-row and a 1-column remainder tile (every pass but the first is skipped there);
  * 5 rows: wave 0 runs both passes (one row in the second), every other wave none;
  * 36 rows: the wave of rows 32..39 runs one full pass and skips the other;
  * every window of pass 0 lives on behind phase A and none of pass 1, and the reverse: the queue offsets across the
    passes, `entered` over both passes against alive[level, stage], and (2048 survivors) the dense continuation;
  * cap - 1, cap and cap + 1 survivors behind stage 8: the queue's boundary on the tall tile."""

import numpy as np
import pytest

import survivor_maps as sm
import test_gpu_survivor_maps as gsm
from waldboost_amd import _native as nat
from waldboost_amd import engine as _engine
from waldboost_amd.plan import PyramidPlan

pytestmark = pytest.mark.gpu

SHAPE, T, DEPTH, FREE = (12, 12, 4), 40, 2, (16,)
TALL, UNIT, WAVES = 64, 32, 8
CAP = 64 * WAVES + 768                   # wb_casc_qcap(64, 8)
LATE = np.array([8, 9, 11, 12, 15, 17, 20, 25, 33, 39, sm.NEVER], np.uint8)     # death stages behind phase A


def early(rng, shape):
    return rng.integers(0, sm.PHASE_A, shape).astype(np.uint8)


def late(rng, shape):
    return LATE[rng.integers(0, LATE.size, shape)]


def mixed_map(nr, nc, seed):
    """Most windows die in phase A, a fifth behind it."""
    rng = np.random.default_rng([seed, nr, nc])
    return np.where(rng.random((nr, nc)) < 0.2, late(rng, (nr, nc)), early(rng, (nr, nc)))


def pass_map(keep, seed):
    """A 64 x 64 tile whose windows of pass `keep` (rows 0..3 or 4..7 of every wave's eight) all outlive phase A and whose
    others all die in it."""
    rng = np.random.default_rng([seed, keep])
    in_pass = (np.arange(TALL) % 8 // 4 == keep)[:, None]
    return np.where(in_pass, late(rng, (TALL, 64)), early(rng, (TALL, 64)))


def count_map(k, seed):
    """A 64 x 64 tile with exactly k windows behind stage 8, anywhere."""
    rng = np.random.default_rng([seed, k])
    D = early(rng, (TALL, 64))
    at = rng.permutation(TALL * 64)[:k]
    D.reshape(-1)[at] = late(rng, k)
    return D


def level_maps(image):
    s = 10 * image
    return [mixed_map(65, 65, s), mixed_map(5, 70, s + 1), mixed_map(36, 64, s + 2), pass_map(image, s + 3), pass_map(1 - image, s + 4),
            count_map(CAP - 1 + image, s + 5), count_map(CAP + image, s + 6)]


_case = {}


def case():
    """The cascade, the two images' maps and channel images, and what the scan must give -- computed once."""
    if not _case:
        casc = sm.designed_cascade(SHAPE, T, DEPTH, FREE)
        maps = [level_maps(0), level_maps(1)]
        behind = [[sm.entering(D, T, casc.free, sm.PHASE_A) for D in per] for per in maps]
        assert behind[0][3:] == [2048, 2048, CAP - 1, CAP] and behind[1][3:] == [2048, 2048, CAP, CAP + 1]
        for image, per in enumerate(maps):                 # one pass alone holds the survivors, then the other alone
            for D, keep in ((per[3], image), (per[4], 1 - image)):
                rows = np.arange(TALL) % 8 // 4 == keep
                assert (sm.eff_stage(D[rows], T, casc.free) >= sm.PHASE_A).all() and (sm.eff_stage(D[~rows], T, casc.free) < sm.PHASE_A).all()
        Xs = [[sm.channel_image(D, SHAPE, 100 * b + l) for l, D in enumerate(per)] for b, per in enumerate(maps)]
        want_alive, want = gsm.expect(casc, maps, Xs)
        assert want[0].size and set(want[0]) == {0, 1}
        _case.update(casc=casc, Xs=Xs, want_alive=want_alive, want=want)
    return _case


def tile_tables(dm, dims):
    full = PyramidPlan._tiles(dims, UNIT, dm.tile_cols)
    starts = PyramidPlan._tiles(dims, TALL, dm.tile_cols)
    starts["ty"] *= TALL // UNIT
    return {"every unit": full, "starting entries": starts}


def scan(dm, kind, images, tiles, first_cap=1 << 15):
    """wb_cascade_launch over images[b][l] with the given tile table -> (records sorted, alive[B, L, T])."""
    import torch
    lib, dev = nat.load(), nat.require_gpu()
    B, L = len(images), len(images[0])
    lv = np.zeros(L, nat.LEVEL_DTYPE)
    off = 0
    for l, a in enumerate(images[0]):
        lv[l]["u"], lv[l]["v"], lv[l]["chn_off"] = a.shape[0], a.shape[1], off
        off += (a.size + 3) // 4 * 4
    stride = off + 16
    host = np.zeros((B, stride), np.uint8)
    for b, im in enumerate(images):
        for l, a in enumerate(im):
            o = int(lv[l]["chn_off"])
            host[b, o:o + a.size] = a.reshape(-1)
    buf, levels = torch.from_numpy(host).to(dev), torch.from_numpy(lv.view(np.uint8).copy()).to(dev)
    tl = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev)
    alive = torch.zeros((B, L, T), dtype=torch.int32, device=dev)
    detb = _engine.DetBuffer(first_cap, dev)
    detb.zero()
    nat.check(lib.wb_cascade_launch(nat.stream_ptr(), dm.handle, nat.ptr(buf), kind, stride, B, nat.ptr(levels), L, nat.ptr(tl),
                                    int(tiles.size), nat.ptr(detb.recs), nat.ptr(detb.counts), detb.cap, nat.ptr(alive)), "wb_cascade_launch")
    assert detb.max_count() <= detb.cap
    d = detb.compact().cpu().numpy().view(nat.DET_DTYPE).reshape(-1)
    return d[np.lexsort((d["c"], d["r"], d["level"], d["image"]))], alive.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("form", ["u8", "rank8"])
def test_tall_tiles_on_designed_maps(form):
    c = case()
    casc, kind = c["casc"], gsm.KIND[form]
    dm = casc.model().device_cascade()
    assert (dm.tile_rows, dm.form_rows(kind), dm.form_rows(nat.WB_DTYPE_F32), dm.form_rows(nat.WB_DTYPE_RANK16)) == (UNIT, TALL, UNIT, UNIT)
    images = [[gsm.form_array(casc, x, form) for x in per] for per in c["Xs"]]
    dims = [(x.shape[0] - SHAPE[0], x.shape[1] - SHAPE[1]) for x in c["Xs"][0]]
    tables = tile_tables(dm, dims)
    assert tables["starting entries"].size < tables["every unit"].size
    assert not dm.specialized()
    for kernel in ("generic", "specialised"):
        if kernel == "specialised":
            assert dm.specialize(kind) and kind in dm.specialized(), nat.last_error()
        for name, tiles in tables.items():
            got, alive = scan(dm, kind, images, tiles)
            gsm.check(f"{form}, {kernel} kernel, table of {name}", got, alive, c["want_alive"], c["want"])
