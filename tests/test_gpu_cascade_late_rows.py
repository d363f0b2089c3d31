"""The stage-parallel tail's row-split pass (four windows x 16 stages per register) on designed survivor maps: the map
decides at which stage every window dies (tests/survivor_maps.py), so alive[], the survivors and -- from the oracle's
fp32 running sum -- their score bits are known exactly.  Every comparison is exact.

A wave walks its own queue through the tail when it leaves the dense segments with a few windows, which takes a tile
that is neither dealt out window by window behind stage 8 nor behind stage 16: every level below is ONE 64 x 64 tile with
448 windows alive behind phase A -- seven pooled chunks of 64, one per wave, in row-major order of the windows -- of
which all but the designed LATE ones die in stages 17 .. 31.  Levels, by the windows alive on entering stage 32:
  * 1, 3, 4, 5, 9, 19, 20 and 21, spread evenly over the chunks: every wave reaches stage 32 with one to three windows, in
    different waves' rows and in both of a wave's 4-row passes (19 .. 21 were the capacity - 1, capacity and capacity + 1 of
    a per-tile list of late survivors that round 19 tried and did not keep: DESIGN 4.4);
  * 4, 5, 8 and 9 in ONE chunk: a full register, one and two full registers with an empty row in the last, and a wave that
    stays on the dense segments to stage 64 (more than sm.SPAR[1] windows) and enters the tail there;
  * 6 of which two sit alone in an eighth chunk (the tile's last row): that wave leaves at stage 16.
The late windows die at stages 33, 47 (a row's last lane), 48 (the next pass's first), 63, at 41 behind the free stage 40
(theta = -inf inside a pass), at the last stage -- stage 74 of 75: lane 10 of a SHORT last pass -- or never, in an order
that differs between the two images of the launch: the windows of one register are rejected at different stages while
their partners go on.  The float32 and 16-bit forms scan the same levels as two 32-row tiles."""

import numpy as np
import pytest

import survivor_maps as sm
import test_gpu_survivor_maps as gsm
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu

SHAPE, T, DEPTH, FREE = (12, 12, 4), 75, 2, (16, 40)
TALL, WAVES = 64, 8
LATE_CAP = 20                            # entries of the per-tile list that round 19 tried (see above)
LATE_AT = 32                             # sm.SPAR[0]: the stage at which a wave with a few windows leaves the segments
POOLED = 7 * 64                          # windows alive behind phase A: one chunk for each of seven waves
DEATHS = np.array([sm.NEVER, 33, 47, sm.NEVER, 48, 63, T - 1, 40, sm.NEVER, 35, 62], np.uint8)
COUNTS = (1, 3, 4, 5, 9, LATE_CAP - 1, LATE_CAP, LATE_CAP + 1)
CLUSTERS = (4, 5, 8, 9)                  # late windows of ONE chunk


def late_map(n_late, image, tail_two=False, cluster=False):
    """(D, late cells): a 64 x 64 tile with POOLED windows behind phase A in rows 0 .. 61, n_late of them -- evenly spread
    in row-major order, or (cluster) neighbours inside the third chunk -- alive on entering stage 32; tail_two: two more
    late windows in row 63, a chunk of their own."""
    ranks = 130 + 3 * np.arange(n_late) if cluster else ((np.arange(n_late) + 0.5) * POOLED / n_late).astype(np.int64)
    for attempt in range(100):                   # (the first draw whose late windows lie in both 4-row passes of a wave)
        rng = np.random.default_rng([n_late, image, int(tail_two), int(cluster), attempt])
        D = rng.integers(0, sm.PHASE_A, (TALL, 64)).astype(np.uint8)
        cells = np.sort(rng.permutation(62 * 64)[:POOLED])
        if n_late < 2 or cluster or np.unique(cells[ranks] // 64 % 8 // 4).size == 2:
            break
    D.reshape(-1)[cells] = rng.integers(17, LATE_AT, POOLED).astype(np.uint8)
    D.reshape(-1)[cells[ranks]] = np.roll(DEATHS, 3 * image + n_late)[np.arange(n_late) % DEATHS.size]
    if tail_two:
        D[63, [5 + image, 60]] = (sm.NEVER, 47 + image)
    return D, cells[ranks]


def level_maps(image):
    return ([late_map(n, image)[0] for n in COUNTS] + [late_map(n, image, cluster=True)[0] for n in CLUSTERS]
            + [late_map(4, image, tail_two=True)[0]])


_case = {}


def case():
    """The cascade, the two images' maps and channel images, and what the scan must give -- computed once."""
    if not _case:
        casc = sm.designed_cascade(SHAPE, T, DEPTH, FREE)
        assert casc.free == {16, 40}
        maps = [level_maps(0), level_maps(1)]
        for image, per in enumerate(maps):
            assert [sm.entering(D, T, casc.free, LATE_AT) for D in per] == list(COUNTS + CLUSTERS) + [6]
            assert all(sm.entering(D, T, casc.free, 16) > sm.SPAR_WG for D in per)         # no hand-out behind stage 8 or 16
            for n, D in zip(COUNTS, per):
                at = late_map(n, image)[1]
                rows, chunk = at // 64, np.searchsorted(np.flatnonzero(sm.eff_stage(D, T, casc.free).reshape(-1) >= sm.PHASE_A), at) // 64
                assert np.bincount(chunk).max() <= 3                                       # every wave leaves at stage 32 ...
                if n >= 3:                                                                 # ... three or more with windows,
                    assert np.unique(chunk).size >= 3 and np.unique(rows // 8).size >= 3   # from different waves' rows,
                    assert {0, 1} == set(rows % 8 // 4)                                    # of both 4-row passes
            for n in CLUSTERS:
                D, at = late_map(n, image, cluster=True)
                chunk = np.searchsorted(np.flatnonzero(sm.eff_stage(D, T, casc.free).reshape(-1) >= sm.PHASE_A), at) // 64
                assert (chunk == 2).all() and (n > sm.SPAR[1]) == (n == 9)
        late = np.concatenate([sm.eff_stage(D, T, casc.free)[sm.eff_stage(D, T, casc.free) >= LATE_AT] for per in maps for D in per])
        assert {33, 47, 48, 63, 41, T - 1, T} <= set(late.tolist())
        assert not np.array_equal(maps[0][4], maps[1][4])
        Xs = [[sm.channel_image(D, SHAPE, 100 * b + l) for l, D in enumerate(per)] for b, per in enumerate(maps)]
        want_alive, want = gsm.expect(casc, maps, Xs)
        assert set(want[0]) == {0, 1} and len(set(want[1])) >= len(COUNTS + CLUSTERS)
        _case.update(casc=casc, Xs=Xs, want_alive=want_alive, want=want)
    return _case


@pytest.mark.parametrize("form", ["u8", "rank8"])
def test_row_split_tail_on_tall_tiles(form):
    """The 64-row one-byte forms, generic and model-specialised kernel."""
    c = case()
    casc, kind = c["casc"], gsm.KIND[form]
    dm = casc.model().device_cascade()
    assert dm.form_rows(kind) == TALL and not dm.specialized()
    images = [[gsm.form_array(casc, x, form) for x in per] for per in c["Xs"]]
    for kernel in ("generic", "specialised"):
        if kernel == "specialised":
            assert dm.specialize(kind) and kind in dm.specialized(), nat.last_error()
        got, alive = gsm.raw_scan(dm, form, images)
        gsm.check(f"{form}, {kernel} kernel", got, alive, c["want_alive"], c["want"])


@pytest.mark.parametrize("form", ["f32", "rank16"])
def test_row_split_tail_on_32_row_tiles(form):
    """The same levels as two 32-row tiles each (four pooled chunks a tile), generic kernel."""
    c = case()
    casc = c["casc"]
    dm = casc.model().device_cascade()
    assert dm.form_rows(gsm.KIND[form]) == 32
    images = [[gsm.form_array(casc, x, form) for x in per] for per in c["Xs"]]
    got, alive = gsm.raw_scan(dm, form, images)
    gsm.check(f"{form}, generic kernel", got, alive, c["want_alive"], c["want"])
