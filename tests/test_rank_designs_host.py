"""The threshold-rank tables on designed threshold sets (tests/rank_designs.py), without a GPU: the library's tables
(WB_DUMP_RANKS) and rank stage records (WB_DUMP_STAGES) against the NumPy mirror, the three epilogue paths restated
against np.searchsorted on probes at every threshold and every cell boundary, and every wrong table caught."""
import ctypes as C
import ctypes.util
import functools
import os
import sys

import numpy as np
import pytest

from oracle import wb_oracle as orc
from waldboost_amd import _native as nat
from waldboost_amd.synth import synth_image
import rank_designs as rd
from test_host import rank_records_mirror
from util import GOLDEN

sys.path.insert(0, GOLDEN)
from make_golden_stages import create as create_with_stage_dump, read_dump  # noqa: E402

NAMES = list(rd.DESIGNS)


@functools.lru_cache(None)
def pools():
    """(pool of the uint8 design image's oracle pyramid, pool of the float32 one's): per channel the distinct values."""
    img = synth_image(*rd.IMAGE_SHAPE, rd.IMAGE_SEED)
    opts = dict(rd.CHANNEL_OPTS, channels="grad_hist")
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(rd.value_pool([chn for chn, _ in orc.channel_pyramid(im, opts)]) for im in (img, rd.float_image(img)))


@functools.lru_cache(None)
def design(name):
    """(thresholds per channel, {wide: mirror tables or None}, {wide: probes per channel})."""
    S = rd.DESIGNS[name][0](pools()[0])
    tables = {w: rd.mirror_tables(S, w) for w in (False, True)}
    return S, tables, {w: rd.probes(t) for w, t in tables.items() if t is not None}


def test_the_design_image_is_what_the_designs_were_made_for():
    """Four levels, 48 x 80 .. 6 x 10; the uint8 pyramid holds 0 and values in (12, 128) only, the float32 one infinite
    values and no NaN; the boundary hits are values of the uint8 pyramid whose unfused cell lies above the fused one."""
    img = synth_image(*rd.IMAGE_SHAPE, rd.IMAGE_SEED)
    shapes = [chn.shape for chn, _ in orc.channel_pyramid(img, dict(rd.CHANNEL_OPTS, channels="grad_hist"))]
    assert shapes == [(48, 80, 4), (24, 40, 4), (12, 20, 4), (6, 10, 4)]
    p8, pf = pools()
    for c in range(4):
        assert p8[c][0] == 0 and p8[c][1] > 12 and p8[c][-1] < 128 and p8[c].size > 2000
        assert np.isinf(pf[c]).any() and not np.isnan(pf[c]).any()
    assert len(rd.BOUNDARY_HITS) == 3
    for i, (c, v, lo, hi) in enumerate(rd.BOUNDARY_HITS):
        v = np.array([v], np.uint32).view(np.float32)
        t = design(f"boundary{i}")[1][False]
        assert v[0] in p8[c] and v[0] in t["S"][c, :3]
        assert rd.cell(v, t["k"][c], t["b"][c], 2048, rd.unfused)[0] == rd.cell(v, t["k"][c], t["b"][c], 2048)[0] + 1


def test_the_fma_emulation_is_the_correctly_rounded_fmaf():
    """rd.fmaf against the C library's fmaf on every probe of three designs, grids included whose k is 1e-36 and 1e5."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float] * 3
    n = differ = 0
    for name in ("specials", "k16", "boundary0"):
        _, tables, pr = design(name)
        for w, t in tables.items():
            for c in range(4):
                v = pr[w][c][:-1]
                want = np.array([libm.fmaf(float(x), float(t["k"][c]), float(t["b"][c])) for x in v], np.float32)
                assert np.array_equal(rd.fmaf(v, t["k"][c], t["b"][c]).view(np.uint32), want.view(np.uint32)), (name, w, c)
                with np.errstate(invalid="ignore"):
                    differ += int((rd.unfused(v, t["k"][c], t["b"][c]) != want).sum())
                n += v.size
    assert n > 10000 and differ > 100          # (the two-rounding form is not the same function)


def create(lib, model, stage_path, rank_path):
    os.environ["WB_DUMP_RANKS"] = rank_path
    try:
        return create_with_stage_dump(lib, model, stage_path)
    finally:
        del os.environ["WB_DUMP_RANKS"]


def canonical(S):
    return (S + np.float32(0.0)).tobytes()             # (which of -0.0 / 0.0 the library's sort keeps is not specified)


@pytest.mark.parametrize("name", NAMES)
def test_designs_against_the_library(name, tmp_path):
    """wb_model_create on the design's cascade with both dumps on (complete before the first device call: no GPU needed):
    the forms present are the design's, the rank stage records equal test_host's mirror, k, b, K, S and base equal
    mirror_tables byte for byte, and the mirror reproduces every constant of the design."""
    S, tables, _ = design(name)
    expect = rd.DESIGNS[name][1]
    # the design itself: interior thresholds are values of the design image's pyramid or their float neighbours
    for c in range(4):
        s = np.asarray(S[c], np.float32)
        inner = s[np.isfinite(s) & (s > 0) & (s < 128) & (s != rd.TINY) & (s != rd.DENORM_MIN)]
        assert np.isin(inner, rd.candidates(pools()[0][c])).all(), (name, c)
    # the mirror against the design's constants
    for w, kk, kt in ((False, "K8", "trim8"), (True, "K16", "trim16")):
        t = tables[w]
        assert (t is not None) == expect["rank16" if w else "rank8"], (name, w)
        assert (None, None) == (expect[kk], expect[kt]) if t is None else (t["K"], tuple(t["trim"])) == (expect[kk], expect[kt]), (name, w)
    # the library against the mirror
    lib = nat.load()
    model = rd.cascade_arrays(S)
    sp, rp = str(tmp_path / "stages.bin"), str(tmp_path / "ranks.bin")
    rc, h = create(lib, model, sp, rp)
    assert rc in (0, nat.WB_ERR_HIP), (name, lib.wb_last_error())
    if rc == 0:
        nat.check(lib.wb_model_destroy(h), "wb_model_destroy")
    hdr, mask, records = read_dump(sp)
    assert mask == 3 | expect["rank8"] << 2 | expect["rank16"] << 3, (name, mask)
    assert hdr[2] == 2 and hdr[0] == model["theta"].size + 4
    dumped = rd.read_rank_dump(rp)
    assert set(dumped) == {w for w in (False, True) if tables[w] is not None}
    for w, d in dumped.items():
        t = tables[w]
        assert np.array_equal(records[3 if w else 2], rank_records_mirror(model, hdr[0], hdr[1], hdr[2], 2 if w else 1)), (name, w)
        assert d["K"] == t["K"], (name, w, d["K"], t["K"])
        assert d["k"].tobytes() == t["k"].tobytes() and d["b"].tobytes() == t["b"].tobytes(), (name, w, d["k"], t["k"], d["b"], t["b"])
        assert canonical(d["S"]) == canonical(t["S"]) and d["base"].tobytes() == t["base"].tobytes(), (name, w)


@pytest.mark.parametrize("name", NAMES)
def test_every_allowed_path_ranks_every_probe_as_searchsorted_does(name):
    _, tables, pr = design(name)
    for w, t in tables.items():
        if t is None:
            continue
        paths = rd.allowed_paths(t["K"], w)
        assert paths[-1] == "loop" and rd.kernel_path(t["K"], w) == paths[0]
        for c in range(4):
            v = pr[w][c]
            assert np.isnan(v[-1]) and (np.diff(rd.key_of(v[:-1])) > 0).all()
            assert (np.diff(rd.cell(v[:-1], t["k"][c], t["b"][c], t["cells"])) >= 0).all(), (name, w, c)
            want = rd.true_ranks(v, t, c)
            top = t["n"][c] - int(np.isposinf(t["S"][c, :t["n"][c]]).any())       # (nothing lies above a threshold +inf)
            assert want[-1] == rd.NAN_RANK[w] and want[:-1].max() == top
            for path in paths:
                assert np.array_equal(rd.rank_by_tables(v, t, path, c), want), (name, w, c, path)


def test_the_designs_take_every_path_in_both_widths():
    """K of the designs against the K ranges that select a path: pair at K = 1 and 2, quad at 3 and 4, the loop from 3
    (narrow) and 5 (wide) up to the 16 / 64 a cell may hold."""
    K = {w: {t["K"] for n in NAMES for t in [design(n)[1][w]] if t is not None} for w in (False, True)}
    assert {1, 2, 3, 4, 5, 16} <= K[False] and max(K[False]) == 16
    assert {1, 2, 3, 4, 5, 16, 17, 64} <= K[True] and max(K[True]) == 64
    trims = {w: {i for n in NAMES for t in [design(n)[1][w]] if t is not None for i in t["trim"]} for w in (False, True)}
    assert trims[False] == trims[True] == {0, 1, 2, 3, 4}


def wrong_counts(name):
    """{design: misranked probes} of one wrong table over all designs, channels and widths, and the number of misranked
    values among those the two design images' pyramids hold."""
    p8, pf = pools()
    per_design, reachable = {}, 0
    for d in NAMES:
        _, tables, pr = design(d)
        n = 0
        for w, t in tables.items():
            if t is None:
                continue
            for c in range(4):
                n += int((rd.WRONG_TABLES[name](pr[w][c], t, c) != rd.true_ranks(pr[w][c], t, c)).sum())
                v = np.union1d(p8[c], pf[c])
                reachable += int((rd.WRONG_TABLES[name](v, t, c) != rd.true_ranks(v, t, c)).sum())
        if n:
            per_design[d] = n
    return per_design, reachable


# misranked probes per design, and misranked values among those the design images' pyramids hold (wrong_counts)
WRONG_COUNTS = {
    "k_short": {"degenerate": 12, "degenerate_rot": 12, "full8": 554, "over8": 32, "full16": 84, "k2": 4, "k3": 4, "k16": 4,
        "k17": 2, "wide_k4": 4, "wide_k5": 4, "wide_k64": 2, "trim0": 425, "trim2": 6, "trim3": 6, "trim4": 5, "wide_trim4":
        3, "last_slot": 76, "last_slot_full8": 635, "last_slot_full8_inf": 631, "last_slot_full16": 2,
        "last_slot_full16_inf": 28, "specials": 4, "boundary0": 47, "boundary1": 42, "boundary2": 48},
    "pair_at_k3": {"k3": 4},
    "quad_at_k5": {"full16": 84, "wide_k5": 4},
    "base_off_by_one": {"degenerate": 16, "degenerate_rot": 16, "full8": 24, "over8": 12, "full16": 12, "k2": 36, "k3": 36,
        "k16": 36, "k17": 18, "wide_k4": 36, "wide_k5": 36, "wide_k64": 18, "trim0": 24, "trim1": 24, "trim2": 24, "trim3":
        24, "trim4": 30, "wide_trim4": 12, "last_slot": 24, "last_slot_inf": 24, "last_slot_full8": 24,
        "last_slot_full8_inf": 24, "last_slot_full16": 12, "last_slot_full16_inf": 12, "specials": 24, "boundary0": 24,
        "boundary1": 24, "boundary2": 24},
    "no_lower_clamp": {"degenerate": 24, "degenerate_rot": 24, "full8": 48, "over8": 24, "full16": 24, "k2": 36, "k3": 36,
        "k16": 36, "k17": 18, "wide_k4": 36, "wide_k5": 36, "wide_k64": 18, "trim0": 48, "trim1": 48, "trim2": 36, "trim3":
        36, "trim4": 36, "wide_trim4": 18, "last_slot": 48, "last_slot_inf": 48, "last_slot_full8": 48,
        "last_slot_full8_inf": 48, "last_slot_full16": 24, "last_slot_full16_inf": 24, "boundary0": 36, "boundary1": 36,
        "boundary2": 36},
    "no_upper_clamp": {"degenerate": 4, "degenerate_rot": 4, "full8": 8, "over8": 4, "full16": 4, "k2": 8, "k3": 8, "k16":
        8, "k17": 4, "wide_k4": 8, "wide_k5": 8, "wide_k64": 4, "trim0": 8, "trim1": 14, "trim2": 26, "trim3": 80, "trim4":
        53, "wide_trim4": 154, "last_slot": 8, "last_slot_inf": 8, "last_slot_full8": 8, "last_slot_full8_inf": 8,
        "last_slot_full16": 4, "last_slot_full16_inf": 4, "specials": 12},
    "unfused": {"full8": 3, "over8": 2, "full16": 2, "k2": 3, "k3": 2, "k16": 2, "k17": 3, "wide_k4": 3, "wide_k5": 1,
        "wide_k64": 1, "trim0": 6, "trim1": 2, "trim2": 2, "trim3": 4, "trim4": 3, "wide_trim4": 1, "last_slot": 2,
        "last_slot_inf": 2, "last_slot_full8": 4, "last_slot_full8_inf": 4, "last_slot_full16": 3, "last_slot_full16_inf":
        3, "specials": 3, "boundary0": 3, "boundary1": 4, "boundary2": 3},
    "ge_compare": {"degenerate": 14, "degenerate_rot": 14, "full8": 534, "over8": 268, "full16": 1033, "k2": 38, "k3": 40,
        "k16": 94, "k17": 48, "wide_k4": 46, "wide_k5": 48, "wide_k64": 143, "trim0": 226, "trim1": 230, "trim2": 236,
        "trim3": 264, "trim4": 149, "wide_trim4": 212, "last_slot": 44, "last_slot_inf": 42, "last_slot_full8": 534,
        "last_slot_full8_inf": 532, "last_slot_full16": 1033, "last_slot_full16_inf": 1032, "specials": 66, "boundary0": 32,
        "boundary1": 32, "boundary2": 32},
    "ftz_compare": {"specials": 42},
    "no_nan_code": {"degenerate": 8, "degenerate_rot": 8, "full8": 8, "over8": 4, "full16": 4, "k2": 8, "k3": 8, "k16": 8,
        "k17": 4, "wide_k4": 8, "wide_k5": 8, "wide_k64": 4, "trim0": 8, "trim1": 8, "trim2": 8, "trim3": 8, "trim4": 8,
        "wide_trim4": 4, "last_slot": 8, "last_slot_inf": 8, "last_slot_full8": 8, "last_slot_full8_inf": 8,
        "last_slot_full16": 4, "last_slot_full16_inf": 4, "specials": 8, "boundary0": 8, "boundary1": 8, "boundary2": 8},
}
REACHABLE = {"k_short": 17778, "pair_at_k3": 2380, "quad_at_k5": 2515, "base_off_by_one": 51939, "no_lower_clamp": 346129, "no_upper_clamp": 3444, "unfused": 8, "ge_compare": 3111, "ftz_compare": 6, "no_nan_code": 0}


@pytest.mark.parametrize("name", list(rd.WRONG_TABLES))
def test_every_wrong_table_misranks_a_probe(name):
    per_design, reachable = wrong_counts(name)
    assert sum(per_design.values()) > 0
    assert per_design == WRONG_COUNTS[name] and reachable == REACHABLE[name], (name, per_design, reachable)
    assert (reachable > 0) == (name in rd.GPU_RELEVANT)
