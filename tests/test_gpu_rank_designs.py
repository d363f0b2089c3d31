"""The rank epilogue of the channel kernel and the rank tables on designed threshold sets (tests/rank_designs.py; the
tables themselves are checked against the library without a GPU in test_rank_designs_host.py): for every design the
forms the model has are the design's, every pixel of every level of the design image -- uint8, and float32 with
infinite channel values -- is ranked as np.searchsorted ranks it, in one byte and forced into two, and the detections
equal the oracle's bit for bit in each form.  A batch's second image; two models over one rank pyramid at 254 and 255
thresholds of their union.  No model is specialised here: the generic tile kernel scans."""
import functools
import os

import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import engine as _engine
from waldboost_amd import _native as nat
from waldboost_amd.channels import read_opts
from waldboost_amd.synth import synth_image
from oracle import wb_oracle as orc
import rank_designs as rd
from util import oracle_detect

pytestmark = pytest.mark.gpu
OPTS = dict(wb.default_channel_opts, **rd.CHANNEL_OPTS)
WIDTHS = ((False, nat.WB_DTYPE_RANK8), (True, nat.WB_DTYPE_RANK16))


@pytest.fixture(autouse=True)
def no_specialised_kernels(monkeypatch):
    """A second scan of a cascade would build its specialised kernel (seconds of compilation per model and width)."""
    monkeypatch.setattr(_engine, "_JIT_AUTO", False)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def images():
    """The design image as uint8 and as float32 with overflow patches, and a second uint8 image for the batch."""
    img = synth_image(*rd.IMAGE_SHAPE, rd.IMAGE_SEED)
    return img, rd.float_image(img), synth_image(*rd.IMAGE_SHAPE, rd.IMAGE_SEED + 1)


@functools.lru_cache(None)
def oracle_levels(i):
    """The oracle's pyramid of images()[i]: computed once, shared, never written."""
    with np.errstate(invalid="ignore", over="ignore"):
        lv = [chn for chn, _ in orc.channel_pyramid(images()[i], dict(rd.CHANNEL_OPTS, channels="grad_hist"))]
    for a in lv:
        a.setflags(write=False)
    return lv


@functools.lru_cache(None)
def pool():
    return rd.value_pool(oracle_levels(0))


def model_of(S, seed=0):
    a = rd.cascade_arrays(S, seed)
    M = wb.Model(rd.WINDOW, dict(OPTS))
    for s in range(a["theta"].size):
        o = slice(7 * s, 7 * s + 7)
        M.append(wb.DTree(a["feature"][o], a["threshold"][o], a["left"][o], a["right"][o], a["prediction"][o]), float(a["theta"][s]))
    return M


def engine_for(img, batch=1):
    shrink, n_per_oct, smooth, spec = read_opts(OPTS)
    return _engine.get_engine(img.shape[-2], img.shape[-1], img.dtype, shrink, n_per_oct, smooth, batch, channels=spec)


def check_rank_levels(eng, b, t, levels, floats=True):
    """Image b's ranks in `eng`, value by value, against np.searchsorted over the tables' thresholds on the oracle's
    channel values (which the float channels of the same launch must equal bit for bit)."""
    assert eng.plan.n_levels == len(levels) == 4
    for l, ref in enumerate(levels):
        if floats:
            assert np.array_equal(bits(eng.read_level(b, l)), bits(ref)), l
        rank = eng.read_rank_level(b, l)
        assert rank.dtype == (np.uint16 if t["wide"] else np.uint8) and rank.shape == ref.shape
        for c in range(4):
            want = rd.true_ranks(ref[..., c], t, c).reshape(ref.shape[:2])
            assert np.array_equal(rank[..., c].astype(np.int64), want), (l, c, rd.kernel_path(t["K"], t["wide"]))


def check_detect(M, img):
    with np.errstate(invalid="ignore", over="ignore"):
        ref = oracle_detect(M, img)
    res = M.detect_raw(img)
    assert np.array_equal(res["alive"], ref["alive"])
    assert np.array_equal(res["level"], ref["level"]) and np.array_equal(res["r"], ref["r"]) and np.array_equal(res["c"], ref["c"])
    assert np.array_equal(bits(res["scores"]), bits(ref["scores"])) and np.array_equal(bits(res["boxes"]), bits(ref["boxes"]))
    return res


@pytest.mark.parametrize("name", list(rd.DESIGNS))
def test_design(name):
    fn, expect = rd.DESIGNS[name]
    S = fn(pool())
    tables = {w: rd.mirror_tables(S, w) for w in (False, True)}
    M = model_of(S)
    dm = M.device_cascade()
    assert (dm.rank_ok, dm.rank16_ok) == (expect["rank8"], expect["rank16"])
    first = nat.WB_DTYPE_RANK8 if expect["rank8"] else nat.WB_DTYPE_RANK16 if expect["rank16"] else None
    assert dm.rank_dtype == first
    for i in (0, 1):
        img = images()[i]
        eng = engine_for(img)
        ref = None
        for w, dtype in WIDTHS:
            if tables[w] is None:
                continue
            dm.rank_dtype = dtype
            eng.load_images(img)
            eng.run_channels(dm, floats=True)
            check_rank_levels(eng, 0, tables[w], oracle_levels(i))
            res = check_detect(M, img)                       # (scans the ranks of that width)
            assert ref is None or np.array_equal(bits(res["scores"]), bits(ref["scores"]))
            ref = res
        dm.rank_dtype = first
        if first is None:
            check_detect(M, img)                             # float32 channels, the planar tile


@pytest.mark.parametrize("name", ["k3", "last_slot_full8"])
def test_second_image_of_a_batch(name):
    """rank_stride counts bytes for one-byte ranks and 16-bit elements for two-byte ranks: image 1's ranks value by value."""
    S = rd.DESIGNS[name][0](pool())
    M = model_of(S)
    dm = M.device_cascade()
    assert dm.rank_ok and dm.rank16_ok
    img0, _, img1 = images()
    eng = engine_for(img0, batch=2)
    for w, dtype in WIDTHS:
        dm.rank_dtype = dtype
        eng.load_images(np.stack([img0, img1]))
        eng.run_channels(dm, floats=True)
        t = rd.mirror_tables(S, w)
        check_rank_levels(eng, 1, t, oracle_levels(2))
        check_rank_levels(eng, 0, t, oracle_levels(0))
    dm.rank_dtype = nat.WB_DTYPE_RANK8
    assert not np.array_equal(eng.read_rank_level(0, 0), eng.read_rank_level(1, 0))


@pytest.mark.parametrize("n", [254, 255])
def test_two_models_over_one_pyramid_at_the_edge_of_the_union(n, tmp_path):
    """The union of two models' thresholds on channel 0 is n: at 254 waldboost.detect runs both on ONE pyramid of ranks
    over the union's tables (dumped by wb_rankgroup_create, equal to the mirror of the union), at 255 on the float32
    pyramid; either way each model detects what it detects alone."""
    p = pool()
    union = rd.spread(p[0], n)
    parts = [rd.with_channel(p, 0, union[:150]), rd.with_channel(p, 0, union[n - 150:])]
    models = [model_of(s, seed) for seed, s in enumerate(parts)]
    assert all(m.device_cascade().rank_ok for m in models)
    img = images()[0]
    alone = [m.detect_raw(img) for m in models]
    assert sum(a["scores"].size for a in alone) > 0
    path = str(tmp_path / "ranks.bin")
    os.environ["WB_DUMP_RANKS"] = path
    try:
        out = wb.detect(img, *models)
    finally:
        del os.environ["WB_DUMP_RANKS"]
    label = out.get_field("label")
    for k, a in enumerate(alone):
        assert np.array_equal(bits(out.get_field("scores")[label == k]), bits(a["scores"]))
        assert np.array_equal(bits(out.get()[label == k]), bits(a["boxes"]))
    group = _engine.rank_group([m.device_cascade() for m in models])
    dumped = rd.read_rank_dump(path)
    if n == 255:
        assert group is None and dumped == {}
        return
    t = rd.mirror_tables([np.concatenate(both) for both in zip(*parts)], False)
    assert t is not None and t["n"][0] == 254 and group is not None and set(dumped) == {False}
    d = dumped[False]
    assert d["K"] == t["K"] and d["k"].tobytes() == t["k"].tobytes() and d["b"].tobytes() == t["b"].tobytes()
    assert d["S"].tobytes() == t["S"].tobytes() and d["base"].tobytes() == t["base"].tobytes()
    assert all(v.rank_ok and not v.rank16_ok and v.rank_dtype == nat.WB_DTYPE_RANK8 for v in group.views)
    # the pyramid the call left resident: ranks over the union's tables
    check_rank_levels(engine_for(img), 0, t, oracle_levels(0), floats=False)
