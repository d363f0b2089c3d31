"""The invalidation matrix of PyramidEngine: every re-allocation of a buffer that captured graphs address, against
everything the engine keeps a graph for.

    re-allocations   the detection buffer (grown), the control block (a longer cascade arrives on the engine), the rank
                     buffer (another cascade's ranks of the other width: RANK8 <-> RANK16)
    graph keepers    Model.detect's graph, a detect_stream(batch=2) step, a two-model waldboost.detect sequence

For each pair: warm until the graph exists, force the re-allocation, see that the engine keeps no graph any more
(PyramidEngine._buffers_moved is the one place that drops them), call again twice: the oracle's results, bit for bit, both
times.  Model.detect against the grown detection buffer and against the rank buffer changing width are held by
test_gpu_graph.py::test_model_detect_replays_one_graph_per_cascade_vs_oracle and
test_gpu_ranks.py::test_the_same_cascade_in_one_and_in_two_byte_ranks."""
import os

import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import engine as E
from waldboost_amd import _native as nat
from waldboost_amd.synth import synth_image
from test_gpu_ranks import model_with_thresholds
from util import GOLDEN, oracle_detect

pytestmark = pytest.mark.gpu

H, W = 200, 264
SEEDS = (19, 23)
PAIRS = [(k, r) for k in ("detect", "stream", "multi") for r in ("det", "ctrl", "rank")
         if (k, r) not in (("detect", "det"), ("detect", "rank"))]
_shared = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def keeper_model(seed=43, T=40):
    """The model of test_the_same_cascade_in_one_and_in_two_byte_ranks: one-byte ranks, two-byte ranks possible.  Its
    rejection thresholds are raised until about 2000 windows of a 200x264 image pass: more than the shrunken detection
    buffer takes (16 per shard), fewer than one finish block holds (4096)."""
    rng = np.random.default_rng(seed)
    M = model_with_thresholds(rng, T, 2, lambda n: rng.uniform(0, 60, n))
    M.theta = [t + 0.5 if np.isfinite(t) else t for t in M.theta[:-1]] + [1.0]
    return M


def shared():
    """Images and the oracle's results for the keeper model and its partner in waldboost.detect: computed once."""
    if not _shared:
        imgs = [synth_image(H, W, s) for s in SEEDS]
        K, P = keeper_model(), wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
        _shared.update(imgs=imgs, K=[oracle_detect(K, im) for im in imgs], P=[oracle_detect(P, im) for im in imgs])
        assert all(16 * nat.WB_DET_SHARDS < r["scores"].size <= 4096 for r in _shared["K"])
        assert all(0 < r["scores"].size <= 4096 for r in _shared["P"])
    return _shared


def compose(refs):
    """waldboost.detect's order over per-model results: level-major, then model (reference __init__.py:118-128)."""
    boxes, scores = [np.empty((0, 4), np.float32)], [np.empty(0, np.float32)]
    for lv in range(refs[0]["alive"].shape[0]):
        for r in refs:
            boxes.append(r["boxes"][r["level"] == lv])
            scores.append(r["scores"][r["level"] == lv])
    return np.concatenate(boxes), np.concatenate(scores)


def kept(eng, dm, keeper):
    """The graph the engine keeps for this keeper; None when it keeps none."""
    if keeper == "multi":
        return next((st.graph for st in eng._multi.values() if st.graph is not None), None)
    stt = eng._casc.get(id(dm))
    return None if stt is None else stt.graph if keeper == "detect" else stt.step


@pytest.mark.parametrize("keeper,realloc", PAIRS)
def test_a_reallocation_drops_every_kept_graph_and_the_next_calls_equal_the_oracle(keeper, realloc):
    sh = shared()
    imgs = sh["imgs"]
    K, P = keeper_model(), wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    dm = K.device_cascade()
    assert dm.rank_dtype == nat.WB_DTYPE_RANK8 and dm.rank16_ok
    E._ENGINES.clear()

    def call(i):
        """One call of the keeper (detect_stream: two steps of two images), compared with the oracle."""
        if keeper == "detect":
            res, ref = K.detect_raw(imgs[i]), sh["K"][i]
            assert np.array_equal(res["alive"], ref["alive"])
            assert all(np.array_equal(res[k], ref[k]) for k in ("level", "r", "c"))
            assert np.array_equal(bits(res["scores"]), bits(ref["scores"])) and np.array_equal(bits(res["boxes"]), bits(ref["boxes"]))
        elif keeper == "stream":
            order = [i, 1 - i, 1 - i, i]
            outs = list(K.detect_stream([imgs[j] for j in order], lanes=1, batch=2))
            assert len(outs) == 4
            for j, b in zip(order, outs):
                assert np.array_equal(bits(b.get()), bits(sh["K"][j]["boxes"]))
                assert np.array_equal(bits(b.get_field("scores")), bits(sh["K"][j]["scores"]))
        else:
            out = wb.detect(imgs[i], K, P)
            boxes, scores = compose([sh["K"][i], sh["P"][i]])
            assert np.array_equal(bits(out.get()), bits(boxes)) and np.array_equal(bits(out.get_field("scores")), bits(scores))

    def engine():
        if keeper == "stream":
            (lanes,) = K._lanes.values()
            assert len(lanes) == 1
            return lanes[0][0]
        (eng,) = E._ENGINES.values()
        return eng

    for n in range(4):                                       # eager, (the rank buffer arrives,) captured
        call(n % 2)
        if kept(engine(), dm, keeper) is not None:
            break
    eng = engine()
    assert kept(eng, dm, keeper) is not None, "no graph after four calls"
    generation, others = eng.generation, []
    if realloc == "det":
        eng.det_capacity = 64                                # far below the image's detections: the calls grow it again
        eng._alloc_det()
    elif realloc == "ctrl":
        others.append(keeper_model(44, 64))
        words = eng._alive_words
        eng._casc_state(others[0].device_cascade())          # 64 stages of statistics: a larger control block
        assert eng._alive_words > words
    else:
        others.append(keeper_model())
        wide = others[0].device_cascade()
        wide.rank_dtype = nat.WB_DTYPE_RANK16
        assert eng.rank.element_size() == 1
        eng.run_channels(wide, floats=False)                 # the other width
        assert eng.rank.element_size() == 2
    assert eng.generation > generation
    assert kept(eng, dm, keeper) is None
    for i in range(2):
        call(i)
    if realloc == "rank":
        assert eng.rank.element_size() == 1                  # (back at the keeper's width: a second re-allocation)
