"""What waldboost_amd.calibration decides on the host, without a GPU: the argument errors, the keep arithmetic, the result
object, pools as input, and the two declarations in the header."""
import math
import os
import re

import numpy as np
import pytest

import calib_designs as cd
import calib_reference as ref
import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd import calibration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model():
    return cd.designs()["ties-257x4"].model()


def X(n=5, shape=cd.SHAPE):
    return np.zeros((n,) + tuple(shape), np.uint8)


def test_the_module_is_exported():
    assert wb.calibration is calibration and wb.calibrate is calibration.calibrate
    assert "calibration" in wb.__all__ and "calibrate" in wb.__all__
    assert callable(wb.Model.stage_scores)


@pytest.mark.parametrize("recall", [0.0, -0.1, 1.0000001, 2, float("nan"), float("inf")])
def test_recall_outside_0_1_is_refused(recall):
    with pytest.raises(ValueError, match="recall"):
        wb.calibrate(model(), X(), recall=recall)


@pytest.mark.parametrize("margin", [-1e-9, -1, float("nan"), float("inf"), float("-inf")])
def test_a_negative_or_non_finite_margin_is_refused(margin):
    with pytest.raises(ValueError, match="margin"):
        wb.calibrate(model(), X(), margin=margin)


def test_shape_count_and_model_errors():
    M = model()
    for bad in (X(5, (8, 8, 3)), X(5, (7, 8, 4)), np.zeros((5, 8, 8), np.uint8), np.zeros(5, np.uint8)):
        with pytest.raises(ValueError, match="shape"):
            wb.calibrate(M, bad)
        with pytest.raises(ValueError, match="shape"):
            M.stage_scores(bad)
        with pytest.raises(ValueError, match="shape"):
            calibration.stage_survival(M, bad)
        with pytest.raises(ValueError, match="shape"):
            calibration.expected_cost(M, bad)
    with pytest.raises(ValueError, match="at least one positive"):
        wb.calibrate(M, X(0))
    with pytest.raises(ValueError, match="at least one sample"):
        calibration.expected_cost(M, X(0))
    with pytest.raises(ValueError, match="at least one stage"):
        wb.calibrate(wb.Model(cd.SHAPE, dict(wb.default_channel_opts)), X())
    assert M.theta == cd.designs()["ties-257x4"].thetas                    # a refused call changes nothing


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_prediction_is_refused(bad):
    M = model()
    M.classifier[2].prediction[1] = bad                                    # a leaf of stage 2
    with pytest.raises(ValueError, match="stage 2 has a non-finite prediction"):
        wb.calibrate(M, X())
    M = model()
    M.classifier[2].prediction[0] = bad                                    # the root's own entry is never a score
    with pytest.raises(ValueError, match="at least one positive"):
        wb.calibrate(M, X(0))


def test_stage_scores_refuses_2_31_entries_and_answers_empty_inputs_without_a_launch():
    M = model()

    class Many:
        shape = (2 ** 29, ) + cd.SHAPE
        dtype = np.dtype(np.uint8)

    with pytest.raises(ValueError, match=r"2\*\*31"):
        M.stage_scores(Many())
    got = M.stage_scores(X(0))
    assert got.shape == (0, 4) and got.dtype == np.float32
    E = wb.Model(cd.SHAPE, dict(wb.default_channel_opts))
    got = E.stage_scores(X(3))
    assert got.shape == (3, 0) and got.dtype == np.float32
    assert np.array_equal(calibration.stage_survival(M, X(0)), np.zeros(5, np.int64))


def test_keep_arithmetic():
    k = calibration.keep_count
    assert [k(r, 100) for r in (1e-9, 0.01, 0.0101, 0.5, 0.99, 0.991, 1.0)] == [1, 1, 2, 50, 99, 100, 100]
    assert k(0.25, 257) == 65 and k(0.249, 257) == 64                      # either side of a ceil step
    assert k(0.3, 1) == 1 and k(1.0, 1) == 1
    for n in (1, 2, 63, 1000):
        for r in (1e-6, 0.1, 1 / 3, 0.5, 0.999, 1.0):
            assert k(r, n) == ref.keep_count(r, n) == min(n, max(1, math.ceil(r * n)))
            assert 1 <= k(r, n) <= n


def test_the_result_object():
    res = calibration.Calibration(np.array([1.5, -2.0], np.float32), [float("-inf"), 0.25], -0.5, 8, 6)
    assert (res.n, res.retained, res.recall, res.floor) == (8, 6, 0.75, -0.5)
    assert res.old_theta == [float("-inf"), 0.25] and res.theta.dtype == np.float32
    assert "6/8" in repr(res) and "stages=2" in repr(res)
    with pytest.raises(AttributeError):
        res.other = 1


class StubPool:
    """A pool as calibrate sees one: get_true_positives() -> (X, H)."""

    def __init__(self, X):
        self.X, self.asked = X, 0

    def get_true_positives(self):
        self.asked += 1
        return self.X, np.zeros(len(self.X), np.float32)

    def get_false_positives(self):
        raise AssertionError("calibrate prunes on the positives")


def test_a_pool_hands_in_its_true_positives():
    M = model()
    pool = StubPool(X(0))
    with pytest.raises(ValueError, match="at least one positive"):
        wb.calibrate(M, pool)
    assert pool.asked == 1
    pool = StubPool(X(4, (8, 8, 3)))
    with pytest.raises(ValueError, match=r"given \(4, 8, 8, 3\)"):
        wb.calibrate(M, pool)
    assert pool.asked == 1
    for cls in (wb.SamplePool, wb.DeviceSamplePool):
        assert callable(cls.get_true_positives)


def test_the_header_declares_the_two_exports_and_the_binding_follows():
    header = open(os.path.join(ROOT, "include", "waldboost_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int wb_samples_trace_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples, "
            "int reject, float *trace, float *final, uint32_t *alive);") in flat
    assert ("int wb_calib_min_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples, "
            "float floor, float *stage_min, uint32_t *n_retained);") in flat
    assert re.search(r"^int wb_samples_trace_launch\(", header, re.M) and re.search(r"^int wb_calib_min_launch\(", header, re.M)
    assert len(nat.SYMBOLS["wb_samples_trace_launch"][1]) == 9 and len(nat.SYMBOLS["wb_calib_min_launch"][1]) == 8
    lib = nat.load()
    assert hasattr(lib, "wb_samples_trace_launch") and hasattr(lib, "wb_calib_min_launch")
    assert "#define WB_ABI_VERSION 8" in header
    # argument checks that need no device
    assert lib.wb_samples_trace_launch(None, None, None, nat.WB_DTYPE_U8, 0, 0, None, None, None) == 0
    assert lib.wb_samples_trace_launch(None, None, None, nat.WB_DTYPE_U8, -1, 0, None, None, None) == nat.WB_ERR_INVALID
    assert lib.wb_samples_trace_launch(None, None, None, nat.WB_DTYPE_U8, 3, 0, None, None, None) == nat.WB_ERR_INVALID
    assert lib.wb_calib_min_launch(None, None, None, nat.WB_DTYPE_U8, 3, 0.0, None, None) == nat.WB_ERR_INVALID
