"""The designs of tests/verify_designs.py prove themselves on the host: every design's chains stay below 2^24 (so the
integer expectation holds in any accumulation order), the NumPy contract reproduces the expectation bit for bit, and every
emulated wrong kernel is caught by a design that is named here."""
import numpy as np
import pytest

import verify_designs as vd
import verify_reference as ref

SHAPES = [(2, 2, 1), (3, 5, 2), (12, 12, 4), (14, 14, 1)]          # ((32, 32, 16) alike: tests/test_gpu_verify_designs.py)
SLIP_SHAPE = (5, 7, 3)                                             # odd both ways, m != n, C no power of two

# wrong kernel -> the design of SLIP_SHAPE on which it differs from the contract
CAUGHT_BY = {
    "convolution": "corners_edges",
    "swapped_ky_kx": "corners_edges",
    "chw_flatten": "flat_pick",
    "pool_ceil": "flat_pick",
    "pool_before_bn": "batchnorm",
    "bn_without_mean": "batchnorm",
    "dense_transposed": "mixed",
    "score_before_last": "mixed",
    "pad_replicate": "corners_edges",
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES + [SLIP_SHAPE], ids=str)
def test_designs_are_exact_integers_and_the_contract_reproduces_them(shape):
    names = []
    for d in vd.designs(shape):
        want, bound, lows = vd.expected(d)
        assert bound < 2 ** 24, (d["name"], bound)
        got = ref.predict(d["arrays"], d["epsilon"], d["X"], d["scores"])
        assert np.array_equal(bits(got), bits(want)), (d["name"], got, want)
        if d["name"] == "mixed":
            assert all(v < 0 for v in lows), lows              # a negative pre-activation in front of every ReLU
            assert np.any(d["scores"] > 0) and np.any(d["scores"] < 0)
        names.append(d["name"])
    assert names == ["corners_edges", "routes", "pool_winners", "flat_pick", "batchnorm", "mixed"]


def test_designs_of_the_largest_shape_stay_below_2_to_24():
    for d in vd.designs((32, 32, 16)):
        d = dict(d, X=d["X"][:2], scores=d["scores"][:2])
        assert vd.expected(d)[1] < 2 ** 24, d["name"]


def test_pool_design_lets_every_candidate_win():
    d = next(d for d in vd.designs((4, 6, 2)) if d["name"] == "pool_winners")
    for k in range(4):
        cell = d["X"][k, :2, :2, 0]
        assert np.argmax(cell) == k and np.sum(cell == cell.max()) == 1


def test_batchnorm_design_has_power_of_two_scales_and_a_negative_one():
    d = next(d for d in vd.designs(SLIP_SHAPE) if d["name"] == "batchnorm")
    for k, want in enumerate((2.0, -2.0, 4.0, 2.0)):
        gamma, beta, mean, var = (d["arrays"][6 * k + j].astype(np.float64) for j in (2, 3, 4, 5))
        assert np.array_equal(gamma / np.sqrt(var + d["epsilon"]), np.full(gamma.shape, want))
        assert np.all(mean != 0) and np.any(beta != 0)


@pytest.mark.parametrize("slip", sorted(vd.WRONG))
def test_every_wrong_kernel_is_caught_by_its_design(slip):
    d = next(d for d in vd.designs(SLIP_SHAPE) if d["name"] == CAUGHT_BY[slip])
    want = vd.expected(d)[0]
    wrong = vd.WRONG[slip](d)
    assert wrong.shape == want.shape and not np.array_equal(wrong, want), slip


def test_the_list_of_wrong_kernels_is_the_designed_one():
    assert set(vd.WRONG) == set(CAUGHT_BY) and len(vd.WRONG) == 9
