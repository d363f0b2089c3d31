"""The designs of tests/regress_designs.py, proved on the CPU: the emulated kernels give the exact answers, and every
emulated mistake -- the f32 C/D row map on the f64 MFMA, swapped row and column on write-back, a missing mirror, a dropped
tail chunk, a dropped k-remainder N % 4, an fp32 accumulator, the (c, r, ch) feature order, a missing intercept row,
inv_scale in place of inv64 -- shows on them.  tests/test_gpu_regress_designs.py holds the kernels to the same answers."""
from fractions import Fraction

import numpy as np
import pytest

import regress_designs as rd
import regress_reference as rr


@pytest.mark.parametrize("D", rd.GRAM_D)
def test_the_emulated_gram_is_exact_at_every_size(D):
    for N in rd.GRAM_N:
        X, T, want = rd.gram_case(N, D)
        A = rd.integer_design(X, T)
        assert want.dtype == np.int64 and want[D, D] == N and int(want.max()) < 2 ** 53
        assert np.array_equal(rd.emulate_gram(A), want), (N, D)
        assert np.array_equal(rr.gram(X, T), want.astype(np.float64))         # float64 holds every partial sum exactly
        if N > 1:
            h = N // 2
            assert np.array_equal(rd.emulate_gram(A[h:], S0=rd.emulate_gram(A[:h])), want)


def test_the_gram_designs_are_asymmetric_and_beyond_fp32():
    X, T, want = rd.gram_case(513, 123)
    assert want[0, 0] == 255 ** 2 * 513 > 2 ** 24 and want[0, 0] % 2 == 1
    assert np.float32(want[0, 0]) != want[0, 0]
    A = rd.integer_design(X, T)
    assert len({tuple(c) for c in A.T}) == A.shape[1]                         # no two columns agree


# where each mistake must show: (N, D) chosen so that the mistaken path exists at all
SHOWS = {
    "f32_cd_map": [(5, 1), (257, 123)],                       # one tile is enough: rows 1, 2, 3 of it are misplaced
    "swapped_write_back": [(5, 12), (257, 123)],              # needs an off-diagonal tile: P >= 17
    "missing_mirror": [(5, 1), (257, 123)],
    "dropped_tail_chunk": [(255, 11), (257, 59), (513, 123)], # N % 256 != 0
    "dropped_k_remainder": [(1, 11), (3, 1), (5, 60), (257, 123)],   # N % 4 != 0
    "fp32_accumulator": [(513, 1), (513, 123)],
}


@pytest.mark.parametrize("fault", rd.GRAM_FAULTS)
def test_every_emulated_gram_mistake_shows(fault):
    for N, D in SHOWS[fault]:
        X, T, want = rd.gram_case(N, D)
        got = rd.emulate_gram(rd.integer_design(X, T), fault)
        assert not np.array_equal(got, want), (fault, N, D)


def test_the_float_gram_case_and_its_bound():
    X, T, exact, absgram = rd.float_gram_case()
    N, P = X.shape[0], X.shape[1] + 5
    assert (N, P) == (261, 21) and X.dtype == np.float32 and np.any(X != np.round(X))
    assert isinstance(exact[0, 1], Fraction) and exact[16, 16] == N
    bound = rd.gram_bound(N, absgram)
    S = rr.gram(X, T)
    assert rd.within(S, exact, bound)                          # NumPy's own order lies inside the any-order bound
    assert not rd.within(S + 4 * bound, exact, bound)
    # an fp32 accumulator is far outside it
    A32 = rr.design(X, T).astype(np.float32)
    assert not rd.within((A32.T @ A32).astype(np.float64), exact, bound)


@pytest.mark.parametrize("shape", rd.WINDOW_SHAPES)
def test_predict_designs_are_exact_and_pin_the_feature_order(shape):
    m, nn, C = shape
    for n in rd.PREDICT_N:
        X = rd.window_case(shape, n, np.uint8)
        W, b, picks = rd.one_hot_weights(shape)
        want = np.stack([X[:, r, c, ch] for r, c, ch in picks], 1).astype(np.float64) + b
        assert np.array_equal(rd.emulate_predict(X, W, b), want)
        Wi, bi = rd.integer_weights(shape)
        assert np.array_equal(rd.emulate_predict(X, Wi, bi), rd.exact_predict(X, Wi, bi))
    X = rd.window_case(shape, 65, np.uint8)
    for W, b in (rd.one_hot_weights(shape)[:2], rd.integer_weights(shape)):
        want = rd.emulate_predict(X, W, b)
        for fault in rd.PREDICT_FAULTS:
            assert not np.array_equal(rd.emulate_predict(X, W, b, fault), want), (shape, fault)


def test_the_refine_design_tells_inv64_from_inv_scale():
    boxes, pred, scales, level = rd.refine_case()
    inv64 = 1.0 / scales
    inv32 = np.array([np.float32(v) for v in inv64], np.float32)
    assert np.all(inv32.astype(np.float64) != inv64)
    want = rr.refine(boxes, pred, inv64[level])
    wrong = rr.refine(boxes, pred, inv32.astype(np.float64)[level])
    assert want.dtype == np.float32 and (want != wrong).mean() > 0.1
    # the rule, element by element in exact arithmetic: one rounding of the product, one of the difference, one to float32
    for i in range(0, 64, 7):
        for k in range(4):
            prod = float(Fraction(float(pred[i, k])) * Fraction(float(inv64[level[i]])))
            assert want[i, k] == np.float32(float(Fraction(float(boxes[i, k])) - Fraction(prod)))


def test_pyramid_designs_reach_the_last_row_and_column():
    for shape in rd.WINDOW_SHAPES:
        for dtype in (np.uint8, np.float32):
            buf, levels, C = rd.pyramid_case(shape, dtype)
            recs = rd.pyramid_records(shape, levels, 65)
            m, nn, _ = shape
            assert buf.shape[0] == 2 and len(levels) == 3 and recs.shape == (65, 4)
            assert all(off + u * v * C <= buf.shape[1] for off, u, v in levels)
            for l, (off, u, v) in enumerate(levels):
                assert any(tuple(w[1:]) == (l, u - m, v - nn) for w in recs)
            assert all(r + m <= levels[l][1] and c + nn <= levels[l][2] for _, l, r, c in recs)
            crops = rd.crops_of(buf, levels, C, shape, recs)
            b, l, r, c = recs[-1]
            off, u, v = levels[l]
            assert crops[-1][m - 1, nn - 1, C - 1] == buf[b, off + ((r + m - 1) * v + c + nn - 1) * C + C - 1]
