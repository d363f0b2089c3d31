"""The box-regression kernels at the C ABI on the designs of tests/regress_designs.py (proved on the CPU by
tests/test_regress_designs_host.py): wb_gram_launch against exact integer Grams and the any-order bound,
wb_regress_predict_launch and wb_regress_apply_launch bit for bit against the statement (tests/regress_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import regress_designs as rd
import regress_reference as rr
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu


def dev():
    return nat.require_gpu()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def code(dtype):
    return nat.WB_DTYPE_U8 if np.dtype(dtype) == np.uint8 else nat.WB_DTYPE_F32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def gram(X, T, S=None, fill=0xFF):
    """S (+)= A^T A through wb_gram_launch on a scratch pre-filled with `fill` bytes; the host array."""
    lib = nat.load()
    N, D = X.shape
    S = torch.zeros((D + 5, D + 5), dtype=torch.float64, device=dev()) if S is None else up(S)
    need = C.c_size_t()
    nat.check(lib.wb_gram_scratch_bytes(N, D, C.byref(need)), "wb_gram_scratch_bytes")
    scratch = torch.full((max(need.value, 8),), fill, dtype=torch.uint8, device=dev())
    Xd, Td = up(X), up(np.asarray(T, np.float64).reshape(N, 4))
    nat.check(lib.wb_gram_launch(nat.stream_ptr(), nat.ptr(Xd), code(X.dtype), nat.ptr(Td), N, D, nat.ptr(S), nat.ptr(scratch), need.value),
              "wb_gram_launch")
    return S.cpu().numpy()


@pytest.mark.parametrize("D", rd.GRAM_D)
def test_gram_is_exact_on_integer_designs(D):
    """uint8 X and integer T: == against int64 A^T A at every N; two calls on the halves equal one call; a non-zero S on entry
    is kept; the scratch's content on entry (0xFF bytes: NaNs) does not matter."""
    for N in rd.GRAM_N:
        X, T, want = rd.gram_case(N, D)
        got = gram(X, T)
        assert np.array_equal(got, want.astype(np.float64)), (N, D, np.argwhere(got != want)[:8])
        assert np.array_equal(gram(X, T, fill=0), got)
        if N > 1:
            h = N // 2
            assert np.array_equal(gram(X[h:], T[h:], S=gram(X[:h], T[:h])), got), (N, D)
        S0 = rd.gram_case(7, D, seed=1)[2].astype(np.float64)
        assert np.array_equal(gram(X, T, S=S0), S0 + want), (N, D)


def test_gram_takes_no_rows():
    S0 = rd.gram_case(7, 11, seed=1)[2].astype(np.float64)
    assert np.array_equal(gram(np.zeros((0, 11), np.uint8), np.zeros((0, 4)), S=S0), S0)


def test_gram_of_floats_lies_within_the_any_order_bound_and_is_deterministic():
    """float32 X with non-integers and double T at N = 261, P = 21: every entry within (N + 8) * 2^-52 * (|A|^T |A|) of the
    exact rational value; bitwise symmetric; two runs bit-identical."""
    X, T, exact, absgram = rd.float_gram_case()
    N = X.shape[0]
    bound = rd.gram_bound(N, absgram)
    got = gram(X, T)
    worst = max(float(abs(rd.Fraction(float(got[i, j])) - exact[i, j]) / rd.Fraction(float(bound[i, j])))
                for i in range(got.shape[0]) for j in range(got.shape[1]))
    print(f"float Gram, N = {N}, P = {got.shape[0]}: largest |error| / bound = {worst:.3g}")
    assert rd.within(got, exact, bound)
    assert np.array_equal(bits(got), bits(got.T))
    assert np.array_equal(bits(gram(X, T)), bits(got))
    assert np.array_equal(bits(gram(X, T, fill=0)), bits(got))
    # a second batch on top: still symmetric, still the same bits run to run
    again = gram(X[::-1], T[::-1], S=got)
    assert np.array_equal(bits(again), bits(again.T)) and np.array_equal(bits(gram(X[::-1], T[::-1], S=got)), bits(again))


def predict(X, W, b):
    lib = nat.load()
    n, m, nn, Cc = X.shape
    out = torch.full((n, 4), np.nan, dtype=torch.float64, device=dev())
    Xd, Wb = up(X), up(np.concatenate([W, np.asarray(b)[None]]))
    nat.check(lib.wb_regress_predict_launch(nat.stream_ptr(), nat.ptr(Xd), code(X.dtype), n, m, nn, Cc, nat.ptr(Wb), nat.ptr(out)),
              "wb_regress_predict_launch")
    return out.cpu().numpy()


def apply(buf, levels, Cc, shape, recs, W, b, scales, n_images=2, want_pred=True):
    """(pred or None, boxes, err) of wb_regress_apply_launch on records (image, level, r, c)."""
    lib = nat.load()
    m, nn, _ = shape
    table = np.zeros(len(levels), nat.MINE_LEVEL_DTYPE)
    for l, (off, u, v) in enumerate(levels):
        table[l] = (off, u, v)
    det = np.zeros(len(recs), nat.DET_DTYPE)
    det["image"], det["level"], det["r"], det["c"] = recs[:, 0], recs[:, 1], recs[:, 2], recs[:, 3]
    inv32 = np.array([np.float32(1.0 / s) for s in scales], np.float32)
    inv64 = np.array([1.0 / s for s in scales], np.float64)
    n = len(recs)
    bufd, tabd, detd, Wb = up(buf), up(table.view(np.uint8)), up(det.view(np.uint8)), up(np.concatenate([W, np.asarray(b)[None]]))
    i32, i64 = up(inv32), up(inv64)
    pred = torch.full((n, 4), np.nan, dtype=torch.float64, device=dev()) if want_pred else None
    boxes = torch.full((n, 4), np.nan, dtype=torch.float32, device=dev())
    err = torch.full((1,), 7, dtype=torch.int32, device=dev())
    nat.check(lib.wb_regress_apply_launch(nat.stream_ptr(), nat.ptr(bufd), code(buf.dtype), buf.shape[1], n_images, nat.ptr(tabd), len(levels), Cc,
                                          nat.ptr(detd), n, m, nn, nat.ptr(Wb), nat.ptr(i32), nat.ptr(i64), nat.ptr(pred), nat.ptr(boxes),
                                          nat.ptr(err)), "wb_regress_apply_launch")
    return (pred.cpu().numpy() if want_pred else None), boxes.cpu().numpy(), int(err.item())


def grid_boxes(shape, recs, scales):
    m, nn, _ = shape
    inv32 = np.array([np.float32(1.0 / s) for s in scales], np.float32)
    rect = np.stack([recs[:, 3], recs[:, 2], recs[:, 3] + nn, recs[:, 2] + m], 1).astype(np.float32)
    return (rect * inv32[recs[:, 1]][:, None]).astype(np.float32)


SCALES = [0.5 * 2 ** (-k / 8) for k in (1, 3, 6)]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shape", rd.WINDOW_SHAPES)
def test_predict_and_apply_are_the_statement_bit_for_bit(shape, dtype):
    """One-hot weights (the feature order), integer weights (exact for uint8) and random doubles, n in {1, 63, 64, 65}; apply on a
    pyramid of two images and three levels equals predict on the gathered crops, in bits, and refines by the rule."""
    weights = [rd.one_hot_weights(shape)[:2], rd.integer_weights(shape), rd.random_weights(shape)]
    buf, levels, Cc = rd.pyramid_case(shape, dtype)
    for n in rd.PREDICT_N:
        X = rd.window_case(shape, n, dtype)
        recs = rd.pyramid_records(shape, levels, n)
        crops = rd.crops_of(buf, levels, Cc, shape, recs)
        grid = grid_boxes(shape, recs, SCALES)
        inv64 = np.array([1.0 / s for s in SCALES])[recs[:, 1]]
        for k, (W, b) in enumerate(weights):
            want = rr.predict(rr.features(X), W, b)
            got = predict(X, W, b)
            assert np.array_equal(bits(got), bits(want)), (shape, n, k)
            if k == 0:
                picks = rd.one_hot_weights(shape)[2]
                assert np.array_equal(got, np.stack([X[:, r, c, ch] for r, c, ch in picks], 1).astype(np.float64) + b)
            if k == 1 and np.dtype(dtype) == np.uint8:
                assert np.array_equal(got, rd.exact_predict(X, W, b))
            on_crops = predict(crops, W, b)
            assert np.array_equal(bits(on_crops), bits(rr.predict(rr.features(crops), W, b)))
            pred, boxes, err = apply(buf, levels, Cc, shape, recs, W, b, SCALES)
            assert err == 0 and np.array_equal(bits(pred), bits(on_crops)), (shape, n, k)
            assert np.array_equal(bits(boxes), bits(rr.refine(grid, on_crops, inv64))), (shape, n, k)
            if k == 2 and n == 65:
                none, boxes2, err = apply(buf, levels, Cc, shape, recs, W, b, SCALES, want_pred=False)
                assert none is None and err == 0 and np.array_equal(bits(boxes2), bits(boxes))


def test_refine_uses_the_float64_reciprocal():
    """Offsets of a thousand level pixels: float32(1 / scale) in place of inv64 would move the box by more than a float32 ulp."""
    shape = (2, 2, 1)
    boxes, pred, scales, level = rd.refine_case()
    buf, levels, Cc = rd.pyramid_case(shape, np.uint8)
    levels = [levels[i % 3] for i in range(len(scales))]
    recs = np.stack([np.zeros(64, np.int64), level, np.arange(64) % 2, np.arange(64) % 2], 1)
    b = pred[0]                                               # zero weights: every record's pred is the intercept
    got_pred, got, err = apply(buf, levels, Cc, shape, recs, np.zeros((4, 4)), b, list(scales))
    grid = grid_boxes(shape, recs, list(scales))
    assert err == 0 and np.array_equal(got_pred, np.broadcast_to(b, (64, 4)))
    want = rr.refine(grid, got_pred, (1.0 / scales)[level])
    wrong = rr.refine(grid, got_pred, np.array([np.float32(1.0 / s) for s in scales]).astype(np.float64)[level])
    assert (want != wrong).any() and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_record_outside_its_level_sets_err_and_keeps_its_box(dtype):
    shape = (5, 7, 3)
    buf, levels, Cc = rd.pyramid_case(shape, dtype)
    W, b = rd.random_weights(shape)
    recs = rd.pyramid_records(shape, levels, 9)
    good = apply(buf, levels, Cc, shape, recs, W, b, SCALES)
    assert good[2] == 0
    m, nn, _ = shape
    off, u, v = levels[1]
    for bad in ((0, 1, u - m + 1, 0), (1, 1, 0, v - nn + 1), (2, 0, 0, 0), (-1, 0, 0, 0), (0, 3, 0, 0), (0, -1, 0, 0)):
        mixed = recs.copy()
        mixed[4] = bad
        pred, boxes, err = apply(buf, levels, Cc, shape, mixed, W, b, SCALES)
        assert err == 1, bad
        keep = np.arange(9) != 4
        assert np.array_equal(bits(pred[keep]), bits(good[0][keep])) and np.array_equal(bits(boxes[keep]), bits(good[1][keep]))
        clamped = np.array([[0, min(max(bad[1], 0), 2), bad[2], bad[3]]])
        assert np.array_equal(bits(boxes[4:5]), bits(grid_boxes(shape, clamped, SCALES))) and np.all(pred[4] == 0), bad
    # a level that leaves the image's stride
    short = [levels[0], levels[1], (buf.shape[1] - 8, levels[2][1], levels[2][2])]
    on2 = recs[recs[:, 1] == 2]
    pred, boxes, err = apply(buf, short, Cc, shape, on2, W, b, SCALES)
    assert err == 1 and np.array_equal(bits(boxes), bits(grid_boxes(shape, on2, SCALES)))
    # no records: err is cleared, nothing is launched
    assert apply(buf, levels, Cc, shape, recs[:0], W, b, SCALES)[2] == 0
