"""Host side of the verification CNN: the fmaf emulation of tests/verify_reference.py is correctly rounded (against
fractions.Fraction, and on constructed ties where the float64 shortcut rounds the other way), the batch-normalisation
fold, Verifier's construction, files and errors.  No GPU here: predict must say so."""
from fractions import Fraction

import numpy as np
import pytest

import verify_reference as ref
import waldboost_amd as wb
from waldboost_amd import verification as ver


def f32(x):
    return np.float32(x)


def exact_fmaf(a, b, c):
    """fma(a, b, c) rounded once to float32 (nearest, ties to even), by rational arithmetic; finite normal results."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    lo = np.float32(float(v))                       # a float32 near v: fix it up against its neighbours
    cands = sorted({lo, np.nextafter(lo, f32(np.inf)), np.nextafter(lo, f32(-np.inf))}, key=float)
    best = min(cands, key=lambda q: (abs(Fraction(float(q)) - v), int(np.float32(q).view(np.uint32)) & 1))
    return np.float32(best)


def test_fmaf_is_correctly_rounded_on_seeded_cases():
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(4000) * 2.0 ** rng.integers(-20, 20, 4000)).astype(np.float32)
    b = (rng.standard_normal(4000) * 2.0 ** rng.integers(-20, 20, 4000)).astype(np.float32)
    c = (rng.standard_normal(4000) * 2.0 ** rng.integers(-20, 20, 4000)).astype(np.float32)
    c[::5] = (-a[::5].astype(np.float64) * b[::5]).astype(np.float32)          # heavy cancellation
    got = ref.fmaf(a, b, c)
    want = np.array([exact_fmaf(*t) for t in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fmaf_on_ties_where_the_float64_shortcut_rounds_the_other_way():
    # a * b = 2^-24 - 2^-54: just below half an ulp of c; float64 rounds c + a * b to the tie 1 + 2^-23 + 2^-24 exactly
    a, b, c = f32(2.0 ** -24 * (1 + 2.0 ** -15)), f32(1 - 2.0 ** -15), f32(1 + 2.0 ** -23)
    assert ref.fmaf(a, b, c) == f32(1 + 2.0 ** -23) == exact_fmaf(a, b, c)
    assert ref.fmaf_shortcut(a, b, c) == f32(1 + 2.0 ** -22)
    # the mirror image
    assert ref.fmaf(-a, b, -c) == f32(-(1 + 2.0 ** -23)) and ref.fmaf_shortcut(-a, b, -c) == f32(-(1 + 2.0 ** -22))
    # exact ties stay ties to even; signed zeros and infinities pass through
    assert ref.fmaf(f32(2.0 ** -24), f32(1.0), f32(1.0)) == f32(1.0)
    assert ref.fmaf(f32(2.0 ** -24), f32(1.0), f32(1 + 2.0 ** -23)) == f32(1 + 2.0 ** -22)
    assert np.signbit(ref.fmaf(f32(0.0), f32(3.0), f32(-0.0))) == np.signbit(np.float32(0.0 * 3.0 + -0.0))
    assert ref.fmaf(f32(np.inf), f32(1.0), f32(1.0)) == np.inf
    # a subnormal result
    tiny = f32(2.0 ** -149)
    assert ref.fmaf(tiny, f32(0.5), tiny) == f32(2.0 ** -148)          # 1.5 * 2^-149: a tie, to even (2 * 2^-149)
    assert ref.fmaf(tiny, f32(0.5), f32(2.0 ** -148)) == f32(2.0 ** -148)   # 2.5 * 2^-149: a tie, to even


def _random_arrays(shape, seed):
    """model_cnn's arrays with non-trivial batch-normalisation statistics and biases."""
    rng = np.random.default_rng(seed)
    arrays = ver.model_cnn(shape, seed=seed).get_weights()
    for k in range(4):
        cout = arrays[6 * k + 1].size
        arrays[6 * k + 1] = (rng.standard_normal(cout) * 0.1).astype("f")
        arrays[6 * k + 2] = rng.uniform(0.5, 1.5, cout).astype("f") * rng.choice([-1, 1], cout).astype("f")
        arrays[6 * k + 3] = (rng.standard_normal(cout) * 0.2).astype("f")
        arrays[6 * k + 4] = (rng.standard_normal(cout) * 0.3).astype("f")
        arrays[6 * k + 5] = rng.uniform(0.2, 2.0, cout).astype("f")
    arrays[25] = (rng.standard_normal(128) * 0.1).astype("f")
    arrays[27] = np.array([0.25], "f")
    return arrays


def test_fold_agrees_with_the_unfused_float64_evaluation():
    shape = (6, 5, 3)
    arrays = _random_arrays(shape, 3)
    V = ver.Verifier.from_keras_weights(shape, arrays, epsilon=1e-3)
    folded, mine = V.folded(), ref.fold(arrays, 1e-3)
    # block 1 on a random padded window: conv, then BN as Keras states it, in float64, against the folded form.  They differ
    # by the one rounding of W' and of b' to float32: at most 2^-24 of sum |x| |W s| + |b'| per output (plus float64 noise)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6 + 2, 5 + 2, 3))
    W, b, gamma, beta, mean, var = (a.astype(np.float64) for a in arrays[:6])
    s = gamma / np.sqrt(var + 1e-3)
    fw, fb = (v.astype(np.float64) for v in folded[0])
    for r in range(6):
        for c in range(5):
            patch = x[r:r + 3, c:c + 3]
            bn = (np.einsum("yxi,yxio->o", patch, W) + b - mean) / np.sqrt(var + 1e-3) * gamma + beta
            fused = np.einsum("yxi,yxio->o", patch, fw) + fb
            bound = 2.0 ** -24 * (np.einsum("yxi,yxio->o", np.abs(patch), np.abs(W * s)) + np.abs(fb)) + 1e-12
            assert np.all(np.abs(fused - bn) <= bound)
    assert np.any(s < 0) and np.all(mean != 0)
    for (fw, fb), (rw, rb) in zip(folded[:4], mine[:4]):
        assert fw.dtype == np.float32 and np.array_equal(fw, rw) and np.array_equal(fb, rb)
    for a, b in zip(folded[4:], mine[4:]):
        assert np.array_equal(a.reshape(-1), b.reshape(-1))
    # the packed buffer is the header's layout: conv kernels and biases in turn, then the dense layers
    packed = V._packed
    want = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in mine[:4]] + [v.reshape(-1) for v in mine[4:]])
    assert packed.dtype == np.float32 and np.array_equal(packed, want)


def test_from_keras_weights_checks_order_shapes_and_values():
    shape = (6, 5, 3)
    arrays = _random_arrays(shape, 1)
    V = ver.Verifier.from_keras_weights(shape, arrays)
    assert V.input_shape == shape and V.epsilon == 1e-3 and len(V.get_weights()) == 28
    assert [a.shape for a in V.get_weights()][:7] == [(3, 3, 3, 8)] + [(8,)] * 5 + [(3, 3, 8, 8)]
    assert V.get_weights()[24].shape == (3 * 2 * 16, 128) and V.get_weights()[26].shape == (128, 1)
    arrays[0][0, 0, 0, 0] = 5.0                                   # (the verifier keeps copies)
    assert V.get_weights()[0][0, 0, 0, 0] != 5.0
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights(shape, arrays[:27])
    swapped = list(arrays)
    swapped[0], swapped[6] = swapped[6], swapped[0]               # blocks in the wrong order
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights(shape, swapped)
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights((6, 7, 3), arrays)        # dense kernel of another window
    bad = list(arrays)
    bad[3] = bad[3].copy()
    bad[3][2] = np.nan
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights(shape, bad)
    bad = list(arrays)
    bad[5] = np.full(8, -1.0, "f")                                # variance + epsilon < 0: the fold is not finite
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights(shape, bad)
    with pytest.raises(ValueError):
        ver.Verifier.from_keras_weights((6, 5), arrays)


def test_model_cnn_uses_keras_default_initialisers():
    V = ver.model_cnn((14, 14, 4), seed=5)
    a = V.get_weights()
    assert V.input_shape == (14, 14, 4) and V.epsilon == 1e-3
    for k, (cin, cout) in enumerate(zip((4, 8, 8, 16), (8, 8, 16, 16))):
        limit = np.sqrt(6.0 / (9 * cin + 9 * cout))
        W = a[6 * k]
        assert W.shape == (3, 3, cin, cout) and np.abs(W).max() <= limit and np.abs(W).max() > 0.8 * limit
        assert not a[6 * k + 1].any() and np.all(a[6 * k + 2] == 1) and not a[6 * k + 3].any()
        assert not a[6 * k + 4].any() and np.all(a[6 * k + 5] == 1)
    assert a[24].shape == (7 * 7 * 16, 128) and np.abs(a[24]).max() <= np.sqrt(6.0 / (784 + 128))
    assert not a[25].any() and not a[27].any()
    assert np.array_equal(ver.model_cnn((14, 14, 4), seed=5).get_weights()[0], a[0])
    assert not np.array_equal(ver.model_cnn((14, 14, 4), seed=6).get_weights()[0], a[0])


def test_npz_round_trip_without_pickle(tmp_path):
    V = ver.Verifier.from_keras_weights((6, 5, 3), _random_arrays((6, 5, 3), 2), epsilon=0.01)
    path = str(tmp_path / "verifier.npz")
    V.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert len(z.files) == 30
    W = ver.Verifier.load(path)
    assert W.input_shape == V.input_shape and W.epsilon == V.epsilon
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(V.get_weights(), W.get_weights()))
    assert np.array_equal(V._packed, W._packed)


def test_train_points_to_the_reference_and_exploss_is_the_reference_formula():
    with pytest.raises(NotImplementedError) as e:
        ver.train(None, None, None, None, None)
    assert "from_keras_weights" in str(e.value) and "get_weights()" in str(e.value) and "reference" in str(e.value)
    y, p = np.array([1.0, -1.0, 1.0, -1.0]), np.array([0.5, 0.5, 100.0, 100.0])
    assert np.allclose(ver.exploss(y, p), [np.exp(-0.5), np.exp(0.5), 1e-6, 1e3])
    assert wb.verification is ver


def test_predict_checks_its_input_and_needs_a_gpu():
    import torch
    V = ver.model_cnn((6, 5, 3), seed=0)
    X, H = np.zeros((4, 6, 5, 3), "f"), np.zeros(4, "f")
    with pytest.raises(ValueError):
        V.predict([X[:, :5], H])
    with pytest.raises(ValueError):
        V.predict([X, H[:3]])
    with pytest.raises(ValueError):
        V.predict([np.where(np.arange(3) == 1, np.nan, X).astype("f"), H])
    with pytest.raises(NotImplementedError):
        V.predict([X.astype(np.float64), H])
    with pytest.raises(NotImplementedError):
        V.predict([X.astype(np.int16), H])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            V.predict([X, H])
        with pytest.raises(RuntimeError):
            V.predict([X.astype(np.uint8), H.reshape(4, 1)])


def test_unsupported_window_shapes_are_refused_at_the_c_abi():
    import ctypes as C
    from waldboost_amd import _native as nat
    lib = nat.load()
    count, nbytes = C.c_int64(), C.c_size_t()
    for shape, F in [((12, 12, 4), 576), ((14, 14, 1), 784), ((14, 14, 4), 784), ((20, 20, 4), 1600), ((32, 32, 16), 4096),
                     ((2, 2, 1), 16), ((3, 5, 2), 32)]:
        assert lib.wb_verify_weights_floats(*shape, C.byref(count)) == 0
        Cc = shape[2]
        assert count.value == 72 * Cc + 8 + 576 + 8 + 1152 + 16 + 2304 + 16 + 128 * F + 128 + 128 + 1
        assert lib.wb_verify_scratch_bytes(*shape, 1000, C.byref(nbytes)) == 0 and nbytes.value == 4000 * F
    for shape in [(1, 12, 4), (12, 33, 4), (12, 12, 0), (12, 12, 17), (33, 2, 1)]:
        assert lib.wb_verify_weights_floats(*shape, C.byref(count)) == nat.WB_ERR_UNSUPPORTED
        assert "window shape" in nat.last_error()
        assert lib.wb_verify_scratch_bytes(*shape, 10, C.byref(nbytes)) == nat.WB_ERR_UNSUPPORTED
        assert lib.wb_verify_launch(None, None, nat.WB_DTYPE_F32, 0, *shape, None, None, None, 0, None) == nat.WB_ERR_UNSUPPORTED
    # nothing to do, and argument errors that need no device
    assert lib.wb_verify_launch(None, None, nat.WB_DTYPE_F32, 0, 12, 12, 4, None, None, None, 0, None) == 0
    assert lib.wb_verify_launch(None, None, nat.WB_DTYPE_F64, 5, 12, 12, 4, None, None, None, 0, None) == nat.WB_ERR_UNSUPPORTED
    assert lib.wb_verify_launch(None, None, nat.WB_DTYPE_F32, -1, 12, 12, 4, None, None, None, 0, None) == nat.WB_ERR_INVALID
    assert lib.wb_verify_launch(None, None, nat.WB_DTYPE_F32, 5, 12, 12, 4, None, None, None, 0, None) == nat.WB_ERR_INVALID
    assert "null" in nat.last_error()
    assert lib.wb_verify_launch(None, 1024, nat.WB_DTYPE_F32, 5, 12, 12, 4, 1024 + 8, 1024, 1024, 1 << 30, 1024) == nat.WB_ERR_INVALID
    assert "aligned" in nat.last_error()
    assert lib.wb_verify_launch(None, 1024, nat.WB_DTYPE_F32, 5, 12, 12, 4, 1024, 1024, 1024, 5 * 576 * 4 - 1, 1024) == nat.WB_ERR_INVALID
    assert "scratch" in nat.last_error()
    V = ver.model_cnn((40, 12, 4), seed=0)          # a verifier may be built for it, the kernels refuse it
    assert V.input_shape == (40, 12, 4)
