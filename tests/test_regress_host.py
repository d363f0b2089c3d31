"""CPU tests of box regression: the NumPy statement (tests/regress_reference.py) against numpy.linalg.lstsq, its residuals,
its prediction order, the end-to-end statement on the planted-square images with the oracle's pyramid, the package's host
side (BoxRegressor.from_state, save / load, the errors) and the new exports' argument checks and resource metadata."""
import ctypes as C
import functools

import numpy as np
import pytest

import regress_reference as rr
import waldboost_amd as wb
from oracle import wb_oracle as orc
from test_host import _kernel_scratch_sizes
from waldboost_amd import _native as nat
from waldboost_amd import regression

EPS = np.finfo(np.float64).eps
KERNELS = ("gram_partial_kernel", "gram_reduce_kernel", "regress_predict_kernel", "regress_apply_kernel")
EXPORTS = ("wb_gram_scratch_bytes", "wb_gram_launch", "wb_regress_predict_launch", "wb_regress_apply_launch")


def _problem(N=300, D=24, seed=0, l2=1e-2):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (N, D)).astype(np.float64) * rng.uniform(0.2, 1.0, D)
    T = X[:, :4] * 0.01 + rng.normal(0, 1, (N, 4)) + np.array([3.0, -2.0, 0.5, 10.0])
    return X, T, rr.gram(X, T), l2


def _ridge_system(S, l2):
    N, mu, tau, Cxx, Cxt, Ctt = rr.moments(S)
    D = mu.size
    lam = l2 * (np.trace(Cxx) / D)
    return lam, np.linalg.cond(Cxx + lam * np.eye(D))


@pytest.mark.parametrize("seed,l2", [(0, 1e-2), (1, 1e-3), (2, 1e-1), (3, 1e-6)])
def test_solve_agrees_with_lstsq_on_the_centred_ridge_system(seed, l2):
    """Relative tolerance 64 * eps * cond(Cxx + lambda I): the classical normal-equations bound, 64 for dimension factors."""
    X, T, S, _ = _problem(seed=seed)
    W, b, rss, tss = rr.solve(S, l2)
    lam, cond = _ridge_system(S, l2)
    N, D = X.shape
    Xc, Tc = X - X.mean(0), T - T.mean(0)
    want = np.linalg.lstsq(np.concatenate([Xc, np.sqrt(lam) * np.eye(D)]), np.concatenate([Tc, np.zeros((D, 4))]), rcond=None)[0]
    tol = 64 * EPS * cond
    print(f"seed {seed} l2 {l2:g}: cond {cond:.3g}, tolerance {tol:.3g}, relative difference {np.linalg.norm(W - want) / np.linalg.norm(want):.3g}")
    assert np.linalg.norm(W - want) <= tol * np.linalg.norm(want)
    assert np.linalg.norm(b - (T.mean(0) - want.T @ X.mean(0))) <= tol * (np.linalg.norm(T.mean(0)) + np.linalg.norm(want) * np.linalg.norm(X.mean(0)))
    # the training residual never exceeds that of predicting tau, and the RSS read from S is the directly computed one
    direct = ((T - (X @ W + b)) ** 2).sum(0)
    assert (direct <= tss).all() and (rss <= tss * (1 + tol)).all()
    assert (np.abs(rss - direct) <= tol * tss).all(), (rss, direct)
    reg = regression.BoxRegressor.from_state((2, 3, 4), S, l2)
    assert np.array_equal(reg.W, W) and np.array_equal(reg.b, b) and np.array_equal(reg.rss, rss) and np.array_equal(reg.tss, tss)
    assert reg.n_samples == N and reg.l2 == l2 and reg.input_shape == (2, 3, 4)


def _straight_predict(x, W, b):
    """The rule read aloud, one window, Python floats."""
    p = [[0.0] * 4 for _ in range(64)]
    for l in range(64):
        for j in range(l, x.size, 64):
            for k in range(4):
                p[l][k] = p[l][k] + float(x[j]) * float(W[j, k])
    for s in (32, 16, 8, 4, 2, 1):
        p = [[p[l][k] + p[l ^ s][k] for k in range(4)] for l in range(64)]
    return np.array([p[0][k] + float(b[k]) for k in range(4)])


def test_the_predict_order_is_observable_and_the_statement_keeps_it():
    differs = 0
    for D in (4, 105, 256):
        rng = np.random.default_rng(D)
        X, W, b = rng.normal(0, 30, (5, D)), rng.normal(0, 1, (D, 4)), rng.normal(0, 1, 4)
        got = rr.predict(X, W, b)
        for i in range(X.shape[0]):
            assert np.array_equal(got[i].view(np.uint64), _straight_predict(X[i], W, b).view(np.uint64))
        differs += int((got != X @ W + b).sum())
    assert differs > 0                                         # a plain x @ W rounds differently: the order can be seen


def test_statement_errors():
    X, T, S, _ = _problem(N=40, D=6)
    for bad in (rr.gram(X[:1], T[:1]), np.where(np.eye(11) > 0, np.nan, S), rr.gram(np.ones((40, 6)), T)):
        with pytest.raises(ValueError):
            rr.solve(bad)
        with pytest.raises(ValueError):
            regression.BoxRegressor.from_state((1, 6, 1), bad)
    with pytest.raises(ValueError):
        regression.BoxRegressor.from_state((1, 5, 1), S)       # another shape's state
    with pytest.raises(ValueError):
        regression.BoxRegressor.from_state((1, 6, 1), S, l2=-1.0)
    with pytest.raises(ValueError):
        regression.BoxRegressor((1, 6, 1), np.full((6, 4), np.inf), np.zeros(4))
    with pytest.raises(NotImplementedError):
        regression.BoxRegressor((32, 32, 2), np.zeros((2048, 4)), np.zeros(4))      # P = 2053
    with pytest.raises(ValueError):
        regression.BoxRegressor((8, 8), np.zeros((64, 4)), np.zeros(4))


def test_save_and_load_round_trip(tmp_path):
    X, T, S, l2 = _problem(N=60, D=12)
    reg = regression.BoxRegressor.from_state((2, 3, 2), S, l2, dtype=np.uint8)
    path = str(tmp_path / "reg.npz")
    reg.save(path)
    back = regression.BoxRegressor.load(path)
    for k in ("W", "b", "rss", "tss"):
        assert np.array_equal(getattr(back, k).view(np.uint64), getattr(reg, k).view(np.uint64)), k
    assert (back.input_shape, back.n_samples, back.l2, back.dtype) == (reg.input_shape, 60, l2, np.dtype(np.uint8))
    regression.BoxRegressor.from_state((2, 3, 2), S, l2).save(path)
    assert regression.BoxRegressor.load(path).dtype is None


def test_the_module_is_exported_and_needs_a_gpu_to_compute():
    assert "regression" in wb.__all__ and wb.regression is regression
    for name in ("targets", "Accumulator", "BoxRegressor", "fit", "detect_and_refine"):
        assert hasattr(regression, name)
    if not __import__("torch").cuda.is_available():
        reg = regression.BoxRegressor((2, 2, 1), np.zeros((4, 4)), np.zeros(4))
        with pytest.raises(nat.NativeError):
            reg.predict(np.zeros((3, 2, 2, 1), np.float32))
        with pytest.raises(nat.NativeError):
            regression.Accumulator((2, 2, 1), np.uint8)
    reg = regression.BoxRegressor((2, 2, 1), np.zeros((4, 4)), np.zeros(4))
    with pytest.raises(ValueError):
        reg.predict(np.zeros((3, 2, 3, 1), np.float32))
    with pytest.raises(NotImplementedError):
        reg.predict(np.zeros((3, 2, 2, 1), np.float64))
    M = wb.Model((8, 8, 4), wb.default_channel_opts)
    with pytest.raises(ValueError):
        regression.detect_and_refine(np.zeros((64, 64), np.uint8), M, reg)                       # window shapes differ
    reg8 = regression.BoxRegressor((8, 8, 4), np.zeros((256, 4)), np.zeros(4), dtype=np.uint8)
    with pytest.raises(ValueError):
        regression.detect_and_refine(np.zeros((64, 64), np.uint8), M, reg8)                      # channel dtypes differ
    with pytest.raises(TypeError):
        regression.detect_and_refine(np.zeros((64, 64), np.uint8), M, None)


def test_regress_kernels_use_no_scratch_memory_and_exports_are_declared():
    nat.load()
    sizes = _kernel_scratch_sizes(open(nat.LIB_PATH, "rb").read())
    mine = {k: v for k, v in sizes.items() if any(name in k for name in KERNELS)}
    assert len(mine) == 7, sorted(mine)                        # gram_partial, predict and apply for two dtypes, one reduce
    assert set(mine.values()) == {0}, mine
    for name in EXPORTS:
        assert name in nat.SYMBOLS
    assert nat.WB_ABI_VERSION == 8 and nat.WB_GRAM_CHUNK == 256 and nat.WB_GRAM_MAX_P == 2048
    header = open(__import__("os").path.join(__import__("os").path.dirname(nat.__file__), "..", "include", "waldboost_hip.h")).read()
    assert "#define WB_GRAM_CHUNK 256" in header and "#define WB_ABI_VERSION 8" in header


def test_regress_entry_points_reject_bad_arguments_without_a_gpu():
    lib = nat.load()
    n = C.c_size_t()
    assert lib.wb_gram_scratch_bytes(513, 123, C.byref(n)) == 0 and n.value >= 3 * 128 * 128 * 8 // 2
    one = n.value
    assert lib.wb_gram_scratch_bytes(256, 123, C.byref(n)) == 0 and 3 * n.value == one           # per chunk of 256 rows
    assert lib.wb_gram_scratch_bytes(0, 123, C.byref(n)) == 0 and n.value == 0
    assert lib.wb_gram_scratch_bytes(10, 123, None) == nat.WB_ERR_INVALID
    assert lib.wb_gram_scratch_bytes(-1, 123, C.byref(n)) == nat.WB_ERR_INVALID
    assert lib.wb_gram_scratch_bytes(10, 0, C.byref(n)) == nat.WB_ERR_INVALID
    assert lib.wb_gram_scratch_bytes(10, 2043, C.byref(n)) == 0                                  # P = 2048
    assert lib.wb_gram_scratch_bytes(10, 2044, C.byref(n)) == nat.WB_ERR_UNSUPPORTED
    fake, odd = C.c_void_p(4096), C.c_void_p(4097)            # (never dereferenced: refused before any HIP call)
    gram = lambda X=fake, dt=nat.WB_DTYPE_U8, T=fake, N=10, D=11, S=fake, scr=fake, nb=1 << 30: lib.wb_gram_launch(None, X, dt, T, N, D, S, scr, nb)
    assert gram(N=0, X=None, T=None, S=None, scr=None, nb=0) == 0                                # nothing to do: no launch
    for kw in (dict(X=None), dict(T=None), dict(S=None), dict(scr=None), dict(T=odd), dict(S=odd), dict(scr=odd),
               dict(X=odd, dt=nat.WB_DTYPE_F32), dict(N=-1), dict(D=0), dict(nb=0), dict(nb=64 * 64 * 8 - 1)):
        assert gram(**kw) == nat.WB_ERR_INVALID, kw
    assert b"scratch" in lib.wb_last_error()
    assert gram(D=2044) == nat.WB_ERR_UNSUPPORTED and gram(dt=nat.WB_DTYPE_F64) == nat.WB_ERR_UNSUPPORTED
    pred = lambda X=fake, dt=nat.WB_DTYPE_U8, n=5, shape=(8, 8, 4), Wb=fake, out=fake: lib.wb_regress_predict_launch(None, X, dt, n, *shape, Wb, out)
    assert pred(n=0, X=None, Wb=None, out=None) == 0
    for kw in (dict(X=None), dict(Wb=None), dict(out=None), dict(Wb=odd), dict(out=odd), dict(X=odd, dt=nat.WB_DTYPE_F32), dict(n=-1),
               dict(shape=(0, 8, 4)), dict(shape=(8, 8, 0))):
        assert pred(**kw) == nat.WB_ERR_INVALID, kw
    assert pred(dt=nat.WB_DTYPE_RANK8) == nat.WB_ERR_UNSUPPORTED and pred(n=(1 << 26) + 1) == nat.WB_ERR_UNSUPPORTED

    def apply(buf=fake, dt=nat.WB_DTYPE_U8, stride=1000, levels=fake, L=3, det=fake, n=5, Wb=fake, inv=fake, inv64=fake, pred=None, boxes=fake, err=fake):
        return lib.wb_regress_apply_launch(None, buf, dt, stride, 2, levels, L, 4, det, n, 8, 8, Wb, inv, inv64, pred, boxes, err)
    for kw in (dict(buf=None), dict(levels=None), dict(det=None), dict(Wb=None), dict(inv=None), dict(inv64=None), dict(boxes=None),
               dict(err=None), dict(det=C.c_void_p(4104)), dict(inv64=odd), dict(pred=odd), dict(Wb=odd), dict(stride=-1), dict(n=-1), dict(L=0),
               dict(err=odd)):
        assert apply(**kw) == nat.WB_ERR_INVALID, kw
    assert apply(dt=nat.WB_DTYPE_F64) == nat.WB_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------ the end-to-end statement, on the CPU
SHAPE = (8, 8, 4)


@functools.lru_cache(None)
def _sets(flavour):
    opts = dict(shrink=2, n_per_oct=8, smooth=1, channels=orc.grad_hist if flavour == "float" else orc.grad_hist_4_u1)
    pyramid_of = lambda image: list(orc.channel_pyramid(image, opts))
    return (rr.image_set(rr.planted_images(range(6)), pyramid_of, SHAPE), rr.image_set(rr.planted_images(range(6, 12)), pyramid_of, SHAPE))


def test_the_planted_images_are_the_training_images_of_the_mining_tests():
    import test_gpu_mine
    for mine, theirs in zip(rr.planted_images(range(6)), test_gpu_mine._training_images()):
        assert np.array_equal(mine["image"], theirs["image"]) and np.array_equal(mine["gt"], theirs["groundtruth_boxes"].get())


@pytest.mark.parametrize("flavour", ["float", "fpga"])
def test_end_to_end_statement_improves_held_out_boxes(flavour):
    """Empty model, window (8, 8, 4), min_iou 0.5, uncapped: 1313 training windows; on the held-out images (seeds 6 .. 11) the
    refined boxes are better on average and for more than half of the windows."""
    train, held = _sets(flavour)
    assert train["X"].shape == (1313, 256)
    W, b, rss, tss = rr.solve(rr.gram(train["X"], train["T"]), 1e-2)
    assert (rss <= tss).all()
    raw_t, ref_t = rr.refined_iou(train, W, b)
    raw, ref = rr.refined_iou(held, W, b)
    print(f"{flavour}: training {raw_t.mean():.3f} -> {ref_t.mean():.3f}; held-out ({raw.size} windows) {raw.mean():.3f} -> {ref.mean():.3f}, "
          f"{(ref > raw).mean():.1%} improved")
    assert ref.mean() > raw.mean() and (ref > raw).mean() > 0.5
