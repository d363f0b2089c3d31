"""Designed inputs for the box-regression kernels (csrc/wb_regress.hip), with answers that exact arithmetic proves, and
NumPy emulations of the kernels' structure that can be told to make one mistake -- so that a test can show that the
designs would catch it (tests/test_regress_designs_host.py) before the kernels are held to them on the GPU
(tests/test_gpu_regress_designs.py).

Gram designs.  X is random uint8 with column 0 all 255 and T small integers, so A = [X | 1 | T] is an integer matrix,
A^T A is exact in int64 and in float64 (every partial sum is below 2^53), and 255^2 * 513 > 2^24 is odd: an fp32
accumulator cannot hold it (one that runs over all rows of a tile: inside one chunk of 256 rows 255^2 * 256 < 2^24 still
fits, and there it is the float case and its bound that tell).  X is asymmetric in the sense that matters: no two columns
agree, so an entry that lands at the transposed place, in the wrong row of a tile or in no place at all is a wrong number.
"""
from fractions import Fraction

import numpy as np

CHUNK = 256                                                  # WB_GRAM_CHUNK
GRAM_N = (1, 3, 4, 5, 255, 256, 257, 513)                    # the MFMA's k-group of 4 and the chunk edge
GRAM_D = (1, 11, 12, 59, 60, 123)                            # P = 6, 16, 17, 64, 65, 128: the 16- and 64-column tile edges
GRAM_FAULTS = ("f32_cd_map", "swapped_write_back", "missing_mirror", "dropped_tail_chunk", "dropped_k_remainder", "fp32_accumulator")
WINDOW_SHAPES = ((2, 2, 1), (5, 7, 3), (8, 8, 4), (12, 12, 4), (32, 32, 1))
PREDICT_N = (1, 63, 64, 65)
PREDICT_FAULTS = ("crc_feature_order", "missing_intercept")


# ------------------------------------------------------------------------------------------------ Gram
def gram_case(N, D, seed=0):
    """(X uint8 (N, D), T float64 (N, 4) of small integers, exact int64 A^T A)."""
    rng = np.random.default_rng([seed, N, D])
    X = rng.integers(0, 256, (N, D), dtype=np.uint8)
    X[:, 0] = 255
    T = rng.integers(-9, 10, (N, 4)).astype(np.float64)
    A = integer_design(X, T)
    return X, T, A.T @ A


def integer_design(X, T):
    X = np.asarray(X)
    return np.concatenate([X.astype(np.int64), np.ones((X.shape[0], 1), np.int64), np.asarray(T).astype(np.int64)], axis=1)


def emulate_gram(A, fault=None, S0=None):
    """S0 + A^T A the way the kernels compute it -- 16 x 16 tiles ti <= tj, chunks of 256 rows, k-groups of 4 rows, the f64
    MFMA's register map on write-back, the mirror -- on an integer A in int64 (exact).  fault: one of GRAM_FAULTS."""
    assert fault is None or fault in GRAM_FAULTS
    A = np.asarray(A, np.int64)
    N, P = A.shape
    S = np.zeros((P, P), np.int64) if S0 is None else np.array(S0, np.int64)
    nt = -(-P // 16)
    Ap = np.zeros((-(-N // CHUNK) * CHUNK, nt * 16), np.int64)
    Ap[:N, :P] = A
    chunks = Ap.shape[0] // CHUNK
    if fault == "dropped_tail_chunk":
        chunks = N // CHUNK
    lanes, regs = np.meshgrid(np.arange(64), np.arange(4), indexing="ij")
    true_row, col = (lanes >> 4) + 4 * regs, lanes & 15                       # the f64 instruction's C/D map
    dest_row = 4 * (lanes >> 4) + regs if fault == "f32_cd_map" else true_row  # where the kernel believes the value belongs
    for ti in range(nt):
        for tj in range(ti, nt):
            total = np.zeros((16, 16), np.float32 if fault == "fp32_accumulator" else np.int64)
            for c in range(chunks):
                rows = Ap[c * CHUNK:(c + 1) * CHUNK]
                if fault == "dropped_k_remainder":
                    real = min(max(N - c * CHUNK, 0), CHUNK)
                    rows = rows[:real // 4 * 4]
                acc = np.zeros((16, 16), np.float32 if fault == "fp32_accumulator" else np.int64)
                for k0 in range(0, rows.shape[0], 4):
                    step = rows[k0:k0 + 4, ti * 16:ti * 16 + 16].T @ rows[k0:k0 + 4, tj * 16:tj * 16 + 16]
                    acc = acc + step.astype(acc.dtype)
                acc = np.asarray(acc).astype(np.int64)
                tile = np.zeros((16, 16), np.int64)
                tile[dest_row, col] = acc[true_row, col]
                total = total + (tile.T if fault == "swapped_write_back" else tile).astype(total.dtype)
            total = total.astype(np.int64)
            for i in range(16):
                for j in range(16):
                    gi, gj = ti * 16 + i, tj * 16 + j
                    if gi > gj or gj >= P:
                        continue
                    S[gi, gj] += total[i, j]
                    if gi != gj and fault != "missing_mirror":
                        S[gj, gi] = S[gi, gj]
    return S


def float_gram_case(N=261, D=16, seed=3):
    """(X float32 (N, D) non-integers, T float64 (N, 4), exact A^T A as Fractions (P, P) object array, |A|^T |A| float64)."""
    rng = np.random.default_rng(seed)
    X = (rng.normal(0, 40, (N, D)) + rng.integers(-3, 4, (N, D)) / 7.0).astype(np.float32)
    T = rng.normal(0, 3, (N, 4))
    A = np.concatenate([X.astype(np.float64), np.ones((N, 1)), T], axis=1)
    F = np.array([[Fraction(float(v)) for v in row] for row in A], dtype=object)
    exact = F.T.dot(F)
    return X, T, exact, np.abs(A).T @ np.abs(A)


def gram_bound(N, absgram):
    """Any-order summation of N products, one rounding per product and per add: (N + 8) * 2^-52 * (|A|^T |A|) covers
    ((1 + u)^(N + 1) - 1) with u = 2^-53 twice over."""
    return (N + 8) * 2.0 ** -52 * absgram


def within(got, exact, bound):
    """Every |got - exact| <= bound, judged in exact rational arithmetic."""
    got, bound = np.asarray(got, np.float64), np.asarray(bound, np.float64)
    return all(abs(Fraction(float(got[i, j])) - exact[i, j]) <= Fraction(float(bound[i, j]))
               for i in range(got.shape[0]) for j in range(got.shape[1]))


# ------------------------------------------------------------------------------------------------ predict
def window_case(shape, n, dtype, seed=0):
    """n crops (n, m, nn, C) of `dtype`: small integers (exact in every order) for uint8, non-integers for float32."""
    rng = np.random.default_rng([seed, n, *shape])
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
    return rng.normal(0, 30, (n,) + tuple(shape)).astype(np.float32)


def one_hot_weights(shape, seed=0):
    """(W, b): coordinate k reads ONE feature, another for every k and none of them symmetric under a swap of row and
    column -- so pred[k] = x[feature k] + b[k] exactly, and it pins the feature order j = (r * nn + c) * C + ch."""
    m, nn, C = shape
    D = m * nn * C
    rng = np.random.default_rng([seed, D])
    W = np.zeros((D, 4))
    picks = []
    for k in range(4):
        r, c, ch = (k + 1) % m, (2 * k + m) % nn, k % C
        if m * nn > 1 and r == c:
            c = (c + 1) % nn
        picks.append((r, c, ch))
        W[(r * nn + c) * C + ch, k] = 1.0
    b = rng.integers(-5, 6, 4).astype(np.float64)
    return W, b, picks


def integer_weights(shape, seed=0):
    """Small integer W and b: with uint8 x every product and partial sum is an integer below 2^53, so every summation order
    gives the one exact answer."""
    D = int(np.prod(shape))
    rng = np.random.default_rng([seed, D, 1])
    return rng.integers(-8, 9, (D, 4)).astype(np.float64), rng.integers(-100, 101, 4).astype(np.float64)


def random_weights(shape, seed=0):
    D = int(np.prod(shape))
    rng = np.random.default_rng([seed, D, 2])
    return rng.normal(0, 1, (D, 4)) / np.sqrt(D), rng.normal(0, 2, 4)


def exact_predict(X, W, b):
    """pred for integer-valued inputs in Python integers: (n, 4) float64, exact."""
    Xi = np.asarray(X).reshape(np.asarray(X).shape[0], -1).astype(np.int64)
    return (Xi @ np.asarray(W).astype(np.int64) + np.asarray(b).astype(np.int64)).astype(np.float64)


def emulate_predict(X, W, b, fault=None):
    """The kernel's predict on crops X (n, m, nn, C) through tests/regress_reference.predict, with one mistake."""
    import regress_reference as rr
    assert fault is None or fault in PREDICT_FAULTS
    X = np.asarray(X)
    if fault == "crc_feature_order":
        X = X.transpose(0, 2, 1, 3)                           # the window walked (c, r, ch)
    return rr.predict(rr.features(X), W, np.zeros(4) if fault == "missing_intercept" else b)


# ------------------------------------------------------------------------------------------------ refine
def refine_case():
    """(boxes float32 (n, 4), pred float64 (n, 4), scales): scales whose 1 / scale is NOT a float32, and offsets large enough
    that float32(1 / scale) in place of the float64 reciprocal (a relative 3e-8, half a float32 ulp) moves many of the refined
    boxes to a neighbouring float32."""
    scales = [0.5 * 2 ** (-k / 8) for k in range(1, 8)]
    rng = np.random.default_rng(5)
    level = np.arange(64) % len(scales)
    rc = rng.integers(0, 40, (64, 2))
    inv32 = np.array([np.float32(1.0 / s) for s in scales], np.float32)
    rect = np.stack([rc[:, 1], rc[:, 0], rc[:, 1] + 8, rc[:, 0] + 8], 1).astype(np.float32)
    boxes = (rect * inv32[level][:, None]).astype(np.float32)
    pred = rng.normal(0, 1, (64, 4)) * 1000.0 + 0.37
    return boxes, pred, np.array(scales), level


# ------------------------------------------------------------------------------------------------ pyramids for apply
def pyramid_case(shape, dtype, seed=0):
    """Two images, three levels, HWC, in one buffer per image as the engine lays them out: (buf (2, stride), levels -- a list
    of (chn_off, u, v) --, C).  The levels are a little larger than the window, of odd sizes, with a gap between them."""
    m, nn, C = shape
    rng = np.random.default_rng([seed, *shape, 7])
    dims = [(m + 5, nn + 9), (m + 2, nn + 3), (m + 1, nn + 1)]
    levels, at = [], 3 * C
    for u, v in dims:
        levels.append((at, u, v))
        at += u * v * C + 5 * C
    stride = at
    if np.dtype(dtype) == np.uint8:
        buf = rng.integers(0, 256, (2, stride), dtype=np.uint8)
    else:
        buf = rng.normal(0, 30, (2, stride)).astype(np.float32)
    return buf, levels, C


def pyramid_records(shape, levels, n, seed=0):
    """n records (image, level, r, c) inside their levels; the first ones sit at the last valid row and column of each."""
    m, nn, _ = shape
    rng = np.random.default_rng([seed, n, 11])
    recs = []
    for b in range(2):
        for l, (_, u, v) in enumerate(levels):
            recs.append((b, l, u - m, v - nn))
    while len(recs) < n:
        l = int(rng.integers(0, len(levels)))
        _, u, v = levels[l]
        recs.append((int(rng.integers(0, 2)), l, int(rng.integers(0, u - m + 1)), int(rng.integers(0, v - nn + 1))))
    return np.array(recs[:n], np.int64)


def crops_of(buf, levels, C, shape, recs):
    m, nn, _ = shape
    out = np.zeros((len(recs), m, nn, C), buf.dtype)
    for i, (b, l, r, c) in enumerate(recs):
        off, u, v = levels[l]
        out[i] = buf[b, off:off + u * v * C].reshape(u, v, C)[r:r + m, c:c + nn]
    return out
