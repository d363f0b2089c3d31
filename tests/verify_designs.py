"""Designed weights and crops for the verification CNN (csrc/wb_verify.hip), and one emulated wrong kernel per way a
rewrite could slip.

Every design holds small integers: the folded weights are integers (batch-normalisation scales are powers of two,
epsilon = 2^-10 with moving_variance = v - 2^-10, so v is what the square root sees), crops and scores too, and every
partial sum of every chain is an integer below 2^24 (`integer_forward` returns the bound: the sum of the magnitudes of a
chain's terms).  Such sums are exact in float32 in ANY order, so the expected output follows from int64 arithmetic alone
-- einsum, no chain -- and the kernels, the NumPy contract (verify_reference) and this expectation must agree to the bit.

The designs (`designs(shape)`, every one for any supported window shape):
  corners_edges   a single hot pixel in each corner, on each edge and in the middle; conv1 has nine distinct taps
  routes          one-hot channel routes with distinct gains in every layer: pins the input / output channel order
  pool_winners    the four candidates of a pool cell win in turn
  flat_pick       dense0 picks single flat indices (row, column, channel all different): pins the flatten
  batchnorm       scales 2, 4 and -2 (a negative gamma in block 2), non-zero mean and beta
  mixed           seeded sparse integers everywhere, negative biases: a negative pre-activation in front of every ReLU,
                  scores of both signs that are added last
An odd m or n (the pool's floor) comes with the shapes the tests choose.

The wrong kernels (`WRONG`), each composed of verify_reference's steps:
  convolution (flipped taps), swapped_ky_kx, chw_flatten, pool_ceil (the pooled map of ceil size, flattened, its first F
  entries), pool_before_bn (see below), bn_without_mean, dense_transposed, score_before_last (added to every hidden
  unit), pad_replicate.
"Pool before the second ReLU's bias" cannot show in exact arithmetic while the scale is positive: the maximum commutes
with adding a constant and with the ReLU.  It is emulated as what such a rewrite does to the folded form: the raw sums
of conv2 are pooled, then scaled and shifted -- which differs as soon as a scale is negative (the batchnorm design)."""
import numpy as np

import verify_reference as ref

EPS = 2.0 ** -10
HIDDEN = 128
CONV_OUT = (8, 8, 16, 16)


def conv_in(C):
    return (C, 8, 8, 16)


def _bn_identity(cout):
    """gamma, beta, mean, variance of a batch normalisation that folds to scale 1, shift 0."""
    return [np.ones(cout, "f"), np.zeros(cout, "f"), np.zeros(cout, "f"), np.full(cout, 1.0 - EPS, "f")]


def _base(shape, rng):
    """Pass-through convolutions (centre tap, channel i -> i), seeded small-integer dense layers."""
    m, n, C = shape
    arrays = []
    for cin, cout in zip(conv_in(C), CONV_OUT):
        W = np.zeros((3, 3, cin, cout), "f")
        for i in range(min(cin, cout)):
            W[1, 1, i, i] = 1
        arrays += [W, np.zeros(cout, "f")] + _bn_identity(cout)
    F = (m // 2) * (n // 2) * 16
    d0 = (rng.integers(0, 4, (F, HIDDEN)) * (rng.random((F, HIDDEN)) < min(0.25, 16.0 / F))).astype("f")
    arrays += [d0, rng.integers(-3, 2, HIDDEN).astype("f"), rng.integers(-2, 4, (HIDDEN, 1)).astype("f"), np.array([5], "f")]
    return arrays


def _design(name, shape, arrays, X, scores):
    return dict(name=name, shape=tuple(shape), arrays=arrays, epsilon=EPS, X=np.ascontiguousarray(X),
                scores=np.asarray(scores, "f"))


def designs(shape, seed=0):
    m, n, C = shape
    m2, n2 = m // 2, n // 2
    rng = np.random.default_rng([seed, m, n, C])
    out = []

    # a single hot pixel in each corner, on each edge, in the middle
    a = _base(shape, rng)
    a[0] = np.zeros((3, 3, C, 8), "f")
    for o in range(8):
        a[0][:, :, (o * 5) % C, o] = (np.arange(9).reshape(3, 3) * (o + 1)) % 11 + 1        # nine distinct taps at o = 0
    spots = [(0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1), (0, n // 2), (m - 1, n // 2), (m // 2, 0), (m // 2, n - 1),
             (m // 2, n // 2)]
    X = np.zeros((len(spots), m, n, C), "f")
    for k, (r, c) in enumerate(spots):
        X[k, r, c, :] = 1 + np.arange(C) % 3
    out.append(_design("corners_edges", shape, a, X, np.zeros(len(spots))))

    # one-hot routes with distinct gains in every layer
    a = _base(shape, rng)
    for k, (cin, cout) in enumerate(zip(conv_in(C), CONV_OUT)):
        W = np.zeros((3, 3, cin, cout), "f")
        for i in range(cin):
            W[1, 1, i, (3 * i + k + 1) % cout] = 1 + (i + k) % 3
        a[6 * k] = W
    out.append(_design("routes", shape, a, rng.integers(0, 3, (4, m, n, C)).astype("f"), [1, -1, 0, 7]))

    # the four candidates of a pool cell win in turn
    a = _base(shape, rng)
    X = np.zeros((4, m, n, C), "f")
    for k in range(4):
        X[k, (k >> 1)::2, (k & 1)::2, :] = 2
        X[k, :, :, 0] += 1
    out.append(_design("pool_winners", shape, a, X, np.zeros(4)))

    # dense0 picks single flat indices
    a = _base(shape, rng)
    a[18] = np.zeros((3, 3, 16, 16), "f")
    a[18][1, 1, np.arange(16), np.arange(16)] = 1
    a[12] = np.zeros((3, 3, 8, 16), "f")
    a[12][1, 1, np.arange(8), np.arange(8)] = 1
    a[12][1, 1, np.arange(8), np.arange(8) + 8] = 2
    d0 = np.zeros(((m2 * n2) * 16, HIDDEN), "f")
    picks = [(m2 - 1, 0, 0), (0, n2 - 1, 8), (m2 // 2, n2 // 3, min(C, 8) + 7)]       # (channels that carry data)
    d1 = np.zeros((HIDDEN, 1), "f")
    for j, (r, c, ch) in enumerate(picks):
        d0[(r * n2 + c) * 16 + ch, 7 * j + 2] = 1
        d1[7 * j + 2] = 64 ** j
    a[24], a[25], a[26], a[27] = d0, np.zeros(HIDDEN, "f"), d1, np.zeros(1, "f")
    out.append(_design("flat_pick", shape, a, rng.integers(0, 8, (3, m, n, C)).astype("f"), np.zeros(3)))

    # batch normalisation: power-of-two scales, a negative one in block 2, non-zero mean and beta
    a = _base(shape, rng)
    for k, (scale, cout) in enumerate(zip((2.0, -2.0, 4.0, 2.0), CONV_OUT)):
        cin = conv_in(C)[k]
        W = (rng.integers(-1, 2, (3, 3, cin, cout)) * (rng.random((3, 3, cin, cout)) < 2.0 / (9 * cin) + 0.02)).astype("f")
        W[1, 1, np.arange(min(cin, cout)), np.arange(min(cin, cout))] = 1 if k != 1 else -1
        a[6 * k] = W
        a[6 * k + 1] = rng.integers(-2, 3, cout).astype("f")                      # bias
        a[6 * k + 2] = np.full(cout, scale / 4.0 if k % 2 else scale, "f")        # gamma
        a[6 * k + 3] = rng.integers(-2, 3, cout).astype("f")                      # beta
        a[6 * k + 4] = rng.integers(1, 4, cout).astype("f") * (-1 if k == 1 else 1)   # moving_mean
        a[6 * k + 5] = np.full(cout, (1.0 / 16.0 if k % 2 else 1.0) - EPS, "f")   # sqrt(variance + eps) = 1/4 or 1
    out.append(_design("batchnorm", shape, a, rng.integers(0, 3, (5, m, n, C)).astype("f"), [0, 1, -2, 3, 100]))

    # seeded sparse integers everywhere, negative biases, scores of both signs
    a = _base(shape, rng)
    for k, (cin, cout) in enumerate(zip(conv_in(C), CONV_OUT)):
        W = (rng.integers(-1, 2, (3, 3, cin, cout)) * (rng.random((3, 3, cin, cout)) < 3.0 / (9 * cin))).astype("f")
        W[1, 1, np.arange(min(cin, cout)), np.arange(min(cin, cout))] = 1
        a[6 * k] = W
        a[6 * k + 1] = rng.integers(-2, 1, cout).astype("f")
    out.append(_design("mixed", shape, a, rng.integers(0, 4, (6, m, n, C)).astype(np.uint8), [0, 1, -1, 1000, -1000, 3]))
    return out


def integer_forward(layers, X, scores):
    """The network on integers, without chains: (expected float32 (N,), the largest sum of magnitudes of any chain, the
    smallest pre-activation in front of each of the five ReLUs)."""
    def ints(v):
        v = np.asarray(v, np.float64)
        assert np.array_equal(v, np.rint(v)), "a design's folded weights and crops are integers"
        return v.astype(np.int64)

    def conv(x, W, b):
        N, H, Wd, _ = x.shape
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
        win = np.stack([xp[:, ky:ky + H, kx:kx + Wd, :] for ky in range(3) for kx in range(3)], axis=3)   # N H W 9 cin
        return np.einsum("nhwti,tio->nhwo", win, W.reshape(9, W.shape[2], W.shape[3])) + b

    a, bound, lows = ints(X), 0, []
    for k in range(4):
        W, b = ints(layers[k][0]), ints(layers[k][1])
        pre = conv(a, W, b)
        bound = max(bound, int(conv(np.abs(a), np.abs(W), np.abs(b)).max()))
        lows.append(int(pre.min()))
        a = np.maximum(pre, 0)
        if k == 1:
            N, H, Wd, C = a.shape
            a = a[:, :H // 2 * 2, :Wd // 2 * 2].reshape(N, H // 2, 2, Wd // 2, 2, C).max(axis=(2, 4))
    f = a.reshape(a.shape[0], -1)
    d0, c0, d1, c1 = (ints(v) for v in layers[4:])
    pre = f @ d0 + c0
    bound = max(bound, int((np.abs(f) @ np.abs(d0) + np.abs(c0)).max()))
    lows.append(int(pre.min()))
    h = np.maximum(pre, 0)
    y = h @ d1 + c1
    bound = max(bound, int((np.abs(h) @ np.abs(d1) + np.abs(c1)).max()))
    total = y + ints(scores).reshape(-1)
    bound = max(bound, int((np.abs(y) + np.abs(ints(scores).reshape(-1))).max()))
    return total.astype(np.float32), bound, lows


def expected(design):
    return integer_forward(ref.fold(design["arrays"], design["epsilon"]), design["X"], design["scores"])


# --------------------------------------------------------------------------------------- emulated wrong kernels
def _run(layers, X, scores, conv=ref.conv3x3, pool=ref.pool2x2, flatten=lambda a: a.reshape(a.shape[0], -1), dense0=None,
         score_first=False):
    (w1, b1), (w2, b2), (w3, b3), (w4, b4), d0, c0, d1, c1 = layers
    a = np.asarray(X).astype(np.float32)
    a = ref.relu(conv(a, w1, b1))
    a = pool(ref.relu(conv(a, w2, b2)))
    a = ref.relu(conv(a, w3, b3))
    a = ref.relu(conv(a, w4, b4))
    f = flatten(a)[:, :d0.shape[0]]
    h = ref.relu(ref.dense(f, d0 if dense0 is None else dense0, c0))
    s = np.asarray(scores, np.float32).reshape(-1)
    if score_first:
        return ref.dense((h + s[:, None]).astype(np.float32), d1.reshape(-1, 1), c1)[:, 0]
    return (ref.dense(h, d1.reshape(-1, 1), c1)[:, 0] + s).astype(np.float32)


def _pool_ceil(a):
    N, H, Wd, C = a.shape
    return ref.pool2x2(np.pad(a, ((0, 0), (0, H % 2), (0, Wd % 2), (0, 0))))


def _pool_before_bn(d):
    """conv2's raw sums (unfolded kernel, no bias) pooled, then scaled and shifted, then the ReLU."""
    layers = ref.fold(d["arrays"], d["epsilon"])
    W, b, gamma, beta, mean, var = (np.asarray(v, np.float64) for v in d["arrays"][6:12])
    s = gamma / np.sqrt(var + d["epsilon"])
    a = ref.relu(ref.conv3x3(np.asarray(d["X"]).astype(np.float32), *layers[0]))
    raw = ref.pool2x2(ref.conv3x3(a, W.astype(np.float32), np.zeros(8, "f")))
    a = ref.relu((raw.astype(np.float64) * s + ((b - mean) * s + beta)).astype(np.float32))
    a = ref.relu(ref.conv3x3(a, *layers[2]))
    a = ref.relu(ref.conv3x3(a, *layers[3]))
    h = ref.relu(ref.dense(a.reshape(a.shape[0], -1), layers[4], layers[5]))
    return (ref.dense(h, layers[6].reshape(-1, 1), layers[7])[:, 0] + d["scores"]).astype(np.float32)


def _without_mean(d):
    arrays = list(d["arrays"])
    for k in range(4):
        arrays[6 * k + 4] = np.zeros_like(arrays[6 * k + 4])
    return _run(ref.fold(arrays, d["epsilon"]), d["X"], d["scores"])


def _layers(d):
    return ref.fold(d["arrays"], d["epsilon"])


def _with_kernels(d, change):
    layers = _layers(d)
    return _run([(change(W), b) for W, b in layers[:4]] + layers[4:], d["X"], d["scores"])


WRONG = {
    "convolution": lambda d: _with_kernels(d, lambda W: W[::-1, ::-1]),
    "swapped_ky_kx": lambda d: _with_kernels(d, lambda W: W.transpose(1, 0, 2, 3)),
    "chw_flatten": lambda d: _run(_layers(d), d["X"], d["scores"], flatten=lambda a: a.transpose(0, 3, 1, 2).reshape(a.shape[0], -1)),
    "pool_ceil": lambda d: _run(_layers(d), d["X"], d["scores"], pool=_pool_ceil),
    "pool_before_bn": _pool_before_bn,
    "bn_without_mean": _without_mean,
    "dense_transposed": lambda d: _run(_layers(d), d["X"], d["scores"],
                                       dense0=_layers(d)[4].reshape(HIDDEN, -1).T.copy()),
    "score_before_last": lambda d: _run(_layers(d), d["X"], d["scores"], score_first=True),
    "pad_replicate": lambda d: _run(_layers(d), d["X"], d["scores"],
                                    conv=lambda x, W, b: ref.conv3x3(x, W, b, pad_mode="edge")),
}
