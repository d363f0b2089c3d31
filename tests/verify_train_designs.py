"""Designed inputs shared by the host and the GPU tests of the verifier's training: the planted two-class pool of the
end-to-end case, and that case run through the NumPy statement with the batches verification.train draws; the comparison
rule of the GPU tests (unit_of, held, compared_mask) and the inputs of their cases, so that the host tests can show from
the statement alone that a case meets the rule's conditions and that its design can tell a wrong kernel from a right one:
long batches, one live window at the edges of the kernels' partitions, pool ties that reach the weight gradients, and a
step away from the default constants."""
import functools

import numpy as np

import verify_train_reference as tr
from waldboost_amd import verification as ver

PLANTED_SHAPE = (8, 8, 2)
PLANTED_SEED = 7
PLANTED_LR = 1e-3
PLANTED_BATCH = 16


def random_arrays(shape, seed):
    """model_cnn's arrays with non-trivial biases, gamma and beta (moving statistics play no part in a training step)."""
    rng = np.random.default_rng(seed)
    arrays = ver.model_cnn(shape, seed=seed).get_weights()
    for k in range(4):
        cout = arrays[6 * k + 1].size
        arrays[6 * k + 1] = (rng.standard_normal(cout) * 0.1).astype("f")
        arrays[6 * k + 2] = rng.uniform(0.5, 1.5, cout).astype("f") * rng.choice([-1, 1], cout).astype("f")
        arrays[6 * k + 3] = (rng.standard_normal(cout) * 0.2).astype("f")
    arrays[25] = (rng.standard_normal(128) * 0.1).astype("f")
    arrays[27] = np.array([0.25], "f")
    return arrays


def random_batch(shape, B, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B,) + shape).astype("f")
    H = (rng.standard_normal(B) * 0.5).astype("f")
    Y = np.array([-1] * (B // 2) + [1] * (B // 2), "f")
    return X, H, Y


def planted_pool(n_each=96, seed=PLANTED_SEED):
    """(X0, H0, X1, H1): uint8 noise crops; the positives carry a brighter centre block.  The detector scores say nothing."""
    rng = np.random.default_rng(seed)
    X0 = rng.integers(0, 128, (n_each,) + PLANTED_SHAPE).astype(np.uint8)
    X1 = rng.integers(0, 128, (n_each,) + PLANTED_SHAPE).astype(np.uint8)
    X1[:, 2:6, 2:6, :] += 100
    H0 = (rng.standard_normal(n_each) * 0.1).astype(np.float32)
    H1 = (rng.standard_normal(n_each) * 0.1).astype(np.float32)
    return X0, H0, X1, H1


def planted_model():
    return ver.model_cnn(PLANTED_SHAPE, seed=PLANTED_SEED)


def planted_statement_run(epochs, steps, dtype=np.float64, max_steps=None):
    """train(planted_model(), *planted_pool(), epochs, 16, steps, lr=1e-3, seed=7) in the statement: (the epochs' mean
    losses, every step's loss); at most `max_steps` steps are run (the batches are the full run's)."""
    X0, H0, X1, H1 = planted_pool()
    X = np.concatenate([X0, X1]).astype(np.float32)
    H = np.concatenate([H0, H1])
    Y = np.concatenate([-np.ones(len(X0), "f"), np.ones(len(X1), "f")])
    state = tr.new_state(planted_model().get_weights(), dtype)
    rng = np.random.default_rng(PLANTED_SEED)
    means, every = [], []
    for _ in range(epochs):
        idx = ver._draw_epoch(rng, len(X0), len(X1), steps, PLANTED_BATCH // 2)
        losses = []
        for row in idx:
            out = tr.train_step(state, X[row], H[row], Y[row], dtype, seed=PLANTED_SEED, dropout=0.2, lr=PLANTED_LR)
            losses.append(float(out["loss"]))
            every.append(float(out["loss"]))
            if max_steps is not None and len(every) >= max_steps:
                return means, every
        means.append(float(np.mean(losses)))
    return means, every


# ---- the comparison rule of the GPU tests: per array, max|gpu - s64| <= FACTOR * max(err32, FLOOR * max|s64|)
FACTOR = 8.0
FLOOR = 2.0 ** -20
LEFT_OUT_CAP = 0.05                     # of the parameters, in a GPU test
LEFT_OUT_HOST = 0.025                   # in the host twin: half, because the GPU's unit equals the statement's
DEFAULTS = dict(lr=1e-4, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99, bn_epsilon=1e-3, dropout=0.2, seed=3)


def pool_for(shape, n_pool, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        X = rng.integers(0, 256, (n_pool,) + shape).astype(np.uint8)
    else:
        X = rng.standard_normal((n_pool,) + shape).astype(np.float32)
    H = (rng.standard_normal(n_pool) * 0.5).astype(np.float32)
    Y = rng.choice([-1.0, 1.0], n_pool).astype(np.float32)
    return X, H, Y


def statement(arrays, X, H, Y, idx, dtype, dropout=0.2, seed=3, lr=1e-4, steps_before=0, m=None, v=None, bn_epsilon=1e-3,
              **adam):
    """One step of the statement on the windows idx, from the parameters `arrays`, Adam's state m and v (zero if None) and
    `steps_before` steps done: (the forward_backward dict, the state after the step)."""
    dt = np.dtype(dtype).type
    state = tr.new_state(arrays, dtype)
    state["t"] = steps_before
    if m is not None:
        state["m"] = [np.asarray(a).astype(dt) for a in m]
    if v is not None:
        state["v"] = [np.asarray(a).astype(dt) for a in v]
    out = tr.train_step(state, X[idx].astype(np.float32), H[idx], Y[idx], dtype, seed=seed, dropout=dropout, epsilon=bn_epsilon,
                        lr=lr, **adam)
    return out, state


def unit_of(s64, s32):
    """The rule's unit of one array.  An array that is zero in both statements has the smallest positive unit: the GPU's
    must be zero too."""
    s64 = np.asarray(s64, np.float64)
    return max(np.abs(np.asarray(s32, np.float64).reshape(s64.shape) - s64).max(), FLOOR * np.abs(s64).max(),
               np.finfo(np.float64).tiny)


def held(got, s64, s32):
    """(largest difference, the rule's unit) of one array."""
    s64 = np.asarray(s64, np.float64)
    return np.abs(np.asarray(got, np.float64).reshape(s64.shape) - s64).max(), unit_of(s64, s32)


def compared_mask(k, arrays, o64, o32):
    """Where the parameters of array k are compared after the update: everywhere for the moving statistics, elsewhere where
    |g64| exceeds the gradient's bound or g64 is exactly zero."""
    if tr.is_moving(k):
        return np.ones(arrays[k].shape, bool)
    g64 = np.asarray(o64["grads"][k], np.float64).reshape(arrays[k].shape)
    return (np.abs(g64) > FACTOR * unit_of(g64, o32["grads"][k])) | (g64 == 0)


def left_out_share(arrays, o64, o32):
    """The share of the parameters that the rule leaves out, from the two statements alone."""
    out = total = 0
    for k in range(28):
        if not tr.is_conv_bias(k):
            mask = compared_mask(k, arrays, o64, o32)
            out, total = out + mask.size - int(mask.sum()), total + mask.size
    return out / total


def both_statements(case):
    """((o64, st64), (o32, st32)) of a case dict: arrays, X, H, Y, idx and, optionally, m, v, steps_before and hyper."""
    kw = dict(case.get("hyper", {}), m=case.get("m"), v=case.get("v"), steps_before=case.get("steps_before", 0))
    return tuple(statement(case["arrays"], case["X"], case["H"], case["Y"], case["idx"], dt, **kw) for dt in (np.float64, np.float32))


# ---- A. one random step, long batches among them
SHORT_CASES = [((2, 2, 1), 2), ((3, 5, 2), 4), ((5, 6, 3), 6), ((14, 14, 4), 64), ((13, 32, 9), 8), ((32, 32, 16), 4)]
# (2,3,1) B=130: wgrad ranges of 1 and 2 windows, an odd pixel count.  (4,4,2) B=1022: ranges of 7 and 8, the head's last
# tree slots are padding.  (6,6,1) B=1024: rows = 36864, G1 capped at 128 with 288 rows each, G2 = 36, the full head tree.
# (10,14,1) B=1024: B * P2 = 35840, G2 capped as well, G1 takes 1120 rows each.
LONG_CASES = [((2, 3, 1), 130), ((4, 4, 2), 1022), ((6, 6, 1), 1024), ((10, 14, 1), 1024)]
# (arrays, pool) seeds: 20 + m and 30 + n unless listed here.  The share that the rule leaves out swings with the seed
# (0.6 % to 30 % over five seeds at (10,14,1) B=1024), so the host twin asserts LEFT_OUT_HOST for every long case; (6,6,1)
# with uint8 crops leaves out 2.3 % under the default seeds and 0.7 % under these.
ONE_STEP_SEEDS = {((6, 6, 1), 1024): (3, 4)}


def one_step_case(shape, B, dtype):
    seeds = ONE_STEP_SEEDS.get((shape, B), (20 + shape[0], 30 + shape[1]))
    arrays = random_arrays(shape, seeds[0])
    X, H, Y = pool_for(shape, B + 3, dtype, seeds[1])
    rng = np.random.default_rng(B)
    idx = rng.integers(0, B + 3, B)
    if B > 2:
        idx[1] = idx[0]                                                 # a duplicate: it counts twice
    else:
        idx = rng.permutation(B + 3)[:B]                                # (two copies of one window: no variance, every gradient 0)
    return dict(arrays=arrays, X=X, H=H, Y=Y, idx=idx)


# ---- B. one live window: H saturates every window but one, so every weight gradient flows from that single window
LIVE_SHAPE = (6, 6, 1)


def wgrad_range(B, g):
    """The windows of weight-gradient workgroup g: g B / G .. (g + 1) B / G, G = min(B, 128)."""
    G = min(B, 128)
    return g * B // G, (g + 1) * B // G


def live_slots(B):
    """Slot 0, slot B - 1, both sides of the first weight-gradient range boundary behind which the ranges are longer (at
    B = 130 the whole first long range and its neighbours), a slot whose head thread owns an earlier window, and the two
    slots where the halves of the loss tree meet."""
    slots = {0, B - 1}
    G = min(B, 128)
    lengths = [wgrad_range(B, g)[1] - wgrad_range(B, g)[0] for g in range(G)]
    if min(lengths) != max(lengths):
        g = lengths.index(max(lengths))
        assert g > 0 and lengths[g - 1] == max(lengths) - 1
        b0, b1 = wgrad_range(B, g)
        slots |= {b0 - 1, b0} | (set(range(b0, b1 + 1)) if B == 130 else set())
    if B > 256:
        slots.add(min(256 + 5, B - 2))          # (head thread 5 owns window 5 first; at B = 258 thread 0 owns 0 and 256)
    if B == 1024:
        slots |= {511, 512}
    return sorted(slots)


LIVE_CASES = [(B, live) for B in (130, 258, 1022, 1024) for live in live_slots(B)]


def one_live_case(B, live, shape=LIVE_SHAPE, saturate_all=False):
    arrays = random_arrays(shape, 13)
    X, H, Y = pool_for(shape, B, np.float32, 14)
    H = (Y * 60).astype("f")                    # every window saturated (e = exp(-60 +- cnn): outside (1e-6, 1e3)) ...
    if not saturate_all:
        H[live] = 0.1                           # ... but one
    return dict(arrays=arrays, X=X, H=H, Y=Y, idx=np.arange(B))


# ---- C. pool ties that reach the weight gradients.  Blocks 1 and 2 are made pointwise (centre-tap kernels, no bias), so
# block 2's output is a function of the input pixel alone: equal pixels give bit-equal activations in float64, in float32
# and on the GPU (the other taps multiply by 0, which adds nothing in any order), while their neighbourhoods, and with
# them the weight gradients that the pool's choice routes, differ.
TIE_SHAPES = [(6, 6, 2), (7, 6, 2)]
TIE_PATTERNS = [[0, 0, 0, 0], [0, 1, 1, 2], [1, 0, 2, 0], [0, 1, 2, 2], [2, 2, 0, 1], [1, 2, 0, 0]]


def pool_tie_case(shape, B=4, seed=17):
    m, n, Cc = shape
    rng = np.random.default_rng(seed)
    arrays = random_arrays(shape, seed)
    W0 = np.zeros((3, 3, Cc, 8), "f")
    W0[1, 1] = rng.choice(np.array([1, -1, 0.5, -0.5, 0.25], "f"), (Cc, 8))
    W6 = np.zeros((3, 3, 8, 8), "f")
    W6[1, 1] = np.diag(rng.choice(np.array([0.5, 1, 2, -1], "f"), 8))
    arrays[0], arrays[6] = W0, W6
    arrays[1], arrays[7] = np.zeros(8, "f"), np.zeros(8, "f")
    X, H, Y = pool_for(shape, B + 2, np.uint8, seed + 1)
    for b in range(B + 2):
        for y2 in range(m // 2):
            for x2 in range(n // 2):
                cell = X[b, 2 * y2:2 * y2 + 2, 2 * x2:2 * x2 + 2].reshape(4, Cc).copy()
                labels = TIE_PATTERNS[(b + 3 * y2 + x2) % len(TIE_PATTERNS)]
                X[b, 2 * y2:2 * y2 + 2, 2 * x2:2 * x2 + 2] = cell[labels].reshape(2, 2, Cc)
    return dict(arrays=arrays, X=X, H=H, Y=Y, idx=np.array([4, 0, 5, 2][:B]))


def _spread(picked, a, dpool):
    B, H, Wd, C = a.shape
    h2, w2 = H // 2, Wd // 2
    cells = picked * dpool[..., None]
    da = np.zeros_like(a)
    da[:, :2 * h2, :2 * w2] = cells.reshape(B, h2, w2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * h2, 2 * w2, C)
    return da


def pool2x2_backward_last(a, dpool):
    """A wrong pool: the gradient goes to the LAST maximum of a cell (a `>=` for the `>` of the kernel)."""
    last = 3 - tr._pool_cells(a)[..., ::-1].argmax(axis=4)
    return _spread(last[..., None] == np.arange(4), a, dpool)


def pool2x2_backward_all(a, dpool):
    """A wrong pool: every tied maximum of a cell receives the gradient."""
    cells = tr._pool_cells(a)
    return _spread(cells == cells.max(axis=4, keepdims=True), a, dpool)


def tie_census(a):
    """Of block 2's output a (B, m, n, 8): (tied, first), tied (B, m2, n2, 8) bool where a cell's positive maximum is held by
    more than one of its four pixels, first the position of the first of them."""
    cells = tr._pool_cells(a)
    top = cells.max(axis=4)
    return ((cells == top[..., None]).sum(axis=4) > 1) & (top > 0), cells.argmax(axis=4)


# ---- D. later steps and other constants
LATER_SHAPE, LATER_B = (5, 6, 3), 6
NONDEFAULT = dict(lr=1e-2, beta1=0.5, beta2=0.9, adam_epsilon=1e-3, momentum=0.5, bn_epsilon=0.1, dropout=0.5, seed=11)


def later_steps_case():
    """Three different index rows over one uint8 pool, default constants."""
    arrays = random_arrays(LATER_SHAPE, 31)
    X, H, Y = pool_for(LATER_SHAPE, 12, np.uint8, 32)
    rows = np.array([[0, 5, 5, 7, 11, 2], [3, 9, 1, 10, 4, 4], [8, 6, 2, 0, 7, 11]])
    return dict(arrays=arrays, X=X, H=H, Y=Y, rows=rows)


@functools.lru_cache(maxsize=None)
def _nondefault_state():
    base = later_steps_case()
    arrays, m, v = base["arrays"], None, None
    for t, row in enumerate(base["rows"][:2]):
        _, st = statement(arrays, base["X"], base["H"], base["Y"], row, np.float32, steps_before=t, m=m, v=v, **NONDEFAULT)
        arrays, m, v = st["params"], st["m"], st["v"]
    return arrays, m, v


def nondefault_case(hyper=None):
    """One step under NONDEFAULT (or `hyper`) from the state that two float32 statement steps under NONDEFAULT leave:
    non-zero m and v and t = 2, so that every constant enters the result."""
    base = later_steps_case()
    arrays, m, v = ([a.copy() for a in part] for part in _nondefault_state())
    return dict(arrays=arrays, m=m, v=v, steps_before=2, X=base["X"], H=base["H"], Y=base["Y"], idx=base["rows"][2],
                hyper=dict(NONDEFAULT if hyper is None else hyper))
