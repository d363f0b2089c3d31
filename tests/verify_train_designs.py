"""Designed inputs shared by the host and the GPU tests of the verifier's training: the planted two-class pool of the
end-to-end case, and that case run through the NumPy statement with the batches verification.train draws."""
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
