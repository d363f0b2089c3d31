"""The training step of the verification CNN in NumPy: what wb_verify_train_step computes, stated in
the dtype asked for (float64 is the yardstick of the GPU tests, float32 gives the error a float32 evaluation of the same
formulas makes).  No fixed summation order is claimed here: the GPU is held to the float64 result within a margin, not to
bits.

    arrays   the 28 arrays of model_cnn(...).get_weights(), Keras's order
    X, H, Y  the batch: crops (B, m, n, C), detector scores (B,), targets (B,) of -1 / +1
    masks    None (no dropout), or (keep0 (B, F) bool, keep1 (B, 128) bool) with `scale` = 1 / (1 - rate)

The dropout generator is restated with uint32 arithmetic (drop_bits); dropout_masks gives a step's masks."""
import numpy as np

HIDDEN = 128
_M32 = np.uint64(0xFFFFFFFF)


# ---- the dropout generator
def fmix32(x):
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def drop_key(seed, step, layer):
    inner = fmix32(np.uint32((2 * int(step) + int(layer) + 0x9E3779B9) & 0xFFFFFFFF))
    return fmix32(np.uint32(int(seed) & 0xFFFFFFFF) ^ inner)


def drop_bits(seed, step, layer, count):
    """The 32 bits of elements 0 .. count - 1 of `layer` (0: the flat features, 1: the hidden units) at `step`."""
    index = np.arange(count, dtype=np.uint32)
    with np.errstate(over="ignore"):
        return fmix32((index * np.uint32(0x9E3779B1)) ^ drop_key(seed, step, layer))


def drop_threshold(rate):
    return int(round(float(rate) * 2 ** 32))


def drop_keep(seed, step, layer, count, rate):
    return drop_bits(seed, step, layer, count).astype(np.uint64) >= np.uint64(drop_threshold(rate))


def dropout_masks(seed, step, B, F, rate):
    return drop_keep(seed, step, 0, B * F, rate).reshape(B, F), drop_keep(seed, step, 1, B * HIDDEN, rate).reshape(B, HIDDEN)


def dropout_scale(rate):
    return float(np.float32(1.0 / (1.0 - float(rate))))


# ---- layers
def conv3x3(x, W):
    B, H, Wd, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, Wd, W.shape[3]), x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + Wd, :] @ W[ky, kx]
    return out


def conv3x3_backward(x, W, dz):
    """(dx, dW) of z = conv3x3(x, W)."""
    B, H, Wd, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dzp = np.pad(dz, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dx, dW = np.zeros_like(x), np.zeros_like(W)
    for ky in range(3):
        for kx in range(3):
            dW[ky, kx] = np.einsum("bhwi,bhwo->io", xp[:, ky:ky + H, kx:kx + Wd, :], dz)
            dx += dzp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + Wd, :] @ W[ky, kx].T
    return dx, dW


def _pool_cells(a):
    B, H, Wd, C = a.shape
    h2, w2 = H // 2, Wd // 2
    return a[:, :2 * h2, :2 * w2].reshape(B, h2, 2, w2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, h2, w2, C, 4)


def pool2x2(a):
    return _pool_cells(a).max(axis=4)


def pool2x2_backward(a, dpool):
    """The gradient goes to the first maximum of a cell in (row, column) order; dropped rows / columns get zero."""
    B, H, Wd, C = a.shape
    h2, w2 = H // 2, Wd // 2
    first = _pool_cells(a).argmax(axis=4)                               # (argmax returns the first maximum)
    cells = (first[..., None] == np.arange(4)) * dpool[..., None]       # (B, h2, w2, C, 4)
    da = np.zeros_like(a)
    da[:, :2 * h2, :2 * w2] = cells.reshape(B, h2, w2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * h2, 2 * w2, C)
    return da


def forward_backward(arrays, X, H, Y, dtype=np.float64, masks=None, scale=1.0, epsilon=1e-3, zero_conv_bias=True):
    """One forward and backward pass in training mode.  Returns a dict: loss, p (B,), grads (28 arrays in Keras's order:
    the moving_mean / moving_variance slots hold the batch mean and the unbiased batch variance), losses (B,)."""
    dt = np.dtype(dtype).type
    P = [np.asarray(a).astype(dt) for a in arrays]
    x = np.asarray(X).astype(dt)
    H, Y = np.asarray(H).astype(dt).reshape(-1), np.asarray(Y).astype(dt).reshape(-1)
    B = x.shape[0]
    eps, scale = dt(epsilon), dt(scale)
    kept = []
    for k in range(4):
        W, bias, gamma, beta = P[6 * k:6 * k + 4]
        z = conv3x3(x, W) + bias
        mu = z.mean(axis=(0, 1, 2), dtype=dt)
        var = ((z - mu) ** 2).mean(axis=(0, 1, 2), dtype=dt)
        inv = dt(1) / np.sqrt(var + eps)
        xhat = (z - mu) * inv
        y = gamma * xhat + beta
        a = np.where(y > 0, y, dt(0))
        kept.append((x, xhat, inv, a, mu, var, z.size // z.shape[3]))
        x = a
        if k == 1:
            x = pool2x2(a)
    flat = x.reshape(B, -1)
    keep0, keep1 = masks if masks is not None else (np.ones(flat.shape, bool), np.ones((B, HIDDEN), bool))
    flat_d = np.where(keep0, flat * scale, dt(0))
    u = flat_d @ P[24] + P[25]
    hd = np.where(keep1, np.where(u > 0, u, dt(0)) * scale, dt(0))
    p = hd @ P[26].reshape(-1) + P[27][0] + H
    e = np.exp(-Y * p)
    losses = np.clip(e, dt(1e-6), dt(1e3))
    loss = losses.mean(dtype=dt)
    dp = np.where((e > dt(1e-6)) & (e < dt(1e3)), -Y * e / dt(B), dt(0))

    grads = [None] * 28
    grads[26] = (hd.T @ dp).reshape(HIDDEN, 1)
    grads[27] = dp.sum(dtype=dt).reshape(1)
    du = np.where((u > 0) & keep1, np.outer(dp, P[26].reshape(-1)) * scale, dt(0))
    grads[24] = flat_d.T @ du
    grads[25] = du.sum(axis=0, dtype=dt)
    da = np.where(keep0, (du @ P[24].T) * scale, dt(0)).reshape(x.shape)
    for k in (3, 2, 1, 0):
        xin, xhat, inv, a, mu, var, n = kept[k]
        if k == 1:
            da = pool2x2_backward(a, da)
        dy = np.where(a > 0, da, dt(0))
        dbeta = dy.sum(axis=(0, 1, 2), dtype=dt)
        dgamma = (dy * xhat).sum(axis=(0, 1, 2), dtype=dt)
        dz = P[6 * k + 2] * inv * (dy - dbeta / dt(n) - xhat * (dgamma / dt(n)))
        da, dW = conv3x3_backward(xin, P[6 * k], dz)
        grads[6 * k] = dW
        grads[6 * k + 1] = np.zeros_like(P[6 * k + 1]) if zero_conv_bias else dz.sum(axis=(0, 1, 2), dtype=dt)
        grads[6 * k + 2], grads[6 * k + 3] = dgamma, dbeta
        grads[6 * k + 4], grads[6 * k + 5] = mu, var * (dt(n) / dt(n - 1))
    return {"loss": loss, "p": p, "grads": grads, "losses": losses}


def loss_of(arrays, X, H, Y, masks=None, scale=1.0, epsilon=1e-3):
    """The float64 training-mode loss alone (finite differences)."""
    return float(forward_backward(arrays, X, H, Y, np.float64, masks, scale, epsilon)["loss"])


# ---- the update
ADAM = dict(lr=1e-4, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99)


def is_moving(k):
    return k < 24 and k % 6 >= 4


def is_conv_bias(k):
    return k < 24 and k % 6 == 1


def new_state(arrays, dtype=np.float64):
    dt = np.dtype(dtype).type
    P = [np.asarray(a).astype(dt) for a in arrays]
    return {"params": P, "m": [np.zeros_like(a) for a in P], "v": [np.zeros_like(a) for a in P], "t": 0}


def update(state, grads, dtype=np.float64, lr=1e-4, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99):
    """Adam on kernels, gamma, beta and the dense layers; the convolution biases stay; the moving statistics follow."""
    dt = np.dtype(dtype).type
    t = state["t"] + 1
    lr_t = dt(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
    b1, b2, mom = dt(beta1), dt(beta2), dt(momentum)
    for k in range(28):
        g = np.asarray(grads[k]).astype(dt).reshape(state["params"][k].shape)
        if is_conv_bias(k):
            continue
        if is_moving(k):
            state["params"][k] = mom * state["params"][k] + (dt(1) - mom) * g
            continue
        state["m"][k] = b1 * state["m"][k] + (dt(1) - b1) * g
        state["v"][k] = b2 * state["v"][k] + (dt(1) - b2) * (g * g)
        state["params"][k] = state["params"][k] - lr_t * state["m"][k] / (np.sqrt(state["v"][k]) + dt(adam_epsilon))
    state["t"] = t
    return state


def train_step(state, X, H, Y, dtype=np.float64, seed=0, dropout=0.2, epsilon=1e-3, **adam):
    """One whole step on `state` (new_state): the masks of step state["t"], forward, backward, update.  Returns the
    forward_backward dict."""
    B = np.asarray(X).shape[0]
    F = (X.shape[1] // 2) * (X.shape[2] // 2) * 16
    masks = dropout_masks(seed, state["t"], B, F, dropout) if dropout > 0 else None
    out = forward_backward(state["params"], X, H, Y, dtype, masks, dropout_scale(dropout), epsilon)
    update(state, out["grads"], dtype, **adam)
    return out


def flatten(arrays):
    """The training layout: the 28 arrays one after the other."""
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
