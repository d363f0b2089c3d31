"""CNN verification -- drop-in for ``waldboost.verification``, inference and training: a small CNN re-scores the
windows a cascade lets through, ``p(X, H) = sigmoid(cnn(X) + H)`` (reference verification.py:1-16).

What runs where:

* the forward pass of ``model_cnn`` (reference verification.py:28-56) is two HIP kernels behind ``wb_verify_launch``
  (csrc/wb_verify.hip), on crops that are already on the GPU;
* ``Verifier`` holds the network's 28 arrays as Keras orders them (``model_cnn(...).get_weights()`` of the reference),
  folds batch normalisation into the convolutions once, on the host, in float64, and uploads the packed result once
  per device;
* ``detect_and_verify`` (reference verification.py:85-105, with ``get_boxes`` for its ``get_bbs`` slip) scans the image
  like ``samples.get_samples_from_image`` does and gathers the crops of every detection on the device: they never travel
  to the host;
* ``train`` (reference verification.py:63-81) and ``Trainer`` run Keras's ``train_on_batch`` for this network on the GPU:
  the forward pass in training mode (batch statistics, dropout), exploss, the backward pass and Adam are HIP kernels
  behind ``wb_verify_train_step`` (csrc/wb_verify_train.hip), over a sample pool that is uploaded
  once; no autograd, no torch.nn.  Training is deterministic to the bit for a seed; it is held to a float64 statement
  within a measured margin, not to bits.  The convolution biases never move (their gradient is zero under batch
  statistics), a deliberate difference from Keras with no effect on the trained function.  A Keras model itself is still
  trained with the reference and imported with ``Verifier.from_keras_weights(input_shape, M.get_weights())``.

The inference arithmetic is fixed to the bit: every pre-activation is one float32 fused-multiply-add chain in a
stated order, so a window's result depends neither on the batch it sits in nor on the run.  It differs from Keras's own
float32 evaluation (batch normalisation applied after the convolution, accumulation order of its backend) by rounding.
"""
import ctypes as C

import numpy as np

from . import _native as nat

HIDDEN = 128
_CONV_OUT = (8, 8, 16, 16)
_SCRATCH_BYTES = 256 << 20          # predict's chunks keep the feature scratch at or below this


def _conv_in(C_in):
    return (int(C_in), 8, 8, 16)


def _flat_features(input_shape):
    m, n, _ = input_shape
    return (m // 2) * (n // 2) * 16


def _expected_shapes(input_shape):
    """Shapes of the 28 arrays of model_cnn(input_shape).get_weights(), in Keras's order."""
    shapes = []
    for cin, cout in zip(_conv_in(input_shape[2]), _CONV_OUT):
        shapes += [(3, 3, cin, cout)] + [(cout,)] * 5      # kernel, bias, gamma, beta, moving_mean, moving_variance
    F = _flat_features(input_shape)
    return shapes + [(F, HIDDEN), (HIDDEN,), (HIDDEN, 1), (1,)]


def fold_batchnorm(kernel, bias, gamma, beta, mean, variance, epsilon):
    """(W', b') float32 of one convolution block: s = gamma / sqrt(variance + epsilon), W' = W * s[o],
    b' = (b - mean) * s + beta, in float64, rounded to float32 once."""
    f8 = lambda a: np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        s = f8(gamma) / np.sqrt(f8(variance) + float(epsilon))
        return (f8(kernel) * s).astype(np.float32), ((f8(bias) - f8(mean)) * s + f8(beta)).astype(np.float32)


class Verifier:
    """The verification CNN for windows of `input_shape` = (m, n, C).  `arrays`: the 28 float arrays of the reference's
    model_cnn(input_shape).get_weights(); they are copied and kept unfolded (get_weights, save)."""

    def __init__(self, input_shape, arrays, epsilon=1e-3):
        shape = tuple(int(x) for x in input_shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"input_shape must be (m, n, C), got {input_shape!r}")
        self.input_shape = shape
        self.epsilon = float(epsilon)
        self._scratch = nat.Scratch()          # the feature scratch
        self.set_weights(arrays)

    def set_weights(self, arrays):
        """Replace the 28 arrays (the constructor's checks), fold again and drop the weights cached on the devices: predict
        uses the new ones from the next call on.  Nothing changes when the arrays are refused."""
        shape = self.input_shape
        arrays = list(arrays)
        want = _expected_shapes(shape)
        if len(arrays) != len(want):
            raise ValueError(f"expected the {len(want)} arrays of model_cnn(...).get_weights(), got {len(arrays)}")
        kept = []
        for k, (a, w) in enumerate(zip(arrays, want)):
            a = np.array(a, dtype=np.float32)
            if a.shape != w:
                raise ValueError(f"array {k} has shape {a.shape}, expected {w} for input_shape {shape}")
            if not np.isfinite(a).all():
                raise ValueError(f"array {k} holds non-finite values")
            a.setflags(write=False)
            kept.append(a)
        before = getattr(self, "arrays", None)
        self.arrays = kept
        try:
            self._packed = self._fold()
        except ValueError:
            self.arrays = before
            raise
        self._device = {}           # device index -> packed weights

    # ---- construction, files
    @staticmethod
    def from_keras_weights(input_shape, arrays, epsilon=1e-3):
        """From model_cnn(input_shape).get_weights() of the reference: per convolution block kernel (3, 3, Cin, Cout), bias,
        gamma, beta, moving_mean, moving_variance; then the dense kernel (F, 128), its bias, the dense kernel (128, 1), its bias."""
        return Verifier(input_shape, arrays, epsilon)

    def get_weights(self):
        return [a.copy() for a in self.arrays]

    def save(self, filename):
        """.npz, no pickle."""
        np.savez(filename, input_shape=np.array(self.input_shape, np.int64), epsilon=np.float64(self.epsilon),
                 **{f"w{k:02d}": a for k, a in enumerate(self.arrays)})

    @staticmethod
    def load(filename):
        with np.load(filename, allow_pickle=False) as z:
            keys = sorted(k for k in z.files if k.startswith("w"))
            return Verifier(tuple(int(x) for x in z["input_shape"]), [z[k] for k in keys], float(z["epsilon"]))

    # ---- weights
    def _fold(self):
        """The packed float32 buffer wb_verify_launch reads (include/waldboost_hip.h has the layout)."""
        parts = []
        for k in range(4):
            w, b = fold_batchnorm(*self.arrays[6 * k:6 * k + 6], self.epsilon)
            parts += [w.reshape(-1), b]
        parts += [self.arrays[24].reshape(-1), self.arrays[25], self.arrays[26].reshape(-1), self.arrays[27]]
        packed = np.ascontiguousarray(np.concatenate(parts), np.float32)
        if not np.isfinite(packed).all():
            raise ValueError("folding batch normalisation gives non-finite weights (moving_variance + epsilon must be positive)")
        return packed

    def folded(self):
        """[(W', b') of the four convolutions] + [dense0 kernel, bias, dense1 kernel, bias], float32 copies."""
        out, at = [], 0
        for cin, cout in zip(_conv_in(self.input_shape[2]), _CONV_OUT):
            out.append((self._packed[at:at + 9 * cin * cout].reshape(3, 3, cin, cout).copy(),
                        self._packed[at + 9 * cin * cout:at + 9 * cin * cout + cout].copy()))
            at += 9 * cin * cout + cout
        return out + [a.copy() for a in self.arrays[24:]]

    def _weights_on(self, dev):
        import torch
        key = dev.index
        if key not in self._device:
            m, n, Cc = self.input_shape
            count = nat.query("wb_verify_weights_floats", m, n, Cc)
            assert count == self._packed.size, (count, self._packed.size)
            self._device[key] = torch.from_numpy(self._packed).to(dev)
        return self._device[key]

    # ---- inference
    def _checked(self, inputs):
        try:
            samples, scores = inputs
        except (TypeError, ValueError):
            raise ValueError("predict takes [samples, scores]") from None
        on_device = nat.is_tensor(samples)
        if not on_device:
            samples = np.asarray(samples)
        if not nat.is_tensor(scores):
            scores = np.asarray(scores)
        if len(samples.shape) != 4 or tuple(samples.shape[1:]) != self.input_shape:
            raise ValueError(f"samples of shape {tuple(samples.shape)}, expected (N,) + {self.input_shape}")
        if nat.window_codes(samples) is None:
            raise NotImplementedError(f"samples must be float32 or uint8, got {nat.dtype_name(samples)}")
        if not on_device and samples.dtype == np.float32 and not np.isfinite(samples).all():
            raise ValueError("samples hold non-finite values")
        N = int(samples.shape[0])
        if tuple(scores.shape) not in ((N,), (N, 1)):
            raise ValueError(f"scores of shape {tuple(scores.shape)}, expected ({N},) or ({N}, 1)")
        return samples, scores, N

    def predict_device(self, inputs, batch_size=None):
        """predict with the result left on the device: a float32 tensor (N, 1).  No host synchronisation when samples and
        scores are device tensors."""
        import torch
        samples, scores, N = self._checked(inputs)
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        dev = nat.require_gpu()
        m, n, Cc = self.input_shape
        weights = self._weights_on(dev)                     # (refuses a window shape the kernels do not take)
        X, wdt = nat.window_tensor(samples, dev)
        H = scores if nat.is_tensor(scores) else torch.from_numpy(np.ascontiguousarray(scores, np.float32))
        H = H.to(dev, torch.float32).reshape(-1).contiguous()
        out = torch.empty((N, 1), dtype=torch.float32, device=dev)
        if N == 0:
            return out
        F = _flat_features(self.input_shape)
        chunk = int(batch_size) if batch_size is not None else max(64, _SCRATCH_BYTES // (4 * F) // 64 * 64)
        chunk = min(chunk, N)
        scratch = self._scratch.on(dev, nat.query("wb_verify_scratch_bytes", m, n, Cc, chunk))
        flat = out.reshape(-1)
        for at in range(0, N, chunk):
            k = min(chunk, N - at)
            nat.launch("wb_verify_launch", X[at:], wdt, k, m, n, Cc, weights, H[at:], scratch, scratch.numel(), flat[at:])
        return out

    def predict(self, inputs, batch_size=None):
        """cnn(samples) + scores as float32 (N, 1), the shape Keras's predict returns.  inputs = [samples, scores]: samples
        (N, m, n, C) float32 or uint8, ndarray or device tensor; scores (N,) or (N, 1).  batch_size: windows per launch
        (None: as many as keep the scratch bounded); the result does not depend on it."""
        return self.predict_device(inputs, batch_size).cpu().numpy()


def model_cnn(input_shape, seed=None):
    """A Verifier with Keras's default initialisers (reference verification.py:28-56): glorot-uniform kernels, zero biases,
    batch normalisation gamma 1, beta 0, moving_mean 0, moving_variance 1.  The generator is NumPy's (`seed`)."""
    rng = np.random.default_rng(seed)

    def glorot(shape, fan_in, fan_out):
        limit = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-limit, limit, shape).astype(np.float32)

    arrays = []
    for cin, cout in zip(_conv_in(input_shape[2]), _CONV_OUT):
        arrays += [glorot((3, 3, cin, cout), 9 * cin, 9 * cout), np.zeros(cout, "f"), np.ones(cout, "f"), np.zeros(cout, "f"),
                   np.zeros(cout, "f"), np.ones(cout, "f")]
    F = _flat_features(input_shape)
    arrays += [glorot((F, HIDDEN), F, HIDDEN), np.zeros(HIDDEN, "f"), glorot((HIDDEN, 1), HIDDEN, 1), np.zeros(1, "f")]
    return Verifier(input_shape, arrays)


def exploss(y_true, y_pred):
    """The reference's training loss (verification.py:59-60), in NumPy."""
    return np.maximum(np.minimum(np.exp(-np.asarray(y_true) * np.asarray(y_pred)), 1e3), 1e-6)


class Trainer:
    """Training state of a Verifier on the GPU: the 28 arrays in the training layout (include/waldboost_hip.h), Adam's m
    and v, and the step count t, all resident.  A step is wb_verify_train_step: Keras's train_on_batch for model_cnn under
    exploss and Adam(lr).  `seed` feeds the dropout generator (None: drawn from the system)."""

    def __init__(self, verifier, lr=1e-4, seed=None, dropout=0.2, momentum=0.99):
        import torch
        if not isinstance(verifier, Verifier):
            raise TypeError(f"Trainer takes a Verifier, got {type(verifier).__name__}")
        if not (np.isfinite(lr) and lr >= 0):
            raise ValueError(f"lr must be finite and not negative, got {lr!r}")
        if not 0 <= dropout < 1:
            raise ValueError(f"dropout must lie in [0, 1), got {dropout!r}")
        if not 0 <= momentum <= 1:
            raise ValueError(f"momentum must lie in [0, 1], got {momentum!r}")
        self.verifier = verifier
        self.seed = int(np.random.SeedSequence(seed).generate_state(1)[0]) if seed is None else int(seed) & 0xFFFFFFFF
        self.hyper = nat.WbVerifyTrainHyper(lr=float(lr), beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=float(momentum),
                                            bn_epsilon=verifier.epsilon, dropout=float(dropout), seed=self.seed, reserved=0)
        count = nat.query("wb_verify_train_param_floats", *verifier.input_shape)
        flat = np.concatenate([a.reshape(-1) for a in verifier.arrays]).astype(np.float32)
        assert flat.size == count, (flat.size, count)
        dev = nat.require_gpu()
        self.device = dev
        self.params = torch.from_numpy(flat).to(dev)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.t = torch.zeros(2, dtype=torch.int32, device=dev)
        self._scratch = nat.Scratch()

    # ---- the pool
    def _pool(self, X, H, Y):
        """(X, x_dtype code, H, Y, N) on the device, checked."""
        import torch
        on_device = nat.is_tensor(X)
        if not on_device:
            X = np.asarray(X)
        if len(X.shape) != 4 or tuple(X.shape[1:]) != self.verifier.input_shape or X.shape[0] < 1:
            raise ValueError(f"samples of shape {tuple(X.shape)}, expected (N,) + {self.verifier.input_shape} with N >= 1")
        if nat.window_codes(X) is None:
            raise NotImplementedError(f"samples must be float32 or uint8, got {nat.dtype_name(X)}")
        if not on_device and X.dtype == np.float32 and not np.isfinite(X).all():
            raise ValueError("samples hold non-finite values")
        N = int(X.shape[0])
        Xd, wdt = nat.window_tensor(X, self.device)
        vecs = []
        for name, v in (("scores", H), ("targets", Y)):
            if not nat.is_tensor(v):
                v = np.ascontiguousarray(v, np.float32)
                if not np.isfinite(v).all():
                    raise ValueError(f"{name} hold non-finite values")
                v = torch.from_numpy(v)
            if tuple(v.shape) not in ((N,), (N, 1)):
                raise ValueError(f"{name} of shape {tuple(v.shape)}, expected ({N},) or ({N}, 1)")
            vecs.append(v.to(self.device, torch.float32).reshape(-1).contiguous())
        return Xd, wdt, vecs[0], vecs[1], N

    def _steps(self, pool, idx, grads=None):
        """idx (steps, B) int32 on the device -> the device losses (steps,).  No host wait."""
        import torch
        Xd, wdt, Hd, Yd, N = pool
        steps, B = (int(x) for x in idx.shape)
        m, n, Cc = self.verifier.input_shape
        losses = torch.empty(steps, dtype=torch.float32, device=self.device)
        scratch = self._scratch.on(self.device, nat.query("wb_verify_train_scratch_bytes", m, n, Cc, B)) if steps else None
        for s in range(steps):
            nat.launch("wb_verify_train_step", Xd, wdt, Hd, Yd, N, idx[s], B, m, n, Cc, self.params, self.adam_m, self.adam_v,
                       self.t, C.byref(self.hyper), scratch, scratch.numel(), losses[s:], grads)
        return losses

    def upload(self, X, H, Y):
        """A resident pool for run: samples (N, m, n, C) float32 or uint8, scores and targets (N,), ndarray or device tensor."""
        return self._pool(X, H, Y)

    def _indices(self, idx, N):
        import torch
        if nat.is_tensor(idx):
            host = idx.detach().cpu().numpy()
        else:
            host = np.asarray(idx)
        if host.ndim != 2 or host.dtype.kind not in "iu":
            raise ValueError("idx must be an integer array of shape (steps, B)")
        if host.size and (host.min() < 0 or host.max() >= N):
            raise ValueError(f"idx must lie in 0 .. {N - 1}")
        B = host.shape[1]
        if B < 2 or B > 1024 or B % 2:
            raise NotImplementedError(f"a batch of {B} windows: supported are even sizes 2 .. 1024")
        return torch.from_numpy(np.ascontiguousarray(host, np.int32)).to(self.device)

    # ---- steps
    def run(self, X, H, Y, idx, pool=None):
        """idx.shape[0] steps over the resident pool (X, H, Y) -- or a pool from upload(): step s trains on the windows
        idx[s] (B indices into the pool, duplicates count).  Returns the steps' losses as a device tensor; no wait."""
        pool = pool if pool is not None else self._pool(X, H, Y)
        return self._steps(pool, self._indices(idx, pool[4]))

    def train_on_batch(self, X, H, Y):
        """One step on the batch (X, H, Y) as it stands; returns its loss (a host wait)."""
        pool = self._pool(X, H, Y)
        idx = np.arange(pool[4], dtype=np.int32)[None]
        return float(self._steps(pool, self._indices(idx, pool[4])).cpu().numpy()[0])

    @property
    def steps_done(self):
        return int(self.t.cpu().numpy()[0])

    def get_weights(self):
        """The 28 arrays as they stand on the device."""
        flat = self.params.cpu().numpy()
        out, at = [], 0
        for a in self.verifier.arrays:
            out.append(flat[at:at + a.size].reshape(a.shape).copy())
            at += a.size
        return out

    def commit(self):
        """Write the parameters back into the verifier (set_weights: re-fold, caches dropped)."""
        self.verifier.set_weights(self.get_weights())
        return self.verifier


def _draw_epoch(rng, N0, N1, steps, b):
    """An epoch's pool indices (steps, 2 b): b negatives (0 .. N0 - 1), then b positives (N0 .. N0 + N1 - 1), with replacement."""
    return np.concatenate([rng.integers(0, N0, (steps, b)), N0 + rng.integers(0, N1, (steps, b))], axis=1)


_TRAIN_REFUSAL = ("waldboost_amd.verification trains its own Verifier only: train a Keras model with the reference "
                  "(waldboost.verification.train) and import the result with Verifier.from_keras_weights(input_shape, M.get_weights())")


def train(M, X0, H0, X1, H1, epochs=10, batch_size=64, steps=1000, *, lr=1e-4, seed=None, trainer=None,
          verbose=True):
    """The reference's train (verification.py:63-81) on the GPU: `epochs` times `steps` steps of Adam(lr) under exploss on
    batches of batch_size // 2 negatives (X0, H0; target -1) and as many positives (X1, H1; target +1), drawn with
    replacement.  M, a Verifier, is updated in place; the epochs' mean losses are returned (and printed when `verbose`,
    as the reference does).  X0 / X1: (N, m, n, C) float32 or uint8, ndarray or device tensor.  The pool is uploaded once;
    per epoch the indices are drawn on the host (numpy's generator from `seed`), uploaded once, and one wait fetches the
    mean.  `trainer`: a Trainer of M to continue with (Adam state, step count, dropout seed).  Anything but a Verifier is
    refused: a Keras model is trained with the reference and imported with from_keras_weights."""
    import torch
    if not isinstance(M, Verifier):
        raise NotImplementedError(_TRAIN_REFUSAL)
    epochs, steps, b = int(epochs), int(steps), int(batch_size) // 2
    if epochs < 0 or steps < 1:
        raise ValueError("epochs must not be negative and steps must be positive")
    if b < 1 or 2 * b > 1024:
        raise NotImplementedError(f"batch_size {batch_size}: supported are 2 .. 1025")
    if trainer is None:
        trainer = Trainer(M, lr=lr, seed=seed)
    elif trainer.verifier is not M:
        raise ValueError("the trainer belongs to another verifier")
    N0, N1 = int(X0.shape[0]), int(X1.shape[0])
    if N0 < 1 or N1 < 1:
        raise ValueError("both classes need samples")
    both = [X0, X1]
    if any(nat.is_tensor(x) for x in both):
        both = [x if nat.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)) for x in both]
        if both[0].dtype != both[1].dtype:
            raise ValueError("X0 and X1 must have one dtype")
        X = torch.cat([x.to(trainer.device) for x in both])
    else:
        both = [np.asarray(x) for x in both]
        if both[0].dtype != both[1].dtype:
            raise ValueError("X0 and X1 must have one dtype")
        X = np.concatenate(both)
    host = lambda v: v.detach().cpu().numpy() if nat.is_tensor(v) else np.asarray(v)
    H = np.concatenate([host(H0).reshape(-1), host(H1).reshape(-1)]).astype(np.float32)
    Y = np.concatenate([-np.ones(N0, np.float32), np.ones(N1, np.float32)])
    pool = trainer.upload(X, H, Y)
    rng = np.random.default_rng(seed)
    means = []
    for e in range(1, epochs + 1):
        if verbose:
            print(f"Epoch {e}/{epochs}")
        idx = _draw_epoch(rng, N0, N1, steps, b)
        losses = trainer.run(None, None, None, idx, pool=pool)
        means.append(float(losses.cpu().numpy().astype(np.float64).mean()))           # the epoch's one wait
        if verbose:
            print(means[-1])
    trainer.commit()
    if verbose:
        print("Done")
    return means


def detect_and_verify(image, model, verifier):
    """Detections of `model` on `image`, re-scored by `verifier` (reference verification.py:85-105): (bbs, scores), a
    float32 (N, 4) array and a float32 (N,) array in Model.detect's order (levels in pyramid order, row-major inside a
    level); ([], []) when nothing is detected.  The scan is Model.scan_resident (float or uint8 channels, not
    rank bytes); the crops are gathered from the resident pyramid and stay on the device.  One upload (the window origins
    and scores) and two host waits: the scan's read-back and the scores.  n_loc / n_weak advance as in a scan."""
    import torch
    if tuple(int(x) for x in model.shape) != verifier.input_shape:
        raise ValueError(f"the model's window shape {tuple(model.shape)} is not the verifier's input_shape {verifier.input_shape}")
    scanned = model.scan_resident(image)                    # wait 1: detections, in (level, r, c) order
    if scanned is None or scanned[1]["scores"].size == 0:
        return [], []
    eng, found = scanned
    N = int(found["scores"].size)
    dev = nat.require_gpu()
    m, n, Cc = verifier.input_shape
    tdt, wdt = eng.chn.dtype, eng.spec.wb_dtype
    # rows, columns and score bits in one upload
    host = np.stack([found["r"].astype(np.int32), found["c"].astype(np.int32),
                     np.ascontiguousarray(found["scores"], np.float32).view(np.int32)])
    sent = torch.from_numpy(host).to(dev)
    crops = torch.empty((N, m, n, Cc), dtype=tdt, device=dev)
    level = found["level"]
    cuts = np.flatnonzero(np.diff(level, prepend=-1, append=-1))      # starts of the runs of one level, then N
    for a, b in zip(cuts[:-1], cuts[1:]):
        chns = eng.level_tensor(0, int(level[a]))
        assert chns.is_contiguous() and chns.dtype == tdt
        u, v, _ = (int(x) for x in chns.shape)
        nat.launch("wb_gather_samples_launch", chns, wdt, u, v, Cc, sent[0, a:], sent[1, a:], int(b - a), m, n, crops[a:])
    scores = verifier.predict_device([crops, sent[2].view(torch.float32)])
    return found["boxes"], scores.cpu().numpy().reshape(-1)              # wait 2
