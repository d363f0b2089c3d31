"""Threshold calibration of a trained cascade: direct backward pruning (Zhang & Viola, "Multiple-Instance Pruning
For Learning Efficient Cascade Detectors", 2007, the single-instance form) on a set of positive samples.

The reference fits a stage's rejection threshold only while that stage is trained (training.py
``fit_rejection_threshold``); another recall / speed trade-off means training again.  Here the thetas of a finished
model are chosen for an operating point:

  * F[i] is the final score of positive i with no rejection at all;
  * ``floor`` is the keep-th largest F, keep = min(N, max(1, ceil(recall * N))); the RETAINED samples are {F >= floor}
    (ties at the floor are all retained);
  * theta[t] is the smallest running score any retained sample has after stage t (minus ``margin``).

So every retained positive passes every stage with its score unchanged, every other positive of the set is rejected
somewhere, and no theta can be raised without losing a retained sample.  The running scores (fp32, ``h = h + pred`` in
stage order) and the minimum (on order-preserving integer keys) come from csrc/wb_cascade.hip:
wb_samples_trace_launch and wb_calib_min_launch; the selection of the floor is a device sort.  tests/calib_reference.py
is the NumPy statement.
"""
import ctypes as C
import math

import numpy as np

from . import _native as nat
from .compare import channel_tensor


def sample_count(model, X):
    """N of samples X[N, m, n, C] for `model`; ValueError for another shape."""
    shape = tuple(int(x) for x in getattr(X, "shape", ()))
    if len(shape) != 4 or shape[1:] != tuple(int(x) for x in model.shape):
        raise ValueError(f"Invalid shape of X. Expected (N, {', '.join(str(int(x)) for x in model.shape)}), given {shape}")
    return shape[0]


def _samples(model, X):
    """(device tensor, WB_DTYPE_*, N) of samples X[N, m, n, C] for `model`; ValueError for another shape."""
    N = sample_count(model, X)
    Xd, wdt = channel_tensor(X, nat.require_gpu())
    return Xd, wdt, N


def trace_launch(model, X, reject, trace=False, final=False, alive=False):
    """wb_samples_trace_launch on samples X -> (trace [T, N], final [N], alive [T + 1]) as device tensors, None for the
    outputs not asked for.  N >= 1."""
    import torch
    Xd, wdt, N = _samples(model, X)
    T = len(model)
    dm = model.device_cascade()
    dev = Xd.device
    out = (torch.empty((T, N), dtype=torch.float32, device=dev) if trace else None,
           torch.empty(N, dtype=torch.float32, device=dev) if final else None,
           torch.empty(T + 1, dtype=torch.int32, device=dev) if alive else None)
    nat.check(nat.load().wb_samples_trace_launch(nat.stream_ptr(), dm.handle, nat.ptr(Xd), wdt, N, int(bool(reject)),
                                                 nat.ptr(out[0]), nat.ptr(out[1]), nat.ptr(out[2])), "wb_samples_trace_launch")
    return out


def stage_scores(model, X, reject=False, device=False):
    """Model.stage_scores (see there)."""
    import torch
    T = len(model)
    N = sample_count(model, X)
    if N * T >= 2 ** 31:
        raise ValueError(f"a trace of {N} samples x {T} stages has 2**31 entries or more: split the samples")
    if N == 0 or T == 0:
        return torch.empty((N, T), dtype=torch.float32, device=nat.require_gpu()) if device else np.empty((N, T), np.float32)
    tr = trace_launch(model, X, reject, trace=True)[0].t()
    return tr if device else tr.cpu().numpy()


def stage_survival(model, X):
    """int64 (T + 1,): how many of the samples X[N, m, n, C] enter each stage of `model` with its thetas applied
    (entry 0 is N), and, last, how many pass every stage -- per-stage survival of a pool."""
    T = len(model)
    N = sample_count(model, X)
    if N == 0:
        return np.zeros(T + 1, np.int64)
    return trace_launch(model, X, True, alive=True)[2].cpu().numpy().view(np.uint32).astype(np.int64)


def expected_cost(model, X):
    """Mean number of weak classifiers evaluated per sample of X: stage_survival(model, X)[:T].sum() / N -- the
    pool-side twin of Model.eval_cost."""
    N = sample_count(model, X)
    if N == 0:
        raise ValueError("expected_cost needs at least one sample")
    return float(stage_survival(model, X)[:len(model)].sum() / N)


def keep_count(recall, n):
    """How many of n samples a recall in (0, 1] asks to keep: min(n, max(1, ceil(recall * n)))."""
    return min(n, max(1, math.ceil(recall * n)))


class Calibration:
    """What calibrate found: theta (float32 [T], the new thresholds), old_theta (the model's list before the call),
    floor (the final-score floor, a float), n (samples), retained (samples with F >= floor) and recall = retained / n."""
    __slots__ = ("theta", "old_theta", "floor", "n", "retained")

    def __init__(self, theta, old_theta, floor, n, retained):
        self.theta, self.old_theta, self.floor, self.n, self.retained = theta, old_theta, floor, n, retained

    @property
    def recall(self):
        return self.retained / self.n

    def __repr__(self):
        return (f"Calibration(stages={self.theta.size}, floor={self.floor!r}, retained={self.retained}/{self.n}, "
                f"recall={self.recall:.4f})")


def calibrate(model, positives, recall=0.99, margin=0.0, inplace=True):
    """Choose all rejection thresholds of `model` by direct backward pruning on `positives` (module docstring).

    positives : (N, m, n, C) ndarray or device tensor of any dtype compare.channel_tensor takes, or a pool (SamplePool,
        DeviceSamplePool: its get_true_positives()[0]; a device tensor stays on the device).
    recall : in (0, 1]: the share of the positives to keep; keep = min(N, max(1, ceil(recall * N))).
    margin : >= 0, subtracted from every threshold: theta[t] = float32(stage_min[t]) - float32(margin), in float32.
    inplace : store the thresholds in model.theta (all T are replaced; the old ones play no part in the calculation).
        They are Python floats holding float32 values, so engine.theta_as_f32 leaves them unchanged and a .pb round trip
        is exact.  Model.device_cascade follows the edit on the next call; a model-specialised kernel is rebuilt for the
        new thetas on the model's second scan, as for any new stage list.

    With margin 0: model.predict(positives) passes exactly the retained samples, with their unrejected scores, and
    every stage has a retained sample whose running score equals its theta.

    ValueError: recall outside (0, 1], margin negative or not finite, samples of another shape, no samples, an empty
    model, a non-finite tree prediction (a NaN running score has no place in the order) or a final score that is not
    finite.  Returns a Calibration."""
    import torch
    recall, margin = float(recall), float(margin)
    if not (0.0 < recall <= 1.0):
        raise ValueError(f"recall must lie in (0, 1], given {recall}")
    if not (math.isfinite(margin) and margin >= 0.0):
        raise ValueError(f"margin must be finite and not negative, given {margin}")
    T = len(model)
    if T == 0:
        raise ValueError("calibrate needs a model with at least one stage")
    for t, w in enumerate(model.classifier):
        if not np.isfinite(np.asarray(w.prediction)[np.asarray(w.left) < 0]).all():
            raise ValueError(f"stage {t} has a non-finite prediction: its running scores cannot be ordered")
    if hasattr(positives, "get_true_positives"):
        positives = positives.get_true_positives()[0]
    N = sample_count(model, positives)
    if N == 0:
        raise ValueError("calibrate needs at least one positive sample")
    keep = keep_count(recall, N)
    Xd, wdt, _ = _samples(model, positives)
    F = trace_launch(model, Xd, False, final=True)[1]
    floor_t = torch.sort(F, descending=True).values[keep - 1]
    floor = float(floor_t.item())
    if not math.isfinite(floor) or not bool(torch.isfinite(F).all().item()):
        raise ValueError("a final score is not finite: the running scores cannot be ordered")
    stage_min = torch.empty(T, dtype=torch.float32, device=Xd.device)
    n_ret = torch.empty(1, dtype=torch.int32, device=Xd.device)
    nat.check(nat.load().wb_calib_min_launch(nat.stream_ptr(), model.device_cascade().handle, nat.ptr(Xd), wdt, N,
                                             C.c_float(floor), nat.ptr(stage_min), nat.ptr(n_ret)), "wb_calib_min_launch")
    with np.errstate(over="ignore"):
        theta = (stage_min.cpu().numpy() - np.float32(margin)).astype(np.float32)
    res = Calibration(theta, list(model.theta), floor, N, int(n_ret.item()))
    if inplace:
        model.theta = [float(x) for x in theta]
    return res
