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

prune_instances is the paper's other half, multiple-instance pruning over whole images: every ground-truth box owns a bag of
acceptable windows (instance_windows) and only one window of a bag has to survive, so the thetas are never below backward
pruning's on the same windows (csrc/wb_mip.hip: wb_mip_windows_launch, wb_mip_prune_launch; DESIGN.md 4.14;
tests/mip_reference.py is the NumPy statement).
"""
import ctypes as C
import math

import numpy as np

from . import _native as nat
from .compare import channel_tensor
from .samples import LabelledBatch, _empty_mined, image_batches, stack_images


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
    nat.launch("wb_samples_trace_launch", dm.handle, Xd, wdt, N, int(bool(reject)), *out)
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


def _check_operating_point(recall, margin):
    if not (0.0 < recall <= 1.0):
        raise ValueError(f"recall must lie in (0, 1], given {recall}")
    if not (math.isfinite(margin) and margin >= 0.0):
        raise ValueError(f"margin must be finite and not negative, given {margin}")


def _check_predictions(model):
    for t, w in enumerate(model.classifier):
        if not np.isfinite(np.asarray(w.prediction)[np.asarray(w.left) < 0]).all():
            raise ValueError(f"stage {t} has a non-finite prediction: its running scores cannot be ordered")


def _lowered(values, margin):
    """float32(values) - float32(margin), in float32."""
    with np.errstate(over="ignore"):
        return (np.asarray(values, np.float32) - np.float32(margin)).astype(np.float32)


def _new_thetas(model, values, margin, inplace):
    """(theta, old_theta): the stage values read back from the device lowered by the margin, and the model's list before
    the call; inplace: the thetas stored in model.theta as Python floats holding float32 values."""
    theta, old = _lowered(values, margin), list(model.theta)
    if inplace:
        model.theta = [float(x) for x in theta]
    return theta, old


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
    _check_operating_point(recall, margin)
    T = len(model)
    if T == 0:
        raise ValueError("calibrate needs a model with at least one stage")
    _check_predictions(model)
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
    nat.launch("wb_calib_min_launch", model.device_cascade().handle, Xd, wdt, N, C.c_float(floor), stage_min, n_ret)
    theta, old = _new_thetas(model, stage_min.cpu().numpy(), margin, inplace)
    return Calibration(theta, old, floor, N, int(n_ret.item()))


# --------------------------------------------------------------------------------------- multiple-instance pruning
def _gt_pairs(flat, gt_off):
    """Flat ground-truth indices of a batch as int64 [K, 2] rows (image, index inside the image's list)."""
    flat = np.asarray(flat, np.int64).reshape(-1)
    image = np.searchsorted(gt_off.astype(np.int64), flat, side="right") - 1
    return np.stack([image, flat - gt_off[image]], axis=1).astype(np.int64).reshape(-1, 2)


def instance_windows(model, images, gt_boxes_per_image, min_iou=0.7):
    """The ACCEPTABLE windows of a batch `images` [B, H, W] (or one [H, W]) for the ground truth of every image (a list
    of B Boxes / None; for one image the Boxes itself), cropped out of the pyramid -- no scan: the thetas play no part.

    The windows of pyramid level l (u x v channels, window m x n) are those the scan visits, r in [0, u - m), c in
    [0, v - n); the box of a window is float32 [c, r, c+n, r+m] * float32(1 / scale[l]); best and owner are mine_batch's
    (boxes.iou's float64 arithmetic, the first argmax).  A window is acceptable when its image has ground truth, best >
    min_iou (strict) and the owner's 'ignore' flag is 0 -- label_boxes' TP rule without caps -- and belongs to the bag
    of its owner only (wb_mip_windows_launch; the crops are wb_mine_gather_launch's).

    Returns (mined, bag, reachable, unreachable): mined a MinedSamples of the acceptable windows in (image, level, row,
    col) order (scores 0, tp_label 1, instance_id the owner); bag a device int32 tensor, the bag of every row = the
    position of its (image, owner) in reachable; reachable / unreachable int64 ndarrays [K, 2] of (image, index in the
    image's list) in that order: the non-ignored ground-truth boxes that own an acceptable window, and those that own
    none (no window of the pyramid overlaps them enough: they are reported, and are no bag).

    Host traffic: two uploads (ground truth, offsets, flags, level table and 1 / scale in one; the images' first flat
    ground-truth indices for the bags), two waits (the number of rows; the gather's error word with the bags'
    ground-truth indices), a third and a second labelling launch when more than 4096 windows per image are acceptable."""
    import torch
    min_iou = float(min_iou)
    if not (0.0 <= min_iou < 1.0):
        raise ValueError(f"min_iou must lie in [0, 1), given {min_iou}")
    b = LabelledBatch(model, images, gt_boxes_per_image, "instance_windows")
    B, L, dev, gt_off = b.B, b.L, b.dev, b.gt_off
    open_gt = np.flatnonzero(b.ignore == 0)
    none = np.zeros((0, 2), np.int64)
    empty = lambda: (_empty_mined(model.shape, b.eng.chn.dtype, dev), torch.empty(0, dtype=torch.int32, device=dev), none,
                     _gt_pairs(open_gt, gt_off))
    if L == 0 or b.gt.shape[0] == 0:
        return empty()
    b.run_channels()
    b.upload()
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    room = 4096 * B
    while True:
        rows = torch.empty((room, 8), dtype=torch.int32, device=dev)
        nat.launch("wb_mip_windows_launch", b.table.ctypes.data_as(C.c_void_p), b.inv.ctypes.data_as(C.c_void_p), L, b.m, b.n, b.ptr["gt"],
                   b.ptr["gt_off"], b.ptr["ignore"], b.gt.shape[0], B, min_iou, rows, room, n_rows)
        N = int(n_rows.item()) & 0xFFFFFFFF
        if N <= room:
            break
        room = N                                           # the full count: the second call has room for all
    if N == 0:
        return empty()
    mined, err = b.mined(rows[:N])
    # bags: the distinct flat ground-truth indices that own a row, in ascending order = (image, index) order
    off_dev = torch.from_numpy(gt_off[:-1].astype(np.int64)).to(dev)
    flat = off_dev[mined.image.to(torch.int64)] + mined.instance_id.to(torch.int64)
    owners, bag = torch.unique(flat, return_inverse=True)
    h = torch.cat([err.to(torch.int64), owners]).cpu().numpy()            # one wait: the error word and the owners
    if int(h[0]):
        raise RuntimeError("instance_windows: a window lies outside its pyramid level")
    return mined, bag.to(torch.int32), _gt_pairs(h[1:], gt_off), _gt_pairs(np.setdiff1d(open_gt, h[1:]), gt_off)


class InstancePruning:
    """What prune_instances found: theta (float32 [T], the new thresholds), old_theta (the model's list before the
    call), floor (the final-score floor, a float), n_bags (reachable ground-truth boxes), retained (bags with a window at
    or above the floor: each keeps a window through every stage), recall = retained / n_bags, unreachable (int64 [K, 2]:
    (position of the image in the iterable, index in its list) of the non-ignored boxes no window reaches), n_windows
    (acceptable windows) and surviving (those that pass every stage)."""
    __slots__ = ("theta", "old_theta", "floor", "n_bags", "retained", "unreachable", "n_windows", "surviving")

    def __init__(self, theta, old_theta, floor, n_bags, retained, unreachable, n_windows, surviving):
        self.theta, self.old_theta, self.floor, self.n_bags, self.retained = theta, old_theta, floor, n_bags, retained
        self.unreachable, self.n_windows, self.surviving = unreachable, n_windows, surviving

    @property
    def recall(self):
        return self.retained / self.n_bags

    def __repr__(self):
        return (f"InstancePruning(stages={self.theta.size}, floor={self.floor!r}, retained={self.retained}/{self.n_bags} bags, "
                f"recall={self.recall:.4f}, unreachable={len(self.unreachable)}, surviving={self.surviving}/{self.n_windows} windows)")


def _ordered_ints(F):
    """int32 values whose signed order is the float order of the float32 tensor F (-0 below +0): wb_f32_key's order."""
    import torch
    b = F.contiguous().view(torch.int32)
    return torch.where(b < 0, b ^ 0x7FFFFFFF, b)


def bag_floor(F, bag, n_bags, recall):
    """The floor of prune_instances on the device: (floor as a one-element float32 tensor, keep) -- the keep-th largest of
    the bags' maxima of F (device float32 [N], N >= 1; bag: device int [N] in [0, n_bags)), keep = keep_count(recall, bags
    that have a window).  One sort of (bag, ordered integer of F) pairs, so the sign of a zero is settled as in the kernels;
    the last pair of every bag is its maximum.  One wait (the number of bags that have windows)."""
    import torch
    pair = (bag.to(torch.int64) << 32) | (_ordered_ints(F).to(torch.int64) + 2 ** 31)
    pair = torch.sort(pair).values
    last = torch.ones_like(pair, dtype=torch.bool)
    last[:-1] = (pair[1:] >> 32) != (pair[:-1] >> 32)
    G = ((pair[last] & 0xFFFFFFFF) - 2 ** 31).to(torch.int32)
    keep = keep_count(recall, int(G.numel()))
    g = torch.sort(G, descending=True).values[keep - 1:keep]
    return torch.where(g < 0, g ^ 0x7FFFFFFF, g).view(torch.float32), keep


def prune_launch(trace, bag, n_bags, floor):
    """wb_mip_prune_launch on a device trace [T, N] (stage-major, contiguous rows) -> (theta float32 [T], removed_at int32
    [N], counts int32 [2]) as device tensors."""
    import torch
    T, N = (int(x) for x in trace.shape)
    assert N <= 1 or trace.stride(1) == 1, "the rows of the trace must be contiguous"
    dev = trace.device
    scratch = torch.empty(max(nat.query("wb_mip_scratch_bytes", n_bags), 4), dtype=torch.uint8, device=dev)
    theta = torch.empty(T, dtype=torch.float32, device=dev)
    removed_at = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    nat.launch("wb_mip_prune_launch", trace, int(trace.stride(0)) if T > 1 else N, T, N, bag, n_bags, C.c_float(floor), scratch,
               scratch.numel(), theta, removed_at, counts)
    return theta, removed_at, counts


def prune_trace(trace, bag, n_bags, recall, margin=0.0):
    """The floor and the prune of prune_instances on a device trace [T, N] (unrejected, stage-major) with the bag of every
    window (device int32 [N] in [0, n_bags), every bag with a window): (theta float32 ndarray [T], floor, retained bags,
    surviving windows, removed_at device int32 [N]).  Two waits: the floor with the finiteness of the final scores; the
    thetas with the counts.  ValueError for a final score that is not finite."""
    import torch
    T = int(trace.shape[0])
    floor_t, _ = bag_floor(trace[T - 1], bag, n_bags, recall)
    finite = torch.isfinite(trace[T - 1]).all()
    h = torch.cat([floor_t.view(torch.int32), finite.to(torch.int32).reshape(1)]).cpu().numpy()
    floor = float(h[:1].view(np.float32)[0])
    if not (h[1] and math.isfinite(floor)):
        raise ValueError("a final score is not finite: the running scores cannot be ordered")
    theta_t, removed_at, counts = prune_launch(trace, bag, n_bags, floor)
    h = torch.cat([theta_t.view(torch.int32), counts]).cpu().numpy()
    return _lowered(h[:T].view(np.float32), margin), floor, int(h[T]), int(h[T + 1]), removed_at


def prune_instances(model, images, recall=0.99, margin=0.0, min_iou=0.7, batch=8, inplace=True):
    """Choose all rejection thresholds of `model` by multiple-instance pruning (Zhang & Viola 2007) over whole images.

    images : an iterable of dicts with 'image' and 'groundtruth_boxes', as train takes it; `batch` images of equal shape
        and dtype go through one pyramid (samples.image_batches).
    Every non-ignored ground-truth box owns a BAG: the acceptable windows it owns (instance_windows: best IoU > min_iou,
    the box the first argmax).  Only one window of a bag has to survive:

      * F[i] is the unrejected final score of window i, G[k] the largest F of bag k; keep = keep_count(recall, n_bags);
        floor is the keep-th largest G; a window is retained at the start when F[i] >= floor, a bag when it has such a
        window (ties at the floor are all kept);
      * for t = 0 .. T - 1, in order: theta[t] is the minimum, over the bags with a retained window, of the maximum of
        the running score after stage t over the bag's retained windows; then every window with `not (score >= theta[t])`
        stops being retained.

    So every retained bag keeps at least one window through all T stages, with its unrejected score, which is at least
    floor; and no theta is below what calibrate(recall=1.0) gives on the windows retained at the start, so no sample set
    costs more under these thresholds than under those.  margin (>= 0) is subtracted from every theta in float32, as in
    calibrate, after the prune (which works with the unlowered values).  Maxima and minima are taken on wb_f32_key keys.

    Per batch: the windows (wb_mip_windows_launch), their crops, their trace (wb_samples_trace_launch, reject = 0); only
    the traces [T][N_b] and the bags are kept.  Then one floor selection on the device and one wb_mip_prune_launch.
    The thresholds are stored in model.theta as Python floats holding float32 values (inplace).

    ValueError: recall outside (0, 1], margin negative or not finite, min_iou outside [0, 1), an empty model, a
    non-finite tree prediction or final score, no reachable ground truth, N * T >= 2**31.  Returns an InstancePruning."""
    import torch
    recall, margin, min_iou = float(recall), float(margin), float(min_iou)
    _check_operating_point(recall, margin)
    if not (0.0 <= min_iou < 1.0):
        raise ValueError(f"min_iou must lie in [0, 1), given {min_iou}")
    T = len(model)
    if T == 0:
        raise ValueError("prune_instances needs a model with at least one stage")
    _check_predictions(model)
    batch = max(int(batch), 1)
    traces, bags, unreachable = [], [], []
    state = dict(n_bags=0, n_images=0, n_windows=0)

    def flush(group):
        mined, bag, reach, unreach = instance_windows(model, stack_images(group), [it["groundtruth_boxes"] for it in group],
                                                      min_iou=min_iou)
        if len(unreach):
            unreachable.append(unreach + np.array([state["n_images"], 0]))
        state["n_images"] += len(group)
        if len(mined):
            state["n_windows"] += len(mined)
            if state["n_windows"] * T >= 2 ** 31:
                raise ValueError(f"a trace of {state['n_windows']} windows x {T} stages has 2**31 entries or more: use fewer images")
            traces.append(trace_launch(model, mined.samples, False, trace=True)[0])          # the crops are dropped here
            bags.append(bag + state["n_bags"])
            state["n_bags"] += len(reach)

    for group in image_batches(images, batch):
        flush(group)
    n_bags, N = state["n_bags"], state["n_windows"]
    unreachable = np.concatenate(unreachable) if unreachable else np.zeros((0, 2), np.int64)
    if n_bags == 0:
        raise ValueError("prune_instances: no ground-truth box is reachable (no window of any pyramid overlaps one enough)")
    trace = traces[0] if len(traces) == 1 else torch.cat(traces, dim=1).contiguous()
    bag = bags[0] if len(bags) == 1 else torch.cat(bags)
    stage_theta, floor, retained, surviving, _ = prune_trace(trace, bag, n_bags, recall)     # margin 0: the unlowered values
    theta, old = _new_thetas(model, stage_theta, margin, inplace)                             # (x - 0.0f is x, bit for bit)
    return InstancePruning(theta, old, floor, n_bags, retained, unreachable, N, surviving)
