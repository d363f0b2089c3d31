"""Box regression: a linear map from a detection's channel window to four box offsets, fitted and applied on the GPU.

A detection's box is the window grid cell ``[c, r, c + n, r + m] / scale``: a lattice of `shrink` pixels spread over the
pyramid's scales.  The reference computes a regression target for it (``samples.get_regression_target``, reference
samples.py:152-157) that nothing consumes; this module does: a ridge regressor from the window's ``(m, n, C)`` channel
values to the offsets between the grid box and the ground-truth box it belongs to, in level pixels.

What runs where (DESIGN.md 4.15 has the rule, tests/regress_reference.py states it in NumPy):

* ``targets`` is torch element-wise arithmetic on the device: ``(float64(box) - gt[owner]) * scale[level]``;
* ``Accumulator`` holds the normal equations ``S = A^T A``, ``A = [X | 1 | T]``, in device float64 and updates them with
  ``wb_gram_launch`` (csrc/wb_regress.hip: float64 matrix instructions, a fixed chunk order, no atomics -- the same inputs
  and calls give the same bits);
* the solve is NumPy float64 on the host, once: centred moments out of ``S``, a ridge of ``l2 * trace(Cxx) / D`` on the
  slopes, none on the intercept;
* ``BoxRegressor.predict`` is ``wb_regress_predict_launch`` on crops, ``detect_and_refine`` is ``wb_regress_apply_launch`` on
  the windows where they lie in the resident pyramid -- no crop is materialised -- followed by non-maximum suppression of
  the refined boxes.
"""
import numpy as np

from . import _native as nat

_SCRATCH_BYTES = 256 << 20          # Accumulator.add feeds rows in blocks that keep the Gram scratch at or below this


def _shape3(shape):
    s = tuple(int(x) for x in shape)
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"shape must be (m, n, C), got {shape!r}")
    if s[0] * s[1] * s[2] + 5 > nat.WB_GRAM_MAX_P:
        raise NotImplementedError(f"a window of {s[0] * s[1] * s[2]} features: at most {nat.WB_GRAM_MAX_P - 5}")
    return s


def _dtype_of(dtype):
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = np.dtype(nat.dtype_name(dtype))
    if dt not in (np.float32, np.uint8):
        raise NotImplementedError(f"channel windows are float32 or uint8, got {dt}")
    return dt


def targets(mined, gt_boxes_per_image, scales):
    """Regression targets of a MinedSamples whose `image` field indexes `gt_boxes_per_image` (a list of Boxes / None), as a
    device float64 (N, 4) tensor: T = (float64(box) - gt[instance_id]) * scale[level] -- the reference's regression_target
    brought to level pixels; subtract first, then multiply, each rounded once.  `scales`: the pyramid's scales as Python
    floats (what detect_raw returns as 'scales').  Every row needs an owner: true positives have one (mine with tp=True,
    fp=False); a row with instance_id < 0 is not looked for here (that would be a host wait) and gets a meaningless target."""
    import torch
    from .samples import _ground_truth_arrays
    dev = mined.boxes.device
    gt, gt_off, _ = _ground_truth_arrays(list(gt_boxes_per_image))
    if len(mined) == 0:
        return torch.empty((0, 4), dtype=torch.float64, device=dev)
    if gt.shape[0] == 0:
        raise ValueError("targets: no ground-truth boxes")
    gt_d = torch.from_numpy(np.ascontiguousarray(gt, np.float64)).to(dev)
    off_d = torch.from_numpy(gt_off[:-1].astype(np.int64)).to(dev)
    sc_d = torch.from_numpy(np.asarray([float(s) for s in scales], np.float64)).to(dev)
    owner = off_d[mined.image.to(torch.int64)] + mined.instance_id.to(torch.int64).clamp_(min=0)
    diff = mined.boxes.to(torch.float64) - gt_d[owner.clamp_(max=gt.shape[0] - 1)]
    return diff * sc_d[mined.level.to(torch.int64)].unsqueeze(1)


class BoxRegressor:
    """pred = W^T x + b for windows of `input_shape` = (m, n, C): the offsets, in level pixels, between a window's grid box
    and the box it should be; the refined box is float32(float64(box) - pred / scale).  W float64 (D, 4), b float64 (4,);
    n_samples, l2, and the training residual / total sums of squares per coordinate (rss, tss) as the fit left them; dtype:
    the channel dtype it was fitted on (None: not recorded -- any is taken)."""

    def __init__(self, input_shape, W, b, n_samples=0, l2=0.0, rss=None, tss=None, dtype=None):
        self.input_shape = _shape3(input_shape)
        D = int(np.prod(self.input_shape))
        self.W = np.array(W, np.float64).reshape(D, 4)
        self.b = np.array(b, np.float64).reshape(4)
        if not (np.isfinite(self.W).all() and np.isfinite(self.b).all()):
            raise ValueError("the weights hold non-finite values")
        self.n_samples, self.l2 = int(n_samples), float(l2)
        self.rss = np.full(4, np.nan) if rss is None else np.array(rss, np.float64).reshape(4)
        self.tss = np.full(4, np.nan) if tss is None else np.array(tss, np.float64).reshape(4)
        self.dtype = None if dtype is None else _dtype_of(dtype)
        self._device = {}

    @staticmethod
    def from_state(input_shape, S, l2=1e-2, dtype=None):
        """Solve an accumulator's state (Accumulator.state()) -- another l2 needs no second pass over the images.
        mu = X^T 1 / N, tau = T^T 1 / N, Cxx = X^T X - N mu mu^T, Cxt = X^T T - N mu tau^T,
        W = solve(Cxx + l2 * (trace(Cxx) / D) * I, Cxt), b = tau - W^T mu.  N < 2, a non-finite S or trace(Cxx) == 0:
        ValueError."""
        shape = _shape3(input_shape)
        D = int(np.prod(shape))
        S = np.asarray(S, np.float64)
        if S.shape != (D + 5, D + 5):
            raise ValueError(f"the state of a {shape} accumulator is {(D + 5, D + 5)}, got {S.shape}")
        if not np.isfinite(S).all():
            raise ValueError("the accumulator holds non-finite values")
        if not (np.isfinite(l2) and l2 >= 0):
            raise ValueError(f"l2 must be finite and not negative, got {l2!r}")
        N = S[D, D]
        if N < 2:
            raise ValueError(f"{N:g} samples: at least 2 are needed")
        mu, tau = S[:D, D] / N, S[D + 1:, D] / N
        Cxx = S[:D, :D] - N * np.outer(mu, mu)
        Cxt = S[:D, D + 1:] - N * np.outer(mu, tau)
        Ctt = S[D + 1:, D + 1:] - N * np.outer(tau, tau)
        tr = np.trace(Cxx)
        if not tr > 0:
            raise ValueError("trace(Cxx) == 0: the features do not vary")
        try:
            W = np.linalg.solve(Cxx + float(l2) * (tr / D) * np.eye(D), Cxt)
        except np.linalg.LinAlgError as e:
            raise ValueError(f"the normal equations are singular (l2 = {l2!r}): {e}") from None
        b = tau - W.T @ mu
        tss = np.diag(Ctt).copy()
        rss = tss - 2.0 * np.einsum("jk,jk->k", W, Cxt) + np.einsum("jk,jl,lk->k", W, Cxx, W)
        return BoxRegressor(shape, W, b, n_samples=int(round(N)), l2=l2, rss=rss, tss=tss, dtype=dtype)

    # ---- files
    def save(self, filename):
        """.npz, no pickle."""
        np.savez(filename, input_shape=np.array(self.input_shape, np.int64), W=self.W, b=self.b, n_samples=np.int64(self.n_samples),
                 l2=np.float64(self.l2), rss=self.rss, tss=self.tss, dtype=np.array("" if self.dtype is None else self.dtype.name))

    @staticmethod
    def load(filename):
        with np.load(filename, allow_pickle=False) as z:
            return BoxRegressor(tuple(int(x) for x in z["input_shape"]), z["W"], z["b"], int(z["n_samples"]), float(z["l2"]), z["rss"],
                                z["tss"], str(z["dtype"]) or None)

    # ---- inference
    def weights_on(self, dev):
        """[W; b] as a device float64 (D + 1, 4) tensor, uploaded once per device."""
        import torch
        if dev.index not in self._device:
            self._device[dev.index] = torch.from_numpy(np.concatenate([self.W, self.b[None]])).to(dev)
        return self._device[dev.index]

    def predict_device(self, X):
        """The offsets of crops X (N, m, n, C), float32 or uint8, ndarray or device tensor, as a device float64 (N, 4) tensor
        (wb_regress_predict_launch).  No host synchronisation when X is a device tensor."""
        import torch
        if not nat.is_tensor(X):
            X = np.asarray(X)
        if len(X.shape) != 4 or tuple(int(x) for x in X.shape[1:]) != self.input_shape:
            raise ValueError(f"crops of shape {tuple(X.shape)}, expected (N,) + {self.input_shape}")
        _dtype_of(X.dtype)                                  # (refuses another dtype before a GPU is asked for)
        dev = nat.require_gpu()
        Xd, wdt = nat.window_tensor(X, dev)
        N = int(Xd.shape[0])
        m, n, Cc = self.input_shape
        out = torch.empty((N, 4), dtype=torch.float64, device=dev)
        nat.launch("wb_regress_predict_launch", Xd, wdt, N, m, n, Cc, self.weights_on(dev), out)
        return out

    def predict(self, X):
        """predict_device, as a float64 ndarray (N, 4)."""
        return self.predict_device(X).cpu().numpy()


class Accumulator:
    """The normal equations of a box regressor for windows of `shape` = (m, n, C) and channel `dtype` (float32 / uint8), on
    the device: S = A^T A, A = [X | 1 | T], float64 (D + 5, D + 5) -- X^T X, the column sums, X^T T, T^T T and N.  It is
    summed over as many batches as the caller feeds; the result depends on the inputs and the order of the calls alone."""

    def __init__(self, shape, dtype=np.float32):
        import torch
        self.shape = _shape3(shape)
        self.dtype = _dtype_of(dtype)
        self.D = int(np.prod(self.shape))
        self.dev = nat.require_gpu()
        self.S = torch.zeros((self.D + 5, self.D + 5), dtype=torch.float64, device=self.dev)
        self.n = 0
        self._scratch = nat.Scratch()
        # rows per launch: whole chunks, the scratch bounded
        per_chunk = nat.query("wb_gram_scratch_bytes", nat.WB_GRAM_CHUNK, self.D)
        self._rows = max(_SCRATCH_BYTES // per_chunk, 1) * nat.WB_GRAM_CHUNK

    def add(self, X, T):
        """S += A^T A of device tensors X (N, m, n, C) in the accumulator's dtype and T (N, 4) float64.  No host wait."""
        import torch
        if not (nat.is_tensor(X) and nat.is_tensor(T)):
            raise TypeError("Accumulator.add takes device tensors")
        if len(X.shape) != 4 or tuple(int(x) for x in X.shape[1:]) != self.shape:
            raise ValueError(f"windows of shape {tuple(X.shape)}, expected (N,) + {self.shape}")
        if _dtype_of(X.dtype) != self.dtype:
            raise ValueError(f"windows of {_dtype_of(X.dtype)}, the accumulator takes {self.dtype}")
        N = int(X.shape[0])
        if tuple(T.shape) != (N, 4) or T.dtype != torch.float64:
            raise ValueError(f"targets of shape {tuple(T.shape)} and {T.dtype}, expected ({N}, 4) float64")
        if N == 0:
            return
        (X, wdt), T = nat.window_tensor(X, self.dev), T.to(self.dev).contiguous()
        for at in range(0, N, self._rows):
            k = min(self._rows, N - at)
            scratch = self._scratch.on(self.dev, nat.query("wb_gram_scratch_bytes", k, self.D))
            nat.launch("wb_gram_launch", X[at:], wdt, T[at:], k, self.D, self.S, scratch, scratch.numel())
        self.n += N

    def add_mined(self, mined, gt_boxes_per_image, scales):
        """add(mined.samples, targets(mined, ...)) of a MinedSamples of true positives."""
        self.add(mined.samples, targets(mined, gt_boxes_per_image, scales))

    def state(self):
        """S as a host float64 array (one download)."""
        return self.S.cpu().numpy()

    def solve(self, l2=1e-2):
        return BoxRegressor.from_state(self.shape, self.state(), l2, dtype=self.dtype)


def fit(model, images, min_iou=0.5, max_candidates=100, l2=1e-2, batch=8, seed=0, accumulator=None):
    """A BoxRegressor for `model`'s detections from `images`, what train takes: an iterable of dicts with 'image' and
    'groundtruth_boxes'.  Consecutive images of one shape and dtype go `batch` at a time (samples.image_batches) through
    samples.mine_batch(tp=True, fp=False, min_tp_iou=min_iou, max_tp_candidates=max_candidates, seed=seed, serial0=the
    images before the batch): the true-positive windows of the model's detections, at most max_candidates per (image,
    level).  Their targets are computed and the Gram update is launched on the device, with no host wait beyond
    mine_batch's own; S comes down once at the end and is solved on the host.  An empty model detects every window.
    accumulator: sum into this one (the caller's: its solve(l2) gives another ridge without a second pass over the
    images).  No positive window at all: ValueError."""
    from . import channels as _channels
    from . import engine as _engine
    from . import samples as _samples
    shrink, n_per_oct, smooth, spec = _channels.read_opts(model.channel_opts)
    acc = accumulator if accumulator is not None else Accumulator(model.shape, spec.dtype)
    if acc.shape != tuple(int(x) for x in model.shape) or acc.dtype != np.dtype(spec.dtype):
        raise ValueError(f"the accumulator is for {acc.shape} {acc.dtype} windows, the model has {tuple(model.shape)} {np.dtype(spec.dtype)}")
    seen = 0
    for group in _samples.image_batches(images, max(int(batch), 1)):
        stack = _samples.stack_images(group)
        gts = [it["groundtruth_boxes"] for it in group]
        mined = _samples.mine_batch(model, stack, gts, tp=True, fp=False, min_tp_iou=min_iou, max_tp_candidates=max_candidates,
                                    seed=seed, serial0=seen)
        seen += len(group)
        if len(mined) == 0:
            continue
        B, H, W = (int(x) for x in stack.shape)
        eng = _engine.get_engine(H, W, _engine.array_dtype(stack), shrink, n_per_oct, smooth, B, channels=spec)
        acc.add_mined(mined, gts, eng.plan.scales)
    if acc.n == 0:
        raise ValueError("fit: no window of the model's detections overlaps a ground-truth box by more than min_iou")
    return acc.solve(l2)


def detect_and_refine(image, model, regressor, iou_threshold=None, score_threshold=None, vote_iou=None, vote_weights="uniform", min_votes=1):
    """Detections of `model` on `image` with their boxes refined by `regressor`: Boxes with 'scores', in Model.detect's
    order (levels in pyramid order, row-major inside a level).  The scan is Model.scan_resident (float or uint8 channels, not
    rank bytes); the scan's records go up in one upload (the level table | the records | 1 / scale in float64 | in float32)
    and wb_regress_apply_launch reads every window where it lies in the resident pyramid.  Scores are untouched.
    iou_threshold / score_threshold: non-maximum suppression (non_max_suppression's semantics) AFTER refinement, on the
    refined boxes (boxes.finish: one more upload and read-back).  Without them two host waits: the scan's read-back and the
    refined boxes with the error word, out of one block.  n_loc / n_weak advance as in a scan.
    vote_iou (needs an iou_threshold), vote_weights, min_votes: box voting on the REFINED boxes -- boxes.merge_detections of
    the complete refined result with these thresholds: every kept box becomes the mean of its cluster and gets a 'votes'
    field, kept boxes with fewer than min_votes voters are left out.  That is one more device round trip after the refined
    boxes' read-back, the same one that suppression alone makes.  None: exactly the call without it."""
    from . import channels as _channels
    from .boxes import Boxes, finish, suppression
    from .samples import level_table
    how = suppression(iou_threshold, score_threshold, vote_iou, vote_weights, min_votes)
    if not isinstance(regressor, BoxRegressor):
        raise TypeError(f"detect_and_refine takes a BoxRegressor, got {type(regressor).__name__}")
    if tuple(int(x) for x in model.shape) != regressor.input_shape:
        raise ValueError(f"the model's window shape {tuple(model.shape)} is not the regressor's input_shape {regressor.input_shape}")
    chn_dtype = np.dtype(_channels.read_opts(model.channel_opts)[3].dtype)
    if regressor.dtype is not None and regressor.dtype != chn_dtype:
        raise ValueError(f"the regressor was fitted on {regressor.dtype} channels, the model's are {chn_dtype}")
    scanned = model.scan_resident(image)                    # wait 1: detections, in (level, r, c) order
    if scanned is None or scanned[1]["scores"].size == 0:
        return finish(Boxes(np.zeros((0, 4), np.float32), scores=np.zeros(0, np.float32)), how)
    eng, found = scanned
    N = int(found["scores"].size)
    dev = nat.require_gpu()
    m, n, Cc = regressor.input_shape
    det = np.zeros(N, nat.DET_DTYPE)
    det["level"], det["r"], det["c"], det["score"] = found["level"], found["r"], found["c"], found["scores"]
    inp = nat.Block.upload(dev, table=level_table(eng), det=det, inv64=np.array([1.0 / float(s) for s in eng.plan.scales], np.float64),
                           inv_scale=np.ascontiguousarray(eng.inv_scales(), np.float32))
    out = nat.Block.empty(dev, boxes=((N, 4), np.float32), err=(1, np.int32))
    out.tensor("err").zero_()
    nat.launch("wb_regress_apply_launch", eng.chn, eng.spec.wb_dtype, eng.chn_stride, 1, inp.ptr["table"], eng.plan.n_levels, Cc,
               inp.ptr["det"], N, m, n, regressor.weights_on(dev), inp.ptr["inv_scale"], inp.ptr["inv64"], None, out.ptr["boxes"],
               out.ptr["err"])
    host = out.host()                                       # wait 2
    if int(host["err"][0]):
        raise RuntimeError("detect_and_refine: a detection's window lies outside its pyramid level")
    return finish(Boxes(host["boxes"].copy(), scores=np.ascontiguousarray(found["scores"], np.float32)), how)
