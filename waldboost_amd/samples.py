"""Samples from images -- drop-in for the detection-side part of ``waldboost.samples``: the training
pipeline's hard-negative mining runs the hot path over every training image, labels the surviving
windows against the ground truth and crops them out of the channel pyramid.

What runs where:

* ``gather_samples`` (reference samples.py:14-43) is a HIP copy kernel (``wb_gather_samples_launch``);
* ``get_samples_from_image`` (reference samples.py:160-216) keeps the channel pyramid on the GPU between
  the cascade scan and the crop -- only detections and the selected crops travel to the host;
* ``label_boxes`` / ``select_candidates`` / ``SampleLabel`` (reference samples.py:46-157) are small NumPy
  host steps with the reference's semantics (TP: best IoU above ``min_tp_iou`` on a non-ignored box; FP:
  best IoU below ``max_fp_iou``; at most ``max_*_candidates`` of each per call, drawn with
  ``np.random.choice``), ``bbx.iou`` replaced by ``boxes.iou``;
* ``SamplePool`` (reference samples.py:219-338) re-scores its samples with ``Model.predict`` on the GPU;
* ``mine_batch`` / ``DeviceSamplePool`` are the batched, device-resident form of the same step: several images per
  scan, labelling, choice and crops in two native calls (``wb_mine_select_launch``, ``wb_mine_gather_launch``), the
  pool's samples in GPU memory.  They state their own selection rule (``mine_batch`` has it).
"""
import logging

import numpy as np

from . import _native as nat
from .boxes import Boxes, concatenate, iou


# --------------------------------------------------------------------------------------- crops
def _np_dtype(chns):
    return np.dtype(nat.dtype_name(chns))


def gather_samples_device(chns, rs, cs, shape):
    """Crops of `shape` = (m, n, C) at the origins (rs[i], cs[i]) of the channel image `chns`
    (ndarray or device tensor, float32 / uint8) as a device tensor (N, m, n, C)."""
    import torch
    dev = nat.require_gpu()
    if nat.window_codes(chns) is None:
        raise TypeError(f"channel image must be float32 or uint8 (as produced by channel_pyramid), got {_np_dtype(chns)}")
    u, v, C = (int(x) for x in chns.shape)
    m, n = int(shape[0]), int(shape[1])
    rows = np.asarray(rs).reshape(-1).astype(np.int64)
    cols = np.asarray(cs).reshape(-1).astype(np.int64)
    if rows.size and (rows.min() < 0 or cols.min() < 0 or rows.max() + m > u or cols.max() + n > v):
        # the reference slices without range checks and would build a ragged object array here
        raise IndexError("sample window outside the channel image")
    src, wdt = nat.window_tensor(chns, dev)
    pos = torch.from_numpy(np.stack([rows, cols]).astype(np.int32)).to(dev)
    out = torch.empty((rows.size, m, n, C), dtype=src.dtype, device=dev)
    nat.launch("wb_gather_samples_launch", src, wdt, u, v, C, pos[0], pos[1], rows.size, m, n, out)
    return out


def gather_samples(chns, rs, cs, shape) -> np.ndarray:
    """X[i] = chns[rs[i]:rs[i]+m, cs[i]:cs[i]+n, :] -> (N, m, n, C) in the dtype of `chns`."""
    n_r, n_c = np.asarray(rs).size, np.asarray(cs).size
    if n_r != n_c:
        raise ValueError("Sizes of 'rs' and 'cs' must match")
    if n_r == 0:
        return np.empty((0,) + tuple(shape), dtype=_np_dtype(chns))
    return gather_samples_device(chns, rs, cs, shape).cpu().numpy()


# --------------------------------------------------------------------------------------- labels
class SampleLabel:
    TRUE_POSITIVE = 1
    FALSE_POSITIVE = -1
    IGNORE = 0


def select_candidates(condition, max_candidates: int) -> np.ndarray:
    """Indices of True entries, thinned to `max_candidates` by ``np.random.choice`` when there are more."""
    hits = np.flatnonzero(condition)
    return hits if hits.size <= max_candidates else np.random.choice(hits, max_candidates)


def _match_ground_truth(dt_boxes, gt_boxes):
    """(best IoU, index of the best ground-truth box, its ignore flag) for every detection."""
    flags = gt_boxes.get_field("ignore") if gt_boxes.has_field("ignore") else np.zeros(len(gt_boxes))
    if flags.ndim != 1:
        raise ValueError("'ignore' field must be single dimension")
    table = iou(dt_boxes, gt_boxes)
    best = table.argmax(axis=1)
    return table[np.arange(table.shape[0]), best], best, flags[best]


def label_boxes(dt_boxes, gt_boxes, min_tp_iou: float = 0.7, max_fp_iou: float = 0.3,
                max_tp_candidates: int = 100, max_fp_candidates: int = 100):
    """Adds the fields 'tp_label' (SampleLabel per box) and 'instance_id' (best ground-truth box, -1
    without ground truth) to `dt_boxes`, in place."""
    if dt_boxes is None:
        return
    n = len(dt_boxes)
    labels = np.full(n, SampleLabel.IGNORE, np.int32)
    if gt_boxes is None or len(gt_boxes) == 0:
        owner = np.full(n, -1, np.int32)
        labels[select_candidates(np.ones(n, bool), max_fp_candidates)] = SampleLabel.FALSE_POSITIVE
    else:
        overlap, owner, ignored = _match_ground_truth(dt_boxes, gt_boxes)
        negatives = select_candidates(overlap < max_fp_iou, max_fp_candidates)
        positives = select_candidates((overlap > min_tp_iou) & (ignored == 0), max_tp_candidates)
        labels[positives] = SampleLabel.TRUE_POSITIVE
        labels[negatives] = SampleLabel.FALSE_POSITIVE          # written last, as in the reference
    dt_boxes.set_field("instance_id", owner)
    dt_boxes.set_field("tp_label", labels)


def get_regression_target(dt_boxes, gt_boxes):
    """Box offsets of labelled detections to the ground truth they belong to, as field
    'regression_target' (reference samples.py:152-157; host arithmetic on a handful of boxes)."""
    if not dt_boxes.has_field("instance_id"):
        raise ValueError("'instance_id' field is missing")
    owner = dt_boxes.get_field("instance_id")
    dt_boxes.add_field("regression_target", dt_boxes.get() - gt_boxes[owner].get())


# --------------------------------------------------------------------------------------- mining
def get_samples_from_image(model, image, gt_boxes, tp=True, fp=True, **kwargs):
    """Generator over the pyramid levels that hold selected detections of `model` on `image`: Boxes
    with 'scores', 'row', 'col', 'instance_id', 'tp_label' and 'samples' (their (m, n, C) crops)."""
    scanned = model.scan_resident(image)
    if scanned is None:
        return
    eng, found = scanned
    wanted = []
    if tp:
        wanted.append(SampleLabel.TRUE_POSITIVE)
    if fp:
        wanted.append(SampleLabel.FALSE_POSITIVE)
    level_of = found["level"]
    for lv in np.unique(level_of):
        idx = np.flatnonzero(level_of == lv)
        boxes = Boxes(found["boxes"][idx], scores=found["scores"][idx], row=found["r"][idx], col=found["c"][idx])
        label_boxes(boxes, gt_boxes, **kwargs)
        keep = np.flatnonzero(np.isin(boxes.get_field("tp_label"), wanted))
        if keep.size == 0:
            continue
        boxes = boxes[keep]
        crops = gather_samples_device(eng.level_tensor(0, int(lv)), boxes.get_field("row"), boxes.get_field("col"),
                                      model.shape)
        boxes.set_field("samples", crops.cpu().numpy())
        yield boxes


class SamplePool(object):
    """Pool of labelled training samples that is topped up from images and re-scored as the model grows."""

    def __init__(self, min_tp=1000, min_fp=1000, logger=None, **kwargs):
        self.samples = None
        self.min_tp, self.min_fp = min_tp, min_fp
        self.label_boxes_args = kwargs
        self.logger = logger or logging.getLogger("SamplePool")

    def _count(self, label):
        return 0 if self.samples is None else int((self.samples.get_field("tp_label") == label).sum())

    def pool_stats(self):
        return dict(num_tp=self._count(SampleLabel.TRUE_POSITIVE), num_fp=self._count(SampleLabel.FALSE_POSITIVE))

    def update_scores(self, model):
        """Re-evaluate the model on every pooled sample ('scores' becomes -inf where it rejects)."""
        if self.samples is not None:
            self.samples.set_field("scores", model.predict(self.samples.get_field("samples"))[0])

    def remove_low_scoring(self, min_score=-np.inf):
        if self.samples is None:
            return
        alive = self.samples.get_field("scores") > min_score
        self.logger.log(15, f"Removed {int((~alive).sum())}/{alive.size} samples (min_score={min_score:.2f})")
        self.samples = self.samples[np.flatnonzero(alive)]

    def update(self, model, iterable):
        """Drop what the current model rejects, then scan images from `iterable` (dicts with 'image' and
        'groundtruth_boxes') until the pool holds min_tp / min_fp samples again."""
        self.update_scores(model)
        self.remove_low_scoring()
        missing = {SampleLabel.TRUE_POSITIVE: max(self.min_tp - self._count(SampleLabel.TRUE_POSITIVE), 0),
                   SampleLabel.FALSE_POSITIVE: max(self.min_fp - self._count(SampleLabel.FALSE_POSITIVE), 0)}
        self.logger.log(15, f"Pool needs tp: {missing[SampleLabel.TRUE_POSITIVE]}, fp: {missing[SampleLabel.FALSE_POSITIVE]}")
        if not any(missing.values()):
            return
        fresh = []
        for item in iterable:
            for boxes in get_samples_from_image(model, item["image"], item["groundtruth_boxes"],
                                                tp=missing[SampleLabel.TRUE_POSITIVE] > 0,
                                                fp=missing[SampleLabel.FALSE_POSITIVE] > 0, **self.label_boxes_args):
                got = boxes.get_field("tp_label")
                for lab in missing:
                    missing[lab] -= int((got == lab).sum())
                fresh.append(boxes)
            if all(v <= 0 for v in missing.values()):
                break
        if fresh:
            self.samples = concatenate(([self.samples] if self.samples is not None else []) + fresh)

    def get_samples(self, label):
        """(X, H): feature maps (N, m, n, C) and scores (N,) of the pooled samples with `label` (copies)."""
        chosen = self.samples[np.flatnonzero(self.samples.get_field("tp_label") == label)]
        return chosen.get_field("samples").copy(), chosen.get_field("scores").flatten().copy()

    def get_true_positives(self):
        return self.get_samples(SampleLabel.TRUE_POSITIVE)

    def get_false_positives(self):
        return self.get_samples(SampleLabel.FALSE_POSITIVE)


# --------------------------------------------------------------------------------------- mining on the device
class MinedSamples:
    """Chosen windows of a mined batch (mine_batch) or of a DeviceSamplePool, as device tensors of N rows in
    (image, level, row, col) order: samples (N, m, n, C) in the channels' dtype, scores float32, tp_label int32
    (SampleLabel), instance_id int32 (index of the best ground-truth box inside its image's list, -1 without ground
    truth), image / level / row / col int32, boxes float32 (N, 4), best float64 (the best IoU)."""
    FIELDS = ("samples", "scores", "tp_label", "instance_id", "image", "level", "row", "col", "boxes", "best")

    def __init__(self, **fields):
        assert set(fields) == set(self.FIELDS)
        for k, v in fields.items():
            setattr(self, k, v)

    def __len__(self):
        return int(self.scores.shape[0])

    def take(self, idx):
        """The rows `idx` (a device index tensor), copied."""
        return MinedSamples(**{k: getattr(self, k)[idx] for k in self.FIELDS})

    @staticmethod
    def cat(parts):
        import torch
        return MinedSamples(**{k: torch.cat([getattr(p, k) for p in parts]) for k in MinedSamples.FIELDS})

    def to_boxes(self, where=True):
        """A host Boxes with the fields get_samples_from_image yields ('scores', 'row', 'col', 'instance_id', 'tp_label',
        'samples') and, with `where`, 'image' and 'level'."""
        host = lambda k: getattr(self, k).cpu().numpy()
        out = Boxes(host("boxes"), scores=host("scores"), row=host("row").astype(np.int64), col=host("col").astype(np.int64),
                    instance_id=host("instance_id"), tp_label=host("tp_label"), samples=host("samples"))
        if where:
            out.set_field("image", host("image"))
            out.set_field("level", host("level"))
        return out


def _ground_truth_arrays(gts):
    """(gt float64 [n_gt, 4], gt_off int32 [B + 1], ignore uint8 [n_gt]) of a list of Boxes / None, validated."""
    from .boxes import _match_coords
    coords, flags = [], []
    for g in gts:
        if g is None or len(g) == 0:
            coords.append(np.zeros((0, 4), np.float64))
            flags.append(np.zeros(0, np.uint8))
            continue
        f = np.asarray(g.get_field("ignore")) if g.has_field("ignore") else np.zeros(len(g))
        if f.ndim != 1:
            raise ValueError("'ignore' field must be single dimension")
        coords.append(_match_coords(g, "ground-truth"))
        flags.append((f != 0).astype(np.uint8))
    off = np.zeros(len(gts) + 1, np.int64)
    np.cumsum([c.shape[0] for c in coords], out=off[1:])
    if off[-1] >= 1 << 31:
        raise ValueError("mine_batch: at most 2**31 - 1 ground-truth boxes")
    return np.concatenate(coords).reshape(-1, 4), off.astype(np.int32), np.concatenate(flags)


def _empty_mined(shape, chn_dtype, dev):
    import torch
    z = lambda dt, *s: torch.empty((0,) + s, dtype=dt, device=dev)
    i32 = torch.int32
    return MinedSamples(samples=z(chn_dtype, *(int(x) for x in shape)), scores=z(torch.float32), tp_label=z(i32), instance_id=z(i32),
                        image=z(i32), level=z(i32), row=z(i32), col=z(i32), boxes=z(torch.float32, 4), best=z(torch.float64))


def order_rows(rows):
    """wb_mine_select_launch's rows (device int32 [N, 8]) in (image, level, r, c) order."""
    from . import engine as _engine
    return _engine.sort_records(rows)


def level_table(eng):
    """The pyramid levels of an engine as wb_mine_gather_launch's table (nat.MINE_LEVEL_DTYPE [L])."""
    table = np.zeros(eng.plan.n_levels, nat.MINE_LEVEL_DTYPE)
    for k in ("chn_off", "u", "v"):
        table[k] = eng.level_np[k]
    return table


class LabelledBatch:
    """What mine_batch and calibration.instance_windows share around their labelling call: a batch `images` [B, H, W] (or
    one [H, W]) with the ground truth of every image (a list of B Boxes / None; for one image the Boxes itself), checked
    (`who` names the caller in the messages), and its engine.  Attributes: images [B, H, W], B, gt / gt_off / ignore
    (_ground_truth_arrays), m, n, C (the model's window), dev, eng, L (pyramid levels; 0: nothing to run) and, after
    run_channels, table (level_table) and inv (float32 1 / scale); after upload, ptr (the device pointers by name)."""

    def __init__(self, model, images, gt_boxes_per_image, who):
        from . import channels as _channels
        from . import engine as _engine
        if getattr(images, "ndim", None) == 2:
            images = images[None]
            gts = list(gt_boxes_per_image) if isinstance(gt_boxes_per_image, (list, tuple)) else [gt_boxes_per_image]
        elif getattr(images, "ndim", None) == 3:
            gts = list(gt_boxes_per_image)
        else:
            raise ValueError("images must have 3 dimensions [B,H,W] (or 2: one image)")
        B, H, W = (int(x) for x in images.shape)
        if len(gts) != B:
            raise ValueError(f"{who}: {B} images, ground truth of {len(gts)}")
        self.images, self.B = images, B
        self.gt, self.gt_off, self.ignore = _ground_truth_arrays(gts)
        shrink, n_per_oct, smooth, spec = _channels.read_opts(model.channel_opts)
        self.m, self.n, self.C = (int(x) for x in model.shape)
        assert self.C == spec.n_channels, f"Invalid number of channels. Expected {self.C} given {spec.n_channels}."
        self.dev = nat.require_gpu()
        self.eng = _engine.get_engine(H, W, _engine.array_dtype(images), shrink, n_per_oct, smooth, B, channels=spec)
        self.L = self.eng.plan.n_levels

    def run_channels(self):
        """The pyramid of the batch, where it stays; the level table and 1 / scale on the host."""
        self.eng.load_images(self.images)
        self.eng.run_channels()
        self.table = level_table(self.eng)
        self.inv = np.ascontiguousarray(self.eng.inv_scales(), np.float32)

    def upload(self, **more):
        """The one upload (nat.Block): gt | table | gt_off | `more` (the caller's own 4-byte arrays) | inv_scale | ignore, as
        ptr[name]."""
        assert hasattr(self, "table"), "LabelledBatch.upload comes after run_channels"
        self.block = nat.Block.upload(self.dev, gt=self.gt, table=self.table, gt_off=self.gt_off, **more, inv_scale=self.inv, ignore=self.ignore)
        self.ptr = self.block.ptr

    def mined(self, rows):
        """The labelled rows (device int32 [N, 8], N >= 1) as a MinedSamples in (image, level, r, c) order -- order_rows,
        the crops (wb_mine_gather_launch), the boxes (wb_boxes_launch) -- and the gather's error word, a device tensor
        that is not waited for here: non-zero when a window lies outside its pyramid level."""
        import torch
        assert hasattr(self, "ptr"), "LabelledBatch.mined comes after run_channels and upload"
        eng, m, n, dev = self.eng, self.m, self.n, self.dev
        N = int(rows.shape[0])
        rows = order_rows(rows)
        crops = torch.empty((N, m, n, self.C), dtype=eng.chn.dtype, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        nat.launch("wb_mine_gather_launch", eng.chn, eng.spec.wb_dtype, eng.chn_stride, self.B, self.ptr["table"], self.L, self.C, rows,
                   N, m, n, crops, err)
        det = rows[:, :4].contiguous()
        boxes = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scores = torch.empty(N, dtype=torch.float32, device=dev)
        nat.launch("wb_boxes_launch", det, N, self.ptr["inv_scale"], m, n, boxes, scores)
        rc = rows[:, 2]
        return MinedSamples(samples=crops, scores=scores, tp_label=rows[:, 7].clone(), instance_id=rows[:, 6].clone(),
                            image=rows[:, 0].clone(), level=rows[:, 1].clone(), row=rc & 0xFFFF, col=(rc >> 16) & 0xFFFF, boxes=boxes,
                            best=rows[:, 4:6].contiguous().view(torch.float64).reshape(-1)), err


def mine_batch(model, images, gt_boxes_per_image, tp=True, fp=True, min_tp_iou=0.7, max_fp_iou=0.3, max_tp_candidates=100,
               max_fp_candidates=100, seed=0, serial0=0):
    """get_samples_from_image for a batch, on the device: `images` [B, H, W] (or one [H, W]; what the engine accepts) go
    through one scan, every surviving window is labelled against its image's ground truth (a list of B Boxes / None;
    for one image the Boxes itself), at most max_*_candidates per (image, pyramid level) and class are chosen, and the
    chosen windows are cropped out of the pyramid -- two native calls (wb_mine_select_launch, wb_mine_gather_launch)
    on the records and the pyramid where they lie.  Returns a MinedSamples; updates model.n_loc / n_weak as a scan does.

    The rule.  Labelling is label_boxes': the box of record (image, level, r, c) is float32 [c, r, c+n, r+m] *
    float32(1 / scale[level]); IoU is boxes.iou's float64 arithmetic; `best` is the largest IoU over the image's ground
    truth, the owner its first argmax; no ground truth: best 0, owner -1, every window an FP hit.  FP hit: best <
    max_fp_iou; TP hit: best > min_tp_iou and the owner's 'ignore' flag is 0.  Choice is per (image, level) and class: of H
    hits the min(H, max_*_candidates) with the smallest keys, key = fmix32(((r << 16) | c) ^ g), g = fmix32(fmix32(seed ^
    fmix32(serial + 0x9E3779B9)) ^ (level * 0x9E3779B1)), serial = serial0 + the image's index in the batch (uint32
    arithmetic; fmix32 is MurmurHash3's 32-bit finaliser, a bijection: keys never tie inside a group).  Labels are written
    TP first, then FP: a window chosen for both is FP.  With tp=False / fp=False that class is neither chosen nor
    returned.  The result is in (image, level, r, c) order.

    Deviation from the reference: select_candidates thins with np.random.choice WITH replacement from NumPy's global
    state (so it can pick fewer than the cap through duplicates, and no two runs agree); this choice is without
    replacement and depends on (seed, serial, level, r, c) alone -- not on the batch an image sits in, the order of the
    scan's records or the run.

    Host traffic: one upload (ground truth, offsets, flags, serials, level table, 1 / scale), four waits (the scan's
    counters twice as in every scan, the number of chosen rows with the scan statistics, the gather's error word); neither
    records, pyramid nor crops leave the device.  Images too small for any level, or no detections: an empty result
    without a mining launch."""
    import torch
    from . import engine as _engine
    b = LabelledBatch(model, images, gt_boxes_per_image, "mine_batch")
    if max_tp_candidates < 0 or max_fp_candidates < 0:
        raise ValueError("max_tp_candidates and max_fp_candidates must not be negative")
    B, L, m, n, dev, eng = b.B, b.L, b.m, b.n, b.dev, b.eng
    chn_dtype = eng.chn.dtype
    if L == 0:
        return _empty_mined(model.shape, chn_dtype, dev)
    b.run_channels()
    dm = model.device_cascade()
    stt = eng.run_cascade(dm)                              # float / uint8 channels, not rank bytes
    total = eng.ensure_capacity(dm)                        # (grows the buffer and scans again when a shard overflowed)
    T = len(model)
    model.n_loc += B * eng.plan.n_loc(m, n)
    if total == 0:
        model.n_weak += int(_engine.alive_host(stt.alive, T).sum())
        return _empty_mined(model.shape, chn_dtype, dev)
    recs = eng.pack()[1:1 + total]                         # the valid records, shard order
    b.upload(serial=((int(serial0) + np.arange(B, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32))
    k_tp = min(int(max_tp_candidates), total) if tp else 0
    k_fp = min(int(max_fp_candidates), total) if fp else 0
    room = min(total, B * L * (k_tp + k_fp))
    scratch = torch.empty(nat.query("wb_mine_scratch_bytes", total, B, L), dtype=torch.uint8, device=dev)
    rows = torch.empty((max(room, 1), 8), dtype=torch.int32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.launch("wb_mine_select_launch", recs, total, b.ptr["inv_scale"], L, m, n, b.ptr["gt"], b.ptr["gt_off"], b.ptr["ignore"],
               b.gt.shape[0], b.ptr["serial"], B, float(min_tp_iou), float(max_fp_iou), int(max_tp_candidates), int(max_fp_candidates),
               int(bool(tp)), int(bool(fp)), int(seed) & 0xFFFFFFFF, scratch, scratch.numel(), rows, room, n_rows)
    h = torch.cat([n_rows, stt.alive.reshape(-1)]).cpu().numpy()      # one wait: the chosen rows' number and the statistics
    N = int(h[0])
    model.n_weak += int(h[1:].reshape(stt.alive.shape)[:, :, :T].astype(np.int64).sum())
    if N == 0:
        return _empty_mined(model.shape, chn_dtype, dev)
    assert N <= room
    got, err = b.mined(rows[:N])
    if int(err.item()):
        raise RuntimeError("mine_batch: a chosen window lies outside its pyramid level (the records do not belong to this pyramid)")
    return got


def image_batches(iterable, batch):
    """The items of `iterable` (dicts with 'image') as lists of at most `batch` consecutive items whose images have one
    (shape, dtype), in order.  A list is yielded as soon as it is full, before the next item is read; an item of another
    kind is read, and then what waits goes first; the remainder comes at the end.  So a caller that stops after a list
    has taken from its iterator exactly the items of the lists it saw -- and the one item whose kind ended the last."""
    group, kind = [], None
    for item in iterable:
        image = item["image"]
        its = (tuple(image.shape), str(image.dtype))
        if group and its != kind:                          # a shape change: what waits goes first
            yield group
            group = []
        kind = its
        group.append(item)
        if len(group) == batch:
            yield group
            group = []
    if group:
        yield group


def stack_images(items):
    """The images of one of image_batches' lists as one [B, H, W] array (ndarrays) or tensor."""
    first = items[0]["image"]
    if isinstance(first, np.ndarray):
        return np.stack([it["image"] for it in items])
    import torch
    return torch.stack([it["image"] for it in items])


class DeviceSamplePool(object):
    """SamplePool with its samples resident on the GPU: `update` mines `batch` images of equal shape and dtype per scan
    (mine_batch: its selection rule, not np.random.choice -- see there), the crops never travel to the host, and the
    re-scoring, the fits and the predictions of a training stage read them where they lie.  Methods and meaning are
    SamplePool's; get_samples returns X as a device tensor (a copy) and H as a float32 ndarray -- what Learner.fit_stage
    takes.  seed: of the selection keys; an image's serial is the number of images this pool consumed before it.
    The pool's order is SamplePool's: old samples first, then the new ones in mining order, (image, level, row, col)."""

    def __init__(self, min_tp=1000, min_fp=1000, logger=None, batch=8, seed=0, **kwargs):
        self.samples = None                    # MinedSamples ('image' holds the images' serials)
        self.min_tp, self.min_fp = min_tp, min_fp
        self.batch = max(int(batch), 1)
        self.seed = int(seed)
        self.images_seen = 0
        self.label_boxes_args = kwargs
        self.logger = logger or logging.getLogger("DeviceSamplePool")

    def _counts(self, labels):
        """{TP: n, FP: n} of an int32 label tensor: one read-back."""
        import torch
        both = torch.stack([(labels == SampleLabel.TRUE_POSITIVE).sum(), (labels == SampleLabel.FALSE_POSITIVE).sum()]).cpu()
        return {SampleLabel.TRUE_POSITIVE: int(both[0]), SampleLabel.FALSE_POSITIVE: int(both[1])}

    def pool_stats(self):
        if self.samples is None:
            return dict(num_tp=0, num_fp=0)
        got = self._counts(self.samples.tp_label)
        return dict(num_tp=got[SampleLabel.TRUE_POSITIVE], num_fp=got[SampleLabel.FALSE_POSITIVE])

    def update_scores(self, model):
        """Re-evaluate the model on every pooled sample, where it lies ('scores' becomes -inf where it rejects)."""
        import torch
        if self.samples is None or len(self.samples) == 0:
            return
        X = self.samples.samples
        assert tuple(X.shape[1:]) == tuple(model.shape), f"Invalid shape of X. Expected {model.shape}, given {tuple(X.shape[1:])}"
        N = int(X.shape[0])
        H = torch.empty(N, dtype=torch.float32, device=X.device)
        mask = torch.empty(N, dtype=torch.uint8, device=X.device)
        X, wdt = nat.window_tensor(X, X.device)
        nat.launch("wb_samples_predict_launch", model.device_cascade().handle, X, wdt, N, H, mask)
        self.samples.scores = H

    def remove_low_scoring(self, min_score=-np.inf):
        import torch
        if self.samples is None:
            return
        alive = self.samples.scores > min_score
        if self.logger.isEnabledFor(15):
            self.logger.log(15, f"Removed {int((~alive).sum())}/{alive.numel()} samples (min_score={min_score:.2f})")
        self.samples = self.samples.take(torch.nonzero(alive).reshape(-1))

    def _mine(self, model, items, missing):
        """Mine one batch of items; the new samples (or None)."""
        got = mine_batch(model, stack_images(items), [it["groundtruth_boxes"] for it in items],
                         tp=missing[SampleLabel.TRUE_POSITIVE] > 0, fp=missing[SampleLabel.FALSE_POSITIVE] > 0, seed=self.seed,
                         serial0=self.images_seen, **self.label_boxes_args)
        if len(got):
            got.image = got.image + (self.images_seen & 0x7FFFFFFF)
        self.images_seen += len(items)
        return got if len(got) else None

    def update(self, model, iterable):
        """Drop what the current model rejects, then mine images from `iterable` (dicts with 'image' and
        'groundtruth_boxes'), `batch` of equal shape and dtype at a time, until the pool holds min_tp / min_fp samples
        again: it stops after the first batch that fills both quotas."""
        self.update_scores(model)
        self.remove_low_scoring()
        have = self._counts(self.samples.tp_label) if self.samples is not None else {SampleLabel.TRUE_POSITIVE: 0, SampleLabel.FALSE_POSITIVE: 0}
        missing = {SampleLabel.TRUE_POSITIVE: max(self.min_tp - have[SampleLabel.TRUE_POSITIVE], 0),
                   SampleLabel.FALSE_POSITIVE: max(self.min_fp - have[SampleLabel.FALSE_POSITIVE], 0)}
        self.logger.log(15, f"Pool needs tp: {missing[SampleLabel.TRUE_POSITIVE]}, fp: {missing[SampleLabel.FALSE_POSITIVE]}")
        if not any(missing.values()):
            return
        fresh = []
        for group in image_batches(iterable, self.batch):
            got = self._mine(model, group, missing)
            if got is not None:
                for lab, cnt in self._counts(got.tp_label).items():
                    missing[lab] -= cnt
                fresh.append(got)
            if all(v <= 0 for v in missing.values()):
                break
        if fresh:
            self.samples = MinedSamples.cat(([self.samples] if self.samples is not None else []) + fresh)

    def get_samples(self, label):
        """(X, H): feature maps (N, m, n, C) as a device tensor and scores (N,) as a float32 ndarray of the pooled
        samples with `label` (copies)."""
        import torch
        if self.samples is None:
            raise RuntimeError("the pool holds no samples")
        idx = torch.nonzero(self.samples.tp_label == label).reshape(-1)
        return self.samples.samples[idx], self.samples.scores[idx].cpu().numpy().reshape(-1)

    def get_true_positives(self):
        return self.get_samples(SampleLabel.TRUE_POSITIVE)

    def get_false_positives(self):
        return self.get_samples(SampleLabel.FALSE_POSITIVE)

    def to_host(self):
        """The pool as an ordinary Boxes, as SamplePool.samples holds it (None while empty)."""
        return None if self.samples is None else self.samples.to_boxes(where=False)
