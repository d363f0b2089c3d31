"""Detection model -- drop-in for ``waldboost.model.Model`` on the detection path
(reference model.py:32-344): same constructor, ``append``/iteration, ``detect``,
``predict_on_image``, ``channels``, ``scan_channels``, ``get_boxes``, ``eval_cost``/``reset``
and the zlib+protobuf ``.pb`` format.  The dense cascade scan runs in csrc/wb_cascade.hip.
"""
import os
import zlib
from typing import NamedTuple

import numpy as np
from google.protobuf.message import DecodeError

from . import _native as nat
from . import channels as _channels
from . import engine as _engine
from . import model_pb2
from .boxes import Boxes, _keep_mask, finish, suppression
from .channels import channel_pyramid
from .compare import channel_tensor
from .readback import Detections, from_finished, from_image_result, from_ordered, from_packed
from .stream import Schedule
from .training import DTree, _REBINDS

# above this many detections per call the compaction, ordering and boxes stay on the GPU
_HOST_POST_MAX = 1 << 16
_HOST_POST_BATCH = 2048          # a batch: more detections than this are ordered on the device
# a batch: split by image and ordered by wb_det_order_batch_launch (tests and WB_NO_ORDER_BATCH switch it off) ...
_ORDER_BATCH = os.environ.get("WB_NO_ORDER_BATCH") is None
_ORDER_BATCH_MAX = 256           # ... up to this many images (the read-back block is fixed-size)
_torch = None                    # torch, from the first detect_stream call on (imported late: reading a .pb needs none)


def symbol_name(s):
    """Name written into .pb files: the reference's own module.qualname for the channel functions
    this build implements, so that the reference can load our files too (model.py:23-24, 302)."""
    spec = _channels.channel_spec(s)
    if spec is not None:
        return spec.reference_name
    return s.__module__ + "." + s.__qualname__


def symbol_from_name(name: str):
    """Allow-list replacement of the reference's eval-based lookup (model.py:27-29)."""
    try:
        return _channels.CHANNEL_FUNCS[name]
    except KeyError:
        raise ValueError(f"unknown channel function {name!r} in model file "
                         f"(known: {sorted(_channels.CHANNEL_FUNCS)})") from None


def _suppress(res, nms):
    """The detections of one image's complete result that non-maximum suppression keeps: by the flags the device left
    behind the scan; without them the result goes through boxes.nms_keep_mask, on the GPU as well."""
    if nms is None:
        return res
    keep = res.keep if res.keep is not None else _keep_mask(res.boxes, res.scores, nms)
    return res.take(np.flatnonzero(keep))


def _orders_batch(eng):
    """Whether a batch on `eng` is split by image and ordered by wb_det_order_batch_launch."""
    return _ORDER_BATCH and eng.batch <= _ORDER_BATCH_MAX


def _as_boxes(res):
    out = Boxes(res.boxes)
    out.set_field("scores", res.scores)
    return out


def _raw(res, alive, scales):
    """The dict detect_raw returns."""
    level, r, c = res.windows()
    return dict(boxes=res.boxes, scores=res.scores, level=level, r=r, c=c, alive=alive, scales=list(scales))


class _BatchToken(NamedTuple):
    """What a lane's scan_batch hands to its collect."""
    stt: object                      # the scan state
    ordered: bool                    # order_batch_enqueue ran behind the scan


class _Lane(NamedTuple):
    """A lane of detect_stream (stream.Schedule has the protocol): an engine and the stream all its work runs on."""
    engine: object
    stream: object

    @property
    def n_levels(self):
        return self.engine.plan.n_levels

    def scan_image(self, image, dm, nms):
        with _torch.cuda.stream(self.stream):
            self.engine.load_images(image)
            return self.engine.detect_enqueue(dm, nms)

    def load_slot(self, b, image):
        with _torch.cuda.stream(self.stream):
            self.engine.load_slot(b, image)

    def scan_batch(self, dm, nms):
        eng = self.engine
        with _torch.cuda.stream(self.stream):
            stt = eng.batch_enqueue(dm)
            # the batch's results split by image, ordered and on their way to the host right behind the scan
            return _BatchToken(stt, bool(_orders_batch(eng) and eng.order_batch_enqueue(dm, stt, nms)))

    def collect(self, model, dm, token, count, nms):
        eng = self.engine
        if isinstance(token, _BatchToken):
            with _torch.cuda.stream(self.stream):
                out, _ = model._assemble(eng, dm, token.stt, count, nms, windows=False, ordered_enqueued=token.ordered)
        else:
            fin = eng.detect_collect(dm, token, self.stream, nms=nms)
            if fin is None:                                   # (more detections than the one read-back holds: further copies)
                with _torch.cuda.stream(self.stream):
                    out, _ = model._assemble(eng, dm, eng._casc_state(dm), 1, nms, windows=False, single=True)
            else:
                out, _ = model._assemble(eng, dm, eng._casc_state(dm), 1, nms, windows=False, single=True, finished=fin)
        return [_as_boxes(res) for res in out]

    def wait_upload(self):
        self.engine.wait_upload()

    def synchronize(self):
        self.stream.synchronize()


class Model:
    def __init__(self, shape, channel_opts):
        self.shape = shape
        self.channel_opts = channel_opts
        self.classifier = []
        self.theta = []
        self._device = None
        self._content = None
        self._lanes = {}             # detect_stream's lanes: (shape, dtype, channel options, batch) -> [_Lane], two keys at most
        self.reset()

    def __getstate__(self):
        """copy / pickle carry the model (the reference's Model is a plain object), not its device-side state."""
        d = dict(self.__dict__)
        d["_device"] = d["_content"] = None
        d.pop("_lanes", None)
        return d

    # ---- statistics (reference model.py:69-89)
    @property
    def eval_cost(self):
        return self.n_weak / self.n_loc if self.n_loc > 0 else 0

    def reset(self):
        self.n_loc = 0
        self.n_weak = 0

    # ---- container (reference model.py:91-92, 261-283)
    def __getitem__(self, i):
        return self.classifier[i], self.theta[i]

    def __len__(self):
        return len(self.classifier)

    def __bool__(self):
        return bool(self.classifier)

    def __iter__(self):
        yield from zip(self.classifier, self.theta)

    def append(self, weak, theta):
        self.classifier.append(weak)
        self.theta.append(theta)
        self._device = None

    def device_cascade(self):
        """The device-side cascade for the current stage list.  `classifier` and `theta` are plain public lists in the
        reference and callers edit them -- and the trees' arrays -- in place, so the cached handle is keyed by the lists'
        current CONTENT: the identity and the bytes of every tree (DTree.content: one private block per tree, joined in
        one call) and the value and kind of every theta.  The GPU holds a private copy; nothing of the caller's is frozen."""
        # (theta by value AND kind: the float kind matters to theta_as_f32; a NaN theta still matches itself -- tuple
        # comparison takes identical objects as equal)
        ids = tuple(map(id, self.classifier))
        cc = self._content
        if cc is None or cc[0] != ids or cc[1] != _REBINDS[0]:
            # (the trees' blocks as buffers, looked up once per stage list; a tree with a rebound array has no block and
            # is read array by array on every call)
            trees = list(self.classifier)                        # (keeps the ids alive and unique)
            views = [memoryview(w._blob) for w in trees] if all(w._blob is not None for w in trees) else None
            cc = self._content = (ids, _REBINDS[0], views, trees)
        content = b"".join(cc[2]) if cc[2] is not None else b"".join([bytes(w.content()) for w in cc[3]])
        sig = (tuple(self.shape), ids, tuple(self.theta), tuple(map(type, self.theta)), content)
        if self._device is None or self._device[0] != sig:
            dev = _engine.DeviceCascade(self.shape, self.classifier, self.theta)
            self._device = (sig, dev, list(self.classifier))     # (the list keeps the ids alive and unique)
        return self._device[1]

    # ---- pyramid (reference model.py:95-134)
    def channels(self, image):
        yield from channel_pyramid(image, self.channel_opts)

    def scan_channels(self, image):
        yield from ((chns, scale, self.predict_on_image(chns)) for chns, scale in self.channels(image))

    def get_boxes(self, r, c, scale) -> Boxes:
        """XYXY boxes of window origins (r, c) at pyramid scale `scale` (reference model.py:136-147)."""
        r = np.asarray(r)
        c = np.asarray(c)
        if r.size == 0:
            return Boxes(np.empty((0, 4), "f"))
        m, n = self.shape[:2]
        x1 = c.reshape(-1, 1)
        y1 = r.reshape(-1, 1)
        rects = np.concatenate([x1, y1, x1 + n, y1 + m], axis=1).astype(np.float32)
        return Boxes(rects).normalized(scale=1.0 / scale)

    # ---- the cascade on one channel image (reference model.py:216-259)
    def predict_on_image(self, X):
        """All windows of X[u,v,C] through the cascade -> (rs, cs, hs) of the survivors in
        row-major order; updates n_loc / n_weak."""
        rs, cs, hs, alive = self.predict_on_image_stats(X)
        return rs, cs, hs

    def predict_on_image_stats(self, X):
        """As predict_on_image, plus alive[t] = windows entering stage t."""
        import torch
        u, v, ch_image = X.shape
        m, n, ch_cls = self.shape
        assert ch_image == ch_cls, f"Invalid number of channels. Expected {ch_cls} given {ch_image}."
        dm = self.device_cascade()
        Xd, wdt = channel_tensor(X, nat.require_gpu())       # any dtype, compared as NumPy would (compare.py)
        eng = _SingleLevel.get(u, v, ch_image, np.uint8 if wdt == nat.WB_DTYPE_U8 else np.float32)
        eng.load(Xd)
        n_det, alive = eng.scan(dm)
        self.n_loc += max(u - m, 0) * max(v - n, 0)
        self.n_weak += int(alive.sum())
        det = eng.sorted(n_det)
        if n_det == 0:
            return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.float32), alive
        d = det.cpu().numpy().view(nat.DET_DTYPE).reshape(-1)
        return d["r"].astype(np.int64), d["c"].astype(np.int64), d["score"].copy(), alive

    # ---- whole-image detection (reference model.py:149-179)
    def detect(self, image, iou_threshold=None, score_threshold=None, vote_iou=None, vote_weights="uniform", min_votes=1) -> Boxes:
        """Detect objects in a 2-D image; returns Boxes with a 'scores' field, levels in pyramid
        order and windows in row-major order within a level, like the reference.
        iou_threshold: greedy non-maximum suppression of the result (boxes.non_max_suppression has the semantics;
        score_threshold drops boxes below it first): the kept detections, still in that order.  It runs on the device
        on the finished detections, enqueued behind the step's graph replay and in front of the call's one wait (the
        plain step's graph is shared: a new threshold captures nothing); n_loc / n_weak are those of the scan.  None: the
        plain call.  Scores are never NaN for a model the loader accepts.
        vote_iou (needs an iou_threshold), vote_weights, min_votes: box voting -- boxes.merge_detections of the call's
        complete, unsuppressed result with these thresholds: every kept box becomes the mean of its cluster and gets a 'votes'
        field; kept boxes with fewer than min_votes voters are left out.  That is a second device round trip (an upload, NMS
        and the vote kernel, a read-back) after the scan's read-back.  None: exactly the call without it."""
        how = suppression(iou_threshold, score_threshold, vote_iou, vote_weights, min_votes)
        voting = how is not None and how.vote is not None
        res, _, _ = self._detect_one(image, None if voting else how, windows=False)
        return finish(_as_boxes(res), how if voting else None)

    def detect_raw(self, image, _nms=None):
        """detect() with everything the parity tests compare: boxes, scores, (level, r, c),
        alive[level, stage]; updates n_loc / n_weak."""
        return _raw(*self._detect_one(image, _nms and suppression(*_nms)))

    def _detect_one(self, image, nms, windows=True):
        """One image -> (its Detections, alive[L, T], the levels' scales); updates n_loc / n_weak."""
        _channels._validate_image(image, allow_tensor=True)
        shrink, n_per_oct, smooth, spec = _channels.read_opts(self.channel_opts, allow_callable=True)
        if spec is None:
            if not isinstance(image, np.ndarray):
                image = image.cpu().numpy()                 # (a caller's own channel function takes host arrays)
            res, alive, scales = self._detect_levelwise(image)
            return _suppress(res, nms), alive, scales
        m, n, Cc = self.shape
        assert Cc == spec.n_channels, f"Invalid number of channels. Expected {Cc} given {spec.n_channels}."
        H, W = (int(x) for x in image.shape)
        dm = self.device_cascade()
        eng = _engine.get_engine(H, W, _engine.array_dtype(image), shrink, n_per_oct, smooth, 1, channels=spec)
        if eng.plan.n_levels == 0:
            return Detections.none(), np.zeros((0, len(self)), np.int64), []
        eng.load_images(image)
        # one memset + octaves + channels (straight to this cascade's threshold ranks when it has rank tables) + cascade
        # + boxes and sort keys + the read-back: one hipGraph replay from the second call on
        fin = eng.detect_run(dm, nms)
        (res,), alive = self._assemble(eng, dm, eng._casc_state(dm), 1, nms, windows=windows, single=True, finished=fin)
        return res, alive[0], eng.plan.scales

    def _detect_levelwise(self, image):
        """_detect_one for a channel function without a kernel: the reference's own loop (model.py:171-177) -- one level at
        a time from the generator (the caller's function runs between the GPU steps), each scanned on the GPU."""
        T = len(self)
        level, r, c, scores, boxes, alive, scales = [], [], [], [], [], [], []
        for lv, (chns, scale) in enumerate(self.channels(image)):
            rs, cs, hs, al = self.predict_on_image_stats(chns)
            alive.append(al)
            scales.append(scale)
            if rs.size:
                level.append(np.full(rs.size, lv, np.int32))
                r.append(rs)
                c.append(cs)
                scores.append(hs)
                boxes.append(self.get_boxes(rs, cs, scale).get())
        cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.empty(0, dt)
        res = Detections(np.concatenate(boxes) if boxes else np.empty((0, 4), "f"), cat(scores, np.float32),
                         windows=(cat(level, np.int32), cat(r, np.int64), cat(c, np.int64)))
        return res, np.stack(alive) if alive else np.zeros((0, T), np.int64), scales

    def scan_engine(self, eng, view=None):
        """Run this cascade over the channel pyramid already resident in `eng` (channels computed
        by the caller: several models can share one pyramid, reference __init__.py:120-124).
        view: this model's member view of a RankGroup whose threshold ranks `eng` holds (scan those instead of the
        float32 channels).  Returns the same dict as detect_raw and updates n_loc / n_weak.  The result is image 0's: of an
        engine that holds a batch, the other images' records are left out."""
        m, n, Cc = self.shape
        assert Cc == eng.spec.n_channels, f"Invalid number of channels. Expected {Cc} given {eng.spec.n_channels}."
        dm = view if view is not None else self.device_cascade()
        return self._scan_result(eng, dm, eng.run_cascade(dm, ranks=view is not None), fetch_final=True)

    def scan_resident(self, image):
        """Scan one host image and leave its pyramid resident: (eng, found) -- the engine that holds the channels and
        scan_engine's dict of it -- or None when the image is too small for any level.  The scan reads the float or uint8
        channels, not rank bytes: what the callers go on to crop, verify or regress from.  One host wait, the scan's
        read-back; n_loc / n_weak advance as in a scan."""
        _channels._validate_image(image)
        shrink, n_per_oct, smooth, spec = _channels.read_opts(self.channel_opts)
        if spec.dtype == np.uint8:
            _channels._require_u8(image, spec.key)
        eng = _engine.get_engine(image.shape[0], image.shape[1], image.dtype, shrink, n_per_oct, smooth, 1, channels=spec)
        if eng.plan.n_levels == 0:
            return None
        eng.load_images(image)
        eng.run_channels()
        return eng, self.scan_engine(eng)                    # every level in one launch group

    def _scan_result(self, eng, dm, stt, **have):
        """The dict detect_raw returns, of the scan `stt` of image 0 of `eng` (have: what _assemble is told of it)."""
        (res,), alive = self._assemble(eng, dm, stt, 1, None, single=True, **have)
        return _raw(res, alive[0], eng.plan.scales)

    def _assemble(self, eng, dm, stt, count, nms, *, windows=True, single=False, finished=None, fetch_final=False,
                  ordered_enqueued=False):
        """The results of the scan `stt` of `eng` with the cascade `dm` (the one that was scanned: detect_stream collects
        late) -> ([Detections of image b for b < count], alive int64 [B, L, T]); updates n_loc / n_weak.  The slots
        behind `count` hold earlier images, whose results are dropped; windows=False: boxes and scores are all the caller
        wants (routes 1 and 2 then leave the sort keys where they are).  Every route has ONE host synchronisation, grows
        the detection buffer and scans again after an overflow, and leaves copies of its read-back.  The first that applies:
          1. single -- one image, in the one-image finish block (sort keys, boxes, scores, statistics in one copy:
             wb_det_finish_sorted_launch): `finished`, what detect_run / detect_collect returned for this scan, or with
             fetch_final the block fetched here.  Up to PyramidEngine._FETCH_ROWS detections.
          2. not single -- a batch, split by image, ordered and finished on the device (wb_det_order_batch_launch), one
             read-back; ordered_enqueued: the launch and the copies are behind the scan already, only the wait is left.  Up
             to PyramidEngine._ORDER_ROWS detections per image and _ORDER_BATCH_MAX images.
          3. the packed records (wb_det_pack_launch): few detections (the usual case) are ordered and their boxes formed on
             the host -- the same float32 arithmetic as boxes_kernel, without three launches and four copies; more than
             _HOST_POST_MAX (single) / _HOST_POST_BATCH stay on the device for a sort and wb_boxes_launch.
        nms: a boxes.Suppression: only the detections non-maximum suppression keeps -- by the flags
        the device left on routes 1 and 2, otherwise of each image's complete result (_suppress)."""
        m, n, Cc = self.shape
        if single and finished is None and fetch_final:
            finished = eng.fetch_final(dm, stt, nms=nms)
        ordered = None
        if not single and _orders_batch(eng):
            ordered = eng.fetch_ordered_batch(dm, stt, ordered_enqueued, nms)
        if finished is not None:
            out, alive = [from_finished(finished, windows)], finished.alive
        elif ordered is not None:
            per_image, alive = ordered
            out = [from_image_result(item, windows) for item in per_image[:count]]
        else:
            got = eng.fetch(dm, stt, limit=_HOST_POST_MAX if single else _HOST_POST_BATCH)
            alive = got.alive
            if got.records is not None:
                out = from_packed(got.records, count, m, n, eng.inv_scales(), one_slot=eng.batch == 1)
            else:
                out = from_ordered(*eng.ordered_host(dm, got.total), count)
        if stt.n_loc is None:
            stt.n_loc = eng.plan.n_loc(m, n)
        self.n_loc += count * stt.n_loc
        self.n_weak += int(alive[:count].sum())
        if nms is not None:
            out = [_suppress(res, nms) for res in out]
        return out, alive

    def detect_stream(self, images, lanes=3, batch=1, iou_threshold=None, score_threshold=None):
        """detect() over an iterable of 2-D images, as a generator of Boxes in the iterable's order -- the loop the
        reference's detection script runs (scripts/waldboost-detect.py:64-67), pipelined: `lanes` engines, each on its
        own stream, hold consecutive images, so image i + 1 is uploaded and image i - 1's detections are read back and
        ordered on the host while image i is scanned (a single detect() call is three quarters upload, waits and host
        work: DESIGN section 5).  Same results, same n_loc / n_weak updates as one detect() call per image.
        batch: consecutive images of one shape and dtype are gathered `batch` at a time and go through every kernel in
        one launch (a shape change or the end of the iterable sends a partly filled batch); ordering and boxes of a
        batch are computed on the device.  Up to lanes * batch - 1 images are taken from the iterable ahead of the one
        whose Boxes are being yielded.
        iou_threshold, score_threshold: as for detect -- every image's result after non-maximum suppression, which is
        enqueued on the lane's stream right behind the image's (or the batch's) scan and ordering, in front of the
        lane's one wait.
        (Measured and left out: the blocking upload on a helper thread -- 0.13 to 0.16 ms per 1080p image against 0.14 to
        0.15 without: what the copy frees, the two threads lose again handing the interpreter lock back and forth.)"""
        global _torch
        import torch as _torch
        lanes, K = max(int(lanes), 1), max(int(batch), 1)
        nms = suppression(iou_threshold, score_threshold)
        shrink, n_per_oct, smooth, spec = _channels.read_opts(self.channel_opts, allow_callable=True)
        if spec is None:                      # (a caller's own channel function runs on the host between the GPU steps)
            for image in images:
                yield self.detect(image, iou_threshold, score_threshold)
            return
        m, n, Cc = self.shape
        assert Cc == spec.n_channels, f"Invalid number of channels. Expected {Cc} given {spec.n_channels}."

        def items():
            """(what a lane must have been built for, the cascade as it is now, the image) per image"""
            for image in images:
                _channels._validate_image(image, allow_tensor=True)
                H, W = map(int, image.shape)
                yield (H, W, _engine.array_dtype(image).str, shrink, n_per_oct, smooth, spec.key, K), self.device_cascade(), image

        def new_lane(key, image):
            H, W = (int(x) for x in image.shape)
            return _Lane(_engine.PyramidEngine(H, W, _engine.array_dtype(image), shrink, n_per_oct, smooth, K, channels=spec),
                         _torch.cuda.Stream())

        pool = getattr(self, "_lanes", None)                  # key -> [_Lane]
        if pool is None:                                      # (a copy: __getstate__ leaves the lanes behind)
            pool = self._lanes = {}
        yield from Schedule(pool, lanes, K, new_lane, lambda image: self.detect(image, iou_threshold, score_threshold),
                            self, nms).run(items())

    def detect_batch(self, images, iou_threshold=None, score_threshold=None):
        """detect() on a batch: `images` is [B,H,W] (ndarray or device tensor) of one shape and dtype;
        the whole batch goes through each kernel in one launch.  Returns a list of B Boxes (same
        content and order as B calls of detect) and updates n_loc / n_weak.
        iou_threshold, score_threshold: as for detect, per image (one wb_nms_finish_launch for the whole batch behind the
        ordering launch, in front of the one wait)."""
        out, _, _ = self._detect_batch(images, suppression(iou_threshold, score_threshold), windows=False)
        return [_as_boxes(res) for res in out]

    def detect_batch_raw(self, images, _nms=None):
        """All detections of a batch as flat arrays (image, level, r, c, boxes, scores, alive[B,L,T])."""
        out, alive, scales = self._detect_batch(images, _nms and suppression(*_nms))
        level, r, c = (np.concatenate(w) for w in zip(*(res.windows() for res in out)))
        return dict(batch=len(out), image=np.repeat(np.arange(len(out), dtype=np.int32), [res.scores.size for res in out]),
                    level=level, r=r, c=c, boxes=np.concatenate([res.boxes for res in out]),
                    scores=np.concatenate([res.scores for res in out]), alive=alive, scales=list(scales))

    def _detect_batch(self, images, nms, windows=True):
        """A batch -> ([Detections per image], alive[B, L, T], the levels' scales); updates n_loc / n_weak."""
        if getattr(images, "ndim", None) != 3 and (not hasattr(images, "dim") or images.dim() != 3):
            raise ValueError("images must have 3 dimensions [B,H,W]")
        B, H, W = (int(x) for x in images.shape)
        dtype = _engine.array_dtype(images)
        shrink, n_per_oct, smooth, spec = _channels.read_opts(self.channel_opts)
        m, n, Cc = self.shape
        assert Cc == spec.n_channels, f"Invalid number of channels. Expected {Cc} given {spec.n_channels}."
        dm = self.device_cascade()
        eng = _engine.get_engine(H, W, dtype, shrink, n_per_oct, smooth, B, channels=spec)
        if eng.plan.n_levels == 0:
            return [Detections.none() for _ in range(B)], np.zeros((B, 0, len(self)), np.int64), []
        eng.load_images(images)
        out, alive = self._assemble(eng, dm, eng.run(dm), B, nms, windows=windows)
        return out, alive, eng.plan.scales

    def predict(self, X):
        """The cascade on samples X[N, m, n, C] -> (H, mask): H[i] is the response accumulated in stage
        order while sample i is alive and -inf once a stage rejected it, mask[i] whether it passed
        every stage (reference model.py:181-214; the training pool re-scores its samples with it)."""
        import torch
        n, *shape = X.shape
        assert tuple(shape) == tuple(self.shape), f"Invalid shape of X. Expected {self.shape}, given {shape}"
        if n == 0:
            return np.zeros(0, np.float32), np.ones(0, bool)
        dm = self.device_cascade()
        dev = nat.require_gpu()
        Xd, wdt = channel_tensor(X, dev)
        H = torch.empty(n, dtype=torch.float32, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        nat.launch("wb_samples_predict_launch", dm.handle, Xd, wdt, n, H, mask)
        return H.cpu().numpy(), mask.cpu().numpy().astype(bool)

    def stage_scores(self, X, reject=False, device=False):
        """The running score of every sample of X[N, m, n, C] after every stage -> (N, T) float32: entry [i, t] is
        ``h = h + pred`` accumulated in fp32 over stages 0 .. t, from 0 (wb_samples_trace_launch; the result is the
        transpose view of the stage-major device trace).  X: an ndarray or device tensor of any dtype
        compare.channel_tensor takes.  reject=False: the thetas are ignored; True: they apply as in predict -- from the
        rejecting stage on a sample's entries are -inf, so ``stage_scores(X, reject=True)[:, -1]`` is ``predict(X)[0]``
        bit for bit.  device=True: a device tensor.  ValueError when N * T >= 2**31 or X has another sample shape.
        What calibration.calibrate prunes the thetas with."""
        from . import calibration
        return calibration.stage_scores(self, X, reject, device)

    # ---- wire format (reference model.py:285-344)
    def as_proto(self, proto):
        proto.Clear()
        proto.shape.extend(int(x) for x in self.shape)
        proto.channel_opts.shrink = self.channel_opts["shrink"]
        proto.channel_opts.n_per_oct = self.channel_opts["n_per_oct"]
        proto.channel_opts.smooth = self.channel_opts["smooth"]
        proto.channel_opts.func = symbol_name(self.channel_opts["channels"])
        for weak, theta in self:
            w_pb = proto.classifier.add()
            weak.as_proto(w_pb)
            proto.theta.append(float(theta))

    @staticmethod
    def from_proto(proto):
        shape = tuple(proto.shape)
        channel_opts = {
            "shrink": proto.channel_opts.shrink,
            "n_per_oct": proto.channel_opts.n_per_oct,
            "smooth": proto.channel_opts.smooth,
            "channels": symbol_from_name(proto.channel_opts.func),
        }
        M = Model(shape, channel_opts)
        for weak_proto, theta_proto in zip(proto.classifier, proto.theta):
            M.append(DTree.from_proto(weak_proto), theta_proto)
        return M

    def save(self, filename):
        proto = model_pb2.Model()
        self.as_proto(proto)
        data = zlib.compress(proto.SerializeToString(), 9)
        with open(filename, "wb") as f:
            f.write(data)

    @staticmethod
    def load(filename):
        with open(filename, "rb") as f:
            data = f.read()
        proto = model_pb2.Model()
        try:
            data = zlib.decompress(data)
            proto.ParseFromString(data)
        except (DecodeError, zlib.error):
            raise ValueError(f"Cannot read model from {filename}")
        return Model.from_proto(proto)


class _SingleLevel:
    """Device state for Model.predict_on_image on a caller-supplied HWC channel image."""
    _cache = {}

    @classmethod
    def get(cls, u, v, C, dtype=np.float32):
        import torch
        dtype = np.dtype(dtype)
        key = (u, v, C, dtype.str, torch.cuda.current_device() if torch.cuda.is_available() else -1)
        e = cls._cache.get(key)
        if e is None:
            if len(cls._cache) >= 8:
                cls._cache.pop(next(iter(cls._cache)))
            e = cls._cache[key] = cls(u, v, C, dtype)
        return e

    def __init__(self, u, v, C, dtype=np.float32):
        import torch
        self.dev = nat.require_gpu()
        if u >= 65536 or v >= 65536:
            raise ValueError("channel image larger than 65535 pixels per side")
        self.u, self.v, self.C = u, v, C
        t = np.zeros(1, nat.LEVEL_DTYPE)
        t[0]["u"], t[0]["v"], t[0]["chn_off"] = u, v, 0
        self.levels = torch.from_numpy(t.view(np.uint8).copy()).to(self.dev)
        self.dtype = np.dtype(dtype)
        self.tdtype, self.wb_dtype = nat.window_codes(self.dtype)
        self.X = torch.empty((max(u * v * C, 1) + 16,), dtype=self.tdtype, device=self.dev)   # + spare bytes (see wb_cascade_launch)
        self.detb = _engine.DetBuffer(1 << 10, self.dev)
        self._tiles = {}

    def load(self, X):
        import torch
        if nat.is_tensor(X):
            self.X[:self.u * self.v * self.C].copy_(X.to(self.tdtype).reshape(-1))
        else:
            self.X[:self.u * self.v * self.C].copy_(torch.from_numpy(np.ascontiguousarray(X, self.dtype).reshape(-1)))

    def scan(self, dm):
        import torch
        from .plan import PyramidPlan
        key = (dm.m, dm.n, dm.tile_rows, dm.tile_cols, dm.n_stages)
        T = dm.n_stages
        if key not in self._tiles:
            tl = PyramidPlan._tiles([(max(self.u - dm.m, 0), max(self.v - dm.n, 0))], dm.tile_rows, dm.tile_cols)
            self._tiles = {key: (int(tl.size), torch.from_numpy(tl.view(np.uint8).copy()).to(self.dev) if tl.size else None)}
        n_tiles, tiles = self._tiles[key]
        alive = torch.empty((1, 1, max(T, 1)), dtype=torch.int32, device=self.dev)
        while True:
            self.detb.zero()
            alive.zero_()
            if n_tiles:
                nat.launch("wb_cascade_launch", dm.handle, self.X, self.wb_dtype, 0, 1, self.levels, 1, tiles, n_tiles, self.detb.recs,
                           self.detb.counts, self.detb.cap, alive)
            need = self.detb.max_count()
            if need <= self.detb.cap:
                break
            self.detb = _engine.DetBuffer(int(need * 1.5) + 16, self.dev)
        n = int(self.detb.counts.sum().item())
        return n, alive[0, 0, :T].cpu().numpy().astype(np.int64)

    def sorted(self, n):
        return _engine.sort_records(self.detb.compact())
