"""Device-side execution of the hot path: buffers, launches, hipGraph capture.

``PyramidEngine`` owns the HBM-resident state of one (image shape, dtype, channel_opts,
batch) configuration and drives the three kernel groups through the C ABI:

    octaves (wb_octaves_launch) -> channels (wb_channels_launch) -> cascade (wb_cascade_launch)

torch is used only for device memory, streams and graph capture; all compute is in
csrc/*.hip.  Nothing here falls back to the CPU.
"""
import contextlib
import ctypes as C
import dataclasses
import logging
import os
import weakref

import numpy as np

from . import _native as nat
from .chanfunc import SPECS
from .plan import PyramidPlan, N_CHANNELS
from .readback import FinishBlock, Finished, ImageResult, Packed, key_fits

_TORCH_DT = {}
_log = logging.getLogger("waldboost_amd")


@contextlib.contextmanager
def capturing(graph, **kw):
    """``torch.cuda.graph(graph, **kw)`` with Python's cyclic collector out of the way.  An object it happens to free in
    the middle of a stream capture -- a page-locked tensor (its allocator records events), another engine's CUDAGraph,
    a stream -- makes HIP calls that invalidate the capture ("operation failed due to a previous error during capture");
    torch no longer collects on entry by itself (>= 2.9).  So: collect first, then keep the collector off until the
    capture has ended."""
    import gc
    import torch
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if was:
            gc.enable()

_NO_DETECT_GRAPH = bool(int(os.environ.get("WB_NO_DETECT_GRAPH", "0")))
_NO_RANKS = bool(os.environ.get("WB_NO_RANKS"))     # diagnostic: float32 channels + planar float tile everywhere
# Model-specialised cascade kernels (csrc/wb_jit.hip): a cascade that has been scanned this many times on byte tiles is
# compiled with its stage records as constants (hiprtc, ~2 s once; cached on disk).  WB_CASC_JIT=0: never automatically
# (DeviceCascade.specialize() still works), WB_CASC_JIT_AFTER=n: after n scans (default 3).
# A freshly specialised cascade kernel is cross-checked against the generic kernel on the first real image it meets (this
# many times; 0 = never): the library's self-test (wb_model_specialize) runs on synthetic bytes, this one on the caller's.
_LIVE_CHECKS = int(os.environ.get("WB_JIT_LIVE_CHECKS", "2"))
_CHECK_KEYS = bool(os.environ.get("WB_CHECK_KEYS"))         # diagnostic: verify the clean-keys flag against the device before every fused step
_NO_FUSED_RESET = bool(os.environ.get("WB_NO_FUSED_RESET"))   # diagnostic: one memset launch per step, as before
_JIT_AUTO = os.environ.get("WB_CASC_JIT", "1") != "0"
_JIT_AFTER = int(os.environ.get("WB_CASC_JIT_AFTER", "3"))
_FORCE_RANK16 = bool(os.environ.get("WB_FORCE_RANK16"))   # diagnostic / bench: 16-bit ranks also where a byte would do


def _torch_dtype(np_dtype):
    import torch
    if not _TORCH_DT:
        _TORCH_DT.update({np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32,
                          np.dtype(np.float64): torch.float64})
    try:
        return _TORCH_DT[np.dtype(np_dtype)]
    except KeyError:
        raise NotImplementedError(f"dtype {np.dtype(np_dtype)} has no HIP kernel") from None


# Image dtypes (reference channels.py:122 keeps image.dtype through the pyramid): uint8 and float32 have their own
# kernels; float64 and the integer types whose values are exact in float64 are held as float64 on the device, with
# a code that tells the kernels how avg_pool_2 wraps and how the resize result is cast back (waldboost_hip.h).
_IMAGE_CODES = {np.dtype(np.uint8): (np.uint8, nat.WB_DTYPE_U8), np.dtype(np.float32): (np.float32, nat.WB_DTYPE_F32),
                np.dtype(np.float64): (np.float64, nat.WB_DTYPE_F64), np.dtype(np.int8): (np.float64, nat.WB_DTYPE_I8),
                np.dtype(np.int16): (np.float64, nat.WB_DTYPE_I16), np.dtype(np.uint16): (np.float64, nat.WB_DTYPE_U16),
                np.dtype(np.int32): (np.float64, nat.WB_DTYPE_I32), np.dtype(np.uint32): (np.float64, nat.WB_DTYPE_U32),
                # (int64 / uint64: only values exact in float64 -- load_images checks; bool adds are logical ors; every
                # float16 add rounds to float16)
                np.dtype(np.int64): (np.float64, nat.WB_DTYPE_I64), np.dtype(np.uint64): (np.float64, nat.WB_DTYPE_U64),
                np.dtype(np.bool_): (np.float64, nat.WB_DTYPE_BOOL), np.dtype(np.float16): (np.float64, nat.WB_DTYPE_F16)}


def image_code(np_dtype):
    """(storage dtype on the device, WB_DTYPE_* code) of an image dtype; NotImplementedError if it has no kernel."""
    try:
        return _IMAGE_CODES[np.dtype(np_dtype)]
    except KeyError:
        raise NotImplementedError(
            f"image dtype {np.dtype(np_dtype)} has no HIP kernel (uint8, float16 / 32 / 64, bool and the 8 to 64 bit "
            "integers are supported)") from None


def array_dtype(images):
    """NumPy dtype of an image batch given as an ndarray or a torch tensor, checked against the kernels' image types
    (NotImplementedError otherwise -- raised before any launch or collective)."""
    dt = images.dtype if isinstance(images, np.ndarray) else nat.dtype_name(images)
    try:
        dt = np.dtype(dt)
    except TypeError:
        raise NotImplementedError(f"image dtype {images.dtype} has no HIP kernel") from None
    image_code(dt)
    return dt


def orientation_constants():
    """cos/sin of the 4 unsigned orientations, built exactly as reference channels.py:43-46
    builds them (NumPy fp64; note cos(pi/2) = 6.1e-17, not 0)."""
    theta = np.linspace(0, np.pi, N_CHANNELS + 1)
    return np.concatenate([np.cos(theta[:-1]), np.sin(theta[:-1])]).astype(np.float64)


def theta_as_f32(theta):
    """The fp32 value t such that ``hs >= theta`` (NumPy-2 promotion) == ``hs >= t`` for every
    fp32 ``hs``.  Python floats are weak scalars (rounded to fp32 by NumPy); NumPy fp64/int
    scalars force an fp64 comparison, which equals comparing with the smallest fp32 >= theta."""
    if isinstance(theta, (np.float32, np.float16)):
        return np.float32(theta)
    if type(theta) in (float, int, bool):
        with np.errstate(over="ignore"):
            return np.float32(theta)
    t64 = np.float64(theta)
    if np.isnan(t64):
        return np.float32(np.nan)
    with np.errstate(over="ignore"):
        t32 = np.float32(t64)
    if np.float64(t32) < t64:
        t32 = np.nextafter(t32, np.float32(np.inf))
    return t32


class DeviceCascade:
    """A WbModel handle built from the Python-side stage list (immutable snapshot)."""

    def __init__(self, shape, classifier, theta):
        lib = nat.load()
        nat.require_gpu()
        m, n, Cc = (int(x) for x in shape)
        T = len(classifier)
        node_off = np.zeros(T + 1, np.int32)
        for i, w in enumerate(classifier):
            node_off[i + 1] = node_off[i] + w.left.size
        cat = lambda name, dt: (np.ascontiguousarray(np.concatenate([getattr(w, name).reshape(-1) for w in classifier]).astype(dt))
                                if T else np.zeros(0, dt))
        feature = cat("feature", np.uint8)
        threshold = cat("threshold", np.float32)
        left = cat("left", np.int8)
        right = cat("right", np.int8)
        pred = cat("prediction", np.float32)
        th = np.array([theta_as_f32(t) for t in theta], np.float32)
        h = C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        nat.call("wb_model_create", T, vp(node_off), vp(feature), vp(threshold), vp(left), vp(right), vp(pred), vp(th), m, n, Cc, C.byref(h))
        # whose rank tables this cascade scans: its own (a RankGroup's for a member view).  An opaque token, compared by
        # identity -- never the cascade or the group itself: a self-reference (or view -> group -> views) is a cycle, and
        # a cycle's __del__ (wb_model_destroy / wb_rankgroup_destroy: hipFree) would run whenever the cyclic collector
        # happens to, e.g. inside somebody's stream capture or between a lane's enqueue and collect
        self._setup(lib, h, True, object())

    def _setup(self, lib, handle, owned, rank_key):
        """What a cascade of its own and a group's member view share: the handle, the per-instance bookkeeping, the info."""
        self._lib, self.handle, self._owned, self.rank_key = lib, handle, owned, rank_key
        self._scans = {}                 # byte-tile scans so far, per channel dtype code
        self._jit_failed = set()
        self._live_left = {}             # live checks a freshly specialised kernel still owes, per channel dtype code
        self._spec_off = False           # use_specialized(False) is in force
        self._form_rows = {}             # form_rows, per channel dtype code
        info = nat.WbModelInfo()
        nat.call("wb_model_info", self.handle, C.byref(info))
        self.n_stages, self.depth = info.n_stages, info.depth
        self.m, self.n, self.C = info.m, info.n, info.C
        self.tile_rows, self.tile_cols, self.lds_bytes = info.tile_rows, info.tile_cols, info.lds_bytes
        # the model's thresholds fit rank tables: the channel kernel can write float32 channels as one-byte ranks
        # (WB_DTYPE_RANK8) and the cascade scan them exactly as it would the floats, from a quarter of the bytes
        self.rank_ok = bool(info.rank_ok)
        # ... or, with more thresholds per channel than a byte ranks (long soft cascades), as two-byte ranks (WB_DTYPE_RANK16)
        self.rank16_ok = bool(info.rank16_ok)
        # the rank form the detection path uses for this cascade (None: float32 channels)
        self.rank_dtype = (nat.WB_DTYPE_RANK16 if (self.rank16_ok and (_FORCE_RANK16 or not self.rank_ok)) else
                           nat.WB_DTYPE_RANK8 if self.rank_ok else None)

    @classmethod
    def _view(cls, handle, group):
        """A member view of a RankGroup: same interface, handle owned by the group."""
        self = cls.__new__(cls)
        self.group = group               # keeps the handle's owner alive; the group does NOT refer back to its views
        self._setup(nat.load(), handle, False, group.token)      # (a token, not the group: see __init__)
        return self

    def form_rows(self, chn_dtype):
        """Window rows of the tile the kernel for channels of chn_dtype scans per workgroup (wb_model_form_rows): tile_rows,
        or a multiple of it on the one-byte forms."""
        rows = self._form_rows.get(chn_dtype)
        if rows is None:
            r = C.c_int()
            nat.call("wb_model_form_rows", self.handle, chn_dtype, C.byref(r), None)
            rows = self._form_rows[chn_dtype] = r.value
        return rows

    def specialized(self):
        """Which byte tiles have a model-specialised kernel loaded: subset of {WB_DTYPE_U8, WB_DTYPE_RANK8, WB_DTYPE_RANK16}."""
        info = nat.WbModelInfo()
        nat.call("wb_model_info", self.handle, C.byref(info))
        return {d for bit, d in ((1, nat.WB_DTYPE_U8), (2, nat.WB_DTYPE_RANK8), (4, nat.WB_DTYPE_RANK16)) if info.specialized & bit}

    def specialize(self, chn_dtype=None):
        """Compile and load the model-specialised tile kernel (wb_model_specialize) for a kind of byte tile: the threshold
        ranks by default when the model has rank tables, else uint8 channels.  Returns False when this model has no
        specialised kernel (node-walk models, cascades beyond the LDS mirror); raises NativeError if the compiler fails."""
        if chn_dtype is None:
            chn_dtype = self.rank_dtype if self.rank_dtype is not None else nat.WB_DTYPE_U8
        had = chn_dtype in self.specialized()
        rc = self._lib.wb_model_specialize(self.handle, chn_dtype)
        if rc == nat.WB_ERR_UNSUPPORTED:
            return False
        nat.check(rc, "wb_model_specialize")
        if not had:
            self._live_left[chn_dtype] = _LIVE_CHECKS      # (PyramidEngine.live_check)
        return True

    def use_specialized(self, enable):
        """The loaded specialised kernels on / off for every later scan of this cascade (off: the generic kernel)."""
        nat.call("wb_model_use_specialized", self.handle, 1 if enable else 0)
        self._spec_off = not enable

    def live_checks_left(self, chn_dtype):
        return 0 if self._spec_off else self._live_left.get(chn_dtype, 0)

    def take_live_check(self, chn_dtype, all_left=False):
        """Consume one of the live checks owed for this tile kind (all_left: every one -- the kernel has been switched
        off); False when none was left."""
        left = self._live_left.get(chn_dtype, 0)
        self._live_left[chn_dtype] = 0 if all_left else max(left - 1, 0)
        return left > 0

    def note_scan(self, chn_dtype, force=False):
        """Called by the engine before a scan on byte tiles: after _JIT_AFTER scans (force: now -- Model.detect is about
        to capture its graph) the cascade is worth specialising.  Never inside a stream capture (compilation and module
        loading are not capturable), never twice after a failure."""
        if not _JIT_AUTO or chn_dtype == nat.WB_DTYPE_F32 or chn_dtype in self._jit_failed:
            return
        n = self._scans.get(chn_dtype, 0) + 1
        if force and n < _JIT_AFTER:
            n = _JIT_AFTER
        self._scans[chn_dtype] = n
        if n == _JIT_AFTER:
            import torch
            if torch.cuda.is_current_stream_capturing():
                self._scans[chn_dtype] = n - 1
                return
            try:
                if not self.specialize(chn_dtype):
                    self._jit_failed.add(chn_dtype)
                    # (said once per cascade and tile kind: the generic kernel is ~10 % slower at batch 1)
                    _log.info("cascade of %d stages, depth %d: no model-specialised kernel for this model (%s); staying on "
                              "the generic tile kernel", self.n_stages, self.depth, nat.last_error())
            except nat.NativeError as exc:
                self._jit_failed.add(chn_dtype)      # (stay on the generic kernel)
                _log.warning("cascade of %d stages, depth %d: building the model-specialised kernel failed, staying on the "
                             "generic tile kernel (slower): %s", self.n_stages, self.depth, exc)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self._owned:
                self._lib.wb_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class RankGroup:
    """Several cascades over ONE pyramid of threshold ranks (wb_rankgroup_create): the rank table of every channel is
    built from the union of the members' thresholds; ``view(i)`` is member i as a DeviceCascade whose rank tables are the
    group's.  Raises NotImplementedError when the union does not fit (more than 255 thresholds on a channel).
    Ownership runs one way -- view -> group -> member cascades -- so that a group nobody scans with any more is freed
    by reference counting, at once (its __del__ issues hipFree calls: not something to leave to the cyclic collector)."""

    def __init__(self, cascades):
        lib = nat.load()
        self._lib = lib
        self.members = list(cascades)                      # (the models must outlive the group)
        arr = (C.c_void_p * len(self.members))(*[dm.handle.value for dm in self.members])
        h = C.c_void_p()
        nat.call("wb_rankgroup_create", arr, len(self.members), C.byref(h))
        self.handle = h
        self.token = object()              # what the engine's rank buffer is tagged with (DeviceCascade.rank_key)

    def view(self, i):
        v = C.c_void_p()
        nat.call("wb_rankgroup_model", self.handle, i, C.byref(v))
        return DeviceCascade._view(v, self)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.wb_rankgroup_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class GroupViews:
    """What rank_group hands out: the group's member views (stable objects: the engine keys its scan states by them)."""

    def __init__(self, group):
        self.group = group
        self.members = group.members
        self.views = [group.view(i) for i in range(len(group.members))]


_GROUPS = {}


def rank_group(cascades):
    """The (cached) member views of the RankGroup of these cascades, or None when they cannot share a rank table."""
    key = tuple(id(dm) for dm in cascades)
    g = _GROUPS.get(key)
    if g is None or (g and any(a is not b for a, b in zip(g.members, cascades))):
        try:
            g = GroupViews(RankGroup(cascades))
        except NotImplementedError:
            g = False
        if len(_GROUPS) >= 8:
            _GROUPS.pop(next(iter(_GROUPS)))
        _GROUPS[key] = g
    return g or None


class DetBuffer:
    """Sharded append buffer of WbDet records (include/waldboost_hip.h: WB_DET_SHARDS regions of `cap` records,
    one counter each).  `counts` may be a view the caller provides -- PyramidEngine keeps the counters in its
    control block, so that ONE memset per step resets them together with the other accumulators."""

    def __init__(self, cap, dev, counts=None):
        import torch
        self.NS = nat.WB_DET_SHARDS
        self.cap = int(cap)
        self.counts = counts if counts is not None else torch.zeros(self.NS, dtype=torch.int32, device=dev)
        self.recs = torch.zeros((self.NS * self.cap, 4), dtype=torch.int32, device=dev)

    def zero(self):
        self.counts.zero_()

    def max_count(self):
        return int(self.counts.max().item())

    def compact(self):
        """All valid records as one int32 [n, 4] tensor (shard order)."""
        import torch
        ar = torch.arange(self.cap, device=self.recs.device, dtype=torch.int32)
        mask = ar[None, :] < self.counts[:, None].clamp(max=self.cap)
        return self.recs.view(self.NS, self.cap, 4)[mask]


def sort_records(d):
    """Records ordered by (image, level, r, c) -- the reference's output order (row-major window
    grid, levels in pyramid order)."""
    import torch
    if d.shape[0] == 0:
        return d
    rc = d[:, 2].to(torch.int64) & 0xFFFFFFFF
    key = (d[:, 0].to(torch.int64) << 44) | (d[:, 1].to(torch.int64) << 32) | ((rc & 0xFFFF) << 16) | (rc >> 16)
    return d[torch.argsort(key)].contiguous()


class CapturedStep:
    """A hipGraph of one engine's step (PyramidEngine.capture).  The graph holds device ADDRESSES: of the control block
    and of the detection buffer, both of which the engine re-allocates when they must grow.  replay() refuses to run
    a graph captured before such a re-allocation (it would add into freed memory) -- capture again."""

    def __init__(self, engine, graph):
        # (a weak reference: an engine that keeps its own captured step -- batch_enqueue -- must not become a reference
        # cycle, to be freed by the collector at some arbitrary later moment)
        self._engine, self.graph, self.generation = weakref.ref(engine), graph, engine.generation

    @property
    def engine(self):
        return self._engine()

    def replay(self):
        if self.engine is None:
            raise RuntimeError("this captured step's engine no longer exists")
        if self.generation != self.engine.generation:
            raise RuntimeError("this captured step is stale: the engine re-allocated its control block or detection "
                               "buffer after the capture (a longer cascade, or a grown detection buffer); capture again")
        self.engine.ensure_clean_keys()          # (the graph holds no memset: see PyramidEngine.run)
        self.graph.replay()


@dataclasses.dataclass(eq=False)
class NmsBuffers:
    """What wb_nms_finish_launch needs for `images` finish blocks of `rows` rows; a scan state or the batch's order
    buffers hold one."""
    rows: int
    images: int
    scratch: object                  # device
    res: object                      # device: per image 16 bytes of info + `rows` keep flags
    h_res: object                    # its page-locked copy
    h: np.ndarray                    # ... as uint8 [images, 16 + rows]


@dataclasses.dataclass(eq=False)
class FinalBuffers:
    """The one-image finish read-back of a scan state: finish block | alive[B, L, T], one copy."""
    dev: object                      # device block
    host: object                     # its page-locked copy
    views: tuple                     # FinishBlock.views of the copy: (header, keys, boxes, scores)
    alive: np.ndarray                # the copy's alive[B, L, T], int32


@dataclasses.dataclass(eq=False)
class ScanState:
    """What an engine keeps per cascade it scans (PyramidEngine._casc_state).  None: not there (yet, or any more)."""
    dm: DeviceCascade                # (held: the states are keyed by id(dm))
    tiles: object                    # the cascade's tile list on the device (None: no tile): every unit of tile_rows
    n_tiles: int
    tall: dict                       # rows -> (tile list, count) of a form whose tile is taller (DeviceCascade.form_rows)
    alive: object                    # alive[B, L, T]: a view into the control block
    ranks: bool = False              # the form of the last scan (a re-scan after a buffer overflow repeats it)
    graph: object = None             # detect_enqueue's captured sequence        } dropped by
    step: CapturedStep = None        # batch_enqueue's captured step             } PyramidEngine._buffers_moved
    detect_calls: int = 0
    batch_calls: int = 0
    n_loc: int = None                # plan.n_loc of the cascade's window (Model._assemble)
    final: FinalBuffers = None
    nms: NmsBuffers = None

    def __getitem__(self, name):
        return getattr(self, name)   # (bench.py reads e._casc_state(dm)["alive"])


@dataclasses.dataclass(eq=False)
class OrderBuffers:
    """The batch's ordered read-back (fetch_ordered_batch).  fits False: the form does not apply, nothing else is set."""
    fits: bool
    scratch: object = None           # device
    out: object = None               # device: 16 bytes of info | one finish block per image
    h_out: object = None             # its page-locked copy
    ev: object = None                # recorded behind the copies
    info: np.ndarray = None          # the copy's info words, int32
    views: list = None               # per image FinishBlock.views of the copy
    nms: NmsBuffers = None


@dataclasses.dataclass(eq=False)
class MultiState:
    """One cascade list's sequence in detect_multi_run."""
    stts: list                       # the scan states it was built on
    dms: list                        # (held: the sequences are keyed by id(dm))
    calls: int = 0
    graph: object = None
    skip: int = 0                    # calls left to sit out after its results did not fit
    fails: int = 0


def checked_input(images, dtype, store_dtype, want):
    """The host or device tensor to copy into an engine's image buffer: `images` (ndarray or tensor, of the engine's image
    dtype `dtype`) as a tensor of shape `want` -- [B, H, W], which a 2-D image also fills when B is 1, or [H, W] for one
    slot -- of the storage dtype (integer types travel as float64: exact); a contiguous ndarray of that dtype is not
    copied.  Checked in this order: the dtype (TypeError), the shape (ValueError), the range of 64-bit integers
    (NotImplementedError: they are held as float64, exact -- also their 2x2 sums -- below 2**51)."""
    import torch
    host = isinstance(images, np.ndarray)
    if (images.dtype if host else array_dtype(images)) != dtype:
        raise TypeError(f"engine built for {dtype} images, got {images.dtype}")
    shape = tuple(images.shape)
    if shape != want and (len(want) != 3 or (1,) + shape != want):
        raise ValueError(f"expected images of shape {want}, got {shape}")
    if len(shape) < len(want):
        images = images[None]
    t = torch.from_numpy(np.ascontiguousarray(images, store_dtype)) if host else images.to(_torch_dtype(store_dtype))
    # (as float64 already: a 64-bit integer is below 2**51 exactly when the float64 nearest to it is)
    if dtype.itemsize == 8 and dtype.kind in "iu" and t.numel() and float(t.abs().max()) >= float(1 << 51):
        raise NotImplementedError("64 bit integer images are supported for values below 2**51 (they are held as float64)")
    return t


def alive_host(alive, T):
    """alive[B, L, :T] of a scan -- device tensor, page-locked tensor or ndarray -- as a fresh int64 ndarray."""
    a = alive if isinstance(alive, np.ndarray) else alive.cpu().numpy()
    return a[:, :, :T].astype(np.int64)


class PyramidEngine:
    # detection records read back with the first copy of fetch() / the one copy of fetch_final() (28 bytes each; the
    # copies inside a captured graph have this fixed size).  WB_FETCH_ROWS: diagnostic override
    _FETCH_ROWS = int(os.environ.get("WB_FETCH_ROWS", "4096"))

    def __init__(self, H, W, dtype, shrink, n_per_oct, smooth, batch=1, exact_single=False, det_capacity=1 << 16,
                 channels=None):
        import torch
        self.lib = nat.load()
        self.dev = nat.require_gpu()
        self.dtype = np.dtype(dtype)
        self.spec = channels if channels is not None else SPECS["grad_hist"]
        if self.spec.dtype == np.uint8 and self.dtype != np.uint8:
            raise NotImplementedError(f"{self.spec.key} takes 8 bit images (uint8), got {self.dtype}")
        self.store_dtype, self.wb_dtype = image_code(self.dtype)       # (how the image sits in HBM, what the kernels are told)
        self.store_dtype = np.dtype(self.store_dtype)
        if self.spec.key != "grad_hist" and self.wb_dtype not in (nat.WB_DTYPE_U8, nat.WB_DTYPE_F32):
            raise NotImplementedError(f"{self.spec.key} has kernels for uint8 and float32 images, got {self.dtype}")
        self.tdtype = _torch_dtype(self.store_dtype)
        self.wide_keys = self.store_dtype == np.float64                # 64-bit (min, max) keys per octave
        self.batch = int(batch)
        self.plan = PyramidPlan(H, W, shrink, n_per_oct, smooth, exact_single=exact_single,
                                n_chn=self.spec.n_channels, chn_bytes=self.spec.dtype.itemsize, chan_func=self.spec.func_id)
        self.exact_single = exact_single
        p = self.plan
        p.batch_hint = self.batch     # (the tile lists' dispatch order depends on the images per launch: plan._short_last)
        dev = self.dev
        # flat allocations with 16 spare elements: the channel kernel fetches source rows with
        # 4-byte-aligned dword loads that may touch a few bytes past the last row
        self._img_flat = torch.zeros(self.batch * p.H * p.W + 16, dtype=self.tdtype, device=dev)
        self.img = self._img_flat[: self.batch * p.H * p.W].view(self.batch, p.H, p.W)
        self._oct_flat = torch.zeros(self.batch * p.oct_total + 16, dtype=self.tdtype, device=dev)
        self.oct = self._oct_flat[: self.batch * p.oct_total].view(self.batch, p.oct_total)
        # control block: [per-octave (min, max) keys | detection shard counters | alive[B, L, T]] -- everything the
        # kernels of one step ACCUMULATE into, contiguous, so that one memset at the start of a step resets it all
        # (three separate fills and the statistics reduction used to be four extra launches per image)
        self._mm_words = self.batch * max(p.n_oct, 1) * 2 * (2 if self.wide_keys else 1)
        self._alive_words = 0
        self.generation = 0           # bumped whenever a buffer a captured graph may address is re-allocated
        self._mm_clean = False        # the octaves' (min, max) keys are known to be zero (see run)
        self._casc = {}               # ScanState by id(cascade)
        self._multi = {}              # detect_multi_run's MultiState by cascade list
        self._alloc_ctrl(0)
        table, total = p.level_table()
        self.chn_stride = int(total)
        self.level_np = table
        self.levels = torch.from_numpy(table.view(np.uint8).copy()).to(dev) if p.n_levels else None
        taps, _ = p.tap_table()
        self.taps = torch.from_numpy(taps.view(np.uint8).copy()).to(dev)
        tiles = p.chan_tiles()
        self.n_chan_tiles = int(tiles.size)
        self.chan_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev) if tiles.size else None
        self.chan_patches = self._tile_patches(tiles)
        # (16 spare elements: the cascade's uint8 tile load fetches 16-byte groups that may run past a level row)
        self._chn_flat = torch.zeros(self.batch * self.chn_stride + 16, dtype=_torch_dtype(self.spec.dtype), device=dev)
        self.chn = self._chn_flat[: self.batch * self.chn_stride].view(self.batch, self.chn_stride)
        self.cs_sn = orientation_constants()
        self._oct_off = (C.c_int64 * max(p.n_oct, 1))(*[int(x) for x in p.oct_off[:max(p.n_oct, 1)]])
        self.rank = self.rank_owner = None
        self._rank_wide = False
        self._level_tiles = None
        self.epoch = 0
        self.det_capacity = int(det_capacity)
        self._h_packed = self._h_alive = None
        self._fetch_ev = torch.cuda.Event()                        # what fetch, fetch_final and detect_multi_run wait on
        self._h2d_ev, self._upload_async = torch.cuda.Event(), False       # what wait_upload waits on
        self._mm_host = None
        self._inv_scales_d = self._key_dims = None
        self._order = None            # OrderBuffers of fetch_ordered_batch, on first use
        self._alloc_det()
        if exact_single:
            # a channel function on a bare image: no resize happens, so the clip range is (-inf, +inf)
            if self.wb_dtype == nat.WB_DTYPE_U8:
                lo, hi = 0, 255
            else:
                lo, hi = int(nat_f32_key(-np.inf)), int(nat_f32_key(np.inf))
            if self.wide_keys:
                raise NotImplementedError("channel functions on a bare image take uint8 or float32 arrays")
            self.minmax[:, :, 0] = int(np.array([~np.uint32(lo)], np.uint32).view(np.int32)[0])   # word 0 stores max(~key), see csrc/wb_octaves.hip
            self.minmax[:, :, 1] = int(np.array([hi], np.uint32).view(np.int32)[0])

    def _tile_patches(self, tiles):
        """The per-tile patch table of wb_channels_launch_x for a tile list (uint8 images, the gradient-histogram kernels):
        filled on the host by the library with its own tile geometry, uploaded once.  None: the kernels compute the extents."""
        import torch
        if self.wb_dtype != nat.WB_DTYPE_U8 or not tiles.size or os.environ.get("WB_NO_TILE_PATCHES"):
            return None
        p = self.plan
        tiles = np.ascontiguousarray(tiles)
        out = np.zeros(tiles.size, nat.PATCH_DTYPE)
        rc = self.lib.wb_channels_tile_patches(self.spec.func_id, p.shrink, p.smooth, self.level_np.ctypes.data_as(C.c_void_p),
                                               p.n_levels, tiles.ctypes.data_as(C.c_void_p), int(tiles.size),
                                               out.ctypes.data_as(C.c_void_p))
        if rc == nat.WB_ERR_UNSUPPORTED:
            return None
        nat.check(rc, "wb_channels_tile_patches")
        return torch.from_numpy(out.view(np.uint8).copy()).to(self.dev)

    def _alloc_ctrl(self, alive_words):
        """(Re)allocate the control block with room for `alive_words` statistics words; the views into it follow."""
        import torch
        old = getattr(self, "ctrl", None)
        self._buffers_moved()
        self._casc.clear()            # (every state's alive[] is a view into the old block)
        NS = nat.WB_DET_SHARDS
        self._alive_words = int(alive_words)
        self.ctrl = torch.zeros(self._mm_words + NS + max(self._alive_words, 1), dtype=torch.int32, device=self.dev)
        mm = self.ctrl[: self._mm_words]
        if old is not None:
            mm.copy_(old[: self._mm_words])            # (exact_single keeps a preset clip range there)
        self.minmax = (mm.view(torch.int64) if self.wide_keys else mm).view(self.batch, -1, 2)
        self._counts = self.ctrl[self._mm_words: self._mm_words + NS]
        if getattr(self, "detb", None) is not None:
            self.detb.counts = self._counts

    def _buffers_moved(self):
        """A buffer that captured graphs address -- the control block, the detection buffer, the rank buffer -- has been
        re-allocated.  THE place where the engine's kept graphs die: every scan state's graph and step, every multi-model
        sequence; a CapturedStep a caller holds is refused by its generation stamp."""
        self.generation += 1
        for stt in self._casc.values():
            stt.graph = stt.step = None
        self._multi.clear()

    def _alive_view(self, T1):
        L = max(self.plan.n_levels, 1)
        need = self.batch * L * T1
        if need > self._alive_words:
            self._alloc_ctrl(need)
        o = self._mm_words + nat.WB_DET_SHARDS
        return self.ctrl[o: o + need].view(self.batch, L, T1)

    def reset_step(self, stt=None, octaves=True):
        """ONE memset: the accumulators the coming launches add into -- the octaves' (min, max) keys (unless they
        are preset / not recomputed), the detection counters and, with a cascade state, its alive[B, L, T]."""
        lo = 0 if (octaves and not self.exact_single) else self._mm_words
        hi = self._mm_words + (nat.WB_DET_SHARDS + stt.alive.numel() if stt is not None else 0)
        if hi > lo:
            self.ctrl[lo:hi].zero_()

    def _alloc_det(self):
        """Sharded detection buffer; det_capacity is the total record capacity, split evenly over
        the shards."""
        cap = max(16, -(-self.det_capacity // nat.WB_DET_SHARDS))
        self.det_capacity = cap * nat.WB_DET_SHARDS
        self._buffers_moved()
        self.detb = DetBuffer(cap, self.dev, counts=self._counts)
        self.packed = None            # header + all valid records back to back (wb_det_pack_launch), allocated on first use

    # ------------------------------------------------------------------ input
    def load_images(self, images):
        """images: ndarray / tensor [B,H,W] (or [H,W]) of the engine's dtype."""
        # (a page-locked staging buffer was measured: memcpy + DMA came out 10 % slower per Model.detect call
        # than torch's own pipelined upload from pageable memory; for detect_stream's lanes, where the DMA would
        # overlap other work, the host copy alone -- np.copyto, 45 us -- costs what the pageable upload blocks the
        # host for, 48 us, and torch's multi-threaded CPU copy, 26 us in a tight loop, takes milliseconds once its
        # worker threads have gone to sleep between images: tools/upload_probe.py)
        self._load(self.img, images, (self.batch, self.plan.H, self.plan.W))

    def _load(self, dst, images, want):
        self.epoch += 1                       # (lazy consumers notice that the resident images changed)
        self._upload_async = False
        self._copy_in(dst, checked_input(images, self.dtype, self.store_dtype, want))

    def _copy_in(self, dst, t):
        """Host or device tensor -> resident image buffer on the current stream.  From PAGE-LOCKED host memory (a caller
        that decodes into pinned buffers: torch's pin_memory, hipHostMalloc / hipHostRegister'ed arrays -- asked of the
        driver per call, a microsecond) the copy is a true asynchronous DMA: nothing blocks the host, and the source must
        stay untouched until `wait_upload` (Model.detect returns after the whole call; detect_stream waits before it takes
        the next image from the caller's iterable).  From pageable memory torch stages the bytes itself and the call
        returns once they have left the caller's array (0.05 ms for a 1080p image)."""
        pinned = t.device.type == "cpu" and t.is_pinned()
        dst.copy_(t, non_blocking=True)
        if pinned:
            self._h2d_ev.record()
            self._upload_async = True

    def wait_upload(self):
        """Block until the last asynchronous upload has left the caller's page-locked buffer (no-op otherwise)."""
        if self._upload_async:
            self._h2d_ev.synchronize()
            self._upload_async = False

    def load_slot(self, b, image):
        """One 2-D host image into slot b of the batch (Model.detect_stream fills a batch image by image)."""
        self._load(self.img[b], image, (self.plan.H, self.plan.W))

    # ------------------------------------------------------------------ launches
    def launch_octaves(self, zero=None):
        """zero: a tensor view of accumulator words the launch's first workgroup resets (see run)."""
        p = self.plan
        if p.n_levels == 0 or self.exact_single:
            return
        self._mm_clean = False
        nat.launch("wb_octaves_launch_z", self.img, self.wb_dtype, self.batch, p.H, p.W, p.H * p.W, self.oct, p.oct_total, self._oct_off,
                   p.n_oct, self.minmax, zero, 0 if zero is None else zero.numel())

    def ensure_clean_keys(self):
        """A captured step holds no memset (run): before it is replayed the octaves' keys must be zero -- they are, unless
        something else (a pyramid for a caller, a bare octave launch) has used this engine since the last step."""
        if not self._mm_clean and not self.exact_single:
            self.ctrl[: self._mm_words].zero_()
            self._mm_clean = True
        elif _CHECK_KEYS and not self.exact_single:
            # WB_CHECK_KEYS=1 (the test suite's interleaving test turns it on): the flag is a host-side promise every user
            # of the engine's octaves has to keep -- read the keys back and see that it was kept
            import torch
            if not torch.cuda.is_current_stream_capturing() and bool(self.ctrl[: self._mm_words].any().item()):
                raise RuntimeError("the octaves' (min, max) keys are flagged clean but are not zero: some path used the "
                                   "engine's octaves without going through launch_octaves / clearing _mm_clean")

    def ranks_for(self, dm):
        """True when the fused detection path applies: grad_hist channels written straight as threshold ranks of
        cascade `dm` (float32 channels never reach HBM)."""
        return dm is not None and dm.rank_dtype is not None and self.spec.key == "grad_hist" and not _NO_RANKS

    def scan_dtype(self, dm):
        """The channel dtype code the detection path scans cascade `dm` on: its rank form, or the channel function's."""
        return dm.rank_dtype if self.ranks_for(dm) else self.spec.wb_dtype

    def launch_channels(self, rank_dm=None, floats=True):
        """The channel pyramid of every resident image.  rank_dm: also (floats=False: only) write the channels as
        WB_DTYPE_RANK8 bytes for that cascade into self.rank."""
        import torch
        p = self.plan
        if p.n_levels == 0:
            return
        wide = rank_dm is not None and rank_dm.rank_dtype == nat.WB_DTYPE_RANK16
        if rank_dm is not None and (self.rank is None or self._rank_wide != wide):
            # one byte per value, or two (WB_DTYPE_RANK16); 16 spare elements for the cascade's 16-byte group loads
            flat = torch.zeros(self.batch * self.chn_stride + 16, dtype=torch.int16 if wide else torch.uint8, device=self.dev)
            self.rank = flat[: self.batch * self.chn_stride].view(self.batch, self.chn_stride)
            self._rank_wide = wide
            self._buffers_moved()
        self._channels_call(self.chan_tiles, self.n_chan_tiles, self.chan_patches,
                            self.chn if floats or rank_dm is None else None, rank_dm)
        self.rank_owner = rank_dm.rank_key if rank_dm is not None else None      # whose ranks self.rank holds (None: stale)

    def _channels_call(self, tiles, n_tiles, patches, chn, rank_dm=None):
        """wb_channels_launch_x over a tile list (with its patch table, or None) into `chn` and / or, as ranks of `rank_dm`,
        into self.rank."""
        p = self.plan
        ranked = rank_dm is not None
        nat.launch("wb_channels_launch_x", self.img, p.H * p.W, self.oct, p.oct_total, self.wb_dtype, self.batch, self.levels, p.n_levels,
                   tiles, n_tiles, self.minmax, max(p.n_oct, 1), self.taps, self.spec.func_id, p.shrink, p.smooth,
                   self.cs_sn.ctypes.data_as(C.POINTER(C.c_double)), chn, self.chn_stride, rank_dm.handle if ranked else None,
                   self.rank if ranked else None, self.chn_stride, patches, rank_dm.rank_dtype if ranked else nat.WB_DTYPE_RANK8)

    def launch_level(self, l):
        """The float/uint8 channels of ONE level of every resident image (after launch_octaves): what a lazy
        consumer of the pyramid asks for, level by level (reference channels.py:125-146 computes a level only
        when the generator is advanced to it)."""
        import torch
        p = self.plan
        if self._level_tiles is None:
            tiles = p.chan_tiles()
            self._level_tiles = []
            for k in range(p.n_levels):
                sel = np.ascontiguousarray(tiles[tiles["level"] == k])
                self._level_tiles.append((int(sel.size), torch.from_numpy(sel.view(np.uint8).copy()).to(self.dev) if sel.size else None,
                                          self._tile_patches(sel)))
        n, tiles_d, patches_d = self._level_tiles[l]
        if n == 0:
            return
        self._channels_call(tiles_d, n, patches_d, self.chn)

    # ------------------------------------------------------------------ around a caller's channel function
    def resize_level(self, l):
        """Level l's resized image of resident image 0, cast back to the image dtype, as a host ndarray [nh, nw]
        (reference channels.py:132) -- after launch_octaves."""
        import torch
        rec = np.ascontiguousarray(self.level_np[l:l + 1])
        lv = rec[0]
        nh, nw = int(lv["nh"]), int(lv["nw"])
        if self._mm_host is None or self._mm_host[0] != self.epoch:
            self._mm_host = (self.epoch, self.minmax[0].cpu().numpy().copy())       # (one read-back per image)
        mm = np.ascontiguousarray(self._mm_host[1][int(lv["oct"])])
        out = torch.empty((nh, nw), dtype=self.tdtype, device=self.dev)
        nat.launch("wb_resize_level_launch", self.img, self.oct, self.wb_dtype, rec.ctypes.data_as(C.c_void_p),
                   mm.ctypes.data_as(C.c_void_p), self.taps, out)
        return out.cpu().numpy().astype(self.dtype, copy=False)

    def pool_smooth(self, chns):
        """avg_pool_2 (shrink 2) and smooth_image_3d (smooth 1) of a host array [H, W, C] uint8 / float32 -> host array
        (reference channels.py:138-142)."""
        import torch
        p = self.plan
        H, W, Cn = chns.shape
        code = nat.WB_DTYPE_U8 if chns.dtype == np.uint8 else nat.WB_DTYPE_F32
        d = torch.from_numpy(np.ascontiguousarray(chns)).to(self.dev)
        oh, ow = (H // 2, W // 2) if p.shrink == 2 else (H, W)
        out = torch.empty((oh, ow, Cn), dtype=d.dtype, device=self.dev)
        tmp = torch.empty_like(out) if (p.shrink == 2 and p.smooth) else None
        if H and W and Cn:
            nat.launch("wb_pool_smooth_launch", d, code, H, W, Cn, p.shrink, p.smooth, tmp, out)
        return out.cpu().numpy()

    def _casc_state(self, dm):
        import torch
        key = id(dm)
        stt = self._casc.get(key)
        if stt is None:
            tiles = self.plan.casc_tiles(dm.m, dm.n, dm.tile_rows, dm.tile_cols)
            up = lambda t: torch.from_numpy(t.view(np.uint8).copy()).to(self.dev)
            tall = {}
            for dt in {self.spec.wb_dtype, dm.rank_dtype} - {None}:
                rows = dm.form_rows(dt)
                if tiles.size and rows != dm.tile_rows and rows not in tall:
                    t = self.plan.casc_tiles(dm.m, dm.n, rows, dm.tile_cols, ty_unit=dm.tile_rows)
                    tall[rows] = (up(t), int(t.size))
            T1 = max(dm.n_stages, 1)
            alive = self._alive_view(T1)                # (may re-allocate the control block and drop other states)
            stt = ScanState(dm, up(tiles) if tiles.size else None, int(tiles.size), tall, alive)
            if len(self._casc) >= 4:         # a few cascades resident per engine (waldboost.detect scans several models)
                self._casc.pop(next(iter(self._casc)))
            self._casc[key] = stt
        return stt

    def launch_cascade(self, dm, ranks=False, stats=True, zero_keys=False):
        """The cascade scan, adding into the detection counters and (stats) alive[B, L, T] -- reset_step first.
        ranks=True scans self.rank (written for `dm` by launch_channels) instead of the channel buffer.
        zero_keys: the launch's first workgroup also resets the octaves' (min, max) keys for the next step (see run)."""
        stt = self._casc_state(dm)
        if stt.n_tiles == 0:
            return stt
        if ranks and self.rank_owner is not dm.rank_key:
            raise RuntimeError("the rank buffer does not hold this cascade's ranks (launch_channels(rank_dm=...) first)")
        chn_dtype = dm.rank_dtype if ranks else self.spec.wb_dtype
        dm.note_scan(chn_dtype)
        zk = self.ctrl[: self._mm_words] if zero_keys else None
        tiles, n_tiles = stt.tall.get(dm.form_rows(chn_dtype), (stt.tiles, stt.n_tiles))
        nat.launch("wb_cascade_launch_z", dm.handle, self.rank if ranks else self.chn, chn_dtype, self.chn_stride, self.batch, self.levels,
                   self.plan.n_levels, tiles, n_tiles, self.detb.recs, self.detb.counts, self.detb.cap, stt.alive if stats else None, zk,
                   0 if zk is None else zk.numel())
        if zero_keys:
            self._mm_clean = True
        return stt

    def run_cascade(self, dm, ranks=False):
        """Reset the counters and statistics, then scan every level of every image with cascade `dm`."""
        stt = self._casc_state(dm)
        self.reset_step(stt, octaves=False)
        stt.ranks = ranks                          # (a re-scan after a buffer overflow repeats the same form)
        return self.launch_cascade(dm, ranks=ranks)

    def run_channels(self, rank_dm=None, floats=True):
        """Octaves and the channel pyramid of the resident images (no cascade)."""
        self.reset_step(None, octaves=True)
        self.launch_octaves()
        self.launch_channels(rank_dm, floats)

    def run(self, dm):
        """octaves -> channels -> cascade for one model: the detection path (reference model.py:149-179): one
        memset and three kernels.  When the cascade has rank tables the channels go to HBM as ranks only."""
        fused = self.ranks_for(dm)
        stt = self._casc_state(dm)
        # No memset launch: the octave kernel's first workgroup resets what the CASCADE accumulates into (shard counters,
        # alive[B, L, T] -- nothing touches them before it), the cascade's first workgroup resets what the next step's
        # OCTAVE kernel accumulates into (the (min, max) keys -- the channel kernel has finished with them).  The keys
        # must be zero on entry: ensure_clean_keys (one memset after anything else has used the engine's octaves).
        if self.exact_single or _NO_FUSED_RESET or stt.n_tiles == 0 or self.plan.n_levels == 0:
            self.reset_step(stt, octaves=True)
            self.launch_octaves()
            self.launch_channels(dm if fused else None, floats=not fused)
            stt.ranks = fused
            return self.launch_cascade(dm, ranks=fused)
        import torch
        if not torch.cuda.is_current_stream_capturing():
            self.ensure_clean_keys()
        elif not self._mm_clean:
            raise RuntimeError("capture a step only after an eager one (PyramidEngine.capture does): the octaves' keys must be clean")
        o = self._mm_words
        self.launch_octaves(zero=self.ctrl[o: o + nat.WB_DET_SHARDS + stt.alive.numel()])
        self.launch_channels(dm if fused else None, floats=not fused)
        stt.ranks = fused
        return self.launch_cascade(dm, ranks=fused, zero_keys=True)

    # ------------------------------------------------------------------ hipGraph
    def capture(self, dm):
        """Capture octaves -> channels -> cascade into one hipGraph (torch.cuda.CUDAGraph on ROCm).
        Returns a CapturedStep; ``.replay()`` re-runs the whole pipeline on the resident images (and raises once the
        engine has re-allocated a buffer the graph addresses)."""
        import torch
        self._casc_state(dm)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.run(dm)                      # warm-up outside capture (module load, attributes)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capturing(g):
            self.run(dm)
        return CapturedStep(self, g)

    # ------------------------------------------------------------------ results
    def ensure_capacity(self, dm):
        """Re-run the cascade with a larger buffer if a shard of the detection buffer overflowed
        in the last scan.  Returns the number of detections."""
        while True:
            need = self.detb.max_count()
            if need <= self.detb.cap:
                return int(self.detb.counts.sum().item())
            self._grow_and_rescan(dm, self._casc_state(dm), need)

    def _grow_and_rescan(self, dm, stt, worst):
        """A shard of the detection buffer overflowed in the scan `stt` (its fullest holds `worst` records): a larger
        buffer, and the same scan again on the resident channels.  Returns the scan state."""
        self.det_capacity = (int(worst * 1.5) + 16) * nat.WB_DET_SHARDS
        self._alloc_det()
        return self.run_cascade(dm, ranks=stt.ranks)

    def pack(self, out=None):
        """Pack the valid records of all shards behind a 4-word header (wb_det_pack_launch) into self.packed --
        the form a collective or a host read-back takes; no synchronisation.  out: an int32 [1 + rows, 4] device
        tensor (16-byte aligned, e.g. a rank's slot of a collective's send buffer) to pack into instead -- the header
        then says how many of the valid records fitted its `rows`."""
        import torch
        if out is None:
            if self.packed is None:
                self.packed = torch.empty((1 + self.detb.NS * self.detb.cap, 4), dtype=torch.int32, device=self.dev)
            out = self.packed
        nat.launch("wb_det_pack_launch", self.detb.recs, self.detb.counts, self.detb.cap, out, out.shape[0] - 1)
        return out

    def fetch(self, dm, stt, limit=None):
        """Everything the host needs from the last scan in ONE synchronisation: the shard contents packed on
        the device (wb_det_pack_launch), then asynchronous copies of the header + first records and of
        alive[B, L, T] into page-locked memory, one event wait.  Grows the buffer and scans again if a shard
        overflowed; a second copy only when there are more than _FETCH_ROWS detections.
        Returns Packed(total, records int32 [total, 4] in shard order, alive int64 [B, L, T]).
        limit: with more than `limit` detections the records stay on the device (self.packed[1:1 + total]; the caller
        orders them there) and `records` is None."""
        import torch
        while True:
            if self._h_packed is None:
                self._h_packed = torch.empty((1 + self._FETCH_ROWS, 4), dtype=torch.int32).pin_memory()
            self.pack()
            rows = min(self._h_packed.shape[0], self.packed.shape[0])
            self._h_packed[:rows].copy_(self.packed[:rows], non_blocking=True)
            self._alive_enqueue(stt)
            self._fetch_ev.record()
            self._fetch_ev.synchronize()
            total, worst = int(self._h_packed[0, 0]), int(self._h_packed[0, 1])
            if worst <= self.detb.cap:
                break
            stt = self._grow_and_rescan(dm, stt, worst)
        alive = alive_host(self._h_alive, dm.n_stages)
        if limit is not None and total > limit:
            return Packed(total, None, alive)
        recs = self._h_packed[1:1 + min(total, rows - 1)].numpy().copy()
        if total > rows - 1:
            recs = np.concatenate([recs, self.packed[rows:1 + total].cpu().numpy()])
        return Packed(total, recs, alive)

    def _alive_enqueue(self, stt):
        """The copy of alive[B, L, T] of the scan `stt` into page-locked memory (self._h_alive), no synchronisation."""
        import torch
        if self._h_alive is None or self._h_alive.shape != stt.alive.shape:
            self._h_alive = torch.empty(stt.alive.shape, dtype=torch.int32).pin_memory()
        self._h_alive.copy_(stt.alive, non_blocking=True)

    def _key_extent(self):
        """(whether this pyramid fits the sort key's bit fields, its largest u, its largest v) -- what the finish launches
        are told; when it fits, they also take the levels' inverse scales, uploaded here on first use."""
        import torch
        if self._key_dims is None:
            p = self.plan
            mu = max((int(lv["u"]) for lv in p.levels), default=0)
            mv = max((int(lv["v"]) for lv in p.levels), default=0)
            self._key_dims = (key_fits(p.n_levels, mu, mv), mu, mv)
            if self._key_dims[0]:
                self._inv_scales_d = torch.from_numpy(self.inv_scales()).to(self.dev)
        return self._key_dims

    def _final_ready(self):
        """Whether Model.detect's one-copy read-back form applies to this engine: one image, a pyramid within the sort
        key's bit fields."""
        return self.batch == 1 and self._key_extent()[0]

    def _final_enqueue(self, dm, stt):
        """wb_det_finish_sorted_launch + the ONE read-back copy into page-locked memory (no synchronisation).  The buffers
        belong to the cascade's scan state: several cascades can be scanned back to back on one engine (waldboost.detect)
        and read back with ONE wait -- the shared detection buffer is free again as soon as this launch has run."""
        import torch
        n_alive = stt.alive.numel()
        fb = stt.final
        if fb is None:
            # the finish block | alive[B, L, T] (the kernel copies the statistics behind it: one read-back copy, not two)
            blk = FinishBlock(self._FETCH_ROWS)
            nbytes = blk.nbytes + 4 * n_alive
            host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            h = host.numpy()
            fb = stt.final = FinalBuffers(torch.empty(nbytes, dtype=torch.uint8, device=self.dev), host, blk.views(h),
                                          h[blk.nbytes:].view(np.int32).reshape(tuple(stt.alive.shape)))
        # (one workgroup sorts up to 4096 keys in LDS and writes the sections in the reference's order: header[3])
        nat.launch("wb_det_finish_sorted_launch", self.detb.recs, self.detb.counts, self.detb.cap, self._inv_scales_d, self.plan.n_levels,
                   self._key_dims[1], self._key_dims[2], dm.m, dm.n, fb.dev, self._FETCH_ROWS, stt.alive, n_alive)
        fb.host.copy_(fb.dev, non_blocking=True)

    def _nms_enqueue(self, holder, fin_ptr, rows, n_images, nms):
        """wb_nms_finish_launch on the `n_images` finish blocks of `rows` rows at `fin_ptr` + the copy of its keep flags
        into page-locked memory, in the current stream, behind the launch that wrote the blocks (no synchronisation).
        Its result block, that block's page-locked copy and its scratch are kept in `holder` (a scan state, the batch's
        order buffers).  Nothing when the rows do not fit the launch: the caller then suppresses the complete result with
        boxes.nms_keep_mask.  nms: a boxes.Suppression."""
        import torch
        if rows < 4 or rows % 4:
            return
        nb = holder.nms
        if nb is None or nb.rows != rows or nb.images != n_images:
            need = nat.query("wb_nms_finish_scratch_bytes", rows, n_images)
            h_res = torch.empty(n_images * (16 + rows), dtype=torch.uint8).pin_memory()
            nb = holder.nms = NmsBuffers(rows, n_images, torch.empty(need, dtype=torch.uint8, device=self.dev),
                                         torch.empty(n_images * (16 + rows), dtype=torch.uint8, device=self.dev),
                                         h_res, h_res.numpy().reshape(n_images, 16 + rows))
        nat.launch("wb_nms_finish_launch", C.c_void_p(fin_ptr), rows, n_images, nms.iou_threshold, *nms.threshold_args, nb.scratch,
                   nb.scratch.numel(), nb.res)
        nb.h_res.copy_(nb.res, non_blocking=True)

    @staticmethod
    def _nms_keep(holder, b, rows, total):
        """Image b's keep flags (bool [total]) from the read-back of _nms_enqueue; None when the device did not
        suppress this image (more detections than a block holds)."""
        nb = holder.nms
        if nb is None or nb.rows != rows:
            return None
        row = nb.h[b]
        info = row[:16].view(np.uint32)
        if int(info[2]) != 1 or int(info[1]) != total:
            return None
        return row[16:16 + total].astype(bool)

    def fetch_final(self, dm, stt, enqueued=False, stream=None, nms=None):
        """fetch() for Model.detect on ONE image: wb_det_finish_sorted_launch leaves sort keys, boxes and scores of all
        valid records in one finish block (readback.FinishBlock); it comes back with ONE copy and ONE event wait together
        with alive[B, L, T].  Returns a readback.Finished, or None when this form does not apply (a batch, a pyramid beyond
        the key's bit fields, more than _FETCH_ROWS detections): use fetch() then.  Grows the detection buffer and scans
        again if a shard overflowed.
        enqueued: the launch and the copies are already in the stream (detect_run's graph replay).
        stream: that stream, when it is not the current one -- then only the wait happens here, and False is returned
        if more than a wait is needed (the caller comes back on that stream).
        nms: a boxes.Suppression -- non-maximum suppression ran (enqueued) or runs (not enqueued)
        on the finish buffer behind the launch that wrote it, a scan repeated after an overflow included; the result's
        `keep` then holds its flags."""
        if not self._final_ready():
            return None
        while True:
            if not enqueued:
                self._final_enqueue(dm, stt)
                if nms is not None:
                    self._nms_enqueue(stt, stt.final.dev.data_ptr(), self._FETCH_ROWS, 1, nms)
            enqueued = False
            self._fetch_ev.record(stream)                     # (None: the current stream)
            self._fetch_ev.synchronize()
            worst = int(stt.final.views[0][1])
            if worst <= self.detb.cap:
                break
            if stream is not None:
                return False
            stt = self._grow_and_rescan(dm, stt, worst)
        return self._finished(stt, dm.n_stages, nms is not None)

    def _finished(self, stt, T, nms=False):
        """The Finished of the read-back in the scan state `stt` (T stages; nms: with the keep flags _nms_enqueue left),
        None when there are more detections than the block holds."""
        hdr, keys, boxes, scores = stt.final.views
        total = int(hdr[0])
        if total > self._FETCH_ROWS:
            return None
        return Finished(keys[:total], boxes, scores, alive_host(stt.final.alive, T), bool(hdr[3]),
                        self._nms_keep(stt, 0, self._FETCH_ROWS, total) if nms else None)

    _ORDER_ROWS = 4096               # per image: what wb_det_order_batch_launch orders (more: the caller's other path)

    def _order_buffers(self):
        """Buffers of the batch's ordered read-back (scratch, output, its page-locked copy), on first use; whether the
        form applies to this pyramid (the sort key's bit fields)."""
        import torch
        if self._order is None:
            od = self._order = OrderBuffers(self._key_extent()[0])
            if od.fits:
                P, B = self._ORDER_ROWS, self.batch
                blk = FinishBlock(P)
                od.scratch = torch.empty(B * (256 + 16 * P), dtype=torch.uint8, device=self.dev)
                od.out = torch.empty(16 + B * blk.nbytes, dtype=torch.uint8, device=self.dev)
                od.h_out = torch.empty(16 + B * blk.nbytes, dtype=torch.uint8).pin_memory()
                od.ev = torch.cuda.Event()
                h = od.h_out.numpy()
                od.info = h[:16].view(np.int32)
                od.views = [blk.views(h, 16 + b * blk.nbytes) for b in range(B)]
        return self._order.fits

    def order_batch_enqueue(self, dm, stt, nms=None):
        """wb_det_order_batch_launch on the last scan's detections + the read-back copies (ordered results, alive[B, L, T])
        into page-locked memory + an event, all in the current stream, no synchronisation: what fetch_ordered_batch
        waits for.  Enqueued right behind the step, the results are on the host by the time they are asked for.
        Returns False when the form does not apply to this pyramid."""
        if not self._order_buffers():
            return False
        od, p = self._order, self.plan
        nat.launch("wb_det_order_batch_launch", self.detb.recs, self.detb.counts, self.detb.cap, self.batch, self._inv_scales_d, p.n_levels,
                   self._key_dims[1], self._key_dims[2], dm.m, dm.n, od.scratch, od.scratch.numel(), od.out, self._ORDER_ROWS)
        od.h_out.copy_(od.out, non_blocking=True)
        self._alive_enqueue(stt)
        if nms is not None:                                   # (every image's block suppressed in the same three launches)
            self._nms_enqueue(od, od.out.data_ptr() + 16, self._ORDER_ROWS, self.batch, nms)
        od.ev.record()
        return True

    def fetch_ordered_batch(self, dm, stt, enqueued=False, nms=None):
        """fetch() for a batch whose results are wanted image by image in the reference's order (Model.detect_stream's
        batches): wb_det_order_batch_launch splits the shards' records by image and orders every image's keys, boxes
        and scores on the device; they come back with ONE copy and ONE event wait together with alive[B, L, T].
        enqueued: order_batch_enqueue has run behind the scan already (only the wait happens here).
        Grows the detection buffer and scans again if a shard overflowed.
        Returns ([readback.ImageResult per image], alive int64 [B, L, T]), or None when this form does not apply (a
        pyramid beyond the sort key's bit fields, an image with more than _ORDER_ROWS detections): use fetch() then.
        nms: as for order_batch_enqueue (with enqueued, what it was given there); every image's `keep` then holds its
        flags."""
        while True:
            if not enqueued and not self.order_batch_enqueue(dm, stt, nms):
                return None
            enqueued = False
            od = self._order
            od.ev.synchronize()
            worst = int(od.info[1])
            if worst <= self.detb.cap:
                break
            stt = self._grow_and_rescan(dm, stt, worst)
        out = []
        for hdr, keys, boxes, scores in od.views:
            n_b = int(hdr[0])
            if int(hdr[1]) > self._ORDER_ROWS or int(hdr[3]) != 1:
                return None
            out.append(ImageResult(keys[:n_b], boxes[:n_b], scores[:n_b],
                                   self._nms_keep(od, len(out), self._ORDER_ROWS, n_b) if nms is not None else None))
        return out, alive_host(self._h_alive, dm.n_stages)

    def live_check(self, dm):
        """A cascade whose specialised kernel has just been built, on the image(s) resident in this engine: the whole step
        with the specialised kernel, then the cascade alone again with the generic kernel on the same channels; per-stage
        alive counts and the ordered detection records must be identical.  If they are not, the specialised kernel is
        switched off for this cascade for good (a warning says so) -- the step's buffers hold the generic kernel's results
        either way.  Runs _LIVE_CHECKS times per cascade and tile kind, outside captures; costs one extra step each."""
        import torch
        dtype = self.scan_dtype(dm)
        if dm.live_checks_left(dtype) <= 0 or dtype not in dm.specialized() or torch.cuda.is_current_stream_capturing():
            return
        while dm.take_live_check(dtype):
            stt = self.run(dm)                                       # specialised kernel
            if int(self.detb.counts.max().item()) > self.detb.cap:
                return                                                # (overflowing buffer: the caller grows it; check another time)
            spec = (sort_records(self.detb.compact()).clone(), stt.alive.clone())
            dm.use_specialized(False)
            self.run_cascade(dm, ranks=stt.ranks)                     # generic kernel, same channels
            gen = (sort_records(self.detb.compact()), stt.alive)
            same = spec[0].shape == gen[0].shape and bool(torch.equal(spec[0], gen[0])) and bool(torch.equal(spec[1], gen[1]))
            if not same:
                dm.take_live_check(dtype, all_left=True)
                _log.warning("cascade of %d stages, depth %d: its model-specialised kernel disagrees with the generic kernel on "
                             "this image (%d against %d detections); the specialised kernel is switched off for this cascade",
                             dm.n_stages, dm.depth, int(spec[0].shape[0]), int(gen[0].shape[0]))
                return                                                # (stays off)
            dm.use_specialized(True)

    def detect_run(self, dm, nms=None):
        """Model.detect's whole device sequence for the resident image -- one memset, octaves, channels, cascade,
        wb_det_finish_sorted_launch (which also carries alive[] behind the scores), the ONE read-back copy -- and its one synchronisation; from the second call with the
        same cascade on it is replayed as ONE hipGraph (one enqueue instead of seven, no gaps between the kernels).
        Returns what fetch_final returns: a readback.Finished, or None (then: use fetch()).
        nms: a boxes.Suppression -- the same step, eager or replayed, then wb_nms_finish_launch and the
        copy of its keep flags enqueued behind it, in front of the one wait: the plain step's graph is shared, a new
        threshold captures nothing."""
        return self.detect_collect(dm, self.detect_enqueue(dm, nms), nms=nms)

    def detect_enqueue(self, dm, nms=None):
        """detect_run up to, not including, its wait: everything is in the current stream when this returns (the image
        must stay resident until detect_collect, on the same stream, has run).  Returns a token for detect_collect."""
        import torch
        stt = self._casc_state(dm)
        if not self._final_ready():
            self.run(dm)
            return None
        g = stt.graph
        if g is None and stt.detect_calls >= 1 and not _NO_DETECT_GRAPH:
            # (the first call ran eagerly: every lazily allocated buffer exists, the kernels are loaded)
            # a cascade that is scanned again is worth its specialised kernel -- built now, so that the graph holds it
            dm.note_scan(self.scan_dtype(dm), force=True)
            self.live_check(dm)               # (a kernel built just now meets its first real image: cross-checked before the capture)
            g = torch.cuda.CUDAGraph()
            self.ensure_clean_keys()          # (the captured step holds no memset: see run)
            torch.cuda.synchronize()
            with capturing(g):
                self.run(dm)
                self._final_enqueue(dm, stt)
            stt.graph = g
        stt.detect_calls += 1
        if g is None:
            self.run(dm)
            self._final_enqueue(dm, stt)
        else:
            self.ensure_clean_keys()
            g.replay()
        if nms is not None:
            self._nms_enqueue(stt, stt.final.dev.data_ptr(), self._FETCH_ROWS, 1, nms)
        return stt

    def batch_enqueue(self, dm):
        """The step -- octaves, channels, cascade -- over the resident batch, without a wait: eager on an engine's first
        call, a replayed hipGraph afterwards (captured again after _buffers_moved has dropped it).
        Returns the scan state fetch() takes."""
        stt = self._casc_state(dm)
        step = stt.step
        if step is None and stt.batch_calls >= 1 and not _NO_DETECT_GRAPH:
            dm.note_scan(self.scan_dtype(dm), force=True)
            self.live_check(dm)
            step = stt.step = self.capture(dm)
        stt.batch_calls += 1
        if step is None:
            self.run(dm)
        else:
            step.replay()
        return stt

    def detect_multi_run(self, dms, ranks):
        """waldboost.detect's whole device sequence for the resident image -- octaves, ONE channel pyramid (as ranks of
        dms[0]'s rank tables -- a rank group's union tables -- or as float32 channels), then per cascade of `dms` its
        scan, wb_det_finish_sorted_launch and the read-back copy -- with ONE wait at its end; from the second call with the
        same cascades on it is one hipGraph replay.  Returns [readback.Finished per cascade] -- None in the place of
        a cascade whose results did not fit (an overflowing detection buffer, more detections than one read-back holds): the
        pyramid stays resident and the caller scans that cascade alone again --, or None when the form does not apply at all
        (more cascades than an engine keeps states for, a pyramid beyond the sort key's fields, a sequence that kept missing
        lately): the caller then builds the pyramid and scans model by model."""
        import torch
        if not self._final_ready() or not 0 < len(dms) <= 4 or len({id(d) for d in dms}) != len(dms):
            return None
        key = tuple(id(d) for d in dms) + (bool(ranks),)
        stts = [self._casc_state(d) for d in dms]            # (may grow the control block, which drops the sequences)
        if any(self._casc.get(id(d)) is not t for d, t in zip(dms, stts)):
            return None
        st = self._multi.get(key)
        if st is None or any(a is not b for a, b in zip(st.stts, stts)):
            if len(self._multi) >= 2:
                self._multi.pop(next(iter(self._multi)))
            st = self._multi[key] = MultiState(stts, list(dms))
        if st.skip > 0:                                       # (its results did not fit lately: do not scan twice per call)
            st.skip -= 1
            return None

        def enqueue():
            self.run_channels(rank_dm=dms[0] if ranks else None, floats=not ranks)
            for d in dms:
                self._final_enqueue(d, self.run_cascade(d, ranks=ranks))

        if st.graph is None and st.calls >= 1 and st.fails == 0 and not _NO_DETECT_GRAPH:
            # (captured after an eager call whose results fitted: a sequence that keeps missing is not worth a capture)
            for d in dms:
                d.note_scan(d.rank_dtype if ranks else self.spec.wb_dtype, force=True)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with capturing(g):
                enqueue()
            st.graph = g
        st.calls += 1
        if st.graph is None:
            enqueue()
        else:
            self._mm_clean = False                            # (the replay's octave launch leaves its keys behind)
            st.graph.replay()
            self.rank_owner = dms[0].rank_key if ranks else None
        self._fetch_ev.record()
        self._fetch_ev.synchronize()
        out = []
        for d, stt in zip(dms, stts):
            # a cascade whose results did not fit (a shard overflowed, or more detections than one read-back holds): None
            # in its place -- the caller scans THAT cascade again on the pyramid this call left resident
            # (Model.scan_engine: run_cascade + fetch, which grows the buffer); the others keep what they have
            out.append(None if int(stt.final.views[0][1]) > self.detb.cap else self._finished(stt, d.n_stages))
        if any(f is None for f in out):
            st.fails += 1                                     # (the whole sequence is tried again after 16, 32, 64 ... calls)
            st.skip = min(8 << st.fails, 4096)
            # (the re-scans may reuse read-back buffers before the caller has collected the fitted results: hand out copies)
            out = [None if f is None else f._replace(keys=f.keys.copy(), boxes=np.array(f.boxes[:f.keys.size]),
                                                     scores=np.array(f.scores[:f.keys.size])) for f in out]
        else:
            st.fails = 0
        return out

    def detect_collect(self, dm, token, stream=None, nms=None):
        """The wait and the read-back that end detect_run, for a token of detect_enqueue.
        stream: the stream detect_enqueue ran on, when that is not the current one."""
        import torch
        if token is None:
            return None
        fin = self.fetch_final(dm, token, enqueued=True, stream=stream, nms=nms)
        if fin is False:
            with torch.cuda.stream(stream):                   # (the rare ways out: launches and copies of their own)
                fin = self.fetch_final(dm, token, enqueued=False, nms=nms)
        return fin

    def sorted_detections(self):
        """Detections ordered by (image, level, r, c) as an int32 [n, 4] tensor of WbDet records."""
        return sort_records(self.detb.compact())

    def boxes(self, det_sorted, dm):
        import torch
        n = det_sorted.shape[0]
        boxes = torch.empty((n, 4), dtype=torch.float32, device=self.dev)
        scores = torch.empty(n, dtype=torch.float32, device=self.dev)
        if n:
            inv_d = torch.from_numpy(self.inv_scales()).to(self.dev)
            nat.launch("wb_boxes_launch", det_sorted, n, inv_d, dm.m, dm.n, boxes, scores)
        return boxes, scores

    def ordered_host(self, dm, total):
        """The `total` records fetch() left on the device (self.packed), put in the reference's order there, with their
        boxes and scores (wb_boxes_launch), as host arrays: (records int32 [total, 4], boxes, scores)."""
        det = sort_records(self.packed[1:1 + total])
        boxes, scores = self.boxes(det, dm)
        return det.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy()

    def inv_scales(self):
        """float32(1.0 / scale) per level: the factor get_boxes multiplies with (reference model.py:147)."""
        if getattr(self, "_inv_scales", None) is None:
            self._inv_scales = np.array([np.float32(1.0 / s) for s in self.plan.scales], np.float32)
        return self._inv_scales

    def _level_slice(self, buf, b, l, C):
        """Level l of image b in a channel or rank buffer, as a device view [u,v,C]."""
        lv = self.plan.levels[l]
        off = int(self.level_np[l]["chn_off"])
        u, v = lv["u"], lv["v"]
        return buf[b, off:off + u * v * C].view(u, v, C)

    def level_tensor(self, b, l):
        """Channels of level l of image b as a device view [u,v,C] into the pyramid buffer."""
        return self._level_slice(self.chn, b, l, self.spec.n_channels)

    def read_rank_level(self, b, l):
        """Ranks of level l of image b as a uint8 ndarray [u,v,4] (after launch_channels(rank_dm=...))."""
        r = self._level_slice(self.rank, b, l, 4).cpu().numpy()
        return r.view(np.uint16) if r.dtype == np.int16 else r

    def read_level(self, b, l):
        """Channels of level l of image b as a fresh HWC ndarray [u,v,C] of the channel function's dtype."""
        return self.level_tensor(b, l).cpu().numpy()


def nat_f32_key(f):
    b = np.array([f], np.float32).view(np.uint32)[0]
    return np.uint32(~b & 0xFFFFFFFF) if (b & 0x80000000) else np.uint32(b | 0x80000000)


_ENGINES = {}


def get_engine(H, W, dtype, shrink, n_per_oct, smooth, batch=1, exact_single=False, channels=None):
    """Small cache of engines keyed by configuration (buffers are reused across calls)."""
    import torch
    channels = channels if channels is not None else SPECS["grad_hist"]
    key = (int(H), int(W), np.dtype(dtype).str, int(shrink), int(n_per_oct), int(smooth), int(batch),
           bool(exact_single), channels.key, torch.cuda.current_device() if torch.cuda.is_available() else -1)
    e = _ENGINES.get(key)
    if e is None:
        if len(_ENGINES) >= 4:
            _ENGINES.pop(next(iter(_ENGINES)))
        e = PyramidEngine(H, W, dtype, shrink, n_per_oct, smooth, batch, exact_single, channels=channels)
        _ENGINES[key] = e
    return e
