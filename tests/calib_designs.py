"""Models and samples whose stage-score traces are planted, for the calibration kernels (csrc/wb_cascade.hip:
wb_samples_trace_launch, wb_calib_min_launch).

A design fixes, for every sample i and stage t, the LEAF sample i lands in (leaf[i, t]) and, for every stage, the leaves'
predictions (values[t, leaf]): the increment sample i takes at stage t is values[t, leaf[i, t]], a chosen float32.  The
model is made of complete trees of depth D; level l of stage t's tree tests one pixel of the window, pixel number
t * D + l, and the samples carry `lo` (<= threshold: left, bit 0) or `hi` (right, bit 1) there: the bits of leaf[i, t],
first level first.  Depth 1 is one pixel per stage and two increments.

tests/test_calib_designs_host.py proves what the designs claim (exact rational arithmetic) and that they tell wrong
kernels from the statement (tests/calib_reference.py); tests/test_gpu_calib_designs.py runs them on the GPU.
"""
import functools

import numpy as np

from oracle import wb_oracle as orc

SHAPE = (8, 8, 4)                       # 256 pixels: up to 256 // D stages
STAGE_COUNTS = (1, 2, 63, 64, 65, 200)
SAMPLE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
WG, WAVE = 256, 64                      # samples per workgroup and per wave of the kernels
NINF = float("-inf")


class Design:
    """name; leaf (N, T) int; values (T, 2**D) float32; D; dtype of the samples; thetas: the model's own (the "old"
    ones: what reject=1 applies, what calibrate must ignore); recalls to calibrate at; exact: every running score is
    the exact sum of its increments; owners: {recall: (T,) sample that alone holds stage t's minimum among the retained,
    -1 where not claimed}."""

    def __init__(self, name, leaf, values, D=1, dtype=np.uint8, thetas=None, recalls=(1.0,), exact=True, owners=None):
        self.name, self.D, self.dtype, self.exact = name, D, np.dtype(dtype), exact
        self.leaf = np.asarray(leaf, np.int64)
        self.values64 = np.asarray(values, np.float64)          # as planned; the host test proves them float32 values
        self.values = self.values64.astype(np.float32)
        self.N, self.T = self.leaf.shape
        assert self.values.shape == (self.T, 1 << D) and self.T * D <= SHAPE[0] * SHAPE[1] * SHAPE[2]
        assert self.leaf.min() >= 0 and self.leaf.max() < (1 << D)
        self.thetas = [NINF] * self.T if thetas is None else list(thetas)
        self.recalls = tuple(recalls)
        self.owners = owners or {}
        # pixel values and the threshold between them, per dtype
        self.lo, self.hi, self.thr = (0, 255, 127.0) if self.dtype == np.uint8 else (-1.5, 2.25, 0.0)

    def pixel(self, t, l):
        """(row, col, channel) of the pixel level l of stage t tests."""
        p = t * self.D + l
        return p // (SHAPE[1] * SHAPE[2]), (p // SHAPE[2]) % SHAPE[1], p % SHAPE[2]

    @functools.cached_property
    def X(self):
        X = np.full((self.N,) + SHAPE, self.lo, self.dtype)
        for t in range(self.T):
            for l in range(self.D):
                bit = (self.leaf[:, t] >> (self.D - 1 - l)) & 1
                r, c, ch = self.pixel(t, l)
                X[:, r, c, ch] = np.where(bit == 1, self.hi, self.lo).astype(self.dtype)
        return X

    def tree_arrays(self, t):
        """Stage t's complete tree in pre-order (left first): feature, threshold, left, right, prediction lists."""
        feature, threshold, left, right, prediction = [], [], [], [], []

        def grow(level, path):
            at = len(left)
            for a in (feature, threshold, left, right, prediction):
                a.append(None)
            if level == self.D:
                feature[at], threshold[at], left[at], right[at], prediction[at] = (0, 0, 0), -2.0, -1, -1, float(self.values[t, path])
                return at
            feature[at], threshold[at], prediction[at] = self.pixel(t, level), self.thr, 0.0
            left[at] = grow(level + 1, path << 1)
            right[at] = grow(level + 1, (path << 1) | 1)
            return at

        grow(0, 0)
        return feature, threshold, left, right, prediction

    @functools.cached_property
    def trees(self):
        """The oracle's plain-array trees."""
        return [orc.make_tree(*self.tree_arrays(t)) for t in range(self.T)]

    def model(self):
        """A fresh waldboost_amd.Model with the design's trees and thetas."""
        import waldboost_amd as wb
        M = wb.Model(SHAPE, dict(wb.default_channel_opts))
        for t in range(self.T):
            M.append(wb.DTree(*self.tree_arrays(t)), self.thetas[t])
        return M

    @functools.cached_property
    def increments(self):
        """(N, T) float32: the planted increment of every sample at every stage."""
        return self.values[np.arange(self.T)[None, :], self.leaf]


def owner_cycle(N):
    """Samples by their place in the launch: lane 0 and lane 63 of the first wave, the first lane of the second, the last
    sample (the last lane of a partial wave), the first lane of the last wave and of the last workgroup, the last lane of
    the first workgroup, the sample before the last."""
    want = [0, WAVE - 1, WAVE, N - 1, (N - 1) // WAVE * WAVE, (N - 1) // WG * WG, WG - 1, N - 2, WG, WG + WAVE - 1]
    out = []
    for i in want:
        if 0 <= i < N and i not in out:
            out.append(i)
    return out


def owners_design(N, T, base=0.0, dtype=np.uint8, thetas=None):
    """Stage t's minimum belongs to owner[t] alone: everybody takes `base` at every stage except the owner, who takes what
    puts it one below the lowest running score so far.  Integers (plus multiples of `base`, a small dyadic): exact."""
    cyc = owner_cycle(N)
    owner = np.array([cyc[t % len(cyc)] for t in range(T)])
    leaf = np.zeros((N, T), np.int64)
    values = np.zeros((T, 2), np.float64)
    dev = np.zeros(N)                                     # running score minus base * (t + 1)
    for t in range(T):
        o = owner[t]
        step = (dev.min() - 1.0) - dev[o]                 # <= -1
        leaf[o, t] = 1
        values[t] = base, base + step
        dev[o] += step
    return Design(f"owners-{N}x{T}-{np.dtype(dtype).name}" + (f"-base{base}" if base else "") + ("-thetas" if thetas else ""),
                  leaf, values, dtype=dtype, thetas=thetas, owners={1.0: owner})


def order_design():
    """Increments on which the order and the precision of the sum show: 1, 2^25, -2^25, 2^25, 1, -2^25 sums to 0 in fp32
    in stage order, to 2 exactly (and in float64), to 1 in fp32 in reverse order.  Leaf 1 takes small integers."""
    a = [1.0, 2.0 ** 25, -2.0 ** 25, 2.0 ** 25, 1.0, -2.0 ** 25]
    b = [3.0, -5.0, 7.0, -2.0, 4.0, -6.0]
    rng = np.random.default_rng(7)
    leaf = rng.integers(0, 2, (65, 6))
    leaf[0] = 0                                           # sample 0 takes the whole ill-conditioned row
    leaf[64] = 1
    return Design("order-65x6", leaf, np.stack([a, b], 1), dtype=np.float32, exact=False, recalls=(1.0, 0.5))


TIES_KEEP = {0.3891: (100, 128), 0.249: (64, 64), 0.25: (65, 128), 1e-9: (1, 64), 1.0: (257, 257), 0.75: (193, 257)}


def ties_design():
    """Final scores in four groups (F = i % 4) and, inside every group, samples that dip by 8 at stage 2 and come back at
    stage 3 -- the LAST samples of each group.  A recall whose floor falls inside a group retains the whole group; the
    samples below the floor have the lowest running scores at stages 0 and 1."""
    N = 257
    i = np.arange(N)
    g = i % 4
    dip = (i >= 200).astype(np.int64)
    leaf = np.stack([g >> 1, g & 1, dip, dip], 1)
    values = [(0.0, 2.0), (0.0, 1.0), (0.0, -8.0), (0.0, 8.0)]
    # F: 65 samples at 0 (i % 4 == 0), 64 each at 1, 2, 3.  TIES_KEEP: recall -> (keep, retained): keep = 100 falls inside
    # group 2 (128 retained); 0.249 * 257 = 63.99 and 0.25 * 257 = 64.25 lie on either side of a ceil step: keep = 64 is
    # exactly group 3, keep = 65 takes all of group 2 as well; keep = 1; keep = N; keep = 193 reaches the lowest group
    recalls = tuple(TIES_KEEP)
    thetas = [0.5, NINF, -7.5, NINF]                      # old thetas that would reject retained samples: they play no part
    return Design("ties-257x4", leaf, values, thetas=thetas, recalls=recalls)


def reject_design(dtype=np.uint8):
    """Rejection at h == theta (passes) and one ulp below theta (rejected), -inf thetas between finite ones.  Running
    scores: stage 0: 0.75 or 1.5; stage 1: + 0.25; stage 2: + 1 or + 3; stage 3: - 0.5; stage 4: +0.125 or -0.125."""
    N = 130
    i = np.arange(N)
    leaf = np.stack([i & 1, np.zeros(N, np.int64), (i >> 1) & 1, np.zeros(N, np.int64), (i >> 2) & 1], 1)
    values = [(0.75, 1.5), (0.25, 0.25), (1.0, 3.0), (-0.5, -0.5), (0.125, -0.125)]
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    # stage 0: theta == 0.75 exactly: both values pass.  stage 2: running scores 2, 2.75, 4, 4.75; theta one ulp above 2.75:
    # 2 and 2.75 rejected.  stage 4: of 3.5 / 4.25 -+ 0.125, theta == 3.625 exactly: 3.375 rejected, 3.625 passes
    thetas = [0.75, NINF, up(2.75), NINF, 3.625]
    return Design(f"reject-130x5-{np.dtype(dtype).name}", leaf, values, dtype=dtype, thetas=thetas, recalls=(1.0, 0.3))


def deep_design(D, N, T, seed):
    """Complete trees of depth D (4: the node-walk form), random leaves, increments in multiples of 1/8 up to 16: exact."""
    rng = np.random.default_rng(seed)
    leaf = rng.integers(0, 1 << D, (N, T))
    values = rng.integers(-128, 129, (T, 1 << D)) / 8.0
    thetas = [NINF if t % 3 else float(np.float32(-6.0 - t)) for t in range(T)]
    return Design(f"depth{D}-{N}x{T}", leaf, values, D=D, dtype=np.float32 if D == 3 else np.uint8, thetas=thetas,
                  recalls=(1.0, 0.9, 0.05))


# every stage count and every sample count, in pairs
GRID = [(1, 1), (63, 2), (64, 63), (65, 64), (255, 65), (256, 200), (257, 1), (1000, 2), (1000, 200), (257, 64), (64, 200), (65, 63)]


@functools.lru_cache(maxsize=None)
def designs():
    out = []
    for k, (N, T) in enumerate(GRID):
        some = [-0.5 - t if t % 4 == 1 else NINF for t in range(T)] if k % 3 == 2 else None
        out.append(owners_design(N, T, base=(0.0, 0.25)[k % 2], dtype=(np.uint8, np.float32)[(k // 2) % 2], thetas=some))
    out += [order_design(), ties_design(), reject_design(np.uint8), reject_design(np.float32),
            deep_design(2, 300, 24, 2), deep_design(3, 257, 16, 3), deep_design(4, 321, 12, 4)]
    assert {d.T for d in out} >= set(STAGE_COUNTS) and {d.N for d in out} >= set(SAMPLE_COUNTS)
    return {d.name: d for d in out}
