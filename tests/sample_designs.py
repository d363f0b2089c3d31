"""Designed inputs for the sample kernels of csrc/wb_cascade.hip -- gather_samples_kernel (wb_gather_samples_launch),
tree_eval_kernel (wb_tree_eval_launch), tree_apply_kernel (wb_tree_apply_launch) and samples_predict_kernel
(wb_samples_predict_launch): NumPy and the oracle, no GPU, no torch.

Each kernel is restated here on FLAT arrays, index for index (crop_kernel, walk_leaf / tree_apply_kernel / tree_eval_kernel,
predict_kernel), with a `wrong=` switch for the mistakes such a kernel could make (WRONG_CROP, WRONG_WALK, WRONG_PREDICT).
test_sample_designs_host.py proves that the restatement equals the oracle on every design and that every wrong kernel is
separated by the designs it is named for, with the exact counts (RECORDED); test_gpu_sample_designs.py runs the designs
through the kernels at the C ABI, byte for byte and bit for bit.  A wrong kernel that reads outside its array is restated
with the index wrapped into the array (`% size`): what a real one would read there is nobody's business, the count only
has to be positive.

Crops
  images   23 x 37 x C, position-coded: float32 holds the flat element index (exact below 2^24), uint8 holds
           (31 r + 17 c + 5 ch) mod 251; a pitch of 37 pixels is no multiple of anything
  cells    CROP_CELLS: (dtype, C, byte offset of X, byte offset of out) with the path crop_path() says the launch takes --
           16-byte vectors, 4-byte words or bytes, from px = C * esz and the two pointers.  The offsets are what a torch
           allocation never has: float32 x 4 with X or out 4 bytes in (words), uint8 x 4 with X or out 1 byte in (bytes),
           uint8 x 16 with X 4 bytes in (words).  `u8 x 43` is there for one shape only: 129 elements per crop fit a
           23 x 37 image only as 1 x 3 pixels of 43 bytes
  shapes   CROP_SHAPES: 1, 63, 64, 65 and 130 pixels per crop (the kernel's loop makes 1, 1, 1, 2 and 3 trips where an
           element is a pixel), one row, one column, the whole image
  origins  crop_origins: the four corners first -- (u - m, v - n) reads the buffer's last element --, then repeated
           positions in unsorted order; N = 1 and N = 300

Tree walks
  trees    TREE_SHAPES: one leaf; the 127-node right chain of 63 internal nodes (children up to 126) and its mirror; a
           depth-2 tree numbered breadth first (as fit_reference numbers them) and the same tree in pre-order; an
           unbalanced tree with a leaf at depth 1 beside depth 6.  Every node's prediction is another multiple of 0.25, so
           a prediction names its leaf
  noise    walk_design(): integer pixels 0 .. 15 and integer thresholds, so that about one comparison in sixteen is a
           tie; chain nodes are `always on` (-1 / 16) but for seven real ones, so that a few samples reach the last leaf;
           windows include the one at (u - m, v - n) and the root reads (m - 1, n - 1, C - 1); C = 1, 3, 4, uint8 and
           float32, 1 / 255 / 256 / 257 / 513 windows
  big      features with bit 7 set: windows of (130, 2, 1) and (2, 130, 1) on a 140 x 140 x 1 image, (1, 1, 200) on a
           9 x 11 x 200 image
  ties     one split node at (m - 1, n - 1, C - 1), one launch per threshold: float32 pixels TIE_VALUES against
           tie_thresholds() = every value and its two neighbours, +-0, NaN; uint8 pixels 0, 1, 254, 255 against
           U8_THRESHOLDS

Cascades on samples
  SCORE_DESIGNS: two-path cascades of split nodes on pixel (0, 0, 0) <= 0.5 (path A: pixel 0, path B: pixel 1) whose
  leaves and thetas are chosen stage by stage (_SCORES says what each is for); `shapes`: every tree shape twice, T = 12,
  thetas free or equal to a running sum that a sample attains; `shapes_shallow`: the same with leaves and depth-2 trees
  only, which stays on the tile forms; `ties`: the tie values under three split nodes.  MODEL_CELLS are the windows and
  sample dtypes every design runs at, with the counts 1 / 255 / 256 / 257 / 513 handed round (model_count).  The
  (1, 1, 200) window and every cascade with a chain run under the handle's node-walk flag (`generic`).
  wb_model_create refuses none of these shapes (REFUSED is empty): parent < child holds in breadth-first and in
  pre-order numbering alike, and 127 nodes is its limit, not beyond it.

Findings (asserted by the host test)
  * `cs not scaled by C` cannot show where a pixel is one element of the path (float32 x 4 as 16-byte vectors, uint8 x 4
    as words, one channel): it is named for the other cells.
  * A walk capped at 7 steps is right on every tree but the chains; one capped at 3 also on the unbalanced tree.
  * `theta -inf compared` differs from the skip on a NaN score alone (NaN >= -inf is false): the nan_free design.
"""
import functools

import numpy as np

from oracle import wb_oracle as orc

IMG_H, IMG_W = 23, 37
CANARY = 0xCD
PAD = 64                               # canary bytes in front of and behind `out`
COUNTS = (1, 255, 256, 257, 513)
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.float32(2.0 ** -126)


def _f32(x):
    return np.asarray(x, np.float32)


def _up(x):
    with np.errstate(over="ignore"):                 # (FLT_MAX -> inf)
        return np.nextafter(_f32(x), np.float32(np.inf))


def _down(x):
    with np.errstate(over="ignore"):
        return np.nextafter(_f32(x), np.float32(-np.inf))


# ------------------------------------------------------------------------------ crops
def crop_image(dtype, C, H=IMG_H, W=IMG_W):
    if np.dtype(dtype) == np.float32:
        assert H * W * C < 1 << 24
        return np.arange(H * W * C, dtype=np.float32).reshape(H, W, C)
    r, c, ch = np.indices((H, W, C))
    return ((31 * r + 17 * c + 5 * ch) % 251).astype(np.uint8)


def crop_path(C, esz, x_off=0, out_off=0):
    """Bytes per element the launch moves: the dispatch of wb_gather_samples_launch from px = C * esz and the two pointers'
    offsets from a 16-byte boundary."""
    px = C * esz
    if px % 16 == 0 and (x_off | out_off) % 16 == 0:
        return 16
    if px % 4 == 0 and (x_off | out_off) % 4 == 0:
        return 4
    return 1


# (name, dtype, C, byte offset of X, byte offset of out, element bytes of the path it must take)
CROP_CELLS = (
    ("f32x4", np.float32, 4, 0, 0, 16), ("f32x8", np.float32, 8, 0, 0, 16), ("u8x16", np.uint8, 16, 0, 0, 16),
    ("f32x1", np.float32, 1, 0, 0, 4), ("f32x3", np.float32, 3, 0, 0, 4), ("f32x5", np.float32, 5, 0, 0, 4),
    ("u8x4", np.uint8, 4, 0, 0, 4), ("u8x8", np.uint8, 8, 0, 0, 4), ("u8x12", np.uint8, 12, 0, 0, 4),
    ("u8x1", np.uint8, 1, 0, 0, 1), ("u8x2", np.uint8, 2, 0, 0, 1), ("u8x3", np.uint8, 3, 0, 0, 1), ("u8x5", np.uint8, 5, 0, 0, 1),
    ("f32x4/X+4", np.float32, 4, 4, 0, 4), ("f32x4/out+4", np.float32, 4, 0, 4, 4),
    ("u8x4/X+1", np.uint8, 4, 1, 0, 1), ("u8x4/out+1", np.uint8, 4, 0, 1, 1), ("u8x16/X+4", np.uint8, 16, 4, 0, 4),
    ("u8x43", np.uint8, 43, 0, 0, 1),
)
CROP_CELL = {c[0]: c for c in CROP_CELLS}
FALLBACK_CELLS = tuple(c[0] for c in CROP_CELLS if c[3] or c[4])
CROP_SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (10, 13), (1, IMG_W), (IMG_H, 1), (IMG_H, IMG_W))


def crop_shapes(cell):
    return ((1, 3),) if cell == "u8x43" else CROP_SHAPES


def crop_origins(m, n, N, u=IMG_H, v=IMG_W):
    """(rs, cs) int32 [N]: the corners (the last one first when N = 1), then seeded positions, some of them repeated, in no
    order."""
    corners = [(u - m, v - n), (0, 0), (0, v - n), (u - m, 0)]
    rng = np.random.default_rng(1000 * m + n)
    k = max(N - 4, 0)
    rs, cs = rng.integers(0, u - m + 1, k), rng.integers(0, v - n + 1, k)
    if k > 8:
        rs[k // 2:k // 2 + 4], cs[k // 2:k // 2 + 4] = rs[:4], cs[:4]          # repeated, far from their first use
        rs[-1], cs[-1] = u - m, v - n
    pos = (corners + list(zip(rs.tolist(), cs.tolist())))[:N]
    return np.array([p[0] for p in pos], np.int32), np.array([p[1] for p in pos], np.int32)


WRONG_CROP = ("pitch_n", "rows_cols_swapped", "cs_unscaled", "tail_dropped", "stride_16")


def crop_kernel(img, rs, cs, m, n, unit, wrong=None):
    """gather_samples_kernel<E> with sizeof(E) = unit on the image's bytes -> (out bytes [N * m * n * px], the PAD bytes in
    front, the PAD bytes behind); bytes a wrong kernel never writes keep CANARY."""
    u, v, C = img.shape
    px = C * img.itemsize
    assert px % unit == 0
    X = np.ascontiguousarray(img).view(np.uint8).reshape(-1, unit)
    xs = px // unit
    rowlen = n * xs
    total = m * rowlen
    N = rs.size
    out = np.full((PAD + N * total * unit + PAD) // unit * unit + 16 * N + 16, CANARY, np.uint8)
    pitch = n if wrong == "pitch_n" else v
    stride = total * unit
    if wrong == "stride_16":
        stride = -(-stride // 16) * 16
    e = np.arange(total if wrong != "tail_dropped" else total // 64 * 64)
    y = e // rowlen
    x = e - y * rowlen
    for i in range(N):
        r, c = int(rs[i]), int(cs[i])
        if wrong == "rows_cols_swapped":
            r, c = c, r
        src0 = (r * pitch + c) * xs if wrong != "cs_unscaled" else r * pitch * xs + c
        src = (src0 + y * pitch * xs + x) % X.shape[0]
        o = PAD + i * stride
        out[o:o + e.size * unit] = X[src].reshape(-1)
    end = PAD + N * total * unit
    return out[PAD:end], out[:PAD], out[end:end + PAD]


# ------------------------------------------------------------------------------ trees
def _tree(feature, threshold, left, right):
    k = len(left)
    t = dict(feature=np.array(feature, np.uint8).reshape(k, 3), threshold=np.array(threshold, np.float32),
             left=np.array(left, np.int8), right=np.array(right, np.int8),
             prediction=((np.arange(k) * 7 % 128 - 40) * np.float32(0.25)).astype(np.float32))     # distinct: 7 is odd, k <= 127
    assert np.unique(t["prediction"]).size == k
    return t


def tree_links(shape):
    """(left, right) lists of a tree shape; -1 on leaves."""
    if shape == "leaf":
        return [-1], [-1]
    if shape in ("right_chain", "left_chain"):
        # internal nodes at 0, 2, .. 124: one child the leaf beside them, the other the next internal node (126: the last leaf)
        a = [i + 1 if i % 2 == 0 else -1 for i in range(127)]
        b = [i + 2 if i % 2 == 0 else -1 for i in range(127)]
        a[126] = b[126] = -1
        return (a, b) if shape == "right_chain" else (b, a)
    if shape == "bfs":
        return [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1]
    if shape == "preorder":
        return [1, 2, -1, -1, 5, -1, -1], [4, 3, -1, -1, 6, -1, -1]
    assert shape == "unbalanced"
    # root: a leaf on the left; on the right five more splits, each with a leaf on the left, down to depth 6
    return [1, -1, 3, -1, 5, -1, 7, -1, 9, -1, 11, -1, -1], [2, -1, 4, -1, 6, -1, 8, -1, 10, -1, 12, -1, -1]


TREE_SHAPES = ("leaf", "right_chain", "left_chain", "bfs", "preorder", "unbalanced")
# the bfs tree's node -> the pre-order tree's node
BFS_TO_PREORDER = (0, 1, 4, 2, 3, 5, 6)
CHAIN_REAL = (0, 2, 5, 9, 20, 40, 62)       # the chain's internal nodes with a real threshold


def tree_depth(t, node=0):
    return 0 if t["left"][node] < 0 else 1 + max(tree_depth(t, int(t["left"][node])), tree_depth(t, int(t["right"][node])))


def noise_tree(shape, window, seed, lo=0, hi=15):
    """A tree of `shape` on window (m, n, C): seeded features -- the root's (m - 1, n - 1, C - 1) --, integer thresholds in
    lo + 4 .. hi - 4; a chain's nodes pass everything on (lo - 1 / hi + 1) but for CHAIN_REAL."""
    m, n, C = window
    left, right = tree_links(shape)
    rng = np.random.default_rng(seed)
    k = len(left)
    feature = np.zeros((k, 3), np.int64)
    threshold = np.full(k, -2.0)
    internal = [i for i in range(k) if left[i] >= 0]
    for j, i in enumerate(internal):
        feature[i] = (rng.integers(0, m), rng.integers(0, n), rng.integers(0, C)) if j else (m - 1, n - 1, C - 1)
        threshold[i] = rng.integers(lo + 4, hi - 3)
        if shape.endswith("chain"):             # real nodes pass about 0.7 of the windows on: a few per hundred reach the end
            real = rng.integers(lo + 3, lo + 7) if shape == "right_chain" else rng.integers(hi - 6, hi - 2)
            threshold[i] = real if j in CHAIN_REAL else (lo - 1 if shape == "right_chain" else hi + 1)
    if shape == "preorder":                                          # the bfs tree of the same seed, renumbered
        b = noise_tree("bfs", window, seed, lo, hi)
        for i, p in enumerate(BFS_TO_PREORDER):
            feature[p], threshold[p] = b["feature"][i], b["threshold"][i]
    return _tree(feature, threshold, left, right)


def split_node(feature, threshold):
    """One split node and two leaves (predictions: -10, -8.25, -6.5 ... whatever _tree gives; left is node 1)."""
    return _tree([feature, (0, 0, 0), (0, 0, 0)], [threshold, -2, -2], [1, -1, -1], [2, -1, -1])


def window_origins(u, v, m, n, N, seed):
    """(rs, cs) int32 [N] of windows inside a u x v image: (u - m, v - n) first, then the other corners, then seeded ones."""
    rng = np.random.default_rng(seed)
    pos = [(u - m, v - n), (0, 0), (0, v - n), (u - m, 0)]
    pos += list(zip(rng.integers(0, u - m + 1, N).tolist(), rng.integers(0, v - n + 1, N).tolist()))
    pos = pos[:N]
    return np.array([p[0] for p in pos], np.int32), np.array([p[1] for p in pos], np.int32)


def noise_image(u, v, C, dtype, seed, hi=15):
    return np.random.default_rng(seed).integers(0, hi + 1, (u, v, C)).astype(dtype)


# (name, image shape, window, count): every count, every C and both dtypes at small windows; the big features
WALK_CELLS = (
    ("c1", (19, 31, 1), (5, 4, 1), 513), ("c3", (19, 31, 3), (5, 4, 3), 257), ("c4", (19, 31, 4), (3, 7, 4), 256),
    ("c3/255", (19, 31, 3), (5, 4, 3), 255), ("c4/1", (19, 31, 4), (3, 7, 4), 1),
    ("rows130", (140, 140, 1), (130, 2, 1), 257), ("cols130", (140, 140, 1), (2, 130, 1), 257), ("chan200", (9, 11, 200), (1, 1, 200), 257),
)
WALK_CELL = {c[0]: c for c in WALK_CELLS}
BIG_FEATURES = {"rows130": ((129, 1, 0), (128, 0, 0), (1, 1, 0)), "cols130": ((1, 129, 0), (0, 128, 0), (1, 1, 0)),
                "chan200": ((0, 0, 199), (0, 0, 128), (0, 0, 71))}


@functools.lru_cache(None)
def walk_design(cell, shape, dtype):
    """dict(image [u, v, C], rs, cs, window, tree): windows (rs[i], cs[i]) of `image` for wb_tree_eval_launch; samples()
    gives the same windows as crops for wb_tree_apply_launch."""
    name, (u, v, C), window, N = WALK_CELL[cell]
    seed = 17 * WALK_CELLS.index(WALK_CELL[cell]) + TREE_SHAPES.index(shape)
    tree = noise_tree(shape, window, seed)
    if cell in BIG_FEATURES:                      # the first three internal nodes read the features with bit 7 set
        internal = np.flatnonzero(tree["left"] >= 0)
        for i, f in zip(internal, BIG_FEATURES[cell]):
            tree["feature"][i] = f
    rs, cs = window_origins(u, v, window[0], window[1], N, seed)
    return dict(image=noise_image(u, v, C, dtype, seed + 5), rs=rs, cs=cs, window=window, tree=tree)


def samples(d):
    return orc.gather_samples(d["image"], d["rs"], d["cs"], d["window"])


def as_image(X):
    """Samples [N, m, n, C] stacked along the rows: an image of N * m x n whose window i starts at (i * m, 0)."""
    N, m, n, C = X.shape
    return X.reshape(N * m, n, C), (np.arange(N) * m).astype(np.int32), np.zeros(N, np.int32)


# ---- ties
TIE_VALUES = np.array([1.5, -3.25, 100.0, 0.0, -0.0, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], np.float32)
TIE_WINDOWS = ((2, 3, 1), (2, 3, 3), (2, 3, 4))
U8_VALUES = np.array([0, 1, 254, 255], np.uint8)
U8_THRESHOLDS = np.array([-1e-45, -0.0, 0.0, 0.5, 254.5, 255.0, float(np.nextafter(np.float32(255), np.float32(np.inf)))], np.float32)


def tie_thresholds():
    """float32: every finite or infinite TIE_VALUE, the float32 above it and the one below it, and NaN -- by bits, so that
    0.0 and -0.0 both stay."""
    v = TIE_VALUES[~np.isnan(TIE_VALUES)]
    t = np.concatenate([v, _up(v), _down(v)])
    bits = np.unique(t.view(np.uint32))
    return np.concatenate([bits.view(np.float32), np.array([np.nan], np.float32)])


def tie_samples(dtype, window):
    """One sample per value: the value at (m - 1, n - 1, C - 1), 7 everywhere else."""
    vals = U8_VALUES if np.dtype(dtype) == np.uint8 else TIE_VALUES
    X = np.full((vals.size,) + tuple(window), 7, dtype)
    X[:, -1, -1, -1] = vals
    return X


def tie_tree(window, threshold):
    m, n, C = window
    return split_node((m - 1, n - 1, C - 1), threshold)


# ------------------------------------------------------------------------------ the walks, restated
WRONG_WALK = ("lt_for_le", "nan_goes_left", "flushing_compare", "children_swapped", "cap_3_steps", "cap_7_steps", "child_unsigned",
              "feature_mask_127", "feature_row_col_swapped", "window_pitch_for_image")


def _flush(x):
    x = _f32(x)
    return np.where(np.abs(x) < FLT_MIN, np.copysign(np.float32(0), x), x)


def _goes_left(x, thr, wrong):
    with np.errstate(invalid="ignore"):
        if wrong == "lt_for_le":
            return x < thr
        if wrong == "nan_goes_left":
            return ~(x > thr)
        if wrong == "flushing_compare":
            return _flush(x) <= _flush(thr)
        return x <= thr


def walk_leaf(tree, fetch, N, wrong=None):
    """tree_leaf of the kernel for N windows at once: fetch(fr, fc, ch) -> float32 [N] with per-window feature arrays."""
    f, thr = tree["feature"].astype(np.int64), tree["threshold"]
    k = thr.size
    conv = (lambda a: a.view(np.uint8).astype(np.int64)) if wrong == "child_unsigned" else (lambda a: a.astype(np.int64))
    L, R = conv(tree["left"]), conv(tree["right"])
    mask = 127 if wrong == "feature_mask_127" else 255
    steps = {"cap_3_steps": 3, "cap_7_steps": 7}.get(wrong, k)
    node = np.zeros(N, np.int64)
    done = np.zeros(N, bool)
    for _ in range(steps):
        nd = node % k                                # (only a wrong kernel leaves the arrays)
        l = L[nd]
        done |= l < 0
        if done.all():
            break
        fr, fc, ch = f[nd, 0] & mask, f[nd, 1] & mask, f[nd, 2] & mask
        if wrong == "feature_row_col_swapped":
            fr, fc = fc, fr
        go = _goes_left(fetch(fr, fc, ch), thr[nd], wrong)
        if wrong == "children_swapped":
            go = ~go
        node = np.where(done, node, np.where(go, l, R[nd]))
    return node


def tree_apply_kernel(tree, X, wrong=None):
    """tree_apply_kernel: int32 [N] leaf indices of samples X [N, m, n, C]."""
    N, m, n, C = X.shape
    flat = X.reshape(-1)
    base = np.arange(N, dtype=np.int64) * (m * n * C)
    fetch = lambda fr, fc, ch: flat[(base + ((fr * n + fc) * C + ch)) % flat.size].astype(np.float32)
    return walk_leaf(tree, fetch, N, wrong).astype(np.int32)


def tree_eval_kernel(tree, image, rs, cs, window=None, wrong=None):
    """tree_eval_kernel: float32 [N] predictions of the windows at (rs, cs) (window: only the wrong pitch needs it)."""
    u, v, C = image.shape
    flat = image.reshape(-1)
    pitch = window[1] if wrong == "window_pitch_for_image" else v
    r, c = rs.astype(np.int64), cs.astype(np.int64)
    fetch = lambda fr, fc, ch: flat[(((r + fr) * pitch + (c + fc)) * C + ch) % flat.size].astype(np.float32)
    return tree["prediction"][walk_leaf(tree, fetch, rs.size, wrong) % tree["prediction"].size]


# ------------------------------------------------------------------------------ cascades on samples
WRONG_PREDICT = ("gt_for_ge", "neg_inf_theta_compared", "fp64_sum", "rejected_keeps_sum")


def predict_kernel(window, trees, thetas, X, wrong=None):
    """samples_predict_kernel: (H float32 [N], mask uint8 [N])."""
    N = X.shape[0]
    assert tuple(X.shape[1:]) == tuple(window)
    acc = np.float64 if wrong == "fp64_sum" else np.float32
    h = np.zeros(N, acc)
    alive = np.ones(N, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for tree, th in zip(trees, thetas):
            p = tree["prediction"][tree_apply_kernel(tree, X)].astype(acc)
            h = np.where(alive, h + p, h)
            th = np.float32(th)
            if wrong == "gt_for_ge":
                ok = h > th
            else:
                ok = h >= th
            if wrong != "neg_inf_theta_compared":
                ok = ok | (th == np.float32(-np.inf))
            alive = alive & ok
        H = h.astype(np.float32)
    if wrong != "rejected_keeps_sum":
        H = np.where(alive, H, np.float32(-np.inf))
    return H, alive.astype(np.uint8)


NEG = -np.inf
# name -> (leaves of path A, leaves of path B, thetas); None: see score_design
_SCORES = {
    # theta exactly the running sum of path A (>=: it survives every stage); B falls a quarter short at stage 2
    "ge_exact": ([0.25, 0.5, -0.25, 1.75], [0.25, 0.5, -0.5, 1.75], "A"),
    # one float32 above A's running sum at stage 1 (A is rejected there), below B's
    "ulp_above": ([0.25, 0.5, 0.25], [0.25, 0.75, 0.25], "A+1@1"),
    "ulp_below": ([0.25, 0.5, 0.25], [0.25, 0.25, 0.25], "A-1@1"),
    # fp32 absorbs the 1 into 1e8: A sums to 1 (2 in fp64), which the last theta 1.5 rejects; B = -1e8, 1, 1e8, 1 likewise
    "absorb": ([1e8, 1, -1e8, 1], [-1e8, 1, 1e8, 1], [NEG, NEG, NEG, 1.5]),
    # the same without a rejection: the sums themselves come back, 1.25 where fp64 gives 2.25
    "absorb_kept": ([1e8, 1, -1e8, 1.25], [0.5, 1e8, -1e8, 1], [NEG, NEG, NEG, NEG]),
    "inf_leaves": ([np.inf, 1.0], [-np.inf, 1.0], [NEG, 0.0]),
    # inf then -inf: a NaN score; a free stage keeps it (mask 1, H NaN), B stays finite
    "nan_free": ([np.inf, -np.inf, 0.25], [1.0, 1.0, 0.25], [NEG, NEG, NEG]),
    "nan_finite_theta": ([np.inf, -np.inf, 0.25], [1.0, 1.0, 0.25], [NEG, NEG, 0.0]),
    "nan_nan_theta": ([np.inf, -np.inf, 0.25], [1.0, 1.0, 0.25], [NEG, NEG, np.nan]),
    # theta +inf: a finite score is rejected, a +inf score passes (inf >= inf)
    "theta_inf": ([1.0], [np.inf], [np.inf]),
    "empty": ([], [], []),
}
SCORE_DESIGNS = tuple(_SCORES) + ("shapes", "shapes_shallow", "ties")
# (name, window, dtype of the samples): every SCORE_DESIGN runs at each
MODEL_CELLS = (("w231/f32", (2, 3, 1), np.float32), ("w231/u8", (2, 3, 1), np.uint8), ("w543/f32", (5, 4, 3), np.float32),
               ("w374/u8", (3, 7, 4), np.uint8), ("w374/f32", (3, 7, 4), np.float32), ("chan200/u8", (1, 1, 200), np.uint8),
               ("chan200/f32", (1, 1, 200), np.float32), ("rows130/f32", (130, 2, 1), np.float32), ("cols130/u8", (2, 130, 1), np.uint8))
MODEL_CELL = {c[0]: c for c in MODEL_CELLS}
# (design, cell) -> the error text wb_model_create refuses it with: none of these shapes is refused
REFUSED = {}


def model_count(design, cell):
    return COUNTS[(SCORE_DESIGNS.index(design) + [c[0] for c in MODEL_CELLS].index(cell)) % len(COUNTS)]


@functools.lru_cache(None)
def score_design(design, cell):
    """dict(window, trees, thetas float32 [T], X [N, m, n, C], generic): one cascade and its samples.  Two-path designs: every
    stage splits on pixel (0, 0, 0) <= 0.5; path A's samples hold 0 there, path B's 1, in the pattern A B B A B A A A ..."""
    _, window, dtype = MODEL_CELL[cell]
    m, n, C = window
    N = model_count(design, cell)
    seed = 31 * SCORE_DESIGNS.index(design) + len(cell)
    if design in ("shapes", "shapes_shallow"):
        shapes = TREE_SHAPES if design == "shapes" else ("leaf", "bfs", "preorder", "leaf", "bfs")
        trees = [noise_tree(s, window, seed + i) for i, s in enumerate(shapes)] * 2             # T = 12 / 10
        if cell[:7] in BIG_FEATURES:
            for t in trees:
                for i, f in zip(np.flatnonzero(t["left"] >= 0), BIG_FEATURES[cell[:7]]):
                    t["feature"][i] = f
        # thetas: free stages, and floors at multiples of 0.25 around where the running sums lie (ties with `>=` happen)
        X = noise_image(N, m * n, C, dtype, seed + 3).reshape(N, m, n, C)
        thetas, h = [], np.zeros(N, np.float32)
        for i, t in enumerate(trees):
            h = h + t["prediction"][orc.tree_apply(t, X)]
            thetas.append(NEG if i % 3 == 0 else float(np.sort(h)[N // 5]))                     # an attained sum: a tie
        return dict(window=window, trees=trees, thetas=np.array(thetas, np.float32), X=X, generic=design == "shapes" or C == 200)
    if design == "ties":
        # the float32 / uint8 tie values under three split nodes at (m - 1, n - 1, C - 1), thresholds a value, its upper
        # neighbour and NaN; all stages free, so H is the sum of three leaves
        X = tie_samples(dtype, window)
        th = [1.0, _up(1.0), np.nan] if np.dtype(dtype) == np.uint8 else [1e-40, -0.0, np.nan]
        trees = [tie_tree(window, t) for t in th]
        return dict(window=window, trees=trees, thetas=np.full(3, NEG, np.float32), X=X, generic=C == 200)
    a, b, th = _SCORES[design]
    T = len(a)
    trees = []
    for i in range(T):
        t = split_node((0, 0, 0), 0.5)
        t["prediction"][1], t["prediction"][2] = a[i], b[i]
        trees.append(t)
    with np.errstate(invalid="ignore"):
        run = np.cumsum(np.array(a, np.float32), dtype=np.float32) if T else np.zeros(0, np.float32)
    if th == "A":
        th = run.copy()
    elif isinstance(th, str):
        th = np.full(T, NEG, np.float32)
        th[1] = _up(run[1]) if "+1" in _SCORES[design][2] else _down(run[1])
    thetas = np.array(th, np.float32)
    X = noise_image(N, m * n, C, dtype, seed, hi=9).reshape(N, m, n, C)
    i = np.arange(N)
    X[:, 0, 0, 0] = ((i * i + i // 3) % 8 < 4).astype(dtype) if N > 1 else 0                      # path B where 1; N = 1: path A
    return dict(window=window, trees=trees, thetas=thetas, X=X, generic=C == 200)


def flat_arrays(trees):
    """The arrays wb_model_create takes: (node_off int32 [T + 1], feature uint8, threshold, left int8, right int8,
    prediction)."""
    off = np.zeros(len(trees) + 1, np.int32)
    for i, t in enumerate(trees):
        off[i + 1] = off[i] + t["left"].size
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([t[k].reshape(-1) for t in trees]).astype(dt)) if trees else np.zeros(0, dt)
    return off, cat("feature", np.uint8), cat("threshold", np.float32), cat("left", np.int8), cat("right", np.int8), cat("prediction", np.float32)


def same_floats(a, b):
    """Equal by bits, a NaN equal to any NaN (x86 makes 0xFFC00000, the GPU 0x7FC00000)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


# ------------------------------------------------------------------------------ what the host test found
# wrong kernel -> number of bytes / windows / samples it gets wrong over the designs it is named for
# (test_sample_designs_host.py says which those are and asserts every entry)
RECORDED = {
    "crop/pitch_n": 15410495, "crop/rows_cols_swapped": 15864426, "crop/cs_unscaled": 9530557, "crop/tail_dropped": 4208768,
    "crop/stride_16": 21498334,
    "walk/lt_for_le": 1500, "walk/nan_goes_left": 111, "walk/flushing_compare": 54, "walk/children_swapped": 20520,
    "walk/cap_3_steps": 4050, "walk/cap_7_steps": 2550, "walk/child_unsigned": 24552, "walk/feature_mask_127": 4136,
    "walk/feature_row_col_swapped": 11550, "walk/window_pitch_for_image": 12656,
    # tie launches (float32, uint8) of the first tie window that a wrong compare gets wrong
    "tie_launches": {"lt_for_le": (11, 3), "nan_goes_left": (26, 0), "flushing_compare": (8, 1)},
    "predict/gt_for_ge": 3437, "predict/neg_inf_theta_compared": 1277, "predict/fp64_sum": 4615, "predict/rejected_keeps_sum": 10378,
}
