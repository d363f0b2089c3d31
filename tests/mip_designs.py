"""Designed inputs for the kernels of multiple-instance pruning (csrc/wb_mip.hip: wb_mip_windows_launch,
wb_mip_prune_launch).  No GPU, no torch.

Window designs are pure geometry: level sizes, 1 / scale per level and ground-truth boxes whose IoUs with the windows are
small rationals.  Prune designs plant the trace itself: which window holds the smallest bag maximum of every stage, and
which windows fall when.

tests/test_mip_designs_host.py proves what the designs claim (exact rational arithmetic, an independent bag-by-bag
evaluation) and that they tell wrong kernels from the statement (tests/mip_reference.py); tests/test_gpu_mip_designs.py
runs them on the GPU.
"""
import functools

import numpy as np

WG, WAVE = 256, 64                      # windows per workgroup and per wave of the kernels
M = N_ = 12                             # the window of the window designs: 12 x 12


# ----------------------------------------------------------------------------------------------- window designs
class WindowDesign:
    """name; levels [(u, v)]; inv_scale float32 per level; gts / ignores per image; min_iou; what it claims: reachable
    and unreachable (image, index) pairs; exact_half: the windows (image, level, r, c) -> owner whose best IoU is 1/2
    exactly (excluded at min_iou = 0.5, included one rounding below it); hits: windows that must be rows, with their
    owner; absent: windows that must not be."""

    def __init__(self, name, min_iou, reachable, unreachable, exact_half, hits, absent):
        self.name, self.min_iou = name, min_iou
        self.levels = [(40, 56), (20, 28), (13, 30), (12, 40), (11, 30)]      # 28 x 44, 8 x 16 and 1 x 18 windows; none; none
        self.inv_scale = np.array([1.0, 2.0, np.float32(10.0) / np.float32(3.0), 1.0, 2.0], np.float32)
        s = self.inv_scale[2]
        f = lambda v: float(np.float32(v) * s)                                 # wb_boxes_launch's float32 product, as a double
        image0 = [[4, 3, 28, 15],               # 0: twice a window's area (12 x 24): the windows inside it have IoU 1/2 exactly
                  [30, 20, 42, 32],             # 1: the level-0 window (20, 30) itself
                  [30, 20, 42, 32],             # 2: its twin: the first owns, so this one owns nothing
                  [0, 0, 24, 24],               # 3: the level-1 window (0, 0); ignored
                  [30, 14, 54, 38],             # 4: the level-1 window (7, 15): last row, last column of its grid
                  [43, 27, 55, 39],             # 5: the level-0 window (27, 43): last row, last column of its grid
                  [-100, -100, 300, 300],       # 6: too large for any level
                  [f(5), f(0), f(16), f(12)]]   # 7: eleven columns of the level-2 window (0, 5) (one row of windows, a non-dyadic scale)
        self.gts = [np.array(image0, np.float64), None]                         # the second image has no ground truth
        self.ignores = [np.array([0, 0, 0, 1, 0, 0, 0, 0], np.uint8), np.zeros(0, np.uint8)]
        self.reachable, self.unreachable = reachable, unreachable
        self.exact_half, self.hits, self.absent = exact_half, hits, absent


HALF_DOWN = float(np.nextafter(0.5, 0.0))
# windows (image, level, r, c) -> owner whose best IoU is 1/2 exactly (and whose owner is not ignored): the 13 level-0 windows
# inside box 0, the windows four columns or rows from box 1's and box 5's, the level-1 windows four columns or rows (8 pixels)
# from box 4's
EXACT_HALF = {**{(0, 0, 3, c): 0 for c in range(4, 17)}, (0, 0, 20, 26): 1, (0, 0, 20, 34): 1, (0, 0, 16, 30): 1, (0, 0, 24, 30): 1,
              (0, 1, 7, 11): 4, (0, 1, 3, 15): 4, (0, 0, 23, 43): 5, (0, 0, 27, 39): 5}
HITS = {(0, 0, 20, 30): 1, (0, 0, 21, 31): 1, (0, 1, 7, 15): 4, (0, 1, 6, 14): 4, (0, 0, 27, 43): 5, (0, 0, 26, 43): 5, (0, 0, 27, 42): 5,
        (0, 2, 0, 5): 7, (0, 2, 0, 4): 7, (0, 2, 0, 6): 7}
ABSENT = [(0, 1, 0, 0), (0, 1, 0, 1), (0, 1, 0, 2)]       # owned by the ignored box 3 (IoU 1, 11/13 and 5/7)


@functools.lru_cache(None)
def window_designs():
    pairs = lambda *ks: [(0, k) for k in ks]
    at = WindowDesign("half", 0.5, pairs(1, 4, 5, 7), pairs(0, 2, 6), EXACT_HALF, HITS, ABSENT + list(EXACT_HALF))
    above = WindowDesign("half-down", HALF_DOWN, pairs(0, 1, 4, 5, 7), pairs(2, 6), EXACT_HALF, {**HITS, **EXACT_HALF}, ABSENT)
    strict = WindowDesign("default", 0.7, pairs(1, 4, 5, 7), pairs(0, 2, 6), EXACT_HALF, HITS, ABSENT + list(EXACT_HALF))
    return {d.name: d for d in (at, above, strict)}


# ----------------------------------------------------------------------------------------------- prune designs
class PruneDesign:
    """name; trace (N, T) float32; bag (N,) int32; n_bags; recalls; what it claims: theta[recall] (T,) float32 and
    owners[recall] (T,): the window that alone holds stage t's smallest bag maximum (-1: not claimed), removed: {recall:
    {window: removed_at}}."""

    def __init__(self, name, trace, bag, n_bags, recalls=(1.0,), theta=None, owners=None, removed=None):
        self.name = name
        self.trace64 = np.asarray(trace, np.float64)              # as planned; the host test proves them float32 values
        self.trace = self.trace64.astype(np.float32)
        self.bag = np.asarray(bag, np.int32)
        self.N, self.T = self.trace.shape
        self.n_bags, self.recalls = int(n_bags), tuple(recalls)
        self.theta, self.owners, self.removed = theta or {}, owners or {}, removed or {}


def position_cycle(N):
    """Windows by their place in the launch: lane 0 and lane 63 of the first wave, the first lane of the second, the last
    window (the last lane of a partial wave), the first lane of the last wave and of the last workgroup, the last lane of the
    first workgroup, the window before the last, the first lane and the last lane of the first wave of the second workgroup."""
    want = [0, WAVE - 1, WAVE, N - 1, (N - 1) // WAVE * WAVE, (N - 1) // WG * WG, WG - 1, N - 2, WG, WG + WAVE - 1]
    out = []
    for i in want:
        if 0 <= i < N and i not in out:
            out.append(i)
    return out


def layout(kind, N):
    """bag (N,) and n_bags.  single: one window per bag;  blocks: bags of consecutive windows with edges on wave and
    workgroup boundaries, one of 129 windows, and a bag id nobody has;  interleaved: window i in bag i % 8 (129 windows in
    bag 0 at N = 1025)."""
    i = np.arange(N)
    if kind == "single":
        return i.astype(np.int32), N
    if kind == "interleaved":
        return (i % 8).astype(np.int32), 8
    edges = [e for e in (0, 64, 256, 385, 512, 1024) if e < N] + [N]           # [256, 385): 129 windows
    bag = np.zeros(N, np.int32)
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        bag[a:b] = k if k < 2 else k + 1                                        # id 2 is empty
    return bag, int(bag.max()) + 1


def owners_design(N, T, kind):
    """Stage t's smallest bag maximum belongs to owners[t] alone, a window chosen by its place in the launch: it takes
    v[t] = 40 - 5 t (negative from stage 9 on), the other windows of its bag less (they fall at that stage, if they have
    not before), every window of another bag something above 1000.  Owners of different stages sit in different bags or
    are the same window, so an owner is never removed."""
    bag, n_bags = layout(kind, N)
    chosen, used = [], set()
    for p in position_cycle(N):
        if int(bag[p]) not in used:
            used.add(int(bag[p]))
            chosen.append(p)
    owner = np.array([chosen[t % len(chosen)] for t in range(T)])
    i = np.arange(N)
    tr = np.zeros((N, T), np.float64)
    removed = np.full(N, T, np.int64)
    for t in range(T):
        o = owner[t]
        v = 40.0 - 5.0 * t
        tr[:, t] = 1000.0 + (i * 7 + t * 3) % 11
        mates = np.flatnonzero(bag == bag[o])
        tr[mates, t] = v - 1.0 - (mates % 3)
        tr[o, t] = v
        first = mates[(mates != o) & (removed[mates] == T)]
        removed[first] = t
    # recall 1: the floor is the smallest bag maximum of the last stage, v[T - 1]: the mates of the last owner are below it
    last = np.flatnonzero((bag == bag[owner[-1]]) & (i != owner[-1]))
    removed[last] = -1
    return PruneDesign(f"owners-{kind}-{N}x{T}", tr, bag, n_bags, recalls=(1.0, 0.5),
                       theta={1.0: (40.0 - 5.0 * np.arange(T)).astype(np.float32)}, owners={1.0: owner},
                       removed={1.0: {int(k): int(removed[k]) for k in range(N)}})


def features_design():
    """257 windows in bags of consecutive windows [0, 64), [64, 256), [256, 257) (ids 0, 1, 3; id 2 is empty); six stages;
    recall 0.6 keeps 2 of the 3 bags: the floor is 20, bag 0 is dropped; recall 1 keeps every bag.  At recall 0.6:

    bag 0 = [0, 64): wholly below the floor (final scores -8), with extreme scores (+-2^127) that play no part.
    bag 1 = [64, 256): final scores 20 -- tied at the floor, all retained -- except window 101 (3: never retained), which
        carries 7000 at stage 3: a kernel that applies the floor to bags only would take it for the bag's maximum.
    bag 3 = [256, 257): window 256, the last window and the last bag.
    stage 0: bag 1: 50 (windows 200 .. 255: 49), bag 3: 60: theta = 50 and windows 200 .. 255 fall.
    stage 1: bag 1: 30 + i % 3, but window 64, a holder of the maximum of stage 0, takes 5; bag 3: 32.5: theta = 32, and
        window 64 and the windows at 30 and 31 fall: 65, 68, 71, ... survive.  At stages 2 to 4 window 64 carries 5000, which
        a kernel that looks at removed windows would take for the bag's maximum.
    stage 2: a tie: bag 1's survivors all take 7, bag 3 takes 7: theta = 7, nobody falls.
    stage 3: bag 1: -3, but windows 68 and 71 take -2.5 and window 74 one float32 below it; bag 3: -1: theta = -2.5; window
        71 sits exactly at theta and stays, window 74 and the windows at -3 fall.
    stage 4: bag 1: window 68 takes -0.0, window 71 -1; bag 3: +0.0: theta is -0.0 (it is below +0.0 in the keys' order),
        window 256 stays (+0.0 >= -0.0), window 71 falls.
    stage 5 (the final scores): bag 1's maximum 20, bag 3's 30: theta = 20."""
    N, T = 257, 6
    bag = np.zeros(N, np.int32)
    bag[64:256], bag[256] = 1, 3
    tr = np.zeros((N, T), np.float64)
    down = float(np.nextafter(np.float32(-2.5), np.float32(-np.inf)))
    b1 = np.arange(64, 256)
    tr[b1, 0] = 50.0
    tr[200:256, 0] = 49.0
    tr[b1, 1] = 30.0 + (b1 % 3)
    tr[b1, 2] = 7.0
    tr[b1, 3] = -3.0
    tr[68, 3] = tr[71, 3] = -2.5
    tr[74, 3] = down
    tr[b1, 4] = -1.0
    tr[68, 4] = -0.0
    tr[b1, 5] = 20.0
    tr[64, 1], tr[64, 2:5] = 5.0, 5000.0
    tr[101, 3], tr[101, 5] = 7000.0, 3.0
    tr[256] = [60.0, 32.5, 7.0, -1.0, 0.0, 30.0]
    tr[:64, :5] = np.where(np.arange(64)[:, None] % 2 == 0, 2.0 ** 127, -2.0 ** 127)
    tr[:64, 5] = -8.0
    return PruneDesign("features-257x6", tr, bag, 4, recalls=(0.6, 1.0),
                       theta={0.6: np.array([50.0, 32.0, 7.0, -2.5, -0.0, 20.0], np.float32)},
                       owners={0.6: np.array([-1, -1, -1, -1, 68, -1])},
                       removed={0.6: {0: -1, 63: -1, 101: -1, 64: 1, 200: 0, 255: 0, 66: 1, 67: 1, 65: 3, 74: 3, 71: 4, 68: 6, 256: 6}})


GRID = [(1, 1, "single"), (63, 2, "single"), (64, 24, "interleaved"), (65, 1, "blocks"), (257, 24, "blocks"), (257, 2, "interleaved"),
        (1025, 24, "blocks"), (1025, 2, "interleaved"), (1025, 1, "single"), (65, 24, "interleaved"), (63, 24, "blocks"), (64, 2, "blocks")]


@functools.lru_cache(None)
def prune_designs():
    out = [owners_design(N, T, kind) for N, T, kind in GRID] + [features_design()]
    assert {d.N for d in out} >= {1, 63, 64, 65, 257, 1025} and {d.T for d in out} >= {1, 2, 24}
    return {d.name: d for d in out}
