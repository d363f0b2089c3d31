"""Designed survivor maps for the cascade kernels (NumPy only: no GPU, no torch).

A test that scans a random image under a random cascade leaves to chance how many windows a tile keeps behind stage
8 and 16, which lanes, rows and waves hold them, and whether a tile sits just under or over the survivor queue's
capacity.  Here the test decides, window by window, at which stage each window dies, and knows the answer in closed form.

The map.  Channel 0 of the channel image X[u, v, C] carries the map: pixel X[r, c, 0] is the top-left pixel of window
(r, c) -- and of no other window -- and holds that window's death stage D[r, c] (NEVER = 255: it never dies).
Stage t of the designed cascade has the root feature (0, 0, 0) with threshold t; every leaf under the root's left child
(X <= t) predicts -1000; the right subtree has depth 0 .. depth-1, tests random features of the noise channels 1..C-1
and has leaves |p| <= 1.  theta[t] is -500, or -inf for the stages named `free`.  So a window alive at stage t is
rejected there exactly when D <= t and t is not free: it dies at the first non-free stage >= D (eff_stage), or survives
when there is none; alive[t] is a count over D and the detections are the windows without such a stage, row-major.
Survivors that passed a free stage carry -1000 terms, which partly absorb their later small leaves: the order of the
fp32 accumulation is observable in the score bits.

The bait.  Pixels of channel 0 that are no window's origin (rows >= u - m, columns >= v - n) hold NEVER: a kernel that
evaluates or emits an out-of-grid lane produces an extra record.

Ranks.  Channel 0's thresholds are 0 .. T-1, so the rank of an integer D is min(D, T); the noise channels are ranked
with np.searchsorted among their sorted distinct thresholds.  One uint8 design yields the float32, uint8, RANK8 and RANK16
tile inputs.
"""
import numpy as np

from oracle import wb_oracle as orc

# ---- the kernel's regime constants, each read from ONE place here
# (paths below: waldboost_amd/csrc/)
TILE_COLS = 64            # WB_CASC_TC (wb_common.h): windows per tile row = lanes of a wave
PHASE_A = 8               # S0 in wb_cascade_tile.h: dense stages before the workgroup-wide re-pack
WAVES = 8                 # wb_model.hip, choose_geometry: `int rpw = 4, waves = 8;` (tile_rows = rpw * waves); wb_model_info does
#                           not report it: the GPU module checks it, and queue_cap with it, through lds_bytes() below
GENERIC_WAVES = 4         # ... and `M->waves = 4` for the node-walk kernel (tile_rows 4)
SPAR = (32, 8, 16, 2)     # wb_cascade.hip, CascEnv: `int spar[4] = {32, 8, 16, 2};`
SPAR_WG = 32              # same function: `... atoi(getenv("WB_CASC_SPAR_WG")) : 32`
NEVER = 255               # a death stage no cascade here reaches (T <= 200), and a valid uint8 pixel
REJECT = -1000.0
THETA = -500.0

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 24, 33, 64, 65, 73, 130, 200)
FREE_STAGES = (7, 8, 15, 16)


def queue_cap(tile_rows, waves=WAVES):
    """Entries of a workgroup's survivor queue: wb_casc_qcap in wb_cascade_tile.h."""
    return min(tile_rows * TILE_COLS, TILE_COLS * waves + 512)


def lds_bytes(shape, tile_rows, waves, T, depth):
    """WbModelInfo.lds_bytes of a tile-kernel model (wb_cascade_lds_bytes for the float32 tile): the channel tile, the
    survivor queue of queue_cap(tile_rows, waves) entries, the per-stage counters, the stage mirror, the control words.
    The one field of wb_model_info that the wave count and the queue capacity show in."""
    m, n, C = shape
    ni, nl = (1 << depth) - 1, 1 << depth
    sd = (2 * ni + nl + 1 + 3) // 4 * 4                           # WB_STAGE_DWORDS
    mirror = T if T * sd * 4 <= 16 * 1024 else 0
    tile = C * (tile_rows + m - 1) * (TILE_COLS + n) * 4
    return (tile + queue_cap(tile_rows, waves) * 8 + T * 4 + 15) // 16 * 16 + mirror * sd * 4 + 256


# --------------------------------------------------------------------------- the designed cascade
class Cascade:
    """shape, stage arrays [(feature, threshold, left, right, prediction)], theta, free (set of stages with theta -inf)."""

    def __init__(self, shape, stages, theta, free, depth):
        self.shape, self.stages, self.theta, self.free, self.depth = tuple(shape), stages, theta, frozenset(free), depth
        self.T = len(stages)
        self.name = f"designed(shape={self.shape}, T={self.T}, depth={depth}, free={sorted(self.free)})"

    def model(self):
        """The cascade as a waldboost_amd.Model of DTree stages."""
        import waldboost_amd as wb
        M = wb.Model(self.shape, dict(wb.default_channel_opts))
        for arrays, th in zip(self.stages, self.theta):
            M.append(wb.DTree(*arrays), th)
        return M

    def oracle(self):
        """(shape, trees, thetas) in the oracle's plain form."""
        return self.shape, [orc.make_tree(*a) for a in self.stages], list(self.theta)


def _grow(rng, shape, depth, leaf, nodes):
    """Append a subtree of `depth` in pre-order (parent index < child index); leaf() gives the leaf values."""
    m, n, C = shape
    at = len(nodes)
    if depth == 0:
        nodes.append([(0, 0, 0), 0.0, -1, -1, leaf()])
        return at
    # noise features: any pixel of channels 1..C-1; thresholds on a grid of 1.5 (integer and half-integer, < 254 distinct)
    node = [(int(rng.integers(0, m)), int(rng.integers(0, n)), int(rng.integers(1, C))), float(rng.integers(1, 160)) * 1.5,
            -1, -1, 0.0]
    nodes.append(node)
    node[2] = _grow(rng, shape, depth - 1, leaf, nodes)
    node[3] = _grow(rng, shape, depth - 1, leaf, nodes)
    return at


def designed_cascade(shape, T, depth, free=(), seed=0):
    assert shape[2] >= 2 and 1 <= depth and T < NEVER
    rng = np.random.default_rng([seed, T, depth])
    free = frozenset(t for t in free if 0 <= t < T)
    stages = []
    for t in range(T):
        nodes = [[(0, 0, 0), float(t), -1, -1, 0.0]]
        # (every third stage carries the full depth, so the model's depth is `depth` for any T >= 1)
        nodes[0][2] = _grow(rng, shape, int(rng.integers(0, depth)), lambda: REJECT, nodes)
        nodes[0][3] = _grow(rng, shape, depth - 1 if t % 3 == 0 else int(rng.integers(0, depth)),
                            lambda: float(np.float32(rng.uniform(-1.0, 1.0))), nodes)
        stages.append((np.array([x[0] for x in nodes], np.uint8), np.array([x[1] for x in nodes], np.float32),
                       np.array([x[2] for x in nodes], np.int8), np.array([x[3] for x in nodes], np.int8),
                       np.array([x[4] for x in nodes], np.float32)))
    theta = [float("-inf") if t in free else THETA for t in range(T)]
    return Cascade(shape, stages, theta, free, depth)


# --------------------------------------------------------------------------- the closed form
def eff_stage(D, T, free):
    """The stage that rejects a window of death stage D: the first non-free stage >= D, T when there is none."""
    lut = np.full(256, T, np.int64)
    for d in range(T - 1, -1, -1):
        lut[d] = lut[d + 1] if d in free else d
    return lut[np.asarray(D, np.uint8)]


def entering(D, T, free, t):
    """Windows of the map D that enter stage t (t = T: the survivors)."""
    return int((eff_stage(D, T, free) >= t).sum())


def closed_form(D, T, free):
    """(alive[T], rs, cs): windows entering each stage, and the survivors in row-major order."""
    e = eff_stage(D, T, free)
    below = np.cumsum(np.bincount(e.reshape(-1), minlength=T + 1))           # below[t] = windows with eff <= t
    alive = (e.size - np.concatenate([[0], below[:T - 1]])).astype(np.int64) if T else np.zeros(0, np.int64)
    rs, cs = np.nonzero(e == T)
    return alive, rs.astype(np.int64), cs.astype(np.int64)


def survivor_scores(casc, X, rs, cs):
    """The oracle's fp32 running sums of the windows (rs, cs) through ALL stages -- what cascade_predict_on_image leaves
    for its survivors (same trees, same stage order, one float32 add per stage); the host module proves them bit-equal."""
    _, trees, _ = casc.oracle()
    hs = np.zeros(rs.size, np.float32)
    for tree in trees:
        hs += orc.tree_predict_on_image(tree, X, rs, cs)
    return hs


# --------------------------------------------------------------------------- channel and rank images
def channel_image(D, shape, seed=0):
    """uint8 X[nr + m, nc + n, C]: the map in channel 0 (bait = NEVER outside the window grid), noise elsewhere."""
    m, n, C = shape
    nr, nc = D.shape
    rng = np.random.default_rng([seed, nr, nc])
    X = rng.integers(0, 256, (nr + m, nc + n, C), dtype=np.uint8)
    X[..., 0] = NEVER
    X[:nr, :nc, 0] = D
    return X


def sorted_thresholds(casc):
    """Per channel: the distinct thresholds of the internal nodes, ascending."""
    out = [[] for _ in range(casc.shape[2])]
    for feature, threshold, left, _, _ in casc.stages:
        for i in np.flatnonzero(left >= 0):
            out[int(feature[i, 2])].append(threshold[i])
    return [np.unique(np.array(s, np.float32)) for s in out]


def rank_image(casc, X, dtype):
    """The threshold ranks of X as the channel kernel writes them, [u][v][4] of uint8 (RANK8) or uint16 (RANK16)."""
    assert casc.shape[2] == 4
    S = sorted_thresholds(casc)
    R = np.stack([np.searchsorted(S[c], X[..., c].astype(np.float32), side="left") for c in range(4)], -1)
    assert R.max() <= np.iinfo(dtype).max - 1
    return R.astype(dtype)


# --------------------------------------------------------------------------- tile patterns
class Tile:
    """One tile's map D[tile_rows, 64] with the regime it is named for: claims = [(stage, op, count)] on the number of
    its windows entering `stage`, checked from D alone (test_survivor_maps_host.py)."""

    def __init__(self, name, D, claims=()):
        self.name, self.D, self.claims = name, D, list(claims)


PLACEMENTS = ("first_rows", "last_rows", "first_wave", "last_wave", "lane0", "lane63", "random")


def placement_order(kind, TR, waves, rng):
    """All windows of a tile as flat indices r * 64 + lane, in the order a placement fills them."""
    r, c = np.divmod(np.arange(TR * TILE_COLS), TILE_COLS)
    rpw = max(TR // waves, 1)
    if kind == "first_rows":
        key = r * 64 + c
    elif kind == "last_rows":
        key = -(r * 64 + c)
    elif kind == "first_wave":                   # the rows of wave 0, lane by lane, then wave 1, ...
        key = ((r // rpw) * 64 + c) * rpw + r % rpw
    elif kind == "last_wave":
        key = -(((r // rpw) * 64 + (63 - c)) * rpw + r % rpw)
    elif kind == "lane0":
        key = c * TR + r
    elif kind == "lane63":
        key = (63 - c) * TR + r
    else:
        key = rng.permutation(r.size)
    return np.argsort(key, kind="stable")


def _dying_before(T, free, lo, hi, stop):
    """Death stages d in [lo, hi] whose rejecting stage exists and lies before `stop`."""
    d = np.arange(lo, min(hi, T - 1) + 1)
    return d[eff_stage(d, T, free) < min(stop, T)] if d.size else d


def steps_tile(name, TR, waves, T, free, steps, kind, rng, claims=None):
    """A staircase: steps = [(stage s_0, n_0), (s_1, n_1), ...] with s ascending and n descending: exactly n_i windows enter
    stage s_i; the first n_last windows of the placement never die, the others die at random stages in front of their
    step.  Stages s_i >= T are dropped (their windows never die)."""
    full = TR * TILE_COLS
    steps = [(s, min(n, full)) for s, n in steps if s < T]
    order = placement_order(kind, TR, waves, rng)
    D = np.empty(full, np.uint8)
    prev_s, prev_n = 0, full
    made = []
    for s, n in steps:
        pool = _dying_before(T, free, prev_s, s - 1, s)      # (d >= prev_s: these windows do enter stage prev_s)
        if n < prev_n:
            if pool.size == 0:
                raise ValueError(f"{name}: no stage in [{prev_s}, {s}) rejects, the step to {n} at stage {s} cannot be made")
            D[order[n:prev_n]] = rng.choice(pool, prev_n - n)
        made.append((s, "==", n))
        prev_s, prev_n = s, n
    # behind the last step: half die at random later stages, the rest (at least one when any are left) never
    rest = order[:prev_n]
    later = _dying_before(T, free, prev_s, T - 1, T)
    D[rest] = NEVER
    k = prev_n // 2 if later.size and prev_n > 1 else 0
    D[rest[prev_n - k:]] = rng.choice(later, k) if k else NEVER
    made.append((T, "==", prev_n - k))
    return Tile(name, D.reshape(TR, TILE_COLS), made if claims is None else claims(made))


def uniform_tiles(TR, T, free):
    """Every window of a tile dies at stage d: one tile per d in 0..T, and one for never."""
    full, out = TR * TILE_COLS, []
    for d in list(range(T + 1)) + [NEVER]:
        e = int(eff_stage(d, T, free))
        out.append(Tile(f"uniform[d={d}]", np.full((TR, TILE_COLS), d, np.uint8),
                        [(e, "==", full)] + ([(e + 1, "==", 0)] if e < T else [])))
    return out


def count_values(TR, waves):
    """The survivor counts behind phase A that the sweep visits."""
    cap, full, room = queue_cap(TR, waves), TR * TILE_COLS, queue_cap(TR, waves) - TILE_COLS * waves
    vals = [0, 1, 2, 3, SPAR[3], SPAR[1], SPAR_WG - 1, SPAR_WG, SPAR_WG + 1, 63, 64, 65, room - 1, room, room + 1,
            cap - 1, cap, cap + 1, full - 1, full]
    return sorted({v for v in vals if 0 <= v <= full})


def count_tiles(TR, waves, T, free, rng):
    """Exactly N windows of a full tile enter stage 8 and then die at d2 (or never); the rest die at random stages in
    phase A.  N over count_values, each in every placement; d2 paired with (N, placement) sparsely."""
    d2s = [d for d in (8, 9, 15, 16, 17, 31, 32, 33, T - 1) if PHASE_A <= d < T] + [NEVER]
    early = _dying_before(T, free, 0, PHASE_A - 1, PHASE_A)
    full = TR * TILE_COLS
    tiles = []
    for i, N in enumerate(count_values(TR, waves)):
        for j, kind in enumerate(PLACEMENTS):
            d2 = d2s[(i + 3 * j) % len(d2s)]
            order = placement_order(kind, TR, waves, rng)
            D = np.empty(full, np.uint8)
            n = N if early.size else full            # (a cascade whose phase A never rejects keeps every window)
            D[order[:n]] = d2
            D[order[n:]] = rng.choice(early, full - n) if early.size else NEVER
            claims = [(PHASE_A, "==", n)] if T > PHASE_A else []
            if d2 != NEVER and eff_stage(d2, T, free) < T:
                claims.append((int(eff_stage(d2, T, free)) + 1, "==", 0))
            else:
                claims.append((T, "==", n))
            tiles.append(Tile(f"count[N={N},{kind},d2={d2}]", D.reshape(TR, TILE_COLS), claims))
    return tiles


def staircase_tiles(TR, waves, T, free, rng):
    """Tiles that hold more than the queue at stage 8 and drop to cap + 1, cap or cap - 1 at the re-count at 16, 24 or 32
    -- or never drop, so the cascade ends on the dense state and emits from it.  (Only the 32-row tile has a queue smaller
    than its window count; for the others cap is the full count and the values are clipped to it.)"""
    cap, full = queue_cap(TR, waves), TR * TILE_COLS
    dense = cap < full
    tiles = []
    kinds = ("random", "last_rows", "lane63", "first_rows", "lane0", "last_wave", "first_wave")
    k = 0
    for r in (16, 24, 32):
        if r >= T:
            continue
        for v in (cap + 1, cap, cap - 1):
            for n8 in (full, cap + 1):
                steps = [(PHASE_A, n8)] + [(s, n8) for s in range(16, r, 8)] + [(r, min(v, n8))]
                if v > cap:
                    steps.append((r + 8, SPAR_WG + 1))
                kind = kinds[k % len(kinds)]
                k += 1

                def claims(made, r=r, v=v):
                    out = list(made)
                    if dense:                        # the regime by name: over the queue at every re-count in front of r
                        out += [(s, ">", cap) for s in range(PHASE_A, r, 8)]
                        out.append((r, ">" if v > cap else "<=", cap))
                    return out
                tiles.append(steps_tile(f"staircase[n8={n8},r={r},v={v},{kind}]", TR, waves, T, free, steps, kind, rng, claims))
    # never drops: more than the queue holds survive every stage (the dense emit), from every placement
    for kind in PLACEMENTS:
        for asked in ("cap+1", "full-1"):
            n = min(cap + 1 if asked == "cap+1" else full - 1, full)
            order = placement_order(kind, TR, waves, rng)
            early = _dying_before(T, free, 0, T - 1, T)
            D = np.full(full, NEVER, np.uint8)
            if early.size:
                D[order[n:]] = rng.choice(early, full - n)
            else:
                n = full
            claims = [(T, "==", n)] + ([(T, ">", cap)] if dense else [])
            tiles.append(Tile(f"dense_to_the_end[n={asked},{kind}]", D.reshape(TR, TILE_COLS), claims))
    # the second count (stage 16) around spar_wg, and the stage-parallel tail's entry counts
    for n16 in (0, 1, SPAR[3], SPAR[3] + 1, SPAR[1], SPAR[1] + 1, SPAR_WG - 1, SPAR_WG, SPAR_WG + 1):
        for n8 in (SPAR_WG + 1, 200, TILE_COLS * waves):
            kind = kinds[k % len(kinds)]
            k += 1
            tiles.append(steps_tile(f"second_count[n8={n8},n16={n16},{kind}]", TR, waves, T, free,
                                    [(PHASE_A, n8), (16, n16)], kind, rng))
    return tiles


def all_tiles(TR, waves, T, free, seed=0):
    rng = np.random.default_rng([seed, TR, T, len(free)])
    return uniform_tiles(TR, T, free) + count_tiles(TR, waves, T, free, rng) + staircase_tiles(TR, waves, T, free, rng)


def compose(tiles, TR, per_row=16, extra_rows=0, extra_cols=0, seed=0):
    """The tiles side by side and stacked, `per_row` across, as one window grid D[nr, nc] (spare tiles die at stage 0);
    extra_rows / extra_cols: a partial tile row / column of random deaths with survivors, so that full tiles have
    neighbours.  Returns (D, origins) with origins[k] = (r0, c0) of tile k."""
    rng = np.random.default_rng([seed, len(tiles)])
    ny = -(-len(tiles) // per_row)
    D = np.zeros((ny * TR + extra_rows, per_row * TILE_COLS + extra_cols), np.uint8)
    D[ny * TR:, :] = rng.choice(np.array([0, 3, 9, 20, NEVER], np.uint8), (extra_rows, D.shape[1]))
    D[:, per_row * TILE_COLS:] = rng.choice(np.array([0, 3, 9, 20, NEVER], np.uint8), (D.shape[0], extra_cols))
    origins = []
    for k, t in enumerate(tiles):
        ty, tx = divmod(k, per_row)
        D[ty * TR:(ty + 1) * TR, tx * TILE_COLS:(tx + 1) * TILE_COLS] = t.D
        origins.append((ty * TR, tx * TILE_COLS))
    return D, origins


def which_tile(r, c, TR, per_row, tiles):
    """Name of the composed tile that holds window (r, c): what a failing record is reported with."""
    k = (int(r) // TR) * per_row + int(c) // TILE_COLS
    return tiles[k].name if int(c) < per_row * TILE_COLS and k < len(tiles) else "edge"


# --------------------------------------------------------------------------- edge and partial grids
def edge_grids(TR):
    """Window grids (rows, cols) that end inside a tile, are thinner than one, or hold no window at all."""
    return [(TR + 1, 2 * TILE_COLS + 1), (1, 1), (1, 200), (100, 1), (TR - 1, TILE_COLS), (TR, TILE_COLS - 1), (0, 5), (3, 0),
            (2 * TR + 1, TILE_COLS + 1), (TR, TILE_COLS - 1), (TR - 1, TILE_COLS)]


DENSE_EDGES = 2           # the last levels of edge_grids: partial tiles on the dense continuation (dense_edge_map)


def dense_edge_map(nr, nc, TR, waves, T, free, kind, seed=0):
    """A partial tile (out-of-grid lanes or rows, bait next to them) that holds more than the queue behind phase A -- the
    regime of the recorded defect.  The last valid row and column never die.  kind "end": so many windows
    never die that the cascade ends on the dense state and emits from it; "drop": as many enter stages 8 and 16, then all
    but the border die at random later stages (they never die when no stage from 16 on rejects).  (Tiles whose queue holds every window: the same maps, no dense state.)"""
    rng = np.random.default_rng([seed, nr, nc, len(kind)])
    n, cap = nr * nc, queue_cap(TR, waves)
    keep = cap + 1 + (n - cap - 1) // 2 if n > cap else n
    border = np.zeros((nr, nc), bool)
    border[-1, :] = border[:, -1] = True
    inner = rng.permutation(np.flatnonzero(~border.reshape(-1)))
    kept, rest = inner[:keep - int(border.sum())], inner[keep - int(border.sum()):]
    D = np.full(n, NEVER, np.uint8)
    early = _dying_before(T, free, 0, PHASE_A - 1, PHASE_A) if kind == "drop" else _dying_before(T, free, 0, T - 1, T)
    if early.size:
        D[rest] = rng.choice(early, rest.size)
    if kind == "drop":
        late = _dying_before(T, free, 16, T - 1, T)
        if late.size:
            D[kept] = rng.choice(late, kept.size)
    return D.reshape(nr, nc)


def edge_map(nr, nc, T, kind, seed=0):
    """kind 0: survivors exactly in the last valid row and the last valid column (the bait is next to them), the others
    die at random stages; 1: survivors in the first and last lanes and rows, random deaths and a few survivors inside;
    2: random deaths only, and the four corners survive."""
    rng = np.random.default_rng([seed, nr, nc, kind])
    D = rng.integers(0, T, (nr, nc)).astype(np.uint8)
    if nr == 0 or nc == 0:
        return D
    if kind == 0:
        D[-1, :] = NEVER
        D[:, -1] = NEVER
    elif kind == 1:
        D[0, :] = NEVER
        D[:, 0] = NEVER
        D[-1, ::2] = NEVER
        D[::3, -1] = NEVER
        D[rng.random((nr, nc)) < 0.02] = NEVER
    else:
        D[0, 0] = D[0, -1] = D[-1, 0] = D[-1, -1] = NEVER
    return D


# --------------------------------------------------------------------------- the parametrisations both modules use
GEOMETRIES = {
    # window shape -> tile rows wb_model_create is expected to choose (its LDS budget halves rows-per-wave for large
    # windows; the GPU module reads the value back from wb_model_info and fails if it differs)
    (12, 12, 4): 32,
    (24, 24, 4): 16,
    (40, 24, 4): 8,
}


def scan_cases():
    """(shape, tile_rows, waves, T, depth, free): depth 2 at every length with and without free stages, depths 1 and 3 at
    every length with the free stages alternating; the two smaller tile geometries and the node-walk kernel (depth 4,
    4-row tiles) at a few lengths."""
    out = []
    for i, T in enumerate(LENGTHS):
        last = (T - 1,)
        out.append(((12, 12, 4), 32, WAVES, T, 2, ()))
        out.append(((12, 12, 4), 32, WAVES, T, 2, FREE_STAGES + last))
        out.append(((12, 12, 4), 32, WAVES, T, 1, FREE_STAGES + last if i % 2 else ()))
        out.append(((12, 12, 4), 32, WAVES, T, 3, () if i % 2 else FREE_STAGES + last))
    for shape, TR in list(GEOMETRIES.items())[1:]:
        for T, depth, free in ((9, 2, ()), (33, 1, FREE_STAGES), (40, 3, (15, 16, 39)), (130, 2, FREE_STAGES)):
            out.append((shape, TR, WAVES, T, depth, free))
    for T, free in ((7, ()), (17, FREE_STAGES), (73, (8, 72))):
        out.append(((12, 12, 4), 4, GENERIC_WAVES, T, 4, free))
    return out


def case_id(case):
    shape, TR, waves, T, depth, free = case
    return f"{shape[0]}x{shape[1]}-rows{TR}-T{T}-d{depth}-{'free' if free else 'strict'}"


def specialised_cases():
    """The scan cases whose byte forms are scanned again by their model-specialised kernels."""
    want = {((12, 12, 4), 16, 1), ((12, 12, 4), 7, 2), ((12, 12, 4), 9, 2), ((12, 12, 4), 73, 2), ((12, 12, 4), 200, 2),
            ((12, 12, 4), 33, 3), ((12, 12, 4), 130, 3), ((24, 24, 4), 130, 2), ((40, 24, 4), 9, 2)}
    out = []
    for case in scan_cases():
        key = (case[0], case[3], case[4])
        if key in want and (case[5] or key[1] in (9, 200)):          # (of depth 2's two variants: the one named here)
            want.discard(key)
            out.append(case)
    assert not want
    return out


def build_case(case, seed=0):
    """(cascade, tiles, per_row, D, X) of a scan case: every tile pattern of the case composed into one channel image,
    with a partial tile row and column at its far edges."""
    shape, TR, waves, T, depth, free = case
    casc = designed_cascade(shape, T, depth, free, seed)
    tiles = all_tiles(TR, waves, T, casc.free, seed)
    per_row = 16
    D, _ = compose(tiles, TR, per_row, extra_rows=1, extra_cols=1, seed=seed)
    return casc, tiles, per_row, D, channel_image(D, shape, seed)


def edge_levels(case, n_images=2, seed=0):
    """maps[b][l]: the edge grids of a case as the levels of one launch, a different map for every image and level."""
    shape, TR, waves, T, depth, free = case
    free = frozenset(t for t in free if 0 <= t < T)
    grids = edge_grids(TR)
    plain = len(grids) - DENSE_EDGES
    return [[edge_map(nr, nc, T, (b + l) % 3, seed + 7 * b) if l < plain else
             dense_edge_map(nr, nc, TR, waves, T, free, ("end", "drop")[(b + l) % 2], seed + 7 * b)
             for l, (nr, nc) in enumerate(grids)] for b in range(n_images)]


# --------------------------------------------------------------------------- the sample-side kernels on the same cascade
SAMPLE_T = 40
SAMPLE_FREE = FREE_STAGES + (SAMPLE_T - 1,)
SAMPLE_COUNTS = (1, 255, 256, 257, 3000)


def sample_case(depth, N, seed=0):
    """(cascade, D, X, rs, cs): N windows -- the first N, row-major, of a map of random death stages and survivors -- for
    Model.predict(gather_samples(X, rs, cs, shape)): mask is eff_stage(D[rs, cs]) == T in closed form."""
    casc = designed_cascade((12, 12, 4), SAMPLE_T, depth, SAMPLE_FREE, seed)
    nc = min(N, 50)
    nr = -(-N // nc)
    rng = np.random.default_rng([seed, N, depth])
    D = rng.choice(np.array(list(range(SAMPLE_T)) + [NEVER] * 8, np.uint8), (nr, nc))
    rs, cs = np.divmod(np.arange(N), nc)
    return casc, D, channel_image(D, casc.shape, seed), rs.astype(np.int64), cs.astype(np.int64)
