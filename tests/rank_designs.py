"""Designed threshold sets for the threshold-rank path: NumPy only, no torch, no GPU.

The channel kernel's epilogue writes rank(v) = #{thresholds of the channel below v} per channel value
(wb_common.h: wb_bin_cell, wb_bin_rank; the three epilogue paths in wb_channels.hip) from tables the host builds
(wb_stage_records.h: build_rank_tables).  This module restates both in NumPy -- mirror_tables, rank_by_tables -- and
holds threshold sets made so that ONE property of the tables or of the epilogue decides each of them.  A design is a
function of the pool: per channel the distinct values of the design image's oracle pyramid (96 x 160 uint8,
synth_image seed 21, shrink 2, smooth 1, one level per octave: 48 x 80 .. 6 x 10; on every channel 0.0 and some 2 400
values in (12, 116)).  A pixel can only be what the image yields, so interior thresholds are pool values or their
+-1-ulp neighbours (candidates); anchors, outliers and special values are free.  Each design carries what it is
expected to be -- the forms present, K (most thresholds in a cell) of each width, the trim index per channel: by
construction where the design is built for it, recorded from the mirror otherwise -- and the library's own tables
(WB_DUMP_RANKS) must equal the mirror's byte for byte (test_rank_designs_host.py).

What pins what, and the mistake it would reveal:
  * the 16/17 edge (narrow KMAX): k16 / k17 -- 16 or 17 neighbouring candidates in the cell [0, >= 128) of symmetric
    grids between anchors +-131072 j, enough anchors that no trim cuts them all off: k16 has rank8 at K = 16 (the
    longest narrow loop), k17 has none at any trim (and rank16 at K = 17: the wide limit is not 16).  A builder
    comparing < for <=, or an epilogue looping K - 1 times, fails here first.
  * the 64/65 edge (wide KMAX): wide_k64 (rank16 at K = 64, no rank8), wide_k65 (neither: float32 channels).
  * the 254/255 edge: full8 / over8, last_slot_full8(_inf) -- 254 thresholds on a channel are ranked in a byte
    (ranks 0 .. 254, 255 stays the NaN code), 255 are not; the rank group test takes two models whose union is 254 / 255.
  * the 1020/1021 edge: full16 / over16, last_slot_full16(_inf) -- likewise for two bytes; over16 has no form at all.
  * each trim level: trim0 .. trim3 (both widths), trim4 (narrow), wide_trim4 (wide) -- a cluster of thinned pool
    values between o outliers +-1e30 (j + 1) a side; a grid spanning an outlier holds the cluster in one cell, so
    trim i is the first to place the set exactly when its cut int(q n) first reaches o; the cut-off values land in
    the end cells (cut below lo in cell 0, cut + 1 from hi up in the last), which is what K becomes there.  A builder
    with another cut, another order of the trims or an unclamped cell() gives other tables.
  * each epilogue path: K selects it -- pair fetch S[r], S[r + 1] for K <= 2 (degenerate, trim0, last_slot: K = 1;
    k2, full8 wide: K = 2), quad fetch S[r .. r + 3] for two-byte ranks with K <= 4 (k3, wide_k4 forced into two
    bytes), the K-step loop otherwise (k3 narrow: the shortest; wide_k5: the shortest wide; k16, wide_k64: the
    longest).  The pair path at K = 3 or the quad path at K = 5 misses the cluster's last threshold (WRONG_TABLES
    pair_at_k3, quad_at_k5).
  * the padding: last_slot* -- the largest threshold alone in the last used cell, pool values above it: their fetch
    starts at slot size - 1 or size and reads +inf padding (S[254], S[255]; S[1020 .. 1023]); with +inf itself a
    threshold the padding equals a real entry.
  * the degenerate grids: degenerate(_rot) -- one threshold, none, only +-inf, all equal (hi == lo: k = 1), on each
    channel position; specials -- -0.0 / 0.0 (one entry), +-1e-40 around the most common pixel 0.0 (a compare that
    flushes denormals ranks 0.0 beside them: ftz_compare), +-FLT_MAX (k = 3e-36), +-inf, NaN (dropped; a NaN-only
    channel is an empty one); tiny_only -- see Findings.
  * host/device agreement of cell(): boundary0 .. boundary2 -- a pool value v that is itself a threshold, in a grid
    where fl(fl(v k) + b) falls one cell ABOVE fma(v, k, b) (BOUNDARY_HITS, found by find_boundary at design time).

WRONG_TABLES restates mistakes a kernel or a builder could make; every one misranks at least one probe (probes():
every threshold +-1 ulp, the special values, both sides of every cell boundary found by bisection over the float key),
with the counts recorded in test_rank_designs_host.py.

Findings.
  * No design exposed a bug: the library's tables equal the mirror on all of them, and on the MI355X every pixel of
    both design images is ranked as np.searchsorted ranks it, in both widths.
  * The boundary search is cheap when it is directed at the anchors: 3 hits in 3 000 random anchor pairs (half a
    second), although no value of the image is sensitive under a few hundred undirected grids.  Only a device cell
    ABOVE the host's shows: below, the compares walk up through the thresholds of the lower cell and still end at the
    right rank as long as K covers them.  So `unfused` is image-reachable (8 pyramid values in all) and
    the GPU file does test it: a library built with the two-rounding cell() on the device failed boundary0 .. boundary2,
    trim0, trim2 and trim3 on the MI355X and passed everything else -- exactly the designs on which the restated
    mistake misranks a pyramid value (in the trim designs the cluster's end values sit on the edge of an end cell).
  * Host-only -- no value the design images' pyramids hold reveals it: no_nan_code.  grad_hist rectifies a NaN
    gradient to 0 (np.fmax), and the overflowing float32 image yields +inf but no NaN; the 255 / 65535 substitution is
    checked by the NumPy restatement alone.
  * no_lower_clamp is reachable as restated here (a negative product-sum wraps into the table: pixel 0.0 under any grid
    whose lo is positive), but on gfx950 the float -> uint32 conversion saturates at 0, so a device cell() that lost only
    its lower bound would still rank correctly there: the GPU file cannot tell, the host restatement can.
  * ftz_compare shows on exactly one pixel value, 0.0, and only on `specials`.
  * A channel whose finite thresholds span less than about 6e-36 (tiny_only: -1e-40 and 1e-40 alone) has no grid at any
    trim -- k = cells / (hi - lo) overflows float32 -- so the whole model has no rank form and scans the float32
    channels: correct, slower, and pinned here as it is.
  * Which of -0.0 / 0.0 the library keeps in S is left to its sort; the comparison with the mirror takes them as one.
"""
import numpy as np

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = F32(1e-45)                                   # 2^-149
TINY = F32(1e-40)                                         # a denormal
TRIMS = (0.0, 0.01, 0.03, 0.1, 0.25)
# (slots, cells, most thresholds per channel, most thresholds per cell) of the one- and the two-byte form
FORM = {False: (256, 2048, 254, 16), True: (1024, 512, 1020, 64)}
NAN_RANK = {False: 255, True: 65535}

# the design image (tests build it with waldboost_amd.synth.synth_image) and its pyramid
IMAGE_SHAPE, IMAGE_SEED = (96, 160), 21
CHANNEL_OPTS = dict(shrink=2, n_per_oct=1, smooth=1)      # levels 48 x 80, 24 x 40, 12 x 20, 6 x 10
WINDOW = (5, 6, 4)                                        # fits the smallest level


def float_image(img):
    """The design image as float32 with the overflow patches of test_gpu_ranks: infinite channel values."""
    imf = (img.astype(np.float32) * F32(0.25)).astype(np.float32)
    imf[40:44, 60:64] = 3.0e38
    imf[90, 20] = -3.0e38
    return imf


# ------------------------------------------------------------------------------ the lookup grid, restated
def fmaf(a, b, c):
    """fp32 fma(a, b, c), exactly: a * b is exact in fp64; the fp64 sum is rounded TO ODD (its error term from TwoSum
    says on which side the true value lies), and a round-to-odd value of 53 bits rounds to 24 bits as the true value
    does -- so the double rounding gradient_designs.fmaf checks for cannot show, at any operand.  inf and NaN pass
    through the fp64 arithmetic unchanged."""
    a = np.asarray(a, np.float32)
    p = a.astype(np.float64) * np.float64(F32(b))
    c = np.float64(F32(c))
    with np.errstate(invalid="ignore", over="ignore"):
        t = p + c
        bv = t - p
        err = (p - (t - bv)) + (c - bv)
        odd = np.isfinite(t) & (err != 0) & ((t.view(np.int64) & 1) == 0)
        t = np.where(odd, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
        return t.astype(np.float32)


def unfused(a, b, c):
    """fl(fl(a * b) + c): what a contraction switched off, or a mul and an add written apart, would compute."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(a, np.float32) * F32(b) + F32(c)).astype(np.float32)


def cell(v, k, b, cells, fma=fmaf, lower=True, upper=True):
    """The grid cell of v (bin_cell of wb_stage_records.h = wb_bin_cell of wb_common.h: trunc(clamp(fma(v, k, b), 0,
    cells - 1)), NaN in cell 0).  lower / upper = False leave a clamp out: the integer then indexes wherever it points in
    the four channels' base counts (taken modulo their number)."""
    q = fma(v, k, b).astype(np.float64)
    q = np.where(np.isnan(q), 0.0, q)
    if lower:
        q = np.maximum(q, 0.0)
    if upper:
        q = np.minimum(q, float(cells - 1))
    return np.trunc(np.clip(q, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def distinct(s):
    """The sorted distinct non-NaN thresholds of a channel, -0.0 = 0.0 (written as 0.0)."""
    s = np.asarray(s, np.float32).reshape(-1)
    return np.unique(s[~np.isnan(s)] + F32(0.0))


def mirror_tables(S_per_channel, wide):
    """build_rank_tables of wb_stage_records.h in NumPy, step by step: dedupe, refuse more than 254 / 1020 on a
    channel, per channel the first of the five trims whose grid (k, b computed in fp64, cast to fp32) puts at most
    16 / 64 thresholds in a cell, the per-cell counts, base[], K.  None where the library refuses the set; else a dict:
    wide, K, slots, cells, k[4], b[4], S[4][slots], base[4][cells], trim[4], count[4][cells], n[4]."""
    slots, cells, most, kmax = FORM[bool(wide)]
    S = [distinct(s) for s in S_per_channel]
    if any(s.size > most for s in S):
        return None
    t = dict(wide=bool(wide), K=1, slots=slots, cells=cells, k=np.zeros(4, np.float32), b=np.zeros(4, np.float32),
             S=np.full((4, slots), INF, np.float32), base=np.zeros((4, cells), np.uint16 if wide else np.uint8),
             trim=[None] * 4, count=np.zeros((4, cells), np.int64), n=[s.size for s in S])
    for c, s in enumerate(S):
        fin = s[np.isfinite(s)]
        n = fin.size
        for ti, q in enumerate(TRIMS):
            lo, hi = np.float64(np.inf), np.float64(-np.inf)
            if n:
                cut = min(int(q * float(n)), n - 1)
                lo, hi = np.float64(fin[cut]), np.float64(fin[n - 1 - cut])
                if hi < lo:
                    lo, hi = hi, lo
            k = b = np.float64(1.0)
            if hi > lo:
                k = np.float64(cells - 2) / (hi - lo)
            if lo <= hi:
                b = 1.0 - lo * k
            with np.errstate(over="ignore"):
                kf, bf = F32(k), F32(b)
            if not (np.isfinite(kf) and np.isfinite(bf) and kf > 0):
                continue
            count = np.bincount(cell(s, kf, bf, cells), minlength=cells)
            if count.max(initial=0) <= kmax:
                t["k"][c], t["b"][c], t["trim"][c], t["count"][c] = kf, bf, ti, count
                break
        else:
            return None
        t["base"][c] = (np.cumsum(count) - count).astype(t["base"].dtype)
        t["S"][c, :s.size] = s
        t["K"] = max(t["K"], int(count.max(initial=0)))
    return t


def allowed_paths(K, wide):
    """The epilogue paths channels_kernel may take at this K (wb_channels.hip): the pair fetch S[r], S[r + 1] for K <= 2,
    the quad fetch S[r .. r + 3] for 16-bit ranks with K <= 4, the K-step loop always."""
    return (("pair",) if K <= 2 else ()) + (("quad",) if wide and K <= 4 else ()) + ("loop",)


def kernel_path(K, wide):
    """... and the one it does take."""
    return allowed_paths(K, wide)[0]


def _ftz(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) < np.finfo(np.float32).tiny, F32(0.0), x).astype(np.float32)


def rank_by_tables(v, t, path, c=0, K=None, fma=fmaf, lower=True, upper=True, ge=False, ftz=False, nan_code=True, bump=None):
    """Ranks of the float32 values v on channel c as the channel kernel's epilogue computes them from the tables t along
    one of its three paths -- r = base[cell(v)], then "pair": r += (v > S[r]) + (v > S[r + 1]); "quad": the same over
    S[r .. r + 3]; "loop": K times r += v > S[r] -- and 255 / 65535 for NaN.
    The keyword arguments are the mistakes of WRONG_TABLES: K another number of steps, fma another product-sum, a clamp
    left out, >= for >, denormals flushed in the compare, no NaN code, bump = a cell whose base count is one too high."""
    v = np.asarray(v, np.float32).reshape(-1)
    cells, slots = t["cells"], t["slots"]
    base = t["base"].astype(np.int64).reshape(-1)
    if bump is not None:
        base = base.copy()
        base[c * cells + bump] += 1
    at = cell(v, t["k"][c], t["b"][c], cells, fma, lower, upper)
    r = base[(c * cells + at) % base.size]
    S = t["S"].reshape(-1)
    a, s = (_ftz(v), _ftz(S)) if ftz else (v, S)

    def above(r, i):                                       # v > S[r + i] of this channel's table (reads stay in the lut)
        x = s[np.minimum(c * slots + r + i, s.size - 1)]
        with np.errstate(invalid="ignore"):
            return (a >= x if ge else a > x).astype(np.int64)
    if path == "loop":
        for _ in range(t["K"] if K is None else K):
            r = r + above(r, 0)
    else:
        r = r + sum(above(r, i) for i in range({"pair": 2, "quad": 4}[path]))
    if nan_code:
        r = np.where(np.isnan(v), NAN_RANK[t["wide"]], r)
    return r


def true_ranks(v, t, c=0):
    """np.searchsorted(S, v, "left"): the number of the channel's thresholds below v; the NaN code for NaN."""
    v = np.asarray(v, np.float32).reshape(-1)
    r = np.searchsorted(t["S"][c, :t["n"][c]], v, side="left").astype(np.int64)
    return np.where(np.isnan(v), NAN_RANK[t["wide"]], r)


def _median_cell(t, c):
    """The cell holding the channel's median threshold (0 on an empty channel)."""
    n = t["n"][c]
    return int(cell(t["S"][c, n // 2:n // 2 + 1], t["k"][c], t["b"][c], t["cells"])[0]) if n else 0


# name -> ranks(v, tables, c): mistakes a kernel or a builder could make, each on the path the kernel takes at the tables' K
WRONG_TABLES = {
    "k_short": lambda v, t, c: rank_by_tables(v, t, "loop", c, K=t["K"] - 1),
    "pair_at_k3": lambda v, t, c: rank_by_tables(v, t, "pair" if t["K"] == 3 else kernel_path(t["K"], t["wide"]), c),
    "quad_at_k5": lambda v, t, c: rank_by_tables(v, t, "quad" if t["K"] == 5 else kernel_path(t["K"], t["wide"]), c),
    "base_off_by_one": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, bump=_median_cell(t, c)),
    "no_lower_clamp": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, lower=False),
    "no_upper_clamp": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, upper=False),
    "unfused": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, fma=unfused),
    "ge_compare": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, ge=True),
    "ftz_compare": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, ftz=True),
    "no_nan_code": lambda v, t, c: rank_by_tables(v, t, kernel_path(t["K"], t["wide"]), c, nan_code=False),
}


# ------------------------------------------------------------------------------ probes
def key_of(f):
    """The order-preserving uint32 key of float32 values (as int64)."""
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def float_of(key):
    key = np.asarray(key, np.int64)
    u = np.where(key & 0x80000000, key & 0x7FFFFFFF, 0xFFFFFFFF - key)
    return u.astype(np.uint32).view(np.float32)


def neighbours(v):
    v = np.asarray(v, np.float32).reshape(-1)
    with np.errstate(over="ignore"):
        return np.concatenate([np.nextafter(v, -INF), v, np.nextafter(v, INF)]).astype(np.float32)


def cell_firsts(t, c):
    """For every cell j >= 1 of channel c the first float (from -inf up) whose cell is >= j, by bisection over the key:
    cell() is non-decreasing."""
    j = np.arange(1, t["cells"], dtype=np.int64)
    lo = np.full(j.size, int(key_of(-INF)), np.int64)      # cell(lo) < j: cell(-inf) = 0
    hi = np.full(j.size, int(key_of(INF)), np.int64)       # cell(hi) >= j: cell(+inf) = cells - 1
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        up = cell(float_of(mid), t["k"][c], t["b"][c], t["cells"]) >= j
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return float_of(np.unique(hi))


def probes(t):
    """Per channel, sorted float32 values (NaN last): every threshold and its two float neighbours; +-0.0, +-denormal-min,
    +-1e-40, +-FLT_MAX, +-inf and NaN; for every cell boundary the first float of the cell and its predecessor."""
    special = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, TINY, -TINY, FLT_MAX, -FLT_MAX, INF, -INF, NAN], np.float32)
    out = []
    for c in range(4):
        first = cell_firsts(t, c)
        v = np.concatenate([neighbours(t["S"][c, :t["n"][c]]), special, first, np.nextafter(first, -INF)])
        out.append(float_of(np.unique(key_of(v[~np.isnan(v)]))).tolist() + [NAN])
        out[-1] = np.array(out[-1], np.float32)
    return out


# ------------------------------------------------------------------------------ the pool: what a pixel can be
def value_pool(levels):
    """Per channel the sorted distinct values of a pyramid's levels ([u, v, 4] float32 arrays)."""
    return [np.unique(np.concatenate([np.asarray(l, np.float32)[..., c].reshape(-1) for l in levels])) for c in range(4)]


def candidates(pool_c):
    """The positive finite values of a channel's pool with their +-1-ulp neighbours: what an interior threshold may be."""
    p = pool_c[np.isfinite(pool_c) & (pool_c > 0)]
    return np.unique(neighbours(p))


def spread(pool_c, n, upto=1.0):
    """n distinct candidates, evenly by index over the lower `upto` of them."""
    cand = candidates(pool_c)
    cand = cand[:max(int(cand.size * upto), 1)]
    assert cand.size >= n, "the design image's pool is too small for this design"
    return cand[np.unique(np.round(np.linspace(0, cand.size - 1, n)).astype(np.int64))]


def thinned(pool_c, m):
    """m pool values (no neighbours) at least (max - min) / (1.6 m) apart, from the smallest up."""
    p = pool_c[np.isfinite(pool_c) & (pool_c > 0)]
    gap, out = (p[-1] - p[0]) / (1.6 * m), [p[0]]
    for x in p[1:]:
        if x - out[-1] >= gap and len(out) < m:
            out.append(x)
    assert len(out) == m, "the design image's pool is too small for this design"
    return np.array(out, np.float32)


ANCHOR = 131072.0      # anchors at +-ANCHOR j: symmetric grids whose cell above 0 is at least 128 wide -- every positive pool value


def anchors_for(m):
    """Enough anchors per side that no trim level cuts all of them off: int(0.25 (m + 2 a)) < a."""
    a = 1
    while int(0.25 * (m + 2 * a)) >= a:
        a += 1
    return a


def cluster(pool_c, m):
    """m neighbouring candidates around the pool's median, between anchors +-ANCHOR j: under every trim the grid is
    symmetric about 0 and spanned by anchors, the cell [0, >= 128) holds the whole cluster, every anchor a cell of its
    own (or an end cell, at most 16 of them) -- exactly m thresholds in one cell, whatever the trim."""
    cand = candidates(pool_c)
    assert cand.size >= m + 2 and cand[-1] < 128.0
    i = (cand.size - m) // 2
    a = np.arange(1, anchors_for(m) + 1, dtype=np.float32) * F32(ANCHOR)
    return np.concatenate([-a, cand[i:i + m], a]).astype(np.float32)


def few(pool, c):
    """Three far-apart pool values: a quiet channel (one threshold per cell)."""
    return spread(pool[c], 3)


def outliers(pool_c, m, o):
    """m thinned pool values between o outliers +-1e30 (j + 1) per side: a grid that spans an outlier holds the whole
    cluster in one cell, so the first trim that places the set is the first whose cut reaches o."""
    out = F32(1e30) * np.arange(1, o + 1, dtype=np.float32)
    return np.concatenate([-out, thinned(pool_c, m), out]).astype(np.float32)


def last_slot(pool_c, n, extra=()):
    """n - 1 candidates from the lower 60 % and, far above them, the pool's third largest value: the largest threshold is
    alone in the last used cell, values above it exist, and their fetch S[r], S[r + 1] (..., S[r + 3]) reads the padding."""
    p = pool_c[np.isfinite(pool_c)]
    return np.concatenate([spread(pool_c, n - 1 - len(extra), 0.6), [p[-3]], np.array(extra, np.float32)]).astype(np.float32)


# the boundary search's hits (find_boundary below, run at design time): (channel, v, lo anchor, hi anchor) as float32 bit
# patterns -- v is a value of the design image's pyramid on that channel, and in the grid the anchors span, fused and
# unfused cell(v) differ
BOUNDARY_HITS = ((2, 1106018304, 3263480020, 1132150593), (3, 1107132271, 3229813781, 1137647706),
                 (1, 1109230095, 3240020201, 1142438464))


def find_boundary(pool, budget=20000, seed=5, want=4):
    """Design-time search (not run by the tests): random anchors lo < 0 < hi over many binades; a hit is a pool value v
    whose unfused cell in the narrow grid over [lo, hi] lies ABOVE its fused one (below is harmless: the compares walk
    up through v's own cell) with {lo, v, hi} as the channel's thresholds."""
    rng = np.random.default_rng(seed)
    hits = []
    for _ in range(budget):
        c = int(rng.integers(0, 4))
        lo = F32(-np.exp(rng.uniform(np.log(1.0), np.log(1e6))))
        hi = F32(np.exp(rng.uniform(np.log(200.0), np.log(1e6))))
        v = pool[c][np.isfinite(pool[c]) & (pool[c] > 0)]
        k64 = 2046.0 / (np.float64(hi) - np.float64(lo))
        k, b = F32(k64), F32(1.0 - np.float64(lo) * k64)
        d = cell(v, k, b, 2048, unfused) - cell(v, k, b, 2048)
        for x in v[d > 0][:1]:
            hits.append((c, int(x.view(np.uint32)), int(lo.view(np.uint32)), int(hi.view(np.uint32))))
        if len(hits) >= want:
            break
    return tuple(hits)


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def boundary(pool, hit=0):
    c, v, lo, hi = BOUNDARY_HITS[hit]
    S = [few(pool, ch) for ch in range(4)]
    S[c] = np.array([_bits(lo), _bits(v), _bits(hi)], np.float32)
    return S


def with_channel(pool, c, s):
    S = [few(pool, ch) for ch in range(4)]
    S[c] = np.asarray(s, np.float32)
    return S


def degenerate(pool, rot=0):
    v = [candidates(p)[candidates(p).size // 2] for p in pool]
    S = [[v[0]], [], [-INF, INF], [v[3], v[3], v[3]]]
    S = S[rot:] + S[:rot]
    return [np.array(s, np.float32) for s in S]


def specials(pool):
    return [np.concatenate([[-0.0, 0.0, TINY, -TINY, FLT_MAX, -FLT_MAX, INF, -INF, NAN], spread(pool[0], 5)]).astype(np.float32),
            np.concatenate([[-TINY, TINY, -10.0], spread(pool[1], 4)]).astype(np.float32),
            np.array([NAN, NAN], np.float32),
            np.concatenate([[0.0, DENORM_MIN, -DENORM_MIN], spread(pool[3], 6)]).astype(np.float32)]


def cascade_arrays(S, seed=0):
    """A cascade of complete depth-2 trees whose internal nodes carry exactly the thresholds S[c] on channel c (each
    entry once, NaN and duplicates included; the last repeated to fill the last tree), in the flat arrays wb_model_create
    takes: window, node_off, feature [n][3], threshold, left, right, prediction, theta."""
    rng = np.random.default_rng(seed)
    nodes = [(c, x) for c in range(4) for x in np.asarray(S[c], np.float32).reshape(-1)]
    nodes = [nodes[i] for i in rng.permutation(len(nodes))]
    nodes += [nodes[-1]] * (-len(nodes) % 3)
    T = len(nodes) // 3
    feature, threshold = np.zeros((T, 7, 3), np.uint8), np.zeros((T, 7), np.float32)
    feature[:, :3, 0] = rng.integers(0, WINDOW[0], (T, 3))
    feature[:, :3, 1] = rng.integers(0, WINDOW[1], (T, 3))
    feature[:, :3, 2] = np.array([c for c, _ in nodes], np.uint8).reshape(T, 3)
    threshold[:, :3] = np.array([x for _, x in nodes], np.float32).reshape(T, 3)
    prediction = np.zeros((T, 7), np.float32)
    prediction[:, 3:] = rng.uniform(-1, 1, (T, 4))
    theta = (-0.5 * np.sqrt(np.arange(1, T + 1))).astype(np.float32)
    theta[3::4] = -INF
    return dict(window=np.array(WINDOW, np.int32), node_off=(7 * np.arange(T + 1)).astype(np.int32), feature=feature.reshape(-1, 3),
                threshold=threshold.reshape(-1), left=np.tile(np.array([1, 3, 5, -1, -1, -1, -1], np.int8), T),
                right=np.tile(np.array([2, 4, 6, -1, -1, -1, -1], np.int8), T), prediction=prediction.reshape(-1), theta=theta)


def read_rank_dump(path):
    """The forms of a WB_DUMP_RANKS file: int32 {wide, K, slots, cells}, float32 k[4], b[4], then the lut -- float32
    S[4][slots], base[4][cells] (uint8; wide: uint16) -- per rank form built.  {wide: dict like mirror_tables'}."""
    raw, at, out = np.fromfile(path, np.uint8), 0, {}
    while at < raw.size:
        wide, K, slots, cells = (int(x) for x in raw[at:at + 16].view(np.int32))
        assert (slots, cells) == FORM[bool(wide)][:2]
        kb = raw[at + 16:at + 48].view(np.float32)
        at += 48
        S = raw[at:at + 16 * slots].view(np.float32).reshape(4, slots)
        at += 16 * slots
        nb = 4 * cells * (2 if wide else 1)
        base = raw[at:at + nb].view(np.uint16 if wide else np.uint8).reshape(4, cells)
        at += nb
        assert bool(wide) not in out
        out[bool(wide)] = dict(wide=bool(wide), K=K, slots=slots, cells=cells, k=kb[:4].copy(), b=kb[4:].copy(), S=S.copy(), base=base.copy())
    assert at == raw.size
    return out


def E(rank8, rank16, K8=None, K16=None, trim8=None, trim16=None):
    return dict(rank8=rank8, rank16=rank16, K8=K8, K16=K16, trim8=trim8, trim16=trim16)


# name -> (function of the pool, what the set is expected to be: the forms present, K of each width, the trim index per channel)
DESIGNS = {
    "degenerate": (degenerate, E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "degenerate_rot": (lambda p: degenerate(p, 2), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "full8": (lambda p: with_channel(p, 0, spread(p[0], 254)), E(True, True, 1, 2, (0, 0, 0, 0), (0, 0, 0, 0))),
    "over8": (lambda p: with_channel(p, 0, spread(p[0], 255)), E(False, True, None, 2, None, (0, 0, 0, 0))),
    "full16": (lambda p: with_channel(p, 1, spread(p[1], 1020)), E(False, True, None, 5, None, (0, 0, 0, 0))),
    "over16": (lambda p: with_channel(p, 1, spread(p[1], 1021)), E(False, False)),
    "k2": (lambda p: with_channel(p, 0, cluster(p[0], 2)), E(True, True, 2, 2, (0, 0, 0, 0), (0, 0, 0, 0))),
    "k3": (lambda p: with_channel(p, 1, cluster(p[1], 3)), E(True, True, 3, 3, (0, 0, 0, 0), (0, 0, 0, 0))),
    "k16": (lambda p: with_channel(p, 2, cluster(p[2], 16)), E(True, True, 16, 16, (0, 0, 0, 0), (0, 0, 0, 0))),
    "k17": (lambda p: with_channel(p, 3, cluster(p[3], 17)), E(False, True, None, 17, None, (0, 0, 0, 0))),
    "wide_k4": (lambda p: with_channel(p, 3, cluster(p[3], 4)), E(True, True, 4, 4, (0, 0, 0, 0), (0, 0, 0, 0))),
    "wide_k5": (lambda p: with_channel(p, 2, cluster(p[2], 5)), E(True, True, 5, 5, (0, 0, 0, 0), (0, 0, 0, 0))),
    "wide_k64": (lambda p: with_channel(p, 1, cluster(p[1], 64)), E(False, True, None, 64, None, (0, 0, 0, 0))),
    "wide_k65": (lambda p: with_channel(p, 0, cluster(p[0], 65)), E(False, False)),
    "trim0": (lambda p: with_channel(p, 0, outliers(p[0], 100, 0)), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "trim1": (lambda p: with_channel(p, 1, outliers(p[1], 100, 1)), E(True, True, 2, 2, (0, 1, 0, 0), (0, 1, 0, 0))),
    "trim2": (lambda p: with_channel(p, 2, outliers(p[2], 100, 3)), E(True, True, 4, 4, (0, 0, 2, 0), (0, 0, 2, 0))),
    "trim3": (lambda p: with_channel(p, 3, outliers(p[3], 100, 10)), E(True, True, 13, 13, (0, 0, 0, 3), (0, 0, 0, 3))),
    "trim4": (lambda p: with_channel(p, 0, outliers(p[0], 38, 12)), E(True, True, 16, 38, (4, 0, 0, 0), (0, 0, 0, 0))),
    "wide_trim4": (lambda p: with_channel(p, 1, outliers(p[1], 140, 30)), E(False, True, None, 51, None, (0, 4, 0, 0))),
    "last_slot": (lambda p: with_channel(p, 1, last_slot(p[1], 9)), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "last_slot_inf": (lambda p: with_channel(p, 2, last_slot(p[2], 9, [INF])), E(True, True, 2, 2, (0, 0, 0, 0), (0, 0, 0, 0))),
    "last_slot_full8": (lambda p: with_channel(p, 3, last_slot(p[3], 254)), E(True, True, 1, 2, (0, 0, 0, 0), (0, 0, 0, 0))),
    "last_slot_full8_inf": (lambda p: with_channel(p, 3, last_slot(p[3], 254, [INF])), E(True, True, 1, 2, (0, 0, 0, 0), (0, 0, 0, 0))),
    "last_slot_full16": (lambda p: with_channel(p, 0, last_slot(p[0], 1020)), E(False, True, None, 9, None, (0, 0, 0, 0))),
    "last_slot_full16_inf": (lambda p: with_channel(p, 0, last_slot(p[0], 1020, [INF])), E(False, True, None, 8, None, (0, 0, 0, 0))),
    "specials": (specials, E(True, True, 8, 8, (0, 0, 0, 0), (0, 0, 0, 0))),
    "tiny_only": (lambda p: with_channel(p, 0, [-TINY, TINY]), E(False, False)),
    "boundary0": (lambda p: boundary(p, 0), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "boundary1": (lambda p: boundary(p, 1), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
    "boundary2": (lambda p: boundary(p, 2), E(True, True, 1, 1, (0, 0, 0, 0), (0, 0, 0, 0))),
}
# the wrong tables that misrank a value the design images' pyramids hold (test_rank_designs_host.REACHABLE)
GPU_RELEVANT = ("k_short", "pair_at_k3", "quad_at_k5", "base_off_by_one", "no_lower_clamp", "no_upper_clamp", "unfused", "ge_compare", "ftz_compare")
