"""Host proofs for tests/mip_designs.py (CPU; no GPU, no torch): every design's claims from exact rational arithmetic and
an independent window-by-window / bag-by-bag evaluation, the statement (tests/mip_reference.py) against that evaluation,
and that every emulated wrong kernel differs from the statement on some design."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import mip_designs as md
import mip_reference as ref

WIN = md.window_designs()
PRUNE = md.prune_designs()
m = n = md.M


# ----------------------------------------------------------------------------------------------- windows, exactly
def exact_iou(a, b):
    """IoU of two boxes of exact rationals."""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    inter = iw * ih
    uni = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / uni if uni > 0 else Fr(0)


def exact_windows(d, flaw=None):
    """{(image, level, r, c): (owner, exact best IoU)} of the acceptable windows, window by window on rationals.  A window
    whose best IoU is within 1e-9 of min_iou without being settled exactly would make the float64 decision uncertain: the
    design has none (asserted).  flaw: an emulated wrong kernel."""
    out = {}
    thr = Fr(d.min_iou)
    for b, g in enumerate(d.gts):
        if g is None:
            continue
        boxes = [[Fr(float(x)) for x in row] for row in g]
        for l, (u, v) in enumerate(d.levels):
            nr, nc = (u - m, v - n) if flaw != "grid+1" else (u - m + 1, v - n + 1)
            s = Fr(float(d.inv_scale[l]))
            for r in range(max(nr, 0)):
                for c in range(max(nc, 0)):
                    # float32(c) * float32(s) rounded to float32: exact for the dyadic scales; for the other the design's
                    # boxes are the rounded products themselves
                    w = [Fr(float(np.float32(x) * d.inv_scale[l])) for x in (c, r, c + n, r + m)]
                    if s in (1, 2):
                        assert w == [x * s for x in (c, r, c + n, r + m)]
                    ious = [exact_iou(w, k) for k in boxes]
                    best = max(ious)
                    owner = ious.index(best) if flaw != "last-argmax" else len(ious) - 1 - ious[::-1].index(best)
                    if s in (1, 2):
                        # integers throughout and one division: the float64 IoU is the exact one, correctly rounded
                        best_f = Fr(float(best))
                    else:
                        # several roundings: the decision is settled only at a distance from min_iou
                        assert abs(best - thr) > Fr(1, 10 ** 9), (d.name, l, r, c, float(best))
                        best_f = best
                    ok = best_f >= thr if flaw == ">=" else best_f > thr
                    if ok and not d.ignores[b][owner]:
                        out[(b, l, r, c)] = (owner, best)
    return out


def as_dict(rows):
    return {(int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])): int(w["owner"]) for w in rows}


@pytest.mark.parametrize("name", list(WIN))
def test_window_designs_are_what_they_claim(name):
    d = WIN[name]
    assert [ref.window_grid(u, v, m, n) for u, v in d.levels] == [(28, 44), (8, 16), (1, 18), (0, 28), (0, 18)]
    assert float(d.inv_scale[2]) * 3 != 10 and d.gts[1] is None                  # a non-dyadic scale; an image without ground truth
    exact = exact_windows(d)
    got = ref.windows(d.levels, d.inv_scale, m, n, d.gts, d.ignores, d.min_iou)
    rows = got["rows"]
    assert as_dict(rows) == {k: v[0] for k, v in exact.items()}                  # the statement is the exact evaluation
    order = np.lexsort((rows["c"], rows["r"], rows["level"], rows["image"]))
    assert np.array_equal(order, np.arange(rows.size)) and (rows["label"] == 1).all() and (rows["score"] == 0).all()
    for w in rows:                                                               # best: the correctly rounded exact value
        e = exact[(int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"]))][1]
        assert abs(Fr(float(w["best"])) - e) <= Fr(1, 2 ** 50)
    assert [tuple(x) for x in got["reachable"]] == d.reachable and [tuple(x) for x in got["unreachable"]] == d.unreachable
    for k, owner in d.hits.items():
        assert exact.get(k, (None,))[0] == owner, k
    for k in d.absent:
        assert k not in exact, k
    # the windows at 1/2 exactly, with an owner that counts: all of them and no other
    half = {k: v[0] for k, v in exact_windows(md.WindowDesign(name, md.HALF_DOWN, None, None, None, None, None)).items() if v[1] == Fr(1, 2)}
    assert half == d.exact_half
    assert 20 <= len(exact) <= 5000 and {k[1] for k in exact} == {0, 1, 2}
    # hits on the last row and the last column of two grids; twins: the first owns
    assert (0, 0, 27, 43) in exact and (0, 1, 7, 15) in exact and 2 not in {v[0] for v in exact.values()}


def test_half_is_excluded_and_one_rounding_below_it_included():
    at, down = exact_windows(WIN["half"]), exact_windows(WIN["half-down"])
    assert md.HALF_DOWN < 0.5 and np.nextafter(md.HALF_DOWN, 1.0) == 0.5
    assert set(down) - set(at) == set(md.EXACT_HALF) and set(at) <= set(down)
    # a box of twice a window's area: IoU 1/2 for the windows inside it
    assert exact_iou([Fr(4), Fr(3), Fr(16), Fr(15)], [Fr(4), Fr(3), Fr(28), Fr(15)]) == Fr(1, 2)


@pytest.mark.parametrize("flaw,name", [("last-argmax", "half"), (">=", "half"), ("grid+1", "half"), ("grid+1", "default")])
def test_wrong_window_kernels_differ(flaw, name):
    d = WIN[name]
    want = as_dict(ref.windows(d.levels, d.inv_scale, m, n, d.gts, d.ignores, d.min_iou)["rows"])
    wrong = {k: v[0] for k, v in exact_windows(d, flaw).items()}
    assert wrong != want


# ----------------------------------------------------------------------------------------------- prune, bag by bag
def order_key(x):
    """A float32 as (exact value, 0 for -0.0 / 1 otherwise at zero): the order of wb_f32_key."""
    x = np.float32(x)
    return (Fr(float(x)), 0 if (x == 0 and np.signbit(x)) else 1)


def slow_prune(d, floor, flaw=None):
    """The rule, window by window and bag by bag on exact values.  flaw: an emulated wrong kernel."""
    tr, bag, N, T = d.trace, d.bag, d.N, d.T
    windows = range(N - 1) if flaw == "last-window" else range(N)
    bags = range(d.n_bags - 1) if flaw == "last-bag" else range(d.n_bags)
    G = {}
    for i in range(N):
        k = order_key(tr[i, -1])
        G[int(bag[i])] = max(G[int(bag[i])], k) if int(bag[i]) in G else k
    fl = Fr(float(np.float32(floor)))
    if flaw == "floor-on-bags":
        live = {i for i in windows if G[int(bag[i])][0] >= fl}
    else:
        live = {i for i in windows if Fr(float(tr[i, -1])) >= fl}
    initial = set(live)
    removed = {i: (T if i in live else -1) for i in range(N)}
    theta, owners = [], []
    carried = {}
    for t in range(T):
        best = {} if flaw != "no-reset" else carried
        pool = live if flaw != "non-retained" else {i for i in windows if G[int(bag[i])][0] >= fl}
        for i in pool:
            b = int(bag[i])
            if b in bags:
                k = order_key(tr[i, t]) if flaw != "raw-bits" else (int(np.float32(tr[i, t]).view(np.uint32)), 0)
                if b not in best or k > best[b]:
                    best[b] = k
        carried = best
        if flaw == "backward":
            best = {i: order_key(tr[i, t]) for i in live}
        if not best:
            theta.append(np.float32(np.inf))
            owners.append(-1)
            continue
        low = min(best.values())
        if flaw == "raw-bits":
            th = np.uint32(low[0]).view(np.float32)
        else:
            th = np.float32(float(low[0])) if low[0] != 0 or low[1] == 1 else np.float32(-0.0)
        theta.append(th)
        holders = [i for i in live if (order_key(tr[i, t]) if flaw != "raw-bits" else (int(np.float32(tr[i, t]).view(np.uint32)), 0)) == low]
        owners.append(holders[0] if len(holders) == 1 else -1)
        if flaw == "no-removal":
            continue
        for i in list(live):
            stays = Fr(float(tr[i, t])) > Fr(float(th)) if flaw == ">" else Fr(float(tr[i, t])) >= Fr(float(th))
            if not stays:
                live.discard(i)
                removed[i] = t
    return dict(theta=np.array(theta, np.float32), removed_at=np.array([removed[i] for i in range(N)], np.int32), owners=owners,
                initial=initial, retained_bags=len({int(bag[i]) for i in initial}), surviving=len(live))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(PRUNE))
def test_prune_designs_are_what_they_claim(name):
    d = PRUNE[name]
    assert np.array_equal(d.trace.astype(np.float64), d.trace64)                 # the planned scores are float32 values
    assert d.bag.min() >= 0 and d.bag.max() < d.n_bags
    for recall in d.recalls:
        floor, keep = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, recall)
        present = np.unique(d.bag).size
        G = sorted((max(order_key(x) for x in d.trace[d.bag == b, -1]) for b in np.unique(d.bag)), reverse=True)
        assert keep == ref.keep_count(recall, present) and order_key(floor) == G[keep - 1]
        want = slow_prune(d, floor)
        got = ref.prune(d.trace, d.bag, d.n_bags, floor)
        assert np.array_equal(bits(got["theta"]), bits(want["theta"])), (name, recall)      # the sign of a zero included
        assert np.array_equal(got["removed_at"], want["removed_at"])
        assert (got["retained_bags"], got["surviving"]) == (want["retained_bags"], want["surviving"])
        assert got["retained_bags"] >= keep
        if recall in d.theta:
            assert np.array_equal(bits(got["theta"]), bits(d.theta[recall])), (name, got["theta"])
        if recall in d.owners:
            claimed = np.asarray(d.owners[recall])
            assert all(o == -1 or want["owners"][t] == o for t, o in enumerate(claimed)), (name, want["owners"], claimed)
        for i, at in d.removed.get(recall, {}).items():
            assert got["removed_at"][i] == at, (name, i, got["removed_at"][i], at)
        # the consequences: every retained bag keeps a window through all stages, with a final score at or above the floor;
        # no theta is below backward pruning's on the windows retained at the start
        alive = got["removed_at"] == d.T
        assert set(np.unique(d.bag[alive])) == set(np.unique(d.bag[got["initial"]])) and (d.trace[alive, -1] >= floor).all()
        assert (got["theta"] >= ref.backward(d.trace, got["initial"])).all()
        # a margin lowers every theta by its float32 value and changes nothing else
        lowered = ref.prune(d.trace, d.bag, d.n_bags, floor, margin=0.375)
        assert np.array_equal(lowered["theta"], got["theta"] - np.float32(0.375)) and np.array_equal(lowered["removed_at"], got["removed_at"])


def test_the_sizes_and_places_asked_for_occur():
    ds = list(PRUNE.values())
    assert {d.N for d in ds} >= {1, 63, 64, 65, 257, 1025} and {d.T for d in ds} >= {1, 2, 24}
    sizes = set()
    for d in ds:
        sizes |= set(np.bincount(d.bag, minlength=d.n_bags).tolist())
    assert {0, 1, 129} <= sizes                                                  # an empty bag id, bags of 1 and of 129 windows
    d = PRUNE["owners-blocks-1025x24"]
    edges = set(np.flatnonzero(np.diff(d.bag)) + 1)
    assert {64, 256, 1024} <= edges                                              # bag edges on wave and workgroup boundaries
    owners = set(int(o) for o in d.owners[1.0])
    assert {0, 64, 1024, 256} <= owners or len(owners) >= 5                      # owners by workgroup, wave and lane
    assert 1024 in owners                                                        # the last window, alone in the last bag
    i = PRUNE["owners-interleaved-1025x2"]
    assert np.bincount(i.bag)[0] == 129 and (np.diff(i.bag[:8]) == 1).all()
    # negative scores, +-0, a leader that falls, a tie, a window at theta and one a float32 below (features design)
    f = PRUNE["features-257x6"]
    th = f.theta[0.6]
    assert np.signbit(th[4]) and th[4] == 0 and f.trace[256, 4] == 0 and not np.signbit(f.trace[256, 4])
    assert f.trace[64, 0] == th[0] and f.removed[0.6][64] == 1                   # a holder of stage 0's maximum falls at stage 1
    assert f.trace[68, 2] == f.trace[256, 2] == th[2]                            # two bags tie at the minimum
    assert f.trace[71, 3] == th[3] and f.trace[74, 3] == np.nextafter(th[3], np.float32(-np.inf))
    assert np.abs(f.trace[:64, :5]).min() == 2.0 ** 127 and (f.trace[:64, 5] < 20).all()
    assert (PRUNE["owners-blocks-257x24"].theta[1.0] < 0).any()


def test_theta_is_strictly_above_backward_pruning_somewhere():
    for d in PRUNE.values():
        if d.N > 64 and d.T >= 2 and "single" not in d.name:        # (bags of several windows; one stage alone is the floor)
            recall = d.recalls[0]
            floor, _ = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, recall)
            got = ref.prune(d.trace, d.bag, d.n_bags, floor)
            assert (got["theta"] > ref.backward(d.trace, got["initial"])).any(), d.name


FLAWS = {"no-removal": "features-257x6", "backward": "owners-blocks-257x24", "non-retained": "features-257x6", ">": "features-257x6",
         "floor-on-bags": "features-257x6", "raw-bits": "owners-blocks-257x24", "no-reset": "owners-blocks-257x24",
         "last-window": "owners-blocks-1025x24", "last-bag": "owners-blocks-1025x24"}


@pytest.mark.parametrize("flaw", list(FLAWS))
def test_wrong_prune_kernels_differ(flaw):
    d = PRUNE[FLAWS[flaw]]
    recall = d.recalls[0]
    floor, _ = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, recall)
    want = ref.prune(d.trace, d.bag, d.n_bags, floor)
    wrong = slow_prune(d, floor, flaw)
    assert not (np.array_equal(bits(wrong["theta"]), bits(want["theta"])) and np.array_equal(wrong["removed_at"], want["removed_at"])), flaw
    assert not np.array_equal(bits(wrong["theta"]), bits(want["theta"])) or flaw in (">", "last-window")


def test_a_zero_sign_flaw_shows_on_the_features_design():
    """Unsigned compare of raw float bits puts -0.0 above +0.0 (and every negative above every positive)."""
    d = PRUNE["features-257x6"]
    floor, _ = ref.bag_floor(d.trace[:, -1], d.bag, d.n_bags, 0.6)
    assert not np.array_equal(bits(slow_prune(d, floor, "raw-bits")["theta"]), bits(ref.prune(d.trace, d.bag, d.n_bags, floor)["theta"]))
