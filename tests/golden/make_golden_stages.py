#!/usr/bin/env python3
"""Golden fixture of the canonical stage records (wb_common.h): designed cascades, each the smallest that takes one
branch of wb_model_create's canonicalisation, handed to wb_model_create through ctypes with WB_DUMP_STAGES set.
Writes tests/golden/stage_records.npz: per model its arrays, the dump's header and the dumped tables.

The fixture was recorded at the commit BEFORE the model handle was reorganised (one record per tile form), so that the
test that reads it (tests/test_host.py) holds the reorganised code to the bytes the old code wrote.  That commit wrote the
dump behind its device uploads (a GPU was needed), with the header {records, stage_dwords, depth, rank_ok} and always
three tables (float32, uint8, rank8: the last one empty records when rank_ok is 0); it never dumped the rank16 table, which
the test rebuilds from the model arrays instead.  From the reorganised commit on header[3] is a mask of the forms present
and the tables of those forms follow in order; read_dump() takes either.  Which forms a model has is taken from
wb_model_info where the call succeeds (a GPU), else from the dump's mask.
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

F32, U8, RANK8, RANK16 = range(4)                 # the tile forms, in the order of the dump (bit f of the mask: form f)
FORMS = ("f32", "u8", "rank8", "rank16")
NAN, INF = float("nan"), float("inf")

# what each designed model must turn out to be: (mask of forms, depth of the records); None: the node-walk model, no dump
EXPECT = {"shapes": (15, 3), "thresholds": (15, 2), "cluster": (11, 3), "long": (11, 3), "c3": (3, 2), "c10": (3, 2),
          "lds": (3, 2), "generic": None}


# ------------------------------------------------------------------------------ trees
# a tree is a leaf (its prediction, a float) or a split ((row, col, channel), threshold, left subtree, right subtree)
def flatten(tree):
    """The reference's five flat arrays (training.py:24-31) of a nested tree, parents before children."""
    feat, thr, left, right, pred = [], [], [], [], []

    def visit(t):
        i = len(feat)
        feat.append((0, 0, 0)), thr.append(0.0), left.append(-1), right.append(-1), pred.append(0.0)
        if isinstance(t, tuple):
            feat[i], thr[i] = t[0], t[1]
            left[i] = visit(t[2])
            right[i] = visit(t[3])
        else:
            pred[i] = float(t)
        return i

    visit(tree)
    return (np.array(feat, np.uint8), np.array(thr, np.float32), np.array(left, np.int8), np.array(right, np.int8),
            np.array(pred, np.float32))


def full_tree(rng, window, depth, splits):
    """A complete tree of `depth` whose splits take their (channel, threshold) from the iterator `splits`."""
    if depth == 0:
        return float(np.float32(rng.uniform(-1, 1)))
    ch, th = next(splits)
    f = (int(rng.integers(window[0])), int(rng.integers(window[1])), ch)
    return (f, th, full_tree(rng, window, depth - 1, splits), full_tree(rng, window, depth - 1, splits))


def cascade(window, trees, thetas):
    flat = [flatten(t) for t in trees]
    out = dict(window=np.array(window, np.int32), node_off=np.cumsum([0] + [f[0].shape[0] for f in flat]).astype(np.int32),
               theta=np.array(thetas, np.float32))
    for k, name in enumerate(("feature", "threshold", "left", "right", "prediction")):
        out[name] = np.ascontiguousarray(np.concatenate([f[k] for f in flat]))
    return out


def full_cascade(seed, window, depth, splits):
    """Complete trees of `depth` over the (channel, threshold) list, shuffled; every third theta is -inf."""
    rng = np.random.default_rng(seed)
    splits = [splits[i] for i in rng.permutation(len(splits))]
    per = (1 << depth) - 1
    assert len(splits) % per == 0
    it = iter(splits)
    trees = [full_tree(rng, window, depth, it) for _ in range(len(splits) // per)]
    thetas = [-INF if s % 3 == 2 else -0.25 * (s + 1) for s in range(len(trees))]
    return cascade(window, trees, thetas)


def spread(seed, n, lo, hi, channels):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(channels)), float(np.float32(rng.uniform(lo, hi)))) for _ in range(n)]


def designs():
    W = (5, 6, 4)
    d = {}
    # tree shapes: a single leaf; depth 1; depth 2 with one child a leaf (a dummy split in the records); depth 3, unbalanced
    d["shapes"] = cascade(W, [
        0.25,
        ((1, 2, 0), 3.5, -0.5, 0.5),
        ((0, 0, 1), 7.0, 0.75, ((4, 5, 3), 20.0, -0.25, 0.125)),
        ((2, 3, 2), 12.0, ((1, 1, 1), 5.0, ((3, 4, 0), 2.0, -1.0, 1.0), 0.5), -0.75),
        ((4, 0, 3), 9.0, -0.125, ((0, 5, 2), 30.0, ((2, 2, 2), 12.0, 0.375, -0.375), 0.625)),
    ], [-INF, -1.0, -INF, -2.0, -2.5])
    # thresholds: NaN, negative, both zeros, the uint8 form's edges (254.5, 255, 300), both infinities, on channel 0; values
    # around 10 next to 1e30 on channel 1 (the trimmed lookup grid); duplicates across stages
    special = [NAN, -1.5, -0.0, 0.0, 254.5, 255.0, 300.0, INF, -INF]
    ch1 = [5.0 + 0.5 * i for i in range(20)] + [1e30]
    d["thresholds"] = full_cascade(11, W, 2, [(0, t) for t in special + [NAN, 0.0, 255.0]] + [(1, t) for t in ch1])
    # twenty consecutive floats in one cell of the byte ranks' grid whatever it is trimmed to: no rank8, rank16
    run = [np.float32(10.0)]
    while len(run) < 20:
        run.append(np.nextafter(run[-1], np.float32(INF)))
    rng = np.random.default_rng(12)
    around = [float(x) for x in np.float32(rng.uniform(0, 9, 14))] + [float(x) for x in np.float32(rng.uniform(11, 60, 14))]
    d["cluster"] = full_cascade(13, W, 3, [(2, float(t)) for t in run] + [(2, t) for t in around] +
                                [(c if c != 2 else 3, t) for c, t in spread(14, 8, 0, 60, 4)])
    # 280 distinct thresholds on one channel: more than a byte ranks, fewer than two bytes do
    d["long"] = full_cascade(15, W, 3, [(1, float(t)) for t in np.linspace(0, 70, 280).astype(np.float32)])
    # other channel counts: no rank tables
    d["c3"] = full_cascade(16, (5, 6, 3), 2, spread(17, 9, 0, 60, 3))
    d["c10"] = full_cascade(18, (5, 6, 10), 2, spread(19, 9, 0, 60, 10))
    # a window whose float32 tile does not fit the LDS budget until the rows per wave are halved twice
    d["lds"] = full_cascade(20, (30, 30, 10), 2, spread(21, 9, 0, 60, 10))
    # deeper than the tile kernels go: the node-walk model, no records
    d["generic"] = full_cascade(22, W, 4, spread(23, 15, 0, 60, 4))
    return d


# ------------------------------------------------------------------------------ the library
def create(lib, model, dump_path):
    """wb_model_create with the dump switched on: (return code, handle)."""
    os.environ["WB_DUMP_STAGES"] = dump_path
    try:
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        m, n, Cc = (int(x) for x in model["window"])
        rc = lib.wb_model_create(int(model["theta"].size), vp(model["node_off"]), vp(model["feature"]), vp(model["threshold"]),
                                 vp(model["left"]), vp(model["right"]), vp(model["prediction"]), vp(model["theta"]), m, n, Cc, C.byref(h))
    finally:
        del os.environ["WB_DUMP_STAGES"]
    return rc, h


def read_dump(path):
    """(header[:3], mask or None, {form: table}) of a WB_DUMP_STAGES file in either of its two formats (module docstring)."""
    raw = np.fromfile(path, np.int32)
    hdr, body = raw[:4], raw[4:]
    words = int(hdr[0]) * int(hdr[1])
    if hdr[3] in (0, 1):                                   # before the reorganisation: rank_ok, three tables
        assert body.size == 3 * words
        forms = [F32, U8] + ([RANK8] if hdr[3] else [])
        mask = None
    else:
        mask = int(hdr[3])
        forms = [f for f in range(4) if mask >> f & 1]
        assert body.size == len(forms) * words
    return hdr[:3].copy(), mask, {f: body[i * words:(i + 1) * words].copy() for i, f in enumerate(forms)}


def main():
    from waldboost_amd import _native as nat
    lib = nat.load()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, model in designs().items():
            for k, v in model.items():
                out[f"{name}/{k}"] = v
            path = os.path.join(tmp, name + ".bin")
            rc, h = create(lib, model, path)
            assert rc in (0, nat.WB_ERR_HIP), (name, rc, nat.last_error())
            info = nat.WbModelInfo()
            if rc == 0:
                nat.check(lib.wb_model_info(h, C.byref(info)), "wb_model_info")
                nat.check(lib.wb_model_destroy(h), "wb_model_destroy")
                out[f"{name}/info"] = np.array([info.n_stages, info.depth, info.tile_rows, info.tile_cols, info.lds_bytes], np.int32)
            if EXPECT[name] is None:
                assert not os.path.exists(path), name
                print(f"{name:11s} node-walk model, no dump; info {out.get(name + '/info')}")
                continue
            hdr, mask, tables = read_dump(path)
            if rc == 0:
                seen = 3 | info.rank_ok << 2 | info.rank16_ok << 3
                assert mask in (None, seen), (name, mask, seen)
                mask = seen
            assert mask is not None, "a dump without its mask needs wb_model_info: run on a GPU"
            assert (mask, int(hdr[2])) == EXPECT[name], (name, mask, hdr)
            assert (mask >> RANK8 & 1) == (RANK8 in tables)
            out[f"{name}/hdr"], out[f"{name}/mask"] = hdr, np.int32(mask)
            for f in (F32, U8, RANK8):
                if f in tables:
                    out[f"{name}/{FORMS[f]}"] = tables[f]
            print(f"{name:11s} records {hdr[0]:3d} x {hdr[1]:2d} dwords, depth {hdr[2]}, mask {mask:2d}, info {out.get(name + '/info')}")
    path = os.path.join(HERE, "stage_records.npz")
    np.savez_compressed(path, **out)
    print(f"stage record fixture written: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
