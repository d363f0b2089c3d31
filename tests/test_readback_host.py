"""CPU tests of waldboost_amd/readback.py: the finish block's layout, the sort key's fields, the host's ordering and box
arithmetic, and the shapes of the engine's read-back results."""
import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.readback import (Detections, FinishBlock, Finished, ImageResult, Packed, from_finished, from_image_result,
                                    from_ordered, from_packed, host_boxes, key_fits, key_positions, split_keys)


@pytest.mark.parametrize("rows", [4, 64, 4096])
def test_finish_block_views_sit_at_the_documented_offsets(rows):
    blk = FinishBlock(rows)
    assert blk.nbytes == 16 + 28 * rows
    # a block at offset 0, and block 2 of three behind a 16-byte prefix
    for size, at in ((blk.nbytes, 0), (16 + 3 * blk.nbytes, 16 + 2 * blk.nbytes)):
        buf = np.zeros(size, np.uint8)
        for k, (o, nb) in enumerate(((0, 16), (16, 8 * rows), (16 + 8 * rows, 16 * rows), (16 + 24 * rows, 4 * rows))):
            buf[at + o:at + o + nb] = 0x11 * (k + 1)
        hdr, keys, boxes, scores = blk.views(buf, at)
        assert (hdr.dtype, hdr.shape) == (np.int32, (4,)) and (keys.dtype, keys.shape) == (np.uint64, (rows,))
        assert (boxes.dtype, boxes.shape) == (np.float32, (rows, 4)) and (scores.dtype, scores.shape) == (np.float32, (rows,))
        for k, v in enumerate((hdr, keys, boxes, scores)):
            assert np.all(v.reshape(-1).view(np.uint8) == 0x11 * (k + 1))
            assert np.shares_memory(v, buf)
        rest = buf.copy()
        rest[at:at + blk.nbytes] = 0
        assert not rest.any()                         # (the patterns went into this block only)
        keys[rows - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)       # a write through a view lands in the buffer
        assert np.all(buf[at + 16 + 8 * (rows - 1):at + 16 + 8 * rows] == 0xFF)


def test_sort_keys_round_trip_at_the_corners_of_their_fields():
    corners = [(lv, r, c, pos) for lv in (0, 1023) for r in (0, 16383) for c in (0, 16383) for pos in (0, (1 << 26) - 1)]
    keys = np.array([lv << 54 | r << 40 | c << 26 | pos for lv, r, c, pos in corners], np.uint64)
    level, r, c = split_keys(keys)
    pos = key_positions(keys)
    assert (level.dtype, r.dtype, c.dtype, pos.dtype) == (np.int32, np.int64, np.int64, np.intp)
    assert [tuple(int(x) for x in row) for row in zip(level, r, c, pos)] == corners
    empty = split_keys(np.empty(0, np.uint64))
    assert [a.dtype for a in empty] == [np.int32, np.int64, np.int64] and all(a.size == 0 for a in empty)


def test_key_fits_on_both_sides_of_each_limit():
    assert not key_fits(0, 100, 100)
    assert key_fits(1, 100, 100) and key_fits(1024, 16384, 16384)
    assert not key_fits(1025, 100, 100)
    assert key_fits(3, 16384, 100) and not key_fits(3, 16385, 100)
    assert key_fits(3, 100, 16384) and not key_fits(3, 100, 16385)


SCALES = (1.0, 0.7937005, 0.5)


def random_records(n_images, seed):
    """50 WbDet records of distinct windows over 3 levels (and n_images images), shuffled."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(n_images * 3 * 40 * 50, 50, replace=False)
    d = np.zeros(50, nat.DET_DTYPE)
    d["image"], d["level"], d["r"], d["c"] = cells // 6000, cells // 2000 % 3, cells // 50 % 40, cells % 50
    d["score"] = rng.standard_normal(50).astype(np.float32)
    return d


@pytest.mark.parametrize("n_images", [1, 2])
def test_host_boxes_orders_like_the_reference_and_forms_get_boxes(n_images):
    m, n = 13, 9
    M = wb.Model((m, n, 4), {})
    inv = np.array([np.float32(1.0 / s) for s in SCALES], np.float32)
    d = random_records(n_images, 5 + n_images)
    assert len(set(d["level"].tolist())) == 3 and len(set(d["image"].tolist())) == n_images
    # (once as records, once as the int32 [k, 4] rows they are read back as)
    image, level, r, c, boxes, scores = host_boxes(d if n_images == 1 else d.view(np.int32).reshape(-1, 4), m, n, inv,
                                                   with_image=n_images > 1)
    rows = sorted((int(x["image"]), int(x["level"]), int(x["r"]), int(x["c"]), float(x["score"])) for x in d)
    assert (level.dtype, r.dtype, c.dtype, boxes.dtype, scores.dtype) == (np.int32, np.int64, np.int64, np.float32, np.float32)
    if n_images == 1:
        assert image is None
    else:
        assert image.dtype == np.int64 and image.tolist() == [x[0] for x in rows]
    assert list(zip(level.tolist(), r.tolist(), c.tolist())) == [x[1:4] for x in rows]
    assert scores.tolist() == [x[4] for x in rows]
    want = [M.get_boxes([x[2] for x in rows if x[:2] == (b, lv)], [x[3] for x in rows if x[:2] == (b, lv)], SCALES[lv]).get()
            for b in range(n_images) for lv in range(3)]
    want = np.concatenate(want)
    assert boxes.shape == want.shape == (50, 4) and want.dtype == np.float32
    assert np.array_equal(boxes.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("with_image", [False, True])
def test_host_boxes_of_no_records(with_image):
    inv = np.array([np.float32(1.0 / s) for s in SCALES], np.float32)
    image, level, r, c, boxes, scores = host_boxes(np.zeros(0, nat.DET_DTYPE), 13, 9, inv, with_image=with_image)
    assert (image is None) != with_image
    assert level.shape == r.shape == c.shape == scores.shape == (0,) and boxes.shape == (0, 4)
    assert (level.dtype, r.dtype, c.dtype, boxes.dtype, scores.dtype) == (np.int32, np.int64, np.int64, np.float32, np.float32)


def test_result_tuples_have_their_fields():
    assert Finished._fields == ("keys", "boxes", "scores", "alive", "ordered", "keep")
    assert ImageResult._fields == ("keys", "boxes", "scores", "keep")
    assert Packed._fields == ("total", "records", "alive")


# ------------------------------------------------------------------------------ one result type, one converter per form
WIN = (13, 9)
INV = np.array([np.float32(1.0 / s) for s in SCALES], np.float32)


def designed(counts, seed, stale=0):
    """Per image of `counts` that many detections at distinct windows over 3 levels, as the reference orders them:
    [(level, r, c, boxes, scores, keep)], the boxes by Model.get_boxes; and WbDet records of all of them in a shuffled
    order, with `stale` more that belong to the slot behind the last image."""
    rng = np.random.default_rng(seed)
    M = wb.Model(WIN + (4,), {})
    want, recs = [], []
    for b, k in enumerate(list(counts) + [stale]):
        cells = np.sort(rng.choice(3 * 40 * 50, k, replace=False))
        level, r, c = (cells // 2000).astype(np.int32), (cells // 50 % 40).astype(np.int64), (cells % 50).astype(np.int64)
        scores = rng.standard_normal(k).astype(np.float32)
        d = np.zeros(k, nat.DET_DTYPE)
        d["image"], d["level"], d["r"], d["c"], d["score"] = b, level, r, c, scores
        recs.append(d)
        if b < len(counts):
            boxes = [M.get_boxes(r[level == lv], c[level == lv], SCALES[lv]).get() for lv in range(3)]
            want.append((level, r, c, np.concatenate(boxes).astype(np.float32), scores, rng.random(k) < 0.5))
    recs = np.concatenate(recs)
    return want, recs[rng.permutation(recs.size)]


def keys_of(level, r, c, pos):
    return (level.astype(np.uint64) << np.uint64(54) | r.astype(np.uint64) << np.uint64(40) | c.astype(np.uint64) << np.uint64(26)
            | pos.astype(np.uint64))


def block(w, rows, pos):
    """One image's finish-block sections of `rows` rows with detection i at row pos[i] (stale values elsewhere):
    (keys by detection, boxes, scores, keep by row)."""
    level, r, c, boxes, scores, keep = w
    bx, sc, kp = np.full((rows, 4), -7.0, np.float32), np.full(rows, -7.0, np.float32), np.zeros(rows, bool)
    bx[pos], sc[pos], kp[pos] = boxes, scores, keep
    return keys_of(level, r, c, pos), bx, sc, kp


def forms(want, recs, seed):
    """name -> (convert() -> [Detections per image], the arrays it reads, whether it carries keep flags)."""
    rng = np.random.default_rng(seed)
    count, m, n = len(want), *WIN
    out = {}
    if count == 1:
        k = want[0][0].size
        alive = np.zeros((1, 3, 2), np.int64)
        keys, bx, sc, kp = block(want[0], k + 5, np.arange(k))
        out["finished_ordered"] = (lambda: [from_finished(Finished(keys, bx, sc, alive, True, kp[:k]))], [keys, bx, sc, kp], True)
        pos = rng.permutation(k + 5)[:k]
        ukeys, ubx, usc, ukp = block(want[0], k + 5, pos)
        mix = rng.permutation(k)
        ukeys = ukeys[mix]
        assert k < 2 or (not np.array_equal(pos, np.arange(k)) and not np.array_equal(ukeys, np.sort(ukeys)))
        out["finished_unordered"] = (lambda: [from_finished(Finished(ukeys, ubx, usc, alive, False, ukp))], [ukeys, ubx, usc, ukp], True)
    blocks = [block(w, w[0].size + 3, np.arange(w[0].size)) for w in want]
    out["image_results"] = (lambda: [from_image_result(ImageResult(ks, bx[:ks.size], sc[:ks.size], kp[:ks.size])) for ks, bx, sc, kp in blocks],
                            [a for blk in blocks for a in blk], True)
    rows = recs.view(np.int32).reshape(-1, 4).copy()
    out["packed"] = (lambda: from_packed(rows, count, m, n, INV), [rows], False)
    if count == 1 and recs.size == want[0][0].size:          # (no other slot's records: what a one-image engine packs)
        rows1 = rows.copy()
        out["packed_one_slot"] = (lambda: from_packed(rows1, 1, m, n, INV, one_slot=True), [rows1], False)
    image, level, r, c, boxes, scores = host_boxes(recs, m, n, INV, with_image=True)     # (its order and boxes: tested above)
    srt = np.zeros(recs.size, nat.DET_DTYPE)
    srt["image"], srt["level"], srt["r"], srt["c"], srt["score"] = image, level, r, c, scores
    srt = srt.view(np.int32).reshape(-1, 4)
    out["device_ordered"] = (lambda: from_ordered(srt, boxes, scores, count), [srt], False)
    return out


def same(got, w, with_keep):
    level, r, c = got.windows()
    assert [a.dtype for a in (got.boxes, got.scores, level, r, c)] == [np.float32, np.float32, np.int32, np.int64, np.int64]
    assert got.boxes.shape == (w[0].size, 4) and got.scores.shape == level.shape == r.shape == c.shape == (w[0].size,)
    assert np.array_equal(level, w[0]) and np.array_equal(r, w[1]) and np.array_equal(c, w[2])
    assert np.array_equal(got.boxes.view(np.uint32), w[3].view(np.uint32))
    assert np.array_equal(got.scores.view(np.uint32), w[4].view(np.uint32))
    if with_keep:
        assert got.keep.dtype == bool and np.array_equal(got.keep, w[5])
    else:
        assert got.keep is None


@pytest.mark.parametrize("counts,stale", [((0,), 0), ((1,), 0), ((200,), 0), ((200,), 30), ((40, 0, 60), 0), ((40, 0, 60), 25),
                                          ((0, 0, 0), 7)])
def test_every_read_back_form_gives_the_same_detections_and_owns_them(counts, stale):
    want, recs = designed(counts, 31 + sum(counts) + stale, stale)
    assert recs.size == sum(counts) + stale
    fs = forms(want, recs, 77)
    assert set(fs) == ({"image_results", "packed", "device_ordered"} | ({"finished_ordered", "finished_unordered"} if len(counts) == 1 else set())
                       | ({"packed_one_slot"} if len(counts) == 1 and not stale else set()))
    for name, (convert, sources, with_keep) in fs.items():
        got = convert()
        assert len(got) == len(counts) and all(isinstance(g, Detections) for g in got), name
        for g, w in zip(got, want):
            same(g, w, with_keep)
        # the results are the caller's own: the read-back buffers are written again by the next scan
        for g in got:
            for a in (g.boxes, g.scores, g.keep, g._keys) + (g._windows or ()):
                assert a is None or not any(np.shares_memory(a, s) for s in sources), name
        for s in sources:
            s.view(np.uint8)[...] = 0xA5
        for g, w in zip(got, want):
            same(g, w, with_keep)


def test_windows_are_split_on_demand_and_taken_rows_follow():
    (w,), recs = designed((50,), 3)
    keys, bx, sc, kp = block(w, 50, np.arange(50))
    got = from_finished(Finished(keys, bx, sc, np.zeros((1, 3, 2), np.int64), True, kp[:50]))
    assert got._windows is None                           # (Model.detect never pays for them)
    at = np.flatnonzero(w[5])
    for part in (got.take(at), (got.windows(), got.take(at))[1]):      # before and after the split
        same(part, tuple(a[at] for a in w), False)
    # a caller that wants boxes and scores alone does not even have the keys copied
    fin = Finished(keys, bx, sc, np.zeros((1, 3, 2), np.int64), True, kp[:50])
    for bare in (from_finished(fin, windows=False), from_finished(fin._replace(ordered=False), windows=False),
                 from_image_result(ImageResult(keys, bx, sc, kp[:50]), windows=False)):
        assert bare._keys is None and np.array_equal(bare.boxes, w[3]) and np.array_equal(bare.scores, w[4])
        assert np.array_equal(bare.take(at).scores, w[4][at])
        with pytest.raises(ValueError):
            bare.windows()
    none = Detections.none()
    same(none, tuple(a[:0] for a in w), False)
