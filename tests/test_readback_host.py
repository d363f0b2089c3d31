"""CPU tests of waldboost_amd/readback.py: the finish block's layout, the sort key's fields, the host's ordering and box
arithmetic, and the shapes of the engine's read-back results."""
import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.readback import (FinishBlock, Finished, ImageResult, Packed, host_boxes, key_fits, key_positions,
                                    split_keys)


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
