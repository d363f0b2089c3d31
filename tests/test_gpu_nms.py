"""Non-maximum suppression on the device: waldboost_amd.non_max_suppression (wb_nms_launch) and the iou_threshold /
score_threshold keywords of Model.detect, detect_stream, detect_batch and waldboost_amd.detect (wb_nms_finish_launch
behind the scan) against the NumPy yardstick of tests/nms_reference.py -- keep masks equal exactly, boxes and scores
bit-identical and in the same order."""
import ctypes as C
import os

import numpy as np
import pytest

import waldboost_amd as wb
from waldboost_amd import _native as nat
from waldboost_amd.boxes import Boxes, nms_keep_mask
from waldboost_amd.synth import synth_image
from nms_designs import finish_block
from nms_reference import detector_like_boxes, hand_cases, nms_boxes, nms_keep
from util import GOLDEN

pytestmark = pytest.mark.gpu

HAND = list(hand_cases())


def same_boxes(a, b):
    return (len(a) == len(b) and np.array_equal(a.get().view(np.uint32), b.get().view(np.uint32))
            and np.array_equal(a.get_field("scores").view(np.uint32), b.get_field("scores").view(np.uint32)))


def fixture_boxes(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))["det"]
    return Boxes(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], 1).astype(np.float32), scores=d["score"].astype(np.float32))


def detect_cases():
    yield "cfg1", os.path.join(GOLDEN, "cfg1_d1_T32.pb"), synth_image(480, 640, 0), synth_image(480, 640, 1)
    img = np.load(os.path.join(GOLDEN, "mixed_200x264.npz"))["image"]
    yield "mixed", os.path.join(GOLDEN, "mixed_d2_T24.pb"), img, np.ascontiguousarray(img[::-1])


def check_not_vacuous(plain, kept):
    assert len(plain) >= 50, len(plain)
    assert 1 <= len(kept) < len(plain), (len(kept), len(plain))


@pytest.mark.parametrize("t", [0.0, 0.2, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4095, 4096, 4097, 20000])
def test_non_max_suppression_equals_the_yardstick(n, t):
    boxes, scores = detector_like_boxes(n, 1000 + n)
    want = nms_keep(boxes, scores, t)
    got = nms_keep_mask(boxes, scores, t)
    print(f"n={n} t={t}: kept {int(want.sum())} (yardstick) {int(got.sum())} (device), differing flags {int((want != got).sum())}")
    assert np.array_equal(got, want)
    bx = Boxes(boxes, scores=scores, tag=np.arange(n))
    out = wb.non_max_suppression(bx, iou_threshold=t)
    assert np.array_equal(out.get_field("tag"), np.flatnonzero(want)) and same_boxes(out, bx[np.flatnonzero(want)])


@pytest.mark.parametrize("n", [1, 65, 4097, 20000])
def test_non_max_suppression_through_the_callers_order(n, monkeypatch):
    """Above 2**16 boxes the visiting order comes from a stable torch.sort and wb_nms_ordered_launch skips the rank pass;
    lowered to 0 here, so that the usual sizes go that way."""
    from waldboost_amd import boxes as B
    monkeypatch.setattr(B, "_NMS_RANK_MAX", 0)
    boxes, scores = detector_like_boxes(n, 3000 + n)
    scores[::7] = -0.0
    scores[3::7] = 0.0
    group = np.arange(n) % 3
    for t in (0.0, 0.2):
        assert np.array_equal(nms_keep_mask(boxes, scores, t), nms_keep(boxes, scores, t))
        assert np.array_equal(nms_keep_mask(boxes, scores, t, score_threshold=0.0, group=group),
                              nms_keep(boxes, scores, t, score_threshold=0.0, group=group))


def test_non_max_suppression_of_more_boxes_than_the_rank_pass_takes():
    """70 000 boxes: torch.sort + wb_nms_ordered_launch, eighteen bands of 4096 rows."""
    n = 70000
    boxes, scores = detector_like_boxes(n, 9)
    want = nms_keep(boxes, scores, 0.2)
    got = nms_keep_mask(boxes, scores, 0.2)
    print(f"n={n}: kept {int(want.sum())} (yardstick) {int(got.sum())} (device)")
    assert 0 < want.sum() < n and np.array_equal(got, want)


@pytest.mark.parametrize("n", [65, 1000, 4097, 20000])
def test_non_max_suppression_with_groups_and_a_score_threshold(n):
    boxes, scores = detector_like_boxes(n, 2000 + n)
    group = np.random.default_rng(n).integers(0, 3, n) * 7 - 3        # three groups, arbitrary labels
    for t in (0.0, 0.2):
        want = nms_keep(boxes, scores, t, group=group)
        assert np.array_equal(nms_keep_mask(boxes, scores, t, group=group), want)
        assert want.sum() > nms_keep(boxes, scores, t).sum() or n < 100
        want = nms_keep(boxes, scores, t, score_threshold=0.125)
        assert 0 < want.sum() and not want[scores < 0.125].any()
        assert np.array_equal(nms_keep_mask(boxes, scores, t, score_threshold=0.125), want)
        want = nms_keep(boxes, scores, t, group=group, score_threshold=-1.0)
        assert np.array_equal(nms_keep_mask(boxes, scores, t, score_threshold=-1.0, group=group), want)


def test_non_max_suppression_in_bands_with_a_small_scratch():
    """The caller's scratch decides the band: with room for 64 matrix rows 1000 boxes take sixteen bands; same flags."""
    import torch
    lib = nat.load()
    n = 1000
    boxes, scores = detector_like_boxes(n, 77)
    n64, W = 1024, 16
    fixed = (25 * n64 + 16 * W + 16 + 255) // 256 * 256
    for rows in (64, 192):
        d_b, d_s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        scratch = torch.empty(fixed + rows * W * 8, dtype=torch.uint8, device="cuda")
        out = torch.zeros(4 + n, dtype=torch.uint8, device="cuda")
        nat.check(lib.wb_nms_launch(nat.stream_ptr(), nat.ptr(d_b), nat.ptr(d_s), None, n, 0.2, 0, 0.0, nat.ptr(scratch), scratch.numel(),
                                    C.c_void_p(out.data_ptr() + 4), nat.ptr(out)), "wb_nms_launch")
        h = out.cpu().numpy()
        want = nms_keep(boxes, scores, 0.2)
        assert np.array_equal(h[4:].astype(bool), want) and int(h[:4].view(np.uint32)[0]) == int(want.sum())


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written_answers_on_the_device(case):
    _, boxes, scores, t, group, st, expected = case
    assert nms_keep_mask(boxes, scores, t, score_threshold=st, group=group).astype(int).tolist() == expected


@pytest.mark.parametrize("t,kept", [(0.0, 85), (0.2, 198), (0.5, 366)])
def test_recorded_reference_detections(t, kept):
    bx = fixture_boxes("cfg1_640x480")
    want = nms_boxes(bx, t)
    assert len(bx) == 855 and len(want) == kept
    assert same_boxes(wb.non_max_suppression(bx, iou_threshold=t), want)
    mx = fixture_boxes("mixed_200x264")
    assert same_boxes(wb.non_max_suppression(mx, iou_threshold=t), nms_boxes(mx, t))


@pytest.mark.parametrize("t", [0.2, 0.5])
@pytest.mark.parametrize("case", list(detect_cases()), ids=["cfg1", "mixed"])
def test_detect_with_a_threshold_equals_the_yardstick_on_the_plain_result(case, t):
    _, path, img, other = case
    P, M = wb.load(path), wb.load(path)
    for k, im in enumerate((img, img, img, other, other)):           # first call, graph capture, replay; then another image
        plain = P.detect(im)
        want = nms_boxes(plain, t)
        got = M.detect(im, iou_threshold=t)
        print(f"call {k}: {len(plain)} detections, yardstick keeps {len(want)}, device {len(got)}")
        check_not_vacuous(plain, want)
        assert same_boxes(got, want), f"call {k}"
        assert (M.n_loc, M.n_weak) == (P.n_loc, P.n_weak)
    want = nms_boxes(plain, t, score_threshold=0.0)
    assert same_boxes(M.detect(other, iou_threshold=t, score_threshold=0), want) and len(want) >= 1


@pytest.mark.parametrize("case", list(detect_cases()), ids=["cfg1", "mixed"])
def test_detect_with_a_threshold_on_the_fall_back_route(case, monkeypatch):
    """More detections than the one read-back holds (shrunk to 64 rows): the result comes by further copies and goes
    through non_max_suppression as a whole."""
    from waldboost_amd import engine as E
    _, path, img, other = case
    E._ENGINES.clear()                                  # (cached engines hold read-back buffers of the usual size)
    monkeypatch.setattr(E.PyramidEngine, "_FETCH_ROWS", 64)
    monkeypatch.setattr(E.PyramidEngine, "_ORDER_ROWS", 64)
    try:
        P, M = wb.load(path), wb.load(path)
        for im in (img, img, img, other):
            plain = P.detect(im)
            want = nms_boxes(plain, 0.2)
            assert len(plain) > 64
            check_not_vacuous(plain, want)
            assert same_boxes(M.detect(im, iou_threshold=0.2), want)
        ims = [img, other, img, other, img]
        got = list(M.detect_stream(ims, lanes=2, batch=4, iou_threshold=0.2))
        assert all(same_boxes(g, nms_boxes(P.detect(im), 0.2)) for g, im in zip(got, ims))
    finally:
        E._ENGINES.clear()


def fixture_variants(k):
    """k images of the 'mixed' fixture's shape with detections enough in each: the fixture image mirrored and shifted."""
    img = np.load(os.path.join(GOLDEN, "mixed_200x264.npz"))["image"]
    forms = [img, img[::-1], img[:, ::-1], img[::-1, ::-1]]
    return [np.ascontiguousarray(np.roll(forms[i % 4], 5 * (i // 4), axis=1)) for i in range(k)]


def stream_images():
    """Eight images of two shapes."""
    wide = [np.ascontiguousarray(np.concatenate([v, v[:, :40]], 1)) for v in fixture_variants(3)]
    v = fixture_variants(5)
    return [v[0], v[1], wide[0], v[2], wide[1], wide[2], v[3], v[4]]


@pytest.mark.parametrize("batch", [1, 4])
def test_detect_stream_with_a_threshold_equals_the_per_image_result(batch):
    path = os.path.join(GOLDEN, "mixed_d2_T24.pb")
    P, M = wb.load(path), wb.load(path)
    ims = stream_images() * 2                           # (the second pass finds every lane's graph captured)
    plain = [P.detect(im) for im in ims]
    want = [nms_boxes(p, 0.2) for p in plain]
    got = list(M.detect_stream(iter(ims), lanes=3, batch=batch, iou_threshold=0.2))
    print("detections", [len(p) for p in plain], "kept", [len(w) for w in want])
    assert len(got) == len(ims) and len({im.shape for im in ims}) == 2
    for i, (g, w, p) in enumerate(zip(got, want, plain)):
        check_not_vacuous(p, w)
        assert same_boxes(g, w), f"image {i}"
    assert (M.n_loc, M.n_weak) == (P.n_loc, P.n_weak)
    got = list(M.detect_stream(iter(ims[:4]), lanes=3, batch=batch, iou_threshold=0.5, score_threshold=0.0))
    for i, (g, p) in enumerate(zip(got, plain)):
        assert same_boxes(g, nms_boxes(p, 0.5, score_threshold=0.0)), f"image {i}"
    # ... and the plain stream afterwards is the plain result
    for g, p in zip(M.detect_stream(iter(ims[:4]), lanes=3, batch=batch), plain):
        assert same_boxes(g, p)


def test_detect_batch_with_a_threshold():
    path = os.path.join(GOLDEN, "mixed_d2_T24.pb")
    P, M = wb.load(path), wb.load(path)
    ims = np.stack(fixture_variants(5))
    plain = [P.detect(im) for im in ims]
    for t in (0.2, 0.5):
        got = M.detect_batch(ims, iou_threshold=t)
        want = [nms_boxes(p, t) for p in plain]
        for p, w in zip(plain, want):
            check_not_vacuous(p, w)
        assert len(got) == 5 and all(same_boxes(g, w) for g, w in zip(got, want))
    assert all(same_boxes(g, p) for g, p in zip(M.detect_batch(ims), plain))


def test_detect_batch_of_more_images_than_the_ordered_read_back_takes():
    """More than 256 images: the batch's records are ordered by a device sort of all of them and suppressed image by
    image (wb_nms_launch per image; never one call over the whole batch)."""
    path = os.path.join(GOLDEN, "mixed_d2_T24.pb")
    P, M = wb.load(path), wb.load(path)
    forms = fixture_variants(4)
    ims = np.stack([forms[i % 4] for i in range(260)])
    plain = [P.detect(f) for f in forms]
    want = [nms_boxes(p, 0.2) for p in plain]
    for p, w in zip(plain, want):
        check_not_vacuous(p, w)
    got = M.detect_batch(ims, iou_threshold=0.2)
    assert len(got) == 260
    for i, g in enumerate(got):
        assert same_boxes(g, want[i % 4]), f"image {i}"
    assert M.n_loc == 65 * P.n_loc and M.n_weak == 65 * P.n_weak
    full = M.detect_batch(ims)
    assert all(same_boxes(g, plain[i % 4]) for i, g in enumerate(full))


def test_detect_with_a_threshold_when_the_detection_buffer_overflows():
    """A shard overflows: the scan is repeated with a larger buffer, and NMS runs again on the new scan."""
    from waldboost_amd import engine as E
    path = os.path.join(GOLDEN, "models", "cfg2_d2_T128.pb")
    P, M = wb.load(path), wb.load(path)
    img = synth_image(1080, 1920, 0)
    plain = P.detect(img)
    want = nms_boxes(plain, 0.3)
    check_not_vacuous(plain, want)
    assert len(plain) > 16 * nat.WB_DET_SHARDS                  # (more than 64 shards of 16 records hold)
    E._ENGINES.clear()
    try:
        assert same_boxes(M.detect(img, iou_threshold=0.3), want)
        for k in range(3):                                       # (before the capture, and with a captured graph)
            eng = next(iter(E._ENGINES.values()))
            eng.det_capacity = 16 * nat.WB_DET_SHARDS
            eng._alloc_det()
            assert same_boxes(M.detect(img, iou_threshold=0.3), want), f"call {k}"
            assert eng.det_capacity > 16 * nat.WB_DET_SHARDS    # (it did overflow and grow)
            assert same_boxes(M.detect(img, iou_threshold=0.3), want), f"call {k}, again"
    finally:
        E._ENGINES.clear()


def test_multi_model_detect_with_a_threshold_separate_or_not():
    A = wb.load(os.path.join(GOLDEN, "mixed_d2_T24.pb"))
    B = wb.load(os.path.join(GOLDEN, "models", "cfg2_d2_T128.pb"))
    img = synth_image(240, 320, 3)
    scale = [1.0, 0.5]
    plain = wb.detect(img, A, B, response_scale=scale)
    labels = plain.get_field("label")
    assert len(plain) >= 50 and 0 < (labels == 0).sum() < len(plain)
    for _ in range(2):
        for t in (0.2, 0.5):
            one = wb.detect(img, A, B, response_scale=scale, iou_threshold=t)
            sep = wb.detect(img, A, B, response_scale=scale, iou_threshold=t, separate=True)
            w_one, w_sep = nms_boxes(plain, t), nms_boxes(plain, t, group=labels)
            assert 0 < len(w_one) < len(plain) and len(w_one) <= len(w_sep) < len(plain)
            assert same_boxes(one, w_one) and np.array_equal(one.get_field("label"), w_one.get_field("label"))
            assert same_boxes(sep, w_sep) and np.array_equal(sep.get_field("label"), w_sep.get_field("label"))
    assert same_boxes(wb.detect(img, A, B, response_scale=scale), plain)


@pytest.mark.parametrize("case", list(detect_cases()), ids=["cfg1", "mixed"])
def test_the_threshold_does_not_leak_into_the_plain_call(case):
    _, path, img, _ = case
    M = wb.load(path)
    for _ in range(3):
        kept = M.detect(img, iou_threshold=0.2)
        full = M.detect(img)
        fresh = wb.load(path).detect(img)
        want = nms_boxes(fresh, 0.2)
        check_not_vacuous(fresh, want)
        assert same_boxes(full, fresh) and same_boxes(kept, want)


def test_nms_on_hand_built_finish_blocks():
    """wb_nms_finish_launch on three blocks built here: one in packed order (header[3] = 0: the input order is the KEY
    order, the flags belong to the positions), one in key order (header[3] = 1), one that says it holds more detections
    than fit (done = 0, nothing else written for it)."""
    import torch
    lib, P = nat.load(), 1024
    rng = np.random.default_rng(5)
    n0, n1 = 700, 333
    b0, s0 = detector_like_boxes(n0, 11)
    b1, s1 = detector_like_boxes(n1, 12)
    keys0 = (rng.permutation(n0).astype(np.uint64) << np.uint64(26)) | np.arange(n0, dtype=np.uint64)     # unique, unsorted
    keys1 = np.sort(rng.permutation(5000)[:n1]).astype(np.uint64) << np.uint64(26)
    blocks = [finish_block(P, keys0, b0, s0, [n0, n0, n0, 0]), finish_block(P, keys1, b1, s1, [n1, n1, n1, 1]),
              finish_block(P, keys1, b1, s1, [P + 1, P + 1, P, 1])]
    fin = torch.from_numpy(np.concatenate(blocks)).cuda()
    need = C.c_size_t()
    nat.check(lib.wb_nms_finish_scratch_bytes(P, 3, C.byref(need)), "wb_nms_finish_scratch_bytes")
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    res = torch.full((3 * (16 + P),), 7, dtype=torch.uint8, device="cuda")
    nat.check(lib.wb_nms_finish_launch(nat.stream_ptr(), nat.ptr(fin), P, 3, 0.2, 0, 0.0, nat.ptr(scratch), scratch.numel(), nat.ptr(res)),
              "wb_nms_finish_launch")
    r = res.cpu().numpy().reshape(3, 16 + P)
    at = np.argsort(keys0)
    want0 = nms_keep(b0[at], s0[at], 0.2)
    assert 0 < want0.sum() < n0 and not np.array_equal(want0, nms_keep(b0, s0, 0.2)[at])     # (the order matters here)
    assert r[0, :16].view(np.uint32).tolist() == [int(want0.sum()), n0, 1, 0]
    assert np.array_equal(r[0, 16:16 + n0][at].astype(bool), want0)
    want1 = nms_keep(b1, s1, 0.2)
    assert r[1, :16].view(np.uint32).tolist() == [int(want1.sum()), n1, 1, 0]
    assert np.array_equal(r[1, 16:16 + n1].astype(bool), want1)
    assert r[2, :16].view(np.uint32).tolist() == [0, 0, 0, 0] and (r[2, 16:] == 7).all()
