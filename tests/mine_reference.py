"""The mining rule of samples.mine_batch / wb_mine_select_launch / wb_mine_gather_launch, stated in NumPy.
No GPU, no torch.  From detection records, ground truth and parameters: every record's label, owner and best IoU, and the
chosen rows in (image, level, r, c) order; crops out of a pyramid buffer; fmix32 and its inverse."""
import numpy as np

DET = np.dtype([("image", "<i4"), ("level", "<i4"), ("r", "<u2"), ("c", "<u2"), ("score", "<f4")], align=True)
ROW = np.dtype([("image", "<i4"), ("level", "<i4"), ("r", "<u2"), ("c", "<u2"), ("score", "<f4"), ("best", "<f8"), ("owner", "<i4"),
                ("label", "<i4")], align=True)
LEVEL = np.dtype([("chn_off", "<i8"), ("u", "<i4"), ("v", "<i4")], align=True)
assert DET.itemsize == 16 and ROW.itemsize == 32 and LEVEL.itemsize == 16
TP, FP, IGNORE = 1, -1, 0
_M = 0xFFFFFFFF
_INV1, _INV2 = pow(0x85EBCA6B, -1, 1 << 32), pow(0xC2B2AE35, -1, 1 << 32)


def fmix32(x):
    """MurmurHash3's 32-bit finaliser on uint32 values (scalar or array): a bijection of the 32-bit words."""
    x = np.asarray(x, np.uint64) & _M
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M
    x ^= x >> 16
    return x.astype(np.uint32)


def unfmix32(y):
    """The inverse of fmix32."""
    y = np.asarray(y, np.uint64) & _M
    y ^= y >> 16
    y = (y * _INV2) & _M
    y ^= (y >> 13) ^ (y >> 26)
    y = (y * _INV1) & _M
    y ^= y >> 16
    return y.astype(np.uint32)


def group_word(seed, serial, level):
    s = fmix32((np.asarray(serial, np.uint64) + 0x9E3779B9) & _M)
    return fmix32(fmix32(np.uint64(int(seed) & _M) ^ s.astype(np.uint64)).astype(np.uint64) ^ ((np.asarray(level, np.uint64) * 0x9E3779B1) & _M))


def window_keys(seed, serial, level, r, c):
    rc = (np.asarray(r, np.uint64) << 16) | np.asarray(c, np.uint64)
    return fmix32(rc ^ group_word(seed, serial, level).astype(np.uint64))


def window_of_key(seed, serial, level, key):
    """(r, c) of the window of group (serial, level) that carries `key`."""
    rc = unfmix32(key).astype(np.uint64) ^ group_word(seed, serial, level).astype(np.uint64)
    return (rc >> 16).astype(np.uint16), (rc & 0xFFFF).astype(np.uint16)


def record_boxes(level, r, c, inv_scale, m, n):
    """float32 [c, r, c + n, r + m] * inv_scale[level]: wb_boxes_launch's arithmetic."""
    sc = np.asarray(inv_scale, np.float32)[level]
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    f = lambda v: v.astype(np.float32) * sc
    return np.stack([f(c), f(r), f(c + n), f(r + m)], axis=1).astype(np.float32)


def iou_table(dt, gt):
    """boxes.iou, operation by operation, float64."""
    A, B = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    ax1, ay1, ax2, ay2 = (A[:, None, k] for k in range(4))
    bx1, by1, bx2, by2 = (B[None, :, k] for k in range(4))
    iw = np.where(ax2 < bx2, ax2, bx2) - np.where(ax1 > bx1, ax1, bx1)
    ih = np.where(ay2 < by2, ay2, by2) - np.where(ay1 > by1, ay1, by1)
    iw, ih = np.where(iw < 0, 0.0, iw), np.where(ih < 0, 0.0, ih)
    inter = iw * ih
    uni = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter
    return np.where(uni > 0, inter / np.where(uni > 0, uni, 1), 0.0)


def match(det, inv_scale, m, n, gts):
    """(best float64, owner int32) of every record: gts[b] is image b's float64 [G, 4] (None / empty: no ground truth)."""
    det = np.asarray(det, DET)
    best, owner = np.zeros(det.size, np.float64), np.full(det.size, -1, np.int32)
    boxes = record_boxes(det["level"], det["r"], det["c"], inv_scale, m, n)
    for b in np.unique(det["image"]):
        g = gts[b]
        at = np.flatnonzero(det["image"] == b)
        if g is None or len(g) == 0:
            continue
        t = iou_table(boxes[at], g)
        o = np.argmax(t, axis=1)
        best[at], owner[at] = t[np.arange(at.size), o], o
    return best, owner


def mine(det, inv_scale, m, n, gts, ignores, serial, min_tp_iou=0.7, max_fp_iou=0.3, max_tp=100, max_fp=100, want_tp=True,
         want_fp=True, seed=0):
    """The rule.  det: DET records in any order (image in [0, len(gts)), level in [0, len(inv_scale))); ignores[b]: the
    flags of gts[b].  Returns dict(label, owner, best: per record, in the records' order; rows: the chosen records as ROW
    in (image, level, r, c) order)."""
    det = np.asarray(det, DET)
    best, owner = match(det, inv_scale, m, n, gts)
    has_gt = owner >= 0
    ign = np.zeros(det.size, bool)
    for b in np.unique(det["image"]):
        at = np.flatnonzero((det["image"] == b) & has_gt)
        if at.size:
            ign[at] = np.asarray(ignores[b])[owner[at]] != 0
    fp_hit = (~has_gt | (best < float(max_fp_iou))) & bool(want_fp)
    tp_hit = has_gt & (best > float(min_tp_iou)) & ~ign & bool(want_tp)
    keys = window_keys(seed, np.asarray(serial, np.uint32)[det["image"]], det["level"], det["r"], det["c"])
    label = np.full(det.size, IGNORE, np.int32)
    group = det["image"].astype(np.int64) * len(inv_scale) + det["level"]
    for hit, cap, lab in ((tp_hit, max_tp, TP), (fp_hit, max_fp, FP)):          # TP first, then FP
        for g in np.unique(group[hit]):
            at = np.flatnonzero(hit & (group == g))
            assert np.unique(keys[at]).size == at.size, "keys tie inside a group: (r, c) not unique"
            label[at[np.argsort(keys[at])[:min(at.size, int(cap))]]] = lab
    chosen = np.flatnonzero(label != IGNORE)
    chosen = chosen[np.lexsort((det["c"][chosen], det["r"][chosen], det["level"][chosen], det["image"][chosen]))]
    rows = np.zeros(chosen.size, ROW)
    for k in DET.names:
        rows[k] = det[k][chosen]
    rows["best"], rows["owner"], rows["label"] = best[chosen], owner[chosen], label[chosen]
    return dict(label=label, owner=owner, best=best, keys=keys, rows=rows)


def ordered(rows):
    """ROW records in (image, level, r, c) order."""
    rows = np.asarray(rows, ROW)
    return rows[np.lexsort((rows["c"], rows["r"], rows["level"], rows["image"]))]


def gather(buf, img_stride, levels, C, rows, m, n):
    """(out [N, m, n, C], err): the crops of `rows` out of the flat pyramid buffer; a window outside its level is zeros and
    sets err."""
    levels = np.asarray(levels, LEVEL)
    out = np.zeros((len(rows), m, n, C), buf.dtype)
    err = 0
    n_images = buf.size // img_stride if img_stride else 0
    for i, w in enumerate(rows):
        b, l, r, c = int(w["image"]), int(w["level"]), int(w["r"]), int(w["c"])
        ok = 0 <= b < n_images and 0 <= l < levels.size
        if ok:
            off, u, v = int(levels[l]["chn_off"]), int(levels[l]["u"]), int(levels[l]["v"])
            ok = r + m <= u and c + n <= v and off >= 0 and off + u * v * C <= img_stride
        if not ok:
            err = 1
            continue
        lev = buf[b * img_stride + off: b * img_stride + off + u * v * C].reshape(u, v, C)
        out[i] = lev[r:r + m, c:c + n]
    return out, err
