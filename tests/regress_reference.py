"""The box regressor's rule as a NumPy statement: what waldboost_amd.regression and csrc/wb_regress.hip are
held to.  Pure NumPy, float64 throughout.

features   x = the (m, n, C) crop flattened row-major, j = (r * n + c) * C + ch, widened exactly; D = m * n * C
target     T = (float64(box_f32) - gt[owner]) * scale[level]: subtract first, then multiply, each rounded once
gram       S = A^T A, A = [X | 1 | T] (N x P, P = D + 5): X^T X, the column sums, X^T T, T^T T and N = S[D, D]
solve      mu = X^T 1 / N, tau = T^T 1 / N, Cxx = X^T X - N mu mu^T, Cxt = X^T T - N mu tau^T,
           W = solve(Cxx + l2 * (trace(Cxx) / D) * I, Cxt), b = tau - W^T mu (the intercept is not penalised)
predict    lane l of 64 keeps four partials from 0, adds x[j] * W[j][k] for j = l, l + 64, ... ascending (product and sum
           rounded separately), then for s = 32 .. 1: p[l] = p[l] + p[l ^ s]; pred[k] = p[0][k] + b[k]
refine     out = float32(float64(box_f32) - pred * inv64[level]), inv64 = 1.0 / scale[level]
"""
import numpy as np

LANES = 64


def features(crops):
    """(N, m, n, C) crops -> float64 (N, D), row-major."""
    crops = np.asarray(crops)
    return crops.reshape(crops.shape[0], -1).astype(np.float64)


def targets(boxes_f32, gt, owner, scale_of_row):
    """boxes_f32 (N, 4) float32, gt (N_gt, 4) float64, owner (N,) indices into gt, scale_of_row (N,) float64."""
    boxes_f32 = np.asarray(boxes_f32)
    assert boxes_f32.dtype == np.float32
    diff = boxes_f32.astype(np.float64) - np.asarray(gt, np.float64)[np.asarray(owner)]
    return diff * np.asarray(scale_of_row, np.float64)[:, None]


def design(X, T):
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64)
    return np.concatenate([X, np.ones((X.shape[0], 1)), T], axis=1)


def gram(X, T):
    """S = A^T A in float64 (NumPy's own order of summation: the kernel is held to a bound around the exact value)."""
    A = design(X, T)
    return A.T @ A


def moments(S):
    """(N, mu, tau, Cxx, Cxt, Ctt) of an accumulator; ValueError for N < 2 or non-finite entries."""
    S = np.asarray(S, np.float64)
    D = S.shape[0] - 5
    if S.ndim != 2 or S.shape[0] != S.shape[1] or D < 1:
        raise ValueError(f"an accumulator is (D + 5) x (D + 5), got {S.shape}")
    if not np.isfinite(S).all():
        raise ValueError("the accumulator holds non-finite values")
    N = S[D, D]
    if N < 2:
        raise ValueError(f"{N:g} samples: at least 2 are needed")
    mu, tau = S[:D, D] / N, S[D + 1:, D] / N
    Cxx = S[:D, :D] - N * np.outer(mu, mu)
    Cxt = S[:D, D + 1:] - N * np.outer(mu, tau)
    Ctt = S[D + 1:, D + 1:] - N * np.outer(tau, tau)
    return N, mu, tau, Cxx, Cxt, Ctt


def solve(S, l2=1e-2):
    """(W (D, 4), b (4,), rss (4,), tss (4,)) of an accumulator."""
    N, mu, tau, Cxx, Cxt, Ctt = moments(S)
    D = mu.size
    tr = np.trace(Cxx)
    if not tr > 0:
        raise ValueError("trace(Cxx) == 0: the features do not vary")
    W = np.linalg.solve(Cxx + l2 * (tr / D) * np.eye(D), Cxt)
    b = tau - W.T @ mu
    tss = np.diag(Ctt).copy()
    rss = tss - 2.0 * np.einsum("jk,jk->k", W, Cxt) + np.einsum("jk,jl,lk->k", W, Cxx, W)
    return W, b, rss, tss


def predict(X, W, b):
    """The lane / tree order, bit for bit what the kernel computes: X (N, D) float64, W (D, 4), b (4,) -> (N, 4)."""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    N, D = X.shape
    p = np.zeros((N, LANES, 4))
    for j0 in range(0, D, LANES):
        k = min(LANES, D - j0)
        prod = X[:, j0:j0 + k, None] * W[None, j0:j0 + k, :]
        p[:, :k] = p[:, :k] + prod
    lanes = np.arange(LANES)
    for s in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ s]
    return p[:, 0] + b


def refine(boxes_f32, pred, inv64_of_row):
    boxes_f32 = np.asarray(boxes_f32)
    assert boxes_f32.dtype == np.float32
    return (boxes_f32.astype(np.float64) - np.asarray(pred, np.float64) * np.asarray(inv64_of_row, np.float64)[:, None]).astype(np.float32)


def iou_rows(a, b):
    """IoU of box a[i] with box b[i], float64 (boxes.iou's arithmetic, row by row)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = np.maximum(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), 0)
    ih = np.maximum(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), 0)
    inter = iw * ih
    union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


# ---- the end-to-end statement on whole images, with the oracle's pyramid and an empty model (every window a detection)
def windows_of_image(pyramid, shape, gt, min_iou):
    """Every window of `pyramid` (a list of (chns, scale)) whose float32 grid box has IoU > min_iou to a box of gt
    (float64 (G, 4)): dict of crops, boxes (float32), owner, level -- in (level, r, c) order."""
    m, n, C = shape
    gt = np.asarray(gt, np.float64)
    out = dict(crops=[], boxes=[], owner=[], level=[])
    for li, (chns, scale) in enumerate(pyramid):
        u, v = chns.shape[:2]
        rs, cs = np.indices((max(u - m, 0), max(v - n, 0)))
        rs, cs = rs.reshape(-1), cs.reshape(-1)
        if rs.size == 0:
            continue
        rect = np.stack([cs, rs, cs + n, rs + m], 1).astype(np.float32)
        box = (rect * np.float32(1.0 / scale)).astype(np.float32)
        table = np.stack([iou_rows(box, np.broadcast_to(g, box.shape)) for g in gt], 1)
        owner = table.argmax(1)
        best = table[np.arange(box.shape[0]), owner]
        keep = np.flatnonzero(best > min_iou)
        out["crops"].append(np.stack([chns[r:r + m, c:c + n] for r, c in zip(rs[keep], cs[keep])]) if keep.size
                            else np.zeros((0, m, n, C), chns.dtype))
        out["boxes"].append(box[keep])
        out["owner"].append(owner[keep])
        out["level"].append(np.full(keep.size, li))
    return {k: np.concatenate(v) for k, v in out.items()}


def planted_images(seeds, size=(96, 128)):
    """The planted-square images of tests/test_gpu_mine.py::_training_images (its seeds are 0 .. 5), for any seeds: dicts of
    'image' (uint8) and 'gt' (float64 (2, 4))."""
    from waldboost_amd.synth import synth_image
    items = []
    for seed in seeds:
        img = synth_image(size[0], size[1], 100 + seed).astype(np.int32)
        rng = np.random.default_rng(seed)
        gt = []
        for side, x_lo in ((24, 4), (32, 60)):
            x, y = x_lo + int(rng.integers(0, 30)), 4 + int(rng.integers(0, size[0] - side - 8))
            img[y:y + side, x:x + side] += 90
            gt.append([x, y, x + side, y + side])
        items.append(dict(image=np.clip(img, 0, 255).astype(np.uint8), gt=np.array(gt, "f").astype(np.float64)))
    return items


def image_set(items, pyramid_of, shape, min_iou=0.5):
    """The statement's windows of a list of planted images: dict of X (N, D) float64, T (N, 4), boxes float32, gt (N, 4) the
    owning boxes, scale (N,).  pyramid_of(image) -> list of (chns, scale)."""
    parts = dict(X=[], T=[], boxes=[], gt=[], scale=[])
    for it in items:
        pyr = pyramid_of(it["image"])
        w = windows_of_image(pyr, shape, it["gt"], min_iou)
        scale = np.array([pyr[l][1] for l in w["level"]], np.float64)
        parts["X"].append(features(w["crops"]))
        parts["T"].append(targets(w["boxes"], it["gt"], w["owner"], scale))
        parts["boxes"].append(w["boxes"])
        parts["gt"].append(it["gt"][w["owner"]])
        parts["scale"].append(scale)
    return {k: np.concatenate(v) for k, v in parts.items()}


def refined_iou(data, W, b):
    """(raw IoU, refined IoU) per window of an image_set, to the owning box."""
    out = refine(data["boxes"], predict(data["X"], W, b), 1.0 / data["scale"])
    return iou_rows(data["boxes"], data["gt"]), iou_rows(out, data["gt"])
