"""The end-to-end scene of the multiple-instance pruning tests (tests/test_mip_host.py proves it is not empty, on the host;
tests/test_gpu_mip.py runs it): the committed models with every theta at -inf, two 120 x 136 images, and ground truth
planted on windows of the pyramid plan -- with every theta at -inf each of them is a detection of the open model.

Image 0: three boxes, the windows (level, r, c) of PLANTED[0].  Image 1: two boxes (PLANTED[1]), an ignored one (a window
too) and one far too large for any level.  No GPU is needed for anything here: the statement's side (the oracle's pyramid
and trees) is computed on the host."""
import functools
import os

import numpy as np

import calib_reference as cref
import mip_reference as ref
import waldboost_amd as wb
from oracle import wb_oracle as orc
from waldboost_amd import channels as _channels
from waldboost_amd.plan import PyramidPlan
from waldboost_amd.synth import synth_image
from util import GOLDEN, oracle_model

CASES = {"f32": "mixed_d2_T24.pb", "u8": "grad_hist_4_u1_d2_T24.pb"}
H, W = 120, 136
SEEDS = (11, 12)
MIN_IOU = 0.7


def open_model(tag):
    """The committed model with every theta at -inf."""
    M = wb.load(os.path.join(GOLDEN, CASES[tag]))
    M.theta = [float("-inf")] * len(M)
    return M


def window_box(inv_scale, l, r, c, m, n):
    return ref.mref.record_boxes(np.array([l]), np.array([r]), np.array([c]), inv_scale, m, n)[0]


@functools.lru_cache(None)
def scene(tag):
    """dict(images [2, H, W] uint8, levels [(u, v)], inv_scale, planted: per image the windows (level, r, c) of its boxes,
    gts: per image float64 [G, 4], ignores: per image uint8 [G], boxes: per image a wb.Boxes with the 'ignore' field)."""
    M = open_model(tag)
    m, n, _ = M.shape
    shrink, n_per_oct, smooth, _ = _channels.read_opts(M.channel_opts)
    plan = PyramidPlan(H, W, shrink, n_per_oct, smooth)
    levels = [(lv["u"], lv["v"]) for lv in plan.levels]
    inv_scale = np.array([np.float32(1.0 / s) for s in plan.scales], np.float32)
    grid = [ref.window_grid(u, v, m, n) for u, v in levels]
    ok = [l for l, (nr, nc) in enumerate(grid) if nr >= 3 and nc >= 3]
    assert len(ok) >= 4, "the plan has too few levels with windows for this scene"
    at = lambda l, fr, fc: (l, int((grid[l][0] - 1) * fr), int((grid[l][1] - 1) * fc))
    planted = [[at(ok[0], 1 / 3, 1 / 4), at(ok[len(ok) // 2], 1 / 2, 1 / 2), at(ok[-1], 1.0, 1.0)],
               [at(ok[1], 0.0, 0.0), at(ok[len(ok) // 3], 1 / 2, 1 / 3), at(ok[2], 1 / 2, 3 / 4)]]          # the last one: ignored
    gts, ignores, boxes = [], [], []
    for b, ws in enumerate(planted):
        g = [window_box(inv_scale, l, r, c, m, n) for l, r, c in ws]
        ign = [0] * len(g)
        if b == 1:
            ign[-1] = 1
            g.append(np.array([-2 * W, -2 * H, 3 * W, 3 * H], np.float32))      # too large for any level: unreachable
            ign.append(0)
        gts.append(np.array(g, np.float64))
        ignores.append(np.array(ign, np.uint8))
        bx = wb.Boxes(np.array(g, np.float32))
        bx.set_field("ignore", np.array(ign))
        boxes.append(bx)
    images = np.stack([synth_image(H, W, s) for s in SEEDS])
    return dict(images=images, levels=levels, inv_scale=inv_scale, planted=planted, gts=gts, ignores=ignores, boxes=boxes, shape=(m, n))


@functools.lru_cache(None)
def statement(tag):
    """The statement on the oracle's pyramid and trees: dict(rows, bag, reachable, unreachable, trace (N, T), crops, level0)."""
    s = scene(tag)
    M = open_model(tag)
    m, n = s["shape"]
    win = ref.windows(s["levels"], s["inv_scale"], m, n, s["gts"], s["ignores"], MIN_IOU)
    rows = win["rows"]
    shape, opts, trees, _ = oracle_model(M)
    pyramids = [[chns for chns, _ in orc.channel_pyramid(img, opts)] for img in s["images"]]
    assert [p.shape[:2] for p in pyramids[0]] == s["levels"]
    crops = np.stack([pyramids[w["image"]][w["level"]][w["r"]:w["r"] + m, w["c"]:w["c"] + n] for w in rows])
    # bags over the whole scene: the reachable boxes in (image, index) order
    bag = ref.bags_of(rows, win["reachable"])
    return dict(rows=rows, bag=bag, reachable=win["reachable"], unreachable=win["unreachable"], trace=cref.trace(trees, crops), crops=crops,
                level0=pyramids[0][0])


def level0(tag):
    """The first pyramid level of image 0 (the oracle's), for random crops."""
    return statement(tag)["level0"]


def pruned(tag, recall, margin=0.0):
    """The statement's prune of the scene at `recall`: ref.prune's dict with floor and keep added."""
    st = statement(tag)
    n_bags = len(st["reachable"])
    floor, keep = ref.bag_floor(st["trace"][:, -1], st["bag"], n_bags, recall)
    out = ref.prune(st["trace"], st["bag"], n_bags, floor, margin)
    out.update(floor=floor, keep=keep, n_bags=n_bags)
    return out
