#!/usr/bin/env python3
"""Time of multiple-instance pruning's two kernels' calls on the GPU against their NumPy statement on the host
(tests/mip_reference.py), on the same machine and inputs:

  * the prune: a planted trace of `--windows` windows x `--stages` stages (running sums of random float32 increments) in
    `--bags` bags of random membership, resident on the device, recall 0.99: wb_mip_prune_launch alone (the chain of
    2 T + 3 launches, the floor given), calibration.prune_trace (the floor selection, the chain and the two read-backs),
    and ref.bag_floor + ref.prune in NumPy;
  * the windows: the window grids of `--images` 1080p pyramids (shrink 2, 8 levels per octave, window 12 x 12) against
    four boxes per image planted on windows, min_iou 0.7: wb_mip_windows_launch (its memset and one launch per level,
    the ground truth resident), and ref.windows in NumPy;
  * a host clock around each call, the device synchronised before the clock starts and before it stops; `--warmup`
    calls are not counted; median, minimum and maximum of `--runs` calls (the statement: of `--host-runs`).

The results are compared before anything is timed.  Needs a GPU; prints one line per measurement.
    python tools/mip_timing.py [--windows 65536] [--bags 4096] [--stages 128] [--images 8] [--runs 30] [--warmup 5]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import mip_reference as ref  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd import calibration  # noqa: E402
from waldboost_amd.plan import PyramidPlan  # noqa: E402


def timed(f, runs, warmup, sync=True):
    out = []
    for k in range(warmup + runs):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        if sync:
            torch.cuda.synchronize()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    return np.array(out)


def line(what, t):
    print(f"{what}: median {np.median(t) * 1e3:.3f} ms, min {t.min() * 1e3:.3f}, max {t.max() * 1e3:.3f} ({t.size} runs)", flush=True)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--bags", type=int, default=4096)
    ap.add_argument("--stages", type=int, default=128)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    nat.require_gpu()
    lib = nat.load()
    rng = np.random.default_rng(0)

    # ---- the prune
    N, K, T = a.windows, a.bags, a.stages
    tr = np.cumsum(rng.normal(0.1, 1.0, (N, T)).astype(np.float32), axis=1, dtype=np.float32)
    bag = rng.permutation(np.concatenate([np.arange(K), rng.integers(0, K, N - K)])).astype(np.int32)      # every bag has a window
    trace, bag_d = torch.from_numpy(np.ascontiguousarray(tr.T)).cuda(), torch.from_numpy(bag).cuda()
    floor, keep = ref.bag_floor(tr[:, -1], bag, K, 0.99)
    want = ref.prune(tr, bag, K, floor)
    theta, fl, retained, surviving, removed = calibration.prune_trace(trace, bag_d, K, 0.99)
    assert np.array_equal(theta.view(np.uint32), want["theta"].view(np.uint32)) and fl == float(floor)
    assert (retained, surviving) == (want["retained_bags"], want["surviving"]) and np.array_equal(removed.cpu().numpy(), want["removed_at"])
    print(f"prune: {N} windows, {K} bags, {T} stages; keep {keep}, {retained} bags retained, {surviving} windows survive", flush=True)
    g_chain = line("wb_mip_prune_launch (the chain alone)", timed(lambda: calibration.prune_launch(trace, bag_d, K, float(floor)), a.runs, a.warmup))
    g_all = line("prune_trace (floor, chain, two read-backs)", timed(lambda: calibration.prune_trace(trace, bag_d, K, 0.99), a.runs, a.warmup))
    h_pr = line("NumPy statement: floor + prune", timed(lambda: ref.prune(tr, bag, K, ref.bag_floor(tr[:, -1], bag, K, 0.99)[0]),
                                                        a.host_runs, 1, sync=False))
    print(f"prune: x{h_pr / g_all:.1f} against the statement with the floor and the read-backs, x{h_pr / g_chain:.1f} the chain alone", flush=True)

    # ---- the windows
    B, m, n = a.images, 12, 12
    plan = PyramidPlan(1080, 1920, 2, 8, 1)
    levels = [(lv["u"], lv["v"]) for lv in plan.levels]
    inv = np.array([np.float32(1.0 / s) for s in plan.scales], np.float32)
    grid = [ref.window_grid(u, v, m, n) for u, v in levels]
    ok = [l for l, (nr, nc) in enumerate(grid) if nr >= 1 and nc >= 1]
    gts = []
    for b in range(B):
        ls = rng.choice(ok, 4)
        gts.append(np.array([ref.mref.record_boxes(np.array([l]), np.array([rng.integers(0, grid[l][0])]),
                                                   np.array([rng.integers(0, grid[l][1])]), inv, m, n)[0] for l in ls], np.float64))
    ignores = [np.zeros(4, np.uint8)] * B
    table = np.zeros(len(levels), nat.MINE_LEVEL_DTYPE)
    table["u"], table["v"] = [u for u, _ in levels], [v for _, v in levels]
    gt = torch.from_numpy(np.concatenate(gts)).cuda()
    off = torch.from_numpy((4 * np.arange(B + 1)).astype(np.int32)).cuda()
    ign = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
    room = 1 << 16
    rows = torch.empty((room, 8), dtype=torch.int32, device="cuda")
    n_rows = torch.zeros(1, dtype=torch.int32, device="cuda")

    def windows():
        nat.check(lib.wb_mip_windows_launch(nat.stream_ptr(), table.ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p), len(levels),
                                            m, n, nat.ptr(gt), nat.ptr(off), nat.ptr(ign), 4 * B, B, 0.7, nat.ptr(rows), room,
                                            nat.ptr(n_rows)), "wb_mip_windows_launch")

    windows()
    want = ref.windows(levels, inv, m, n, gts, ignores, 0.7)["rows"]
    got = rows[:int(n_rows.item())].cpu().numpy().view(ref.ROW).reshape(-1)
    assert got.size == want.size <= room and ref.mref.ordered(got).tobytes() == want.tobytes()
    total = B * sum(nr * nc for nr, nc in grid)
    print(f"windows: {B} images, {len(ok)} levels with windows, {total} windows, 4 boxes per image, {want.size} acceptable", flush=True)
    g_win = line("wb_mip_windows_launch", timed(windows, a.runs, a.warmup))
    h_win = line("NumPy statement: windows", timed(lambda: ref.windows(levels, inv, m, n, gts, ignores, 0.7), a.host_runs, 1, sync=False))
    print(f"windows: x{h_win / g_win:.0f} against the statement", flush=True)


if __name__ == "__main__":
    main()
