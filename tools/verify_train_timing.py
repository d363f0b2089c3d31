#!/usr/bin/env python3
"""Times of one training step of the verification CNN (waldboost_amd.verification.Trainer) at (14, 14, 4) and
(32, 32, 16), batches of 64 windows out of a resident pool of 4096 uint8 crops:

  * step: device events around 200 steps of Trainer.run (no host wait inside), milliseconds per step, the minimum and the
    median of `rounds`;
  * torch_autograd: the same step -- the same network in training mode, exploss, Adam -- written with torch.nn.functional
    and torch.optim.Adam on the same GPU, timed the same way: what a user would pay without these kernels.  If torch's
    convolution does not run here, the entry says why instead;
  * kernels (--kernels): the split of the step by kernel, from one separate `rocprofv3 --kernel-trace --stats` run of a child
    process that does nothing but steps (started before this process touches the GPU).

Every timed shape is warmed up first.  Asserts nothing; prints one JSON line.  Needs a GPU.
    python tools/verify_train_timing.py [--steps 200] [--rounds 7] [--kernels] [--no-torch]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((14, 14, 4), (32, 32, 16))
BATCH = 64
POOL = 4096


def pool_of(shape, rng):
    X = rng.integers(0, 256, (POOL,) + shape).astype(np.uint8)
    H = rng.standard_normal(POOL).astype(np.float32)
    Y = np.where(np.arange(POOL) % 2 == 0, -1.0, 1.0).astype(np.float32)
    return X, H, Y


def device_clock(fn, rounds, steps):
    import torch
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return dict(min_ms=min(out), median_ms=float(np.median(out)))


def child(steps):
    """Steps only, for the profiler."""
    import torch
    from waldboost_amd import verification as ver
    rng = np.random.default_rng(0)
    for shape in SHAPES:
        T = ver.Trainer(ver.model_cnn(shape, seed=0), seed=1)
        pool = T.upload(*pool_of(shape, rng))
        T.run(None, None, None, rng.integers(0, POOL, (steps, BATCH)), pool=pool)
        torch.cuda.synchronize()


def kernel_split(steps):
    """{kernel: {calls, total_ms, percent}} of the child's run, or {"error": ...}."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 is not on the PATH"}
    out = tempfile.mkdtemp(prefix="verify_train_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--steps", str(steps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if done.returncode != 0 or not files:
            return {"error": f"rocprofv3 ended with {done.returncode}: {done.stdout[-400:]}"}
        rows = {}
        with open(files[0], newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "vt_" not in name:
                    continue
                short = name[name.index("vt_"):].split("<")[0].split("(")[0]
                e = rows.setdefault(short, dict(calls=0, total_ms=0.0))
                e["calls"] += int(r["Calls"])
                e["total_ms"] += float(r["TotalDurationNs"]) * 1e-6
        whole = sum(e["total_ms"] for e in rows.values()) or 1.0
        for e in rows.values():
            e["percent"] = round(100.0 * e["total_ms"] / whole, 2)
        return rows
    except Exception as err:            # a profiler that cannot run is reported, not fatal
        return {"error": repr(err)}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def torch_step_factory(shape, arrays, X, H, Y, dev):
    """The same step with autograd: returns run(idx) doing idx.shape[0] steps."""
    import torch
    import torch.nn.functional as F
    P = [torch.from_numpy(a.copy()).to(dev) for a in arrays]
    for k in range(4):
        P[6 * k] = P[6 * k].permute(3, 2, 0, 1).contiguous()                 # (ky, kx, in, out) -> (out, in, ky, kx)
    P[26] = P[26].reshape(-1)
    trained = [k for k in range(28) if not (k < 24 and k % 6 >= 4)]
    for k in trained:
        P[k].requires_grad_(True)
    opt = torch.optim.Adam([P[k] for k in trained], lr=1e-4, eps=1e-7)
    Xd = torch.from_numpy(X).to(dev)
    Hd, Yd = torch.from_numpy(H).to(dev), torch.from_numpy(Y).to(dev)

    def run(idx):
        for row in idx:
            x = Xd[row].float().permute(0, 3, 1, 2)
            for k in range(4):
                x = F.conv2d(x, P[6 * k], P[6 * k + 1], padding=1)
                x = F.relu(F.batch_norm(x, P[6 * k + 4], P[6 * k + 5], P[6 * k + 2], P[6 * k + 3], training=True, momentum=0.01,
                                        eps=1e-3))
                if k == 1:
                    x = F.max_pool2d(x, 2)
            x = F.dropout(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1), 0.2)
            x = F.dropout(F.relu(x @ P[24] + P[25]), 0.2)
            p = x @ P[26] + P[27] + Hd[row]
            loss = torch.exp(-Yd[row] * p).clamp(1e-6, 1e3).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="leave the autograd figure out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    result = dict(tool="verify_train_timing", batch=BATCH, pool=POOL, steps=a.steps, rounds=a.rounds, shapes=[])
    if a.kernels:
        result["kernels"] = kernel_split(min(a.steps, 50))
    import torch
    from waldboost_amd import _native as nat
    from waldboost_amd import verification as ver
    dev = nat.require_gpu()
    rng = np.random.default_rng(0)
    for shape in SHAPES:
        X, H, Y = pool_of(shape, rng)
        M = ver.model_cnn(shape, seed=0)
        T = ver.Trainer(M, seed=1)
        pool = T.upload(X, H, Y)
        idx = rng.integers(0, POOL, (a.steps, BATCH))
        idx_dev = T._indices(idx, POOL)
        T._steps(pool, idx_dev[:10])                                 # warm-up
        torch.cuda.synchronize()
        row = dict(shape=list(shape), step=device_clock(lambda: T._steps(pool, idx_dev), a.rounds, a.steps))
        if a.no_torch:
            result["shapes"].append(row)
            continue
        try:
            run = torch_step_factory(shape, M.get_weights(), X, H, Y, dev)
            rows = torch.from_numpy(idx).to(dev)
            run(rows[:10])
            torch.cuda.synchronize()
            row["torch_autograd"] = device_clock(lambda: run(rows), a.rounds, a.steps)
        except Exception as err:        # (no MIOpen kernel for the shape, no convolution at all, ...)
            row["torch_autograd"] = {"error": repr(err)[:300]}
        result["shapes"].append(row)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
