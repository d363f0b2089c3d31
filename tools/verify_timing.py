#!/usr/bin/env python3
"""Times of the verification CNN (waldboost_amd.verification) for windows of (14, 14, 4), at about 1 000 and 20 000 windows:

  * predict_resident: Verifier.predict_device on crops and scores that are on the device already -- device events around
    `reps` calls (two launches each);
  * predict_host: Verifier.predict as a caller with host arrays sees it: upload, the launches, the read-back -- a host clock
    around the call, which ends in the read-back's synchronise;
  * crops_to_host: what a user pays today before another framework can start: the same crops, resident, copied to the host
    (`.cpu()` only) -- a host clock;
  * detect_and_verify: the whole call on an image whose pyramid holds about that many windows, scanned by a one-stage
    cascade that accepts every window (so the number of detections is the number of windows) -- a host clock; and
    detect alone on the same image, for the difference.

Every timed shape is warmed up first; each figure is the minimum and the median over `rounds`.  Asserts nothing; prints one
JSON line.  Needs a GPU.
    python tools/verify_timing.py [--reps 20] [--rounds 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import waldboost_amd as wb  # noqa: E402
from waldboost_amd import _native as nat  # noqa: E402
from waldboost_amd import verification as ver  # noqa: E402
from waldboost_amd.synth import synth_image  # noqa: E402

SHAPE = (14, 14, 4)


def host_clock(fn, rounds):
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return dict(min_ms=min(times) * 1e3, median_ms=float(np.median(times)) * 1e3)


def device_clock(fn, reps, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return dict(min_ms=min(out), median_ms=float(np.median(out)))


def accept_all_model():
    """One stage of a trained cascade on a (14, 14, 4) window, rejection threshold -inf: every window is a detection."""
    trained = wb.load(os.path.join(ROOT, "tests", "golden", "mixed_d2_T24.pb"))
    M = wb.Model(SHAPE, trained.channel_opts)
    M.append(trained.classifier[0], -np.inf)
    return M


def image_with_windows(M, target):
    """A 4:3 synthetic image whose pyramid holds about `target` windows (bisection on the height)."""
    lo, hi = 32, 1200
    while hi - lo > 4:
        mid = (lo + hi) // 2
        if len(M.detect(synth_image(mid, mid * 4 // 3, 1))) < target:
            lo = mid
        else:
            hi = mid
    return synth_image(hi, hi * 4 // 3, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = nat.require_gpu()
    V = ver.model_cnn(SHAPE, seed=0)
    M = accept_all_model()
    rng = np.random.default_rng(0)
    result = dict(tool="verify_timing", shape=list(SHAPE), reps=a.reps, rounds=a.rounds, sizes=[])
    for N in (1000, 20000):
        X = rng.standard_normal((N,) + SHAPE).astype(np.float32)
        H = rng.standard_normal(N).astype(np.float32)
        Xd, Hd = torch.from_numpy(X).to(dev), torch.from_numpy(H).to(dev)
        for _ in range(3):                                   # warm-up of every timed shape
            V.predict_device([Xd, Hd])
            V.predict([X, H])
            Xd.cpu()
        torch.cuda.synchronize()
        row = dict(n_windows=N,
                   predict_resident=device_clock(lambda: V.predict_device([Xd, Hd]), a.reps, a.rounds),
                   predict_host=host_clock(lambda: V.predict([X, H]), a.rounds),
                   crops_to_host=host_clock(lambda: Xd.cpu(), a.rounds))
        row["multiply_adds"] = N * sum(p * 9 * ci * co for p, ci, co in ((196, 4, 8), (196, 8, 8), (49, 8, 16), (49, 16, 16))) \
            + N * (784 * 128 + 128)
        img = image_with_windows(M, N)
        for _ in range(3):
            bbs, scores = ver.detect_and_verify(img, M, V)
            M.detect(img)
        row["image"] = list(img.shape)
        row["detections"] = int(len(scores))
        row["detect_and_verify"] = host_clock(lambda: ver.detect_and_verify(img, M, V), a.rounds)
        row["detect_alone"] = host_clock(lambda: M.detect(img), a.rounds)
        result["sizes"].append(row)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
