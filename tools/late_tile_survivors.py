"""How many windows of a 64-row cascade tile are still alive on entering stage 32, per tile, on the benchmark images --
counted with the CPU oracle: how many windows a tile's waves bring to the stage-parallel tail between them (DESIGN
section 4.4, round 19; profiles/r19/late_tile_survivors.txt).

    python tools/late_tile_survivors.py [seeds ...]        (default: 0 1 2 3; 1080p synth images, the benchmark model)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import waldboost_amd as wb                                   # noqa: E402
from oracle import wb_oracle as orc                          # noqa: E402
from util import oracle_model                                # noqa: E402
from waldboost_amd.synth import synth_image                  # noqa: E402

LATE = 32
ROWS = 64


def main():
    seeds = [int(x) for x in sys.argv[1:]] or [0, 1, 2, 3]
    M = wb.load(os.path.join(ROOT, "tests", "golden", "models", "cfg2_d2_T128.pb"))
    shape, opts, trees, thetas = oracle_model(M)
    counts = []
    for seed in seeds:
        for X, _ in orc.channel_pyramid(synth_image(1080, 1920, seed), opts):
            nr, nc = max(X.shape[0] - shape[0], 0), max(X.shape[1] - shape[1], 0)
            if nr == 0 or nc == 0:
                continue
            rs, cs, _, _ = orc.cascade_predict_on_image(shape, trees[:LATE], thetas[:LATE], X)
            grid = np.zeros((-(-nr // ROWS), -(-nc // 64)), np.int64)
            np.add.at(grid, (rs // ROWS, cs // 64), 1)
            counts.append(grid.reshape(-1))
    c = np.concatenate(counts)
    print(f"{ROWS}-row tiles: {c.size} over {len(seeds)} images; windows alive on entering stage {LATE}: total {c.sum()}, "
          f"mean {c.mean():.2f}, median {np.median(c):.0f}, 99th percentile {np.percentile(c, 99):.0f}, max {c.max()}")
    print("windows  tiles  share  cumulative")
    hist = np.bincount(c)
    cum = 0.0
    for k, n in enumerate(hist):
        if n:
            cum += n / c.size
            print(f"{k:7d} {n:6d} {100.0 * n / c.size:6.2f} {100.0 * cum:7.2f}")
    for cap in (12, 16, 20, 24, 32):
        print(f"more than {cap}: {(c > cap).sum()} tiles ({100.0 * (c > cap).mean():.2f} %)")


if __name__ == "__main__":
    main()
