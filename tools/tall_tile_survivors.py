"""How many windows of a cascade tile are left behind phase A (stage 8), per tile, on the benchmark images -- counted with
the CPU oracle: the numbers behind the survivor queue's capacity for 32-row and 64-row tiles.

    python tools/tall_tile_survivors.py [seeds ...]        (default: 0 1 2 3; 1080p synth images, the benchmark model)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import waldboost_amd as wb                                   # noqa: E402
from oracle import wb_oracle as orc                          # noqa: E402
from util import oracle_model                                # noqa: E402
from waldboost_amd.synth import synth_image                  # noqa: E402

PHASE_A = 8


def main():
    seeds = [int(x) for x in sys.argv[1:]] or [0, 1, 2, 3]
    M = wb.load(os.path.join(ROOT, "tests", "golden", "models", "cfg2_d2_T128.pb"))
    shape, opts, trees, thetas = oracle_model(M)
    for rows, caps in ((32, (1024,)), (64, (1024, 1280))):
        counts = []
        for seed in seeds:
            for X, _ in orc.channel_pyramid(synth_image(1080, 1920, seed), opts):
                nr, nc = max(X.shape[0] - shape[0], 0), max(X.shape[1] - shape[1], 0)
                if nr == 0 or nc == 0:
                    continue
                rs, cs, _, _ = orc.cascade_predict_on_image(shape, trees[:PHASE_A], thetas[:PHASE_A], X)
                grid = np.zeros((-(-nr // rows), -(-nc // 64)), np.int64)
                np.add.at(grid, (rs // rows, cs // 64), 1)
                counts.append(grid.reshape(-1))
        c = np.concatenate(counts)
        over = ", ".join(f"more than {cap}: {(c > cap).sum()} ({100.0 * (c > cap).mean():.2f} %)" for cap in caps)
        print(f"{rows}-row tiles: {c.size} over {len(seeds)} images, survivors behind stage {PHASE_A}: mean {c.mean():.0f}, "
              f"median {np.median(c):.0f}, 99th percentile {np.percentile(c, 99):.0f}, max {c.max()}; at most 512: "
              f"{100.0 * (c <= 512).mean():.1f} %; {over}")


if __name__ == "__main__":
    main()
