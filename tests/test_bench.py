"""bench.py: a plain run's line (exactly --steps timed steps, nothing of --full) and --dump-outputs, whose arrays are what
the last timed step computed -- compared with the oracle for that step's image (GPU); the output writer's float dtypes,
its 64 MB bound and its fixed sample (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from waldboost_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(n, seed=0):
    rng = np.random.default_rng(seed)
    d = np.zeros(n, nat.DET_DTYPE)
    d["image"] = rng.integers(0, 4, n)
    d["level"] = rng.integers(0, 64, n)
    d["r"] = rng.integers(0, 500, n)
    d["c"] = rng.integers(0, 900, n)
    d["score"] = rng.standard_normal(n).astype(np.float32)
    return d


def test_write_outputs_keeps_everything_under_the_bound(tmp_path):
    d = _records(3000)
    alive = np.random.default_rng(1).integers(0, 3_000_000, (2, 64, 128)).astype(np.int32)
    out = bench.write_outputs(str(tmp_path), d, alive)
    assert sorted(out) == ["alive", "det_c", "det_image", "det_level", "det_r", "det_score"]
    for name, a in out.items():
        back = np.load(tmp_path / f"{name}.npy")
        assert back.dtype in (np.float32, np.float64) and np.array_equal(back, a)
    assert np.array_equal(out["alive"], alive) and out["alive"].dtype == np.float64
    for k in ("image", "level", "r", "c"):
        assert np.array_equal(out[f"det_{k}"], d[k])
    assert np.array_equal(out["det_score"].view(np.uint32), d["score"].view(np.uint32))


def test_write_outputs_samples_past_the_bound_the_same_way_every_time(tmp_path):
    d = _records(50_000, seed=2)
    alive = np.arange(16 * 64 * 128, dtype=np.int32).reshape(16, 64, 128)
    limit = 400_000                                  # alive as float64: 1 MB > limit / 2; the records: 1.8 MB
    a = bench.write_outputs(str(tmp_path / "a"), d, alive, limit=limit)
    b = bench.write_outputs(str(tmp_path / "b"), d, alive, limit=limit)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= limit
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit + 1024 * len(a)
    imgs, rows = a["alive_images"].astype(np.int64), a["det_rows"].astype(np.int64)
    assert 0 < imgs.size < 16 and np.all(np.diff(imgs) > 0) and np.array_equal(a["alive"], alive[imgs])
    assert 0 < rows.size < d.size and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["det_level"], d["level"][rows]) and np.array_equal(a["det_score"], d["score"][rows])


def test_dump_outputs_needs_a_whole_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--only", "channels", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--only all" in r.stderr


@pytest.mark.gpu
def test_plain_run_line_and_the_last_steps_outputs_vs_oracle(tmp_path):
    """A plain run times exactly --steps steps and carries nothing of --full; what it dumps is the last timed step's work:
    with a pool of 4 single-image engines, step 3 of 3 ran engine 2, whose image is seed 2."""
    import waldboost_amd as wb
    from util import oracle_detect
    from waldboost_amd.synth import synth_image
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout
    out = json.loads(r.stdout)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value_spread"]["repeats"] == 1
    assert out["unit"] == "windows/s" and out["higher_is_better"] is True and out["dtype"] and out["metric"]
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert not out["config"]["full"]
    for k in ("parity", "kernels", "roofline", "through_api", "cpu_baseline", "config3"):
        assert not out[k], k
    M = wb.load(bench.MODELS["grad_hist"])
    ref = oracle_detect(M, synth_image(1080, 1920, 2))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["alive", "det_c", "det_image", "det_level", "det_r", "det_score"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.all(got["det_image"] == 0)
    assert np.array_equal(got["det_level"], ref["level"]) and np.array_equal(got["det_r"], ref["r"])
    assert np.array_equal(got["det_c"], ref["c"])
    assert np.array_equal(got["det_score"].view(np.uint32), ref["scores"].view(np.uint32))
    assert np.array_equal(got["alive"][0], ref["alive"])
