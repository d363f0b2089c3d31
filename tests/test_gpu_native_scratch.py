"""The shared grow-only scratch (nat.Scratch) under the two callers that keep one across calls: a Verifier predicting in
chunks of changing size and a Trainer stepping on batches of changing size.  A buffer that is larger than a call needs,
and holds what another call left in it, must not change a bit of the result."""
import numpy as np
import pytest
import torch

from waldboost_amd import verification as ver

pytestmark = pytest.mark.gpu

SHAPE = (5, 6, 3)


def _windows(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n,) + SHAPE).astype(np.float32), rng.normal(size=n).astype(np.float32)


def test_predict_reuses_one_scratch_across_chunk_sizes():
    X, H = _windows(70, 5)
    Xd, Hd = torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda()
    fresh = ver.model_cnn(SHAPE, seed=1).predict_device([Xd, Hd]).cpu().numpy()
    assert fresh.shape == (70, 1) and np.isfinite(fresh).all()
    V = ver.model_cnn(SHAPE, seed=1)
    held = []
    for batch_size in (64, None, 8):
        got = V.predict_device([Xd, Hd], batch_size=batch_size).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32)), batch_size
        held.append(V._scratch.on(Xd.device, 0))
    assert held[1].numel() >= held[0].numel()      # 64, then all 70 windows per launch: it may grow
    assert held[2] is held[1]                      # 8 per launch fit into what is there


def test_train_steps_reuse_one_scratch_across_batch_sizes():
    X, H = _windows(6, 7)
    Y = np.array([1, -1, 1, -1, 1, -1], np.float32)

    def step(trainer, B):
        return np.float32(trainer.train_on_batch(X[:B], H[:B], Y[:B]))

    def fresh():
        return ver.Trainer(ver.model_cnn(SHAPE, seed=1), seed=3)

    one = fresh()
    first, second = step(one, 6), step(one, 4)
    big = one._scratch.on(one.device, 0)
    # the second step alone, from the state the first one left, in a scratch of its own size
    a = fresh()
    assert step(a, 6).view(np.uint32) == first.view(np.uint32)
    b = fresh()
    for name in ("params", "adam_m", "adam_v", "t"):
        getattr(b, name).copy_(getattr(a, name))
    assert b._scratch.on(b.device, 0).numel() == 16            # nothing held yet: B = 4 allocates what B = 4 needs
    assert step(b, 4).view(np.uint32) == second.view(np.uint32)
    assert b._scratch.on(b.device, 0).numel() < big.numel()
    assert one._scratch.on(one.device, 0) is big               # B = 4 after B = 6 kept the larger buffer
    assert np.isfinite(first) and np.isfinite(second)
