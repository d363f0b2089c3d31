"""wb_verify_train_step, Trainer and train on the GPU against the NumPy statement of the step (tests/verify_train_reference.py).

The rule of every comparison with the statement: per array, max|gpu - s64| <= 8 * max(err32, 2^-20 * max|s64|), where s64 is
the float64 statement and err32 = max|s32 - s64| the error of the same statement evaluated in float32, computed in the same
test.  8 is headroom for another accumulation order of the same length; the floor 2^-20 of an array's maximum is what a
float32 evaluation of this network costs.  Each test prints its largest ratio.

The parameters after the update are compared where |g64| exceeds the gradient's bound (below it the sign of a gradient, and
with it Adam's first step of size lr, is not determined) and where g64 is exactly zero (dropout and ReLU zero most of the
dense kernel's gradient at these batch sizes: there the step must be exactly zero too); at most 5 % of the parameters may
be left out, which depends on the statement alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import verify_reference as ref
import verify_train_designs as designs
import verify_train_reference as tr
from verify_train_designs import random_arrays
from waldboost_amd import _native as nat
from waldboost_amd import verification as ver

pytestmark = pytest.mark.gpu

GUARD = 64                              # guard words on either side of every buffer the step writes
SENTINEL = np.float32(-7.25e33)
FACTOR = 8.0
FLOOR = 2.0 ** -20


def split(flat, shape):
    out, at = [], 0
    for s in ver._expected_shapes(shape):
        size = int(np.prod(s))
        out.append(flat[at:at + size].reshape(s).copy())
        at += size
    assert at == flat.size
    return out


class Device:
    """One training state at the C ABI, every written buffer between guard words."""

    def __init__(self, shape, arrays, X, H, Y, B, dropout=0.2, seed=3, lr=1e-4, scratch_fill=0):
        self.lib, self.dev, self.shape, self.B = nat.load(), nat.require_gpu(), shape, B
        flat = tr.flatten(arrays).astype(np.float32)
        self.params, self.m, self.v = self._guarded(flat), self._guarded(np.zeros_like(flat)), self._guarded(np.zeros_like(flat))
        self.grads, self.loss = self._guarded(np.zeros_like(flat)), self._guarded(np.zeros(1, "f"))
        self.t = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.X = torch.from_numpy(np.ascontiguousarray(X)).to(self.dev)
        self.code = nat.WB_DTYPE_U8 if X.dtype == np.uint8 else nat.WB_DTYPE_F32
        self.H, self.Y = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(self.dev) for v in (H, Y))
        need = C.c_size_t()
        nat.check(self.lib.wb_verify_train_scratch_bytes(*shape, B, C.byref(need)), "scratch_bytes")
        self.scratch = torch.full((need.value,), scratch_fill, dtype=torch.uint8, device=self.dev)
        self.hyper = nat.WbVerifyTrainHyper(lr=lr, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99, bn_epsilon=1e-3,
                                            dropout=dropout, seed=seed, reserved=0)

    def _guarded(self, values):
        buf = torch.full((values.size + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device=self.dev)
        buf[GUARD:GUARD + values.size] = torch.from_numpy(values).to(self.dev)
        return buf

    def _inner(self, buf):
        host = buf.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), "a guard word was written"
        return host[GUARD:-GUARD].copy()

    def step(self, idx, with_grads=True):
        """One step on the windows idx (B,); returns what the step left, as host arrays."""
        assert idx.shape == (self.B,)
        padded = torch.full((self.B + GUARD,), 2 ** 30, dtype=torch.int32, device=self.dev)      # (nothing behind idx[B - 1] is read)
        padded[:self.B] = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(self.dev)
        m, n, Cc = self.shape
        p = lambda buf: nat.ptr(buf[GUARD:])
        nat.check(self.lib.wb_verify_train_step(nat.stream_ptr(), nat.ptr(self.X), self.code, nat.ptr(self.H), nat.ptr(self.Y),
                                                int(self.X.shape[0]), nat.ptr(padded), self.B, m, n, Cc, p(self.params), p(self.m),
                                                p(self.v), nat.ptr(self.t), C.byref(self.hyper), nat.ptr(self.scratch),
                                                self.scratch.numel(), p(self.loss), p(self.grads) if with_grads else None),
                  "wb_verify_train_step")
        torch.cuda.synchronize()
        t = self.t.cpu().numpy()
        assert t[1] == 0
        flat = {k: self._inner(getattr(self, k)) for k in ("params", "m", "v", "grads")}
        return {"loss": self._inner(self.loss)[0], "t": int(t[0]), "flat": flat,
                **{k: split(v, self.shape) for k, v in flat.items()}}


def pool_for(shape, n_pool, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        X = rng.integers(0, 256, (n_pool,) + shape).astype(np.uint8)
    else:
        X = rng.standard_normal((n_pool,) + shape).astype(np.float32)
    H = (rng.standard_normal(n_pool) * 0.5).astype(np.float32)
    Y = rng.choice([-1.0, 1.0], n_pool).astype(np.float32)
    return X, H, Y


def statement(arrays, X, H, Y, idx, dtype, dropout=0.2, seed=3, lr=1e-4, steps_before=0):
    state = tr.new_state(arrays, dtype)
    state["t"] = steps_before
    out = tr.train_step(state, X[idx].astype(np.float32), H[idx], Y[idx], dtype, seed=seed, dropout=dropout, lr=lr)
    return out, state


def held(gpu, s64, s32):
    """(largest difference, the rule's unit) of one array.  An array that is zero in both statements has the smallest
    positive unit: the GPU's must be zero too."""
    s64 = np.asarray(s64, np.float64)
    unit = max(np.abs(np.asarray(s32, np.float64) - s64).max(), FLOOR * np.abs(s64).max(), np.finfo(np.float64).tiny)
    return np.abs(np.asarray(gpu, np.float64).reshape(s64.shape) - s64).max(), unit


def check_step(got, arrays, o64, st64, o32, st32, label):
    """The one-step rule on the loss, every gradient, the moving statistics and the parameters after the update."""
    diff, unit = held(got["loss"], o64["loss"], o32["loss"])
    report = [("loss", diff / unit)]
    assert diff <= FACTOR * unit, (label, "loss", diff, unit)
    left_out = total = 0
    for k in range(28):
        if tr.is_conv_bias(k):
            assert not got["grads"][k].any() and np.array_equal(got["params"][k], arrays[k]), (label, k)
            assert not got["m"][k].any() and not got["v"][k].any()
            continue
        diff, unit = held(got["grads"][k], o64["grads"][k], o32["grads"][k])
        report.append((f"g{k}", diff / unit))
        assert diff <= FACTOR * unit, (label, "gradient", k, diff, unit)
        g64 = np.asarray(o64["grads"][k], np.float64).reshape(arrays[k].shape)
        compared = np.ones(arrays[k].shape, bool) if tr.is_moving(k) else (np.abs(g64) > FACTOR * unit) | (g64 == 0)
        left_out += compared.size - compared.sum()
        total += compared.size
        if compared.any():
            p64, p32 = st64["params"][k][compared], st32["params"][k][compared]
            diff, unit = held(got["params"][k][compared], p64, p32)
            report.append((f"p{k}", diff / unit))
            assert diff <= FACTOR * unit, (label, "parameter", k, diff, unit)
    worst = max(r for _, r in report)
    print(f"{label}: largest ratio {worst:.3f} ({max(report, key=lambda x: x[1])[0]}), {left_out} of {total} parameters left out")
    assert left_out <= 0.05 * total, (label, left_out, total)
    assert got["t"] == st64["t"]
    return worst


CASES = [((2, 2, 1), 2), ((3, 5, 2), 4), ((5, 6, 3), 6), ((14, 14, 4), 64), ((13, 32, 9), 8), ((32, 32, 16), 4)]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,B", CASES, ids=str)
def test_one_step_against_the_statement(shape, B, dtype):
    arrays = random_arrays(shape, 20 + shape[0])
    X, H, Y = pool_for(shape, B + 3, dtype, 30 + shape[1])
    rng = np.random.default_rng(B)
    idx = rng.integers(0, B + 3, B)
    if B > 2:
        idx[1] = idx[0]                                                 # a duplicate: it counts twice
    else:
        idx = rng.permutation(B + 3)[:B]                                # (two copies of one window: no variance, every gradient 0)
    o64, st64 = statement(arrays, X, H, Y, idx, np.float64)
    o32, st32 = statement(arrays, X, H, Y, idx, np.float32)
    got = Device(shape, arrays, X, H, Y, B).step(idx)
    check_step(got, arrays, o64, st64, o32, st32, f"{shape} B={B} {np.dtype(dtype).name}")


def test_a_saturated_batch_moves_nothing_but_the_moving_statistics():
    shape, B = (5, 6, 3), 6
    arrays = random_arrays(shape, 4)
    X, _, Y = pool_for(shape, B, np.float32, 5)
    H = (Y * np.array([50, -50, 40, -30, 60, 20])).astype("f")
    dev = Device(shape, arrays, X, H, Y, B)
    got = dev.step(np.arange(B))
    want = float(np.mean(tr.forward_backward(arrays, X, H, Y, np.float32, tr.dropout_masks(3, 0, B, 96, 0.2), 1.25)["losses"]))
    assert abs(got["loss"] - want) <= 1e-6 * want
    moved = 0
    for k in range(28):
        if tr.is_moving(k):
            moved += not np.array_equal(got["params"][k], arrays[k])
            continue
        assert np.array_equal(got["params"][k].view(np.uint32), arrays[k].view(np.uint32)), k
        assert not got["grads"][k].any()
    assert moved == 8 and got["t"] == 1
    assert not got["flat"]["m"].any() and not got["flat"]["v"].any()
    assert not np.signbit(got["flat"]["m"]).any() and not np.signbit(got["flat"]["v"]).any()


def same_bits(a, b):
    return a["loss"].view(np.uint32) == b["loss"].view(np.uint32) and a["t"] == b["t"] and all(
        np.array_equal(a["flat"][k].view(np.uint32), b["flat"][k].view(np.uint32)) for k in a["flat"])


def test_no_dropout_is_the_all_keep_mask_and_the_scratch_needs_no_clearing():
    shape, B = (5, 6, 3), 6
    arrays = random_arrays(shape, 6)
    X, H, Y = pool_for(shape, B + 2, np.uint8, 7)
    idx = np.array([7, 0, 3, 3, 1, 6])
    off = Device(shape, arrays, X, H, Y, B, dropout=0.0).step(idx)
    # a rate whose threshold round(rate * 2^32) is 0 and whose scale rounds to 1: every element kept, through the generator
    keep = Device(shape, arrays, X, H, Y, B, dropout=1e-12).step(idx)
    assert tr.drop_threshold(1e-12) == 0 and tr.dropout_scale(1e-12) == 1.0
    assert same_bits(off, keep)
    o64, st64 = statement(arrays, X, H, Y, idx, np.float64, dropout=0.0)
    o32, st32 = statement(arrays, X, H, Y, idx, np.float32, dropout=0.0)
    check_step(off, arrays, o64, st64, o32, st32, "no dropout")
    rows = (idx, idx[::-1].copy())
    dirty = Device(shape, arrays, X, H, Y, B, scratch_fill=0xFF)
    clean = Device(shape, arrays, X, H, Y, B, scratch_fill=0)
    for row in rows:
        a, b = dirty.step(row), clean.step(row)
        assert same_bits(a, b)
    # grads_out is optional: the same two steps without it
    quiet = Device(shape, arrays, X, H, Y, B)
    for row in rows:
        last = quiet.step(row, with_grads=False)
    assert not last["flat"]["grads"].any() and last["loss"] == b["loss"] and last["t"] == 2
    assert all(np.array_equal(last["flat"][k].view(np.uint32), b["flat"][k].view(np.uint32)) for k in ("params", "m", "v"))


def test_three_steps_twice_give_the_same_bits():
    shape, B = (14, 14, 4), 64
    arrays = random_arrays(shape, 9)
    X, H, Y = pool_for(shape, 100, np.uint8, 10)
    rows = np.random.default_rng(1).integers(0, 100, (3, B))
    runs = []
    for _ in range(2):
        dev = Device(shape, arrays, X, H, Y, B)
        runs.append([dev.step(row) for row in rows])
    for a, b in zip(*runs):
        assert same_bits(a, b)
    assert runs[0][2]["t"] == 3 and not same_bits(runs[0][0], runs[0][1])
    # the masks follow the step: the second step from a fresh state with t = 1 in the statement
    st = tr.new_state(arrays, np.float64)
    for k, row in enumerate(rows[:2]):
        o64 = tr.train_step(st, X[row].astype("f"), H[row], Y[row], np.float64, seed=3, dropout=0.2)
        assert abs(runs[0][k]["loss"] - o64["loss"]) <= 1e-4 * o64["loss"]


@pytest.mark.parametrize("B", [2, 62, 64, 66])
@pytest.mark.parametrize("slot", ["first", "last"])
def test_one_live_window_at_either_end_of_the_batch(B, slot):
    shape = (14, 14, 4)
    arrays = random_arrays(shape, 13)
    X, H, Y = pool_for(shape, B, np.float32, 14)
    live = 0 if slot == "first" else B - 1
    H = (Y * 60).astype("f")                    # every window saturated (e = exp(-60 +- cnn): outside (1e-6, 1e3)) ...
    H[live] = 0.1                               # ... but one
    idx = np.arange(B)
    o64, st64 = statement(arrays, X, H, Y, idx, np.float64)
    o32, st32 = statement(arrays, X, H, Y, idx, np.float32)
    inside = (o64["losses"] > 1e-6) & (o64["losses"] < 1e3)
    assert inside[live] and inside.sum() == 1
    got = Device(shape, arrays, X, H, Y, B).step(idx)
    assert got["grads"][24].any() and got["grads"][0].any()
    check_step(got, arrays, o64, st64, o32, st32, f"B={B}, live window {live}")


# ---- Trainer and train, end to end on the planted pool
@pytest.fixture(scope="module")
def planted():
    X0, H0, X1, H1 = designs.planted_pool()
    M = designs.planted_model()
    start = M.get_weights()
    means = ver.train(M, X0, H0, X1, H1, epochs=4, batch_size=designs.PLANTED_BATCH, steps=50, lr=designs.PLANTED_LR,
                      seed=designs.PLANTED_SEED, verbose=False)
    return {"pool": (X0, H0, X1, H1), "M": M, "start": start, "means": means}


def manual_run(pool, chunks, steps=50):
    """The same training by hand: one Trainer, the epochs' batches as train draws them, run in `chunks` pieces per epoch."""
    X0, H0, X1, H1 = pool
    M = designs.planted_model()
    T = ver.Trainer(M, lr=designs.PLANTED_LR, seed=designs.PLANTED_SEED)
    X, H = np.concatenate([X0, X1]), np.concatenate([H0, H1])
    Y = np.concatenate([-np.ones(len(X0), "f"), np.ones(len(X1), "f")])
    rng = np.random.default_rng(designs.PLANTED_SEED)
    losses = []
    for _ in range(4):
        idx = ver._draw_epoch(rng, len(X0), len(X1), steps, designs.PLANTED_BATCH // 2)
        for part in np.array_split(idx, chunks):
            losses.append(T.run(X, H, Y, part).cpu().numpy())
    return M, T, np.concatenate(losses)


def test_train_learns_the_planted_difference(planted):
    means = planted["means"]
    print("epoch means on the GPU:", means)
    assert len(means) == 4 and means[-1] < 0.5 * means[0]
    changed = [not np.array_equal(a, b) for a, b in zip(planted["M"].get_weights(), planted["start"])]
    assert all(changed[k] != tr.is_conv_bias(k) for k in range(28))
    # the first three step losses against the statement, by the one-step rule
    M, T, losses = manual_run(planted["pool"], 1)
    _, s64 = designs.planted_statement_run(1, 50, np.float64, max_steps=3)
    _, s32 = designs.planted_statement_run(1, 50, np.float32, max_steps=3)
    for k in range(3):
        diff, unit = held(losses[k], s64[k], s32[k])
        print(f"step {k}: gpu {losses[k]:.9g}, float64 {s64[k]:.9g}, float32 {s32[k]:.9g}, ratio {diff / unit:.3f}")
        assert diff <= FACTOR * unit
    # train is this loop: the same means, and after commit the same weights
    assert T.steps_done == 200
    assert [float(losses[50 * e:50 * e + 50].astype(np.float64).mean()) for e in range(4)] == means
    T.commit()
    assert all(np.array_equal(a, b) for a, b in zip(M.get_weights(), planted["M"].get_weights()))


def test_train_prints_what_the_reference_prints(planted, capsys):
    small = designs.planted_model()
    X0, H0, X1, H1 = planted["pool"]
    got = ver.train(small, X0, H0, X1, H1, epochs=2, batch_size=16, steps=2, seed=1)
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "Epoch 1/2" and float(out[1]) == got[0] and out[2] == "Epoch 2/2" and out[4] == "Done"


def test_predict_after_train_is_the_inference_contract_on_the_new_weights(planted):
    M = planted["M"]
    X0, H0, X1, H1 = planted["pool"]
    X, H = np.concatenate([X0[:20], X1[:20]]), np.concatenate([H0[:20], H1[:20]])
    stale = designs.planted_model()
    before = stale.predict([X, H])                       # (fills the device cache that set_weights must drop)
    stale.set_weights(M.get_weights())
    want = ref.predict(M.get_weights(), M.epsilon, X, H)
    for V in (M, stale):
        got = V.predict([X, H])[:, 0]
        assert np.array_equal(got, want)
    assert not np.array_equal(before[:, 0], want)


def test_continuing_a_trainer_equals_one_longer_run(planted):
    whole_M, whole_T, whole = manual_run(planted["pool"], 1)
    parts_M, parts_T, parts = manual_run(planted["pool"], 3)
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    for name in ("params", "adam_m", "adam_v", "t"):
        assert torch.equal(getattr(whole_T, name), getattr(parts_T, name)), name
    # device tensors and float32 crops take the same path as host uint8 ones
    X0, H0, X1, H1 = planted["pool"]
    M = designs.planted_model()
    dev = nat.require_gpu()
    means = ver.train(M, torch.from_numpy(X0).to(dev), H0, torch.from_numpy(X1).to(dev), H1, epochs=4, batch_size=16, steps=50,
                      lr=designs.PLANTED_LR, seed=designs.PLANTED_SEED, verbose=False)
    assert means == planted["means"]
    loss = ver.Trainer(designs.planted_model(), seed=1).train_on_batch(X0[:8].astype(np.float32), H0[:8], -np.ones(8, "f"))
    assert np.isfinite(loss) and loss > 0
    with pytest.raises(ValueError):
        whole_T.run(X0, H0, -np.ones(len(X0), "f"), np.full((1, 16), len(X0)))       # an index outside the pool
    with pytest.raises(NotImplementedError):
        whole_T.run(X0, H0, -np.ones(len(X0), "f"), np.zeros((1, 3), np.int64))
