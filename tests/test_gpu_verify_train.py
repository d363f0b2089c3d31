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
from verify_train_designs import FACTOR, held, pool_for, random_arrays, statement
from waldboost_amd import _native as nat
from waldboost_amd import verification as ver

pytestmark = pytest.mark.gpu

GUARD = 64                              # guard words on either side of every buffer the step writes
SENTINEL = np.float32(-7.25e33)


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

    def __init__(self, shape, arrays, X, H, Y, B, dropout=0.2, seed=3, lr=1e-4, scratch_fill=0, beta1=0.9, beta2=0.999,
                 adam_epsilon=1e-7, momentum=0.99, bn_epsilon=1e-3, m=None, v=None, steps_before=0):
        self.lib, self.dev, self.shape, self.B = nat.load(), nat.require_gpu(), shape, B
        flat = tr.flatten(arrays).astype(np.float32)
        state = [np.zeros_like(flat) if part is None else tr.flatten(part).astype(np.float32) for part in (m, v)]
        self.params, self.m, self.v = self._guarded(flat), self._guarded(state[0]), self._guarded(state[1])
        self.grads, self.loss = self._guarded(np.zeros_like(flat)), self._guarded(np.zeros(1, "f"))
        self.t = torch.tensor([steps_before, 0], dtype=torch.int32, device=self.dev)
        self.X = torch.from_numpy(np.ascontiguousarray(X)).to(self.dev)
        self.code = nat.WB_DTYPE_U8 if X.dtype == np.uint8 else nat.WB_DTYPE_F32
        self.H, self.Y = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(self.dev) for v in (H, Y))
        need = C.c_size_t()
        nat.check(self.lib.wb_verify_train_scratch_bytes(*shape, B, C.byref(need)), "scratch_bytes")
        self.scratch = torch.full((need.value,), scratch_fill, dtype=torch.uint8, device=self.dev)
        self.hyper = nat.WbVerifyTrainHyper(lr=lr, beta1=beta1, beta2=beta2, adam_epsilon=adam_epsilon, momentum=momentum,
                                            bn_epsilon=bn_epsilon, dropout=dropout, seed=seed, reserved=0)

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


def check_step(got, arrays, o64, st64, o32, st32, label):
    """The one-step rule on the loss, every gradient, the moving statistics, the parameters after the update and Adam's
    m and v (on all their elements: they are smooth in g).  `arrays` are the parameters before the step."""
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
        compared = designs.compared_mask(k, arrays, o64, o32)
        left_out += compared.size - compared.sum()
        total += compared.size
        if compared.any():
            p64, p32 = st64["params"][k][compared], st32["params"][k][compared]
            diff, unit = held(got["params"][k][compared], p64, p32)
            report.append((f"p{k}", diff / unit))
            assert diff <= FACTOR * unit, (label, "parameter", k, diff, unit)
        if tr.is_moving(k):
            assert not got["m"][k].any() and not got["v"][k].any()
            continue
        for name in ("m", "v"):
            diff, unit = held(got[name][k], st64[name][k], st32[name][k])
            report.append((f"{name}{k}", diff / unit))
            assert diff <= FACTOR * unit, (label, "Adam's " + name, k, diff, unit)
    worst = max(r for _, r in report)
    print(f"{label}: largest ratio {worst:.3f} ({max(report, key=lambda x: x[1])[0]}), {left_out} of {total} parameters left out")
    assert left_out <= 0.05 * total, (label, left_out, total)
    assert got["t"] == st64["t"]
    return worst


def run_case(case, label):
    """One step of a case of verify_train_designs on the device, held to its two statements."""
    (o64, st64), (o32, st32) = designs.both_statements(case)
    shape, B = case["X"].shape[1:], len(case["idx"])
    dev = Device(shape, case["arrays"], case["X"], case["H"], case["Y"], B, m=case.get("m"), v=case.get("v"),
                 steps_before=case.get("steps_before", 0), **case.get("hyper", {}))
    got = dev.step(case["idx"])
    return got, o64, check_step(got, case["arrays"], o64, st64, o32, st32, label)


CASES = designs.SHORT_CASES + designs.LONG_CASES


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,B", CASES, ids=str)
def test_one_step_against_the_statement(shape, B, dtype):
    """The long batches reach what B <= 66 leaves unused: weight-gradient ranges of several windows and of unequal length,
    the cap of 128 per-channel partials (rows_per above 256, 128-long combines) for the full-size and the pooled layers,
    and the head's second to fourth window per thread and its whole loss tree."""
    run_case(designs.one_step_case(shape, B, dtype), f"{shape} B={B} {np.dtype(dtype).name}")


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


@pytest.mark.parametrize("B,live", designs.LIVE_CASES)
def test_one_live_window_at_the_partition_edges(B, live):
    """(6,6,1): the live window at slot 0, at slot B - 1, on both sides of the weight-gradient range boundary where the
    ranges grow by a window, in a slot that is its head thread's second window, and where the loss tree's halves meet.  A
    kernel that drops or doubles the window at such an edge loses or doubles every weight gradient
    (test_verify_train_host.py: a dropped live window moves arrays 0, 6, 12, 18 and 24 by thousands of units)."""
    case = designs.one_live_case(B, live)
    got, o64, _ = run_case(case, f"{designs.LIVE_SHAPE} B={B}, live window {live}")
    inside = (o64["losses"] > 1e-6) & (o64["losses"] < 1e3)
    assert inside[live] and inside.sum() == 1
    assert got["grads"][24].any() and got["grads"][0].any()


@pytest.mark.parametrize("shape", designs.TIE_SHAPES, ids=str)
def test_pool_ties_at_positive_maxima_go_to_the_first_maximum(shape):
    """Equal input pixels inside a pool cell give bit-equal maxima of block 2 (blocks 1 and 2 are pointwise by design), in
    more than half of the (cell, channel) pairs; the pool's choice among them routes the gradient of kernels 0 and 6
    through different neighbourhoods.  The last maximum, or every maximum, in vt_pool_bwd would move those two gradients
    by 1e5 units and more (test_verify_train_host.py); (7,6,2) puts the dropped row next to tied cells."""
    got, _, _ = run_case(designs.pool_tie_case(shape), f"pool ties {shape}")
    assert got["grads"][0].any() and got["grads"][6].any()


def test_steps_two_and_three_from_the_devices_own_state():
    """Each step's statements start from what the device held before it (parameters, m, v, t), so no error compounds and
    the one-step rule holds at every step: the recurrences on a non-zero m and v, lr_t at t >= 1 and the masks of step t."""
    base = designs.later_steps_case()
    shape, B = designs.LATER_SHAPE, designs.LATER_B
    dev = Device(shape, base["arrays"], base["X"], base["H"], base["Y"], B)
    arrays, m, v = base["arrays"], None, None
    for t, row in enumerate(base["rows"]):
        case = dict(base, idx=row, arrays=arrays, m=m, v=v, steps_before=t)
        (o64, st64), (o32, st32) = designs.both_statements(case)
        got = dev.step(row)
        check_step(got, arrays, o64, st64, o32, st32, f"step {t + 1} of three")
        assert got["t"] == t + 1
        arrays, m, v = got["params"], got["m"], got["v"]
    assert any(a.any() for a in m) and any(a.any() for a in v)


def test_one_step_away_from_every_default_constant():
    """lr, beta1, beta2, adam_epsilon, momentum, bn_epsilon, dropout and seed all differ from the defaults, from a state
    with non-zero m and v and t = 2: a constant that is hard-coded or read from the wrong field fails (the host twin shows
    that each constant alone moves some array by more than the bound)."""
    run_case(designs.nondefault_case(), "non-default constants")


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
