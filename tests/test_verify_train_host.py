"""Host side of the verifier's training: the NumPy statement of the step (tests/verify_train_reference.py)
is checked against finite differences, closed forms and designed inputs; the dropout generator's restatement; set_weights,
train's refusals, and the C entry points' validation that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import verify_train_designs as designs
import verify_train_reference as tr
from verify_train_designs import random_arrays, random_batch
from waldboost_amd import _native as nat
from waldboost_amd import verification as ver


@pytest.mark.parametrize("shape,B", [((4, 4, 2), 4), ((5, 6, 3), 6)])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_gradients_against_central_differences(shape, B, dropout):
    arrays = [a.astype(np.float64) for a in random_arrays(shape, 11)]
    X, H, Y = random_batch(shape, B, 12)
    F = (shape[0] // 2) * (shape[1] // 2) * 16
    masks = tr.dropout_masks(5, 0, B, F, dropout) if dropout else None
    scale = tr.dropout_scale(dropout)
    out = tr.forward_backward(arrays, X, H, Y, np.float64, masks, scale, zero_conv_bias=False)
    rng = np.random.default_rng(3)
    h = 1e-5
    for k in range(28):
        if tr.is_moving(k):
            continue
        g = out["grads"][k].reshape(-1)
        for j in rng.choice(g.size, min(g.size, 5), replace=False):
            vals = []
            for sign in (1, -1):
                moved = [a.copy() for a in arrays]
                moved[k].reshape(-1)[j] += sign * h
                vals.append(tr.loss_of(moved, X, H, Y, masks, scale))
            fd = (vals[0] - vals[1]) / (2 * h)
            # (a ReLU or a pool maximum changing hands inside +-h would show as an error of the gradient's own size)
            assert abs(fd - g[j]) <= 1e-6 * np.abs(g).max() + 1e-9, (k, j, fd, g[j])
    # the un-zeroed bias gradient is rounding noise: this is why the contract says zero
    for k in range(4):
        assert np.abs(out["grads"][6 * k + 1]).max() < 1e-12 * np.abs(out["grads"][6 * k]).max()
    zeroed = tr.forward_backward(arrays, X, H, Y, np.float64, masks, scale)
    assert all(not zeroed["grads"][6 * k + 1].any() for k in range(4))


def test_adam_three_steps_against_the_closed_form():
    shape = (4, 4, 2)
    arrays = random_arrays(shape, 2)
    rng = np.random.default_rng(0)
    grads = [rng.standard_normal(a.shape) for a in arrays]
    state = tr.new_state(arrays, np.float64)
    start = [a.copy() for a in state["params"]]
    lr, b1, b2, eps, mom = 1e-4, 0.9, 0.999, 1e-7, 0.99
    for _ in range(3):
        tr.update(state, grads, np.float64)
    assert state["t"] == 3
    for k in range(28):
        if tr.is_conv_bias(k):
            assert np.array_equal(state["params"][k], start[k]) and not state["m"][k].any() and not state["v"][k].any()
        elif tr.is_moving(k):
            assert np.allclose(state["params"][k], mom ** 3 * start[k] + (1 - mom ** 3) * grads[k], rtol=1e-12, atol=0)
        else:
            # a constant gradient: m_t = (1 - b1^t) g, v_t = (1 - b2^t) g^2
            want = start[k].copy()
            for t in (1, 2, 3):
                lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
                want -= lr_t * (1 - b1 ** t) * grads[k] / (np.sqrt(1 - b2 ** t) * np.abs(grads[k]) + eps)
            assert np.allclose(state["params"][k], want, rtol=1e-10, atol=1e-14)
            assert np.allclose(state["m"][k], (1 - b1 ** 3) * grads[k]) and np.allclose(state["v"][k], (1 - b2 ** 3) * grads[k] ** 2)


def test_a_saturated_batch_has_zero_gradients():
    shape, B = (5, 6, 3), 6
    arrays = random_arrays(shape, 4)
    X, _, Y = random_batch(shape, B, 5)
    H = (Y * np.array([50, -50, 40, -30, 60, 20])).astype("f")         # e = exp(-Y p): far below 1e-6 or far above 1e3
    for dt in (np.float64, np.float32):
        out = tr.forward_backward(arrays, X, H, Y, dt)
        assert np.all((out["losses"] == dt(1e-6)) | (out["losses"] == dt(1e3)))
        for k in range(28):
            if not tr.is_moving(k):
                assert not out["grads"][k].any(), k


def test_pool_ties_go_to_the_first_maximum_and_dropped_rows_get_nothing():
    a = np.zeros((1, 5, 5, 2))
    a[0, 0:2, 0:2, 0] = [[3, 3], [3, 3]]          # a four-way tie: (0, 0)
    a[0, 0:2, 2:4, 0] = [[1, 4], [4, 2]]          # two maxima: (0, 1) comes before (1, 0)
    a[0, 2:4, 0:2, 0] = [[0, 0], [0, 5]]
    a[0, 2:4, 2:4, 0] = [[0, 0], [7, 7]]          # (1, 0) before (1, 1)
    a[0, :, :, 1] = np.arange(25).reshape(5, 5)   # strictly increasing: always (1, 1)
    a[0, 4, :, :] = 100                           # the dropped row and column hold the largest values
    a[0, :, 4, :] = 100
    assert np.array_equal(tr.pool2x2(a)[0, :, :, 0], [[3, 4], [5, 7]])
    d = np.arange(1, 9, dtype=np.float64).reshape(1, 2, 2, 2)
    da = tr.pool2x2_backward(a, d)
    want0 = np.zeros((5, 5))
    want0[0, 0], want0[0, 3], want0[3, 1], want0[3, 2] = d[0, 0, 0, 0], d[0, 0, 1, 0], d[0, 1, 0, 0], d[0, 1, 1, 0]
    assert np.array_equal(da[0, :, :, 0], want0)
    want1 = np.zeros((5, 5))
    want1[1, 1], want1[1, 3], want1[3, 1], want1[3, 3] = d[0, 0, 0, 1], d[0, 0, 1, 1], d[0, 1, 0, 1], d[0, 1, 1, 1]
    assert np.array_equal(da[0, :, :, 1], want1)
    assert not da[0, 4].any() and not da[0, :, 4].any()


def test_the_dropout_generator():
    n = 2 ** 20
    keep = tr.drop_keep(1234, 0, 0, n, 0.2)
    assert abs(keep.mean() - 0.8) <= 4 * np.sqrt(0.16 / n)
    assert tr.drop_threshold(0.2) == 858993459 and tr.drop_threshold(0.0) == 0
    assert tr.drop_keep(1234, 0, 0, 4096, 0.0).all()
    seen = {}
    for step in range(3):
        for layer in (0, 1):
            bits = tr.drop_bits(1234, step, layer, 4096)
            assert np.array_equal(bits, tr.drop_bits(1234, step, layer, 4096))
            assert bits.dtype == np.uint32
            for other in seen.values():
                assert np.mean((bits >= tr.drop_threshold(0.2)) != (other >= tr.drop_threshold(0.2))) > 0.2
            seen[(step, layer)] = bits
    assert not np.array_equal(tr.drop_bits(1235, 0, 0, 4096), seen[(0, 0)])
    # a prefix does not depend on the count, and the scalar form is the array form
    assert np.array_equal(tr.drop_bits(1234, 1, 1, 100), seen[(1, 1)][:100])
    x = (77 * 0x9E3779B1) & 0xFFFFFFFF ^ int(tr.drop_key(1234, 1, 1))
    for shift, mul in ((16, 0x85EBCA6B), (13, 0xC2B2AE35)):
        x = ((x ^ (x >> shift)) * mul) & 0xFFFFFFFF
    assert (x ^ (x >> 16)) == int(seen[(1, 1)][77])
    # dropout = 0 is the identity of the statement, bit for bit
    shape, B = (4, 4, 2), 4
    arrays, (X, H, Y) = random_arrays(shape, 1), random_batch(shape, B, 2)
    plain = tr.forward_backward(arrays, X, H, Y, np.float32)
    kept = tr.forward_backward(arrays, X, H, Y, np.float32, tr.dropout_masks(9, 0, B, 64, 0.0), tr.dropout_scale(0.0))
    assert all(np.array_equal(a, b) for a, b in zip(plain["grads"], kept["grads"])) and plain["loss"] == kept["loss"]


def test_set_weights_folds_again():
    shape = (6, 5, 3)
    V = ver.model_cnn(shape, seed=0)
    V._device[0] = "stale"
    arrays = random_arrays(shape, 8)
    arrays[4] = np.full(8, 0.3, "f")
    arrays[5] = np.full(8, 1.7, "f")
    V.set_weights(arrays)
    fresh = ver.Verifier(shape, arrays)
    assert np.array_equal(V._packed, fresh._packed) and V._device == {}
    assert all(np.array_equal(a, b) for a, b in zip(V.get_weights(), arrays))
    before = V._packed.copy()
    with pytest.raises(ValueError):
        V.set_weights(arrays[:27])
    bad = list(arrays)
    bad[5] = np.full(8, -1.0, "f")
    with pytest.raises(ValueError):
        V.set_weights(bad)
    bad = list(arrays)
    bad[0] = np.full_like(bad[0], np.nan)
    with pytest.raises(ValueError):
        V.set_weights(bad)
    assert np.array_equal(V._packed, before) and all(np.array_equal(a, b) for a, b in zip(V.get_weights(), arrays))


def test_train_and_trainer_argument_errors():
    import torch
    for M in (None, object(), "keras"):
        with pytest.raises(NotImplementedError) as e:
            ver.train(M, None, None, None, None)
        assert "from_keras_weights" in str(e.value) and "reference" in str(e.value)
    V = ver.model_cnn((6, 5, 3), seed=0)
    X = np.zeros((4, 6, 5, 3), "f")
    with pytest.raises(NotImplementedError):
        ver.train(V, X, np.zeros(4), X, np.zeros(4), batch_size=1, verbose=False)
    with pytest.raises(NotImplementedError):
        ver.train(V, X, np.zeros(4), X, np.zeros(4), batch_size=2000, verbose=False)
    with pytest.raises(ValueError):
        ver.train(V, X, np.zeros(4), X, np.zeros(4), steps=0, verbose=False)
    with pytest.raises(TypeError):
        ver.Trainer(None)
    with pytest.raises(ValueError):
        ver.Trainer(V, dropout=1.0)
    with pytest.raises(ValueError):
        ver.Trainer(V, lr=-1.0)
    with pytest.raises(ValueError):
        ver.Trainer(V, momentum=1.5)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ver.Trainer(V)
        with pytest.raises(RuntimeError):
            ver.train(V, X, np.zeros(4), X, np.zeros(4), steps=1, epochs=1, verbose=False)
    with pytest.raises(NotImplementedError):
        ver.Trainer(ver.model_cnn((40, 12, 4), seed=0))           # a window shape the kernels do not take


def test_training_entry_points_validate_without_a_gpu():
    lib = nat.load()
    count, nbytes = C.c_int64(), C.c_size_t()
    for shape, F in [((14, 14, 4), 784), ((32, 32, 16), 4096), ((2, 2, 1), 16), ((3, 5, 2), 32), ((13, 32, 9), 1536)]:
        assert lib.wb_verify_train_param_floats(*shape, C.byref(count)) == 0
        Cc = shape[2]
        assert count.value == 72 * Cc + 576 + 1152 + 2304 + 5 * (8 + 8 + 16 + 16) + 128 * F + 128 + 128 + 1
        assert count.value == sum(a.size for a in ver.model_cnn(shape, seed=0).get_weights())
        small, big = C.c_size_t(), C.c_size_t()
        assert lib.wb_verify_train_scratch_bytes(*shape, 2, C.byref(small)) == 0
        assert lib.wb_verify_train_scratch_bytes(*shape, 64, C.byref(big)) == 0
        assert 0 < small.value < big.value and big.value % 16 == 0
    hyper = nat.WbVerifyTrainHyper(lr=1e-4, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99, bn_epsilon=1e-3, dropout=0.2, seed=1)
    hp = C.byref(hyper)
    step = lambda *a: lib.wb_verify_train_step(None, *a)
    ok = dict(X=1024, dt=nat.WB_DTYPE_F32, H=1024, Y=1024, N=10, idx=1024, B=4)
    tail = lambda p=1024, sb=1 << 30: (p, p, p, 1024, hp, 1024, sb, 1024, None)
    for shape in [(1, 12, 4), (12, 33, 4), (12, 12, 0), (12, 12, 17)]:
        assert lib.wb_verify_train_param_floats(*shape, C.byref(count)) == nat.WB_ERR_UNSUPPORTED
        assert "window shape" in nat.last_error()
        assert lib.wb_verify_train_scratch_bytes(*shape, 4, C.byref(nbytes)) == nat.WB_ERR_UNSUPPORTED
        assert step(None, nat.WB_DTYPE_F32, None, None, 0, None, 4, *shape, None, None, None, None, None, None, 0, None, None) == nat.WB_ERR_UNSUPPORTED
    for B in (0, 1, 3, 63, 1026, -2):
        assert lib.wb_verify_train_scratch_bytes(12, 12, 4, B, C.byref(nbytes)) == nat.WB_ERR_UNSUPPORTED
        assert "batch" in nat.last_error()
        assert step(1024, ok["dt"], 1024, 1024, 10, 1024, B, 12, 12, 4, *tail()) == nat.WB_ERR_UNSUPPORTED
    assert step(1024, nat.WB_DTYPE_F64, 1024, 1024, 10, 1024, 4, 12, 12, 4, *tail()) == nat.WB_ERR_UNSUPPORTED
    assert step(None, ok["dt"], None, None, 10, None, 4, 12, 12, 4, None, None, None, None, None, None, 0, None, None) == nat.WB_ERR_INVALID
    assert "null" in nat.last_error()
    assert step(1024, ok["dt"], 1024, 1024, 0, 1024, 4, 12, 12, 4, *tail()) == nat.WB_ERR_INVALID
    assert "pool" in nat.last_error()
    assert step(1024, ok["dt"], 1024, 1024, 10, 1024, 4, 12, 12, 4, *tail(p=1024 + 8)) == nat.WB_ERR_INVALID
    assert "aligned" in nat.last_error()
    assert step(1024, ok["dt"], 1024, 1024, 10, 1024 + 2, 4, 12, 12, 4, *tail()) == nat.WB_ERR_INVALID
    assert "aligned" in nat.last_error()
    assert lib.wb_verify_train_scratch_bytes(12, 12, 4, 4, C.byref(nbytes)) == 0
    assert step(1024, ok["dt"], 1024, 1024, 10, 1024, 4, 12, 12, 4, *tail(sb=nbytes.value - 1)) == nat.WB_ERR_INVALID
    assert "scratch" in nat.last_error()
    for field, value in (("dropout", 1.0), ("dropout", -0.1), ("beta1", 1.0), ("lr", float("nan")), ("bn_epsilon", 0.0), ("momentum", 2.0)):
        bad = nat.WbVerifyTrainHyper(lr=1e-4, beta1=0.9, beta2=0.999, adam_epsilon=1e-7, momentum=0.99, bn_epsilon=1e-3, dropout=0.2, seed=1)
        setattr(bad, field, value)
        assert lib.wb_verify_train_step(None, 1024, ok["dt"], 1024, 1024, 10, 1024, 4, 12, 12, 4, 1024, 1024, 1024, 1024, C.byref(bad),
                                        1024, 1 << 30, 1024, None) == nat.WB_ERR_INVALID
        assert "hyper" in nat.last_error()
    assert nat.WB_ABI_VERSION == 8 and lib.wb_abi_version() == 8


# ---- host twins of the GPU cases (tests/verify_train_designs.py): from the float64 and float32 statements alone, the rule
# leaves out at most 2.5 % of the parameters -- half the GPU tests' cap, because the GPU's unit is the statement's -- and a
# wrong kernel would move the result by more than the rule allows.
def moved(k, wrong, o64, o32, key="grads"):
    """By how many of the rule's units array k of `wrong` differs from the float64 statement."""
    diff, unit = designs.held(wrong[key][k], o64[key][k], o32[key][k])
    return diff / unit


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,B", designs.LONG_CASES, ids=str)
def test_long_batch_cases_leave_out_little(shape, B, dtype):
    case = designs.one_step_case(shape, B, dtype)
    assert len(set(case["idx"])) < B <= len(case["X"]) - 3
    (o64, _), (o32, _) = designs.both_statements(case)
    share = designs.left_out_share(case["arrays"], o64, o32)
    print(f"{shape} B={B} {np.dtype(dtype).name}: {100 * share:.2f} % left out")
    assert share <= designs.LEFT_OUT_HOST
    # what the case is there to reach
    P, P2 = shape[0] * shape[1], (shape[0] // 2) * (shape[1] // 2)
    lengths = {b1 - b0 for b0, b1 in (designs.wgrad_range(B, g) for g in range(128))}
    want = {((2, 3, 1), 130): ({1, 2}, 4, 1), ((4, 4, 2), 1022): ({7, 8}, 64, 16), ((6, 6, 1), 1024): ({8}, 128, 36),
            ((10, 14, 1), 1024): ({8}, 128, 128)}[(shape, B)]
    assert (lengths, min(128, -(-B * P // 256)), min(128, -(-B * P2 // 256))) == want


def test_live_window_slots_sit_on_the_partition_edges():
    assert designs.live_slots(130) == [0, 62, 63, 64, 65, 129]             # ranges 62: [62, 63), 63: [63, 65), 64: [65, 66)
    assert [designs.wgrad_range(130, g) for g in (62, 63, 64)] == [(62, 63), (63, 65), (65, 66)]
    assert designs.live_slots(258) == [0, 125, 126, 256, 257] and designs.wgrad_range(258, 63) == (126, 129)
    assert designs.live_slots(1022) == [0, 6, 7, 261, 1021] and designs.wgrad_range(1022, 1) == (7, 15)
    assert designs.live_slots(1024) == [0, 261, 511, 512, 1023]
    for B in (130, 258, 1022, 1024):
        assert designs.wgrad_range(B, 0)[0] == 0 and designs.wgrad_range(B, 127)[1] == B


@pytest.mark.parametrize("B,live", designs.LIVE_CASES)
def test_one_live_window_cases_leave_out_little_and_see_the_window(B, live):
    case = designs.one_live_case(B, live)
    (o64, _), (o32, _) = designs.both_statements(case)
    inside = (o64["losses"] > 1e-6) & (o64["losses"] < 1e3)
    assert inside[live] and inside.sum() == 1
    assert designs.left_out_share(case["arrays"], o64, o32) <= designs.LEFT_OUT_HOST
    # a kernel that drops the live window: its dp is 0, which is the statement with that window saturated as well
    dropped, _ = designs.statement(**designs.one_live_case(B, live, saturate_all=True), dtype=np.float64)
    assert not ((dropped["losses"] > 1e-6) & (dropped["losses"] < 1e3)).any()
    for k in (0, 6, 12, 18, 24):
        assert moved(k, dropped, o64, o32) > designs.FACTOR, k


@pytest.fixture
def block2_outputs(monkeypatch):
    """Block 2's output as pool2x2_backward sees it, by dtype name."""
    seen, true_pool = {}, tr.pool2x2_backward

    def spy(a, dpool):
        seen[a.dtype.name] = a.copy()
        return true_pool(a, dpool)
    monkeypatch.setattr(tr, "pool2x2_backward", spy)
    return seen


@pytest.mark.parametrize("shape,ties,first", [((6, 6, 2), 161, [100, 39, 22, 0]), ((7, 6, 2), 156, [98, 39, 19, 0])], ids=str)
def test_pool_tie_design_has_ties_that_reach_the_weight_gradients(shape, ties, first, block2_outputs, monkeypatch):
    assert shape in designs.TIE_SHAPES
    case = designs.pool_tie_case(shape)
    (o64, _), (o32, _) = designs.both_statements(case)
    assert designs.left_out_share(case["arrays"], o64, o32) <= designs.LEFT_OUT_HOST
    tied64, first64 = designs.tie_census(block2_outputs["float64"])
    tied32, first32 = designs.tie_census(block2_outputs["float32"])
    # 288 (cell, channel) pairs; a tie's first maximum cannot be the cell's last pixel
    assert tied64.size == 288 and tied64.sum() == ties and np.bincount(first64[tied64], minlength=4).tolist() == first
    assert np.array_equal(tied64, tied32) and np.array_equal(first64, first32)
    for wrong_pool in (designs.pool2x2_backward_last, designs.pool2x2_backward_all):
        monkeypatch.setattr(tr, "pool2x2_backward", wrong_pool)
        wrong, _ = designs.statement(**case, dtype=np.float64)
        ratios = [moved(k, wrong, o64, o32) for k in (0, 6)]
        print(shape, wrong_pool.__name__, "moves the gradients of kernels 0 and 6 by", ratios, "units")
        assert min(ratios) > designs.FACTOR


def test_the_wrong_pools_are_wrong_only_at_ties():
    a = np.zeros((1, 2, 4, 1))
    a[0, :, 0:2, 0] = [[1, 4], [4, 2]]
    a[0, :, 2:4, 0] = [[0, 3], [1, 2]]
    d = np.array([5.0, 7.0]).reshape(1, 1, 2, 1)
    assert np.array_equal(tr.pool2x2_backward(a, d)[0, :, :, 0], [[0, 5, 0, 7], [0, 0, 0, 0]])
    assert np.array_equal(designs.pool2x2_backward_last(a, d)[0, :, :, 0], [[0, 0, 0, 7], [5, 0, 0, 0]])
    assert np.array_equal(designs.pool2x2_backward_all(a, d)[0, :, :, 0], [[0, 5, 0, 7], [5, 0, 0, 0]])


def test_later_steps_leave_out_little():
    """The GPU test starts each step's statements from the device's state; here the float32 statement's own state stands
    in for it."""
    base = designs.later_steps_case()
    assert len({tuple(row) for row in base["rows"]}) == 3
    arrays, m, v = base["arrays"], None, None
    for t, row in enumerate(base["rows"]):
        (o64, _), (o32, st32) = designs.both_statements(dict(base, idx=row, arrays=arrays, m=m, v=v, steps_before=t))
        assert designs.left_out_share(arrays, o64, o32) <= designs.LEFT_OUT_HOST
        assert st32["t"] == t + 1
        arrays, m, v = st32["params"], st32["m"], st32["v"]


def test_every_non_default_constant_moves_the_step():
    case = designs.nondefault_case()
    assert case["steps_before"] == 2 and all(designs.NONDEFAULT[name] != designs.DEFAULTS[name] for name in designs.DEFAULTS)
    updated = [k for k in range(28) if not tr.is_conv_bias(k)]
    adam = [k for k in updated if not tr.is_moving(k)]
    assert all(case["m"][k].any() and case["v"][k].any() for k in adam)
    (o64, st64), (o32, st32) = designs.both_statements(case)
    assert designs.left_out_share(case["arrays"], o64, o32) <= designs.LEFT_OUT_HOST

    def distance(hyper):
        """Per kind of result, the ratios by which the step under `hyper` differs from the step under NONDEFAULT."""
        (other, st), _ = designs.both_statements(designs.nondefault_case(hyper))
        return {"params": [moved(k, st, st64, st32, "params") for k in updated], "m": [moved(k, st, st64, st32, "m") for k in adam],
                "v": [moved(k, st, st64, st32, "v") for k in adam], "grads": [moved(k, other, o64, o32) for k in updated]}
    # under the defaults every updated array, and Adam's state of each, lands elsewhere
    far = distance(designs.DEFAULTS)
    assert min(far["params"]) > designs.FACTOR and min(far["m"]) > designs.FACTOR and min(far["v"]) > designs.FACTOR
    # and no constant hides behind the others: each one alone, put back to its default, moves what it enters
    enters = dict(lr=["params"], beta1=["params", "m"], beta2=["params", "v"], adam_epsilon=["params"], momentum=["params"],
                  bn_epsilon=["grads", "params", "m", "v"], dropout=["grads", "params", "m", "v"], seed=["grads", "params", "m", "v"])
    for name, kinds in enters.items():
        near = distance(dict(designs.NONDEFAULT, **{name: designs.DEFAULTS[name]}))
        for kind in kinds:
            assert max(near[kind]) > designs.FACTOR, (name, kind)
        if name == "momentum":
            assert min(near["params"][k] for k, a in enumerate(updated) if tr.is_moving(a)) > designs.FACTOR


def test_the_statement_alone_meets_the_loss_cap():
    """The end-to-end case of the GPU suite -- (8, 8, 2), B = 16, planted data, lr = 1e-3, 4 epochs of 50 steps, seed 7 --
    in the float64 statement, with the batches train draws: the last epoch's mean loss is below half the first's."""
    import verify_train_designs as designs
    means, _ = designs.planted_statement_run(epochs=4, steps=50)
    print("epoch means of the float64 statement:", means)
    assert means[-1] < 0.5 * means[0]
