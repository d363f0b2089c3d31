"""The calibration kernels on the designs of tests/calib_designs.py (proved on the host by test_calib_designs_host.py): at
the C ABI (wb_samples_trace_launch, wb_calib_min_launch) bit for bit against the statement (tests/calib_reference.py) --
every NULL / non-NULL combination of outputs, dirty output buffers with guard words, reject 0 and 1, two consecutive
calls -- and through Model.stage_scores, calibration.stage_survival and calibration.calibrate."""
import ctypes as C
import itertools

import numpy as np
import pytest

import calib_designs as cd
import calib_reference as ref
from waldboost_amd import _native as nat
from waldboost_amd import calibration

pytestmark = pytest.mark.gpu

DESIGNS = cd.designs()
GUARD = 64                        # words on either side of an output
FILL = 0x5A5A5A5A

_cache = {}


def setup(name):
    """(design, model, device samples, WB_DTYPE_*, statement: trace, rejecting trace, alive) of a design, made once."""
    import torch
    if name not in _cache:
        d = DESIGNS[name]
        M = d.model()
        rt, alive = ref.trace_rejecting(d.trees, d.thetas, d.X)
        _cache[name] = (d, M, torch.from_numpy(d.X).cuda(), nat.WB_DTYPE_U8 if d.dtype == np.uint8 else nat.WB_DTYPE_F32,
                        ref.trace(d.trees, d.X), rt, alive)
    return _cache[name]


def guarded(words):
    """A device buffer of `words` 32-bit words between guards, all holding FILL; (tensor, pointer to the payload)."""
    import torch
    t = torch.full((words + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
    return t, C.c_void_p(t.data_ptr() + 4 * GUARD)


def payload(t, words):
    h = t.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == FILL).all() and (h[GUARD + words:] == FILL).all(), "words around an output were written"
    return h[GUARD:GUARD + words].copy()


def trace_call(name, reject, want=(True, True, True)):
    """One wb_samples_trace_launch into dirty, guarded buffers -> [trace (T, N), final (N,), alive (T + 1,)] as uint32
    words, None where not asked for."""
    d, M, X, wdt, *_ = setup(name)
    sizes = (d.T * d.N, d.N, d.T + 1)
    bufs = [guarded(s) if w else (None, None) for s, w in zip(sizes, want)]
    rc = nat.load().wb_samples_trace_launch(nat.stream_ptr(), M.device_cascade().handle, nat.ptr(X), wdt, d.N, reject,
                                            bufs[0][1], bufs[1][1], bufs[2][1])
    assert rc == 0, nat.last_error()
    return [payload(t, s) if t is not None else None for (t, _), s in zip(bufs, sizes)]


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


@pytest.mark.parametrize("name", list(DESIGNS))
def test_trace_on_the_designs(name):
    d, M, X, wdt, tr, rt, alive = setup(name)
    for reject, want_tr, want_alive in ((0, tr, np.full(d.T + 1, d.N)), (1, rt, alive)):
        got = trace_call(name, reject)
        assert np.array_equal(got[0], words(want_tr.T)), f"{name}: trace, reject={reject}"
        assert np.array_equal(got[1], words(want_tr[:, -1])), f"{name}: final, reject={reject}"
        assert np.array_equal(got[2].astype(np.int64), want_alive), (name, reject, got[2], want_alive)
        again = trace_call(name, reject)                                   # a second call: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
        # every combination of outputs gives what the full call gives
        for want in itertools.product((False, True), repeat=3):
            if any(want) and not all(want):
                part = trace_call(name, reject, want)
                assert all((p is None) == (not w) and (p is None or np.array_equal(p, g)) for p, g, w in zip(part, got, want)), want


def test_trace_error_returns():
    lib = nat.load()
    d, M, X, wdt, *_ = setup("ties-257x4")
    h = M.device_cascade().handle
    out, p = guarded(d.N)
    call = lambda **k: lib.wb_samples_trace_launch(nat.stream_ptr(), k.get("model", h), k.get("X", nat.ptr(X)), k.get("dtype", wdt),
                                                   k.get("n", d.N), k.get("reject", 0), None, k.get("final", p), None)
    assert call() == 0
    assert call(final=None) == nat.WB_ERR_INVALID and "output" in nat.last_error()      # all three outputs NULL
    assert call(model=None) == nat.WB_ERR_INVALID
    assert call(X=None) == nat.WB_ERR_INVALID
    assert call(dtype=nat.WB_DTYPE_F64) == nat.WB_ERR_INVALID
    assert call(reject=2) == nat.WB_ERR_INVALID
    assert call(n=-1) == nat.WB_ERR_INVALID
    assert call(n=0, X=None, final=None) == 0                              # no samples: no launch, no pointer looked at
    payload(out, d.N)


def calib_call(name, floor):
    """One wb_calib_min_launch into dirty, guarded buffers -> (stage_min float32 (T,), n_retained)."""
    d, M, X, wdt, *_ = setup(name)
    mn, pm = guarded(d.T)
    cnt, pc = guarded(1)
    rc = nat.load().wb_calib_min_launch(nat.stream_ptr(), M.device_cascade().handle, nat.ptr(X), wdt, d.N, C.c_float(floor), pm, pc)
    assert rc == 0, nat.last_error()
    return payload(mn, d.T).view(np.float32), int(payload(cnt, 1)[0])


@pytest.mark.parametrize("name", list(DESIGNS))
def test_calib_min_on_the_designs(name):
    d, M, X, wdt, tr, *_ = setup(name)
    for recall in d.recalls:
        p = ref.prune(tr, recall)
        got, n = calib_call(name, float(p["floor"]))
        assert n == int(p["retained"].sum()), (name, recall)
        assert np.all(got == p["theta"]), (name, recall, np.flatnonzero(got != p["theta"])[:5])
        if recall in d.owners:                                             # the planted owners' running scores
            assert np.all(got == tr[d.owners[recall], np.arange(d.T)])
        again, n2 = calib_call(name, float(p["floor"]))
        assert n2 == n and np.array_equal(again.view(np.uint32), got.view(np.uint32))
    # nobody retained: +inf everywhere; everybody: the minimum over all samples
    got, n = calib_call(name, float("inf"))
    assert n == 0 and np.isposinf(got).all()
    got, n = calib_call(name, float("-inf"))
    assert n == d.N and np.all(got == tr.min(axis=0))
    got, n = calib_call(name, float("nan"))
    assert n == 0 and np.isposinf(got).all()


def test_calib_min_error_returns():
    lib = nat.load()
    d, M, X, wdt, *_ = setup("ties-257x4")
    h = M.device_cascade().handle
    mn, pm = guarded(d.T)
    cnt, pc = guarded(1)
    call = lambda **k: lib.wb_calib_min_launch(nat.stream_ptr(), k.get("model", h), k.get("X", nat.ptr(X)), k.get("dtype", wdt),
                                               k.get("n", d.N), C.c_float(0.0), k.get("mn", pm), k.get("cnt", pc))
    assert call() == 0
    for bad in (dict(model=None), dict(X=None), dict(mn=None), dict(cnt=None), dict(dtype=nat.WB_DTYPE_F64), dict(n=-1)):
        assert call(**bad) == nat.WB_ERR_INVALID, bad
    assert call(n=0, X=None) == 0                                          # no samples: +inf and 0, whatever was there
    assert np.isposinf(payload(mn, d.T).view(np.float32)).all() and payload(cnt, 1)[0] == 0


@pytest.mark.parametrize("name", list(DESIGNS))
def test_python_surface_on_the_designs(name):
    import torch
    d, M, X, wdt, tr, rt, alive = setup(name)
    for src in (d.X, X):                                                   # host array and device tensor
        got = M.stage_scores(src)
        assert got.shape == (d.N, d.T) and got.dtype == np.float32 and np.array_equal(words(got), words(tr))
    got = M.stage_scores(X, reject=True, device=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(words(got.cpu().numpy()), words(rt))
    H, mask = M.predict(d.X)
    assert np.array_equal(words(got[:, -1].cpu().numpy()), words(H))
    surv = calibration.stage_survival(M, d.X)
    assert surv.dtype == np.int64 and np.array_equal(surv, alive) and surv[-1] == mask.sum()
    assert calibration.expected_cost(M, X) == alive[:d.T].sum() / d.N
    for recall in d.recalls:
        p = ref.prune(tr, recall)
        Mc = d.model()
        res = calibration.calibrate(Mc, X if recall == d.recalls[0] else d.X, recall=recall)
        assert np.all(res.theta == p["theta"]) and res.theta.dtype == np.float32
        assert (res.n, res.retained, res.floor) == (d.N, int(p["retained"].sum()), float(p["floor"]))
        assert res.old_theta == d.thetas and all(type(x) is float for x in Mc.theta)
        assert np.all(np.array(Mc.theta, np.float64) == p["theta"].astype(np.float64))
        # the guarantees: exactly the retained pass, with their unrejected scores; every threshold is met by one of them
        H, mask = Mc.predict(d.X)
        assert np.array_equal(mask, p["retained"])
        assert np.array_equal(words(H[mask]), words(tr[mask, -1]))
        assert ((tr[p["retained"]] == p["theta"][None, :]).any(axis=0)).all()
        # inplace=False leaves the model alone; a margin lowers every theta by its float32 value
        Mk = d.model()
        res2 = calibration.calibrate(Mk, d.X, recall=recall, margin=0.375, inplace=False)
        assert Mk.theta == d.thetas and np.all(res2.theta == p["theta"] - np.float32(0.375))


def test_stage_scores_edges():
    d, M, X, *_ = setup("ties-257x4")
    assert M.stage_scores(d.X[:0]).shape == (0, d.T)
    import waldboost_amd as wb
    E = wb.Model(cd.SHAPE, dict(wb.default_channel_opts))
    assert E.stage_scores(d.X).shape == (d.N, 0)
    assert np.array_equal(calibration.stage_survival(E, d.X), [d.N])
    with pytest.raises(ValueError):
        M.stage_scores(d.X[:, :4])
