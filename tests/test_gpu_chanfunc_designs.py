"""The plain channel-function kernels of csrc/wb_chanfunc.hip on designed inputs, straight at the C ABI (wb_grad_hist_launch,
wb_grad_mag_launch; include/waldboost_hip.h): tests/chanfunc_designs.py holds the cases, tests/test_chanfunc_designs_host.py
proves from the oracle alone what they separate, and here the kernels must give the oracle's float32 and float64 bits, a NaN
as NaN, with nothing written behind the output.  Then once each through waldboost_amd.channels."""
import ctypes as C

import numpy as np
import pytest

import chanfunc_designs as cd
from oracle import wb_oracle as orc
from waldboost_amd import _native as nat

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
TAIL = 256


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(nat.require_gpu())


def grad_hist(image, n_bins=4, full=False, bias=0):
    """wb_grad_hist_launch as channels.grad_hist calls it -> float32 / float64 [H, W, n_bins]."""
    import torch
    img = np.ascontiguousarray(image.astype(np.float32))
    H, W = img.shape
    bias_v, wide = cd.scalar_arg(bias)
    cs, sn = orc.orientation_table(n_bins, full)
    cs_sn = np.concatenate([cs, sn]).astype(np.float64)
    dt = np.float64 if wide else np.float32
    nbytes = H * W * n_bins * np.dtype(dt).itemsize
    d = _dev(img)
    out = torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(nat.load().wb_grad_hist_launch(nat.stream_ptr(), nat.ptr(d), H, W, n_bins, int(bool(full)), bias_v, int(wide),
                                             cs_sn.ctypes.data_as(C.POINTER(C.c_double)), nat.ptr(out)), "wb_grad_hist_launch")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[nbytes:] == SENTINEL).all()
    return h[:nbytes].view(dt).reshape(H, W, n_bins)


def grad_mag(image, norm=5, eps=1e-3):
    """wb_grad_mag_launch as channels.grad_mag calls it -> float32 [H, W, 1]."""
    import torch
    img = np.ascontiguousarray(image.astype(np.float32))
    H, W = img.shape
    taps, eps_v, wide, scratch = None, 0.0, False, None
    if norm is not None and norm > 1:
        taps = np.ascontiguousarray(orc.triangle_kernel(int(norm)), np.float32)
        assert taps.size <= cd.MAX_TAPS
        eps_v, wide = cd.scalar_arg(eps)
        scratch = torch.full((2 * H * W * 4 + TAIL,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    d = _dev(img)
    out = torch.full((H * W * 4 + TAIL,), SENTINEL, dtype=torch.uint8, device=nat.require_gpu())
    nat.check(nat.load().wb_grad_mag_launch(nat.stream_ptr(), nat.ptr(d), H, W, 0 if taps is None else int(taps.size),
                                            None if taps is None else taps.ctypes.data_as(C.POINTER(C.c_float)), eps_v, int(wide),
                                            nat.ptr(scratch), nat.ptr(out)), "wb_grad_mag_launch")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[H * W * 4:] == SENTINEL).all()
    if scratch is not None:
        assert (scratch.cpu().numpy()[2 * H * W * 4:] == SENTINEL).all()
    return h[:H * W * 4].view(np.float32).reshape(H, W, 1)


def run(name):
    kind, img, args = cd.cases()[name]
    return grad_mag(img, **args) if kind == "mag" else grad_hist(img, **args)


def groups():
    """The cases by the first letters of their names: one test each, a few dozen launches."""
    out = {}
    for name in sorted(cd.cases()):
        key = name.split("/")[0].rstrip("0123456789x")
        out.setdefault("bias" if key.startswith("bias") else key, []).append(name)
    return out


@pytest.mark.parametrize("group", sorted(groups()))
def test_cases_bit_for_bit(group):
    for name in groups()[group]:
        got, ref = run(name), cd.oracle(name)
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, got.shape)
        bad = cd.differing(got, ref)
        assert bad == 0, (name, bad, np.argwhere(~(np.isnan(got) & np.isnan(ref)) & (got != ref))[:4].tolist())
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name


def test_python_surface_holds_the_same_cases():
    from waldboost_amd import channels
    # grad_hist: seven signed bins under a float64 bias (the wide path, a stride of 7 doubles)
    img = cd.noise(19, 27, 3)
    bias = np.float64(0.3)
    got, ref = channels.grad_hist(img, n_bins=7, full=True, bias=bias), orc.grad_hist(img, n_bins=7, full=True, bias=bias)
    assert got.dtype == np.float64 and cd.same_bits(got, ref)
    # grad_mag: 127 taps on a side of 5, and the float64 eps
    img = cd.cases()["side5x3/n63"][1]
    assert cd.same_bits(channels.grad_mag(img, norm=63, eps=0.25), orc.grad_mag(img, norm=63, eps=0.25))
    e = np.float64(1e-3)
    img = cd.cases()["order3/n5e64"][1]
    assert cd.same_bits(channels.grad_mag(img, norm=5, eps=e), orc.grad_mag(img, norm=5, eps=e))
