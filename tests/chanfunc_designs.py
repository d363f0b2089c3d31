"""Designed inputs for the plain channel-function kernels of csrc/wb_chanfunc.hip -- grad_hist(image, n_bins, full, bias) behind
wb_grad_hist_launch (grad_hist_args_kernel) and grad_mag(image, norm, eps) behind wb_grad_mag_launch (grad_mag_kernel and two
passes of tri_pass_kernel): NumPy, the oracle and the designed images of two neighbouring modules; no GPU, no torch.

hist_kernel and mag_kernel restate the kernels per pixel -- neighbours taken at the reflected coordinate, every pass in fp64
with one fp32 rounding, the projection in fp64, NumPy float32 (or, for a float64 scalar, float64) arithmetic after it -- with a
`wrong=` switch for WRONG_KERNELS.  test_chanfunc_designs_host.py proves the restatement equal to the oracle on every case and
every wrong kernel separated by the cases it is named for (RECORDED); test_gpu_chanfunc_designs.py runs the cases through the
two entry points bit for bit, a NaN as NaN.

Cases (cases(): name -> (kind, image, arguments))
  reused    gradmag_designs' reflect / zero / unit / tiny / squares / order and gradient_designs' words / absorb / zeros /
            extremes at shrink 1, each under REUSED_ARGS: the argument sets that leave the fused kernels -- grad_mag with
            norm 5 and eps 0.25, without a norm, with norm 2, with a float64 eps; grad_hist with a bias of 1e-30, and signed
  sides     noise of 1, 2, 3 and 5 pixels a side on either axis (1 x 1 among them), and 1 x 257, under norm 2, 5 and 63:
            127 taps run through several periods of the reflection
  bins      n_bins 1, 2, 5, 7, 31, 32, unsigned and signed, on 15 x 17 noise
  bias      on 15 x 17 noise: a bias equal to an attained |projection| whose projection is negative (+0 unsigned, -0.0
            signed), one float32 above and below it, a negative bias, a float64 bias (the wide path)
  special   an inf pixel and a NaN pixel one pixel inside the border: NaN signed, 0 through np.fmax unsigned
  flat_eps0 grad_mag with eps 0 over an image that is flat on the left: 0 / 0 = NaN there, as in the reference
  counts    255, 256, 257 and 513 pixels (15 x 17, 16 x 16, 1 x 257, 19 x 27) through both functions

Findings (asserted by the host test)
  * The three-tap gradient passes reach one pixel outside the image, where clamping, one reflection and the full reflection
    name the same pixel: the two wrong border rules show in the triangle filter alone.  On sides of 1 x 1, 1 x 2 and 2 x 1
    the magnitude is one value and no border rule shows at all.  `one reflection then a clamp` shows only on a side
    shorter than the filter's reach: never under norm 2, on sides 2 and 3 under norm 5, on 2, 3 and 5 under norm 63, and
    on none of the reused images.
  * The `order` profiles separate the left-to-right triangle sum in the whole centre row (8 pixels) under a float64 eps of
    1e-3 for all six profiles, and under eps = 0.25 for five of them: on the fourth profile the one-ulp difference of the
    normaliser is lost when 0.25 is added.  The claim is kept to those eleven cases.
  * Contracting the projection to an fma shows on the integer images' residues alone (gx cos(pi/2), gx c1 - gy s1 with
    gx == gy), unsigned; no noise image and no other n_bins here separates it.
  * np.sign gives +0 for -0.0, and so does the kernel's; a sign that hands -0.0 through shows under `full` on flat regions,
    where cos(theta_k) < 0 makes the projection -0.0: the output is then -0.0 for +0, under any bias.
  * An inf pixel gives inf - inf = NaN in the passes that see it twice and +-inf in the others, so around it the unsigned
    output holds 0 and inf; around the NaN pixel it is 0 everywhere and the signed output NaN everywhere.
"""
import functools
from fractions import Fraction

import numpy as np

import gradient_designs as gd
import gradmag_designs as gm
from oracle import wb_oracle as orc

MAX_TAPS = 127


def scalar_arg(x):
    """(value, wide) as channels._scalar_arg hands a bias or eps to the launch: a Python scalar is rounded to float32 and
    the arithmetic stays float32; a float64 NumPy scalar makes it float64."""
    if type(x) in (bool, int, float) or np.result_type(np.float32, x) == np.float32:
        return float(np.float32(x)), False
    return float(np.float64(x)), True


# ------------------------------------------------------------------------------ the kernels, restated
def border_index(i, n, mode="reflect"):
    """The coordinate inside [0, n) that coordinate i stands for."""
    i = np.asarray(i)
    if mode == "reflect":                        # scipy 'reflect': (d c b a | a b c d | d c b a), any number of times
        j = np.mod(i, 2 * n)
        return np.where(j >= n, 2 * n - 1 - j, j)
    if mode == "clamp":
        return np.clip(i, 0, n - 1)
    assert mode == "reflect_once"
    j = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
    return np.clip(j, 0, n - 1)


def _hpass(lo, mid, hi):
    return (mid * 2.0 + (lo + hi) * 1.0).astype(np.float32)


def _dpass(lo, mid, hi):
    return (mid * 0.0 + (lo - hi) * 1.0).astype(np.float32)


def gradients_at(img32, mode="reflect"):
    """gradients_at of the kernel for every pixel: (gx, gy) float32."""
    H, W = img32.shape
    ym, yp = border_index(np.arange(H) - 1, H, mode), border_index(np.arange(H) + 1, H, mode)
    xm, xp = border_index(np.arange(W) - 1, W, mode), border_index(np.arange(W) + 1, W, mode)
    I = img32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        h = _hpass(I[:, xm], I, I[:, xp]).astype(np.float64)
        gy = _dpass(h[ym], h, h[yp])
        v = _hpass(I[ym], I, I[yp]).astype(np.float64)
        gx = _dpass(v[:, xm], v, v[:, xp])
    return gx, gy


def _fma_projection(gx, gy, c, s):
    """float32(fma(gx, c, -(gy * s))) in fp64, in exact rational arithmetic (Fraction -> float is correctly rounded)."""
    out = np.empty(gx.shape, np.float32)
    fc = Fraction(float(c))
    for idx in np.ndindex(gx.shape):
        x, y = float(gx[idx]), float(gy[idx])
        if not (np.isfinite(x) and np.isfinite(y)):
            out[idx] = np.float32(x * c - y * s)
        else:
            out[idx] = np.float32(float(Fraction(x) * fc - Fraction(y * s)))
    return out


WRONG_HIST = ("fp32_projection", "fma_projection", "fmax_keeps_nan", "sign_neg_zero", "stride_4", "wide_computed_narrow")
WRONG_MAG = ("clamp_for_reflect", "one_reflection_then_clamp", "plain_order")
WRONG_KERNELS = WRONG_MAG + WRONG_HIST


def hist_kernel(image, n_bins=4, full=False, bias=0, wrong=None):
    """grad_hist_args_kernel: float32 (float64 for a float64 bias) [H, W, n_bins]."""
    img = image.astype(np.float32)
    H, W = img.shape
    gx, gy = gradients_at(img)
    cs, sn = orc.orientation_table(n_bins, full)
    bias_v, wide = scalar_arg(bias)
    out = np.zeros(H * W * n_bins, np.float64 if wide else np.float32)
    stride = 4 if wrong == "stride_4" else n_bins
    at = np.arange(H * W) * stride
    with np.errstate(invalid="ignore", over="ignore"):
        gxd, gyd = gx.astype(np.float64), gy.astype(np.float64)
        for k in range(n_bins):
            if wrong == "fp32_projection":
                c = gx * np.float32(cs[k]) - gy * np.float32(sn[k])
            elif wrong == "fma_projection":
                c = _fma_projection(gx, gy, float(cs[k]), float(sn[k]))
            else:
                c = (gxd * cs[k] - gyd * sn[k]).astype(np.float32)
            sg = np.where(c == 0, c, np.sign(c)) if wrong == "sign_neg_zero" else np.sign(c)
            if wide and wrong != "wide_computed_narrow":
                x = np.abs(c).astype(np.float64) - np.float64(bias_v)
                sg = sg.astype(np.float64)
            else:
                x = np.abs(c) - np.float32(bias_v)
            value = np.where(x < 0, 0, x).astype(x.dtype) if wrong == "fmax_keeps_nan" else np.fmax(x, x.dtype.type(0))
            res = (sg * value if full else value).astype(out.dtype)
            out[(at + k) % out.size] = res.reshape(-1)          # (only the wrong stride leaves the array; pixels in order)
    return out.reshape(H, W, n_bins)


def tri_pass(a32, w32, axis, mode="reflect", order="symmetric"):
    """tri_pass_kernel without the division: correlate1d with an odd symmetric kernel along `axis`, fp64, float32 result."""
    w = np.asarray(w32, np.float64)
    size1 = w.size // 2
    x = np.moveaxis(a32.astype(np.float64), axis, 0)
    n = x.shape[0]
    l = np.arange(n)
    at = lambda p: x[border_index(p, n, mode)]
    with np.errstate(invalid="ignore", over="ignore"):
        if order == "symmetric":
            t = at(l) * w[size1]
            for jj in range(-size1, 0):
                t = t + (at(l + jj) + at(l - jj)) * w[size1 + jj]
        else:
            t = at(l - size1) * w[0]
            for j in range(1, w.size):
                t = t + at(l - size1 + j) * w[j]
    return np.moveaxis(t, 0, axis).astype(np.float32)


def mag_kernel(image, norm=5, eps=1e-3, wrong=None):
    """wb_grad_mag_launch's three kernels: float32 [H, W, 1]."""
    img = image.astype(np.float32)
    gx, gy = gradients_at(img)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        mag = np.sqrt(gx * gx + gy * gy)
        if norm is not None and norm > 1:
            taps = orc.triangle_kernel(int(norm)).astype(np.float32)
            assert taps.size <= MAX_TAPS
            mode = {"clamp_for_reflect": "clamp", "one_reflection_then_clamp": "reflect_once"}.get(wrong, "reflect")
            order = "plain" if wrong == "plain_order" else "symmetric"
            f = tri_pass(tri_pass(mag, taps, 0, mode, order), taps, 1, mode, order)
            eps_v, wide = scalar_arg(eps)
            if wide:
                mag = (mag.astype(np.float64) / (f.astype(np.float64) + np.float64(eps_v))).astype(np.float32)
            else:
                mag = mag / (f + np.float32(eps_v))
    return mag[..., None]


# ------------------------------------------------------------------------------ cases
REUSED = (("gm", "reflect"), ("gm", "zero"), ("gm", "unit"), ("gm", "tiny"), ("gm", "squares"), ("gm", "order"),
          ("gd", "words"), ("gd", "absorb"), ("gd", "zeros"), ("gd", "extremes"))
REUSED_ARGS = (("mag", "n5e.25", dict(norm=5, eps=0.25)), ("mag", "none", dict(norm=None)), ("mag", "n2", dict(norm=2)),
               ("mag", "n5e64", dict(norm=5, eps=np.float64(1e-3))), ("hist", "b1e-30", dict(n_bins=4, bias=1e-30)),
               ("hist", "full", dict(full=True)))
SIDES = tuple((a, b) for a in (1, 2, 3, 5) for b in (1, 2, 3, 5)) + ((1, 257),)
NORMS = (2, 5, 63)
BINS = (1, 2, 5, 7, 31, 32)
COUNT_SHAPES = ((15, 17), (16, 16), (1, 257), (19, 27))


def noise(H, W, seed):
    return (np.random.default_rng(seed).random((H, W), np.float32) * np.float32(200)).astype(np.float32)


@functools.lru_cache(None)
def bias_image():
    return np.random.default_rng(7).integers(0, 256, (15, 17)).astype(np.uint8)


@functools.lru_cache(None)
def attained_bias(full):
    """(|projection| float32, pixel, bin): an attained |projection| above 1 of bias_image in bin 1 of the 4-bin table
    (unsigned, or signed), whose projection is negative."""
    gx, gy = orc.gradients(bias_image().astype(np.float32))
    cs, sn = orc.orientation_table(4, full)
    c = (gx.astype(np.float64) * cs[1] - gy.astype(np.float64) * sn[1]).astype(np.float32)
    y, x = np.argwhere(c < -1)[5]
    return np.float32(-c[y, x]), (int(y), int(x)), 1


def special_image():
    img = noise(15, 17, 11)
    img[1, 1] = np.inf
    img[13, 15] = np.nan
    return img


def flat_image():
    img = noise(16, 20, 12)
    img[:, :12] = 3.0
    return img


@functools.lru_cache(None)
def cases():
    """name -> (kind, image, arguments); kind "mag" runs grad_mag(image, **arguments), "hist" grad_hist."""
    out = {}
    for mod, name in REUSED:
        for i, img in enumerate((gm if mod == "gm" else gd).design_images(name, 1)):
            for kind, tag, args in REUSED_ARGS:
                out[f"{name}{i}/{tag}"] = (kind, img, args)
    for k, (a, b) in enumerate(SIDES):
        for norm in NORMS:
            out[f"side{a}x{b}/n{norm}"] = ("mag", noise(a, b, 100 + k), dict(norm=norm, eps=0.25))
    for nb in BINS:
        for full in (False, True):
            out[f"bins{nb}/{'full' if full else 'half'}"] = ("hist", noise(15, 17, 20 + nb), dict(n_bins=nb, full=full))
    for full in (False, True):
        b0 = attained_bias(full)[0]
        up, down = np.nextafter(b0, np.float32(np.inf)), np.nextafter(b0, np.float32(0))
        for tag, bias in (("equal", float(b0)), ("above", float(up)), ("below", float(down)), ("negative", -0.5),
                          ("float64", np.float64(float(b0)) + 1e-9), ("float64_equal", np.float64(float(b0)))):
            out[f"bias_{tag}/{'full' if full else 'half'}"] = ("hist", bias_image(), dict(n_bins=4, full=full, bias=bias))
    for full in (False, True):
        out[f"special/{'full' if full else 'half'}"] = ("hist", special_image(), dict(n_bins=6, full=full, bias=0.5))
        out[f"flat_negative_bias/{'full' if full else 'half'}"] = ("hist", flat_image(), dict(n_bins=5, full=full, bias=-0.5))
    out["special/mag"] = ("mag", special_image(), dict(norm=2, eps=0.25))
    out["flat_eps0"] = ("mag", flat_image(), dict(norm=5, eps=0.0))
    for H, W in COUNT_SHAPES:
        out[f"count{H}x{W}/mag"] = ("mag", noise(H, W, H * W), dict(norm=5, eps=0.25))
        out[f"count{H}x{W}/hist"] = ("hist", noise(H, W, H * W + 1), dict(n_bins=6, full=True, bias=0.125))
    assert all(max(v[1].shape) <= 257 and v[1].size <= 140 * 140 for v in out.values())
    return out


def oracle(name):
    kind, img, args = cases()[name]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        return orc.grad_mag(img, **args) if kind == "mag" else orc.grad_hist(img, **args)


def kernel(name, wrong=None):
    kind, img, args = cases()[name]
    return mag_kernel(img, wrong=wrong, **args) if kind == "mag" else hist_kernel(img, wrong=wrong, **args)


def same_bits(a, b):
    """Equal dtype, shape and bits; a NaN equal to any NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u))))


def differing(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return int((~(np.isnan(a) & np.isnan(b)) & (np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u))).sum())


# ------------------------------------------------------------------------------ what the host test found
# wrong kernel -> output elements it gets wrong over the cases it is named for (test_chanfunc_designs_host.py: NAMED)
RECORDED = {
    # (elements, cases)
    "clamp_for_reflect": (5762, 54), "one_reflection_then_clamp": (184, 23), "plain_order": (88, 11),
    "fp32_projection": (21781, 19), "fma_projection": (2594, 6), "fmax_keeps_nan": (98, 1), "sign_neg_zero": (2763, 3),
    "stride_4": (52476, 20), "wide_computed_narrow": (1180, 3),
}
