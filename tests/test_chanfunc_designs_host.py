"""tests/chanfunc_designs.py proven without a GPU: the restated kernels equal the oracle on every case, the cases hold the
edges they claim, and every wrong kernel is separated from the oracle by the cases it is named for, with the exact counts
(chanfunc_designs.RECORDED)."""
import re

import numpy as np
import pytest

import chanfunc_designs as cd
from oracle import wb_oracle as orc

NAMES = sorted(cd.cases())


def test_restatement_is_the_oracle_on_every_case():
    for name in NAMES:
        assert cd.same_bits(cd.kernel(name), cd.oracle(name)), name


def test_cases_hold_what_they_are_called():
    c = cd.cases()
    assert len(c) == len(NAMES) >= 200 and sum(n.endswith(("n5e.25", "none", "n2", "n5e64", "b1e-30", "full")) for n in NAMES if "/" in n) >= 132
    # argument sets that leave the fused kernels, as the wrappers decide it
    for _, tag, args in cd.REUSED_ARGS:
        if "bias" in args or "full" in args:
            assert not (args.get("n_bins", 4) == 4 and not args.get("full", False) and args.get("bias", 0) == 0), tag
        else:
            assert not (args.get("norm", 5) == 5 and type(args.get("eps", 1e-3)) is float and args.get("eps", 1e-3) == 1e-3), tag
    assert cd.scalar_arg(0.25) == (0.25, False) and cd.scalar_arg(np.float64(1e-3)) == (1e-3, True) and cd.scalar_arg(1e-30)[1] is False
    # 127 taps, several periods of the reflection on the short sides
    assert orc.triangle_kernel(63).size == cd.MAX_TAPS == 127 and 63 // (2 * 5) >= 6
    assert {(1, 1), (1, 257), (5, 1), (2, 3)} <= set(cd.SIDES) and sorted(h * w for h, w in cd.COUNT_SHAPES) == [255, 256, 257, 513]
    # the attained bias: +0 unsigned and -0.0 signed at its pixel; one float32 to either side is not a tie
    b0, (y, x), k = cd.attained_bias(False)
    assert cd.oracle("bias_equal/half")[y, x, k].view(np.uint32) == 0 and cd.oracle("bias_below/half")[y, x, k] > 0
    b0, (y, x), k = cd.attained_bias(True)
    eqf = cd.oracle("bias_equal/full")
    assert eqf[y, x, k].view(np.uint32) == 0x80000000
    assert cd.oracle("bias_below/full")[y, x, k] < 0 and cd.oracle("bias_above/full")[y, x, k].view(np.uint32) == 0x80000000
    assert cd.oracle("bias_negative/half").min() >= 0.5
    for name in ("bias_float64/half", "bias_float64/full", "bias_float64_equal/full"):
        assert cd.oracle(name).dtype == np.float64
    assert cd.oracle("bias_float64_equal/full")[y, x, k] == 0 and np.signbit(cd.oracle("bias_float64_equal/full")[y, x, k])
    # inf and NaN pixels: NaN signed, 0 through np.fmax unsigned, one pixel inside the border
    img = cd.special_image()
    assert np.isinf(img[1, 1]) and np.isnan(img[13, 15]) and img.shape == (15, 17)
    half, full = cd.oracle("special/half"), cd.oracle("special/full")
    # (around the NaN pixel every gradient is NaN; around the inf pixel inf - inf is, and a lone inf stays inf)
    assert not np.isnan(half).any() and np.isnan(full[12:15, 14:17]).all() and np.isnan(full[0:3, 0:3]).sum() >= 27
    assert (half[12:15, 14:17] == 0).all() and np.isinf(half[0:3, 0:3]).any() and np.isnan(cd.oracle("special/mag")[1, 1, 0])
    # eps = 0 over the flat region: 0 / 0
    flat = cd.oracle("flat_eps0")
    assert np.isnan(flat[:, :5]).all() and np.isfinite(flat[:, 14:]).all()
    # the flat region's projection is -0.0 where cos(theta_k) < 0, and np.sign makes +0 of it
    neg = cd.oracle("flat_negative_bias/full")
    assert (neg[:, :10].view(np.uint32) == np.float32(0).view(np.uint32)).all()
    assert (cd.oracle("flat_negative_bias/half")[:, :10] == 0.5).all()
    # n_bins other than 3, 4 and 6
    assert not set(cd.BINS) & {3, 4, 6} and max(cd.BINS) == 32


def _kind(name):
    return cd.cases()[name][0]


def _sides(name):
    m = re.match(r"side(\d+)x(\d+)/n(\d+)", name)
    return tuple(int(g) for g in m.groups()) if m else None


CONSTANT_MAG = ((1, 1), (1, 2), (2, 1))          # sides on which the magnitude is one value: no border rule can show


def named(wrong, name):
    """Is `name` a case the wrong kernel is named for."""
    s = _sides(name)
    if wrong == "clamp_for_reflect":
        return (s is not None and s[:2] not in CONSTANT_MAG) or name.startswith("reflect") and name.endswith(("n5e.25", "n2", "n5e64"))
    if wrong == "one_reflection_then_clamp":          # a side shorter than the filter's reach (norm 2: one reflection is enough)
        return s is not None and s[:2] not in CONSTANT_MAG and any(1 < side < {2: 0, 5: 5, 63: 63}[s[2]] for side in s[:2])
    if wrong == "plain_order":                         # (order3 at eps = 0.25: the one profile the larger eps hides)
        return name.startswith("order") and (name.endswith("n5e64") or name.endswith("n5e.25") and not name.startswith("order3"))
    if wrong == "fp32_projection":
        return name.startswith(("words", "extremes", "bins5", "bins7", "bins31", "bins32", "count15x17/h", "count16x16/h", "count19x27/h"))
    if wrong == "fma_projection":                      # the residues of the integer images: cos(pi/2) and gx c1 - gy s1
        return name.startswith(("words", "absorb", "extremes", "zeros")) and name.endswith("b1e-30")
    if wrong == "fmax_keeps_nan":
        return name == "special/half"
    if wrong == "sign_neg_zero":
        return name in ("flat_negative_bias/full", "zero0/full", "extremes0/full")
    if wrong == "stride_4":
        return name.startswith("bins") or name.startswith("count") and _kind(name) == "hist" or name.startswith(("special/h", "special/f", "flat_neg"))
    assert wrong == "wide_computed_narrow"
    return name.startswith("bias_float64/") or name == "bias_float64_equal/half"


@pytest.mark.parametrize("wrong", cd.WRONG_KERNELS)
def test_wrong_kernels_are_separated(wrong):
    kind = "mag" if wrong in cd.WRONG_MAG else "hist"
    total = cases = 0
    for name in NAMES:
        if _kind(name) != kind or (wrong == "fma_projection" and not named(wrong, name)):     # (exact arithmetic: the named cases only)
            continue
        bad = cd.differing(cd.kernel(name, wrong), cd.oracle(name))
        if named(wrong, name):
            assert bad >= 1, (wrong, name)
            total += bad
            cases += 1
        elif wrong in ("one_reflection_then_clamp", "plain_order", "fmax_keeps_nan", "wide_computed_narrow", "stride_4"):
            assert bad == 0, (wrong, name)                     # (sharp: everywhere else such a kernel is right)
    print(f"{wrong}: {total} elements over {cases} cases")
    assert cases >= 1 and cd.RECORDED[wrong] == (total, cases)


def test_the_gradient_passes_do_not_tell_the_border_rules_apart():
    """One pixel outside the image the three rules name the same pixel: the two wrong ones show in the triangle filter only."""
    for n in (1, 2, 3, 5, 257):
        i = np.array([-1, n])
        assert np.array_equal(cd.border_index(i, n), cd.border_index(i, n, "clamp")) and np.array_equal(cd.border_index(i, n), cd.border_index(i, n, "reflect_once"))
    for name in ("side2x3/n63", "side5x5/n5", "reflect0/none"):
        for wrong in ("clamp_for_reflect", "one_reflection_then_clamp"):
            kind, img, args = cd.cases()[name]
            assert cd.same_bits(cd.mag_kernel(img, norm=None, wrong=wrong), orc.grad_mag(img, norm=None))
