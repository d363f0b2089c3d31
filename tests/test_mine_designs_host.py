"""The designs of tests/mine_designs.py, proved on the CPU: the statement (mine_reference) gives what each construction
planted, the emulated kernels agree with the statement, and every emulated fault is caught by the design named for it."""
from fractions import Fraction

import numpy as np
import pytest

import mine_designs as md
import mine_reference as ref
from match_designs import iou_exact


def test_fmix32_and_its_inverse():
    x = np.concatenate([[0, 1, 0xFFFFFFFF, 0x80000000, 0x9E3779B9], np.random.default_rng(0).integers(0, 1 << 32, 4096)]).astype(np.uint64)
    assert np.array_equal(ref.unfmix32(ref.fmix32(x)), x.astype(np.uint32))
    assert np.array_equal(ref.fmix32(ref.unfmix32(x)), x.astype(np.uint32))
    # MurmurHash3's finaliser by hand, in Python integers
    def f(v):
        v ^= v >> 16
        v = v * 0x85EBCA6B & 0xFFFFFFFF
        v ^= v >> 13
        v = v * 0xC2B2AE35 & 0xFFFFFFFF
        return v ^ v >> 16
    assert [int(v) for v in ref.fmix32(x[:64])] == [f(int(v)) for v in x[:64]]
    g = f(f(7 ^ f((5 + 0x9E3779B9) & 0xFFFFFFFF)) ^ (3 * 0x9E3779B1 & 0xFFFFFFFF))
    assert int(ref.group_word(7, 5, 3)) == g
    assert int(ref.window_keys(7, 5, 3, 300, 20)) == f(((300 << 16) | 20) ^ g)
    r, c = ref.window_of_key(7, 5, 3, 12345)
    assert int(ref.window_keys(7, 5, 3, r, c)) == 12345


def test_threshold_ious_from_fractions():
    """A 10 x 10 window s columns off its box: IoU (10 - s) / (10 + s) exactly; the double the kernel's operation sequence
    gives for s = 2 is V2, with s = 1 above and s = 3 below it -- and the neighbouring doubles of V2 lie strictly between."""
    box = md.cell_box(5)
    exact = {}
    for s in (1, 2, 3):
        r, c = md.off_box(5, s)
        w = ref.record_boxes(np.array([0]), [r], [c], [1.0], md.M, md.N)[0]
        exact[s] = Fraction(10 - s, 10 + s)
        assert iou_exact(w, box) == float(exact[s]) == ref.iou_table(w, [box])[0, 0]
    assert float(exact[2]) == md.V2
    lo, hi = np.nextafter(md.V2, 0.0), np.nextafter(md.V2, 1.0)
    assert Fraction(float(exact[3])) < Fraction(lo) < Fraction(md.V2) < Fraction(hi) < Fraction(float(exact[1]))
    # an overlap of nothing is exactly 0, and a window on its own box exactly 1
    assert ref.iou_table(ref.record_boxes(np.array([0]), [0], [0], [1.0], md.M, md.N), [md.cell_box(9)])[0, 0] == 0.0


@pytest.mark.parametrize("name", list(md.scenes()))
def test_statement_gives_what_was_planted(name):
    s = md.scenes()[name]
    got = s.reference()
    assert md.chosen_of(got["rows"]) == s.expect
    rows = got["rows"]
    assert np.array_equal(rows, ref.ordered(rows))
    assert len(md.chosen_of(rows)) == len(rows)


@pytest.mark.parametrize("name", list(md.scenes()))
def test_emulated_kernel_agrees_with_the_statement(name):
    s = md.scenes()[name]
    assert md.emulate_select(s).tobytes() == s.reference()["rows"].tobytes()


def test_scenes_cover_the_cases():
    sc = md.scenes()
    assert [sc[f"sized-{n}"].det.size for n in md.SIZES] == list(md.SIZES)
    labels = lambda name: sorted({v[0] for v in sc[name].expect.values()})
    assert labels("owners") == [ref.FP, ref.TP] and labels("owners-no-tp") == [ref.FP] and labels("owners-no-fp") == [ref.TP]
    assert sc["owners-no-tp-no-fp"].expect == {}
    # a window hit for both classes: FP wins, TP once FP is not wanted
    both, tp_only = sc["owners-both"], sc["owners-both-no-fp"]
    key = (0, 0) + md.off_box(0, 1)
    assert both.expect[key] == (ref.FP, 0) and tp_only.expect[key] == (ref.TP, 0)
    # select: H = 0, K - 1, K, K + 1 at levels 0 .. 3 of image 0
    s = sc["select-fp-K4"]
    H = lambda b, l: int(((s.det["image"] == b) & (s.det["level"] == l)).sum())
    assert [H(0, l) for l in range(4)] == [0, 3, 4, 5]
    keys = s.reference()["keys"]
    at = (s.det["image"] == 0) & (s.det["level"] == 3)
    assert len({int(k) >> 8 for k in keys[at]}) == 1                    # they differ in the last digit only
    at = (s.det["image"] == 1) & (s.det["level"] == 0)
    assert {0, 0xFFFFFFFF} <= {int(k) for k in keys[at]}
    # the same windows in three groups, other winners in each
    trio = [(2, 0), (2, 1), (3, 1)]
    pos = [{(r, c) for (b, l, r, c) in s.expect if (b, l) == g} for g in trio]
    every = [{(int(w["r"]), int(w["c"])) for w in s.det if (int(w["image"]), int(w["level"])) == g} for g in trio]
    assert every[0] == every[1] == every[2] and all(len(p) == 4 for p in pos)
    assert not (pos[0] & pos[1]) and not (pos[1] & pos[2]) and not (pos[0] & pos[2])


def test_digit_select_is_the_k_smallest():
    rng = np.random.default_rng(3)
    for H, K in ((1, 1), (5, 0), (5, 5), (5, 6), (300, 1), (300, 299), (2000, 100)):
        keys = np.unique(rng.integers(0, 1 << 32, H).astype(np.uint64))
        lim = md.digit_select(keys, K)
        assert int((keys < lim).sum()) == min(K, keys.size)


@pytest.mark.parametrize("fault", md.SELECT_FAULTS)
def test_every_select_fault_is_caught(fault):
    s = md.scenes()[md.CAUGHT_BY[fault]]
    want = s.reference()["rows"]
    assert md.emulate_select(s).tobytes() == want.tobytes()
    assert md.emulate_select(s, (fault,)).tobytes() != want.tobytes(), f"{fault} goes unnoticed on {s.name}"


@pytest.mark.parametrize("name", list(md.gather_scenes()))
def test_gather_statement_and_emulation(name):
    g = md.gather_scenes()[name]
    want, err = g.expect()
    got, got_err = ref.gather(g.buf, g.stride, g.levels, g.C, g.rows, g.m, g.n)
    assert got_err == err == 1 and np.array_equal(got, want) and got.dtype == want.dtype
    emu, emu_err = md.emulate_gather(g)
    assert emu_err == 1 and np.array_equal(emu, want)
    # corners with r + m == u and c + n == v are there
    lv = g.levels[g.rows["level"][:-1]]
    assert ((g.rows["r"][:-1] + g.m == lv["u"]) & (g.rows["c"][:-1] + g.n == lv["v"])).any()
    for fault in md.GATHER_FAULTS:
        bad, _ = md.emulate_gather(g, (fault,))
        assert not np.array_equal(bad, want), f"{fault} goes unnoticed on {name}"


def test_the_binding_mirrors_the_statement_layouts():
    from waldboost_amd import _native as nat
    assert nat.MINE_ROW_DTYPE == ref.ROW and nat.MINE_LEVEL_DTYPE == ref.LEVEL and nat.DET_DTYPE == ref.DET
    assert {"wb_mine_scratch_bytes", "wb_mine_select_launch", "wb_mine_gather_launch"} <= set(nat.SYMBOLS)
    assert len(nat.SYMBOLS["wb_mine_select_launch"][1]) == 25 and len(nat.SYMBOLS["wb_mine_gather_launch"][1]) == 14
    assert nat.WB_ABI_VERSION == 8


def test_label_boxes_agrees_with_the_statement_without_choice():
    """samples.label_boxes (the host labelling that stays) on the owners scene with caps nothing reaches: the same labels and
    owners as the statement, image by image."""
    from waldboost_amd.boxes import Boxes
    from waldboost_amd.samples import label_boxes
    s = md.scenes()["owners"]
    got = s.reference()
    for b in range(s.n_images):
        at = np.flatnonzero(s.det["image"] == b)
        bx = Boxes(ref.record_boxes(s.det["level"][at], s.det["r"][at], s.det["c"][at], s.inv_scale, s.m, s.n))
        gt = None
        if s.gts[b] is not None:
            gt = Boxes(s.gts[b])
            gt.set_field("ignore", s.ignores[b])
        label_boxes(bx, gt, max_tp_candidates=10 ** 9, max_fp_candidates=10 ** 9)
        assert np.array_equal(bx.get_field("tp_label"), got["label"][at]) and np.array_equal(bx.get_field("instance_id"), got["owner"][at])


def test_fault_list_is_long_enough():
    assert len(md.SELECT_FAULTS) + len(md.GATHER_FAULTS) >= 12
    assert set(md.CAUGHT_BY) == set(md.SELECT_FAULTS)
