"""CPU tests of the packed device block's layout (_native.block_layout): offsets in the order given, nothing padded, a part
without bytes, and the assertion that names the part an order leaves misaligned."""
import numpy as np
import pytest

from waldboost_amd import _native as nat

PARTS = dict(doubles=np.zeros((3, 4), np.float64), levels=np.zeros(2, nat.LEVEL_DTYPE), ints=np.zeros(3, np.int32), flags=np.zeros(5, np.uint8))


def test_offsets_of_a_mixed_list():
    assert nat.LEVEL_DTYPE.itemsize == 64
    offsets, total = nat.block_layout(**PARTS)
    assert offsets == dict(doubles=0, levels=96, ints=224, flags=236) and total == 241
    assert list(offsets) == list(PARTS)


def test_a_part_without_bytes_takes_none_and_moves_nothing():
    for nothing in (np.zeros(0, np.float64), np.zeros((0, 4), np.float32), ((0, 4), np.float64)):
        offsets, total = nat.block_layout(doubles=PARTS["doubles"], levels=PARTS["levels"], nothing=nothing, ints=PARTS["ints"], flags=PARTS["flags"])
        assert offsets == dict(doubles=0, levels=96, nothing=224, ints=224, flags=236) and total == 241
    # ... wherever it lies: behind five bytes a row of doubles would not be aligned, no row of them is
    assert nat.block_layout(flags=PARTS["flags"], nothing=np.zeros((0, 4), np.float64)) == (dict(flags=0, nothing=5), 5)


def test_an_order_that_breaks_alignment_names_the_part():
    with pytest.raises(AssertionError) as e:
        nat.block_layout(flags=PARTS["flags"], doubles=PARTS["doubles"], levels=PARTS["levels"], ints=PARTS["ints"])
    assert "'doubles'" in str(e.value) and "byte 5" in str(e.value) and "16-byte aligned" in str(e.value)
    with pytest.raises(AssertionError) as e:                                     # one double a row: 8 bytes are what it needs
        nat.block_layout(ints=PARTS["ints"], one=np.zeros(2, np.float64))
    assert "'one'" in str(e.value) and "8-byte aligned" in str(e.value)
    assert nat.block_layout(ints=np.zeros(2, np.int32), one=np.zeros(2, np.float64))[0] == dict(ints=0, one=8)


def test_float4_rows_behind_an_odd_number_of_ints():
    """wb_vote_launch reads boxes and writes merged boxes as float4: 16 bytes, whatever lies in front."""
    with pytest.raises(AssertionError) as e:
        nat.block_layout(votes=np.zeros(3, np.int32), merged=np.zeros((3, 4), np.float32))
    assert "'merged'" in str(e.value) and "byte 12" in str(e.value) and "16-byte aligned" in str(e.value)
    assert nat.block_layout(votes=np.zeros(4, np.int32), merged=np.zeros((3, 4), np.float32)) == (dict(votes=0, merged=16), 64)
    assert nat.block_layout(merged=np.zeros((3, 4), np.float32), votes=np.zeros(3, np.int32)) == (dict(merged=0, votes=48), 60)


def test_output_specs_lay_out_like_arrays():
    specs = {k: (v.shape, v.dtype) for k, v in PARTS.items()}
    assert nat.block_layout(**specs) == nat.block_layout(**PARTS)
    assert nat.block_layout(ints=(3, np.int32), flags=(5, "uint8")) == nat.block_layout(ints=PARTS["ints"], flags=PARTS["flags"])
    with pytest.raises(AssertionError):
        nat.block_layout(flags=(5, np.uint8), doubles=((3, 4), np.float64))
