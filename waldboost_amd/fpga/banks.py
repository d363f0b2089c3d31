"""Pixel banks of the FPGA flavour (reference fpga/banks.py): the features a tree may test at each depth are
restricted to one memory bank of a repeating block pattern, so that trees evaluated in parallel never collide."""
from itertools import count

import numpy as np


def _bank_pattern(shape, block_shape):
    """Bank id of every feature of a (H, W) or (H, W, C) window: `block_shape` blocks of ids 0 .. prod - 1, tiled."""
    assert len(shape) in [2, 3], "Shape must be (H,W) or (H,W,C)"
    if len(shape) == 2:
        shape += (1,)
    b = np.arange(np.prod(block_shape)).reshape(block_shape)
    n = np.ceil(np.array(shape[:2]) / block_shape)
    banks = np.tile(b, n.astype("i").tolist())
    u, v, c = shape
    banks = np.atleast_3d(np.dstack([banks] * c))
    return banks[:u, :v, ...]


class PixelBanks:
    def __init__(self, shape, block_shape):
        self.pattern = _bank_pattern(shape, block_shape)

    def bank_pixels(self, bank_ids):
        """Flat feature indices of the banks `bank_ids`, bank by bank."""
        return np.concatenate([np.flatnonzero(self.pattern == b) for b in bank_ids])


class BankScheduler:
    def __init__(self, n_banks=8):
        self.n_banks = n_banks
        self.bank_counter = count()

    def schedule(self, max_depth=2):
        """One single-bank list per tree depth, round robin over the banks from call to call."""
        return [[next(self.bank_counter) % self.n_banks] for _ in range(max_depth)]
