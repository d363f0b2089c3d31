"""The reference's FPGA flavour -- drop-in for ``waldboost.fpga`` (reference fpga/__init__.py): the integer
channel functions ``grad_hist_4_u1`` and ``grad_mag_u1`` as ``channel_opts["channels"]`` (uint8 channels quarter the
cascade's HBM traffic: one dword per pixel instead of a float4), and the training side that pairs with them:
``DTree`` (the histogram tree learner, its split search a HIP kernel), ``train``, ``PixelBanks`` / ``BankScheduler``,
and ``Learner`` / ``BasicRejectionSchedule`` re-exported as the reference does.
"""
from ..channels import grad_hist_4_u1, grad_mag_u1
from ..training import BasicRejectionSchedule, Learner
from .banks import BankScheduler, PixelBanks
from .training import DTree, train

__all__ = ["grad_hist_4_u1", "grad_mag_u1", "DTree", "train", "Learner", "BasicRejectionSchedule", "PixelBanks",
           "BankScheduler"]
