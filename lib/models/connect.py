"""reference lib/models/connect.py — neck / head parameter trees and `xcorr_depthwise`.  `matrix`, `GroupDW`, `Conf_Fusion`,
`box_tower_reg` and `AdjustLayer` (its three call forms: plain, crop, crop + PrRoIPool) run `forward` and back-propagate on the
HIP kernels (usot_amd.autograd, lib.models.prroi_pool)."""
from usot_amd.autograd import xcorr_depthwise  # noqa: F401  (connect.py:147-157, HIP plane kernels, differentiable)
from usot_amd.net import (ConfFusionSlots as Conf_Fusion, EncoderSlots as matrix,  # noqa: F401
                          GroupDWSlots as GroupDW, HeadSlots as box_tower_reg, NeckSlots as AdjustLayer)
