"""reference lib/models/connect.py — neck / head parameter trees and `xcorr_depthwise`.  `matrix`, `GroupDW`, `Conf_Fusion` and
`box_tower_reg` run `forward` and back-propagate on the HIP kernels (usot_amd.autograd); `AdjustLayer` only holds parameters."""
from usot_amd.autograd import xcorr_depthwise  # noqa: F401  (connect.py:147-157, HIP plane kernels, differentiable)
from usot_amd.net import (ConfFusionSlots as Conf_Fusion, EncoderSlots as matrix,  # noqa: F401
                          GroupDWSlots as GroupDW, HeadSlots as box_tower_reg, NeckSlots as AdjustLayer)
