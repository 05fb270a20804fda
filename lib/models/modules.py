"""reference lib/models/modules.py — Bottleneck / ResNet_plus2: parameter trees and differentiable `forward`s on the HIP kernels
(conv2d, batch_norm, and batch_norm_add for the bottleneck's bn3 - add - ReLU); ResNet_plus2's stem runs frozen."""
from usot_amd.net import BottleneckSlots as Bottleneck, ResNetPlus2Slots as ResNet_plus2  # noqa: F401
