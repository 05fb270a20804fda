"""reference lib/models/backbones.py:12-22 — ResNet50(used_layers=[3]): parameter tree and `forward` -> (x_stages, x).  layer1-3
run and back-propagate on the HIP kernels; the stem runs frozen (bn1.eval(), stem parameters without requires_grad), as the
reference's training recipe runs it - its own gradients are not built."""
from usot_amd.net import BackboneSlots as ResNet50  # noqa: F401
