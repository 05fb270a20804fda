"""Parameter tree of the USOT Siamese tracker, state-dict compatible with the reference.

The classes below hold tensors under the same names the reference registers them (444 state-dict keys, see
reference lib/models/models.py:298-306, modules.py:61-135, connect.py:12-74,
104-121, 160-219, 284-292) and record each convolution's geometry so that
`usot_amd.engine` can lower the graph to HIP launches.  There is deliberately no torch fallback for the tensor math.
Every holder's `forward` hands its tensors to the differentiable HIP bindings of `usot_amd.autograd` (device tensors only):
`GroupDWSlots`, `ConvSlot` and `NormSlot` (with `conv_norm`, which chains the latter two over one conv - BN [- ReLU] holder),
the head's holders built from them - `EncoderSlots`, `ConfFusionSlots` and `HeadSlots` (the reference's `matrix`, `Conf_Fusion`
and `box_tower_reg`) - and the backbone and the neck: `BottleneckSlots` (its tail bn3 - add - ReLU is one kernel pair,
`autograd.batch_norm_add`), `ResNetPlus2Slots`, `BackboneSlots` and `NeckSlots` (`Bottleneck`, `ResNet_plus2`, `ResNet50`,
`AdjustLayer`).  The stem (conv1 - bn1 - ReLU - max-pool) runs frozen, as the reference's recipe always runs it: its own
gradients are not built.  Only the whole model's `forward` (usot_amd/model.py) still raises.  The inference engine does not
come through any `forward` here: it keeps lowering the folded graph.
"""
import torch
import torch.nn as nn


class ConvSlot(nn.Module):
    """Weight (and optional bias) of one convolution plus its geometry."""

    def __init__(self, cin, cout, k, stride=1, pad=0, dil=1, bias=False):
        super().__init__()
        kh, kw = (k, k) if isinstance(k, int) else k
        self.cin, self.cout, self.kh, self.kw = cin, cout, kh, kw
        self.stride = stride
        self.pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
        self.dil = (dil, dil) if isinstance(dil, int) else tuple(dil)
        self.weight = nn.Parameter(torch.zeros(cout, cin, kh, kw), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        else:
            self.register_parameter('bias', None)

    def out_hw(self, h, w):
        oh = (h + 2 * self.pad[0] - self.dil[0] * (self.kh - 1) - 1) // self.stride + 1
        ow = (w + 2 * self.pad[1] - self.dil[1] * (self.kw - 1) - 1) // self.stride + 1
        return oh, ow

    def forward(self, x):
        """The bare convolution (no BatchNorm, no activation) of an NCHW device tensor; differentiable
        (usot_amd.autograd.conv2d).  The engine does not come through here: it lowers the folded graph to HIP launches."""
        from . import autograd
        return autograd.conv2d(x, self.weight, self.bias, self.stride, self.pad, self.dil)


class NormSlot(nn.Module):
    """BatchNorm2d affine + running statistics.  The engine folds them into the conv banks; `forward` is the differentiable
    operator, in the module's own mode."""

    eps = 1e-5
    momentum = 0.1

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer('running_mean', torch.zeros(c))
        self.register_buffer('running_var', torch.ones(c))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))

    def forward(self, x, relu=False, residual=None):
        """nn.BatchNorm2d (and, with `relu`, the ReLU behind it) of an NCHW device tensor; differentiable
        (usot_amd.autograd.batch_norm).  With a `residual` of x's shape the result is [relu](bn(x) + residual), one kernel
        (usot_amd.autograd.batch_norm_add).  self.training chooses batch or running statistics; a training-mode call moves the
        running statistics and counts itself in num_batches_tracked, all on the device."""
        from . import autograd
        args = (self.weight, self.bias, self.running_mean, self.running_var, self.training, self.momentum, self.eps, relu)
        y = autograd.batch_norm(x, *args) if residual is None else autograd.batch_norm_add(x, residual, *args)
        if self.training:
            self.num_batches_tracked.add_(1)
        return y


class _Gap(nn.Module):
    """Occupies the index a ReLU has in the reference's nn.Sequential."""

    def forward(self, *a, **k):
        raise RuntimeError('placeholder')


def _seq(*mods):
    return nn.Sequential(*mods)


def conv_norm(seq, x):
    """Run a `_seq(ConvSlot, NormSlot[, _Gap])` holder as the reference runs its nn.Sequential: conv -> BN, with the ReLU
    fused into the BN kernel iff the `_Gap` is there.  Differentiable; NCHW device tensors."""
    if len(seq) not in (2, 3) or not isinstance(seq[0], ConvSlot) or not isinstance(seq[1], NormSlot) \
            or (len(seq) == 3 and not isinstance(seq[2], _Gap)):
        raise TypeError('conv_norm: a (ConvSlot, NormSlot[, _Gap]) sequence expected')
    return seq[1](seq[0](x), relu=len(seq) == 3)


class BottleneckSlots(nn.Module):
    """reference modules.py:11-58 (geometry rules :18-27)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        pad = 2 - stride
        if downsample is not None and dilation > 1:
            dilation //= 2
            pad = dilation
        if dilation > 1:
            pad = dilation
        self.conv1 = ConvSlot(inplanes, planes, 1)
        self.bn1 = NormSlot(planes)
        self.conv2 = ConvSlot(planes, planes, 3, stride=stride, pad=pad, dil=dilation)
        self.bn2 = NormSlot(planes)
        self.conv3 = ConvSlot(planes, planes * 4, 1)
        self.bn3 = NormSlot(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        """reference modules.py:37-58 on an NCHW device tensor, differentiable, in the module's mode: conv1 - bn1 - ReLU,
        conv2 - bn2 - ReLU, conv3, then relu(bn3(.) + residual) as one kernel, the residual being x or the downsample's
        conv - BN of it."""
        out = self.bn1(self.conv1(x), relu=True)
        out = self.bn2(self.conv2(out), relu=True)
        residual = x if self.downsample is None else conv_norm(self.downsample, x)
        return self.bn3(self.conv3(out), relu=True, residual=residual)


class ResNetPlus2Slots(nn.Module):
    """reference modules.py:61-135 with layers=[3,4,6,3], used_layers=[3]."""

    def __init__(self, layers=(3, 4, 6)):
        super().__init__()
        self.inplanes = 64
        self.conv1 = ConvSlot(3, 64, 7, stride=2, pad=0)
        self.bn1 = NormSlot(64)
        self.layer1 = self._stage(64, layers[0])
        self.layer2 = self._stage(128, layers[1], stride=2)
        self.layer3 = self._stage(256, layers[2], stride=1, dilation=2)

    def _stage(self, planes, blocks, stride=1, dilation=1):
        ds = None
        if stride != 1 or self.inplanes != planes * 4:
            if stride == 1 and dilation == 1:
                ds = _seq(ConvSlot(self.inplanes, planes * 4, 1), NormSlot(planes * 4))
            else:
                pad = dilation // 2 if dilation > 1 else 0
                ds = _seq(ConvSlot(self.inplanes, planes * 4, 3, stride=stride, pad=pad),
                          NormSlot(planes * 4))
        blks = [BottleneckSlots(self.inplanes, planes, stride, ds, dilation)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            blks.append(BottleneckSlots(self.inplanes, planes, dilation=dilation))
        return _seq(*blks)

    def _stem(self):
        """conv1 with bn1's running statistics folded in, float64 as `engine.Weights` folds it: the [147][64] bank and the bias
        that carries the STEM_MU offset of the stem kernel.  Cached on the versions of the five tensors."""
        from .engine import Weights
        ts = (self.conv1.weight, self.bn1.weight, self.bn1.bias, self.bn1.running_mean, self.bn1.running_var)
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if getattr(self, '_stem_key', None) != key:
            w, g, b, rm, rv = (t.detach().double().cpu() for t in ts)
            s = g / torch.sqrt(rv + self.bn1.eps)
            bank = (w * s.view(-1, 1, 1, 1)).permute(1, 2, 3, 0)
            mu = torch.tensor(Weights.STEM_MU, dtype=torch.float64).view(3, 1, 1, 1)
            dev = self.conv1.weight.device
            self._stem_fold = (bank.reshape(147, 64).float().contiguous().to(dev),
                               (b - rm * s + (bank * mu).sum((0, 1, 2))).float().to(dev))
            self._stem_key = key
        return self._stem_fold

    def forward(self, x):
        """reference modules.py:137-151 on an NCHW device image -> ([x_, p1, p2], p3), NCHW-shaped over channels-last memory.
        layer1-3 are differentiable in their own modes.  The stem runs as the reference's recipe always runs it
        (train_usot.py: stem parameters frozen, bn1.eval()): the folded stem kernel, then the max-pool kernel, no graph."""
        from . import hip
        from .engine import Weights
        hip._dev(x)
        if self.bn1.training or x.requires_grad or any(p.requires_grad for p in (self.conv1.weight, self.bn1.weight, self.bn1.bias)):
            raise NotImplementedError("the stem's gradients (7x7 conv with Cin = 3, max-pool) are not built: run the "
                                      'reference recipe - bn1.eval(), stem parameters frozen (conv1.weight, bn1.weight and '
                                      'bn1.bias without requires_grad), an image that does not require grad')
        bank, bias = self._stem()
        stem = hip.stem_conv(x.detach().contiguous(), bank, bias, Weights.STEM_MU)
        x_ = stem.permute(0, 3, 1, 2)
        p1 = self.layer1(hip.maxpool3x3s2(stem).permute(0, 3, 1, 2))
        p2 = self.layer2(p1)
        p3 = self.layer3(p2)
        return [x_, p1, p2], p3


class BackboneSlots(nn.Module):
    """reference backbones.py:12-22 — adds the extra `features.` level to the keys."""

    def __init__(self):
        super().__init__()
        self.features = ResNetPlus2Slots()

    def forward(self, x):
        """reference backbones.py:20-22 -> (x_stages, x)"""
        x_stages, x = self.features(x)
        return x_stages, x


class NeckSlots(nn.Module):
    """reference connect.py:284-292 (AdjustLayer)."""

    def __init__(self, cin=1024, cout=256, pr_pool=False):
        super().__init__()
        self.downsample = _seq(ConvSlot(cin, cout, 1), NormSlot(cout))
        self.pr_pool = bool(pr_pool)         # the reference registers a parameter-free PrRoIPool2D(7, 7, 1.0) here: no key

    def forward(self, x, crop=False, pr_pool=False, bbox=None):
        """reference connect.py:294-314 on an NCHW device tensor, differentiable, in the module's mode: the 1x1 conv - BN;
        with `crop` also the [4:-4] centre (a view), or with `pr_pool` the 7 x 7 PrRoIPool at scale 1.0 of `bbox` [N, 4]
        (one box per map; the batch index is prepended on the device)."""
        x_ori = conv_norm(self.downsample, x)
        if not crop:
            return x_ori
        if not pr_pool:
            return x_ori, x_ori[:, :, 4:-4, 4:-4]
        if not self.pr_pool:
            raise AttributeError('AdjustLayer was built without pr_pool')
        from lib.models.prroi_pool.functional import prroi_pool2d
        index = torch.arange(0, x.shape[0], device=x.device, dtype=torch.float32).view(-1, 1)
        return x_ori, prroi_pool2d(x_ori, torch.cat((index, bbox), dim=1), 7, 7, 1.0)


class EncoderSlots(nn.Module):
    """reference connect.py:12-53 (`matrix`): three parallel 3x3 valid convs per side."""

    GEOMS = (('matrix11', (1, 1)), ('matrix12', (2, 1)), ('matrix21', (1, 2)))

    def __init__(self, cin=256, cout=256):
        super().__init__()
        for name, dil in self.GEOMS:
            for side in ('k', 's'):
                self.add_module('%s_%s' % (name, side),
                                _seq(ConvSlot(cin, cout, 3, dil=dil), NormSlot(cout), _Gap()))

    def forward(self, z=None, x=None):
        """reference connect.py:55-74 on NCHW device tensors: the three encodings of the template `z` and of the search map
        `x`, each side None when its input is; differentiable (conv_norm).  All three convs of a side read the side's input,
        as the reference's do.  The engine does not come through here."""
        zs = xs = None
        if x is not None:
            xs = [conv_norm(getattr(self, name + '_s'), x) for name, _ in self.GEOMS]
        if z is not None:
            zs = [conv_norm(getattr(self, name + '_k'), z) for name, _ in self.GEOMS]
        return zs, xs


class GroupDWSlots(nn.Module):
    """reference connect.py:82-84: three branch logits, softmax-ed at use."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(3), requires_grad=False)

    def forward(self, z, x):
        """reference connect.py:86-102 on triples of NCHW device tensors; differentiable (usot_amd.autograd.groupdw).  The
        inference engine does not come through here: it runs the fused NHWC kernel on this parameter."""
        from . import autograd
        return autograd.groupdw(z, x, self.weight)


class ConfFusionSlots(nn.Module):
    """reference connect.py:109-121."""

    def __init__(self, c=256):
        super().__init__()
        self.conf_gen = _seq(ConvSlot(c, c, 3, pad=1, bias=True), NormSlot(c), _Gap())
        self.value_gen = _seq(ConvSlot(c, c, 3, pad=1, bias=True), NormSlot(c), _Gap())

    def forward(self, x):
        """reference connect.py:123-144: `x` [B, M, C, H, W] on the device -> [B, C, H, W]; the two conv - BN - ReLU branches
        over the [B*M, C, H, W] view, then the fusion kernel (usot_amd.autograd.conf_fusion).  Differentiable."""
        from . import autograd
        batch, mem_size, channel, h, w = x.shape
        x = x.reshape(-1, channel, h, w)
        return autograd.conf_fusion(conv_norm(self.conf_gen, x), conv_norm(self.value_gen, x), batch, mem_size)


def _tower(c, n):
    mods = []
    for _ in range(n):
        mods += [ConvSlot(c, c, 3, pad=1, bias=True), NormSlot(c), _Gap()]
    return _seq(*mods)


def _run_tower(seq, x):
    """a `_tower` holder as the reference runs it: conv - BN - ReLU per stage"""
    for i in range(0, len(seq), 3):
        x = conv_norm(seq[i:i + 3], x)
    return x


class HeadSlots(nn.Module):
    """reference connect.py:160-219 (`box_tower_reg`)."""

    def __init__(self, c=256, tower_num=4):
        super().__init__()
        self.cls_encode = EncoderSlots(c, c)
        self.reg_encode = EncoderSlots(c, c)
        self.cls_dw = GroupDWSlots()
        self.reg_dw = GroupDWSlots()
        self.conf_fusion = ConfFusionSlots(c)
        self.bbox_tower = _tower(c, tower_num)
        self.cls_tower = _tower(c, tower_num)
        self.cls_memory_tower = _tower(c, tower_num)
        self.bbox_pred = ConvSlot(c, 4, 3, pad=1, bias=True)
        self.cls_pred = ConvSlot(c, 1, 3, pad=1, bias=True)
        self.cls_memory_pred = ConvSlot(c, 1, 3, pad=1, bias=True)
        self.adjust = nn.Parameter(0.1 * torch.ones(1), requires_grad=False)
        self.bias = nn.Parameter(torch.ones(1, 4, 1, 1), requires_grad=False)

    def forward(self, search, kernel=None, memory_kernel=None, memory_confidence=None, cls_x_store=None):
        """reference connect.py:221-281 on NCHW device tensors, differentiable, in the module's mode; the same three call
        forms and five-tuple results (None when neither kernel is given).  Only `memory_confidence.shape` is read (a CPU
        tensor is fine).  Nothing in the call waits for the device besides GroupDW's copy of its three branch weights."""
        from . import autograd
        if kernel is not None:
            cls_z, cls_x = self.cls_encode(kernel, search)
            reg_z, reg_x = self.reg_encode(kernel, search)
            cls_dw = self.cls_dw(cls_z, cls_x)
            reg_dw = self.reg_dw(reg_z, reg_x)
            x_bbox = autograd.box_exp(self.bbox_pred(_run_tower(self.bbox_tower, reg_dw)), self.adjust, self.bias)
            cls = 0.1 * self.cls_pred(_run_tower(self.cls_tower, cls_dw))
            if memory_kernel is None:
                return x_bbox, cls, cls_x, reg_x, None
        if memory_kernel is not None:
            if cls_x_store is None:
                cls_mem_zs, cls_x_store = self.cls_encode(memory_kernel, x=search)
            else:
                cls_mem_zs, _ = self.cls_encode(memory_kernel, x=None)
            batch, mem_size = memory_confidence.shape
            store_repeat = []
            for t in cls_x_store:
                _, c, h, w = t.shape
                store_repeat.append(t.view(batch, 1, c, h, w).repeat(1, mem_size, 1, 1, 1).view(-1, c, h, w))
            cls_mem_dw = self.cls_dw(cls_mem_zs, store_repeat)
            _, c, h, w = cls_mem_dw.shape
            cls_mem = 0.1 * self.cls_memory_pred(_run_tower(self.cls_memory_tower,
                                                            self.conf_fusion(cls_mem_dw.reshape(batch, mem_size, c, h, w))))
            if kernel is not None:
                # the reference's loop variable leaves `cls_x` bound to the last encoded map here; no caller reads the third
                # result of the combined call, and the encoded list is what the offline form returns
                return x_bbox, cls, cls_x, reg_x, cls_mem
            return None, None, None, None, cls_mem
        return None
