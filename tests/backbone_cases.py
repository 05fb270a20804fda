"""Shared by test_backbone_host.py, test_gpu_backbone.py and golden/make_golden_backbone_train.py: seeded operands of the
BatchNorm - add - ReLU tests (batchnorm_cases.operands plus a residual of the map's shape), seeded parameters for the holders of
the backbone and the neck, and a PyTorch-CPU restatement - written from torch.nn.functional and the reference's construction
rules, float64 unless asked otherwise - of BN - add - ReLU, the bottleneck (modules.py:37-58), `ResNet_plus2.forward`
(modules.py:137-151) and `AdjustLayer.forward` (connect.py:294-314, with Precise RoI Pooling as the closed-form integral of the
bilinear surface, linear in the features).

Masks.  As in head_grad_cases.py: `BackboneRef` takes the device's own BatchNorm outputs, in call order (`outs`), and layer k's
ReLU becomes a multiplication by outs[k] > 0; without `outs` the restatement forms its own masks.

Parameters come from numpy.random.RandomState seeded per state-dict key (bit-stable across numpy versions, independent of the
registration order), so fixtures need not store them.  Plain helper module."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import batchnorm_cases as bc
from batchnorm_cases import rel_err  # noqa: F401  (the project's scaled error; re-exported)

EPS, MOMENTUM = 1e-5, 0.1
GOLD_SEED = 9                # parameters of tests/golden/backbone_train.npz (golden/make_golden_backbone_train.py)
GOLD_LAYERS = (1, 1, 1)


# ---- raw BN - add - ReLU ----------------------------------------------------------------------------------------------------------
def operands(c, off=0, seed=0):
    """bc.operands(c, off, seed) + (res NHWC,): the residual has the spread of the normalised map, so the sum changes sign often"""
    ops = bc.operands(c, off, seed)
    g = torch.Generator().manual_seed(15485863 * (seed + 1) + 7 * sum(c) + off)
    return ops + (torch.randn(ops[0].shape, generator=g),)


def add_forward_of(ops, training, dtype=torch.float64):
    """bc.forward_of plus the residual leaf: dict with `s` = pre + res (NHWC, in the graph) and `leaves` (x, gamma, beta, res)"""
    fw = bc.forward_of(*ops[:5], training, dtype=dtype)
    r_ = ops[6].detach().to(dtype).clone().requires_grad_(True)
    fw = dict(fw, s=fw['pre'] + r_)
    fw['leaves'] = fw['leaves'] + (r_,)
    return fw


def add_grads_of(fw, dy, mask=None):
    """(dx, dgamma, dbeta, dres) of sum(dy * y), y = s * mask (None: no ReLU), by autograd"""
    s = fw['s']
    y = s if mask is None else s * mask.to(s.dtype)
    return torch.autograd.grad(y, fw['leaves'], dy.to(s.dtype), retain_graph=True)


def add_formulas(x, gamma, beta, mean, invstd, res, dy, training, relu):
    """the header's closed forms on float64 [M, C] tensors -> (y, dx, dgamma, dbeta, dres)"""
    m = x.shape[0]
    xhat = (x - mean) * invstd
    s = xhat * gamma + beta + res
    y = s.clamp(min=0) if relu else s
    dyp = dy * (s > 0).to(dy.dtype) if relu else dy
    dbeta, dgamma = dyp.sum(0), (dyp * xhat).sum(0)
    dx = gamma * invstd * (dyp - dbeta / m - xhat * dgamma / m) if training else gamma * invstd * dyp
    return y, dx, dgamma, dbeta, dyp


# ---- parameters ---------------------------------------------------------------------------------------------------------------------
def module_state(module, prefix='', seed=0):
    """float32 CPU state dict for a holder of usot_amd.net (or the reference's module of the same keys): He-scaled conv weights,
    BN weights in +-[0.5, 1.5) (the sign changes the side of the ReLU a channel lives on), small BN biases, running statistics
    away from (0, 1) so that eval mode is not the identity.  Each tensor from RandomState(crc32(prefix + key) ^ seed)."""
    out = {}
    for k, v in module.state_dict().items():
        rs = np.random.RandomState((zlib.crc32((prefix + k).encode()) ^ (7919 * seed)) & 0x7fffffff)
        shape = tuple(v.shape)
        if k.endswith('num_batches_tracked'):
            a = np.zeros(shape, np.int64)
        elif k.endswith('running_mean'):
            a = 0.2 * rs.standard_normal(shape)
        elif k.endswith('running_var'):
            a = 0.6 + 0.8 * rs.random_sample(shape)
        elif len(shape) == 4:
            a = rs.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif k.endswith('weight'):
            a = (0.5 + rs.random_sample(shape)) * (2.0 * rs.randint(0, 2, shape) - 1.0)
        else:
            a = 0.3 * rs.standard_normal(shape)
        out[k] = torch.from_numpy(np.ascontiguousarray(a)).to(v.dtype)
    return out


def image(n, size, seed=0):
    """an [n, 3, size, size] float32 crop in raw pixel units (what the stem kernel's mean offsets are made for)"""
    rs = np.random.RandomState(4241 + seed)
    return torch.from_numpy((110.0 + 50.0 * rs.standard_normal((n, 3, size, size))).clip(0, 255).astype(np.float32))


def feature_map(n, c, size, seed=0):
    rs = np.random.RandomState(6151 + seed)
    return torch.from_numpy(np.abs(rs.standard_normal((n, c, size, size))).astype(np.float32))


def boxes(n, size, seed=0):
    """[n, 4] float32 (x1, y1, x2, y2) inside a size x size map, at least three cells wide"""
    rs = np.random.RandomState(8089 + seed)
    lo = rs.uniform(0.5, size / 2 - 2.0, (n, 2))
    hi = lo + rs.uniform(3.0, size / 2 - 1.0, (n, 2))
    return torch.from_numpy(np.concatenate([lo, hi], 1).astype(np.float32))


# ---- Precise RoI Pooling, closed form, differentiable in the features ---------------------------------------------------------------
def _hat_integral(t):
    """antiderivative of the unit hat max(0, 1 - |t|): 0 for t <= -1, 1 for t >= 1"""
    t = t.clamp(-1.0, 1.0)
    return torch.where(t < 0, 0.5 * (t + 1.0) ** 2, 1.0 - 0.5 * (1.0 - t) ** 2)


def prroi_pool(features, rois, ph=7, pw=7, scale=1.0):
    """features [B, C, H, W], rois [R, 5] = (batch, x1, y1, x2, y2) -> [R, C, ph, pw]: the mean of the zero-extended bilinear
    surface over each bin (Jiang et al., ECCV 2018, eq. 3-4); 0 for an empty bin"""
    dt = features.dtype
    _, _, h, w = features.shape
    outs = []
    for r in rois.detach().to(dt):
        x1, y1, x2, y2 = (v * scale for v in r[1:])
        bw, bh = (x2 - x1).clamp(min=0) / pw, (y2 - y1).clamp(min=0) / ph
        ys = y1 + bh * torch.arange(ph + 1, dtype=dt)
        xs = x1 + bw * torch.arange(pw + 1, dtype=dt)
        gy = _hat_integral(ys.view(-1, 1) - torch.arange(h, dtype=dt).view(1, -1))
        gx = _hat_integral(xs.view(-1, 1) - torch.arange(w, dtype=dt).view(1, -1))
        wy, wx = gy[1:] - gy[:-1], gx[1:] - gx[:-1]                  # [ph, H], [pw, W]
        area = bw * bh
        pooled = torch.einsum('ih,chw,jw->cij', wy, features[int(r[0])], wx)
        outs.append(pooled / area if float(area) > 0 else pooled * 0)
    return torch.stack(outs)


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
class BackboneRef(object):
    """The restated modules over a dict of tensors keyed like the state dict; parameters may require grad, the BatchNorm buffers
    are updated in place as nn.BatchNorm2d updates them.  Records per BatchNorm that goes through `bn`, in call order: `names`
    (its state-dict path), `pres` (its output before any ReLU - with a residual: the sum -, detached) and `relus` (whether a
    ReLU follows).  The stem's BatchNorm
    is always in eval mode and is not recorded (the holders fold it into the stem kernel)."""

    def __init__(self, params, training, outs=None):
        self.p, self.training, self.outs = params, training, outs
        self.names, self.pres, self.relus = [], [], []

    def conv(self, key, x, stride=1, padding=0, dilation=1):
        return F.conv2d(x, self.p[key + '.weight'], None, stride=stride, padding=padding, dilation=dilation)

    def bn(self, key, x, relu=False, residual=None):
        pre = F.batch_norm(x, self.p[key + '.running_mean'], self.p[key + '.running_var'], self.p[key + '.weight'],
                           self.p[key + '.bias'], self.training, MOMENTUM, EPS)
        if self.training:
            self.p[key + '.num_batches_tracked'] += 1
        s = pre if residual is None else pre + residual
        k = len(self.names)
        self.names.append(key)
        self.pres.append(s.detach())
        self.relus.append(bool(relu))
        if not relu:
            return s
        return F.relu(s) if self.outs is None else s * (self.outs[k] > 0).to(s.dtype)

    def bottleneck(self, prefix, x, stride=1, downsample=None, dilation=1):
        """modules.py:14-58; downsample: None or (kernel, stride, padding) of its conv"""
        padding = 2 - stride
        if downsample is not None and dilation > 1:
            dilation = dilation // 2
            padding = dilation
        if dilation > 1:
            padding = dilation
        out = self.bn(prefix + 'bn1', self.conv(prefix + 'conv1', x), relu=True)
        out = self.bn(prefix + 'bn2', self.conv(prefix + 'conv2', out, stride, padding, dilation), relu=True)
        residual = x
        if downsample is not None:
            k, s, p = downsample
            residual = self.bn(prefix + 'downsample.1', self.conv(prefix + 'downsample.0', x, s, p))
        return self.bn(prefix + 'bn3', self.conv(prefix + 'conv3', out), relu=True, residual=residual)

    def layer(self, prefix, x, inplanes, planes, blocks, stride=1, dilation=1):
        """modules.py:104-135 -> (output, planes * 4)"""
        ds = None
        if stride != 1 or inplanes != planes * 4:
            if stride == 1 and dilation == 1:
                ds = (1, stride, 0)
            else:
                ds = (3, stride, dilation // 2 if dilation > 1 else 0)
        x = self.bottleneck(prefix + '0.', x, stride, ds, dilation)
        for i in range(1, blocks):
            x = self.bottleneck('%s%d.' % (prefix, i), x, dilation=dilation)
        return x, planes * 4

    def resnet(self, x, layers=(3, 4, 6), prefix=''):
        """modules.py:137-151 with used_layers = [3]; the stem without a graph, its BatchNorm in eval mode"""
        p = self.p
        with torch.no_grad():
            s = F.batch_norm(F.conv2d(x, p[prefix + 'conv1.weight'], None, stride=2), p[prefix + 'bn1.running_mean'],
                             p[prefix + 'bn1.running_var'], p[prefix + 'bn1.weight'], p[prefix + 'bn1.bias'], False, MOMENTUM, EPS)
            x_ = F.relu(s)
            x = F.max_pool2d(x_, kernel_size=3, stride=2, padding=1)
        p1, c = self.layer(prefix + 'layer1.', x, 64, 64, layers[0])
        p2, c = self.layer(prefix + 'layer2.', p1, c, 128, layers[1], stride=2)
        p3, c = self.layer(prefix + 'layer3.', p2, c, 256, layers[2], stride=1, dilation=2)
        return [x_, p1, p2], p3

    def neck(self, x, crop=False, pr_pool=False, bbox=None, prefix=''):
        """connect.py:294-314"""
        x_ori = self.bn(prefix + 'downsample.1', self.conv(prefix + 'downsample.0', x))
        if not crop:
            return x_ori
        if not pr_pool:
            return x_ori, x_ori[:, :, 4:-4, 4:-4]
        index = torch.arange(0, x.shape[0], dtype=bbox.dtype).view(-1, 1)
        return x_ori, prroi_pool(x_ori, torch.cat((index, bbox), dim=1), 7, 7, 1.0)


NECK_FORMS = ('plain', 'crop', 'pool')


def neck_args(form, bbox=None):
    return dict(plain={}, crop=dict(crop=True), pool=dict(crop=True, pr_pool=True, bbox=bbox))[form]


def named_neck(res):
    return [('x_ori', res)] if not isinstance(res, tuple) else [('x_ori', res[0]), ('xf', res[1])]


def named_backbone(res):
    (x_, p1, p2), p3 = res
    return [('x_', x_), ('p1', p1), ('p2', p2), ('p3', p3)]
