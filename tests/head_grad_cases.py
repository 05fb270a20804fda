"""Shared by test_head_grad_host.py, test_gpu_head_grad.py and golden/make_golden_head_train.py: the shapes and seeded operands of the
head-gradient tests, and a PyTorch-CPU restatement - written from torch.nn.functional, float64 unless asked otherwise - of
Conf_Fusion's fusion, the box epilogue, and the forward passes of the reference's `matrix`, `Conf_Fusion` and `box_tower_reg`
(connect.py:55-74, 123-144, 221-281).

Masks.  A ReLU or clamp mask formed in float32 and one formed in float64 differ on elements within rounding of the threshold, and
one flipped element is an O(1) error of a gradient.  `HeadRef` therefore takes the device's own BatchNorm - ReLU outputs, layer
by layer in call order (`outs`): layer k's ReLU becomes a multiplication by outs[k] > 0, and Conf_Fusion's clamp passes a
gradient where the device's conf map lies in [-6, 4].  Without `outs` the restatement forms its own masks.  Plain helper module."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from batchnorm_cases import rel_err  # noqa: F401  (the project's scaled error; re-exported)

EPS, MOMENTUM = 1e-5, 0.1
GEOMS = (('matrix11', (1, 1)), ('matrix12', (2, 1)), ('matrix21', (1, 2)))

# ---- raw Conf_Fusion: (B, M, P, C) ---------------------------------------------------------------------------------------------
CF_CASES = [
    (1, 1, 1, 4),            # one lane; M = 1: every weight is 1 and dconf is 0
    (2, 3, 7, 8),            # 28 lanes: the lane count ends inside the only workgroup
    (1, 7, 81, 36),          # the tracker's seven memory slots, nine lanes per pixel: 729 lanes, 2 workgroups and a tail
    (3, 4, 25, 256),         # 4 800 lanes: 18 whole workgroups and three quarters of one (the grid is not capped: no second trip)
]


def cf_id(c):
    return 'b%d_m%d_p%d_c%d' % c


def cf_operands(c, seed=0):
    """float32 CPU tensors conf, value [B*M, P, C] and dout [B, P, C].  conf spreads over the clamp's whole range (some below
    -6, some above 4); its first elements are planted: == 4.0, > 4, == 0, and with room == -6.0 and < -6."""
    b, m, p, ch = c
    g = torch.Generator().manual_seed(104729 * (b * 131 + m) + 7 * p + ch + seed)
    conf = 3.0 * torch.randn(b * m, p, ch, generator=g)
    flat = conf.view(-1)
    planted = [4.0, 5.5, 0.0] + ([-6.0, -7.5, 4.0] if flat.numel() >= 8 else [])
    for i, v in enumerate(planted):
        flat[(i * 5) % flat.numel() if flat.numel() >= 8 else i] = v
    value = torch.randn(b * m, p, ch, generator=g).abs() * 1.5
    dout = torch.randn(b, p, ch, generator=g)
    return conf, value, dout


def conf_fusion_ref(conf, value, batch, mem_size, pass_mask=None):
    """connect.py:129-142 behind the two branches: conf, value [B*M, ...] -> [B, ...].  pass_mask (bool, conf's shape): where
    the clamp passes a gradient; None: torch.clamp's own rule."""
    c = conf.reshape(batch, mem_size, *conf.shape[1:])
    if pass_mask is None:
        cl = torch.clamp(c, max=4, min=-6)
    else:
        cl = c.detach().clamp(max=4, min=-6) + (c - c.detach()) * pass_mask.reshape(c.shape).to(c.dtype)
    e = torch.exp(cl)
    w = e / e.sum(dim=1, keepdim=True)
    return (w * value.reshape(c.shape)).sum(dim=1)


def conf_fusion_formulas(conf, value, dout, batch, mem_size):
    """the header's closed forms on float64 tensors -> (out, dconf, dvalue)"""
    c, v = conf.reshape(batch, mem_size, *conf.shape[1:]), value.reshape(batch, mem_size, *conf.shape[1:])
    e = torch.exp(c.clamp(min=-6, max=4))
    w = e / e.sum(1, keepdim=True)
    out = (w * v).sum(1)
    g = dout.unsqueeze(1)
    dvalue = w * g
    dconf = ((c >= -6) & (c <= 4)).to(c.dtype) * w * (v - out.unsqueeze(1)) * g
    return out, dconf.reshape(conf.shape), dvalue.reshape(conf.shape)


# ---- raw box-exp ------------------------------------------------------------------------------------------------------------------
def box_operands(rows, seed=0):
    """float32 CPU tensors p [R, 4], adjust [1], bias [1, 4, 1, 1], dy [R, 4]: log-boxes around 3.4 as usot_amd.synth makes them"""
    g = torch.Generator().manual_seed(6007 * rows + seed)
    p = 5.0 * torch.randn(rows, 4, generator=g)
    adjust = torch.tensor([0.1]) + 0.01 * torch.randn(1, generator=g)
    bias = (3.4 + 0.25 * torch.randn(4, generator=g)).view(1, 4, 1, 1)
    dy = torch.randn(rows, 4, generator=g)
    return p, adjust, bias, dy


def box_exp_ref(p, adjust, bias):
    """connect.py:236-237: p [..., 4] rows (bias viewed as [4]) or NCHW [N, 4, H, W] (bias [1, 4, 1, 1])"""
    return torch.exp(adjust * p + (bias if p.dim() == 4 else bias.reshape(4)))


def box_exp_formulas(p, adjust, bias, dy):
    """the header's closed forms on float64 [R, 4] tensors -> (y, dp, dadjust, dbias, |terms| of dadjust, |terms| of dbias)"""
    y = torch.exp(adjust * p + bias.reshape(4))
    g = dy * y
    return y, adjust * g, (g * p).sum().reshape(1), g.sum(0), (g * p).abs().sum(), g.abs().sum(0)


# ---- the modules -----------------------------------------------------------------------------------------------------------------
HEAD_C, BATCH, MEM, ZK, XS = 32, 2, 3, 7, 15
GOLD_SEED = 5                # parameters of tests/golden/head_train.npz (golden/make_golden_head_train.py)


def module_state(module, prefix, seed=0, stats=False):
    """float32 CPU state dict for a holder of usot_amd.net (or the reference's module of the same keys) from usot_amd.synth's
    rules; `prefix` places it in the reference's tree (e.g. 'connect_model.').  stats: running statistics away from (0, 1), so
    that eval mode is not the identity."""
    from usot_amd import synth
    shapes = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = synth.make_state_dict(shapes, seed, calibrated=False)
    out = {k[len(prefix):]: torch.from_numpy(np.ascontiguousarray(v)).reshape(shapes[k]) for k, v in sd.items()}
    if stats:
        g = torch.Generator().manual_seed(977 + seed)
        for k in sorted(out):
            if k.endswith('running_mean'):
                out[k] = 0.2 * torch.randn(out[k].shape, generator=g)
            elif k.endswith('running_var'):
                out[k] = 0.6 + 0.8 * torch.rand(out[k].shape, generator=g)
    return out


def head_inputs(seed=0, c=HEAD_C):
    """float32 CPU search map, template, memory templates and the (CPU) confidence table whose shape the head reads"""
    g = torch.Generator().manual_seed(31337 + seed)
    return dict(search=torch.randn(BATCH, c, XS, XS, generator=g), kernel=torch.randn(BATCH, c, ZK, ZK, generator=g),
                memory_kernel=torch.randn(BATCH * MEM, c, ZK, ZK, generator=g), memory_confidence=torch.ones(BATCH, MEM))


FORMS = ('offline', 'memory', 'both')


def form_args(form, inp):
    """(search, kernel, memory_kernel, memory_confidence) of a call form"""
    off, mem = form != 'memory', form != 'offline'
    return (inp['search'], inp['kernel'] if off else None, inp['memory_kernel'] if mem else None,
            inp['memory_confidence'] if mem else None)


def flat_outputs(res):
    """the five-tuple of box_tower_reg.forward -> [(name, tensor)] of the maps it holds"""
    names = ('x_bbox', 'cls', 'cls_x', 'reg_x', 'cls_mem')
    out = []
    for n, r in zip(names, res):
        if isinstance(r, (list, tuple)):
            out += [('%s%d' % (n, i), t) for i, t in enumerate(r)]
        elif r is not None:
            out.append((n, r))
    return out


@functools.lru_cache(maxsize=None)
def _loss_weight(shape, k):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + k).reshape(shape)


def fixed_loss(named):
    """the fixed scalar of the module tests: sum_k <map_k, cos(0.37 i + k)> over the maps of flat_outputs, in their order"""
    return sum((t * _loss_weight(tuple(t.shape), k).to(device=t.device, dtype=t.dtype)).sum() for k, (_, t) in enumerate(named))


def loss_outputs(form, res):
    """the maps the fixed loss runs over.  In the combined call the reference's third result is not the encoded list but the
    map its loop variable was last bound to (connect.py:260); no caller reads it, and it stays out of the loss."""
    if form == 'both':
        res = (res[0], res[1], None, res[3], res[4])
    return flat_outputs(res)


def sampled(name, t, n=1024):
    """what tests/golden/head_train.npz keeps of a tensor: all of it up to n elements, else n seeded sample points"""
    a = t.detach().cpu().double().numpy().reshape(-1)
    if a.size > n:
        from sampling import sample_index
        a = a[sample_index(name, a.size, n)]
    return a


def xcorr(x, kernel):
    """connect.py:147-157"""
    b, c, hk, wk = kernel.shape
    out = F.conv2d(x.reshape(1, b * c, x.shape[2], x.shape[3]), kernel.reshape(b * c, 1, hk, wk), groups=b * c)
    return out.reshape(b, c, out.shape[2], out.shape[3])


class HeadRef(object):
    """The restated modules over a dict of tensors keyed like the state dict (`prefix` + key); parameters may require grad, the
    BatchNorm buffers are updated in place as nn.BatchNorm2d updates them.  Records per BatchNorm, in call order: `names` (the
    state-dict path of the BatchNorm), `pres` (its output before the ReLU, detached) and `convs` (its input, kept in the
    graph: the gradient of a conv bias in front of a training-mode BatchNorm is a cancelling sum, judged against
    sum |d loss / d conv output|)."""

    def __init__(self, params, training, outs=None, tower_num=1):
        self.p, self.training, self.outs, self.tower_num = params, training, outs, tower_num
        self.names, self.pres, self.convs, self.conf_maps = [], [], [], []

    def conv(self, key, x, padding=0, dilation=1):
        return F.conv2d(x, self.p[key + '.weight'], self.p.get(key + '.bias'), padding=padding, dilation=dilation)

    def conv_bn_relu(self, ckey, bkey, x, padding=0, dilation=1):
        conv = self.conv(ckey, x, padding, dilation)
        pre = F.batch_norm(conv, self.p[bkey + '.running_mean'], self.p[bkey + '.running_var'], self.p[bkey + '.weight'],
                           self.p[bkey + '.bias'], self.training, MOMENTUM, EPS)
        if self.training:
            self.p[bkey + '.num_batches_tracked'] += 1
        k = len(self.names)
        self.names.append(bkey)
        self.pres.append(pre.detach())
        self.convs.append(conv)
        return F.relu(pre) if self.outs is None else pre * (self.outs[k] > 0).to(pre.dtype)

    def matrix(self, prefix, z=None, x=None):
        zs = xs = None
        if x is not None:
            xs = [self.conv_bn_relu('%s%s_s.0' % (prefix, n), '%s%s_s.1' % (prefix, n), x, 0, d) for n, d in GEOMS]
        if z is not None:
            zs = [self.conv_bn_relu('%s%s_k.0' % (prefix, n), '%s%s_k.1' % (prefix, n), z, 0, d) for n, d in GEOMS]
        return zs, xs

    def groupdw(self, key, zs, xs):
        w = F.softmax(self.p[key + '.weight'], 0)
        s = 0
        for i in range(3):
            s = s + w[i] * xcorr(xs[i], zs[i])
        return s

    def conf_fusion(self, prefix, x):
        batch, mem_size, ch, h, w = x.shape
        x = x.reshape(-1, ch, h, w)
        k = len(self.names)
        conf = self.conv_bn_relu(prefix + 'conf_gen.0', prefix + 'conf_gen.1', x, 1)
        value = self.conv_bn_relu(prefix + 'value_gen.0', prefix + 'value_gen.1', x, 1)
        mask = None
        if self.outs is not None:
            dev = self.outs[k]
            mask = (dev >= -6) & (dev <= 4)
        self.conf_maps.append(k)
        return conf_fusion_ref(conf, value, batch, mem_size, mask)

    def tower(self, name, x):
        for i in range(self.tower_num):
            x = self.conv_bn_relu('%s.%d' % (name, 3 * i), '%s.%d' % (name, 3 * i + 1), x, 1)
        return x

    def head(self, search, kernel=None, memory_kernel=None, memory_confidence=None, cls_x_store=None):
        p = self.p
        if kernel is not None:
            cls_z, cls_x = self.matrix('cls_encode.', kernel, search)
            reg_z, reg_x = self.matrix('reg_encode.', kernel, search)
            cls_dw = self.groupdw('cls_dw', cls_z, cls_x)
            reg_dw = self.groupdw('reg_dw', reg_z, reg_x)
            x_bbox = box_exp_ref(self.conv('bbox_pred', self.tower('bbox_tower', reg_dw), 1), p['adjust'], p['bias'])
            cls = 0.1 * self.conv('cls_pred', self.tower('cls_tower', cls_dw), 1)
            if memory_kernel is None:
                return x_bbox, cls, cls_x, reg_x, None
        if memory_kernel is not None:
            if cls_x_store is None:
                mem_zs, cls_x_store = self.matrix('cls_encode.', memory_kernel, search)
            else:
                mem_zs, _ = self.matrix('cls_encode.', memory_kernel, None)
            batch, mem_size = memory_confidence.shape
            rep = [t.unsqueeze(1).repeat(1, mem_size, 1, 1, 1).reshape(-1, *t.shape[1:]) for t in cls_x_store]
            dw = self.groupdw('cls_dw', mem_zs, rep)
            fused = self.conf_fusion('conf_fusion.', dw.reshape(batch, mem_size, *dw.shape[1:]))
            cls_mem = 0.1 * self.conv('cls_memory_pred', self.tower('cls_memory_tower', fused), 1)
            if kernel is not None:
                return x_bbox, cls, cls_x, reg_x, cls_mem
            return None, None, None, None, cls_mem
        return None


def leaves_of(state, dtype=torch.float64):
    """state dict -> dict of `dtype` clones: floating-point parameters require grad, the BatchNorm buffers do not"""
    out = {}
    for k, v in state.items():
        if k.endswith(('running_mean', 'running_var')):
            out[k] = v.detach().to(dtype).clone()
        elif k.endswith('num_batches_tracked'):
            out[k] = v.detach().clone()
        else:
            out[k] = v.detach().to(dtype).clone().requires_grad_(True)
    return out


def is_param(k):
    return not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))


def cancelling_biases(names, training):
    """{conv bias key: indices of the calls of the BatchNorm behind it} for the convs whose bias a training-mode BatchNorm
    subtracts again (the conv sits one place in front of its BatchNorm in every holder)"""
    out = {}
    if training:
        for k, n in enumerate(names):
            stem, idx = n.rsplit('.', 1)
            out.setdefault('%s.%d.bias' % (stem, int(idx) - 1), []).append(k)
    return out
