"""CPU: the BatchNorm - add - ReLU entry points (csrc/batchnorm.hip, usot_bn_add_desc) are declared, exported and bound without
joining the frozen `hip.EXPORTS`; the launchers reject bad descriptors before they touch a device and leave every output as it
was; the bindings, the autograd function and the holders of the backbone and the neck have no CPU fallback; the closed forms of
the header are the gradients of the float64 restatement (tests/backbone_cases.py); and that restatement is the reference's own
`ResNet_plus2` and `AdjustLayer` (tests/golden/backbone_train.npz)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import backbone_cases as bk
import batchnorm_cases as bc
import head_grad_cases as hc
from backbone_cases import rel_err
from sampling import N_SAMPLES
from usot_amd import autograd as hip_autograd, build, hip
from usot_amd.net import BackboneSlots, BottleneckSlots, ConvSlot, NeckSlots, NormSlot, ResNetPlus2Slots, _seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_batchnorm_add_fwd_f32', 'usot_batchnorm_add_bwd_f32')
BN_PTRS = ('x', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'save_mean', 'save_invstd', 'dy', 'dx', 'dgamma', 'dbeta', 'ws')
OUTS = ('y', 'save_mean', 'save_invstd', 'running_mean', 'running_var', 'dx', 'dgamma', 'dbeta', 'ws', 'dres')
M_, C_ = 6, 8


class Host(object):
    """16-byte aligned host arrays behind every pointer of a descriptor, filled with a pattern: a launcher that answers
    USOT_EINVAL must leave them as they are (and a launcher that went on would fail its launch, not crash: no device here)"""

    def __init__(self):
        self.raw = {p: np.full(M_ * C_ + 4, 7.25, np.float32) for p in BN_PTRS + ('res', 'dres')}

    def addr(self, p):
        a = self.raw[p].ctypes.data
        return a + (-a) % 16

    def desc(self, **kw):
        args = dict(M=M_, C=C_, training=True, act=hip.ACT_RELU, **{p: self.addr(p) for p in self.raw})
        args.update(kw)
        return hip.bn_add_desc(**args)

    def untouched(self):
        return all(bool((a == 7.25).all()) for a in self.raw.values())


def both(d):
    L = hip.lib()
    return L.usot_batchnorm_add_fwd_f32(None, ctypes.byref(d)), L.usot_batchnorm_add_bwd_f32(None, ctypes.byref(d))


def test_symbols_declared_bound_and_not_in_exports():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    L = ctypes.CDLL(build.build(force=False))
    for s in SYMS:
        assert re.search(r'\bint\s+%s\s*\(\s*void\s*\*\s*stream\s*,\s*const\s+usot_bn_add_desc\s*\*' % s, text), s
        assert hasattr(L, s), s
        assert s not in hip.EXPORTS
        assert getattr(hip.lib(), s).argtypes == [ctypes.c_void_p, ctypes.c_void_p], s
    L.usot_abi_version.restype = ctypes.c_int
    assert L.usot_abi_version() == 6
    with open(os.path.join(ROOT, 'tests', 'golden', 'hip_argtypes.json')) as f:
        pinned = json.load(f)
    names = pinned if isinstance(pinned, list) else list(pinned)
    for s in SYMS:
        assert s not in json.dumps(names)
    for name in ('BnAddDesc', 'bn_add_desc', 'batch_norm_add_forward', 'batch_norm_add_backward'):
        assert hasattr(hip, name)
    assert hasattr(hip_autograd, 'BatchNormAddFunction') and hasattr(hip_autograd, 'batch_norm_add')


def test_descriptor_mirror_matches_the_header():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    m = re.search(r'typedef\s+struct\s+usot_bn_add_desc\s*\{(.*?)\}', text, flags=re.S)
    decls = [re.sub(r'\s+', ' ', d.strip()) for d in m.group(1).split(';') if d.strip()]
    assert decls == ['usot_bn_desc bn', 'const float *res', 'float *dres']
    assert [f[0] for f in hip.BnAddDesc._fields_] == ['bn', 'res', 'dres'] and hip.BnAddDesc._fields_[0][1] is hip.BnDesc
    assert ctypes.sizeof(hip.BnDesc) == 136                             # usot_bn_desc is ABI: unchanged
    assert hip.BnAddDesc.bn.offset == 0 and hip.BnAddDesc.res.offset == 136 and hip.BnAddDesc.dres.offset == 144
    assert ctypes.sizeof(hip.BnAddDesc) == 152


def test_bn_add_desc_round_trip():
    d = hip.bn_add_desc(M=189, C=64, eps=1e-3, momentum=0.2, training=False, act=hip.ACT_RELU, slices=3, x=16, gamma=32, beta=48,
                        running_mean=64, running_var=80, y=96, dy=112, dx=128, res=144, dres=160)
    assert (d.bn.M, d.bn.C, d.bn.training, d.bn.act, d.bn.slices) == (189, 64, 0, hip.ACT_RELU, 3)
    assert abs(d.bn.eps - 1e-3) < 1e-9 and abs(d.bn.momentum - 0.2) < 1e-7
    assert (d.bn.x, d.bn.gamma, d.bn.beta, d.bn.running_mean, d.bn.running_var, d.bn.y, d.bn.dy, d.bn.dx) == (16, 32, 48, 64, 80, 96, 112, 128)
    assert d.bn.save_mean is None and d.bn.ws is None and d.bn.dgamma is None
    assert (d.res, d.dres) == (144, 160)
    e = hip.bn_add_desc(M=4, C=4)
    assert e.res is None and e.dres is None and e.bn.training == 1 and e.bn.x is None
    # the workspace is the plain descriptor's
    assert hip.lib().usot_batchnorm_ws_floats(ctypes.byref(d.bn)) == 2 * 3 * 64


BAD = [dict(C=0), dict(C=2), dict(C=6), dict(C=-4), dict(M=0), dict(M=-3), dict(M=1, training=True), dict(slices=-1),
       dict(M=5, slices=6), dict(eps=-1.0), dict(eps=float('nan')), dict(momentum=float('inf')), dict(act=2), dict(act=-1)]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '_'.join('%s%s' % kv for kv in b.items()).replace(' ', ''))
def test_bad_descriptors_are_rejected_without_a_device(bad):
    h = Host()
    assert both(h.desc(**bad)) == (-1, -1)
    assert h.untouched()


def test_missing_and_misaligned_pointers_are_rejected_without_a_device():
    L, h = hip.lib(), Host()
    fwd = lambda **kw: L.usot_batchnorm_add_fwd_f32(None, ctypes.byref(h.desc(**kw)))
    bwd = lambda **kw: L.usot_batchnorm_add_bwd_f32(None, ctypes.byref(h.desc(**kw)))
    assert L.usot_batchnorm_add_fwd_f32(None, None) == -1 and L.usot_batchnorm_add_bwd_f32(None, None) == -1
    d = h.desc()
    d.bn.training = 2
    assert both(d) == (-1, -1)
    for missing in ('x', 'gamma', 'beta', 'y', 'save_mean', 'save_invstd', 'ws', 'res'):
        assert fwd(**{missing: None}) == -1, missing
    for missing in ('x', 'gamma', 'beta', 'y', 'running_mean', 'running_var', 'res'):
        assert fwd(training=False, **{missing: None}) == -1, missing
    for missing in ('x', 'gamma', 'beta', 'dy', 'save_mean', 'save_invstd', 'ws', 'res'):
        assert bwd(**{missing: None}) == -1, missing
    for missing in ('x', 'gamma', 'dy', 'running_mean', 'running_var', 'ws', 'res'):
        assert bwd(training=False, **{missing: None}) == -1, missing
    assert bwd(act=hip.ACT_NONE, res=None) == -1                               # required although only the mask reads it
    assert bwd(training=True, dgamma=None, dbeta=None, ws=None) == -1          # training-mode dx needs the sums
    for p in ('x', 'gamma', 'beta', 'y', 'save_mean', 'save_invstd', 'ws', 'running_mean', 'running_var', 'res', 'dres'):
        assert fwd(**{p: h.addr(p) + 4}) == -1, p
    for p in ('x', 'gamma', 'beta', 'dy', 'dx', 'dgamma', 'dbeta', 'ws', 'save_mean', 'save_invstd', 'res', 'dres'):
        assert bwd(**{p: h.addr(p) + 8}) == -1, p
    for p in ('running_mean', 'running_var', 'res', 'dres'):
        assert bwd(training=False, **{p: h.addr(p) + 4}) == -1, p
    # a backward call that wants nothing is an error here (the plain entry point calls it a no-op)
    for training in (True, False):
        assert bwd(training=training, dx=None, dgamma=None, dbeta=None, dres=None) == -1
    assert h.untouched()


@pytest.mark.parametrize('grad', [False, True])
def test_no_cpu_fallback(grad):
    x, gamma, beta, rmean, rvar, dy, res = bk.operands(bc.CASES[1], 2)
    with pytest.raises(hip.HipError):
        hip.batch_norm_add_forward(x, res, gamma, beta, rmean, rvar, training=True)
    with pytest.raises(hip.HipError):
        hip.batch_norm_add_backward(dy, x, res, gamma, beta, rmean, rvar, None, None, training=True)
    for training in (True, False):
        with pytest.raises(hip.HipError):
            hip_autograd.batch_norm_add(bc.nchw(x).requires_grad_(grad), bc.nchw(res), gamma, beta, rmean, rvar, training)
    with pytest.raises(hip.HipError):
        NormSlot(36)(bc.nchw(x), relu=True, residual=bc.nchw(res))
    ds = _seq(ConvSlot(32, 128, 3, stride=2), NormSlot(128))
    mods = [(BottleneckSlots(128, 32), torch.zeros(1, 128, 5, 5)), (BottleneckSlots(32, 32, stride=2, downsample=ds), torch.zeros(1, 32, 5, 5)),
            (NeckSlots(64, 32), torch.zeros(1, 64, 9, 9)), (ResNetPlus2Slots((1, 1, 1)), torch.zeros(1, 3, 31, 31)),
            (BackboneSlots(), torch.zeros(1, 3, 31, 31))]
    for mod, inp in mods:
        if not isinstance(mod, (ResNetPlus2Slots, BackboneSlots)):           # the stem's parameters stay frozen: its own guard
            for p_ in mod.parameters():
                p_.requires_grad_(grad)
        for m in (mod.train(), mod.eval()):
            if isinstance(m, ResNetPlus2Slots):
                m.bn1.eval()
            if isinstance(m, BackboneSlots):
                m.features.bn1.eval()
            with pytest.raises(hip.HipError):
                m(inp)
    with pytest.raises(hip.HipError):
        NeckSlots(64, 32, pr_pool=True)(torch.zeros(1, 64, 9, 9), crop=True, pr_pool=True, bbox=torch.zeros(1, 4))


def test_bindings_reject_bad_shapes_before_any_launch(monkeypatch):
    monkeypatch.setattr(hip, '_dev', lambda t, dtype=torch.float32: t)
    monkeypatch.setattr(hip, 'lib', lambda: pytest.fail('the library was called'))
    x, gamma, beta, rmean, rvar, dy, res = bk.operands(bc.CASES[1], 2)
    bad = [lambda: hip.batch_norm_add_forward(x, res[:, :-1], gamma, beta, rmean, rvar, training=True),
           lambda: hip.batch_norm_add_forward(x, res[..., :32].contiguous(), gamma, beta, rmean, rvar, training=True),
           lambda: hip.batch_norm_add_forward(x[..., :-1], res[..., :-1], gamma, beta, rmean, rvar, training=True),      # not dense
           lambda: hip.batch_norm_add_forward(x, res, gamma[:-4], beta, rmean, rvar, training=True),
           lambda: hip.batch_norm_add_backward(dy[:, :-1], x, res, gamma, beta, rmean, rvar, None, None, training=True),
           lambda: hip.batch_norm_add_backward(dy, x, res[:, :-1], gamma, beta, rmean, rvar, None, None, training=True),
           lambda: hip.batch_norm_add_backward(dy, x, res, gamma, beta, rmean, rvar, None, None, training=True, need=(0, 0, 0, 0)),
           lambda: hip_autograd.batch_norm_add(bc.nchw(x), bc.nchw(res)[:, :, :-1], gamma, beta, rmean, rvar, True),
           lambda: hip_autograd.batch_norm_add(bc.nchw(x), bc.nchw(res), gamma[:-4], beta, rmean, rvar, True),
           lambda: hip_autograd.batch_norm_add(bc.nchw(x), bc.nchw(res), gamma, beta, None, None, False)]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError):
            fn()
            pytest.fail('case %d was accepted' % i)


def test_stem_guard_names_the_recipe(monkeypatch):
    monkeypatch.setattr(hip, '_dev', lambda t, dtype=torch.float32: t)
    monkeypatch.setattr(hip, 'lib', lambda: pytest.fail('the library was called'))
    img = torch.zeros(1, 3, 31, 31)
    net = ResNetPlus2Slots((1, 1, 1))
    cases = [lambda n: n.train(), lambda n: n.eval().conv1.weight.requires_grad_(True), lambda n: n.eval().bn1.weight.requires_grad_(True),
             lambda n: n.eval().bn1.bias.requires_grad_(True)]
    for prepare in cases:
        net = ResNetPlus2Slots((1, 1, 1))
        prepare(net)
        with pytest.raises(NotImplementedError, match=r"stem's gradients.*bn1\.eval\(\).*frozen"):
            net(img)
    with pytest.raises(NotImplementedError, match=r"stem's gradients"):
        ResNetPlus2Slots((1, 1, 1)).eval()(img.clone().requires_grad_(True))


close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('c', bc.CASES[:3], ids=bc.case_id)
def test_closed_forms_are_the_float64_gradients(c, training, relu):
    """relu(pre + r): dres = dy * (s > 0), and dx / dgamma / dbeta are plain BatchNorm's with that dy'"""
    ops = bk.operands(c, 2)
    fw = bk.add_forward_of(ops, training)
    s = fw['s'].detach()
    ref = bk.add_grads_of(fw, ops[5], (s > 0) if relu else None)
    ch = c[3]
    flat = lambda t: t.double().reshape(-1, ch)
    y, dx, dg, db, dr = bk.add_formulas(flat(ops[0]), ops[1].double(), ops[2].double(), fw['save_mean'], fw['save_invstd'], flat(ops[6]),
                                        flat(ops[5]), training, relu)
    assert close(y, flat(s.clamp(min=0) if relu else s))
    for got, want in zip((dx, dg, db, dr), ref):
        assert close(got, want.reshape(got.shape))
    assert close(dr, flat(ops[5]) * (flat(s) > 0).double() if relu else flat(ops[5]))
    assert 0.2 < float((s > 0).double().mean()) < 0.8                          # the residual does move the mask


def test_pool_restatement_is_the_exact_oracle():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import prroi_exact
    f = bk.feature_map(2, 8, 15, seed=3).double() - 0.5
    rois = torch.cat((torch.arange(2.0).view(-1, 1), bk.boxes(2, 15)), 1).double()
    fg = f.clone().requires_grad_(True)
    out = bk.prroi_pool(fg, rois)
    assert close(out.detach(), torch.from_numpy(prroi_exact.prroi_pool_exact(f.numpy(), rois.numpy(), 7, 7, 1.0)))
    g = torch.cos(torch.arange(out.numel(), dtype=torch.float64)).reshape(out.shape)
    back, = torch.autograd.grad(out, fg, g)
    assert close(back, torch.from_numpy(prroi_exact.prroi_pool_exact_backward(tuple(f.shape), rois.numpy(), g.numpy(), 7, 7, 1.0)))


@pytest.fixture(scope='module')
def fixture():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'backbone_train.npz')) as z:
        return {k: z[k] for k in z.files}


def against(fixture, key, t, errs):
    errs[key] = rel_err(hc.sampled(key, t, N_SAMPLES), fixture[key])
    mean = float(fixture[key + '#mean'])
    assert abs(float(t.detach().double().mean()) - mean) <= 1e-6 * float(t.detach().double().abs().mean()) + 1e-12, key


def test_fixture_is_small_and_holds_the_seeded_inputs(fixture):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'backbone_train.npz')) < 512 * 1024
    assert fixture['in/image'].dtype == np.float32 and np.array_equal(fixture['in/image'], bk.image(2, 63).numpy())
    assert np.array_equal(fixture['in/boxes'], bk.boxes(2, 15).numpy())
    assert np.array_equal(fixture['in/map'], hc.sampled('in/map', bk.feature_map(2, 1024, 15), N_SAMPLES).astype(np.float32))
    assert not any('weight' in k and '/grad/' not in k for k in fixture)      # no parameters are stored


def test_restatement_is_the_reference_backbone_in_the_training_configuration(fixture):
    """float64 on both sides; the fixture stores float32, so the difference is its rounding: 1e-6 (the project's scaled error)"""
    net = ResNetPlus2Slots(bk.GOLD_LAYERS)
    state = bk.module_state(net, 'features.features.', seed=bk.GOLD_SEED)
    params = hc.leaves_of(state)
    ref = bk.BackboneRef(params, training=True)
    res = ref.resnet(torch.from_numpy(fixture['in/image']).double(), bk.GOLD_LAYERS)
    named_out = bk.named_backbone(res)
    errs = {}
    for name, t in named_out:
        against(fixture, 'backbone/out/' + name, t, errs)
    loss = hc.fixed_loss(named_out[1:])
    assert abs(float(loss.detach()) - float(fixture['backbone/loss'])) <= 1e-9 * abs(float(fixture['backbone/loss']))
    named = [(k, v) for k, v in params.items() if hc.is_param(k) and not k.startswith(('conv1.', 'bn1.'))]
    assert {k for k, _ in named} == {k.split('/', 2)[2] for k in fixture if k.startswith('backbone/grad/') and '#' not in k}
    for (name, _), g in zip(named, torch.autograd.grad(loss, [t for _, t in named])):
        against(fixture, 'backbone/grad/' + name, g, errs)
    worst = max(errs, key=errs.get)
    print('backbone: %d tensors, worst %s %.3g' % (len(errs), worst, errs[worst]))
    assert errs[worst] <= 1e-6, (worst, errs[worst])
    assert ref.names == ['layer1.0.bn1', 'layer1.0.bn2', 'layer1.0.downsample.1', 'layer1.0.bn3', 'layer2.0.bn1', 'layer2.0.bn2',
                         'layer2.0.downsample.1', 'layer2.0.bn3', 'layer3.0.bn1', 'layer3.0.bn2', 'layer3.0.downsample.1', 'layer3.0.bn3']
    for n in ref.names:                                  # training mode moved layer1-3's statistics once; the stem's stayed
        assert int(params[n + '.num_batches_tracked']) == 1 and not torch.equal(params[n + '.running_mean'], state[n + '.running_mean'].double())
    assert int(params['bn1.num_batches_tracked']) == 0 and torch.equal(params['bn1.running_mean'], state['bn1.running_mean'].double())


@pytest.mark.parametrize('form', bk.NECK_FORMS)
def test_restatement_is_the_reference_neck_in_training_mode(form, fixture):
    state = bk.module_state(NeckSlots(1024, 256, pr_pool=True), 'neck.', seed=bk.GOLD_SEED)
    params = hc.leaves_of(state)
    x = bk.feature_map(2, 1024, 15).double().requires_grad_(True)
    ref = bk.BackboneRef(params, training=True)
    named_out = bk.named_neck(ref.neck(x, **bk.neck_args(form, torch.from_numpy(fixture['in/boxes']).double())))
    assert [tuple(t.shape) for _, t in named_out] == [(2, 256, 15, 15)] + ([(2, 256, 7, 7)] if form != 'plain' else [])
    errs = {}
    for name, t in named_out:
        against(fixture, 'neck/%s/out/%s' % (form, name), t, errs)
    loss = hc.fixed_loss(named_out)
    assert abs(float(loss.detach()) - float(fixture['neck/%s/loss' % form])) <= 1e-9 * abs(float(fixture['neck/%s/loss' % form]))
    named = [('x', x)] + [(k, v) for k, v in params.items() if hc.is_param(k)]
    for (name, _), g in zip(named, torch.autograd.grad(loss, [t for _, t in named])):
        against(fixture, 'neck/%s/grad/%s' % (form, name), g, errs)
    worst = max(errs, key=errs.get)
    print('neck %s: %d tensors, worst %s %.3g' % (form, len(errs), worst, errs[worst]))
    assert errs[worst] <= 1e-6, (worst, errs[worst])


def test_state_dict_keys_and_exports_are_unchanged():
    from usot_amd.model import USOT
    with open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_keys.json')) as f:
        want = json.load(f)
    keys = list(USOT().state_dict().keys())
    assert len(keys) == 444 and sorted(keys) == sorted(want if isinstance(want, list) else list(want))
    assert USOT().neck.pr_pool is True and USOT({'mem_size': 4, 'pr_pool': False}).neck.pr_pool is False
    assert not any(s in hip.EXPORTS for s in SYMS)
    with pytest.raises(NotImplementedError):
        USOT()(torch.zeros(1, 3, 127, 127))
