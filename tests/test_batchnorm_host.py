"""CPU: the batch-norm entry points (csrc/batchnorm.hip) are declared, exported and bound; the launchers reject bad descriptors
before they touch a device; the differentiable surface (autograd.batch_norm, net.NormSlot, net.conv_norm) has no CPU fallback;
and the float64 reference the GPU tests lean on is the operator the header defines."""
import ctypes
import os
import re

import pytest
import torch

import batchnorm_cases as bc
from usot_amd import autograd as hip_autograd, build, hip
from usot_amd.net import ConvSlot, NormSlot, _Gap, _seq, conv_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_batchnorm_fwd_f32', 'usot_batchnorm_bwd_f32', 'usot_batchnorm_ws_floats', 'usot_batchnorm_slices',
        'usot_batchnorm_geometry')
ONE = 16                                               # an address that is never dereferenced on the paths tested here
PTRS = ('x', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'save_mean', 'save_invstd', 'dy', 'dx', 'dgamma', 'dbeta', 'ws')


def desc(M=1875, C=256, **kw):
    args = dict(M=M, C=C, training=True, **{p: ONE for p in PTRS})
    args.update(kw)
    return hip.bn_desc(**args)


def test_batchnorm_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    L = ctypes.CDLL(build.build(force=False))
    for s in SYMS:
        assert re.search(r'\b(int|int64_t)\s+%s\s*\(' % s, text), s
        assert s in hip.EXPORTS
        assert hasattr(L, s), s
        assert hasattr(hip.lib(), s)
    L.usot_abi_version.restype = ctypes.c_int
    assert L.usot_abi_version() == 6                    # symbols were added, no signature changed
    # the ctypes mirror has the header's fields, in its order
    m = re.search(r'typedef\s+struct\s+usot_bn_desc\s*\{(.*?)\}', text, flags=re.S)
    names = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(float|int32_t)\s*', '', decl).split(',')]
    assert names == [f[0] for f in hip.BnDesc._fields_]
    assert set(PTRS) == set(names[:13])
    assert ctypes.sizeof(hip.BnDesc) == 13 * 8 + 7 * 4 + 4              # padded to the pointers' alignment
    for name in ('BnDesc', 'bn_desc', 'batch_norm_forward', 'batch_norm_backward', 'batchnorm_geometry'):
        assert hasattr(hip, name)
    assert hasattr(hip_autograd, 'BatchNormFunction') and hasattr(hip_autograd, 'batch_norm')


def test_geometry_slices_and_workspace_queries():
    L = hip.lib()
    R, CB = hip.batchnorm_geometry()
    assert R > 0 and R % 4 == 0 and CB >= 4 and CB % 4 == 0
    for ps in (1, 2, 3, 7):
        d = desc(slices=ps)
        assert L.usot_batchnorm_slices(ctypes.byref(d)) == ps
        assert L.usot_batchnorm_ws_floats(ctypes.byref(d)) == 2 * ps * 256
    for c in bc.CASES:
        m = c[0] * c[1] * c[2]
        for training in (True, False):
            d = desc(M=m, C=c[3], training=training)
            auto = L.usot_batchnorm_slices(ctypes.byref(d))
            steps = -(-m // R)
            assert 1 <= auto <= max(1, steps // 2), (c, auto)           # no automatic slice below two row steps
            assert L.usot_batchnorm_ws_floats(ctypes.byref(d)) == 2 * auto * c[3]
    assert L.usot_batchnorm_slices(ctypes.byref(desc(M=3 * R - 1, slices=3 * R - 1))) == 3 * R - 1    # slices without a row step


BAD = [dict(C=0), dict(C=2), dict(C=6), dict(C=255), dict(C=-4), dict(M=0), dict(M=-3), dict(M=1, training=True),
       dict(slices=-1), dict(M=5, slices=6), dict(eps=-1.0), dict(eps=float('nan')), dict(act=2), dict(act=-1)]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '_'.join('%s%s' % kv for kv in b.items()).replace(' ', ''))
def test_bad_descriptors_are_rejected_without_a_device(bad):
    L = hip.lib()
    d = desc(**bad)
    assert L.usot_batchnorm_fwd_f32(None, ctypes.byref(d)) == -1
    assert L.usot_batchnorm_bwd_f32(None, ctypes.byref(d)) == -1
    assert L.usot_batchnorm_slices(ctypes.byref(d)) == -1
    assert L.usot_batchnorm_ws_floats(ctypes.byref(d)) == -1


def test_training_flag_outside_0_1_is_rejected():
    L = hip.lib()
    d = desc()
    d.training = 2
    assert L.usot_batchnorm_fwd_f32(None, ctypes.byref(d)) == -1 and L.usot_batchnorm_bwd_f32(None, ctypes.byref(d)) == -1


def test_missing_and_misaligned_pointers_are_rejected_without_a_device():
    L = hip.lib()
    fwd = lambda **kw: L.usot_batchnorm_fwd_f32(None, ctypes.byref(desc(**kw)))
    bwd = lambda **kw: L.usot_batchnorm_bwd_f32(None, ctypes.byref(desc(**kw)))
    assert L.usot_batchnorm_fwd_f32(None, None) == -1 and L.usot_batchnorm_bwd_f32(None, None) == -1
    assert L.usot_batchnorm_slices(None) == -1 and L.usot_batchnorm_ws_floats(None) == -1
    for missing in ('x', 'gamma', 'beta', 'y', 'save_mean', 'save_invstd', 'ws'):
        assert fwd(**{missing: None}) == -1, missing
    for missing in ('x', 'gamma', 'beta', 'y', 'running_mean', 'running_var'):
        assert fwd(training=False, **{missing: None}) == -1, missing
    for missing in ('x', 'gamma', 'dy', 'save_mean', 'save_invstd', 'ws'):
        assert bwd(**{missing: None}) == -1, missing
    assert bwd(act=hip.ACT_RELU, beta=None) == -1                            # the mask is recomputed: it needs beta
    for missing in ('x', 'gamma', 'dy', 'running_mean', 'running_var', 'ws'):
        assert bwd(training=False, **{missing: None}) == -1, missing
    for p in ('x', 'gamma', 'beta', 'y', 'save_mean', 'ws'):
        assert fwd(**{p: ONE + 4}) == -1, p
    for p in ('x', 'dy', 'dx', 'dgamma', 'dbeta', 'save_invstd'):
        assert bwd(**{p: ONE + 4}) == -1, p
    # a backward call that wants nothing is a no-op; M = 1 is a map in eval mode only
    assert bwd(dx=None, dgamma=None, dbeta=None) == 0
    assert L.usot_batchnorm_slices(ctypes.byref(desc(M=1, training=False))) == 1


@pytest.mark.parametrize('grad', [False, True])
def test_no_cpu_fallback_on_the_differentiable_surface(grad):
    x = torch.zeros(2, 8, 5, 5, requires_grad=grad)
    w, b = torch.ones(8, requires_grad=grad), torch.zeros(8, requires_grad=grad)
    rm, rv = torch.zeros(8), torch.ones(8)
    for training in (True, False):
        with pytest.raises(hip.HipError):
            hip_autograd.batch_norm(x, w, b, rm, rv, training)
    for slot in (NormSlot(8).train(), NormSlot(8).eval()):                   # was: the holder's RuntimeError('parameter holder')
        slot.weight.requires_grad_(grad)
        with pytest.raises(hip.HipError):
            slot(x)
        with pytest.raises(hip.HipError):
            slot(x, relu=True)
        assert int(slot.num_batches_tracked) == 0
    seq = _seq(ConvSlot(32, 40, 3, pad=1, bias=True), NormSlot(40), _Gap())
    with pytest.raises(hip.HipError):
        conv_norm(seq, torch.zeros(1, 32, 9, 9))
    with pytest.raises(TypeError):
        conv_norm(_seq(NormSlot(40), _Gap()), torch.zeros(1, 40, 9, 9))
    with pytest.raises(RuntimeError):
        _Gap()(x)                                                            # still a placeholder
    xh = torch.zeros(2, 5, 5, 8)
    with pytest.raises(hip.HipError):
        hip.batch_norm_forward(xh, w.detach(), b.detach(), rm, rv, training=True)
    with pytest.raises(hip.HipError):
        hip.batch_norm_backward(xh, xh, w.detach(), b.detach(), rm, rv, None, None, training=True)


def formulas(x, gamma, beta, rmean, rvar, dy, training, relu):
    """the header's definitions on float64 [M][C] arrays -> (y, mean, invstd, new running mean / var, dx, dgamma, dbeta)"""
    M = x.shape[0]
    mean = x.mean(0) if training else rmean
    var = ((x - mean) ** 2).mean(0) if training else rvar
    invstd = 1.0 / torch.sqrt(var + bc.EPS)
    xhat = (x - mean) * invstd
    pre = xhat * gamma + beta
    y = pre.clamp(min=0) if relu else pre
    dyp = dy * (pre > 0) if relu else dy
    dbeta, dgamma = dyp.sum(0), (dyp * xhat).sum(0)
    dx = gamma * invstd * (dyp - dbeta / M - xhat * dgamma / M) if training else gamma * invstd * dyp
    if training:
        rmean = (1 - bc.MOMENTUM) * rmean + bc.MOMENTUM * mean
        rvar = (1 - bc.MOMENTUM) * rvar + bc.MOMENTUM * var * M / (M - 1)
    return y, mean, invstd, rmean, rvar, dx, dgamma, dbeta


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('c,off', [(bc.CASES[1], 2), (bc.CASES[2], 0), (bc.CASES[2], 32)], ids=lambda v: str(v).replace(' ', ''))
def test_float64_reference_is_the_definition(c, off, training, relu):
    ops, fw = bc.reference(c, off, training)
    x, gamma, beta, rmean, rvar, dy = ops
    ch = c[3]
    y, mean, invstd, rm, rv, dx, dgamma, dbeta = formulas(x.double().reshape(-1, ch), gamma.double(), beta.double(), rmean.double(),
                                                          rvar.double(), dy.double().reshape(-1, ch), training, relu)
    pre = fw['pre'].detach()
    mask = (pre > 0) if relu else None
    gx, gg, gb = bc.grads_of(fw, dy, mask)
    ref_y = pre.clamp(min=0) if relu else pre
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))
    assert close(y, ref_y.reshape(-1, ch))
    assert close(mean, fw['save_mean']) and close(invstd, fw['save_invstd'])
    assert close(rm, fw['running_mean']) and close(rv, fw['running_var'])
    assert close(dx, gx.reshape(-1, ch)) and close(dgamma, gg) and close(dbeta, gb)
    if not training:
        assert torch.equal(fw['running_mean'], rmean.double()) and torch.equal(fw['running_var'], rvar.double())
