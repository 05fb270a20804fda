"""CPU: the gradient entry points of the plane xcorr are declared, exported and bound; the differentiable surface has no
CPU fallback; and the float64 autograd reference the GPU tests lean on is the operator's definition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import usot_oracle as orc
from usot_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_xcorr_depthwise_bwd_x_f32', 'usot_xcorr_depthwise_bwd_k_f32')


def test_gradient_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for s in SYMS:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % s, text)
        assert m, s
        args = [a.strip() for a in m.group(1).split(',')]
        assert len(args) == 10 and args[0].startswith('void *') and args[-1] == 'float scale', args
        assert s in hip.EXPORTS
    L = ctypes.CDLL(build.build(force=False))
    for s in SYMS:
        assert hasattr(L, s), s
    L.usot_abi_version.restype = ctypes.c_int
    assert L.usot_abi_version() == 6                    # symbols were added, no signature changed


def test_argument_errors_need_no_gpu():
    """the launchers reject what the forward rejects before touching the device; P == 0 is a no-op"""
    L = ctypes.CDLL(build.build(force=False))
    one = ctypes.c_void_p(16)                            # never dereferenced on these paths
    for s in SYMS:
        fn = getattr(L, s)
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_float]
        assert fn(None, None, one, one, 1, 9, 9, 3, 3, 1.0) == -1
        assert fn(None, one, one, one, -1, 9, 9, 3, 3, 1.0) == -1
        assert fn(None, one, one, one, 1, 2, 9, 3, 3, 1.0) == -1
        assert fn(None, one, one, one, 1, 9, 9, 0, 3, 1.0) == -1
        assert fn(None, one, one, one, 0, 9, 9, 3, 3, 1.0) == 0


@pytest.mark.parametrize('grad', [False, True])
def test_no_cpu_fallback_on_the_differentiable_surface(grad):
    from lib.models import connect
    x = torch.zeros(1, 4, 9, 9, requires_grad=grad)
    k = torch.zeros(1, 4, 3, 3, requires_grad=grad)
    with pytest.raises(hip.HipError):
        connect.xcorr_depthwise(x, k)
    geo = ((5, 5), (3, 5), (5, 3))
    zs = [torch.zeros(1, 4, hk, wk, requires_grad=grad) for hk, wk in geo]
    xs = [torch.zeros(1, 4, 8 + hk, 8 + wk, requires_grad=grad) for hk, wk in geo]
    m = connect.GroupDW()
    m.weight.requires_grad_(grad)
    with pytest.raises(hip.HipError):
        m(zs, xs)
    with pytest.raises(hip.HipError):
        hip.xcorr_depthwise_backward_x(torch.zeros(1, 4, 7, 7), k.detach(), x.shape)
    with pytest.raises(hip.HipError):
        hip.xcorr_depthwise_backward_k(torch.zeros(1, 4, 7, 7), x.detach(), k.shape)


def formulas(x, k, dout):
    """dx[p][a][b] = sum_uv dout[p][a-u][b-v] k[p][u][v];  dk[p][u][v] = sum_ij dout[p][i][j] x[p][i+u][j+v]"""
    P, Hx, Wx = x.shape
    _, Hk, Wk = k.shape
    OH, OW = Hx - Hk + 1, Wx - Wk + 1
    dx, dk = np.zeros_like(x), np.zeros_like(k)
    for u in range(Hk):
        for v in range(Wk):
            dx[:, u:u + OH, v:v + OW] += dout * k[:, u:u + 1, v:v + 1]
            dk[:, u, v] = (dout * x[:, u:u + OH, v:v + OW]).sum((1, 2))
    return dx, dk


@pytest.mark.parametrize('shape', [(2, 3, 9, 8, 3, 5), (1, 5, 6, 7, 4, 2)])
def test_float64_autograd_reference_is_the_definition(shape):
    b, c, hx, wx, hk, wk = shape
    g = torch.Generator().manual_seed(hx * 10 + wk)
    x = torch.randn(b, c, hx, wx, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(b, c, hk, wk, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(b, c, hx - hk + 1, wx - wk + 1, generator=g, dtype=torch.float64)
    rx, rk = torch.autograd.grad(orc.xcorr_depthwise(x, k), (x, k), dout)
    dx, dk = formulas(x.detach().numpy().reshape(-1, hx, wx), k.detach().numpy().reshape(-1, hk, wk),
                      dout.numpy().reshape(b * c, hx - hk + 1, wx - wk + 1))
    assert np.abs(dx - rx.numpy().reshape(dx.shape)).max() < 1e-12
    assert np.abs(dk - rk.numpy().reshape(dk.shape)).max() < 1e-12
