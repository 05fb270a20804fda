"""CPU: the gradient entry points of the fp32 convolution (csrc/conv_grad.hip) are declared, exported and bound; their launchers
reject bad descriptors before they touch a device; the differentiable surface has no CPU fallback; and the float64 autograd
reference and the rotate-transpose identity the GPU tests lean on are the operator's definition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_cases as cg
from usot_amd import autograd as hip_autograd, build, hip
from usot_amd.net import ConvSlot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_conv2d_wgrad_f32', 'usot_conv2d_dgrad_f32', 'usot_conv2d_wgrad_ws_floats', 'usot_conv2d_wgrad_psplit',
        'usot_conv2d_wgrad_geometry', 'usot_conv_pack_dgrad_f32', 'usot_conv2d_dgrad_route')
ONE = 16                                               # an address that is never dereferenced on the paths tested here


def desc(c=cg.TOWER, **kw):
    n, h, w, cin, cout, k, s, pad, dil = c
    args = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=k, KW=k, stride=s, pad=pad, dil=dil,
                x=ONE, w=ONE, wt=ONE, dy=ONE, dx=ONE, dw=ONE, db=ONE, ws=ONE)
    fields = {f: kw.pop(f) for f in list(kw) if f in ('OH', 'OW')}
    args.update(kw)
    d = hip.grad_desc(**args)
    for f, v in fields.items():
        setattr(d, f, v)
    return d


def test_gradient_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'typedef\s+struct\s+usot_conv_grad_desc\s*\{', text)
    L = ctypes.CDLL(build.build(force=False))
    for s in SYMS:
        assert re.search(r'\b(int|int64_t)\s+%s\s*\(' % s, text), s
        assert s in hip.EXPORTS
        assert hasattr(L, s), s
        assert hasattr(hip.lib(), s)
    L.usot_abi_version.restype = ctypes.c_int
    assert L.usot_abi_version() == 6                    # symbols were added, no signature changed
    # the ctypes mirror has the header's fields, in its order
    m = re.search(r'typedef\s+struct\s+usot_conv_grad_desc\s*\{(.*?)\}', text, flags=re.S)
    names = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(float|int32_t)\s*', '', decl).split(',')]
    assert names == [f[0] for f in hip.GradDesc._fields_]
    assert ctypes.sizeof(hip.GradDesc) == 8 * 8 + 16 * 4
    for name in ('GradDesc', 'conv2d_backward_w', 'conv2d_backward_x', 'pack_dgrad'):
        assert hasattr(hip, name)
    assert hasattr(hip_autograd, 'Conv2dFunction') and hasattr(hip_autograd, 'conv2d')


BAD = [dict(N=-1), dict(H=0), dict(W=0), dict(Cin=0), dict(Cout=0), dict(KH=0), dict(KW=0), dict(stride=0),
       dict(pad=(-1, 0)), dict(dil=(0, 1)), dict(Cin=48), dict(Cin=16), dict(OH=24), dict(OW=26), dict(OH=0)]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '_'.join('%s%s' % kv for kv in b.items()).replace(' ', ''))
def test_bad_geometry_is_rejected_without_a_device(bad):
    L = hip.lib()
    d = desc(**bad)
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(d)) == -1
    assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(d)) == -1
    assert L.usot_conv2d_dgrad_route(ctypes.byref(d)) == -1
    assert L.usot_conv2d_wgrad_ws_floats(ctypes.byref(d)) == -1


def test_bad_pointers_and_splits_are_rejected_without_a_device():
    L = hip.lib()
    assert L.usot_conv2d_wgrad_f32(None, None) == -1 and L.usot_conv2d_dgrad_f32(None, None) == -1
    for missing in ('x', 'dy', 'dw'):
        assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(**{missing: None}))) == -1, missing
    for missing in ('dy', 'w', 'dx'):
        assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(desc(**{missing: None}))) == -1, missing
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(x=ONE + 4))) == -1            # alignment
    m = 3 * 25 * 25
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(psplit=m + 1))) == -1         # more slices than pixels
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(psplit=-1))) == -1
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(psplit=2, ws=None))) == -1    # a split needs its workspace
    assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(desc(route=3))) == -1
    assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(desc(cg.RAW[5], route=1))) == -1   # route A forced on a thin head
    assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(desc(route=1, wt=None))) == -1     # ... or without the rotated bank
    assert L.usot_conv_pack_dgrad_f32(None, None, ONE, 4, 32, 3, 3) == -1
    assert L.usot_conv_pack_dgrad_f32(None, ONE, ONE, 0, 32, 3, 3) == -1
    # N == 0: nothing to do
    assert L.usot_conv2d_wgrad_f32(None, ctypes.byref(desc(N=0))) == 0
    assert L.usot_conv2d_dgrad_f32(None, ctypes.byref(desc(N=0))) == 0


def test_workspace_split_and_geometry_queries():
    L = hip.lib()
    bco, bk, chunk = hip.wgrad_geometry()
    assert bco % 16 == 0 and bk in (32, 64) and chunk % 4 == 0 and chunk > 0
    n, h, w, cin, cout, k, s, pad, dil = cg.TOWER
    K = k * k * cin
    assert L.usot_conv2d_wgrad_ws_floats(ctypes.byref(desc(psplit=1))) == 0
    for ps in (2, 3, 7):
        # slabs [psplit][Cout][K] and, as the header documents, [psplit][Cout] partial bias sums behind them
        assert L.usot_conv2d_wgrad_ws_floats(ctypes.byref(desc(psplit=ps))) == ps * cout * K + ps * cout
        assert L.usot_conv2d_wgrad_psplit(ctypes.byref(desc(psplit=ps))) == ps
    for c in cg.RAW:
        auto = L.usot_conv2d_wgrad_psplit(ctypes.byref(desc(c)))
        m = c[0] * cg.out_hw(c)[0] * cg.out_hw(c)[1]
        assert 1 <= auto <= max(1, m // (2 * chunk)) and auto <= 32, (c, auto)
        want = 0 if auto == 1 else auto * c[4] * (c[5] * c[5] * c[3] + 1)
        assert L.usot_conv2d_wgrad_ws_floats(ctypes.byref(desc(c))) == want


def test_data_gradient_routes():
    L = hip.lib()
    route = lambda c, **kw: L.usot_conv2d_dgrad_route(ctypes.byref(desc(c, **kw)))
    assert route(cg.TOWER) == 1 and route(cg.ENCODER) == 1
    for c in cg.RAW:
        assert route(c) == (1 if cg.route_a(c) else 2), c
        assert route(c, route=2) == 2
        assert route(c, wt=None) == 2                       # no rotated bank: the direct kernel
    thin4, thin1, res40, strided = cg.RAW[5], cg.RAW[6], cg.RAW[1], cg.RAW[8]
    assert (thin4[4], thin1[4], res40[4], strided[6]) == (4, 1, 40, 2)
    for c in (thin4, thin1, res40, strided):
        assert route(c) == 2 and route(c, route=1) == -1
    assert route((1, 9, 9, 32, 32, 3, 1, (3, 3), (1, 1))) == 2          # pad > dil*(k-1): pad' would be negative


@pytest.mark.parametrize('grad', [False, True])
def test_no_cpu_fallback_on_the_differentiable_surface(grad):
    x = torch.zeros(1, 32, 9, 9, requires_grad=grad)
    w = torch.zeros(40, 32, 3, 3, requires_grad=grad)
    b = torch.zeros(40, requires_grad=grad)
    with pytest.raises(hip.HipError):
        hip_autograd.conv2d(x, w, b, 1, 1, 1)
    with pytest.raises(hip.HipError):
        hip_autograd.conv2d(x, w, None, padding=(1, 1), relu=True)
    slot = ConvSlot(32, 40, 3, pad=1, bias=True)
    slot.weight.requires_grad_(grad)
    with pytest.raises(hip.HipError):
        slot(x)
    xh, dy = torch.zeros(1, 9, 9, 32), torch.zeros(1, 9, 9, 40)
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_w(xh, dy, KH=3, KW=3, pad=(1, 1))
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_x(dy, torch.zeros(40, 288), xh.shape, KH=3, KW=3, pad=(1, 1))
    with pytest.raises(hip.HipError):
        hip.pack_dgrad(torch.zeros(40, 288), 32, 3, 3)


def formulas(x, w, dy, stride, pad, dil):
    """the three definitions of csrc/conv_grad.hip on NHWC arrays and the packed bank, tap by tap"""
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    KH = KW = int(round((w.shape[1] // Cin) ** 0.5))
    dx, dw, db = np.zeros_like(x), np.zeros_like(w), dy.sum((0, 1, 2))
    for kh in range(KH):
        for kw in range(KW):
            k0 = (kh * KW + kw) * Cin
            for oh in range(OH):
                ih = oh * stride - pad[0] + kh * dil[0]
                if not 0 <= ih < H:
                    continue
                for ow in range(OW):
                    iw = ow * stride - pad[1] + kw * dil[1]
                    if not 0 <= iw < W:
                        continue
                    dw[:, k0:k0 + Cin] += dy[:, oh, ow, :].T @ x[:, ih, iw, :]
                    dx[:, ih, iw, :] += dy[:, oh, ow, :] @ w[:, k0:k0 + Cin]
    return dx, dw, db


@pytest.mark.parametrize('c', [(2, 6, 5, 32, 3, 3, 2, (1, 0), (1, 1)), (1, 7, 8, 32, 5, 3, 1, (2, 1), (2, 1))], ids=cg.case_id)
def test_float64_autograd_reference_is_the_definition(c):
    x, wt, b, dy = (t.double() for t in cg.inputs(c))
    rx, rw, rb = cg.ref_grads_of(x, wt, b, dy, c[6], c[7], c[8])
    dx, dw, db = formulas(cg.nhwc(x).numpy(), cg.pack(wt).numpy(), cg.nhwc(dy).numpy(), c[6], c[7], c[8])
    assert np.abs(dx - cg.nhwc(rx).numpy()).max() < 1e-12
    assert np.abs(dw - cg.pack(rw).numpy()).max() < 1e-12
    assert np.abs(db - rb.numpy()).max() < 1e-12


@pytest.mark.parametrize('c', cg.ROUTE_A, ids=cg.case_id)
def test_rotate_transpose_identity_of_route_a(c):
    """at stride 1, dx = conv(dy, w rotated by 180 degrees and transposed) at pad' = dil*(k-1) - pad"""
    n, h, w, cin, cout, k, s, pad, dil = c
    (x, wt, b, dy), (rx, _, _) = cg.reference(c)
    padp = (dil[0] * (k - 1) - pad[0], dil[1] * (k - 1) - pad[1])
    dx = F.conv2d(dy.double(), cg.rotated_oihw(wt.double()), None, stride=1, padding=padp, dilation=dil)
    assert dx.shape == rx.shape
    assert float((dx - rx).abs().max()) < 1e-12 * max(1.0, float(rx.abs().max()))
