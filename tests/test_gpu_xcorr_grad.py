"""GPU: gradients of the plane xcorr (csrc/xcorr_grad.hip) and the autograd surface over them (usot_amd/autograd.py,
lib.models.connect.xcorr_depthwise / GroupDW) against the oracle's operators in float64 under torch autograd on the CPU.

Metric: the project's scaled error max |got - ref| / max(|ref|, mean|ref|); bar 1e-5, the bar test_xcorr_depthwise_planes
holds the forward to (PyTorch's own float32 gradients sit at <= 1.4e-6 (dx) and <= 3.9e-6 (dk) from float64 on the CPU).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import usot_oracle as orc  # noqa: E402
from usot_amd import autograd as hip_autograd, hip  # noqa: E402

DEV = 'cuda:0'
BAR = 1e-5
GEO = ((5, 5), (3, 5), (5, 3))                    # GroupDW's three templates
HEAD = [(29, 29, 5, 5), (27, 29, 3, 5), (29, 27, 5, 3)]
XC = HEAD + [(31, 31, 5, 5), (33, 31, 5, 3), (12, 9, 4, 2), (64, 64, 5, 5), (70, 70, 5, 5), (7, 7, 7, 7), (31, 31, 7, 7)]
# dispatch edges of the plane kernels: Wx 32 | 33 (two planes per wavefront | one), Wx 64 | 65 (specialised | generic), OH = 1 and
# OW = 1 on the specialised templates, a single output
XC_EDGES = [(9, 32, 5, 5), (9, 33, 5, 5), (9, 64, 5, 3), (9, 65, 5, 3), (5, 29, 5, 5), (29, 5, 5, 5), (3, 5, 3, 5)]
XC = XC + XC_EDGES
CASES = [(s, p) for s in XC for p in ((1, 1), (2, 24), (3, 257))] + [(s, (12, 256)) for s in HEAD]


@pytest.fixture(autouse=True)
def _memory_guard():
    """Every output a wrapper of usot_amd.hip / usot_amd.autograd allocates starts as NaN and sits between canaries
    (tests/guarded.py); the guards are checked when the test ends."""
    with guarded.patched(hip, hip_autograd):
        yield


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).mean() + 1e-30)
    return float(np.max(np.abs(got - ref) / scale))


def inputs(shape, planes, seed=0):
    hx, wx, hk, wk = shape
    b, c = planes
    g = torch.Generator().manual_seed(hx * 100 + wk + 7 * b + seed)
    return (torch.randn(b, c, hx, wx, generator=g), torch.randn(b, c, hk, wk, generator=g),
            torch.randn(b, c, hx - hk + 1, wx - wk + 1, generator=g))


def ref_grads(x, k, dout):
    """float64, CPU, torch autograd through the oracle's xcorr_depthwise"""
    x64, k64 = x.double().requires_grad_(True), k.double().requires_grad_(True)
    return torch.autograd.grad(orc.xcorr_depthwise(x64, k64), (x64, k64), dout.double())


def raw_grads(x, k, dout, scale=1.0):
    """The two C entry points on NaN-filled outputs between canaries (an element nobody wrote stays NaN).  Device tensors in
    and out."""
    (b, c, hx, wx), (hk, wk) = x.shape, k.shape[2:]
    dx = guarded.alloc(x.shape, x.dtype, x.device)
    dk = guarded.alloc(k.shape, k.dtype, k.device)
    L = hip.lib()
    hip.check(L.usot_xcorr_depthwise_bwd_x_f32(hip.stream(), hip.ptr(dout), hip.ptr(k), hip.ptr(dx), b * c, hx, wx, hk, wk,
                                               C.c_float(scale)), 'usot_xcorr_depthwise_bwd_x_f32')
    hip.check(L.usot_xcorr_depthwise_bwd_k_f32(hip.stream(), hip.ptr(dout), hip.ptr(x), hip.ptr(dk), b * c, hx, wx, hk, wk,
                                               C.c_float(scale)), 'usot_xcorr_depthwise_bwd_k_f32')
    return dx, dk


def dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ---- 1. raw entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,planes', CASES)
def test_raw_gradients(shape, planes):
    x, k, dout = inputs(shape, planes)
    rx, rk = ref_grads(x, k, dout)
    dx, dk = raw_grads(*dev(x, k, dout))
    ex, ek = rel_err(dx.cpu().numpy(), rx.numpy()), rel_err(dk.cpu().numpy(), rk.numpy())
    print('shape %s planes %s: dx %.3g dk %.3g' % (shape, planes, ex, ek))
    assert ex < BAR and ek < BAR, (ex, ek)                 # NaN (an unwritten element) fails the comparison too


def test_python_binding_matches_raw_entry_points():
    x, k, dout = dev(*inputs(HEAD[1], (3, 257)))
    dx, dk = raw_grads(x, k, dout, 0.5)
    assert torch.equal(hip.xcorr_depthwise_backward_x(dout, k, x.shape, 0.5), dx)
    assert torch.equal(hip.xcorr_depthwise_backward_k(dout, x, k.shape, 0.5), dk)
    with pytest.raises(hip.HipError):
        hip.xcorr_depthwise_backward_x(dout, k[:2], x.shape)
    with pytest.raises(hip.HipError):
        hip.xcorr_depthwise_backward_k(dout, x[:2], k.shape)
    with pytest.raises(hip.HipError):
        hip.xcorr_depthwise_backward_x(dout[..., :-1], k, x.shape)


# ---- 2. scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', HEAD + [(12, 9, 4, 2), (70, 70, 5, 5)])
def test_scale(shape):
    x, k, dout = dev(*inputs(shape, (3, 257), seed=1))
    dx1, dk1 = raw_grads(x, k, dout, 1.0)
    dxs, dks = raw_grads(x, k, dout, 0.37)
    for got, one in ((dxs, dx1), (dks, dk1)):
        want = 0.37 * one.double()
        assert float(((got.double() - want).abs() / want.abs().clamp_min(1e-30)).max()) < 1e-6
    dx0, dk0 = raw_grads(x, k, dout, 0.0)
    assert torch.equal(dx0, torch.zeros_like(dx0)) and torch.equal(dk0, torch.zeros_like(dk0))


# ---- 3. bit reproducibility ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [(3, 257), (12, 256)])
@pytest.mark.parametrize('shape', HEAD)
def test_bit_reproducible(shape, planes):
    x, k, dout = dev(*inputs(shape, planes, seed=2))
    a = raw_grads(x, k, dout)
    b = raw_grads(x, k, dout)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        junk = torch.randn(512, 512, device=DEV)
        junk = (junk @ junk).relu_().sum()
        c = raw_grads(x, k, dout)
    side.synchronize()
    assert bool(torch.isfinite(junk))
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])


# ---- 4. autograd surface ------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """counts calls of the two gradient bindings (usot_amd.autograd looks them up on the module at call time)"""
    n = {'x': 0, 'k': 0}
    bx, bk = hip.xcorr_depthwise_backward_x, hip.xcorr_depthwise_backward_k

    def cx(*a, **kw):
        n['x'] += 1
        return bx(*a, **kw)

    def ck(*a, **kw):
        n['k'] += 1
        return bk(*a, **kw)
    monkeypatch.setattr(hip, 'xcorr_depthwise_backward_x', cx)
    monkeypatch.setattr(hip, 'xcorr_depthwise_backward_k', ck)
    return n


@pytest.mark.parametrize('shape', HEAD + [(12, 9, 4, 2)])
def test_autograd_both_gradients(shape, launches):
    from lib.models import connect
    x, k, dout = inputs(shape, (2, 24), seed=3)
    rx, rk = ref_grads(x, k, dout)
    xd, kd, dd = dev(x, k, dout)
    plain = hip.xcorr_depthwise(xd, kd)
    xd.requires_grad_(True), kd.requires_grad_(True)
    out = connect.xcorr_depthwise(xd, kd)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    (out * dd).sum().backward()
    assert launches == {'x': 1, 'k': 1}
    assert rel_err(xd.grad.cpu().numpy(), rx.numpy()) < BAR and rel_err(kd.grad.cpu().numpy(), rk.numpy()) < BAR


def test_autograd_only_what_is_asked(launches):
    from lib.models import connect
    x, k, dout = inputs(HEAD[0], (2, 24), seed=4)
    rx, rk = ref_grads(x, k, dout)
    xd, kd, dd = dev(x, k, dout)
    xg = xd.clone().requires_grad_(True)
    gx, = torch.autograd.grad(connect.xcorr_depthwise(xg, kd), (xg,), dd)
    assert launches == {'x': 1, 'k': 0} and rel_err(gx.cpu().numpy(), rx.numpy()) < BAR
    kg = kd.clone().requires_grad_(True)
    out = connect.xcorr_depthwise(xd, kg)
    out.backward(dd)
    assert launches == {'x': 1, 'k': 1} and xd.grad is None and rel_err(kg.grad.cpu().numpy(), rk.numpy()) < BAR


def test_autograd_noncontiguous_grad_output():
    from lib.models import connect
    x, k, dout = inputs(HEAD[2], (2, 24), seed=5)
    rx, rk = ref_grads(x, k, dout)
    xd, kd, dd = dev(x, k, dout)
    xd.requires_grad_(True), kd.requires_grad_(True)
    dperm = dd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)          # same values, transposed strides
    assert not dperm.is_contiguous()
    connect.xcorr_depthwise(xd, kd).backward(dperm)
    assert rel_err(xd.grad.cpu().numpy(), rx.numpy()) < BAR and rel_err(kd.grad.cpu().numpy(), rk.numpy()) < BAR
    # and non-contiguous inputs
    xt = xd.detach().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    gx, = torch.autograd.grad(connect.xcorr_depthwise(xt, kd.detach()), (xt,), dd)
    assert torch.equal(gx, xd.grad)


def test_autograd_off_means_plain_forward():
    from lib.models import connect
    x, k, _ = inputs(HEAD[0], (2, 24), seed=6)
    xd, kd = dev(x, k)
    plain = hip.xcorr_depthwise(xd, kd)
    out = connect.xcorr_depthwise(xd, kd)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, plain)
    xd.requires_grad_(True)
    with torch.no_grad():
        out = connect.xcorr_depthwise(xd, kd)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, plain)


def test_autograd_forward_on_the_golden_fixtures(gold_model):
    from lib.models import connect
    for i in range(5):
        x = torch.from_numpy(gold_model['xcorr%d/x' % i]).to(DEV).requires_grad_(True)
        k = torch.from_numpy(gold_model['xcorr%d/k' % i]).to(DEV).requires_grad_(True)
        out = connect.xcorr_depthwise(x, k)
        assert out.grad_fn is not None
        assert rel_err(out.detach().cpu().numpy(), gold_model['xcorr%d/out' % i]) < 1e-5


# ---- 5. GroupDW ---------------------------------------------------------------------------------------------------------
LOGITS = (0.3, -0.2, 0.9)


def groupdw_inputs(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    zs = [torch.randn(B, C, hk, wk, generator=g) for hk, wk in GEO]
    xs = [torch.randn(B, C, 24 + hk, 24 + wk, generator=g) for hk, wk in GEO]     # 29x29, 27x29, 29x27 -> 25x25
    dout = torch.randn(B, C, 25, 25, generator=g)
    return zs, xs, dout


def groupdw_ref(zs, xs, dout, which='cls_dw'):
    w = torch.tensor(LOGITS, dtype=torch.float64, requires_grad=True)
    z64 = [t.double().requires_grad_(True) for t in zs]
    x64 = [t.double().requires_grad_(True) for t in xs]
    out = orc.groupdw({'connect_model.%s.weight' % which: w}, which, z64, x64)
    grads = torch.autograd.grad(out, [w] + z64 + x64, dout.double())
    return out.detach(), grads[0], grads[1:4], grads[4:7]


@pytest.mark.parametrize('B', [2, 12, 14])               # 14 = the memory form, B = 2 x N_mem = 7 planes sets
def test_groupdw_module(B, launches):
    from lib.models import connect
    zs, xs, dout = groupdw_inputs(B, 256, seed=B)
    rout, rw, rz, rx = groupdw_ref(zs, xs, dout, 'reg_dw' if B == 12 else 'cls_dw')
    m = connect.GroupDW()
    with torch.no_grad():
        m.weight.copy_(torch.tensor(LOGITS))
    m = m.to(DEV)
    m.weight.requires_grad_(True)
    zd = [t.to(DEV).requires_grad_(True) for t in zs]
    xd = [t.to(DEV).requires_grad_(True) for t in xs]
    out = m(zd, xd)
    assert rel_err(out.detach().cpu().numpy(), rout.numpy()) < BAR
    out.backward(dout.to(DEV))
    assert launches == {'x': 3, 'k': 3}
    for i in range(3):
        ez, ex = rel_err(zd[i].grad.cpu().numpy(), rz[i].numpy()), rel_err(xd[i].grad.cpu().numpy(), rx[i].numpy())
        print('B %d branch %d: dz %.3g dx %.3g' % (B, i, ez, ex))
        assert ez < BAR and ex < BAR, (i, ez, ex)
    ew = float((m.weight.grad.cpu().double() - rw).abs().max() / rw.abs().max())
    print('B %d: dweight %.3g' % (B, ew))
    assert ew <= 1e-5


def test_groupdw_partial_requirements(launches):
    """weight alone still needs the three template gradients (s_i = <dk_i, z_i>); inputs alone take the weights as `scale`"""
    from usot_amd import autograd
    zs, xs, dout = groupdw_inputs(2, 256, seed=21)
    rout, rw, rz, rx = groupdw_ref(zs, xs, dout)
    zd, xd, dd = dev(*zs), dev(*xs), dout.to(DEV)
    w = torch.tensor(LOGITS, device=DEV)
    plain = autograd.groupdw(zd, xd, w)
    assert plain.grad_fn is None and rel_err(plain.cpu().numpy(), rout.numpy()) < BAR
    wg = w.clone().requires_grad_(True)
    out = autograd.groupdw(zd, xd, wg)
    assert torch.equal(out.detach(), plain)
    gw, = torch.autograd.grad(out, (wg,), dd)
    assert launches == {'x': 0, 'k': 3}
    assert float((gw.cpu().double() - rw).abs().max() / rw.abs().max()) <= 1e-5
    x1 = xd[1].clone().requires_grad_(True)
    z2 = zd[2].clone().requires_grad_(True)
    out = autograd.groupdw([zd[0], zd[1], z2], [xd[0], x1, xd[2]], w)
    gx1, gz2 = torch.autograd.grad(out, (x1, z2), dd)
    assert launches == {'x': 1, 'k': 4}
    assert rel_err(gx1.cpu().numpy(), rx[1].numpy()) < BAR and rel_err(gz2.cpu().numpy(), rz[2].numpy()) < BAR


# ---- 6. chained: encoders in front, gradients reach their weights ---------------------------------------------------
class TinySiamese(torch.nn.Module):
    """one Conv2d per side in front of GroupDW; the three templates / search maps are crops of the two feature maps"""

    def __init__(self, C=32):
        super().__init__()
        self.enc_z = torch.nn.Conv2d(3, C, 3)
        self.enc_x = torch.nn.Conv2d(3, C, 3)
        self.weight = torch.nn.Parameter(torch.tensor(LOGITS))

    def forward(self, z, x, groupdw):
        fz, fx = torch.tanh(self.enc_z(z)), torch.tanh(self.enc_x(x))           # [B][C][5][5], [B][C][29][29]
        zs = [fz, fz[:, :, 1:4, :], fz[:, :, :, 1:4]]
        xs = [fx, fx[:, :, 1:28, :], fx[:, :, :, 1:28]]
        out = groupdw(zs, xs, self.weight)
        return (out * out).mean() + out[:, :, ::3, ::2].sum() * 1e-3


def test_chained_encoder_gradients():
    from usot_amd import autograd
    torch.manual_seed(11)
    net = TinySiamese()
    g = torch.Generator().manual_seed(12)
    z, x = torch.randn(4, 3, 7, 7, generator=g), torch.randn(4, 3, 31, 31, generator=g)

    def oracle_groupdw(zs, xs, w):
        return orc.groupdw({'connect_model.cls_dw.weight': w}, 'cls_dw', zs, xs)

    def grads(model, z, x, groupdw):
        model.zero_grad()
        loss = model(z, x, groupdw)
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().cpu().double().numpy() for n, p in model.named_parameters()}

    l64, g64 = grads(copy.deepcopy(net).double(), z.double(), x.double(), oracle_groupdw)
    l32, g32 = grads(copy.deepcopy(net), z, x, oracle_groupdw)
    lgpu, ggpu = grads(copy.deepcopy(net).to(DEV), z.to(DEV), x.to(DEV), autograd.groupdw)
    assert abs(lgpu - l64) <= 1e-4 * abs(l64)
    for name in g64:
        cpu32, got = rel_err(g32[name], g64[name]), rel_err(ggpu[name], g64[name])
        bar = max(1e-4, 4 * cpu32)
        print('%s: device %.3g, float32 on the CPU %.3g, bar %.3g' % (name, got, cpu32, bar))
        assert got <= bar, (name, got, bar)
