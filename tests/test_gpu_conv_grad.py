"""GPU: gradients of the fp32 convolution (csrc/conv_grad.hip: the MFMA weight gradient with its bias sums, the data gradient's
two routes, the rotated-bank pack kernel) and the autograd surface over them (usot_amd.autograd.conv2d, net.ConvSlot) against
float64 torch autograd through F.conv2d on the CPU.

Metric: the project's scaled error max |got - ref| / max(|ref|, mean|ref|); bar 1e-5, the bar tests/test_gpu_xcorr_grad.py
holds gradients to (PyTorch-CPU's own float32 gradients sit at 2e-7 ... 5.8e-6 from float64 on the shapes of RAW).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_grad_cases as cg  # noqa: E402
import guarded  # noqa: E402
import usot_oracle as orc  # noqa: E402
from usot_amd import autograd as hip_autograd, hip  # noqa: E402
from usot_amd.net import ConvSlot  # noqa: E402

DEV = 'cuda:0'
BAR = 1e-5


@pytest.fixture(autouse=True)
def _memory_guard():
    """Every output a wrapper of usot_amd.hip / usot_amd.autograd allocates starts as NaN and sits between canaries
    (tests/guarded.py); the guards are checked when the test ends."""
    with guarded.patched(hip, hip_autograd):
        yield


def rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.maximum(np.abs(ref), np.abs(ref).mean() + 1e-30)
    return float(np.max(np.abs(got - ref) / scale))             # NaN (an unwritten element) fails every comparison with the bar


def geo(c):
    n, h, w, cin, cout, k, s, pad, dil = c
    return dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=k, KW=k, stride=s, pad=pad, dil=dil)


def operands(c, seed=0):
    """device operands in the kernels' layouts: x NHWC, packed bank, dy NHWC"""
    (x, wt, b, dy), _ = cg.reference(c, seed)
    return guarded.put(cg.nhwc(x), DEV), guarded.put(cg.pack(wt), DEV), guarded.put(cg.nhwc(dy), DEV)     # a NaN on both sides


def raw_wgrad(c, xh, dyh, psplit=0, bias=True):
    """usot_conv2d_wgrad_f32 on NaN-filled outputs and a NaN-filled workspace between canaries -> (dw, db | None, ws | None)"""
    n, h, w, cin, cout, k, s, pad, dil = c
    L = hip.lib()
    d = hip.grad_desc(psplit=psplit, **geo(c))
    need = L.usot_conv2d_wgrad_ws_floats(C.byref(d))
    assert need >= 0
    dw = guarded.alloc((cout, k * k * cin), torch.float32, DEV)
    db = guarded.alloc((cout,), torch.float32, DEV) if bias else None
    ws = guarded.alloc((need,), torch.float32, DEV) if need else None
    d.x, d.dy, d.dw, d.db, d.ws = xh.data_ptr(), dyh.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None, \
        ws.data_ptr() if need else None
    hip.check(L.usot_conv2d_wgrad_f32(hip.stream(), C.byref(d)), 'usot_conv2d_wgrad_f32')
    return dw, db, ws


def raw_dgrad(c, dyh, wp, route=0):
    """usot_conv_pack_dgrad_f32 + usot_conv2d_dgrad_f32 on NaN-filled outputs between canaries -> dx NHWC"""
    n, h, w, cin, cout, k, s, pad, dil = c
    L = hip.lib()
    wt = None
    if route != 2 and cg.route_a(c):
        wt = guarded.alloc((cin, k * k * cout), torch.float32, DEV)
        hip.check(L.usot_conv_pack_dgrad_f32(hip.stream(), hip.ptr(wp), hip.ptr(wt), cout, cin, k, k), 'usot_conv_pack_dgrad_f32')
    dx = guarded.alloc((n, h, w, cin), torch.float32, DEV)
    d = hip.grad_desc(route=route, dy=dyh.data_ptr(), w=wp.data_ptr(), wt=wt.data_ptr() if wt is not None else None,
                      dx=dx.data_ptr(), **geo(c))
    assert L.usot_conv2d_dgrad_route(C.byref(d)) == (1 if wt is not None else 2)
    hip.check(L.usot_conv2d_dgrad_f32(hip.stream(), C.byref(d)), 'usot_conv2d_dgrad_f32')
    return dx


def ref_packed(c, seed=0):
    """float64 references in the kernels' layouts: (dx NHWC, dw packed, db)"""
    _, (rx, rw, rb) = cg.reference(c, seed)
    return cg.nhwc(rx), cg.pack(rw), rb


# ---- 1. raw entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', cg.RAW, ids=cg.case_id)
def test_raw_gradients(c):
    xh, wp, dyh = operands(c)
    rx, rw, rb = ref_packed(c)
    dw, db, _ = raw_wgrad(c, xh, dyh)
    dx = raw_dgrad(c, dyh, wp)
    ew, eb, ex = rel_err(dw, rw), rel_err(db, rb), rel_err(dx, rx)
    print('%s: dw %.3g db %.3g dx %.3g (route %d)' % (cg.case_id(c), ew, eb, ex, 1 if cg.route_a(c) else 2))
    assert ew < BAR and eb < BAR and ex < BAR, (ew, eb, ex)


# ---- 2. pixel-slice edges of the weight gradient ----------------------------------------------------------------------
EDGE_M = {'chunk-1': lambda ch: ch - 1, 'chunk': lambda ch: ch, 'chunk+1': lambda ch: ch + 1, '2chunk+1': lambda ch: 2 * ch + 1,
          '3chunk-1': lambda ch: 3 * ch - 1}
EDGES = [(m, ps) for m in EDGE_M for ps in (1, 2, 3)] + [('chunk-1', 'M')]


@pytest.mark.parametrize('mname,ps', EDGES)
def test_pixel_slice_edges(mname, ps):
    """1x1 convolution of a 1 x M map: slices and chunks that end on, one before and one behind a chunk edge, and slices of
    one pixel each"""
    chunk = hip.wgrad_geometry()[2]
    M = EDGE_M[mname](chunk)
    ps = M if ps == 'M' else ps
    c = (1, 1, M, 32, 32, 1, 1, (0, 0), (1, 1))
    xh, wp, dyh = operands(c)
    rx, rw, rb = ref_packed(c)
    dw, db, ws = raw_wgrad(c, xh, dyh, psplit=ps)
    assert (ws is None) == (ps == 1)
    ew, eb = rel_err(dw, rw), rel_err(db, rb)
    print('M %d psplit %d: dw %.3g db %.3g' % (M, ps, ew, eb))
    assert ew < BAR and eb < BAR, (ew, eb)


# ---- 3. bit reproducibility ---------------------------------------------------------------------------------------------
def test_deterministic():
    xh, wp, dyh = operands(cg.TOWER)
    for ps in (0, 3):
        a = raw_wgrad(cg.TOWER, xh, dyh, psplit=ps)
        b = raw_wgrad(cg.TOWER, xh, dyh, psplit=ps)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ps
    for route in (1, 2):
        assert torch.equal(raw_dgrad(cg.TOWER, dyh, wp, route), raw_dgrad(cg.TOWER, dyh, wp, route)), route


# ---- 4. the two routes of the data gradient ------------------------------------------------------------------------------
@pytest.mark.parametrize('c', cg.ROUTE_A, ids=cg.case_id)
def test_routes_agree(c):
    xh, wp, dyh = operands(c)
    rx = ref_packed(c)[0]
    ea, eb = rel_err(raw_dgrad(c, dyh, wp, 1), rx), rel_err(raw_dgrad(c, dyh, wp, 2), rx)
    print('%s: route A %.3g route B %.3g' % (cg.case_id(c), ea, eb))
    assert ea < BAR and eb < BAR, (ea, eb)


@pytest.mark.parametrize('c', cg.ROUTE_B_ONLY, ids=cg.case_id)
def test_route_a_refuses_what_it_cannot_do(c):
    xh, wp, dyh = operands(c)
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_x(dyh, wp, xh.shape, KH=c[5], KW=c[5], stride=c[6], pad=c[7], dil=c[8], route=1)


# ---- 5. optional outputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ps', [1, 2])
def test_bias_gradient_is_optional(ps):
    c = cg.RAW[1]
    xh, wp, dyh = operands(c)
    dw, db, _ = raw_wgrad(c, xh, dyh, psplit=ps)
    dw0, none, ws0 = raw_wgrad(c, xh, dyh, psplit=ps, bias=False)
    assert none is None and torch.equal(dw, dw0)
    if ps > 1:                        # the partial bias sums' part of the workspace was left alone (still the NaN pattern)
        tail = ws0[ps * dw.numel():]
        assert tail.numel() == ps * c[4] and bool(torch.isnan(tail).all())
        assert bool(torch.isfinite(ws0[:ps * dw.numel()]).all())


# ---- 6. python wrappers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [cg.RAW[1], cg.RAW[4], cg.RAW[8]], ids=cg.case_id)
def test_python_bindings_match_raw_entry_points(c):
    n, h, w, cin, cout, k, s, pad, dil = c
    xh, wp, dyh = operands(c)
    kw = dict(KH=k, KW=k, stride=s, pad=pad, dil=dil)
    for ps in (0, 2):
        dw, db, _ = raw_wgrad(c, xh, dyh, psplit=ps)
        gw, gb = hip.conv2d_backward_w(xh, dyh, bias=True, psplit=ps, **kw)
        assert torch.equal(gw, dw) and torch.equal(gb, db)
        gw, gb = hip.conv2d_backward_w(xh, dyh, psplit=ps, **kw)
        assert gb is None and torch.equal(gw, dw)
    for route in (0, 2):
        assert torch.equal(hip.conv2d_backward_x(dyh, wp, xh.shape, route=route, **kw), raw_dgrad(c, dyh, wp, route))
    (x, wt, b, dy), _ = cg.reference(c)
    assert torch.equal(hip.pack_dgrad(wp, cin, k, k).cpu(), cg.pack(cg.rotated_oihw(wt)))
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_w(xh, dyh[:, :-1], **kw)
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_w(xh[:1], dyh, **kw) if n > 1 else hip.conv2d_backward_w(xh, dyh[..., :-1], **kw)
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_x(dyh, wp[:, :-cin], xh.shape, **kw)
    with pytest.raises(hip.HipError):
        hip.conv2d_backward_x(dyh, wp, (n, h + 2, w, cin), **kw)           # + 2: another OH at stride 2 as well
    with pytest.raises(hip.HipError):
        hip.pack_dgrad(wp, cin, k, k + 1)


# ---- 7. autograd surface ------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """counts calls of the two gradient bindings (usot_amd.autograd looks them up on the module at call time)"""
    n = {'x': 0, 'w': 0}
    bx, bw = hip.conv2d_backward_x, hip.conv2d_backward_w

    def cx(*a, **kw):
        n['x'] += 1
        return bx(*a, **kw)

    def cw(*a, **kw):
        n['w'] += 1
        return bw(*a, **kw)
    monkeypatch.setattr(hip, 'conv2d_backward_x', cx)
    monkeypatch.setattr(hip, 'conv2d_backward_w', cw)
    return n


AUTOGRAD_CASES = [cg.RAW[1], cg.RAW[2], cg.RAW[3], cg.RAW[5], cg.RAW[6]]          # rows 2, 3 and 5 of the table


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('c', AUTOGRAD_CASES, ids=cg.case_id)
def test_autograd_conv2d(c, relu, launches):
    n, h, w, cin, cout, k, s, pad, dil = c
    (x, wt, b, dy), _ = cg.reference(c)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    y64 = F.conv2d(x64, w64, b64, stride=s, padding=pad, dilation=dil)
    ref = torch.autograd.grad(y64.relu() if relu else y64, (x64, w64, b64), dy.double())
    xd, wd, bd, dd = (t.to(DEV) for t in (x, wt, b, dy))
    plain = hip.conv2d(cg.nhwc(x).to(DEV), cg.pack(wt).to(DEV), bd, KH=k, KW=k, stride=s, pad=pad, dil=dil,
                       act=hip.ACT_RELU if relu else hip.ACT_NONE)
    off = hip_autograd.conv2d(xd, wd, bd, s, pad, dil, relu=relu)
    assert off.grad_fn is None and not off.requires_grad and torch.equal(off.permute(0, 2, 3, 1), plain)
    xd.requires_grad_(True), wd.requires_grad_(True), bd.requires_grad_(True)
    with torch.no_grad():
        assert hip_autograd.conv2d(xd, wd, bd, s, pad, dil, relu=relu).grad_fn is None
    out = hip_autograd.conv2d(xd, wd, bd, s, pad, dil, relu=relu)
    assert out.grad_fn is not None and out.shape == y64.shape and torch.equal(out.detach().permute(0, 2, 3, 1), plain)
    got = torch.autograd.grad(out, (xd, wd, bd), dd)
    assert launches == {'x': 1, 'w': 1}
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print('%s relu %d: dx %.3g dw %.3g db %.3g' % (cg.case_id(c), relu, *errs))
    assert max(errs) < BAR, errs


def test_autograd_only_what_is_asked(launches):
    c = cg.RAW[1]
    n, h, w, cin, cout, k, s, pad, dil = c
    (x, wt, b, dy), (rx, rw, rb) = cg.reference(c)
    xd, wd, bd, dd = (t.to(DEV) for t in (x, wt, b, dy))
    xg = xd.clone().requires_grad_(True)
    gx, = torch.autograd.grad(hip_autograd.conv2d(xg, wd, bd, s, pad, dil), (xg,), dd)
    assert launches == {'x': 1, 'w': 0} and rel_err(gx, rx) < BAR
    wg = wd.clone().requires_grad_(True)
    hip_autograd.conv2d(xd, wg, bd, s, pad, dil).backward(dd)
    assert launches == {'x': 1, 'w': 1} and xd.grad is None and bd.grad is None and rel_err(wg.grad, rw) < BAR
    bg = bd.clone().requires_grad_(True)
    gb, = torch.autograd.grad(hip_autograd.conv2d(xd, wd, bg, s, pad, dil), (bg,), dd)
    assert launches == {'x': 1, 'w': 2} and rel_err(gb, rb) < BAR
    # a gradient with the strides of an expanded scalar (what .sum().backward() hands over), and no bias
    out = hip_autograd.conv2d(xg, wd, None, s, pad, dil)
    gx1, = torch.autograd.grad(out.sum(), (xg,))
    ones = cg.ref_grads_of(x, wt, b, torch.ones_like(dy), s, pad, dil)[0]
    assert rel_err(gx1, ones) < BAR


def test_conv_slot_is_differentiable():
    c = cg.RAW[1]                                   # 32 -> 40, 3x3, pad 1
    (x, wt, b, dy), _ = cg.reference(c)
    slot = ConvSlot(32, 40, 3, pad=1)
    with torch.no_grad():
        slot.weight.copy_(wt)
    slot = slot.to(DEV)
    slot.weight.requires_grad_(True)
    slot(x.to(DEV)).sum().backward()
    ref = cg.ref_grads_of(x, wt, b, torch.ones_like(dy), 1, (1, 1), (1, 1))[1]
    err = rel_err(slot.weight.grad, ref)
    print('ConvSlot(32, 40, 3, pad=1): dweight %.3g' % err)
    assert slot.weight.grad.shape == slot.weight.shape and err < BAR
    biased = ConvSlot(32, 40, 3, pad=1, bias=True).to(DEV)
    with torch.no_grad():
        biased.weight.copy_(wt.to(DEV)), biased.bias.copy_(b.to(DEV))
    y = biased(x.to(DEV))
    assert y.grad_fn is None
    y64 = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    assert rel_err(y, y64) < BAR


# ---- 8. chained: what the feature is for ---------------------------------------------------------------------------------
DILS = ((1, 1), (2, 1), (1, 2))                      # the encoders of the 5x5, 3x5 and 5x3 branches
LOGITS = (0.3, -0.2, 0.9)


def chain(conv, groupdw, z, x, banks, logits):
    """three encoders per side -> GroupDW -> conv + ReLU -> conv to 4 channels -> sum of squares"""
    zs = [conv(z, banks[i], dilation=DILS[i]) for i in range(3)]
    xs = [conv(x, banks[3 + i], dilation=DILS[i]) for i in range(3)]
    f = groupdw(zs, xs, logits)
    f = conv(f, banks[6], padding=1, relu=True)
    return conv(f, banks[7], padding=1).square().sum()


def test_chain_of_encoders_correlation_and_tower():
    C_ = 32
    g = torch.Generator().manual_seed(2024)
    z, x = torch.randn(2, C_, 7, 7, generator=g), torch.randn(2, C_, 15, 15, generator=g)
    banks = [torch.randn(C_, C_, 3, 3, generator=g) / (9 * C_) ** 0.5 for _ in range(7)]
    banks.append(torch.randn(4, C_, 3, 3, generator=g) / (9 * C_) ** 0.5)
    logits = torch.tensor(LOGITS)

    def conv64(t, w, padding=0, dilation=1, relu=False):
        y = F.conv2d(t, w, None, padding=padding, dilation=dilation)
        return y.relu() if relu else y

    def gdw64(zs, xs, w):
        return orc.groupdw({'connect_model.cls_dw.weight': w}, 'cls_dw', zs, xs)

    def gconv(t, w, padding=0, dilation=1, relu=False):
        return hip_autograd.conv2d(t, w, None, 1, padding, dilation, relu=relu)

    leaves64 = [t.double().requires_grad_(True) for t in banks + [logits, z, x]]
    loss64 = chain(conv64, gdw64, leaves64[9], leaves64[10], leaves64[:8], leaves64[8])
    ref = torch.autograd.grad(loss64, leaves64)
    leaves = [t.to(DEV).requires_grad_(True) for t in banks + [logits, z, x]]
    loss = chain(gconv, hip_autograd.groupdw, leaves[9], leaves[10], leaves[:8], leaves[8])
    got = torch.autograd.grad(loss, leaves)
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    names = ['enc_z%d' % i for i in range(3)] + ['enc_x%d' % i for i in range(3)] + ['tower', 'pred', 'logits', 'z', 'x']
    errs = {}
    for name, gt, rf in zip(names, got, ref):
        errs[name] = rel_err(gt, rf)
    print('chain: ' + ' '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) < BAR, errs
