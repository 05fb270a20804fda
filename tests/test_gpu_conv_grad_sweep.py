"""GPU: the gradient kernels of the fp32 convolution (csrc/conv_grad.hip) - the MFMA weight gradient with its pixel slices, bias sums and
reduce launch, the rotate-and-transpose pack, the direct data gradient (route B) and route A through the forward launcher - against the
int64 reference of tests/conv_grad_sweep_cases.py, over its lists:

  M_SWEEP       every pixel count 1 .. 3 chunks + 1 at psplit 1, 2, 3, M and the launcher's own choice; both operand families
  COUT_SWEEP    every Cout through two channel blocks and four: both dy loader paths, db on both; the same Couts through route B
  K_SWEEP       Cin 32 .. 160 x eight filters, three of them rectangular: weight gradient, pack, routes A, B and auto
  GEOMETRY      ten small maps x nine widths x two batch sizes under twenty (filter, stride, pad, dil) configurations
  BIG           route B and the pack past their launch caps: the second pass of either grid-stride loop
  UNREACHED     NaN in every x element no tap reads; dx exactly +0.0 there
  REFUSED       what the launchers refuse on the host: the return code, and every output still the canary pattern

The operands are integers whose every partial sum stays below 2^24 (tests/test_conv_grad_sweep_lists.py asserts it), so float32 is exact
in any order of summation and EVERY comparison here is an equality of bits.  Inputs are guarded copies with a NaN pattern on both sides
and are compared with a snapshot afterwards; outputs and workspaces are NaN-prefilled between canaries (tests/guarded.py) and sized as
usot_conv2d_wgrad_ws_floats answers.  An explicit route = 1 must SUCCEED wherever route_a admits the case: the launcher does not fall
back to route B then, so a forward launcher that refuses a geometry shows here and nowhere else.

One item = one (list, kernel, family or stride); it loops over its list, collects every failing case and reports them all at the end.
The counts it prints are the ones tests/test_conv_grad_sweep_lists.py asserts."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_grad_cases as cg  # noqa: E402
import conv_grad_sweep_cases as sc  # noqa: E402
import guarded  # noqa: E402
from test_gpu_groupdw_sweep import mismatch, same_bits  # noqa: E402
from usot_amd import autograd as hip_autograd, hip  # noqa: E402

DEV = 'cuda:0'
OK, EINVAL = 0, -1
CANARY32 = 0x7FC17FC1
FAMILY = pytest.mark.parametrize('fam', sc.FAMILIES)


@pytest.fixture(autouse=True)
def _memory_guard():
    """allocations of the wrappers of usot_amd.hip / usot_amd.autograd are guarded too; every guard is checked when the item ends"""
    with guarded.patched(hip, hip_autograd):
        yield


def L():
    return hip.lib()


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # exact: integers below 2^24 (or already float32)


def put(a):
    return guarded.put(f32(a), DEV)


def up(a):
    return f32(a).to(DEV)


def new(*shape):
    return guarded.alloc(shape, torch.float32, DEV)


def untouched(t):
    return bool((t.contiguous().view(torch.int32) == CANARY32).all())


def diff(out, want):
    """'' when the device tensor `out` holds exactly the bits of the device tensor `want`, else what differs"""
    return '' if same_bits(out, want) else mismatch(out, want)


def geo(c):
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    return dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=kh, KW=kw, stride=s, pad=pad, dil=dil)


def inputs_unchanged(pairs):
    out = []
    for name, t, snap in pairs:
        try:
            guarded.unchanged(t, snap, name)
        except guarded.GuardError as e:
            out.append(str(e))
    return out


def report(what, n, bad, t0, extra=''):
    torch.cuda.synchronize()
    print('%s: %d cases%s, %d failing, %.2f s' % (what, n, extra, len(bad), time.perf_counter() - t0))
    guarded.check()
    assert not bad, bad[:20]


# ---- the weight gradient ------------------------------------------------------------------------------------------------------------
def wgrad(c, x, dy, psplit, bias=True):
    """one usot_conv2d_wgrad_f32 on fresh outputs -> (return code, dw, db | None, ws | None, the psplit in effect)"""
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    d = hip.grad_desc(psplit=psplit, **geo(c))
    need, eff = L().usot_conv2d_wgrad_ws_floats(C.byref(d)), L().usot_conv2d_wgrad_psplit(C.byref(d))
    assert need == (0 if eff == 1 else eff * cout * (kh * kw * cin + 1)) and eff >= 1, (c, psplit, need, eff)
    dw, db, ws = new(cout, kh * kw * cin), new(cout) if bias else None, new(need) if need else None
    d.x, d.dy, d.dw, d.db, d.ws = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None, ws.data_ptr() if need else None
    return L().usot_conv2d_wgrad_f32(hip.stream(), C.byref(d)), dw, db, ws, eff


def wgrad_case(c, listed, fam, x=None):
    """dw and db at every listed psplit and at the launcher's own, with and without db -> failure texts"""
    xd, dyd = put(sc.operand(c, fam, 'x') if x is None else x), put(sc.operand(c, fam, 'dy'))
    snaps = [('x', xd, guarded.snapshot(xd)), ('dy', dyd, guarded.snapshot(dyd))]
    rw, rb = (up(a) for a in sc.reference_w(c, fam))
    bad = []
    for ps in tuple(listed) + (0,):
        tag = '%s %s psplit %d' % (sc.case_id(c), fam, ps)
        rc, dw, db, ws, eff = wgrad(c, xd, dyd, ps)
        if rc != OK:
            bad.append('%s: return code %d' % (tag, rc))
            continue
        bad += ['%s (%d slices) %s: %s' % (tag, eff, name, m) for name, got, want in (('dw', dw, rw), ('db', db, rb)) for m in [diff(got, want)] if m]
        if ws is not None and not bool(torch.isfinite(ws).all()):
            bad.append('%s: part of the workspace was not written' % tag)
        rc, dw0, _, ws0, eff0 = wgrad(c, xd, dyd, ps, bias=False)
        if rc != OK or eff0 != eff or not same_bits(dw0, dw):
            bad.append('%s: dw without db differs from dw with it (return code %d)' % (tag, rc))
        if ws0 is not None:
            tail = ws0[eff * dw.numel():]
            if tail.numel() != eff * c[4] or not untouched(tail):
                bad.append('%s: the partial bias sums were written with db off' % tag)
    return bad + inputs_unchanged(snaps)


def wgrad_sweep(what, entries, fam, t0):
    entries = [(c, listed) for c, listed in entries if sc.applies(c, fam, 'w')]
    bad = []
    for c, listed in entries:
        bad += wgrad_case(c, listed, fam)
    report(what + ' ' + fam, len(entries), bad, t0, ' (%d listed psplits, and psplit 0 on each)' % len(sc.pairs(entries)))


@FAMILY
def test_m_sweep(fam):
    wgrad_sweep('M_SWEEP weight gradient', sc.M_SWEEP, fam, time.perf_counter())


@FAMILY
def test_cout_sweep_weight_gradient(fam):
    wgrad_sweep('COUT_SWEEP weight gradient', sc.COUT_SWEEP, fam, time.perf_counter())


@FAMILY
def test_k_sweep_weight_gradient(fam):
    wgrad_sweep('K_SWEEP weight gradient', [(c, (1, 2)) for c in sc.K_SWEEP], fam, time.perf_counter())


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_geometry_weight_gradient(stride):
    wgrad_sweep('GEOMETRY stride %d weight gradient' % stride, [(c, (1,)) for c in sc.GEOMETRY if c[7] == stride], 'small', time.perf_counter())


# ---- the pack and the data gradient ------------------------------------------------------------------------------------------------
def pack(c, w):
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    wt = new(cin, kh * kw * cout)
    return L().usot_conv_pack_dgrad_f32(hip.stream(), hip.ptr(w), hip.ptr(wt), cout, cin, kh, kw), wt


def dgrad(c, dy, w, wt, route):
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    dx = new(n, h, w_, cin)
    d = hip.grad_desc(route=route, dy=dy.data_ptr(), w=w.data_ptr(), wt=wt.data_ptr() if wt is not None else None, dx=dx.data_ptr(), **geo(c))
    return L().usot_conv2d_dgrad_f32(hip.stream(), C.byref(d)), dx


def dgrad_case(c, fam, holes=False):
    """route 1 (where route_a admits the case: it must succeed), 2 and 0 -> failure texts"""
    wd, dyd = put(sc.operand(c, fam, 'w')), put(sc.operand(c, fam, 'dy'))
    snaps = [('w', wd, guarded.snapshot(wd)), ('dy', dyd, guarded.snapshot(dyd))]
    rx = up(sc.reference_x(c, fam))
    tag = '%s %s' % (sc.case_id(c), fam)
    bad, wt = [], None
    if cg.route_a(c):
        rc, wt = pack(c, wd)
        m = 'return code %d' % rc if rc != OK else diff(wt, up(sc.ref_pack(c, sc.operand(c, fam, 'w'))))
        if m:
            bad.append('%s pack: %s' % (tag, m))
    for route in ((1, 2, 0) if wt is not None else (2, 0)):
        rc, dx = dgrad(c, dyd, wd, wt if route != 2 else None, route)
        m = 'return code %d' % rc if rc != OK else diff(dx, rx)
        if m:
            bad.append('%s route %d: %s' % (tag, route, m))
        elif holes and route == 2:
            hole = torch.from_numpy(~sc.reached(c)).to(DEV)
            if bool(dx[:, hole].contiguous().view(torch.int32).any()):
                bad.append('%s route 2: a pixel of dx no tap reaches is not +0.0' % tag)
    return bad + inputs_unchanged(snaps)


def dgrad_sweep(what, cases, fam, t0, holes=False):
    cases = [c for c in cases if sc.applies(c, fam, 'x')]
    bad = []
    for c in cases:
        bad += dgrad_case(c, fam, holes)
    report(what + ' ' + fam, len(cases), bad, t0, ', %d of them also with an explicit route 1' % sum(cg.route_a(c) for c in cases))


@FAMILY
def test_cout_sweep_route_b(fam):
    dgrad_sweep('COUT_ROUTE_B data gradient', sc.COUT_ROUTE_B, fam, time.perf_counter())


@FAMILY
def test_k_sweep_data_gradient(fam):
    dgrad_sweep('K_SWEEP data gradient', sc.K_SWEEP, fam, time.perf_counter())


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_geometry_data_gradient(stride):
    dgrad_sweep('GEOMETRY stride %d data gradient' % stride, [c for c in sc.GEOMETRY if c[7] == stride], 'small', time.perf_counter())


@FAMILY
def test_route_b_past_its_launch_cap(fam):
    c = sc.BIG['route_b']
    assert c[0] * c[1] * c[2] * c[3] // 4 > sc.DGRAD_CAP * sc.THREADS
    dgrad_sweep('BIG route B', [c], fam, time.perf_counter())


def test_pack_is_the_permutation():
    """arbitrary float32 bit patterns: the pack only moves them; BIG's bank needs a second pass of the grid-stride loop"""
    t0 = time.perf_counter()
    cases = sc.K_SWEEP + [sc.BIG['pack']]
    assert cases[-1][3] * cases[-1][4] * 9 > sc.PACK_CAP * sc.THREADS
    bad = []
    for c in cases:
        bank = sc.random_bank(c)
        wd = put(bank)
        snap = guarded.snapshot(wd)
        rc, wt = pack(c, wd)
        m = 'return code %d' % rc if rc != OK else diff(wt, up(sc.ref_pack(c, bank)))
        if m:
            bad.append('%s: %s' % (sc.case_id(c), m))
        bad += inputs_unchanged([('w', wd, snap)])
    report('K_SWEEP + BIG pack', len(cases), bad, t0)


# ---- x pixels no tap reads ------------------------------------------------------------------------------------------------------------
def test_unreached_pixels():
    """NaN in every x element that no (pixel, tap) reads: dw and db stay exact; dx is exactly +0.0 at those pixels"""
    t0 = time.perf_counter()
    bad, planted = [], 0
    for c in sc.UNREACHED:
        x = sc.operand(c, 'small', 'x').astype(np.float32)
        x[:, ~sc.reached(c)] = np.nan
        planted += int(np.isnan(x).sum())
        bad += wgrad_case(c, (1,), 'small', x=x)
        bad += dgrad_case(c, 'small', holes=True)
    assert planted > 0
    report('UNREACHED weight and data gradient', len(sc.UNREACHED), bad, t0, ', %d NaN planted' % planted)


# ---- refused launches ---------------------------------------------------------------------------------------------------------------
def test_refused_weight_gradient():
    """every entry is rejected by a host-side check of usot_conv2d_wgrad_f32 before anything is launched"""
    c = sc.REFUSED_BASE
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    m = sc.pixels(c)
    x, dy = put(sc.operand(c, 'small', 'x')), put(sc.operand(c, 'small', 'dy'))
    dw, db, ws = new(cout, kh * kw * cin), new(cout), new(3 * cout * (kh * kw * cin + 1))
    ptrs = dict(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(), ws=ws.data_ptr())

    def call(psplit=1, fields=(), **over):
        d = hip.grad_desc(psplit=psplit, **dict(geo(c), **{k: v for k, v in over.items() if k not in ptrs}))
        for k, v in dict(ptrs, **{k: v for k, v in over.items() if k in ptrs}).items():
            setattr(d, k, v)
        for k, v in fields:
            setattr(d, k, v)
        return L().usot_conv2d_wgrad_f32(hip.stream(), C.byref(d))
    refused = {
        'psplit_gt_M': lambda: call(psplit=m + 1),
        'psplit_no_ws': lambda: call(psplit=2, ws=None),
        'x_off4': lambda: call(x=ptrs['x'] + 4),
        'dy_off4': lambda: call(dy=ptrs['dy'] + 4),
        'dw_off4': lambda: call(dw=ptrs['dw'] + 4),
        'ws_off4': lambda: call(psplit=2, ws=ptrs['ws'] + 4),
        'cin48': lambda: call(Cin=48),
        'bad_oh': lambda: call(fields=[('OH', sc.out_hw(c)[0] + 1)]),
    }
    assert set(refused) | {'n0'} == set(sc.REFUSED_W)
    for name, fn in refused.items():
        assert fn() == EINVAL, name
    assert call(fields=[('N', 0)]) == OK and call(psplit=2, fields=[('N', 0)]) == OK        # no images: nothing to do, nothing written
    torch.cuda.synchronize()
    assert untouched(dw) and untouched(db) and untouched(ws)
    assert call(psplit=3) == OK                                                            # the same buffers do take a launch
    rw, rb = (up(a) for a in sc.reference_w(c, 'small'))
    assert not diff(dw, rw) and not diff(db, rb)


def test_refused_data_gradient():
    """every entry is rejected by a host-side check of usot_conv2d_dgrad_f32 (or of its route query) before anything is launched"""
    c = sc.REFUSED_BASE
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    w, dy = put(sc.operand(c, 'small', 'w')), put(sc.operand(c, 'small', 'dy'))
    rc, wt = pack(c, w)
    assert rc == OK
    dx = new(n, h, w_, cin)
    ptrs = dict(dy=dy.data_ptr(), w=w.data_ptr(), wt=wt.data_ptr(), dx=dx.data_ptr())

    def call(route=0, fields=(), **over):
        d = hip.grad_desc(route=route, **dict(geo(c), **{k: v for k, v in over.items() if k not in ptrs}))
        for k, v in dict(ptrs, **{k: v for k, v in over.items() if k in ptrs}).items():
            setattr(d, k, v)
        for k, v in fields:
            setattr(d, k, v)
        return L().usot_conv2d_dgrad_f32(hip.stream(), C.byref(d))
    for route in (0, 1, 2):
        assert call(route, dy=ptrs['dy'] + 4) == EINVAL and call(route, w=ptrs['w'] + 4) == EINVAL and call(route, dx=ptrs['dx'] + 4) == EINVAL
        assert call(route, Cin=48) == EINVAL and call(route, fields=[('OH', sc.out_hw(c)[0] + 1)]) == EINVAL
        assert call(route, fields=[('N', 0)]) == OK
    torch.cuda.synchronize()
    assert untouched(dx)
    rx = up(sc.reference_x(c, 'small'))
    assert call(1) == OK and not diff(dx, rx)
    # route A asked for on every configuration only route B serves: refused, no fall-back
    names = []
    for cfg in sc.ROUTE_B_ONLY_CONFIGS:
        cb = (1, 5, 9, 32, 32) + cfg
        names.append('route1_' + sc.config_id(cfg))
        assert not cg.route_a(cb)
        wb, dyb = put(sc.operand(cb, 'small', 'w')), put(sc.operand(cb, 'small', 'dy'))
        wtb = new(32, cfg[0] * cfg[1] * 32)
        rc, dxb = dgrad(cb, dyb, wb, wtb, 1)
        assert rc == EINVAL, cfg
        torch.cuda.synchronize()
        assert untouched(dxb) and untouched(wtb), cfg
        rc, dxb = dgrad(cb, dyb, wb, wtb, 0)
        assert rc == OK and not diff(dxb, up(sc.reference_x(cb, 'small'))) and untouched(wtb), cfg
    assert set(names) | {'dy_off4', 'w_off4', 'dx_off4', 'cin48', 'bad_oh', 'n0'} == set(sc.REFUSED_X)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', sc.PYTHON_SURFACE, ids=sc.case_id)
def test_python_surface(c):
    """hip.conv2d_backward_w / _x, hip.pack_dgrad and usot_amd.autograd.conv2d under torch.autograd.grad: the same references, =="""
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    x, w, dy = (put(sc.operand(c, 'small', name)) for name in ('x', 'w', 'dy'))
    snaps = [(name, t, guarded.snapshot(t)) for name, t in (('x', x), ('w', w), ('dy', dy))]
    rw, rb = (up(a) for a in sc.reference_w(c, 'small'))
    rx = up(sc.reference_x(c, 'small'))
    kws = dict(KH=kh, KW=kw, stride=s, pad=pad, dil=dil)
    for ps in (0, 1, 2):
        gw, gb = hip.conv2d_backward_w(x, dy, bias=True, psplit=ps, **kws)
        assert not diff(gw, rw) and not diff(gb, rb), ps
        gw, none = hip.conv2d_backward_w(x, dy, psplit=ps, **kws)
        assert none is None and not diff(gw, rw), ps
    for route in (0, 1, 2):
        assert not diff(hip.conv2d_backward_x(dy, w, x.shape, route=route, **kws), rx), route
    assert not diff(hip.pack_dgrad(w, cin, kh, kw), up(sc.ref_pack(c, sc.operand(c, 'small', 'w'))))
    xn = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
    wo = w.view(cout, kh, kw, cin).permute(0, 3, 1, 2).detach().requires_grad_(True)
    b = guarded.alloc((cout,), torch.float32, DEV, 'zero').requires_grad_(True)
    out = hip_autograd.conv2d(xn, wo, b, s, pad, dil)
    gx, gw, gb = torch.autograd.grad(out, (xn, wo, b), dy.permute(0, 3, 1, 2))
    assert gx.shape == xn.shape and gw.shape == wo.shape
    assert not diff(gx.permute(0, 2, 3, 1).contiguous(), rx)
    assert not diff(gw.permute(0, 2, 3, 1).reshape(cout, -1).contiguous(), rw) and not diff(gb, rb)
    assert not inputs_unchanged(snaps)
