"""GPU: BatchNorm2d forward and gradients (csrc/batchnorm.hip) and the surfaces over them (usot_amd.hip.batch_norm_forward /
batch_norm_backward, usot_amd.autograd.batch_norm, net.NormSlot, net.conv_norm) against F.batch_norm in float64 on the CPU.

Metric: the project's scaled error max |got - ref| / max(|ref|, mean|ref|); bar 1e-5, the bar tests/test_gpu_conv_grad.py holds
gradients to (PyTorch-CPU's own float32 batch_norm sits at <= 2e-6 from float64 on the families off = 0 and off = 2 of
tests/batchnorm_cases.py, for every output).  The float64 gradient reference takes its ReLU mask from the device's own y > 0;
separately no element outside rounding distance of zero may have the wrong mask (bc.mask_violations)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import batchnorm_cases as bc  # noqa: E402
import guarded  # noqa: E402
import usot_oracle as orc  # noqa: E402
from batchnorm_cases import rel_err  # noqa: E402
from usot_amd import autograd as hip_autograd, hip  # noqa: E402
from usot_amd.net import ConvSlot, NormSlot, _Gap, _seq, conv_norm  # noqa: E402

DEV = 'cuda:0'
BAR = 1e-5


@pytest.fixture(autouse=True)
def _memory_guard():
    """Every output a wrapper of usot_amd.hip / usot_amd.autograd allocates starts as NaN and sits between canaries
    (tests/guarded.py); the guards are checked when the test ends."""
    with guarded.patched(hip, hip_autograd):
        yield


def raw_forward(ops, training, relu, slices=0):
    """usot_batchnorm_fwd_f32 on NaN-filled outputs and a NaN-filled workspace of exactly usot_batchnorm_ws_floats floats, all
    between canaries -> dict of device tensors (y, save_mean, save_invstd, running_mean, running_var after the call, ws)"""
    x, gamma, beta, rmean, rvar, _ = ops
    ch = x.shape[-1]
    L = hip.lib()
    o = dict(x=guarded.put(x, DEV), gamma=guarded.put(gamma, DEV), beta=guarded.put(beta, DEV),
             running_mean=guarded.put(rmean, DEV), running_var=guarded.put(rvar, DEV))
    d = hip.bn_desc(M=x.numel() // ch, C=ch, eps=bc.EPS, momentum=bc.MOMENTUM, training=training,
                    act=hip.ACT_RELU if relu else hip.ACT_NONE, slices=slices)
    need = L.usot_batchnorm_ws_floats(C.byref(d))
    assert need > 0
    o['y'] = guarded.alloc(tuple(x.shape), torch.float32, DEV)
    o['save_mean'], o['save_invstd'] = guarded.alloc((ch,), torch.float32, DEV), guarded.alloc((ch,), torch.float32, DEV)
    o['ws'] = guarded.alloc((need,), torch.float32, DEV)
    for f in ('x', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'save_mean', 'save_invstd', 'ws'):
        setattr(d, f, o[f].data_ptr())
    snaps = {f: guarded.snapshot(o[f]) for f in ('x', 'gamma', 'beta')}
    if not training:
        d.save_mean = d.save_invstd = d.ws = None
        snaps.update({f: guarded.snapshot(o[f]) for f in ('running_mean', 'running_var', 'save_mean', 'save_invstd', 'ws')})
    hip.check(L.usot_batchnorm_fwd_f32(hip.stream(), C.byref(d)), 'usot_batchnorm_fwd_f32')
    for f, s in snaps.items():
        guarded.unchanged(o[f], s, f)
    o['slices'] = L.usot_batchnorm_slices(C.byref(d))
    return o


def raw_backward(ops, fwd, training, relu, slices=0, need=(True, True, True)):
    """usot_batchnorm_bwd_f32 on the operands and statistics of raw_forward -> (dx, dgamma, dbeta, ws), None where not asked"""
    x, dy = fwd['x'], guarded.put(ops[5], DEV)
    ch = x.shape[-1]
    L = hip.lib()
    d = hip.bn_desc(M=x.numel() // ch, C=ch, eps=bc.EPS, training=training, act=hip.ACT_RELU if relu else hip.ACT_NONE,
                    slices=slices, x=x.data_ptr(), dy=dy.data_ptr(), gamma=fwd['gamma'].data_ptr(), beta=fwd['beta'].data_ptr())
    if training:
        d.save_mean, d.save_invstd = fwd['save_mean'].data_ptr(), fwd['save_invstd'].data_ptr()
    else:
        d.running_mean, d.running_var = fwd['running_mean'].data_ptr(), fwd['running_var'].data_ptr()
    dx = guarded.alloc(tuple(x.shape), torch.float32, DEV) if need[0] else None
    dg = guarded.alloc((ch,), torch.float32, DEV) if need[1] else None
    db = guarded.alloc((ch,), torch.float32, DEV) if need[2] else None
    ws = guarded.alloc((L.usot_batchnorm_ws_floats(C.byref(d)),), torch.float32, DEV)
    d.dx, d.dgamma, d.dbeta, d.ws = hip.ptr(dx), hip.ptr(dg), hip.ptr(db), ws.data_ptr()
    ins = (x, dy, fwd['gamma'], fwd['beta'], fwd['running_mean'], fwd['running_var'], fwd['save_mean'], fwd['save_invstd'], fwd['y'])
    snaps = [guarded.snapshot(t) for t in ins]
    hip.check(L.usot_batchnorm_bwd_f32(hip.stream(), C.byref(d)), 'usot_batchnorm_bwd_f32')
    for t, s in zip(ins, snaps):
        guarded.unchanged(t, s)
    return dx, dg, db, ws


def check_against_float64(ops, fw64, training, relu, slices=0, tag=''):
    """forward and backward through the raw entry points; every output against float64 at BAR; the mask condition"""
    fwd = raw_forward(ops, training, relu, slices)
    dx, dg, db, _ = raw_backward(ops, fwd, training, relu, slices)
    pre = fw64['pre'].detach()
    errs = {'y': rel_err(fwd['y'], pre.clamp(min=0) if relu else pre)}
    if training:
        for f in ('save_mean', 'save_invstd', 'running_mean', 'running_var'):
            errs[f] = rel_err(fwd[f], fw64[f])
    mask = (fwd['y'].cpu() > 0) if relu else None
    if relu:
        assert bc.mask_violations(fwd['y'], pre) == 0
    rx, rg, rb = bc.grads_of(fw64, ops[5], mask)
    errs.update(dx=rel_err(dx, rx), dgamma=rel_err(dg, rg), dbeta=rel_err(db, rb))
    print('%s train %d relu %d slices %d: ' % (tag, training, relu, fwd['slices']) + ' '.join('%s %.3g' % kv for kv in errs.items()))
    return errs


# ---- 1. + 2. raw entry points, every output, and the ReLU mask -----------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('off', [0, 2])
@pytest.mark.parametrize('c', bc.CASES, ids=bc.case_id)
def test_raw_entry_points(c, off, training, relu):
    ops, fw64 = bc.reference(c, off, training)
    errs = check_against_float64(ops, fw64, training, relu, tag='%s off %d' % (bc.case_id(c), off))
    assert max(errs.values()) < BAR, errs


# ---- 3. the ill-conditioned family -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('c', bc.CASES, ids=bc.case_id)
def test_ill_conditioned_family(c, relu):
    """off = 32: channel means 32 spreads away from zero, where E[x^2] - E[x]^2 loses five digits.  PyTorch-CPU float32 is
    itself 1e-5 ... 3e-5 from float64 on y here, so the project's acceptance rule applies: per output, the
    HIP error may be at most max(1.5 x the float32 reference's error on the same operands, 1e-5)."""
    ops, fw64 = bc.reference(c, 32, True)
    hip_errs = check_against_float64(ops, fw64, True, relu, tag='%s off 32' % bc.case_id(c))
    fw32 = bc.forward_of(*ops[:5], True, dtype=torch.float32)
    pre64, pre32 = fw64['pre'].detach(), fw32['pre'].detach()
    t_errs = {'y': rel_err(pre32.clamp(min=0) if relu else pre32, pre64.clamp(min=0) if relu else pre64)}
    for f in ('running_mean', 'running_var'):
        t_errs[f] = rel_err(fw32[f], fw64[f])
    mask = (pre32 > 0) if relu else None                 # each float32 implementation is judged on its own mask
    for name, g32, g64 in zip(('dx', 'dgamma', 'dbeta'), bc.grads_of(fw32, ops[5], mask), bc.grads_of(fw64, ops[5], mask)):
        t_errs[name] = rel_err(g32, g64)
    print('%s off 32 relu %d: torch-cpu float32 ' % (bc.case_id(c), relu) + ' '.join('%s %.3g' % kv for kv in t_errs.items()))
    for name, e in hip_errs.items():
        bound = max(1.5 * t_errs.get(name, 0.0), BAR)    # save_mean / save_invstd: PyTorch does not hand them out; BAR
        assert e <= bound, (name, e, bound)


# ---- 4. slice and tile edges -------------------------------------------------------------------------------------------------
EDGE_M = {'R-1': lambda r: r - 1, 'R': lambda r: r, 'R+1': lambda r: r + 1, '2R+1': lambda r: 2 * r + 1, '3R-1': lambda r: 3 * r - 1}


def edge_case(m, ch, slices):
    c = (1, 1, m, ch)
    ops = bc.operands(c, 2)
    errs = check_against_float64(ops, bc.forward_of(*ops[:5], True), True, True, slices, tag='M %d C %d' % (m, ch))
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize('slices', [1, 2, 3, 'M'])
@pytest.mark.parametrize('mname', list(EDGE_M))
def test_row_slice_edges(mname, slices):
    """maps that end on, one before and one behind a row step, cut into slices of whole steps; slices = M: most own no step"""
    m = EDGE_M[mname](hip.batchnorm_geometry()[0])
    edge_case(m, 8, m if slices == 'M' else slices)


@pytest.mark.parametrize('cname', ['36', 'CB-4', 'CB', 'CB+4'])
def test_channel_block_edges(cname):
    r, cb = hip.batchnorm_geometry()
    edge_case(r + 1, {'36': 36, 'CB-4': cb - 4, 'CB': cb, 'CB+4': cb + 4}[cname], 2)


def test_workspace_is_exactly_what_the_query_says():
    """ws is [slices][2][C]: every float of a slice that owns rows is written, a slice without rows keeps the NaN pattern"""
    r, cb = hip.batchnorm_geometry()
    m, ch = 2 * r + 1, 36                                # three row steps
    ops = bc.operands((1, 1, m, ch), 2)
    for slices in (2, 5):
        fwd = raw_forward(ops, True, True, slices)
        _, _, _, bws = raw_backward(ops, fwd, True, True, slices)
        for ws in (fwd['ws'], bws):
            assert ws.numel() == 2 * slices * ch
            owns = [3 * (s + 1) // slices > 3 * s // slices for s in range(slices)]
            for s in range(slices):
                part = ws[2 * ch * s:2 * ch * (s + 1)]
                assert bool(torch.isfinite(part).all()) if owns[s] else bool(torch.isnan(part).all()), (slices, s)


# ---- 5. bit reproducibility ----------------------------------------------------------------------------------------------------
def test_deterministic():
    c = bc.CASES[5]
    ops, _ = bc.reference(c, 2, True)
    runs = []
    for _ in range(2):
        fwd = raw_forward(ops, True, True)
        runs.append([fwd[f] for f in ('y', 'save_mean', 'save_invstd', 'running_mean', 'running_var')]
                    + list(raw_backward(ops, fwd, True, True)[:3]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 6. python wrappers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [bc.CASES[1], bc.CASES[4]], ids=bc.case_id)
def test_python_bindings_match_raw_entry_points(c):
    ops, _ = bc.reference(c, 2, True)
    x, gamma, beta, rmean, rvar, dy = (t.to(DEV) for t in ops)
    for training in (True, False):
        for relu in (False, True):
            fwd = raw_forward(ops, training, relu)
            rm, rv = rmean.clone(), rvar.clone()
            y, mean, invstd = hip.batch_norm_forward(x, gamma, beta, rm, rv, training=training, momentum=bc.MOMENTUM, eps=bc.EPS,
                                                     relu=relu)
            assert torch.equal(y, fwd['y']) and torch.equal(rm, fwd['running_mean']) and torch.equal(rv, fwd['running_var'])
            if training:
                assert torch.equal(mean, fwd['save_mean']) and torch.equal(invstd, fwd['save_invstd'])
            else:
                assert mean is None and invstd is None
            raw = raw_backward(ops, fwd, training, relu)[:3]
            got = hip.batch_norm_backward(dy, x, gamma, beta, mean, invstd, rm, rv, training=training, eps=bc.EPS, relu=relu)
            assert all(torch.equal(a, b) for a, b in zip(got, raw))
            only = hip.batch_norm_backward(dy, x, gamma, beta, mean, invstd, rm, rv, training=training, eps=bc.EPS, relu=relu,
                                           need=(False, True, False))
            assert only[0] is None and only[2] is None and torch.equal(only[1], raw[1])
    with pytest.raises(hip.HipError):
        hip.batch_norm_forward(x[..., :-1], gamma, beta, rmean, rvar, training=True)             # not dense
    with pytest.raises(hip.HipError):
        hip.batch_norm_forward(x, gamma[:-4], beta, rmean, rvar, training=True)
    with pytest.raises(hip.HipError):
        hip.batch_norm_forward(x, gamma, beta, None, None, training=False)                       # eval needs the statistics
    with pytest.raises(hip.HipError):
        hip.batch_norm_backward(dy[:, :-1], x, gamma, beta, rmean, rvar, None, None, training=True)


# ---- 7. autograd surface -----------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """records the `need` of every call of hip.batch_norm_backward (usot_amd.autograd looks it up on the module at call time)"""
    calls = []
    real = hip.batch_norm_backward

    def counted(*a, **kw):
        calls.append(tuple(bool(v) for v in kw['need']))
        return real(*a, **kw)
    monkeypatch.setattr(hip, 'batch_norm_backward', counted)
    return calls


AUTOGRAD_CASE = bc.CASES[2]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
def test_autograd_batch_norm(training, relu, launches):
    ops, fw64 = bc.reference(AUTOGRAD_CASE, 2, training)
    x, gamma, beta, rmean, rvar, dy = (t.to(DEV) for t in ops)
    xn, dyn = bc.nchw(x), bc.nchw(dy)                    # NCHW-shaped views of channels-last memory
    plain, _, _ = hip.batch_norm_forward(x, gamma, beta, rmean.clone(), rvar.clone(), training=training, momentum=bc.MOMENTUM,
                                         eps=bc.EPS, relu=relu)
    # nothing requires grad: no node, but the running statistics move in training mode
    rm, rv = rmean.clone(), rvar.clone()
    off = hip_autograd.batch_norm(xn, gamma, beta, rm, rv, training, bc.MOMENTUM, bc.EPS, relu)
    assert off.grad_fn is None and not off.requires_grad and torch.equal(off.permute(0, 2, 3, 1), plain)
    assert off.shape == xn.shape and off.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(rm, rmean) != training and torch.equal(rv, rvar) != training
    assert rel_err(rm, fw64['running_mean']) < BAR and rel_err(rv, fw64['running_var']) < BAR
    xg, gg, bg = xn.clone(memory_format=torch.preserve_format).requires_grad_(True), gamma.clone().requires_grad_(True), \
        beta.clone().requires_grad_(True)
    rm2, rv2 = rmean.clone(), rvar.clone()
    with torch.no_grad():
        assert hip_autograd.batch_norm(xg, gg, bg, rm2, rv2, training, bc.MOMENTUM, bc.EPS, relu).grad_fn is None
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv)
    rm3, rv3 = rmean.clone(), rvar.clone()
    out = hip_autograd.batch_norm(xg, gg, bg, rm3, rv3, training, bc.MOMENTUM, bc.EPS, relu)
    assert out.grad_fn is not None and torch.equal(out.detach().permute(0, 2, 3, 1), plain)
    assert torch.equal(rm3, rm) and torch.equal(rv3, rv)
    got = torch.autograd.grad(out, (xg, gg, bg), dyn)
    assert launches == [(True, True, True)]
    mask = (plain.cpu() > 0) if relu else None
    ref = bc.grads_of(fw64, ops[5], mask)
    errs = [rel_err(got[0].permute(0, 2, 3, 1), ref[0]), rel_err(got[1], ref[1]), rel_err(got[2], ref[2])]
    print('train %d relu %d: dx %.3g dgamma %.3g dbeta %.3g' % (training, relu, *errs))
    assert max(errs) < BAR, errs


def test_autograd_only_what_is_asked(launches):
    ops, fw64 = bc.reference(AUTOGRAD_CASE, 2, True)
    x, gamma, beta, rmean, rvar, dy = (t.to(DEV) for t in ops)
    xn, dyn = bc.nchw(x), bc.nchw(dy)
    mask = hip.batch_norm_forward(x, gamma, beta, None, None, training=True, relu=True)[0].cpu() > 0
    rx, rg, rb = bc.grads_of(fw64, ops[5], mask)
    bn = lambda a, w, b, training=True: hip_autograd.batch_norm(a, w, b, rmean.clone(), rvar.clone(), training, relu=True)
    xg = xn.clone(memory_format=torch.preserve_format).requires_grad_(True)
    gx, = torch.autograd.grad(bn(xg, gamma, beta), (xg,), dyn)
    assert launches == [(True, False, False)] and rel_err(gx.permute(0, 2, 3, 1), rx) < BAR
    wg = gamma.clone().requires_grad_(True)
    bn(xn, wg, beta).backward(dyn)
    assert launches[1:] == [(False, True, False)] and rel_err(wg.grad, rg) < BAR
    bg = beta.clone().requires_grad_(True)
    gb, = torch.autograd.grad(bn(xn, gamma, bg), (bg,), dyn)
    assert launches[2:] == [(False, False, True)] and rel_err(gb, rb) < BAR
    # eval mode, dx alone: the elementwise launch, no workspace
    gxe, = torch.autograd.grad(bn(xg, gamma, beta, training=False), (xg,), dyn)
    assert launches[3:] == [(True, False, False)]
    fe = bc.reference(AUTOGRAD_CASE, 2, False)[1]
    ye = hip.batch_norm_forward(x, gamma, beta, rmean, rvar, training=False, relu=True)[0].cpu()
    assert rel_err(gxe.permute(0, 2, 3, 1), bc.grads_of(fe, ops[5], ye > 0)[0]) < BAR
    # a gradient with the strides of an expanded scalar (what .sum().backward() hands over), and untracked statistics
    out = hip_autograd.batch_norm(xg, gamma, beta, None, None, True, relu=True)
    gx1, = torch.autograd.grad(out.sum(), (xg,))
    assert rel_err(gx1.permute(0, 2, 3, 1), bc.grads_of(fw64, torch.ones_like(ops[5]), mask)[0]) < BAR


def test_nchw_and_channels_last_inputs_agree():
    ops, _ = bc.reference(AUTOGRAD_CASE, 2, True)
    x, gamma, beta, rmean, rvar, dy = (t.to(DEV) for t in ops)
    res = []
    for xin, dyin in ((bc.nchw(x), bc.nchw(dy)), (bc.nchw(x).contiguous(), bc.nchw(dy).contiguous())):
        assert xin.is_contiguous() == (len(res) == 1)
        xg, gg, bg = xin.clone(memory_format=torch.preserve_format).requires_grad_(True), gamma.clone().requires_grad_(True), \
            beta.clone().requires_grad_(True)
        rm, rv = rmean.clone(), rvar.clone()
        out = hip_autograd.batch_norm(xg, gg, bg, rm, rv, True, relu=True)
        res.append([out.detach(), rm, rv] + list(torch.autograd.grad(out, (xg, gg, bg), dyin)))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_channels_last_input_is_not_copied(monkeypatch):
    """what autograd.conv2d returns goes into the kernel as it is: the permute kernel does not run"""
    ops, _ = bc.reference(AUTOGRAD_CASE, 2, True)
    x, gamma, beta = (t.to(DEV) for t in ops[:3])
    seen = []
    real = hip.batch_norm_forward
    monkeypatch.setattr(hip, 'batch_norm_forward', lambda xh, *a, **kw: (seen.append(xh.data_ptr()), real(xh, *a, **kw))[1])
    xg = bc.nchw(x).requires_grad_(True)
    hip_autograd.batch_norm(xg, gamma, beta, None, None, True)
    hip_autograd.batch_norm(bc.nchw(x), gamma, beta, None, None, True)
    assert seen == [x.data_ptr(), x.data_ptr()]


# ---- 8. NormSlot and conv_norm ---------------------------------------------------------------------------------------------
def norm_slot(ops):
    x, gamma, beta, rmean, rvar, dy = ops
    slot = NormSlot(x.shape[-1])
    with torch.no_grad():
        slot.weight.copy_(gamma), slot.bias.copy_(beta), slot.running_mean.copy_(rmean), slot.running_var.copy_(rvar)
    return slot.to(DEV)


def test_norm_slot_training():
    ops, fw64 = bc.reference(AUTOGRAD_CASE, 2, True)
    x, dy = bc.nchw(ops[0].to(DEV)), bc.nchw(ops[5].to(DEV))
    slot = norm_slot(ops).train()
    y = slot(x)
    assert y.grad_fn is None and int(slot.num_batches_tracked) == 1
    assert rel_err(y.permute(0, 2, 3, 1), fw64['pre']) < BAR
    assert rel_err(slot.running_mean, fw64['running_mean']) < BAR and rel_err(slot.running_var, fw64['running_var']) < BAR
    slot.weight.requires_grad_(True), slot.bias.requires_grad_(True)
    y = slot(x, relu=True)
    assert int(slot.num_batches_tracked) == 2 and slot.num_batches_tracked.is_cuda
    y.backward(dy)
    _, rg, rb = bc.grads_of(fw64, ops[5], y.detach().permute(0, 2, 3, 1).cpu() > 0)
    eg, eb = rel_err(slot.weight.grad, rg), rel_err(slot.bias.grad, rb)
    print('NormSlot(%d).train(): dweight %.3g dbias %.3g' % (ops[0].shape[-1], eg, eb))
    assert eg < BAR and eb < BAR


def test_norm_slot_eval_is_the_folded_inference_arithmetic():
    ops, _ = bc.reference(AUTOGRAD_CASE, 2, False)
    x, gamma, beta, rmean, rvar, _ = ops
    slot = norm_slot(ops).eval()
    y = slot(bc.nchw(x.to(DEV)))
    a = gamma.double() / torch.sqrt(rvar.double() + NormSlot.eps)          # what the engine folds into the conv bank
    b = beta.double() - rmean.double() * a
    assert int(slot.num_batches_tracked) == 0
    assert torch.equal(slot.running_mean.cpu(), rmean) and torch.equal(slot.running_var.cpu(), rvar)
    assert rel_err(y.permute(0, 2, 3, 1), x.double() * a + b) < BAR
    assert rel_err(slot(bc.nchw(x.to(DEV)), relu=True).permute(0, 2, 3, 1), (x.double() * a + b).clamp(min=0)) < BAR


def test_conv_norm_holder():
    """conv (bias) -> BN (training) -> ReLU through the holders against float64 autograd: dx and the gradients of the conv's
    weight and bias and the BN's weight and bias.  The conv bias cancels in a training-mode BN: its gradient is a sum that
    is zero in exact arithmetic, so it is held to 1e-5 of the sum of the magnitudes of its terms, not of itself."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 32, 9, 8, generator=g)
    w = torch.randn(40, 32, 3, 3, generator=g) / 288 ** 0.5
    b = torch.randn(40, generator=g)
    gamma = (0.5 + torch.rand(40, generator=g)) * (torch.randint(0, 2, (40,), generator=g).float() * 2 - 1)
    beta = 0.3 * torch.randn(40, generator=g)
    dy = torch.randn(2, 40, 9, 8, generator=g)
    seq = _seq(ConvSlot(32, 40, 3, pad=1, bias=True), NormSlot(40), _Gap())
    with torch.no_grad():
        seq[0].weight.copy_(w), seq[0].bias.copy_(b), seq[1].weight.copy_(gamma), seq[1].bias.copy_(beta)
    seq = seq.to(DEV).train()
    params = [seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias]
    for p in params:
        p.requires_grad_(True)
    xd = x.to(DEV).requires_grad_(True)
    y = conv_norm(seq, xd)
    assert int(seq[1].num_batches_tracked) == 1
    got = torch.autograd.grad(y, [xd] + params, dy.to(DEV))
    leaves = [t.double().requires_grad_(True) for t in (x, w, b, gamma, beta)]
    conv = F.conv2d(leaves[0], leaves[1], leaves[2], padding=1)
    pre = F.batch_norm(conv, None, None, leaves[3], leaves[4], True, 0.1, NormSlot.eps)
    assert bc.mask_violations(y.detach().permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)) == 0
    mask = (y.detach().cpu() > 0).double()
    assert rel_err(y, pre.detach().clamp(min=0)) < BAR
    ref = torch.autograd.grad(pre * mask, leaves + [conv], dy.double())
    errs = {n: rel_err(a, r) for n, a, r in zip(('dx', 'conv.weight', 'conv.bias', 'bn.weight', 'bn.bias'), got, ref) if n != 'conv.bias'}
    terms = ref[5].abs().sum((0, 2, 3)).mean()           # per channel: sum over pixels of |d loss / d conv output|
    errs['conv.bias'] = float((got[2].cpu().double() - ref[2]).abs().max() / terms)
    print('conv_norm: ' + ' '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) < BAR, errs
    with torch.no_grad():                                # without the _Gap: no ReLU
        y2 = conv_norm(_seq(seq[0], seq[1]), xd)
    assert rel_err(y2, pre.detach()) < BAR and float(y2.min()) < 0


# ---- 9. chained: the head's encoder -> GroupDW -> tower -> prediction path with its BatchNorms -----------------------------
DILS = ((1, 1), (2, 1), (1, 2))
LOGITS = (0.3, -0.2, 0.9)
CHAIN_SEED = 2024


def chain(conv_bn, conv, groupdw, z, x, banks, affine, logits):
    """three encoders (conv + BN + ReLU) per side -> GroupDW -> tower conv + BN + ReLU -> conv to 4 channels -> sum of squares"""
    zs = [conv_bn(z, banks[i], affine[2 * i], affine[2 * i + 1], dilation=DILS[i]) for i in range(3)]
    xs = [conv_bn(x, banks[3 + i], affine[6 + 2 * i], affine[7 + 2 * i], dilation=DILS[i]) for i in range(3)]
    f = groupdw(zs, xs, logits)
    f = conv_bn(f, banks[6], affine[12], affine[13], padding=1)
    return conv(f, banks[7], padding=1).square().sum()


def test_chain_of_encoders_correlation_and_tower_with_batch_norm():
    C_ = 32
    g = torch.Generator().manual_seed(CHAIN_SEED)
    z, x = torch.randn(2, C_, 7, 7, generator=g), torch.randn(2, C_, 15, 15, generator=g)
    banks = [torch.randn(C_, C_, 3, 3, generator=g) / (9 * C_) ** 0.5 for _ in range(7)]
    banks.append(torch.randn(4, C_, 3, 3, generator=g) / (9 * C_) ** 0.5)
    affine = []
    for _ in range(7):
        affine.append((0.5 + torch.rand(C_, generator=g)) * (torch.randint(0, 2, (C_,), generator=g).float() * 2 - 1))
        affine.append(0.3 * torch.randn(C_, generator=g))
    logits = torch.tensor(LOGITS)
    outs, pres = [], []

    def gconv(t, w, padding=0, dilation=1):
        return hip_autograd.conv2d(t, w, None, 1, padding, dilation)

    def gconv_bn(t, w, gamma, beta, padding=0, dilation=1):
        y = hip_autograd.batch_norm(gconv(t, w, padding, dilation), gamma, beta, None, None, True, relu=True)
        outs.append(y.detach().cpu())
        return y

    def conv64(t, w, padding=0, dilation=1):
        return F.conv2d(t, w, None, padding=padding, dilation=dilation)

    def conv_bn64(t, w, gamma, beta, padding=0, dilation=1):
        pre = F.batch_norm(conv64(t, w, padding, dilation), None, None, gamma, beta, True, 0.1, 1e-5)
        pres.append(pre.detach())
        return pre * (outs[len(pres) - 1] > 0).double()             # the device's own mask, layer by layer

    def gdw64(zs, xs, w):
        return orc.groupdw({'connect_model.cls_dw.weight': w}, 'cls_dw', zs, xs)

    leaves = [t.to(DEV).requires_grad_(True) for t in banks + affine + [logits, z, x]]
    loss = chain(gconv_bn, gconv, hip_autograd.groupdw, leaves[23], leaves[24], leaves[:8], leaves[8:22], leaves[22])
    got = torch.autograd.grad(loss, leaves)
    leaves64 = [t.double().requires_grad_(True) for t in banks + affine + [logits, z, x]]
    loss64 = chain(conv_bn64, conv64, gdw64, leaves64[23], leaves64[24], leaves64[:8], leaves64[8:22], leaves64[22])
    ref = torch.autograd.grad(loss64, leaves64)
    assert len(outs) == len(pres) == 7
    for i, (y, pre) in enumerate(zip(outs, pres)):       # a seed that puts an element inside the band is replaced, not excused
        assert bc.mask_violations(y.permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)) == 0, i
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    layers = ['enc_z%d' % i for i in range(3)] + ['enc_x%d' % i for i in range(3)] + ['tower']
    names = layers + ['pred'] + [n + s for n in layers for s in ('.gamma', '.beta')] + ['logits', 'z', 'x']
    errs = {name: rel_err(gt, rf) for name, gt, rf in zip(names, got, ref)}
    print('chain: ' + ' '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) < BAR, errs
