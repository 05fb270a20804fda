"""GPU: BatchNorm - add - ReLU (csrc/batchnorm.hip, usot_bn_add_desc), its bindings (usot_amd.hip.batch_norm_add_forward /
_backward, usot_amd.autograd.batch_norm_add, NormSlot's `residual`) and the holders that run on it - BottleneckSlots,
ResNetPlus2Slots, BackboneSlots, NeckSlots - against the float64 restatement of tests/backbone_cases.py on the CPU.

Metric: the project's scaled error max |got - ref| / max(|ref|, mean|ref|).  Raw entry points, bindings and autograd: bar 1e-5,
the bar of tests/test_gpu_batchnorm.py.  Holders: the acceptance rule of DESIGN.md section 5 as tests/test_gpu_head_grad.py
applies it - per tensor the HIP error may be at most max(1e-5, 1.5 x the error of the float32 CPU restatement with the same
masks); both are printed.  The float64 reference takes its ReLU masks from the device's own outputs (forward hooks on the
NormSlots); separately no element outside rounding distance of zero may have the wrong mask (bc.mask_violations).

Worst measured per group on one MI355X (HIP, and beside it the float32 CPU restatement where the rule applies): raw entry points
1.6e-6 (dgamma, M = 3); reduction edges 7.6e-7; autograd over the 15 subsets 3.9e-7; BottleneckSlots 1.39e-5 / 1.26e-5
(conv2.weight gradient, layer3's first block, eval); ResNetPlus2Slots depth 1 1.41e-5 / 1.46e-5, full depth 2.7e-5 / 2.14e-5
(layer1.0.bn1.weight gradient); NeckSlots 7.5e-6 / 8.4e-6 (input gradient, pooled form); eval forward against engine.features
9.9e-6; backbone -> neck -> head chain 2.46e-5 / 2.28e-5 (cls_encode.matrix21_k.1.weight gradient, 93 tensors)."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_cases as bk  # noqa: E402
import batchnorm_cases as bc  # noqa: E402
import guarded  # noqa: E402
import head_grad_cases as hc  # noqa: E402
from batchnorm_cases import rel_err  # noqa: E402
from usot_amd import autograd as hip_autograd, hip, synth  # noqa: E402
from usot_amd.net import (BackboneSlots, BottleneckSlots, ConvSlot, HeadSlots, NeckSlots, NormSlot, ResNetPlus2Slots,  # noqa: E402
                          _seq)

DEV = 'cuda:0'
BAR = 1e-5


@pytest.fixture(autouse=True)
def _memory_guard():
    with guarded.patched(hip, hip_autograd):
        yield


# ---- raw calls -----------------------------------------------------------------------------------------------------------------------
def raw_forward(ops, training, relu, slices=0, res=None):
    """usot_batchnorm_add_fwd_f32 on NaN-filled outputs and a NaN-filled workspace of exactly usot_batchnorm_ws_floats floats, all
    between canaries -> dict of device tensors"""
    x, gamma, beta, rmean, rvar = ops[:5]
    res = ops[6] if res is None else res
    ch = x.shape[-1]
    L = hip.lib()
    o = dict(x=guarded.put(x, DEV), gamma=guarded.put(gamma, DEV), beta=guarded.put(beta, DEV), res=guarded.put(res, DEV),
             running_mean=guarded.put(rmean, DEV), running_var=guarded.put(rvar, DEV))
    d = hip.bn_add_desc(M=x.numel() // ch, C=ch, eps=bc.EPS, momentum=bc.MOMENTUM, training=training,
                        act=hip.ACT_RELU if relu else hip.ACT_NONE, slices=slices)
    need = L.usot_batchnorm_ws_floats(C.byref(d.bn))
    assert need > 0
    o['y'] = guarded.alloc(tuple(x.shape), torch.float32, DEV)
    o['save_mean'], o['save_invstd'] = guarded.alloc((ch,), torch.float32, DEV), guarded.alloc((ch,), torch.float32, DEV)
    o['ws'] = guarded.alloc((need,), torch.float32, DEV)
    for f in ('x', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'save_mean', 'save_invstd', 'ws'):
        setattr(d.bn, f, o[f].data_ptr())
    d.res = o['res'].data_ptr()
    snaps = {f: guarded.snapshot(o[f]) for f in ('x', 'gamma', 'beta', 'res')}
    if not training:
        d.bn.save_mean = d.bn.save_invstd = d.bn.ws = None
        snaps.update({f: guarded.snapshot(o[f]) for f in ('running_mean', 'running_var', 'save_mean', 'save_invstd', 'ws')})
    hip.check(L.usot_batchnorm_add_fwd_f32(hip.stream(), C.byref(d)), 'usot_batchnorm_add_fwd_f32')
    for f, s in snaps.items():
        guarded.unchanged(o[f], s, f)
    o['slices'] = L.usot_batchnorm_slices(C.byref(d.bn))
    return o


def raw_backward(ops, fwd, training, relu, slices=0, need=(True, True, True), dy=None):
    """usot_batchnorm_add_bwd_f32 on the operands and statistics of raw_forward; need = (dx, dgamma and dbeta, dres) ->
    (dx, dgamma, dbeta, dres), None where not asked"""
    x, dy = fwd['x'], guarded.put(ops[5] if dy is None else dy, DEV)
    ch = x.shape[-1]
    L = hip.lib()
    d = hip.bn_add_desc(M=x.numel() // ch, C=ch, eps=bc.EPS, training=training, act=hip.ACT_RELU if relu else hip.ACT_NONE,
                        slices=slices, x=x.data_ptr(), dy=dy.data_ptr(), gamma=fwd['gamma'].data_ptr(), beta=fwd['beta'].data_ptr(),
                        res=fwd['res'].data_ptr())
    if training:
        d.bn.save_mean, d.bn.save_invstd = fwd['save_mean'].data_ptr(), fwd['save_invstd'].data_ptr()
    else:
        d.bn.running_mean, d.bn.running_var = fwd['running_mean'].data_ptr(), fwd['running_var'].data_ptr()
    dx = guarded.alloc(tuple(x.shape), torch.float32, DEV) if need[0] else None
    dg = guarded.alloc((ch,), torch.float32, DEV) if need[1] else None
    db = guarded.alloc((ch,), torch.float32, DEV) if need[1] else None
    dr = guarded.alloc(tuple(x.shape), torch.float32, DEV) if need[2] else None
    ws = guarded.alloc((L.usot_batchnorm_ws_floats(C.byref(d.bn)),), torch.float32, DEV)
    d.bn.dx, d.bn.dgamma, d.bn.dbeta, d.bn.ws, d.dres = hip.ptr(dx), hip.ptr(dg), hip.ptr(db), ws.data_ptr(), hip.ptr(dr)
    reduces = need[1] or (training and need[0])
    ins = [x, dy, fwd['res'], fwd['gamma'], fwd['beta'], fwd['running_mean'], fwd['running_var'], fwd['save_mean'], fwd['save_invstd'],
           fwd['y']] + ([] if reduces else [ws])         # a call without a reduction leaves the workspace alone
    snaps = [guarded.snapshot(t) for t in ins]
    hip.check(L.usot_batchnorm_add_bwd_f32(hip.stream(), C.byref(d)), 'usot_batchnorm_add_bwd_f32')
    for t, s in zip(ins, snaps):
        guarded.unchanged(t, s)
    return dx, dg, db, dr


_refs = {}


def reference(c, off, training):
    """(operands, float64 forward with the residual leaf) of a case; shared between tests, read-only"""
    key = (c, off, training)
    if key not in _refs:
        ops = bk.operands(c, off)
        _refs[key] = (ops, bk.add_forward_of(ops, training))
    return _refs[key]


def check_against_float64(ops, fw64, training, relu, slices=0, tag=''):
    fwd = raw_forward(ops, training, relu, slices)
    dx, dg, db, dr = raw_backward(ops, fwd, training, relu, slices)
    s = fw64['s'].detach()
    errs = {'y': rel_err(fwd['y'], s.clamp(min=0) if relu else s)}
    if training:
        for f in ('save_mean', 'save_invstd', 'running_mean', 'running_var'):
            errs[f] = rel_err(fwd[f], fw64[f])
    mask = (fwd['y'].cpu() > 0) if relu else None
    if relu:
        assert bc.mask_violations(fwd['y'], s) == 0
    rx, rg, rb, rr = bk.add_grads_of(fw64, ops[5], mask)
    errs.update(dx=rel_err(dx, rx), dgamma=rel_err(dg, rg), dbeta=rel_err(db, rb), dres=rel_err(dr, rr))
    print('%s train %d relu %d slices %d: ' % (tag, training, relu, fwd['slices']) + ' '.join('%s %.3g' % kv for kv in errs.items()))
    return errs, fwd, (dx, dg, db, dr)


# ---- 1. raw entry points against float64, every combination of wanted outputs ----------------------------------------------------
RAW = [(c, off, training, relu) for c in bc.CASES[:6] for off in (0, 2) for training in (True, False) for relu in (False, True)] \
    + [(bc.CASES[6], 2, training, True) for training in (True, False)]
NEEDS = [n for n in itertools.product((True, False), repeat=3) if any(n)]


@pytest.mark.parametrize('c,off,training,relu', RAW, ids=lambda v: bc.case_id(v) if isinstance(v, tuple) else str(int(v)))
def test_raw_entry_points(c, off, training, relu):
    ops, fw64 = reference(c, off, training)
    errs, fwd, full = check_against_float64(ops, fw64, training, relu, tag='%s off %d' % (bc.case_id(c), off))
    assert max(errs.values()) < BAR, errs
    for need in NEEDS[1:]:                               # a subset: the wanted ones are the full call's bits, the others are NULL
        dx, dg, db, dr = raw_backward(ops, fwd, training, relu, need=need)
        assert (dx is None) == (not need[0]) and (dg is None) == (not need[1]) and (dr is None) == (not need[2])
        for got, want in zip((dx, dg, db, dr), full):
            assert got is None or torch.equal(got, want), need


# ---- 2. the tie to the plain kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('c', [bc.CASES[1], bc.CASES[2]], ids=bc.case_id)
def test_zero_residual_is_the_plain_batch_norm_bit_for_bit(c, training, relu):
    ops = bk.operands(c, 2)
    x, gamma, beta, rmean, rvar, dy = (t.to(DEV) for t in ops[:6])
    fwd = raw_forward(ops, training, relu, res=torch.zeros_like(ops[0]))
    dx, dg, db, dr = raw_backward(ops, fwd, training, relu)
    rm, rv = rmean.clone(), rvar.clone()
    y, mean, invstd = hip.batch_norm_forward(x, gamma, beta, rm, rv, training=training, momentum=bc.MOMENTUM, eps=bc.EPS, relu=relu)
    px, pg, pb = hip.batch_norm_backward(dy, x, gamma, beta, mean, invstd, rm, rv, training=training, eps=bc.EPS, relu=relu)
    assert torch.equal(fwd['y'], y) and torch.equal(fwd['running_mean'], rm) and torch.equal(fwd['running_var'], rv)
    if training:
        assert torch.equal(fwd['save_mean'], mean) and torch.equal(fwd['save_invstd'], invstd)
    assert torch.equal(dx, px) and torch.equal(dg, pg) and torch.equal(db, pb)
    assert torch.equal(dr, dy * (y > 0) if relu else dy)


# ---- 3. the mask at the threshold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('training', [True, False])
def test_forward_and_backward_agree_on_the_mask_at_the_threshold(training):
    """on a seeded third of the elements res = -fl32(pre64) + k ulp, k in {-1, 0, 1}: the sum is zero or an ulp from it.  With
    dy = 1, dres is the backward's mask and y > 0 the forward's: equal element for element, whatever float64 says."""
    c = bc.CASES[2]
    ops = bk.operands(c, 2)
    pre = bc.forward_of(*ops[:5], training)['pre'].detach().float()
    g = torch.Generator().manual_seed(2718 + training)
    pick = torch.rand(pre.shape, generator=g) < 1 / 3
    k = torch.randint(-1, 2, pre.shape, generator=g)
    planted = -pre
    for kk, toward in ((-1, -float('inf')), (1, float('inf'))):
        planted = torch.where(k == kk, torch.nextafter(-pre, torch.full_like(pre, toward)), planted)
    res = torch.where(pick, planted, ops[6])
    fwd = raw_forward(ops, training, True, res=res)
    _, _, _, dr = raw_backward(ops, fwd, training, True, need=(False, False, True), dy=torch.ones_like(ops[5]))
    y = fwd['y']
    assert torch.equal(dr, (y > 0).float())
    near = (y.cpu().abs() <= 1e-5 * (pre.abs() + pre.abs().mean())) & pick
    assert int(near.sum()) > 0.25 * pre.numel()          # the planted elements did land on the threshold
    assert 0 < int((y.cpu()[near] > 0).sum()) < int(near.sum())
    dx, dg, db, dr2 = raw_backward(ops, fwd, training, True, dy=torch.ones_like(ops[5]))
    assert torch.equal(dr2, dr) and rel_err(db, dr.double().reshape(-1, c[3]).sum(0)) < BAR          # dbeta counts that very mask


# ---- 4. reduction edges, reproducibility -------------------------------------------------------------------------------------------
def _edges():
    m = bc.CASES[2][0] * bc.CASES[2][1] * bc.CASES[2][2]
    steps = -(-m // 64)
    return [(bc.CASES[2], s) for s in (1, 2, steps, steps + 1, m)] + [(bc.CASES[0], 0), (bc.CASES[0], 3), (bc.CASES[1], 0), (bc.CASES[1], 2)]


@pytest.mark.parametrize('c,slices', _edges(), ids=lambda v: bc.case_id(v) if isinstance(v, tuple) else 's%d' % v)
def test_reduction_edges_twice(c, slices):
    assert hip.batchnorm_geometry() == (64, 64)
    ops = bk.operands(c, 2)
    fw64 = bk.add_forward_of(ops, True)
    runs = []
    for _ in range(2):
        errs, fwd, grads = check_against_float64(ops, fw64, True, True, slices, tag='%s slices %d' % (bc.case_id(c), slices))
        assert max(errs.values()) < BAR, errs
        runs.append([fwd[f] for f in ('y', 'save_mean', 'save_invstd', 'running_mean', 'running_var')] + list(grads))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 5. bindings and autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [bc.CASES[1], bc.CASES[4]], ids=bc.case_id)
def test_python_bindings_match_raw_entry_points(c):
    ops = bk.operands(c, 2)
    x, gamma, beta, rmean, rvar, dy, res = (t.to(DEV) for t in ops)
    for training in (True, False):
        for relu in (False, True):
            fwd = raw_forward(ops, training, relu)
            rm, rv = rmean.clone(), rvar.clone()
            y, mean, invstd = hip.batch_norm_add_forward(x, res, gamma, beta, rm, rv, training=training, momentum=bc.MOMENTUM,
                                                         eps=bc.EPS, relu=relu)
            assert torch.equal(y, fwd['y']) and torch.equal(rm, fwd['running_mean']) and torch.equal(rv, fwd['running_var'])
            if training:
                assert torch.equal(mean, fwd['save_mean']) and torch.equal(invstd, fwd['save_invstd'])
            else:
                assert mean is None and invstd is None
            raw = raw_backward(ops, fwd, training, relu)
            got = hip.batch_norm_add_backward(dy, x, res, gamma, beta, mean, invstd, rm, rv, training=training, eps=bc.EPS, relu=relu)
            assert all(torch.equal(a, b) for a, b in zip(got, raw))
            only = hip.batch_norm_add_backward(dy, x, res, gamma, beta, mean, invstd, rm, rv, training=training, eps=bc.EPS, relu=relu,
                                               need=(False, False, False, True))
            assert only[:3] == (None, None, None) and torch.equal(only[3], raw[3])
    with pytest.raises(hip.HipError):
        hip.batch_norm_add_forward(x, res, gamma, beta, None, None, training=False)              # eval needs the statistics
    with pytest.raises(hip.HipError):
        hip.batch_norm_add_forward(x, res.cpu(), gamma, beta, rmean, rvar, training=True)


AUTOGRAD_CASE = bc.CASES[2]
SUBSETS = [s for s in itertools.product((False, True), repeat=4) if any(s)]


@pytest.mark.parametrize('training', [True, False])
def test_autograd_batch_norm_add_every_subset_of_inputs(training, monkeypatch):
    ops, fw64 = reference(AUTOGRAD_CASE, 2, training)
    x, gamma, beta, rmean, rvar, dy, res = (t.to(DEV) for t in ops)
    xn, rn, dyn = bc.nchw(x), bc.nchw(res), bc.nchw(dy)
    plain = hip.batch_norm_add_forward(x, res, gamma, beta, rmean.clone(), rvar.clone(), training=training, momentum=bc.MOMENTUM,
                                       eps=bc.EPS)[0]
    ref = bk.add_grads_of(fw64, ops[5], plain.cpu() > 0)
    ref = (ref[0], ref[3], ref[1], ref[2])               # the order of batch_norm_add's arguments: x, residual, weight, bias
    needs = []
    real = hip.batch_norm_add_backward
    monkeypatch.setattr(hip, 'batch_norm_add_backward', lambda *a, **kw: (needs.append(tuple(bool(v) for v in kw['need'])), real(*a, **kw))[1])
    # nothing requires grad, or grad mode is off: no node, but the running statistics move in training mode
    rm, rv = rmean.clone(), rvar.clone()
    off = hip_autograd.batch_norm_add(xn, rn, gamma, beta, rm, rv, training, bc.MOMENTUM, bc.EPS)
    assert off.grad_fn is None and torch.equal(off.permute(0, 2, 3, 1), plain) and off.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(rm, rmean) != training and torch.equal(rv, rvar) != training
    rm2, rv2 = rmean.clone(), rvar.clone()
    with torch.no_grad():
        assert hip_autograd.batch_norm_add(xn.clone(memory_format=torch.preserve_format).requires_grad_(True), rn, gamma, beta, rm2, rv2,
                                           training, bc.MOMENTUM, bc.EPS).grad_fn is None
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv)
    worst = 0.0
    for sub in SUBSETS:
        leaves = [t.clone(memory_format=torch.preserve_format).requires_grad_(s) for t, s in zip((xn, rn, gamma, beta), sub)]
        rm3, rv3 = rmean.clone(), rvar.clone()
        out = hip_autograd.batch_norm_add(*leaves, rm3, rv3, training, bc.MOMENTUM, bc.EPS)
        assert torch.equal(out.detach().permute(0, 2, 3, 1), plain) and torch.equal(rm3, rm) and torch.equal(rv3, rv)
        got = torch.autograd.grad(out, [t for t, s in zip(leaves, sub) if s], dyn)
        assert needs[-1] == (sub[0], sub[2], sub[3], sub[1]), sub
        for g, r in zip(got, [r for r, s in zip(ref, sub) if s]):
            worst = max(worst, rel_err(g.permute(0, 2, 3, 1) if g.dim() == 4 else g, r))
    assert len(needs) == len(SUBSETS)
    print('autograd.batch_norm_add train %d: worst of %d subsets %.3g' % (training, len(SUBSETS), worst))
    assert worst < BAR


def test_channels_last_inputs_are_not_copied(monkeypatch):
    ops = bk.operands(AUTOGRAD_CASE, 2)
    x, gamma, beta, res = ops[0].to(DEV), ops[1].to(DEV), ops[2].to(DEV), ops[6].to(DEV)
    seen = []
    real = hip.batch_norm_add_forward
    monkeypatch.setattr(hip, 'batch_norm_add_forward',
                        lambda xh, rh, *a, **kw: (seen.append((xh.data_ptr(), rh.data_ptr())), real(xh, rh, *a, **kw))[1])
    hip_autograd.batch_norm_add(bc.nchw(x).requires_grad_(True), bc.nchw(res), gamma, beta, None, None, True)
    hip_autograd.batch_norm_add(bc.nchw(x), bc.nchw(res), gamma, beta, None, None, True)
    assert seen == [(x.data_ptr(), res.data_ptr())] * 2
    slot = NormSlot(AUTOGRAD_CASE[3]).to(DEV).train()
    y = slot(bc.nchw(x), relu=True, residual=bc.nchw(res))
    assert seen[2] == seen[0] and int(slot.num_batches_tracked) == 1 and float(y.min()) == 0.0


# ---- the holders: device against the restatement under the acceptance rule ---------------------------------------------------------
def on_device(module, prefix, seed, training, stem=None):
    """the holder with backbone_cases' parameters on the device in the given mode, every parameter requiring grad - but the
    stem (`stem`: the ResNetPlus2Slots inside), which stays frozen in eval mode -> (module, its float32 CPU state)"""
    state = bk.module_state(module, prefix, seed=seed)
    module.load_state_dict(state, strict=True)
    module = module.to(DEV).train(training)
    frozen = set()
    if stem is not None:
        stem.bn1.eval()
        frozen = {id(p) for p in list(stem.conv1.parameters()) + list(stem.bn1.parameters())}
    for p in module.parameters():
        p.requires_grad_(id(p) not in frozen)
    return module, state


def run_device(module, inputs, call, grad_inputs=True):
    leaves = {k: v.to(DEV).requires_grad_(grad_inputs) for k, v in inputs.items()}
    names, outs = [], []

    def record(name):
        def hook(_module, _args, y):
            names.append(name)
            outs.append(y.detach().cpu())
        return hook
    handles = [mod.register_forward_hook(record(n)) for n, mod in module.named_modules() if isinstance(mod, NormSlot)]
    named = [(n, t) for n, t in list(leaves.items()) + list(module.named_parameters()) if t.requires_grad]
    everything = list(leaves.items()) + list(module.named_parameters())
    snaps = [guarded.snapshot(t) for _, t in everything]
    named_out, loss_out = call(module, leaves)
    grads = torch.autograd.grad(hc.fixed_loss(loss_out), [t for _, t in named], allow_unused=True)
    for h in handles:
        h.remove()
    for (n, t), s in zip(everything, snaps):
        guarded.unchanged(t, s, n)
    return dict(out=dict(named_out), grad={n: g for (n, _), g in zip(named, grads) if g is not None}, names=names, outs=outs,
                buf={k: v for k, v in module.state_dict().items() if not hc.is_param(k)})


def run_reference(state, inputs, call, training, outs, dtype, grad_inputs=True, frozen=()):
    params = hc.leaves_of(state, dtype)
    for k in frozen:
        params[k].requires_grad_(False)
    leaves = {k: v.to(dtype).clone().requires_grad_(grad_inputs) for k, v in inputs.items()}
    ref = bk.BackboneRef(params, training, outs)
    named_out, loss_out = call(ref, leaves)
    named = [(n, t) for n, t in list(leaves.items()) + [(k, v) for k, v in params.items() if hc.is_param(k)] if t.requires_grad]
    grads = torch.autograd.grad(hc.fixed_loss(loss_out), [t for _, t in named], allow_unused=True)
    return dict(out={n: t.detach() for n, t in named_out}, grad={n: g for (n, _), g in zip(named, grads) if g is not None}, ref=ref,
                buf={k: v for k, v in params.items() if not hc.is_param(k)})


def errors(got, ref):
    assert sorted(got['out']) == sorted(ref['out']) and sorted(got['grad']) == sorted(ref['grad']), \
        (sorted(set(got['grad']) ^ set(ref['grad'])), sorted(set(got['out']) ^ set(ref['out'])))
    e = {'out/' + n: rel_err(got['out'][n], ref['out'][n]) for n in ref['out']}
    for n, r in ref['grad'].items():
        e['grad/' + n] = rel_err(got['grad'][n], r)
    for n, r in ref['buf'].items():
        if not n.endswith('num_batches_tracked'):
            e['buf/' + n] = rel_err(got['buf'][n], r)
    return e


def check_module(tag, module, state, inputs, call, training, grad_inputs=True, frozen=(), calls=1, verbose=True):
    """device against float64 under the acceptance rule, both errors printed per tensor; the mask condition; the statistics"""
    dev = run_device(module, inputs, call, grad_inputs)
    r64 = run_reference(state, inputs, call, training, dev['outs'], torch.float64, grad_inputs, frozen)
    r32 = run_reference(state, inputs, call, training, dev['outs'], torch.float32, grad_inputs, frozen)
    ref = r64['ref']
    assert dev['names'] == ref.names                     # the hooks saw the BatchNorms in the restatement's order
    for k, (y, pre) in enumerate(zip(dev['outs'], ref.pres)):
        if ref.relus[k]:                                 # a seed inside the band is replaced, not excused
            assert bc.mask_violations(y.permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)) == 0, (k, ref.names[k])
    e_hip, e_f32 = errors(dev, r64), errors(r32, r64)
    if verbose:
        for n in sorted(e_hip):
            print('%s %-44s hip %.3g  torch-cpu float32 %.3g' % (tag, n, e_hip[n], e_f32[n]))
    worst = max(e_hip, key=lambda n: e_hip[n] / max(BAR, 1.5 * e_f32[n]))
    print('%s worst: %s hip %.3g float32 %.3g (%d tensors)' % (tag, worst, e_hip[worst], e_f32[worst], len(e_hip)))
    for n, e in e_hip.items():
        bound = max(BAR, 1.5 * e_f32[n])
        assert e <= bound, (tag, n, e, bound)
    for n, r in r64['buf'].items():                      # moved by a training-mode call, once per call; eval and the stem: untouched
        ran = ref.names.count(n.rsplit('.', 1)[0]) if training else 0
        if n.endswith('num_batches_tracked'):
            assert int(dev['buf'][n]) == int(r) == ran, n
        else:
            assert torch.equal(dev['buf'][n].cpu(), state[n]) == (ran == 0), n
    return dev


# ---- 6. BottleneckSlots ---------------------------------------------------------------------------------------------------------------
def _bottleneck(kind):
    if kind == 'plain':
        return BottleneckSlots(256, 64), 256, dict()
    if kind == 'layer2_first':
        return (BottleneckSlots(256, 128, stride=2, downsample=_seq(ConvSlot(256, 512, 3, stride=2), NormSlot(512))), 256,
                dict(stride=2, downsample=(3, 2, 0)))
    if kind == 'layer3_first':
        return (BottleneckSlots(512, 256, downsample=_seq(ConvSlot(512, 1024, 3, pad=1), NormSlot(1024)), dilation=2), 512,
                dict(downsample=(3, 1, 1), dilation=2))
    return BottleneckSlots(1024, 256, dilation=2), 1024, dict(dilation=2)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('kind', ['plain', 'layer2_first', 'layer3_first', 'dilated'])
def test_bottleneck_slots(kind, training):
    block, cin, geo = _bottleneck(kind)
    module, state = on_device(block, 'block.', 21, training)
    inputs = dict(x=bk.feature_map(2, cin, 9, seed=5))

    def call(fwd, lv):
        y = fwd(lv['x']) if isinstance(fwd, torch.nn.Module) else fwd.bottleneck('', lv['x'], **geo)
        return [('out', y)], [('out', y)]
    dev = check_module('bottleneck %s %s' % (kind, 'train' if training else 'eval'), module, state, inputs, call, training)
    assert tuple(dev['out']['out'].shape) == (2, block.conv3.cout, 4 if kind == 'layer2_first' else 9, 4 if kind == 'layer2_first' else 9)
    assert dev['names'] == ['bn1', 'bn2'] + (['downsample.1'] if block.downsample is not None else []) + ['bn3']
    assert len(dev['grad']) == 1 + len(list(module.parameters()))


# ---- 7. ResNetPlus2Slots -----------------------------------------------------------------------------------------------------------
STEM_KEYS = ('conv1.weight', 'bn1.weight', 'bn1.bias')


def backbone_call(layers):
    def call(fwd, lv):
        res = fwd(lv['image']) if isinstance(fwd, torch.nn.Module) else fwd.resnet(lv['image'], layers)
        named = bk.named_backbone(res)
        return named, named[1:]
    return call


@pytest.mark.parametrize('layers,size', [((1, 1, 1), 63), ((3, 4, 6), 127)], ids=['depth1_63', 'full_127'])
def test_resnet_plus2_slots(layers, size):
    net = ResNetPlus2Slots(layers)
    module, state = on_device(net, 'features.features.', 23, True, stem=net)
    dev = check_module('resnet %s' % (layers,), module, state, dict(image=bk.image(2, size, seed=1)), backbone_call(layers), True,
                       grad_inputs=False, frozen=STEM_KEYS, verbose=layers == (1, 1, 1))
    hf = ((size - 7) // 2 + 1 - 1) // 2 + 1
    hs = (hf - 3) // 2 + 1
    assert [tuple(dev['out'][n].shape) for n in ('x_', 'p1', 'p2', 'p3')] == \
        [(2, 64, (size - 7) // 2 + 1, (size - 7) // 2 + 1), (2, 256, hf, hf), (2, 512, hs, hs), (2, 1024, hs, hs)]
    assert len(dev['grad']) == len(list(module.parameters())) - 3 and not any(k in dev['grad'] for k in STEM_KEYS)
    assert int(module.bn1.num_batches_tracked) == 0


def test_stem_guard():
    img = bk.image(1, 63).to(DEV)
    net = ResNetPlus2Slots((1, 1, 1)).to(DEV)
    with pytest.raises(NotImplementedError, match="stem's gradients"):
        net.train()(img)
    net.eval().conv1.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="stem's gradients"):
        net(img)
    net.conv1.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="stem's gradients"):
        net(img.clone().requires_grad_(True))
    (x_, p1, p2), p3 = net(img)                          # the recipe's configuration runs
    assert p3.shape == (1, 1024, 7, 7) and x_.shape == (1, 64, 29, 29)
    # the fold follows the parameters
    with torch.no_grad():
        net.bn1.bias.add_(1.0)
    assert not torch.equal(net(img)[0][0], x_)


# ---- 8. NeckSlots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', bk.NECK_FORMS)
def test_neck_slots(form):
    module, state = on_device(NeckSlots(1024, 256, pr_pool=True), 'neck.', 27, True)
    box = bk.boxes(2, 15, seed=2)

    def call(fwd, lv):
        if isinstance(fwd, torch.nn.Module):
            res = fwd(lv['x'], **bk.neck_args(form, box.to(DEV)))
        else:
            res = fwd.neck(lv['x'], **bk.neck_args(form, box.to(lv['x'].dtype)))
        named = bk.named_neck(res)
        return named, named
    dev = check_module('neck %s' % form, module, state, dict(x=bk.feature_map(2, 1024, 15, seed=4)), call, True)
    assert tuple(dev['out']['x_ori'].shape) == (2, 256, 15, 15)
    assert ('xf' in dev['out']) == (form != 'plain') and (form == 'plain' or tuple(dev['out']['xf'].shape) == (2, 256, 7, 7))
    assert sorted(dev['grad']) == ['downsample.0.weight', 'downsample.1.bias', 'downsample.1.weight', 'x']
    with pytest.raises(AttributeError):
        NeckSlots(1024, 256).to(DEV)(bk.feature_map(2, 1024, 15).to(DEV), crop=True, pr_pool=True, bbox=box.to(DEV))


# ---- 9. chain: backbone -> neck -> head -------------------------------------------------------------------------------------------
class Chain(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.features = BackboneSlots()
        self.features.features = ResNetPlus2Slots((1, 1, 1))
        self.neck = NeckSlots(1024, 256)
        self.connect_model = HeadSlots(256, tower_num=1)

    def forward(self, z, x):
        _, zf = self.features(z)
        _, xf = self.features(x)
        _, zk = self.neck(zf, crop=True)
        res = self.connect_model(self.neck(xf), zk)
        return res[0], res[1]


def test_chain_backbone_neck_head():
    chain = Chain()
    bstate = bk.module_state(chain.features, 'features.', seed=31)
    nstate = bk.module_state(chain.neck, 'neck.', seed=31)
    hstate = hc.module_state(chain.connect_model, 'connect_model.', seed=31)
    chain.features.load_state_dict(bstate), chain.neck.load_state_dict(nstate), chain.connect_model.load_state_dict(hstate)
    chain = chain.to(DEV).train()
    stem = chain.features.features
    stem.bn1.eval()
    frozen = {id(p) for p in list(stem.conv1.parameters()) + list(stem.bn1.parameters())}
    for p in chain.parameters():
        p.requires_grad_(id(p) not in frozen)
    z, x = bk.image(2, 127, seed=7), bk.image(2, 159, seed=8)
    names, outs = [], []
    handles = [m.register_forward_hook(lambda _m, _a, y, n=n: (names.append(n), outs.append(y.detach().cpu()))[0] and None)
               for n, m in chain.named_modules() if isinstance(m, NormSlot)]
    x_bbox, cls = chain(z.to(DEV), x.to(DEV))
    for h in handles:
        h.remove()
    named = [(n, p) for n, p in chain.named_parameters() if p.requires_grad]
    loss = hc.fixed_loss([('x_bbox', x_bbox), ('cls', cls)])
    grads = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    got = {n: g for (n, _), g in zip(named, grads) if g is not None}       # the offline form does not reach the memory branch
    assert x_bbox.shape == (2, 4, 13, 13) and cls.shape == (2, 1, 13, 13)
    nb = 2 * 12 + 2                                      # BatchNorm calls of the two backbone passes and the two neck calls

    def reference(dtype):
        bp = {'features.' + k: v for k, v in hc.leaves_of(bstate, dtype).items()}
        bp.update({'neck.' + k: v for k, v in hc.leaves_of(nstate, dtype).items()})
        for k in STEM_KEYS:
            bp['features.features.' + k].requires_grad_(False)
        hp = hc.leaves_of(hstate, dtype)
        bref = bk.BackboneRef(bp, True, outs[:nb])
        href = hc.HeadRef(hp, True, outs[nb:], tower_num=1)
        _, zf = bref.resnet(z.to(dtype), (1, 1, 1), prefix='features.features.')
        _, xf = bref.resnet(x.to(dtype), (1, 1, 1), prefix='features.features.')
        z_ori, zk = bref.neck(zf, crop=True, prefix='neck.')
        x_ori = bref.neck(xf, prefix='neck.')
        res = href.head(x_ori, zk)
        leaves = [(k, v) for k, v in bp.items() if hc.is_param(k) and v.requires_grad] \
            + [('connect_model.' + k, v) for k, v in hp.items() if hc.is_param(k)]
        l_ = hc.fixed_loss([('x_bbox', res[0]), ('cls', res[1])])
        grads = torch.autograd.grad(l_, [v for _, v in leaves] + href.convs + [z_ori, x_ori], allow_unused=True)
        grad = {n: g for (n, _), g in zip(leaves, grads) if g is not None}
        conv_g = grads[len(leaves):-2]
        terms = {'connect_model.' + key: float(sum(conv_g[k].abs().sum((0, 2, 3)) for k in idx).mean())
                 for key, idx in hc.cancelling_biases(href.names, True).items() if 'connect_model.' + key in grad}
        # the neck's BatchNorm bias is a constant per channel on both maps, and every path from them starts with a conv into a
        # training-mode BatchNorm, which subtracts it again: its gradient is a sum that is zero in exact arithmetic, judged like
        # the head's conv biases against the magnitude of its terms
        terms['neck.downsample.1.bias'] = float(sum(g.abs().sum((0, 2, 3)) for g in grads[-2:]).mean())
        return dict(grad=grad, terms=terms, bref=bref, href=href, out=dict(x_bbox=res[0].detach(), cls=res[1].detach()))
    r64, r32 = reference(torch.float64), reference(torch.float32)
    assert names == r64['bref'].names + ['connect_model.' + n for n in r64['href'].names]
    for k, (y, pre) in enumerate(zip(outs, r64['bref'].pres + r64['href'].pres)):
        if k >= nb or r64['bref'].relus[k]:
            assert bc.mask_violations(y.permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)) == 0, (k, names[k])
    assert sorted(got) == sorted(r64['grad'])

    def err(g, n):
        r = r64['grad'][n]
        if n in r64['terms']:
            return float((g.detach().cpu().double() - r.double()).abs().max() / r64['terms'][n])
        return rel_err(g, r)
    e_hip = {n: err(got[n], n) for n in r64['grad']}
    e_f32 = {n: err(r32['grad'][n], n) for n in r64['grad']}
    for o, t in (('x_bbox', x_bbox), ('cls', cls)):
        e_hip['out/' + o], e_f32['out/' + o] = rel_err(t, r64['out'][o]), rel_err(r32['out'][o], r64['out'][o])
    worst = max(e_hip, key=lambda n: e_hip[n] / max(BAR, 1.5 * e_f32[n]))
    print('chain worst: %s hip %.3g float32 %.3g (%d tensors)' % (worst, e_hip[worst], e_f32[worst], len(e_hip)))
    for n, e in e_hip.items():
        assert e <= max(BAR, 1.5 * e_f32[n]), (n, e, e_f32[n])
    assert any(n.startswith('features.features.layer1') for n in e_hip) and 'neck.downsample.0.weight' in e_hip


# ---- 10. against the product path ---------------------------------------------------------------------------------------------------
def test_eval_forward_agrees_with_the_engine():
    from usot_amd.model import USOT
    m = USOT()
    m.load_state_dict(synth.torch_state_dict(m, seed=0, calibrated=True), strict=True)
    m = m.to(DEV).eval()
    x = torch.from_numpy(synth.crop(3, 1, 127)).to(DEV)
    want = m.engine.features(x).clone()
    with torch.no_grad():
        got = m.neck(m.features(x)[1])
    e = rel_err(got, want)
    print('neck(backbone(x)) against engine.features(x): %.3g' % e)
    assert got.shape == want.shape == (1, 256, 15, 15) and e < 1e-4


# ---- 11. the recipe --------------------------------------------------------------------------------------------------------------------
def test_the_training_recipe_moves_exactly_layer1_3_and_the_neck():
    """the reference's build_opt_lr at an epoch past UNFIX_EPOCH with TRAINABLE_LAYER = layer1-3, restated: freeze the backbone and
    put its BatchNorms in eval mode, then unfreeze the three layers and put theirs in training mode; the neck trains throughout"""
    feats, neck = BackboneSlots(), NeckSlots(1024, 256, pr_pool=True)
    feats.features = ResNetPlus2Slots((1, 1, 1))
    feats.load_state_dict(bk.module_state(feats, 'features.', seed=41))
    neck.load_state_dict(bk.module_state(neck, 'neck.', seed=41))
    feats, neck = feats.to(DEV).train(), neck.to(DEV).train()
    net = feats.features
    for p in net.parameters():
        p.requires_grad = False
    for mod in net.modules():
        if isinstance(mod, NormSlot):
            mod.eval()
    for layer in ('layer1', 'layer2', 'layer3'):
        for p in getattr(net, layer).parameters():
            p.requires_grad = True
        for mod in getattr(net, layer).modules():
            if isinstance(mod, NormSlot):
                mod.train()
    for p in neck.parameters():
        p.requires_grad = True
    before = {k: v.detach().clone() for k, v in list(feats.state_dict(prefix='features.').items()) + list(neck.state_dict(prefix='neck.').items())}
    opt = torch.optim.SGD([p for p in list(net.parameters()) + list(neck.parameters()) if p.requires_grad], lr=0.01)
    _, p3 = feats(bk.image(2, 127, seed=9).to(DEV))
    x_ori, zf = neck(p3, crop=True, pr_pool=True, bbox=bk.boxes(2, 15, seed=3).to(DEV))
    hc.fixed_loss([('x_ori', x_ori), ('zf', zf)]).backward()
    opt.step()
    after = dict(list(feats.state_dict(prefix='features.').items()) + list(neck.state_dict(prefix='neck.').items()))
    for k, v in after.items():
        stem = k.startswith(('features.features.conv1.', 'features.features.bn1.'))
        if k.endswith('num_batches_tracked'):
            assert int(v) == (0 if stem else 1), k
        else:
            assert torch.equal(v, before[k]) == stem, k
    assert sum(1 for k in after if k.startswith('features.features.layer')) > 0 and 'neck.downsample.0.weight' in after
