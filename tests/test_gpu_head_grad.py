"""GPU: Conf_Fusion and the box epilogue, forward and gradients (csrc/head_grad.hip), and the surfaces over them -
usot_amd.hip.conf_fusion_* / box_exp_*, usot_amd.autograd.conf_fusion / box_exp, and the forward passes of net.EncoderSlots,
net.ConfFusionSlots and net.HeadSlots (the reference's matrix, Conf_Fusion and box_tower_reg) - against the float64 restatement
of tests/head_grad_cases.py, which tests/test_head_grad_host.py holds to the reference itself.

Metric: the project's scaled error max |got - ref| / max(|ref|, mean|ref|).  The raw kernels and the autograd functions are held
to 1e-5.  The module tests differentiate up to eleven conv - BN - ReLU stages, three correlations, the fusion and an exp in a row
and use the project's acceptance rule: per tensor, the HIP error may be at most max(1e-5, 1.5 x the error
of the same restatement in PyTorch-CPU float32 with the same masks).  Masks: the float64 and float32 restatements take every
ReLU mask, and Conf_Fusion's clamp mask, from the device's own maps (forward hooks on the NormSlots, in call order); separately
no element outside rounding distance of a threshold may sit on the wrong side (bc.mask_violations, clamp_violations).

Worst pair measured on an MI355X (test_head_slots, printed per tensor by every module test): HIP 1.19e-5 beside PyTorch-CPU
float32 1.20e-5, the gradient of bbox_tower.0.weight in eval mode (DESIGN.md section 3.3.4 lists the other cases)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import batchnorm_cases as bc  # noqa: E402
import guarded  # noqa: E402
import head_grad_cases as hc  # noqa: E402
from head_grad_cases import rel_err  # noqa: E402
from usot_amd import autograd as hip_autograd, hip  # noqa: E402
from usot_amd.net import ConfFusionSlots, EncoderSlots, HeadSlots, NormSlot  # noqa: E402

DEV = 'cuda:0'
BAR = 1e-5


@pytest.fixture(autouse=True)
def _memory_guard():
    """Every output a wrapper of usot_amd.hip / usot_amd.autograd allocates starts as NaN and sits between canaries
    (tests/guarded.py); the guards are checked when the test ends."""
    with guarded.patched(hip, hip_autograd):
        yield


# ---- 1. raw Conf_Fusion ------------------------------------------------------------------------------------------------------
def raw_conf_fusion(c, need=(True, True)):
    """usot_conf_fusion_fwd_f32 and _bwd_f32 on NaN-filled outputs between canaries -> dict of device tensors (None where a
    gradient was not asked for); the inputs, and `out` across the backward call, must stay bit-identical"""
    b, m, p, ch = c
    conf, value, dout = hc.cf_operands(c)
    L = hip.lib()
    o = dict(conf=guarded.put(conf, DEV), value=guarded.put(value, DEV), dout=guarded.put(dout, DEV),
             out=guarded.alloc((b, p, ch), torch.float32, DEV))
    snaps = {f: guarded.snapshot(o[f]) for f in ('conf', 'value', 'dout')}
    d = hip.conf_fusion_desc(B=b, M=m, P=p, C=ch, conf=o['conf'].data_ptr(), value=o['value'].data_ptr(), out=o['out'].data_ptr())
    hip.check(L.usot_conf_fusion_fwd_f32(hip.stream(), C.byref(d)), 'usot_conf_fusion_fwd_f32')
    snaps['out'] = guarded.snapshot(o['out'])
    o['dconf'] = guarded.alloc((b * m, p, ch), torch.float32, DEV) if need[0] else None
    o['dvalue'] = guarded.alloc((b * m, p, ch), torch.float32, DEV) if need[1] else None
    d = hip.conf_fusion_desc(B=b, M=m, P=p, C=ch, conf=o['conf'].data_ptr(), value=o['value'].data_ptr(), dout=o['dout'].data_ptr())
    d.dconf, d.dvalue = hip.ptr(o['dconf']), hip.ptr(o['dvalue'])
    hip.check(L.usot_conf_fusion_bwd_f32(hip.stream(), C.byref(d)), 'usot_conf_fusion_bwd_f32')
    for f, s in snaps.items():
        guarded.unchanged(o[f], s, f)
    return o


@pytest.mark.parametrize('need', [(True, True), (True, False), (False, True)], ids=['both', 'dconf', 'dvalue'])
@pytest.mark.parametrize('c', hc.CF_CASES, ids=hc.cf_id)
def test_raw_conf_fusion(c, need):
    """CF_CASES[1]: the lane count ends inside a workgroup; CF_CASES[2] and [3]: several workgroups and a tail.  The grid is
    one lane per thread, uncapped: there is no second trip to test.  Each nullable output is run as NULL."""
    b, m, _, _ = c
    o = raw_conf_fusion(c, need)
    conf, value, dout = (t.double() for t in hc.cf_operands(c))
    out, dconf, dvalue = hc.conf_fusion_formulas(conf, value, dout, b, m)
    errs = {'out': rel_err(o['out'], out)}
    if need[0]:
        errs['dconf'] = rel_err(o['dconf'], dconf)
        got, cf = o['dconf'].cpu().reshape(-1), conf.reshape(-1)
        planted = {0: 4.0, 1: 5.5, 2: 0.0} if cf.numel() < 8 else {0: 4.0, 5: 5.5, 10: 0.0, 15: -6.0, 20: -7.5, 25: 4.0}
        for i, v in planted.items():
            assert float(cf[i]) == v
            if m > 1:                                    # M = 1: the weight is 1 and every dconf is an exact zero
                assert (float(got[i]) != 0.0) == (-6.0 <= v <= 4.0), (i, v, float(got[i]))
        if m == 1:
            assert not bool(got.any())
    if need[1]:
        errs['dvalue'] = rel_err(o['dvalue'], dvalue)
    print('%s need %s: ' % (hc.cf_id(c), need) + ' '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) < BAR, errs


def test_conf_fusion_bindings_match_raw_entry_points():
    c = hc.CF_CASES[2]
    b, m, _, _ = c
    raw = raw_conf_fusion(c)
    conf, value, dout = (t.to(DEV) for t in hc.cf_operands(c))
    assert torch.equal(hip.conf_fusion_forward(conf, value, b, m), raw['out'])
    dc, dv = hip.conf_fusion_backward(dout, conf, value, b, m)
    assert torch.equal(dc, raw['dconf']) and torch.equal(dv, raw['dvalue'])
    only = hip.conf_fusion_backward(dout, conf, value, b, m, need=(False, True))
    assert only[0] is None and torch.equal(only[1], raw['dvalue'])
    for bad in (lambda: hip.conf_fusion_forward(conf, value, b + 1, m), lambda: hip.conf_fusion_forward(conf, value[:-1], b, m),
                lambda: hip.conf_fusion_forward(conf[..., :32], value[..., :32], b, m),                # not dense
                lambda: hip.conf_fusion_backward(dout[:, :-1], conf, value, b, m),
                lambda: hip.conf_fusion_forward(conf.cpu(), value, b, m), lambda: hip.conf_fusion_forward(conf.double(), value, b, m)):
        with pytest.raises(hip.HipError):
            bad()


# ---- 2. raw box-exp ------------------------------------------------------------------------------------------------------------
def raw_box_exp(rows, need=(True, True, True)):
    """usot_box_exp_fwd_f32 and _bwd_f32 on NaN-filled outputs and a NaN-filled workspace of exactly usot_box_exp_ws_floats
    floats -> dict of device tensors; p, adjust, bias, dy (and y across the backward call) must stay bit-identical"""
    p, adjust, bias, dy = hc.box_operands(rows)
    L = hip.lib()
    o = dict(p=guarded.put(p, DEV), adjust=guarded.put(adjust, DEV), bias=guarded.put(bias, DEV), dy=guarded.put(dy, DEV),
             y=guarded.alloc((rows, 4), torch.float32, DEV))
    snaps = {f: guarded.snapshot(o[f]) for f in ('p', 'adjust', 'bias', 'dy')}
    ptrs = dict(p=o['p'].data_ptr(), adjust=o['adjust'].data_ptr(), bias=o['bias'].data_ptr())
    d = hip.box_exp_desc(R=rows, y=o['y'].data_ptr(), **ptrs)
    hip.check(L.usot_box_exp_fwd_f32(hip.stream(), C.byref(d)), 'usot_box_exp_fwd_f32')
    snaps['y'] = guarded.snapshot(o['y'])
    o['dp'] = guarded.alloc((rows, 4), torch.float32, DEV) if need[0] else None
    o['dadjust'] = guarded.alloc((1,), torch.float32, DEV) if need[1] else None
    o['dbias'] = guarded.alloc((4,), torch.float32, DEV) if need[2] else None
    o['ws'] = guarded.alloc((hip.box_exp_ws_floats(rows),), torch.float32, DEV) if need[1] or need[2] else None
    d = hip.box_exp_desc(R=rows, dy=o['dy'].data_ptr(), **ptrs)
    d.dp, d.dadjust, d.dbias, d.ws = (hip.ptr(o[f]) for f in ('dp', 'dadjust', 'dbias', 'ws'))
    hip.check(L.usot_box_exp_bwd_f32(hip.stream(), C.byref(d)), 'usot_box_exp_bwd_f32')
    for f, s in snaps.items():
        guarded.unchanged(o[f], s, f)
    return o


BOX_ROWS = {'1': lambda s: 1, 'step-1': lambda s: s - 1, 'step': lambda s: s, 'step+1': lambda s: s + 1, '5step+3': lambda s: 5 * s + 3}


@pytest.mark.parametrize('rname', list(BOX_ROWS))
def test_raw_box_exp(rname):
    """row counts around the reduction's row step (one workgroup's rows, one partial) and a six-partial one.  dbias and dadjust
    are sums of terms of both signs: judged against the sum of the magnitudes of their terms.  The backward pass runs twice
    and must give the same bits; adjust and bias stay as they were (raw_box_exp)."""
    step = hip.box_exp_row_step()
    rows = BOX_ROWS[rname](step)
    o = raw_box_exp(rows)
    again = raw_box_exp(rows)
    for f in ('y', 'dp', 'dadjust', 'dbias', 'ws'):
        assert torch.equal(o[f], again[f]), f
    assert o['ws'].numel() == 5 * -(-rows // step) and bool(torch.isfinite(o['ws']).all())
    p, adjust, bias, dy = (t.double() for t in hc.box_operands(rows))
    y, dp, dadjust, dbias, ta, tb = hc.box_exp_formulas(p, adjust, bias, dy)
    errs = {'y': rel_err(o['y'], y), 'dp': rel_err(o['dp'], dp),
            'dadjust': float((o['dadjust'].cpu().double() - dadjust).abs().max() / ta),
            'dbias': float(((o['dbias'].cpu().double() - dbias).abs() / tb).max())}
    print('R %d (step %d): ' % (rows, step) + ' '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize('need', [(True, False, False), (False, True, False), (False, False, True), (True, False, True)],
                         ids=['dp', 'dadjust', 'dbias', 'dp_dbias'])
def test_raw_box_exp_nullable_outputs(need):
    """each output as NULL; dp alone is the one launch without a reduction and runs without a workspace"""
    rows = 2 * hip.box_exp_row_step() + 5
    full, part = raw_box_exp(rows), raw_box_exp(rows, need)
    for f, n in zip(('dp', 'dadjust', 'dbias'), need):
        assert (part[f] is not None) == n and (not n or torch.equal(part[f], full[f])), f
    assert (part['ws'] is None) == (not (need[1] or need[2]))


def test_box_exp_bindings_match_raw_entry_points():
    rows = 3 * hip.box_exp_row_step() - 7
    raw = raw_box_exp(rows)
    p, adjust, bias, dy = (t.to(DEV) for t in hc.box_operands(rows))
    assert torch.equal(hip.box_exp_forward(p, adjust, bias), raw['y'])
    dp, da, db = hip.box_exp_backward(dy, p, adjust, bias)
    assert torch.equal(dp, raw['dp']) and torch.equal(da, raw['dadjust']) and torch.equal(db.reshape(4), raw['dbias'])
    assert da.shape == adjust.shape and db.shape == bias.shape
    only = hip.box_exp_backward(dy, p, adjust, bias, need=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], raw['dadjust'])
    for bad in (lambda: hip.box_exp_forward(p[:, :3], adjust, bias), lambda: hip.box_exp_forward(p, torch.zeros(2, device=DEV), bias),
                lambda: hip.box_exp_forward(p, adjust, bias.reshape(4)[:3]), lambda: hip.box_exp_backward(dy[:-1], p, adjust, bias),
                lambda: hip.box_exp_forward(p, adjust.cpu(), bias), lambda: hip.box_exp_forward(p.cpu(), adjust, bias)):
        with pytest.raises(hip.HipError):
            bad()


# ---- 3. the autograd functions -----------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """records the `need` of every backward call and the data pointers of the maps every forward call receives (usot_amd.autograd
    looks the bindings up on the module at call time)"""
    rec = {'need': [], 'ptrs': []}
    for fwd, bwd in (('conf_fusion_forward', 'conf_fusion_backward'), ('box_exp_forward', 'box_exp_backward')):
        rf, rb = getattr(hip, fwd), getattr(hip, bwd)
        monkeypatch.setattr(hip, fwd, lambda *a, _r=rf, **kw: (rec['ptrs'].append(a[0].data_ptr()), _r(*a, **kw))[1])
        monkeypatch.setattr(hip, bwd, lambda *a, _r=rb, **kw: (rec['need'].append(tuple(bool(v) for v in kw['need'])), _r(*a, **kw))[1])
    return rec


def test_autograd_conf_fusion(calls):
    b, m, p, ch = c = hc.CF_CASES[3]
    conf, value, dout = (t.to(DEV).reshape(t.shape[0], 5, 5, ch) for t in hc.cf_operands(c))
    cn, vn, dn = bc.nchw(conf), bc.nchw(value), bc.nchw(dout)           # NCHW-shaped views of channels-last memory
    plain = hip.conf_fusion_forward(conf, value, b, m)
    off = hip_autograd.conf_fusion(cn, vn, b, m)
    assert off.grad_fn is None and off.shape == (b, ch, 5, 5) and torch.equal(off.permute(0, 2, 3, 1), plain)
    assert off.permute(0, 2, 3, 1).is_contiguous()
    cg, vg = cn.detach().requires_grad_(True), vn.detach().requires_grad_(True)
    with torch.no_grad():
        assert hip_autograd.conf_fusion(cg, vg, b, m).grad_fn is None
    out = hip_autograd.conf_fusion(cg, vg, b, m)
    assert out.grad_fn is not None and torch.equal(out.detach(), off)    # the recorded path computes the same bits
    assert calls['ptrs'] == [conf.data_ptr()] * 4                        # the channels-last inputs went in as they are
    gc, gv = torch.autograd.grad(out, (cg, vg), dn)
    assert calls['need'] == [(True, True)]
    c64, v64, d64 = (t.double() for t in hc.cf_operands(c))
    _, rc, rv = hc.conf_fusion_formulas(c64, v64, d64, b, m)
    errs = [rel_err(gc.permute(0, 2, 3, 1).reshape(rc.shape), rc), rel_err(gv.permute(0, 2, 3, 1).reshape(rv.shape), rv)]
    print('autograd conf_fusion: dconf %.3g dvalue %.3g' % tuple(errs))
    assert max(errs) < BAR
    # only what is asked for
    g1, = torch.autograd.grad(hip_autograd.conf_fusion(cg, vn, b, m), (cg,), dn)
    g2, = torch.autograd.grad(hip_autograd.conf_fusion(cn, vg, b, m), (vg,), dn)
    assert calls['need'][1:] == [(True, False), (False, True)] and torch.equal(g1, gc) and torch.equal(g2, gv)
    # a dense NCHW input is the same function (it goes through the permute kernel), and so is an expanded gradient
    out2 = hip_autograd.conf_fusion(cg.contiguous(), vg.contiguous(), b, m)
    assert torch.equal(out2.detach(), off)
    g3, = torch.autograd.grad(out2.sum(), (cg,))
    assert rel_err(g3.permute(0, 2, 3, 1).reshape(rc.shape), hc.conf_fusion_formulas(c64, v64, torch.ones_like(d64), b, m)[1]) < BAR


def test_autograd_box_exp(calls):
    rows = 2 * 9 * 9
    p, adjust, bias, dy = (t.to(DEV) for t in hc.box_operands(rows))
    ph, dh = p.reshape(2, 9, 9, 4), dy.reshape(2, 9, 9, 4)
    pn, dn = bc.nchw(ph), bc.nchw(dh)
    plain = hip.box_exp_forward(ph, adjust, bias)
    off = hip_autograd.box_exp(pn, adjust, bias)
    assert off.grad_fn is None and off.shape == (2, 4, 9, 9) and torch.equal(off.permute(0, 2, 3, 1), plain)
    leaves = [t.detach().clone().requires_grad_(True) for t in (adjust, bias)]
    pg = pn.detach().requires_grad_(True)
    with torch.no_grad():
        assert hip_autograd.box_exp(pg, *leaves).grad_fn is None
    out = hip_autograd.box_exp(pg, *leaves)
    assert out.grad_fn is not None and torch.equal(out.detach(), off)
    assert calls['ptrs'] == [ph.data_ptr()] * 4
    gp, ga, gb = torch.autograd.grad(out, [pg] + leaves, dn)
    assert calls['need'] == [(True, True, True)] and ga.shape == adjust.shape and gb.shape == bias.shape
    p64, a64, b64, d64 = (t.double() for t in hc.box_operands(rows))
    _, rp, ra, rb, ta, tb = hc.box_exp_formulas(p64, a64, b64, d64)
    errs = [rel_err(gp.permute(0, 2, 3, 1).reshape(rows, 4), rp), float((ga.cpu().double() - ra).abs().max() / ta),
            float(((gb.cpu().double().reshape(4) - rb).abs() / tb).max())]
    print('autograd box_exp: dp %.3g dadjust %.3g dbias %.3g' % tuple(errs))
    assert max(errs) < BAR
    for k, need in enumerate(((True, False, False), (False, True, False), (False, False, True))):
        args = [pg if k == 0 else pn, leaves[0] if k == 1 else adjust, leaves[1] if k == 2 else bias]
        g, = torch.autograd.grad(hip_autograd.box_exp(*args), (args[k],), dn)
        assert calls['need'][-1] == need and torch.equal(g, (gp, ga, gb)[k])


# ---- 4. the modules ------------------------------------------------------------------------------------------------------------
CONF = torch.ones(hc.BATCH, hc.MEM)                     # a CPU tensor, as models.py:256 passes one: only its shape is read


def on_device(module, prefix, seed, training):
    """the holder with usot_amd.synth's parameters (eval: running statistics away from (0, 1)) on the device, every parameter
    requiring grad -> (module, its float32 CPU state)"""
    state = hc.module_state(module, prefix, seed=seed, stats=not training)
    module.load_state_dict(state, strict=True)
    module = module.to(DEV).train(training)
    for p in module.parameters():
        p.requires_grad_(True)
    return module, state


def run_device(module, inputs, call):
    """forward and the gradients of the fixed loss on the device; the NormSlots' outputs in call order through forward hooks;
    the inputs and the parameters must stay bit-identical"""
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in inputs.items()}
    names, outs = [], []

    def record(name):
        def hook(_module, _args, y):                     # returns None: the output stays what it is
            names.append(name)
            outs.append(y.detach().cpu())
        return hook
    handles = [mod.register_forward_hook(record(n)) for n, mod in module.named_modules() if isinstance(mod, NormSlot)]
    named = list(leaves.items()) + list(module.named_parameters())
    snaps = [guarded.snapshot(t) for _, t in named]
    named_out, loss_out = call(module, leaves)
    grads = torch.autograd.grad(hc.fixed_loss(loss_out), [t for _, t in named], allow_unused=True)
    for h in handles:
        h.remove()
    for (n, t), s in zip(named, snaps):
        guarded.unchanged(t, s, n)
    return dict(out=dict(named_out), grad={n: g for (n, _), g in zip(named, grads) if g is not None}, names=names, outs=outs,
                buf={k: v for k, v in module.state_dict().items() if not hc.is_param(k)})


def run_reference(state, inputs, call, training, tower_num, outs, dtype):
    """the restatement in `dtype` with the device's masks -> the same dict, plus per cancelling conv bias the scale it is judged
    against (mean over channels of sum |d loss / d conv output|) and the HeadRef itself"""
    params = hc.leaves_of(state, dtype)
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    ref = hc.HeadRef(params, training, outs, tower_num)
    named_out, loss_out = call(ref, leaves)
    named = list(leaves.items()) + [(k, v) for k, v in params.items() if hc.is_param(k)]
    grads = torch.autograd.grad(hc.fixed_loss(loss_out), [t for _, t in named] + ref.convs, allow_unused=True)
    grad = {n: g for (n, _), g in zip(named, grads) if g is not None}
    conv_g = grads[len(named):]
    terms = {key: float(sum(conv_g[k].abs().sum((0, 2, 3)) for k in idx).mean())
             for key, idx in hc.cancelling_biases(ref.names, training).items() if key in grad}
    return dict(out={n: t.detach() for n, t in named_out}, grad=grad, terms=terms, ref=ref,
                buf={k: v for k, v in params.items() if not hc.is_param(k)})


def errors(got, ref, terms):
    """scaled error per output, gradient and BatchNorm statistic; a cancelling conv bias against the magnitude of its terms"""
    assert sorted(got['out']) == sorted(ref['out']) and sorted(got['grad']) == sorted(ref['grad'])
    e = {'out/' + n: rel_err(got['out'][n], ref['out'][n]) for n in ref['out']}
    for n, r in ref['grad'].items():
        g = got['grad'][n].detach().cpu().double()
        e['grad/' + n] = float((g - r.double()).abs().max() / terms[n]) if n in terms else rel_err(g, r)
    for n, r in ref['buf'].items():
        if not n.endswith('num_batches_tracked'):
            e['buf/' + n] = rel_err(got['buf'][n], r)
    return e


def clamp_violations(conf_dev):
    """device conf elements within 1e-4 * mean|conf| of the clamp's upper bound that are not the bound itself (the lower bound,
    -6, is out of a ReLU's reach): there a float32 and a float64 clamp mask may differ.  A condition on the seed."""
    near = ((conf_dev - 4.0).abs() <= 1e-4 * conf_dev.abs().mean()) & (conf_dev != 4.0)
    return int(near.sum())


def check_module(tag, module, state, inputs, call, training, tower_num=1):
    """device against float64 under the acceptance rule, both errors printed per tensor; the mask conditions; the statistics"""
    dev = run_device(module, inputs, call)
    r64 = run_reference(state, inputs, call, training, tower_num, dev['outs'], torch.float64)
    r32 = run_reference(state, inputs, call, training, tower_num, dev['outs'], torch.float32)
    ref = r64['ref']
    assert dev['names'] == ref.names                     # the hooks saw the BatchNorms in the restatement's order
    for k, (y, pre) in enumerate(zip(dev['outs'], ref.pres)):            # a seed inside the band is replaced, not excused
        assert bc.mask_violations(y, pre) == 0, (k, ref.names[k])
    for k in ref.conf_maps:
        assert clamp_violations(dev['outs'][k]) == 0, ref.names[k]
    e_hip, e_f32 = errors(dev, r64, r64['terms']), errors(r32, r64, r64['terms'])
    for n in sorted(e_hip):
        print('%s %-48s hip %.3g  torch-cpu float32 %.3g' % (tag, n, e_hip[n], e_f32[n]))
    worst = max(e_hip, key=e_hip.get)
    print('%s worst: %s hip %.3g float32 %.3g (%d tensors)' % (tag, worst, e_hip[worst], e_f32[worst], len(e_hip)))
    for n, e in e_hip.items():
        bound = max(BAR, 1.5 * e_f32[n])
        assert e <= bound, (tag, n, e, bound)
    for n, r in r64['buf'].items():                      # the statistics: moved by a training-mode call, once per call; eval: untouched
        if n.endswith('num_batches_tracked'):
            assert int(dev['buf'][n]) == int(r) == int(state[n]) + (ref.names.count(n.rsplit('.', 1)[0]) if training else 0), n
        elif not training or n.rsplit('.', 1)[0] not in ref.names:
            assert torch.equal(dev['buf'][n].cpu(), state[n]), n
        else:
            assert not torch.equal(dev['buf'][n].cpu(), state[n]), n
    return dev


def head_call(form):
    def call(fwd, lv):
        f = fwd if callable(fwd) and not isinstance(fwd, hc.HeadRef) else fwd.head
        res = f(*hc.form_args(form, dict(lv, memory_confidence=CONF)))
        return hc.flat_outputs(res), hc.loss_outputs(form, res)
    return call


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('form', hc.FORMS)
def test_head_slots(form, training):
    """HeadSlots(32, tower_num=2), batch 2, mem_size 3, 7 x 7 kernels, a 15 x 15 search map: every returned map, and every
    gradient of the fixed loss - the inputs, adjust, bias, both GroupDW logits, the BN affines, every conv - in each call form"""
    module, state = on_device(HeadSlots(hc.HEAD_C, tower_num=2), 'connect_model.', 11, training)
    inputs = {k: v for k, v in hc.head_inputs().items() if k != 'memory_confidence'}
    dev = check_module('head %s %s' % (form, 'train' if training else 'eval'), module, state, inputs, head_call(form), training, 2)
    want = {'offline': ['adjust', 'bias', 'reg_dw.weight', 'cls_dw.weight', 'bbox_tower.4.weight', 'cls_tower.1.bias'],
            'memory': ['cls_dw.weight', 'conf_fusion.conf_gen.1.weight', 'cls_memory_tower.4.bias', 'cls_memory_pred.weight'],
            'both': ['adjust', 'bias', 'reg_dw.weight', 'cls_dw.weight', 'conf_fusion.value_gen.1.bias', 'cls_memory_tower.1.weight']}
    for n in want[form] + ['search']:
        assert n in dev['grad'], n
    assert ('adjust' in dev['grad']) == (form != 'memory') and ('kernel' in dev['grad']) == (form != 'memory')
    assert ('memory_kernel' in dev['grad']) == (form != 'offline')


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_call_forms_and_the_cached_search_encoding(training):
    """the three call forms return the reference's five-tuples, share their maps bit for bit, and the memory form on the cached
    `cls_x` of an earlier offline call (`cls_x_store`) equals the uncached one bit for bit"""
    module, _ = on_device(HeadSlots(hc.HEAD_C, tower_num=2), 'connect_model.', 11, training)
    inp = {k: (v if k == 'memory_confidence' else v.to(DEV)) for k, v in hc.head_inputs().items()}
    s, z, mk = inp['search'], inp['kernel'], inp['memory_kernel']
    with torch.no_grad():
        assert module(s) is None
        off = module(s, z)
        mem = module(s, None, mk, CONF)
        cached = module(s, memory_kernel=mk, memory_confidence=CONF, cls_x_store=off[2])
        both = module(s, z, mk, CONF)
    assert len(off) == len(mem) == len(both) == 5 and off[4] is None and mem[:4] == (None, None, None, None)
    assert off[0].shape == (hc.BATCH, 4, 9, 9) and off[1].shape == (hc.BATCH, 1, 9, 9) and mem[4].shape == (hc.BATCH, 1, 9, 9)
    assert [tuple(t.shape[2:]) for t in off[2]] == [tuple(t.shape[2:]) for t in off[3]] == [(13, 13), (11, 13), (13, 11)]
    assert torch.equal(cached[4], mem[4]) and cached[:4] == (None, None, None, None)
    assert torch.equal(both[4], mem[4]) and torch.equal(both[0], off[0]) and torch.equal(both[1], off[1])
    for a, b in zip(both[2] + both[3], off[2] + off[3]):
        assert torch.equal(a, b)
    assert float(off[0].min()) > 0.0                     # exp


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_conf_fusion_slots(training):
    module, state = on_device(ConfFusionSlots(hc.HEAD_C), 'connect_model.conf_fusion.', 12, training)
    g = torch.Generator().manual_seed(4242)
    inputs = {'x': torch.randn(hc.BATCH, hc.MEM, hc.HEAD_C, 9, 9, generator=g)}

    def call(fwd, lv):
        out = fwd.conf_fusion('', lv['x']) if isinstance(fwd, hc.HeadRef) else fwd(lv['x'])
        return [('out', out)], [('out', out)]
    dev = check_module('conf_fusion %s' % ('train' if training else 'eval'), module, state, inputs, call, training)
    assert dev['out']['out'].shape == (hc.BATCH, hc.HEAD_C, 9, 9) and set(dev['grad']) == {'x'} | {n for n, _ in module.named_parameters()}


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_encoder_slots(training):
    module, state = on_device(EncoderSlots(hc.HEAD_C, hc.HEAD_C), 'connect_model.cls_encode.', 13, training)
    inp = hc.head_inputs()
    inputs = {'z': inp['kernel'], 'x': inp['search']}

    def call(fwd, lv):
        zs, xs = fwd.matrix('', lv['z'], lv['x']) if isinstance(fwd, hc.HeadRef) else fwd(lv['z'], lv['x'])
        named = [('z%d' % i, t) for i, t in enumerate(zs)] + [('x%d' % i, t) for i, t in enumerate(xs)]
        return named, named
    dev = check_module('encoder %s' % ('train' if training else 'eval'), module, state, inputs, call, training)
    # the None combinations of connect.py:67-74, on the same maps
    z, x = inputs['z'].to(DEV), inputs['x'].to(DEV)
    with torch.no_grad():
        zs, none = module(z, None)
        none2, xs = module(None, x)
        assert none is None and none2 is None and module() == (None, None) and module(x=None, z=None) == (None, None)
        for i in range(3):
            assert torch.equal(zs[i], dev['out']['z%d' % i]) and torch.equal(xs[i], dev['out']['x%d' % i])
