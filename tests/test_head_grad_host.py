"""CPU: the Conf_Fusion and box-exp entry points (csrc/head_grad.hip) are declared, exported and bound without joining the frozen
`hip.EXPORTS`; the launchers reject bad descriptors before they touch a device; the bindings, the autograd functions and the
head's holders have no CPU fallback; the closed forms of the header are the gradients of the float64 restatement
(tests/head_grad_cases.py); and that restatement is the reference's own `box_tower_reg` (tests/golden/head_train.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_grad_cases as hc
from head_grad_cases import rel_err
from usot_amd import autograd as hip_autograd, build, hip
from usot_amd.net import ConfFusionSlots, EncoderSlots, HeadSlots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_conf_fusion_fwd_f32', 'usot_conf_fusion_bwd_f32', 'usot_box_exp_fwd_f32', 'usot_box_exp_bwd_f32',
        'usot_box_exp_ws_floats')
ONE = 16                                               # an address that is never dereferenced on the paths tested here
CF_PTRS = ('conf', 'value', 'out', 'dout', 'dconf', 'dvalue')
BX_PTRS = ('p', 'adjust', 'bias', 'y', 'dy', 'dp', 'dadjust', 'dbias', 'ws')


def cf_desc(B=16, M=4, P=625, C=256, **kw):
    args = dict(B=B, M=M, P=P, C=C, **{p: ONE for p in CF_PTRS})
    args.update(kw)
    return hip.conf_fusion_desc(**args)


def bx_desc(R=10000, C=4, **kw):
    args = dict(R=R, C=C, **{p: ONE for p in BX_PTRS})
    args.update(kw)
    return hip.box_exp_desc(**args)


def struct_fields(text, name):
    m = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}' % name, text, flags=re.S)
    names = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(float|int32_t)\s*', '', decl).split(',')]
    return names


def test_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    L = ctypes.CDLL(build.build(force=False))
    for s in SYMS:
        assert re.search(r'\b(int|int64_t)\s+%s\s*\(' % s, text), s
        assert hasattr(L, s), s
        assert s not in hip.EXPORTS                     # the list the plan-replay golden mirrors stays as it is
        assert getattr(hip.lib(), s).argtypes is not None, s
    assert hip.lib().usot_box_exp_ws_floats.restype is ctypes.c_int64
    L.usot_abi_version.restype = ctypes.c_int
    assert L.usot_abi_version() == 6                    # symbols were added, no signature changed
    assert struct_fields(text, 'usot_conf_fusion_desc') == [f[0] for f in hip.ConfFusionDesc._fields_]
    assert struct_fields(text, 'usot_box_exp_desc') == [f[0] for f in hip.BoxExpDesc._fields_]
    assert ctypes.sizeof(hip.ConfFusionDesc) == 6 * 8 + 4 * 4 and ctypes.sizeof(hip.BoxExpDesc) == 9 * 8 + 2 * 4
    for name in ('conf_fusion_forward', 'conf_fusion_backward', 'box_exp_forward', 'box_exp_backward'):
        assert hasattr(hip, name)
    for name in ('ConfFusionFunction', 'conf_fusion', 'BoxExpFunction', 'box_exp'):
        assert hasattr(hip_autograd, name)


def test_box_exp_workspace_query():
    step = hip.box_exp_row_step()
    assert step >= 1
    for rows, parts in ((1, 1), (step - 1 or 1, 1), (step, 1), (step + 1, 2), (16 * 625, -(-16 * 625 // step))):
        assert hip.box_exp_ws_floats(rows) == 5 * parts, rows
    L = hip.lib()
    assert L.usot_box_exp_ws_floats(None) == -1
    assert L.usot_box_exp_ws_floats(ctypes.byref(bx_desc(R=0))) == -1 and L.usot_box_exp_ws_floats(ctypes.byref(bx_desc(C=8))) == -1


CF_BAD = [dict(B=0), dict(B=-1), dict(M=0), dict(M=-2), dict(P=0), dict(P=-5), dict(C=0), dict(C=2), dict(C=6), dict(C=255), dict(C=-4)]
BX_BAD = [dict(R=0), dict(R=-7), dict(C=0), dict(C=3), dict(C=8), dict(C=-4)]
ident = lambda b: '_'.join('%s%s' % kv for kv in b.items())


@pytest.mark.parametrize('bad', CF_BAD, ids=ident)
def test_bad_conf_fusion_descriptors_are_rejected_without_a_device(bad):
    L = hip.lib()
    assert L.usot_conf_fusion_fwd_f32(None, ctypes.byref(cf_desc(**bad))) == -1
    assert L.usot_conf_fusion_bwd_f32(None, ctypes.byref(cf_desc(**bad))) == -1


@pytest.mark.parametrize('bad', BX_BAD, ids=ident)
def test_bad_box_exp_descriptors_are_rejected_without_a_device(bad):
    L = hip.lib()
    assert L.usot_box_exp_fwd_f32(None, ctypes.byref(bx_desc(**bad))) == -1
    assert L.usot_box_exp_bwd_f32(None, ctypes.byref(bx_desc(**bad))) == -1
    assert L.usot_box_exp_ws_floats(ctypes.byref(bx_desc(**bad))) == -1


def test_missing_and_misaligned_pointers_are_rejected_without_a_device():
    L = hip.lib()
    cf_fwd = lambda **kw: L.usot_conf_fusion_fwd_f32(None, ctypes.byref(cf_desc(**kw)))
    cf_bwd = lambda **kw: L.usot_conf_fusion_bwd_f32(None, ctypes.byref(cf_desc(**kw)))
    bx_fwd = lambda **kw: L.usot_box_exp_fwd_f32(None, ctypes.byref(bx_desc(**kw)))
    bx_bwd = lambda **kw: L.usot_box_exp_bwd_f32(None, ctypes.byref(bx_desc(**kw)))
    for fn in (L.usot_conf_fusion_fwd_f32, L.usot_conf_fusion_bwd_f32, L.usot_box_exp_fwd_f32, L.usot_box_exp_bwd_f32):
        assert fn(None, None) == -1
    for missing in ('conf', 'value', 'out'):
        assert cf_fwd(**{missing: None}) == -1, missing
    for missing in ('conf', 'value', 'dout'):
        assert cf_bwd(**{missing: None}) == -1, missing
    for p in ('conf', 'value', 'out'):
        assert cf_fwd(**{p: ONE + 4}) == -1, p
    for p in ('conf', 'value', 'dout', 'dconf', 'dvalue'):
        assert cf_bwd(**{p: ONE + 8}) == -1, p
    for missing in ('p', 'adjust', 'bias', 'y'):
        assert bx_fwd(**{missing: None}) == -1, missing
    for missing in ('p', 'adjust', 'bias', 'dy', 'ws'):
        assert bx_bwd(**{missing: None}) == -1, missing
    for p in ('p', 'adjust', 'bias', 'y'):
        assert bx_fwd(**{p: ONE + 4}) == -1, p
    for p in ('p', 'adjust', 'bias', 'dy', 'dp', 'dadjust', 'dbias', 'ws'):
        assert bx_bwd(**{p: ONE + 4}) == -1, p
    # a backward call that wants nothing is a no-op, and says so without a device
    assert cf_bwd(dconf=None, dvalue=None) == 0
    assert bx_bwd(dp=None, dadjust=None, dbias=None, ws=None) == 0


@pytest.mark.parametrize('grad', [False, True])
def test_no_cpu_fallback(grad):
    conf, value = (t.reshape(6, 1, 7, 8) for t in hc.cf_operands(hc.CF_CASES[1])[:2])
    dout = torch.zeros(2, 1, 7, 8)
    with pytest.raises(hip.HipError):
        hip.conf_fusion_forward(conf, value, 2, 3)
    with pytest.raises(hip.HipError):
        hip.conf_fusion_backward(dout, conf, value, 2, 3)
    p, adjust, bias, dy = hc.box_operands(9)
    with pytest.raises(hip.HipError):
        hip.box_exp_forward(p, adjust, bias)
    with pytest.raises(hip.HipError):
        hip.box_exp_backward(dy, p, adjust, bias)
    cn, vn = conf.permute(0, 3, 1, 2).requires_grad_(grad), value.permute(0, 3, 1, 2)
    with pytest.raises(hip.HipError):
        hip_autograd.conf_fusion(cn, vn, 2, 3)
    with pytest.raises(hip.HipError):
        hip_autograd.box_exp(torch.zeros(1, 4, 3, 3, requires_grad=grad), adjust, bias)
    inp = hc.head_inputs()
    for mod, args in ((EncoderSlots(32, 32), (inp['kernel'], inp['search'])), (ConfFusionSlots(32), (torch.zeros(2, 3, 32, 9, 9),)),
                      (HeadSlots(32, tower_num=1), (inp['search'], inp['kernel'])),
                      (HeadSlots(32, tower_num=1), (inp['search'], None, inp['memory_kernel'], inp['memory_confidence']))):
        for p_ in mod.parameters():
            p_.requires_grad_(grad)
        for m in (mod.train(), mod.eval()):
            with pytest.raises(hip.HipError):
                m(*args)
    assert HeadSlots(32, tower_num=1)(inp['search']) is None and EncoderSlots(32, 32)() == (None, None)


def test_bindings_reject_bad_shapes_before_any_launch(monkeypatch):
    """with the device check out of the way the shape checks are reached on CPU tensors: each raises before the library is called"""
    monkeypatch.setattr(hip, '_dev', lambda t, dtype=torch.float32: t)
    monkeypatch.setattr(hip, 'lib', lambda: pytest.fail('the library was called'))
    conf, value, dout = hc.cf_operands(hc.CF_CASES[1])
    p, adjust, bias, dy = hc.box_operands(9)
    bad = [lambda: hip.conf_fusion_forward(conf, value, 3, 3),                      # B * M is not the map count
           lambda: hip.conf_fusion_forward(conf, value[:-1], 2, 3),
           lambda: hip.conf_fusion_forward(conf[..., :6], value[..., :6], 2, 3),    # not dense
           lambda: hip.conf_fusion_forward(conf[..., :6].contiguous(), value[..., :6].contiguous(), 2, 3),     # C % 4
           lambda: hip.conf_fusion_forward(conf, value, 0, 3),
           lambda: hip.conf_fusion_backward(dout[:1], conf, value, 2, 3),
           lambda: hip.conf_fusion_backward(dout[..., :4].contiguous(), conf, value, 2, 3),
           lambda: hip.box_exp_forward(p[:, :3].contiguous(), adjust, bias),
           lambda: hip.box_exp_forward(p, torch.zeros(2), bias),
           lambda: hip.box_exp_forward(p, adjust, torch.zeros(8)),
           lambda: hip.box_exp_backward(dy[:-1], p, adjust, bias),
           lambda: hip_autograd.conf_fusion(conf.reshape(6, 7, 8), value.reshape(6, 7, 8), 2, 3),
           lambda: hip_autograd.conf_fusion(conf.reshape(6, 8, 7, 1), value.reshape(6, 8, 7, 1), 3, 3),
           lambda: hip_autograd.box_exp(torch.zeros(1, 8, 3, 3), adjust, bias),
           lambda: hip_autograd.box_exp(torch.zeros(1, 4, 3, 3), adjust, torch.zeros(3))]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError):
            fn()
            pytest.fail('case %d was accepted' % i)


close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('c', hc.CF_CASES, ids=hc.cf_id)
def test_conf_fusion_closed_forms_are_the_float64_gradients(c):
    """the planted elements: conf == 4.0 and == -6.0 pass a gradient (torch.clamp's rule), conf > 4 and < -6 do not"""
    b, m, _, _ = c
    conf, value, dout = (t.double() for t in hc.cf_operands(c))
    cg, vg = conf.clone().requires_grad_(True), value.clone().requires_grad_(True)
    ref = hc.conf_fusion_ref(cg, vg, b, m)
    rc, rv = torch.autograd.grad(ref, (cg, vg), dout)
    out, dconf, dvalue = hc.conf_fusion_formulas(conf, value, dout, b, m)
    assert close(out, ref.detach()) and close(dconf, rc) and close(dvalue, rv)
    flat, gflat = conf.reshape(-1), rc.reshape(-1)
    assert float(flat[0]) == 4.0 and float(flat[1] if flat.numel() < 8 else flat[5]) == 5.5
    if m > 1:
        assert float(gflat[0]) != 0.0                                          # == 4.0: inside
        assert float(gflat[5]) == 0.0 and float(gflat[20]) == 0.0              # 5.5 and -7.5: outside
        assert float(flat[15]) == -6.0 and float(gflat[15]) != 0.0             # == -6.0: inside
    # the mask handed in (what the GPU tests do with the device's conf map) is the same function when it is the true mask
    cg2 = conf.clone().requires_grad_(True)
    masked = hc.conf_fusion_ref(cg2, value, b, m, (conf >= -6) & (conf <= 4))
    assert close(masked.detach(), ref.detach()) and close(torch.autograd.grad(masked, cg2, dout)[0], rc)


@pytest.mark.parametrize('rows', [1, 255, 257, 10000])
def test_box_exp_closed_forms_are_the_float64_gradients(rows):
    p, adjust, bias, dy = (t.double() for t in hc.box_operands(rows))
    leaves = [t.clone().requires_grad_(True) for t in (p, adjust, bias)]
    ref = hc.box_exp_ref(*leaves)
    rp, ra, rb = torch.autograd.grad(ref, leaves, dy)
    y, dp, dadjust, dbias, ta, tb = hc.box_exp_formulas(p, adjust, bias, dy)
    assert close(y, ref.detach()) and close(dp, rp)
    assert float((dadjust - ra).abs().max()) <= 1e-12 * float(ta) and float((dbias - rb.reshape(4)).abs().max()) <= 1e-12 * float(tb.max())
    # the NCHW form the module uses is the same function
    n = hc.box_exp_ref(p.t().reshape(1, 4, rows, 1), adjust, bias)
    assert close(n.reshape(4, rows).t(), y)


@pytest.fixture(scope='module')
def fixture():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'head_train.npz')) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_small_and_holds_the_seeded_inputs(fixture):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'head_train.npz')) < 1024 * 1024
    inp = hc.head_inputs()
    for k in ('search', 'kernel', 'memory_kernel'):
        assert fixture['in/' + k].dtype == np.float32 and np.array_equal(fixture['in/' + k], inp[k].numpy()), k


@pytest.mark.parametrize('form', hc.FORMS)
def test_restatement_is_the_reference_head_in_training_mode(form, fixture):
    """float64 on both sides; the fixture stores float32, so the difference is its rounding: 1e-6 (the project's scaled error)"""
    inp = {k: torch.from_numpy(fixture['in/' + k]) for k in ('search', 'kernel', 'memory_kernel')}
    state = hc.module_state(HeadSlots(hc.HEAD_C, tower_num=1), 'connect_model.', seed=hc.GOLD_SEED)
    params = hc.leaves_of(state)
    leaves = {k: v.double().requires_grad_(True) for k, v in inp.items()}
    ref = hc.HeadRef(params, training=True, tower_num=1)
    res = ref.head(*hc.form_args(form, dict(leaves, memory_confidence=torch.ones(hc.BATCH, hc.MEM))))
    outs = dict(hc.flat_outputs(res))
    if form == 'both':                                   # the reference's third result: the last map of the encoded list
        outs = {k: v for k, v in outs.items() if not k.startswith('cls_x')}
        outs['cls_x'] = res[2][2]
    want = sorted(k.split('/', 2)[2] for k in fixture if k.startswith(form + '/out/'))
    assert sorted(outs) == want
    errs = {}
    for name, t in outs.items():
        key = '%s/out/%s' % (form, name)
        errs[key] = rel_err(hc.sampled(key, t), fixture[key])
    loss = hc.fixed_loss(hc.loss_outputs(form, res))
    assert abs(float(loss.detach()) - float(fixture[form + '/loss'])) <= 1e-9 * abs(float(fixture[form + '/loss']))
    named = list(leaves.items()) + [(k, v) for k, v in params.items() if hc.is_param(k)]
    grads = torch.autograd.grad(loss, [t for _, t in named], allow_unused=True)
    got = {name for (name, _), g in zip(named, grads) if g is not None}
    assert got == {k.split('/', 2)[2] for k in fixture if k.startswith(form + '/grad/')}
    cancel = hc.cancelling_biases(ref.names, True)
    for (name, _), g in zip(named, grads):
        if g is None:
            continue
        key = '%s/grad/%s' % (form, name)
        if name in cancel:                               # zero in exact arithmetic: float64 noise on both sides
            assert float(np.abs(fixture[key]).max()) < 1e-9 and float(g.abs().max()) < 1e-9, key
        else:
            errs[key] = rel_err(hc.sampled(key, g), fixture[key])
    worst = max(errs, key=errs.get)
    print('%s: %d tensors, worst %s %.3g' % (form, len(errs), worst, errs[worst]))
    assert errs[worst] <= 1e-6, (worst, errs[worst])
    # training mode moved the statistics of every BatchNorm that ran, once per call
    for n in set(ref.names):
        assert int(params[n + '.num_batches_tracked']) == int(state[n + '.num_batches_tracked']) + ref.names.count(n)
        assert not torch.equal(params[n + '.running_mean'], state[n + '.running_mean'].double())
