"""CPU: the fused SGD step's entry points (csrc/sgd.hip) are declared, exported and bound without joining the frozen `hip.EXPORTS`;
the ctypes mirrors are the header's structs; the host-only table functions chunk every tensor exactly once and refuse bad records
with the image untouched; the launcher refuses bad descriptors before it touches a device; the float64 reference of
tests/sgd_cases.py is torch.optim.SGD; and usot_amd.optim.SGD keeps PyTorch's constructor, refusals and state-dict format and has
no CPU fallback.

The header's usot_sgd_tensor is 56 bytes, not 48: three pointers, an int64 and four floats are 48 already, and the flags word
with its padding brings the record to 56."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sgd_cases as sc
from usot_amd import build, hip, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('usot_sgd_chunk_elems', 'usot_sgd_grid_cap', 'usot_sgd_table_bytes', 'usot_sgd_table_fill', 'usot_sgd_step_f32')
ONE = 16                                               # an address that is never dereferenced here


def struct_fields(text, name):
    m = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}' % name, text, flags=re.S)
    names = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(float|int32_t|int64_t|void)\s*', '', decl).split(',')]
    return names


def test_symbols_declared_bound_and_not_in_exports():
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    L = C.CDLL(build.build(force=False))
    for s in SYMS:
        assert re.search(r'\b(int|int64_t)\s+%s\s*\(' % s, text), s
        assert hasattr(L, s), s
        assert s not in hip.EXPORTS
        assert getattr(hip.lib(), s).argtypes is not None, s
    assert hip.lib().usot_sgd_table_bytes.restype is C.c_int64
    L.usot_abi_version.restype = C.c_int
    assert L.usot_abi_version() == 6
    assert struct_fields(text, 'usot_sgd_tensor') == [f[0] for f in hip.SgdTensor._fields_]
    assert struct_fields(text, 'usot_sgd_launch') == [f[0] for f in hip.SgdLaunch._fields_]
    assert C.sizeof(hip.SgdTensor) == 3 * 8 + 8 + 4 * 4 + 2 * 4 == 56 and C.sizeof(hip.SgdLaunch) == 3 * 8 + 8 + 2 * 4 == 40
    assert (hip.SGD_FIRST, hip.SGD_NESTEROV, hip.SGD_MAXIMIZE) == (1, 2, 4)
    for name, value in (('USOT_SGD_FIRST', 1), ('USOT_SGD_NESTEROV', 2), ('USOT_SGD_MAXIMIZE', 4)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), text), name
    assert hip.sgd_chunk_elems() % 4 == 0 and hip.sgd_grid_cap() >= 1
    for name in ('sgd_table', 'sgd_step', 'sgd_chunk_elems', 'sgd_grid_cap'):
        assert hasattr(hip, name)
    from lib.utils import train_utils
    assert train_utils.is_valid_number is optim.is_valid_number


def record(n=5, p=ONE, g=2 * ONE, buf=3 * ONE, lr=0.1, weight_decay=0.01, momentum=0.9, grad_scale=1.0, flags=0, reserved=0):
    r = hip.SgdTensor()
    r.p, r.g, r.buf, r.n = p, g, buf, n
    r.lr, r.weight_decay, r.momentum, r.grad_scale, r.flags, r.reserved = lr, weight_decay, momentum, grad_scale, flags, reserved
    return r


def table_bytes(ns):
    arr, chunks = (C.c_int64 * max(len(ns), 1))(*ns), C.c_int64(-7)
    return hip.lib().usot_sgd_table_bytes(arr, len(ns), C.byref(chunks)), chunks.value


def test_chunks_cover_every_element_exactly_once():
    chunk = hip.sgd_chunk_elems()
    ns = sc.count_sizes(chunk) + [3, 0, 2 * chunk]
    want = [0, 1, 1, 1, 2, 4, 1, 0, 2]
    nbytes, chunks = table_bytes(ns)
    assert chunks == sum(want) == sc.n_chunks(ns, chunk) and nbytes == 56 * len(ns) + 8 * chunks
    recs = [record(n=n, p=ONE * (i + 1), flags=i % 8, lr=i) for i, n in enumerate(ns)]
    image, got = hip.sgd_table(recs)
    assert got == chunks and len(image) == nbytes
    raw = bytes(image)
    back = (hip.SgdTensor * len(ns)).from_buffer_copy(raw[:56 * len(ns)])
    for r, b in zip(recs, back):
        assert [getattr(b, f[0]) for f in hip.SgdTensor._fields_] == [getattr(r, f[0]) for f in hip.SgdTensor._fields_]
    lst = np.frombuffer(raw[56 * len(ns):], dtype=np.int32).reshape(-1, 2)
    assert lst.shape[0] == chunks
    covered = [np.zeros(n, dtype=np.int32) for n in ns]
    for t, c in lst.tolist():
        assert 0 <= t < len(ns) and 0 <= c * chunk < ns[t], (t, c)
        covered[t][c * chunk:min((c + 1) * chunk, ns[t])] += 1
    assert all((cv == 1).all() for cv in covered)
    assert [int((lst[:, 0] == t).sum()) for t in range(len(ns))] == want
    assert lst[:, 0].tolist() == sorted(lst[:, 0].tolist())             # tensor by tensor, chunks ascending
    # `reserved` does not reach the image: equal records give equal bytes
    again, _ = hip.sgd_table([record(n=n, p=ONE * (i + 1), flags=i % 8, lr=i, reserved=99) for i, n in enumerate(ns)])
    assert bytes(again) == raw
    assert table_bytes([0, 0]) == (2 * 56, 0)
    L = hip.lib()
    assert L.usot_sgd_table_bytes(None, 1, None) == -1 and table_bytes([])[0] == -1 and table_bytes([4, -1])[0] == -1
    assert table_bytes([(1 << 31) * chunk])[0] == -1                    # more chunks than an int32 indexes
    one = (C.c_int64 * 1)(7)
    assert L.usot_sgd_table_bytes(one, 1, None) == 56 + 8               # the chunk count is optional


NAN, INF = float('nan'), float('inf')
REFUSED = [dict(p=None), dict(g=None), dict(buf=None), dict(p=ONE + 2), dict(g=ONE + 1), dict(buf=ONE + 3), dict(n=-1),
           dict(lr=NAN), dict(lr=INF), dict(lr=-0.1), dict(weight_decay=NAN), dict(weight_decay=INF), dict(weight_decay=-1e-4),
           dict(momentum=NAN), dict(momentum=INF), dict(momentum=-0.9), dict(grad_scale=NAN), dict(grad_scale=INF),
           dict(grad_scale=-INF), dict(flags=2, momentum=0.0), dict(flags=2, grad_scale=0.5), dict(flags=8), dict(flags=-1),
           dict(flags=1 << 16)]
ident = lambda b: '_'.join('%s%s' % kv for kv in b.items())


@pytest.mark.parametrize('bad', REFUSED, ids=ident)
def test_bad_records_are_refused_with_the_image_untouched(bad):
    L = hip.lib()
    for where in (0, 2):
        recs = [record(n=9), record(n=0), record(n=5000)]
        recs[where] = record(**dict(dict(n=9), **bad))
        arr = (hip.SgdTensor * 3)(*recs)
        image = (C.c_ubyte * 4096)(*([0xA5] * 4096))
        assert L.usot_sgd_table_fill(arr, 3, image, 4096) == -1, where
        assert bytes(image) == b'\xa5' * 4096
    with pytest.raises(hip.HipError):
        hip.sgd_table([record(**bad)])


def test_table_fill_refusals_that_are_not_about_one_record():
    L = hip.lib()
    chunk = hip.sgd_chunk_elems()
    arr = (hip.SgdTensor * 2)(record(n=chunk + 1), record(n=3))
    need = 2 * 56 + 3 * 8
    image = (C.c_ubyte * need)(*([0xA5] * need))
    for args in ((None, 2, image, need), (arr, 0, image, need), (arr, -1, image, need), (arr, 2, None, need),
                 (arr, 2, image, need - 1), (arr, 2, image, 0), (arr, 2, image, -5)):
        assert L.usot_sgd_table_fill(*args) == -1
        assert bytes(image) == b'\xa5' * need
    assert L.usot_sgd_table_fill(arr, 2, image, need) == 0 and bytes(image) != b'\xa5' * need
    # what is allowed: no buffer without momentum, a negative grad_scale (dampening above 1), n == 0, every flag at once
    for ok in (dict(buf=None, momentum=0.0), dict(grad_scale=-0.5), dict(n=0), dict(flags=7), dict(lr=0.0, weight_decay=0.0)):
        hip.sgd_table([record(**ok)])
    with pytest.raises(hip.HipError):
        hip.sgd_table([])


def test_launcher_refuses_bad_descriptors_without_a_device():
    L = hip.lib()

    def launch(**kw):
        d = hip.SgdLaunch()
        d.table, d.T, d.n_chunks = ONE, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return L.usot_sgd_step_f32(None, C.byref(d))
    assert L.usot_sgd_step_f32(None, None) == -1
    for bad in (dict(table=None), dict(table=ONE + 4), dict(T=0), dict(T=-3), dict(n_chunks=-1), dict(n_chunks=1 << 31),
                dict(guard=ONE + 2), dict(counters=ONE + 1)):
        assert launch(**bad) == -1, bad
    assert launch(n_chunks=0) == 0                       # nothing to do: no launch, no device
    assert launch(n_chunks=0, guard=ONE, counters=ONE, zero_grads=1) == 0


@pytest.mark.parametrize('flags,momentum', [(f, m) for f in sc.FLAGS for m in (0.5, 0.0) if m or not f[1]], ids=str)
def test_reference_is_torch_sgd(flags, momentum):
    """three steps from a missing buffer on the exact operands: float64 restatement == torch.optim.SGD in float64 AND in float32,
    bit for bit; on the rounding family float64 agrees with float64 to its own rounding"""
    damp, nest, maxi = flags
    for family, dtypes in (('exact', (torch.float64, torch.float32)), ('rounding', (torch.float64,))):
        h = sc.hyp(damp, nest, maxi, momentum=momentum) if family == 'exact' else dict(sc.REFERENCE, dampening=damp, nesterov=nest,
                                                                                         maximize=maxi, momentum=momentum and sc.REFERENCE['momentum'])
        n = 777
        p0 = sc.exact_operand(n, 1) if family == 'exact' else sc.rounding_operands(n, 1)[0]
        grads = [sc.exact_operand(n, 10 + s) if family == 'exact' else sc.rounding_operands(n, 10 + s)[1] for s in range(sc.STEPS)]
        rp, rb = p0.double(), None
        for s in range(sc.STEPS):
            rp, rb = sc.ref_step(rp, grads[s], rb, h, first=s == 0, exact=family == 'exact')
        for dtype in dtypes:
            q = torch.nn.Parameter(p0.to(dtype))
            opt = torch.optim.SGD([q], **h)
            for s in range(sc.STEPS):
                q.grad = grads[s].to(dtype)
                opt.step()
            buf = opt.state[q].get('momentum_buffer')
            if family == 'exact':
                assert torch.equal(q.detach().double(), rp)
                assert (buf is None and rb is None) or torch.equal(buf.double(), rb)
            else:
                assert float((q.detach() - rp).abs().max()) <= 1e-14 * float(rp.abs().max())
                assert buf is None or float((buf - rb).abs().max()) <= 1e-14 * float(rb.abs().max())


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 4), (5,), (1,))]


def test_state_dict_round_trips_both_ways():
    kw = dict(lr=0.005, momentum=0.9, weight_decay=1e-4)
    # torch -> this class
    tp = _params()
    theirs = torch.optim.SGD([dict(params=tp[:2]), dict(params=tp[2:], lr=0.05)], **kw)
    for p in tp:
        p.grad = torch.ones_like(p)
    theirs.step()
    ours = optim.SGD([dict(params=_params()[:2]), dict(params=_params()[2:], lr=0.5)], **kw)
    ours.load_state_dict(theirs.state_dict())
    assert [g['lr'] for g in ours.param_groups] == [0.005, 0.05]
    for mine, their in zip((p for g in ours.param_groups for p in g['params']), tp):
        assert torch.equal(ours.state[mine]['momentum_buffer'], theirs.state[their]['momentum_buffer'])
    assert ours.state_dict()['state'].keys() == theirs.state_dict()['state'].keys()
    # this class -> torch, including a parameter that never stepped
    op = _params(1)
    ours = optim.SGD([dict(params=op[:1], lr=0.1), dict(params=op[1:])], nesterov=True, zero_grads=True, **kw)
    ours.state[op[0]]['momentum_buffer'] = torch.full_like(op[0], 0.25)
    ours.state[op[1]]['momentum_buffer'] = torch.full_like(op[1], -2.0)
    sd = ours.state_dict()
    assert set(sd['param_groups'][0]) == set(theirs.state_dict()['param_groups'][0])          # the same group keys: no zero_grads
    tp = _params(1)
    theirs = torch.optim.SGD([dict(params=tp[:1]), dict(params=tp[1:])], lr=1.0)
    theirs.load_state_dict(sd)
    assert theirs.param_groups[0]['lr'] == 0.1 and theirs.param_groups[1]['nesterov'] is True
    assert float(theirs.state[tp[0]]['momentum_buffer'][0, 0]) == 0.25 and float(theirs.state[tp[1]]['momentum_buffer'][0]) == -2.0
    assert tp[2] not in theirs.state
    for p in tp:
        p.grad = torch.ones_like(p)
    theirs.step()                                        # the loaded state is one torch can step from
    # and through a file, as the reference's save_model / restore_from do
    import io
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    again = optim.SGD([dict(params=_params(1)[:1]), dict(params=_params(1)[1:])], lr=1.0)
    again.load_state_dict(torch.load(f))
    assert again.param_groups[0]['lr'] == 0.1 and len(again.state) == 2 and again.zero_grads is False


def test_is_valid_number_matches_its_definition():
    f = optim.is_valid_number
    assert [f(NAN), f(INF), f(-INF), f(1e4), f(float(np.nextafter(1e4, np.inf))), f(-1e30), f(0.5)] == \
        [False, False, False, True, False, True, True]
    for loss, valid in sc.GUARD_LOSSES:
        assert f(loss) == valid == sc.is_valid_number(loss)
    assert f(torch.tensor(3.0)) and not f(torch.tensor(NAN))              # as the loop calls it on loss.item() or a tensor


def test_constructor_refusals_are_pytorchs():
    for kw in (dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1),
               dict(lr=torch.tensor([0.1, 0.2]))):
        msgs = []
        for cls in (torch.optim.SGD, optim.SGD):
            with pytest.raises(ValueError) as e:
                cls(_params(), **dict(dict(lr=0.1), **kw))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], kw
    with pytest.raises(ValueError):
        optim.SGD([], lr=0.1)                            # the base class's empty-list refusal
    o = optim.SGD(_params(), lr=0.1, momentum=0.9, foreach=True, fused=False, differentiable=False, zero_grads=True)
    assert o.defaults['foreach'] is True and o.defaults['fused'] is False and 'zero_grads' not in o.defaults and o.zero_grads
    assert set(o.defaults) == set(torch.optim.SGD(_params(), lr=0.1).defaults)
    assert o.counters() == (0, 0) and o.uploads == 0


def test_no_cpu_fallback():
    ps = _params()
    o = optim.SGD(ps, lr=0.1, momentum=0.9)
    assert o.step() is None                              # no gradients: nothing to do, as in PyTorch
    before = [p.detach().clone() for p in ps]
    ps[1].grad = torch.ones_like(ps[1])
    with pytest.raises(hip.HipError):
        o.step()
    with pytest.raises(hip.HipError):
        o.step(loss=torch.tensor(0.5))
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, ps)) and o.uploads == 0
    with pytest.raises(hip.HipError):
        hip.sgd_step(torch.zeros(64, dtype=torch.uint8), 1, 1)
    o.zero_grad()
    assert ps[1].grad is not None and not ps[1].grad.any()              # kept, zeroed
    o.zero_grad(set_to_none=True)
    assert ps[1].grad is None
