"""GPU: the fused SGD step (csrc/sgd.hip) through the raw table and launcher, and usot_amd.optim.SGD over it, against the float64
restatement of tests/sgd_cases.py, which tests/test_sgd_host.py holds to torch.optim.SGD itself.

Every p, g and buf is the interior of a canary allocation of tests/guarded.py; a tensor that starts 1, 2 or 3 floats into its
allocation (the scalar path) has a sentinel in that slack, which must survive.  A first-step tensor's buffer holds the NaN canary
before the launch: the kernel may not read it.  g is compared with a snapshot whenever zero_grads is off.

EXACT family: equality with float64 (sgd_cases asserts that every intermediate is a float32 number).  ROUNDING family: the bound
of sgd_cases' docstring, |p' - ref| <= 8u(|p| + lr S) and |buf' - ref| <= 8u S_b; the test first shows that PyTorch-CPU float32
itself stays below it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import sgd_cases as sc  # noqa: E402
from usot_amd import hip, optim  # noqa: E402

DEV = 'cuda:0'
SENT = -77.0
CANARY32 = 0x7FC17FC1


@pytest.fixture(autouse=True)
def _memory_guard():
    """device allocations of usot_amd.optim (buffers, table, counters) sit between canaries too; every guard handed out during the
    test is checked when it ends"""
    with guarded.patched(optim):
        yield


class Placed(object):
    """n floats starting `off` floats into a canary allocation; what is not the tensor holds SENT"""

    def __init__(self, n, off, init=None):
        self.whole = guarded.alloc(off + max(n, 1), torch.float32, DEV, 'full', SENT)
        self.view = self.whole[off:off + n]
        self.n, self.off, self.ptr = n, off, self.whole.data_ptr() + 4 * off
        if init is None:
            self.view.view(torch.int32).fill_(CANARY32)
        else:
            self.view.copy_(init)

    def slack(self):
        """0-d bool tensors: the floats around the tensor are untouched"""
        return [(self.whole[:self.off] == SENT).all(), (self.whole[self.off + self.n:] == SENT).all()]


class Slot(object):
    def __init__(self, n, h, offs=(0, 0, 0), first=True, seed=0, family='exact'):
        self.n, self.h, self.first, self.seed, self.family = n, h, first, seed, family
        if family == 'exact':
            p0, b0 = sc.exact_operand(n, seed), sc.exact_operand(n, seed + 1)
        else:
            p0, _, b0 = sc.rounding_operands(n, seed)
        mom = h['momentum'] != 0
        self.rp, self.rb = p0.double(), b0.double() if mom and not first else None
        self.P, self.G = Placed(n, offs[0], p0), Placed(n, offs[1], torch.zeros(n))
        self.B = Placed(n, offs[2], None if first else b0) if mom else None

    def grad(self, step):
        if self.family == 'exact':
            return sc.exact_operand(self.n, self.seed + 100 + step)
        return sc.rounding_operands(self.n, self.seed + 100 + step)[1]

    def record(self):
        r, h = hip.SgdTensor(), self.h
        r.p, r.g, r.buf, r.n = self.P.ptr, self.G.ptr, self.B.ptr if self.B else None, self.n
        r.lr, r.weight_decay, r.momentum, r.grad_scale = h['lr'], h['weight_decay'], h['momentum'], sc.grad_scale(h)
        r.flags = sc.flags_of(h, self.first)
        return r


def launch(slots, guard=None, counters=None, zero=False):
    image, n_chunks = hip.sgd_table([s.record() for s in slots])
    table = guarded.put(torch.frombuffer(bytearray(image), dtype=torch.uint8), DEV)
    hip.sgd_step(table, len(slots), n_chunks, guard=guard, counters=counters, zero_grads=zero)
    return n_chunks


def run_steps(slots, steps=1, zero=False, exact=True, check=True):
    """`steps` launches over the slots with a fresh gradient each; after every launch each p and buf equals the float64 step
    (exact family), g is its snapshot or zero, and the slack is untouched"""
    for step in range(steps):
        grads = [s.grad(step) for s in slots]
        for s, g in zip(slots, grads):
            s.G.view.copy_(g)
        launch(slots, zero=zero)
        oks = []
        for s, g in zip(slots, grads):
            s.rp, s.rb = sc.ref_step(s.rp, g, s.rb, s.h, s.first, exact=exact)
            s.first = False
            if check:
                assert torch.equal(s.P.view.cpu().double(), s.rp), ('p', s.n, s.h, step)
                if s.B:
                    assert torch.equal(s.B.view.cpu().double(), s.rb), ('buf', s.n, s.h, step)
                assert torch.equal(s.G.view.cpu(), torch.zeros(s.n) if zero else g), ('g', s.n, step)
            for pl in (s.P, s.G) + ((s.B,) if s.B else ()):
                oks += pl.slack()
        assert bool(torch.stack(oks).all()), 'a float beside a tensor was overwritten'


# ---- 1. exact family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero', [False, True], ids=['keep_g', 'zero_g'])
@pytest.mark.parametrize('flags', sc.FLAGS, ids=str)
def test_exact_sweep_of_sizes(flags, zero):
    """every size of the sweep in ONE table, three steps from a missing buffer: one, two and three chunks, every n % 4 tail"""
    sizes = sc.sweep_sizes(hip.sgd_chunk_elems())
    slots = [Slot(n, sc.hyp(*flags), seed=7 * i) for i, n in enumerate(sizes)]
    run_steps(slots, steps=sc.STEPS, zero=zero)


def test_exact_offsets_take_the_scalar_path():
    """p, g and buf each 0 .. 3 floats off 16-byte alignment, independently: only (0, 0, 0) may use 16-byte accesses"""
    sizes = sc.offset_sizes(hip.sgd_chunk_elems())
    slots = [Slot(n, sc.hyp(*sc.FLAGS[(i + j) % len(sc.FLAGS)]), offs=offs, seed=11 * i + j)
             for i, offs in enumerate(sc.OFFSETS) for j, n in enumerate(sizes)]
    assert {s.P.ptr % 16 for s in slots} == {0, 4, 8, 12} == {s.G.ptr % 16 for s in slots} == {s.B.ptr % 16 for s in slots}
    run_steps(slots, steps=sc.STEPS, zero=True)


def test_exact_without_momentum_and_a_null_buffer():
    chunk = hip.sgd_chunk_elems()
    slots = [Slot(n, sc.hyp(0.0, False, maxi, momentum=0.0), offs=(o, 0, 0), seed=n) for n in (1, 5, 64, chunk + 2) for maxi in (False, True)
             for o in (0, 1)]
    assert all(s.B is None and s.record().buf is None for s in slots)
    run_steps(slots, steps=sc.STEPS)


def mix_slots(family='exact'):
    """300 tensors, per-tensor hyper-parameters; two of three are on their first step, the others bring a buffer"""
    sizes = sc.mix_sizes(hip.sgd_chunk_elems())
    return [Slot(n, sc.mix_hyp(i), first=i % 3 != 0, seed=13 * i, family=family) for i, n in enumerate(sizes)]


def test_exact_mixed_table():
    slots = mix_slots()
    assert any(s.first and s.B for s in slots) and any(not s.first and s.B for s in slots) and any(s.B is None for s in slots)
    assert sum(s.n == 0 for s in slots) == 50
    run_steps(slots, steps=2, zero=False)


@pytest.mark.parametrize('extra', [1, sc.RAGGED])
def test_exact_more_chunks_than_the_grid(extra):
    """cap + 1 and cap + RAGGED chunks: some workgroups take a second chunk, most do not"""
    chunk, cap = hip.sgd_chunk_elems(), hip.sgd_grid_cap()
    sizes = sc.over_cap_sizes(chunk, cap, extra)
    slots = [Slot(n, sc.hyp(*sc.FLAGS[i % len(sc.FLAGS)]), first=i % 2 == 0, seed=3 * i) for i, n in enumerate(sizes)]
    grads = [s.grad(0) for s in slots]
    for s, g in zip(slots, grads):
        s.G.view.copy_(g)
    assert launch(slots) == cap + extra
    for s, g in zip(slots, grads):
        rp, rb = sc.ref_step(s.rp, g, s.rb, s.h, s.first, exact=True)
        assert torch.equal(s.P.view.cpu().double(), rp) and torch.equal(s.B.view.cpu().double(), rb), s.n
        assert torch.equal(s.G.view.cpu(), g)


# ---- 2. position independence ----------------------------------------------------------------------------------------------------
def test_position_independence_and_repeatability():
    """operands that round (the rounding family under per-tensor hyper-parameters): each tensor of the mixed table stepped alone in
    a one-tensor table, and the whole table stepped again from the same inputs, give the same bits"""
    def fresh():
        slots = mix_slots('rounding')
        for i, s in enumerate(slots):
            s.h = dict(s.h, lr=s.h['lr'] * 0.37, weight_decay=s.h['weight_decay'] * 0.011, momentum=s.h['momentum'] * 1.7)
            s.G.view.copy_(s.grad(0))
        return slots
    bits = lambda s: (s.P.view.cpu().view(torch.int32), s.B.view.cpu().view(torch.int32) if s.B else None)
    same = lambda a, b: torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))
    first = fresh()
    launch(first)
    again = fresh()
    launch(again)
    alone = fresh()
    for s in alone:
        launch([s])
    for a, b, c in zip(first, again, alone):
        assert same(bits(a), bits(b)), ('twice', a.n, a.h)
        assert same(bits(a), bits(c)), ('alone', a.n, a.h)
    big = [s for s in first if s.n > 64]
    rp, _ = sc.ref_step(big[0].rp, big[0].grad(0), big[0].rb, big[0].h, big[0].first)
    assert not torch.equal(big[0].P.view.cpu().double(), rp)           # these operands do round: the comparison above is not vacuous


# ---- 3. rounding family ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [0, 1], ids=['vector', 'scalar'])
@pytest.mark.parametrize('nesterov', [False, True])
def test_rounding_family_within_the_bound(nesterov, off):
    n = (1 << 20) + 3
    h = dict(sc.REFERENCE, dampening=0.0, nesterov=nesterov, maximize=False)
    s = Slot(n, h, offs=(off, off, off), first=False, seed=5, family='rounding')
    p, g, buf = sc.rounding_operands(n, 5)
    g = s.grad(0)
    rp, rb = sc.ref_step(p, g, buf, h, first=False)
    bp, bb = sc.bound(p, g, buf, h, first=False)
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    cpu = torch.optim.SGD([q], **h)
    cpu.state[q]['momentum_buffer'] = buf.clone()
    cpu.step()
    ratio = lambda gp, gb: max(float(((gp.double() - rp).abs() / bp).max()), float(((gb.double() - rb).abs() / bb).max()))
    ref_ratio = ratio(q.detach(), cpu.state[q]['momentum_buffer'])
    s.G.view.copy_(g)
    snap = guarded.snapshot(s.G.view)
    launch([s])
    got = ratio(s.P.view.cpu(), s.B.view.cpu())
    print('nesterov %s off %d: HIP at %.3f of the bound, PyTorch-CPU float32 at %.3f' % (nesterov, off, got, ref_ratio))
    assert ref_ratio < 1.0
    assert got <= 1.0
    guarded.unchanged(s.G.view, snap, 'g')


# ---- 4. guard, counters, zero_grads ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero', [False, True], ids=['keep_g', 'zero_g'])
@pytest.mark.parametrize('loss,valid', sc.GUARD_LOSSES, ids=[repr(l) for l, _ in sc.GUARD_LOSSES])
def test_guard(loss, valid, zero):
    chunk = hip.sgd_chunk_elems()
    slots = [Slot(n, sc.hyp(*sc.FLAGS[i % len(sc.FLAGS)]), offs=(i % 2,) * 3, first=False, seed=i) for i, n in enumerate((1, 5, 64, chunk + 3, 2 * chunk))]
    grads = [s.grad(0) for s in slots]
    for s, g in zip(slots, grads):
        s.G.view.copy_(g)
    before = [(guarded.snapshot(s.P.view), guarded.snapshot(s.B.view)) for s in slots]
    guard = guarded.put(torch.tensor([loss], dtype=torch.float32), DEV)
    counters = guarded.put(torch.tensor([40, 2], dtype=torch.int32), DEV)
    gsnap = guarded.snapshot(guard)
    launch(slots, guard=guard, counters=counters, zero=zero)
    assert counters.tolist() == ([41, 2] if valid else [40, 3])
    guarded.unchanged(guard, gsnap, 'guard')
    oks = []
    for s, g, (sp, sb) in zip(slots, grads, before):
        if valid:
            rp, rb = sc.ref_step(s.rp, g, s.rb, s.h, False, exact=True)
            assert torch.equal(s.P.view.cpu().double(), rp) and torch.equal(s.B.view.cpu().double(), rb)
        else:
            guarded.unchanged(s.P.view, sp, 'p of a skipped step')
            guarded.unchanged(s.B.view, sb, 'buf of a skipped step')
        assert torch.equal(s.G.view.cpu(), torch.zeros(s.n) if zero else g)
        for pl in (s.P, s.G, s.B):
            oks += pl.slack()
    assert bool(torch.stack(oks).all())


def test_no_guard_no_counters_and_an_empty_table():
    s = Slot(0, sc.hyp(), first=False)
    assert launch([s]) == 0                              # n == 0: no chunk, no launch
    assert bool(torch.stack(s.P.slack() + s.G.slack() + s.B.slack()).all())


# ---- 5. the class ----------------------------------------------------------------------------------------------------------------
def test_a_skipped_first_step_leaves_the_buffer_unborn():
    """dampening 0.5: a buffer that was taken for initialised would give buf = 0.5 d instead of d on the next step"""
    h = sc.hyp(0.5, False, False)
    p0, g0 = sc.exact_operand(4099, 1), sc.exact_operand(4099, 2)
    p = guarded.put(p0, DEV).requires_grad_(True)
    p.grad = guarded.put(g0, DEV)
    opt = optim.SGD([p], **h)
    nan, fine = (guarded.put(torch.tensor(v, dtype=torch.float32), DEV) for v in (float('nan'), 0.5))
    opt.step(loss=nan)
    assert torch.equal(p.detach().cpu(), p0) and torch.equal(p.grad.cpu(), g0)
    assert 'momentum_buffer' not in opt.state[p] and opt.counters() == (0, 1) and opt.uploads == 1
    opt.step(loss=fine)
    rp, rb = sc.ref_step(p0, g0, None, h, first=True, exact=True)
    assert torch.equal(p.detach().cpu().double(), rp) and torch.equal(opt.state[p]['momentum_buffer'].cpu().double(), rb)
    assert opt.counters() == (1, 1) and opt.uploads == 1               # the same image as the skipped step's: no second copy
    opt.step(loss=fine)
    rp, rb = sc.ref_step(rp, g0, rb, h, first=False, exact=True)
    assert torch.equal(p.detach().cpu().double(), rp) and torch.equal(opt.state[p]['momentum_buffer'].cpu().double(), rb)
    assert opt.counters() == (2, 1) and opt.uploads == 2               # the first-step flag was cleared


def test_steady_state_notices_what_moves():
    """after a fully validated step the class re-checks identities and addresses only; whatever is replaced must still be honoured.
    Steps 1 - 3 are the exact family's; later ones start from the device's own values and are held to the one-step bound."""
    h = sc.hyp(0.5, False, True)
    p0, grads = sc.exact_operand(4099, 1), [sc.exact_operand(4099, 20 + i) for i in range(4)]
    p = guarded.put(p0, DEV).requires_grad_(True)
    p.grad = guarded.put(grads[0], DEV)
    opt = optim.SGD([p], **h)
    rp, rb = p0.double(), None
    for i in range(2):
        p.grad.copy_(grads[i])
        opt.step()
        rp, rb = sc.ref_step(rp, grads[i], rb, h, first=i == 0, exact=True)
    assert opt.uploads == 2 and opt._plan is not None and torch.equal(p.detach().cpu().double(), rp)
    p.grad = guarded.put(grads[2], DEV)                               # another gradient tensor at another address
    opt.step()
    rp, rb = sc.ref_step(rp, grads[2], rb, h, first=False, exact=True)
    assert opt.uploads == 3 and torch.equal(p.detach().cpu().double(), rp)
    assert torch.equal(opt.state[p]['momentum_buffer'].cpu().double(), rb)

    def one_more(g, buf):
        start = p.detach().cpu()
        opt.step()
        want_p, want_b = sc.ref_step(start, g, buf, h, first=False)
        bp, bb = sc.bound(start, g, buf, h, first=False)
        assert bool(((p.detach().cpu().double() - want_p).abs() <= bp).all())
        assert bool(((opt.state[p]['momentum_buffer'].cpu().double() - want_b).abs() <= bb).all())
    fresh = sc.exact_operand(4099, 77)
    opt.state[p]['momentum_buffer'] = guarded.put(fresh, DEV)         # a buffer replaced by hand (or by load_state_dict)
    one_more(grads[2], fresh)
    assert opt.uploads == 4
    one_more(grads[2], opt.state[p]['momentum_buffer'].cpu())
    assert opt.uploads == 4 and opt._plan is not None                 # steady again
    keep = p.detach().clone()
    p.grad.data = p.grad.data.half()                                  # what module.half() does to a gradient
    with pytest.raises(hip.HipError):
        opt.step()
    assert torch.equal(p.detach(), keep)


SHAPES = [(64, 64, 3, 3), (256,), (1,), (4,), (1000, 7), (33,)]
LRS = [sc.f32(0.005), sc.f32(0.05), sc.f32(0.0005)]
NO_GRAD = 5


def _class_grads(step):
    return [None if i == NO_GRAD else sc.rounding_operands(torch.Size(s).numel(), 50 * step + i)[1].reshape(s) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize('zero', [False, True], ids=['keep_g', 'zero_g'])
@pytest.mark.parametrize('nesterov', [False, True])
def test_class_against_torch_sgd_in_float64(nesterov, zero):
    """three groups with their own lr, one parameter without a gradient, five steps with an lr changed between steps 2 and 3,
    against torch.optim.SGD on CPU float64 with the same (fp32-rounded) hyper-parameters.  Tolerance: the one-step bound of
    sgd_cases plus what the step - linear in p and buf - carries over of the previous steps' allowance (sc.spread)."""
    kw = dict(momentum=sc.REFERENCE['momentum'], weight_decay=sc.REFERENCE['weight_decay'], nesterov=nesterov)
    init = [sc.rounding_operands(torch.Size(s).numel(), i)[0].reshape(s) for i, s in enumerate(SHAPES)]
    dev = [guarded.put(t, DEV).requires_grad_(True) for t in init]
    ref = [torch.nn.Parameter(t.double()) for t in init]
    groups = lambda ps: [dict(params=ps[2 * k:2 * k + 2], lr=LRS[k]) for k in range(3)]
    ours, theirs = optim.SGD(groups(dev), lr=1.0, zero_grads=zero, **kw), torch.optim.SGD(groups(ref), lr=1.0, **kw)
    keep = guarded.snapshot(dev[NO_GRAD])
    ep = [torch.zeros(t.numel(), dtype=torch.float64) for t in init]
    eb = [torch.zeros(t.numel(), dtype=torch.float64) for t in init]
    uploads, worst = [], 0.0
    for step in range(5):
        if step == 2:
            ours.param_groups[0]['lr'] = theirs.param_groups[0]['lr'] = sc.f32(0.001)
        grads = _class_grads(step)
        for i, g in enumerate(grads):
            if g is not None:
                if dev[i].grad is None:
                    dev[i].grad = guarded.put(g, DEV)
                else:
                    dev[i].grad.copy_(g)
                ref[i].grad = g.double()
        addr = [None if p.grad is None else p.grad.data_ptr() for p in dev]
        for k, group in enumerate(theirs.param_groups):               # the allowance, from the float64 state before the step
            h = dict(lr=group['lr'], momentum=group['momentum'], weight_decay=group['weight_decay'], dampening=0.0,
                     nesterov=nesterov, maximize=False)
            for i in (2 * k, 2 * k + 1):
                if grads[i] is None:
                    continue
                b = theirs.state[ref[i]].get('momentum_buffer')
                flat = lambda t: None if t is None else t.detach().reshape(-1)
                bp, bb = sc.bound(flat(ref[i]), flat(grads[i]), flat(b), h, first=step == 0)
                cp, cb = sc.spread(ep[i], 0 * ep[i], eb[i], h, first=step == 0)
                ep[i], eb[i] = cp + bp, cb + bb
        ours.step()
        theirs.step()
        uploads.append(ours.uploads)
        for i, g in enumerate(grads):
            if g is None:
                continue
            dp = (dev[i].detach().cpu().double() - ref[i].detach()).abs().reshape(-1)
            db = (ours.state[dev[i]]['momentum_buffer'].cpu().double() - theirs.state[ref[i]]['momentum_buffer']).abs().reshape(-1)
            worst = max(worst, float((dp / ep[i]).max()), float((db / eb[i]).max()))
            assert bool((dp <= ep[i]).all()) and bool((db <= eb[i]).all()), (step, i, float((dp / ep[i]).max()), float((db / eb[i]).max()))
            assert dev[i].grad.data_ptr() == addr[i]
            assert torch.equal(dev[i].grad.cpu(), torch.zeros_like(g) if zero else g), (step, i)
    print('nesterov %s: worst error / allowance over five steps %.3f' % (nesterov, worst))
    assert uploads == [1, 2, 3, 3, 3]                    # first step, flag cleared, lr change; then one launch and no copy
    guarded.unchanged(dev[NO_GRAD], keep, 'the parameter without a gradient')
    assert 'momentum_buffer' not in ours.state.get(dev[NO_GRAD], {}) and ours.counters() == (5, 0)
    # the state loads into torch.optim.SGD, and one more step from there agrees under the one-step bound
    start = [p.detach().cpu().double() for p in dev]
    ref = [torch.nn.Parameter(t.clone()) for t in start]
    theirs = torch.optim.SGD(groups(ref), lr=1.0)
    theirs.load_state_dict(ours.state_dict())
    assert theirs.param_groups[0]['lr'] == sc.f32(0.001) and theirs.param_groups[0]['nesterov'] == nesterov
    grads = _class_grads(9)
    for i, g in enumerate(grads):
        if g is not None:
            dev[i].grad.copy_(g)
            ref[i].grad = g.double()
    bufs = [None if g is None else ours.state[dev[i]]['momentum_buffer'].cpu().double() for i, g in enumerate(grads)]
    ours.step()
    theirs.step()
    for k, group in enumerate(theirs.param_groups):
        h = dict(lr=group['lr'], momentum=group['momentum'], weight_decay=group['weight_decay'], dampening=0.0, nesterov=nesterov,
                 maximize=False)
        for i in (2 * k, 2 * k + 1):
            if grads[i] is None:
                continue
            bp, bb = sc.bound(start[i].reshape(-1), grads[i].reshape(-1), bufs[i].reshape(-1), h, first=False)
            assert bool(((dev[i].detach().cpu().double() - ref[i].detach()).abs().reshape(-1) <= bp).all()), i
            assert bool(((ours.state[dev[i]]['momentum_buffer'].cpu().double()
                          - theirs.state[ref[i]]['momentum_buffer']).abs().reshape(-1) <= bb).all()), i
    assert ours.uploads == 3 and ours.counters() == (6, 0)
