"""CPU: the lists of tests/sgd_cases.py are the ones the fused SGD step's tests were specified with, its exact operands stay float32
numbers through three steps under every flag combination, its float64 reference can tell a subtly wrong step from a right one,
and its error bound holds for PyTorch-CPU float32 with room to spare - the cap that keeps a later edit from thinning
tests/test_gpu_sgd.py into something a wrong kernel would pass.  The chunk size and the grid cap are host queries of the library."""
import math

import pytest
import torch

import sgd_cases as sc
from usot_amd import build, hip


@pytest.fixture(scope='module', autouse=True)
def library():
    build.build(force=False)


def test_the_lists_are_the_specified_ones():
    chunk, cap = hip.sgd_chunk_elems(), hip.sgd_grid_cap()
    assert chunk % 4 == 0 and chunk >= 256 and 1024 <= cap <= 4096
    assert sc.EXACT == dict(lr=0.125, momentum=0.5, weight_decay=0.25)
    assert sc.REFERENCE == dict(lr=sc.f32(0.005), momentum=sc.f32(0.9), weight_decay=sc.f32(1e-4))
    assert sc.FLAGS == [(0.0, False, False), (0.0, False, True), (0.0, True, False), (0.0, True, True), (0.5, False, False),
                        (0.5, False, True)]
    assert sc.STEPS == 3 and sc.BOUND == 8.0 and sc.U == 2.0 ** -24
    sizes = sc.sweep_sizes(chunk)
    assert set(range(1, 68)) <= set(sizes) and sizes[-1] == 2 * chunk + 5 and sizes[0] == 1
    for several in (0, 1, 2):                            # every residue mod 4 inside one, two and three chunks
        assert {n % 4 for n in sizes if several * chunk < n <= (several + 1) * chunk} == {0, 1, 2, 3}, several
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1} <= set(sizes)
    assert max(b - a for a, b in zip(sizes, sizes[1:])) <= sc.SWEEP_STEP
    assert len(sc.OFFSETS) == 64 and set(sc.OFFSETS) == {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
    assert sc.offset_sizes(chunk) == [1, 3, 4, 7, 67, chunk + 5]
    assert sc.count_sizes(chunk) == [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    mix = sc.mix_sizes(chunk)
    assert len(mix) == 300 and set(mix) == {0, 1, 3, 4, 64, 5 * chunk + 1} and mix.count(0) == 50
    hyps = [sc.mix_hyp(i) for i in range(300)]
    assert len({(h['lr'], h['weight_decay'], h['momentum']) for h in hyps}) == 18
    assert any(h['momentum'] == 0 for h in hyps) and any(h['nesterov'] for h in hyps) and any(h['maximize'] for h in hyps)
    assert any(h['dampening'] for h in hyps) and not any(h['nesterov'] and (h['dampening'] or not h['momentum']) for h in hyps)
    for extra in (1, sc.RAGGED):
        over = sc.over_cap_sizes(chunk, cap, extra)
        assert sc.n_chunks(over, chunk) == cap + extra and len(over) == extra + 10
    assert sc.RAGGED % 2 == 1 and 1 < sc.RAGGED < cap
    assert [v for _, v in sc.GUARD_LOSSES] == [False, False, False, False, True, True, True]
    assert sc.MUTATIONS == ['no_weight_decay', 'first_ignored', 'nesterov_old_buf', 'dampening_ignored', 'maximize_ignored', 'lr_on_d']


def test_guard_losses_are_judged_by_the_definition():
    for loss, valid in sc.GUARD_LOSSES:
        as_f32 = float(torch.tensor(loss, dtype=torch.float32))
        assert sc.is_valid_number(as_f32) == valid, loss
    nxt = sc.GUARD_LOSSES[3][0]
    assert nxt > 1e4 and float(torch.tensor(nxt, dtype=torch.float32)) == nxt and nxt - 1e4 < 1e-3
    assert math.isinf(float(torch.tensor(1e39, dtype=torch.float32)))


def _three_steps(h, n=4099, mutation=None, exact=True):
    p, buf = sc.exact_operand(n, 1).double(), None
    for s in range(sc.STEPS):
        g = sc.exact_operand(n, 10 + s)
        p, buf = sc.ref_step(p, g, buf, h, first=s == 0, exact=exact, mutation=mutation)
    return p, buf


@pytest.mark.parametrize('flags', sc.FLAGS, ids=str)
def test_exact_operands_stay_float32_numbers(flags):
    """ref_step(exact=True) asserts it for every intermediate of every step; also from a given buffer, and without momentum"""
    h = sc.hyp(*flags)
    _three_steps(h)
    p, g, buf = sc.exact_operand(999, 3), sc.exact_operand(999, 4), sc.exact_operand(999, 5)
    assert float(p.abs().max()) == 2.0 and set((p * 4).tolist()) == set(range(-8, 9))
    for s in range(sc.STEPS):
        p, buf = sc.ref_step(p, g, buf, h, first=False, exact=True)
    _three_steps(sc.hyp(0.0, False, flags[2], momentum=0.0))
    for i in range(300):
        q, b = sc.exact_operand(64, i).double(), None
        for s in range(sc.STEPS):
            q, b = sc.ref_step(q, sc.exact_operand(64, 1000 + i + s), b, sc.mix_hyp(i), first=s == 0, exact=True)


@pytest.mark.parametrize('mut', sc.MUTATIONS)
def test_reference_tells_a_wrong_step(mut):
    """each mutation changes the parameters after three steps under the flags it concerns, and only there"""
    hit = 0
    for flags in sc.FLAGS:
        h = sc.hyp(*flags)
        true, _ = _three_steps(h)
        wrong, _ = _three_steps(h, mutation=mut, exact=False)
        concerned = {'first_ignored': flags[0] != 0, 'nesterov_old_buf': flags[1], 'dampening_ignored': flags[0] != 0, 'maximize_ignored': flags[2]}.get(mut, True)
        assert torch.equal(true, wrong) == (not concerned), (mut, flags)
        hit += concerned
    assert hit >= 2


def test_bound_holds_for_float32_on_the_cpu_with_room():
    """PyTorch-CPU float32 against float64 on the rounding family: the worst ratio error / bound stays below 1 (0.33 measured)"""
    n = 1 << 20
    p, g, buf = sc.rounding_operands(n, 7)
    assert 1e-5 < float(g.abs().median()) < 1.0 and float(g.abs().max()) > 10 and float((g.abs() < 1e-3).float().mean()) > 0.1
    for nest in (False, True):
        h = dict(sc.REFERENCE, dampening=0.0, nesterov=nest, maximize=False)
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        opt = torch.optim.SGD([q], **h)
        opt.state[q]['momentum_buffer'] = buf.clone()
        opt.step()
        rp, rb = sc.ref_step(p, g, buf, h, first=False)
        bp, bb = sc.bound(p, g, buf, h, first=False)
        ratio = max(float(((q.detach().double() - rp).abs() / bp).max()), float(((opt.state[q]['momentum_buffer'].double() - rb).abs() / bb).max()))
        print('nesterov %s: float32 CPU at %.3f of the bound' % (nest, ratio))
        assert 0.05 < ratio < 1.0
