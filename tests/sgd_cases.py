"""Lists, operands, float64 reference, error bound and mutations of the fused SGD step's tests (csrc/sgd.hip, usot_amd/optim.py).
Plain helper module: no fixtures, no device.  tests/test_sgd_lists.py pins what is here.

The arithmetic (include/usot_hip.h):
    g' = maximize ? -g : g;  d = g' + wd * p;  buf' = first ? d : mu * buf + c * d  (mu != 0; c = 1 - dampening)
    step = mu == 0 ? d : nesterov ? d + mu * buf' : buf';  p' = p - lr * step

EXACT family: p, g and buf are multiples of 1/4 in [-2, 2] and every hyper-parameter is a power of two, so over three steps every
intermediate is a dyadic number of few bits and float32, fused or not, computes what float64 computes: the comparison is equality
(ref_step(exact=True) asserts the representability of every intermediate).

ROUNDING family: the reference's hyper-parameters.  Per element, with u = 2^-24:
    D = |g| + wd |p|;  S_b = first ? D : mu |buf| + c D;  S = S_b, or D + mu S_b with nesterov (D when mu == 0)
    |p' - ref| <= 8 u (|p| + lr S),   |buf' - ref| <= 8 u S_b
At most five roundings lie between the operands and p' (wd*p + g, c*d, mu*buf + ., d + mu*buf', p - lr*step), each of at most u
times the magnitude of the terms entering it, fused or not; 8 leaves room for the way they compound."""
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
BOUND = 8.0
f32 = lambda v: float(np.float32(v))

EXACT = dict(lr=2.0 ** -3, momentum=2.0 ** -1, weight_decay=2.0 ** -2)
REFERENCE = dict(lr=f32(0.005), momentum=f32(0.9), weight_decay=f32(1e-4))
# (dampening, nesterov, maximize): every combination torch.optim.SGD accepts
FLAGS = [(damp, nest, maxi) for damp in (0.0, 0.5) for nest in (False, True) for maxi in (False, True) if not (nest and damp)]
STEPS = 3
SMALL = list(range(1, 68))
SWEEP_STEP = 129                                     # odd: 1, 130, 259, ... visits every residue mod 4
OFFSETS = list(itertools.product(range(4), repeat=3))      # floats in front of p, g and buf, independently
MIX = (0, 1, 3, 4, 64, 'big')                        # 'big' = 5 * chunk + 1
MIX_TENSORS = 300
COUNT_N = ('0', '1', 'chunk-1', 'chunk', 'chunk+1', '3*chunk+5')
RAGGED = 37                                          # chunks beyond the grid cap in the second over-cap table
MUTATIONS = ['no_weight_decay', 'first_ignored', 'nesterov_old_buf', 'dampening_ignored', 'maximize_ignored', 'lr_on_d']
# (loss, is it valid) - the reference's is_valid_number on the fp32 value the device reads
GUARD_LOSSES = [(float('nan'), False), (float('inf'), False), (float('-inf'), False),
                (float(np.nextafter(np.float32(1e4), np.float32(np.inf))), False), (1e4, True), (0.5, True), (-1e30, True)]


def hyp(dampening=0.0, nesterov=False, maximize=False, **kw):
    h = dict(EXACT, dampening=dampening, nesterov=nesterov, maximize=maximize)
    h.update(kw)
    return h


def grad_scale(h):
    """1 - dampening, formed in double and rounded to fp32 once"""
    return f32(1.0 - h['dampening'])


def flags_of(h, first):
    return (1 if first and h['momentum'] != 0 else 0) | (2 if h['nesterov'] else 0) | (4 if h['maximize'] else 0)


def sweep_sizes(chunk):
    edge = [chunk - 1, chunk, chunk + 1] + list(range(2 * chunk - 1, 2 * chunk + 6))
    return sorted(set(SMALL + list(range(1, 2 * chunk + 6, SWEEP_STEP)) + edge))


def offset_sizes(chunk):
    return [1, 3, 4, 7, 67, chunk + 5]


def count_sizes(chunk):
    return [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]


def mix_sizes(chunk):
    return [5 * chunk + 1 if MIX[i % len(MIX)] == 'big' else MIX[i % len(MIX)] for i in range(MIX_TENSORS)]


def mix_hyp(i):
    """a different lr, weight decay and momentum per tensor, all powers of two (or 0): the six sizes of one round of MIX share a
    triple, and the 50 rounds walk through the 18 triples"""
    r = i // len(MIX)
    mu = (0.5, 0.25, 0.0)[(r // 6) % 3]
    nest = mu == 0.5 and i % 7 == 3                  # with momentum 1/4 the third step of the finest triple needs 25 bits
    return dict(lr=2.0 ** -(1 + r % 3), weight_decay=2.0 ** -(1 + (r // 3) % 2), momentum=mu,
                dampening=0.5 if (i % 4 == 1 and not nest) else 0.0, nesterov=nest, maximize=i % 11 == 5)


def over_cap_sizes(chunk, cap, extra):
    """element counts whose chunks number cap + extra: one long tensor, then `extra + 9` tensors of one (short) chunk each"""
    return [(cap - 9) * chunk] + [1 + (7 * i) % chunk for i in range(extra + 9)]


def n_chunks(sizes, chunk):
    return sum(-(-n // chunk) for n in sizes)


def exact_operand(n, seed):
    """multiples of 1/4 in [-2, 2], float32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n,), generator=g).float() / 4


def rounding_operands(n, seed):
    """p ~ N(0, 1), buf ~ 0.1 N(0, 1), g ~ N(0, 1) * 10^U(-4, 1): five decades"""
    g = torch.Generator().manual_seed(seed)
    p, buf = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 10.0 ** (5 * torch.rand(n, generator=g) - 4)
    return p, grad, buf


def _exact(*ts):
    for t in ts:
        assert torch.equal(t.float().double(), t), 'an intermediate is not a float32 number'


def ref_step(p, g, buf, h, first, exact=False, mutation=None):
    """float64 (p', buf') of one step; buf and buf' are None when momentum == 0.  exact: assert that every intermediate is a
    float32 number.  mutation: one of MUTATIONS - a subtly wrong step."""
    lr, mu, wd, c = h['lr'], h['momentum'], h['weight_decay'], grad_scale(h)
    if mutation == 'dampening_ignored':
        c = 1.0
    p, g = p.double(), g.double()
    gp = -g if h['maximize'] and mutation != 'maximize_ignored' else g
    wp = wd * p if mutation != 'no_weight_decay' else 0 * p
    d = gp + wp
    inter = [wp, d]
    if mu != 0:
        if first and mutation != 'first_ignored':
            nb = d.clone()
        else:
            old = buf.double() if buf is not None else torch.zeros_like(d)
            nb = mu * old + c * d
            inter += [mu * old, c * d, nb]
        if h['nesterov']:
            step = d + mu * (nb if mutation != 'nesterov_old_buf' else (buf.double() if buf is not None and not first else 0 * d))
            inter += [mu * nb, step]
        else:
            step = nb
    else:
        nb, step = None, d
    if mutation == 'lr_on_d':
        step = d
    p2 = p - lr * step
    inter += [lr * step, p2]
    if exact:
        _exact(*inter)
    return p2, nb


def bound(p, g, buf, h, first):
    """(bound on |p' - ref|, bound on |buf' - ref|) per element, float64; the second is None when momentum == 0"""
    sp, sb = spread(p.double().abs(), g.double().abs(), None if buf is None else buf.double().abs(), h, first)
    return BOUND * U * sp, None if sb is None else BOUND * U * sb


def spread(ap, ag, ab, h, first):
    """(|p| + lr S, S_b) of the module docstring on magnitudes ap, ag, ab.  With ag = 0 and the operands' errors for ap and ab it is
    also how far one step carries those errors: the step is linear in p and buf."""
    lr, mu, wd, c = h['lr'], h['momentum'], h['weight_decay'], abs(grad_scale(h))
    D = ag + wd * ap
    if mu == 0:
        return ap + lr * D, None
    Sb = D if first else mu * (ab if ab is not None else 0 * D) + c * D
    S = D + mu * Sb if h['nesterov'] else Sb
    return ap + lr * S, Sb


def is_valid_number(x):
    """the reference's lib/utils/train_utils.py:8-9, restated"""
    return not (math.isnan(x) or math.isinf(x) or x > 1e4)
