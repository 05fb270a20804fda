"""Shared by test_batchnorm_host.py and test_gpu_batchnorm.py: the map shapes of the batch-norm tests, their seeded operands, and
the float64 reference - F.batch_norm in float64 on the CPU, differentiated by torch autograd, with the ReLU mask handed in (a
float64 mask and a float32 mask differ on elements within rounding of zero, and one flipped element is an O(1) error of dx).
References of the forward pass are computed once per (case, family, mode) and never modified.  Plain helper module."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1

# (N, H, W, C)
CASES = [
    (1, 1, 3, 4),            # M = 3: one partial row step, one lane of sixteen
    (1, 3, 5, 36),           # nine lanes: a channel block with a tail
    (3, 7, 9, 64),           # one whole channel block, M = 189: three steps, the last partial
    (1, 5, 5, 256),          # the template side of the head at batch 1
    (2, 25, 25, 256),        # the tower maps
    (4, 29, 29, 256),        # the search-side encoder maps
    (2, 31, 31, 1024),       # the neck's input width: sixteen channel blocks, 2 M floats
]
FAMILIES = (0, 2, 32)        # offset of the channel means in units of the channel's spread; 32 is the ill-conditioned one


def case_id(c):
    return 'n%d_%dx%d_c%d' % c


def operands(c, off=0, seed=0):
    """float32 CPU tensors of one case and family: x NHWC, gamma, beta, running_mean, running_var, dy NHWC"""
    n, h, w, ch = c
    g = torch.Generator().manual_seed(7919 * (n * 1000003 + h * 10007 + w * 101 + ch) % (2 ** 31) + 31 * off + seed)
    s = 0.5 + torch.rand(ch, generator=g)
    sign = torch.randint(0, 2, (ch,), generator=g).float() * 2 - 1
    x = torch.randn(n, h, w, ch, generator=g) * s + off * s * sign
    gamma = (0.5 + torch.rand(ch, generator=g)) * (torch.randint(0, 2, (ch,), generator=g).float() * 2 - 1)
    beta = 0.3 * torch.randn(ch, generator=g)
    rmean = x.reshape(-1, ch).double().mean(0).float() + 0.1 * s * torch.randn(ch, generator=g)
    rvar = 0.5 + torch.rand(ch, generator=g)
    dy = torch.randn(n, h, w, ch, generator=g)
    return x, gamma, beta, rmean, rvar, dy


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_err(got, ref):
    """the project's scaled error, max |got - ref| / max(|ref|, mean|ref|); NaN (an unwritten element) fails every bar"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.maximum(np.abs(ref), np.abs(ref).mean() + 1e-30)
    return float(np.max(np.abs(got - ref) / scale))


def forward_of(x, gamma, beta, rmean, rvar, training, dtype=torch.float64):
    """F.batch_norm in `dtype` on the CPU -> dict of NHWC / [C] tensors: pre (the output before any ReLU), save_mean,
    save_invstd, and the running statistics after the call (unchanged in eval).  `leaves`: the differentiable inputs."""
    x_, g_, b_ = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rmean.detach().to(dtype).clone(), rvar.detach().to(dtype).clone()
    pre = F.batch_norm(nchw(x_), rm, rv, g_, b_, training, MOMENTUM, EPS).permute(0, 2, 3, 1)
    flat = x_.detach().reshape(-1, x.shape[-1])
    mean = flat.mean(0) if training else rm
    var = flat.var(0, unbiased=False) if training else rv
    return dict(pre=pre, leaves=(x_, g_, b_), save_mean=mean, save_invstd=(var + EPS).rsqrt(), running_mean=rm, running_var=rv)


def grads_of(fw, dy, mask=None):
    """(dx NHWC, dgamma, dbeta) of sum(dy * y), y = pre * mask (mask None: no ReLU), by autograd through forward_of's graph"""
    pre = fw['pre']
    y = pre if mask is None else pre * mask.to(pre.dtype)
    return torch.autograd.grad(y, fw['leaves'], dy.to(pre.dtype), retain_graph=True)


@functools.lru_cache(maxsize=None)
def reference(c, off, training, seed=0):
    """(operands, float64 forward) of a case; shared between tests, read-only"""
    ops = operands(c, off, seed)
    return ops, forward_of(*ops[:5], training)


def mask_violations(y_dev, pre64):
    """elements whose device mask (y > 0) is wrong although the float64 pre-activation is not within rounding of zero:
    |pre| > 1e-4 * mean|pre|.  A condition, not a tolerance: float32 implementations flip elements with |pre| <= 1.5e-6 only."""
    pre = pre64.detach()
    wrong = (y_dev.detach().cpu() > 0) != (pre > 0)
    return int((wrong & (pre.abs() > 1e-4 * pre.abs().mean())).sum())
