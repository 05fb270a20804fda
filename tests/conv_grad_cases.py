"""Shared by test_conv_grad_host.py and test_gpu_conv_grad.py: the convolution geometries of the gradient tests, their seeded
inputs, and the float64 torch-autograd reference (computed once per case, never modified).  Plain helper module."""
import functools
import math

import torch
import torch.nn.functional as F

# (N, H, W, Cin, Cout, k, stride, pad, dil)
RAW = [
    (1, 7, 7, 32, 32, 3, 1, (0, 0), (1, 1)),         # M = 25: a single partial pixel chunk; the template-side encoder's map
    (2, 9, 8, 32, 40, 3, 1, (1, 1), (1, 1)),         # Cout residue (2 1/2 MFMA blocks), padded taps, a chunk straddling two images
    (1, 13, 12, 64, 64, 3, 1, (0, 0), (2, 1)),       # asymmetric dilations; route A with pad' (4, 2)
    (1, 13, 12, 64, 64, 3, 1, (0, 0), (1, 2)),       # ... and (2, 4)
    (1, 13, 13, 64, 64, 3, 1, (2, 2), (2, 2)),       # layer3's geometry
    (2, 25, 25, 256, 4, 3, 1, (1, 1), (1, 1)),       # the prediction heads: thin Cout, route B
    (2, 25, 25, 256, 1, 3, 1, (1, 1), (1, 1)),
    (1, 5, 5, 1024, 256, 1, 1, (0, 0), (1, 1)),      # the neck: 32 k-blocks, 25 pixels
    (2, 15, 15, 32, 64, 3, 2, (0, 0), (1, 1)),       # stride in the weight-gradient loader; route B gather parity
    (3, 25, 25, 256, 256, 3, 1, (1, 1), (1, 1)),     # one tower conv at batch 3 (M = 1875)
    (1, 31, 31, 256, 256, 3, 1, (0, 0), (2, 1)),     # one search-side encoder
]
TOWER = RAW[9]
ENCODER = RAW[10]


def case_id(c):
    n, h, w, cin, cout, k, s, pad, dil = c
    return 'n%d_%dx%d_%dto%d_k%d_s%d_p%d%d_d%d%d' % (n, h, w, cin, cout, k, s, pad[0], pad[1], dil[0], dil[1])


def out_hw(c):
    n, h, w, cin, cout, k, s, pad, dil = c
    return (h + 2 * pad[0] - dil[0] * (k - 1) - 1) // s + 1, (w + 2 * pad[1] - dil[1] * (k - 1) - 1) // s + 1


def route_a(c):
    """stride 1, whole 32-channel blocks of dy, pad' = dil*(k-1) - pad >= 0.  Also takes the ten-field cases of
    conv_grad_sweep_cases.py, (.., KH, KW, stride, pad, dil): rectangular filters."""
    n, h, w, cin, cout, kh = c[:6]
    kw, (s, pad, dil) = (kh if len(c) == 9 else c[6]), c[-3:]
    return s == 1 and cout % 32 == 0 and dil[0] * (kh - 1) >= pad[0] and dil[1] * (kw - 1) >= pad[1]


ROUTE_A = [c for c in RAW if route_a(c)]
ROUTE_B_ONLY = [c for c in RAW if not route_a(c)]


def inputs(c, seed=0):
    """float32 CPU tensors: x NCHW, weight OIHW scaled by 1/sqrt(K), bias, dy NCHW"""
    n, h, w, cin, cout, k, s, pad, dil = c
    g = torch.Generator().manual_seed(1000 * RAW.index(c) + 17 + seed if c in RAW else 99991 + seed + h * 131 + w)
    oh, ow = out_hw(c)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(k * k * cin)
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, oh, ow, generator=g)
    return x, wt, b, dy


def ref_grads_of(x, wt, b, dy, stride, pad, dil):
    """float64, CPU, torch autograd through F.conv2d: (dx NCHW, dw OIHW, db)"""
    x64, w64, b64 = (t.detach().double().clone().requires_grad_(True) for t in (x, wt, b))
    y = F.conv2d(x64, w64, b64, stride=stride, padding=pad, dilation=dil)
    return torch.autograd.grad(y, (x64, w64, b64), dy.double())


@functools.lru_cache(maxsize=None)
def reference(c, seed=0):
    """(inputs, float64 gradients) of a case; shared between tests, read-only"""
    ins = inputs(c, seed)
    return ins, ref_grads_of(*ins, c[6], c[7], c[8])


def rotated_oihw(wt):
    """OIHW weight -> the OIHW weight of the convolution that IS the data gradient at stride 1: rotated by 180 degrees, in / out swapped"""
    return wt.flip(2, 3).transpose(0, 1).contiguous()


def pack(wt):
    """OIHW -> packed bank [Cout][KH*KW*Cin], k = (kh*KW + kw)*Cin + ci"""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


def unpack(wp, cin, k):
    return wp.reshape(wp.shape[0], k, k, cin).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()
