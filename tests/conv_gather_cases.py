"""Shared by test_conv_gather_lists.py and test_gpu_conv_gather.py: WHAT ENTERS THE SUM of a convolution - the geometries of the
im2col gather (stride, pad_h / pad_w, dil_h / dil_w, KH / KW, H / W, image borders), the problems of the k-tile walk and of the
split-K distribution, their seeded INTEGER operands and the float64 reference (computed once per problem, never modified).

Every operand is integer-valued (x -4 .. 4, w -2 .. 2, bias / res -8 .. 8, dy -2 .. 2) and the largest reduction is K = 1 728:
every partial sum of every summation order is an integer below 2^24, so any correct fp32 kernel gives the float64 result bit for
bit.  The bar of the GPU tests is therefore EQUALITY (one storage ulp for 16-bit outputs), not a tolerance.  The split-fp16 tiles
are held to the same equality: 8 x <= 32 and w 2^e lands on multiples of 256 below 1 024, so the hi halves carry the values exactly
and the lo halves are zero (asserted by the list test).  Plain helper module."""
import functools
import re
import zlib

import torch
import torch.nn.functional as F

X_MAX, W_MAX, B_MAX, R_MAX, DY_MAX = 4, 2, 8, 8, 2
EXACT = 1 << 24
CIN, COUT = 64, 32

# (N, H, W, KH, KW, stride, (pad_h, pad_w), (dil_h, dil_w)); rows are numbered from 1 in the comments and the reports
GEOMS = [
    (1, 5, 9, 1, 3, 1, (0, 1), (1, 1)), (1, 9, 5, 3, 1, 1, (1, 0), (1, 1)), (2, 6, 7, 2, 2, 1, (0, 0), (1, 1)), (1, 6, 7, 2, 2, 2, (1, 1), (1, 1)),
    (1, 9, 8, 5, 5, 1, (2, 2), (1, 1)), (2, 7, 9, 3, 5, 1, (0, 2), (1, 1)), (1, 7, 7, 7, 7, 1, (0, 0), (1, 1)), (1, 4, 4, 7, 7, 1, (3, 3), (1, 1)),
    (2, 7, 6, 3, 3, 1, (0, 2), (1, 1)), (2, 6, 7, 3, 3, 1, (2, 0), (1, 1)), (1, 5, 6, 3, 3, 1, (3, 3), (1, 1)),
    (2, 8, 10, 3, 3, 2, (1, 1), (1, 1)), (2, 9, 7, 3, 3, 2, (1, 1), (1, 1)), (3, 8, 9, 1, 1, 2, (0, 0), (1, 1)), (1, 10, 11, 3, 3, 3, (1, 0), (1, 1)),
    (1, 9, 9, 1, 1, 3, (1, 1), (1, 1)),
    (1, 9, 10, 3, 3, 1, (3, 3), (3, 3)), (1, 11, 9, 3, 3, 1, (0, 0), (3, 1)), (2, 9, 11, 3, 3, 2, (2, 2), (2, 2)), (1, 7, 8, 3, 3, 2, (1, 2), (1, 2)),
    (1, 3, 3, 3, 3, 1, (4, 4), (4, 4)),
    (3, 5, 7, 3, 3, 1, (1, 1), (1, 1)), (1, 3, 9, 3, 3, 1, (0, 1), (1, 1)), (1, 9, 3, 3, 3, 1, (1, 0), (1, 1)), (2, 2, 2, 3, 3, 1, (1, 1), (1, 1)),
    (1, 1, 1, 1, 1, 1, (0, 0), (1, 1)), (4, 1, 1, 3, 3, 1, (1, 1), (1, 1)),
]
BATCH_ROWS = [(5, 1), (12, 2), (17, 1), (19, 3)]         # G2: (row number, ksplit) of the four problems of one batched launch
ROUTE_A_CLOSED = [4, 11, 12, 13, 14, 15, 16, 19, 20]     # G4: rows 11 and 16 (pad beyond the kernel's reach) and every strided row
ONLY_CENTRE_TAP = [21, 27]                               # rows whose eight outer taps never land inside the image: dilation and
                                                         # padding 4 on a 3 x 3 image, and 3x3 / pad 1 on one-pixel images
LP_BK = 64                                               # csrc/conv_bf16.hip: BKB

K1_J = list(range(1, 13))                                # k-tile counts 1 .. 12: one tile up to past the deepest ring (five stages)
K2_CCH = [1, 3]                                          # 3x3 at Cin = bk and 3 bk: 9 and 27 k-tiles, cch = 3 wraps on a non-power of two
S1_KSPLIT = [2, 4, 5, 7, 13, 26, 27]                     # KT = 27: slices of 13 / 14 down to one k-tile, mid-tap and odd starts
S1_REJECTED = 28                                         # K / bk + 1
S2_KSPLIT = [2, 3, 4, 5]                                 # KT = 5
S2_J = 5
WGRAD_PSPLIT = [1, 0, 3]                                 # 3 where M >= 6


def row_of(number):
    return GEOMS[number - 1]


def row_id(g):
    return 'row%d' % (GEOMS.index(g) + 1) if g in GEOMS else 'n%d_%dx%d_k%dx%d_s%d_p%d%d_d%d%d' % (g[:6] + g[6] + g[7])


def out_hw(g):
    n, h, w, kh, kw, s, pad, dil = g
    return (h + 2 * pad[0] - dil[0] * (kh - 1) - 1) // s + 1, (w + 2 * pad[1] - dil[1] * (kw - 1) - 1) // s + 1


def pixels(g):
    oh, ow = out_hw(g)
    return g[0] * oh * ow


def valid(g):
    n, h, w, kh, kw, s, pad, dil = g
    oh, ow = out_hw(g)
    return min(n, h, w, kh, kw, s, dil[0], dil[1], oh, ow) >= 1 and min(pad) >= 0


def route_a_open(g, cout=COUT):
    """usot_hip.h: stride 1, whole 32-channel blocks of dy, pad <= dil (K - 1) in both directions"""
    n, h, w, kh, kw, s, pad, dil = g
    return s == 1 and cout % 32 == 0 and dil[0] * (kh - 1) >= pad[0] and dil[1] * (kw - 1) >= pad[1]


def pw_geom(m):
    """K1 / S2: 1x1 on x [1, 1, m, Cin]"""
    return (1, 1, m, 1, 1, 1, (0, 0), (1, 1))


def k3_geom(m):
    """K2 / S1: 3x3, pad (0, 1), on x [1, 3, m, Cin]: OH = 1, OW = m, all three filter rows real data"""
    return (1, 3, m, 3, 3, 1, (0, 1), (1, 1))


def tile_bk(name):
    """k-tile of an fp32 conv tile from usot_conv_tile_name: `BK=<n>`; the in-workgroup k-split rows spell their template
    arguments `<bm,bn,bk,ksw> ksw=<n>`; the first generation (no BK) walks 32 channels a step"""
    m = re.search(r'BK=(\d+)', name) or re.search(r'<\d+,\d+,(\d+),\d+> ksw=', name)
    return int(m.group(1)) if m else 32


def k_problems(bk):
    """K1 and K2 of a tile with k-tile bk: (geometry, Cin, Cout, k-tiles)"""
    return [(pw_geom(17), j * bk, COUT, j) for j in K1_J] + [(k3_geom(17), c * bk, COUT, 9 * c) for c in K2_CCH]


def k3_problems():
    """K3 (usot_conv2d_lp): the shapes of K1 at Cin = 64 j, and of K2 at Cin = 64 and 192"""
    return k_problems(LP_BK)


def s_corners(bm):
    """(M, Cout): scalar stores at a ragged corner, and one pixel past the tile"""
    return [(17, 33), (bm + 1, 32)]


def s_problems(bm, bk):
    """S1 and S2 of a tile: (part, geometry, Cin, Cout, KT, ksplit list)"""
    out = []
    for m, co in s_corners(bm):
        out.append(('S1', k3_geom(m), 3 * bk, co, 27, S1_KSPLIT))
        out.append(('S2', pw_geom(m), S2_J * bk, co, S2_J, S2_KSPLIT))
    return out


def slices(kt, ksplit):
    """the launcher's cut: slice ks walks k-tiles [kt ks / ksplit, kt (ks + 1) / ksplit)"""
    return [(kt * ks // ksplit, kt * (ks + 1) // ksplit) for ks in range(ksplit)]


def _randint(g, shape, amax):
    return torch.randint(-amax, amax + 1, shape, generator=g).float()


def operands(g, cin=CIN, cout=COUT):
    """seeded float32 CPU tensors, every value an integer: x NCHW, w OIHW, bias, res NCHW (the output's shape), dy NCHW"""
    n, h, w, kh, kw, s, pad, dil = g
    oh, ow = out_hw(g)
    gen = torch.Generator().manual_seed(zlib.crc32(repr((g, cin, cout)).encode()))
    return (_randint(gen, (n, cin, h, w), X_MAX), _randint(gen, (cout, cin, kh, kw), W_MAX), _randint(gen, (cout,), B_MAX),
            _randint(gen, (n, cout, oh, ow), R_MAX), _randint(gen, (n, cout, oh, ow), DY_MAX))


def bound(g, cin=CIN, cout=COUT):
    """sum |x| |w| + |b| + |res| over the longest reduction of the problem (forward, and the gradients' own reductions over
    pixels and over (tap, channel)): everything below EXACT means every fp32 partial sum is an exact integer"""
    n, h, w, kh, kw, s, pad, dil = g
    fwd = kh * kw * cin * X_MAX * W_MAX + B_MAX + R_MAX
    dw = pixels(g) * X_MAX * DY_MAX
    dx = kh * kw * cout * W_MAX * DY_MAX
    return max(fwd, dw, dx)


def conv64(x, w, b, g):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), g[5], g[6], g[7])


def gather64(x, w, b, g, pad, dil):
    """float64 result of a gather that walks the OUTPUT pixels of geometry g but reads its taps with another padding / dilation:
    y[oh][ow] = sum over taps of x[oh s - pad[0] + kh dil[0]][ow s - pad[1] + kw dil[1]] (zero outside the image) - what a kernel
    that swapped two descriptor fields would compute; equals conv64 at g's own pad and dil"""
    oh, ow = out_hw(g)
    far = 32
    xp = F.pad(x.double(), (far, far, far, far))[:, :, far - pad[0]:, far - pad[1]:]
    return F.conv2d(xp, w.double(), b.double(), g[5], 0, dil)[:, :, :oh, :ow]


@functools.lru_cache(maxsize=None)
def problem(g, cin=CIN, cout=COUT):
    """(operands, float64 conv + bias NCHW) of one problem; shared between tests, read-only"""
    ops = operands(g, cin, cout)
    return ops, conv64(ops[0], ops[1], ops[2], g)


@functools.lru_cache(maxsize=None)
def gradients(g, cin=CIN, cout=COUT):
    """float64 autograd through F.conv2d: (dx NCHW, dw OIHW, db); read-only"""
    x, w, b, _, dy = problem(g, cin, cout)[0]
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    return torch.autograd.grad(F.conv2d(x64, w64, b64, g[5], g[6], g[7]), (x64, w64, b64), dy.double())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pack(w):
    """OIHW -> packed bank [Cout][KH*KW*Cin], k = (kh*KW + kw)*Cin + ci"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def storage_ulp(ref, dtype):
    """one unit in the last place of the 16-bit storage type at |ref| (float64 tensor): 8 significant bits bf16, 11 fp16"""
    bits = 8 if dtype == torch.bfloat16 else 11
    mag = ref.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(mag)) - (bits - 1))


def within_one_ulp(got, ref, dtype):
    """16-bit outputs: every rounding of the exact integer lies within one storage ulp of it; an exact 0 stays 0"""
    return (got.double() - ref).abs() <= torch.where(ref == 0, torch.zeros_like(ref), storage_ulp(ref, dtype))


def tap_lands(g, kh, kw):
    """whether tap (kh, kw) reads a pixel of the image for at least one output pixel"""
    n, h, w, KH, KW, s, pad, dil = g
    oh, ow = out_hw(g)
    rows = any(0 <= o * s - pad[0] + kh * dil[0] < h for o in range(oh))
    cols = any(0 <= o * s - pad[1] + kw * dil[1] < w for o in range(ow))
    return rows and cols


def padding_only_pixels(g):
    """output pixels (per image) none of whose taps lands inside the image: they must equal the bias"""
    n, h, w, KH, KW, s, pad, dil = g
    oh, ow = out_hw(g)
    live_r = [any(0 <= o * s - pad[0] + k * dil[0] < h for k in range(KH)) for o in range(oh)]
    live_c = [any(0 <= o * s - pad[1] + k * dil[1] < w for k in range(KW)) for o in range(ow)]
    return oh * ow - sum(live_r) * sum(live_c)
