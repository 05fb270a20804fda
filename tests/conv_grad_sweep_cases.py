"""Shared by test_conv_grad_sweep_lists.py and test_gpu_conv_grad_sweep.py: the lists of the convolution-gradient sweep (csrc/conv_grad.hip),
their seeded integer operands, an int64 reference written from the three formulas of that file's header, and the mutations - plausible
wrong kernels as wrong references.  Plain helper module: no fixtures, no pytest hooks.

A case is (N, H, W, Cin, Cout, KH, KW, stride, (ph, pw), (dh, dw)).  Layouts are the kernels': x NHWC, dy dense NHWC, the packed bank
w[Cout][KH*KW*Cin] with k = (kh*KW + kw)*Cin + ci.

Operands are integers small enough that every partial sum, in any order, is an integer below 2^24 (bound(), asserted by the lists test):
float32 arithmetic is then exact whatever the order of summation, and every comparison of the sweep is an equality.
  small  x, w, dy in [-3, 3]
  wide   dy in {-1, 0, 1}, x and w in [-4095, 4095] - thirteen significant bits, which no bf16, fp16 or xf32 operand keeps; on the cases
         with M <= 2048 (weight gradient) and Cout*KH*KW <= 2048 (data gradient)."""
import functools
import os
import re

import numpy as np

import conv_grad_cases as cg
from usot_amd import hip



def _wgrad_geometry():
    """(BCO, BKK, CHUNK) as the library answers; where it is not built, as the source it would be built from states them"""
    try:
        return hip.wgrad_geometry()
    except hip.HipError:
        with open(os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), 'csrc', 'conv_grad.hip')) as f:
            m = re.search(r'constexpr int BCO = (\d+), BKK = (\d+), CHUNK = (\d+);', f.read())
        return tuple(int(v) for v in m.groups())


BCO, BKK, CHUNK = _wgrad_geometry()             # tile of dw (channels x k) and pixels staged per step
DGRAD_CAP, PACK_CAP, THREADS = 16384, 8192, 256   # the launch caps of route B and of the pack (blocks), as conv_grad.hip states them
SEED = 4711
FAMILIES = ('small', 'wide')
WIDE_TERMS = 2048
LIMIT = 1 << 24


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def out_hw(c):
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    return (h + 2 * pad[0] - dil[0] * (kh - 1) - 1) // s + 1, (w + 2 * pad[1] - dil[1] * (kw - 1) - 1) // s + 1


def valid(c):
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    return h + 2 * pad[0] - dil[0] * (kh - 1) - 1 >= 0 and w + 2 * pad[1] - dil[1] * (kw - 1) - 1 >= 0


def pixels(c):
    oh, ow = out_hw(c)
    return c[0] * oh * ow


def config(c):
    return c[5:]


def case_id(c):
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    return 'n%d_%dx%d_%dto%d_k%dx%d_s%d_p%d%d_d%d%d' % (n, h, w, cin, cout, kh, kw, s, pad[0], pad[1], dil[0], dil[1])


route_a = cg.route_a          # extended there to the ten-field cases: what route_a_eligible of conv_grad.hip admits, given a rotated bank


def reached(c):
    """[H][W] bool: the x pixels some (output pixel, tap) reads"""
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    oh, ow = out_hw(c)
    rows, cols = np.zeros(h, bool), np.zeros(w, bool)
    for k in range(kh):
        rows[_reach(oh, h, s, pad[0], k * dil[0])[1]] = True
    for k in range(kw):
        cols[_reach(ow, w, s, pad[1], k * dil[1])[1]] = True
    return rows[:, None] & cols[None, :]


def straddles(c):
    """some staged chunk of pixels holds pixels of two images: an image does not end on a chunk edge"""
    oh, ow = out_hw(c)
    return c[0] > 1 and (oh * ow) % CHUNK != 0


def config_id(cfg):
    kh, kw, s, pad, dil = cfg
    return 'k%dx%d_s%d_p%d%d_d%d%d' % (kh, kw, s, pad[0], pad[1], dil[0], dil[1])


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def applies(c, family, kind):
    """kind 'w': the weight gradient, 'x': the data gradient"""
    if family == 'small':
        return True
    return pixels(c) <= WIDE_TERMS if kind == 'w' else c[4] * c[5] * c[6] <= WIDE_TERMS


def _amp(family, name):
    if family == 'small':
        return 3
    return 1 if name == 'dy' else 4095


def bound(c, family, kind=None):
    """the largest possible |partial sum| of the gradients of `kind` (None: of both, where the family applies) on these operands"""
    if kind is None:
        return max([bound(c, family, k) for k in 'wx' if applies(c, family, k)] or [0])
    terms = pixels(c) if kind == 'w' else c[4] * c[5] * c[6]
    return terms * _amp(family, 'dy') * max(_amp(family, 'x' if kind == 'w' else 'w'), 1)      # max(.., 1): the bias gradient's terms


def _flat(c):
    return [int(v) for part in c for v in (part if isinstance(part, tuple) else (part,))]


@functools.lru_cache(maxsize=None)
def operand(c, family, name):
    """int64, read-only: 'x' [N][H][W][Cin], 'w' [Cout][KH*KW*Cin] or 'dy' [N][OH][OW][Cout]"""
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    oh, ow = out_hw(c)
    shape = {'x': (n, h, w, cin), 'w': (cout, kh * kw * cin), 'dy': (n, oh, ow, cout)}[name]
    rng = np.random.default_rng([SEED, FAMILIES.index(family), ('x', 'w', 'dy').index(name)] + _flat(c))
    a = _amp(family, name)
    v = rng.integers(-a, a + 1, shape, dtype=np.int64)
    v.setflags(write=False)
    return v


def random_bank(c):
    """float32 normal values (arbitrary bit patterns) for the pack, which only moves them"""
    n, h, w, cin, cout, kh, kw, s, pad, dil = c
    return np.random.default_rng([SEED, 9] + _flat(c)).standard_normal((cout, kh * kw * cin), dtype=np.float32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _reach(O, L, s, p, off):
    """formula (1), one axis: output index o reads input index i = o*s - p + off; -> (o, i) where 0 <= i < L"""
    o = np.arange(O)
    i = o * s - p + off
    keep = (i >= 0) & (i < L)
    return o[keep], i[keep]


def _gather(L, O, s, p, off, floor=False):
    """formula (3), one axis: input index h is reached from o = (h + p - off) / s where that is a whole number in [0, O); -> (h, o)"""
    h = np.arange(L)
    t = h + p - off
    keep = (t >= 0) & (t // s < O)
    if not floor:
        keep &= t % s == 0
    return h[keep], t[keep] // s


def ref_dw(c, x, dy, weight=None, tap_of=None, pad=None, dil=None):
    """dw[co][k] = sum_m dy[m][co] * xcol[m][k].  The keywords are the mutations' handles: a multiplicity per pixel m, another decoding
    of a 32-wide k block into (kh, kw, first channel), other paddings and dilations."""
    n, h, w, cin, cout, KH, KW, s, p, d = c
    p, d = pad or p, dil or d
    oh, ow = out_hw(c)
    if weight is not None:
        dy = dy * np.asarray(weight, np.int64).reshape(n, oh, ow, 1)
    K = KH * KW * cin
    blk = cin if tap_of is None else BKK
    dw = np.zeros((cout, K), np.int64)
    for k0 in range(0, K, blk):
        if tap_of is None:
            (kh, kw), c0 = divmod(k0 // cin, KW), 0
        else:
            kh, kw, c0 = tap_of(k0)
        o_h, i_h = _reach(oh, h, s, p[0], kh * d[0])
        o_w, i_w = _reach(ow, w, s, p[1], kw * d[1])
        if len(o_h) and len(o_w):
            a = dy[:, o_h[:, None], o_w[None, :], :].reshape(-1, cout)
            b = x[:, i_h[:, None], i_w[None, :], c0:c0 + blk].reshape(-1, blk)
            dw[:, k0:k0 + blk] = a.T @ b
    return dw


def ref_db(c, dy, weight=None):
    """db[co] = sum_m dy[m][co]"""
    if weight is not None:
        oh, ow = out_hw(c)
        dy = dy * np.asarray(weight, np.int64).reshape(c[0], oh, ow, 1)
    return dy.sum((0, 1, 2))


def ref_dx(c, w, dy, floor=False, tap_index=None, pad=None, dil=None, couts=None):
    """dx[n][h][w][ci] = sum over (co, kh, kw) with (h + ph - kh*dh) % s == 0 ... of dy[n][(h + ph - kh*dh)/s][..][co] * w[co][k]"""
    n, h, w_, cin, cout, KH, KW, s, p, d = c
    p, d = pad or p, dil or d
    oh, ow = out_hw(c)
    couts = cout if couts is None else couts
    dx = np.zeros((n, h, w_, cin), np.int64)
    for kh in range(KH):
        i_h, o_h = _gather(h, oh, s, p[0], kh * d[0], floor)
        for kw in range(KW):
            i_w, o_w = _gather(w_, ow, s, p[1], kw * d[1], floor)
            if len(i_h) and len(i_w):
                t = kh * KW + kw if tap_index is None else tap_index(kh, kw)
                dx[:, i_h[:, None], i_w[None, :], :] += dy[:, o_h[:, None], o_w[None, :], :couts] @ w[:couts, t * cin:(t + 1) * cin]
    return dx


def ref_pack(c, w, rotate=True):
    """wt[ci][(kh*KW + kw)*Cout + co] = w[co][((KH-1-kh)*KW + (KW-1-kw))*Cin + ci]; a permutation, of any element type"""
    n, h, w_, cin, cout, KH, KW, s, p, d = c
    v = w.reshape(cout, KH, KW, cin)
    if rotate:
        v = v[:, ::-1, ::-1, :]
    return np.ascontiguousarray(v.transpose(3, 1, 2, 0)).reshape(cin, KH * KW * cout)


def ref_forward(x, w, KH, KW, s, p, d):
    """the forward definition on NHWC x and a packed bank [Cout][KH*KW*Cin], taps outside x contribute 0 -> y NHWC"""
    n, h, w_, cin = x.shape
    oh, ow = (h + 2 * p[0] - d[0] * (KH - 1) - 1) // s + 1, (w_ + 2 * p[1] - d[1] * (KW - 1) - 1) // s + 1
    y = np.zeros((n, oh, ow, w.shape[0]), np.int64)
    for kh in range(KH):
        o_h, i_h = _reach(oh, h, s, p[0], kh * d[0])
        for kw in range(KW):
            o_w, i_w = _reach(ow, w_, s, p[1], kw * d[1])
            if len(o_h) and len(o_w):
                t = kh * KW + kw
                y[:, o_h[:, None], o_w[None, :], :] += x[:, i_h[:, None], i_w[None, :], :] @ w[:, t * cin:(t + 1) * cin].T
    return y


@functools.lru_cache(maxsize=None)
def reference_w(c, family):
    """(dw, db) int64 of the case's own operands; computed once per process, read-only"""
    x, dy = operand(c, family, 'x'), operand(c, family, 'dy')
    out = ref_dw(c, x, dy), ref_db(c, dy)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_x(c, family):
    """dx int64 of the case's own operands; computed once per process, read-only"""
    dx = ref_dx(c, operand(c, family, 'w'), operand(c, family, 'dy'))
    dx.setflags(write=False)
    return dx


# ---- the lists --------------------------------------------------------------------------------------------------------------------
ONE = (1, 1)


def _point(m, cin=32, cout=64):
    return (1, 1, m, cin, cout, 1, 1, 1, (0, 0), ONE)


# weight-gradient entries are (case, listed psplits); the launcher's own choice (psplit 0) runs on every one of them as well
M_MAX = 3 * CHUNK + 1                                   # every residue of M mod CHUNK at 0, 1 and 2 whole chunks, and one pixel more
M_SWEEP = [(_point(m), tuple(sorted({1} | {ps for ps in (2, 3, m) if ps <= m}))) for m in range(1, M_MAX + 1)]

COUTS = tuple(range(1, 2 * BCO + 5))
COUT_SWEEP = [((1, 3, 11, 32, co, 1, 1, 1, (0, 0), ONE), (1, 2)) for co in COUTS]
COUT_ROUTE_B = [(1, 3, 11, cin, co, 1, 1, 1, (0, 0), ONE) for cin in (32, 64) for co in COUTS]

K_CIN = (32, 64, 96, 160)
K_FILTERS = ((1, 1), (3, 3), (1, 3), (3, 1), (2, 2), (2, 3), (5, 5), (7, 7))
K_SWEEP = [(2, 9, 8, cin, 32, kh, kw, 1, ((kh - 1) // 2, (kw - 1) // 2), ONE) for cin in K_CIN for kh, kw in K_FILTERS]

# (KH, KW, stride, pad, dil)
CONFIGS = [
    (3, 3, 1, (0, 0), (1, 1)), (3, 3, 1, (1, 1), (1, 1)),
    (3, 3, 1, (2, 2), (2, 2)), (3, 3, 1, (0, 0), (2, 1)), (3, 3, 1, (0, 0), (1, 2)),
    (3, 3, 1, (2, 2), (1, 1)),                          # pad' = 0
    (3, 3, 1, (3, 3), (1, 1)),                          # pad' < 0: route B only, OH > H
    (1, 1, 1, (1, 1), (1, 1)),                          # route B only; the border of dy sees only padding
    (1, 3, 1, (0, 1), (1, 1)), (3, 1, 1, (1, 0), (1, 1)), (2, 2, 1, (0, 0), (1, 1)), (2, 2, 2, (1, 1), (1, 1)),
    (3, 3, 2, (0, 0), (1, 1)), (3, 3, 2, (1, 1), (1, 1)), (3, 3, 2, (1, 0), (2, 1)), (3, 3, 3, (1, 1), (1, 1)),
    (1, 1, 2, (0, 0), (1, 1)), (1, 1, 3, (0, 0), (1, 1)),   # x pixels no tap reaches
    (5, 5, 1, (2, 2), (1, 1)),
    # beyond the specified ones: 2x2 at stride 2 and pad 1 reaches every pixel of x, so the only rows of dx that route B must leave at 0
    # because EVERY tap fails `% stride` would be those of the 1x1 filters, where the tap loops run once.  Stride 3 under two taps has such
    # rows and columns (index 2 mod 3) with both taps walked.
    (2, 2, 3, (0, 0), (1, 1)),
]
GEO_MAPS = [(n, h, w) for n in (1, 2) for h in range(1, 6) for w in range(1, 10)]
GEO_WIDE_W = (1, 4, 9)                                  # the maps that also run 64 -> 40 channels
GEOMETRY = [c for n, h, w in GEO_MAPS for cfg in CONFIGS for cin, cout in ((32, 32), (64, 40))
            if (cin == 32 or w in GEO_WIDE_W) for c in [(n, h, w, cin, cout) + cfg] if valid(c)]

BIG = {
    'route_b': (1, 1, DGRAD_CAP + 37, 1024, 1, 1, 1, 1, (0, 0), ONE),     # DGRAD_CAP + 37 blocks of 256 threads: 37 go round twice
    'pack': (1, 1, 1, 512, 520, 3, 3, 1, (1, 1), ONE),                    # 9360 blocks' worth of elements under a cap of 8192
}

UNREACHED_CONFIGS = [(1, 1, 2, (0, 0), ONE), (1, 1, 3, (0, 0), ONE), (2, 2, 2, (1, 1), ONE), (2, 2, 3, (0, 0), ONE)]
UNREACHED = [c for c in GEOMETRY if config(c) in UNREACHED_CONFIGS and c[3] == 32]

ROUTE_B_ONLY_CONFIGS = [cfg for cfg in CONFIGS if not route_a((1, 5, 9, 32, 32) + cfg)]
REFUSED_BASE = (1, 3, 11, 32, 32, 3, 3, 1, (1, 1), ONE)
REFUSED_W = ['psplit_gt_M', 'psplit_no_ws', 'x_off4', 'dy_off4', 'dw_off4', 'ws_off4', 'cin48', 'bad_oh', 'n0']
REFUSED_X = ['dy_off4', 'w_off4', 'dx_off4', 'cin48', 'bad_oh', 'n0'] + ['route1_' + config_id(cfg) for cfg in ROUTE_B_ONLY_CONFIGS]

PYTHON_SURFACE = [c for c in K_SWEEP if (c[3], c[5], c[6]) in ((96, 1, 3), (32, 3, 1), (96, 3, 3), (64, 2, 3), (160, 1, 1), (32, 5, 5))]


def pairs(entries):
    return [(c, ps) for c, listed in entries for ps in listed]


def all_cases():
    """every case of every list, once each, in list order"""
    seen = dict.fromkeys([c for c, _ in M_SWEEP] + [c for c, _ in COUT_SWEEP] + COUT_ROUTE_B + K_SWEEP + GEOMETRY + list(BIG.values())
                         + [REFUSED_BASE])
    return list(seen)


# ---- mutations: plausible wrong kernels, as wrong references ---------------------------------------------------------------------
def slice_starts(m, psplit):
    return [m * s // psplit for s in range(psplit)]


def _one_pass(a, first):
    a = a.astype(np.float64).reshape(-1).copy()
    a[first:] = np.nan                                  # what the second pass of the loop would have written stays the canary
    return a


def mutate(name, c, family='small', psplit=1):
    """{output name: wrong reference} of mutation `name` on the case's own operands ('pack': on random_bank); {} where it does not apply"""
    n, h, w_, cin, cout, KH, KW, s, p, d = c
    op = lambda nm: operand(c, family, nm)
    if name == 'no_rotate':
        return {'pack': ref_pack(c, random_bank(c), rotate=False)}
    if name == 'swap_khkw':                             # the tap decoded with KH in place of KW
        def tap_of(k0):
            tap = k0 // cin
            return tap // KH, tap - tap // KH * KH, k0 - tap * cin
        return {'dw': ref_dw(c, op('x'), op('dy'), tap_of=tap_of),
                'dx': ref_dx(c, op('w'), op('dy'), tap_index=lambda kh, kw: (kh * KH + kw) % (KH * KW))}
    if name in ('swap_pad', 'swap_dil'):
        kw = {'pad': p[::-1]} if name == 'swap_pad' else {'dil': d[::-1]}
        return {'dw': ref_dw(c, op('x'), op('dy'), **kw), 'dx': ref_dx(c, op('w'), op('dy'), **kw)}
    if name == 'tap_of_32':                             # the k block's tap computed as if Cin were 32
        return {'dw': ref_dw(c, op('x'), op('dy'), tap_of=lambda k0: divmod(k0 // 32, KW) + (k0 - k0 // 32 * 32,))}
    if name in ('drop_last_pixel', 'slice_overlap'):
        m = pixels(c)
        weight = np.ones(m, np.int64)
        if name == 'drop_last_pixel':
            weight[-1] = 0
        elif psplit > 1:
            weight[slice_starts(m, psplit)[1:]] += 1    # the first pixel of every later slice also ends the slice before it
        else:
            return {}
        return {'dw': ref_dw(c, op('x'), op('dy'), weight=weight), 'db': ref_db(c, op('dy'), weight=weight)}
    if name == 'stride_floor':
        return {'dx': ref_dx(c, op('w'), op('dy'), floor=True)}
    if name == 'cout_block':
        return {'dx': ref_dx(c, op('w'), op('dy'), couts=64)}
    if name == 'one_pass':
        out = {}
        if c == BIG['route_b']:
            out['dx'] = _one_pass(reference_x(c, family), DGRAD_CAP * THREADS * 4)
        if c == BIG['pack']:
            out['pack'] = _one_pass(ref_pack(c, random_bank(c)), PACK_CAP * THREADS)
        return out
    raise KeyError(name)


# mutation -> (the list it targets, the outputs it must change on at least one entry of it)
MUTATIONS = {
    'no_rotate': ('K_SWEEP', ('pack',)),
    'swap_khkw': ('K_SWEEP', ('dw', 'dx')),
    'swap_pad': ('GEOMETRY', ('dw', 'dx')),
    'swap_dil': ('GEOMETRY', ('dw', 'dx')),
    'tap_of_32': ('K_SWEEP', ('dw',)),
    'drop_last_pixel': ('M_SWEEP', ('dw', 'db')),
    'slice_overlap': ('M_SWEEP', ('dw', 'db')),
    'stride_floor': ('GEOMETRY', ('dx',)),
    'cout_block': ('COUT_ROUTE_B', ('dx',)),
    'one_pass': ('BIG', ('dx', 'pack')),
}


def targets(list_name):
    """[(case, psplit)] of a list, for the mutations"""
    if list_name in ('M_SWEEP', 'COUT_SWEEP'):
        return pairs(globals()[list_name])
    if list_name == 'BIG':
        return [(c, 1) for c in BIG.values()]
    return [(c, 1) for c in globals()[list_name]]
