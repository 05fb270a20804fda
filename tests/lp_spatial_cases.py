"""Lists, operands, float64 references and reference mutations of the low-precision spatial sweep: usot_conv3x3_halo_lp,
usot_bneck_first_lp / usot_bneck_tail_lp, usot_conv_kstream_lp, usot_conv_pw_lp / usot_conv_pw_pair_lp.

Plain module: no fixtures, nothing launched.  tests/test_lp_spatial_lists.py pins what is here, tests/test_gpu_lp_spatial_sweep.py
runs it.

EXACT OPERANDS.  Inputs are integers 0 .. 3, filters are ternary times a power of two, biases and residuals are integers times a
power of two.  The GRANULE of a sum is the largest power of two that divides every addend; bounds() computes, for every stage of
every case and storage type, max over the outputs of (sum |products| + |bias| + |residual|) / granule, and the list test asserts
it below 2^24: every partial sum of every summation order is then a multiple of the granule below 2^24 granules - an fp32 number -
so the fp32 accumulators of the kernels hold the exact sum whatever their order (per-tap or row-shared k-loop, either panel form,
MFMA lanes, unfused launches), and EVERY comparison is equality, in bf16 and in fp16.  The reference is float64 from the definition
with an explicit index gather (taps()), rounded to nearest even into the storage type where a kernel stores or re-reads a 16-bit
value: t1, t2, y, t of the bneck kernels, T2, Y, T of conv_pw, the one output of the others (usot_pack2_lp converts that way).
The fine granule of the biases (2^-7 and below) is what makes the rounding real: sums of some tens at that granule need more
than the 8 or 11 significant bits of the storage types.

MUTATIONS.  Each is a wrong kernel one can name, applied to the reference: expected(case, dtype, mut).  meaningful(mut, case) says
from the geometry alone (the gather indices differ / the ragged tile exists / ...) whether the mutation can change the result; the
list test asserts that it then DOES, for these operands - a case that cannot see a named defect it should see is blind."""
import collections
import functools
import zlib

import torch

DTYPES = (('bf16', torch.bfloat16, 0), ('fp16', torch.float16, 1))
ACT_NONE, ACT_RELU = 0, 1
LIMIT = float(2 ** 24)

Halo = collections.namedtuple('Halo', 'N H W act bias')
Bneck = collections.namedtuple('Bneck', 'kind N H W cn')                         # kind: 'first' | 'tail'
KStream = collections.namedtuple('KStream', 'N H W Cin Cout stride pad dil act bias plan')
ConvPw = collections.namedtuple('ConvPw', 'N H W KH KW stride pad_h pad_w dil_h dil_w cm cn act2')      # cn 0: usot_conv_pw_lp
Geo = collections.namedtuple('Geo', 'N H W KH KW stride pad_h pad_w dil_h dil_w')

MUTATIONS = ('tap_row', 'tap_col', 'pad_clamp', 'row_wrap', 'image_wrap', 'last_row', 'last_col', 't1_pad', 'shortcut_centre',
             'round_skip', 'k_chunk', 'stride_phase')
TAP_MUTATIONS = ('tap_row', 'tap_col', 'pad_clamp', 'row_wrap', 'image_wrap', 'stride_phase')
HALO_TILE = (16, 16)                        # csrc/conv3x3_halo.hip: HT x HT output pixels
BNECK_TILE = (8, 16)                        # csrc/bneck_lp.hip: TH x TW
KSTREAM_PANEL = 256                         # csrc/conv_kstream.hip: CK_BM
CORNERS = ((1, 1), (16, 16), (17, 17), (15, 33), (33, 15), (32, 32), (33, 33))


# ------------------------------------------------------------------------------------------------------------------ geometry
def out_hw(g):
    return ((g.H + 2 * g.pad_h - g.dil_h * (g.KH - 1) - 1) // g.stride + 1, (g.W + 2 * g.pad_w - g.dil_w * (g.KW - 1) - 1) // g.stride + 1)


def geo_of(case):
    if isinstance(case, (Halo, Bneck)):
        return Geo(case.N, case.H, case.W, 3, 3, 1, 1, 1, 1, 1)
    if isinstance(case, KStream):
        return Geo(case.N, case.H, case.W, 3, 3, case.stride, case.pad, case.pad, case.dil, case.dil)
    return Geo(*case[:10])


def pixels(case):
    g = geo_of(case)
    oh, ow = out_hw(g)
    return g.N * oh * ow


def taps(g, mut=None):
    """int64 [KH * KW][M]: for every tap and output pixel the flat input pixel (n * H + ih) * W + iw it reads, -1 = a zero.
    mut: one of TAP_MUTATIONS - the indices a kernel with that defect would read."""
    oh, ow = out_hw(g)
    n = torch.arange(g.N).view(-1, 1, 1)
    ph = 1 if mut == 'stride_phase' and g.stride > 1 else 0
    ih0 = (torch.arange(oh) * g.stride - g.pad_h + ph).view(1, -1, 1)
    iw0 = (torch.arange(ow) * g.stride - g.pad_w + ph).view(1, 1, -1)
    total = g.N * g.H * g.W
    out = []
    for kh in range(g.KH):
        for kw in range(g.KW):
            first = kh == 0 and kw == 0
            ih = ih0 + (kh + (1 if mut == 'tap_row' and first else 0)) * g.dil_h
            iw = iw0 + (kw + (1 if mut == 'tap_col' and first else 0)) * g.dil_w
            if mut == 'pad_clamp':
                ih, iw = ih.clamp(0, g.H - 1), iw.clamp(0, g.W - 1)
            okh, okw = (ih >= 0) & (ih < g.H), (iw >= 0) & (iw < g.W)
            flat = (n * g.H + ih) * g.W + iw
            ok = okh & okw
            if mut == 'row_wrap':           # a kw tap past a row end: the flattened neighbour, where the buffer has one
                ok = okh & (okw | ((flat >= 0) & (flat < total)))
            elif mut == 'image_wrap':       # a kh tap past an image end: the neighbouring image's row (or this one's, for iw)
                ok = okw & (okh | ((flat >= 0) & (flat < total)))
            out.append(torch.where(ok, flat, torch.full_like(flat, -1)).reshape(-1))
    return torch.stack(out)


def gather_conv(x, w, src, pad_row=None):
    """sum over taps of X[src[tap]] . w[:, tap]^T in float64: x [N][H][W][C], w [Cout][KH * KW][C], src from taps() -> [M][Cout].
    pad_row: what a -1 reads (default zeros)"""
    C = x.shape[-1]
    X = torch.cat([x.reshape(-1, C), (torch.zeros(1, C, dtype=x.dtype) if pad_row is None else pad_row.view(1, C))])
    out = torch.zeros(src.shape[1], w.shape[0], dtype=torch.float64)
    for t in range(src.shape[0]):
        out += X[src[t]] @ w[:, t].t()
    return out


def rne(v, dtype):
    """float64 -> storage type, round to nearest even -> float64 (exact through fp32: every value here is an fp32 number)"""
    f = v.float()
    assert torch.equal(f.double(), v), 'a reference value is not an fp32 number: the exactness bound cannot hold'
    return f.to(dtype).double()


def granule(*tensors):
    """the largest power of two (down to 2^-40) dividing every element of the given float64 tensors"""
    for k in range(-8, 41):
        s = 2.0 ** k
        if all(torch.equal((t * s).round(), t * s) for t in tensors):
            return 2.0 ** -k
    raise AssertionError('finer than 2^-40')


# ------------------------------------------------------------------------------------------------------------------ operands
def _gen(case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(repr((tuple(case), type(case).__name__, salt)).encode()))


def _ints(g, shape, lo, hi, scale=1.0):
    return torch.randint(lo, hi + 1, shape, generator=g).double() * scale


def _tern(g, shape, density, scale=1.0):
    keep = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (keep * sign).double() * scale


B_FINE = 2.0 ** -7                          # granule of the bias that precedes a rounding of sums of tens


@functools.lru_cache(maxsize=8)
def halo_ops(case):
    g = _gen(case)
    return dict(x=_ints(g, (case.N, case.H, case.W, 64), 0, 3), w=_tern(g, (64, 9, 64), 0.5),
                b=_ints(g, (64,), -1024, 1024, B_FINE) if case.bias else None)


@functools.lru_cache(maxsize=8)
def kstream_ops(case):
    g = _gen(case)
    return dict(x=_ints(g, (case.N, case.H, case.W, case.Cin), 0, 3), w=_tern(g, (case.Cout, 9, case.Cin), 0.25),
                b=_ints(g, (case.Cout,), -1024, 1024, B_FINE) if case.bias else None)


@functools.lru_cache(maxsize=8)
def bneck_ops(case):
    g = _gen(case)
    o = dict(w2=_tern(g, (64, 9, 64), 0.25), b2=_ints(g, (64,), -1024, 1024, B_FINE),
             w3=_tern(g, (256, 64), 0.5, 0.25), b3=_ints(g, (256,), -8, 8),
             wn=_tern(g, (case.cn, 256), 0.25, 0.125), bn=_ints(g, (case.cn,), -8, 8))
    if case.kind == 'first':
        o.update(x=_ints(g, (case.N, case.H, case.W, 64), 0, 3), w1=_tern(g, (64, 64), 0.5), b1=_ints(g, (64,), 1, 512, B_FINE),
                 wd=_tern(g, (256, 64), 0.5))
    else:
        o.update(t1=_ints(g, (case.N, case.H, case.W, 64), 0, 3), res=_ints(g, (case.N, case.H, case.W, 256), 0, 15))
    return o


@functools.lru_cache(maxsize=8)
def convpw_ops(case):
    g = _gen(case)
    cm, co = case.cm, 4 * case.cm
    M = pixels(case)
    o = dict(x=_ints(g, (case.N, case.H, case.W, cm), 0, 3), w2=_tern(g, (cm, case.KH * case.KW, cm), 0.25),
             b2=_ints(g, (cm,), -1024, 1024, B_FINE), w3=_tern(g, (co, cm), 0.25, 0.25), b3=_ints(g, (co,), -8, 8),
             res=_ints(g, (M, co), 0, 15))
    if case.cn:
        o.update(w1=_tern(g, (case.cn, co), 0.125, 0.125), b1=_ints(g, (case.cn,), -8, 8))
    return o


def ops_of(case):
    return {Halo: halo_ops, KStream: kstream_ops, Bneck: bneck_ops, ConvPw: convpw_ops}[type(case)](case)


# ------------------------------------------------------------------------------------------------------------------ references
def _last_tile(v, g, tile, mut):
    """the ragged tile row / column of an output [N][H][W][C] taken from the neighbouring tile"""
    th, tw = tile
    v = v.clone()
    if mut == 'last_row' and g.H % th and g.H > th:
        r0 = g.H - g.H % th
        v[:, r0:] = v[:, r0 - th:g.H - th]
    if mut == 'last_col' and g.W % tw and g.W > tw:
        c0 = g.W - g.W % tw
        v[:, :, c0:] = v[:, :, c0 - tw:g.W - tw]
    return v


def _swap_chunks(w):
    """the first two 64-channel chunks of the middle tap of a bank [Cout][taps][Cin] swapped"""
    w = w.clone()
    t = w.shape[1] // 2
    w[:, t, 0:64], w[:, t, 64:128] = w[:, t, 64:128].clone(), w[:, t, 0:64].clone()
    return w


def _stage(name, pre, dtype, stages, relu=True, skip=False):
    v = pre.relu() if relu else pre
    r = v if skip else rne(v, dtype)
    if stages is not None:
        stages[name] = (v, r)
    return r


def compute(case, dtype, mut=None, stages=None):
    """-> dict of the outputs (float64 values of the storage type, shaped as the kernel stores them).  stages: a dict that
    receives name -> (value before rounding, value after) for every rounded stage."""
    o, g = ops_of(case), geo_of(case)
    src = taps(g, mut if mut in TAP_MUTATIONS else None)
    oh, ow = out_hw(g)
    if isinstance(case, (Halo, KStream)):
        w = _swap_chunks(o['w']) if mut == 'k_chunk' else o['w']
        pre = gather_conv(o['x'], w, src) + (o['b'] if o['b'] is not None else 0.0)
        y = _stage('y', pre, dtype, stages, relu=case.act == ACT_RELU).view(g.N, oh, ow, -1)
        if isinstance(case, Halo):
            y = _last_tile(y, g, HALO_TILE, mut)
        return {'y': y}
    if isinstance(case, Bneck):
        M = g.N * g.H * g.W
        pad_row = None
        if case.kind == 'first':
            x = o['x'].view(M, 64)
            t1 = _stage('t1', x @ o['w1'].t() + o['b1'], dtype, stages, skip=mut == 'round_skip').view(g.N, g.H, g.W, 64)
            if mut == 't1_pad':             # conv1 of a zero x instead of a zero: what a halo computed without a border mask holds
                pad_row = rne(o['b1'].relu(), dtype)
        else:
            t1 = o['t1']
        t2 = _stage('t2', gather_conv(t1, o['w2'], src, pad_row) + o['b2'], dtype, stages, skip=mut == 'round_skip' and case.kind == 'tail')
        pre = t2 @ o['w3'].t() + o['b3']
        if case.kind == 'first':
            xs = o['x']
            if mut == 'shortcut_centre':    # the halo tile's origin instead of its centre: pixel (h - 1, w - 1)
                xs = torch.zeros_like(xs)
                xs[:, 1:, 1:] = o['x'][:, :-1, :-1]
            pre = pre + xs.reshape(M, 64) @ o['wd'].t()
        else:
            pre = pre + o['res'].view(M, 256)
        y = _stage('y', pre, dtype, stages)
        t = _stage('t', y @ o['wn'].t() + o['bn'], dtype, stages)
        return {'y': _last_tile(y.view(g.N, g.H, g.W, 256), g, BNECK_TILE, mut), 't': _last_tile(t.view(g.N, g.H, g.W, -1), g, BNECK_TILE, mut)}
    w2 = _swap_chunks(o['w2']) if mut == 'k_chunk' else o['w2']
    t2 = _stage('t2', gather_conv(o['x'], w2, src) + o['b2'], dtype, stages, skip=mut == 'round_skip')
    y = _stage('y', t2 @ o['w3'].t() + o['b3'] + o['res'], dtype, stages)
    out = {'y': y}
    if case.cn:
        out['t'] = _stage('t', y @ o['w1'].t() + o['b1'], dtype, stages, relu=case.act2 == ACT_RELU)
    return out


def expected(case, dtype, mut=None):
    """the outputs as tensors of the storage type: the bits the kernel owes"""
    return {k: v.float().to(dtype) for k, v in compute(case, dtype, mut).items()}


def bounds(case, dtype):
    """name of the stage -> max over its outputs of (sum |products| + |bias| + |residual|) / granule: exact in fp32 below 2^24"""
    o, g = ops_of(case), geo_of(case)
    st = {}
    compute(case, dtype, None, st)
    src = taps(g)
    out = {}

    def one(name, absum, *addends):
        gr = granule(*addends)
        out[name] = float(absum.max()) / gr

    if isinstance(case, (Halo, KStream)):
        b = o['b'] if o['b'] is not None else torch.zeros(1, dtype=torch.float64)
        one('y', gather_conv(o['x'].abs(), o['w'].abs(), src) + b.abs(), b, torch.tensor(granule(o['x']) * granule(o['w'])))
        return out
    if isinstance(case, Bneck):
        M = g.N * g.H * g.W
        if case.kind == 'first':
            x = o['x'].view(M, 64)
            one('t1', x @ o['w1'].abs().t() + o['b1'].abs(), o['b1'], torch.tensor(granule(x) * granule(o['w1'])))
            t1 = st['t1'][1].view(g.N, g.H, g.W, 64)
        else:
            t1 = o['t1']
        one('t2', gather_conv(t1.abs(), o['w2'].abs(), src) + o['b2'].abs(), o['b2'], torch.tensor(granule(t1) * granule(o['w2'])))
        t2, y = st['t2'][1], st['y'][1]
        if case.kind == 'first':
            one('y', t2 @ o['w3'].abs().t() + x @ o['wd'].abs().t() + o['b3'].abs(), o['b3'],
                torch.tensor(granule(t2) * granule(o['w3'])), torch.tensor(granule(x) * granule(o['wd'])))
        else:
            res = o['res'].view(M, 256)
            one('y', t2 @ o['w3'].abs().t() + res + o['b3'].abs(), o['b3'], res, torch.tensor(granule(t2) * granule(o['w3'])))
        one('t', y @ o['wn'].abs().t() + o['bn'].abs(), o['bn'], torch.tensor(granule(y) * granule(o['wn'])))
        return out
    one('t2', gather_conv(o['x'], o['w2'].abs(), src) + o['b2'].abs(), o['b2'], torch.tensor(granule(o['x']) * granule(o['w2'])))
    t2, y = st['t2'][1], st['y'][1]
    one('y', t2 @ o['w3'].abs().t() + o['res'] + o['b3'].abs(), o['b3'], o['res'], torch.tensor(granule(t2) * granule(o['w3'])))
    if case.cn:
        one('t', y @ o['w1'].abs().t() + o['b1'].abs(), o['b1'], torch.tensor(granule(y) * granule(o['w1'])))
    return out


# ------------------------------------------------------------------------------------------------------------------ mutations
def applies(mut, case):
    """the mutation names a defect the case's kernel could have at all"""
    if mut in ('last_row', 'last_col'):
        return isinstance(case, (Halo, Bneck))
    if mut in ('t1_pad', 'shortcut_centre'):
        return isinstance(case, Bneck) and case.kind == 'first'
    if mut == 'round_skip':
        return isinstance(case, (Bneck, ConvPw))
    if mut == 'k_chunk':
        return isinstance(case, (KStream, ConvPw))
    if mut == 'stride_phase':
        return isinstance(case, (KStream, ConvPw)) and case.stride > 1
    return True


def meaningful(mut, case):
    """from the geometry alone: the defect changes what the kernel reads / where it stores / what it rounds in this case"""
    if not applies(mut, case):
        return False
    g = geo_of(case)
    if mut in TAP_MUTATIONS:
        return not torch.equal(taps(g, mut), taps(g))
    if mut in ('last_row', 'last_col'):
        th, tw = HALO_TILE if isinstance(case, Halo) else BNECK_TILE
        return (g.H % th != 0 and g.H > th) if mut == 'last_row' else (g.W % tw != 0 and g.W > tw)
    if mut == 't1_pad':
        return bool((taps(g) < 0).any())
    if mut == 'shortcut_centre':
        return True
    if mut == 'k_chunk':                    # the middle tap is read somewhere
        return bool((taps(g)[g.KH * g.KW // 2] >= 0).any())
    return True                             # round_skip: every case of the kernels it applies to


# ------------------------------------------------------------------------------------------------------------------ the lists
def halo_cases():
    out = [Halo(1, h, 17, h & 1, True) for h in range(1, 34)]
    out += [Halo(1, 5, w, (w >> 1) & 1, True) for w in range(1, 34)]
    out += [Halo(2, h, w, i & 1, True) for i, (h, w) in enumerate(CORNERS)]
    out += [Halo(2, 17, 18, 1, False)]                           # bias = NULL
    out += [Halo(HALO_MANY_TILES, 3, 2, 1, True)]                # more tiles than any grid (one workgroup per CU)
    return out


HALO_MANY_TILES = 520


def bneck_images(h, w, tiles=8):
    """the smallest batch with at least `tiles` 8 x 16 tiles"""
    per = -(-h // BNECK_TILE[0]) * -(-w // BNECK_TILE[1])
    return -(-tiles // per)


def bneck_tiles(case):
    return case.N * -(-case.H // BNECK_TILE[0]) * -(-case.W // BNECK_TILE[1])


def bneck_cases(kind, cn):
    mk = lambda n, h, w: Bneck(kind, n, h, w, cn)
    out = [mk(bneck_images(h, 17), h, 17) for h in range(1, 18)]
    out += [mk(bneck_images(9, w), 9, w) for w in range(1, 34)]
    out += [mk(bneck_images(h, w), h, w) for h, w in CORNERS]
    out += [mk(11, 7, 13), mk(3, 9, 33)]                          # 11 and 18 tiles: blocks 0 .. 2 / 0 .. 1 of a grid of 8 / 16 take a second tile
    return list(dict.fromkeys(out))                               # (9, 17) and (17, 17) are in two of the sweeps


BNECK_FAMILIES = (('first', 64), ('tail', 64), ('tail', 128))


def kstream_smallest(stride, pad, dil):
    """the smallest (H, W) the launcher accepts at N = 3: at least one output pixel, more than dil * (W + 1) pixels in the batch"""
    for s in range(1, 64):
        g = Geo(3, s, s, 3, 3, stride, pad, pad, dil, dil)
        if min(out_hw(g)) >= 1 and kstream_accepts(3, s, s, stride, pad, dil):
            return (s, s)
    raise AssertionError


def kstream_accepts(N, H, W, stride, pad, dil):
    """the geometry rules of usot_conv_kstream_lp (csrc/conv_kstream.hip)"""
    if not (1 <= stride <= 2 and dil >= 1 and 0 <= pad <= dil and N > 0 and H > 0 and W > 0):
        return False
    oh, ow = out_hw(Geo(N, H, W, 3, 3, stride, pad, pad, dil, dil))
    if oh <= 0 or ow <= 0:
        return False
    if (oh - 1) * stride - pad + dil >= H or (ow - 1) * stride - pad + dil >= W:
        return False
    return N * H * W > dil * (W + 1)


def kstream_parked(N, H, W, stride, pad, dil):
    """the address model of set_tap (csrc/conv_kstream.hip): the set of flat pixels of x a launch reads - a tap inside the image
    reads its pixel; a tap outside it is parked on the lane's centre pixel c, or on the tap's offset `rel` from it where
    c - rel <= 0 (the lane then reads x + rel)"""
    g = Geo(N, H, W, 3, 3, stride, pad, pad, dil, dil)
    src = taps(g)
    centre = src[4]
    assert bool((centre >= 0).all())
    read = set()
    for t in range(9):
        rel = (t // 3 - 1) * dil * W + (t % 3 - 1) * dil
        parked = torch.where(centre - rel > 0, centre, torch.full_like(centre, rel))
        read.update(torch.where(src[t] >= 0, src[t], parked).tolist())
    return read


def kstream_cases():
    out = []
    k = 0
    for stride in (1, 2):
        for dil in (1, 2, 3):
            for pad in range(dil + 1):
                for hw in (kstream_smallest(stride, pad, dil), (7, 9), (9, 7), (5, 23)):
                    g = Geo(3, hw[0], hw[1], 3, 3, stride, pad, pad, dil, dil)
                    if min(out_hw(g)) < 1:
                        continue                                  # (7, 9) at dil 3 without padding has no output: the refusal list
                    cin, cout = (256, 512)[(k >> 1) & 1], (256, 512)[k & 1]
                    out.append(KStream(3, hw[0], hw[1], cin, cout, stride, pad, dil, int(k % 3 != 0), True, False))
                    k += 1
    # M = 255, 256, 257, 511, 513 (stride 1, pad = dil = 1: M = N H W)
    out += [KStream(n, h, w, 256, 256, 1, 1, 1, 1, True, False) for n, h, w in ((5, 3, 17), (4, 8, 8), (1, 257, 1), (7, 1, 73), (3, 9, 19))]
    out += [KStream(3, 6, 7, 512, 512, 1, 1, 1, 1, True, False), KStream(2, 5, 9, 256, 768, 2, 1, 1, 0, True, False),
            KStream(2, 7, 5, 256, 1024, 1, 2, 2, 1, True, False), KStream(3, 7, 9, 256, 256, 1, 1, 2, 1, False, False),
            KStream(3, 9, 7, 256, 512, 2, 1, 1, 1, True, True)]
    return out


# conv_pw: (cm, cn, act2) - cn 0 is usot_conv_pw_lp
CONVPW_FAMILIES = ((128, 0, 0), (256, 0, 0), (128, 128, 1), (128, 128, 0), (128, 256, 1), (128, 256, 0), (256, 256, 1), (256, 256, 0))
CONVPW_FORMS = (1, 2)                       # c2->tile & 3: 256- / 128-pixel panels
CONVPW_MAPS = ((1, 1), (1, 9), (9, 1), (3, 5), (7, 4), (13, 6))
CONVPW_M = (127, 128, 129, 255, 256, 257, 385)


def rowshared_eligible(c):
    """cp_fill's predicate (csrc/conv_pw_lp.hip) for the row-shared k-loop, tile & 4 clear"""
    oh, ow = out_hw(geo_of(c))
    return (c.KH == 3 and c.KW == 3 and c.stride == 1 and c.pad_h == c.dil_h and c.pad_w == c.dil_w and 1 <= c.dil_w <= 4
            and ow == c.W and oh == c.H and c.N * c.H * c.W * c.cm < 0x7fffffff)


def convpw_loops(c):
    """c2->tile & 4 values a case runs with: the per-tap loop, and the launcher's choice where that is the row-shared loop"""
    return (4, 0) if rowshared_eligible(c) or (c.KH == 3 and c.KW == 3 and c.stride == 1 and c.dil_w == 5) else (4,)


def convpw_pertap_cases():
    fam = lambda i: CONVPW_FAMILIES[i % len(CONVPW_FAMILIES)]
    rows = []
    # the pixel counts: a 1 x 1 map, a 1 x 1 filter (every panel edge at an image end) ...
    rows += [(m, 1, 1, 1, 1, 1, 0, 0, 1, 1) for m in CONVPW_M]
    # ... filters x strides over the maps, N in 1, 3, 5; unequal pads and dilations; padding beyond the filter's reach
    rows += [
        (3, 1, 9, 1, 1, 2, 0, 0, 1, 1), (5, 9, 1, 1, 1, 3, 0, 0, 1, 1), (1, 13, 6, 1, 1, 1, 1, 2, 1, 1),      # 1 x 1 (padded: pixels that see no input)
        (3, 3, 5, 1, 3, 1, 0, 1, 1, 1), (5, 1, 9, 1, 3, 2, 0, 2, 1, 2), (1, 7, 4, 1, 3, 3, 1, 3, 1, 3),       # 1 x 3
        (3, 9, 1, 3, 1, 1, 1, 0, 1, 1), (5, 13, 6, 3, 1, 2, 2, 0, 2, 1), (1, 7, 4, 3, 1, 3, 3, 1, 2, 1),      # 3 x 1 (pad_h 3 > reach 2)
        (3, 3, 5, 2, 2, 1, 0, 1, 1, 2), (5, 7, 4, 2, 2, 2, 1, 0, 2, 1), (1, 13, 6, 2, 2, 3, 2, 2, 1, 1),      # 2 x 2 (pad 2 > reach 1)
        (3, 3, 5, 3, 3, 1, 1, 1, 1, 1), (5, 7, 4, 3, 3, 2, 0, 1, 1, 1), (1, 13, 6, 3, 3, 3, 2, 1, 2, 1),      # 3 x 3
        (3, 1, 1, 3, 3, 1, 1, 1, 1, 1), (1, 1, 9, 3, 3, 1, 2, 1, 2, 1), (5, 9, 1, 3, 3, 1, 1, 3, 1, 3),       # ... on maps thinner than its reach
        (1, 13, 6, 3, 3, 1, 1, 2, 1, 2), (3, 7, 4, 3, 3, 1, 2, 1, 1, 1), (1, 3, 5, 3, 3, 1, 4, 5, 1, 2),      # pad != dil; pad beyond the reach
        (3, 13, 6, 3, 3, 2, 1, 2, 1, 2),
    ]
    out = [ConvPw(*r, *fam(i)) for i, r in enumerate(rows)]
    assert all(min(out_hw(geo_of(c))) >= 1 for c in out)
    return out


def convpw_rowshared_cases():
    """3 x 3 / stride 1 / pad = dil: dil_w 1 .. 4 x dil_h 1, 2, 5; every W of the list at every (dil_h, dil_w), H walking through
    1, 2, dil_h, dil_h + 1, 7; N the smallest batch with more than 256 pixels (a 128- and a 256-pixel panel edge inside); once
    dil_w = 5 (the launcher falls back to the per-tap loop)"""
    out = []
    i = 0
    for dh in (1, 2, 5):
        hs = sorted({1, 2, dh, dh + 1, 7})
        for dw in (1, 2, 3, 4):
            for j, w in enumerate((1, 2, 3, 4, 5, 8, 9)):
                h = hs[(j + dw + dh) % len(hs)]
                n = 257 // (h * w) + 1
                out.append(ConvPw(n, h, w, 3, 3, 1, dh, dw, dh, dw, *CONVPW_FAMILIES[i % len(CONVPW_FAMILIES)]))
                i += 1
    out.append(ConvPw(6, 7, 8, 3, 3, 1, 2, 5, 2, 5, 128, 128, 1))
    return out


def panel_edge_kinds(c):
    """how the edges of the 128-pixel panels inside the map meet it: 'row' = cut an image row, 'row_end', 'image_end'"""
    P, W = c.H * c.W, c.W
    kinds = set()
    for e in range(128, pixels(c), 128):
        kinds.add('image_end' if e % P == 0 else 'row_end' if e % W == 0 else 'row')
    return kinds


# ------------------------------------------------------------------------------------------------------------------ refusals
# (name, entry point, base case, the one change): every USOT_EINVAL branch of the six launchers.  Changes: ('arg', name, value) sets
# a scalar argument or descriptor field, ('null', name) passes NULL, ('misalign', name) passes the pointer + 2 bytes,
# ('geometry', ...) replaces N, H, W (operands are allocated for the base case, which is at least as large).
_HB = Halo(2, 17, 18, 1, True)
_BF = Bneck('first', 8, 9, 17, 64)
_BT = Bneck('tail', 8, 9, 17, 64)
_KB = KStream(3, 10, 9, 256, 256, 1, 1, 1, 1, True, False)
_PW = ConvPw(3, 7, 4, 3, 3, 1, 1, 1, 1, 1, 128, 0, 0)
_PP = ConvPw(3, 7, 4, 3, 3, 1, 1, 1, 1, 1, 128, 128, 1)


def refusals():
    R = []
    R += [('halo %s' % n, 'halo', _HB, ch) for n, ch in (
        ('Cin 128', ('arg', 'Cin', 128)), ('Cout 128', ('arg', 'Cout', 128)), ('act 2', ('arg', 'act', 2)), ('dtype 2', ('arg', 'dtype', 2)),
        ('N 0', ('arg', 'N', 0)), ('H 0', ('arg', 'H', 0)), ('W 0', ('arg', 'W', 0)),
        ('x NULL', ('null', 'x')), ('w NULL', ('null', 'w')), ('y NULL', ('null', 'y')),
        ('x misaligned', ('misalign', 'x')), ('w misaligned', ('misalign', 'w')), ('bias misaligned', ('misalign', 'b')),
        ('y misaligned', ('misalign', 'y')))]
    for ent, base in (('bneck_first', _BF), ('bneck_tail', _BT)):
        ptrs = ('x', 'w1', 'w2', 'w3c', 'wn', 'b2', 'b3c', 'bn', 'y', 't') + (('b1',) if ent == 'bneck_first' else ())
        R += [('%s %s NULL' % (ent, p), ent, base, ('null', p)) for p in ptrs]
        R += [('%s %s misaligned' % (ent, p), ent, base, ('misalign', p)) for p in ptrs]
        R += [('%s %s' % (ent, n), ent, base, ch) for n, ch in (
            ('dtype 2', ('arg', 'dtype', 2)), ('N 0', ('arg', 'N', 0)), ('H 0', ('arg', 'H', 0)), ('W 0', ('arg', 'W', 0)),
            ('7 tiles', ('geometry', 7, 8, 16)), ('1 tile', ('geometry', 1, 8, 16)))]
    R += [('bneck_tail Cnext 96', 'bneck_tail', _BT, ('arg', 'Cnext', 96)), ('bneck_tail Cnext 256', 'bneck_tail', _BT, ('arg', 'Cnext', 256))]
    R += [('kstream %s' % n, 'kstream', _KB, ch) for n, ch in (
        ('Cin 128', ('arg', 'Cin', 128)), ('Cout 384', ('arg', 'Cout', 384)), ('Cout 0', ('arg', 'Cout', 0)), ('act 2', ('arg', 'act', 2)),
        ('dtype 2', ('arg', 'dtype', 2)), ('stride 3', ('arg', 'stride', 3)), ('stride 0', ('arg', 'stride', 0)), ('pad > dil', ('arg', 'pad', 2)),
        ('pad -1', ('arg', 'pad', -1)), ('dil 0', ('arg', 'dil', 0)), ('N 0', ('arg', 'N', 0)), ('H 0', ('arg', 'H', 0)), ('W 0', ('arg', 'W', 0)),
        ('OH <= 0', ('geometry', 3, 2, 9, dict(pad=0))), ('OW <= 0', ('geometry', 3, 7, 2, dict(pad=0))),
        ('x NULL', ('null', 'x')), ('w NULL', ('null', 'w')), ('y NULL', ('null', 'y')),
        ('x misaligned', ('misalign', 'x')), ('w misaligned', ('misalign', 'w')), ('bias misaligned', ('misalign', 'b')),
        ('y misaligned', ('misalign', 'y')))]
    # the parked tap beyond the end of x: N H W <= dil (W + 1)
    R += [('kstream parked tap %s' % (geo,), 'kstream', _KB, ('geometry',) + geo) for geo in KSTREAM_PARKED_REFUSED]
    R += [('kstream plan: parked tap', 'kstream_plan', _KB, ('geometry',) + KSTREAM_PARKED_REFUSED[0])]
    for ent, base in (('conv_pw', _PW), ('conv_pw_pair', _PP)):
        ptrs = ('x', 'w2', 'b2', 'w3', 'b3', 'res', 'y') + (('w1', 'b1', 't') if ent == 'conv_pw_pair' else ())
        R += [('%s %s NULL' % (ent, p), ent, base, ('null', p)) for p in ptrs]
        R += [('%s %s misaligned' % (ent, p), ent, base, ('misalign', p)) for p in ptrs]
        R += [('%s %s' % (ent, n), ent, base, ch) for n, ch in (
            ('dtype 2', ('arg', 'dtype', 2)), ('conv2 without ReLU', ('arg', 'act', 0)), ('groups 2', ('arg', 'groups', 2)),
            ('ksplit 2', ('arg', 'ksplit', 2)), ('res in conv2', ('arg', 'res', 'x')), ('Cin 64', ('arg', 'Cin', 64)),
            ('Cout 64', ('arg', 'Cout', 64)), ('N 0', ('arg', 'N', 0)), ('KH 0', ('arg', 'KH', 0)), ('KW 0', ('arg', 'KW', 0)),
            ('stride 0', ('arg', 'stride', 0)), ('OH off by one', ('arg', 'OH', 8)), ('OW off by one', ('arg', 'OW', 5)),
            ('no output', ('arg', 'dil_h', 5)), ('descriptor NULL', ('null', 'c2')))]
    R += [('conv_pw_pair %s' % n, 'conv_pw_pair', _PP, ch) for n, ch in (
        ('pd.M != M', ('arg', 'pd.M', 85)), ('act2 2', ('arg', 'pd.act2', 2)), ('CN 64', ('arg', 'pd.CN', 64)), ('CO 256', ('arg', 'pd.CO', 256)),
        ('pd.CM 256', ('arg', 'pd.CM', 256)), ('pair descriptor NULL', ('null', 'pd')))]
    return R


# (N, H, W, {pad, dil}) at stride 1 with N H W <= dil (W + 1): one image no higher than the dilation, 1 x 1 x 257, H = 2 at dil = pad = 2, ...
KSTREAM_PARKED_REFUSED = ((1, 1, 9, dict(pad=1, dil=1)), (1, 1, 257, dict(pad=1, dil=1)), (1, 2, 9, dict(pad=2, dil=2)),
                          (1, 3, 7, dict(pad=3, dil=3)), (1, 2, 3, dict(pad=2, dil=2)), (2, 1, 1, dict(pad=1, dil=1)))
