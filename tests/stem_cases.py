"""Shared by test_stem_lists.py and test_gpu_stem_sweep.py: the case lists of the stem and max-pool sweep (usot_stem_conv_mu_f32,
usot_maxpool3x3s2_f32 / _lp, usot_stem_pool_mu_f32 / _ind_f32, usot_stem_pool_lp at every tile residue and strip length), their seeded
operands and the float64 reference, written from the operator's definition (include/usot_hip.h; reference lib/models/modules.py:70-74,
138-141): y = max_pool2d(relu(conv2d(x, w, b, stride 2)), 3, 2, 1).

Every comparison of the GPU tests is an EQUALITY, because of the operands:
  crops    multiples of 1/4 in [0, 255.75], every image of a batch different.  With MU = (-104, 117, -123) x - mu reaches 378.75 =
           1515 quarter units: exact in fp32 and in fp16 (< 2048), and in bf16 exact as hi + lo with a non-zero lo for most values
           (asserted: the second MFMA chain of the bf16 kernel carries real data).
  filters  multiples of 1/4 with |w| <= 1, biases multiples of 1/4: every product is a multiple of 1/16 and every partial sum of
           w (x - mu) + (b + sum w mu), in any order, is bounded by BOUND = max_c sum |w| 378.75 + |b + sum w mu| < 2^24 / 16: exact in
           fp32 (asserted), and below the fp16 maximum.  The folded bias b + sum w mu is exact in fp32 as well (asserted).
  A correct fp32 kernel therefore returns the float64 value bit for bit, a 16-bit output its round-to-nearest-even (rounding is
  monotonic: the pool of the rounded stem map is the rounding of the pooled map).

The 64 filters come in four families, channel c belonging to family c % 4, so that every channel block, quad and 8-channel piece
of a kernel holds all four:
  0  negative   weights -1/4 .. -1/2 on 44 taps, among them the whole last row and column of the window, bias +4096: the output
                stays above 0 and GROWS with every real pixel that goes missing - a pool that admits a halo stem pixel past OH / OW,
                or a patch padded wrongly, raises it
  1  positive   all 147 taps in 1/4 .. 1: a dropped or zeroed real pixel lowers it
  2  mixed      all taps in -1 .. 1, biases in -512 .. 512
  3  single     weight 1 at one (ci, kh, kw), bias 128: the four corners and the centre of the window for each input channel and one
                off-diagonal tap; the output is the crop at a known offset plus 128

Plain helper module."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

MU = (-104.0, 117.0, -123.0)
NO_MU = (0.0, 0.0, 0.0)
GRAIN = 1.0 / 16
X_MAX = 378.75                                      # max |x - mu|

Case = collections.namedtuple('Case', 'H W N B')    # N images gathered from B distinct base images (B == N: the batch itself)

# ------------------------------------------------------------------------------------------------------------------ geometries
ROWS = [(h, 30) for h in range(7, 46)]              # PH 1 .. 10, OH 1 .. 20
COLS = [(18, w) for w in range(7, 77)]              # PW 1 .. 18, OW 1 .. 35
CORNERS = [(7, 7), (8, 8), (7, 76), (45, 7), (44, 75), (45, 76)]
PRODUCTION = [127, 255, 271]
IND = [(7, 7), (18, 37), (45, 76)]                  # usot_stem_pool_ind_f32: one pooled pixel, two tiles, the largest corner


def out_hw(H, W):
    """-> OH, OW, PH, PW"""
    OH, OW = (H - 7) // 2 + 1, (W - 7) // 2 + 1
    return OH, OW, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1


def row_cases():
    return [Case(h, w, 2, 2) for h, w in ROWS]


def col_cases():
    return [Case(h, w, 2, 2) for h, w in COLS]


def corner_cases():
    return [Case(h, w, 3, 3) for h, w in CORNERS]


def production_cases():
    return [Case(s, s, 1, 1) for s in PRODUCTION]


def sweep_cases():
    return row_cases() + col_cases() + corner_cases() + production_cases()


def ind_cases():
    return [Case(h, w, 2, 2) for h, w in IND]


# --------------------------------------------------------------------------------------------------------------- strip cases
STRIP_BASE = 5                                      # distinct images of a strip case
STRIP_WIDE = (21, 153)                              # PH 4, PW 37: one tile row of five tiles, the last with five live columns
STRIP_TALL = (39, 175)                              # PH 9, PW 43: three tile rows of six tiles, the last with three live columns


def strip_of(N, PH, PW):
    """the strip length a usot_stem_pool_lp launch takes: the launcher's own host-side query"""
    from usot_amd import hip
    return int(hip.lib().usot_stem_pool_lp_strip(int(N), int(PH), int(PW)))


def tiles(PH, PW):
    """-> tiles_x, tiles_y of the 4 x 8 pooled tile"""
    return -(-PW // 8), -(-PH // 4)


@functools.lru_cache(maxsize=None)
def fewest_images(shape, strip):
    """the smallest batch at which `shape` reaches `strip`"""
    _, _, PH, PW = out_hw(*shape)
    n = 1
    while strip_of(n, PH, PW) < strip:
        n += 1
    return n


def strip_cases():
    """(case, why).  The expected strip of each is strip_of(): test_stem_lists.py pins 4, 2, 4 and 1."""
    return [(Case(STRIP_WIDE[0], STRIP_WIDE[1], 768, STRIP_BASE), 'strip 4: workgroups of 4 + 1 tiles'),
            (Case(STRIP_WIDE[0], STRIP_WIDE[1], 767, STRIP_BASE), 'strip 2, one image below the threshold: 2 + 2 + 1 tiles'),
            (Case(STRIP_TALL[0], STRIP_TALL[1], fewest_images(STRIP_TALL, 4), STRIP_BASE), 'strip 4: 4 + 2 tiles in three tile rows'),
            (Case(18, 76, 2, 2), 'strip 1: a sweep shape')]


def case_strip(case):
    _, _, PH, PW = out_hw(case.H, case.W)
    return strip_of(case.N, PH, PW)


# ------------------------------------------------------------------------------------------------------------ max-pool alone
POOL_HW = [(h, w) for h in range(1, 8) for w in range(1, 8)]
POOL_C_F32, POOL_C_LP, POOL_N = [4, 64, 68], [8, 64, 72], 2
POOL_BIG = (9, 121, 121, 256)                       # N, H, W, C: 2 143 296 channel quads against a grid of 8192 x 256 threads
POOL_CAP = 8192 * 256


def pool_input(N, H, W, C, dtype=torch.float32):
    """NHWC multiples of 1/4 in [-32, 31.75] (exact in bf16 and fp16); in every odd image the first row is one value, in every image
    the last column of channel 0 is: ties in both directions"""
    gen = torch.Generator().manual_seed(_seed('pool', N, H, W, C))
    x = torch.randint(-128, 128, (N, H, W, C), generator=gen, dtype=torch.int16).float() / 4
    x[1::2, 0] = -3.0
    x[:, :, -1, 0] = -31.5
    return x.to(dtype)


def pool64(x, dtype=torch.float64):
    """max_pool2d(x, 3, 2, 1) of an NHWC tensor, computed in `dtype` (a maximum rounds nothing: fp32 serves the one large case)"""
    return F.max_pool2d(x.to(dtype).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------- operands
def _seed(*key):
    return zlib.crc32(repr(key).encode())


SINGLE_TAPS = [(ci, kh, kw) for ci in range(3) for kh, kw in ((0, 0), (0, 6), (6, 0), (6, 6), (3, 3))] + [(1, 2, 5)]


@functools.lru_cache(maxsize=None)
def filters():
    """-> w [64][3][7][7], b [64] (float64); family of channel c = c % 4"""
    gen = torch.Generator().manual_seed(_seed('stem filters'))
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
    b = torch.zeros(64, dtype=torch.float64)
    edge = torch.zeros(3, 7, 7, dtype=torch.bool)
    edge[0, 6, :] = edge[0, :, 6] = edge[2, 6, :] = edge[2, :, 6] = True           # 26 taps: the last row and column, ci 0 and 2
    rest = (~edge).reshape(-1).nonzero().reshape(-1)
    for k in range(16):
        neg = torch.zeros(147, dtype=torch.float64)
        neg[edge.reshape(-1)] = -0.25
        pick = rest[torch.randperm(rest.numel(), generator=gen)[:18]]
        neg[pick] = -torch.randint(1, 3, (18,), generator=gen).double() / 4        # sum |w| <= 6.5 + 9: 15.5 * 255.75 < 4096
        w[4 * k + 0] = neg.reshape(3, 7, 7)
        b[4 * k + 0] = 4096.0
        w[4 * k + 1] = torch.randint(1, 5, (3, 7, 7), generator=gen).double() / 4
        b[4 * k + 1] = torch.randint(-64, 65, (1,), generator=gen).double().item() / 4
        w[4 * k + 2] = torch.randint(-4, 5, (3, 7, 7), generator=gen).double() / 4
        b[4 * k + 2] = torch.randint(-2048, 2049, (1,), generator=gen).double().item() / 4
        w[(4 * k + 3,) + SINGLE_TAPS[k]] = 1.0
        b[4 * k + 3] = 128.0
    return w, b


def folded_bias(mu=MU):
    """b + sum w mu in float64: what a kernel that convolves x - mu is handed"""
    w, b = filters()
    return b + (w * torch.tensor(mu, dtype=torch.float64).view(1, 3, 1, 1)).sum((1, 2, 3))


def bound(mu=MU):
    """max_c sum |w| max|x - mu| + |folded bias|: no partial sum of a kernel, in any order, exceeds it"""
    w, _ = filters()
    xmax = max(max(abs(0.0 - m), abs(255.75 - m)) for m in mu)
    return float((w.abs().sum((1, 2, 3)) * xmax + folded_bias(mu).abs()).max())


def packed():
    """[147][64] fp32, row (ci * 7 + kh) * 7 + kw: the bank usot_stem_conv_mu_f32 reads and engine.pack_stem_* swizzle"""
    w, _ = filters()
    return w.permute(1, 2, 3, 0).reshape(147, 64).float().contiguous()


def _rows(frag, ch, row, tap):
    rows = torch.full((24, 8, 64), float('nan'))
    rows[row.reshape(-1), tap.reshape(-1), ch.reshape(-1)] = frag.float().reshape(-1)
    return rows[:21, :7].reshape(147, 64), torch.cat([rows[21:].reshape(-1), rows[:21, 7].reshape(-1)])


def unpack_f32(frag):
    """[4][48][64] of engine.pack_stem_f32 read the way stem_pool_f32_kernel reads it - k-step s of lane (l15, quad) in channel
    block cb is channel cb * 16 + l15, k-row s / 2, tap (s & 1) * 4 + quad -> ([147][64], the entries the kernel needs to be zero)"""
    cb, s, lane = torch.meshgrid(torch.arange(4), torch.arange(48), torch.arange(64), indexing='ij')
    return _rows(frag, cb * 16 + (lane & 15), s // 2, (s & 1) * 4 + (lane >> 4))


def unpack_lp(frag):
    """[4][6][64][8] of engine.pack_stem_lp read the way stem_pool_lp_kernel reads it - element e of k-step ks of lane (l15, quad)
    in channel block cb is channel cb * 16 + l15, k-row 4 * ks + quad, tap e -> ([147][64], the entries the kernel needs to be zero)"""
    cb, ks, lane, e = torch.meshgrid(torch.arange(4), torch.arange(6), torch.arange(64), torch.arange(8), indexing='ij')
    return _rows(frag, cb * 16 + (lane & 15), 4 * ks + (lane >> 4), e)


@functools.lru_cache(maxsize=None)
def crops(case):
    """the B base images [B][3][H][W] fp32 of a case, all different"""
    gen = torch.Generator().manual_seed(_seed('crop', case.H, case.W, case.B))
    x = torch.randint(0, 1024, (case.B, 3, case.H, case.W), generator=gen).float() / 4
    assert all(not torch.equal(x[i], x[j]) for i in range(case.B) for j in range(i))
    return x


@functools.lru_cache(maxsize=None)
def index(case):
    """which base image each of the N batch images is: the identity, or a seeded non-periodic draw that uses every base image"""
    if case.B == case.N:
        return torch.arange(case.N)
    gen = torch.Generator().manual_seed(_seed('index', case.H, case.W, case.N, case.B))
    idx = torch.randint(0, case.B, (case.N,), generator=gen)
    idx[:case.B] = torch.arange(case.B)
    assert all(not torch.equal(idx, idx.roll(p)) for p in range(1, min(case.N, 65)))
    return idx


# --------------------------------------------------------------------------------------------------------------------- reference
MUTATIONS = ['pool_row', 'pool_col', 'tap_row', 'tap_col', 'channel', 'mu_pad', 'last_col', 'last_row', 'image', 'strip_stale']


def meaningful(mut, case):
    """whether the deliberate mistake `mut` of ref64 can change this case's pooled map at all"""
    OH, OW, PH, PW = out_hw(case.H, case.W)
    if mut == 'pool_row':                           # the last pooled row's window ends at stem row OH only when OH is odd
        return OH % 2 == 1
    if mut == 'pool_col':
        return OW % 2 == 1
    if mut == 'mu_pad':
        return OH % 2 == 1 or OW % 2 == 1
    if mut == 'image':
        return case.N > 1
    if mut == 'strip_stale':
        return case_strip(case) > 1 and tiles(PH, PW)[0] > 1
    return True


def ref64(case, mut=None, mu=MU):
    """float64 (stem map [B][OH][OW][64], pooled map [B][PH][PW][64]) of the case's BASE images from the operator's definition; image
    n of the batch is base image index(case)[n] (expected() gathers).  mu: what the kernel under test subtracts while it stages the
    crop - it enters the true result nowhere, only the value a halo stem pixel has in pool_row / pool_col.
    mut: one of MUTATIONS - a subtly wrong kernel, for the list test:
      pool_row, pool_col  the pool admits stem row OH / column OW, computed from the kernel's zero-padded patch of x - mu
      mu_pad              the same slip in both axes of a kernel that pads the raw crop: the halo pixels see x = 0, i.e. a patch
                          filled with -mu.  (By itself a wrong padding value is invisible: no valid output of this pad-0 convolution
                          reads padding.)
      tap_row, tap_col    tap (ci 0, kh 0, kw 0) reads the pixel one row / column further on
      channel             input channels 0 and 1 swapped
      last_col, last_row  the last input column / row a valid output reads comes in as zero
      image               image n reads image n - 1 (of the batch: applied by expected(); here for B == N)
      strip_stale         a tile that is not the first of its strip returns the previous tile's pooled values"""
    assert mut is None or mut in MUTATIONS
    w, b = filters()
    x = crops(case).double()
    H, W = case.H, case.W
    OH, OW, PH, PW = out_hw(H, W)
    if mut == 'channel':
        x = x[:, [1, 0, 2]]
    if mut == 'last_col':
        x = x.clone()
        x[..., 2 * (OW - 1) + 6] = 0
    if mut == 'last_row':
        x = x.clone()
        x[..., 2 * (OH - 1) + 6, :] = 0
    if mut in ('tap_row', 'tap_col'):
        w = w.clone()
        if mut == 'tap_row':
            w[:, 0, 1, 0] += w[:, 0, 0, 0]
        else:
            w[:, 0, 0, 1] += w[:, 0, 0, 0]
        w[:, 0, 0, 0] = 0
    if mut == 'image' and case.B == case.N:
        x = x.roll(1, 0)
    # the image continued past its edge with what the kernel's padding stands for: x - mu = 0, or x = 0 for mu_pad
    fill = torch.zeros(3, dtype=torch.float64) if mut == 'mu_pad' else torch.tensor(mu, dtype=torch.float64)
    ext = fill.view(1, 3, 1, 1).expand(x.shape[0], 3, 2 * OH + 7, 2 * OW + 7).clone()
    ext[:, :, :H, :W] = x
    full = torch.relu(F.conv2d(ext, w, b, stride=2))                 # [B][64][OH + 1][OW + 1]: the halo row and column included
    assert full.shape[-2:] == (OH + 1, OW + 1)
    stem = full[:, :, :OH, :OW]
    rows = OH + 1 if mut in ('pool_row', 'mu_pad') else OH
    cols = OW + 1 if mut in ('pool_col', 'mu_pad') else OW
    pooled = F.max_pool2d(full[:, :, :rows, :cols], 3, 2, 1)[:, :, :PH, :PW]
    assert pooled.shape[-2:] == (PH, PW)
    if mut == 'strip_stale':
        strip, tx = case_strip(case), tiles(PH, PW)[0]
        true = pooled
        pooled = true.clone()
        for t in range(tx):
            if t % strip:
                n = min(8, PW - 8 * t)
                pooled[..., 8 * t:8 * t + n] = true[..., 8 * (t - 1):8 * (t - 1) + n]
    return stem.permute(0, 2, 3, 1).contiguous(), pooled.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def build(case):
    """-> (stem, pooled) float64 references of the case's base images; shared between tests, read-only"""
    stem, pooled = ref64(case)
    for t in (stem, pooled):                        # every value a multiple of 1/16 below the bound: fp32 holds it exactly
        assert torch.equal(t, (t / GRAIN).round() * GRAIN) and float(t.max()) <= bound() and torch.equal(t, t.float().double())
    return stem, pooled


def stored(ref, dtype):
    """what a correct kernel stores for the float64 value: itself in fp32, its round-to-nearest-even in fp16 and bf16"""
    return ref.float().to(dtype)


def expected(case, ref, mut=None):
    """the batch's map from the base images' map `ref` (one of ref64's pair)"""
    idx = index(case)
    if mut == 'image' and case.B != case.N:
        idx = idx.roll(1)
    return ref if case.B == case.N else ref[idx]


# --------------------------------------------------------------------------------------------------------------------- refusals
# (id, change): entries 'conv' (usot_stem_conv_f32, usot_stem_conv_mu_f32), 'pool' (usot_stem_pool_f32, _ind_f32, _mu_f32), 'lp'
# (usot_stem_pool_lp); the base launch is R_SHAPE with operands allocated for it
R_SHAPE = Case(18, 30, 2, 2)
R_ALL = [('OH+1', ('OH', 1)), ('OW+1', ('OW', 1)), ('OH-1', ('OH', -1)), ('OW-1', ('OW', -1)), ('H6', ('H', 6)), ('W6', ('W', 6)),
         ('N0', ('N', 0)), ('N65536', ('N', 65536))]
R_POOLED = [('PH+1', ('PH', 1)), ('PW+1', ('PW', 1)), ('PH-1', ('PH', -1)), ('PW-1', ('PW', -1))]
R_ALIGN = {'conv': ['y', 'w'], 'pool': ['y', 'bias'], 'lp': ['y', 'bias', 'w']}       # the operands each launcher checks


def r_cases(entry):
    rows = R_ALL + (R_POOLED if entry != 'conv' else [])
    rows = rows + [('%s+4' % a, ('advance', a)) for a in R_ALIGN[entry]]
    return rows + ([('dtype3', ('dtype', 3)), ('dtype-1', ('dtype', -1))] if entry == 'lp' else [])
