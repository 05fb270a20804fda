"""Shared by test_groupdw_lists.py and test_gpu_groupdw_sweep.py: the case lists of the GroupDW variant sweep (every kernel that
usot_groupdw_multi_f32 / _lp / _dyn_f32 front, at every geometry, channel count, segment layout and operand stride the launcher
accepts), their seeded operands and the float64 reference, written from the operator's definition (include/usot_hip.h; reference
lib/models/connect.py:86-102): for each sample s, branch b and channel, correlate search map s // x_rep with template s, weight by
wsm[b] and sum the three branches.

Every operand of parts G, C, S, D, L, Y, P is integer-valued (-2 .. 2) and the branch weights are permutations of (0.5, 0.25, 1.0):
every product wsm z x, and every partial sum in any order, fused or not, is a multiple of 2^-2 bounded by 4 (25 + 15 + 15) = 220.  Any
correct fp32 kernel therefore returns the float64 result bit for bit, an fp16 output equals it exactly and a bf16 output is its
round-to-nearest-even: the bar of the GPU tests is EQUALITY.  Part B alone runs normal-distributed operands, at the existing
rel_err < 1e-5.

Operands with a pixel stride above C are NaN in every channel outside [co, co + C): a read outside the slice poisons the result.
Plain helper module."""
import collections
import functools
import zlib

import torch

CODES = [1, 5, 50, 52, 2, 3, 4, 6, 7, 8, 9]        # cols_per_thread: strips, three patch budgets, columns, LDS rows, ring, four LDS-DMA
PATCH, COLS, ROWS, DMA, PERSISTENT = [1, 5, 50, 52], [2], [3, 4], [6, 7, 8, 9], [8, 9]
GEO = ((5, 5), (3, 5), (5, 3))
WSM = [(0.5, 0.25, 1.0), (1.0, 0.5, 0.25), (0.25, 1.0, 0.5)]          # one triple per segment
V_MAX = 2
GRAIN = 0.25
BOUND = 4 * (25 + 15 + 15)

Case = collections.namedtuple('Case', 'part cols OH OW C segs layout')      # segs: ((S, x_rep), ...)
Seg = collections.namedtuple('Seg', 'x z wsm S x_rep x_cs x_co z_cs z_co')  # x, z: three CPU buffers [n][h][w][cs]

ONE = ((3, 1),)
SEGS3 = ((3, 1), (2, 2), (5, 3))                    # XS = 3, 1, 2; at C = 256 the sample pairs (2, 3) and (4, 5) straddle both borders
SEGS2 = ((1, 1), (1, 1))

# ---------------------------------------------------------------------------------------------------------------- G. geometry
G_PATCH_HW = [1, 4, 5, 6, 11]                       # squared: every 5-row / 5-column residue, non-square both ways
G_COL_OH, G_COL_OW = [1, 5, 31, 32], [1, 3, 4, 5, 9]
G_ROWS = [(3, ow) for ow in range(21, 31)] + [(oh, ow) for oh in (1, 2, 6, 29) for ow in (21, 25, 26, 30)]
G_DMA_OH, G_DMA_OW = [1, 2, 3, 4, 5, 6, 7, 25, 27, 28], [25, 27]
# auto (cols 0) at OH = 2, C = 128: (segments, OW, usot_groupdw_auto_variant(total, OW)).  The launcher turns the 6 of an
# all-x_rep-1 launch into 7; the query does not say so
AUTO = [(ONE, 25, 1), (((64, 1),), 25, 6), (((32, 1), (32, 2)), 25, 6), (((64, 1),), 23, 4)]
AUTO_C = 128


def geometries(code):
    if code in PATCH:
        return [(oh, ow) for oh in G_PATCH_HW for ow in G_PATCH_HW]
    if code in COLS:
        return [(oh, ow) for oh in G_COL_OH for ow in G_COL_OW]
    if code in ROWS:
        return list(G_ROWS)
    return [(oh, ow) for ow in G_DMA_OW for oh in G_DMA_OH]


def small_geo(code):
    """the variant's smallest part-G width at OH = 2: the geometry of parts C, S and D"""
    return (2, min(ow for _, ow in geometries(code)))


def g_cases(code):
    return [Case('G', code, oh, ow, 64, ONE, 'dense') for oh, ow in geometries(code)]


def auto_cases():
    return [(Case('G', 0, 2, ow, AUTO_C, segs, 'dense'), variant) for segs, ow, variant in AUTO]


# ---------------------------------------------------------------------------------------------------------------- C. channels
C_CHANNELS, C_SAMPLES = [64, 128, 192, 256, 320, 512], [1, 2, 5]


def c_cases(code):
    oh, ow = small_geo(code)
    return [Case('C', code, oh, ow, c, ((s, 1),), 'dense') for c in C_CHANNELS for s in C_SAMPLES]


# ---------------------------------------------------------------------------------------------------------------- S. segments
S_CHANNELS = [256, 128]


def s_cases(code):
    oh, ow = small_geo(code)
    return [Case('S', code, oh, ow, c, segs, 'dense') for c in S_CHANNELS for segs in (SEGS3, SEGS2)]


# ------------------------------------------------------------------------------------------------------- D. strides and offsets
def layout(name, C):
    """-> x_cs, x_co, z_cs, z_co (three values each)"""
    three = lambda v: (v, v, v)
    if name == 'dense':
        return three(C), three(0), three(C), three(0)
    if name in ('hi', 'lo'):                        # the engine's merged maps: one channel half of 2C-wide pixels
        co = C if name == 'hi' else 0
        return three(2 * C), three(co), three(2 * C), three(co)
    if name == 'branch':                            # per-branch values, all multiples of 4
        return (C + 4, 2 * C, C + 64), (4, C, 0), (C + 8, C, 2 * C), (8, 0, C)
    if name == 'odd':                               # dword loaders only
        return three(C + 1), three(1), three(C + 3), three(3)
    if name == 'oddz':                              # 16-byte search rows, dword taps
        return three(C), three(0), three(C + 3), three(3)
    raise KeyError(name)


D_SHAPES = [(64, ONE), (128, ((5, 3),))]            # the default shape, and one with a second channel group and shared maps
D_ODD = {1: 'odd', 2: 'odd', 4: 'odd', 5: 'odd', 50: 'odd', 52: 'odd', 3: 'oddz', 6: 'oddz', 7: 'oddz'}


def d_layouts(code):
    return ['hi', 'lo', 'branch'] + ([D_ODD[code]] if code in D_ODD else [])


def d_cases(code):
    oh, ow = small_geo(code)
    return [Case('D', code, oh, ow, c, segs, name) for name in d_layouts(code) for c, segs in D_SHAPES]


# ------------------------------------------------------------------------------------------------------------ L. 16-bit outputs
L_OW, L_OH, L_CHANNELS = [25, 27], [1, 6, 25], [64, 256]


def l_cases():
    return [Case('L', 0, oh, ow, c, segs, 'dense') for ow in L_OW for oh in L_OH for c in L_CHANNELS for segs in (ONE, SEGS3)]


# ------------------------------------------------------------------------------------------------------------ Y. run-time count
Y_GEO, Y_CHANNELS, Y_CAPACITY, Y_COUNTS = (2, 6), [128, 256], 5, [-3, 0, 1, 4, 5, 9]


def y_cases():
    assert SEGS3[-1][0] == Y_CAPACITY
    return [Case('Y', 1, Y_GEO[0], Y_GEO[1], c, SEGS3, 'dense') for c in Y_CHANNELS]


# ---------------------------------------------------------------------------------------------------------- P. persistent rounds
P_OW, P_OH, P_XREP = [25, 27], [1, 6], 3


def p_resident(cu):
    """the launcher's grid of the persistent kernels: two workgroups per CU, rounded down to a multiple of 8"""
    return 2 * cu - (2 * cu) % 8


def p_units(total, C):
    return 8 * ((total + 1) // 2) if C == 256 else (C // 64) * total


def p_counts(cu):
    """{C: sample counts}: unit counts G - 8, G, G + 8, 2 G + 8 at C = 256 (the odd and the even total of each), G - 1, G, G + 1,
    2 G + 1 at C = 64, and the first total past G at C = 192"""
    G = p_resident(cu)
    c256 = [n for units in (G - 8, G, G + 8, 2 * G + 8) for n in (units // 4 - 1, units // 4)]
    return {256: c256, 64: [G - 1, G, G + 1, 2 * G + 1], 192: [G // 3 + 1]}


def p_case(oh, ow, C, total):
    return Case('P', 8, oh, ow, C, ((total, P_XREP),), 'dense')


# -------------------------------------------------------------------------------------------------- B. real-valued operands
B_GEO, B_CHANNELS = [(6, 25), (27, 27)], [64, 256]


def b_cases():
    return [Case('B', 0, oh, ow, c, SEGS3, 'dense') for oh, ow in B_GEO for c in B_CHANNELS]


# ---------------------------------------------------------------------------------------------------------------- R. rejections
# (id, entry, code, OH, OW, what, argument): entry 'f32' | 'lp' | 'dyn'; C = 64, one segment of three samples unless `what` says
# otherwise.  Operands are always allocated for the geometry the descriptor claims.
def r_cases():
    out = []
    add = lambda *row: out.append(row)
    for c in (0, 32, 96):
        add('C%d' % c, 'f32', 1, 2, 6, 'field', ('C', c))
    add('OH0', 'f32', 1, 2, 6, 'field', ('OH', 0))
    add('OW0', 'f32', 1, 2, 6, 'field', ('OW', 0))
    add('nseg0', 'f32', 1, 2, 6, 'nseg', 0)
    add('nseg4', 'f32', 1, 2, 6, 'nseg', 4)
    for f, v in (('OH', 3), ('OW', 7), ('C', 128)):
        add('seg2_' + f, 'f32', 1, 2, 6, 'seg2', (f, v))
    add('S0', 'f32', 1, 2, 6, 'field', ('S', 0))
    add('x_rep0', 'f32', 1, 2, 6, 'field', ('x_rep', 0))
    add('null_x', 'f32', 1, 2, 6, 'elem', ('x', 1, None))
    add('null_z', 'f32', 1, 2, 6, 'elem', ('z', 2, None))
    add('null_out', 'f32', 1, 2, 6, 'field', ('out', None))
    add('hk', 'f32', 1, 2, 6, 'elem', ('hk', 1, 5))
    add('wk', 'f32', 1, 2, 6, 'elem', ('wk', 2, 5))
    for code in (-1, 10, 51):
        add('code%d' % code, 'f32', code, 2, 6, None, None)
    add('cols_oh33', 'f32', 2, 33, 1, None, None)
    for code in ROWS:
        for ow in (20, 31):
            add('v%d_ow%d' % (code, ow), 'f32', code, 2, ow, None, None)
    for code in DMA:
        add('v%d_ow26' % code, 'f32', code, 2, 26, None, None)
    for dt in (1, 2):
        add('lp%d_ow26' % dt, 'lp', 0, 2, 26, 'out_dtype', dt)
    for dt in (0, 3):
        add('lp_dtype%d' % dt, 'lp', 0, 2, 25, 'out_dtype', dt)
    for code in DMA + [3]:
        for op in ('x', 'z') if code in PERSISTENT else ('x',):
            add('v%d_%s_co2' % (code, op), 'f32', code, 2, 25, 'elem', (op + '_co', 1, 2))
            add('v%d_%s_cs' % (code, op), 'f32', code, 2, 25, 'elem', (op + '_cs', 2, 64 + 2))
            add('v%d_%s_base' % (code, op), 'f32', code, 2, 25, 'advance', (op, 0, 4))
    for code in CODES[1:]:
        add('dyn_v%d' % code, 'dyn', code, 2, small_geo(code)[1], None, None)
    add('dyn_misaligned', 'dyn', 1, 2, 6, 'count_advance', 2)
    return out


# ------------------------------------------------------------------------------------------------------- operands and reference
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def embed(t, cs, co):
    """[..][C] -> [..][cs] with the data in channels [co, co + C) and NaN everywhere else"""
    C = t.shape[-1]
    if cs == C and co == 0:
        return t
    buf = torch.full(t.shape[:-1] + (cs,), float('nan'), dtype=t.dtype)
    buf[..., co:co + C] = t
    return buf


def segment(OH, OW, C, S, x_rep, k, name='dense', real=False):
    """seeded segment k of a launch: three search maps [ceil(S / x_rep)][OH + hk - 1][OW + wk - 1], three templates [S][hk][wk]"""
    gen = torch.Generator().manual_seed(_seed(OH, OW, C, S, x_rep, k, real))
    if real:
        draw = lambda shape: torch.randn(shape, generator=gen)
        wsm = tuple(float(v) for v in torch.softmax(torch.randn(3, generator=gen), 0))
    else:
        draw = lambda shape: torch.randint(-V_MAX, V_MAX + 1, shape, generator=gen).float()
        wsm = WSM[k % 3]
    XS = -(-S // x_rep)
    x_cs, x_co, z_cs, z_co = layout(name, C)
    xs = [embed(draw((XS, OH + hk - 1, OW + wk - 1, C)), x_cs[b], x_co[b]) for b, (hk, wk) in enumerate(GEO)]
    zs = [embed(draw((S, hk, wk, C)), z_cs[b], z_co[b]) for b, (hk, wk) in enumerate(GEO)]
    return Seg(xs, zs, wsm, S, x_rep, x_cs, x_co, z_cs, z_co)


MUTATIONS = ['weights', 'roles', 'tap_col', 'tap_row', 'map', 'group', 'template', 'x_co', 'last_col']


def meaningful(mut, case):
    """whether the deliberate mistake `mut` of ref64 can change this case's result at all"""
    if mut == 'map':                                # map s for s // x_rep: needs shared maps and a second map to go wrong on
        return any(rep > 1 and -(-s // rep) > 1 for s, rep in case.segs)
    if mut == 'group':                              # channel group g + 1 mod C / 64
        return case.C > 64
    if mut == 'template':                           # the neighbouring sample's template
        return any(s > 1 for s, _ in case.segs)
    if mut == 'x_co':
        return any(layout(case.layout, case.C)[1])
    return True


def ref64(seg, OH, OW, C, mut=None):
    """float64 [S][OH][OW][C] of one segment from the operator's definition; x_cs / x_co / z_cs / z_co are honoured by slicing.
    mut: one of MUTATIONS - a wrong kernel, for the list test"""
    S = seg.S
    w = list(seg.wsm)
    if mut == 'weights':
        w[0], w[1] = w[1], w[0]
    out = torch.zeros(S, OH, OW, C, dtype=torch.float64)
    for b, (hk, wk) in enumerate(GEO):
        co = 0 if mut == 'x_co' else seg.x_co[b]
        x = seg.x[b][..., co:co + C].double()
        zb = 3 - b if mut == 'roles' and b else b   # the 3x5 branch walks the 5x3 template's fifteen taps and the reverse
        z = seg.z[zb][..., seg.z_co[zb]:seg.z_co[zb] + C].double().reshape(S, hk, wk, C)
        if mut == 'template':
            z = z.roll(-1, 0)
        which = torch.arange(S)
        which = which.clamp(max=x.shape[0] - 1) if mut == 'map' else which // seg.x_rep
        xr = x[which]
        for u in range(hk):
            for v in range(wk):
                du = 1 if mut == 'tap_row' and (b, u, v) == (0, 0, 0) else 0
                dv = 1 if mut == 'tap_col' and (b, u, v) == (0, 0, 0) else 0
                out.addcmul_(xr[:, u + du:u + du + OH, v + dv:v + dv + OW, :], z[:, u, v, :][:, None, None, :], value=w[b])
    if mut == 'group':
        out = out.roll(-64, 3)
    if mut == 'last_col':
        out[:, :, -1, :] = 0
    return out


@functools.lru_cache(maxsize=None)
def build(case, real=False):
    """-> (segments, float64 references) of a case; shared between tests, read-only"""
    segs = [segment(case.OH, case.OW, case.C, s, rep, k, case.layout, real) for k, (s, rep) in enumerate(case.segs)]
    return segs, [ref64(g, case.OH, case.OW, case.C) for g in segs]


def stored(ref, dtype):
    """what a correct kernel stores for the float64 value: itself in fp32 and fp16, its round-to-nearest-even in bf16"""
    return ref.float().to(dtype)
