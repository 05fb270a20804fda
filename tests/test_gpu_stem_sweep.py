"""GPU: the kernels in front of the conv stack - the 7x7 stem (usot_stem_conv_mu_f32), the 3x3/s2 max-pool (usot_maxpool3x3s2_f32 /
_lp) and the two fused stem + pool kernels (usot_stem_pool_mu_f32 / _ind_f32, usot_stem_pool_lp in its three modes) - against the
float64 reference of tests/stem_cases.py:

  every geometry of the sweep (H 7 .. 45 at W 30, W 7 .. 76 at H 18, six corners, the production sizes 127, 255, 271): every residue
  of the 4 x 4 and 4 x 8 pooled tiles and of the unfused stem's 8 x 16 tile at one and at several tiles, both parities of H, W, OH
  and OW, H != W;
  the low-precision kernel's strips of 4, 2 and 1 tiles, each strip it reaches asserted from usot_stem_pool_lp_strip, a ragged
  last workgroup at 4 and at 2;
  the max-pool alone at H, W 1 .. 7 and one fp32 map past the launcher's cap of 8192 blocks (a second pass of the grid-stride loop);
  everything the launchers refuse: USOT_EINVAL and the output's bits untouched.

The operands are exact (stem_cases.py), so every comparison is EQUALITY: bit for bit in fp32, the round-to-nearest-even of the float64
value in fp16 and bf16.  Outputs are NaN-prefilled between canaries (tests/guarded.py), inputs lie between NaNs, every test ends
with guarded.check.

One item loops over its list and reports every failing case, not the first one.  The lists are asserted by tests/test_stem_lists.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import stem_cases as sc  # noqa: E402
from test_gpu_groupdw_sweep import mismatch, same_bits  # noqa: E402
from usot_amd import hip  # noqa: E402
from usot_amd.engine import pack_stem_f32, pack_stem_lp  # noqa: E402

DEV = 'cuda:0'
EINVAL = -1
LISTS = {'rows': sc.row_cases, 'cols': sc.col_cases, 'corners_production': lambda: sc.corner_cases() + sc.production_cases()}
LIST = [pytest.param(k, id=k) for k in LISTS]
MUS = [pytest.param(sc.MU, id='mu'), pytest.param(sc.NO_MU, id='no_mu')]
# usot_stem_pool_lp's dtype, the fragments' type, the output's type
MODES = [pytest.param(0, torch.bfloat16, torch.bfloat16, id='bf16'), pytest.param(1, torch.float16, torch.float16, id='fp16'),
         pytest.param(2, torch.float16, torch.bfloat16, id='bf16_out_fp16_math')]

_ops = {}


def ops(name, mu=None):
    """guarded device copies of the filter bank in its four layouts and of the bias as each mu needs it; made once"""
    key = (name, mu)
    if key not in _ops:
        if name == 'bias':
            t = sc.folded_bias(mu).float()
        elif name == 'bank':
            t = sc.packed()
        elif name == 'f32':
            t = pack_stem_f32(sc.packed())
        else:
            t = pack_stem_lp(sc.packed(), name)
        _ops[key] = guarded.put(t, DEV)
    return _ops[key]


def geometry(case):
    return (case.N, case.H, case.W) + sc.out_hw(case.H, case.W)


def stem_conv(x, y, case, mu):
    N, H, W, OH, OW, _, _ = geometry(case)
    return hip.lib().usot_stem_conv_mu_f32(hip.stream(), hip.ptr(x), hip.ptr(ops('bank')), hip.ptr(ops('bias', mu)), hip.ptr(y),
                                           N, H, W, OH, OW, *mu)


def maxpool(x, y, lp=None):
    N, H, W, Cc = x.shape
    if lp is None:
        return hip.lib().usot_maxpool3x3s2_f32(hip.stream(), hip.ptr(x), hip.ptr(y), N, H, W, Cc, y.shape[1], y.shape[2])
    return hip.lib().usot_maxpool3x3s2_lp(hip.stream(), hip.ptr(x), hip.ptr(y), N, H, W, Cc, y.shape[1], y.shape[2], lp)


def stem_pool(x, y, case, mu, xptr=None):
    return hip.lib().usot_stem_pool_mu_f32(hip.stream(), hip.ptr(x), hip.ptr(ops('f32')), hip.ptr(ops('bias', mu)), hip.ptr(y),
                                           *geometry(case), xptr, *mu)


def stem_pool_lp(x, y, case, mode, wdtype, mu=sc.MU):
    return hip.lib().usot_stem_pool_lp(hip.stream(), hip.ptr(x), hip.ptr(ops(wdtype)), hip.ptr(ops('bias', mu)), hip.ptr(y),
                                       *geometry(case), mode, *mu)


def two_launches(case, x, mu):
    """the unfused path -> (return codes, stem map, pooled map)"""
    N, _, _, OH, OW, PH, PW = geometry(case)
    stem = guarded.alloc((N, OH, OW, 64), torch.float32, DEV)
    pooled = guarded.alloc((N, PH, PW, 64), torch.float32, DEV)
    return (stem_conv(x, stem, case, mu), maxpool(stem, pooled)), stem, pooled


def finish(what, start, launches, bad):
    torch.cuda.synchronize()
    guarded.check(start)
    print('%s: %d cases, %d failing' % (what, launches, len(bad)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ fp32, every geometry
@pytest.mark.parametrize('mu', MUS)
@pytest.mark.parametrize('which', LIST)
def test_stem_then_pool_f32(which, mu):
    """usot_stem_conv_mu_f32's map equals the float64 stem map and usot_maxpool3x3s2_f32 of it the pooled one, with and without mu."""
    start = guarded.registry_size()
    cases, bad = LISTS[which](), []
    for case in cases:
        want_stem, want_pooled = sc.build(case)
        rcs, stem, pooled = two_launches(case, guarded.put(sc.crops(case), DEV), mu)
        bad += [(tuple(case), 'return codes %s' % (rcs,))] if rcs != (0, 0) else []
        bad += [(tuple(case), 'stem', m) for m in [mismatch(stem, sc.stored(want_stem, torch.float32))] if m]
        bad += [(tuple(case), 'pool', m) for m in [mismatch(pooled, sc.stored(want_pooled, torch.float32))] if m]
    finish('stem + pool %s' % which, start, len(cases), bad)


@pytest.mark.parametrize('mu', MUS)
@pytest.mark.parametrize('which', LIST)
def test_stem_pool_f32(which, mu):
    """usot_stem_pool_mu_f32 equals the float64 pooled map and is bit-equal to the two-launch path, with and without mu."""
    start = guarded.registry_size()
    cases, bad = LISTS[which](), []
    for case in cases:
        _, want = sc.build(case)
        x = guarded.put(sc.crops(case), DEV)
        y = guarded.alloc(want.shape, torch.float32, DEV)
        rc = stem_pool(x, y, case, mu)
        rcs, _, pooled = two_launches(case, x, mu)
        bad += [(tuple(case), 'return codes %s' % ((rc,) + rcs,))] if (rc,) + rcs != (0, 0, 0) else []
        bad += [(tuple(case), m) for m in [mismatch(y, sc.stored(want, torch.float32))] if m]
        bad += [(tuple(case), 'differs from the two-launch path')] if not same_bits(y, pooled) else []
    finish('fused fp32 %s' % which, start, len(cases), bad)


def test_stem_pool_ind_f32():
    """usot_stem_pool_ind_f32: with the crop's address in a device word pair the baked x (a NaN-filled decoy) is not read; with a
    zero address word, and with no word at all, the baked x is."""
    start = guarded.registry_size()
    bad = []
    for case in sc.ind_cases():
        _, want = sc.build(case)
        want = sc.stored(want, torch.float32)
        real = guarded.put(sc.crops(case), DEV)
        decoy = guarded.alloc(real.shape, torch.float32, DEV)
        assert bool(torch.isnan(decoy).all())
        word = guarded.alloc((2,), torch.int32, DEV, 'zero')
        signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        launch = lambda x, y, w: hip.lib().usot_stem_pool_ind_f32(hip.stream(), hip.ptr(x), hip.ptr(ops('f32')),
                                                                  hip.ptr(ops('bias', sc.NO_MU)), hip.ptr(y), *geometry(case), hip.ptr(w))
        for what, x, addr, w in (('address word', decoy, real.data_ptr(), word), ('zero word', real, 0, word), ('no word', real, 0, None)):
            word.copy_(torch.tensor([signed(addr & 0xffffffff), signed(addr >> 32)], dtype=torch.int32))
            y = guarded.alloc(want.shape, torch.float32, DEV)
            rc = launch(x, y, w)
            bad += [(tuple(case), what, 'return code %d' % rc)] if rc else []
            bad += [(tuple(case), what, m) for m in [mismatch(y, want)] if m]
    finish('fused fp32, indirect crop', start, 9, bad)


# ------------------------------------------------------------------------------------------------------- low precision, three modes
@pytest.mark.parametrize('mode,wdtype,dtype', MODES)
@pytest.mark.parametrize('which', LIST)
def test_stem_pool_lp(which, mode, wdtype, dtype):
    """usot_stem_pool_lp on every geometry (all of them strips of one tile): the round-to-nearest-even of the float64 pooled map."""
    start = guarded.registry_size()
    cases, bad = LISTS[which](), []
    for case in cases:
        _, want = sc.build(case)
        y = guarded.alloc(want.shape, dtype, DEV)
        rc = stem_pool_lp(guarded.put(sc.crops(case), DEV), y, case, mode, wdtype)
        bad += [(tuple(case), 'return code %d' % rc)] if rc else []
        bad += [(tuple(case), m) for m in [mismatch(y, sc.stored(want, dtype))] if m]
    finish('fused lp %s' % which, start, len(cases), bad)


STRIPS = [4, 2, 4, 1]


@pytest.mark.parametrize('mode,wdtype,dtype', MODES)
@pytest.mark.parametrize('k', range(len(STRIPS)), ids=['wide768', 'wide767', 'tall256', 'small'])
def test_stem_pool_lp_strips(k, mode, wdtype, dtype):
    """The strip walk: workgroups of 4 + 1 tiles, of 2 + 2 + 1 one image below that threshold, of 4 + 2 in three tile rows, and of one.
    The batch is gathered from five base images by a non-periodic index; two launches into the same buffers are bit-equal and
    right; the strip each case takes is the launcher's own (usot_stem_pool_lp_strip)."""
    case, why = sc.strip_cases()[k]
    assert sc.case_strip(case) == STRIPS[k], why
    start = guarded.registry_size()
    _, want = sc.build(case)
    idx = sc.index(case).to(DEV)
    want = sc.stored(want, dtype).to(DEV)[idx]
    x = guarded.alloc((case.N, 3, case.H, case.W), torch.float32, DEV, 'none')
    x.copy_(sc.crops(case).to(DEV)[idx])
    y = guarded.alloc(want.shape, dtype, DEV)
    bad = []
    for run in range(2):
        rc = stem_pool_lp(x, y, case, mode, wdtype)
        bad += [(run, 'return code %d' % rc)] if rc else []
        got = y.clone()
        bad += [(run, m) for m in [mismatch(got, want)] if m]
        bad += [(run, 'differs from the first launch')] if run and not same_bits(got, first) else []
        first = got
    finish('fused lp strip %d (%s)' % (STRIPS[k], why), start, 2, bad)


# ------------------------------------------------------------------------------------------------------------------ max-pool alone
def test_maxpool_f32_sweep():
    """usot_maxpool3x3s2_f32 at H, W 1 .. 7 and 4, 64, 68 channels equals max_pool2d."""
    start = guarded.registry_size()
    bad = []
    for Cc in sc.POOL_C_F32:
        for H, W in sc.POOL_HW:
            x = sc.pool_input(sc.POOL_N, H, W, Cc)
            want = sc.pool64(x).float()
            y = guarded.alloc(want.shape, torch.float32, DEV)
            rc = maxpool(guarded.put(x, DEV), y)
            bad += [((H, W, Cc), 'return code %d' % rc)] if rc else []
            bad += [((H, W, Cc), m) for m in [mismatch(y, want)] if m]
    finish('max-pool fp32', start, len(sc.POOL_C_F32) * len(sc.POOL_HW), bad)


@pytest.mark.parametrize('lp,dtype', [pytest.param(0, torch.bfloat16, id='bf16'), pytest.param(1, torch.float16, id='fp16')])
def test_maxpool_lp_sweep(lp, dtype):
    """usot_maxpool3x3s2_lp at H, W 1 .. 7 and 8, 64, 72 channels equals max_pool2d."""
    start = guarded.registry_size()
    bad = []
    for Cc in sc.POOL_C_LP:
        for H, W in sc.POOL_HW:
            x = sc.pool_input(sc.POOL_N, H, W, Cc, dtype)
            want = sc.pool64(x).to(dtype)
            y = guarded.alloc(want.shape, dtype, DEV)
            rc = maxpool(guarded.put(x, DEV), y, lp)
            bad += [((H, W, Cc), 'return code %d' % rc)] if rc else []
            bad += [((H, W, Cc), m) for m in [mismatch(y, want)] if m]
    finish('max-pool %s' % dtype, start, len(sc.POOL_C_LP) * len(sc.POOL_HW), bad)


def test_maxpool_f32_past_the_grid_cap():
    """N 9, H = W 121, C 256: 2 143 296 channel quads on a grid capped at 8192 blocks of 256 - the only case in which a thread of
    usot_maxpool3x3s2_f32 runs its loop a second time."""
    start = guarded.registry_size()
    N, H, W, Cc = sc.POOL_BIG
    x = sc.pool_input(N, H, W, Cc)
    want = sc.pool64(x, torch.float32)
    assert want.numel() // 4 > sc.POOL_CAP
    y = guarded.alloc(want.shape, torch.float32, DEV)
    rc = maxpool(guarded.put(x, DEV), y)
    bad = ['return code %d' % rc] if rc else []
    bad += [m for m in [mismatch(y, want)] if m]
    finish('max-pool fp32 past the cap', start, 1, bad)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _entries():
    """name -> (row list of stem_cases.r_cases, output type, call(a)); a: the arguments of one launch, pointers as integers"""
    L, st = hip.lib(), hip.stream
    p = C.c_void_p
    conv = lambda a: (p(a['x']), p(a['w']), p(a['bias']), p(a['y']), a['N'], a['H'], a['W'], a['OH'], a['OW'])
    pool = lambda a: conv(a) + (a['PH'], a['PW'])
    return {
        'usot_stem_conv_f32': ('conv', 'bank', torch.float32, lambda a: L.usot_stem_conv_f32(st(), *conv(a))),
        'usot_stem_conv_mu_f32': ('conv', 'bank', torch.float32, lambda a: L.usot_stem_conv_mu_f32(st(), *conv(a), *sc.NO_MU)),
        'usot_stem_pool_f32': ('pool', 'f32', torch.float32, lambda a: L.usot_stem_pool_f32(st(), *pool(a))),
        'usot_stem_pool_ind_f32': ('pool', 'f32', torch.float32, lambda a: L.usot_stem_pool_ind_f32(st(), *pool(a), p(a['word']))),
        'usot_stem_pool_mu_f32': ('pool', 'f32', torch.float32, lambda a: L.usot_stem_pool_mu_f32(st(), *pool(a), None, *sc.NO_MU)),
        'usot_stem_pool_lp': ('lp', torch.bfloat16, torch.bfloat16, lambda a: L.usot_stem_pool_lp(st(), *pool(a), a['dtype'], *sc.NO_MU)),
    }


@pytest.mark.parametrize('name', ['usot_stem_conv_f32', 'usot_stem_conv_mu_f32', 'usot_stem_pool_f32', 'usot_stem_pool_ind_f32',
                                  'usot_stem_pool_mu_f32', 'usot_stem_pool_lp'])
def test_refusals(name):
    """Every refusal of a stem entry point - inconsistent OH, OW, PH, PW, H or W below 7, no image, more images than grid planes,
    a misaligned operand where the launcher checks it, an unknown dtype - returns USOT_EINVAL and writes nothing; the same launch
    without the change is accepted and right."""
    entry, wname, dtype, call = _entries()[name]
    start = guarded.registry_size()
    case = sc.R_SHAPE
    want_stem, want_pooled = sc.build(case)
    want = sc.stored(want_stem if entry == 'conv' else want_pooled, dtype)
    N, H, W, OH, OW, PH, PW = geometry(case)
    word = guarded.alloc((2,), torch.int32, DEV, 'zero')
    x = guarded.put(sc.crops(case), DEV)
    base = dict(x=x.data_ptr(), w=ops(wname).data_ptr(), bias=ops('bias', sc.NO_MU).data_ptr(), word=word.data_ptr(),
                N=N, H=H, W=W, OH=OH,OW=OW, PH=PH, PW=PW, dtype=0)
    y = guarded.alloc(want.shape, dtype, DEV)
    rc = call(dict(base, y=y.data_ptr()))
    bad = [('unchanged', 'return code %d' % rc)] if rc else []
    bad += [('unchanged', m) for m in [mismatch(y, want)] if m]
    rows = sc.r_cases(entry)
    for rid, (field, arg) in rows:
        y = guarded.alloc(want.shape, dtype, DEV)
        snap = guarded.snapshot(y)
        a = dict(base, y=y.data_ptr())
        if field == 'advance':
            a[arg] += 4
        elif field in ('H', 'W', 'N', 'dtype'):
            a[field] = arg
        else:
            a[field] += arg
        rc = call(a)
        torch.cuda.synchronize()
        untouched = torch.equal(guarded.snapshot(y), snap)
        if rc != EINVAL or not untouched:
            bad.append((rid, 'return code %d' % rc, 'output untouched' if untouched else 'THE OUTPUT WAS WRITTEN'))
    finish('%s: refusals' % name, start, len(rows), bad)


def test_maxpool_refusals():
    """usot_maxpool3x3s2_f32 with 6 channels and usot_maxpool3x3s2_lp with 4: USOT_EINVAL, nothing written; 8 channels are accepted."""
    start = guarded.registry_size()
    bad = []
    for dtype, lp, Cc, ok in ((torch.float32, None, 6, False), (torch.float32, None, 8, True), (torch.bfloat16, 0, 4, False),
                              (torch.bfloat16, 0, 8, True)):
        x = guarded.put(sc.pool_input(1, 3, 3, 8, dtype), DEV)
        y = guarded.alloc((1, 2, 2, 8), dtype, DEV)
        snap = guarded.snapshot(y)
        N, H, W, _ = x.shape
        args = (hip.stream(), hip.ptr(x), hip.ptr(y), N, H, W, Cc, 2, 2)
        rc = hip.lib().usot_maxpool3x3s2_f32(*args) if lp is None else hip.lib().usot_maxpool3x3s2_lp(*args, lp)
        torch.cuda.synchronize()
        if ok:
            bad += [(str(dtype), Cc, 'return code %d' % rc)] if rc else []
        elif rc != EINVAL or not torch.equal(guarded.snapshot(y), snap):
            bad.append((str(dtype), Cc, 'return code %d' % rc, 'written' if not torch.equal(guarded.snapshot(y), snap) else ''))
    finish('max-pool refusals', start, 4, bad)
