"""GPU: the spatial kernels of the batched low-precision backbone at every tile residue and border geometry of
tests/lp_spatial_cases.py, bit for bit against float64: usot_conv3x3_halo_lp, usot_bneck_first_lp / usot_bneck_tail_lp,
usot_conv_kstream_lp (and its plan op), usot_conv_pw_lp / usot_conv_pw_pair_lp on both panel forms and both k-loops.

The operands are exact (lp_spatial_cases.py: every fp32 partial sum of every summation order is an integer number of granules
below 2^24), so EVERY comparison is torch.equal on the bits, in bf16 and in fp16; the reference rounds to nearest even where the
kernels store or re-read a 16-bit value.  The row-shared and per-tap loops and the two panel forms of conv_pw are compared with
each other as well.  Inputs lie between NaNs and are checked unchanged, outputs are NaN-prefilled between canaries
(tests/guarded.py), every test ends with guarded.check.

One item = one (entry point, list, storage type); it loops over its list and reports every failing case.  R: every USOT_EINVAL
branch of the six launchers, outputs untouched - among them the usot_conv_kstream_lp geometries whose parked taps would read
past the end of x.  The lists are asserted by tests/test_lp_spatial_lists.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import lp_spatial_cases as lc  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
EINVAL = -1
LP = [pytest.param(dtype, dt, id=name) for name, dtype, dt in lc.DTYPES]


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def mismatch(out, want):
    """'' when the device tensor holds exactly the bits of `want` (a CPU tensor of the same type and shape), else what differs"""
    want = want.to(DEV).reshape(out.shape)
    ne = bits(out) != bits(want)
    if not bool(ne.any()):
        return ''
    first = int(ne.reshape(-1).nonzero()[0])
    idx = []
    for n in reversed(out.shape):
        idx.insert(0, first % n)
        first //= n
    return '%d of %d elements differ (%d NaN), first at %s: got %r, want %r' % (
        int(ne.sum()), out.numel(), int(torch.isnan(out).sum()), idx, float(out[tuple(idx)]), float(want[tuple(idx)]))


class Operands(object):
    """guarded device copies of a case's operands (16-bit ones in the storage type, biases fp32), snapshotted"""

    def __init__(self, tensors, dtype):
        self.t, self.snap = {}, {}
        for k, v in tensors.items():
            if v is None:
                self.t[k] = None
                continue
            self.t[k] = guarded.put((v.float() if k.startswith('b') else v.float().to(dtype)).contiguous(), DEV)
            self.snap[k] = guarded.snapshot(self.t[k])

    def __getitem__(self, k):
        return self.t[k]

    def addr(self, k):
        return self.t[k].data_ptr() if self.t.get(k) is not None else None

    def changed(self):
        out = []
        for k, s in self.snap.items():
            try:
                guarded.unchanged(self.t[k], s, k)
            except guarded.GuardError as e:
                out.append(str(e))
        return out


def sweep(what, cases, run):
    """run(case) -> failure texts; every case runs, the guards of everything it allocated are checked at the end"""
    start = guarded.registry_size()
    bad, launches = [], 0
    for case in cases:
        n, msgs = run(case)
        launches += n
        bad += [(tuple(case), m) for m in msgs]
    torch.cuda.synchronize()
    guarded.check(start)
    print('%s: %d cases, %d launches, %d failing' % (what, len(cases), launches, len(bad)))
    assert not bad, bad[:20]


def compare(outs, want, tag=''):
    return ['%s%s: %s' % (tag, k, m) for k in want for m in [mismatch(outs[k], want[k])] if m]


# ------------------------------------------------------------------------------------------------------------------ operands on the device
def halo_tensors(case):
    o = lc.halo_ops(case)
    return dict(x=o['x'], w=o['w'].reshape(64, 576), b=o['b'])


def kstream_tensors(case):
    o = lc.kstream_ops(case)
    return dict(x=o['x'], w=o['w'].reshape(case.Cout, 9 * case.Cin), b=o['b'])


def bneck_tensors(case):
    """named as the fields of usot_bneck_desc the launch reads them from"""
    o = lc.bneck_ops(case)
    if case.kind == 'first':
        return dict(x=o['x'], w1=o['w1'], b1=o['b1'], w2=o['w2'].reshape(64, 576), b2=o['b2'], w3c=torch.cat([o['w3'], o['wd']], 1),
                    b3c=o['b3'], wn=o['wn'], bn=o['bn'])
    return dict(x=o['t1'], w1=o['res'], b1=None, w2=o['w2'].reshape(64, 576), b2=o['b2'], w3c=o['w3'], b3c=o['b3'], wn=o['wn'], bn=o['bn'])


def convpw_tensors(case):
    o = dict(lc.convpw_ops(case))
    o['w2'] = o['w2'].reshape(case.cm, case.KH * case.KW * case.cm)
    return o


# ------------------------------------------------------------------------------------------------------------------ launches
def halo_launch(ops, out_y, N, H, W, Cin=64, Cout=64, act=1, dtype=0, **ptrs):
    a = dict(x=ops.addr('x'), w=ops.addr('w'), b=ops.addr('b'), y=out_y.data_ptr())
    a.update(ptrs)
    return hip.lib().usot_conv3x3_halo_lp(hip.stream(), a['x'], a['w'], a['b'], a['y'], N, H, W, Cin, Cout, act, dtype)


def kstream_launch(ops, out_y, N, H, W, Cin, Cout, stride, pad, dil, act, dtype, plan=False, **ptrs):
    a = dict(x=ops.addr('x'), w=ops.addr('w'), b=ops.addr('b'), y=out_y.data_ptr())
    a.update(ptrs)
    args = (a['x'], a['w'], a['b'], a['y'], N, H, W, Cin, Cout, stride, pad, dil, act, dtype)
    if not plan:
        return hip.lib().usot_conv_kstream_lp(hip.stream(), *args)
    L = hip.lib()
    pl = C.c_void_p(L.usot_plan_create())
    try:
        rc = L.usot_plan_add_conv_kstream(pl, *args)
        return rc if rc else L.usot_plan_run(pl, hip.stream())
    finally:
        L.usot_plan_destroy(pl)


def bneck_launch(kind, ops, out_y, out_t, N, H, W, Cnext=64, dtype=0, **ptrs):
    a = {k: ops.addr(k) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'w3c', 'b3c', 'wn', 'bn')}
    a.update(y=out_y.data_ptr(), t=out_t.data_ptr())
    a.update(ptrs)
    d = hip.bneck_desc(a['x'], a['w1'], a['b1'], a['w2'], a['b2'], a['w3c'], a['b3c'], a['wn'], a['bn'], a['y'], a['t'], N, H, W)
    if kind == 'first':
        return hip.lib().usot_bneck_first_lp(hip.stream(), C.byref(d), dtype)
    return hip.lib().usot_bneck_tail_lp(hip.stream(), C.byref(d), Cnext, dtype)


def convpw_launch(case, ops, y, t, tile, dtype, fields=None, ptrs=None):
    """fields: overrides of usot_conv_desc fields ('N', 'act', ...), of the pair descriptor ('pd.M', ...) and 'dtype'; ptrs: overrides
    of the pointers, 'c2' / 'pd' = None pass no descriptor at all"""
    fields, ptrs = dict(fields or {}), dict(ptrs or {})
    oh, ow = lc.out_hw(lc.geo_of(case))
    M, cm, co = case.N * oh * ow, case.cm, 4 * case.cm
    a = {k: ops.addr(k) for k in ('x', 'w2', 'b2', 'w3', 'b3', 'res', 'w1', 'b1')}
    a.update(y=y.data_ptr(), t=t.data_ptr() if t is not None else None)
    a.update({k: v for k, v in ptrs.items() if k not in ('c2', 'pd')})
    d = hip.conv_desc(a['x'], a['w2'], a['b2'], None, N=case.N, H=case.H, W=case.W, Cin=cm, OH=oh, OW=ow, Cout=cm, KH=case.KH, KW=case.KW,
                      stride=case.stride, pad=(case.pad_h, case.pad_w), dil=(case.dil_h, case.dil_w), act=lc.ACT_RELU, tile=tile)
    for k, v in fields.items():
        if k == 'res':
            d.res = a[v]
        elif not k.startswith('pd.') and k != 'dtype':
            setattr(d, k, v)
    dtype = fields.get('dtype', dtype)
    c2 = None if 'c2' in ptrs else C.byref(d)
    if not case.cn:
        return hip.lib().usot_conv_pw_lp(hip.stream(), c2, a['w3'], a['b3'], a['res'], a['y'], dtype)
    pd = hip.pw_pair_desc(None, a['w3'], a['b3'], a['res'], a['y'], a['w1'], a['b1'], a['t'], M, cm, co, case.cn, case.act2)
    for k, v in fields.items():
        if k.startswith('pd.'):
            setattr(pd, k[3:], v)
    return hip.lib().usot_conv_pw_pair_lp(hip.stream(), c2, None if 'pd' in ptrs else C.byref(pd), dtype)


# ------------------------------------------------------------------------------------------------------------------ conv3x3_halo
@pytest.mark.parametrize('dtype,dt', LP)
def test_conv3x3_halo(dtype, dt):
    """H = 1 .. 33 at W = 17, W = 1 .. 33 at H = 5, the corners at two images, both activations, no bias, 520 tiles"""
    def run(case):
        ops = Operands(halo_tensors(case), dtype)
        y = guarded.alloc((case.N, case.H, case.W, 64), dtype, DEV)
        rc = halo_launch(ops, y, case.N, case.H, case.W, act=case.act, dtype=dt)
        if rc:
            return 1, ['return code %d' % rc]
        return 1, compare({'y': y}, lc.expected(case, dtype)) + ops.changed()
    sweep('conv3x3_halo %s' % dtype, lc.halo_cases(), run)


# ------------------------------------------------------------------------------------------------------------------ bneck_first, bneck_tail
@pytest.mark.parametrize('dtype,dt', LP)
@pytest.mark.parametrize('kind,cn', lc.BNECK_FAMILIES, ids=['%s_%d' % f for f in lc.BNECK_FAMILIES])
def test_bneck(kind, cn, dtype, dt):
    """H = 1 .. 17 at W = 17, W = 1 .. 33 at H = 9, the corners, the smallest batch with eight tiles; 11 and 18 tiles (some
    workgroups take a second tile).  y and t, both bit for bit."""
    def run(case):
        ops = Operands(bneck_tensors(case), dtype)
        y = guarded.alloc((case.N, case.H, case.W, 256), dtype, DEV)
        t = guarded.alloc((case.N, case.H, case.W, cn), dtype, DEV)
        rc = bneck_launch(kind, ops, y, t, case.N, case.H, case.W, cn, dt)
        if rc:
            return 1, ['return code %d' % rc]
        return 1, compare({'y': y, 't': t}, lc.expected(case, dtype)) + ops.changed()
    sweep('bneck_%s Cnext %d %s' % (kind, cn, dtype), lc.bneck_cases(kind, cn), run)


# ------------------------------------------------------------------------------------------------------------------ conv_kstream
@pytest.mark.parametrize('dtype,dt', LP)
def test_conv_kstream(dtype, dt):
    """stride 1, 2 x dil 1, 2, 3 x every pad 0 .. dil on the smallest legal map, (7, 9), (9, 7), (5, 23) at three images; M = 255,
    256, 257, 511, 513; Cin 256 | 512; Cout 256, 512, 768, 1024; no bias; the plan op"""
    def run(case):
        ops = Operands(kstream_tensors(case), dtype)
        oh, ow = lc.out_hw(lc.geo_of(case))
        y = guarded.alloc((case.N, oh, ow, case.Cout), dtype, DEV)
        rc = kstream_launch(ops, y, case.N, case.H, case.W, case.Cin, case.Cout, case.stride, case.pad, case.dil, case.act, dt, plan=case.plan)
        if rc:
            return 1, ['return code %d' % rc]
        return 1, compare({'y': y}, lc.expected(case, dtype)) + ops.changed()
    sweep('conv_kstream %s' % dtype, lc.kstream_cases(), run)


# ------------------------------------------------------------------------------------------------------------------ conv_pw, conv_pw_pair
def convpw_run(dtype, dt):
    def run(case):
        ops = Operands(convpw_tensors(case), dtype)
        want = lc.expected(case, dtype)
        M = lc.pixels(case)
        msgs, n, first = [], 0, None
        for loop in lc.convpw_loops(case):
            for form in lc.CONVPW_FORMS:
                y = guarded.alloc((M, 4 * case.cm), dtype, DEV)
                t = guarded.alloc((M, case.cn), dtype, DEV) if case.cn else None
                rc = convpw_launch(case, ops, y, t, form | loop, dt)
                n += 1
                tag = 'form %d loop %d ' % (form, loop)
                if rc:
                    msgs.append(tag + 'return code %d' % rc)
                    continue
                outs = {'y': y, 't': t} if case.cn else {'y': y}
                msgs += compare(outs, want, tag)
                if first is None:
                    first = outs
                else:                       # ... and the forms and loops among themselves
                    msgs += [tag + '%s differs from the first launch' % k for k in outs if not torch.equal(bits(outs[k]), bits(first[k]))]
        return n, msgs + ops.changed()
    return run


@pytest.mark.parametrize('dtype,dt', LP)
def test_conv_pw_per_tap_list(dtype, dt):
    """filters 1 x 1, 1 x 3, 3 x 1, 2 x 2, 3 x 3 at stride 1, 2, 3, unequal pads and dilations, padding beyond the filter's reach,
    M = 127 .. 385: every family, both panel forms; both k-loops where the row-shared one is eligible"""
    sweep('conv_pw per-tap list %s' % dtype, lc.convpw_pertap_cases(), convpw_run(dtype, dt))


@pytest.mark.parametrize('dtype,dt', LP)
@pytest.mark.parametrize('dil_h', [1, 2, 5])
def test_conv_pw_row_shared_list(dil_h, dtype, dt):
    """3 x 3 / stride 1 / pad = dil: dil_w 1 .. 4 (and 5 once: the per-tap fall-back) at W = 1 .. 9 - rows shorter than the
    dilation, than the 4-pixel stage halo - H = 1 .. 7, panel edges inside a row, at a row end, at an image end: both loops, both
    forms, all four launches bit-equal to float64 and to each other"""
    cases = [c for c in lc.convpw_rowshared_cases() if c.dil_h == dil_h]
    assert len(cases) >= 28
    sweep('conv_pw row-shared list dil_h %d %s' % (dil_h, dtype), cases, convpw_run(dtype, dt))


# ------------------------------------------------------------------------------------------------------------------ R
def _refusal(row, dtype=torch.bfloat16, changed=True):
    """the base launch with the one change the row names (or without it) -> (return code, outputs untouched)"""
    name, entry, base, change = row
    scal, ptrs = {}, {}
    tensors = {'halo': halo_tensors, 'kstream': kstream_tensors, 'kstream_plan': kstream_tensors, 'bneck_first': bneck_tensors,
               'bneck_tail': bneck_tensors, 'conv_pw': convpw_tensors, 'conv_pw_pair': convpw_tensors}[entry](base)
    ops = Operands(tensors, dtype)
    M = lc.pixels(base)
    if entry == 'halo':
        outs = {'y': guarded.alloc((M, 64), dtype, DEV)}
    elif entry.startswith('kstream'):
        outs = {'y': guarded.alloc((M, base.Cout), dtype, DEV)}
    elif entry.startswith('bneck'):
        outs = {'y': guarded.alloc((M, 256), dtype, DEV), 't': guarded.alloc((M, 128), dtype, DEV)}
    else:
        outs = {'y': guarded.alloc((M, 4 * base.cm), dtype, DEV), 't': guarded.alloc((M, base.cn), dtype, DEV) if base.cn else None}
    snaps = {k: guarded.snapshot(v) for k, v in outs.items() if v is not None}
    if changed:
        if change[0] == 'arg':
            scal[change[1]] = change[2]
        elif change[0] == 'null':
            ptrs[change[1]] = None
        elif change[0] == 'misalign':
            src = outs[change[1]] if change[1] in outs else ops[change[1]]
            ptrs[change[1]] = src.data_ptr() + 2
        elif change[0] == 'geometry':
            scal.update(N=change[1], H=change[2], W=change[3])
            scal.update(change[4] if len(change) > 4 else {})
        else:
            raise AssertionError(change)
    if entry == 'halo':
        a = dict(N=base.N, H=base.H, W=base.W, act=base.act, dtype=0)
        a.update(scal)
        rc = halo_launch(ops, outs['y'], **a, **ptrs)
    elif entry.startswith('kstream'):
        a = dict(N=base.N, H=base.H, W=base.W, Cin=base.Cin, Cout=base.Cout, stride=base.stride, pad=base.pad, dil=base.dil, act=base.act, dtype=0)
        a.update(scal)
        rc = kstream_launch(ops, outs['y'], plan=entry == 'kstream_plan', **a, **ptrs)
    elif entry.startswith('bneck'):
        a = dict(N=base.N, H=base.H, W=base.W, Cnext=base.cn, dtype=0)
        a.update(scal)
        rc = bneck_launch(base.kind, ops, outs['y'], outs['t'], **a, **ptrs)
    else:
        rc = convpw_launch(base, ops, outs['y'], outs['t'], 1, 0, fields=scal, ptrs=ptrs)
    torch.cuda.synchronize()
    return rc, all(torch.equal(guarded.snapshot(outs[k]), s) for k, s in snaps.items()) and not ops.changed()


def test_r_refusals():
    """R.  Every USOT_EINVAL branch of the six launchers, the parked-tap geometries of usot_conv_kstream_lp among them (directly and
    through the plan op): USOT_EINVAL, nothing launched, nothing written."""
    start = guarded.registry_size()
    rows = lc.refusals()
    bad = []
    for row in rows:
        rc, untouched = _refusal(row)
        if rc != EINVAL or not untouched:
            bad.append((row[0], 'return code %d' % rc, 'outputs untouched' if untouched else 'AN OUTPUT WAS WRITTEN'))
    guarded.check(start)
    print('R: %d refusals, %d failing' % (len(rows), len(bad)))
    assert not bad, bad


def test_r_base_launches_are_accepted():
    """the launches of part R differ from an accepted launch in the named change only"""
    start = guarded.registry_size()
    seen, bad = set(), []
    for row in lc.refusals():
        if row[1] in seen:
            continue
        seen.add(row[1])
        rc, _ = _refusal(row, changed=False)
        if rc != 0:
            bad.append((row[1], 'the unchanged launch returns %d' % rc))
    guarded.check(start)
    assert len(seen) == 7 and not bad, bad
