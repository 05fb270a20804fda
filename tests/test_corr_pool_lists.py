"""CPU: the lists of tests/corr_pool_cases.py are the ones the correlation and RoI-pool sweep was specified with, the operands keep every
`==` of tests/test_gpu_corr_pool_sweep.py a fact about the operands (integer xcorr sums; for PrRoIPool the float32 restatement equals
the float64 oracle, every expectation is a float32, and no order of the atomics can round), the RoI list really reaches every alignment
class, and every listed mutation - a plausible wrong kernel - changes the reference on the sweep's own operands."""
import numpy as np
import pytest
import torch

import corr_pool_cases as cp
import prroi_exact as ex
import usot_oracle as orc

PR_LISTS = [(ph, pw, s) for ph, pw in cp.PR_SHAPES for s in cp.PR_SCALES]


def is_f32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


def differs(a, b):
    """not bit-equal as values (a NaN equals a NaN); a different shape differs"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ============================================================================================================================ xcorr
def test_xcorr_lists_are_the_specified_ones():
    assert cp.TEMPLATES == ((5, 5), (3, 5), (5, 3)) and cp.XC_P == (1, 2, 3, 4, 5, 7, 8, 9, 17)
    for hk, wk in cp.TEMPLATES:
        ws = cp.wx_sweep((hk, wk))
        assert {c[1] for c in ws} == set(range(wk, 67)) and {(c[0], c[2], c[3], c[4]) for c in ws} == {(hk + 1, hk, wk, 9)}
        assert {cp.xc_kernel(c) for c in ws} == {'planes2', 'planes1', 'generic'}
        assert [cp.xc_kernel(c) for c in ws if c[1] in (32, 33, 64, 65)] == ['planes2', 'planes1', 'planes1', 'generic']
        # every residue of a lane's column in both layouts: OW from 1 up to the full half (two planes) and the full wavefront
        assert {c[1] for c in ws if cp.xc_kernel(c) == 'planes2'} == set(range(wk, 33))
        assert {c[1] for c in ws if cp.xc_kernel(c) == 'planes1'} == set(range(33, 65))
        ps = cp.p_sweep((hk, wk))
        assert {(c[4], c[1], c[0]) for c in ps} == {(p, wx, hx) for p in cp.XC_P for wx in (31, 33) for hx in (hk, hk + 1, hk + 6)}
        assert len(ps) == 54 and {cp.xc_kernel(c) for c in ps} == {'planes2', 'planes1'}
    assert {c[2:4] for c in cp.XC_GENERIC} == {(1, 1), (2, 4), (7, 7), (5, 5)}
    assert all(cp.xc_kernel(c) == 'generic' for c in cp.XC_GENERIC) and all(c[1] == 65 for c in cp.XC_GENERIC if c[2:4] == (5, 5))
    assert any(min(cp.xc_counts(c).values()) > 256 for c in cp.XC_GENERIC)                     # more than one block
    assert {(c[1], c[4] % 2, cp.xc_kernel(c)) for c in cp.XC_ISOLATION} == {(16, 0, 'planes2'), (16, 1, 'planes2'), (32, 0, 'planes2'),
                                                                             (32, 1, 'planes2'), (33, 0, 'planes1'), (33, 1, 'planes1')}
    assert cp.XC_MUTATIONS == ['flip', 'shift', 'drop_col', 'dead_half', 'one_pass']


def test_xcorr_big_problems_pass_their_grid_caps():
    assert cp.XC_BIG['planes2'] == (5, 6, 5, 5, 32768 + 9) and cp.XC_BIG['planes1'] == (5, 33, 5, 5, 16384 + 5)
    assert cp.XC_BIG['generic_dk'][:4] == (12, 13, 12, 12)
    for name, case in cp.XC_BIG.items():
        assert cp.xc_kernel(case) == name.split('_')[0]
        n, first = cp.xc_counts(case), cp.xc_first_pass(case)
        for e in cp.XC_BIG_ENTRIES[name]:
            assert first[e] < n[e], (name, e)
            if name.startswith('generic'):
                assert n[e] > 2097152 and (n[e] - 2097152) % 256, (name, e)                    # ragged: the last block is partial
        idx = cp.xc_big_index(name)
        assert idx.min() == 0 and idx.max() == cp.XC_BASE_PLANES - 1 and len(idx) == case[4]
        for e in cp.XC_BIG_ENTRIES[name]:                                                        # not periodic in the pass length
            per = n[e] // case[4]
            step = first[e] // per if first[e] % per == 0 else None
            if step:
                assert not np.array_equal(idx[step:], idx[:len(idx) - step]), (name, e)
    for case in [c for t in cp.TEMPLATES for c in cp.wx_sweep(t) + cp.p_sweep(t)] + cp.XC_GENERIC + cp.XC_ISOLATION:
        assert cp.xc_first_pass(case) == cp.xc_counts(case)                                      # the small lists fit one pass


@pytest.mark.parametrize('case', [(6, 9, 5, 5, 3), (4, 33, 3, 5, 2), (11, 16, 5, 3, 5), (9, 12, 2, 4, 3), (12, 13, 12, 12, 2), (6, 65, 5, 5, 2)])
def test_xcorr_reference_is_the_oracles_autograd(case):
    x, k, dout = cp.xc_operands(case)
    x64, k64 = (torch.from_numpy(a).double()[None].requires_grad_(True) for a in (x, k))
    out = orc.xcorr_depthwise(x64, k64)
    gx, gk = torch.autograd.grad(out, (x64, k64), torch.from_numpy(dout).double()[None])
    s = cp.xc_scale(case)
    ref = cp.xc_ref(x, k, dout, s)
    assert np.array_equal(ref['out'], out.detach().numpy()[0])
    assert np.array_equal(ref['dx'], s * gx.numpy()[0]) and np.array_equal(ref['dk'], s * gk.numpy()[0])


def test_xcorr_operands_keep_float32_exact():
    """integers in [-3, 3]: |sum| <= 9 Hk Wk (out, dx) or 9 OH OW (dk), times a power of two"""
    worst = 0
    for case in [c for t in cp.TEMPLATES for c in cp.wx_sweep(t) + cp.p_sweep(t)] + cp.XC_GENERIC + cp.XC_ISOLATION \
            + [cp.xc_base(n) for n in cp.XC_BIG]:
        hx, wx, hk, wk, p = case
        ops = cp.xc_operands(case)
        assert all(a.dtype == np.float32 and np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 3 for a in ops)
        assert cp.xc_scale(case) in (0.25, 0.5, 2.0)
        worst = max(worst, 9 * hk * wk, 9 * (hx - hk + 1) * (wx - wk + 1))
    assert worst * 2 < 2 ** 24
    ref = cp.xc_ref(*cp.xc_operands((6, 31, 5, 5, 9)), 0.25)
    assert all(is_f32(a) for a in ref.values())


def test_xcorr_mutations_change_the_reference():
    touched = {'flip': cp.XC_ENTRIES, 'shift': ('out', 'dk'), 'drop_col': cp.XC_ENTRIES}
    for t in cp.TEMPLATES:
        for case in cp.wx_sweep(t):
            ops, s = cp.xc_operands(case), cp.xc_scale(case)
            ref = cp.xc_ref(*ops, s)
            for m, entries in touched.items():
                got = cp.xc_ref(*ops, s, mutate=m)
                assert all(differs(got[e], ref[e]) for e in entries), (case, m)
            dead = cp.xc_ref(*ops, s, mutate='dead_half')
            # the idle half of the last wavefront: a kernel that lets it work stores one plane behind the output, into the guard
            assert all((dead[e].shape[0] == case[4] + 1) == (case[1] <= 32) for e in cp.XC_ENTRIES), case
    for name, case in cp.XC_BIG.items():
        idx = cp.xc_big_index(name)
        base = cp.xc_ref(*cp.xc_operands(cp.xc_base(name)), 0.5)
        first = cp.xc_first_pass(case)
        for e in cp.XC_BIG_ENTRIES[name]:
            want = base[e][idx]
            one = want.copy()
            one.reshape(-1)[first[e]:] = np.nan
            assert differs(one, want) and not differs(one.reshape(-1)[:first[e]], want.reshape(-1)[:first[e]])
    small = (5, 6, 5, 5, 3)
    assert not differs(cp.xc_ref(*cp.xc_operands(small), 1.0, mutate='one_pass')['dx'], cp.xc_ref(*cp.xc_operands(small), 1.0)['dx'])


# ========================================================================================================================= PrRoIPool
def test_prroi_lists_are_the_specified_ones():
    assert cp.PR_MAP == (2, 4, 9, 11) and cp.PR_BINS == (0.25, 0.5, 1.0, 2.0, 4.0) and cp.PR_SCALES == (1.0, 0.5)
    assert cp.PR_SHAPES == ((7, 7), (3, 5), (1, 1), (4, 8), (8, 8), (2, 1)) and cp.PR_ROI_EXACT == ((1, 1), (4, 8), (8, 8), (2, 1))
    assert cp.pr_starts() == ((-2.25, -1.0, 0.0, 0.5, 3.75, 9.0, 10.0, 10.75, 12.0), (-1.5, 0.0, 2.25, 8.0))
    assert cp.PR_MUTATIONS == ['floor_plus_1', 'cell_le', 'pixel_lt', 'clamp', 'roi_area', 'scale_width', 'fx1']
    f = cp.pr_features()
    assert f.shape == cp.PR_MAP and np.array_equal(f, np.rint(f)) and f.min() == -4 and f.max() == 4
    for ph, pw, s in PR_LISTS:
        rois = cp.pr_rois(ph, pw, s)
        assert rois.shape == (186, 5) and np.array_equal(rois[:, 0], np.arange(186) % 2)
        assert np.array_equal(rois[:, 1:] * 4 * s, np.rint(rois[:, 1:] * 4 * s))                 # corners: multiples of 1/4 of a pixel
        geo = [cp.pr_geometry(r, ph, pw, s) for r in rois[:180]]
        assert {(g[2], g[3]) for g in geo} == {(a, b) for a in cp.PR_BINS for b in cp.PR_BINS}
        assert {(g[0], g[1]) for g in geo} == {(x, y) for x in cp.pr_starts()[0] for y in cp.pr_starts()[1]}
        assert {g[2] for g in geo[:36]} == {0.25} and len({(g[0], g[1]) for g in geo[:36]}) == 36     # bin width x start x x start y
        deg = [cp.pr_geometry(r, ph, pw, s) for r in rois[180:]]
        assert [g[2] * g[3] > 0 for g in deg] == [False, False, False, False, True, True]       # the last two lie outside the map
        g = cp.pr_top_diff(186, ph, pw)
        assert np.array_equal(g, np.rint(g)) and g.min() == -3 and g.max() == 3
    assert not cp.pr_case(7, 7, 1.0)['out'][184:].any()


@pytest.mark.parametrize('ph,pw,scale', PR_LISTS)
def test_prroi_equality_is_a_fact_about_the_operands(ph, pw, scale):
    """conditions 1 - 3: the float32 restatement equals the float64 oracle, every expectation is a float32, and for the two atomically
    accumulated outputs sum |terms| / (finest power of two dividing a term) < 2^24 per element: every partial sum, in any order, is a
    multiple of that power of two below 2^24 of them, hence a float32"""
    c = cp.pr_case(ph, pw, scale)
    f, rois, g = c['f'].copy(), c['rois'].copy(), c['g'].copy()
    exact_roi = (ph, pw) in cp.PR_ROI_EXACT
    fwd32 = orc.prroi_pool(torch.from_numpy(f), torch.from_numpy(rois), ph, pw, scale).numpy()
    assert np.array_equal(fwd32, c['out']) and is_f32(c['out'])
    assert np.array_equal(orc.prroi_pool_backward(f.shape, rois, g, ph, pw, scale).numpy(), c['gin']) and is_f32(c['gin'])
    roi32 = orc.prroi_pool_coor_backward(f, rois, fwd32, g, ph, pw, scale).numpy()
    err = float(np.abs(roi32 - c['groi']).max())
    print('%d x %d scale %g: RoI gradient float32 - float64 %.3g on values up to %.4g' % (ph, pw, scale, err, np.abs(c['groi']).max()))
    if exact_roi:
        assert err == 0.0 and is_f32(c['groi'])
    else:
        mag = np.maximum(1.0, np.abs(c['groi']).max(1))
        assert 0.0 < err and np.all(np.abs(roi32 - c['groi']).max(1) / mag <= cp.PR_ROI_BAR)
    gin, mag, quantum = cp.pr_backward_terms(f.shape, rois, g, ph, pw, scale)
    assert np.array_equal(gin, c['gin'])
    assert np.all(mag[mag > 0] / quantum[mag > 0] < 2 ** 24)
    terms = cp.pr_coor_terms(f, rois, g, ph, pw, scale)
    if exact_roi:
        assert np.array_equal(terms.sum((1, 2, 3)), c['groi'][:, 1:])
        q = cp.lowest_bit(terms).min((1, 2, 3))
        m = np.abs(terms).sum((1, 2, 3))
        assert np.all(m[m > 0] / q[m > 0] < 2 ** 24)
    else:
        assert np.allclose(terms.sum((1, 2, 3)), c['groi'][:, 1:], rtol=0, atol=1e-11)
    assert np.array_equal(cp.pr_forward_cells(f, rois, ph, pw, scale), c['out'])


def test_prroi_list_reaches_every_alignment_class():
    """condition 4, counted over the twelve lists (bins, each counted once per bin of the other axis)"""
    total = {}
    for ph, pw, s in PR_LISTS:
        one = cp.pr_alignment(cp.pr_rois(ph, pw, s), ph, pw, s)
        assert set(one) == set(ALIGNMENT) and all(one.values()), (ph, pw, s)        # each list reaches every class by itself
        for k, v in one.items():
            total[k] = total.get(k, 0) + v
    print(sorted(total.items()))
    assert total == ALIGNMENT


ALIGNMENT = {'x left aligned': 27116, 'x right aligned': 26324, 'x one cell': 28400, 'x edge at -1': 1328, 'x edge at 0': 2080,
             'x edge at n-1': 2408, 'x edge at n': 3288, 'y left aligned': 25302, 'y right aligned': 24784, 'y one cell': 28174,
             'y edge at -1': 2088, 'y edge at 0': 4158, 'y edge at n-1': 4554, 'y edge at n': 2772}


def test_prroi_mutations_change_the_reference():
    changed = {m: 0 for m in cp.PR_MUTATIONS}
    for ph, pw, s in [(4, 8, 0.5), (3, 5, 1.0)]:
        c = cp.pr_case(ph, pw, s)
        f, rois, g = c['f'], c['rois'], c['g']
        for m in ('floor_plus_1', 'cell_le', 'clamp', 'roi_area', 'scale_width'):
            got = cp.pr_forward_cells(f, rois, ph, pw, s, mutate=m)
            if m == 'floor_plus_1':
                assert not differs(got, c['out'])          # on a finite map the extra cell has no width: see the Inf case below
            elif m == 'scale_width':
                assert differs(got, c['out']) == (s != 1.0)
            else:
                assert differs(got, c['out']), m
            changed[m] += differs(got, c['out'])
        for m in ('pixel_lt', 'roi_area', 'scale_width'):
            got = cp.pr_backward_terms(f.shape, rois, g, ph, pw, s, mutate=m)[0]
            assert differs(got, c['gin']) == (m != 'scale_width' or s != 1.0), m
            changed[m] += 1
        # an aligned right edge's extra cell, and the pixel behind an aligned edge, carry no weight: the gradient's loop bounds may run
        # one further, never one short
        assert not differs(cp.pr_backward_terms(f.shape, rois, g, ph, pw, s, mutate='floor_plus_1')[0], c['gin'])
        terms = cp.pr_coor_terms(f, rois, g, ph, pw, s, mutate='fx1').sum((1, 2, 3))
        assert np.abs(terms - c['groi'][:, 1:]).max() > 1.0
        changed['fx1'] += 1
    assert all(changed[m] for m in cp.PR_MUTATIONS if m != 'floor_plus_1')
    # floor + 1 for ceil: the walk enters the cell behind an aligned edge with zero width; +Inf there turns 0 * Inf into NaN
    ph, pw = cp.PR_INF_SHAPE
    f = cp.pr_inf_features()
    finite = np.where(np.isinf(f), 0.0, f)
    want = ex.prroi_pool_exact(finite, cp.PR_INF_ROIS, ph, pw, 1.0)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(cp.pr_forward_cells(f, cp.PR_INF_ROIS, ph, pw, 1.0), want) and want.any()
        assert np.isnan(cp.pr_forward_cells(f, cp.PR_INF_ROIS, ph, pw, 1.0, mutate='floor_plus_1')).any()
    assert np.array_equal(orc.prroi_pool(torch.from_numpy(finite), torch.from_numpy(cp.PR_INF_ROIS), ph, pw, 1.0).numpy(), want)
    al = cp.pr_alignment(cp.PR_INF_ROIS, ph, pw, 1.0)
    assert al['x right aligned'] and al['y right aligned']


def test_prroi_problems_past_the_caps():
    B, C, H, W = cp.PR_MAP
    assert cp.PR_BIG_R * C * 49 > cp.PR_FWD_CAP and (cp.PR_BIG_R * C * 49 - cp.PR_FWD_CAP) % 256
    base, idx, g = cp.pr_big_base(), cp.pr_big_index(), cp.pr_big_top_diff()
    assert base.shape == (64, 5) and set(idx) == set(range(64)) and len(idx) == cp.PR_BIG_R
    per_pass = cp.PR_FWD_CAP // (C * 49)
    assert not np.array_equal(idx[per_pass:], idx[:len(idx) - per_pass])
    tot, mag = cp.pr_big_summed(idx, g)
    f = cp.pr_features()
    want = ex.prroi_pool_exact_backward(f.shape, base, tot, 7, 7, 1.0)
    gin, m, q = cp.pr_backward_terms(f.shape, base, tot, 7, 7, 1.0, g_abs=mag)
    assert np.array_equal(gin, want) and is_f32(want) and np.all(m[m > 0] / q[m > 0] < 2 ** 24)
    assert is_f32(ex.prroi_pool_exact(f, base, 7, 7, 1.0))
    # the RoI gradient's 64-block grid, twice round
    per_roi = cp.PR_WIDE_C * 64
    assert cp.PR_COOR_CAP < per_roi < 2 * cp.PR_COOR_CAP                   # 256 elements for the second pass
    fw, gw = cp.pr_features(C=cp.PR_WIDE_C, B=1, seed=3), cp.pr_top_diff(3, 8, 8, C=cp.PR_WIDE_C, seed=3)
    want = ex.prroi_pool_exact_coor_backward(fw, cp.PR_WIDE_ROIS, gw, 8, 8, 1.0)
    terms = cp.pr_coor_terms(fw, cp.PR_WIDE_ROIS, gw, 8, 8, 1.0)
    assert np.array_equal(terms.sum((1, 2, 3)), want[:, 1:]) and is_f32(want) and want[:, 1:].all()
    assert np.all(np.abs(terms).sum((1, 2, 3)) / cp.lowest_bit(terms).min((1, 2, 3)) < 2 ** 24)
    fw32 = orc.prroi_pool(torch.from_numpy(fw), torch.from_numpy(cp.PR_WIDE_ROIS), 8, 8, 1.0)
    assert np.array_equal(orc.prroi_pool_coor_backward(fw, cp.PR_WIDE_ROIS, fw32, gw, 8, 8, 1.0).numpy(), want)
    one = terms.reshape(3, -1, 4)[:, :cp.PR_COOR_CAP].sum(1)                  # one pass of the grid only
    assert np.abs(one - want[:, 1:]).min() > 0
    # 65 535 RoIs: rows of the unit gradients times top_diff
    unit = cp.pr_unit_rows()
    assert is_f32(unit * 3) and np.abs(unit).max() < 2 ** 10 and unit[:180].any(1).sum() > 100
