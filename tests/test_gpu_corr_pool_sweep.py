"""GPU: the per-plane xcorr with its two gradients (csrc/xcorr.hip, csrc/xcorr_grad.hip) and Precise RoI Pooling with its two
(csrc/head_ops.hip) against the float64 references of tests/corr_pool_cases.py:

  xcorr    all three entry points at every Wx from Wk to 66 for the three specialised templates (both wavefront layouts, 32 | 33,
           64 | 65 into the generic kernels), P 1 .. 17 around the 4-wavefront block at Wx 31 and 33 and three heights, four generic
           templates; one problem past the grid cap of each kernel, gathered on the device from 64 base planes and bit-equal to the
           gathered base result; +Inf over the neighbouring planes; everything the launchers refuse;
  prroi    the dyadic RoI family (bin edges on quarter pixels, bins of 1/4 .. 4 pixels, boxes over every border, degenerate boxes) at six
           pooled shapes and two scales through the forward and both gradients; the forward's strides as NCHW, NHWC, a channel slice of
           a wider NHWC map and of a wider output; usot_plan_add_prroi; the three PrRoIPooling*Gpu symbols; lists past the caps of all
           three kernels, R = 65 535 and the refused 65 536; batch indices outside the batch; +Inf behind an aligned edge; refusals.

Every comparison is an EQUALITY with float64 (tests/test_corr_pool_lists.py shows why it can be), except the RoI gradient at 7 x 7 and
3 x 5, where pw / PW is no dyadic number: there the bar of test_gpu_ops.py::test_prroi_roi_gradient_vs_oracles holds.  Outputs are
NaN-prefilled between canaries (tests/guarded.py), inputs lie between NaNs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import corr_pool_cases as cp  # noqa: E402
import guarded  # noqa: E402
import prroi_exact as ex  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
OK, EINVAL = 0, -1
CANARY32 = 0x7FC17FC1


@pytest.fixture(autouse=True)
def _memory_guard():
    with guarded.patched(hip):
        yield


def L():
    return hip.lib()


def st():
    return hip.stream()


def P(t, offset=0):
    """the address of a device tensor (+ floats), None for None"""
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


def put(a):
    return guarded.put(torch.from_numpy(np.array(a, order='C')), DEV)           # a copy: the cached lists are read-only


def new(*shape):
    return guarded.alloc(shape, torch.float32, DEV)


def untouched(t):
    return bool((t.contiguous().view(torch.int32) == CANARY32).all())


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def differ(got, want):
    """'' when the device tensor `got` holds exactly the float64 values `want`, else what differs (an unwritten NaN differs)"""
    got = host(got)
    if got.shape != want.shape:
        return 'shape %s, want %s' % (got.shape, want.shape)
    ne = got != want
    if not ne.any():
        return ''
    first = tuple(int(i) for i in np.argwhere(ne)[0])
    return '%d of %d differ, first at %s: got %r, want %r' % (int(ne.sum()), ne.size, first, got[first], want[first])


# ============================================================================================================================ xcorr
def xc_launch(entry, a, b, out, case, scale):
    hx, wx, hk, wk, p = case
    if entry == 'out':
        return L().usot_xcorr_depthwise_f32(st(), P(a), P(b), P(out), p, hx, wx, hk, wk)
    fn = L().usot_xcorr_depthwise_bwd_x_f32 if entry == 'dx' else L().usot_xcorr_depthwise_bwd_k_f32
    return fn(st(), P(a), P(b), P(out), p, hx, wx, hk, wk, scale)


def xc_args(entry, x, k, dout):
    return {'out': (x, k), 'dx': (dout, k), 'dk': (dout, x)}[entry]


def xc_run(x, k, dout, case, scale):
    """the three entry points on device operands -> {'out', 'dx', 'dk'} in guarded, NaN-prefilled outputs"""
    hx, wx, hk, wk, p = case
    res = {'out': new(p, hx - hk + 1, wx - wk + 1), 'dx': new(p, hx, wx), 'dk': new(p, hk, wk)}
    for e in cp.XC_ENTRIES:
        hip.check(xc_launch(e, *xc_args(e, x, k, dout), res[e], case, scale), e)
    return res


def xc_sweep(cases):
    bad = []
    for case in cases:
        ops, s = cp.xc_operands(case), cp.xc_scale(case)
        ref = cp.xc_ref(*ops, s)
        got = xc_run(*[put(a) for a in ops], case, s)
        bad += ['%s %s (%s): %s' % (case, e, cp.xc_kernel(case), m) for e in cp.XC_ENTRIES for m in [differ(got[e], ref[e])] if m]
    print('%d shapes x 3 entry points, %d failing' % (len(cases), len(bad)))
    assert not bad, bad[:20]


@pytest.mark.parametrize('t', cp.TEMPLATES)
def test_xcorr_every_wx(t):
    """Wx = Wk .. 66 at Hk + 1 rows and 9 planes (an odd count: the last wavefront's second half idles where two planes share one)"""
    xc_sweep(cp.wx_sweep(t))


@pytest.mark.parametrize('t', cp.TEMPLATES)
def test_xcorr_planes_around_the_block(t):
    xc_sweep(cp.p_sweep(t))


@pytest.mark.parametrize('t', [(1, 1), (2, 4), (7, 7), (5, 5)])
def test_xcorr_generic_templates(t):
    xc_sweep([c for c in cp.XC_GENERIC if c[2:4] == t])


@pytest.mark.parametrize('name', list(cp.XC_BIG))
def test_xcorr_past_the_grid_cap(name):
    """the second pass of the grid-stride loop: the big problem's planes are base planes picked by a seeded index on the device; the
    base result is held to float64, the big one to the gathered base result, bit for bit"""
    case, base_case = cp.XC_BIG[name], cp.xc_base(name)
    ops = cp.xc_operands(base_case)
    ref = cp.xc_ref(*ops, 0.5)
    base_d = [put(a) for a in ops]
    base = xc_run(*base_d, base_case, 0.5)
    for e in cp.XC_ENTRIES:
        assert not differ(base[e], ref[e]), (e, differ(base[e], ref[e]))
    idx = torch.from_numpy(cp.xc_big_index(name)).to(DEV)
    big_d = []
    for t in base_d:
        g = new(case[4], *t.shape[1:])
        torch.index_select(t, 0, idx, out=g)
        big_d.append(g)
    big = xc_run(*big_d, case, 0.5)
    n, first = cp.xc_counts(case), cp.xc_first_pass(case)
    bad = []
    for e in cp.XC_ENTRIES:
        assert big[e].numel() == n[e] and (e not in cp.XC_BIG_ENTRIES[name] or first[e] < n[e])
        want = base[e][idx]
        if not torch.equal(big[e], want):
            ne = (big[e] != want).reshape(-1).nonzero().reshape(-1)
            bad.append('%s %s: %d of %d elements differ from the gathered base, first at %d (one pass writes %d)'
                       % (name, e, ne.numel(), n[e], int(ne[0]), first[e]))
    assert not bad, bad


@pytest.mark.parametrize('case', cp.XC_ISOLATION)
def test_xcorr_inf_in_the_neighbouring_planes(case):
    """+Inf over every plane of one parity, in x, k and dout in turn: the planes of the other parity - the other half of the wavefront,
    the next wavefront of the block - still equal float64.  (The planes holding Inf are not compared.)"""
    ops, s = cp.xc_operands(case), cp.xc_scale(case)
    ref = cp.xc_ref(*ops, s)
    bad = []
    for which in range(3):
        for parity in (0, 1):
            planted = [a.copy() for a in ops]
            planted[which][parity::2] = np.inf
            got = xc_run(*[put(a) for a in planted], case, s)
            keep = slice(1 - parity, None, 2)
            bad += ['%s Inf in %s planes %d::2, %s: %s' % (case, 'xkd'[which], parity, e, m)
                    for e in cp.XC_ENTRIES for m in [differ(got[e][keep], ref[e][keep])] if m]
    assert not bad, bad[:10]


@pytest.mark.parametrize('entry', cp.XC_ENTRIES)
def test_xcorr_refusals(entry):
    case = (6, 9, 5, 5, 3)
    x, k, dout = [put(a) for a in cp.xc_operands(case)]
    a, b = xc_args(entry, x, k, dout)
    shape = {'out': (3, 2, 5), 'dx': (3, 6, 9), 'dk': (3, 5, 5)}[entry]
    out = new(*shape)
    bad = {'P -1': (6, 9, 5, 5, -1), 'Hk 0': (6, 9, 0, 5, 3), 'Wk 0': (6, 9, 5, 0, 3), 'Hk -1': (6, 9, -1, 5, 3),
           'Hx < Hk': (4, 9, 5, 5, 3), 'Wx < Wk': (6, 4, 5, 5, 3)}
    for what, c in bad.items():
        assert xc_launch(entry, a, b, out, c, 1.0) == EINVAL, what
    assert xc_launch(entry, None, b, out, case, 1.0) == EINVAL and xc_launch(entry, a, None, out, case, 1.0) == EINVAL
    assert xc_launch(entry, a, b, None, case, 1.0) == EINVAL
    assert xc_launch(entry, a, b, out, (6, 9, 5, 5, 0), 1.0) == OK                    # no planes: nothing to do, nothing written
    torch.cuda.synchronize()
    assert untouched(out)
    hip.check(xc_launch(entry, a, b, out, case, 1.0))
    assert not differ(out, cp.xc_ref(*cp.xc_operands(case), 1.0)[entry])


# ========================================================================================================================= PrRoIPool
PR_LISTS = [(ph, pw, s) for ph, pw in cp.PR_SHAPES for s in cp.PR_SCALES]


def dense(C_, H, W, PH, PW):
    """the eight strides of dense NCHW features and a dense [R][C][PH][PW] output"""
    return (C_ * H * W, H * W, W, 1, C_ * PH * PW, PH * PW, PW, 1)


def pr_forward(f, rois, out, ph, pw, scale, strides=None, R=None):
    B, C_, H, W = f.shape
    strides = strides or dense(C_, H, W, ph, pw)
    return L().usot_prroi_pool_forward_f32(st(), P(f), P(rois), P(out), len(rois) if R is None else R, C_, H, W, ph, pw, scale, *strides)


def pr_backward(rois, g, gin, shape, ph, pw, scale, R=None):
    B, C_, H, W = shape
    return L().usot_prroi_pool_backward_f32(st(), P(rois), P(g), P(gin), len(rois) if R is None else R, B, C_, H, W, ph, pw, scale)


def pr_coor(f, rois, top, g, groi, ph, pw, scale, R=None, B=None):
    B_, C_, H, W = f.shape
    return L().usot_prroi_pool_coor_backward_f32(st(), P(f), P(rois), P(top), P(g), P(groi), len(rois) if R is None else R,
                                                 B_ if B is None else B, C_, H, W, ph, pw, scale)


def pr_dev(ph, pw, scale):
    c = cp.pr_case(ph, pw, scale)
    return c, put(c['f']), put(c['rois']), put(c['g'])


@pytest.mark.parametrize('ph,pw,scale', PR_LISTS)
def test_prroi_forward_is_exact(ph, pw, scale):
    c, f, rois, g = pr_dev(ph, pw, scale)
    out = new(*c['out'].shape)
    hip.check(pr_forward(f, rois, out, ph, pw, scale))
    assert not differ(out, c['out']), differ(out, c['out'])


@pytest.mark.parametrize('ph,pw,scale', PR_LISTS)
def test_prroi_feature_gradient_is_exact(ph, pw, scale):
    c, f, rois, g = pr_dev(ph, pw, scale)
    gin = new(*c['f'].shape)
    hip.check(pr_backward(rois, g, gin, c['f'].shape, ph, pw, scale))
    assert not differ(gin, c['gin']), differ(gin, c['gin'])


@pytest.mark.parametrize('ph,pw,scale', PR_LISTS)
def test_prroi_roi_gradient(ph, pw, scale):
    """== where PH and PW are powers of two; at 7 x 7 and 3 x 5 (pw / PW not dyadic) the bar test_prroi_roi_gradient_vs_oracles holds
    bins of at least 0.2 pixel to, against the RoI's largest component"""
    c, f, rois, g = pr_dev(ph, pw, scale)
    top = put(c['out'].astype(np.float32))
    groi = new(len(c['rois']), 5)
    hip.check(pr_coor(f, rois, top, g, groi, ph, pw, scale))
    got, want = host(groi), c['groi']
    assert np.isfinite(got).all() and not got[:, 0].any() and not got[180:184].any()
    err = np.abs(got - want).max(1) / np.maximum(1.0, np.abs(want).max(1))
    print('%d x %d scale %g: largest error %.3g of the RoI\'s largest component' % (ph, pw, scale, err.max()))
    if (ph, pw) in cp.PR_ROI_EXACT:
        assert not differ(groi, want), differ(groi, want)
    else:
        assert np.all(err <= cp.PR_ROI_BAR), (err.max(), int(err.argmax()))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'nhwc_slice', 'out_slice'])
def test_prroi_forward_strides(layout):
    for ph, pw, scale in ((3, 5, 0.5), (4, 8, 1.0)):
        c = cp.pr_case(ph, pw, scale)
        B, C_, H, W = c['f'].shape
        R, rois = len(c['rois']), put(c['rois'])
        wide = C_ + 3
        if layout == 'nchw':
            f, off, fs = put(c['f']), 0, (C_ * H * W, H * W, W, 1)
        elif layout == 'nhwc':
            f, off, fs = put(c['f'].transpose(0, 2, 3, 1)), 0, (H * W * C_, 1, W * C_, C_)
        else:                                               # channels 2 .. 2 + C of a map of C + 3; the others hold NaN
            w = np.full((B, H, W, wide), np.nan, np.float32)
            w[..., 2:2 + C_] = c['f'].transpose(0, 2, 3, 1)
            f, off, fs = put(w), 2, (H * W * wide, 1, W * wide, wide)
        if layout == 'nchw':
            out, ooff, os_ = new(R, C_, ph, pw), 0, (C_ * ph * pw, ph * pw, pw, 1)
        elif layout == 'out_slice':                         # channels 1 .. 1 + C of an [R][C + 3][PH][PW] buffer
            out, ooff, os_ = new(R, wide, ph, pw), ph * pw, (wide * ph * pw, ph * pw, pw, 1)
        else:
            out, ooff, os_ = new(R, ph, pw, C_), 0, (ph * pw * C_, 1, pw * C_, C_)
        hip.check(L().usot_prroi_pool_forward_f32(st(), P(f, off), P(rois), P(out, ooff), R, C_, H, W, ph, pw, scale, *fs, *os_))
        if layout == 'out_slice':
            assert not differ(out[:, 1:1 + C_], c['out'])
            assert untouched(out[:, :1]) and untouched(out[:, 1 + C_:])
        elif layout == 'nchw':
            assert not differ(out, c['out'])
        else:
            assert not differ(out.permute(0, 3, 1, 2), c['out'])


def test_prroi_plan_op_equals_the_direct_launch():
    ph, pw, scale = 4, 8, 0.5
    c, f, rois, g = pr_dev(ph, pw, scale)
    direct, planned = new(*c['out'].shape), new(*c['out'].shape)
    hip.check(pr_forward(f, rois, direct, ph, pw, scale))
    B, C_, H, W = c['f'].shape
    plan = C.c_void_p(L().usot_plan_create())
    try:
        hip.check(L().usot_plan_add_prroi(plan, P(f), P(rois), P(planned), len(c['rois']), C_, H, W, ph, pw, scale,
                                          *dense(C_, H, W, ph, pw)))
        torch.cuda.synchronize()
        assert untouched(planned)                                        # recorded, not run
        hip.check(L().usot_plan_run(plan, st()))
        torch.cuda.synchronize()
    finally:
        L().usot_plan_destroy(plan)
    assert torch.equal(planned, direct) and not differ(planned, c['out'])


@pytest.mark.parametrize('which', ['forward', 'backward', 'coor'])
def test_prroi_reference_symbols_equal_the_entry_points(which):
    """PrRoIPooling{Forward,Backward,CoorBackward}Gpu on a dyadic list each: the bits of usot_prroi_pool_*; the gradients overwrite"""
    ph, pw, scale = {'forward': (4, 8, 1.0), 'backward': (3, 5, 0.5), 'coor': (8, 8, 0.5)}[which]
    c, f, rois, g = pr_dev(ph, pw, scale)
    B, C_, H, W = c['f'].shape
    top = put(c['out'].astype(np.float32))
    if which == 'forward':
        a, b = new(*c['out'].shape), new(*c['out'].shape)
        hip.check(pr_forward(f, rois, a, ph, pw, scale))
        L().PrRoIPoolingForwardGpu(st(), P(f), P(rois), P(b), C_, H, W, ph, pw, scale, b.numel())
        want = c['out']
    elif which == 'backward':
        a = new(*c['f'].shape)
        b = guarded.alloc(c['f'].shape, torch.float32, DEV, 'full', 3.0)
        hip.check(pr_backward(rois, g, a, c['f'].shape, ph, pw, scale))
        L().PrRoIPoolingBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(b), C_, H, W, ph, pw, scale, top.numel(), b.numel())
        want = c['gin']
    else:
        a = new(len(c['rois']), 5)
        b = guarded.alloc((len(c['rois']), 5), torch.float32, DEV, 'full', 3.0)
        hip.check(pr_coor(f, rois, top, g, a, ph, pw, scale))
        L().PrRoIPoolingCoorBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(b), C_, H, W, ph, pw, scale, top.numel(), b.numel())
        want = c['groi']
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not differ(b, want)


def test_prroi_forward_past_the_grid_cap():
    f, base = put(cp.pr_features()), put(cp.pr_big_base())
    want = ex.prroi_pool_exact(cp.pr_features(), cp.pr_big_base(), 7, 7, 1.0)
    small = new(cp.PR_BIG_BASE, cp.PR_MAP[1], 7, 7)
    hip.check(pr_forward(f, base, small, 7, 7, 1.0))
    assert not differ(small, want)
    idx = torch.from_numpy(cp.pr_big_index()).to(DEV)
    rois = new(cp.PR_BIG_R, 5)
    torch.index_select(base, 0, idx, out=rois)
    big = new(cp.PR_BIG_R, cp.PR_MAP[1], 7, 7)
    assert big.numel() > cp.PR_FWD_CAP
    hip.check(pr_forward(f, rois, big, 7, 7, 1.0))
    assert torch.equal(big, small[idx])


def test_prroi_feature_gradient_past_the_grid_cap():
    """5351 RoIs gathered from 64: the gradient is linear in top_diff, so it equals float64 on the 64 with top_diff summed per base RoI"""
    idx, g = cp.pr_big_index(), cp.pr_big_top_diff()
    tot, _ = cp.pr_big_summed(idx, g)
    want = ex.prroi_pool_exact_backward(cp.PR_MAP, cp.pr_big_base(), tot, 7, 7, 1.0)
    rois = put(cp.pr_big_base()[idx])
    gin = new(*cp.PR_MAP)
    assert g.size > cp.PR_FWD_CAP
    hip.check(pr_backward(rois, put(g), gin, cp.PR_MAP, 7, 7, 1.0))
    assert not differ(gin, want), differ(gin, want)


def test_prroi_roi_gradient_past_the_grid_cap():
    """260 channels at 8 x 8: 16 640 elements per RoI, the 64 blocks of a RoI go round twice"""
    fw, gw = cp.pr_features(C=cp.PR_WIDE_C, B=1, seed=3), cp.pr_top_diff(3, 8, 8, C=cp.PR_WIDE_C, seed=3)
    want = ex.prroi_pool_exact_coor_backward(fw, cp.PR_WIDE_ROIS, gw, 8, 8, 1.0)
    f, rois, g = put(fw), put(cp.PR_WIDE_ROIS), put(gw)
    top = new(3, cp.PR_WIDE_C, 8, 8)
    hip.check(pr_forward(f, rois, top, 8, 8, 1.0))
    assert not differ(top, ex.prroi_pool_exact(fw, cp.PR_WIDE_ROIS, 8, 8, 1.0))
    groi = new(3, 5)
    hip.check(pr_coor(f, rois, top, g, groi, 8, 8, 1.0))
    assert not differ(groi, want), differ(groi, want)


def test_prroi_roi_gradient_takes_65535_rois_and_refuses_65536():
    c = cp.pr_case(1, 1, 1.0)
    unit = cp.pr_unit_rows()
    rng = np.random.default_rng(65535)
    idx = rng.integers(0, len(c['rois']), cp.PR_MAX_R + 1)
    gv = rng.integers(-3, 4, cp.PR_MAX_R + 1).astype(np.float32)
    f, rois, g = put(c['f'][:, :1]), put(c['rois'][idx]), put(gv.reshape(-1, 1, 1, 1))
    top = new(cp.PR_MAX_R + 1, 1, 1, 1)
    hip.check(pr_forward(f, rois, top, 1, 1, 1.0))
    groi = new(cp.PR_MAX_R + 1, 5)
    assert pr_coor(f, rois, top, g, groi, 1, 1, 1.0) == EINVAL                     # gridDim.y = R
    torch.cuda.synchronize()
    assert untouched(groi)
    hip.check(pr_coor(f, rois, top, g, groi, 1, 1, 1.0, R=cp.PR_MAX_R))
    want = unit[idx] * gv[:, None].astype(np.float64)
    assert not differ(groi[:cp.PR_MAX_R], want[:cp.PR_MAX_R]) and untouched(groi[cp.PR_MAX_R:])


def test_prroi_gradients_skip_batch_indices_outside_the_batch():
    """index -1 and B: no contribution to the feature gradient, a zero row of the RoI gradient.  The forward is NOT given such a RoI: it
    carries no batch count and, like the reference's, would read outside the map."""
    ph, pw, scale = 4, 8, 1.0
    c = cp.pr_case(ph, pw, scale)
    rois = c['rois'].copy()
    out_of = np.zeros(len(rois), bool)
    out_of[3::7] = True
    rois[3::14, 0], rois[10::14, 0] = -1.0, cp.PR_MAP[0]
    assert set(rois[out_of, 0]) == {-1.0, 2.0} and set(rois[~out_of, 0]) == {0.0, 1.0}
    g = c['g'].copy()
    g[out_of] = 3.0
    rd, gd, f = put(rois), put(g), put(c['f'])
    gin = new(*cp.PR_MAP)
    hip.check(pr_backward(rd, gd, gin, cp.PR_MAP, ph, pw, scale))
    want = ex.prroi_pool_exact_backward(cp.PR_MAP, rois[~out_of], g[~out_of], ph, pw, scale)
    assert not differ(gin, want), differ(gin, want)
    top = c['out'].astype(np.float32).copy()
    top[out_of] = 1.0
    groi = new(len(rois), 5)
    hip.check(pr_coor(f, rd, put(top), gd, groi, ph, pw, scale))
    want = c['groi'].copy()
    want[out_of] = 0.0
    assert not differ(groi, want), differ(groi, want)


def test_prroi_forward_with_inf_behind_an_aligned_edge():
    """bins ending exactly on a pixel, +Inf in the next column and row: a cell walk that goes one cell too far (floor + 1 for ceil)
    meets it with weight 0 and stores NaN"""
    ph, pw = cp.PR_INF_SHAPE
    fi = cp.pr_inf_features()
    want = ex.prroi_pool_exact(np.where(np.isinf(fi), 0.0, fi), cp.PR_INF_ROIS, ph, pw, 1.0)
    out = new(*want.shape)
    hip.check(pr_forward(put(fi), put(cp.PR_INF_ROIS), out, ph, pw, 1.0))
    assert not differ(out, want), differ(out, want)


DIMS = ('R', 'B', 'C', 'H', 'W', 'PH', 'PW')


def test_prroi_forward_refusals():
    ph, pw, scale = 2, 1, 1.0
    c, f, rois, g = pr_dev(ph, pw, scale)
    B, C_, H, W = c['f'].shape
    R = len(c['rois'])
    out = new(R, C_, ph, pw)
    good = dict(R=R, C=C_, H=H, W=W, PH=ph, PW=pw)

    def call(fp=f, rp=rois, op=out, **kw):
        d = dict(good, **kw)
        return L().usot_prroi_pool_forward_f32(st(), P(fp), P(rp), P(op), d['R'], d['C'], d['H'], d['W'], d['PH'], d['PW'], scale,
                                               *dense(C_, H, W, ph, pw))
    for name in ('C', 'H', 'W', 'PH', 'PW'):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(R=-1) == EINVAL
    assert call(fp=None) == EINVAL and call(rp=None) == EINVAL and call(op=None) == EINVAL
    assert call(R=0) == OK
    L().PrRoIPoolingForwardGpu(st(), P(f), P(rois), P(out), C_, H, W, ph, pw, scale, out.numel() - 1)
    L().PrRoIPoolingForwardGpu(st(), P(f), P(rois), P(out), 0, H, W, ph, pw, scale, out.numel())
    L().PrRoIPoolingForwardGpu(st(), P(f), P(rois), P(out), C_, H, W, ph, pw, scale, -C_ * ph * pw)
    torch.cuda.synchronize()
    assert untouched(out)
    assert call() == OK and not differ(out, c['out'])


def test_prroi_feature_gradient_refusals():
    ph, pw, scale = 2, 1, 1.0
    c, f, rois, g = pr_dev(ph, pw, scale)
    B, C_, H, W = c['f'].shape
    R = len(c['rois'])
    gin = new(B, C_, H, W)
    top = put(c['out'].astype(np.float32))
    good = dict(R=R, B=B, C=C_, H=H, W=W, PH=ph, PW=pw)

    def call(rp=rois, gp=g, op=gin, **kw):
        d = dict(good, **kw)
        return L().usot_prroi_pool_backward_f32(st(), P(rp), P(gp), P(op), *[d[n] for n in DIMS], scale)
    for name in DIMS[1:]:
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(R=-1) == EINVAL
    assert call(rp=None) == EINVAL and call(gp=None) == EINVAL and call(op=None) == EINVAL
    for top_count, bottom_count in ((top.numel() - 1, gin.numel()), (top.numel(), gin.numel() - 1), (top.numel(), 0), (-1, gin.numel())):
        L().PrRoIPoolingBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(gin), C_, H, W, ph, pw, scale, top_count, bottom_count)
    L().PrRoIPoolingBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(gin), C_, H, W, 0, pw, scale, top.numel(), gin.numel())
    torch.cuda.synchronize()
    assert untouched(gin)
    # no RoIs: the gradient is zero, and the two lists need not exist
    assert call(R=0, rp=None, gp=None) == OK
    torch.cuda.synchronize()
    assert not differ(gin, np.zeros((B, C_, H, W)))
    assert call() == OK and not differ(gin, c['gin'])


def test_prroi_roi_gradient_refusals():
    ph, pw, scale = 2, 1, 1.0
    c, f, rois, g = pr_dev(ph, pw, scale)
    B, C_, H, W = c['f'].shape
    R = len(c['rois'])
    top = put(c['out'].astype(np.float32))
    groi = new(R, 5)
    good = dict(R=R, B=B, C=C_, H=H, W=W, PH=ph, PW=pw)
    ptrs = dict(f=f, r=rois, t=top, g=g, o=groi)

    def call(null=None, **kw):
        d, p = dict(good, **kw), dict(ptrs)
        if null:
            p[null] = None
        return L().usot_prroi_pool_coor_backward_f32(st(), P(p['f']), P(p['r']), P(p['t']), P(p['g']), P(p['o']),
                                                     *[d[n] for n in DIMS], scale)
    for name in DIMS[1:]:
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(R=-1) == EINVAL
    for null in ptrs:
        assert call(null=null) == EINVAL, null
    assert call(R=0) == OK                                                      # nothing to do: not even zeroed
    for top_count, bottom_count in ((top.numel(), groi.numel() - 5), (top.numel() - 1, groi.numel()), (top.numel(), groi.numel() + 5)):
        L().PrRoIPoolingCoorBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(groi), C_, H, W, ph, pw, scale, top_count, bottom_count)
    L().PrRoIPoolingCoorBackwardGpu(st(), P(f), P(rois), P(top), P(g), P(groi), C_, H, W, ph, 0, scale, top.numel(), groi.numel())
    torch.cuda.synchronize()
    assert untouched(groi)
    assert call() == OK and not differ(groi, c['groi'])
