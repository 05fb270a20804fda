"""GPU: where the LAST TILE ends.  The exact-fp32 kernels at every pixel residue and every channel residue of their tiles: the
small-M fp32 kernels (csrc/smallm_f32.hip, 16-pixel tiles behind a `m < M` mask) at every M = 1 .. 49 - every residue of
M mod 16 at zero, one and two full tiles, whole numbers of tiles included - and on every 3x3 geometry of up to 3 x 4 x 9 pixels;
the routed conv_igemm tiles (csrc/conv_igemm.hip) at M = bm - 1, bm, bm + 1, ... 2 bm + 1, at Cout = 1 .. 2 bn + 1 (scalar
stores, half-used tiles) and under split-K at a ragged row-and-channel corner.

Every launch follows tests/test_gpu_memory_contract.py: inputs placed with a NaN on both sides and compared bit for bit
afterwards, outputs NaN-prefilled between canaries, split-K / slice workspaces NaN-prefilled as well (only their ticket words
start at zero, and must be zero again afterwards), no NaN in a result, parity against a float64 CPU reference at the bar of the
kernel's own parity test (1e-5 small-M, 2e-5 conv tiles, tests/test_gpu_ops.py: rel_err).  rel_err's floor is the mean |ref| of
the rows compared; the smallest comparison here has 17 values (Cout = 1 at M = bm + 1) and every M = 1 case has >= 32 channels,
so the floor is never ill-posed and is used unchanged.

Pointwise kernels run ONE seeded problem of M_max rows on its first M rows, each M in an allocation of exactly M rows, against
the first M rows of ONE float64 reference.  A row's result depends on its own inputs only and its lane is m % 16 whatever M is,
so with the same instantiation, slice count and ksplit the result must also be BIT-equal to the first M rows of the M_max run.

One item = one (kernel, shape, form); it loops over its list.  The lists are asserted by tests/test_tile_edge_lists.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402
from test_gpu_memory_contract import contract, no_nan  # noqa: E402
from test_gpu_ops import pack_w, rel_err  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
RELU, NONE = hip.ACT_RELU, hip.ACT_NONE

# ---------------------------------------------------------------------------------------------------------------- the lists
PW_M = list(range(1, 50))                         # every residue at 0, 1 and 2 full tiles, and the 2 -> 3 tile boundary
DEFER_M = [1, 15, 16, 17, 32, 33]
PAIR_SHAPES = [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256), (256, 1024, 256)]
PAIR_SLICED = [(128, 512, 128), (256, 1024, 256)]                 # usot_pw_pair_f32_ws_floats > 0 at these M
PAIR_FORMS = [(s, 'default') for s in PAIR_SHAPES] + [((128, 512, 128), 'unsliced'), ((256, 1024, 256), 'split16')]
SINGLE_SHAPES = [(1024, 256), (256, 1024), (512, 128), (128, 512)]
STREAM_SHAPES = [(256, 256), (128, 128)]
TRIPLE_SHAPES = [(64, 64, 256, 64), (64, 64, 256, 128), (128, 128, 512, 128)]
GRID = [(nb, h, w) for nb in (1, 2, 3) for h in (1, 2, 3, 4) for w in range(1, 10)]       # OH = H, OW = W (pad = dil)


def b1_m_list(bm):
    return [1, 2, 3] + [16 * j + d for j in range(1, 2 * bm // 16 + 1) for d in (-1, 0, 1)]


def b2_cout_list(bn):
    return sorted({1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, bn - 1, bn, bn + 1, 2 * bn - 4, 2 * bn + 1})


def b3_cases(bm, bn):
    return [(bm - 1, bn + 1), (bm + 1, 4), (17, 33), (2 * bm, bn)]


def sweep_tiles():
    """Every conv tile id the in-tree library holds (host-side query): on the default build exactly the routed ones.  An
    experiments build also holds tiles with a launch protocol of their own (weight-stationary, stream-K, fragment-order or
    split input maps): those are outside this sweep, whose launcher packs row-major and split-fp16 banks only."""
    L = conftest._lib()
    if L is None:
        return []
    ids = [t for t in range(1, L.usot_conv_tile_count() + 1) if L.usot_conv_tile_built(t)]
    if L.usot_experiments_built():
        ids = [t for t in ids if not (L.usot_conv_tile_kreq(t, None) or L.usot_conv_tile_streamk(t) or L.usot_conv_tile_xsplit(t)
                                      or L.usot_conv_tile_wfrag(t) == 1)]
    return ids


TILES = conftest.tile_params(sweep_tiles())


def report(family, what, worst, label='worst rel_err'):
    print('tile_edges %s %s: %s %.3g' % (family, what, label, worst))


def _act(v, act):
    return v.relu() if act == RELU else v


# ------------------------------------------------------------------------------------------------- A. small-M fp32 kernels
def _pair_problem(cm, co, cn, M, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    t2 = torch.randn(M, cm, generator=g)
    if positive:
        t2 = t2.abs()
    w3 = torch.randn(co, cm, generator=g) / np.sqrt(cm)
    b3 = torch.randn(co, generator=g)
    res = torch.randn(M, co, generator=g)
    w1 = torch.randn(cn, co, generator=g) / np.sqrt(co)
    b1 = torch.randn(cn, generator=g)
    return t2, w3, b3, res, w1, b1


def _pair_ref(t2, w3, b3, res, w1, b1, act2):
    y = (t2.double() @ w3.double().t() + b3.double() + res.double()).relu()
    return y, _act(y @ w1.double().t() + b1.double(), act2)


def _pair_ws(c, M, cm, co, cn):
    """(workspace or None, first ticket word): the slabs hold the NaN pattern, the ticket words behind them zero"""
    n = int(hip.lib().usot_pw_pair_f32_ws_floats(M, cm, co, cn))
    if n <= 0:
        return None, 0
    ws = c.out((n,))
    ws[n - (M + 15) // 16:].zero_()
    return ws, n - (M + 15) // 16


def _pair_launch(c, shape, M, t2, w3p, b3, res, w1p, b1, act2, ws, split16=False, ovf=None, **parts):
    cm, co, cn = shape
    y, t = c.out((M, co)), c.out((M, cn))
    kw = {k: (v.data_ptr() if hasattr(v, 'data_ptr') else v) for k, v in parts.items()}
    d = hip.pw_pair_desc(t2.data_ptr(), w3p.data_ptr(), b3.data_ptr(), res.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1.data_ptr(),
                         t.data_ptr(), M, cm, co, cn, act2, ws.data_ptr() if ws is not None else None,
                         ovf=ovf.data_ptr() if ovf is not None else None, **kw)
    fn = hip.lib().usot_pw_pair_f32s if split16 else hip.lib().usot_pw_pair_f32
    hip.check(fn(hip.stream(), C.byref(d)), 'pw_pair_f32 %s M = %d' % (shape, M))
    return y, t


@pytest.mark.parametrize('act2', [RELU, NONE], ids=['relu', 'none'])
@pytest.mark.parametrize('shape,form', PAIR_FORMS, ids=['%d_%d_%d_%s' % (s + (f,)) for s, f in PAIR_FORMS])
def test_pw_pair_f32_every_pixel_residue(shape, form, act2):
    """A1.  `default` is the form the frame runs (channel-sliced where the library asks for a workspace: launched twice on one
    workspace, both launches checked, tickets zero afterwards), `unsliced` the same shape without a workspace, `split16` the
    split-fp16 form (non-negative t2, range word stays 0)."""
    cm, co, cn = shape
    split16 = form == 'split16'
    mx = max(PW_M)
    t2, w3, b3, res, w1, b1 = _pair_problem(cm, co, cn, mx, cm + co + cn + act2, positive=split16)
    y64, t64 = _pair_ref(t2, w3, b3, res, w1, b1, act2)
    pack = hip.pw_pair_s16_pack if split16 else hip.pw_pair_f32_pack
    worst = 0.0
    with contract() as c:
        w3p, w1p, b3d, b1d = c.puts(pack(w3.to(DEV)), pack(w1.to(DEV)), b3, b1)
        ovf = c.out((1,), torch.int32, 'zero')

        def run(M):
            t2d, rd = c.puts(t2[:M].contiguous(), res[:M].contiguous())
            ws, tick = _pair_ws(c, M, cm, co, cn) if form != 'unsliced' else (None, 0)
            assert (ws is not None) == (form != 'unsliced' and shape in PAIR_SLICED), M
            outs = [_pair_launch(c, shape, M, t2d, w3p, b3d, rd, w1p, b1d, act2, ws, split16, ovf if split16 else None)
                    for _ in range(2 if ws is not None else 1)]
            for y, t in outs:
                no_nan(y, t)
            if ws is not None:                      # the second launch found the tickets reset, and left them so
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), M
                assert not bool(ws[tick:].view(torch.int32).any()), M
            return outs[-1]

        ymax, tmax = run(mx)
        for M in PW_M:
            y, t = run(M)
            ey, et = rel_err(y.cpu().numpy(), y64[:M].numpy()), rel_err(t.cpu().numpy(), t64[:M].numpy())
            worst = max(worst, ey, et)
            assert ey < 1e-5 and et < 1e-5, (M, ey, et)
            assert torch.equal(y, ymax[:M]) and torch.equal(t, tmax[:M]), M
        assert int(ovf.item()) == 0
    report('A1', 'pair %s %s act2=%d' % (shape, form, act2), worst)


@pytest.mark.parametrize('shape', [(256, 1024, 256), (128, 512, 128)], ids=['256_1024_256', '128_512_128'])
def test_pw_pair_f32_deferred_parts_at_ragged_m(shape):
    """A2.  t2 and the residual as three partial sums each (usot_pw_pair_desc.t2_parts / res_parts; the part stride is M rows, so a
    ragged M moves every part): float64 of parts + bias (+ ReLU for t2), and bit-equality with the same launch on the tiles
    summed beforehand in the kernel's order."""
    cm, co, cn = shape
    mx = max(DEFER_M)
    g = torch.Generator().manual_seed(cm + cn + 3)
    tp, rp = torch.randn(3, mx, cm, generator=g), torch.randn(3, mx, co, generator=g)
    tb, rb = torch.randn(cm, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1
    _, w3, b3, _, w1, b1 = _pair_problem(cm, co, cn, 1, cm + 7)
    tsum = (((tp[0] + tp[1]) + tp[2]) + tb).relu()                  # the kernel's order: part 0, 1, 2, then the bias
    rsum = ((rp[0] + rp[1]) + rp[2]) + rb
    y64, t64 = _pair_ref((tp.double().sum(0) + tb.double()).relu(), w3, b3, rp.double().sum(0) + rb.double(), w1, b1, RELU)
    worst = 0.0
    with contract() as c:
        w3p, w1p, b3d, b1d, tbd, rbd = c.puts(hip.pw_pair_f32_pack(w3.to(DEV)), hip.pw_pair_f32_pack(w1.to(DEV)), b3, b1, tb, rb)
        for M in DEFER_M:
            tpd, rpd, tsd, rsd = c.puts(tp[:, :M].contiguous(), rp[:, :M].contiguous(), tsum[:M].contiguous(), rsum[:M].contiguous())
            ws, tick = _pair_ws(c, M, cm, co, cn)
            assert ws is not None
            y, t = _pair_launch(c, shape, M, tpd, w3p, b3d, rpd, w1p, b1d, RELU, ws, t2_parts=3, t2_bias=tbd, res_parts=3, res_bias=rbd)
            ys, ts = _pair_launch(c, shape, M, tsd, w3p, b3d, rsd, w1p, b1d, RELU, ws)
            no_nan(y, t, ys, ts)
            assert not bool(ws[tick:].view(torch.int32).any()), M
            assert torch.equal(y, ys) and torch.equal(t, ts), M
            ey, et = rel_err(y.cpu().numpy(), y64[:M].numpy()), rel_err(t.cpu().numpy(), t64[:M].numpy())
            worst = max(worst, ey, et)
            assert ey < 1e-5 and et < 1e-5, (M, ey, et)
    report('A2', 'deferred pair %s' % (shape,), worst)


@pytest.mark.parametrize('act', [RELU, NONE], ids=['relu', 'none'])
@pytest.mark.parametrize('res', [True, False], ids=['res', 'plain'])
@pytest.mark.parametrize('K,N', SINGLE_SHAPES)
def test_pw_single_f32_every_pixel_residue(K, N, res, act):
    """A3."""
    mx = max(PW_M)
    g = torch.Generator().manual_seed(K + N + act + 2 * res)
    x = torch.randn(mx, K, generator=g)
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(mx, N, generator=g) if res else None
    ref = _act(x.double() @ w.double().t() + b.double() + (r.double() if res else 0), act)
    worst = 0.0
    with contract() as c:
        wp, bd = c.puts(hip.pw_pair_f32_pack(w.to(DEV)), b)

        def run(M):
            xd, rd = c.puts(x[:M].contiguous(), r[:M].contiguous() if res else None)
            y = c.out((M, N))
            hip.check(hip.lib().usot_pw_single_f32(hip.stream(), hip.ptr(xd), hip.ptr(wp), hip.ptr(bd), hip.ptr(rd), hip.ptr(y), M, K, N, act),
                      'pw_single_f32 M = %d' % M)
            return y

        ymax = run(mx)
        for M in PW_M:
            y = run(M)
            no_nan(y)
            e = rel_err(y.cpu().numpy(), ref[:M].numpy())
            worst = max(worst, e)
            assert e < 1e-5, (M, e)
            assert torch.equal(y, ymax[:M]), M
    report('A3', 'single (%d, %d) res=%d act=%d' % (K, N, res, act), worst)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('pd', [1, 2], ids=['pd1', 'pd2'])
@pytest.mark.parametrize('cin,n', STREAM_SHAPES)
def test_stream_conv3x3_f32_every_small_geometry(cin, n, pd):
    """A4.  Every map of GRID at pad = dil = pd (pd1: residual + ReLU, pd2: residual, no activation): every residue of M mod 16,
    M < 16, a tile spanning three images, rows and columns shorter than the dilation (every off-centre tap is padding)."""
    act = RELU if pd == 1 else NONE
    g = torch.Generator().manual_seed(cin + n + pd)
    x = torch.randn(3, cin, 4, 9, generator=g)
    w = torch.randn(n, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b = torch.randn(n, generator=g)
    r = torch.randn(3, 4, 9, n, generator=g)
    worst = 0.0
    with contract() as c:
        wp, bd = c.puts(hip.pw_pair_f32_pack(pack_w(w).to(DEV)), b)
        for nb, h, w_ in GRID:
            xs, rs = x[:nb, :, :h, :w_], r[:nb, :h, :w_].contiguous()
            ref = _act(F.conv2d(xs.double(), w.double(), b.double(), 1, pd, pd).permute(0, 2, 3, 1) + rs.double(), act)
            xd, rd = c.puts(_nhwc(xs), rs)
            y = c.out((nb, h, w_, n))
            hip.check(hip.lib().usot_stream_conv3x3_f32(hip.stream(), hip.ptr(xd), hip.ptr(wp), hip.ptr(bd), hip.ptr(rd), hip.ptr(y),
                                                        nb, h, w_, cin, h, w_, n, pd, pd, pd, pd, act), 'stream_conv3x3_f32 %s' % ((nb, h, w_),))
            no_nan(y)
            e = rel_err(y.cpu().numpy(), ref.numpy())
            worst = max(worst, e)
            assert e < 1e-5, (nb, h, w_, e)
    report('A4', 'streamed (%d, %d) pd%d' % (cin, n, pd), worst)


@pytest.mark.parametrize('pd', [1, 2], ids=['pd1', 'pd2'])
@pytest.mark.parametrize('cin,cm,co,cn', TRIPLE_SHAPES)
def test_pw_triple_f32_every_small_geometry(cin, cm, co, cn, pd):
    """A4.  The bottleneck tail in one launch on every map of GRID at pad = dil = pd, against float64 conv2d and the float64 pair."""
    g = torch.Generator().manual_seed(cin + cn + pd)
    x = torch.randn(3, cin, 4, 9, generator=g)
    w2 = torch.randn(cm, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b2 = torch.randn(cm, generator=g)
    _, w3, b3, _, w1, b1 = _pair_problem(cm, co, cn, 1, cin + cn + pd + 1)
    r = torch.randn(3, 4, 9, co, generator=g)
    worst = 0.0
    with contract() as c:
        pk = lambda t: hip.pw_pair_f32_pack(t.to(DEV))
        w2p, b2d, w3p, b3d, w1p, b1d = c.puts(pk(pack_w(w2)), b2, pk(w3), b3, pk(w1), b1)
        for nb, h, w_ in GRID:
            M = nb * h * w_
            xs, rs = x[:nb, :, :h, :w_], r[:nb, :h, :w_].contiguous()
            t2 = F.conv2d(xs.double(), w2.double(), b2.double(), 1, pd, pd).relu().permute(0, 2, 3, 1).reshape(M, cm)
            y64, t64 = _pair_ref(t2, w3, b3, rs.reshape(M, co), w1, b1, RELU)
            xd, rd = c.puts(_nhwc(xs), rs)
            y, t = c.out((M, co)), c.out((M, cn))
            d = hip.pw_pair_desc(None, w3p.data_ptr(), b3d.data_ptr(), rd.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1d.data_ptr(), t.data_ptr(),
                                 M, cm, co, cn, RELU)
            hip.check(hip.lib().usot_pw_triple_f32(hip.stream(), hip.ptr(xd), hip.ptr(w2p), hip.ptr(b2d), C.byref(d), nb, h, w_, cin, h, w_,
                                                   pd, pd, pd, pd), 'pw_triple_f32 %s' % ((nb, h, w_),))
            no_nan(y, t)
            ey, et = rel_err(y.cpu().numpy(), y64.numpy()), rel_err(t.cpu().numpy(), t64.numpy())
            worst = max(worst, ey, et)
            assert ey < 1e-5 and et < 1e-5, (nb, h, w_, ey, et)
    report('A4', 'triple %s pd%d' % ((cin, cm, co, cn), pd), worst)


# ------------------------------------------------------------------------------------------------- B. routed conv_igemm tiles
def _conv_bank(c, tile, w, b):
    """packed [Cout][K] filters and bias -> guarded device copies in the layout the tile reads: (w, w_scale or None, bias, w_frag)"""
    frag = hip.tile_wfrag(tile)
    assert frag in (0, 2), (tile, frag)
    wd = w.to(DEV)
    if frag == 2:
        wd, sc = hip.split16_pack(wd)
        return c.put(wd), c.put(sc), c.put(b), frag
    return c.put(wd), None, c.put(b), frag


def _conv_setup(c, tile, x, bank, *, Cout, KH=1, KW=1, pad=(0, 0), res=None, act=NONE, ksplit=1, y_nchw=False, ovf=None, y=None,
                xshape=None, stride=1, dil=(1, 1), **fields):
    """descriptor of one usot_conv2d_f32 launch (stride 1, dilation 1 unless given) -> (desc, y, ws, first ticket word); the
    split-K workspace holds the NaN pattern in its slabs and zero ticket words.  `y`: an output the caller made (a channel slice,
    group gaps: the caller checks it, prefill included); `xshape`: (N, H, W, Cin) of one group when x is a flat buffer of several;
    `fields`: the remaining descriptor fields, passed through (act2, act_split, y_cstride, y_coff, res_cstride, res_coff, groups,
    *_gs)."""
    wd, sc, bd, frag = bank
    N, H, W_, Cin = xshape or x.shape
    OH, OW = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // stride + 1, (W_ + 2 * pad[1] - dil[1] * (KW - 1) - 1) // stride + 1
    M = N * OH * OW
    G = fields.get('groups', 1)
    if y is None:
        assert G == 1
        y = c.out((N, Cout, OH, OW) if y_nchw else (N, OH, OW, Cout))
    ws, tick = None, 0
    if ksplit > 1:
        tick = ksplit * G * M * Cout
        ws = c.out((tick + G * ((M + 15) // 16) * ((Cout + 31) // 32),))
        ws[tick:].zero_()
    d = hip.conv_desc(x.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N=N, H=H, W=W_, Cin=Cin, OH=OH, OW=OW, Cout=Cout, KH=KH, KW=KW,
                      stride=stride, pad=pad, dil=dil, res=res.data_ptr() if res is not None else None, act=act, tile=tile, ksplit=ksplit,
                      ws=ws.data_ptr() if ws is not None else None, y_nchw=int(y_nchw), w_frag=frag,
                      w_scale=sc.data_ptr() if sc is not None else None, ovf=ovf.data_ptr() if ovf is not None else None, **fields)
    return d, y, ws, tick


def _conv(c, tile, x, bank, *, Cout, ksplit=1, y=None, **kw):
    """one usot_conv2d_f32 launch through its descriptor (_conv_setup); no NaN in an output made here, and the ticket words of
    the split-K workspace must be zero again afterwards"""
    d, out, ws, tick = _conv_setup(c, tile, x, bank, Cout=Cout, ksplit=ksplit, y=y, **kw)
    hip.check(hip.lib().usot_conv2d_f32(hip.stream(), C.byref(d)), 'usot_conv2d_f32 tile %d Cout = %d ksplit = %d' % (tile, Cout, ksplit))
    if y is None:
        no_nan(out)
    if ws is not None:
        assert not bool(ws[tick:].view(torch.int32).any()), (tile, Cout, ksplit)
    return out


def _pw_problem(M, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 64, generator=g)
    w = torch.randn(Cout, 64, generator=g) / 8
    b = torch.randn(Cout, generator=g)
    res = torch.randn(M, Cout, generator=g)
    return x, w, b, res, x.double() @ w.double().t() + b.double()


@pytest.mark.parametrize('form', ['plain', 'res_relu'])
@pytest.mark.parametrize('tile', TILES)
def test_conv_tile_every_pixel_edge(tile, form):
    """B1.  1x1, Cin = 64, Cout = bn, x [1, 1, M, 64] at M = 1, 2, 3 and 16 j - 1, 16 j, 16 j + 1 up to 2 bm + 1."""
    bm, bn = hip.tile_table()[tile]
    ms = b1_m_list(bm)
    mx = max(ms)
    x, w, b, res, ref = _pw_problem(mx, bn, 100 + tile)
    if form == 'res_relu':
        ref = (ref + res.double()).relu()
    worst = 0.0
    with contract() as c:
        bank = _conv_bank(c, tile, w, b)

        def run(M):
            xd, rd = c.puts(x[:M].reshape(1, 1, M, 64).contiguous(), res[:M].contiguous() if form == 'res_relu' else None)
            return _conv(c, tile, xd, bank, Cout=bn, res=rd, act=RELU if form == 'res_relu' else NONE).reshape(M, bn)

        ymax = run(mx)
        for M in ms:
            y = run(M)
            e = rel_err(y.cpu().numpy(), ref[:M].numpy())
            worst = max(worst, e)
            assert e < 2e-5, (tile, M, e)
            assert torch.equal(y, ymax[:M]), (tile, M)
    report('B1', 'tile %d (%d x %d) %s' % (tile, bm, bn, form), worst)


def test_conv_heuristic_tile_switches_at_192_pixels():
    """B1.  tile = 0 at M = 192 and 193: pick_tile()'s last M for the 16 x 64 tile and the first one past it."""
    x, w, b, res, ref = _pw_problem(193, 64, 99)
    worst = 0.0
    with contract() as c:
        bank = _conv_bank(c, 0, w, b)
        picked = []
        for M in (192, 193):
            xd = c.put(x[:M].reshape(1, 1, M, 64).contiguous())
            d = hip.conv_desc(xd.data_ptr(), bank[0].data_ptr(), None, xd.data_ptr(), N=1, H=1, W=M, Cin=64, OH=1, OW=M, Cout=64, KH=1, KW=1)
            picked.append(int(hip.lib().usot_conv_resolve_tile(C.byref(d))))
            y = _conv(c, 0, xd, bank, Cout=64).reshape(M, 64)
            e = rel_err(y.cpu().numpy(), ref[:M].numpy())
            worst = max(worst, e)
            assert e < 2e-5, (M, e)
        assert picked[0] == 8 and picked[1] != 8, picked
    report('B1', 'tile 0 at M = 192 | 193 (tiles %s)' % (picked,), worst)


@pytest.mark.parametrize('layout', ['nhwc_res_relu', 'nchw'])
@pytest.mark.parametrize('tile', TILES)
def test_conv_tile_every_channel_edge(tile, layout):
    """B2.  The same conv at M = bm + 1 on the first Cout filters of one bank of 2 bn + 1: vector and scalar stores, a tile with
    one live channel, bn - 1, bn + 1; NHWC with residual + ReLU, NCHW plain.  Every routed tile accepts every Cout."""
    bm, bn = hip.tile_table()[tile]
    M, couts = bm + 1, b2_cout_list(bn)
    x, w, b, res, ref = _pw_problem(M, max(couts), 200 + tile)
    worst = 0.0
    with contract() as c:
        xd = c.put(x.reshape(1, 1, M, 64).contiguous())
        for co in couts:
            bank = _conv_bank(c, tile, w[:co].contiguous(), b[:co].contiguous())
            if layout == 'nchw':
                got = _conv(c, tile, xd, bank, Cout=co, y_nchw=True).reshape(co, M).t()
                want = ref[:, :co]
            else:
                rd = c.put(res[:, :co].contiguous())
                got = _conv(c, tile, xd, bank, Cout=co, res=rd, act=RELU).reshape(M, co)
                want = (ref[:, :co] + res[:, :co].double()).relu()
            e = rel_err(got.cpu().numpy(), want.numpy())
            worst = max(worst, e)
            assert e < 2e-5, (tile, co, e)
    report('B2', 'tile %d (%d x %d) %s' % (tile, bm, bn, layout), worst)


@pytest.mark.parametrize('ksplit', [2, 3])
@pytest.mark.parametrize('tile', TILES)
def test_conv_tile_splitk_at_a_ragged_corner(tile, ksplit):
    """B3.  3x3, Cin = 64, x [1, 3, M, 64], pad (0, 1): OH = 1, OW = M, K = 576, all three filter rows real data.  The in-launch
    combine at a ragged row AND channel corner, with ReLU; the split-fp16 tiles' range word stays 0."""
    bm, bn = hip.tile_table()[tile]
    worst = 0.0
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        for M, co in b3_cases(bm, bn):
            g = torch.Generator().manual_seed(300 + tile + M + co)
            x = torch.randn(1, 64, 3, M, generator=g)
            w = torch.randn(co, 64, 3, 3, generator=g) / 24
            b = torch.randn(co, generator=g)
            ref = F.conv2d(x.double(), w.double(), b.double(), 1, (0, 1)).relu()
            bank = _conv_bank(c, tile, pack_w(w), b)
            y = _conv(c, tile, c.put(_nhwc(x)), bank, Cout=co, KH=3, KW=3, pad=(0, 1), act=RELU, ksplit=ksplit,
                      ovf=ovf if bank[3] == 2 else None)
            e = rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy())
            worst = max(worst, e)
            assert e < 2e-5, (tile, M, co, e)
        assert int(ovf.item()) == 0
    report('B3', 'tile %d (%d x %d) ksplit %d' % (tile, bm, bn, ksplit), worst)
