"""GPU: the memory contract of every routed entry point - one small ragged case each, EVERY input placed with guarded.put (a NaN
on both sides of it) and every output with guarded.alloc (NaN-filled, between canaries; tests/guarded.py).  Asserted: the result
meets the bar of the entry point's parity test against a float64 CPU reference, holds no NaN (an element nobody wrote, or a read
of memory nobody wrote that reached the result), no guard is damaged, and the inputs are bit-unchanged.

Shapes are the smallest ragged rows of the existing parametrisations (tests/test_gpu_ops.py), tolerances the ones used there."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import usot_oracle as orc  # noqa: E402
from conftest import tile_params  # noqa: E402
from test_gpu_ops import BF16_CASES, CONV_CASES, ROIS, _prroi_tol, pack_w, rel_err  # noqa: E402
from usot_amd import autograd, hip  # noqa: E402

DEV = 'cuda:0'
GEO = ((5, 5), (3, 5), (5, 3))
LP = [pytest.param(torch.bfloat16, id='bf16'), pytest.param(torch.float16, id='fp16')]


class Contract(object):
    def __init__(self):
        self.inputs = []

    def put(self, t):
        """guarded device copy of a CPU (or device) tensor, remembered bit for bit"""
        g = guarded.put(t, DEV)
        self.inputs.append((g, guarded.snapshot(g)))
        return g

    def puts(self, *ts):
        return [self.put(t) if t is not None else None for t in ts]

    @staticmethod
    def out(shape, dtype=torch.float32, prefill='canary'):
        return guarded.alloc(shape, dtype, DEV, prefill)


@contextlib.contextmanager
def contract():
    """Inside: wrappers of usot_amd.hip allocate through the guard.  On exit: inputs bit-unchanged, every guard intact."""
    c = Contract()
    with guarded.patched(hip, autograd):
        yield c
        torch.cuda.synchronize()
        for k, (g, snap) in enumerate(c.inputs):
            guarded.unchanged(g, snap, 'input %d' % k)


def no_nan(*ts):
    for t in ts:
        assert not bool(torch.isnan(t).any()), 'NaN in an output of shape %s' % (tuple(t.shape),)


def lp_err(got, ref):
    """the low-precision parity tests' metric: |got - ref| / max(|ref|, 1)"""
    return float(((got.float().cpu().double() - ref).abs() / ref.abs().clamp_min(1.0)).max())


def ulp_of(dtype, out=True):
    return 2.0 ** (-8 if dtype == torch.bfloat16 else -11)


def dt_of(dtype):
    return 1 if dtype == torch.float16 else 0


def same_up_to_ties(got, ref32):
    """the bar of test_groupdw_and_conf_reduce_low_precision_outputs: the fp32 launch's value stored once in the low-precision type"""
    want = ref32.to(got.dtype)
    ne = got != want
    ulp = 2.0 ** (-10 if got.dtype == torch.float16 else -7)
    err = ((got.float() - ref32).abs() / ref32.abs().clamp_min(1e-3)).max()
    return int(ne.sum()) <= 1e-3 * got.numel() and float(err) <= 0.51 * ulp * 1.01


# ------------------------------------------------------------------------------------------------------ fp32 convolution
MC_CONV = [CONV_CASES[0], CONV_CASES[1], CONV_CASES[2], CONV_CASES[9], CONV_CASES[8]]
assert [(c[1], c[4], c[5]) for c in MC_CONV] == [(64, 64, 1), (64, 96, 3), (128, 128, 3), (256, 1, 3), (256, 4, 3)]


def _conv_tile_cases():
    from usot_amd import build
    if not os.path.exists(build.LIB):
        return [pytest.param(c, 0) for c in MC_CONV]
    n = hip.lib().usot_conv_tile_count()
    out = []
    for c in MC_CONV:
        for p in tile_params(range(0, n + 1)):
            tile = p.values[0]
            if hip.tile_supports(tile, c[1], c[4], c[5] * c[5] * c[1]):
                out.append(pytest.param(c, tile, marks=p.marks))
    return out


def _conv_inputs(case, seed):
    N, Cin, H, W, Cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad, dil)
    return x, w, b, ref


@pytest.mark.parametrize('case,tile', _conv_tile_cases())
def test_conv_f32(case, tile):
    N, Cin, H, W, Cout, k, stride, pad, dil = case
    x, w, b, ref = _conv_inputs(case, 1000 + Cin + Cout + k)
    res = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3))
    with contract() as c:
        xd, wd, bd, rd = c.puts(x.permute(0, 2, 3, 1).contiguous(), pack_w(w), b, res.permute(0, 2, 3, 1).contiguous())
        y = hip.conv2d(xd, wd, bd, KH=k, KW=k, stride=stride, pad=pad, dil=dil, res=rd, act=hip.ACT_RELU, tile=tile)
        yn = hip.conv2d(xd, wd, bd, KH=k, KW=k, stride=stride, pad=pad, dil=dil, tile=tile, y_nchw=True) if Cout in (96, 1, 4) else None
    no_nan(y)
    assert rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), F.relu(ref + res.double()).numpy()) < 2e-5
    if yn is not None:
        no_nan(yn)
        assert rel_err(yn.cpu().numpy(), ref.numpy()) < 2e-5


@pytest.mark.parametrize('ksplit', [3, 9])
def test_conv_f32_splitk(ksplit):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 256, 25, 25, generator=g)
    w = torch.randn(256, 256, 3, 3, generator=g) / 48
    b = torch.randn(256, generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1))
    with contract() as c:
        xd, wd, bd = c.puts(x.permute(0, 2, 3, 1).contiguous(), pack_w(w), b)
        y = hip.conv2d(xd, wd, bd, KH=3, KW=3, pad=(1, 1), act=hip.ACT_RELU, ksplit=ksplit, tile=4)
    no_nan(y)
    assert rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < 2e-5


@pytest.mark.parametrize('tile', [91, 99, 106, 97, 94, 111])
@pytest.mark.parametrize('ks', [1, 3])
def test_conv_f32_split_fp16_tiles_in_range(tile, ks):
    """the shape and the in-range data of test_split_fp16_tiles_range_contract: per output channel, against that channel's scale"""
    g = torch.Generator().manual_seed(17 + tile)
    N, Cin, H, W, Cout, k = 1, 128, 13, 11, 128, 3
    x = torch.randn(N, Cin, H, W, generator=g)
    x[:, ::5] *= 1e-6
    x[:, 3::7] *= 5e3 / 4.5
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    w[5] *= 1e-12
    w[6] *= 1e3
    w[7] = 0.0
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1).float()
    with contract() as c:
        xd, wd, bd = c.puts(x.permute(0, 2, 3, 1).contiguous(), pack_w(w), b)
        ovf = c.out((1,), torch.int32, 'zero')
        y = hip.conv2d(xd, wd, bd, KH=k, KW=k, pad=(1, 1), tile=tile, ksplit=ks, ovf=ovf)
    y = y.permute(0, 3, 1, 2).cpu()
    assert torch.isfinite(y).all() and int(ovf.item()) == 0
    err = (y - ref).abs().amax((0, 2, 3)) / (ref.abs().amax((0, 2, 3)) + 1e-30)
    err[7] = (y[:, 7] - ref[:, 7]).abs().max()
    assert err.max() < 2e-5, (err.max(), int(err.argmax()))


@pytest.mark.parametrize('n,hw', [(1, 7), (2, 27)])
def test_thin_conv3x3(n, hw):
    g = torch.Generator().manual_seed(n * 100 + hw)
    x = torch.randn(3, n, 256, hw, hw, generator=g)
    wb = torch.randn(4, 256, 3, 3, generator=g) / 48
    bb = torch.randn(4, generator=g) * 0.1
    wc = torch.randn(2, 256, 3, 3, generator=g) / 48
    bc = torch.randn(2, generator=g)
    with contract() as c:
        xd, wbd, wcd, bbd, bcd = c.puts(x.permute(0, 1, 3, 4, 2).contiguous(), pack_w(wb), pack_w(wc), bb, bc)
        yb, yc = c.out((n, 4, hw, hw)), c.out((2, n, 1, hw, hw))
        gs = n * hw * hw * 256
        descs = [hip.conv_desc(xd[0].data_ptr(), wbd.data_ptr(), bbd.data_ptr(), yb.data_ptr(), N=n, H=hw, W=hw, Cin=256, OH=hw, OW=hw,
                               Cout=4, KH=3, KW=3, pad=(1, 1), act=hip.ACT_EXP, y_nchw=1),
                 hip.conv_desc(xd[1].data_ptr(), wcd.data_ptr(), bcd.data_ptr(), yc.data_ptr(), N=n, H=hw, W=hw, Cin=256, OH=hw, OW=hw,
                               Cout=1, KH=3, KW=3, pad=(1, 1), y_nchw=1, groups=2, x_gs=gs, w_gs=2304, b_gs=1, y_gs=n * hw * hw)]
        hip.check(hip.lib().usot_thin_conv3x3_f32(hip.stream(), (hip.ConvDesc * 2)(*descs), 2), 'thin')
    no_nan(yb, yc)
    assert rel_err(yb.cpu().numpy(), torch.exp(F.conv2d(x[0].double(), wb.double(), bb.double(), 1, 1)).numpy()) < 1e-5
    for gi in range(2):
        ref = F.conv2d(x[1 + gi].double(), wc[gi:gi + 1].double(), bc[gi:gi + 1].double(), 1, 1)
        assert rel_err(yc[gi].cpu().numpy(), ref.numpy()) < 1e-5


# ------------------------------------------------------------------------------------------------------ stem, max-pool
STEM = [(63, 3), (64, 1)]


@pytest.mark.parametrize('size,n', STEM)
def test_stem_conv_and_maxpool(size, n):
    g = torch.Generator().manual_seed(size)
    x = torch.rand(n, 3, size, size, generator=g) * 255
    w = torch.randn(64, 3, 7, 7, generator=g) / 12
    b = torch.randn(64, generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), 2, 0))
    with contract() as c:
        xd, wd, bd = c.puts(x, w.permute(1, 2, 3, 0).reshape(147, 64).contiguous(), b)
        y = hip.stem_conv(xd, wd, bd)
        torch.cuda.synchronize()
        ysnap = guarded.snapshot(y)
        p = hip.maxpool3x3s2(y)
        torch.cuda.synchronize()
        guarded.unchanged(y, ysnap, 'max-pool input')
    no_nan(y, p)
    assert rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < 1e-5
    assert torch.equal(p.permute(0, 3, 1, 2).cpu(), F.max_pool2d(y.permute(0, 3, 1, 2).cpu(), 3, 2, 1))         # max-pool is exact


@pytest.mark.parametrize('size,n', STEM)
def test_stem_pool_f32(size, n):
    from usot_amd.engine import pack_stem_f32
    g = torch.Generator().manual_seed(size * 3 + n)
    x = torch.rand(n, 3, size, size, generator=g) * 255
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.02
    w = w - w.mean((1, 2, 3), keepdim=True)
    b = torch.randn(64, generator=g) * 0.1
    packed = w.permute(1, 2, 3, 0).reshape(147, 64).contiguous()
    ref = F.max_pool2d(F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2)).float(), 3, 2, 1).permute(0, 2, 3, 1)
    with contract() as c:
        xd, wd, bd = c.puts(x, pack_stem_f32(packed), b)
        got = hip.stem_pool(xd, wd, bd)
    no_nan(got)
    assert got.shape == ref.shape and rel_err(got.cpu().numpy(), ref.numpy()) < 2e-5


@pytest.mark.parametrize('dtype,wdtype', [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.bfloat16, torch.float16)],
                         ids=['bf16', 'fp16', 'bf16_out_fp16_math'])
@pytest.mark.parametrize('size,n', STEM)
def test_stem_pool_lp(size, n, dtype, wdtype):
    from usot_amd.engine import pack_stem_lp
    g = torch.Generator().manual_seed(size + n)
    x = (torch.rand(n, 3, size, size, generator=g) * 2 - 1) * 3
    mu = (0.25, -0.5, 1.0)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    packed = w.permute(1, 2, 3, 0).reshape(147, 64).contiguous()
    with contract() as c:
        xd, wd, bd = c.puts(x, pack_stem_lp(packed, wdtype), b)
        got = hip.stem_pool_lp(xd, wd, bd, dtype, mu)
    no_nan(got)
    got = got.float().cpu()
    xc = x - torch.tensor(mu).view(1, 3, 1, 1)
    xr, wr = xc.to(wdtype).double(), w.to(wdtype).double()
    if wdtype == torch.bfloat16:
        xr = xr + (xc - xc.to(wdtype).float()).to(wdtype).double()
    ref = torch.relu(F.conv2d(xr, wr, b.double(), stride=2)).float().to(dtype).float()
    ref = F.max_pool2d(ref, 3, 2, 1).permute(0, 2, 3, 1)
    assert got.shape == ref.shape
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    err = (got - ref).abs() / ref.abs().clamp_min(1.0)
    assert float(err.max()) <= 1.01 * ulp, float(err.max())


@pytest.mark.parametrize('dtype', LP)
def test_cvt_and_maxpool_lp(dtype):
    """usot_cvt_f32_to_lp on an odd number of 8-element groups (the entry point takes whole groups only) and usot_maxpool3x3s2_lp
    on an odd map: the conversion is torch's round-to-nearest-even, the max-pool exact."""
    g = torch.Generator().manual_seed(9)
    src = torch.randn(8 * 37, generator=g) * 100
    x = torch.randn(2, 7, 9, 64, generator=g).to(dtype)
    L = hip.lib()
    with contract() as c:
        sd, xd = c.puts(src, x)
        dst = c.out((8 * 37,), dtype)
        hip.check(L.usot_cvt_f32_to_lp(hip.stream(), hip.ptr(sd), hip.ptr(dst), C.c_int64(8 * 37), dt_of(dtype)), 'cvt')
        y = c.out((2, 4, 5, 64), dtype)
        hip.check(L.usot_maxpool3x3s2_lp(hip.stream(), hip.ptr(xd), hip.ptr(y), 2, 7, 9, 64, 4, 5, dt_of(dtype)), 'maxpool_lp')
    no_nan(dst, y)
    assert torch.equal(dst.cpu(), src.to(dtype))
    assert torch.equal(y.float().cpu(), F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------ small-M fp32 kernels
def _pair_inputs(cm, co, cn, M, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    t2 = torch.randn(M, cm, generator=g)
    if positive:
        t2 = t2.abs()
    w3 = torch.randn(co, cm, generator=g) / np.sqrt(cm)
    b3 = torch.randn(co, generator=g)
    res = torch.randn(M, co, generator=g)
    w1 = torch.randn(cn, co, generator=g) / np.sqrt(co)
    b1 = torch.randn(cn, generator=g)
    y64 = F.relu(t2.double() @ w3.double().t() + b3.double() + res.double())
    t64 = F.relu(y64 @ w1.double().t() + b1.double())
    return (t2.reshape(1, 1, M, cm), w3, b3, res.reshape(1, 1, M, co), w1, b1), y64, t64


@pytest.mark.parametrize('split16', [False, True], ids=['f32', 'f32s'])
def test_pw_pair_f32(split16):
    cm, co, cn, M = 256, 1024, 256, 37
    args, y64, t64 = _pair_inputs(cm, co, cn, M, cm + cn + M, positive=split16)
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        y, t = hip.pw_pair_f32(*c.puts(*args), split16=split16, ovf=ovf if split16 else None)
    no_nan(y, t)
    e_y, e_t = rel_err(y.reshape(M, co).cpu().numpy(), y64.numpy()), rel_err(t.reshape(M, cn).cpu().numpy(), t64.numpy())
    assert e_y < 1e-5 and e_t < 1e-5 and int(ovf.item()) == 0, (e_y, e_t)


@pytest.mark.parametrize('res', [True, False])
def test_pw_single_f32(res):
    K, N, M = 256, 1024, 5
    g = torch.Generator().manual_seed(K + N + M)
    x = torch.randn(1, 1, M, K, generator=g)
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(1, 1, M, N, generator=g) if res else None
    ref = F.relu(x.double().reshape(M, K) @ w.double().t() + b.double() + (r.double().reshape(M, N) if res else 0)).numpy()
    with contract() as c:
        y = hip.pw_single_f32(*c.puts(x, w, b, r), hip.ACT_RELU)
    no_nan(y)
    assert rel_err(y.reshape(M, N).cpu().numpy(), ref) < 1e-5


def test_stream_conv3x3_f32():
    cin, n, nb, h, w_, pad, dil = 256, 256, 1, 15, 15, 1, 1
    g = torch.Generator().manual_seed(cin + h * w_ + pad)
    x = torch.randn(nb, cin, h, w_, generator=g)
    w4 = torch.randn(n, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b = torch.randn(n, generator=g)
    ref = F.relu(F.conv2d(x.double(), w4.double(), b.double(), 1, pad, dil)).numpy()
    with contract() as c:
        xd, wd, bd = c.puts(x.permute(0, 2, 3, 1).contiguous(), pack_w(w4), b)
        y = hip.stream_conv3x3_f32(xd, wd, bd, (pad, pad), (dil, dil), None, hip.ACT_RELU)
    no_nan(y)
    assert rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), ref) < 1e-5


def test_pw_triple_f32():
    cin, cn, nb, h, w_ = 64, 64, 2, 9, 7
    cm, co = cin, 4 * cin
    g = torch.Generator().manual_seed(cn + h)
    x = torch.randn(nb, cin, h, w_, generator=g)
    w2 = torch.randn(cm, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b2 = torch.randn(cm, generator=g)
    w3 = torch.randn(co, cm, generator=g) / np.sqrt(cm)
    b3 = torch.randn(co, generator=g)
    res = torch.randn(nb, h, w_, co, generator=g)
    w1 = torch.randn(cn, co, generator=g) / np.sqrt(co)
    b1 = torch.randn(cn, generator=g)
    t2 = F.relu(F.conv2d(x.double(), w2.double(), b2.double(), 1, 1, 1)).permute(0, 2, 3, 1)
    y64 = F.relu(t2 @ w3.double().t() + b3.double() + res.double())
    t64 = F.relu(y64 @ w1.double().t() + b1.double())
    with contract() as c:
        y, t = hip.pw_triple_f32(*c.puts(x.permute(0, 2, 3, 1).contiguous(), pack_w(w2), b2, w3, b3, res, w1, b1))
    no_nan(y, t)
    e_y, e_t = rel_err(y.cpu().numpy(), y64.numpy()), rel_err(t.cpu().numpy(), t64.numpy())
    assert e_y < 1e-5 and e_t < 1e-5, (e_y, e_t)


# ------------------------------------------------------------------------------------------------------ low precision
@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('tile', tile_params([0, 4, 13, 21], lp=True))
def test_conv2d_lp(tile, dtype):
    N, Cin, H, W, Cout, k, stride, pad, dil = BF16_CASES[0]
    g = torch.Generator().manual_seed(77 + tile)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)).to(dtype)
    b = torch.randn(Cout, generator=g)
    res = torch.randn(N, Cout, H, W, generator=g).to(dtype)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride, pad, dil) + res.double())
    with contract() as c:
        xd, wd, bd, rd = c.puts(x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous(), b,
                                res.permute(0, 2, 3, 1).contiguous())
        y = hip.conv2d_bf16(xd, wd, bd, KH=k, KW=k, stride=stride, pad=pad, dil=dil, res=rd, act=hip.ACT_RELU, tile=tile)
        y32 = hip.conv2d_bf16(xd, wd, bd, KH=k, KW=k, stride=stride, pad=pad, dil=dil, res=rd, act=hip.ACT_RELU, tile=tile, out_f32=True)
    no_nan(y, y32)
    assert rel_err(y.float().permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < (6e-3 if dtype == torch.bfloat16 else 1e-3)
    assert rel_err(y32.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < 2e-5


@pytest.mark.parametrize('dtype', LP)
def test_pw_pair_lp(dtype):
    cm, co, cn, M = 256, 1024, 256, 50
    g = torch.Generator().manual_seed(cm + co + cn + M)
    t2 = torch.randn(M, cm, generator=g).relu().to(dtype)
    res = torch.randn(M, co, generator=g).relu().to(dtype)
    w3 = (torch.randn(co, cm, generator=g) / np.sqrt(cm)).to(dtype)
    w1 = (torch.randn(cn, co, generator=g) / np.sqrt(co)).to(dtype)
    b3, b1 = torch.randn(co, generator=g), torch.randn(cn, generator=g)
    with contract() as c:
        y, t = hip.pw_pair(*c.puts(t2, w3, b3, res, w1, b1))
    no_nan(y, t)
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    yt = torch.relu(t2.double() @ w3.double().t() + b3.double() + res.double())
    assert rel_err(y.float().cpu().numpy(), yt.numpy()) < 4 * ulp
    tt = torch.relu(y.cpu().double() @ w1.double().t() + b1.double())
    assert rel_err(t.float().cpu().numpy(), tt.numpy()) < 4 * ulp


@pytest.mark.parametrize('dtype', LP)
def test_pw_panel_lp(dtype):
    K, N, M = 256, 1024, 77
    g = torch.Generator().manual_seed(K + N + M)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(N, generator=g) * 0.1
    ref = x.double() @ w.double().t() + b.double()
    with contract() as c:
        xd, wd, bd = c.puts(x, w, b)
        y = c.out((M, N), dtype)
        hip.check(hip.lib().usot_pw_panel_lp(hip.stream(), hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), None, hip.ptr(y), M, K, N, 0, dt_of(dtype)),
                  'usot_pw_panel_lp')
    no_nan(y)
    assert lp_err(y, ref) <= ulp_of(dtype) * 1.01


@pytest.mark.parametrize('dtype', LP)
def test_pw_panel_pair_lp(dtype):
    cm, co, cn, M, act2 = 128, 512, 128, 61, 0
    g = torch.Generator().manual_seed(cm + co + cn + M)
    t2 = torch.randn(M, cm, generator=g).to(dtype)
    w3 = (torch.randn(co, cm, generator=g) / cm ** 0.5).to(dtype)
    w1 = (torch.randn(cn, co, generator=g) / co ** 0.5).to(dtype)
    b3, b1 = torch.randn(co, generator=g) * 0.1, torch.randn(cn, generator=g) * 0.1
    res = torch.randn(M, co, generator=g).to(dtype)
    with contract() as c:
        t2d, w3d, w1d, b3d, b1d, resd = c.puts(t2, w3, w1, b3, b1, res)
        y, t = c.out((M, co), dtype), c.out((M, cn), dtype)
        d = hip.pw_pair_desc(t2d.data_ptr(), w3d.data_ptr(), b3d.data_ptr(), resd.data_ptr(), y.data_ptr(), w1d.data_ptr(), b1d.data_ptr(),
                             t.data_ptr(), M, cm, co, cn, act2)
        hip.check(hip.lib().usot_pw_panel_pair_lp(hip.stream(), C.byref(d), dt_of(dtype)), 'usot_pw_panel_pair_lp')
    no_nan(y, t)
    yref = (t2.double() @ w3.double().t() + b3.double() + res.double()).relu()
    assert lp_err(y, yref) <= ulp_of(dtype) * 1.01                   # one rounding of the output (the panel kernel's own bar)
    tref = y.cpu().double() @ w1.double().t() + b1.double()
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    assert lp_err(t, tref) <= ulp


def _conv_pw_inputs(n, h, pad, dil, cm, dtype, seed, cn=0):
    g = torch.Generator().manual_seed(seed)
    co = 4 * cm
    M = n * h * h
    t1 = torch.randn(n, h, h, cm, generator=g).relu().to(dtype)
    w2 = (torch.randn(cm, 9 * cm, generator=g) / (9 * cm) ** 0.5).to(dtype)       # [Cout][kh][kw][Cin]
    w3 = (torch.randn(co, cm, generator=g) / cm ** 0.5).to(dtype)
    b2, b3 = torch.randn(cm, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1
    res = torch.randn(M, co, generator=g).to(dtype)
    w1 = (torch.randn(cn, co, generator=g) / co ** 0.5).to(dtype) if cn else None
    b1 = torch.randn(cn, generator=g) * 0.1 if cn else None
    x64 = t1.double().permute(0, 3, 1, 2)
    w64 = w2.double().view(cm, 3, 3, cm).permute(0, 3, 1, 2)
    t2r = F.conv2d(x64, w64, b2.double(), padding=pad, dilation=dil).relu().permute(0, 2, 3, 1).reshape(M, cm)
    ref = (t2r.to(dtype).double() @ w3.double().t() + b3.double() + res.double()).relu()
    return (t1, w2, b2, w3, b3, res, w1, b1), ref, M, co


@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('rs', [False, True], ids=['pertap', 'rowshared'])
@pytest.mark.parametrize('h,cm', [(13, 256), (12, 128)], ids=['h13_c256', 'h12_c128'])
@pytest.mark.parametrize('form', [1, 2], ids=['panel256', 'panel128'])
def test_conv_pw_lp(form, h, cm, rs, dtype):
    """conv2 -> conv3 in one launch at n = 1: layer3's widths at h = 13 and layer2's at h = 12 (the two instantiations of the
    four-phase kernel; one ragged panel each, waves without any pixel)"""
    n, pad, dil = 1, 1, 1
    ins, ref, M, co = _conv_pw_inputs(n, h, pad, dil, cm, dtype, n * 1000 + h * 10 + pad)
    with contract() as c:
        t1d, w2d, b2d, w3d, b3d, resd = c.puts(*ins[:6])
        y = c.out((M, co), dtype)
        d = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                          pad=(pad, pad), dil=(dil, dil), act=1, tile=form | (0 if rs else 4))
        hip.check(hip.lib().usot_conv_pw_lp(hip.stream(), C.byref(d), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(resd), hip.ptr(y), dt_of(dtype)),
                  'usot_conv_pw_lp')
    no_nan(y)
    assert lp_err(y, ref) <= 4 * ulp_of(dtype)


@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('rs', [False, True], ids=['pertap', 'rowshared'])
@pytest.mark.parametrize('h,cm,act2', [(13, 256, 0), (12, 128, 1)], ids=['h13_c256', 'h12_c128'])
@pytest.mark.parametrize('form', [1, 2], ids=['panel256', 'panel128'])
def test_conv_pw_pair_lp(form, h, cm, act2, rs, dtype):
    """the next conv1 as the fifth phase at n = 1: layer3's block into the neck (no ReLU) at h = 13, layer2's last block into
    layer3's first conv1 at h = 12 (the two instantiations of the five-phase kernel)"""
    n, pad, cn = 1, 1, 256
    ins, ref, M, co = _conv_pw_inputs(n, h, pad, pad, cm, dtype, n * 100 + h + act2 + cm, cn=cn)
    with contract() as c:
        t1d, w2d, b2d, w3d, b3d, resd, w1d, b1d = c.puts(*ins)
        y, t = c.out((M, co), dtype), c.out((M, cn), dtype)
        d = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                          pad=(pad, pad), dil=(pad, pad), act=1, tile=form | (0 if rs else 4))
        pd = hip.pw_pair_desc(None, w3d.data_ptr(), b3d.data_ptr(), resd.data_ptr(), y.data_ptr(), w1d.data_ptr(), b1d.data_ptr(),
                              t.data_ptr(), M, cm, co, cn, act2)
        hip.check(hip.lib().usot_conv_pw_pair_lp(hip.stream(), C.byref(d), C.byref(pd), dt_of(dtype)), 'usot_conv_pw_pair_lp')
    no_nan(y, t)
    assert lp_err(y, ref) <= 4 * ulp_of(dtype)
    tref = y.cpu().double() @ ins[6].double().t() + ins[7].double()
    assert lp_err(t, tref.relu() if act2 else tref) <= ulp_of(dtype) * 1.01


@pytest.mark.parametrize('dtype', LP)
def test_conv_kstream_lp(dtype):
    """The (1, 7, 9) row of test_conv_kstream's list, with its bias: M = 63, the smallest ragged row this entry point is tested
    at (its parity test has no M = 300 row and no bias-free form; those belong to usot_pw_kstream_lp, below)."""
    N, H, W, Cin, Cout, stride, pad, dil, act = 1, 7, 9, 256, 256, 1, 1, 1, 1
    g = torch.Generator().manual_seed(N + H * 7 + Cin + Cout + stride + dil)
    x = torch.randn(N, H, W, Cin, generator=g).to(dtype)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (3 * Cin ** 0.5)).to(dtype)
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(), stride=stride, padding=pad,
                   dilation=dil).permute(0, 2, 3, 1).relu()
    with contract() as c:
        xd, wd, bd = c.puts(x, w.reshape(Cout, 9 * Cin).contiguous(), b)
        y = c.out((N, H, W, Cout), dtype)
        hip.check(hip.lib().usot_conv_kstream_lp(hip.stream(), hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(y), N, H, W, Cin, Cout, stride,
                                                 pad, dil, act, dt_of(dtype)), 'conv_kstream')
    no_nan(y)
    assert lp_err(y, ref) <= ulp_of(dtype) * 1.01


@pytest.mark.parametrize('dtype', LP)
def test_pw_kstream_lp(dtype):
    M, K, N = 300, 1024, 256
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / 32).to(dtype)
    ref = x.double() @ w.double().t()
    with contract() as c:
        xd, wd = c.puts(x, w)
        y = c.out((M, N), dtype)
        hip.check(hip.lib().usot_pw_kstream_lp(hip.stream(), hip.ptr(xd), hip.ptr(wd), None, hip.ptr(y), M, K, N, 0, dt_of(dtype)),
                  'usot_pw_kstream_lp')
    no_nan(y)
    assert lp_err(y, ref) <= 1.5 * ulp_of(dtype)


@pytest.mark.parametrize('dtype', LP)
def test_conv3x3_halo_lp(dtype):
    N, H, W, act = 1, 5, 40, 1
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    x = torch.randn(N, H, W, 64, generator=g).to(dtype)
    w = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dtype)
    b = torch.randn(64, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(), padding=1).permute(0, 2, 3, 1).relu()
    with contract() as c:
        xd, wd, bd = c.puts(x, w.reshape(64, 576).contiguous(), b)
        y = c.out((N, H, W, 64), dtype)
        hip.check(hip.lib().usot_conv3x3_halo_lp(hip.stream(), hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(y), N, H, W, 64, 64, act,
                                                 dt_of(dtype)), 'halo')
    no_nan(y)
    assert lp_err(y, ref) <= ulp_of(dtype) * 1.01


BNECK = [(1, 5, 130), (9, 8, 16)]


@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('N,H,W', BNECK)
def test_bneck_first_lp(N, H, W, dtype):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(N, H, W, 64).relu().to(dtype)
    w1 = (rnd(64, 64) / 8).to(dtype); b1 = rnd(64) * 0.1
    w2 = (rnd(64, 3, 3, 64) / 24).to(dtype); b2 = rnd(64) * 0.1
    w3 = (rnd(256, 64) / 8).to(dtype); wd = (rnd(256, 64) / 8).to(dtype); b3c = rnd(256) * 0.1
    wn = (rnd(64, 256) / 16).to(dtype); bn = rnd(64) * 0.1
    rq = lambda v: v.to(dtype).double()
    xd_ = x.double()
    t1 = rq((xd_ @ w1.double().t() + b1.double()).relu())
    t2 = rq(F.conv2d(t1.permute(0, 3, 1, 2), w2.double().permute(0, 3, 1, 2), b2.double(), padding=1).permute(0, 2, 3, 1).relu())
    y_ref = (t2 @ w3.double().t() + xd_ @ wd.double().t() + b3c.double()).relu()
    t_ref = (rq(y_ref) @ wn.double().t() + bn.double()).relu()
    with contract() as c:
        ins = c.puts(x, w1, b1, w2.reshape(64, 576).contiguous(), b2, torch.cat([w3, wd], 1).contiguous(), b3c, wn, bn)
        y, t = c.out((N, H, W, 256), dtype), c.out((N, H, W, 64), dtype)
        d = hip.bneck_desc(*[hip.ptr(v) for v in ins + [y, t]], N, H, W)
        hip.check(hip.lib().usot_bneck_first_lp(hip.stream(), C.byref(d), dt_of(dtype)), 'bneck_first')
    no_nan(y, t)
    ey, et = lp_err(y, y_ref), lp_err(t, t_ref)
    assert ey <= 3 * ulp_of(dtype) and et <= 4 * ulp_of(dtype), (ey, et)


@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('N,H,W', BNECK)
def test_bneck_tail_lp(N, H, W, dtype):
    cn = 64
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W + cn)
    rnd = lambda *s: torch.randn(*s, generator=g)
    t1 = rnd(N, H, W, 64).relu().to(dtype)
    res = rnd(N, H, W, 256).relu().to(dtype)
    w2 = (rnd(64, 3, 3, 64) / 24).to(dtype); b2 = rnd(64) * 0.1
    w3 = (rnd(256, 64) / 8).to(dtype); b3 = rnd(256) * 0.1
    wn = (rnd(cn, 256) / 16).to(dtype); bn = rnd(cn) * 0.1
    rq = lambda v: v.to(dtype).double()
    t2 = rq(F.conv2d(t1.double().permute(0, 3, 1, 2), w2.double().permute(0, 3, 1, 2), b2.double(), padding=1).permute(0, 2, 3, 1).relu())
    y_ref = (t2 @ w3.double().t() + b3.double() + res.double()).relu()
    t_ref = (rq(y_ref) @ wn.double().t() + bn.double()).relu()
    with contract() as c:
        t1d, resd, w2d, b2d, w3d, b3d, wnd, bnd = c.puts(t1, res, w2.reshape(64, 576).contiguous(), b2, w3, b3, wn, bn)
        y, t = c.out((N, H, W, 256), dtype), c.out((N, H, W, cn), dtype)
        d = hip.bneck_desc(hip.ptr(t1d), hip.ptr(resd), None, hip.ptr(w2d), hip.ptr(b2d), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(wnd), hip.ptr(bnd),
                           hip.ptr(y), hip.ptr(t), N, H, W)
        hip.check(hip.lib().usot_bneck_tail_lp(hip.stream(), C.byref(d), cn, dt_of(dtype)), 'bneck_tail')
    no_nan(y, t)
    ey, et = lp_err(y, y_ref), lp_err(t, t_ref)
    assert ey <= 3 * ulp_of(dtype) and et <= 4 * ulp_of(dtype), (ey, et)


# ------------------------------------------------------------------------------------------------------ cross-correlation
XC_MC = [(29, 29, 5, 5), (27, 29, 3, 5), (29, 27, 5, 3), (12, 9, 4, 2),
         # dispatch edges: Wx 32 | 33, Wx 64 | 65, OH = 1, OW = 1, a single output
         (9, 32, 5, 5), (9, 33, 5, 5), (9, 64, 5, 3), (9, 65, 5, 3), (5, 29, 5, 5), (29, 5, 5, 5), (3, 5, 3, 5)]


def _xc_inputs(shape, planes, seed=0):
    hx, wx, hk, wk = shape
    b, c = planes
    g = torch.Generator().manual_seed(hx * 100 + wk + 7 * b + seed)
    return (torch.randn(b, c, hx, wx, generator=g), torch.randn(b, c, hk, wk, generator=g),
            torch.randn(b, c, hx - hk + 1, wx - wk + 1, generator=g))


@pytest.mark.parametrize('planes', [(1, 1), (3, 257)])        # 771 planes: the last wavefront's second half has no plane
@pytest.mark.parametrize('shape', XC_MC)
def test_xcorr_forward_and_gradients(shape, planes):
    x, k, dout = _xc_inputs(shape, planes)
    x64, k64 = x.double().requires_grad_(True), k.double().requires_grad_(True)
    ref = orc.xcorr_depthwise(x64, k64)
    rx, rk = torch.autograd.grad(ref, (x64, k64), dout.double())
    with contract() as c:
        xd, kd, dd = c.puts(x, k, dout)
        out = hip.xcorr_depthwise(xd, kd)
        dx = hip.xcorr_depthwise_backward_x(dd, kd, x.shape)
        dk = hip.xcorr_depthwise_backward_k(dd, xd, k.shape)
    no_nan(out, dx, dk)
    assert rel_err(out.cpu().numpy(), ref.detach().numpy()) < 1e-5
    assert rel_err(dx.cpu().numpy(), rx.numpy()) < 1e-5 and rel_err(dk.cpu().numpy(), rk.numpy()) < 1e-5


@pytest.mark.parametrize('kernel', ['forward', 'bwd_x', 'bwd_k'])
def test_xcorr_plane_isolation(kernel):
    """One whole input plane set to NaN: every other plane's result is bit-identical to the run without it (the masks of the
    two-planes-per-wavefront units; 771 planes, Wx = 29).  Planes tried: an even one, its odd partner, and the last plane, whose
    wavefront has no second plane."""
    x, k, dout = _xc_inputs((29, 29, 5, 5), (3, 257), seed=8)
    run = {'forward': lambda x_, k_, d_: hip.xcorr_depthwise(x_, k_),
           'bwd_x': lambda x_, k_, d_: hip.xcorr_depthwise_backward_x(d_, k_, x.shape),
           'bwd_k': lambda x_, k_, d_: hip.xcorr_depthwise_backward_k(d_, x_, k.shape)}[kernel]
    used = {'forward': (0, 1), 'bwd_x': (1, 2), 'bwd_k': (0, 2)}[kernel]
    with contract() as c:
        base = run(*c.puts(x, k, dout))
        no_nan(base)
        for which in used:
            for plane in (384, 385, 770):
                ins = [x.clone(), k.clone(), dout.clone()]
                ins[which].view(771, -1)[plane] = float('nan')
                got = run(*c.puts(*ins)).view(771, -1)
                assert bool(torch.isnan(got[plane]).all()), (which, plane)
                keep = torch.arange(771, device=DEV) != plane
                assert torch.equal(got[keep], base.view(771, -1)[keep]), (which, plane)


# ------------------------------------------------------------------------------------------------------ GroupDW, Conf_Fusion
def _groupdw_case(S, x_rep, OW, seed):
    g = torch.Generator().manual_seed(seed)
    XS = S // x_rep
    xs = [torch.randn(XS, 256, OW + hk - 1, OW + wk - 1, generator=g) for hk, wk in GEO]
    zs = [torch.randn(S, 256, hk, wk, generator=g) for hk, wk in GEO]
    wsm = torch.softmax(torch.randn(3, generator=g), 0)
    ref = 0
    for i in range(3):
        ref = ref + wsm[i].double() * orc.xcorr_depthwise(xs[i].double().repeat_interleave(x_rep, 0), zs[i].double())
    return xs, zs, wsm, ref


@pytest.mark.parametrize('S,x_rep,OW,cols', [(5, 1, ow, cols) for ow in (25, 27) for cols in (0, 1, 6, 8)] + [(14, 7, 27, 0), (14, 7, 27, 9)])
def test_groupdw_f32(S, x_rep, OW, cols):
    xs, zs, wsm, ref = _groupdw_case(S, x_rep, OW, S * 31 + OW)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with contract() as c:
        out = hip.groupdw(c.puts(*[nh(t) for t in xs]), c.puts(*[nh(t) for t in zs]), wsm.numpy(), x_rep=x_rep, cols=cols)
    no_nan(out)
    assert rel_err(out.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < 1e-5


@pytest.mark.parametrize('dtype', [pytest.param(torch.float32, id='f32')] + LP)
def test_groupdw_multi_three_segments(dtype):
    """the three-segment layout of test_groupdw_three_segments_one_launch with b = 1 (reg, cls on the merged maps' channel halves,
    memory with x_rep = 7), fp32 and with the output maps in fp16 | bf16"""
    g = torch.Generator().manual_seed(400)
    b, m, OW = 1, 7, 25
    es = [torch.randn(b, OW + hk - 1, OW + wk - 1, 512, generator=g) for hk, wk in GEO]
    zk = [torch.randn(b, hk, wk, 512, generator=g) for hk, wk in GEO]
    mk = [torch.randn(b * m, hk, wk, 256, generator=g) for hk, wk in GEO]
    w_reg, w_cls = torch.softmax(torch.randn(3, generator=g), 0).numpy(), torch.softmax(torch.randn(3, generator=g), 0).numpy()
    with contract() as c:
        esd, zkd, mkd = c.puts(*es), c.puts(*zk), c.puts(*mk)
        outs = [c.out((b, OW, OW, 256), dtype), c.out((b, OW, OW, 256), dtype), c.out((b * m, OW, OW, 256), dtype)]
        mk_desc = lambda xs, zs, out, wsm, S, rep, x_co, z_cs: hip.groupdw_desc(
            [t.data_ptr() for t in xs], [t.data_ptr() for t in zs], out.data_ptr(), wsm, S=S, x_rep=rep, OH=OW, OW=OW, Cc=256,
            x_cs=[512] * 3, x_co=[x_co] * 3, z_cs=[z_cs] * 3, z_co=[x_co if z_cs == 512 else 0] * 3)
        arr = (hip.GroupDWDesc * 3)(mk_desc(esd, zkd, outs[0], w_reg, b, 1, 256, 512), mk_desc(esd, zkd, outs[1], w_cls, b, 1, 0, 512),
                                    mk_desc(esd, mkd, outs[2], w_cls, b * m, m, 0, 256))
        if dtype == torch.float32:
            hip.check(hip.lib().usot_groupdw_multi_f32(hip.stream(), arr, 3), 'groupdw_multi')
            lp_outs = None
        else:
            # the low-precision launch (always the LDS-DMA kernel, variant 6) is held to the fp32 launch of the SAME kernel on the
            # same maps, as in test_groupdw_and_conf_reduce_low_precision_outputs; that fp32 launch is held to float64
            hip.check(hip.lib().usot_groupdw_multi_lp(hip.stream(), arr, 3, 1 if dtype == torch.float16 else 2), 'groupdw_multi_lp')
            lp_outs, outs = outs, [c.out(tuple(o.shape)) for o in outs]
            for k in range(3):
                arr[k].out = outs[k].data_ptr()
                arr[k].cols_per_thread = 6
            hip.check(hip.lib().usot_groupdw_multi_f32(hip.stream(), arr, 3), 'groupdw_multi')
    no_nan(*outs)
    if lp_outs is not None:
        no_nan(*lp_outs)
        for lo, o in zip(lp_outs, outs):
            assert same_up_to_ties(lo, o)
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    for out, wsm, co, zs, rep in ((outs[0], w_reg, 256, [z[..., 256:] for z in zk], 1), (outs[1], w_cls, 0, [z[..., :256] for z in zk], 1),
                                  (outs[2], w_cls, 0, mk, m)):
        ref = 0
        for i in range(3):
            ref = ref + float(wsm[i]) * orc.xcorr_depthwise(nchw(es[i][..., co:co + 256]).repeat_interleave(rep, 0), nchw(zs[i]))
        assert rel_err(nchw(out.cpu()).numpy(), ref.numpy()) < 1e-5


@pytest.mark.parametrize('dtype', [pytest.param(torch.float32, id='f32')] + LP)
def test_conf_fusion_reduce(dtype):
    B, M = 3, 4
    g = torch.Generator().manual_seed(B * 10 + M)
    conf = torch.exp(torch.clamp(torch.randn(B, M, 256, 5, 6, generator=g) * 3, 0, 4))
    val = F.relu(torch.randn(B, M, 256, 5, 6, generator=g))
    ref = ((conf.double() / conf.double().sum(1, keepdim=True)) * val.double()).sum(1)
    cv = torch.cat([conf, val], 2).reshape(B * M, 512, 5, 6).permute(0, 2, 3, 1).contiguous()
    with contract() as c:
        cvd = c.put(cv)
        out = hip.conf_fusion_reduce(cvd, B, M)
        if dtype != torch.float32:          # the low-precision launch is held to the fp32 launch, the fp32 launch to float64
            lo = c.out((B, 5, 6, 256), dtype)
            hip.check(hip.lib().usot_conf_fusion_reduce_lp(hip.stream(), hip.ptr(cvd), 0, hip.ptr(lo), B, M, 30, 256,
                                                           1 if dtype == torch.float16 else 2), 'conf_reduce_lp')
    no_nan(out)
    assert rel_err(out.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < 1e-5
    if dtype != torch.float32:
        no_nan(lo)
        assert same_up_to_ties(lo, out)


# ------------------------------------------------------------------------------------------------------ PrRoIPool
def _prroi_case():
    g = torch.Generator().manual_seed(77)
    f = torch.randn(2, 32, 15, 17, generator=g)
    rois = torch.tensor(ROIS, dtype=torch.float32)
    top_diff = torch.randn(len(ROIS), 32, 7, 7, generator=g)
    return f, rois, top_diff


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_prroi_pool_forward(layout):
    import prroi_exact as ex
    f, rois, _ = _prroi_case()
    ref = orc.prroi_pool(f, rois, 7, 7, 1.0)
    want = ex.prroi_pool_exact(f.numpy(), rois.numpy(), 7, 7)
    with contract() as c:
        fd = c.put(f if layout == 'nchw' else f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
        out = hip.prroi_pool(fd, c.put(rois), 7, 7, 1.0, out_nhwc=(layout == 'nhwc'))
    no_nan(out)
    got = out.cpu().numpy()
    assert np.max(np.abs(got - ref.numpy())) < 2e-6 * max(1.0, float(ref.abs().max()))
    assert np.all(got[3] == 0) and np.all(got[6] == 0)        # zero-width roi, fully outside roi
    err = np.abs(got - want).reshape(len(ROIS), -1).max(1) / max(1.0, float(f.abs().max()))
    assert not (err > _prroi_tol(rois.numpy())).any(), err


def test_prroi_pool_gradients():
    """feature gradient (its output is allocated with `empty` and zero-filled by the entry point: every element must come back
    finite) and coordinate gradient on the ROIS list, against the float64 oracle and the float32 restatement"""
    import prroi_exact as ex
    f, rois, g = _prroi_case()
    rn = rois.numpy()
    with contract() as c:
        fd, rd, gd = c.puts(f, rois, g)
        top = hip.prroi_pool(fd, rd, 7, 7, 1.0)
        torch.cuda.synchronize()
        tsnap = guarded.snapshot(top)
        gf = hip.prroi_pool_backward(f.shape, rd, gd, 7, 7, 1.0)
        gr = hip.prroi_pool_coor_backward(fd, rd, top, gd, 7, 7, 1.0)
        torch.cuda.synchronize()
        guarded.unchanged(top, tsnap, 'top_data')
    assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gr).all())
    gf, gr = gf.cpu().numpy(), gr.cpu().numpy()
    want = ex.prroi_pool_exact_backward(f.shape, rn, g.numpy(), 7, 7, 1.0)
    ref = orc.prroi_pool_backward(f.shape, rn, g, 7, 7, 1.0).numpy()
    scale = max(1.0, float(np.abs(want).max()))
    assert np.max(np.abs(gf - want)) < 1.5e-4 * scale and np.max(np.abs(gf - ref)) < 1e-5 * scale
    wantr = ex.prroi_pool_exact_coor_backward(f.numpy(), rn, g.numpy(), 7, 7, 1.0)
    refr = orc.prroi_pool_coor_backward(f, rn, top.cpu(), g, 7, 7, 1.0).numpy()
    assert np.all(gr[:, 0] == 0)
    bins = np.minimum(rn[:, 3] - rn[:, 1], rn[:, 4] - rn[:, 2]) / 7
    mag = np.maximum(1.0, np.abs(wantr).max(1))
    e_exact, e_ref = np.abs(gr - wantr).max(1) / mag, np.abs(gr - refr).max(1) / mag
    assert np.all(e_exact[bins >= 0.2] <= 3e-5) and np.all(e_ref[bins >= 0.2] <= 3e-5), (e_exact, e_ref)
    assert np.all(e_exact[bins >= 0.05] <= 1.5e-4) and np.all(e_ref[bins >= 0.05] <= 1.5e-4)
    assert np.all(e_exact <= 5e-2)
    assert not gr[~(bins > 0)].any()


# ------------------------------------------------------------------------------------------------------ decode, crop
def test_decode_and_decode_dev(gold_host):
    p = orc.Hyper(255)
    S = p.score_size
    assert S == 25
    window = np.outer(np.hanning(S), np.hanning(S))
    for case in range(4):
        k = 'i255/decode%d' % case
        cls, cm, bbox = gold_host[k + '/cls'], gold_host[k + '/cls_mem'], gold_host[k + '/bbox']
        tsz, sz = gold_host[k + '/tsz'], float(gold_host[k + '/scale_z'])
        pos, szo, score, box, rc = orc.decode(p, cls[0, 0], cm[0, 0], bbox[0], gold_host[k + '/tpos'], tsz * sz, window, sz)
        with contract() as c:
            dcls, dcm, dbox, wd = c.puts(torch.from_numpy(cls).reshape(-1), torch.from_numpy(cm).reshape(-1),
                                         torch.from_numpy(bbox).reshape(4, -1), torch.from_numpy(window).reshape(-1))
            out = hip.decode(dcls, dcm, dbox, wd, S, 255, 8, p.ratio, p.penalty_k, p.window_influence, tsz[0] * sz, tsz[1] * sz)
            ctl = torch.zeros(8, dtype=torch.float64)
            ctl[0], ctl[1], ctl[6] = tsz[0] * sz, tsz[1] * sz, 42.0
            ctld = c.put(ctl)
            out2, roi = c.out((9,), torch.float64), c.out((5,))
            hip.check(hip.lib().usot_decode_dev_f32(hip.stream(), hip.ptr(dcls), hip.ptr(dcm), hip.ptr(dbox), hip.ptr(wd), hip.ptr(out2),
                                                    S, 255, 8, C.c_float(p.ratio), C.c_double(p.penalty_k), C.c_double(p.window_influence),
                                                    hip.ptr(ctld), hip.ptr(roi)), 'decode_dev')
        no_nan(out, out2, roi)
        for o in (out.cpu().numpy(), out2.cpu().numpy()):
            assert int(o[0]) == rc[0] * S + rc[1] and abs(o[1] - score) < 1e-6
            np.testing.assert_allclose(o[3:7], box, rtol=1e-9)
        assert out2.cpu().numpy()[8] == 42.0 and roi.cpu().numpy()[0] == 0.0
        if case == 1:                                           # the case test_decode_dev_writes_roi_and_tag holds to the golden box
            np.testing.assert_array_equal(roi.cpu().numpy()[1:], gold_host[k + '/out_poolbox'][0])


def _ctl(B, tag=7.0):
    from usot_amd.engine import SLOT_REC, STEP_HDR
    ctl = np.zeros(STEP_HDR + B * SLOT_REC.itemsize, np.uint8)
    ctl[:8].view(np.float64)[0] = tag
    return ctl, ctl[STEP_HDR:].view(SLOT_REC)


def test_decode_batch(gold_host):
    """B = 3 slots at S = 25: the golden decode cases 0..2, each slot against the oracle's decode and, bit for bit, against
    usot_decode_dev_f32 on the same slot"""
    p = orc.Hyper(255)
    S, B = p.score_size, 3
    window = np.outer(np.hanning(S), np.hanning(S))
    keys = ['i255/decode%d' % k for k in range(B)]
    cls = np.stack([gold_host[k + '/cls'][0, 0] for k in keys]).astype(np.float32)
    cm = np.stack([gold_host[k + '/cls_mem'][0, 0] for k in keys]).astype(np.float32)
    bbox = np.stack([gold_host[k + '/bbox'][0] for k in keys]).astype(np.float32)
    ctl, recs = _ctl(B, tag=41.0)
    for b, k in enumerate(keys):
        recs[b]['tsz'] = gold_host[k + '/tsz'] * float(gold_host[k + '/scale_z'])
    with contract() as c:
        dcls, dcm, dbox, wd, ctld = c.puts(torch.from_numpy(cls), torch.from_numpy(cm), torch.from_numpy(bbox),
                                           torch.from_numpy(window).reshape(-1), torch.from_numpy(ctl))
        out, roi = c.out((B, 16), torch.float64, 'zero'), c.out((B, 5))
        hip.decode_batch(dcls, dcm, dbox, wd, out, ctld, roi, S, 255, 8, p.ratio, p.penalty_k, p.window_influence)
        singles = []
        for b in range(B):
            c8 = torch.zeros(8, dtype=torch.float64)
            c8[0], c8[1], c8[6] = float(recs[b]['tsz'][0]), float(recs[b]['tsz'][1]), 41.0
            ref, rroi = c.out((10,), torch.float64, 'zero'), c.out((5,))
            hip.check(hip.lib().usot_decode_dev_f32(hip.stream(), hip.ptr(dcls[b]), hip.ptr(dcm[b]), hip.ptr(dbox[b]), hip.ptr(wd),
                                                    hip.ptr(ref), S, 255, 8, C.c_float(p.ratio), C.c_double(p.penalty_k),
                                                    C.c_double(p.window_influence), hip.ptr(c.put(c8)), hip.ptr(rroi)), 'decode_dev')
            singles.append((ref, rroi))
    o, r_ = out.cpu().numpy(), roi.cpu().numpy()
    assert np.isfinite(o[:, :9]).all() and np.isfinite(r_).all()
    for b, k in enumerate(keys):
        tsz, sz = gold_host[k + '/tsz'], float(gold_host[k + '/scale_z'])
        pos, szo, score, box, rc = orc.decode(p, cls[b], cm[b], bbox[b], gold_host[k + '/tpos'], tsz * sz, window, sz)
        assert int(o[b, 0]) == rc[0] * S + rc[1] and abs(o[b, 1] - score) < 1e-6
        np.testing.assert_allclose(o[b, 3:7], box, rtol=1e-9)
        assert o[b, 8] == 41.0 and r_[b, 0] == b
        ref, rroi = singles[b][0].cpu().numpy(), singles[b][1].cpu().numpy()
        assert np.array_equal(o[b, :8].view(np.int64), ref[:8].view(np.int64))
        assert np.array_equal(r_[b, 1:].view(np.int32), rroi[1:].view(np.int32))


CROPS = [((10.2, 8.9), 255), ((470.0, 350.0), 301)]          # the window hangs over the top-left / the bottom-right border


def test_crop_resize_and_batch():
    from usot_amd import hostutils, synth
    from usot_amd.engine import crop_fields
    im, _ = synth.frame(5, t=3)
    avg = np.mean(im, axis=(0, 1))
    S = 255
    B = len(CROPS)
    ctl, recs = _ctl(B)
    with contract() as c:
        imd = c.put(torch.from_numpy(np.ascontiguousarray(im)))
        singles = []
        for b, (pos, win) in enumerate(CROPS):
            x0, y0, w_, fill = crop_fields(im.shape, pos, win, avg)
            recs[b]['im'], recs[b]['H'], recs[b]['W'] = imd.data_ptr(), im.shape[0], im.shape[1]
            recs[b]['x0'], recs[b]['y0'], recs[b]['win'], recs[b]['fill'] = x0, y0, w_, fill
            singles.append(hip.crop_resize(imd, c.out((3, S, S)), x0, y0, w_, fill))
        out = c.out((B, 3, S, S))
        hip.crop_resize_batch(c.put(torch.from_numpy(ctl)), out)
    no_nan(out, *singles)
    for b, (pos, win) in enumerate(CROPS):
        want, _ = hostutils.get_subwindow_tracking(im, np.array(pos), S, win, avg)
        assert torch.equal(singles[b].cpu(), want) and torch.equal(out[b].cpu(), want), (pos, win)


# ------------------------------------------------------------------------------------------------------ copies
def test_permute4():
    t = torch.randn(3, 40, 7, 9, generator=torch.Generator().manual_seed(1))
    with contract() as c:
        d = c.put(t)
        nh = hip.to_nhwc(d)
        back = hip.to_nchw(nh)
        crop = hip.to_nhwc(d[:, :, 2:-2, 1:-3])
    assert torch.equal(nh.cpu(), t.permute(0, 2, 3, 1)) and torch.equal(back.cpu(), t)
    assert torch.equal(crop.cpu(), t[:, :, 2:-2, 1:-3].permute(0, 2, 3, 1))


def test_rows_copy_and_multi():
    g = torch.Generator().manual_seed(2)
    L = hip.lib()
    lens = [64, 128, 32, 256]
    pp = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])
    rl = (C.c_int32 * 4)(*lens)
    with contract() as c:
        bank = c.put(torch.randn(16, 64, generator=g))
        idx = c.put(torch.tensor([3, 0, 15, 7], dtype=torch.int32))
        out = c.out((4, 64))
        hip.check(L.usot_rows_copy_f32(hip.stream(), hip.ptr(bank), hip.ptr(idx), hip.ptr(out), 4, 64, 0), 'gather')
        dst = c.out((16, 64), prefill='zero')
        hip.check(L.usot_rows_copy_f32(hip.stream(), hip.ptr(out), hip.ptr(idx), hip.ptr(dst), 4, 64, 1), 'scatter')
        banks = c.puts(*[torch.randn(12, n, generator=g) for n in lens])
        idx7 = c.put(torch.tensor([5, 0, 11, 7, 9, 1234, -77], dtype=torch.int32))      # 4 rows (one the bank's last) + the stash
        outs = [c.out((4, n)) for n in lens]
        stash = c.out((4,), torch.int32, 'zero')
        hip.check(L.usot_rows_copy_multi_f32(hip.stream(), 4, pp(banks), hip.ptr(idx7), pp(outs), 4, rl, 0, hip.ptr(stash)), 'gather')
        dsts = [c.out((12, n), prefill='zero') for n in lens]
        hip.check(L.usot_rows_copy_multi_f32(hip.stream(), 4, pp(outs), hip.ptr(idx7), pp(dsts), 4, rl, 1, None), 'scatter')
    assert torch.equal(out, bank[idx.long()])
    want = torch.zeros(16, 64, device=DEV)
    want[idx.long()] = out
    assert torch.equal(dst, want)
    assert stash.tolist() == [9, 1234, -77, 0]
    for b, o, d in zip(banks, outs, dsts):
        assert torch.equal(o, b[idx7[:4].long()])
        want = torch.zeros_like(d)
        want[idx7[:4].long()] = o
        assert torch.equal(d, want)


def test_rows_append_gather_on_the_last_row():
    lens = [7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 64]
    g = torch.Generator().manual_seed(11)
    picks, slot = [0, 1, 2, 11, 11, 2, 11], 11                         # the append lands on the last row of the 12-row banks
    nq = len(picks)
    p4 = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])
    bank_cpu = [torch.randn(12, n, generator=g) for n in lens]
    with contract() as c:
        banks = [guarded.put(b, DEV) for b in bank_cpu]                 # written in place: not in the unchanged list
        fresh = c.puts(*[torch.randn(1, n, generator=g) for n in lens])
        idx = c.put(torch.tensor(picks + [-5, 123, 456, slot], dtype=torch.int32))
        picked = [c.out((nq, n)) for n in lens[1:]]
        p3 = (C.c_void_p * 3)(*[t.data_ptr() for t in picked])
        hip.check(hip.lib().usot_rows_append_gather_f32(hip.stream(), p4(fresh), p4(banks), p3, (C.c_int32 * 4)(*lens),
                                                        hip.ptr(idx), nq, nq + 3), 'rows_append_gather')
    no_nan(*picked)
    for k in range(4):
        want = bank_cpu[k].clone()
        want[slot] = fresh[k][0].cpu()
        assert torch.equal(banks[k].cpu(), want), k
        if k:
            assert torch.equal(picked[k - 1].cpu(), want[torch.tensor(picks).long()]), k


def test_rows_append_gather_batch_on_the_last_row():
    B, cap, nq = 3, 10, 7
    lens = [7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 5 * 3 * 256]
    g = torch.Generator().manual_seed(5)
    bank_cpu = [torch.randn(B * cap, n, generator=g) for n in lens]
    ctl, recs = _ctl(B)
    app = [9, 19, 29]                                   # every slot appends to the last row of its part; slot 2's is the bank's last
    picks = [[0, 1, 2, 3, 9, 9, 2], [10, 11, 12, 19, 19, 13, 12], [20, 21, 22, 29, 25, 23, 29]]
    for b in range(B):
        recs[b]['append_row'] = app[b]
        recs[b]['picks'][:nq] = picks[b]
    with contract() as c:
        banks = [guarded.put(b, DEV) for b in bank_cpu]
        fresh = c.puts(*[torch.randn(B, n, generator=g) for n in lens])
        picked = [c.out((B * nq, n)) for n in lens[1:]]
        hip.rows_append_gather_batch(fresh, banks, picked, c.put(torch.from_numpy(ctl)), nq)
    no_nan(*picked)
    for k in range(4):
        want = bank_cpu[k].clone()
        for b in range(B):
            want[app[b]] = fresh[k][b].cpu()
        assert torch.equal(banks[k].cpu(), want), k
        if k:
            wp = torch.stack([want[r] for b in range(B) for r in picks[b]])
            assert torch.equal(picked[k - 1].cpu(), wp), k
