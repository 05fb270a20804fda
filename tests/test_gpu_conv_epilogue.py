"""GPU: what the conv EPILOGUE does with a finished sum - the part of usot_conv_desc (include/usot_hip.h) behind the k-loop.
fp32 (usot_conv2d_f32, every tile of test_gpu_tile_edges.sweep_tiles()): act / act2 with act_split at every residue of the
four-channel vector group, output into and residual out of a channel slice (y_cstride / y_coff / res_cstride / res_coff), EXP and
CONF on every epilogue code path, groups with gaps between the groups, and a batch launch that mixes all of it.  Low precision
(usot_conv2d_lp, every built tile id, bf16 and fp16): Cout on both sides of the tile edge in both Cout % 8 classes (the 16-byte LDS
epilogue and the 8-byte piece epilogue), M on both sides of the pixel edge, legal split activations, padded groups - and the
descriptor fields that launcher does not support, which it must REJECT rather than ignore.

Every launch follows tests/test_gpu_memory_contract.py: inputs placed with a NaN on both sides and compared bit for bit
afterwards, outputs NaN-prefilled between canaries, split-K workspaces NaN-prefilled with zero ticket words that must be zero
again afterwards.  References are float64 on the CPU (low precision: on the operands rounded to the storage type).  Bars are the
kernels' own (tests/test_gpu_ops.py: rel_err): 2e-5 for fp32 results, 6e-3 / 1e-3 for bf16 / fp16 results.  With a split
activation the bar holds on the `act` channels and on the `act2` channels SEPARATELY (seg_err): rel_err's floor is the mean
|ref| of what is compared, and a CONF half (values up to e^4) must not raise it under the other half.  The smallest comparison
is one channel of M = bm + 1 >= 17 rows.

Where an output is a slice of a larger buffer, every other element of the buffer must still hold the prefill BIT PATTERN.

One item = one (tile, family); it loops over its list and reports every failing case, not the first one.  The lists are asserted
by tests/test_conv_epilogue_lists.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402
import guarded  # noqa: E402
from test_gpu_memory_contract import contract, no_nan  # noqa: E402
from test_gpu_ops import pack_w, rel_err  # noqa: E402
from test_gpu_tile_edges import _conv, _conv_bank, _conv_setup, report, sweep_tiles  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
NONE, RELU, EXP, CONF = hip.ACT_NONE, hip.ACT_RELU, hip.ACT_EXP, hip.ACT_CONF
EINVAL = -1
BAR = 2e-5
NAN = float('nan')
PREFILL16 = guarded.CANARY
PREFILL32 = (guarded.CANARY << 16) | guarded.CANARY

# ---------------------------------------------------------------------------------------------------------------- the lists
PAIRS = [(CONF, RELU), (RELU, NONE), (NONE, EXP)]
GEO = {1: {}, 2: dict(KH=3, KW=3, pad=(0, 1))}        # ksplit -> geometry: 1x1 (K = 64), or 3x3 on x [1, 3, M, 64] (K = 576)
LP_ROUTED = [1, 4, 5, 11, 12, 13, 14, 21, 25, 26, 32, 37]
LP_FORMS = ['lp', 'lp_res_relu', 'f32']


def a1_couts(bn):
    return [(bn + 8, 'vector'), (bn + 7, 'scalar')]


def a1_splits(bn, cout):
    return [1, 2, 3, 4, 5, 6, 7, 8, bn - 1, bn, bn + 1, cout - 1]


def a2_cases(bn):
    """(Cout, y_cstride, y_coff, store path)"""
    return [(bn, bn + 4, 4, 'vector'), (bn, 2 * bn, bn, 'vector'), (bn + 4, 2 * bn + 8, bn + 4, 'vector'),
            (bn, bn + 3, 1, 'scalar'), (bn - 1, 2 * bn, bn, 'scalar')]


def a3_cases(cout):
    """(res_cstride, res_coff)"""
    return [(cout + 4, 4), (2 * cout, cout), (cout + 3, 1)]


def a5_forms(M, cout):
    """form -> (gaps behind the dense size of x, w, bias, y, res per group; y_nchw)"""
    return {'vector': (dict(x=4, w=8, b=4, y=8, r=12), False),
            'scalar': (dict(x=4, w=8, b=3, y=5, r=7), False),
            'nchw': (dict(x=4, w=8, b=4, y=8, r=12), True)}


def a6_couts(bn):
    return sorted({4, 8, 12, 60, 68, bn - 4, bn, bn + 4, bn + 8, bn + 12})


def a7_m_list(bm):
    return [1, 2, bm - 1, bm, bm + 1, 2 * bm + 1]


def a8_splits(bn):
    return [8, bn - 8, bn, bn + 8]


def takes_vector_store(cout, act=NONE, act2=NONE, act_split=0, y_cstride=0, y_coff=0, res=False, res_cstride=0, res_coff=0, y_nchw=False):
    """the documented rule (usot_hip.h): 16-byte epilogue iff NHWC, every stride / offset a multiple of 4 and the activation
    constant over each group of four channels; Cout % 4 != 0 leaves the last group to the scalar code"""
    ycs, rcs = y_cstride or cout, res_cstride or cout
    return (not y_nchw and ycs % 4 == 0 and y_coff % 4 == 0 and (not res or (rcs % 4 == 0 and res_coff % 4 == 0))
            and (act_split <= 0 or act_split % 4 == 0 or act == act2) and cout % 4 == 0)


# ------------------------------------------------------------------------------------------------------------ the reference
def act_ref(v, a):
    """usot_hip.h: NONE, RELU, EXP = exp(x), CONF = exp(min(max(x, 0), 4)) - float64"""
    if a == RELU:
        return v.clamp_min(0)
    if a == EXP:
        return v.exp()
    if a == CONF:
        return v.clamp(0, 4).exp()
    assert a == NONE
    return v


def split_act_ref(pre, act, act2, act_split):
    """usot_hip.h: act on channels [0, act_split), act2 on [act_split, Cout); act_split <= 0 or >= Cout: act everywhere.
    pre [..., Cout] float64.  Decided per CHANNEL."""
    first = torch.arange(pre.shape[-1]) < (act_split if act_split > 0 else pre.shape[-1])
    return torch.where(first, act_ref(pre, act), act_ref(pre, act2))


def seg_err(got, ref, act_split):
    """rel_err on the `act` channels and on the `act2` channels, each against its own floor: the larger of the two"""
    cout = ref.shape[-1]
    s = act_split if 0 < act_split < cout else cout
    got, ref = np.asarray(got), np.asarray(ref)
    return max(rel_err(got[:, a:b], ref[:, a:b]) for a, b in ((0, s), (s, cout)) if b > a)


def untouched(buf, written):
    """every element of `buf` outside the boolean mask `written` still holds the prefill bit pattern"""
    if buf.element_size() == 4:
        bits, want = buf.view(torch.int32), PREFILL32
    else:
        bits, want = buf.view(torch.int16), PREFILL16
    return bool((bits[~written.to(buf.device)] == want).all())


def _cols(M, cs, lo, hi):
    m = torch.zeros(M, cs, dtype=torch.bool)
    m[:, lo:hi] = True
    return m


def _problem(M, cout, seed, k3):
    """-> x NHWC, packed bank [cout][K], bias = 3 randn (pre-activations below 0, in (0, 4) and above 4), residual [M][cout],
    float64 conv + bias [M][cout]"""
    g = torch.Generator().manual_seed(seed)
    if k3:
        x = torch.randn(1, 64, 3, M, generator=g)
        w = torch.randn(cout, 64, 3, 3, generator=g) / 24
        b = 3 * torch.randn(cout, generator=g)
        pre = F.conv2d(x.double(), w.double(), b.double(), 1, (0, 1))[0, :, 0].t().contiguous()
        xn, wp = x.permute(0, 2, 3, 1).contiguous(), pack_w(w)
    else:
        x = torch.randn(M, 64, generator=g)
        wp = torch.randn(cout, 64, generator=g) / 8
        b = 3 * torch.randn(cout, generator=g)
        pre = x.double() @ wp.double().t() + b.double()
        xn = x.reshape(1, 1, M, 64)
    res = torch.randn(M, cout, generator=g)
    return xn, wp, b, res, pre


TILES = conftest.tile_params(sweep_tiles())


# ---------------------------------------------------------------------------------------------------------- A1 - A5: fp32
@pytest.mark.parametrize('ksplit', [1, 2], ids=['k1', 'k2'])
@pytest.mark.parametrize('tile', TILES)
def test_act_split_at_every_residue(tile, ksplit):
    """A1.  M = bm + 1; Cout = bn + 8 (16-byte stores) and bn + 7 (scalar stores); every act_split of a1_splits() under every
    pair of PAIRS (ksplit 2, the in-launch combine: the (CONF, RELU) pair), against float64 with the activation chosen per
    channel.  A split inside a group of four channels must take the per-channel epilogue (fill_params: vec_store)."""
    bm, bn = hip.tile_table()[tile]
    M = bm + 1
    xn, wp, b, _, pre = _problem(M, bn + 8, 1000 + tile + ksplit, ksplit == 2)
    worst, bad = 0.0, []
    with contract() as c:
        xd = c.put(xn)
        ovf = c.out((1,), torch.int32, 'zero')
        for cout, path in a1_couts(bn):
            bank = _conv_bank(c, tile, wp[:cout].contiguous(), b[:cout].contiguous())
            for act, act2 in (PAIRS if ksplit == 1 else PAIRS[:1]):
                for split in a1_splits(bn, cout):
                    y = _conv(c, tile, xd, bank, Cout=cout, act=act, act2=act2, act_split=split, ksplit=ksplit,
                              ovf=ovf if bank[3] == 2 else None, **GEO[ksplit]).reshape(M, cout)
                    e = seg_err(y.cpu().numpy(), split_act_ref(pre[:, :cout], act, act2, split).numpy(), split)
                    print('A1 tile %d %s Cout %d acts (%d, %d) act_split %d ksplit %d: %.3g' % (tile, path, cout, act, act2, split, ksplit, e))
                    worst = max(worst, e)
                    if not e < BAR:
                        bad.append((path, cout, (act, act2), split, e))
        assert int(ovf.item()) == 0
    report('E1', 'tile %d (%d x %d) ksplit %d' % (tile, bm, bn, ksplit), worst)
    assert not bad, bad


@pytest.mark.parametrize('tile', TILES)
def test_output_into_a_channel_slice(tile):
    """A2.  y = columns [coff, coff + Cout) of a NaN-prefilled [M][cs] map: plain and residual + ReLU, ksplit 1 and 2; every
    other element keeps its bits.  Two launches that fill the halves of one [M][2 bn] map against one launch of Cout = 2 bn."""
    bm, bn = hip.tile_table()[tile]
    M = bm + 1
    worst, bad = 0.0, []
    for ks in (1, 2):
        xn, wp, b, res, pre = _problem(M, 2 * bn, 2000 + tile + ks, ks == 2)
        with contract() as c:
            xd = c.put(xn)
            ovf = c.out((1,), torch.int32, 'zero')
            banks = {}

            def bank_of(lo, hi):
                if (lo, hi) not in banks:
                    banks[lo, hi] = _conv_bank(c, tile, wp[lo:hi].contiguous(), b[lo:hi].contiguous())
                return banks[lo, hi]

            def launch(lo, hi, y, cs, coff, rd=None, act=NONE):
                bank = bank_of(lo, hi)
                return _conv(c, tile, xd, bank, Cout=hi - lo, y=y, y_cstride=cs, y_coff=coff, res=rd, act=act, ksplit=ks,
                             ovf=ovf if bank[3] == 2 else None, **GEO[ks])

            for cout, cs, coff, path in a2_cases(bn):
                for form in ('plain', 'res_relu'):
                    rd = c.put(res[:, :cout].contiguous()) if form == 'res_relu' else None
                    want = (pre[:, :cout] + res[:, :cout].double()).relu() if rd is not None else pre[:, :cout]
                    y = launch(0, cout, c.out((M, cs)), cs, coff, rd, RELU if rd is not None else NONE)
                    got = y[:, coff:coff + cout]
                    no_nan(got)
                    e = rel_err(got.cpu().numpy(), want.numpy())
                    kept = untouched(y, _cols(M, cs, coff, coff + cout))
                    print('A2 tile %d %s (Cout %d, cs %d, coff %d) %s ksplit %d: %.3g, rest untouched: %s' % (tile, path, cout, cs, coff, form, ks, e, kept))
                    worst = max(worst, e)
                    if not (e < BAR and kept):
                        bad.append((path, cout, cs, coff, form, ks, e, kept))
            y2 = c.out((M, 2 * bn))
            launch(0, bn, y2, 2 * bn, 0)
            launch(bn, 2 * bn, y2, 2 * bn, bn)
            y1 = _conv(c, tile, xd, bank_of(0, 2 * bn), Cout=2 * bn, ksplit=ks, ovf=ovf if bank_of(0, 2 * bn)[3] == 2 else None,
                       **GEO[ks]).reshape(M, 2 * bn)
            no_nan(y2)
            e2, e1, e21 = (rel_err(y2.cpu().numpy(), pre.numpy()), rel_err(y1.cpu().numpy(), pre.numpy()),
                           rel_err(y2.cpu().numpy(), y1.cpu().double().numpy()))
            print('A2 tile %d two halves ksplit %d: %.3g, one launch %.3g, halves against it %.3g' % (tile, ks, e2, e1, e21))
            worst = max(worst, e2, e1, e21)
            if not (e2 < BAR and e1 < BAR and e21 < BAR):
                bad.append(('halves', ks, e2, e1, e21))
            assert int(ovf.item()) == 0
    report('E2', 'tile %d (%d x %d)' % (tile, bm, bn), worst)
    assert not bad, bad


@pytest.mark.parametrize('tile', TILES)
def test_residual_from_a_channel_slice(tile):
    """A3.  res = columns [rcoff, rcoff + Cout) of an [M][rcs] map that is NaN everywhere else; dense y, ReLU, Cout = bn + 4,
    ksplit 1 and 2.  The last case writes a channel slice as well, with another stride than the residual's."""
    bm, bn = hip.tile_table()[tile]
    M, cout = bm + 1, bn + 4
    worst, bad = 0.0, []
    for ks in (1, 2):
        xn, wp, b, res, pre = _problem(M, cout, 3000 + tile + ks, ks == 2)
        want = (pre + res.double()).relu()
        with contract() as c:
            xd = c.put(xn)
            ovf = c.out((1,), torch.int32, 'zero')
            bank = _conv_bank(c, tile, wp, b)
            for (rcs, rcoff), yslice in [(rc, None) for rc in a3_cases(cout)] + [((cout + 4, 4), (2 * bn + 8, bn + 4))]:
                rbuf = torch.full((M, rcs), NAN)
                rbuf[:, rcoff:rcoff + cout] = res
                kw = dict(res=c.put(rbuf), res_cstride=rcs, res_coff=rcoff, act=RELU, ksplit=ks, ovf=ovf if bank[3] == 2 else None, **GEO[ks])
                kept = True
                if yslice is None:
                    y = _conv(c, tile, xd, bank, Cout=cout, **kw).reshape(M, cout)
                else:
                    cs, coff = yslice
                    buf = _conv(c, tile, xd, bank, Cout=cout, y=c.out((M, cs)), y_cstride=cs, y_coff=coff, **kw)
                    y = buf[:, coff:coff + cout]
                    no_nan(y)
                    kept = untouched(buf, _cols(M, cs, coff, coff + cout))
                e = rel_err(y.cpu().numpy(), want.numpy())
                print('A3 tile %d (rcs %d, rcoff %d) y slice %s ksplit %d: %.3g, rest untouched: %s' % (tile, rcs, rcoff, yslice, ks, e, kept))
                worst = max(worst, e)
                if not (e < BAR and kept):
                    bad.append((rcs, rcoff, yslice, ks, e, kept))
            assert int(ovf.item()) == 0
    report('E3', 'tile %d (%d x %d)' % (tile, bm, bn), worst)
    assert not bad, bad


@pytest.mark.parametrize('tile', TILES)
def test_exp_and_conf_on_every_tile(tile):
    """A4.  EXP and CONF, with and without a residual, at Cout = bn + 4 (16-byte stores) and bn + 3 (scalar stores; NHWC and NCHW),
    pre-activations spread as in A1."""
    bm, bn = hip.tile_table()[tile]
    M = bm + 1
    xn, wp, b, res, pre = _problem(M, bn + 4, 4000 + tile, False)
    worst, bad = 0.0, []
    with contract() as c:
        xd = c.put(xn)
        ovf = c.out((1,), torch.int32, 'zero')
        for cout, layouts in ((bn + 4, (False,)), (bn + 3, (False, True))):
            bank = _conv_bank(c, tile, wp[:cout].contiguous(), b[:cout].contiguous())
            rd = c.put(res[:, :cout].contiguous())
            for act in (EXP, CONF):
                for r in (None, rd):
                    for nchw in layouts:
                        y = _conv(c, tile, xd, bank, Cout=cout, act=act, res=r, y_nchw=nchw, ovf=ovf if bank[3] == 2 else None)
                        got = y.reshape(cout, M).t() if nchw else y.reshape(M, cout)
                        want = act_ref(pre[:, :cout] + (res[:, :cout].double() if r is not None else 0), act)
                        e = rel_err(got.cpu().numpy(), want.numpy())
                        print('A4 tile %d Cout %d act %d res %d nchw %d: %.3g' % (tile, cout, act, r is not None, nchw, e))
                        worst = max(worst, e)
                        if not e < BAR:
                            bad.append((cout, act, r is not None, nchw, e))
        assert int(ovf.item()) == 0
    report('E4', 'tile %d (%d x %d)' % (tile, bm, bn), worst)
    assert not bad, bad


def _flat(parts, stride, dtype=torch.float32):
    """CPU buffer [len(parts) * stride]: part g at g * stride (copied bit for bit), NaN in the gaps"""
    buf = torch.full((len(parts) * stride,), NAN, dtype=dtype)
    bits = torch.int32 if buf.element_size() == 4 else torch.int16
    for g, p in enumerate(parts):
        p = p.detach().cpu().contiguous().reshape(-1)
        assert p.dtype == dtype and p.numel() <= stride
        buf.view(bits)[g * stride:g * stride + p.numel()] = p.view(bits)
    return buf


def _group_bank(c, tile, ws, bs, w_gs, b_gs):
    """_conv_bank for several groups: the banks w_gs floats apart, biases (and split-fp16 row factors) b_gs apart, NaN between"""
    frag = hip.tile_wfrag(tile)
    assert frag in (0, 2), (tile, frag)
    if frag == 2:
        packed = [hip.split16_pack(w.to(DEV)) for w in ws]
        return c.put(_flat([p[0] for p in packed], w_gs)), c.put(_flat([p[1] for p in packed], b_gs)), c.put(_flat(bs, b_gs)), frag
    return c.put(_flat(ws, w_gs)), None, c.put(_flat(bs, b_gs)), frag


@pytest.mark.parametrize('tile', TILES)
def test_groups_with_gaps_between_them(tile):
    """A5.  groups = 3, Cout = bn + 4, residual + ReLU; x_gs, w_gs, b_gs, y_gs, r_gs each larger than the dense size with NaN in the
    gaps: by multiples of 4 (16-byte stores), with y_gs / r_gs / b_gs larger by an odd count (scalar stores), and NCHW.  The gaps
    of y keep the prefill."""
    bm, bn = hip.tile_table()[tile]
    G, M, cout = 3, bm + 1, bn + 4
    probs = [_problem(M, cout, 5000 + tile + 7 * g, False) for g in range(G)]
    worst, bad = 0.0, []
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        for form, (gap, nchw) in a5_forms(M, cout).items():
            gs = dict(x_gs=M * 64 + gap['x'], w_gs=cout * 64 + gap['w'], b_gs=cout + gap['b'], y_gs=M * cout + gap['y'], r_gs=M * cout + gap['r'])
            bank = _group_bank(c, tile, [p[1] for p in probs], [p[2] for p in probs], gs['w_gs'], gs['b_gs'])
            xd = c.put(_flat([p[0] for p in probs], gs['x_gs']))
            rd = c.put(_flat([p[3] for p in probs], gs['r_gs']))
            y = _conv(c, tile, xd, bank, Cout=cout, y=c.out((G * gs['y_gs'],)), xshape=(1, 1, M, 64), res=rd, act=RELU, y_nchw=nchw,
                      groups=G, ovf=ovf if bank[3] == 2 else None, **gs)
            written = torch.zeros(G * gs['y_gs'], dtype=torch.bool)
            for g in range(G):
                written[g * gs['y_gs']:g * gs['y_gs'] + M * cout] = True
                blk = y[g * gs['y_gs']:g * gs['y_gs'] + M * cout]
                got = blk.reshape(cout, M).t() if nchw else blk.reshape(M, cout)
                no_nan(got)
                e = rel_err(got.cpu().numpy(), (probs[g][4] + probs[g][3].double()).relu().numpy())
                print('A5 tile %d %s group %d: %.3g' % (tile, form, g, e))
                worst = max(worst, e)
                if not e < BAR:
                    bad.append((form, g, e))
            if not untouched(y, written):
                bad.append((form, 'a gap of y was written'))
        assert int(ovf.item()) == 0
    report('E5', 'tile %d (%d x %d)' % (tile, bm, bn), worst)
    assert not bad, bad


def test_batch_of_three_descriptors_equals_the_single_launches():
    """A5.  One usot_conv2d_batch_f32 launch on the heuristic tile of three descriptors of one geometry (M = 40, Cout = 72) that
    carry an unaligned act_split, an output slice and a residual slice: bit-equal to the three single launches, and right."""
    M, cout = 40, 72
    probs = [_problem(M, cout, 6000 + i, False) for i in range(3)]
    wants = [split_act_ref(probs[0][4], CONF, RELU, 5), probs[1][4], (probs[2][4] + probs[2][3].double()).relu()]
    rbuf = torch.full((M, 2 * cout), NAN)
    rbuf[:, cout:] = probs[2][3]
    worst = 0.0
    with contract() as c:
        xs = [c.put(p[0]) for p in probs]
        banks = [_conv_bank(c, 0, p[1], p[2]) for p in probs]
        rd = c.put(rbuf)
        fields = [dict(act=CONF, act2=RELU, act_split=5),
                  dict(y_cstride=cout + 4, y_coff=4),
                  dict(res=rd, res_cstride=2 * cout, res_coff=cout, act=RELU)]
        shapes = [(M, cout), (M, cout + 4), (M, cout)]
        single = [_conv(c, 0, xs[i], banks[i], Cout=cout, y=c.out(shapes[i]), **fields[i]) for i in range(3)]
        setups = [_conv_setup(c, 0, xs[i], banks[i], Cout=cout, y=c.out(shapes[i]), **fields[i]) for i in range(3)]
        arr = (hip.ConvDesc * 3)(*[s[0] for s in setups])
        assert len({int(hip.lib().usot_conv_resolve_tile(C.byref(s[0]))) for s in setups}) == 1       # one tile: bit-equality is owed
        hip.check(hip.lib().usot_conv2d_batch_f32(hip.stream(), arr, 3), 'usot_conv2d_batch_f32')
        for i, (s, one) in enumerate(zip(setups, single)):
            assert torch.equal(s[1].view(torch.int32), one.view(torch.int32)), i
            got = s[1][:, 4:] if i == 1 else s[1]
            no_nan(got)
            e = seg_err(got.cpu().numpy(), wants[i].numpy(), 5 if i == 0 else 0)
            worst = max(worst, e)
            assert e < BAR, (i, e)
        assert untouched(setups[1][1], _cols(M, cout + 4, 4, cout + 4))
    report('E5', 'batch of three on the heuristic tile', worst)


# ------------------------------------------------------------------------------------------------- A6 - A9: low precision
def lp_tile_ids():
    L = conftest._lib()
    return list(range(1, L.usot_conv_bf16_tile_count() + 1)) if L is not None else []


LP_TILES = conftest.tile_params(lp_tile_ids(), lp=True)
LP_DT = [pytest.param(torch.bfloat16, id='bf16'), pytest.param(torch.float16, id='fp16')]
BAR16 = {torch.bfloat16: 6e-3, torch.float16: 1e-3}       # test_conv_bf16 / test_conv_fp16_and_f32_out


def _lp_problem(M, cin, cout, dtype, seed, bias_scale=1.0):
    """operands rounded to the storage type first; float64 conv + bias of the ROUNDED operands"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, cin, generator=g).to(dtype)
    w = (torch.randn(cout, cin, generator=g) / np.sqrt(cin)).to(dtype)
    b = bias_scale * torch.randn(cout, generator=g)
    res = torch.randn(M, cout, generator=g).to(dtype)
    return x, w, b, res, x.double() @ w.double().t() + b.double()


def _lp(c, tile, x, w, b, *, M, Cin, Cout, res=None, act=NONE, out_f32=False, y=None, expect=0, **fields):
    """one usot_conv2d_lp launch of the 1x1 problem x [1, 1, M, Cin]; `expect`: the status the launcher must return"""
    out = y if y is not None else c.out((M, Cout), torch.float32 if out_f32 else x.dtype)
    d = hip.conv_desc(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), N=1, H=1, W=M, Cin=Cin, OH=1, OW=M, Cout=Cout, KH=1, KW=1,
                      res=res.data_ptr() if res is not None else None, act=act, tile=tile, **fields)
    rc = int(hip.lib().usot_conv2d_lp(hip.stream(), C.byref(d), 1 if x.dtype == torch.float16 else 0, int(out_f32)))
    assert rc == expect, 'usot_conv2d_lp tile %d M = %d Cout = %d %s: status %d, expected %d' % (tile, M, Cout, fields, rc, expect)
    if y is None and expect == 0:
        no_nan(out)
    return out


def _lp_bar(dtype, out_f32):
    return BAR if out_f32 else BAR16[dtype]


@pytest.mark.parametrize('dtype', LP_DT)
@pytest.mark.parametrize('tile', LP_TILES)
def test_lp_channel_edge(tile, dtype):
    """A6.  1x1, Cin = 192 (three k-tiles), M = bm + 1, Cout of a6_couts(): both Cout % 8 classes (16-byte LDS epilogue, 8-byte piece
    epilogue) on both sides of the tile edge, filter rows >= Cout redirected; 16-bit plain, 16-bit residual + ReLU, fp32 plain."""
    bm, bn = hip.tile_table_lp()[tile]
    M, couts = bm + 1, a6_couts(bn)
    x, w, b, res, pre = _lp_problem(M, 192, max(couts), dtype, 7000 + tile)
    worst, bad = {f: 0.0 for f in LP_FORMS}, []
    with contract() as c:
        xd = c.put(x)
        for cout in couts:
            wd, bd, rd = c.puts(w[:cout].contiguous(), b[:cout].contiguous(), res[:, :cout].contiguous())
            for form in LP_FORMS:
                r = rd if form == 'lp_res_relu' else None
                y = _lp(c, tile, xd, wd, bd, M=M, Cin=192, Cout=cout, res=r, act=RELU if r is not None else NONE, out_f32=form == 'f32')
                want = (pre[:, :cout] + res[:, :cout].double()).relu() if r is not None else pre[:, :cout]
                e = rel_err(y.float().cpu().numpy(), want.numpy())
                print('A6 lp tile %d %s Cout %d %s: %.3g' % (tile, dtype, cout, form, e))
                worst[form] = max(worst[form], e)
                if not e < _lp_bar(dtype, form == 'f32'):
                    bad.append((cout, form, e))
    for form in LP_FORMS:
        report('E6', 'lp tile %d (%d x %d) %s %s' % (tile, bm, bn, dtype, form), worst[form])
    assert not bad, bad


@pytest.mark.parametrize('dtype', LP_DT)
@pytest.mark.parametrize('tile', LP_TILES)
def test_lp_pixel_edge(tile, dtype):
    """A7.  1x1, Cin = 64 (one k-tile: the pipelines' prologue only), Cout = bn, M of a7_m_list() in allocations of exactly M rows
    (pixel rows >= M come from the zero page); 16-bit residual + ReLU and fp32 plain.  A row's lane is m % bm whatever M is:
    bit-equal to the first M rows of the 2 bm + 1 run."""
    bm, bn = hip.tile_table_lp()[tile]
    ms = a7_m_list(bm)
    mx = max(ms)
    x, w, b, res, pre = _lp_problem(mx, 64, bn, dtype, 8000 + tile)
    worst, bad = {'lp_res_relu': 0.0, 'f32': 0.0}, []
    with contract() as c:
        wd, bd = c.puts(w, b)
        for form in ('lp_res_relu', 'f32'):
            want = (pre + res.double()).relu() if form == 'lp_res_relu' else pre

            def run(M):
                xd, rd = c.puts(x[:M].contiguous(), res[:M].contiguous() if form == 'lp_res_relu' else None)
                return _lp(c, tile, xd, wd, bd, M=M, Cin=64, Cout=bn, res=rd, act=RELU if rd is not None else NONE, out_f32=form == 'f32')

            ymax = run(mx)
            for M in ms:
                y = run(M)
                e = rel_err(y.float().cpu().numpy(), want[:M].numpy())
                same = torch.equal(y, ymax[:M])
                print('A7 lp tile %d %s M %d %s: %.3g, bit-equal to the long run: %s' % (tile, dtype, M, form, e, same))
                worst[form] = max(worst[form], e)
                if not (e < _lp_bar(dtype, form == 'f32') and same):
                    bad.append((M, form, e, same))
    for form, e in worst.items():
        report('E7', 'lp tile %d (%d x %d) %s %s' % (tile, bm, bn, dtype, form), e)
    assert not bad, bad


@pytest.mark.parametrize('dtype', LP_DT)
@pytest.mark.parametrize('tile', LP_TILES)
def test_lp_contract_edges(tile, dtype):
    """A8.  The legal split activations - act_split of a8_splits() (multiples of 8), Cout = bn + 16, (CONF, RELU), 16-bit and fp32
    output, each activation segment against its own floor - and groups = 3 with x_gs / w_gs / b_gs / y_gs padded by multiples of
    8, NaN in the input gaps, the gaps of y keeping their prefill."""
    bm, bn = hip.tile_table_lp()[tile]
    G, M, cout = 3, bm + 1, bn + 16
    probs = [_lp_problem(M, 64, cout, dtype, 9000 + tile + 7 * g, 3.0) for g in range(G)]
    x, w, b, _, pre = probs[0]
    worst, bad = {False: 0.0, True: 0.0}, []
    with contract() as c:
        xd, wd, bd = c.puts(x, w, b)
        for out_f32 in (False, True):
            for split in a8_splits(bn):
                y = _lp(c, tile, xd, wd, bd, M=M, Cin=64, Cout=cout, act=CONF, act2=RELU, act_split=split, out_f32=out_f32)
                e = seg_err(y.float().cpu().numpy(), split_act_ref(pre, CONF, RELU, split).numpy(), split)
                print('A8 lp tile %d %s act_split %d f32 %d: %.3g' % (tile, dtype, split, out_f32, e))
                worst[out_f32] = max(worst[out_f32], e)
                if not e < _lp_bar(dtype, out_f32):
                    bad.append(('split', split, out_f32, e))
        gs = dict(x_gs=M * 64 + 8, w_gs=cout * 64 + 16, b_gs=cout + 8, y_gs=M * cout + 24)
        xg = c.put(_flat([p[0] for p in probs], gs['x_gs'], dtype))
        wg = c.put(_flat([p[1] for p in probs], gs['w_gs'], dtype))
        bg = c.put(_flat([p[2] for p in probs], gs['b_gs']))
        for out_f32 in (False, True):
            y = _lp(c, tile, xg, wg, bg, M=M, Cin=64, Cout=cout, act=RELU, out_f32=out_f32, groups=G,
                    y=c.out((G * gs['y_gs'],), torch.float32 if out_f32 else dtype), **gs)
            written = torch.zeros(G * gs['y_gs'], dtype=torch.bool)
            for g in range(G):
                written[g * gs['y_gs']:g * gs['y_gs'] + M * cout] = True
                got = y[g * gs['y_gs']:g * gs['y_gs'] + M * cout].reshape(M, cout)
                no_nan(got)
                e = rel_err(got.float().cpu().numpy(), probs[g][4].relu().numpy())
                print('A8 lp tile %d %s group %d f32 %d: %.3g' % (tile, dtype, g, out_f32, e))
                worst[out_f32] = max(worst[out_f32], e)
                if not e < _lp_bar(dtype, out_f32):
                    bad.append(('group', g, out_f32, e))
            if not untouched(y, written):
                bad.append(('a gap of y was written', out_f32))
    for out_f32, e in worst.items():
        report('E8', 'lp tile %d (%d x %d) %s %s' % (tile, bm, bn, dtype, 'f32' if out_f32 else 'lp'), e)
    assert not bad, bad


LP_REJECTED = [dict(y_coff=8), dict(y_cstride=128), dict(res_cstride=128), dict(res_coff=8), dict(act=CONF, act2=RELU, act_split=12)]
LP_ACCEPTED = [dict(act=RELU, act2=RELU, act_split=12), dict(act=CONF, act2=RELU, act_split=64), dict(act=CONF, act2=RELU, act_split=100)]


def test_lp_launcher_rejects_what_it_does_not_support():
    """A9.  usot_conv2d_lp stores a dense [M][Cout] map and picks the activation per 8 channels: a channel slice on either side, or
    a split inside a group of 8, is USOT_EINVAL with y untouched - never a dense map in the wrong place with USOT_OK.  Every buffer
    holds BOTH readings of the descriptor (the sliced one and the dense one), so ignoring a field stays inside the allocation."""
    M, cout = 33, 64
    x, w, b, _, pre = _lp_problem(M, 64, cout, torch.bfloat16, 9900, 3.0)
    wide = torch.randn(M, 2 * cout + 8, generator=torch.Generator().manual_seed(1)).bfloat16()      # a residual map for either reading
    missed, wrong = [], []
    with contract() as c:
        xd, wd, bd, rd = c.puts(x, w, b, wide)
        for fields in LP_REJECTED:
            y = c.out((M, 2 * cout + 8), torch.bfloat16)
            d = hip.conv_desc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N=1, H=1, W=M, Cin=64, OH=1, OW=M, Cout=cout, KH=1, KW=1,
                              res=rd.data_ptr() if any(k.startswith('res') for k in fields) else None, **fields)
            rc = int(hip.lib().usot_conv2d_lp(hip.stream(), C.byref(d), 0, 0))
            kept = untouched(y, torch.zeros(y.shape, dtype=torch.bool))
            print('A9 %s: status %d, y untouched: %s' % (fields, rc, kept))
            if rc != EINVAL or not kept:
                missed.append((fields, rc, kept))
        for fields in LP_ACCEPTED:
            y = _lp(c, 0, xd, wd, bd, M=M, Cin=64, Cout=cout, **fields)
            e = seg_err(y.float().cpu().numpy(), split_act_ref(pre, fields['act'], fields['act2'], fields['act_split']).numpy(), fields['act_split'])
            print('A9 %s: accepted, %.3g' % (fields, e))
            if not e < BAR16[torch.bfloat16]:
                wrong.append((fields, e))
    assert not missed and not wrong, (missed, wrong)
