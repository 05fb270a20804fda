"""GPU: WHAT ENTERS THE SUM of a convolution - the third part of the conv launchers next to where the last tile ends
(tests/test_gpu_tile_edges.py) and what happens to a finished sum (tests/test_gpu_conv_epilogue.py): the im2col gather (stride,
pad_h / pad_w, dil_h / dil_w, KH / KW, H / W, image borders) and the walk over the k-tiles, including how split-K slices it.

  G   the 27 geometries of conv_gather_cases.GEOMS (Cin 64, Cout 32, M <= 105): G1 usot_conv2d_f32 on tile 0 and every swept
      tile, plain | residual + ReLU | NCHW; G2 one usot_conv2d_batch_f32 launch of four rows of different geometry, each with a
      ksplit of its own, bit-equal to the single launches; G3 usot_conv2d_lp on every built tile, bf16 and fp16, fp32 out | 16-bit
      out | 16-bit residual + ReLU; G4 usot_conv2d_wgrad_f32 (psplit 1, 0, 3) and usot_conv2d_dgrad_f32 (route 2 everywhere,
      routes 1 and 0 where route A is open, USOT_EINVAL with dx untouched where it is closed).
  K   every k-tile count from one to twelve (1x1, Cin = j bk), and 3x3 at Cin = bk and 3 bk (27 k-tiles, three chunks a tap: the
      tap and chunk counters wrap on a non-power of two); the tile's bk as the launcher enforces it.
  S   split-K at two output corners with ReLU: 27 k-tiles cut into 2 .. 27 slices (13 / 14 down to ONE k-tile, starting inside a
      tap and at odd k-tiles), 5 k-tiles into 2 .. 5; ksplit = K / bk + 1 rejected with y and the workspace untouched; every case
      launched twice on one workspace whose ticket words nobody touches in between.

Operands are integers (conv_gather_cases.py), so every comparison is EQUALITY with the float64 reference - the split-fp16 tiles
included, their range word staying 0 - and one storage ulp of the exact integer for 16-bit outputs.  Every launch follows
tests/test_gpu_memory_contract.py: inputs between NaNs and compared bit for bit afterwards, outputs and split-K slabs NaN-prefilled
between canaries, ticket words zero before and zero again after, no NaN in a result.

One item = one (tile, part); it loops over its list and reports every failing case, not the first one.  The lists are asserted by
tests/test_conv_gather_lists.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402
import conv_gather_cases as gc  # noqa: E402
from test_gpu_conv_epilogue import PREFILL32, lp_tile_ids, untouched  # noqa: E402
from test_gpu_memory_contract import contract, no_nan  # noqa: E402
from test_gpu_tile_edges import _conv, _conv_bank, _conv_setup, report, sweep_tiles  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
RELU, NONE = hip.ACT_RELU, hip.ACT_NONE
EINVAL = -1
G1_FORMS = ['plain', 'res_relu', 'nchw']
LP_FORMS = ['f32', 'lp', 'lp_res_relu']

TILES = conftest.tile_params(sweep_tiles())
TILES0 = conftest.tile_params([0] + sweep_tiles())
LP_TILES = conftest.tile_params(lp_tile_ids(), lp=True)
LP_DT = [pytest.param(torch.bfloat16, id='bf16'), pytest.param(torch.float16, id='fp16')]


def geo_kw(g):
    n, h, w, kh, kw, s, pad, dil = g
    return dict(KH=kh, KW=kw, stride=s, pad=pad, dil=dil)


def differing(got, ref):
    """elements of a device result that are not the float64 reference's (a NaN differs from everything)"""
    return int((got.detach().cpu().double() != ref).sum())


def done(part, what, launches, bad):
    report(part, '%s: %d launches' % (what, launches), len(bad), label='failing cases')
    assert not bad, bad


def fwd_refs(g, cin=gc.CIN, cout=gc.COUT):
    """-> operands and the float64 results NHWC: plain, residual + ReLU"""
    ops, y64 = gc.problem(g, cin, cout)
    return ops, gc.nhwc(y64), gc.nhwc((y64 + ops[3].double()).relu())


# ------------------------------------------------------------------------------------------------------- G. the geometry list
@pytest.mark.parametrize('tile', TILES0)
def test_g1_every_geometry_on_every_tile(tile):
    """G1.  usot_conv2d_f32, every row of GEOMS: plain, residual + ReLU, NCHW."""
    bad, n = [], 0
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        for g in gc.GEOMS:
            (x, w, b, res, _), plain, rr = fwd_refs(g)
            bank = _conv_bank(c, tile, gc.pack(w), b)
            xd, rd = c.puts(gc.nhwc(x), gc.nhwc(res))
            kw = dict(Cout=gc.COUT, ovf=ovf if bank[3] == 2 else None, **geo_kw(g))
            for form in G1_FORMS:
                n += 1
                try:
                    if form == 'plain':
                        k = differing(_conv(c, tile, xd, bank, **kw), plain)
                    elif form == 'res_relu':
                        k = differing(_conv(c, tile, xd, bank, res=rd, act=RELU, **kw), rr)
                    else:
                        k = differing(_conv(c, tile, xd, bank, y_nchw=True, **kw).permute(0, 2, 3, 1), plain)
                except (hip.HipError, AssertionError) as e:
                    bad.append((gc.row_id(g), form, str(e)))
                    continue
                if k:
                    bad.append((gc.row_id(g), form, '%d of %d elements differ' % (k, plain.numel())))
        if int(ovf.item()) != 0:
            bad.append('the split-fp16 range word was set')
    done('G1', 'tile %d' % tile, n, bad)


@pytest.mark.parametrize('tile', TILES0)
def test_g2_batch_of_four_geometries(tile):
    """G2.  One usot_conv2d_batch_f32 launch of rows 5, 12, 17 and 19 with ksplit 1, 2, 1, 3: every output bit-equal to its
    single launch, and right."""
    bad, n = [], 0
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        single, setups, refs = [], [], []
        for number, ks in gc.BATCH_ROWS:
            g = gc.row_of(number)
            (x, w, b, _, _), plain, _ = fwd_refs(g)
            bank = _conv_bank(c, tile, gc.pack(w), b)
            xd = c.put(gc.nhwc(x))
            kw = dict(Cout=gc.COUT, ksplit=ks, ovf=ovf if bank[3] == 2 else None, **geo_kw(g))
            single.append(_conv(c, tile, xd, bank, **kw))
            setups.append(_conv_setup(c, tile, xd, bank, **kw))
            refs.append(plain)
            n += 1
        arr = (hip.ConvDesc * len(setups))(*[s[0] for s in setups])
        hip.check(hip.lib().usot_conv2d_batch_f32(hip.stream(), arr, len(setups)), 'usot_conv2d_batch_f32 tile %d' % tile)
        n += 1
        for (number, ks), (d, y, ws, tick), one, ref in zip(gc.BATCH_ROWS, setups, single, refs):
            if bool(torch.isnan(y).any()):
                bad.append((number, ks, 'NaN in the batched output'))
            if ws is not None and bool(ws[tick:].view(torch.int32).any()):
                bad.append((number, ks, 'ticket words not zero after the launch'))
            if not torch.equal(y.view(torch.int32), one.view(torch.int32)):
                bad.append((number, ks, 'batched and single launch differ in %d elements' % int((y != one).sum())))
            if differing(y, ref) or differing(one, ref):
                bad.append((number, ks, 'batched %d, single %d of %d elements differ from float64' % (differing(y, ref), differing(one, ref), ref.numel())))
        if int(ovf.item()) != 0:
            bad.append('the split-fp16 range word was set')
    done('G2', 'tile %d' % tile, n, bad)


def _lp_geo(c, tile, xd, wd, bd, g, *, Cin, Cout, res=None, act=NONE, out_f32=False):
    """one usot_conv2d_lp launch of geometry g on operands of the storage type of xd"""
    n, h, w, kh, kw, s, pad, dil = g
    oh, ow = gc.out_hw(g)
    y = c.out((n, oh, ow, Cout), torch.float32 if out_f32 else xd.dtype)
    d = hip.conv_desc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N=n, H=h, W=w, Cin=Cin, OH=oh, OW=ow, Cout=Cout, KH=kh, KW=kw,
                      stride=s, pad=pad, dil=dil, res=res.data_ptr() if res is not None else None, act=act, tile=tile)
    hip.check(hip.lib().usot_conv2d_lp(hip.stream(), C.byref(d), 1 if xd.dtype == torch.float16 else 0, int(out_f32)),
              'usot_conv2d_lp tile %d' % tile)
    no_nan(y)
    return y


def _lp_forms(c, tile, dtype, g, cin, cout, forms, bad, tag):
    """the forms of one low-precision problem: fp32 output equal to float64, 16-bit outputs within one storage ulp of the exact integer"""
    (x, w, b, res, _), plain, rr = fwd_refs(g, cin, cout)
    xd, wd, bd, rd = c.puts(gc.nhwc(x).to(dtype), gc.pack(w).to(dtype), b, gc.nhwc(res).to(dtype))
    for form in forms:
        try:
            if form == 'f32':
                k = differing(_lp_geo(c, tile, xd, wd, bd, g, Cin=cin, Cout=cout, out_f32=True), plain)
            elif form == 'lp':
                k = int((~gc.within_one_ulp(_lp_geo(c, tile, xd, wd, bd, g, Cin=cin, Cout=cout).cpu(), plain, dtype)).sum())
            else:
                k = int((~gc.within_one_ulp(_lp_geo(c, tile, xd, wd, bd, g, Cin=cin, Cout=cout, res=rd, act=RELU).cpu(), rr, dtype)).sum())
        except (hip.HipError, AssertionError) as e:
            bad.append((tag, form, str(e)))
            continue
        if k:
            bad.append((tag, form, '%d of %d elements %s' % (k, plain.numel(), 'differ' if form == 'f32' else 'are more than one ulp off')))
    return len(forms)


@pytest.mark.parametrize('dtype', LP_DT)
@pytest.mark.parametrize('tile', LP_TILES)
def test_g3_every_geometry_low_precision(tile, dtype):
    """G3.  usot_conv2d_lp, every row of GEOMS: fp32 out, 16-bit out, 16-bit residual + ReLU."""
    bad, n = [], 0
    with contract() as c:
        for g in gc.GEOMS:
            n += _lp_forms(c, tile, dtype, g, gc.CIN, gc.COUT, LP_FORMS, bad, gc.row_id(g))
    done('G3', 'lp tile %d %s' % (tile, dtype), n, bad)


def _grad_geo(g):
    n, h, w, kh, kw, s, pad, dil = g
    return dict(N=n, H=h, W=w, Cin=gc.CIN, Cout=gc.COUT, KH=kh, KW=kw, stride=s, pad=pad, dil=dil)


def test_g4_weight_gradient_on_every_geometry():
    """G4.  usot_conv2d_wgrad_f32, every row: dw and db at psplit 1, 0 (the launcher's choice) and 3 (M >= 6), the workspace
    NaN-prefilled (its contents before the launch do not matter)."""
    L = hip.lib()
    bad, n = [], 0
    with contract() as c:
        for g in gc.GEOMS:
            x, w, b, _, dy = gc.problem(g)[0]
            _, rw, rb = gc.gradients(g)
            rw = gc.pack(rw)
            xd, dyd = c.puts(gc.nhwc(x), gc.nhwc(dy))
            for ps in gc.WGRAD_PSPLIT:
                if ps > 1 and gc.pixels(g) < 6:
                    continue
                n += 1
                d = hip.grad_desc(psplit=ps, **_grad_geo(g))
                need = int(L.usot_conv2d_wgrad_ws_floats(C.byref(d)))
                if need < 0 or (need > 0) != (int(L.usot_conv2d_wgrad_psplit(C.byref(d))) > 1):
                    bad.append((gc.row_id(g), ps, 'workspace query answered %d' % need))
                    continue
                dw, db = c.out(tuple(rw.shape)), c.out((gc.COUT,))
                ws = c.out((need,)) if need else None
                d.x, d.dy, d.dw, d.db, d.ws = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr() if need else None
                rc = int(L.usot_conv2d_wgrad_f32(hip.stream(), C.byref(d)))
                kw_, kb = differing(dw, rw), differing(db, rb)
                if rc != 0 or kw_ or kb:
                    bad.append((gc.row_id(g), ps, 'status %d, dw: %d of %d elements differ, db: %d of %d' % (rc, kw_, rw.numel(), kb, rb.numel())))
    done('G4', 'weight gradient', n, bad)


def test_g4_data_gradient_on_every_geometry():
    """G4.  usot_conv2d_dgrad_f32, every row: route 2; routes 1 and 0 on the bank usot_conv_pack_dgrad_f32 wrote where
    usot_conv2d_dgrad_route says route A is open - exactly the rows the documented rule opens - and, where it is closed,
    route 1 answers USOT_EINVAL with dx still holding its prefill."""
    L = hip.lib()
    bad, n = [], 0
    with contract() as c:
        for g in gc.GEOMS:
            number = gc.GEOMS.index(g) + 1
            n_, h, w_, kh, kw, s, pad, dil = g
            x, w, b, _, dy = gc.problem(g)[0]
            rx = gc.nhwc(gc.gradients(g)[0])
            wd, dyd = c.puts(gc.pack(w), gc.nhwc(dy))
            wt = c.out((gc.CIN, kh * kw * gc.COUT))
            hip.check(L.usot_conv_pack_dgrad_f32(hip.stream(), hip.ptr(wd), hip.ptr(wt), gc.COUT, gc.CIN, kh, kw), 'usot_conv_pack_dgrad_f32')
            n += 1
            rot = gc.pack(w.flip(2, 3).transpose(0, 1).contiguous())
            if not torch.equal(wt.cpu(), rot):
                bad.append((gc.row_id(g), 'rotated bank differs'))
            q = hip.grad_desc(route=0, dy=dyd.data_ptr(), w=wd.data_ptr(), wt=wt.data_ptr(), **_grad_geo(g))
            is_open = int(L.usot_conv2d_dgrad_route(C.byref(q))) == 1
            if is_open != gc.route_a_open(g) or is_open != (number not in gc.ROUTE_A_CLOSED):
                bad.append((gc.row_id(g), 'usot_conv2d_dgrad_route says route A is %s' % ('open' if is_open else 'closed')))
            for route in (2, 1, 0):
                if route == 0 and not is_open:
                    continue                                      # route 0 is route B there: the launch route = 2 made
                dx = c.out((n_, h, w_, gc.CIN))
                d = hip.grad_desc(route=route, dy=dyd.data_ptr(), w=wd.data_ptr(), wt=wt.data_ptr(), dx=dx.data_ptr(), **_grad_geo(g))
                rc = int(L.usot_conv2d_dgrad_f32(hip.stream(), C.byref(d)))
                n += 1
                if route == 1 and not is_open:
                    kept = untouched(dx, torch.zeros(dx.shape, dtype=torch.bool))
                    if rc != EINVAL or not kept:
                        bad.append((gc.row_id(g), route, 'closed route A: status %d, dx untouched: %s' % (rc, kept)))
                    continue
                k = differing(dx, rx)
                if rc != 0 or k:
                    bad.append((gc.row_id(g), route, 'status %d, %d of %d elements differ' % (rc, k, rx.numel())))
    done('G4', 'data gradient', n, bad)


# --------------------------------------------------------------------------------------------------------- K. the k-tile walk
@pytest.mark.parametrize('tile', TILES)
def test_k_every_k_tile_count(tile):
    """K1, K2.  M = 17, Cout = 32: 1x1 at Cin = j bk, j = 1 .. 12; 3x3, pad (0, 1), at Cin = bk and 3 bk.  The tile's bk, read from
    its name, is the one the launcher enforces: Cin = 32 is accepted exactly when bk == 32, Cin = 48 never, a rejected launch
    leaves y untouched."""
    L = hip.lib()
    bk = gc.tile_bk(hip.tile_name(tile))
    bad, n = [], 0
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        for g, cin, cout, kt in gc.k_problems(bk):
            (x, w, b, _, _), plain, _ = fwd_refs(g, cin, cout)
            assert g[3] * g[4] * cin == kt * bk
            n += 1
            try:
                bank = _conv_bank(c, tile, gc.pack(w), b)
                k = differing(_conv(c, tile, c.put(gc.nhwc(x)), bank, Cout=cout, ovf=ovf if bank[3] == 2 else None, **geo_kw(g)), plain)
            except (hip.HipError, AssertionError) as e:
                bad.append((gc.row_id(g), cin, str(e)))
                continue
            if k:
                bad.append((gc.row_id(g), cin, '%d k-tiles: %d of %d elements differ' % (kt, k, plain.numel())))
        # Cin = 32 (where bk is not 32) and Cin = 48 on buffers of a Cin = 64 problem: either reading of the descriptor stays inside them
        g = gc.pw_geom(17)
        (x, w, b, _, _), _, _ = fwd_refs(g, 64, gc.COUT)
        bank = _conv_bank(c, tile, gc.pack(w), b)
        xd = c.put(gc.nhwc(x))
        for cin in ([48] if bk == 32 else [32, 48]):
            y = c.out((1, 1, 17, gc.COUT))
            d = hip.conv_desc(xd.data_ptr(), bank[0].data_ptr(), bank[2].data_ptr(), y.data_ptr(), N=1, H=1, W=17, Cin=cin, OH=1, OW=17,
                              Cout=gc.COUT, KH=1, KW=1, tile=tile, w_frag=bank[3], w_scale=bank[1].data_ptr() if bank[1] is not None else None)
            rc = int(L.usot_conv2d_f32(hip.stream(), C.byref(d)))
            kept = untouched(y, torch.zeros(y.shape, dtype=torch.bool))
            if rc != EINVAL or not kept:
                bad.append(('Cin = %d with bk = %d' % (cin, bk), 'status %d, y untouched: %s' % (rc, kept)))
        if int(ovf.item()) != 0:
            bad.append('the split-fp16 range word was set')
    done('K1-K2', 'tile %d bk %d' % (tile, bk), n, bad)


@pytest.mark.parametrize('dtype', LP_DT)
@pytest.mark.parametrize('tile', LP_TILES)
def test_k3_every_k_tile_count_low_precision(tile, dtype):
    """K3.  usot_conv2d_lp on the shapes of K1 at Cin = 64 j, j = 1 .. 12, and of K2 at Cin = 64 and 192: fp32 and 16-bit output."""
    bad, n = [], 0
    with contract() as c:
        for g, cin, cout, kt in gc.k3_problems():
            n += _lp_forms(c, tile, dtype, g, cin, cout, LP_FORMS[:2], bad, '%s Cin %d' % (gc.row_id(g), cin))
    done('K3', 'lp tile %d %s' % (tile, dtype), n, bad)


# ------------------------------------------------------------------------------------------------- S. split-K distribution
def _launch(d, what):
    hip.check(hip.lib().usot_conv2d_f32(hip.stream(), C.byref(d)), what)


@pytest.mark.parametrize('tile', TILES)
def test_s_split_k_distribution(tile):
    """S1, S2.  (M, Cout) = (17, 33) and (bm + 1, 32), ReLU.  S1: 3x3 at Cin = 3 bk (27 k-tiles) with ksplit of S1_KSPLIT, and
    ksplit 28 rejected with y and the whole workspace untouched.  S2: 1x1 at Cin = 5 bk with ksplit 2 .. 5.  Every case runs
    twice on one workspace - the slabs refilled with the NaN pattern, the ticket words as the first launch left them."""
    L = hip.lib()
    bm, bn = hip.tile_table()[tile]
    bk = gc.tile_bk(hip.tile_name(tile))
    bad, n = [], 0
    with contract() as c:
        ovf = c.out((1,), torch.int32, 'zero')
        for part, g, cin, cout, kt, ksplits in gc.s_problems(bm, bk):
            (x, w, b, _, _), plain, _ = fwd_refs(g, cin, cout)
            want = plain.relu()
            assert g[3] * g[4] * cin == kt * bk
            bank = _conv_bank(c, tile, gc.pack(w), b)
            xd = c.put(gc.nhwc(x))
            kw = dict(Cout=cout, act=RELU, ovf=ovf if bank[3] == 2 else None, **geo_kw(g))
            for ks in ksplits:
                tag = (part, 'M %d Cout %d' % (gc.pixels(g), cout), 'ksplit %d' % ks)
                d, y1, ws, tick = _conv_setup(c, tile, xd, bank, ksplit=ks, **kw)
                n += 2
                try:
                    _launch(d, 'usot_conv2d_f32 tile %d %s' % (tile, tag,))
                    t1 = bool(ws[tick:].view(torch.int32).any())
                    ws[:tick].view(torch.int32).fill_(PREFILL32)
                    y2 = c.out(tuple(y1.shape))
                    d.y = y2.data_ptr()
                    _launch(d, 'usot_conv2d_f32 tile %d %s, second launch' % (tile, tag,))
                    t2 = bool(ws[tick:].view(torch.int32).any())
                except hip.HipError as e:
                    bad.append(tag + (str(e),))
                    continue
                k1, k2 = differing(y1, want), differing(y2, want)
                if k1 or k2 or t1 or t2 or not torch.equal(y1.view(torch.int32), y2.view(torch.int32)):
                    bad.append(tag + ('first launch: %d of %d elements differ, tickets left set: %s; second: %d, %s' % (k1, want.numel(), t1, k2, t2),))
            if part == 'S1':
                d, y, ws, tick = _conv_setup(c, tile, xd, bank, ksplit=gc.S1_REJECTED, **kw)
                rc = int(L.usot_conv2d_f32(hip.stream(), C.byref(d)))
                kept = (untouched(y, torch.zeros(y.shape, dtype=torch.bool)) and untouched(ws[:tick], torch.zeros(tick, dtype=torch.bool))
                        and not bool(ws[tick:].view(torch.int32).any()))
                if rc != EINVAL or not kept:
                    bad.append((part, 'M %d Cout %d' % (gc.pixels(g), cout), 'ksplit %d: status %d, y and workspace untouched: %s' % (gc.S1_REJECTED, rc, kept)))
        if int(ovf.item()) != 0:
            bad.append('the split-fp16 range word was set')
    done('S1-S2', 'tile %d (%d x %d) bk %d' % (tile, bm, bn, bk), n, bad)
