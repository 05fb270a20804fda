"""CPU: the lists of tests/conv_gather_cases.py are the ones the gather sweep was specified with, their integer operands keep
every fp32 partial sum exact, and the float64 reference can tell a wrong tap from a right one - the cap that keeps a later edit
from thinning tests/test_gpu_conv_gather.py into something a wrong gather would pass.  Tile sizes come from the in-tree library,
queried host-side (nothing is launched); those checks skip when the library has not been built."""
import ast

import pytest
import torch
import torch.nn.functional as F

import conftest
import conv_gather_cases as gc
import test_gpu_conv_gather as tg
from usot_amd import hip

SPEC = """
(1,5,9,1,3,1,(0,1),(1,1))   (1,9,5,3,1,1,(1,0),(1,1))   (2,6,7,2,2,1,(0,0),(1,1))   (1,6,7,2,2,2,(1,1),(1,1))
(1,9,8,5,5,1,(2,2),(1,1))   (2,7,9,3,5,1,(0,2),(1,1))   (1,7,7,7,7,1,(0,0),(1,1))   (1,4,4,7,7,1,(3,3),(1,1))
(2,7,6,3,3,1,(0,2),(1,1))   (2,6,7,3,3,1,(2,0),(1,1))   (1,5,6,3,3,1,(3,3),(1,1))
(2,8,10,3,3,2,(1,1),(1,1))  (2,9,7,3,3,2,(1,1),(1,1))   (3,8,9,1,1,2,(0,0),(1,1))   (1,10,11,3,3,3,(1,0),(1,1))  (1,9,9,1,1,3,(1,1),(1,1))
(1,9,10,3,3,1,(3,3),(3,3))  (1,11,9,3,3,1,(0,0),(3,1))  (2,9,11,3,3,2,(2,2),(2,2))  (1,7,8,3,3,2,(1,2),(1,2))   (1,3,3,3,3,1,(4,4),(4,4))
(3,5,7,3,3,1,(1,1),(1,1))   (1,3,9,3,3,1,(0,1),(1,1))   (1,9,3,3,3,1,(1,0),(1,1))   (2,2,2,3,3,1,(1,1),(1,1))    (1,1,1,1,1,1,(0,0),(1,1))   (4,1,1,3,3,1,(1,1),(1,1))
"""
BMS, BKS = (16, 32, 64, 128), (32, 64)              # every tile shape of csrc/conv_igemm.hip's table that the sweep reaches


def _all_problems():
    """(geometry, Cin, Cout) of every problem of parts G, K and S at every tile shape"""
    out = [(g, gc.CIN, gc.COUT) for g in gc.GEOMS]
    for bk in BKS:
        out += [p[:3] for p in gc.k_problems(bk)]
        for bm in BMS:
            out += [p[1:4] for p in gc.s_problems(bm, bk)]
    out += [p[:3] for p in gc.k3_problems()]
    return sorted(set(out))


def test_the_lists_are_the_specified_ones():
    want = [ast.literal_eval(t) for t in SPEC.split()]
    assert gc.GEOMS == want and len(want) == 27
    for g in gc.GEOMS:
        assert gc.valid(g) and gc.pixels(g) <= 105, g
    assert (gc.CIN, gc.COUT) == (64, 32)
    assert gc.BATCH_ROWS == [(5, 1), (12, 2), (17, 1), (19, 3)]
    assert gc.K1_J == list(range(1, 13)) and gc.K2_CCH == [1, 3]
    assert gc.S1_KSPLIT == [2, 4, 5, 7, 13, 26, 27] and gc.S1_REJECTED == 28 and gc.S2_KSPLIT == [2, 3, 4, 5] and gc.S2_J == 5
    assert gc.WGRAD_PSPLIT == [1, 0, 3]
    assert (gc.X_MAX, gc.W_MAX, gc.B_MAX, gc.R_MAX, gc.DY_MAX) == (4, 2, 8, 8, 2)
    assert tg.G1_FORMS == ['plain', 'res_relu', 'nchw'] and tg.LP_FORMS == ['f32', 'lp', 'lp_res_relu']


def test_what_the_rows_cover():
    rows = gc.GEOMS
    assert any(g[3] != g[4] for g in rows) and any(g[3] % 2 == 0 for g in rows)                     # non-square, even kernels
    assert any(g[3] > g[1] and g[4] > g[2] for g in rows)                                           # a kernel larger than the image
    assert any(g[6][0] > g[6][1] for g in rows) and any(g[6][0] < g[6][1] for g in rows)            # pad_h != pad_w, both ways
    assert gc.padding_only_pixels(gc.row_of(11)) == 34                                              # padding beyond the kernel's reach
    for s in (2, 3):                                                                                # strides with padding; 1x1 strided
        assert any(g[5] == s and max(g[6]) > 0 and g[3] > 1 for g in rows) and any(g[5] == s and g[3] == g[4] == 1 for g in rows)
    assert any(g[5] == 2 and g[1] % 2 == 0 for g in rows) and any(g[5] == 2 and g[1] % 2 == 1 for g in rows)
    assert any(g[7][0] != g[7][1] for g in rows) and any(g[5] > 1 and max(g[7]) > 1 for g in rows) and any(max(g[7]) >= 4 for g in rows)
    assert any(g[0] == 3 and gc.pixels(g) == 105 for g in rows)                                     # 35 pixels an image, three images
    assert any(gc.out_hw(g)[0] == 1 and gc.out_hw(g)[1] > 1 for g in rows) and any(gc.out_hw(g)[1] == 1 and gc.out_hw(g)[0] > 1 for g in rows)
    assert any(g[2] < g[4] for g in rows) and any(g[0] == 4 and g[1] == g[2] == 1 for g in rows)
    closed = [i + 1 for i, g in enumerate(rows) if not gc.route_a_open(g)]
    assert closed == gc.ROUTE_A_CLOSED and {11, 16} <= set(closed)
    assert set(closed) - {11, 16} == {i + 1 for i, g in enumerate(rows) if g[5] > 1} - {16}


def test_every_partial_sum_is_an_exact_integer():
    probs = _all_problems()
    assert max(g[3] * g[4] * cin for g, cin, _ in probs if g not in gc.GEOMS) == 1728              # parts K and S: 27 k-tiles of 64
    assert max(g[3] * g[4] * cin for g, cin, _ in probs) == 7 * 7 * 64                             # part G: the 7x7 rows
    assert 7 * 7 * 64 * gc.X_MAX * hip.SPLIT16_X_SCALE * 512 < gc.EXACT * hip.SPLIT16_X_SCALE * 256      # split-fp16: sums of multiples of 8 x 256
    for g, cin, cout in probs:
        assert gc.valid(g) and gc.pixels(g) <= 129 and cin % 32 == 0, (g, cin, cout)
        assert gc.bound(g, cin, cout) < gc.EXACT, (g, cin, cout)
        x, w, b, res, dy = gc.operands(g, cin, cout)
        for t, amax in ((x, gc.X_MAX), (w, gc.W_MAX), (b, gc.B_MAX), (res, gc.R_MAX), (dy, gc.DY_MAX)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= amax
            assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)       # exact in both storage types
        assert float(x.abs().max()) == gc.X_MAX and float(w.abs().max()) == gc.W_MAX               # the ranges are used, not just allowed


def test_float32_reproduces_float64_on_every_row():
    worst = 0.0
    for g in gc.GEOMS:
        (x, w, b, res, dy), y64 = gc.problem(g)
        y32 = F.conv2d(x, w, b, g[5], g[6], g[7])
        assert torch.equal(y32.double(), y64), g
        assert torch.equal(y64, y64.round())
        worst = max(worst, float(y64.abs().max()))
    assert worst < 1024                                   # 16-bit outputs: the exact integers stay far inside fp16's range


def test_split_fp16_banks_carry_these_weights_in_their_hi_halves():
    """hip.split16_pack on every bank with whole 64-wide k-tiles: the lo halves are zero, the hi halves multiples of 256 below
    1 024, and hi x the row factor x 8 gives the weight back - so the split-fp16 tiles owe the same equality as the exact ones"""
    seen = 0
    for g, cin, cout in _all_problems():
        if cin % 64:
            continue
        w = gc.pack(gc.operands(g, cin, cout)[1])
        packed, scale = hip.split16_pack(w)
        halves = packed.view(torch.float16).view(cout, w.shape[1] // 64, 128)
        hi, lo = halves[:, :, :64].float(), halves[:, :, 64:]
        assert not bool(lo.view(torch.int16).any()), (g, cin, cout)
        assert torch.equal(hi % 256, torch.zeros_like(hi)) and float(hi.abs().max()) < 1024
        assert torch.equal(hi.reshape(cout, -1) * scale[:, None] * hip.SPLIT16_X_SCALE, w)
        seen += 1
    assert seen >= len(gc.GEOMS)
    x8 = torch.arange(-gc.X_MAX, gc.X_MAX + 1).float() * hip.SPLIT16_X_SCALE
    assert torch.equal(x8.half().float(), x8)             # the activations' hi halves are exact as well


def test_every_tap_is_seen_by_the_reference():
    """zeroing the weights of one tap changes the reference wherever that tap ever lands inside the image; the taps that never
    do are exactly the eight outer taps of rows 21 and 27"""
    dead = []
    for g in gc.GEOMS:
        (x, w, b, _, _), y64 = gc.problem(g)
        for kh in range(g[3]):
            for kw in range(g[4]):
                w0 = w.clone()
                w0[:, :, kh, kw] = 0
                changed = not torch.equal(gc.conv64(x, w0, b, g), y64)
                assert changed == gc.tap_lands(g, kh, kw), (g, kh, kw)
                if not changed:
                    dead.append((gc.GEOMS.index(g) + 1, kh, kw))
    assert gc.ONLY_CENTRE_TAP == [21, 27]
    assert sorted(dead) == sorted((r, kh, kw) for r in gc.ONLY_CENTRE_TAP for kh in range(3) for kw in range(3) if (kh, kw) != (1, 1))


def test_swapped_padding_and_dilation_change_the_reference():
    """a gather over the row's own output pixels that reads pad_w for pad_h (or dil_w for dil_h) and the reverse - the launchers
    check OH / OW, so a swap inside a kernel keeps the output's shape - differs from the reference on every row where the two
    differ; no row's output shape survives the swap in the DESCRIPTOR, where the launchers' OH / OW check would catch it"""
    seen = {'pad': [], 'dil': []}
    for g in gc.GEOMS:
        (x, w, b, _, _), y64 = gc.problem(g)
        assert torch.equal(gc.gather64(x, w, b, g, g[6], g[7]), y64), g
        for name, pad, dil in (('pad', g[6][::-1], g[7]), ('dil', g[6], g[7][::-1])):
            if (pad, dil) == (g[6], g[7]):
                continue
            assert not torch.equal(gc.gather64(x, w, b, g, pad, dil), y64), (name, g)
            assert gc.out_hw(g[:6] + (pad, dil)) != gc.out_hw(g)
            seen[name].append(gc.GEOMS.index(g) + 1)
    assert seen == {'pad': [1, 2, 6, 9, 10, 15, 20, 23, 24], 'dil': [18, 20]}, seen


def test_sixteen_bit_bar_is_one_storage_ulp():
    for dtype, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        ref = torch.tensor([0.0, 1.0, -3.0, 255.0, 256.0, 257.0, -530.0, 1023.0]).double()
        assert bool(gc.within_one_ulp(ref.float().to(dtype), ref, dtype).all())                    # every rounding of the exact value
        ulp = gc.storage_ulp(ref, dtype)
        assert float(ulp[-1]) == 2.0 ** (9 - (bits - 1)) and float(ulp[1]) == 2.0 ** -(bits - 1)
        off = ref + 2 * ulp
        assert not bool(gc.within_one_ulp(off, ref, dtype)[1:].any())                              # two ulps off fails everywhere
        assert not bool(gc.within_one_ulp(torch.tensor([2.0 ** -20]), torch.zeros(1).double(), dtype).any())     # an exact 0 stays 0


def test_slices_reach_one_k_tile_mid_tap_and_odd_starts():
    cch = 3                                                                   # Cin = 3 bk: three k-tiles a tap
    for ks in gc.S1_KSPLIT:
        cut = gc.slices(27, ks)
        assert cut[0][0] == 0 and cut[-1][1] == 27 and all(a[1] == b[0] for a, b in zip(cut, cut[1:])) and all(b > a for a, b in cut)
    lens = {ks: sorted({b - a for a, b in gc.slices(27, ks)}) for ks in gc.S1_KSPLIT}
    assert lens[2] == [13, 14] and lens[27] == [1] and lens[26] == [1, 2] and lens[13] == [2, 3]
    assert any(a % cch for ks in gc.S1_KSPLIT for a, _ in gc.slices(27, ks))                        # a slice starts inside a tap
    assert any(a % 2 for ks in gc.S1_KSPLIT for a, _ in gc.slices(27, ks))                          # ... and at an odd k-tile
    assert any(len({b - a for a, b in gc.slices(gc.S2_J, ks)}) > 1 for ks in gc.S2_KSPLIT) and max(gc.S2_KSPLIT) == gc.S2_J
    assert max(gc.K1_J) > 5 + 4                                               # past the five-stage ring and its four-tile prefetch


def test_tile_names_carry_their_k_tile():
    assert gc.tile_bk('conv_igemm_f32<128,128>') == 32
    assert gc.tile_bk('conv_igemm_f32_v2<32,64,BK=64>') == 64 and gc.tile_bk('conv_igemm_f32_v3<32,32,BK=64,D=3,NPW=8,PF=4>') == 64
    assert gc.tile_bk('conv_igemm_f32_v2<16,64,64,2> ksw=2') == 64 and gc.tile_bk('conv_igemm_f32_v2<32,32,32,4> ksw=4') == 32


def test_every_gpu_item_iterates_a_non_empty_list():
    assert gc.GEOMS and gc.BATCH_ROWS and gc.WGRAD_PSPLIT and tg.G1_FORMS and tg.LP_FORMS
    for bk in BKS:
        assert len(gc.k_problems(bk)) == 14
        for bm in BMS:
            probs = gc.s_problems(bm, bk)
            assert len(probs) == 4 and all(p[5] for p in probs) and {p[3] for p in probs} == {32, 33}
    assert len(gc.k3_problems()) == 14
    assert any(not gc.route_a_open(g) for g in gc.GEOMS) and any(gc.route_a_open(g) for g in gc.GEOMS)
    L = conftest._lib()
    if L is None:
        pytest.skip('libusot_hip.so has not been built')
    tiles = tg.sweep_tiles()
    assert tiles and [p.values[0] for p in tg.TILES] == tiles and [p.values[0] for p in tg.TILES0] == [0] + tiles
    assert [p.values[0] for p in tg.LP_TILES] == tg.lp_tile_ids() and any(L.usot_conv_bf16_tile_built(t) for t in tg.lp_tile_ids())
    for t in tiles:
        bm, bn = hip.tile_table()[t]
        assert bm in BMS and gc.tile_bk(hip.tile_name(t)) in BKS, (t, bm, hip.tile_name(t))
