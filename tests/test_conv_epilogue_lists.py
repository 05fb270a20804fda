"""CPU: the case lists of tests/test_gpu_conv_epilogue.py still reach every edge they exist for, and its split-activation
reference is the header's definition.  Tile sizes come from the in-tree library, queried host-side (nothing is launched);
those checks skip when the library has not been built."""
import ctypes as C
import math

import pytest
import torch

import conftest
import test_gpu_conv_epilogue as ce


def test_act_split_list_holds_every_residue_and_the_tile_edge():
    assert set(ce.PAIRS) == {(ce.CONF, ce.RELU), (ce.RELU, ce.NONE), (ce.NONE, ce.EXP)} and ce.PAIRS[0] == (ce.CONF, ce.RELU)
    for bn in (32, 64, 128, 256):
        (cv, pv), (cs, ps) = ce.a1_couts(bn)
        assert (cv, pv, cs, ps) == (bn + 8, 'vector', bn + 7, 'scalar')
        for cout in (cv, cs):
            sp = ce.a1_splits(bn, cout)
            assert set(range(1, 9)) <= set(sp) and {bn - 1, bn, bn + 1, cout - 1} <= set(sp)
            assert {s % 4 for s in sp} == {0, 1, 2, 3} and all(0 < s < cout for s in sp)
        # the store path of each case by the documented rule: an unaligned split leaves the 16-byte epilogue, an aligned one keeps it
        for act, act2 in ce.PAIRS:
            assert all(ce.takes_vector_store(cv, act, act2, s) == (s % 4 == 0) for s in ce.a1_splits(bn, cv))
            assert not any(ce.takes_vector_store(cs, act, act2, s) for s in ce.a1_splits(bn, cs))
    assert ce.takes_vector_store(512, ce.CONF, ce.RELU, 256)                          # the frame's only split
    assert ce.takes_vector_store(72, ce.RELU, ce.RELU, 5)


def test_slice_lists_cover_the_vector_and_the_scalar_stores():
    for bn in (32, 64, 128, 256):
        cases = ce.a2_cases(bn)
        assert {(bn, bn + 4, 4), (bn, 2 * bn, bn), (bn + 4, 2 * bn + 8, bn + 4), (bn, bn + 3, 1), (bn - 1, 2 * bn, bn)} == {k[:3] for k in cases}
        for cout, cs, coff, path in cases:
            assert coff + cout <= cs and cs > cout                                    # a slice, inside its map, with columns left over
            assert ce.takes_vector_store(cout, y_cstride=cs, y_coff=coff) == (path == 'vector'), (cout, cs, coff)
        assert sum(k[3] == 'vector' for k in cases) == 3 and sum(k[3] == 'scalar' for k in cases) == 2
        cout = bn + 4
        rc = ce.a3_cases(cout)
        assert set(rc) == {(cout + 4, 4), (2 * cout, cout), (cout + 3, 1)} and all(o + cout <= s for s, o in rc)
        assert [ce.takes_vector_store(cout, res=True, res_cstride=s, res_coff=o) for s, o in rc] == [True, True, False]
    forms = ce.a5_forms(17, 36)
    assert set(forms) == {'vector', 'scalar', 'nchw'}
    for name, (gap, nchw) in forms.items():
        assert all(v > 0 for v in gap.values()) and gap['x'] % 4 == 0 and gap['w'] % 4 == 0         # x_gs / w_gs must keep 16 bytes
        odd = [gap[k] % 2 == 1 for k in ('b', 'y', 'r')]
        assert all(odd) if name == 'scalar' else not any(odd) and all(gap[k] % 4 == 0 for k in ('b', 'y', 'r'))
        assert nchw == (name == 'nchw')


def test_low_precision_lists_hold_both_cout_classes_around_the_tile_edge():
    for bn in (64, 128, 256):
        cs = ce.a6_couts(bn)
        assert {4, 8, 12, 60, 68, bn - 4, bn, bn + 4, bn + 8, bn + 12} == set(cs) and all(c % 4 == 0 for c in cs)
        for cls in (0, 4):                                           # Cout % 8 == 0: LDS epilogue; == 4: piece epilogue (16-bit output)
            assert any(c % 8 == cls and c < bn for c in cs) and any(c % 8 == cls and c > bn for c in cs), (bn, cls)
        assert 4 in cs                                               # a tile with one live 4-channel piece
        assert ce.a8_splits(bn) == [8, bn - 8, bn, bn + 8] and all(s % 8 == 0 and 0 < s < bn + 16 for s in ce.a8_splits(bn))
    for bm in (32, 64, 128, 256):
        assert ce.a7_m_list(bm) == [1, 2, bm - 1, bm, bm + 1, 2 * bm + 1]
    assert ce.LP_FORMS == ['lp', 'lp_res_relu', 'f32']
    keys = [tuple(sorted(d)) for d in ce.LP_REJECTED]
    assert keys == [('y_coff',), ('y_cstride',), ('res_cstride',), ('res_coff',), ('act', 'act2', 'act_split')]
    assert ce.LP_REJECTED[4]['act_split'] == 12 and ce.LP_REJECTED[4]['act'] != ce.LP_REJECTED[4]['act2']
    assert ce.LP_REJECTED[1]['y_cstride'] == 2 * 64 and ce.LP_REJECTED[2]['res_cstride'] == 2 * 64          # 2 Cout of the A9 problem
    assert [(d['act'] == d['act2'], d['act_split']) for d in ce.LP_ACCEPTED] == [(True, 12), (False, 64), (False, 100)]


def test_low_precision_sweep_runs_every_built_tile():
    L = conftest._lib()
    if L is None:
        pytest.skip('libusot_hip.so has not been built')
    ids = ce.lp_tile_ids()
    assert ids == list(range(1, L.usot_conv_bf16_tile_count() + 1)) and [p.values[0] for p in ce.LP_TILES] == ids
    built = [t for t in ids if L.usot_conv_bf16_tile_built(t)]
    assert L.usot_experiments_built() or built == ce.LP_ROUTED
    unmarked = [p.values[0] for p in ce.LP_TILES if not p.marks]
    assert unmarked == built                                          # every built tile runs; the others carry `experiments`
    L.usot_conv_bf16_tile_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for t in built:
        bm, bn = C.c_int(), C.c_int()
        assert L.usot_conv_bf16_tile_info(t, C.byref(bm), C.byref(bn)) == 0
        assert bm.value in (32, 64, 128, 256) and bn.value in (64, 128, 256), (t, bm.value, bn.value)
    assert L.usot_conv_bf16_tile_info(0, None, None) == -1 and L.usot_conv_bf16_tile_info(len(ids) + 1, None, None) == -1
    assert [p.values[0] for p in ce.TILES] == ce.sweep_tiles()


def test_split_activation_reference_on_a_hand_written_case():
    """eight channels, one row of pre-activations that visits every branch: below 0, inside (0, 4), above 4"""
    pre = torch.tensor([[-2.0, 0.5, 5.0, -0.25, 3.0, 4.5, -1.0, 2.0]], dtype=torch.float64)
    e = math.exp
    got = ce.split_act_ref(pre, ce.CONF, ce.RELU, 3)
    assert got.tolist() == [[1.0, e(0.5), e(4.0), 0.0, 3.0, 4.5, 0.0, 2.0]]
    got = ce.split_act_ref(pre, ce.RELU, ce.NONE, 5)
    assert got.tolist() == [[0.0, 0.5, 5.0, 0.0, 3.0, 4.5, -1.0, 2.0]]
    got = ce.split_act_ref(pre, ce.NONE, ce.EXP, 7)
    assert got.tolist() == [[-2.0, 0.5, 5.0, -0.25, 3.0, 4.5, -1.0, e(2.0)]]
    for split in (0, 8, 9, -1):                                      # act everywhere
        assert ce.split_act_ref(pre, ce.CONF, ce.RELU, split).tolist() == [[1.0, e(0.5), e(4.0), 1.0, e(3.0), e(4.0), 1.0, e(2.0)]]
    assert ce.split_act_ref(pre, ce.EXP, ce.NONE, 1).tolist() == [[e(-2.0)] + pre[0, 1:].tolist()]
    # seg_err: a wrong value in the small half is not hidden by the large half's floor
    ref = ce.split_act_ref(pre.repeat(4, 1) * 2, ce.CONF, ce.RELU, 3).numpy()
    bad = ref.copy()
    bad[0, 4] += 1e-3
    assert ce.seg_err(ref, ref, 3) == 0.0 and ce.seg_err(bad, ref, 3) > 1e-4
