"""CPU: the case lists of tests/test_gpu_tile_edges.py still reach every edge they exist for - the cap that keeps a later edit
from thinning the sweep into nothing.  The conv tiles' sizes come from the in-tree library, queried host-side (nothing is
launched); those checks skip when the library has not been built."""
import ctypes as C

import pytest

import conftest
import test_gpu_tile_edges as te


def test_pointwise_m_list_holds_every_residue_at_zero_one_and_two_full_tiles():
    ms = set(te.PW_M)
    for full in (0, 1, 2):
        for r in range(16):
            if 16 * full + r > 0:
                assert 16 * full + r in ms, (full, r)
    assert {47, 48, 49} <= ms and min(ms) == 1                       # the 2 -> 3 tile boundary
    assert set(te.DEFER_M) >= {1, 15, 16, 17, 32, 33}
    assert max(te.PW_M) <= 1200                                      # slices(M, ..) is constant over the list: prefix bit-equality holds
    assert len(te.PAIR_SHAPES) == 5 and set(te.PAIR_SLICED) <= set(te.PAIR_SHAPES) and len(te.SINGLE_SHAPES) == 4
    forms = set(te.PAIR_FORMS)
    assert {(s, 'default') for s in te.PAIR_SHAPES} <= forms and ((128, 512, 128), 'unsliced') in forms and ((256, 1024, 256), 'split16') in forms
    assert len(te.STREAM_SHAPES) == 2 and len(te.TRIPLE_SHAPES) == 3


def test_small_geometry_grid_reaches_every_residue_and_a_three_image_tile():
    ms = [nb * h * w for nb, h, w in te.GRID]
    assert {m % 16 for m in ms} == set(range(16))
    assert any(m < 16 for m in ms) and any(m % 16 == 0 for m in ms)
    assert any(nb == 3 and h * w <= 5 for nb, h, w in te.GRID)        # one 16-pixel tile spans three images
    assert any(w == 1 for _, _, w in te.GRID) and any(h == 1 for _, h, _ in te.GRID)          # shorter than the dilation
    assert len(te.GRID) == 3 * 4 * 9


def test_conv_tile_lists_hold_the_edges_of_every_routed_tile():
    L = conftest._lib()
    if L is None:
        pytest.skip('libusot_hip.so has not been built')
    tiles = te.sweep_tiles()
    built = [t for t in range(1, L.usot_conv_tile_count() + 1) if L.usot_conv_tile_built(t)]
    assert tiles and (L.usot_experiments_built() or tiles == built)  # the default build: every tile it holds
    assert [p.values[0] for p in te.TILES] == tiles
    for t in tiles:
        bm, bn = C.c_int(), C.c_int()
        assert L.usot_conv_tile_info(t, C.byref(bm), C.byref(bn)) == 0
        bm, bn = bm.value, bn.value
        assert bm % 16 == 0 and bn % 32 == 0, (t, bm, bn)
        ms, cs = te.b1_m_list(bm), te.b2_cout_list(bn)
        assert {1, 2, 3, 15, 16, 17, bm - 1, bm, bm + 1, 2 * bm - 1, 2 * bm, 2 * bm + 1} <= set(ms), (t, ms)
        assert {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, bn - 1, bn, bn + 1, 2 * bn - 4, 2 * bn + 1} <= set(cs), (t, cs)
        assert set(te.b3_cases(bm, bn)) >= {(bm - 1, bn + 1), (bm + 1, 4), (17, 33), (2 * bm, bn)}
