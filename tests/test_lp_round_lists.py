"""CPU: the shapes tests/test_gpu_lp_rounds.py derives from the CU count still do what they exist for - every base problem is one
round on the form of its big problem, every big problem reaches exactly the intended number of rounds and ends in a ragged unit.
The launchers' rules are restated here (grid = min(units, CUs) unless noted; csrc/pw_kstream.hip, pw_panel.hip, pw_pair.hip,
conv3x3_halo.hip, bneck_lp.hip); nothing is launched."""
import pytest
import torch

import test_gpu_lp_rounds as lr

CUS = [256, 304, 64]


def cdiv(a, b):
    return -(-a // b)


def rounds_of(units, G):
    return cdiv(units, min(units, G))


def panel_form(M, K):
    """usot_pw_panel_lp: pixels per panel"""
    if K == 64:
        return 512
    return 128 if cdiv(M, 256) < 192 else 256


def pointwise_ok(case, rounds, tail, bm):
    units = cdiv(case['M'], bm)
    assert rounds_of(units, case['G']) == rounds and units == (rounds - 1) * case['G'] + 2, (case, units)
    assert case['M'] % bm == tail and 0 < tail < bm                                  # the last unit is ragged ...
    assert tail % 16 != 0 and tail in (19, 37, 77)                                  # ... inside a 16-pixel block
    base_units = case['base_m'] // bm
    assert case['base_m'] % bm == 0 and 16 <= base_units <= case['G']               # the base: whole panels, one round
    assert rounds_of(base_units, case['G']) == 1


def all_cases(cus):
    """(name, case) of every shape the GPU file runs at `cus` CUs"""
    out = []
    for r in lr.ROUNDS:
        out.append(('kstream', r, lr.kstream_case(cus, r)))
        out.append(('panel_large', r, lr.panel_large_case(cus, r)))
        for s in lr.PANEL_PAIR_SHAPES:
            out.append(('panel_pair', r, lr.panel_pair_case(cus, s, r)))
        for H in lr.HALO_HS:
            out.append(('halo', r, lr.halo_case(cus, r, H)))
        out.append(('bneck', r, lr.bneck_case(cus, r)))
    out.append(('panel_small', 2, lr.panel_small_case(cus)))
    out.append(('panel_k64', 3, lr.panel_k64_case(cus)))
    for s in lr.PW_PAIR_SHAPES:
        out.append(('pw_pair', None, lr.pw_pair_case(cus, s)))
    return out


def test_no_case_skips_at_256_cus():
    assert [n for n, _, c in all_cases(256) if c['skip']] == []


@pytest.mark.parametrize('cus', CUS)
def test_a_skip_always_carries_its_reason(cus):
    for name, _, c in all_cases(cus):
        assert c['skip'] is None or (isinstance(c['skip'], str) and str(cus) in c['skip'] and len(c['skip']) > 20), (name, c)
    if cus == 304:                              # every case the launchers' rules allow runs there too
        assert [n for n, _, c in all_cases(cus) if c['skip']] == []
    if cus == 64:                               # 130 panels of 256 pixels never reach the large form; 72 halo tiles are two rounds
        assert {n for n, _, c in all_cases(cus) if c['skip']} == {'panel_large', 'halo'}


@pytest.mark.parametrize('cus', CUS)
def test_pointwise_shapes_reach_their_rounds_on_the_form_of_their_base(cus):
    for r in lr.ROUNDS:
        c = lr.kstream_case(cus, r)
        pointwise_ok(c, r, 37, 256)
        c = lr.panel_large_case(cus, r)
        if not c['skip']:
            pointwise_ok(c, r, lr.TAIL[r], 256)
            for K in (256, 128):
                assert panel_form(c['M'], K) == 256 and panel_form(c['base_m'], K) == 256
        else:
            assert cus < 192
        for s in lr.PANEL_PAIR_SHAPES:
            c = lr.panel_pair_case(cus, s, r)
            pointwise_ok(c, r, lr.TAIL[r], lr.PANEL_PAIR_PIXELS[s])
    c = lr.panel_small_case(cus)
    assert c['M'] == 128 * cus + 128 + 77
    if not c['skip']:
        pointwise_ok(c, 2, 77, 128)
        for K in (256, 128):
            assert panel_form(c['M'], K) == 128 and panel_form(c['base_m'], K) == 128
    else:
        assert cdiv(c['M'], 256) >= 192
    c = lr.panel_k64_case(cus)
    pointwise_ok(c, 3, 37, 512)
    assert panel_form(c['M'], 64) == 512 == panel_form(c['base_m'], 64)
    assert set(lr.TAIL.values()) == {19, 37}
    # the fused pair's three filter-bank shapes: >= 3 rounds at one and at two workgroups per CU, and a third use of the LDS image
    assert [lr.pw_pair_wgs_per_cu(cm, co) for cm, co, _ in lr.PW_PAIR_SHAPES] == [1, 1, 2]
    for s in lr.PW_PAIR_SHAPES:
        c = lr.pw_pair_case(cus, s)
        units = cdiv(c['M'], 64)
        assert units == 4 * cus + 2 and c['M'] % 64 == 37 and c['G'] in (cus, 2 * cus)
        assert rounds_of(units, c['G']) == (5 if c['G'] == cus else 3)
        assert c['base_m'] == 16 * 64 and rounds_of(16, c['G']) == 1


@pytest.mark.parametrize('cus', CUS)
def test_spatial_shapes_reach_their_rounds(cus):
    seen = set()
    for H in lr.HALO_HS:
        seen |= lr.halo_stores_prev(H)
        assert cdiv(H, 16) == 3 and cdiv(lr.HALO_W, 16) == 3
        for r in lr.ROUNDS:
            c = lr.halo_case(cus, r, H)
            assert c['tpi'] == 9 and c['ntiles'] == 9 * c['N'] and c['N'] == cdiv((r - 1) * cus + 2, 9)
            assert rounds_of(c['ntiles'], c['G']) == r, c
            assert c['base_n'] >= 8 and (c['skip'] or rounds_of(9 * c['base_n'], c['G']) == 1)
    assert seen == {0, 1, 2, 3, 4}                                                  # every counted wait of the halo kernel
    assert [H - 32 for H in lr.HALO_HS] == [1, 6, 11, 16]
    for r in lr.ROUNDS:
        c = lr.bneck_case(cus, r)
        G = cus & ~7
        assert c['G'] == G and c['tpi'] == 4 and c['ntiles'] == 4 * c['N']
        assert c['ntiles'] > (r - 1) * G and c['ntiles'] % 8 != 0
        grid = G if G <= c['ntiles'] else c['ntiles'] & ~7                           # the launcher's grid
        assert grid == G and cdiv(c['ntiles'], grid) == r
        base_tiles = 4 * c['base_n']
        assert base_tiles == 32 and (base_tiles & ~7) == base_tiles <= G            # the base: grid = 32, one tile per workgroup
        assert lr.BNECK_H % lr.BNECK_TH == 7 and lr.BNECK_W % lr.BNECK_TW == 15
        # the walk the reporter inverts covers every tile exactly once
        tiles = sorted((8 * k + (b & 7)) * (grid // 8) + (b >> 3) for k in range(r) for b in range(grid))
        assert tiles[:c['ntiles']] == list(range(c['ntiles']))
        for t in (0, 1, grid - 1, grid, c['ntiles'] - 1):
            k, b = lr.bneck_walk(t, grid)
            assert (8 * k + (b & 7)) * (grid // 8) + (b >> 3) == t and 0 <= b < grid


def test_indices_keep_the_position_in_the_unit_and_never_repeat_an_image():
    idx = lr.row_index(5 * 256 + 19, 256, 16, 3)
    assert torch.equal(idx % 256, torch.arange(idx.numel()) % 256) and int(idx.max()) < 16 * 256
    per_unit = (idx[:5 * 256] // 256).reshape(5, 256)
    assert all(torch.unique(u).numel() >= 12 for u in per_unit)                     # a unit mixes the base panels ...
    assert not torch.equal(per_unit[0], per_unit[1])                                # ... and no two units the same way
    assert torch.equal(idx, lr.row_index(5 * 256 + 19, 256, 16, 3))                 # seeded
    im = lr.image_index(131, 8, 5)
    assert bool((im[1:] != im[:-1]).all()) and set(im.tolist()) == set(range(8))
    period = [p for p in range(1, 66) if torch.equal(im[p:], im[:-p])]
    assert period == []


def test_conv_pw_sweep_reaches_every_panel_count():
    assert lr.conv_pw_panel_counts() >= set(range(1, 21))
    for cus in CUS:
        n = lr.automatic_form_images(cus, 12)
        n256 = cdiv(n * 144, 256)
        assert n256 == cus + 1 and (n256 < 192 or (n256 > cus and 2 * n256 < 3 * cus))   # usot_conv_pw_pixels: the 128-pixel form


def test_mismatch_reporter_names_unit_round_workgroup_and_row():
    G, bm = 256, 256
    want = torch.arange(600 * bm * 4, dtype=torch.int32).reshape(600 * bm, 4).to(torch.bfloat16)
    assert lr.mismatch(want.clone(), want, lr.rows_locator(bm), G) is None
    got = want.clone()
    bits = got.view(torch.int16)
    bits[(2 * G + 5) * bm + 17, 3] ^= 1                                             # third round, workgroup 5, row 17: one last bit
    bits[(2 * G + 9) * bm + 2, 0] ^= 1
    bits[(2 * G + 9) * bm + 2, 1] ^= 1
    msg = lr.mismatch(got, want, lr.rows_locator(bm), G, what='y')
    assert msg.startswith('y: 3 wrong elements in 2 rows of 2 units')
    assert 'first wrong unit 517 (round 2, workgroup 5), row 17 of the unit' in msg
    # a spatial map: pixel (y = 9, x = 20) of image 70 of 15 x 31 is row 1 * 16 + 4 of tile 70 * 4 + 3; walk of a grid of 256 blocks
    H, W = lr.BNECK_H, lr.BNECK_W
    want = torch.zeros(80 * H * W, 8, dtype=torch.float16)
    got = want.clone()
    got[(70 * H + 9) * W + 20, 5] = 1.0
    got[(70 * H + 14) * W + 30, 5] = 1.0                                            # same tile, a later row: not the first
    msg = lr.mismatch(got, want, lr.tiles_locator(H, W, lr.BNECK_TH, lr.BNECK_TW), 256, lr.bneck_walk, 't')
    k, b = lr.bneck_walk(283, 256)
    assert (k, b) == (1, 27 * 8 + 0) and (8 * k + (b & 7)) * 32 + (b >> 3) == 283
    assert 't: 2 wrong elements in 2 rows of 1 units; first wrong unit 283 (round 1, workgroup 216), row 20 of the unit' == msg
    # a NaN that is bit-equal on both sides is not a mismatch; another NaN pattern is
    a = torch.tensor([[float('nan'), 1.0]], dtype=torch.bfloat16)
    assert lr.mismatch(a.clone(), a, lr.rows_locator(1), 4) is None
    b2 = a.clone()
    b2.view(torch.int16)[0, 0] ^= 1
    assert 'first wrong unit 0 (round 0, workgroup 0), row 0' in lr.mismatch(b2, a, lr.rows_locator(1), 4)
