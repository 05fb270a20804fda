"""CPU: the lists of tests/lp_spatial_cases.py still do what they exist for.  Nothing is launched.

  * the lists are pinned: counts and named members;
  * every (case, storage type, stage) is exact in fp32 in ANY summation order: sum |addends| < 2^24 granules;
  * the operands cannot hide a defect: every k index of every bank is live, b1 > 0, a share of every stage's values is changed by
    the rounding, neighbouring pixels / rows / images differ;
  * every reference mutation changes the expected bits wherever meaningful() says the geometry lets it, and is meaningful somewhere
    in every list it applies to;
  * the shape choosers agree with the launchers' rules (restated here from csrc/conv3x3_halo.hip, bneck_lp.hip, conv_kstream.hip,
    conv_pw_lp.hip): tiles per image, grid = ntiles - (ntiles & 7), PERK, the row-shared predicate of cp_fill;
  * the parked-tap address model of usot_conv_kstream_lp stays inside x for every case the sweep launches, leaves it for every
    geometry of the refusal list, and the launcher's rule N H W > dil (W + 1) is what separates the two."""
import os
import re

import pytest
import torch

import lp_spatial_cases as lc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'usot_amd', 'csrc')

LISTS = {'halo': lc.halo_cases(), 'kstream': lc.kstream_cases(), 'convpw_pertap': lc.convpw_pertap_cases(),
         'convpw_rowshared': lc.convpw_rowshared_cases()}
for _kind, _cn in lc.BNECK_FAMILIES:
    LISTS['bneck_%s_%d' % (_kind, _cn)] = lc.bneck_cases(_kind, _cn)
NAMES = sorted(LISTS)
MIN_ROUNDED = 0.03          # of a stage's values over a list: thousands of elements a kernel that forgot the rounding gets wrong


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    return int(re.search(r'constexpr int [^;]*\b%s = (\d+)' % name, text).group(1))


# ------------------------------------------------------------------------------------------------------------------ the lists
def test_the_lists_are_pinned():
    assert {n: len(v) for n, v in LISTS.items()} == {'halo': 75, 'kstream': 80, 'convpw_pertap': 29, 'convpw_rowshared': 85,
                                                     'bneck_first_64': 57, 'bneck_tail_64': 57, 'bneck_tail_128': 57}
    for v in LISTS.values():
        assert len(set(v)) == len(v)
    halo = LISTS['halo']
    assert {(c.H, c.W) for c in halo if c.N == 1} >= {(h, 17) for h in range(1, 34)} | {(5, w) for w in range(1, 34)}
    assert {(c.H, c.W) for c in halo if c.N == 2} >= set(lc.CORNERS)
    assert {c.act for c in halo} == {0, 1} and sum(not c.bias for c in halo) == 1
    assert lc.Halo(lc.HALO_MANY_TILES, 3, 2, 1, True) in halo and lc.HALO_MANY_TILES > 512       # more tiles than CUs on any device
    for kind, cn in lc.BNECK_FAMILIES:
        b = LISTS['bneck_%s_%d' % (kind, cn)]
        assert {(c.H, c.W) for c in b} >= {(h, 17) for h in range(1, 18)} | {(9, w) for w in range(1, 34)} | set(lc.CORNERS)
        assert lc.Bneck(kind, 11, 7, 13, cn) in b and lc.Bneck(kind, 1, 33, 33, cn) in b
    ks = LISTS['kstream']
    assert {(c.stride, c.dil, c.pad) for c in ks} == {(s, d, p) for s in (1, 2) for d in (1, 2, 3) for p in range(d + 1)}
    assert {(c.H, c.W) for c in ks} >= {(1, 1), (7, 9), (9, 7), (5, 23)}
    assert {lc.pixels(c) for c in ks} >= {255, 256, 257, 511, 513}
    assert {c.Cin for c in ks} == {256, 512} and {c.Cout for c in ks} == {256, 512, 768, 1024}
    assert sum(c.Cout == 768 for c in ks) == 1 and sum(c.Cout == 1024 for c in ks) == 1
    assert sum(not c.bias for c in ks) == 1 and sum(c.plan for c in ks) == 1 and {c.act for c in ks} == {0, 1}
    pt = LISTS['convpw_pertap']
    assert {(c.KH, c.KW) for c in pt} == {(1, 1), (1, 3), (3, 1), (2, 2), (3, 3)}
    assert {(c.KH, c.KW, c.stride) for c in pt} >= {(kh, kw, s) for kh, kw in ((1, 1), (1, 3), (3, 1), (2, 2), (3, 3)) for s in (1, 2, 3)}
    assert {(c.H, c.W) for c in pt} == set(lc.CONVPW_MAPS) and {c.N for c in pt} >= {1, 3, 5}
    assert {lc.pixels(c) for c in pt} >= set(lc.CONVPW_M)
    assert any(c.pad_h != c.pad_w for c in pt) and any(c.dil_h != c.dil_w for c in pt)
    assert any(c.pad_h > c.dil_h * (c.KH - 1) or c.pad_w > c.dil_w * (c.KW - 1) for c in pt)      # padding beyond the filter's reach
    rs = LISTS['convpw_rowshared']
    assert {(c.dil_h, c.dil_w) for c in rs if c.dil_w < 5} == {(dh, dw) for dh in (1, 2, 5) for dw in (1, 2, 3, 4)}
    for dh in (1, 2, 5):
        for dw in (1, 2, 3, 4):
            assert {c.W for c in rs if (c.dil_h, c.dil_w) == (dh, dw)} == {1, 2, 3, 4, 5, 8, 9}
        assert {c.H for c in rs if c.dil_h == dh and c.dil_w < 5} == {1, 2, dh, dh + 1, 7}
    assert any(c.W <= c.dil_w for c in rs) and any(c.W == c.dil_w + 1 for c in rs) and any(c.H != c.W for c in rs)
    assert sum(c.dil_w == 5 for c in rs) == 1
    for name in ('convpw_pertap', 'convpw_rowshared'):            # every family is in both lists
        assert {(c.cm, c.cn, c.act2) for c in LISTS[name]} == set(lc.CONVPW_FAMILIES)
    assert {(c.cm, c.cn) for c in rs} == {(128, 0), (256, 0), (128, 128), (128, 256), (256, 256)}
    assert set(lc.MUTATIONS) == {'tap_row', 'tap_col', 'pad_clamp', 'row_wrap', 'image_wrap', 'last_row', 'last_col', 't1_pad',
                                 'shortcut_centre', 'round_skip', 'k_chunk', 'stride_phase'}


# ------------------------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize('name', NAMES)
def test_every_stage_is_exact_in_fp32_in_any_order_and_really_rounded(name):
    """sum |products| + |bias| + |residual| < 2^24 granules for every (case, storage type, stage); every stored value finite in
    fp16 with room to spare; per stage and storage type a share of the values is changed by the rounding, and between a fifth and
    four fifths of them survive the ReLU"""
    changed, count, positive = {}, {}, {}
    for case in LISTS[name]:
        for dn, dtype, _ in lc.DTYPES:
            st = {}
            lc.compute(case, dtype, None, st)
            for stage, b in lc.bounds(case, dtype).items():
                assert b < lc.LIMIT, (case, dn, stage, b)
            for stage, (pre, post) in st.items():
                assert float(post.abs().max()) < 4096.0, (case, dn, stage)
                k = (dn, stage)
                changed[k] = changed.get(k, 0) + int((pre != post).sum())
                positive[k] = positive.get(k, 0) + int((post > 0).sum())
                count[k] = count.get(k, 0) + pre.numel()
    assert len(count) == 2 * {'halo': 1, 'kstream': 1, 'bneck_first_64': 4, 'bneck_tail_64': 3, 'bneck_tail_128': 3}.get(name, 3)
    for k in count:
        assert changed[k] >= MIN_ROUNDED * count[k], (name, k, changed[k] / count[k])
        assert 0.2 * count[k] <= positive[k] <= 0.8 * count[k], (name, k, positive[k] / count[k])


@pytest.mark.parametrize('name', NAMES)
def test_the_operands_cannot_hide_a_defect(name):
    """every k index (tap, channel) of every filter bank is non-zero in at least one output channel; b1 > 0 (relu(conv1(0) + b1) is
    not the zero bneck_first owes outside the image); inputs are integers 0 .. 3 that differ between neighbouring pixels, rows
    and images; everything is a value of both storage types"""
    for case in LISTS[name]:
        o = lc.ops_of(case)
        for key, v in o.items():
            if v is None:
                continue
            if key.startswith('w'):
                assert bool((v != 0).any(0).all()), (case, key)
            if not key.startswith('b'):                             # biases are fp32
                for _, dtype, _ in lc.DTYPES:
                    assert torch.equal(v.float().to(dtype).double(), v), (case, key)
        if isinstance(case, lc.Bneck) and case.kind == 'first':
            assert bool((o['b1'] > 0).all())
        x = o['t1'] if 't1' in o else o['x']
        assert float(x.min()) >= 0 and float(x.max()) <= 3 and torch.equal(x, x.round())
        if x.shape[2] > 1:
            assert bool((x[:, :, 1:] != x[:, :, :-1]).any(-1).all()), case
        if x.shape[1] > 1:
            assert bool((x[:, 1:] != x[:, :-1]).any(-1).all()), case
        if x.shape[0] > 1:
            assert bool((x[1:] != x[:-1]).any(-1).all()), case


# ------------------------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize('name', NAMES)
def test_every_mutation_shows_wherever_it_is_meaningful(name):
    cases = LISTS[name]
    seen = {m: 0 for m in lc.MUTATIONS if any(lc.applies(m, c) for c in cases)}
    assert {'tap_row', 'tap_col', 'pad_clamp', 'row_wrap', 'image_wrap'} <= set(seen)
    for i, case in enumerate(cases):
        _, dtype, _ = lc.DTYPES[i & 1]
        true = lc.expected(case, dtype)
        for mut in seen:
            if not lc.meaningful(mut, case):
                continue
            seen[mut] += 1
            got = lc.expected(case, dtype, mut)
            assert any(not torch.equal(got[k].view(torch.int16), true[k].view(torch.int16)) for k in true), (case, mut)
    assert all(seen.values()), (name, seen)


def test_which_mutations_apply_where():
    ap = {n: {m for m in lc.MUTATIONS if any(lc.applies(m, c) for c in v)} for n, v in LISTS.items()}
    tap = {'tap_row', 'tap_col', 'pad_clamp', 'row_wrap', 'image_wrap'}
    assert ap['halo'] == tap | {'last_row', 'last_col'}
    assert ap['bneck_first_64'] == tap | {'last_row', 'last_col', 't1_pad', 'shortcut_centre', 'round_skip'}
    assert ap['bneck_tail_64'] == ap['bneck_tail_128'] == tap | {'last_row', 'last_col', 'round_skip'}
    assert ap['kstream'] == tap | {'k_chunk', 'stride_phase'}
    assert ap['convpw_pertap'] == tap | {'k_chunk', 'stride_phase', 'round_skip'}
    assert ap['convpw_rowshared'] == tap | {'k_chunk', 'round_skip'}          # stride 1 throughout: no stride phase to get wrong


# ------------------------------------------------------------------------------------------------------------------ shape choosers
def test_tile_arithmetic_matches_the_launchers():
    halo, bneck, ks, pw = source('conv3x3_halo.hip'), source('bneck_lp.hip'), source('conv_kstream.hip'), source('conv_pw_lp.hip')
    assert (constant(halo, 'HT'),) * 2 == lc.HALO_TILE
    assert (constant(bneck, 'TH'), constant(bneck, 'TW')) == lc.BNECK_TILE
    assert constant(ks, 'CK_BM') == lc.KSTREAM_PANEL
    assert 'grid = p.ntiles - (p.ntiles & 7)' in bneck and 'if (grid < 8) return USOT_EINVAL' in bneck
    for kind, cn in lc.BNECK_FAMILIES:
        cases = LISTS['bneck_%s_%d' % (kind, cn)]
        tiles = [lc.bneck_tiles(c) for c in cases]
        assert min(tiles) >= 8
        for c, nt in zip(cases, tiles):                             # the smallest batch that has eight tiles, except the two uneven walks
            if (c.N, c.H, c.W) not in ((11, 7, 13), (3, 9, 33)):
                assert c.N == 1 or lc.bneck_tiles(c._replace(N=c.N - 1)) < 8, c
        # grid = ntiles - (ntiles & 7) below the CU count: ntiles & 7 workgroups take a second tile, the others do not
        uneven = [nt for nt in tiles if nt & 7 and nt < 64]
        assert {11, 18} <= set(uneven)
        for nt in uneven:
            grid = nt - (nt & 7)
            assert grid >= 8 and 0 < nt - grid < grid
    # conv_pw: the staged tile of the row-shared loop
    assert 'XROWS = BM + 8, NBLK = XROWS / 8, PERK = (NBLK + 2) / 3' in pw
    for bm, nw in ((256, 16), (128, 8)):
        nblk = (bm + 8) // 8
        perk = (nblk + 2) // 3
        assert perk <= nw and 3 * perk >= nblk                      # every 8-row block of the stage has a wave and a k-tile
    assert 'c2->dil_w >= 1 && c2->dil_w <= 4' in pw                  # ... and its 4-pixel halo covers every eligible dil_w
    for c in LISTS['convpw_rowshared']:
        assert lc.rowshared_eligible(c) == (c.dil_w <= 4), c
        assert lc.convpw_loops(c) == (4, 0)
    assert sum(lc.rowshared_eligible(c) for c in LISTS['convpw_pertap']) >= 4
    assert any(not lc.rowshared_eligible(c) and c.KH == 3 and c.KW == 3 and c.stride == 1 for c in LISTS['convpw_pertap'])
    for c in LISTS['convpw_pertap'] + LISTS['convpw_rowshared']:
        assert min(lc.out_hw(lc.geo_of(c))) >= 1
    kinds = set()
    for c in LISTS['convpw_rowshared']:
        assert lc.pixels(c) > 256                                   # a 128- and a 256-pixel panel edge inside the map
        kinds |= lc.panel_edge_kinds(c)
    assert kinds == {'row', 'row_end', 'image_end'}
    assert {lc.pixels(c) % 128 for c in LISTS['convpw_pertap']} >= {127, 0, 1}


# ------------------------------------------------------------------------------------------------------------------ the parked tap
def test_kstream_parked_taps_stay_inside_x():
    """set_tap parks a tap outside the image on max(centre pixel, the tap's offset from the centre) - counted in pixels from the
    start of x.  Launched cases: every pixel read exists.  Refused geometries: one does not; the launcher's rule is exactly
    N H W > dil (W + 1) for them and accepts everything the sweep launches."""
    text = source('conv_kstream.hip')
    assert 'park > 0 ? park : 0' in text and '(long)N * H * W <= (long)dil * (W + 1)' in text
    for c in LISTS['kstream']:
        assert lc.kstream_accepts(c.N, c.H, c.W, c.stride, c.pad, c.dil), c
        read = lc.kstream_parked(c.N, c.H, c.W, c.stride, c.pad, c.dil)
        assert min(read) >= 0 and max(read) < c.N * c.H * c.W, c
    for N, H, W, kw in lc.KSTREAM_PARKED_REFUSED:
        assert not lc.kstream_accepts(N, H, W, 1, kw['pad'], kw['dil'])
        read = lc.kstream_parked(N, H, W, 1, kw['pad'], kw['dil'])
        assert max(read) >= N * H * W, (N, H, W, kw)                # the read the refusal prevents
        assert max(read) <= kw['dil'] * (W + 1)
    # the rule is not wider than needed by more than the model shows: wherever it refuses a small map, the model leaves x
    for dil in (1, 2, 3):
        for H in range(1, 6):
            for W in range(1, 8):
                for N in (1, 2):
                    if min(lc.out_hw(lc.Geo(N, H, W, 3, 3, 1, dil, dil, dil, dil))) < 1:
                        continue
                    inside = max(lc.kstream_parked(N, H, W, 1, dil, dil)) < N * H * W
                    assert inside == lc.kstream_accepts(N, H, W, 1, dil, dil), (N, H, W, dil)


def test_the_refusal_list_names_every_launcher():
    rows = lc.refusals()
    assert len({r[0] for r in rows}) == len(rows)
    assert {r[1] for r in rows} == {'halo', 'bneck_first', 'bneck_tail', 'kstream', 'kstream_plan', 'conv_pw', 'conv_pw_pair'}
    names = ' | '.join(r[0] for r in rows)
    for word in ('Cin 128', 'act 2', 'misaligned', 'NULL', '7 tiles', 'Cnext 96', 'pad > dil', 'stride 3', 'OH <= 0', 'pd.M != M',
                 'without ReLU', 'groups', 'ksplit', 'res in conv2', 'parked tap'):
        assert word in names, word
