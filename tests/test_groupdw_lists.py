"""CPU: the lists of tests/groupdw_cases.py are the ones the GroupDW variant sweep was specified with, their operands keep every
partial sum an exact multiple of 2^-2 below 220, the float64 reference agrees with the oracle's xcorr_depthwise and can tell a wrong
kernel from a right one - the cap that keeps a later edit from thinning tests/test_gpu_groupdw_sweep.py into something a wrong
kernel would pass.  Nothing here needs the library."""
import ast

import torch

import groupdw_cases as gw
import usot_oracle as orc

SPEC = """
codes        [1,5,50,52,2,3,4,6,7,8,9]
patch_hw     [1,4,5,6,11]
col_oh       [1,5,31,32]
col_ow       [1,3,4,5,9]
rows         [(3,21),(3,22),(3,23),(3,24),(3,25),(3,26),(3,27),(3,28),(3,29),(3,30),(1,21),(1,25),(1,26),(1,30),(2,21),(2,25),(2,26),(2,30),(6,21),(6,25),(6,26),(6,30),(29,21),(29,25),(29,26),(29,30)]
dma_oh       [1,2,3,4,5,6,7,25,27,28]
dma_ow       [25,27]
auto         [(((3,1),),25,1),(((64,1),),25,6),(((32,1),(32,2)),25,6),(((64,1),),23,4)]
c_channels   [64,128,192,256,320,512]
c_samples    [1,2,5]
s_channels   [256,128]
segs3        ((3,1),(2,2),(5,3))
segs2        ((1,1),(1,1))
wsm          [(0.5,0.25,1.0),(1.0,0.5,0.25),(0.25,1.0,0.5)]
d_shapes     [(64,((3,1),)),(128,((5,3),))]
l_ow         [25,27]
l_oh         [1,6,25]
l_channels   [64,256]
y_geo        (2,6)
y_channels   [128,256]
y_counts     [-3,0,1,4,5,9]
p_ow         [25,27]
p_oh         [1,6]
b_geo        [(6,25),(27,27)]
b_channels   [64,256]
"""
R_IDS = """C0 C32 C96 OH0 OW0 nseg0 nseg4 seg2_OH seg2_OW seg2_C S0 x_rep0 null_x null_z null_out hk wk code-1 code10 code51 cols_oh33
v3_ow20 v3_ow31 v4_ow20 v4_ow31 v6_ow26 v7_ow26 v8_ow26 v9_ow26 lp1_ow26 lp2_ow26 lp_dtype0 lp_dtype3
v6_x_co2 v6_x_cs v6_x_base v7_x_co2 v7_x_cs v7_x_base v8_x_co2 v8_x_cs v8_x_base v8_z_co2 v8_z_cs v8_z_base
v9_x_co2 v9_x_cs v9_x_base v9_z_co2 v9_z_cs v9_z_base v3_x_co2 v3_x_cs v3_x_base
dyn_v5 dyn_v50 dyn_v52 dyn_v2 dyn_v3 dyn_v4 dyn_v6 dyn_v7 dyn_v8 dyn_v9 dyn_misaligned"""
MI355X_CU = 256


def _small_cases():
    """every case of parts G, C, S, D, L and Y (part P is sized by the device: test_persistent_round_counts)"""
    out = [c for c, _ in gw.auto_cases()]
    for code in gw.CODES:
        out += gw.g_cases(code) + gw.c_cases(code) + gw.s_cases(code) + gw.d_cases(code)
    return out + gw.l_cases() + gw.y_cases()


def _problems(cases):
    """the distinct operand sets behind a list of cases (the variant code does not enter the seed)"""
    seen = {}
    for c in cases:
        seen.setdefault(c._replace(cols=0, part=''), c)
    return list(seen.values())


def test_the_lists_are_the_specified_ones():
    spec = {ln.split()[0]: ast.literal_eval(ln.split(None, 1)[1]) for ln in SPEC.strip().splitlines()}
    have = dict(codes=gw.CODES, patch_hw=gw.G_PATCH_HW, col_oh=gw.G_COL_OH, col_ow=gw.G_COL_OW, rows=gw.G_ROWS, dma_oh=gw.G_DMA_OH,
                dma_ow=gw.G_DMA_OW, auto=gw.AUTO, c_channels=gw.C_CHANNELS, c_samples=gw.C_SAMPLES, s_channels=gw.S_CHANNELS,
                segs3=gw.SEGS3, segs2=gw.SEGS2, wsm=gw.WSM, d_shapes=gw.D_SHAPES, l_ow=gw.L_OW, l_oh=gw.L_OH,
                l_channels=gw.L_CHANNELS, y_geo=gw.Y_GEO, y_channels=gw.Y_CHANNELS, y_counts=gw.Y_COUNTS, p_ow=gw.P_OW, p_oh=gw.P_OH,
                b_geo=gw.B_GEO, b_channels=gw.B_CHANNELS)
    assert have == spec
    assert (gw.PATCH, gw.COLS, gw.ROWS, gw.DMA, gw.PERSISTENT) == ([1, 5, 50, 52], [2], [3, 4], [6, 7, 8, 9], [8, 9])
    assert (gw.V_MAX, gw.GRAIN, gw.BOUND, gw.Y_CAPACITY, gw.P_XREP, gw.AUTO_C) == (2, 0.25, 220, 5, 3, 128)
    assert [len(gw.g_cases(c)) for c in gw.CODES] == [25, 25, 25, 25, 20, 26, 26, 20, 20, 20, 20] and len(gw.auto_cases()) == 4
    assert all(len(gw.c_cases(c)) == 18 and len(gw.s_cases(c)) == 4 for c in gw.CODES)
    assert [len(gw.d_cases(c)) for c in gw.CODES] == [8, 8, 8, 8, 8, 8, 8, 8, 8, 6, 6]
    assert [gw.d_layouts(c)[3:] for c in gw.CODES] == [['odd']] * 5 + [['oddz'], ['odd'], ['oddz'], ['oddz'], [], []]
    assert len(gw.l_cases()) == 24 and len(gw.y_cases()) == 2 and len(gw.b_cases()) == 4
    assert [r[0] for r in gw.r_cases()] == R_IDS.split()
    assert {c: gw.small_geo(c) for c in gw.CODES} == {1: (2, 1), 5: (2, 1), 50: (2, 1), 52: (2, 1), 2: (2, 1), 3: (2, 21), 4: (2, 21),
                                                     6: (2, 25), 7: (2, 25), 8: (2, 25), 9: (2, 25)}
    C = 64
    assert gw.layout('hi', C) == ((128,) * 3, (64,) * 3, (128,) * 3, (64,) * 3) and gw.layout('lo', C)[1] == (0, 0, 0)
    assert gw.layout('branch', C) == ((C + 4, 2 * C, C + 64), (4, C, 0), (C + 8, C, 2 * C), (8, 0, C))
    assert gw.layout('odd', C) == ((C + 1,) * 3, (1,) * 3, (C + 3,) * 3, (3,) * 3)
    assert gw.layout('oddz', C) == ((C,) * 3, (0,) * 3, (C + 3,) * 3, (3,) * 3)
    for name in ('hi', 'lo', 'branch'):                                      # what the 16-byte loaders are given is 16-byte aligned
        assert all(v % 4 == 0 for c in (64, 128) for vals in gw.layout(name, c) for v in vals)
    assert all(v % 4 == 0 for vals in gw.layout('oddz', C)[:2] for v in vals)


def test_what_the_lists_cover():
    for code in gw.PATCH:                                                    # every residue of a 5-row / 5-column patch, both axes
        geo = gw.geometries(code)
        assert {oh % 5 for oh, _ in geo} == {0, 1, 4} and {ow % 5 for _, ow in geo} == {0, 1, 4}
        assert any(oh > 5 for oh, _ in geo) and any(oh > ow for oh, ow in geo) and any(oh < ow for oh, ow in geo)
    assert {n % 5 for n in gw.G_PATCH_HW} == {0, 1, 4} and {(n + 4) // 5 for n in gw.G_PATCH_HW} == {1, 2, 3}
    geo = gw.geometries(2)
    assert {ow % 4 for _, ow in geo} == {0, 1, 3} and max(oh for oh, _ in geo) == 32 and any(ow > 8 for _, ow in geo)
    for code in gw.ROWS:                                                     # every accepted width; both strip counts; ragged last strip
        geo = gw.geometries(code)
        assert {ow for _, ow in geo} == set(range(21, 31)) and {(ow + 4) // 5 for _, ow in geo} == {5, 6}
        assert {ow % 5 for _, ow in geo} == {0, 1, 2, 3, 4} and {oh for oh, _ in geo} == {1, 2, 3, 6, 29}
    for code in gw.DMA:                                                      # every residue of the five-way unrolled row loop, one and several trips
        geo = gw.geometries(code)
        for ow in (25, 27):
            assert {(oh + 4) % 5 for oh, w in geo if w == ow and oh + 4 <= 10} == {0, 1, 2, 3, 4}
            assert {(oh + 4) % 5 for oh, w in geo if w == ow and oh + 4 > 10} >= {1, 2, 4} and any(oh + 4 == 5 for oh, w in geo if w == ow)
        assert any(oh != ow for oh, ow in geo)
    assert [gw.p_units(s + t, 256) for (s, _), (t, _) in [gw.SEGS2]] == [8]
    assert sum(s for s, _ in gw.SEGS3) == 10 and [-(-s // r) for s, r in gw.SEGS3] == [3, 1, 2]
    border = [gw.SEGS3[0][0], gw.SEGS3[0][0] + gw.SEGS3[1][0]]              # C = 256 pairs samples (2 k, 2 k + 1): both borders are odd
    assert border == [3, 5] and all(b % 2 == 1 for b in border)
    assert {c.C // 64 for code in gw.CODES for c in gw.c_cases(code)} == {1, 2, 3, 4, 5, 8}
    totals = [sum(s for s, _ in segs) for segs, _, _ in gw.AUTO]
    assert totals == [3, 64, 64, 64] and [max(r for _, r in segs) for segs, _, _ in gw.AUTO] == [1, 1, 2, 1]


def test_persistent_round_counts():
    G = gw.p_resident(MI355X_CU)
    assert G == 512 and gw.p_resident(304) == 608 and gw.p_resident(255) == 504
    counts = gw.p_counts(MI355X_CU)
    assert counts == {256: [125, 126, 127, 128, 129, 130, 257, 258], 64: [511, 512, 513, 1025], 192: [171]}
    assert [gw.p_units(n, 256) for n in counts[256]] == [504, 504, 512, 512, 520, 520, 1032, 1032]
    assert [gw.p_units(n, 64) for n in counts[64]] == [G - 1, G, G + 1, 2 * G + 1] and gw.p_units(171, 192) == G + 1
    assert max(counts[64]) * 6 * 25 * 64 * 4 < 64 << 20                      # the largest response: tens of MB
    for cu in (64, 255, 256, 304):                                           # whatever the device: same shape of list
        G, cs = gw.p_resident(cu), gw.p_counts(cu)
        assert sorted({gw.p_units(n, 256) for n in cs[256]}) == [G - 8, G, G + 8, 2 * G + 8] and {n % 2 for n in cs[256]} == {0, 1}
        assert gw.p_units(cs[192][0], 192) > G >= gw.p_units(cs[192][0] - 1, 192)


def _check_operands(seg, C):
    for b in range(3):
        for t, cs, co in ((seg.x[b], seg.x_cs[b], seg.x_co[b]), (seg.z[b], seg.z_cs[b], seg.z_co[b])):
            assert t.shape[-1] == cs and co + C <= cs
            inside = t[..., co:co + C]
            assert torch.equal(inside, inside.round()) and float(inside.abs().max()) <= gw.V_MAX
            assert int(torch.isnan(t).sum()) == (cs - C) * t[..., 0].numel()   # NaN in exactly the channels outside the slice
    assert sorted(seg.wsm) == [0.25, 0.5, 1.0]


def test_every_partial_sum_is_an_exact_multiple_of_a_quarter():
    assert gw.BOUND == max(abs(w) for t in gw.WSM for w in t) * gw.V_MAX * gw.V_MAX * 55 == 220
    assert gw.BOUND / gw.GRAIN < 1 << 11                                     # exact in fp16's 11 bits, a fortiori in fp32's 24
    assert len(set(gw.WSM)) == 3 and all(sorted(t) == [0.25, 0.5, 1.0] for t in gw.WSM)
    seen_max = 0.0
    for case in _problems(_small_cases()):
        segs, refs = gw.build(case)
        assert len({g.wsm for g in segs}) == len(segs)                       # a triple of its own per segment
        for g, ref in zip(segs, refs):
            _check_operands(g, case.C)
            assert float(ref.abs().max()) <= gw.BOUND and torch.equal(ref * 4, (ref * 4).round()), case
            assert torch.equal(ref.float().double(), ref) and torch.equal(ref.half().double(), ref)
            assert torch.equal(gw.stored(ref, torch.float16).double(), ref)
            bf = gw.stored(ref, torch.bfloat16).double()
            assert bool(((bf - ref).abs() <= ref.abs() * 2.0 ** -8).all())   # half a unit in the last of bf16's 8 bits
            chan = ref.reshape(-1, case.C)
            assert len({tuple(col) for col in chan.t().tolist()}) > case.C // 2 or chan.shape[0] < 4, case     # channels differ
            seen_max = max(seen_max, float(ref.abs().max()))
    assert seen_max > 16                                                     # the range is used
    for oh in gw.P_OH:                                                       # part P: the operands of the largest launch
        for ow in gw.P_OW:
            for C, counts in gw.p_counts(MI355X_CU).items():
                g = gw.segment(oh, ow, C, max(counts), gw.P_XREP, 0)
                _check_operands(g, C)


def _oracle(seg, C):
    ref = 0
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    for b in range(3):
        x = seg.x[b][..., seg.x_co[b]:seg.x_co[b] + C]
        z = seg.z[b][..., seg.z_co[b]:seg.z_co[b] + C]
        ref = ref + seg.wsm[b] * orc.xcorr_depthwise(nchw(x).repeat_interleave(seg.x_rep, 0)[:seg.S], nchw(z))
    return ref.permute(0, 2, 3, 1)


def test_reference_is_the_oracles_xcorr_depthwise():
    n = 0
    for case in _problems(_small_cases()):
        segs, refs = gw.build(case)
        for g, ref in zip(segs, refs):
            assert torch.equal(_oracle(g, case.C), ref), case               # exact operands: equality here as well
            n += 1
    assert n > 200
    for case in gw.b_cases()[:1]:                                            # real-valued operands: two float64 summation orders
        segs, refs = gw.build(case, True)
        for g, ref in zip(segs, refs):
            assert float((_oracle(g, case.C) - ref).abs().max()) < 1e-12


MUT_PARTS = {'weights': 'GCSD', 'roles': 'GCSD', 'tap_col': 'GCSD', 'tap_row': 'GCSD', 'last_col': 'GCSD', 'template': 'GCSD',
             'group': 'GCSD',
             'map': 'GSD',          # part C runs x_rep = 1 throughout: nothing to get wrong
             'x_co': 'D'}           # only part D offsets its search maps


def test_reference_tells_a_wrong_kernel_from_a_right_one():
    """each mistake of gw.MUTATIONS changes the expected output of EVERY case where gw.meaningful says it can; MUT_PARTS names the
    parts that hold such a case"""
    assert sorted(MUT_PARTS) == sorted(gw.MUTATIONS)
    cases = [c for c in _small_cases() if c.part in 'GCSD']
    hit = {m: set() for m in gw.MUTATIONS}
    for case in _problems(cases):
        parts = {c.part for c in cases if c._replace(cols=0, part='') == case._replace(cols=0, part='')}
        segs, refs = gw.build(case)
        for mut in gw.MUTATIONS:
            got = [gw.ref64(g, case.OH, case.OW, case.C, mut) for g in segs]
            changed = any(not torch.equal(a, b) for a, b in zip(got, refs))
            assert changed == gw.meaningful(mut, case), (mut, case)
            if changed:
                hit[mut] |= parts
    assert {m: ''.join(p for p in 'GCSD' if p in hit[m]) for m in gw.MUTATIONS} == MUT_PARTS
