"""CPU: the lists of tests/tail_cases.py are the ones the frame-tail sweep was specified with, their operands keep every comparison
of tests/test_gpu_tail_sweep.py an equality (decode margins, exact thin-conv partial sums, power-of-two Conf_Fusion denominators),
the Hanning window is bitwise symmetric, the float64 decode agrees with the oracle's on the golden cases, the restated OpenCV resize
has its closed forms, and every listed mutation - a plausible wrong kernel - changes the reference's output on the sweep's own
operands, so that a kernel with that defect fails the GPU file."""
import numpy as np
import pytest
import torch

import tail_cases as tc
import usot_oracle as orc
from usot_amd import hostutils


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b):
    """bit-equal, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# =========================================================================================================================== decode
def test_decode_lists_are_the_specified_ones():
    assert tc.DEC_S_F32 == list(range(1, 65)) and tc.DEC_S_DEV == list(range(2, 65)) and tc.DEC_S_BATCH == list(range(2, 33))
    assert tc.DEC_BATCH_B == [1, 5]
    assert (tc.STRIDE, tc.RATIO, tc.PENALTY_K, tc.WINDOW_INFLUENCE) == (8, orc.Hyper.ratio, orc.Hyper.penalty_k, orc.Hyper.window_influence)
    assert tc.instance_size(25) == 255 and tc.instance_size(27) == 271
    assert tc.placements(1) == [0] and tc.placements(8) == [0, 63] and tc.placements(9) == [0, 63, 64, 80]
    assert tc.placements(32) == [0, 63, 64, 1023] and tc.placements(33) == [0, 63, 64, 1023, 1024, 1088]
    assert tc.placements(64) == [0, 63, 64, 1023, 1024, 4095]
    assert tc.DEC_MUTATIONS == ['argmax_last', 'argmax_thread', 'clamp_no_gap']
    for S in range(33, 65):
        pairs = tc.tie_pairs(S)
        assert {(5, 1029, 0.0), (1000, 1029, 0.0), (3, 40, 0.0), (10, 100, 0.0), (0, S * S - 1, 0.0)} <= set(pairs)
        mirrored = [(a, b) for a, b, wi in pairs if wi]
        assert all(a + b == S * S - 1 for a, b in mirrored)
        assert any(b >= 1024 and b % 1024 < a % 1024 for a, b in mirrored)            # the later cell on a lower thread
        assert (S % 2 == 0) or any(b == a + 1024 for a, b in mirrored)                # one thread, two passes
    for S in tc.DEC_S_F32:
        kinds = {c.kind for c in tc.decode_cases(S)}
        assert kinds == set(tc.DEC_KINDS) - ({'tie'} if S == 1 else set())
        assert all(c < S * S for case in tc.decode_cases(S) for c in case.cells)
    assert sum(len(tc.decode_cases(S)) for S in tc.DEC_S_F32) == 2470
    assert tc.DEC_REFUSALS['batch'][:4] == ['S0', 'S33', 'B0', 'B65536'] and tc.DEC_REFUSALS['f32'][:2] == ['S0', 'S65']


def test_hanning_window_is_bitwise_symmetric():
    for S in range(1, 65):
        w = tc.window(S)
        assert np.array_equal(bits(w), bits(w[::-1])), S


def test_planted_score_is_stable():
    """sigmoid(12) sits 0.04 ulp from a rounding boundary of 1 + exp(-12) - 1e4 times any expf error - and its blend with itself
    rounds alike in two roundings and through either fused multiply-add"""
    f = np.float32
    e = float(np.exp(np.float64(-12.0)))
    frac = (e / 2.0 ** -23) % 1.0
    assert 0.03 < abs(frac - 0.5) < 0.05
    s = f(1) / (f(1) + np.exp(f(-12.0)))
    r, q = f(tc.RATIO), f(1) - f(tc.RATIO)
    two = f(f(r * s) + f(q * s))
    assert two == f(float(r) * float(s) + float(f(q * s))) == f(float(q) * float(s) + float(f(r * s)))


@pytest.mark.parametrize('lo,hi', [(1, 33), (33, 49), (49, 65)])
def test_decode_reference_margins(lo, hi):
    """every finite case: the planted cell wins with penalty exactly 1 and leads every other cell by >= 1e-4 (0.018 by construction);
    every tie: both cells hold the same bits, the first wins; every NaN case: the first NaN wins"""
    for S in range(lo, hi):
        for case in tc.decode_cases(S):
            ref = tc.decode_expected(case)
            if case.kind in ('win', 'clamp_out', 'clamp_flip'):
                assert ref['i'] == case.cells[0] and ref['pen'] == 1.0, case
                assert tc.decode_margin(case, ref) >= 1e-4, case
            elif case.kind == 'tie':
                a, b = case.cells
                assert ref['i'] == a and bits(ref['pscore'][[a]]) == bits(ref['pscore'][[b]]) and ref['pen'] == 1.0, case
                assert tc.decode_margin(case, ref) >= 1e-4, case
            elif case.kind == 'all_nan':
                assert ref['i'] == 0 and np.isnan(ref['ps'])
            else:
                assert ref['i'] == case.cells[0] and np.isnan(ref['ps']), case
                assert np.isnan(ref['pscore']).sum() == len(case.cells)
            if case.kind.startswith('clamp'):
                top = 2 * (S // 2) + 1.0
                want = [-1.0, -1.0, top, top] if case.kind == 'clamp_out' else [top, top, -1.0, -1.0]
                assert S == 1 or ref['roi'].tolist() == want, case                     # all four clamps, both sides of each axis


def test_decode_mutations_change_the_reference():
    hit = {m: 0 for m in tc.DEC_MUTATIONS}
    for S in (8, 25, 33, 64):
        for case in tc.decode_cases(S):
            ref = tc.decode_expected(case)
            for m in tc.DEC_MUTATIONS:
                mut = tc.decode_expected(case, m)
                hit[m] += (mut['i'] != ref['i']) if m.startswith('argmax') else not same(mut['roi'], ref['roi'])
    assert all(hit.values()), hit
    # the pair (1000, 1029) is what tells "ordered by thread" from "first": thread 5 owns the later cell
    case = tc.Dec(33, 'tie', (1000, 1029), 0.0)
    assert tc.decode_expected(case, 'argmax_thread')['i'] == 1029 and tc.decode_expected(case)['i'] == 1000


@pytest.mark.parametrize('inst', [255, 271])
def test_decode_reference_agrees_with_the_oracle(gold_host, inst):
    p = orc.Hyper(inst)
    S = p.score_size
    for k in range(4):
        c = 'i%d/decode%d' % (inst, k)
        cls, cm, bbox = gold_host[c + '/cls'][0, 0], gold_host[c + '/cls_mem'][0, 0], gold_host[c + '/bbox'][0]
        tsz = gold_host[c + '/tsz'] * float(gold_host[c + '/scale_z'])
        win2d = np.outer(np.hanning(S), np.hanning(S))
        _, _, score, box, rc = orc.decode(p, cls, cm, bbox, gold_host[c + '/tpos'], tsz, win2d, float(gold_host[c + '/scale_z']))
        ref = tc.decode_ref(cls.reshape(-1), cm.reshape(-1), bbox.reshape(4, -1), win2d.reshape(-1), S, inst, p.total_stride, p.ratio,
                            p.penalty_k, p.window_influence, float(tsz[0]), float(tsz[1]))
        assert ref['i'] == rc[0] * S + rc[1]
        assert np.array_equal(ref['box'], np.array(box)) and ref['sc'] == score
        assert np.array_equal(ref['roi'], orc.pool_label_search(p, box).astype(np.float32))
        assert np.array_equal(ref['roi'], gold_host[c + '/out_poolbox'][0])


# ============================================================================================================================= thin
def _thin_all():
    out = [c for cin in tc.THIN_CIN for c in tc.thin_pixel_cases(cin)] + tc.thin_multi_cases()
    return out + [c for W in tc.ROW_W for c in tc.thin_row_cases(W)] + [c for c, _, _, _ in tc.thin_split_cases()]


def test_thin_lists_are_the_specified_ones():
    assert tc.THIN_CIN == [4, 64, 252, 256, 260, 512] and tc.THIN_HW == [(1, 1), (1, 5), (5, 1), (3, 4), (7, 7)]
    assert tc.ROW_W == [1, 2, 25, 63, 64] and tc.THIN_MUTATIONS == ['pad_row', 'row_lane']
    singles = [c for cin in tc.THIN_CIN for c in tc.thin_pixel_cases(cin)]
    assert len(singles) == 6 * 4 * 5 * 4 == len(set(singles))
    assert {(c.Cin, c.probs[0].cout, (c.H, c.W), c.probs[0].act) for c in singles} == {
        (ci, co, hw, a) for ci in tc.THIN_CIN for co in range(1, 5) for hw in tc.THIN_HW for a in range(4)}
    multi = tc.thin_multi_cases()
    assert len(multi) == 28 and {len(c.probs) for c in multi} == {1, 2, 3, 4}
    assert {p.groups for c in multi for p in c.probs} == {1, 2, 3} and any(p.pad for c in multi for p in c.probs)
    assert any(not p.bias for c in multi for p in c.probs) and {p.act for c in multi for p in c.probs} == {0, 1, 2, 3}
    assert all(tc.thin_plan(c)[0] == 'pixel' for c in singles + multi)
    rows = [c for W in tc.ROW_W for c in tc.thin_row_cases(W)]
    assert len(rows) == 20 and {(c.W, c.probs[0].cout) for c in rows} == {(w, co) for w in tc.ROW_W for co in range(1, 5)}
    assert {p.act for c in rows for p in c.probs} == {0, 1, 2, 3}
    for c in rows:
        assert tc.thin_plan(c) == ('row', [0] if c.probs[0].cout == 4 else []) and tc.thin_plan(c, 70)[0] == 'pixel'
        assert sum(p.groups * c.N * c.H for p in c.probs) == 1032
    for c, form, split, why in tc.thin_split_cases():
        assert tc.thin_plan(c) == (form, split), why
    assert [why.split(':')[0] for _, _, _, why in tc.thin_split_cases()] == [
        'a single 4-channel problem', 'a single 4-channel problem', 'two 4-channel problems among three',
        'four problems, one of 4 channels', '4 channels in two groups', 'W = 65', '1023 rows', '1024 rows']
    assert len(tc.THIN_REFUSALS) == 32 == len(set(tc.THIN_REFUSALS))


def test_thin_operands_are_exact():
    """filters, biases and activations are multiples of 1/4, |x| <= 4, |w| <= 1, and no partial sum of any order reaches 2^24 / 16;
    every filter family and every single-tap position is there"""
    fams, taps = set(), set()
    for case in _thin_all():
        for pi, p in enumerate(case.probs):
            w, b = tc._filters(case, pi)
            assert bool(((w * 4) == (w * 4).round()).all()) and bool(((b * 4) == (b * 4).round()).all()) and float(w.abs().max()) <= 1.0
            assert float((w.abs().sum((2, 3, 4)) * 4.0 + b.abs()).max()) * 16 < 2 ** 24, case
            if p.act in tc.EXACT_ACTS:
                for g in range(p.groups):
                    for c in range(p.cout):
                        fams.add(tc._family(case, pi, g, c))
                        if tc._family(case, pi, g, c) == 'tap':
                            nz = w[g, c].nonzero()
                            assert len(nz) == 1
                            taps.add((int(nz[0, 1]), int(nz[0, 2])))
    assert fams == set(tc.FAMILIES) and taps == set(tc.TAPS)
    for case in tc.thin_multi_cases() + tc.thin_pixel_cases(260):
        for pi in range(len(case.probs)):
            x = tc._activations(case, pi)
            assert bool(((x * 4) == (x * 4).round()).all()) and float(x.abs().max()) <= 4.0
            pre = tc.thin_pre(case, pi)
            assert bool(((pre * 16) == (pre * 16).round()).all()) and float(pre.abs().max()) * 16 < 2 ** 24
            assert torch.equal(pre.float().double(), pre)


def test_thin_conf_edges_and_exp_allowance():
    """the ACT_CONF problems see every clamp edge (-1/16, 0, 1/16, 63/16, 4, 65/16), and torch-CPU's float32 exp is within EXP_CPU_ERR
    of float64 on the arguments of the sweep - the figure the device's allowance is four times of"""
    seen, worst = set(), 0.0
    for case in [c for cin in tc.THIN_CIN for c in tc.thin_pixel_cases(cin)] + tc.thin_multi_cases() + tc.thin_row_cases(2):
        for pi, p in enumerate(case.probs):
            if p.act == tc.ACT_CONF:
                here = set(tc.thin_pre(case, pi).reshape(-1).tolist())
                seen |= here & set(tc.CONF_EDGES)
                if p.cout >= 2:
                    assert set(tc.CONF_EDGES) <= here, case
            if p.act in (tc.ACT_EXP, tc.ACT_CONF):
                args = tc.thin_exp_args(case, pi)
                assert float(args.abs().max()) <= 8.0
                worst = max(worst, tc.exp_cpu_err(args))
    assert seen == set(tc.CONF_EDGES)
    print('torch-CPU float32 exp vs float64: max relative error %.3e' % worst)
    assert 0.75 * tc.EXP_CPU_ERR <= worst <= 1.25 * tc.EXP_CPU_ERR and tc.EXP_ALLOW == 4 * tc.EXP_CPU_ERR    # the recorded figure is the measured one


def test_thin_mutations_change_the_reference():
    for case in tc.thin_pixel_cases(4) + tc.thin_multi_cases():
        for pi, p in enumerate(case.probs):
            ref, mut = tc.thin_act64(tc.thin_pre(case, pi), p.act), tc.thin_act64(tc.thin_pre(case, pi, 'pad_row'), p.act)
            if p.act == tc.ACT_NONE:
                assert not torch.equal(ref[..., 0, :], mut[..., 0, :]), case
            assert torch.equal(ref[..., 1:, :], mut[..., 1:, :])
    for case in tc.thin_row_cases(1) + tc.thin_row_cases(2):
        for pi, p in enumerate(case.probs):
            ref, mut = tc.thin_act64(tc.thin_pre(case, pi), p.act), tc.thin_act64(tc.thin_pre(case, pi, 'row_lane'), p.act)
            assert not same(ref.float().numpy(), mut.float().numpy()), case


# ============================================================================================================================= crop
def test_crop_lists_are_the_specified_ones():
    assert tc.CROP_S == [15, 16, 127, 255] and tc.CROP_IMAGES['tiny'] == (8, 5)
    for S in (15, 16):
        assert tc.crop_wins(S) == list(range(1, 2 * S + 4))
    for S in (127, 255):
        w = tc.crop_wins(S)
        assert {1, 2, 3} | set(range(S - 2, S + 3)) | set(range(2 * S - 2, 2 * S + 3)) | set(range(37, 1101, 37)) == set(w)
        assert max(w) == 1073
    for S in tc.CROP_S:
        cases = tc.crop_cases(S)
        H, W = tc.CROP_IMAGES[cases[0].image]
        inside = lambda c: c.x0 < W and c.y0 < H and c.x0 + c.win > 0 and c.y0 + c.win > 0
        big = [c for c in cases if c.image != 'tiny']
        assert sum(not inside(c) for c in big) == 16                                   # wholly outside: four sides at four windows
        assert any(c.x0 < 0 <= c.y0 and inside(c) for c in big) and any(c.x0 < 0 and c.y0 < 0 and inside(c) for c in big)
        assert any(c.x0 + c.win > W and c.y0 + c.win > H and inside(c) for c in big)
        assert sum(c.image == 'tiny' for c in cases) == 7
        assert any(c.win > 2 * S for c in cases) and any(2 * c.win < S for c in cases)  # down by more than 2, up by more than 2
    assert tc.CROP_SKIPPED == ['im0', 'H0', 'W-1', 'win0'] and tc.CROP_MUTATIONS == ['double_coord']


def test_crop_origin_reaches_the_window():
    from usot_amd.engine import crop_fields
    for S in (15, 255):
        for c in tc.crop_cases(S):
            x0, y0, win, fill = crop_fields(tc.crop_image(c.image).shape, tc.crop_pos(c), c.win, tc.CROP_FILL)
            assert (x0, y0, win, fill) == (c.x0, c.y0, c.win, tc.CROP_FILL), c


def test_resize_restatement_closed_forms():
    """win == S is the identity, win == 2 S the rounded 2 x 2 mean, a constant image stays constant, a horizontal ramp monotone;
    resize_with on the host's own axis rule is the host's resize"""
    g = np.random.default_rng(3)
    for S in (15, 16, 127):
        im = g.integers(0, 256, (S, S, 3)).astype(np.uint8)
        assert np.array_equal(hostutils.resize_bilinear_u8(im, S, S), im)
        im2 = g.integers(0, 256, (2 * S, 2 * S, 3)).astype(np.uint8)
        q = im2.astype(np.float64)
        mean = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]) / 4
        assert np.array_equal(hostutils.resize_bilinear_u8(im2, S, S), np.floor(mean + 0.5).astype(np.uint8))
        for n in (1, 2, 3, S - 1, S + 1, 2 * S - 1, 2 * S + 1, 5 * S + 2):
            const = np.full((n, n, 3), 173, np.uint8)
            assert (hostutils.resize_bilinear_u8(const, S, S) == 173).all(), (S, n)
            ramp = np.repeat(np.linspace(0, 255, n).astype(np.uint8)[None, :, None], n, 0).repeat(3, 2)
            out = hostutils.resize_bilinear_u8(ramp, S, S).astype(np.int64)
            assert (np.diff(out, axis=1) >= 0).all(), (S, n)
            r = g.integers(0, 256, (n, n, 3)).astype(np.uint8)
            assert np.array_equal(tc.resize_with(r, S, hostutils._resize_axis), hostutils.resize_bilinear_u8(r, S, S))


def test_crop_mutation_changes_the_reference():
    """a kernel that floors the coordinate in double (no rounding to float first) moves a weight in dozens of the windows of the two
    production sizes (in none at S = 15 and 16: there the two roundings agree at every window)"""
    for S in (127, 255):
        hit = sum(not np.array_equal(tc.crop_ref(c, S), tc.crop_ref(c, S, 'double_coord')) for c in tc.crop_cases(S))
        assert hit >= 30, (S, hit)


# =========================================================================================================================== reduce
def _pow2(t):
    m, _ = np.frexp(t.numpy())
    return bool((m == 0.5).all())


def test_reduce_lists_and_exactness():
    assert tc.RED_M == [1, 2, 4, 7] and tc.RED_C == [4, 8, 36, 256] and tc.CONFS[7] == (1, 1, 2, 4, 8, 8, 8)
    assert len(tc.reduce_cases()) == 16 and len(tc.RED_DTYPES) == 6
    assert [m for m, _ in tc.RED_MAPS if len(m) == 7] == [(0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (0, 1, 2, 3, 3, 3, 3)]
    assert any(len(set(m)) == 1 for m, _ in tc.RED_MAPS)
    B, M, P, C = tc.RED_BIG
    assert (M, B * P * C // 4 - tc.RED_CAP) == (1, 32)

    def exact(cv, case, smap=None):
        out, den = tc.reduce_ref(cv, case, smap)
        assert _pow2(den) and torch.equal(den.float().double(), den)
        assert bool(((out * 1024) == (out * 1024).round()).all()) and float(out.abs().max()) * 1024 < 2 ** 24
        assert torch.equal(out.float().double(), out)
        for dt in (torch.float16, torch.bfloat16):                                     # a 16-bit input map holds the same numbers
            assert torch.equal(cv.to(dt).float(), cv)
    for case in tc.reduce_cases():
        exact(tc.reduce_operands(case), case)
    for smap, confs in tc.RED_MAPS:
        case = tc.Red(2, len(smap), 5, 8)
        exact(tc.reduce_operands(case, confs), case, smap)


def test_reduce_mutations_change_the_reference():
    smap, confs = tc.RED_MAPS[-1]
    case = tc.Red(2, 7, 5, 8)
    cv = tc.reduce_operands(case, confs)
    ref, _ = tc.reduce_ref(cv, case, smap)
    for m in tc.RED_MUTATIONS:
        assert not torch.equal(tc.reduce_ref(cv, case, smap, m)[0], ref), m
    # a kernel that ignores the map reads every map once: a different answer unless the map is a permutation (the sums are exact)
    for smap, confs in tc.RED_MAPS:
        case = tc.Red(2, len(smap), 5, 8)
        cv = tc.reduce_operands(case, confs)
        assert torch.equal(tc.reduce_ref(cv, case, smap)[0], tc.reduce_ref(cv, case)[0]) == (len(set(smap)) == len(smap))


# ================================================================================================================== movers, gather
def test_mover_lists_pass_their_caps():
    assert len(tc.PERMS) == 24 and tc.PERM_SHAPES == [(3, 4, 5, 6), (3, 1, 5, 6)]
    assert int(np.prod(tc.PERM_BIG)) == 2097152 + 256 + 1 == tc.PERM_CAP + 257
    n, length, bank = tc.ROWS_BIG
    assert n * length // 4 > tc.ROWS_CAP and bank > n
    n, lens, bank = tc.MULTI_BIG
    assert n * max(lens) // 4 > tc.MULTI_CAP and bank > n and len(set(lens)) == 4 and all(v % 4 == 0 for v in lens)
    assert len(set(tc.scatter_rows(2050, 2100, 0).tolist())) == 2050
    assert len(set(tc.gather_rows(2050, 2100, 0).tolist())) < 2050
    base, view = tc.perm_source((3, 4, 5, 6), True)
    assert view.shape == (3, 4, 5, 6) and not view.is_contiguous() and view.storage_offset() > 0


def test_append_gather_list_and_mutation():
    a = tc.AG
    rows = a['bank_rows']
    assert rows == 24 and len(a['append']) == a['B'] == len(a['picks']) and all(len(p) == a['n_pick'] for p in a['picks'])
    assert {-1, rows, tc.INT32_MIN, tc.INT32_MAX} <= set(a['append'])
    flat = {r for p in a['picks'] for r in p}
    assert {-1, rows, rows + 1, tc.INT32_MIN, tc.INT32_MAX} <= flat
    both_out = [b for b in range(a['B']) if not 0 <= a['append'][b] < rows and a['append'][b] in a['picks'][b]]
    assert both_out == [1, 2, 3, 4]                                                    # pick == append_row, both out of range
    assert any(0 <= a['append'][b] < rows and a['append'][b] in a['picks'][b] for b in range(a['B']))
    fresh = [tc.rows_data(a['B'], n, 'fresh%d' % k) for k, n in enumerate(a['lens'])]
    banks = [tc.rows_data(rows, n, 'bank%d' % k) for k, n in enumerate(a['lens'])]
    after, picked = tc.ag_ref(fresh, banks)
    _, wrong = tc.ag_ref(fresh, banks, 'app_first')
    assert tc.AG_MUTATIONS == ['app_first'] and all(not torch.equal(p, q) for p, q in zip(picked, wrong))
    changed = {r for k in range(4) for r in range(rows) if not torch.equal(after[k][r], banks[k][r])}
    assert changed == {2, 21}
    nq = a['n_pick']
    for b in both_out:
        j = a['picks'][b].index(a['append'][b])
        assert all(not p[b * nq + j].any() for p in picked)
