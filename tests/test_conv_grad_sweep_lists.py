"""CPU: the lists of tests/conv_grad_sweep_cases.py are the ones the convolution-gradient sweep was specified with (counts, residue sets,
every named configuration), their operands keep every `==` of tests/test_gpu_conv_grad_sweep.py a fact about integers below 2^24, the
int64 reference is the operator's definition (float64 torch autograd through F.conv2d; the rotate-and-transpose identity of route A on
rectangular filters), every listed mutation - a plausible wrong kernel - changes the reference on the list it targets, and route_a
answers what the launcher's route query answers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conv_grad_cases as cg
import conv_grad_sweep_cases as sc
from usot_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 16                                               # an address that is never dereferenced by the host-only route query

# the counts the GPU items print (tests/test_gpu_conv_grad_sweep.py)
COUNTS = {'M_SWEEP': 97, 'M_SWEEP pairs': 382, 'COUT_SWEEP': 132, 'COUT_ROUTE_B': 264, 'K_SWEEP': 32, 'GEOMETRY': 1936, 'BIG': 2,
          'GEOMETRY by stride': {1: 1148, 2: 468, 3: 320}, 'UNREACHED': 334, 'GEOMETRY route A': 690, 'K_SWEEP route A': 32}


def test_the_lists_are_the_specified_ones():
    bco, bkk, chunk = sc.BCO, sc.BKK, sc.CHUNK
    try:
        assert hip.wgrad_geometry() == (bco, bkk, chunk)
    except hip.HipError:
        pass                                           # not built: the constants of the source (conv_grad_sweep_cases._wgrad_geometry)
    # M_SWEEP: a 1x1 convolution of a 1 x M map, 32 -> 64, every M up to three chunks and one; psplit 1, and 2, 3, M where <= M
    assert [c for c, _ in sc.M_SWEEP] == [(1, 1, m, 32, 64, 1, 1, 1, (0, 0), (1, 1)) for m in range(1, 3 * chunk + 2)]
    assert all(sc.pixels(c) == c[2] for c, _ in sc.M_SWEEP)
    for c, listed in sc.M_SWEEP:
        m = c[2]
        assert set(listed) == {ps for ps in (1, 2, 3, m) if ps <= m}, c
    assert len(sc.M_SWEEP) == COUNTS['M_SWEEP'] and len(sc.pairs(sc.M_SWEEP)) == COUNTS['M_SWEEP pairs']
    assert {(c[2] // chunk, c[2] % chunk) for c, _ in sc.M_SWEEP} >= {(q, r) for q in range(3) for r in range(chunk)} - {(0, 0)}
    assert all(c[3] % bkk == 0 and c[4] == bco for c, _ in sc.M_SWEEP)
    # COUT_SWEEP: M = 33, every Cout through two channel blocks and a bit: both dy loader paths in full
    assert [c for c, _ in sc.COUT_SWEEP] == [(1, 3, 11, 32, co, 1, 1, 1, (0, 0), (1, 1)) for co in range(1, 2 * bco + 5)]
    assert all(listed == (1, 2) and sc.pixels(c) == 33 for c, listed in sc.COUT_SWEEP)
    couts = {c[4] for c, _ in sc.COUT_SWEEP}
    assert {co for co in couts if co % 4} and {co for co in couts if co % 4 == 0} >= {16, 32, 48, bco, 2 * bco}
    assert {bco + 1, 2 * bco + 1} <= couts and any(co % 4 and co > bco for co in couts)      # db for co0 > 0 on the scalar path
    assert sc.COUT_ROUTE_B == [(1, 3, 11, cin, co, 1, 1, 1, (0, 0), (1, 1)) for cin in (32, 64) for co in range(1, 2 * bco + 5)]
    assert len(sc.COUT_SWEEP) == COUNTS['COUT_SWEEP'] and len(sc.COUT_ROUTE_B) == COUNTS['COUT_ROUTE_B']
    # K_SWEEP
    assert sc.K_CIN == (32, 64, 96, 160) and sc.K_FILTERS == ((1, 1), (3, 3), (1, 3), (3, 1), (2, 2), (2, 3), (5, 5), (7, 7))
    assert sc.K_SWEEP == [(2, 9, 8, cin, 32, kh, kw, 1, ((kh - 1) // 2, (kw - 1) // 2), (1, 1)) for cin in sc.K_CIN for kh, kw in sc.K_FILTERS]
    assert len(sc.K_SWEEP) == COUNTS['K_SWEEP'] and all(cg.route_a(c) for c in sc.K_SWEEP)
    assert any(c[3] // bkk == 3 for c in sc.K_SWEEP) and any(c[5] != c[6] for c in sc.K_SWEEP)
    # BIG: both grid-stride loops go round twice, and the second round is a partial one
    rb, pk = sc.BIG['route_b'], sc.BIG['pack']
    assert rb[3:7] == (1024, 1, 1, 1) and rb[0] * rb[1] * rb[2] == sc.DGRAD_CAP + 37 and not cg.route_a(rb)
    threads = rb[0] * rb[1] * rb[2] * rb[3] // 4
    assert sc.DGRAD_CAP * 256 < threads < 2 * sc.DGRAD_CAP * 256
    assert pk[3:7] == (512, 520, 3, 3)
    assert sc.PACK_CAP * 256 < pk[3] * pk[4] * 9 < 2 * sc.PACK_CAP * 256
    with open(os.path.join(ROOT, 'usot_amd', 'csrc', 'conv_grad.hip')) as f:
        text = f.read()
    assert re.search(r'blocks > %d \? %d : blocks\)\), dim3\(256\), 0, \(hipStream_t\)stream, p\)' % (sc.DGRAD_CAP, sc.DGRAD_CAP), text)
    assert re.search(r'blocks > %d \? %d : blocks\)\), dim3\(256\), 0, \(hipStream_t\)stream,\s*w, wt' % (sc.PACK_CAP, sc.PACK_CAP), text)
    assert len(sc.BIG) == COUNTS['BIG']
    assert list(sc.MUTATIONS) == ['no_rotate', 'swap_khkw', 'swap_pad', 'swap_dil', 'tap_of_32', 'drop_last_pixel', 'slice_overlap',
                                  'stride_floor', 'cout_block', 'one_pass']
    assert len(sc.PYTHON_SURFACE) == 6 and sum(c[5] != c[6] for c in sc.PYTHON_SURFACE) >= 2 and any(c[3] == 96 for c in sc.PYTHON_SURFACE)


NAMED = [(3, 3, 1, (0, 0), (1, 1)), (3, 3, 1, (1, 1), (1, 1)), (3, 3, 1, (2, 2), (2, 2)), (3, 3, 1, (0, 0), (2, 1)), (3, 3, 1, (0, 0), (1, 2)),
         (3, 3, 1, (2, 2), (1, 1)), (3, 3, 1, (3, 3), (1, 1)), (1, 1, 1, (1, 1), (1, 1)), (1, 3, 1, (0, 1), (1, 1)), (3, 1, 1, (1, 0), (1, 1)),
         (2, 2, 1, (0, 0), (1, 1)), (2, 2, 2, (1, 1), (1, 1)), (3, 3, 2, (0, 0), (1, 1)), (3, 3, 2, (1, 1), (1, 1)), (3, 3, 2, (1, 0), (2, 1)),
         (3, 3, 3, (1, 1), (1, 1)), (1, 1, 2, (0, 0), (1, 1)), (1, 1, 3, (0, 0), (1, 1)), (5, 5, 1, (2, 2), (1, 1))]


def test_geometry_list():
    assert sc.CONFIGS[:len(NAMED)] == NAMED and len(set(sc.CONFIGS)) == len(sc.CONFIGS)
    maps = [(n, h, w) for n in (1, 2) for h in range(1, 6) for w in range(1, 10)]
    want = [(n, h, w, cin, cout) + cfg for n, h, w in maps for cfg in sc.CONFIGS for cin, cout in ((32, 32), (64, 40))
            if cin == 32 or w in (1, 4, 9)]
    want = [c for c in want if min(sc.out_hw(c)) >= 1 and sc.valid(c)]
    assert sc.GEOMETRY == want and len(set(want)) == len(want) == COUNTS['GEOMETRY']
    assert {s: sum(c[7] == s for c in sc.GEOMETRY) for s in (1, 2, 3)} == COUNTS['GEOMETRY by stride']       # one GPU item per stride
    assert {sc.config(c) for c in sc.GEOMETRY} == set(sc.CONFIGS)                      # every configuration fits some map
    assert sum(cg.route_a(c) for c in sc.GEOMETRY) == COUNTS['GEOMETRY route A']
    # pad' = dil*(k-1) - pad of the named route-A configurations: 0 .. 4 per axis, and the two that have none
    padp = {(c[9][0] * (c[5] - 1) - c[8][0], c[9][1] * (c[6] - 1) - c[8][1]) for c in sc.GEOMETRY if cg.route_a(c)}
    assert {(2, 2), (1, 1), (4, 2), (2, 4), (0, 0), (0, 1), (1, 0)} <= padp and all(min(p) >= 0 for p in padp)
    assert sc.ROUTE_B_ONLY_CONFIGS == [cfg for cfg in sc.CONFIGS if cfg[2] > 1 or cfg[4][0] * (cfg[0] - 1) < cfg[3][0]
                                       or cfg[4][1] * (cfg[1] - 1) < cfg[3][1]]
    for s in (2, 3):                     # every residue of the floor in OH = (H + 2 ph - dh (KH - 1) - 1) / stride + 1, both axes
        strided = [c for c in sc.GEOMETRY if c[7] == s]
        assert {(c[1] + 2 * c[8][0] - c[9][0] * (c[5] - 1) - 1) % s for c in strided} == set(range(s))
        assert {(c[2] + 2 * c[8][1] - c[9][1] * (c[6] - 1) - 1) % s for c in strided} == set(range(s))
        for cfg in {sc.config(c) for c in strided}:                                        # ... of every strided configuration
            assert {((c[1] + 2 * c[8][0] - c[9][0] * (c[5] - 1) - 1) % s, (c[2] + 2 * c[8][1] - c[9][1] * (c[6] - 1) - 1) % s)
                    for c in strided if sc.config(c) == cfg} == {(a, b) for a in range(s) for b in range(s)}, cfg
    assert any(sc.out_hw(c)[0] > c[1] and sc.out_hw(c)[1] > c[2] for c in sc.GEOMETRY)
    assert any(sc.straddles(c) for c in sc.GEOMETRY) and any(sc.pixels(c) > sc.CHUNK and sc.straddles(c) for c in sc.GEOMETRY)
    assert any(not sc.reached(c).any(1).all() for c in sc.GEOMETRY)                        # a row of x no tap reaches
    assert {sc.pixels(c) for c in sc.GEOMETRY} >= {1, 2}


def test_unreached_list():
    assert sc.UNREACHED == [c for c in sc.GEOMETRY if c[3] == 32 and c[7] > 1 and c[5:7] in ((1, 1), (2, 2))]
    assert len(sc.UNREACHED) == COUNTS['UNREACHED']
    holes = {}
    for c in sc.UNREACHED:
        r = sc.reached(c)
        holes.setdefault(sc.config(c), []).append(int((~r).sum()))
        # reached() against the definition, pixel by pixel and tap by tap
        n, h, w, cin, cout, kh, kw, s, pad, dil = c
        oh, ow = sc.out_hw(c)
        slow = np.zeros((h, w), bool)
        for o in range(oh):
            for p in range(ow):
                for a in range(kh):
                    for b in range(kw):
                        i, j = o * s - pad[0] + a * dil[0], p * s - pad[1] + b * dil[1]
                        if 0 <= i < h and 0 <= j < w:
                            slow[i, j] = True
        assert np.array_equal(r, slow), c
    assert set(holes) == set(sc.UNREACHED_CONFIGS)
    for cfg in ((1, 1, 2, (0, 0), (1, 1)), (1, 1, 3, (0, 0), (1, 1)), (2, 2, 3, (0, 0), (1, 1))):
        assert max(holes[cfg]) > 0, cfg
    assert max(holes[(2, 2, 2, (1, 1), (1, 1))]) == 0          # reaches every pixel: why (2, 2, 3, ..) was added to CONFIGS


def test_every_partial_sum_stays_below_2_to_the_24():
    """the condition that makes `==` legitimate: the sum of the absolute values of the terms bounds every partial sum in any order"""
    for fam in sc.FAMILIES:
        for c in sc.all_cases():
            for kind in 'wx':
                if sc.applies(c, fam, kind):
                    assert sc.bound(c, fam, kind) < 2 ** 24, (c, fam, kind)
            assert sc.bound(c, fam) < 2 ** 24
    assert sc.bound((1, 1, 2048, 32, 64, 1, 1, 1, (0, 0), (1, 1)), 'wide', 'w') == 2048 * 4095 < 2 ** 24
    assert not sc.applies((1, 1, 2049, 32, 64, 1, 1, 1, (0, 0), (1, 1)), 'wide', 'w')
    assert not sc.applies((1, 1, 1, 32, 2049, 1, 1, 1, (0, 0), (1, 1)), 'wide', 'x')
    # the operands are what bound() assumes, and the wide ones need their thirteen bits
    for c in (sc.K_SWEEP[9], sc.GEOMETRY[700]):
        for name in ('x', 'w', 'dy'):
            assert np.abs(sc.operand(c, 'small', name)).max() == 3
        assert np.abs(sc.operand(c, 'wide', 'dy')).max() == 1
        for name in ('x', 'w'):
            v = sc.operand(c, 'wide', name)
            assert 2048 < np.abs(v).max() <= 4095
            f = torch.tensor(v).float()
            assert not torch.equal(f.bfloat16().float(), f) and not torch.equal(f.half().float(), f)
    # on the sweep's own operands the references stay inside the bound
    for c in sc.K_SWEEP:
        for fam in sc.FAMILIES:
            dw, db = sc.reference_w(c, fam)
            assert max(np.abs(dw).max(), np.abs(db).max()) <= sc.bound(c, fam, 'w')
            assert np.abs(sc.reference_x(c, fam)).max() <= sc.bound(c, fam, 'x')


def oihw(c, w):
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    return torch.from_numpy(w.reshape(cout, kh, kw, cin).transpose(0, 3, 1, 2).copy()).double()


def autograd(c, x, w, dy):
    """conv_grad_cases.ref_grads_of on the kernels' layouts -> (dx NHWC, dw packed, db) as float64 numpy"""
    nchw = lambda a: torch.from_numpy(a.transpose(0, 3, 1, 2).copy()).double()
    rx, rw, rb = cg.ref_grads_of(nchw(x), oihw(c, w), torch.zeros(c[4], dtype=torch.float64), nchw(dy), c[7], c[8], c[9])
    return cg.nhwc(rx).numpy(), cg.pack(rw).numpy(), rb.numpy()


def thinned_rest():
    rest = [c for c, _ in sc.M_SWEEP] + [c for c, _ in sc.COUT_SWEEP] + sc.COUT_ROUTE_B + list(sc.BIG.values())
    return rest[::10] + list(sc.BIG.values())


@pytest.mark.parametrize('which', ['K_SWEEP', 'GEOMETRY', 'rest'])
def test_int64_reference_equals_float64_autograd(which):
    cases = thinned_rest() if which == 'rest' else getattr(sc, which)
    fams = sc.FAMILIES if which != 'GEOMETRY' else ('small',)
    bad = []
    for c in cases:
        for fam in fams:
            x, w, dy = (sc.operand(c, fam, name) for name in ('x', 'w', 'dy'))
            rx, rw, rb = autograd(c, x, w, dy)                       # integers far below 2^53: float64 is exact as well
            (dw, db), dx = sc.reference_w(c, fam), sc.reference_x(c, fam)
            if not (np.array_equal(dx, rx) and np.array_equal(dw, rw) and np.array_equal(db, rb)):
                bad.append((c, fam))
    assert not bad, bad[:10]


def test_rotated_bank_through_the_forward_definition_is_the_data_gradient():
    """at stride 1, dx = conv(dy, ref_pack(w)) at pad' = dil*(k-1) - pad: the identity of test_conv_grad_host.py, on rectangular filters"""
    cases = sc.K_SWEEP + [c for c in sc.GEOMETRY if cg.route_a(c)][::5]
    assert any(c[5] != c[6] for c in cases) and any(c[9][0] != c[9][1] for c in cases)
    for c in cases:
        n, h, w_, cin, cout, kh, kw, s, pad, dil = c
        w, dy = sc.operand(c, 'small', 'w'), sc.operand(c, 'small', 'dy')
        padp = (dil[0] * (kh - 1) - pad[0], dil[1] * (kw - 1) - pad[1])
        got = sc.ref_forward(dy, sc.ref_pack(c, w), kh, kw, 1, padp, dil)
        assert np.array_equal(got, sc.reference_x(c, 'small')), c
    # ref_pack is the header's formula (2), element by element
    c = sc.K_SWEEP[5]                                               # 32 -> 32, 2 x 3
    n, h, w_, cin, cout, kh, kw, s, pad, dil = c
    w = sc.random_bank(c)
    wt = sc.ref_pack(c, w)
    assert wt.shape == (cin, kh * kw * cout) and wt.dtype == np.float32
    for ci in (0, 7, 31):
        for a in range(kh):
            for b in range(kw):
                for co in (0, 5, 31):
                    assert wt[ci, (a * kw + b) * cout + co] == w[co, ((kh - 1 - a) * kw + (kw - 1 - b)) * cin + ci]


def truth(c, fam, key):
    if key == 'pack':
        return sc.ref_pack(c, sc.random_bank(c))
    return sc.reference_x(c, fam) if key == 'dx' else sc.reference_w(c, fam)[key == 'db']


def differs(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return a.shape != b.shape or not np.array_equal(a, b)                # a NaN (an element left unwritten) differs


@pytest.mark.parametrize('name', list(sc.MUTATIONS))
def test_every_mutation_changes_the_reference_on_its_list(name):
    """a mutation that no entry distinguishes would mean the list has a hole"""
    list_name, keys = sc.MUTATIONS[name]
    fams = sc.FAMILIES if list_name != 'GEOMETRY' else ('small',)
    for fam in fams:
        seen = dict.fromkeys(keys, 0)
        for c, ps in sc.targets(list_name):
            for key, wrong in sc.mutate(name, c, fam, ps).items():
                seen[key] += differs(wrong, truth(c, fam, key))
        print(name, fam, seen)
        assert all(seen.values()), (name, fam, seen)


def test_mutation_handles_are_neutral_when_unused():
    """the keywords the mutations turn are the reference's own parameters: with the true values they change nothing"""
    for c in (sc.K_SWEEP[13], sc.K_SWEEP[21], sc.GEOMETRY[1234]):
        n, h, w_, cin, cout, kh, kw, s, pad, dil = c
        x, w, dy = (sc.operand(c, 'small', name) for name in ('x', 'w', 'dy'))
        true_tap = lambda k0: divmod(k0 // cin, kw) + (k0 % cin,)
        assert np.array_equal(sc.ref_dw(c, x, dy, weight=np.ones(sc.pixels(c)), tap_of=true_tap, pad=pad, dil=dil), sc.reference_w(c, 'small')[0])
        assert np.array_equal(sc.ref_dx(c, w, dy, tap_index=lambda a, b: a * kw + b, pad=pad, dil=dil, couts=cout), sc.reference_x(c, 'small'))
    assert sc.slice_starts(7, 3) == [0, 2, 4] and sc.slice_starts(97, 2) == [0, 48]


def test_route_a_predicate_is_the_launchers():
    """host-only query; every case of every list, at route 0 with a rotated bank, without one, and with route 1 or 2 asked for"""
    try:
        L = hip.lib()
    except hip.HipError:
        pytest.skip('the library is not built')
    n_a = 0
    for c in sc.all_cases():
        n, h, w, cin, cout, kh, kw, s, pad, dil = c
        geo = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=kh, KW=kw, stride=s, pad=pad, dil=dil, dy=ONE, w=ONE, dx=ONE)
        q = lambda **kw_: L.usot_conv2d_dgrad_route(ctypes.byref(hip.grad_desc(**dict(geo, **kw_))))
        a = cg.route_a(c)
        n_a += a
        assert q(wt=ONE) == (1 if a else 2), c
        assert q(wt=ONE, route=1) == (1 if a else -1), c
        assert q(wt=ONE, route=2) == 2 and q() == 2 and q(route=1) == -1, c
    assert n_a >= COUNTS['GEOMETRY route A'] + COUNTS['K_SWEEP route A']
    # the nine-field cases of conv_grad_cases.py still get the same answer
    assert [cg.route_a(c) for c in cg.RAW] == [cg.route_a(c[:5] + (c[5],) + c[5:]) for c in cg.RAW]
