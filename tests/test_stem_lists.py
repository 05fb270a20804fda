"""CPU: the lists of tests/stem_cases.py are the ones the stem and max-pool sweep was specified with and cover every tile residue they
are there for, their operands keep every partial sum an exact multiple of 1/16 below 2^24 / 16, the strip cases reach strips of 4, 2
and 1 by the launcher's own query, the fragment layouts unpack to the filters, and the float64 reference can tell a subtly wrong
kernel from a right one - the cap that keeps a later edit from thinning tests/test_gpu_stem_sweep.py into something a wrong kernel
would pass.  The strip query is host code of the library: nothing here needs a GPU."""
import pytest
import torch

import stem_cases as sc
from usot_amd import build
from usot_amd.engine import pack_stem_f32, pack_stem_lp


@pytest.fixture(scope='module', autouse=True)
def library():
    build.build(force=False)


def _lists():
    return {'rows': sc.row_cases(), 'cols': sc.col_cases(), 'corners': sc.corner_cases(), 'production': sc.production_cases(),
            'ind': sc.ind_cases(), 'strips': [c for c, _ in sc.strip_cases()]}


def test_the_lists_are_the_specified_ones():
    assert sc.ROWS == [(h, 30) for h in range(7, 46)] and len(sc.ROWS) == 39
    assert sc.COLS == [(18, w) for w in range(7, 77)] and len(sc.COLS) == 70
    assert sc.CORNERS == [(7, 7), (8, 8), (7, 76), (45, 7), (44, 75), (45, 76)]
    assert sc.PRODUCTION == [127, 255, 271]
    assert {c.N for c in sc.row_cases() + sc.col_cases()} == {2} and {c.N for c in sc.corner_cases()} == {3}
    assert {c.N for c in sc.production_cases()} == {1}
    assert len(sc.sweep_cases()) == 39 + 70 + 6 + 3 and len(set(sc.sweep_cases())) == 117      # (18, 30) is a row and a column
    assert len(sc.ind_cases()) == 3 and set(sc.IND) <= set(sc.ROWS + sc.COLS + sc.CORNERS)
    assert sc.MU == (-104.0, 117.0, -123.0)
    assert sc.MUTATIONS == ['pool_row', 'pool_col', 'tap_row', 'tap_col', 'channel', 'mu_pad', 'last_col', 'last_row', 'image',
                            'strip_stale']
    assert sc.POOL_HW == [(h, w) for h in range(1, 8) for w in range(1, 8)]
    assert (sc.POOL_C_F32, sc.POOL_C_LP, sc.POOL_BIG) == ([4, 64, 68], [8, 64, 72], (9, 121, 121, 256))
    assert [i for i, _ in sc.r_cases('conv')] == 'OH+1 OW+1 OH-1 OW-1 H6 W6 N0 N65536 y+4 w+4'.split()
    assert [i for i, _ in sc.r_cases('pool')] == 'OH+1 OW+1 OH-1 OW-1 H6 W6 N0 N65536 PH+1 PW+1 PH-1 PW-1 y+4 bias+4'.split()
    assert [i for i, _ in sc.r_cases('lp')] == ('OH+1 OW+1 OH-1 OW-1 H6 W6 N0 N65536 PH+1 PW+1 PH-1 PW-1 y+4 bias+4 w+4 dtype3 '
                                               'dtype-1').split()


def test_the_sweep_covers_every_tile_residue():
    """every PH mod 4 (fp32 and low-precision tiles are 4 pooled rows), PW mod 4 and PW mod 8 at one and at several tiles; every OH mod
    8 and OW mod 16 of the unfused stem's tile; both parities of H, W, OH, OW; H != W"""
    geo = [(c.H, c.W) + sc.out_hw(c.H, c.W) for c in sc.row_cases() + sc.col_cases() + sc.corner_cases()]
    for several in (False, True):
        assert {PH % 4 for _, _, _, _, PH, _ in geo if (PH > 4) == several} == set(range(4))
        assert {PW % 4 for _, _, _, _, _, PW in geo if (PW > 4) == several} == set(range(4))
        assert {PW % 8 for _, _, _, _, _, PW in geo if (PW > 8) == several} == set(range(8))
        assert {OH % 8 for _, _, OH, _, _, _ in geo if (OH > 8) == several} == set(range(8))
        assert {OW % 16 for _, _, _, OW, _, _ in geo if (OW > 16) == several} == set(range(16))
    assert {PH for _, _, _, _, PH, _ in geo} == set(range(1, 11)) and {PW for _, _, _, _, _, PW in geo} == set(range(1, 19))
    assert {OH for _, _, OH, _, _, _ in geo} == set(range(1, 21)) and {OW for _, _, _, OW, _, _ in geo} == set(range(1, 36))
    for k in range(4):                               # H, W, OH, OW
        assert {g[k] % 2 for g in geo} == {0, 1}
    assert {(g[2] % 2, g[3] % 2) for g in geo} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sum(H != W for H, W, _, _, _, _ in geo) >= 100 and any(H > W for H, W, _, _, _, _ in geo)
    # what the existing stem tests run, for the record: one residue class, OH odd, square
    old = [sc.out_hw(s, s) for s in (63, 64, 127, 255, 271)]
    assert {PH % 4 for _, _, PH, _ in old} == {3} and {OH % 2 for OH, _, _, _ in old} == {1}


def test_operands_are_exact():
    w, b = sc.filters()
    assert torch.equal(w, (w * 4).round() / 4) and float(w.abs().max()) == 1.0 and torch.equal(b, (b * 4).round() / 4)
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(w.float().to(dtype).double(), w)
    for mu in (sc.MU, sc.NO_MU):
        fb = sc.folded_bias(mu)
        assert torch.equal(fb.float().double(), fb) and torch.equal(fb, (fb * 4).round() / 4)
        assert sc.bound(mu) / sc.GRAIN < 2 ** 24 and sc.bound(mu) < 65504
    assert 30000 < sc.bound() < 45000                # the all-positive family: ~92 * 378.75 + the folded bias
    case = sc.Case(45, 76, 3, 3)
    x = sc.crops(case)
    assert x.dtype == torch.float32 and float(x.min()) == 0.0 and float(x.max()) == 255.75 and torch.equal(x, (x * 4).round() / 4)
    d = x - torch.tensor(sc.MU).view(1, 3, 1, 1)
    assert float(d.abs().max()) == sc.X_MAX
    assert torch.equal(d.to(torch.float16).float(), d)
    hi = d.to(torch.bfloat16).float()
    lo = (d - hi).to(torch.bfloat16).float()
    assert torch.equal(hi + lo, d)
    assert float((lo != 0).float().mean()) > 0.5     # the second MFMA chain of the bf16 kernel carries real data
    stem, pooled = sc.build(case)                    # asserts the 1/16 grain, the bound and fp32 exactness itself
    assert stem.shape == (3, 20, 35, 64) and pooled.shape == (3, 10, 18, 64)


def test_the_four_families():
    w, b = sc.filters()
    neg, pos, mixed, single = w[0::4], w[1::4], w[2::4], w[3::4]
    assert float(neg.max()) == 0.0 and (neg[:, [0, 2], 6, :] < 0).all() and (neg[:, [0, 2], :, 6] < 0).all()
    assert (b[0::4] == 4096).all() and float(neg.abs().sum((1, 2, 3)).max()) * 255.75 < 4096
    assert float(pos.min()) == 0.25 and float(pos.max()) == 1.0
    assert float(mixed.min()) == -1.0 and float(mixed.max()) == 1.0 and len(set(b[2::4].tolist())) == 16
    assert (single.sum((1, 2, 3)) == 1).all() and (single.abs().sum((1, 2, 3)) == 1).all() and (b[3::4] == 128).all()
    assert len(set(sc.SINGLE_TAPS)) == 16
    for ci in range(3):
        assert {(kh, kw) for c, kh, kw in sc.SINGLE_TAPS if c == ci} >= {(0, 0), (0, 6), (6, 0), (6, 6), (3, 3)}
    case = sc.Case(18, 37, 2, 2)
    stem, _ = sc.build(case)
    x = sc.crops(case).double()
    OH, OW, _, _ = sc.out_hw(18, 37)
    assert float(stem[..., 0::4].min()) > 0                      # the negative family never meets the ReLU
    assert float((stem[..., 2::4] == 0).double().mean()) > 0.1   # the mixed family does
    for k, (ci, kh, kw) in enumerate(sc.SINGLE_TAPS):            # the crop itself at a known offset
        assert torch.equal(stem[..., 4 * k + 3], x[:, ci, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] + 128)


def test_strip_cases_reach_four_two_and_one():
    got = []
    for case, why in sc.strip_cases():
        OH, OW, PH, PW = sc.out_hw(case.H, case.W)
        tx, ty = sc.tiles(PH, PW)
        got.append((case.H, case.W, case.N, PH, PW, tx, ty, sc.case_strip(case)))
    assert got == [(21, 153, 768, 4, 37, 5, 1, 4), (21, 153, 767, 4, 37, 5, 1, 2), (39, 175, 256, 9, 43, 6, 3, 4),
                   (18, 76, 2, 3, 18, 3, 1, 1)]
    assert all(tx % s for _, _, _, _, _, tx, _, s in got[:3])    # a ragged last workgroup at strip 4 (twice) and at strip 2
    assert all(PW % 8 for _, _, _, _, PW, _, _, _ in got[:3])    # ... whose last tile is ragged itself
    # 255 fewer images do not reach strip 4 on the tall shape; every geometry of the sweep runs strip 1
    assert sc.strip_of(255, 9, 43) == 2 and sc.fewest_images(sc.STRIP_TALL, 4) == 256
    assert {sc.case_strip(c) for c in sc.sweep_cases()} == {1}
    # the largest case of test_gpu_ops.py::test_stem_pool_lp and the batch-64 bf16 backbone
    assert sc.strip_of(9, 63, 63) == 1 and sc.strip_of(64, 63, 63) == 4
    assert [sc.strip_of(*a) for a in ((0, 4, 8), (1, 0, 8), (1, 4, 0))] == [0, 0, 0]
    for case, _ in sc.strip_cases():
        idx = sc.index(case)
        assert idx.shape == (case.N,) and set(idx.tolist()) == set(range(case.B))


def test_pool_lists():
    N, H, W, C = sc.POOL_BIG
    quads = lambda n: n * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4)
    assert quads(N) == 2143296 > sc.POOL_CAP == 2097152 > quads(N - 1)
    x = sc.pool_input(3, 5, 7, 8)
    assert float(x.min()) < 0 and torch.equal(x, x.to(torch.bfloat16).float()) and torch.equal(x, x.half().float())
    assert set(x[1, 0, :, 1:].reshape(-1).tolist()) == {-3.0} and len(set(x[0, 0].reshape(-1).tolist())) > 1
    assert set(x[:, :, -1, 0].reshape(-1).tolist()) == {-31.5}
    assert torch.isfinite(x).all()
    ref = sc.pool64(x)
    assert ref.shape == (3, 3, 4, 8)
    for oy in range(3):                              # the definition, spelled out
        for ox in range(4):
            win = x[:, max(2 * oy - 1, 0):2 * oy + 2, max(2 * ox - 1, 0):2 * ox + 2].double()
            assert torch.equal(ref[:, oy, ox], win.amax((1, 2)))


def test_fragment_layouts_unpack_to_the_filters():
    """engine.pack_stem_f32 / pack_stem_lp against the lane layout the kernels read (csrc/stem_pool.hip, csrc/conv_bf16.hip)"""
    bank = sc.packed()
    w, _ = sc.filters()
    assert torch.equal(bank.reshape(3, 7, 7, 64).permute(3, 0, 1, 2).double(), w)
    got, zeros = sc.unpack_f32(pack_stem_f32(bank))
    assert torch.equal(got, bank) and zeros.numel() == (3 * 8 + 21) * 64 and not zeros.any()
    for dtype in (torch.bfloat16, torch.float16):
        frag = pack_stem_lp(bank, dtype)
        assert frag.dtype == dtype and frag.shape == (4, 6, 64, 8)
        got, zeros = sc.unpack_lp(frag)
        assert torch.equal(got, bank) and not zeros.any()


@pytest.mark.parametrize('mut', sc.MUTATIONS)
def test_reference_tells_a_wrong_kernel(mut):
    """on every case where the mistake is meaningful the mutated pooled reference differs from the true one (in fp32 and after the
    bf16 rounding of a 16-bit output); where it is not, it is the same; and every list has a case where it is meaningful"""
    for name, cases in _lists().items():
        hit = 0
        for case in cases:
            _, true = sc.build(case)
            for mu in (sc.MU, sc.NO_MU) if mut in ('pool_row', 'pool_col') else (sc.MU,):
                _, wrong = sc.ref64(case, mut, mu)
                want, got = true, wrong              # the base images' maps: every one of them is in the batch
                if mut == 'image':
                    want, got = sc.expected(case, true), sc.expected(case, wrong, mut)
                if sc.meaningful(mut, case):
                    assert not torch.equal(got, want), (mut, case, mu)
                    assert not torch.equal(sc.stored(got, torch.bfloat16), sc.stored(want, torch.bfloat16)), (mut, case, mu)
                    hit += 1
                else:
                    assert torch.equal(got, want), (mut, case, mu)
        if mut == 'strip_stale':
            assert (hit == 3) == (name == 'strips') and (hit == 0) == (name != 'strips'), (name, hit)
        elif mut == 'image':
            assert hit == sum(c.N > 1 for c in cases), (name, hit)
        else:                                        # OH is 6 in every column case, OW 12 in every row case
            assert (hit == 0) == ((mut, name) in (('pool_row', 'cols'), ('pool_col', 'rows'))), (mut, name, hit)


def test_stem_mutations_show_in_the_stem_map_too():
    """the mutations that are not the pool's change the unfused stem's map on every case"""
    for case in sc.corner_cases() + sc.ind_cases():
        true, _ = sc.build(case)
        for mut in ('tap_row', 'tap_col', 'channel', 'last_col', 'last_row', 'image'):
            assert not torch.equal(sc.ref64(case, mut)[0], true), (mut, case)
