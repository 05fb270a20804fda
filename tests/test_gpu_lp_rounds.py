"""GPU: what a PERSISTENT workgroup of the batched low-precision backbone does when it finishes one unit of work and starts
the next.  Seven entry points launch min(units, CUs) workgroups and loop `unit += gridDim.x`, carrying LDS ring slots,
double-buffered halo tiles, counted s_waitcnt vmcnt(n) and barriers that exist only when there is a next unit; the other parity
and memory-contract tests stop just below the CU count, where every workgroup runs exactly one unit.

Method - a small verified problem, replicated without becoming periodic:
  * a BASE problem that every workgroup finishes in one round (the full-wait paths) is held to float64 at the bar its entry
    point has in tests/test_gpu_memory_contract.py;
  * the BIG problem is gathered from base rows ON THE DEVICE with a seeded index.  Pointwise kernels (unit = BM rows): big row
    m is base row BM * rho(m) + (m mod BM), rho(m) drawn per row from the base's >= 16 panels - the position inside the unit is
    kept, every big unit is another mixture of base rows, the residual follows the same index.  Spatial kernels (halo, bneck):
    big image n is base image rho(n) of >= 8, consecutive big images never the same one;
  * a row (an image) depends on its own inputs only, its position in the unit is unchanged, tile form and k order are the
    same: the WHOLE big output must be BIT-equal to y_base[index] (stale data of a previous unit cannot hide: neighbouring units
    hold other base rows), and a second launch on the same buffers bit-equal to the first.
Unit counts, from the device's CU count (the launchers read the same property): G + 1 full units and a ragged one (one
workgroup takes a second unit while the others exit) and 2 G + 1 and a ragged one (a third round: ring / slot parity is back at
its first value).  Every input goes through the guarded `put`, every output is NaN-prefilled between canaries.

The shape choosers are plain functions of the CU count; tests/test_lp_round_lists.py holds them to the launchers' rules."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_gpu_memory_contract import LP, _conv_pw_inputs, contract, dt_of, lp_err, no_nan, ulp_of  # noqa: E402
from test_gpu_ops import rel_err  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
ROUNDS = (2, 3)                                  # G + 1 (+ ragged) units, 2 G + 1 (+ ragged) units
TAIL = {2: 19, 3: 37}                            # rows of the last unit: rows missing in one wave | whole waves empty
BASE_PANELS = 16                                 # base units of the pointwise kernels
BASE_IMAGES = 8                                  # base images of the spatial kernels
PANEL_LARGE_MIN = 192                            # usot_pw_panel_lp: fewer panels of 256 pixels run on panels of 128

PANEL_SHAPES = ((256, 1024), (128, 512))
PANEL_PAIR_SHAPES = ((128, 512, 128), (128, 512, 256), (64, 256, 64), (64, 256, 128))
PANEL_PAIR_PIXELS = {(128, 512, 128): 256, (128, 512, 256): 128, (64, 256, 64): 256, (64, 256, 128): 256}
PW_PAIR_SHAPES = ((256, 1024, 256), (128, 512, 128), (64, 256, 64))
HALO_W, HALO_HS, HALO_TILE = 47, (33, 38, 43, 48), 16
BNECK_H, BNECK_W, BNECK_TH, BNECK_TW = 15, 31, 8, 16


# ------------------------------------------------------------------------------------------------------ shape choosers
def pointwise_m(G, bm, rounds, tail):
    """(rounds - 1) G + 1 full units of bm rows and a last unit of `tail` rows"""
    return ((rounds - 1) * G + 1) * bm + tail


def kstream_case(cus, rounds):
    G, bm = cus, 256
    U = (rounds - 1) * G + 2
    return dict(G=G, bm=bm, M=U * 256 - 256 + 37, base_m=BASE_PANELS * bm, skip=None)


def panel_large_case(cus, rounds):
    """usot_pw_panel_lp at 256 -> 1024 and 128 -> 512 on panels of 256 pixels: base and big on the two-blocks-per-wave form"""
    G, bm = cus, 256
    M = pointwise_m(G, bm, rounds, TAIL[rounds])
    skip = None
    if -(-M // 256) < PANEL_LARGE_MIN:
        skip = '%d CUs: %d panels of 256 pixels run on the 128-pixel form' % (cus, -(-M // 256))
    elif cus < PANEL_LARGE_MIN:
        skip = '%d CUs: the smallest base on the 256-pixel form (%d panels) takes two rounds' % (cus, PANEL_LARGE_MIN)
    return dict(G=G, bm=bm, M=M, base_m=PANEL_LARGE_MIN * bm, skip=skip)


def panel_small_case(cus):
    """... on panels of 128 pixels (fewer than 192 panels of 256): G + 1 panels and 77 rows"""
    G, bm = cus, 128
    M = 128 * cus + 128 + 77
    skip = None if -(-M // 256) < PANEL_LARGE_MIN else '%d CUs: a second round of 128-pixel panels needs %d >= 192 panels of 256' % (cus, -(-M // 256))
    return dict(G=G, bm=bm, M=M, base_m=BASE_PANELS * bm, skip=skip)


def panel_k64_case(cus):
    """usot_pw_panel_lp at 64 -> 256: panels of 512 pixels, 2 G + 1 of them and a ragged one"""
    G, bm = cus, 512
    return dict(G=G, bm=bm, M=pointwise_m(G, bm, 3, TAIL[3]), base_m=BASE_PANELS * bm, skip=None)


def panel_pair_case(cus, shape, rounds, bm=None):
    G, bm = cus, bm or PANEL_PAIR_PIXELS[shape]
    return dict(G=G, bm=bm, M=pointwise_m(G, bm, rounds, TAIL[rounds]), base_m=BASE_PANELS * bm, skip=None)


def pw_pair_wgs_per_cu(cm, co):
    """usot_pw_pair_lp: one workgroup per CU when its LDS image (64 rows of t2 and of Y) exceeds 48 KiB, else two"""
    return 1 if 64 * (cm + co) * 2 > 48 * 1024 else 2


def pw_pair_case(cus, shape):
    """4 CUs + 1 tiles of 64 rows and a ragged one: five rounds at one workgroup per CU, three at two"""
    cm, co, _ = shape
    G, bm = cus * pw_pair_wgs_per_cu(cm, co), 64
    return dict(G=G, bm=bm, M=(4 * cus + 1) * bm + 37, base_m=BASE_PANELS * bm, skip=None)


def halo_case(cus, rounds, H):
    """images of 3 x 3 tiles of 16 x 16 (W = 47; H = 33, 38, 43, 48: a bottom tile row of 1, 6, 11, 16 rows)"""
    G = cus
    tpi = -(-H // HALO_TILE) * -(-HALO_W // HALO_TILE)
    U = (rounds - 1) * G + 2
    N = -(-U // tpi)
    skip = None if BASE_IMAGES * tpi <= cus else '%d CUs: the base of %d images (%d tiles) takes two rounds' % (cus, BASE_IMAGES, BASE_IMAGES * tpi)
    return dict(G=G, N=N, H=H, W=HALO_W, tpi=tpi, ntiles=N * tpi, base_n=BASE_IMAGES, skip=skip)


def halo_stores_prev(H):
    """the values `stores_prev` of conv3x3_halo_kernel takes on an image of height H: rows of a wave's row quarter inside the image"""
    return {min(4, max(0, H - (ty * HALO_TILE + rq * 4))) for ty in range(-(-H // HALO_TILE)) for rq in range(4)}


def bneck_case(cus, rounds):
    """images of 15 x 31 (2 x 2 tiles of 8 x 16, 7-row bottom tiles): G + 4 | 2 G + 4 tiles, never a multiple of 8"""
    G = cus & ~7
    tpi = -(-BNECK_H // BNECK_TH) * -(-BNECK_W // BNECK_TW)
    N = (rounds - 1) * G // tpi + 1
    skip = None if BASE_IMAGES * tpi <= G else '%d CUs: the base of %d tiles takes two rounds' % (cus, BASE_IMAGES * tpi)
    return dict(G=G, N=N, H=BNECK_H, W=BNECK_W, tpi=tpi, ntiles=N * tpi, base_n=BASE_IMAGES, skip=skip)


def bneck_walk(tile, G):
    """(round, workgroup) of a tile in the XCD-grouped walk of the bneck kernels: tile_of(k) of block b = (8 k + (b & 7)) G / 8 + (b >> 3)"""
    g8 = G // 8
    kx, j = divmod(int(tile), g8)
    k, x = divmod(kx, 8)
    return k, j * 8 + x


def plain_walk(unit, G):
    return int(unit) // G, int(unit) % G


def row_index(M, bm, panels, seed):
    """big row m <- base row bm * rho(m) + (m mod bm), rho(m) seeded, per row"""
    g = torch.Generator().manual_seed(seed)
    rho = torch.randint(0, panels, (M,), generator=g)
    return bm * rho + torch.arange(M) % bm


def image_index(N, images, seed):
    """big image n <- base image rho(n); rho(n) != rho(n - 1)"""
    g = torch.Generator().manual_seed(seed)
    step = torch.randint(1, images, (N,), generator=g)
    return torch.cumsum(step, 0) % images


# ------------------------------------------------------------------------------------------------------ mismatch reporter
def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous()


def mismatch(got, want, locate, G, walk=plain_walk, what='y'):
    """None when `got` and `want` ([rows][C], any device) are bit-equal; else one line naming the number of wrong elements, the
    first wrong unit, its round and workgroup and the row inside the unit.  locate(rows) -> (unit, row in unit) of each row."""
    ne = _bits(got) != _bits(want)
    if not bool(ne.any()):
        return None
    ne = ne.reshape(ne.shape[0], -1)
    rows = ne.any(1).nonzero().reshape(-1).cpu()
    unit, inrow = locate(rows)
    k = int(torch.argmin(unit * (int(inrow.max()) + 1) + inrow))
    u = int(unit[k])
    rnd, wg = walk(u, G)
    return ('%s: %d wrong elements in %d rows of %d units; first wrong unit %d (round %d, workgroup %d), row %d of the unit'
            % (what, int(ne.sum()), rows.numel(), int(torch.unique(unit).numel()), u, rnd, wg, int(inrow[k])))


def rows_locator(bm):
    return lambda rows: (rows // bm, rows % bm)


def tiles_locator(H, W, th, tw):
    """rows = pixels of an [N][H][W] map in memory order; unit = tile in the kernels' order (image, tile row, tile column)"""
    tx_n, ty_n = -(-W // tw), -(-H // th)

    def locate(rows):
        n, r = rows // (H * W), rows % (H * W)
        y, x = r // W, r % W
        return (n * ty_n + y // th) * tx_n + x // tw, (y % th) * tw + x % tw
    return locate


# ------------------------------------------------------------------------------------------------------ the shared runner
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_BASE = {}                                       # one slot: the newest base problem (inputs on the host, verified outputs on the device)


def _base(key, build):
    if key not in _BASE:
        _BASE.clear()
        _BASE[key] = build()
    return _BASE[key]


def _run_base(gathered, fixed, alloc, launch, verify, units):
    """Base launch under the memory contract; verify(outs) holds it to float64.  gathered: host tensors whose first axis is the
    unit axis (rows | images), fixed: the others (None allowed)."""
    with contract() as c:
        gd, fd = c.puts(*gathered), c.puts(*fixed)
        outs = alloc(c, units)
        launch(gd, fd, outs, units)
    no_nan(*outs)
    verify(outs)
    return dict(gathered=gd, fixed=fixed, outs=outs)


def _run_big(base, idx, units, alloc, launch, locate, G, walk=plain_walk, names=('y', 't')):
    """The big problem: gathered on the device, launched twice on the same buffers, compared with base[idx] bit for bit."""
    idx = idx.to(DEV)
    with contract() as c:
        gd = [c.put(t[idx]) for t in base['gathered']]
        fd = c.puts(*base['fixed'])
        outs = alloc(c, units)
        launch(gd, fd, outs, units)
        torch.cuda.synchronize()
        first = [o.clone() for o in outs]
        launch(gd, fd, outs, units)
    no_nan(*first)
    for o, o1, ob, name in zip(outs, first, base['outs'], names):
        flat = lambda t: t.reshape(-1, t.shape[-1])
        want = ob[idx]
        msg = mismatch(flat(o1), flat(want), locate, G, walk, name)
        assert msg is None, msg
        msg = mismatch(flat(o), flat(o1), locate, G, walk, name + ' (second launch against the first)')
        assert msg is None, msg
    del c, gd, fd, outs, first, want
    torch.cuda.empty_cache()                     # up to 270 MB per buffer: returned before the next case


def _skip_or(case):
    if case['skip']:
        pytest.skip(case['skip'])
    return case


def _ids(*parts):
    return '-'.join(str(p) for p in parts)


def _rounds_params(*axes):
    """the product of the given axes with the round count varying fastest (the base problem of a shape is built once)"""
    out = []
    for combo in itertools.product(*axes):
        vals = [v.values[0] if hasattr(v, 'values') else v for v in combo]
        ids = [v.id if hasattr(v, 'values') else ('x'.join(str(e) for e in v) if isinstance(v, tuple) else str(v)) for v in combo]
        for r in ROUNDS:
            out.append(pytest.param(*vals, r, id=_ids(*ids, 'rounds%d' % r)))
    return out


# ------------------------------------------------------------------------------------------------------ usot_pw_kstream_lp
def _kstream_base(dtype, biased, base_m):
    K, N = 1024, 256
    g = torch.Generator().manual_seed(base_m + biased)
    x = torch.randn(base_m, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / 32).to(dtype)
    b = torch.randn(N, generator=g) * 0.1 if biased else None
    ref = x.double() @ w.double().t()
    if biased:
        ref = (ref + b.double()).relu()

    def verify(outs):
        assert lp_err(outs[0], ref) <= 1.5 * ulp_of(dtype)
    return _run_base([x], [w, b], _kstream_alloc(dtype), _kstream_launch(dtype, biased), verify, base_m)


def _kstream_alloc(dtype):
    return lambda c, M: [c.out((M, 256), dtype)]


def _kstream_launch(dtype, biased):
    def launch(gd, fd, outs, M):
        hip.check(hip.lib().usot_pw_kstream_lp(hip.stream(), hip.ptr(gd[0]), hip.ptr(fd[0]), hip.ptr(fd[1]) if biased else None,
                                               hip.ptr(outs[0]), M, 1024, 256, 1 if biased else 0, dt_of(dtype)), 'usot_pw_kstream_lp')
    return launch


@pytest.mark.parametrize('dtype,biased,rounds', _rounds_params(LP, [pytest.param(True, id='bias_relu'), pytest.param(False, id='nobias_noact')]))
def test_pw_kstream_lp_rounds(dtype, biased, rounds):
    """1024 -> 256: the slab ring across panels (the barrier at the top of a panel guards the previous panel's slabs)"""
    case = _skip_or(kstream_case(cus(), rounds))
    base = _base(('kstream', dtype, biased), lambda: _kstream_base(dtype, biased, case['base_m']))
    idx = row_index(case['M'], case['bm'], BASE_PANELS, 11 + rounds)
    _run_big(base, idx, case['M'], _kstream_alloc(dtype), _kstream_launch(dtype, biased), rows_locator(case['bm']), case['G'])


# ------------------------------------------------------------------------------------------------------ usot_pw_panel_lp
def _panel_base(dtype, K, N, base_m):
    g = torch.Generator().manual_seed(K + N + base_m)
    x = torch.randn(base_m, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(base_m, N, generator=g).to(dtype)

    def verify(outs):
        ref = (x.double() @ w.double().t() + b.double() + r.double()).relu()
        assert lp_err(outs[0], ref) <= ulp_of(dtype) * 1.01
    return _run_base([x, r], [w, b], _panel_alloc(dtype, N), _panel_launch(dtype, K, N), verify, base_m)


def _panel_alloc(dtype, N):
    return lambda c, M: [c.out((M, N), dtype)]


def _panel_launch(dtype, K, N):
    def launch(gd, fd, outs, M):
        hip.check(hip.lib().usot_pw_panel_lp(hip.stream(), hip.ptr(gd[0]), hip.ptr(fd[0]), hip.ptr(fd[1]), hip.ptr(gd[1]), hip.ptr(outs[0]),
                                             M, K, N, 1, dt_of(dtype)), 'usot_pw_panel_lp')
    return launch


def _panel_rounds(case, form, dtype, K, N, seed):
    assert hip.lib().usot_pw_panel_pixels(K, N, 0) == (512 if K == 64 else 256) and hip.lib().usot_pw_panel_min_pixels(K, N) == (512 if K == 64 else 128)
    base = _base(('panel', form, dtype, K), lambda: _panel_base(dtype, K, N, case['base_m']))
    idx = row_index(case['M'], case['bm'], case['base_m'] // case['bm'], seed)
    _run_big(base, idx, case['M'], _panel_alloc(dtype, N), _panel_launch(dtype, K, N), rows_locator(case['bm']), case['G'])


@pytest.mark.parametrize('dtype,shape,rounds', _rounds_params(LP, PANEL_SHAPES))
def test_pw_panel_lp_large_form_rounds(dtype, shape, rounds):
    """256 -> 1024 and 128 -> 512 on panels of 256 pixels, residual + ReLU: the three-slot ring is refilled by the next panel's
    prologue with no barrier of its own between panels; lead and trail waves.  The base (192 panels: the smallest on this form)
    is the size tests/test_gpu_ops.py::test_pw_panel_lp_expansion_conv checks against float64."""
    case = _skip_or(panel_large_case(cus(), rounds))
    _panel_rounds(case, 'large', dtype, shape[0], shape[1], 21 + rounds)


@pytest.mark.parametrize('dtype,shape', [pytest.param(d.values[0], s, id=_ids(d.id, '%dx%d' % s)) for d in LP for s in PANEL_SHAPES])
def test_pw_panel_lp_small_form_rounds(dtype, shape):
    """... on panels of 128 pixels (one pixel block per wave): G + 1 panels and 77 rows"""
    case = _skip_or(panel_small_case(cus()))
    _panel_rounds(case, 'small', dtype, shape[0], shape[1], 31)


@pytest.mark.parametrize('dtype', LP)
def test_pw_panel_lp_k64_rounds(dtype):
    """64 -> 256 on panels of 512 pixels (four pixel blocks per wave): 2 G + 1 panels and a ragged one"""
    case = _skip_or(panel_k64_case(cus()))
    _panel_rounds(case, 'k64', dtype, 64, 256, 41)


# ------------------------------------------------------------------------------------------------------ usot_pw_panel_pair_lp
def _pair_inputs(dtype, cm, co, cn, base_m, relu_inputs, bias_scale):
    g = torch.Generator().manual_seed(cm + co + cn + base_m)
    t2 = torch.randn(base_m, cm, generator=g)
    res = torch.randn(base_m, co, generator=g)
    if relu_inputs:
        t2, res = t2.relu(), res.relu()
    w3 = (torch.randn(co, cm, generator=g) / cm ** 0.5).to(dtype)
    w1 = (torch.randn(cn, co, generator=g) / co ** 0.5).to(dtype)
    b3, b1 = torch.randn(co, generator=g) * bias_scale, torch.randn(cn, generator=g) * bias_scale
    return t2.to(dtype), res.to(dtype), w3, w1, b3, b1


def _pair_alloc(dtype, co, cn):
    return lambda c, M: [c.out((M, co), dtype), c.out((M, cn), dtype)]


def _panel_pair_launch(dtype, cm, co, cn, act2):
    def launch(gd, fd, outs, M):
        d = hip.pw_pair_desc(gd[0].data_ptr(), fd[0].data_ptr(), fd[2].data_ptr(), gd[1].data_ptr(), outs[0].data_ptr(), fd[1].data_ptr(),
                             fd[3].data_ptr(), outs[1].data_ptr(), M, cm, co, cn, act2)
        hip.check(hip.lib().usot_pw_panel_pair_lp(hip.stream(), C.byref(d), dt_of(dtype)), 'usot_pw_panel_pair_lp')
    return launch


def _panel_pair_base(dtype, shape, act2, base_m):
    cm, co, cn = shape
    t2, res, w3, w1, b3, b1 = _pair_inputs(dtype, cm, co, cn, base_m, False, 0.1)

    def verify(outs):
        y, t = outs
        yref = (t2.double() @ w3.double().t() + b3.double() + res.double()).relu()
        assert lp_err(y, yref) <= ulp_of(dtype) * 1.01               # one rounding of the output (the panel kernel's own bar)
        tref = y.cpu().double() @ w1.double().t() + b1.double()
        assert lp_err(t, tref.relu() if act2 else tref) <= (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)
    return _run_base([t2, res], [w3, w1, b3, b1], _pair_alloc(dtype, co, cn), _panel_pair_launch(dtype, cm, co, cn, act2), verify, base_m)


@pytest.mark.parametrize('dtype,shape,act2,rounds', _rounds_params(LP, PANEL_PAIR_SHAPES, [pytest.param(0, id='none'), pytest.param(1, id='relu')]))
def test_pw_panel_pair_lp_rounds(dtype, shape, act2, rounds):
    """the pair form: the same ring with W1's k-slices riding in it, and the barrier that runs only when a next panel exists (the
    trailers' last epilogue reads the second GEMM's slab after the interval loop's last barrier)"""
    bm = hip.lib().usot_pw_panel_pixels(*shape)
    assert bm == PANEL_PAIR_PIXELS[shape]
    case = _skip_or(panel_pair_case(cus(), shape, rounds, bm))
    base = _base(('panel_pair', dtype, shape, act2), lambda: _panel_pair_base(dtype, shape, act2, case['base_m']))
    idx = row_index(case['M'], bm, BASE_PANELS, 51 + rounds)
    _run_big(base, idx, case['M'], _pair_alloc(dtype, shape[1], shape[2]), _panel_pair_launch(dtype, *shape, act2), rows_locator(bm), case['G'])


# ------------------------------------------------------------------------------------------------------ usot_pw_pair_lp
def _pw_pair_launch(dtype, cm, co, cn):
    def launch(gd, fd, outs, M):
        d = hip.pw_pair_desc(gd[0].data_ptr(), fd[0].data_ptr(), fd[2].data_ptr(), gd[1].data_ptr(), outs[0].data_ptr(), fd[1].data_ptr(),
                             fd[3].data_ptr(), outs[1].data_ptr(), M, cm, co, cn, 1)
        hip.check(hip.lib().usot_pw_pair_lp(hip.stream(), C.byref(d), dt_of(dtype)), 'usot_pw_pair_lp')
    return launch


def _pw_pair_base(dtype, shape, base_m):
    cm, co, cn = shape
    t2, res, w3, w1, b3, b1 = _pair_inputs(dtype, cm, co, cn, base_m, True, 1.0)

    def verify(outs):
        y, t = outs
        ulp = ulp_of(dtype)
        yt = torch.relu(t2.double() @ w3.double().t() + b3.double() + res.double())
        assert rel_err(y.float().cpu().numpy(), yt.numpy()) < 4 * ulp
        tt = torch.relu(y.cpu().double() @ w1.double().t() + b1.double())
        assert rel_err(t.float().cpu().numpy(), tt.numpy()) < 4 * ulp
    fixed = [hip.pw_pair_pack(w3, cm, co, cn, 0), hip.pw_pair_pack(w1, cm, co, cn, 1), b3, b1]
    return _run_base([t2, res], fixed, _pair_alloc(dtype, co, cn), _pw_pair_launch(dtype, cm, co, cn), verify, base_m)


@pytest.mark.parametrize('dtype,shape', [pytest.param(d.values[0], s, id=_ids(d.id, '%dx%dx%d' % s)) for d in LP for s in PW_PAIR_SHAPES])
def test_pw_pair_lp_rounds(dtype, shape):
    """the tiled pair: the next tile's t2 DMA and residual loads run under the second GEMM; 4 CUs + 1 tiles of 64 rows and a ragged
    one reuse the LDS image a third time at one and at two workgroups per CU"""
    case = _skip_or(pw_pair_case(cus(), shape))
    base = _base(('pw_pair', dtype, shape), lambda: _pw_pair_base(dtype, shape, case['base_m']))
    idx = row_index(case['M'], 64, BASE_PANELS, 61)
    _run_big(base, idx, case['M'], _pair_alloc(dtype, shape[1], shape[2]), _pw_pair_launch(dtype, *shape), rows_locator(64), case['G'])


# ------------------------------------------------------------------------------------------------------ usot_conv3x3_halo_lp
def _halo_alloc(dtype, H, W):
    return lambda c, N: [c.out((N, H, W, 64), dtype)]


def _halo_launch(dtype, H, W):
    def launch(gd, fd, outs, N):
        hip.check(hip.lib().usot_conv3x3_halo_lp(hip.stream(), hip.ptr(gd[0]), hip.ptr(fd[0]), hip.ptr(fd[1]), hip.ptr(outs[0]), N, H, W, 64, 64, 1,
                                                 dt_of(dtype)), 'usot_conv3x3_halo_lp')
    return launch


def _halo_base(dtype, H, W, N):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    x = torch.randn(N, H, W, 64, generator=g).to(dtype)
    w = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dtype)
    b = torch.randn(64, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(), padding=1).permute(0, 2, 3, 1).relu()

    def verify(outs):
        assert lp_err(outs[0], ref) <= ulp_of(dtype) * 1.01
    return _run_base([x], [w.reshape(64, 576).contiguous(), b], _halo_alloc(dtype, H, W), _halo_launch(dtype, H, W), verify, N)


@pytest.mark.parametrize('dtype,H,rounds', _rounds_params(LP, HALO_HS))
def test_conv3x3_halo_lp_rounds(dtype, H, rounds):
    """the halo double buffer and the counted wait that is reached from a workgroup's second tile on: nine tiles per image, so a
    workgroup alternates between full and ragged tiles and a wave's store count takes every value 0 .. 4 over the four heights"""
    case = _skip_or(halo_case(cus(), rounds, H))
    base = _base(('halo', dtype, H), lambda: _halo_base(dtype, H, HALO_W, BASE_IMAGES))
    idx = image_index(case['N'], BASE_IMAGES, 71 + rounds + H)
    _run_big(base, idx, case['N'], _halo_alloc(dtype, H, HALO_W), _halo_launch(dtype, H, HALO_W),
             tiles_locator(H, HALO_W, HALO_TILE, HALO_TILE), case['G'])


# ------------------------------------------------------------------------------------------------------ usot_bneck_first_lp, usot_bneck_tail_lp
def _bneck_alloc(dtype, H, W, cn):
    return lambda c, N: [c.out((N, H, W, 256), dtype), c.out((N, H, W, cn), dtype)]


def _bneck_verify(dtype, y_ref, t_ref):
    def verify(outs):
        ey, et = lp_err(outs[0], y_ref), lp_err(outs[1], t_ref)
        assert ey <= 3 * ulp_of(dtype) and et <= 4 * ulp_of(dtype), (ey, et)
    return verify


def _bneck_first_launch(dtype, H, W):
    def launch(gd, fd, outs, N):
        d = hip.bneck_desc(*[hip.ptr(v) for v in [gd[0]] + list(fd) + list(outs)], N, H, W)
        hip.check(hip.lib().usot_bneck_first_lp(hip.stream(), C.byref(d), dt_of(dtype)), 'usot_bneck_first_lp')
    return launch


def _bneck_first_base(dtype, N, H, W):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(N, H, W, 64).relu().to(dtype)
    w1 = (rnd(64, 64) / 8).to(dtype); b1 = rnd(64) * 0.1
    w2 = (rnd(64, 3, 3, 64) / 24).to(dtype); b2 = rnd(64) * 0.1
    w3 = (rnd(256, 64) / 8).to(dtype); wd = (rnd(256, 64) / 8).to(dtype); b3c = rnd(256) * 0.1
    wn = (rnd(64, 256) / 16).to(dtype); bn = rnd(64) * 0.1
    rq = lambda v: v.to(dtype).double()
    xd_ = x.double()
    t1 = rq((xd_ @ w1.double().t() + b1.double()).relu())
    t2 = rq(F.conv2d(t1.permute(0, 3, 1, 2), w2.double().permute(0, 3, 1, 2), b2.double(), padding=1).permute(0, 2, 3, 1).relu())
    y_ref = (t2 @ w3.double().t() + xd_ @ wd.double().t() + b3c.double()).relu()
    t_ref = (rq(y_ref) @ wn.double().t() + bn.double()).relu()
    fixed = [w1, b1, w2.reshape(64, 576).contiguous(), b2, torch.cat([w3, wd], 1).contiguous(), b3c, wn, bn]
    return _run_base([x], fixed, _bneck_alloc(dtype, H, W, 64), _bneck_first_launch(dtype, H, W), _bneck_verify(dtype, y_ref, t_ref), N)


def _bneck_tail_launch(dtype, H, W, cn):
    def launch(gd, fd, outs, N):
        w2, b2, w3, b3, wn, bn = fd
        d = hip.bneck_desc(hip.ptr(gd[0]), hip.ptr(gd[1]), None, hip.ptr(w2), hip.ptr(b2), hip.ptr(w3), hip.ptr(b3), hip.ptr(wn), hip.ptr(bn),
                           hip.ptr(outs[0]), hip.ptr(outs[1]), N, H, W)
        hip.check(hip.lib().usot_bneck_tail_lp(hip.stream(), C.byref(d), cn, dt_of(dtype)), 'usot_bneck_tail_lp')
    return launch


def _bneck_tail_base(dtype, N, H, W, cn):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W + cn)
    rnd = lambda *s: torch.randn(*s, generator=g)
    t1 = rnd(N, H, W, 64).relu().to(dtype)
    res = rnd(N, H, W, 256).relu().to(dtype)
    w2 = (rnd(64, 3, 3, 64) / 24).to(dtype); b2 = rnd(64) * 0.1
    w3 = (rnd(256, 64) / 8).to(dtype); b3 = rnd(256) * 0.1
    wn = (rnd(cn, 256) / 16).to(dtype); bn = rnd(cn) * 0.1
    rq = lambda v: v.to(dtype).double()
    t2 = rq(F.conv2d(t1.double().permute(0, 3, 1, 2), w2.double().permute(0, 3, 1, 2), b2.double(), padding=1).permute(0, 2, 3, 1).relu())
    y_ref = (t2 @ w3.double().t() + b3.double() + res.double()).relu()
    t_ref = (rq(y_ref) @ wn.double().t() + bn.double()).relu()
    fixed = [w2.reshape(64, 576).contiguous(), b2, w3, b3, wn, bn]
    return _run_base([t1, res], fixed, _bneck_alloc(dtype, H, W, cn), _bneck_tail_launch(dtype, H, W, cn), _bneck_verify(dtype, y_ref, t_ref), N)


def _bneck_rounds(case, base, dtype, cn, launch, seed):
    idx = image_index(case['N'], BASE_IMAGES, seed)
    _run_big(base, idx, case['N'], _bneck_alloc(dtype, BNECK_H, BNECK_W, cn), launch,
             tiles_locator(BNECK_H, BNECK_W, BNECK_TH, BNECK_TW), case['G'], bneck_walk)


@pytest.mark.parametrize('dtype,rounds', _rounds_params(LP))
def test_bneck_first_lp_rounds(dtype, rounds):
    """layer1's first bottleneck: the `slot ^ 1` halo prefetch, the counted wait keyed to the previous tile's stores (7-row bottom
    tiles: another count than a full tile's) and the XCD-grouped tile walk, at G + 4 and 2 G + 4 tiles"""
    case = _skip_or(bneck_case(cus(), rounds))
    base = _base(('bneck_first', dtype), lambda: _bneck_first_base(dtype, BASE_IMAGES, BNECK_H, BNECK_W))
    _bneck_rounds(case, base, dtype, 64, _bneck_first_launch(dtype, BNECK_H, BNECK_W), 81 + rounds)


@pytest.mark.parametrize('dtype,cn,rounds', _rounds_params(LP, [64, 128]))
def test_bneck_tail_lp_rounds(dtype, cn, rounds):
    """the rest of a layer1 bottleneck with the next conv1 of 64 and of 128 channels"""
    case = _skip_or(bneck_case(cus(), rounds))
    base = _base(('bneck_tail', dtype, cn), lambda: _bneck_tail_base(dtype, BASE_IMAGES, BNECK_H, BNECK_W, cn))
    _bneck_rounds(case, base, dtype, cn, _bneck_tail_launch(dtype, BNECK_H, BNECK_W, cn), 91 + rounds + cn)


# ------------------------------------------------------------------------------------------------------ usot_conv_pw_lp, usot_conv_pw_pair_lp
# Not persistent, but the panel of a workgroup comes from cp_xcd_remap(blockIdx.x, npanels), which must be a bijection for
# every npanels mod 8: n = 1 .. 15 images of 12 x 12 (CM = 128) and 13 x 13 (CM = 256) give every panel count from 1 to 20.
CONV_PW_NMAX = 15
CONV_PW_GEO = [pytest.param(13, 256, id='h13_c256'), pytest.param(12, 128, id='h12_c128')]


def conv_pw_panel_counts():
    return {-(-n * h * h // bm) for n in range(1, CONV_PW_NMAX + 1) for h in (12, 13) for bm in (128, 256)}


def automatic_form_images(cus, h):
    """the most h x h images whose pixels still fit CUs + 1 panels of 256"""
    return (cus + 1) * 256 // (h * h)


def _conv_pw_case(h, cm, dtype, cn):
    """inputs of the CONV_PW_NMAX-image problem and its float64 reference; the n-image problem is its first n images"""
    def build():
        ins, ref, M, co = _conv_pw_inputs(CONV_PW_NMAX, h, 1, 1, cm, dtype, CONV_PW_NMAX * 1000 + h * 10 + cn, cn=cn)
        return dict(ins=ins, ref=ref)
    return _base(('conv_pw', h, cm, dtype, cn), build)


def _conv2_then(c, t1d, w2d, b2d, n, h, cm, dtype):
    """usot_conv2d_lp on the tile the fused kernel is bit-identical to (tests/test_gpu_ops.py): conv2's output t2"""
    t2 = c.out((n, h, h, cm), dtype)
    d2 = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), t2.data_ptr(), N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                       pad=(1, 1), dil=(1, 1), act=1, tile=32 if cm == 256 else 37)
    hip.check(hip.lib().usot_conv2d_lp(hip.stream(), C.byref(d2), dt_of(dtype), 0), 'usot_conv2d_lp')
    return t2


@pytest.mark.parametrize('form', [1, 2], ids=['panel256', 'panel128'])
@pytest.mark.parametrize('rs', [False, True], ids=['pertap', 'rowshared'])
@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('h,cm', CONV_PW_GEO)
def test_conv_pw_lp_panel_remap_sweep(h, cm, form, rs, dtype):
    """conv2 -> conv3 in one launch at every panel count: per-tap loop bit-equal to usot_conv2d_lp followed by usot_pw_panel_lp (as
    include/usot_hip.h promises), row-shared loop within 4 ulp of float64"""
    case = _conv_pw_case(h, cm, dtype, 0)
    t1, w2, b2, w3, b3, res = case['ins'][:6]
    co, P = 4 * cm, h * h
    for n in range(1, CONV_PW_NMAX + 1):
        M = n * P
        with contract() as c:
            t1d, w2d, b2d, w3d, b3d, resd = c.puts(t1[:n], w2, b2, w3, b3, res[:M])
            y = c.out((M, co), dtype)
            d = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                              pad=(1, 1), dil=(1, 1), act=1, tile=form | (0 if rs else 4))
            hip.check(hip.lib().usot_conv_pw_lp(hip.stream(), C.byref(d), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(resd), hip.ptr(y), dt_of(dtype)),
                      'usot_conv_pw_lp')
            if not rs:
                t2 = _conv2_then(c, t1d, w2d, b2d, n, h, cm, dtype)
                y2 = c.out((M, co), dtype)
                hip.check(hip.lib().usot_pw_panel_lp(hip.stream(), hip.ptr(t2), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(resd), hip.ptr(y2), M, cm, co, 1,
                                                     dt_of(dtype)), 'usot_pw_panel_lp')
        no_nan(y)
        bm = 256 if form == 1 else 128
        if rs:
            err = lp_err(y, case['ref'][:M])
            assert err <= 4 * ulp_of(dtype), (n, err)
        else:
            msg = mismatch(y, y2, rows_locator(bm), 1 << 30)
            assert msg is None, 'n = %d (%d panels): %s' % (n, -(-M // bm), msg)


@pytest.mark.parametrize('form', [1, 2], ids=['panel256', 'panel128'])
@pytest.mark.parametrize('rs', [False, True], ids=['pertap', 'rowshared'])
@pytest.mark.parametrize('dtype', LP)
@pytest.mark.parametrize('h,cm', CONV_PW_GEO)
def test_conv_pw_pair_lp_panel_remap_sweep(h, cm, form, rs, dtype):
    """... with the next conv1 in the launch.  Per-tap loop: layer2's widths (128, 512, 128) bit-equal to usot_conv2d_lp followed by
    usot_pw_panel_pair_lp; layer3's (256, 1024, 256), which the panel pair does not run, Y bit-equal to usot_conv2d_lp followed by
    usot_pw_panel_lp and T to usot_conv2d_lp on that Y (the fifth phase's promise).  Row-shared loop: Y within 4 ulp of float64, T
    within one rounding of float64 on the launch's own Y."""
    cn, act2 = (256, 0) if cm == 256 else (128, 1)
    case = _conv_pw_case(h, cm, dtype, cn)
    t1, w2, b2, w3, b3, res, w1, b1 = case['ins']
    co, P = 4 * cm, h * h
    for n in range(1, CONV_PW_NMAX + 1):
        M = n * P
        with contract() as c:
            t1d, w2d, b2d, w3d, b3d, resd, w1d, b1d = c.puts(t1[:n], w2, b2, w3, b3, res[:M], w1, b1)
            y, t = c.out((M, co), dtype), c.out((M, cn), dtype)
            d = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                              pad=(1, 1), dil=(1, 1), act=1, tile=form | (0 if rs else 4))
            pd = hip.pw_pair_desc(None, w3d.data_ptr(), b3d.data_ptr(), resd.data_ptr(), y.data_ptr(), w1d.data_ptr(), b1d.data_ptr(),
                                  t.data_ptr(), M, cm, co, cn, act2)
            hip.check(hip.lib().usot_conv_pw_pair_lp(hip.stream(), C.byref(d), C.byref(pd), dt_of(dtype)), 'usot_conv_pw_pair_lp')
            if not rs:
                t2 = _conv2_then(c, t1d, w2d, b2d, n, h, cm, dtype)
                y2, tt = c.out((M, co), dtype), c.out((M, cn), dtype)
                if cm == 128:
                    pd2 = hip.pw_pair_desc(t2.data_ptr(), w3d.data_ptr(), b3d.data_ptr(), resd.data_ptr(), y2.data_ptr(), w1d.data_ptr(),
                                           b1d.data_ptr(), tt.data_ptr(), M, cm, co, cn, act2)
                    hip.check(hip.lib().usot_pw_panel_pair_lp(hip.stream(), C.byref(pd2), dt_of(dtype)), 'usot_pw_panel_pair_lp')
                else:
                    hip.check(hip.lib().usot_pw_panel_lp(hip.stream(), hip.ptr(t2), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(resd), hip.ptr(y2), M, cm, co,
                                                         1, dt_of(dtype)), 'usot_pw_panel_lp')
                    d1 = hip.conv_desc(y2.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), tt.data_ptr(), N=1, H=M, W=1, Cin=co, OH=M, OW=1, Cout=cn,
                                       KH=1, KW=1, act=act2, tile=32)
                    hip.check(hip.lib().usot_conv2d_lp(hip.stream(), C.byref(d1), dt_of(dtype), 0), 'usot_conv2d_lp')
        no_nan(y, t)
        bm = 256 if form == 1 else 128
        if rs:
            err = lp_err(y, case['ref'][:M])
            assert err <= 4 * ulp_of(dtype), (n, err)
            tref = y.cpu().double() @ w1.double().t() + b1.double()
            bar = ulp_of(dtype) * 1.01 if cm == 256 else (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)
            err = lp_err(t, tref.relu() if act2 else tref)
            assert err <= bar, (n, err)
        else:
            for got, want, name in ((y, y2, 'y'), (t, tt, 't')):
                msg = mismatch(got, want, rows_locator(bm), 1 << 30, what=name)
                assert msg is None, 'n = %d (%d panels): %s' % (n, -(-M // bm), msg)


@pytest.mark.parametrize('dtype', LP)
def test_conv_pw_lp_automatic_form_at_one_panel_past_the_cu_count(dtype):
    """ceil(M / 256) = CUs + 1: a second round of 256-pixel panels would be almost empty, so the automatic form (tile & 3 = 0) must be
    the 128-pixel one - usot_conv_pw_pixels says so and the launch equals the forced 128-pixel form bit for bit (12 x 12 maps, 128
    channels, per-tap loop)."""
    h, cm, co = 12, 128, 512
    n = automatic_form_images(cus(), h)
    M = n * h * h
    assert -(-M // 256) == cus() + 1
    assert hip.lib().usot_conv_pw_pixels(M) == 128
    g = torch.Generator(device=DEV).manual_seed(n + cm)
    dev = lambda *s: torch.randn(*s, device=DEV, generator=g)
    t1 = dev(n, h, h, cm).relu().to(dtype)
    w2, w3 = (dev(cm, 9 * cm) / (9 * cm) ** 0.5).to(dtype), (dev(co, cm) / cm ** 0.5).to(dtype)
    b2, b3 = dev(cm) * 0.1, dev(co) * 0.1
    res = dev(M, co).to(dtype)
    outs = []
    with contract() as c:
        t1d, w2d, b2d, w3d, b3d, resd = c.puts(t1, w2, b2, w3, b3, res)
        for form in (0, 2):
            y = c.out((M, co), dtype)
            d = hip.conv_desc(t1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, N=n, H=h, W=h, Cin=cm, OH=h, OW=h, Cout=cm, KH=3, KW=3,
                              pad=(1, 1), dil=(1, 1), act=1, tile=form | 4)
            hip.check(hip.lib().usot_conv_pw_lp(hip.stream(), C.byref(d), hip.ptr(w3d), hip.ptr(b3d), hip.ptr(resd), hip.ptr(y), dt_of(dtype)),
                      'usot_conv_pw_lp')
            outs.append(y)
    no_nan(*outs)
    msg = mismatch(outs[0], outs[1], rows_locator(128), 1 << 30)
    assert msg is None, msg
