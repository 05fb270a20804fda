"""GPU: the frame's memory branch on DISTINCT memory rows only (engine option 'mem_dedupe').

The gather kernel dedupes the picked rows on the device and publishes mem_map = [D, u(0), .., u(n_pick - 1)]; GroupDW's memory
segment, Conf_Fusion's convolution and its reduction are captured for the full queue and read D / the slot map at run time.
Every kernel is checked on its own against its static form - bit for bit on what it computes, prefill bits kept on what it
must not write, canaries (tests/guarded.py) around every buffer - and the Session against a 'mem_dedupe' = False session at the
bars of tests/test_gpu_tracker.py::test_deferred_append_equals_the_append_behind_the_tag."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from usot_amd import engine, hip, synth  # noqa: E402
from usot_amd.model import USOT  # noqa: E402

DEV = 'cuda:0'
EINVAL = -1


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def first_occurrence(rows):
    """Pure-Python reference of the kernel's map: (D, u) with u[j] = rank of the first occurrence of rows[j] among first occurrences."""
    lead, u = [], []
    for r in rows:
        if r not in lead:
            lead.append(r)
        u.append(lead.index(r))
    return len(lead), u, lead


def test_first_occurrence_reference_on_the_steady_state():
    assert first_occurrence([0, 1, 5, 9, 9, 9, 9]) == (4, [0, 1, 2, 3, 3, 3, 3], [0, 1, 5, 9])


# ---------------------------------------------------------------------------------------------------------------- gather
GATHER_CASES = [
    ('steady', [0, 1, 5, 9, 9, 9, 9], 11),
    ('all_distinct', [0, 1, 2, 3, 4, 5, 6], 11),
    ('all_equal', [4] * 7, 11),
    ('appended_among_duplicates', [0, 1, 5, 9, 9, 9, 9], 9),           # row 9 is the row being appended: served from `fresh`
    ('n_pick_1', [7], 3),
    ('n_pick_32', [0, 1] + [2 + (i * 5) % 9 for i in range(30)], 10),   # 11 distinct rows, the appended one among them
]


@pytest.mark.parametrize('name,picks,slot', GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
@pytest.mark.parametrize('prefill', ['canary', 'zero'])
def test_gather_copies_distinct_rows_and_publishes_the_map(name, picks, slot, prefill):
    lens = [7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 64]
    g = torch.Generator().manual_seed(11)
    nq = len(picks)
    start = guarded.registry_size()
    bank_cpu = [torch.randn(12, n, generator=g) for n in lens]
    banks = [guarded.put(b, DEV) for b in bank_cpu]
    fresh = [guarded.put(torch.randn(1, n, generator=g), DEV) for n in lens]
    idx = guarded.put(torch.tensor(picks + [-5, 123, 456, slot], dtype=torch.int32), DEV)
    picked = [guarded.alloc((nq, n), torch.float32, DEV, prefill) for n in lens[1:]]
    before = [p.clone() for p in picked]
    mem_map = guarded.alloc((1 + nq,), torch.int32, DEV, 'full', -7)
    p4 = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])
    p3 = (C.c_void_p * 3)(*[t.data_ptr() for t in picked])
    hip.check(hip.lib().usot_rows_append_gather_dedupe_f32(hip.stream(), p4(fresh), p4(banks), p3, (C.c_int32 * 4)(*lens),
                                                           hip.ptr(idx), nq, nq + 3, hip.ptr(mem_map)), 'rows_append_gather_dedupe')
    torch.cuda.synchronize()
    guarded.check(start)
    D, u, lead = first_occurrence(picks)
    assert mem_map.cpu().tolist() == [D] + u
    for k in range(4):
        want = bank_cpu[k].clone()
        want[slot] = fresh[k][0].cpu()
        assert same_bits(banks[k].cpu(), want), k                        # the append half: one row replaced, nothing else
        if k:
            got = picked[k - 1].cpu()
            assert same_bits(got[:D], want[torch.tensor(lead).long()]), k    # distinct rows in order of first appearance
            assert same_bits(got[D:], before[k - 1][D:].cpu()), k            # rows >= D keep their prefill bits


def test_gather_argument_checks():
    lens = [64, 64, 64, 64]
    banks = [torch.zeros(4, 64, device=DEV) for _ in lens]
    fresh = [torch.zeros(1, 64, device=DEV) for _ in lens]
    picked = [torch.zeros(33, 64, device=DEV) for _ in lens[1:]]
    idx = torch.zeros(40, dtype=torch.int32, device=DEV)
    mm = torch.zeros(40, dtype=torch.int32, device=DEV)
    p4 = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])
    p3 = (C.c_void_p * 3)(*[t.data_ptr() for t in picked])
    L = hip.lib()
    args = (hip.stream(), p4(fresh), p4(banks), p3, (C.c_int32 * 4)(*lens), hip.ptr(idx))
    assert L.usot_rows_append_gather_dedupe_f32(*args, 33, 36, hip.ptr(mm)) == EINVAL
    assert L.usot_rows_append_gather_dedupe_f32(*args, 7, 10, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------------ conv
CONV_TILES = [55, 57]                  # the 32 x 64 tile the frame's Conf_Fusion conv is tuned to and the 64 x 64 candidate
N_MAPS, HW, CIN, COUT = 3, 5, 64, 64   # M = 75: a 32-row tile straddles every map boundary
PIX = HW * HW


@pytest.fixture(scope='module')
def conv_data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N_MAPS, HW, HW, CIN, generator=g)
    w = torch.randn(COUT, 9 * CIN, generator=g) / (9 * CIN) ** 0.5
    b = torch.randn(COUT, generator=g)
    return x, w, b


class ConvRig(object):
    """One geometry on one tile: guarded operands, a descriptor factory, the static reference."""

    def __init__(self, data, tile, ksplit, prefill, x_nan_from=None):
        x, w, b = data
        self.tile, self.ks = tile, ksplit
        self.split16 = hip.tile_wfrag(tile) == 2
        x = x.clone()
        if x_nan_from is not None:
            x[x_nan_from:] = float('nan')
        self.x = guarded.put(x, DEV)
        if self.split16:
            wb, wsc = hip.split16_pack(w)
            self.w, self.wsc = guarded.put(wb, DEV), guarded.put(wsc, DEV)
        else:
            self.w, self.wsc = guarded.put(w, DEV), None
        self.b = guarded.put(b, DEV)
        self.prefill = prefill
        self.ovf = guarded.alloc((1,), torch.int32, DEV, 'zero')
        self.cnt = guarded.alloc((1,), torch.int32, DEV, 'zero')

    def ws(self, n):
        if self.ks == 1:
            return None
        m = n * PIX                      # slabs + one ticket word per tile (usot_conv_ws_floats), zero before first use
        return guarded.alloc((self.ks * m * COUT + ((m + 15) // 16) * ((COUT + 31) // 32),), torch.float32, DEV, 'zero')

    def desc(self, y, first, n, ws, dyn):
        return hip.conv_desc(self.x[first:].data_ptr(), self.w.data_ptr(), self.b.data_ptr(), y[first:].data_ptr(),
                             N=n, H=HW, W=HW, Cin=CIN, OH=HW, OW=HW, Cout=COUT, KH=3, KW=3, pad=(1, 1), act=hip.ACT_RELU,
                             ksplit=self.ks, tile=self.tile, ws=ws.data_ptr() if ws is not None else None,
                             w_frag=2 if self.split16 else 0, w_scale=self.wsc.data_ptr() if self.split16 else None,
                             ovf=self.ovf.data_ptr() if self.split16 else None,
                             n_dyn=self.cnt.data_ptr() if dyn else None, n_first=first if dyn else 0)

    def out(self):
        return guarded.alloc((N_MAPS, HW, HW, COUT), torch.float32, DEV, self.prefill)

    def launch(self, descs):
        arr = (hip.ConvDesc * len(descs))(*descs)
        return hip.lib().usot_conv2d_batch_f32(hip.stream(), arr, len(descs))

    def static(self, count):
        """the static launch over the first `count` maps"""
        y = self.out()
        if count:
            hip.check(self.launch([self.desc(y, 0, count, self.ws(count), False)]), 'static conv')
        torch.cuda.synchronize()
        return y


def tickets(ws, n, ks):
    return ws[ks * n * PIX * COUT:].view(torch.int32)


@pytest.mark.parametrize('prefill', ['canary', 'zero'])
@pytest.mark.parametrize('ks', [1, 2])
@pytest.mark.parametrize('tile', CONV_TILES)
def test_conv_run_time_image_count(conv_data, tile, ks, prefill):
    """Counts 0..3 on ONE problem of three maps, launched one straight after the other on the same workspace: active rows bit-equal
    to the static launch over the first `count` maps, everything else keeps its prefill bits, the tickets are zero afterwards."""
    start = guarded.registry_size()
    rig = ConvRig(conv_data, tile, ks, prefill)
    ws = rig.ws(N_MAPS)
    for count in (2, 0, 3, 1, 5):                       # (5: clamped to the problem's three maps)
        act = min(count, N_MAPS)
        want = rig.static(act)
        y = rig.out()
        blank = y.clone()
        rig.cnt.fill_(count)
        hip.check(rig.launch([rig.desc(y, 0, N_MAPS, ws, True)]), 'dyn conv')
        torch.cuda.synchronize()
        assert same_bits(y[:act], want[:act]), (tile, ks, count)
        assert same_bits(y[act:], blank[act:]), (tile, ks, count)
        assert torch.isfinite(y[:act]).all()
        if ws is not None:
            assert int(tickets(ws, N_MAPS, ks).abs().max()) == 0, (tile, ks, count)
    guarded.check(start)


@pytest.mark.parametrize('prefill', ['canary', 'zero'])
@pytest.mark.parametrize('ks', [1, 2])
@pytest.mark.parametrize('tile', CONV_TILES)
def test_conv_two_problems_share_one_count(conv_data, tile, ks, prefill):
    """A batch of two problems over the same map numbering: maps [0, 2) with n_first = 0 and map 2 with n_first = 2."""
    start = guarded.registry_size()
    rig = ConvRig(conv_data, tile, ks, prefill)
    wsa, wsb = rig.ws(2), rig.ws(1)
    for count in (3, 1, 0, 2):
        want = rig.static(count)
        y = rig.out()
        blank = y.clone()
        rig.cnt.fill_(count)
        hip.check(rig.launch([rig.desc(y, 0, 2, wsa, True), rig.desc(y, 2, 1, wsb, True)]), 'dyn conv batch')
        torch.cuda.synchronize()
        assert same_bits(y[:count], want[:count]), (tile, ks, count)
        assert same_bits(y[count:], blank[count:]), (tile, ks, count)
        if ks > 1:
            assert int(tickets(wsa, 2, ks).abs().max()) == 0 and int(tickets(wsb, 1, ks).abs().max()) == 0
    guarded.check(start)


@pytest.mark.parametrize('ks', [1, 2])
@pytest.mark.parametrize('tile', CONV_TILES)
def test_conv_split_fp16_twin_keeps_inactive_rows_away_from_ovf(conv_data, tile, ks):
    """The split-fp16 twin of each tile with the INACTIVE input maps NaN: a NaN that reached a sum would set the sticky ovf word."""
    twin = engine.SPLIT16_TILES[tile]
    assert hip.tile_wfrag(twin) == 2 and hip.lib().usot_conv_tile_dyn(twin) == 1
    start = guarded.registry_size()
    for count in (0, 1, 2, 3):
        rig = ConvRig(conv_data, twin, ks, 'canary', x_nan_from=count)
        want = rig.static(count)
        assert int(rig.ovf.item()) == 0
        y = rig.out()
        blank = y.clone()
        rig.cnt.fill_(count)
        ws = rig.ws(N_MAPS)
        hip.check(rig.launch([rig.desc(y, 0, N_MAPS, ws, True)]), 'dyn conv split16')
        torch.cuda.synchronize()
        assert int(rig.ovf.item()) == 0, (twin, ks, count)
        assert same_bits(y[:count], want[:count]) and torch.isfinite(y[:count]).all(), (twin, ks, count)
        assert same_bits(y[count:], blank[count:]), (twin, ks, count)
        if ws is not None:
            assert int(tickets(ws, N_MAPS, ks).abs().max()) == 0
    guarded.check(start)


def test_conv_other_tile_families_reject_a_run_time_count(conv_data):
    """n_dyn on a tile outside the producer / consumer family: USOT_EINVAL, `y` untouched."""
    start = guarded.registry_size()
    for tile in (15, 7):
        assert hip.lib().usot_conv_tile_built(tile) and hip.lib().usot_conv_tile_dyn(tile) == 0
        rig = ConvRig(conv_data, tile, 1, 'canary')
        y = rig.out()
        blank = y.clone()
        rig.cnt.fill_(2)
        assert rig.launch([rig.desc(y, 0, N_MAPS, None, True)]) == EINVAL
        torch.cuda.synchronize()
        assert same_bits(y, blank)
        hip.check(rig.launch([rig.desc(y, 0, N_MAPS, None, False)]), 'static conv on tile %d' % tile)     # the same descriptor without it runs
    for tile in CONV_TILES + [engine.SPLIT16_TILES[t] for t in CONV_TILES]:
        assert hip.lib().usot_conv_tile_dyn(tile) == 1
    torch.cuda.synchronize()
    guarded.check(start)


# --------------------------------------------------------------------------------------------------------------- GroupDW
@pytest.mark.parametrize('prefill', ['canary', 'zero'])
@pytest.mark.parametrize('Cc', [256, 64])
def test_groupdw_run_time_sample_count(Cc, prefill):
    """Three segments (2 + 2 + capacity 7 samples, the last one sharing its search maps like the frame's memory branch), OH = OW = 7:
    counts 0, 1, 4, 7 against the static launch with that many samples in the last segment; the rest keeps its prefill bits."""
    S, CAP = 7, 7
    g = torch.Generator().manual_seed(3)
    start = guarded.registry_size()
    xs = [guarded.put(torch.randn(2, S + 4, S + 4, Cc, generator=g), DEV) for _ in range(3)]
    geo = ((5, 5), (3, 5), (5, 3))
    z01 = [[guarded.put(torch.randn(2, hk, wk, Cc, generator=g), DEV) for hk, wk in geo] for _ in range(2)]
    zm = [guarded.put(torch.randn(CAP, hk, wk, Cc, generator=g), DEV) for hk, wk in geo]
    wsm = [(0.5, 0.3, 0.2), (0.2, 0.5, 0.3), (0.3, 0.3, 0.4)]
    cnt = guarded.alloc((1,), torch.int32, DEV, 'zero')

    def descs(outs, last_s):
        mk = lambda zs, out, w, s, rep: hip.groupdw_desc([t.data_ptr() for t in xs], [t.data_ptr() for t in zs], out.data_ptr(), w,
                                                          S=s, x_rep=rep, OH=S, OW=S, Cc=Cc, x_cs=[Cc] * 3, x_co=[0] * 3,
                                                          z_cs=[Cc] * 3, z_co=[0] * 3)
        ds = [mk(z01[0], outs[0], wsm[0], 2, 1), mk(z01[1], outs[1], wsm[1], 2, 1), mk(zm, outs[2], wsm[2], last_s, CAP)]
        return (hip.GroupDWDesc * 3)(*ds)

    def outs():
        return [guarded.alloc((n, S, S, Cc), torch.float32, DEV, prefill) for n in (2, 2, CAP)]

    for count in (4, 0, 7, 1):
        want = outs()
        if count:
            hip.check(hip.lib().usot_groupdw_multi_f32(hip.stream(), descs(want, count), 3), 'static groupdw')
        else:
            hip.check(hip.lib().usot_groupdw_multi_f32(hip.stream(), descs(want, 1), 2), 'static groupdw (two segments)')
        got = outs()
        blank = got[2].clone()
        cnt.fill_(count)
        hip.check(hip.lib().usot_groupdw_multi_dyn_f32(hip.stream(), descs(got, CAP), 3, hip.ptr(cnt)), 'dyn groupdw')
        torch.cuda.synchronize()
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), count
        assert same_bits(got[2][:count], want[2][:count]) and torch.isfinite(got[2][:count]).all(), count
        assert same_bits(got[2][count:], blank[count:]), count
    # another variant with the pointer set: rejected
    d = descs(outs(), CAP)
    d[0].cols_per_thread = 50
    assert hip.lib().usot_groupdw_multi_dyn_f32(hip.stream(), d, 3, hip.ptr(cnt)) == EINVAL
    torch.cuda.synchronize()
    guarded.check(start)


# ------------------------------------------------------------------------------------------------------------- reduction
def test_reduction_through_the_slot_map():
    """With the map [0, 1, 2, 3, 3, 3, 3] the mapped kernel is bit-equal to the static kernel on the seven-map tensor gathered with torch."""
    P, Cc, M = 30, 256, 7
    g = torch.Generator().manual_seed(9)
    start = guarded.registry_size()
    cv_cpu = torch.randn(M, 5, 6, 2 * Cc, generator=g)
    cv_cpu[..., :Cc] = cv_cpu[..., :Cc].clamp(0, 4).exp()
    cv_cpu[4:] = float('nan')                                         # maps no slot points to are not read
    cv = guarded.put(cv_cpu, DEV)
    slot_map = [0, 1, 2, 3, 3, 3, 3]
    mp = guarded.put(torch.tensor(slot_map, dtype=torch.int32), DEV)
    out = guarded.alloc((1, 5, 6, Cc), torch.float32, DEV, 'canary')
    hip.check(hip.lib().usot_conf_fusion_reduce_map_f32(hip.stream(), hip.ptr(cv), hip.ptr(out), 1, M, P, Cc, hip.ptr(mp)), 'reduce_map')
    want = hip.conf_fusion_reduce(cv[torch.tensor(slot_map, device=DEV).long()].contiguous(), 1, M)
    torch.cuda.synchronize()
    guarded.check(start)
    assert torch.isfinite(out).all() and same_bits(out, want)


# --------------------------------------------------------------------------------------------------------------- Session
def _open(net, seed):
    """as tests/test_gpu_tracker.py::_open"""
    from usot_amd.tracker import USOTConfig
    p = USOTConfig()
    p.renew()
    p.sf_size = p.score_size
    t = lambda a: torch.from_numpy(a).to(DEV)
    net.pr_pool = True
    net.template(t(synth.crop(1000 + seed, 1, 127)), template_bbox=torch.tensor([[3.5, 3.5, 10.5, 10.5]]).to(DEV))
    crops = t(synth.crop(2000 + seed, 4, 255))
    roi = torch.tensor([[9.0, 9.0, 16.0, 16.0]]).to(DEV)
    feats = [net.extract_memory_feature(ori_x=crops[0:1], search_bbox=roi),
             net.extract_memory_feature(ori_x=crops[0:1].flip(3), search_bbox=roi)]
    window = np.outer(np.hanning(p.score_size), np.hanning(p.score_size))
    return net.engine.open_session(p, window, feats), crops


def _model(options):
    m = USOT()
    m.load_state_dict(synth.torch_state_dict(m, seed=0, calibrated=True), strict=True)
    m = m.eval().to(DEV)
    m.engine_options['options'] = options
    return m


def _picks(i, n):
    """Frame i of the sequence, n memories stored: frame 0 has one memory (D = 3), frame 5 is hand-made all-distinct (D = 7), the
    others are the tracker's steady state [best, last x 4] (D = 4, D = 3 when best == last)."""
    if i == 5:
        return [0, 1, 2, 3, 4]
    return [max(n - 3, 0)] + [n - 1] * 4


def _eight_frames(options, feats_too=True):
    sess, crops = _open(_model(options), 11)
    outs, dist = [], []
    for i in range(8):
        picks = _picks(i, sess.n)
        dist.append(len({0, 1} | {2 + k for k in picks}))
        outs.append(sess.frame(crops[i % 4], picks, (60.0 + i, 58.0)))
    last = sess.memory_feature(sess.n - 1).clone()                       # flushes: the pooled memory feature of the last frame
    torch.cuda.synchronize()
    rows = 2 + sess.n
    state = (np.array(outs), last.contiguous().cpu().numpy(), sess.bank[:rows].cpu().numpy(), [b[:rows].cpu().numpy() for b in sess.bank_enc])
    return sess, dist, state


@pytest.fixture(scope='module')
def static_session():
    """the 'mem_dedupe' = False session every comparison below shares"""
    sess, dist, state = _eight_frames({'mem_dedupe': False})
    assert not sess.dedupe
    return state


def test_session_on_distinct_rows_under_both_prefills(static_session):
    """Eight frames (D = 3, 4 and 7 among them) on two engines built under the guard, torch.empty = NaN pattern / zeros: finite,
    bit-equal across prefills, guards intact; against the static session the same argmax cell in every frame and results and
    banks within the bars of test_deferred_append_equals_the_append_behind_the_tag."""
    assert engine.DEFAULT_OPTIONS['mem_dedupe'] is True and engine.DEFAULT_OPTIONS['defer_append'] == 2
    res = []
    for prefill in ('canary', 'zero'):
        start = guarded.registry_size()
        with guarded.patched(hip, engine, empty_prefill=prefill):
            sess, dist, state = _eight_frames(None)
            assert sess.dedupe and sess.defer == 2
            assert dist[0] == 3 and 4 in dist and dist[5] == 7, dist
            assert sess.mem_map.cpu().tolist()[0] == dist[-1]
            assert guarded.registry_size() > start
        res.append(state)
        del sess
    a, b = res
    flat = lambda s: [s[0], s[1], s[2]] + list(s[3])
    for x, y in zip(flat(a), flat(b)):
        assert np.isfinite(x).all()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    ref = static_session
    assert np.array_equal(ref[0][:, 0], a[0][:, 0])                                  # the same argmax cell in every frame
    np.testing.assert_allclose(a[0], ref[0], rtol=2e-4, atol=2e-4)
    for x, y in zip(flat(ref)[1:], flat(a)[1:]):
        assert np.abs(x - y).max() <= 2e-5 * max(1.0, np.abs(x).max())


def test_session_unsplit_layout_is_bitwise_the_static_unsplit_session():
    """Both sessions on the tile tuned for the whole convolution and every map unsplit ('conf_tail_split' None against an all-ones
    'conf_map_split'): every copy of a map is then the same computation as its original - result block, pooled memory feature and
    banks bit-equal."""
    _, _, ref = _eight_frames({'mem_dedupe': False, 'conf_tail_split': None})
    sess, _, got = _eight_frames({'mem_dedupe': True, 'conf_map_split': (1,) * 7})
    assert sess.dedupe
    for x, y in zip([ref[0], ref[1], ref[2]] + list(ref[3]), [got[0], got[1], got[2]] + list(got[3])):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_session_log_states_what_the_last_frame_ran():
    """Session.log / f32_bytes (bench.py's roofline): the Conf_Fusion entry follows the distinct rows of the control block last written."""
    sess, crops = _open(_model(None), 11)
    for i in range(6):
        sess.frame(crops[i % 4], _picks(i, sess.n), (60.0, 58.0))
    (i, pix, cout, k), d = sess._conf_log, 7                              # frame 5 was the all-distinct one
    assert sess.log[i][1] == d * pix and sess.log[i][5] == d * pix * cout * k
    sess.frame(crops[0], _picks(6, sess.n), (60.0, 58.0))
    assert sess.log[i][1] == 4 * pix and sess.f32_bytes[i] < 4 * 7 * pix * (256 + cout)
    assert len(sess.log) == len(sess.f32_bytes)
