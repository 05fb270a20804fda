"""GPU: lock-step multi-video tracking (csrc/multitrack.hip, engine.BatchSession, multitrack.MultiVideoTracker).

The three batched kernels against their single-frame kernels (bitwise, per slot) and torch indexing; slot isolation; the
reference trajectories of tests/golden/golden_e2e*.npz tracked beside filler videos in reused slots; flush(); the step graph's
shape; the opt-in fp16 backbone; track_dataset on a synthetic dataset."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from usot_amd import hip, synth  # noqa: E402
from usot_amd.engine import SLOT_REC, STEP_HDR, Engine, crop_fields  # noqa: E402
from usot_amd.io_utils import cxy_wh_2_rect  # noqa: E402
from usot_amd.model import USOT  # noqa: E402
from usot_amd.multitrack import MultiVideoTracker, track_dataset  # noqa: E402
from usot_amd.tracker import USOTConfig  # noqa: E402

DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'golden_e2e.npz')
GOLD_LONG = os.path.join(HERE, 'golden', 'golden_e2e_long.npz')


class Info:
    arch = 'USOT'
    dataset = 'SYNTH'
    epoch_test = False
    version = 'v1'


@pytest.fixture(scope='module')
def net():
    m = USOT()
    m.load_state_dict(synth.torch_state_dict(m, seed=0, calibrated=True), strict=True)
    m.eval()
    return m.cuda()


def _ctl(B, tag=7.0):
    ctl = np.zeros(STEP_HDR + B * SLOT_REC.itemsize, np.uint8)
    ctl[:8].view(np.float64)[0] = tag
    return ctl, ctl[STEP_HDR:].view(SLOT_REC)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.fixture
def guards():
    """The guarded.alloc / guarded.put buffers a kernel test hands to the raw entry points are checked, and forgotten, when the
    test ends - also when one of its own assertions failed first."""
    with guarded.patched():
        yield


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('S', [25, 27])
def test_decode_batch_bitwise_vs_decode_dev(S, B, guards):
    g = np.random.default_rng(100 * S + B)
    cls = g.standard_normal((B, S, S)).astype(np.float32)
    cm = g.standard_normal((B, S, S)).astype(np.float32)
    bbox = (20 * np.exp(0.4 * g.standard_normal((B, 4, S, S)))).astype(np.float32)
    ctl, recs = _ctl(B, tag=41.0)
    recs['tsz'] = g.uniform(20, 90, (B, 2))
    c = S // 2
    tie = ((c - 1) * S + c, (c + 1) * S + c)
    for b in range(B):
        kind = b % 3
        if kind == 0:        # an exact tie of the best penalised score at two cells the cosine window weighs alike: first wins
            for i in tie:
                cls[b].flat[i] = cm[b].flat[i] = 12.0
                bbox[b, :, i // S, i % S] = 18.0
            recs[b]['tsz'] = (36.0, 36.0)          # the tie cells' boxes: no size / ratio penalty
        elif kind == 1:      # NaNs: the first one wins
            cls[b, 9, 3] = np.nan
            cm[b, 20, 1] = np.nan
    window = np.outer(np.hanning(S), np.hanning(S))
    wd = torch.from_numpy(window).reshape(-1).to(DEV)
    p = USOTConfig()
    size = 255 if S == 25 else 271
    out = guarded.alloc((B, 16), torch.float64, DEV, 'zero')            # outputs handed to the raw entry points: between canaries
    roi = guarded.alloc((B, 5), torch.float32, DEV, 'zero')
    dcls, dcm, dbox = (torch.from_numpy(a).to(DEV) for a in (cls, cm, bbox))
    hip.decode_batch(dcls, dcm, dbox, wd, out, torch.from_numpy(ctl).to(DEV), roi, S, size, 8, p.ratio, p.penalty_k,
                     p.window_influence)
    o, r_ = out.cpu().numpy(), roi.cpu().numpy()
    for b in range(B):
        c8 = torch.zeros(8, dtype=torch.float64, device=DEV)
        c8[0], c8[1], c8[6] = float(recs[b]['tsz'][0]), float(recs[b]['tsz'][1]), 41.0
        ref = guarded.alloc((10,), torch.float64, DEV, 'zero')
        rroi = guarded.alloc((5,), torch.float32, DEV, 'zero')
        hip.check(hip.lib().usot_decode_dev_f32(hip.stream(), hip.ptr(dcls[b]), hip.ptr(dcm[b]), hip.ptr(dbox[b]), hip.ptr(wd),
                                                hip.ptr(ref), S, size, 8, C.c_float(p.ratio), C.c_double(p.penalty_k),
                                                C.c_double(p.window_influence), hip.ptr(c8), hip.ptr(rroi)), 'decode_dev')
        ref, rroi = ref.cpu().numpy(), rroi.cpu().numpy()
        assert np.array_equal(_bits(o[b, :8]), _bits(ref[:8])), (b, o[b, :8], ref[:8])
        assert o[b, 8] == 41.0
        assert r_[b, 0] == b and np.array_equal(_bits(r_[b, 1:]), _bits(rroi[1:]))
        if b % 3 == 0:
            assert int(o[b, 0]) == tie[0]
        if b % 3 == 1:
            assert int(o[b, 0]) == 9 * S + 3


def test_append_gather_batch_vs_torch_indexing(guards):
    B, cap, nq = 3, 10, 7
    lens = [7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 5 * 3 * 256]
    g = torch.Generator().manual_seed(5)
    banks = [guarded.put(torch.randn(B * cap, n, generator=g), DEV) for n in lens]
    fresh = [torch.randn(B, n, generator=g).to(DEV) for n in lens]
    picked = [guarded.alloc((B * nq, n), torch.float32, DEV, 'full', float('nan')) for n in lens[1:]]
    ctl, recs = _ctl(B)
    app = [4, 19, 25]                                 # slot 1 appends to its scratch row (nothing pending)
    picks = [[0, 1, 2, 3, 4, 4, 2],                   # the appended row, twice
             [10, 11, 12, 19, 19, 13, 12],            # the scratch row that is being appended to
             [20, 21, 22, 29, 25, 23, 24]]            # slot 2's scratch row while it appends elsewhere: the bank's row
    for b in range(B):
        recs[b]['append_row'] = app[b]
        recs[b]['picks'][:nq] = picks[b]
    before = [t.clone() for t in banks]
    hip.rows_append_gather_batch(fresh, banks, picked, torch.from_numpy(ctl).to(DEV), nq)
    for k in range(4):
        want = before[k].clone()
        for b in range(B):
            want[app[b]] = fresh[k][b]
        assert torch.equal(banks[k], want), k
        if k:
            wp = torch.stack([fresh[k][b] if r == app[b] else before[k][r] for b in range(B) for r in picks[b]])
            assert torch.equal(picked[k - 1], wp), k


def test_crop_batch_vs_single_crop(guards):
    im, _ = synth.frame(5, t=3)
    im2, _ = synth.frame(9, h=240, w=320, t=1)
    S = 255
    cases = [(im, (240.3, 180.7), 301), (im, (10.2, 8.9), 255), (im, (-400.0, -300.0), 301), (im, (240.0, 180.0), 510),
             (im2, (300.0, 10.0), 188), (im2, (160.0, 120.0), 612), (im, (470.0, 350.0), 127), (im2, (100.5, 100.5), 271)]
    B = len(cases) + 1                                 # the last slot names no image: left untouched
    ctl, recs = _ctl(B)
    devs = []
    refs = []
    for b, (img, pos, win) in enumerate(cases):
        d = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
        devs.append(d)
        avg = np.mean(img, axis=(0, 1))
        x0, y0, w_, fill = crop_fields(img.shape, pos, win, avg)
        recs[b]['im'], recs[b]['H'], recs[b]['W'] = d.data_ptr(), img.shape[0], img.shape[1]
        recs[b]['x0'], recs[b]['y0'], recs[b]['win'], recs[b]['fill'] = x0, y0, w_, fill
        ref = guarded.alloc((3, S, S), torch.float32, DEV)
        hip.crop_resize(d, ref, x0, y0, w_, fill)
        refs.append(ref)
    out = guarded.alloc((B, 3, S, S), torch.float32, DEV, 'full', -7.0)
    hip.crop_resize_batch(torch.from_numpy(ctl).to(DEV), out)
    for b in range(len(cases)):
        assert torch.equal(out[b], refs[b]), cases[b][1:]
    assert bool((out[-1] == -7.0).all())


# ------------------------------------------------------------------------------------------------------------ sessions
def _filler_sz(inst):
    return (52.0, 38.0) if inst == 255 else (16.0, 12.0)       # a target area ratio that selects the same instance size


class Lockstep(object):
    """A MultiVideoTracker with three filler videos beside the video under test (its key `key`)."""

    def __init__(self, net, inst, slots=4, capacity=1024, backbone_dtype=torch.float32):
        self.mt = MultiVideoTracker(Info(), net, slots=slots, capacity=capacity, backbone_dtype=backbone_dtype)
        self.inst, self.fillers, self.seed = inst, {}, 300

    def add_filler(self):
        self.seed += 1
        im, (cx, cy) = synth.frame(self.seed, t=0)
        k = self.mt.add(im, np.array([cx, cy]), np.array(_filler_sz(self.inst)))
        self.fillers[k] = [self.seed, 1]
        return k

    def drop_filler(self):
        k = next(iter(self.fillers))
        slot = self.mt.slot(k)
        self.mt.remove(k)
        del self.fillers[k]
        return slot

    def frames(self):
        fr = {}
        for k, st in self.fillers.items():
            fr[k] = synth.frame(st[0], t=st[1])[0]
            st[1] += 1
        return fr


def _lockstep_video(net, z, vid, nframes, forced=False, capacity=1024, npz_track=None):
    """The fixture's video tracked in lock step: 4 fillers take the slots, one ends and the video is loaded into its reused
    slot; half way another filler ends and a new one takes its slot."""
    seed, _, w, h = z['video%d/seed_frames_sz' % vid]
    inst = int(z['video%d/instance_size' % vid])
    want = z['video%d/track' % vid]
    ls = Lockstep(net, inst, capacity=capacity)
    for _ in range(4):
        ls.add_filler()
    for _ in range(2):
        ls.mt.track(ls.frames())
    slot = ls.drop_filler()
    im, (cx, cy) = synth.frame(int(seed), t=0)
    key = ls.mt.add(im, np.array([cx, cy]), np.array([float(w), float(h)]))
    assert ls.mt.slot(key) == slot
    bs = ls.mt.session(inst)
    assert bs is not None and sum(bs.book.active) == 4
    rows = [[cx, cy, w, h, 0.0]]
    for f in range(1, nframes):
        if f == nframes // 2:
            ls.drop_filler()
            ls.add_filler()
        if forced:
            st = ls.mt.state(key)
            st['target_pos'] = want[f - 1, :2].copy()
            st['target_sz'] = want[f - 1, 2:4].copy()
        fr = ls.frames()
        fr[key] = synth.frame(int(seed), t=f)[0]
        st = ls.mt.track(fr)[key]
        rows.append([*st['target_pos'], *st['target_sz'], float(st['cls_score'])])
    return np.array(rows), ls.mt.state(key), ls, key


@pytest.mark.parametrize('vid', [0, 1])
def test_lockstep_trajectory_vs_reference_tracker(net, vid):
    with np.load(GOLD) as zz:
        z = {k: zz[k] for k in zz.files}
    want = z['video%d/track' % vid]
    n = int(z['video%d/seed_frames_sz' % vid][1])
    got, state, ls, key = _lockstep_video(net, z, vid, n)
    assert state['p'].instance_size == int(z['video%d/instance_size' % vid])
    np.testing.assert_allclose(got[:, :4], want[:, :4], atol=2e-2, rtol=0)
    np.testing.assert_allclose(got[:, 4], want[:, 4], atol=2e-4, rtol=0)
    assert len(state['memory_confidences']) == n and len(state['memory_features']) == n


@pytest.mark.parametrize('vid', [0, 1])
def test_lockstep_500_frame_video_vs_reference_tracker(net, vid):
    """The rules of test_gpu_tracker.py::test_500_frame_video_vs_reference_tracker in lock step: free-running up to the first
    near-tie, then teacher-forced over all 499 steps at capacity 128 (every slot's banks grow 128 -> 512 rows)."""
    with np.load(GOLD_LONG) as zz:
        z = {k: zz[k] for k in zz.files}
    want = z['video%d/track' % vid]
    n = int(z['video%d/seed_frames_sz' % vid][1])
    m_tol, r_tol, p_tol = z['video%d/tolerances' % vid]
    mg, rs, ps = z['video%d/margins' % vid], z['video%d/round_slack' % vid], z['video%d/pick_slack' % vid]
    near = np.nonzero((mg < m_tol) | (rs < r_tol) | (ps < p_tol))[0] + 1
    first = int(near[0]) if len(near) else n
    got, _, _, _ = _lockstep_video(net, z, vid, first)
    np.testing.assert_allclose(got[:, :4], want[:first, :4], atol=2e-2, rtol=0)
    np.testing.assert_allclose(got[:, 4], want[:first, 4], atol=2e-4, rtol=0)
    got, state, ls, key = _lockstep_video(net, z, vid, n, forced=True, capacity=128)
    assert state['p'].instance_size == (255, 271)[vid]
    clear = np.concatenate([[True], (mg >= m_tol) & (ps >= p_tol)])
    dpos = np.abs(got[:, :4] - want[:, :4]).max(1)
    dsc = np.abs(got[:, 4] - want[:, 4])
    bad = np.nonzero(clear & ((dpos > 2e-2) | (dsc > 2e-4)))[0]
    assert len(bad) == 0, (bad[:10], dpos[bad[:10]], dsc[bad[:10]])
    assert (dsc[~clear] < 2e-4).mean() > 0.5 if (~clear).any() else True
    bs = ls.mt.session((255, 271)[vid])
    assert bs.cap >= n + 3 and bs.book.n[ls.mt.slot(key)] == n and len(state['memory_features']) == n
    np.testing.assert_allclose(np.asarray(state['memory_confidences'], np.float64)[1:], got[1:, 4], atol=0, rtol=0)


def test_slot_isolation(net):
    """golden_e2e_long video 0, teacher-forced for 30 steps in slot 1 of 4: the same bits whether the other slots track
    videos or sit idle."""
    with np.load(GOLD_LONG) as zz:
        z = {k: zz[k] for k in zz.files}
    seed, _, w, h = z['video0/seed_frames_sz']
    want = z['video0/track']

    def run(busy):
        ls = Lockstep(net, 255, capacity=64)
        ls.add_filler()                               # slot 0
        im, (cx, cy) = synth.frame(int(seed), t=0)
        key = ls.mt.add(im, np.array([cx, cy]), np.array([float(w), float(h)]))
        assert ls.mt.slot(key) == 1
        if busy:
            ls.add_filler()
            ls.add_filler()
        else:
            ls.drop_filler()
        rows = []
        for f in range(1, 31):
            st = ls.mt.state(key)
            st['target_pos'] = want[f - 1, :2].copy()
            st['target_sz'] = want[f - 1, 2:4].copy()
            fr = ls.frames() if busy else {}
            fr[key] = synth.frame(int(seed), t=f)[0]
            st = ls.mt.track(fr)[key]
            rows.append(np.concatenate([st['target_pos'], st['target_sz'], [float(st['cls_score'])]]))
        bs = ls.mt.session(255)
        assert sum(bs.book.active) == (4 if busy else 1)
        return np.array(rows)
    a, b = run(True), run(False)
    assert np.array_equal(_bits(a), _bits(b)), np.abs(a - b).max()


def test_flush_equals_the_in_graph_append(net):
    with np.load(GOLD) as zz:
        seed, n, w, h = zz['video0/seed_frames_sz']
    ls = Lockstep(net, 255, slots=2)
    im, (cx, cy) = synth.frame(int(seed), t=0)
    key = ls.mt.add(im, np.array([cx, cy]), np.array([float(w), float(h)]))
    for f in range(1, 4):
        ls.mt.track({key: synth.frame(int(seed), t=f)[0]})
    bs, slot = ls.mt.session(255), ls.mt.slot(key)
    assert bs.book.pending[slot] and bs.book.n[slot] == 4
    row = bs.book.row(slot, 2 + 3)
    prev = bs.book.prev_row[slot]
    assert prev == row
    bs.flush()
    flushed = [bs.bank[row].clone()] + [e[row].clone() for e in bs.bank_enc]
    # the same pending feature appended by the next step's graph instead
    bs.bank[row].zero_()
    for e in bs.bank_enc:
        e[row].zero_()
    bs.book.pending[slot], bs.book.prev_row[slot] = True, row
    ls.mt.track({key: synth.frame(int(seed), t=4)[0]})
    torch.cuda.synchronize()
    ingraph = [bs.bank[row]] + [e[row] for e in bs.bank_enc]
    for a, b in zip(flushed, ingraph):
        assert torch.equal(a, b)
    mf = ls.mt.state(key)['memory_features']
    assert len(mf) == 5
    init = ls.mt.state(key)['init_features'][0]
    assert torch.equal(mf[0], init)                  # memory 0 = the init feature (bank row 2)
    for i in range(5):
        r = bs.book.row(slot, 2 + i)
        assert torch.equal(mf[i], bs.bank[r:r + 1].permute(0, 3, 1, 2))
    assert float(mf[4].abs().sum()) > 0          # the last feature: flushed on read


def _p255():
    p = USOTConfig()
    p.instance_size = 255
    p.renew()
    p.sf_size = p.score_size
    return p, np.outer(np.hanning(p.score_size), np.hanning(p.score_size))


K_PRROI, K_DECB, K_ROWSAGB, K_CROPB = 5, 33, 34, 35          # plan op kinds (csrc/plan.hip)


def _kinds(h):
    L = hip.lib()
    info = (C.c_int * 4)()
    out = []
    for i in range(L.usot_plan_size(h)):
        hip.check(L.usot_plan_op_info(h, i, info), 'usot_plan_op_info')
        out.append(info[0])
    return out


def test_step_graph_per_video_work_is_one_launch_per_kind(net):
    """The per-video work of a step - crop, append + gather, decode, PrRoIPool - is ONE launch each at 2 and at 8 slots: the
    step graph is the batch-B backbone + heads + encoders (whose lowering follows the batch's conv shapes, Builder) plus
    exactly those four.  An engine with split16_f32 on still builds an exact-fp32 step graph (no range word)."""
    from usot_amd.engine import KGEO, Builder
    p, window = _p255()
    e = net.engine
    sessions = [e.open_batch_session(p, window, B, capacity=16) for B in (2, 8)]
    for B, bs in zip((2, 8), sessions):
        k = _kinds(bs.plan.h)
        assert [k.count(x) for x in (K_CROPB, K_ROWSAGB, K_DECB, K_PRROI)] == [1, 1, 1, 1], (B, k)
        bld = Builder(e.W, e.tuning, 0, bs.opt)
        x, feat = bld.buf(B, 3, 255, 255), bld.buf(B, 7, 7, 256)
        mk = [bld.buf(B * 7, hk, wk, 256) for hk, wk in KGEO]
        bld.encode_kernel(feat, B, 256, 'mem')
        xf, hf = bld.backbone(x, B, 255, need_stem=False)
        bld.heads(xf, B, hf, bs.zk, bld.buf(1), 7, mk=mk)
        assert len(k) == hip.lib().usot_plan_size(bld.plan.h) + 4, (B, len(k))
    e16 = Engine(net, DEV, options={'split16_f32': True})
    bs = e16.open_batch_session(p, window, 2, capacity=16)
    assert e16.opt['split16_f32'] and not bs.opt['split16_f32']
    assert _kinds(bs.plan.h) == _kinds(sessions[0].plan.h)


def test_fp16_backbone_vs_exact(net):
    p, window = _p255()
    e = net.engine
    B = 2
    z = torch.from_numpy(synth.crop(41, 1, 127)).to(DEV)
    net.pr_pool = False
    net.template(z)
    net.pr_pool = True
    feats = [torch.from_numpy(synth.memory_kernels(42 + i, 1)).to(DEV) for i in range(2)]
    x = torch.from_numpy(synth.crop(43, B, 255))
    out = {}
    for dt in (torch.float32, torch.float16):
        bs = e.open_batch_session(p, window, B, capacity=16, backbone_dtype=dt)
        for s in range(B):
            bs.load(s, net.zf, feats)
        res = bs.step({s: dict(crop=x[s], picks=[0] * 5, tsz=(40.0, 30.0)) for s in range(B)})
        torch.cuda.synchronize()
        assert sorted(res) == list(range(B))
        out[dt] = dict(cls=bs.cls2[0].cpu().numpy(), cls_mem=bs.cls2[1].cpu().numpy(), bbox=bs.bbox.cpu().numpy(),
                       xf=bs.xf.float().cpu().numpy())
    a, b = out[torch.float32], out[torch.float16]
    for nm in ('cls', 'cls_mem', 'bbox', 'xf'):
        assert np.isfinite(b[nm]).all() and np.isfinite(a[nm]).all(), nm
    for s in range(B):
        for nm in ('cls', 'cls_mem', 'xf', 'bbox'):
            g_, r_ = b[nm][s], a[nm][s]                 # every map is [B, ...]
            if nm == 'bbox':
                g_, r_ = np.log(g_), np.log(r_)
            rel = np.abs(g_ - r_).mean() / np.abs(r_).mean()
            assert rel <= (1.5e-2 if nm == 'cls_mem' else 1e-2), (s, nm, rel)


def test_track_dataset_synthetic_matches_reference_trajectory(net):
    with np.load(GOLD_LONG) as zz:
        z = {k: zz[k] for k in zz.files}
    seed, n, w, h = z['video0/seed_frames_sz']
    want = z['video0/track']
    m_tol, r_tol, p_tol = z['video0/tolerances']
    mg, rs, ps = z['video0/margins'], z['video0/round_slack'], z['video0/pick_slack']
    near = np.nonzero((mg < m_tol) | (rs < r_tol) | (ps < p_tol))[0] + 1
    first = int(near[0]) if len(near) else int(n)
    _, (cx, cy) = synth.frame(int(seed), t=0)
    gt0 = np.array([cx - float(w) / 2, cy - float(h) / 2, float(w), float(h)])
    ds = {'gold': {'image_files': [(int(seed), f) for f in range(first)], 'gt': [gt0] * first, 'name': 'gold'}}
    for i in range(3):                                # fillers: more videos than slots, refilled as they end
        _, (fx, fy) = synth.frame(500 + i, t=0)
        ds['f%d' % i] = {'image_files': [(500 + i, f) for f in range(5 + 3 * i)],
                         'gt': [np.array([fx - 26.0, fy - 19.0, 52.0, 38.0])] * (5 + 3 * i), 'name': 'f%d' % i}
    regions = track_dataset(net, ds, slots=2, imread=lambda fn: synth.frame(fn[0], t=fn[1])[0])
    assert sorted(regions) == sorted(ds) and all(len(regions[k]) == len(ds[k]['image_files']) for k in ds)
    got = np.array(regions['gold'][1:], np.float64)
    ref = np.array([cxy_wh_2_rect(want[f, :2], want[f, 2:4]) for f in range(1, first)])
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=0)
