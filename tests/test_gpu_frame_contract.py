"""GPU: the frame plans under the guard (tests/guarded.py).  Every Builder.buf map, every split-K workspace and every Session
bank of an engine built inside guarded.patched(hip, engine) sits between canaries; each engine is built twice, once with
`torch.empty` meaning the NaN pattern and once meaning zeros, and every leg runs the same inputs on both engines twice in a row
(the second run sees the first run's leftovers).  Asserted per leg: the four results are finite and BIT-equal to each other (a
kernel that reads a pad row nobody wrote, or skips an element, gives prefill-dependent bits or a NaN), every guard is intact
after each run, and the result meets the bar the parent test of that leg holds (1e-4 against the golden / the oracle for the
fp32 frames, the trajectory bars for the sessions, 6e-2 mean-relative for the bf16 backbone).

Bit-equality of two separately built engines is what test_split16_out_of_range_activation_falls_back_to_exact_fp32 and
test_backbone_lp_chains_are_bitwise_the_single_chain already rely on."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import usot_oracle as orc  # noqa: E402
from sampling import check  # noqa: E402
from usot_amd import engine, hip, synth  # noqa: E402
from usot_amd.model import USOT  # noqa: E402

DEV = 'cuda:0'
TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_E2E = os.path.join(HERE, 'golden', 'golden_e2e.npz')
PREFILLS = ('canary', 'zero')


class Info:
    arch = 'USOT'
    dataset = 'SYNTH'
    epoch_test = False
    version = 'v1'


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def npy(x):
    return x.detach().float().cpu().numpy() if x.dtype in (torch.bfloat16, torch.float16) else x.detach().cpu().numpy()


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean() + 1e-30)))


def model(graphs=True, options=None):
    """as tests/test_gpu_model.py::net: synthetic calibrated weights, seed 0"""
    m = USOT()
    m.load_state_dict(synth.torch_state_dict(m, seed=0, calibrated=True), strict=True)
    m.eval()
    m = m.to(DEV)
    m.engine_options['graphs'] = graphs
    if options:
        m.engine_options['options'] = options
    return m


class Runs(object):
    """leg -> the results of its runs (tuples of numpy arrays, in the order canary 1, canary 2, zero 1, zero 2) and what the
    guard check said after each run"""

    def __init__(self):
        self.results, self.guards = {}, {}

    def record(self, leg, start, outs):
        torch.cuda.synchronize()
        self.results.setdefault(leg, []).append(tuple(np.array(npy(o) if isinstance(o, torch.Tensor) else o, order='C') for o in outs))
        try:
            guarded.check(start, clear=False)
        except guarded.GuardError as e:
            self.guards.setdefault(leg, []).append(str(e))

    def verify(self, leg, runs=4):
        assert leg in self.results and len(self.results[leg]) == runs, (leg, len(self.results.get(leg, ())))
        assert not self.guards.get(leg), '\n'.join(self.guards[leg])
        first = self.results[leg][0]
        for k, r in enumerate(self.results[leg]):
            for j, (a, b) in enumerate(zip(r, first)):
                assert np.isfinite(a).all(), '%s: run %d output %d is not finite (%d elements)' % (leg, k, j, int((~np.isfinite(a)).sum()))
                same = a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
                assert same, '%s: output %d of run %d (%s engine) differs from run 0 in %d elements, max |diff| %.3e' % (
                    leg, j, k, PREFILLS[k // 2], int((a != b).sum()), float(np.abs(a.astype(np.float64) - b).max()))
        return first


def both_prefills(build, legs, runs=None):
    """build() -> model, inside guarded.patched(hip, engine, empty_prefill=...); legs(model, record) runs every leg ONCE and is
    called twice per engine"""
    runs = runs or Runs()
    for prefill in PREFILLS:
        start = guarded.registry_size()
        with guarded.patched(hip, engine, empty_prefill=prefill):
            m = build()
            for rep in range(2):
                legs(m, lambda leg, outs: runs.record(leg, start, outs))
            assert guarded.registry_size() > start            # the engine's maps did go through the guard
        del m
    return runs


# ------------------------------------------------------------------------------------------------------ model-level frames
@pytest.fixture(scope='module')
def prpool_ref(oracle_sd):
    """the oracle side of tests/test_gpu_model.py::test_track_with_prpool_vs_oracle, seed 21"""
    seed = 21
    z, x = t(synth.crop(seed, 1, 127)), t(synth.crop(seed + 50, 1, 255))
    zbox = torch.tensor([[3.2, 4.1, 11.3, 10.6]])
    sbox = torch.tensor([[8.5, 9.25, 17.0, 16.5]])
    with torch.no_grad():
        zf = orc.template(oracle_sd, z, zbox, pr_pool=True)
        xf = orc.neck(oracle_sd, orc.backbone(oracle_sd, x))
        memf = orc.prpool_feature(xf, sbox)
        mem = torch.cat([memf] * 3 + [zf] * 4, 0)
        cls, bbox, cm, _ = orc.track(oracle_sd, x, zf, mem, torch.ones(1, 7))
    return dict(z=z, x=x, zbox=zbox, sbox=sbox, zf=zf, xf=xf, memf=memf, mem=mem, cls=cls, bbox=bbox, cm=cm)


@pytest.fixture(scope='module', params=['graph', 'eager', 'graph_split16'])
def frames(request, prpool_ref):
    mode = request.param
    pr = prpool_ref

    def build():
        return model(graphs=mode != 'eager', options={'split16_f32': True} if mode == 'graph_split16' else None)

    def legs(m, record):
        m.pr_pool = False
        m.template(t(synth.crop(0, 1, 127)).to(DEV))
        record('template_127', [m.zf])
        mem, sm = t(synth.memory_kernels(7, 7)).to(DEV), torch.full((1, 7), 0.9, device=DEV)
        record('track_255', m.track(t(synth.crop(1, 1, 255)).to(DEV), template_mem=mem, score_mem=sm))
        record('track_271', m.track(t(synth.crop(3, 1, 271)).to(DEV), template_mem=mem, score_mem=sm))
        record('features_255_b2', [m.engine.features(t(synth.crop(4, 2, 255)).to(DEV))])
        m.pr_pool = True
        m.template(pr['z'].to(DEV), template_bbox=pr['zbox'].to(DEV))
        gm = m.extract_memory_feature(ori_x=pr['x'].to(DEV), search_bbox=pr['sbox'].to(DEV))
        out = m.track(pr['x'].to(DEV), template_mem=pr['mem'].to(DEV), score_mem=torch.ones(1, 7, device=DEV))
        gm2 = m.extract_memory_feature(xf=out[3], search_bbox=pr['sbox'].to(DEV))
        record('prpool', [m.zf, gm] + list(out) + [gm2])
    return both_prefills(build, legs)


def test_template_127(frames, gold_model):
    zf, = frames.verify('template_127')
    check('template_crop/zf', gold_model, zf, TOL)


def test_track_with_memory_255(frames, gold_model):
    cls, bbox, cm, xf = frames.verify('track_255')
    for nm, a in (('cls', cls), ('bbox', bbox), ('cls_mem', cm), ('xf', xf)):
        check('track_mem/' + nm, gold_model, a, TOL)


def test_track_with_memory_271(frames, gold_model):
    cls, bbox, cm, xf = frames.verify('track_271')
    for nm, a in (('cls', cls), ('bbox', bbox), ('cls_mem', cm)):
        check('track_mem_271/' + nm, gold_model, a, TOL)


def test_features_255_batch_2(frames, gold_model):
    xf, = frames.verify('features_255_b2')
    check('backbone_255_b2/neck', gold_model, xf, TOL)


def test_track_with_prpool(frames, prpool_ref):
    zf, gm, cls, bbox, cm, xf, gm2 = frames.verify('prpool')
    pr = prpool_ref
    assert gm.shape == (1, 256, 7, 7)
    for got, ref in ((zf, pr['zf']), (gm, pr['memf']), (xf, pr['xf']), (cls, pr['cls']), (bbox, pr['bbox']), (cm, pr['cm']), (gm2, pr['memf'])):
        assert rel(got, ref.numpy()) < TOL


# ------------------------------------------------------------------------------------------------------ sessions
def test_session_three_frames():
    """One Session (the fused tracker's device-resident state: banks, control block, the frame graph) stepped 3 frames on the
    golden video 0, against the reference tracker's trajectory at the bars of test_trajectory_vs_reference_tracker."""
    from usot_amd.tracker import USOTTracker
    with np.load(GOLD_E2E) as z:
        seed, _, w, h = z['video0/seed_frames_sz']
        want = z['video0/track']

    def legs(m, record):
        trk = USOTTracker(Info())
        trk.fused = True
        im, (cx, cy) = synth.frame(int(seed), t=0)
        state = trk.init(im, np.array([cx, cy]), np.array([float(w), float(h)]), m)
        assert 'session' in state
        rows = [[cx, cy, w, h, 0.0]]
        for f in range(1, 4):
            state = trk.track(state, synth.frame(int(seed), t=f)[0])
            rows.append([*state['target_pos'], *state['target_sz'], float(state['cls_score'])])
        record('session', [np.array(rows, np.float64)])
    got, = both_prefills(model, legs).verify('session')
    np.testing.assert_allclose(got[:, :4], want[:4, :4], atol=2e-2, rtol=0)
    np.testing.assert_allclose(got[:, 4], want[:4, 4], atol=2e-4, rtol=0)


def test_batch_session_three_slots_two_frames():
    """One BatchSession with 3 slots (the golden video 0 beside two filler videos) stepped 2 frames in lock step, at the bars of
    test_lockstep_trajectory_vs_reference_tracker."""
    from usot_amd.multitrack import MultiVideoTracker
    with np.load(GOLD_E2E) as z:
        seed, _, w, h = z['video0/seed_frames_sz']
        want = z['video0/track']
        inst = int(z['video0/instance_size'])
    fsz = (52.0, 38.0) if inst == 255 else (16.0, 12.0)

    def legs(m, record):
        mt = MultiVideoTracker(Info(), m, slots=3, capacity=64)
        seeds = [301, int(seed), 302]
        keys = []
        for s in seeds:
            im, (cx, cy) = synth.frame(s, t=0)
            keys.append(mt.add(im, np.array([cx, cy]), np.array([float(w), float(h)] if s == int(seed) else fsz)))
        rows = {k: [] for k in keys}
        for f in (1, 2):
            states = mt.track({k: synth.frame(s, t=f)[0] for k, s in zip(keys, seeds)})
            for k in keys:
                st = states[k]
                rows[k].append([*st['target_pos'], *st['target_sz'], float(st['cls_score'])])
        assert mt.session(inst) is not None and sum(mt.session(inst).book.active) == 3
        record('batch_session', [np.array(rows[k], np.float64) for k in keys])
    _, got, _ = both_prefills(model, legs).verify('batch_session')
    np.testing.assert_allclose(got[:, :4], want[1:3, :4], atol=2e-2, rtol=0)
    np.testing.assert_allclose(got[:, 4], want[1:3, 4], atol=2e-4, rtol=0)


# ------------------------------------------------------------------------------------------------------ bf16 backbone
@pytest.fixture(scope='module')
def neck_ref(oracle_sd):
    x = t(synth.crop(40, 2, 255))
    with torch.no_grad():
        return x, orc.neck(oracle_sd, orc.backbone(oracle_sd, x)).numpy()


@pytest.mark.parametrize('options', [{}, {'lp_chains': 2}], ids=['one_chain', 'lp_chains2'])
def test_backbone_bf16_batch_2(options, neck_ref):
    x, ref = neck_ref

    def legs(m, record):
        record('bf16', [m.engine.features_bf16(x.to(DEV))])
    got, = both_prefills(lambda: model(options=options), legs).verify('bf16')
    assert got.shape == ref.shape
    assert np.abs(got - ref).mean() / np.abs(ref).mean() < 6e-2              # test_backbone_bf16_tracks_fp32's bar
    assert np.corrcoef(got.reshape(-1), ref.reshape(-1))[0, 1] > 0.999
