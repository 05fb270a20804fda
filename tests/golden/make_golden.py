#!/usr/bin/env python3
"""Generate the golden fixtures by importing the REFERENCE's own lib/models on PyTorch-CPU.

Runs only in the build container (needs /root/reference).  Nothing from the reference
is written into this repo except numeric inputs/outputs.  Harness-side patches, applied
in this process only:
  1. Tensor.cuda / Module.cuda become identity (models.py:119-120, connect.py:219 call
     .cuda() at construct time);
  2. the PrRoIPool JIT loader is replaced by a raising stub (its hipify step would write
     into /root/reference);
  3. forward passes run under no_grad and eval().

Usage:  python tests/golden/make_golden.py [calib] [model] [host] [e2e] [datasets] [family] [model64] [e2e_long]
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True    # never leave __pycache__ inside /root/reference

import numpy as np

REF = '/root/reference'
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(REPO, 'tests', 'golden')
# `lib` must resolve to the REFERENCE here.  The reference's lib/ has no __init__.py (a
# namespace package) while this repo's lib/ is a regular package, which would win whatever
# the path order — so the repo root joins sys.path only after the reference is imported.
sys.path = [p for p in sys.path if os.path.realpath(p or '.') not in (REPO, os.path.realpath('.'))] \
    if os.path.realpath('.') == REPO else sys.path
sys.path.insert(0, REF)

import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self

import lib.models.prroi_pool.functional as _prf  # noqa: E402


def _no_jit():
    raise RuntimeError('PrRoIPool JIT build is disabled in the golden harness')


_prf._import_prroi_pooling = _no_jit

import lib.models.models as ref_models  # noqa: E402
import lib.models.connect  # noqa: E402,F401

sys.path.insert(1, REPO)
sys.path.insert(2, GOLD)
from usot_amd import synth  # noqa: E402
from sampling import summarize  # noqa: E402
import golden_parts  # noqa: E402

assert ref_models.__file__.startswith(REF), ref_models.__file__
torch.manual_seed(0)
torch.set_num_threads(8)


def build(calibrated, family='zero_dc'):
    net = ref_models.USOT()
    sd = synth.torch_state_dict(net, seed=0, calibrated=calibrated, family=family)
    missing = net.load_state_dict(sd, strict=True)
    return net, sd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def do_calib(family='zero_dc'):
    """One train-mode pass with momentum 1 so running stats == batch stats of this input."""
    net, _ = build(calibrated=False, family=family)
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(os.path.join(GOLD, 'state_dict_keys.json'), 'w') as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = 1.0
    net.pr_pool = False
    with torch.no_grad():
        net.template(t(synth.crop(100, 8, 127)))
        mem = t(synth.memory_kernels(102, 56))
        net.track(t(synth.crop(101, 8, 255)), template_mem=mem, score_mem=torch.ones(8, 7))
    out = {k: v.numpy() for k, v in net.state_dict().items()
           if k.endswith('running_mean') or k.endswith('running_var')}
    os.makedirs(synth.DATA_DIR, exist_ok=True)
    np.savez_compressed(synth.calib_file(family), **out)
    print('calibration: %d tensors -> %s' % (len(out), synth.calib_file(family)))


def do_model():
    net, sd = build(calibrated=True)
    net.eval()
    net.pr_pool = False
    g = {}
    with torch.no_grad():
        # a1-a3 backbone at the three crop sizes (+ batch 2 at 255)
        for size, b, seed in ((127, 1, 0), (255, 1, 1), (271, 1, 3), (255, 2, 4)):
            stages, p3 = net.feature_extractor(t(synth.crop(seed, b, size)))
            tag = 'backbone_%d_b%d' % (size, b)
            for nm, ten in zip(('stem', 'p1', 'p2'), stages):
                g.update(summarize('%s/%s' % (tag, nm), ten.numpy()))
            g.update(summarize(tag + '/p3', p3.numpy()))
            g.update(summarize(tag + '/neck', net.neck(p3).numpy()))
        # a10 template with the centre-crop neck (PrPool has no CPU reference)
        net.template(t(synth.crop(0, 1, 127)))
        zf = net.zf.clone()
        g.update(summarize('template_crop/zf', zf.numpy()))
        # a11 track: offline only, and with N_q = 7 memory, batch 1; 271 crop
        x = t(synth.crop(1, 1, 255))
        mem = t(synth.memory_kernels(7, 7))
        cls, bbox, none1, none2 = net.track(x)
        assert none1 is None and none2 is None
        g.update(summarize('track_offline/cls', cls.numpy()))
        g.update(summarize('track_offline/bbox', bbox.numpy()))
        cls, bbox, cls_mem, xf = net.track(x, template_mem=mem, score_mem=torch.full((1, 7), 0.9))
        for nm, ten in (('cls', cls), ('bbox', bbox), ('cls_mem', cls_mem), ('xf', xf)):
            g.update(summarize('track_mem/' + nm, ten.numpy()))
        x271 = t(synth.crop(3, 1, 271))
        cls, bbox, cls_mem, xf = net.track(x271, template_mem=mem, score_mem=torch.full((1, 7), 0.9))
        for nm, ten in (('cls', cls), ('bbox', bbox), ('cls_mem', cls_mem)):
            g.update(summarize('track_mem_271/' + nm, ten.numpy()))
        # batch 2 (two templates, 14 memory kernels)
        net.template(t(synth.crop(5, 2, 127)))
        mem2 = t(synth.memory_kernels(8, 14))
        cls, bbox, cls_mem, xf = net.track(t(synth.crop(4, 2, 255)), template_mem=mem2,
                                           score_mem=torch.full((2, 7), 0.9))
        for nm, ten in (('cls', cls), ('bbox', bbox), ('cls_mem', cls_mem)):
            g.update(summarize('track_mem_b2/' + nm, ten.numpy()))
        # a5-a9 head pieces on seeded feature maps
        cm = net.connect_model
        xf = t(synth.memory_kernels(20, 1, 256, 31))
        zk = t(synth.memory_kernels(21, 1))
        mk = t(synth.memory_kernels(22, 7))
        cz, cx = cm.cls_encode(zk, xf)
        for i, nm in enumerate(('11', '12', '21')):
            g.update(summarize('enc/cls_s' + nm, cx[i].numpy()))
            g.update(summarize('enc/cls_k' + nm, cz[i].numpy()))
        rz, rx = cm.reg_encode(zk, xf)
        for i, nm in enumerate(('11', '12', '21')):
            g.update(summarize('enc/reg_s' + nm, rx[i].numpy()))
        g.update(summarize('groupdw/cls', cm.cls_dw(cz, cx).numpy()))
        g.update(summarize('groupdw/reg', cm.reg_dw(rz, rx).numpy()))
        mz, _ = cm.cls_encode(mk, None)
        rep = [c.repeat(7, 1, 1, 1) for c in cx]
        dwm = cm.cls_dw(mz, rep)
        g.update(summarize('groupdw/mem', dwm.numpy()))
        g.update(summarize('conf_fusion/out', cm.conf_fusion(dwm.view(1, 7, 256, 25, 25)).numpy()))
        g.update(summarize('tower/bbox', cm.bbox_tower(dwm[:1]).numpy()))
        # a6 xcorr_depthwise alone, the geometries on the path (+ the 271 one)
        from lib.models.connect import xcorr_depthwise
        for i, (hx, wx, hk, wk) in enumerate(((29, 29, 5, 5), (27, 29, 3, 5), (29, 27, 5, 3),
                                              (31, 31, 5, 5), (12, 9, 4, 2))):
            gx = np.random.default_rng(900 + i)
            xa = gx.standard_normal((2, 24, hx, wx)).astype(np.float32)
            ka = gx.standard_normal((2, 24, hk, wk)).astype(np.float32)
            g['xcorr%d/x' % i], g['xcorr%d/k' % i] = xa, ka
            g['xcorr%d/out' % i] = xcorr_depthwise(t(xa), t(ka)).numpy()
    files = golden_parts.save(os.path.join(GOLD, 'golden_model.npz'), g)
    print('model goldens: %d arrays, %.1f KB in %d parts' % (len(g), sum(os.path.getsize(f) for f in files) / 1024, len(files)))


def _import_ref_tracker(resize=None):
    """Import lib.tracker.usot_tracker with import-only shims for cv2 / imgaug."""
    cv2 = types.ModuleType('cv2')

    def _resize(img, size, *a, **k):
        if resize is None:
            raise RuntimeError('cv2.resize reached in a golden that must not need it')
        return resize(img, size)
    cv2.resize = _resize
    sys.modules['cv2'] = cv2

    ia = types.ModuleType('imgaug')
    iaa = types.ModuleType('imgaug.augmenters')
    bbs = types.ModuleType('imgaug.augmentables.bbs')
    aug = types.ModuleType('imgaug.augmentables')

    class BoundingBox:
        def __init__(self, x1, y1, x2, y2):
            self.x1, self.y1, self.x2, self.y2 = x1, y1, x2, y2

    class BoundingBoxesOnImage:
        def __init__(self, boxes, shape):
            self.bounding_boxes, self.shape = boxes, shape

        def __getitem__(self, i):
            return self.bounding_boxes[i]

    class Fliplr:
        def __init__(self, p):
            assert p == 1

    class Sequential:
        def __init__(self, children):
            assert len(children) == 1 and isinstance(children[0], Fliplr)

        def __call__(self, image, bounding_boxes):
            w = image.shape[1]
            out = [BoundingBox(w - b.x2, b.y1, w - b.x1, b.y2) for b in bounding_boxes.bounding_boxes]
            return image[:, ::-1], BoundingBoxesOnImage(out, image.shape)
    iaa.Fliplr, iaa.Sequential = Fliplr, Sequential
    bbs.BoundingBox, bbs.BoundingBoxesOnImage = BoundingBox, BoundingBoxesOnImage
    ia.augmenters, ia.augmentables = iaa, aug
    aug.bbs = bbs
    for n, m in (('imgaug', ia), ('imgaug.augmenters', iaa), ('imgaug.augmentables', aug),
                 ('imgaug.augmentables.bbs', bbs)):
        sys.modules[n] = m
    import lib.tracker.usot_tracker as rt
    return rt


class _Info:
    arch = 'USOT'
    dataset = 'SYNTH'
    epoch_test = False
    version = 'v1'


def do_host():
    """a14-a16: grids, box->feature-coordinate maps, decode, memory selection."""
    rt = _import_ref_tracker()
    g = {}
    trk = rt.USOTTracker(_Info())
    idx_cases = {}
    for inst in (255, 271):
        p = rt.USOTConfig()
        p.instance_size = inst
        p.renew()
        p.sf_size = p.score_size
        trk.grids(p)
        tag = 'i%d' % inst
        g[tag + '/grid_x'], g[tag + '/grid_y'] = trk.grid_to_search_x, trk.grid_to_search_y
        g[tag + '/search_axis'] = trk.search_area_x_axis
        boxes = np.array([[30.2, 41.7, 96.1, 88.8], [-5, -9, 300, 280], [0, 0, 126, 126],
                          [100.5, 90.25, 160.75, 170.0]], np.float32)
        g[tag + '/boxes'] = boxes
        g[tag + '/pool_template'] = np.stack([trk.pool_label_template(p, b) for b in boxes])
        g[tag + '/pool_search'] = np.stack([trk.pool_label_search(p, b) for b in boxes])
        # decode with canned network outputs
        S = p.score_size
        window = np.outer(np.hanning(S), np.hanning(S))
        for case in range(4):
            r = np.random.default_rng(4000 + 10 * inst + case)
            cls = (2.5 * r.standard_normal((1, 1, S, S))).astype(np.float32)
            cmem = (2.5 * r.standard_normal((1, 1, S, S))).astype(np.float32)
            bbox = np.exp(r.uniform(2.0, 4.5, (1, 4, S, S))).astype(np.float32)
            xf = r.standard_normal((1, 4, 31, 31)).astype(np.float32)
            tpos = np.array([200.0 + 3 * case, 150.0 - 2 * case])
            tsz = np.array([60.0 + 7 * case, 45.0 + 3 * case])
            scale_z = 127.0 / np.sqrt((tsz[0] + 0.5 * tsz.sum()) * (tsz[1] + 0.5 * tsz.sum()))
            seen = {}

            class StubNet:
                def track(self, x, template_mem=None, score_mem=None):
                    return t(cls), t(bbox), t(cmem), t(xf)

                def extract_memory_feature(self, xf=None, search_bbox=None, ori_x=None):
                    seen['box'] = search_bbox.numpy().copy()
                    return torch.zeros(1, 4, 7, 7)
            pos, sz, score, _ = trk.update(StubNet(), None, tpos.copy(), tsz * scale_z, window,
                                           scale_z, p)
            c = '%s/decode%d' % (tag, case)
            g[c + '/cls'], g[c + '/cls_mem'], g[c + '/bbox'] = cls, cmem, bbox
            g[c + '/tpos'], g[c + '/tsz'], g[c + '/scale_z'] = tpos, tsz, np.array(scale_z)
            g[c + '/out_pos'], g[c + '/out_sz'] = np.asarray(pos), np.asarray(sz)
            g[c + '/out_score'], g[c + '/out_poolbox'] = np.array(score), seen['box']
    # memory selection: tag feature i with the value i, read the tags the net receives
    p = rt.USOTConfig()
    p.sf_size = p.score_size
    trk.grids(p)
    for n in (1, 2, 3, 5, 8, 20, 57, 200):
        r = np.random.default_rng(7000 + n)
        conf = [0.9] + list(r.uniform(0.1, 1.0, n - 1))
        feats = [torch.full((1, 2, 7, 7), float(i)) for i in range(n)]
        got = {}

        class TagNet:
            def track(self, x, template_mem=None, score_mem=None):
                got['tags'] = template_mem[:, 0, 0, 0].numpy().copy()
                got['score'] = score_mem.numpy().copy()
                S = p.score_size
                return (torch.zeros(1, 1, S, S), torch.full((1, 4, S, S), 20.0),
                        torch.zeros(1, 1, S, S), torch.zeros(1, 2, 31, 31))

            def extract_memory_feature(self, xf=None, search_bbox=None, ori_x=None):
                return torch.zeros(1, 2, 7, 7)
        S = p.score_size
        state = dict(p=p, net=TagNet(), avg_chans=np.zeros(3), window=np.outer(np.hanning(S), np.hanning(S)),
                     target_pos=np.array([320.0, 240.0]), target_sz=np.array([63.5, 63.5]),
                     init_features=[torch.full((1, 2, 7, 7), -1.0), torch.full((1, 2, 7, 7), -2.0)],
                     memory_features=list(feats), memory_confidences=list(conf), im_h=480, im_w=640)
        trk.track(state, np.zeros((480, 640, 3), np.uint8))
        idx_cases[str(n)] = {'conf': [float(c) for c in conf],
                             'tags': [float(v) for v in got['tags']],
                             'score': [float(v) for v in got['score'].reshape(-1)]}
    np.savez_compressed(os.path.join(GOLD, 'golden_host.npz'), **g)
    with open(os.path.join(GOLD, 'golden_memory_indices.json'), 'w') as f:
        json.dump(idx_cases, f)
    print('host goldens: %d arrays' % len(g))


def do_e2e():
    """Whole tracker (reference USOTTracker + reference USOT on CPU) over a synthetic video.
    Third-party pieces the container lacks are substituted and declared unpinned:
    cv2.resize -> usot_amd.hostutils.resize_bilinear_u8, imgaug Fliplr -> array flip,
    PrRoIPool (GPU-only in the reference) -> oracle/prroi_pool_ref.c."""
    from usot_amd import hostutils
    sys.path.insert(3, os.path.join(REPO, 'oracle'))
    import usot_oracle as orc
    rt = _import_ref_tracker(resize=lambda img, size: hostutils.resize_bilinear_u8(img, size[0], size[1]))

    def prroi(features, rois, ph, pw, scale):
        return orc.prroi_pool(features, rois, ph, pw, scale)
    ref_models.prroi_pool2d = prroi
    import lib.models.connect as rc
    rc.PrRoIPool2D.forward = lambda self, f, r: prroi(f, r, self.pooled_height, self.pooled_width,
                                                      self.spatial_scale)
    net, _ = build(calibrated=True)
    net.eval()
    out = {}
    # A trajectory is only a meaningful fixture if every frame's argmax is decided by a clear
    # margin: two fp32 implementations agree to ~1e-4 on the maps, so a frame whose two best
    # cells are closer than that can legitimately go either way.  Record the margin per frame
    # and search seeds until every frame of the video has top-1 minus top-2 > MARGIN.
    MARGIN = 4e-3
    margins = []
    orig_track = net.track

    def spy(x, template_mem=None, score_mem=None):
        res = orig_track(x, template_mem=template_mem, score_mem=score_mem)
        cls, bbox, cmem, xf = res
        p = spy.p
        S = p.score_size
        sig = lambda a: 1.0 / (1.0 + np.exp(-a.numpy().reshape(S, S).astype(np.float32)))
        score = p.ratio * sig(cls) + (1 - p.ratio) * sig(cmem)
        hy = orc.Hyper(p.instance_size)
        gx, gy, _, _ = orc.grids(hy)
        b = bbox.numpy()[0]
        x1, y1, x2, y2 = gx - b[0], gy - b[1], gx + b[2], gy + b[3]
        t = spy.tsz
        ch = lambda r: np.maximum(r, 1.0 / r)
        szf = lambda w, h: np.sqrt((w + (w + h) * 0.5) * (h + (w + h) * 0.5))
        pen = np.exp(-(ch((t[0] / t[1]) / ((x2 - x1) / (y2 - y1))) * ch(szf(x2 - x1, y2 - y1) / szf(t[0], t[1])) - 1) * p.penalty_k)
        win = np.outer(np.hanning(S), np.hanning(S))
        ps = np.sort((pen * score * (1 - p.window_influence) + win * p.window_influence).reshape(-1))
        margins.append(float(ps[-1] - ps[-2]))
        return res
    net.track = spy
    wanted = [(255, 6, (52.0, 38.0)), (271, 4, (16.0, 12.0))]
    vid, seed = 0, 10
    while vid < len(wanted) and seed < 80:
        seed += 1
        inst_want, nframes, sz = wanted[vid]
        trk = rt.USOTTracker(_Info())
        del margins[:]
        with torch.no_grad():
            im, (cx, cy) = synth.frame(seed, t=0)
            state = trk.init(im, np.array([cx, cy]), np.array(sz), net)
            spy.p = state['p']
            rows = [[cx, cy, sz[0], sz[1], 0.0]]
            for f in range(1, nframes):
                im, _ = synth.frame(seed, t=f)
                s_x_scale = state['p'].exemplar_size / np.sqrt(
                    (state['target_sz'][0] + 0.5 * sum(state['target_sz'])) * (state['target_sz'][1] + 0.5 * sum(state['target_sz'])))
                spy.tsz = np.asarray(state['target_sz']) * s_x_scale
                state = trk.track(state, im)
                rows.append([*state['target_pos'], *state['target_sz'], float(state['cls_score'])])
        ok = state['p'].instance_size == inst_want and min(margins) > MARGIN
        print('seed', seed, 'instance', state['p'].instance_size, 'min margin %.2e' % min(margins), 'OK' if ok else 'skip')
        if not ok:
            continue
        out['video%d/seed_frames_sz' % vid] = np.array([seed, nframes, *sz])
        out['video%d/track' % vid] = np.array(rows, np.float64)
        out['video%d/instance_size' % vid] = np.array(state['p'].instance_size)
        out['video%d/margins' % vid] = np.array(margins)
        print(np.array(rows))
        vid += 1
    assert vid == len(wanted), 'no seed with clear margins found'
    np.savez_compressed(os.path.join(GOLD, 'golden_e2e.npz'), **out)


def do_e2e_long():
    """BASELINE configs[3] asks for >= 500 frames per stream so that the online memory queue (usot_tracker.py:222-265:
    confidence-ranked sampling over a growing list) is exercised: the reference tracker + reference model on CPU over
    500-frame synthetic videos, one per instance size (255 and 271), with the same documented stand-ins as do_e2e.
    Two float32 implementations agree to ~1e-4 on the response maps, so a long trajectory is only comparable frame by
    frame while every DISCRETE decision of the tracker is taken with a clear margin.  Recorded per frame, besides the
    trajectory: `margins` (top-1 minus top-2 of the penalised score map: the argmax), `round_slack` (distance of
    pos - c and of s_x from the nearest rounding boundary, pixels: the crop window, track_utils.py:42-47,121-127) and
    `pick_slack` (smallest top-1 minus top-2 confidence inside a sampled memory slice, usot_tracker.py:241-252).
    Seeds are searched until the first frame with a small margin lies beyond frame MIN_CLEAN."""
    from usot_amd import hostutils
    sys.path.insert(3, os.path.join(REPO, 'oracle'))
    import usot_oracle as orc
    rt = _import_ref_tracker(resize=lambda img, size: hostutils.resize_bilinear_u8(img, size[0], size[1]))

    def prroi(features, rois, ph, pw, scale):
        return orc.prroi_pool(features, rois, ph, pw, scale)
    ref_models.prroi_pool2d = prroi
    import lib.models.connect as rc
    rc.PrRoIPool2D.forward = lambda self, f, r: prroi(f, r, self.pooled_height, self.pooled_width, self.spatial_scale)
    net, _ = build(calibrated=True)
    net.eval()
    NFRAMES, MIN_CLEAN = 500, 200
    # what counts as a clear decision (the GPU test reads these from the fixture).  Two float32 evaluations of the logits
    # differ by ~1e-4 absolute, i.e. ~3e-5 in the sigmoid-blended score and ~1e-3 px in the smoothed position.
    M_TOL, R_TOL, P_TOL = 1e-4, 5e-3, 1e-4
    margins = []
    orig_track = net.track

    def spy(x, template_mem=None, score_mem=None):
        res = orig_track(x, template_mem=template_mem, score_mem=score_mem)
        cls, bbox, cmem, xf = res
        p = spy.p
        S = p.score_size
        sig = lambda a: 1.0 / (1.0 + np.exp(-a.numpy().reshape(S, S).astype(np.float32)))
        score = p.ratio * sig(cls) + (1 - p.ratio) * sig(cmem)
        hy = orc.Hyper(p.instance_size)
        gx, gy, _, _ = orc.grids(hy)
        b = bbox.numpy()[0]
        x1, y1, x2, y2 = gx - b[0], gy - b[1], gx + b[2], gy + b[3]
        tz = spy.tsz
        ch = lambda r: np.maximum(r, 1.0 / r)
        szf = lambda w, h: np.sqrt((w + (w + h) * 0.5) * (h + (w + h) * 0.5))
        pen = np.exp(-(ch((tz[0] / tz[1]) / ((x2 - x1) / (y2 - y1))) * ch(szf(x2 - x1, y2 - y1) / szf(tz[0], tz[1])) - 1) * p.penalty_k)
        win = np.outer(np.hanning(S), np.hanning(S))
        ps = np.sort((pen * score * (1 - p.window_influence) + win * p.window_influence).reshape(-1))
        margins.append(float(ps[-1] - ps[-2]))
        return res
    net.track = spy

    def frac_slack(v):
        return abs((v - np.floor(v)) - 0.5)

    out = {}
    wanted = [(255, (52.0, 38.0)), (271, (16.0, 12.0))]
    vid, seed = 0, 10
    while vid < len(wanted) and seed < 60:
        seed += 1
        inst_want, sz = wanted[vid]
        trk = rt.USOTTracker(_Info())
        del margins[:]
        rslack, pslack = [], []
        with torch.no_grad():
            im, (cx, cy) = synth.frame(seed, t=0)
            state = trk.init(im, np.array([cx, cy]), np.array(sz), net)
            if state['p'].instance_size != inst_want:
                print('seed', seed, 'instance', state['p'].instance_size, 'skip')
                continue
            spy.p = p = state['p']
            rows = [[cx, cy, sz[0], sz[1], 0.0]]
            ok = True
            for f in range(1, NFRAMES):
                im, _ = synth.frame(seed, t=f)
                tsz, tpos = state['target_sz'], state['target_pos']
                s_z = np.sqrt((tsz[0] + 0.5 * sum(tsz)) * (tsz[1] + 0.5 * sum(tsz)))
                scale_z = p.exemplar_size / s_z
                s_x = s_z + 2 * ((p.instance_size - p.exemplar_size) / 2) / scale_z
                spy.tsz = np.asarray(tsz) * scale_z
                win = rt.python2round(s_x) if hasattr(rt, 'python2round') else round(s_x)
                c = (win + 1) / 2
                # frame 1 starts from the init box, identical bits in every implementation: no rounding can differ
                rslack.append(1.0 if f == 1 else min(frac_slack(s_x), frac_slack(tpos[0] - c), frac_slack(tpos[1] - c)))
                conf = state['memory_confidences']
                n, upd = len(conf), p.mem_queue_size - 3
                ps_ = 1.0
                if n > 1:
                    gap = (n - 1) / upd
                    for i in range(upd):
                        a, b_ = min(int(int(i * gap) * n), n - 1), min(int(int((i + 1) * gap) * n), n - 1)
                        if a < b_ and b_ - a > 1:
                            top = np.sort(np.array(conf[a:b_], np.float64))
                            ps_ = min(ps_, float(top[-1] - top[-2]))
                pslack.append(ps_)
                state = trk.track(state, im)
                rows.append([*state['target_pos'], *state['target_sz'], float(state['cls_score'])])
                if f < MIN_CLEAN and margins[-1] < M_TOL:
                    ok = False
                    break
        print('seed', seed, 'instance', inst_want, 'frames', len(rows), 'min margin %.2e' % min(margins),
              'min round slack %.2e' % min(rslack), 'min pick slack %.2e' % min(pslack), 'OK' if ok else 'skip')
        if not ok:
            continue
        m, r_, pk = np.array(margins), np.array(rslack), np.array(pslack)
        amb = np.nonzero((m < M_TOL) | (r_ < R_TOL) | (pk < P_TOL))[0]
        print('  first frames with an unclear decision (margin | rounding | pick):', (amb[:12] + 1).tolist())
        out['video%d/seed_frames_sz' % vid] = np.array([seed, NFRAMES, *sz])
        out['video%d/track' % vid] = np.array(rows, np.float64)
        out['video%d/instance_size' % vid] = np.array(inst_want)
        out['video%d/margins' % vid] = m
        out['video%d/round_slack' % vid] = r_
        out['video%d/pick_slack' % vid] = pk
        out['video%d/tolerances' % vid] = np.array([M_TOL, R_TOL, P_TOL])
        vid += 1
    assert vid == len(wanted), 'no seed with clear margins found'
    np.savez_compressed(os.path.join(GOLD, 'golden_e2e_long.npz'), **out)
    print('long e2e goldens: %.1f KB' % (os.path.getsize(os.path.join(GOLD, 'golden_e2e_long.npz')) / 1024))


def do_family():
    """Second weight family ('dc': non-zero-DC filters, ordinary last-BN gains; usot_amd/synth.py): BN
    statistics calibrated like the first, then ONE tracked frame (template by centre crop, N_q = 7) through
    the reference model twice — in its own float32 arithmetic and converted to float64.  The fixture holds
    both; the GPU test reports HIP-vs-float64 beside reference-float32-vs-float64."""
    do_calib('dc')
    g = {}
    for fam in ('zero_dc', 'dc'):
        net, sd = build(calibrated=True, family=fam)
        net.eval()
        net.pr_pool = False
        z, x, mem = t(synth.crop(40, 1, 127)), t(synth.crop(41, 1, 255)), t(synth.memory_kernels(47, 7))
        with torch.no_grad():
            net.template(z)
            o32 = net.track(x, template_mem=mem, score_mem=torch.full((1, 7), 0.9))
            net64 = net.double()
            net64.template(z.double())
            o64 = net64.track(x.double(), template_mem=mem.double(), score_mem=torch.full((1, 7), 0.9).double())
        for nm, a, b in zip(('cls', 'bbox', 'cls_mem'), o32, o64):
            g['%s/%s/f32' % (fam, nm)], g['%s/%s/f64' % (fam, nm)] = a.numpy(), b.numpy()
            d = np.abs(a.numpy().astype(np.float64) - b.numpy())
            s = np.maximum(np.abs(b.numpy()), np.abs(b.numpy()).mean())
            print('%-8s %-8s reference f32 vs f64: scaled max %.2e' % (fam, nm, float((d / s).max())))
    np.savez_compressed(os.path.join(GOLD, 'golden_family.npz'), **g)


def do_model64():
    """Float64 truth for every whole-model fixture: the backbone stages at the four (size, batch)
    cases and every track_* output of do_model(), for BOTH weight families, from the reference model in its own float32
    arithmetic and converted with net.double().  Stored at the sample points of sampling.sample_index (same names as
    golden_model.npz, so the zero_dc float32 entries coincide with it) as float64.  The GPU test gates
    HIP-vs-float64 <= 1.5 x reference-float32-vs-float64 on every entry (tests/test_gpu_model.py)."""
    from sampling import sample_index
    g = {}

    def put(fam, name, a32, a64):
        a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
        if a32.size > 8192:
            idx = sample_index(name, a32.size)
            a32, a64 = a32.reshape(-1)[idx], a64.reshape(-1)[idx]
        g['%s/%s/f32' % (fam, name)], g['%s/%s/f64' % (fam, name)] = a32, a64
        d = np.abs(a32 - a64) / np.maximum(np.abs(a64), np.abs(a64).mean())
        print('%-8s %-28s reference f32 vs f64: scaled max %.2e' % (fam, name, float(d.max())))

    def run(net, cast):
        out = {}
        for size, b, seed in ((127, 1, 0), (255, 1, 1), (271, 1, 3), (255, 2, 4)):
            stages, p3 = net.feature_extractor(cast(t(synth.crop(seed, b, size))))
            tag = 'backbone_%d_b%d' % (size, b)
            for nm, ten in zip(('stem', 'p1', 'p2'), stages):
                out['%s/%s' % (tag, nm)] = ten.numpy()
            out[tag + '/p3'] = p3.numpy()
            out[tag + '/neck'] = net.neck(p3).numpy()
        net.template(cast(t(synth.crop(0, 1, 127))))
        out['template_crop/zf'] = net.zf.numpy().copy()
        x, mem = cast(t(synth.crop(1, 1, 255))), cast(t(synth.memory_kernels(7, 7)))
        cls, bbox, _, _ = net.track(x)
        out['track_offline/cls'], out['track_offline/bbox'] = cls.numpy(), bbox.numpy()
        sm = cast(torch.full((1, 7), 0.9))
        for tag, xx in (('track_mem', x), ('track_mem_271', cast(t(synth.crop(3, 1, 271))))):
            res = net.track(xx, template_mem=mem, score_mem=sm)
            for nm, ten in zip(('cls', 'bbox', 'cls_mem', 'xf'), res):
                out['%s/%s' % (tag, nm)] = ten.numpy()
        net.template(cast(t(synth.crop(5, 2, 127))))
        res = net.track(cast(t(synth.crop(4, 2, 255))), template_mem=cast(t(synth.memory_kernels(8, 14))),
                        score_mem=cast(torch.full((2, 7), 0.9)))
        for nm, ten in zip(('cls', 'bbox', 'cls_mem'), res):
            out['track_mem_b2/' + nm] = ten.numpy()
        return out
    path = os.path.join(GOLD, 'golden_model_f64.npz')
    if golden_parts.parts(path) and os.environ.get('USOT_GOLDEN_REGEN') != '1':
        # families already in the fixture are kept as committed (only missing ones are computed): adding the third family
        # in round 4 must not touch the entries rounds 2-3 were gated on
        g.update(golden_parts.load(path))
    for fam in synth.FAMILIES:
        if any(k.startswith(fam + '/') for k in g):
            print('%s: kept (%d arrays)' % (fam, sum(k.startswith(fam + '/') for k in g)))
            continue
        if not os.path.exists(synth.calib_file(fam)):
            do_calib(fam)
        net, _ = build(calibrated=True, family=fam)
        net.eval()
        net.pr_pool = False
        with torch.no_grad():
            o32 = run(net, lambda a: a)
            o64 = run(net.double(), lambda a: a.double())
        for k in o32:
            put(fam, k, o32[k], o64[k])
    files = golden_parts.save(path, g)
    print('float64 goldens: %d arrays, %.1f KB in %d parts' % (len(g), sum(os.path.getsize(f) for f in files) / 1024, len(files)))


def do_datasets():
    """f3: the REFERENCE's load_dataset (lib/dataset_loader/benchmark.py:8-230, pure Python) run on a
    fake datasets_test/ tree; its results, with paths made relative, are the fixture the CPU test
    compares usot_amd.benchmarks.load_dataset with.  The loader resolves its data root from its own
    __file__ (../../datasets_test), so the module object's __file__ is pointed at a temporary tree —
    nothing is written under /root/reference."""
    import importlib.util
    import tempfile
    import fake_datasets
    spec = importlib.util.spec_from_file_location('ref_benchmark', os.path.join(REF, 'lib', 'dataset_loader', 'benchmark.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = os.path.realpath(tmp)
        fake_datasets.build(tmp)
        os.makedirs(os.path.join(tmp, 'lib', 'dataset_loader'))       # '..' components are resolved by the OS
        mod.__file__ = os.path.join(tmp, 'lib', 'dataset_loader', 'benchmark.py')
        for name in fake_datasets.DATASETS:
            out[name] = fake_datasets.normalise(mod.load_dataset(name), tmp)
        try:
            mod.load_dataset('NOSUCH')
        except ValueError as e:
            out['__unsupported__'] = str(e)
    with open(os.path.join(GOLD, 'golden_datasets.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('datasets:', {k: len(v['order']) for k, v in out.items() if isinstance(v, dict)})


if __name__ == '__main__':
    what = sys.argv[1:] or ['calib', 'model', 'host']
    for w in what:
        {'calib': do_calib, 'model': do_model, 'host': do_host, 'e2e': do_e2e, 'datasets': do_datasets, 'family': do_family,
         'model64': do_model64, 'e2e_long': do_e2e_long}[w]()
