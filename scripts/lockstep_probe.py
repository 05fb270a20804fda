"""Aggregate frames/s of lock-step multi-video tracking (engine.BatchSession) against the same number of Sessions on separate
HIP streams (bench.run_frames_multi's pattern), in one process.  Prints ONE JSON line.

Points: slots in --slots (default 1 4 8 16 32) x {exact fp32 BatchSession, fp16-backbone BatchSession} x {resident crops,
uint8 frames cropped on the device}, and N streamed Sessions with resident crops.  Every point is timed for >= --seconds,
twice, the configurations of one slot count in alternating order (the second pass reversed), so the two numbers show the
spread.  Synthetic weights, crops and frames (usot_amd.synth); memory picks from each video's own confidences.

    timeout -k 10 900 python scripts/lockstep_probe.py > profiles/lockstep_probe_gfx950.json
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from usot_amd import synth  # noqa: E402
from usot_amd.model import USOT  # noqa: E402
from usot_amd.tracker import USOTConfig, select_memory  # noqa: E402

DEV = 'cuda:0'


def _setup(e, p, window):
    z = torch.from_numpy(synth.crop(1, 1, 127)).to(DEV)
    zf = e.template(z, pr_pool=False)
    feats = [torch.from_numpy(synth.memory_kernels(2 + i, 1)).to(DEV) for i in range(2)]
    return zf, feats


def _timed(step, seconds):
    step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n, dt


def lockstep_point(e, p, window, zf, feats, B, dtype, frames, seconds):
    bs = e.open_batch_session(p, window, B, capacity=256, backbone_dtype=dtype)
    for s in range(B):
        bs.load(s, zf, feats)
    crops = torch.from_numpy(synth.crop(7, B, p.instance_size)).to(DEV)
    bs.x.copy_(crops)
    confs = [[0.9] for _ in range(B)]
    ims = [synth.frame(100 + s, t=1)[0] for s in range(B)]

    def step():
        if bs.book.need_grow():                 # keep the banks small: a probe, not a video
            bs.flush()
            for s in range(B):
                bs.book.n[s] = 1
                confs[s] = [0.9]
        items = {}
        for s in range(B):
            it = dict(picks=select_memory(np.asarray(confs[s]), p.mem_queue_size), tsz=(63.5, 63.5))
            if frames:          # a 40 x 40 target at the frame's centre: s_x = 160.6, python2round -> 161
                it.update(image=ims[s], pos=(240.0, 180.0), win=161, avg_chans=(100.0, 110.0, 120.0))
            items[s] = it
        out = bs.step(items)
        for s in range(B):
            confs[s].append(float(out[s][1]))
    n, dt = _timed(step, seconds)
    return B * n / dt, dt / n * 1e3


def streams_point(e, p, window, zf, feats, N, seconds):
    e.set_template(zf)
    sess = [e.open_session(p, window, feats) for _ in range(N)]
    streams = [torch.cuda.Stream() for _ in range(N)]
    crops = torch.from_numpy(synth.crop(7, N, p.instance_size)).to(DEV)
    confs = [[0.9] for _ in range(N)]

    def step():
        for i in range(N):
            if 2 + sess[i].n >= sess[i].cap - 8:     # keep the bank from growing mid-timing
                sess[i].n, confs[i] = 1, [0.9]
            with torch.cuda.stream(streams[i]):
                sess[i].submit(crops[i], select_memory(np.asarray(confs[i]), p.mem_queue_size), (63.5, 63.5), inplace=True)
        for i in range(N):
            confs[i].append(float(sess[i].collect()[1]))
    n, dt = _timed(step, seconds)
    return N * n / dt, dt / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, nargs='+', default=[1, 4, 8, 16, 32])
    ap.add_argument('--seconds', type=float, default=2.0)
    a = ap.parse_args()
    m = USOT()
    m.load_state_dict(synth.torch_state_dict(m, seed=0, calibrated=True), strict=True)
    m = m.eval().to(DEV)
    e = m.engine
    p = USOTConfig()
    p.sf_size = p.score_size
    window = np.outer(np.hanning(p.score_size), np.hanning(p.score_size))
    zf, feats = _setup(e, p, window)
    rows = []
    for B in a.slots:
        confs = [('lockstep_f32_resident', lambda: lockstep_point(e, p, window, zf, feats, B, torch.float32, False, a.seconds)),
                 ('lockstep_f32_uint8', lambda: lockstep_point(e, p, window, zf, feats, B, torch.float32, True, a.seconds)),
                 ('lockstep_fp16bb_resident', lambda: lockstep_point(e, p, window, zf, feats, B, torch.float16, False, a.seconds)),
                 ('lockstep_fp16bb_uint8', lambda: lockstep_point(e, p, window, zf, feats, B, torch.float16, True, a.seconds)),
                 ('streams_f32_resident', lambda: streams_point(e, p, window, zf, feats, B, a.seconds))]
        got = {}
        for rep, order in enumerate((confs, confs[::-1])):
            for name, fn in order:
                fps, ms = fn()
                got.setdefault(name, []).append((round(fps, 1), round(ms, 3)))
                torch.cuda.empty_cache()
        for name, v in got.items():
            rows.append(dict(slots=B, config=name, frames_per_s=[x[0] for x in v], ms_per_step=[x[1] for x in v]))
        print('slots %d: %s' % (B, {k: [x[0] for x in v] for k, v in got.items()}), file=sys.stderr, flush=True)
    print(json.dumps(dict(probe='lockstep', unit='aggregate frames/s (two timed passes each)', device=torch.cuda.get_device_name(0),
                          host=socket.gethostname(), seconds_per_point=a.seconds, instance_size=p.instance_size, rows=rows)))


if __name__ == '__main__':
    main()
