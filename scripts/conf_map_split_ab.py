#!/usr/bin/env python3
"""Same-process A/B of Conf_Fusion's per-map split-K layouts under 'mem_dedupe' (scripts/tail_split_ab.py pattern): three sessions
per candidate, every session in the steady state of the tracker (D = 4 distinct memory rows), alternating timed replays of the
frame graph.  A candidate = engine option overrides + an optional tile for the conv's lead shape.
    python scripts/conf_map_split_ab.py [rounds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, bench
from usot_amd import engine
dev = torch.device('cuda:0')
base_tuning = engine.load_tuning()
CONF = (4375, 512, 2304, 1)                # the shape whose tuned tile leads Conf_Fusion's launch
one = (1,) * 7
cands = [('static (mem_dedupe off)', {'mem_dedupe': False}, None),
         ('unsplit', {'conf_map_split': one}, None),
         ('last distinct map ks 2', {'conf_map_split': (1, 1, 1, 2, 1, 1, 1)}, None),
         ('last distinct map ks 4', {'conf_map_split': (1, 1, 1, 4, 1, 1, 1)}, None),
         ('last two distinct maps ks 2', {'conf_map_split': (1, 1, 2, 2, 1, 1, 1)}, None),
         ('unsplit, 64 x 64 tile', {'conf_map_split': one}, {CONF: (57, 1)}),
         ('last distinct map ks 2, 64 x 64 tile', {'conf_map_split': (1, 1, 1, 2, 1, 1, 1)}, {CONF: (57, 1)})]
sessions = []
for name, opts, tile in cands * 3:          # sessions of one configuration differ by up to ~10 us with where their buffers land
    saved = dict(engine.OPTIONS)
    engine.OPTIONS.update(opts)
    tun = dict(base_tuning)
    if tile:
        tun.update(tile)
    model, _ = bench.build_model(0, 1, dev)
    model.engine_options['tuning'] = tun
    sess, crops, p = bench.open_stream(model, dev, seed=0)
    conf = bench.Confidences()
    bench.run_frames(sess, crops, p, conf, 30)
    d = int(sess.mem_map[0].item()) if sess.dedupe else 7
    sessions.append((name, d, sess))
    engine.OPTIONS.clear(); engine.OPTIONS.update(saved)
res = {}
for rnd in range(int(sys.argv[1]) if len(sys.argv) > 1 else 2):
    for name, d, sess in sessions:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(500): sess.plan.run()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / 500 * 1e6
        res.setdefault(name, []).append(us)
        print('%-40s maps %d  graph %.1f us' % (name, d, us), flush=True)
for name, v in res.items():
    print('%-40s min %.1f  median %.1f  max %.1f us over %d timings' % (name, min(v), sorted(v)[len(v) // 2], max(v), len(v)))
