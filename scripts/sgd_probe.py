"""Microseconds per optimiser step of the fused SGD step (csrc/sgd.hip, usot_amd.optim.SGD) beside PyTorch-ROCm's own
torch.optim.SGD (foreach=True and fused=True, where this build offers them) on the same tensors in the same process, and the
algorithmic bytes over the time.  Prints ONE JSON line.

The tensors are the 234 parameters of USOT() (29.4 M elements; 161 of them hold at most 1 024 elements) with random gradients,
momentum 0.9 and weight decay 1e-4 - the reference's scripts/train_usot.py.  Algorithmic traffic: 20 bytes per element (p, g and
buf read, p and buf written); the rows with zeroing write 4 more, and are reported at 20 all the same, so the rows compare.

Rows: `hip` = SGD.step(); `hip_guard_zero` = SGD(zero_grads=True).step(loss=loss), the guard read on the device and the gradients
zeroed in the same pass; `hip_raw` = the launch alone on the uploaded table (no Python table build); `torch_foreach`,
`torch_fused`; and `*_zero_grad` = the row's step followed by its own zero_grad(set_to_none=False).  Every step() includes its
host side: the calls run back to back between two device events, so a row is the larger of host time and device time per step.

Every configuration owns its tensors, is warmed up, and is timed twice for >= --seconds between device events, the
configurations in alternating order (the second pass reversed), so the two numbers show the spread.

    timeout -k 10 900 python scripts/sgd_probe.py > profiles/sgd_probe_gfx950.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from usot_amd import hip, optim  # noqa: E402
from usot_amd.model import USOT  # noqa: E402

DEV = 'cuda:0'
KW = dict(lr=0.005, momentum=0.9, weight_decay=1e-4)
BYTES_PER_ELEMENT = 20


def timed(fn, seconds):
    """us per call: warm-up, a calibration batch, then >= `seconds` of back-to-back calls between two device events"""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    per = max(e0.elapsed_time(e1) / 10 * 1e-3, 1e-6)
    n = max(20, int(seconds / per))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def tensors(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(DEV)
    return ps


def configs(shapes):
    cfg, keep = [], []
    loss = torch.tensor(0.5, device=DEV)

    def add(name, make, step_kw=None):
        for tail in ('', '_zero_grad'):
            ps = tensors(shapes, 1)
            try:
                opt = make(ps)
                opt.step(**(step_kw or {}))
            except (RuntimeError, ValueError, TypeError) as e:       # this build does not offer the implementation
                print('%s: not offered (%s)' % (name, str(e).splitlines()[0]), file=sys.stderr)
                return
            if tail:
                def fn(opt=opt):
                    opt.step(**(step_kw or {}))
                    opt.zero_grad(set_to_none=False)
            else:
                def fn(opt=opt):
                    opt.step(**(step_kw or {}))
            cfg.append((name + tail, fn))
            keep.append((ps, opt))
    add('hip', lambda ps: optim.SGD(ps, **KW))
    add('hip_guard_zero', lambda ps: optim.SGD(ps, zero_grads=True, **KW), dict(loss=loss))
    add('torch_foreach', lambda ps: torch.optim.SGD(ps, foreach=True, **KW))
    add('torch_fused', lambda ps: torch.optim.SGD(ps, fused=True, **KW))
    raw = keep[0][1]                                                   # the launch alone, on the table `hip` uploaded
    T, n_chunks = raw._shape
    cfg.append(('hip_raw', lambda: hip.sgd_step(raw._table, T, n_chunks, counters=raw._counters)))
    return cfg, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.3)
    a = ap.parse_args()
    shapes = [tuple(p.shape) for p in USOT().parameters()]
    elements = sum(torch.Size(s).numel() for s in shapes)
    cfg, keep = configs(shapes)
    got = {}
    for order in (cfg, cfg[::-1]):
        for name, fn in order:
            got.setdefault(name, []).append(round(timed(fn, a.seconds), 2))
            print('%s: %s' % (name, got[name]), file=sys.stderr, flush=True)
    traffic = elements * BYTES_PER_ELEMENT
    gbs = {k: round(traffic / (min(v) * 1e-6) * 1e-9, 1) for k, v in got.items()}
    ratio = {k: round(min(got[k]) / min(got['hip']), 2) for k in got if k.startswith('torch') and not k.endswith('_zero_grad')}
    ratio.update({k: round(min(got[k]) / min(got['hip_guard_zero']), 2) for k in got if k.startswith('torch') and k.endswith('_zero_grad')})
    print(json.dumps(dict(probe='sgd', unit='us per step (two timed passes each)', device=torch.cuda.get_device_name(0),
                          seconds_per_point=a.seconds, tensors=len(shapes), elements=elements, hyper=KW,
                          chunk_elems=hip.sgd_chunk_elems(), grid_cap=hip.sgd_grid_cap(), table_chunks=keep[0][1]._shape[1],
                          bytes_per_element=BYTES_PER_ELEMENT, algorithmic_bytes=traffic, us_per_step=got,
                          algorithmic_gb_per_s=gbs, torch_over_hip=ratio, torch=torch.__version__)))


if __name__ == '__main__':
    main()
