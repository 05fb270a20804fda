"""Microseconds per call of the head's gradient operators (csrc/head_grad.hip) beside PyTorch-ROCm's composition of the same
operations on the same tensors in the same process, and the algorithmic bytes over the time.  Prints ONE JSON line.

Conf_Fusion at B = 16, M = 4, P = 625, C = 256: the reference's `maximum_batch` x `mem_size` at the 25 x 25 response.  Algorithmic
traffic: forward (2M + 1) * B*P*C*4 bytes (conf and value read, out written), backward (4M + 1) * B*P*C*4 bytes (conf, value and
dout read, dconf and dvalue written; the weights and `out` are recomputed).  The box epilogue at R = 16 * 625 rows of four
channels: forward 2 * R*16 bytes, backward 3 * R*16 bytes (p and dy read, dp written) - 160 KB maps, i.e. launch latency.  The
PyTorch side is clamp - exp - sum - div - mul - sum (connect.py:129-142) and exp(adjust * p + bias) on the same device tensors,
forward under no_grad, backward as torch.autograd.grad on a graph built once (retain_graph): what eager training would run.

Every configuration runs on preallocated buffers through the raw entry points (no allocation inside the timed window), is warmed
up, and is timed twice for >= --seconds between device events, the configurations in alternating order (the second pass
reversed), so the two numbers show the spread.

    timeout -k 10 900 python scripts/head_grad_probe.py > profiles/head_grad_probe_gfx950.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
B, M, P, CH = 16, 4, 625, 256
ROWS = 16 * 625


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


def conf_fusion_configs():
    g = torch.Generator().manual_seed(1)
    conf = torch.relu(1.5 * torch.randn(B * M, 25, 25, CH, generator=g)).to(DEV)
    value = torch.relu(torch.randn(B * M, 25, 25, CH, generator=g)).to(DEV)
    dout = torch.randn(B, 25, 25, CH, generator=g).to(DEV)
    out, dconf, dvalue = torch.empty_like(dout), torch.empty_like(conf), torch.empty_like(conf)
    L, st = hip.lib(), hip.stream()
    d = hip.conf_fusion_desc(B=B, M=M, P=P, C=CH, conf=conf.data_ptr(), value=value.data_ptr(), out=out.data_ptr(),
                             dout=dout.data_ptr(), dconf=dconf.data_ptr(), dvalue=dvalue.data_ptr())

    def compose(c, v):
        e = torch.exp(torch.clamp(c, max=4, min=-6)).view(B, M, 25, 25, CH)
        return ((e / e.sum(dim=1, keepdim=True)) * v.view(B, M, 25, 25, CH)).sum(dim=1)

    def torch_fwd():
        with torch.no_grad():
            return compose(conf, value)
    cg, vg = conf.clone().requires_grad_(True), value.clone().requires_grad_(True)
    graph = compose(cg, vg)
    cfg = [('fwd', lambda: hip.check(L.usot_conf_fusion_fwd_f32(st, C.byref(d)))),
           ('bwd', lambda: hip.check(L.usot_conf_fusion_bwd_f32(st, C.byref(d)))),
           ('torch_fwd', torch_fwd),
           ('torch_bwd', lambda: torch.autograd.grad(graph, (cg, vg), dout, retain_graph=True))]
    unit = B * P * CH * 4
    return cfg, {'fwd': (2 * M + 1) * unit, 'bwd': (4 * M + 1) * unit}, [conf, value, dout, out, dconf, dvalue, cg, vg, graph]


def box_exp_configs():
    g = torch.Generator().manual_seed(2)
    p = (5.0 * torch.randn(ROWS, 4, generator=g)).to(DEV)
    dy = torch.randn(ROWS, 4, generator=g).to(DEV)
    adjust, bias = torch.full((1,), 0.1, device=DEV), torch.full((1, 4, 1, 1), 3.4, device=DEV)
    y, dp, da, db = torch.empty_like(p), torch.empty_like(p), torch.empty_like(adjust), torch.empty_like(bias)
    ws = torch.empty(hip.box_exp_ws_floats(ROWS), device=DEV)
    L, st = hip.lib(), hip.stream()
    d = hip.box_exp_desc(R=ROWS, p=p.data_ptr(), adjust=adjust.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr(), dy=dy.data_ptr(),
                         dp=dp.data_ptr(), dadjust=da.data_ptr(), dbias=db.data_ptr(), ws=ws.data_ptr())
    pn, dn = p.view(16, 25, 25, 4).permute(0, 3, 1, 2), dy.view(16, 25, 25, 4).permute(0, 3, 1, 2)      # as the head holds them

    def torch_fwd():
        with torch.no_grad():
            return torch.exp(adjust * pn + bias)
    leaves = [t.clone().requires_grad_(True) for t in (pn, adjust, bias)]
    graph = torch.exp(leaves[1] * leaves[0] + leaves[2])
    cfg = [('fwd', lambda: hip.check(L.usot_box_exp_fwd_f32(st, C.byref(d)))),
           ('bwd', lambda: hip.check(L.usot_box_exp_bwd_f32(st, C.byref(d)))),
           ('torch_fwd', torch_fwd),
           ('torch_bwd', lambda: torch.autograd.grad(graph, leaves, dn, retain_graph=True))]
    return cfg, {'fwd': 2 * ROWS * 16, 'bwd': 3 * ROWS * 16}, [p, dy, adjust, bias, y, dp, da, db, ws, graph] + leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.3)
    a = ap.parse_args()
    rows = []
    for name, shape, make in (('conf_fusion', dict(B=B, M=M, P=P, C=CH), conf_fusion_configs), ('box_exp', dict(R=ROWS, C=4), box_exp_configs)):
        cfg, traffic, keep = make()
        got = {}
        for order in (cfg, cfg[::-1]):
            for cname, fn in order:
                got.setdefault(cname, []).append(round(timed(fn, a.seconds), 2))
        gbs = {k: round(traffic[k] / (min(got[k]) * 1e-6) * 1e-9, 1) for k in traffic}
        ratio = {k: round(min(got['torch_' + k]) / min(got[k]), 2) for k in traffic}
        rows.append(dict(case=name, shape=shape, us_per_call=got, algorithmic_bytes=traffic, algorithmic_gb_per_s=gbs,
                         torch_over_hip=ratio))
        print('%s: %s %s' % (name, got, gbs), file=sys.stderr, flush=True)
        del cfg, keep
        torch.cuda.empty_cache()
    print(json.dumps(dict(probe='head_grad', unit='us per call (two timed passes each)', device=torch.cuda.get_device_name(0),
                          seconds_per_point=a.seconds, box_exp_rows_per_partial=hip.box_exp_row_step(), torch=torch.__version__,
                          rows=rows)))


if __name__ == '__main__':
    main()
