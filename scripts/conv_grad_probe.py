"""Microseconds per call of the fp32 convolution gradients (csrc/conv_grad.hip) on the model's geometries, beside the forward
launch of the same geometry on this library (same FLOP count: the natural yardstick) and PyTorch-ROCm's own gradients
(torch.nn.grad.conv2d_weight / conv2d_input -> MIOpen, channels-last) on the same box.  Prints ONE JSON line.

Cases: one tower conv (256 -> 256, 3x3, pad 1, 25x25) at batch 1, 8 and 32; the search-side encoder (31x31 -> 27x29, dil (2, 1));
the neck 1x1 (1024 -> 256, 31x31).  Every configuration runs on preallocated buffers (no allocation inside the timed window), is
warmed up, and is timed twice for >= --seconds between device events, the configurations of a case in alternating order (the
second pass reversed), so the two numbers show the spread.  `wgrad` is the launcher's own pixel split (`psplit` in the row),
`wgrad_psplitN` a forced one.  The rotated bank of route A is packed outside the window (a
parameter-sized pass per optimiser step, reported on its own line).

    timeout -k 10 900 python scripts/conv_grad_probe.py > profiles/conv_grad_probe_gfx950.json
"""
import argparse
import ctypes as C
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
SWEEP = (1, 2, 4, 8, 16)            # pixel splits of the weight gradient timed beside the launcher's own choice
# name, (N, H, W, Cin, Cout, k, stride, pad, dil)
CASES = [('tower_b1', (1, 25, 25, 256, 256, 3, 1, (1, 1), (1, 1))),
         ('tower_b8', (8, 25, 25, 256, 256, 3, 1, (1, 1), (1, 1))),
         ('tower_b32', (32, 25, 25, 256, 256, 3, 1, (1, 1), (1, 1))),
         ('encoder_search', (1, 31, 31, 256, 256, 3, 1, (0, 0), (2, 1))),
         ('neck_1x1', (1, 31, 31, 1024, 256, 1, 1, (0, 0), (1, 1)))]


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


def configs(c, with_torch):
    n, h, w, cin, cout, k, s, pad, dil = c
    g = torch.Generator().manual_seed(h * 7 + n)
    L = hip.lib()
    geo = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=k, KW=k, stride=s, pad=pad, dil=dil)
    d0 = hip.grad_desc(**geo)
    oh, ow = d0.OH, d0.OW
    K = k * k * cin
    x = torch.randn(n, h, w, cin, generator=g).to(DEV)
    wp = (torch.randn(cout, K, generator=g) / K ** 0.5).to(DEV)
    dy = torch.randn(n, oh, ow, cout, generator=g).to(DEV)
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(wp), torch.empty(cout, device=DEV)
    need = L.usot_conv2d_wgrad_ws_floats(C.byref(d0))
    sweep = [ps for ps in SWEEP if ps <= n * oh * ow]
    ws = torch.empty(max(int(need), max(sweep) * cout * (K + 1)), device=DEV)
    wt = hip.pack_dgrad(wp, cin, k, k)
    keep = [x, wp, dy, y, dx, dw, db, ws, wt]
    st = hip.stream()

    def gd(route, psplit=0):
        return hip.grad_desc(x=x.data_ptr(), w=wp.data_ptr(), wt=wt.data_ptr(), dy=dy.data_ptr(), dx=dx.data_ptr(),
                             dw=dw.data_ptr(), db=db.data_ptr(), ws=ws.data_ptr(), route=route, psplit=psplit, **geo)
    dg = {r: gd(r) for r in (0, 1, 2)}
    fwd = hip.conv_desc(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), N=n, H=h, W=w, Cin=cin, OH=oh, OW=ow, Cout=cout,
                        KH=k, KW=k, stride=s, pad=pad, dil=dil)
    out = [('forward', lambda: hip.check(L.usot_conv2d_f32(st, C.byref(fwd)))),
           ('wgrad', lambda: hip.check(L.usot_conv2d_wgrad_f32(st, C.byref(dg[0])))),
           ('dgrad_route_b', lambda: hip.check(L.usot_conv2d_dgrad_f32(st, C.byref(dg[2])))),
           ('pack_dgrad', lambda: hip.check(L.usot_conv_pack_dgrad_f32(st, hip.ptr(wp), hip.ptr(wt), cout, cin, k, k)))]
    for ps in sweep:                                                  # the launcher's choice among fixed splits
        out.append(('wgrad_psplit%d' % ps, lambda d=gd(0, ps): hip.check(L.usot_conv2d_wgrad_f32(st, C.byref(d)))))
    if L.usot_conv2d_dgrad_route(C.byref(dg[0])) == 1:
        out.insert(2, ('dgrad_route_a', lambda: hip.check(L.usot_conv2d_dgrad_f32(st, C.byref(dg[1])))))
    if with_torch:
        cl = torch.channels_last
        xt = x.permute(0, 3, 1, 2)                                    # NCHW-shaped views of the same channels-last memory
        dyt = dy.permute(0, 3, 1, 2)
        wo = wp.view(cout, k, k, cin).permute(0, 3, 1, 2)
        assert xt.is_contiguous(memory_format=cl) and wo.is_contiguous(memory_format=cl)
        out.append(('torch_conv2d_weight', lambda: torch.nn.grad.conv2d_weight(xt, wo.shape, dyt, stride=s, padding=pad, dilation=dil)))
        out.append(('torch_conv2d_input', lambda: torch.nn.grad.conv2d_input(xt.shape, wo, dyt, stride=s, padding=pad, dilation=dil)))
    extra = dict(M=n * oh * ow, K=K, Cout=cout, psplit=int(L.usot_conv2d_wgrad_psplit(C.byref(d0))),
                 gflop=round(2.0 * n * oh * ow * K * cout * 1e-9, 4))
    return out, extra, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.4)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    rows = []
    for name, c in CASES:
        cfg, extra, keep = configs(c, not a.no_torch)
        got = {}
        for order in (cfg, cfg[::-1]):
            for cname, fn in order:
                got.setdefault(cname, []).append(round(timed(fn, a.seconds), 2))
        rows.append(dict(case=name, geometry=list(c[:7]) + [list(c[7]), list(c[8])], us_per_call=got, **extra))
        print('%s: %s' % (name, got), file=sys.stderr, flush=True)
        del cfg, keep
        torch.cuda.empty_cache()
    bco, bk, chunk = hip.wgrad_geometry()
    print(json.dumps(dict(probe='conv_grad', unit='us per call (two timed passes each)', device=torch.cuda.get_device_name(0),
                          host=socket.gethostname(), seconds_per_point=a.seconds, wgrad_tile=dict(bco=bco, bk=bk, chunk=chunk),
                          torch=torch.__version__, rows=rows)))


if __name__ == '__main__':
    main()
