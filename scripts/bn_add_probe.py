"""Microseconds per call of BatchNorm - add - ReLU (csrc/batchnorm.hip, usot_bn_add_desc) on the bottleneck outputs of a training
step, in training mode, forward and backward, three ways on the same channels-last buffers in the same process:
  fused     usot_batchnorm_add_fwd_f32 / usot_batchnorm_add_bwd_f32;
  composed  what the library needed before them for the same result: usot_batchnorm_fwd_f32 without ReLU, then torch add_ and
            relu_; torch threshold_backward (into a preallocated buffer), then usot_batchnorm_bwd_f32 (dres is that buffer);
  torch     PyTorch-ROCm's native_batch_norm + add + relu, and threshold_backward + native_batch_norm_backward.
Prints ONE JSON line.

Cases: 256 channels at 63x63 and 31x31, 512 at 31x31 and 15x15, 1024 at 31x31 and 15x15, batch 1, 8 and 32; a configuration whose
preallocated buffers exceed 1 GiB is dropped.  Algorithmic traffic in units of one map (4*M*C bytes): fused forward 3 reads + 1
write; composed forward 5 reads + 3 writes; backward 6 reads + 2 writes either way (the composed one in twice the launches).
Timing as in scripts/batchnorm_probe.py: preallocated buffers, raw entry points, warm-up, then two timed passes of >= --seconds
between device events, the legs of a case in alternating order (the second pass reversed), so the two numbers show the spread.

    timeout -k 10 900 python scripts/bn_add_probe.py > profiles/bn_add_probe_gfx950.json
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
from batchnorm_probe import timed  # noqa: E402

DEV = 'cuda:0'
EPS, MOMENTUM = 1e-5, 0.1
CASES = [('c%d_%dx%d_b%d' % (ch, hw, hw, n), (n, hw, hw, ch)) for ch, hw in ((256, 63), (256, 31), (512, 31), (512, 15), (1024, 31), (1024, 15))
         for n in (1, 8, 32)]
MAPS = {'fused_fwd': 4, 'composed_fwd': 8, 'fused_bwd': 8, 'composed_bwd': 8}      # map-sized transfers per call
N_MAPS = 8                                                                         # x, res, dy, y, dx, dres, y of leg b, dy' of leg b
LIMIT = 1 << 30


def configs(c, with_torch):
    n, h, w, ch = c
    m = n * h * w
    g = torch.Generator().manual_seed(h * 7 + n + ch)
    L = hip.lib()
    x = (torch.randn(n, h, w, ch, generator=g) + 0.5).to(DEV)
    res = torch.randn(n, h, w, ch, generator=g).abs().to(DEV)
    dy = torch.randn(n, h, w, ch, generator=g).to(DEV)
    gamma, beta = (0.5 + torch.rand(ch, generator=g)).to(DEV), (0.3 * torch.randn(ch, generator=g)).to(DEV)
    rm, rv = torch.zeros(ch, device=DEV), torch.ones(ch, device=DEV)
    y, dx, dres, y2, dyp = (torch.empty_like(x) for _ in range(5))
    mean, invstd, dg, db = (torch.empty(ch, device=DEV) for _ in range(4))
    d0 = hip.bn_desc(M=m, C=ch, eps=EPS, momentum=MOMENTUM)
    ws = torch.empty(int(L.usot_batchnorm_ws_floats(C.byref(d0))), device=DEV)
    keep = [x, res, dy, gamma, beta, rm, rv, y, dx, dres, y2, dyp, mean, invstd, dg, db, ws]
    st = hip.stream()
    common = dict(M=m, C=ch, eps=EPS, momentum=MOMENTUM, training=True, x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                  running_mean=rm.data_ptr(), running_var=rv.data_ptr(), save_mean=mean.data_ptr(), save_invstd=invstd.data_ptr(),
                  dx=dx.data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), ws=ws.data_ptr())
    fused = hip.bn_add_desc(act=hip.ACT_RELU, y=y.data_ptr(), dy=dy.data_ptr(), res=res.data_ptr(), dres=dres.data_ptr(), **common)
    plain = hip.bn_desc(act=hip.ACT_NONE, y=y2.data_ptr(), dy=dyp.data_ptr(), **common)
    thr = torch.ops.aten.threshold_backward.grad_input

    def composed_fwd():
        hip.check(L.usot_batchnorm_fwd_f32(st, C.byref(plain)))
        y2.add_(res).relu_()

    def composed_bwd():
        thr(dy, y2, 0, grad_input=dyp)
        hip.check(L.usot_batchnorm_bwd_f32(st, C.byref(plain)))
    hip.check(L.usot_batchnorm_add_fwd_f32(st, C.byref(fused)))        # save_mean / save_invstd and y for the backward legs
    composed_fwd()
    out = [('fused_fwd', lambda: hip.check(L.usot_batchnorm_add_fwd_f32(st, C.byref(fused)))),
           ('composed_fwd', composed_fwd),
           ('fused_bwd', lambda: hip.check(L.usot_batchnorm_add_bwd_f32(st, C.byref(fused)))),
           ('composed_bwd', composed_bwd)]
    if with_torch:
        xt, rt, dyt = (t.permute(0, 3, 1, 2) for t in (x, res, dy))    # NCHW-shaped views of the same channels-last memory
        trm, trv = rm.clone(), rv.clone()
        aten = torch.ops.aten
        _, tmean, tinv = aten.native_batch_norm(xt, gamma, beta, trm, trv, True, MOMENTUM, EPS)
        yt = y.permute(0, 3, 1, 2)
        keep += [trm, trv, tmean, tinv]

        def torch_fwd():
            return aten.native_batch_norm(xt, gamma, beta, trm, trv, True, MOMENTUM, EPS)[0].add_(rt).relu_()

        def torch_bwd():
            return aten.native_batch_norm_backward(aten.threshold_backward(dyt, yt, 0), xt, gamma, trm, trv, tmean, tinv, True, EPS,
                                                   [True, True, True])
        out += [('torch_fwd', torch_fwd), ('torch_bwd', torch_bwd)]
    extra = dict(M=m, C=ch, slices=int(L.usot_batchnorm_slices(C.byref(d0))), map_bytes=4 * m * ch)
    return out, extra, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.15)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    rows, dropped = [], []
    for name, c in CASES:
        if N_MAPS * 4 * c[0] * c[1] * c[2] * c[3] > LIMIT:
            dropped.append(name)
            continue
        cfg, extra, keep = configs(c, not a.no_torch)
        got = {}
        for order in (cfg, cfg[::-1]):
            for cname, fn in order:
                got.setdefault(cname, []).append(round(timed(fn, a.seconds), 2))
        gbs = {k: round(MAPS[k] * extra['map_bytes'] / (min(got[k]) * 1e-6) * 1e-9, 1) for k in MAPS}
        rows.append(dict(case=name, shape=list(c), us_per_call=got, algorithmic_gb_per_s=gbs, **extra))
        print('%s: %s %s' % (name, got, gbs), file=sys.stderr, flush=True)
        del cfg, keep
        torch.cuda.empty_cache()
    print(json.dumps(dict(probe='bn_add', unit='us per call (two timed passes each)', device=torch.cuda.get_device_name(0),
                          seconds_per_point=a.seconds, mode='training, ReLU', maps_moved_per_call=MAPS, dropped_over_1GiB=dropped,
                          torch=torch.__version__, rows=rows)))


if __name__ == '__main__':
    main()
