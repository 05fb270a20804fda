"""Microseconds per call of the BatchNorm2d kernels (csrc/batchnorm.hip) on the maps the reference trains the head on, beside
PyTorch-ROCm's own operator (aten native_batch_norm / native_batch_norm_backward -> MIOpen or ATen's kernels) on the same
channels-last tensors in the same process, and the algorithmic bytes over the time.  Prints ONE JSON line.

Cases: C = 256 at 25x25 (tower), 29x29 (search-side encoder) and 5x5 (template-side encoder) maps, batch 1, 8 and 32, and the
neck's 31x31 map.  Algorithmic traffic in units of one map (4*M*C bytes): forward training 2 reads + 1 write (statistics pass,
normalise pass); forward eval 1 + 1; backward training 4 reads + 1 write (x and dy in the sums pass and again in the dx pass: the
ReLU mask is recomputed from x, y is never read).  Every configuration runs on preallocated buffers through the raw entry
points (no allocation inside the timed window), is warmed up, and is timed twice for >= --seconds between device events, the
configurations of a case in alternating order (the second pass reversed), so the two numbers show the spread.

    timeout -k 10 900 python scripts/batchnorm_probe.py > profiles/batchnorm_probe_gfx950.json
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
EPS, MOMENTUM = 1e-5, 0.1
CASES = [('%s_b%d' % (name, n), (n, hw, hw, 256)) for name, hw in (('tower25', 25), ('search29', 29), ('template5', 5))
         for n in (1, 8, 32)] + [('neck31_b1', (1, 31, 31, 256))]
MAPS = {'fwd_train': 3, 'fwd_eval': 2, 'bwd_train': 5}            # map-sized transfers per call


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
    n, h, w, ch = c
    m = n * h * w
    g = torch.Generator().manual_seed(h * 7 + n)
    L = hip.lib()
    x = (torch.randn(n, h, w, ch, generator=g) + 0.5).to(DEV)
    dy = torch.randn(n, h, w, ch, generator=g).to(DEV)
    gamma, beta = (0.5 + torch.rand(ch, generator=g)).to(DEV), (0.3 * torch.randn(ch, generator=g)).to(DEV)
    rm, rv = torch.zeros(ch, device=DEV), torch.ones(ch, device=DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, invstd, dg, db = (torch.empty(ch, device=DEV) for _ in range(4))
    d0 = hip.bn_desc(M=m, C=ch, eps=EPS, momentum=MOMENTUM)
    ws = torch.empty(int(L.usot_batchnorm_ws_floats(C.byref(d0))), device=DEV)
    keep = [x, dy, gamma, beta, rm, rv, y, dx, mean, invstd, dg, db, ws]
    st = hip.stream()

    def desc(training, relu):
        return hip.bn_desc(M=m, C=ch, eps=EPS, momentum=MOMENTUM, training=training, act=hip.ACT_RELU if relu else hip.ACT_NONE,
                           x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), running_mean=rm.data_ptr(),
                           running_var=rv.data_ptr(), y=y.data_ptr(), save_mean=mean.data_ptr(), save_invstd=invstd.data_ptr(),
                           dy=dy.data_ptr(), dx=dx.data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), ws=ws.data_ptr())
    ds = {(t, r): desc(t, r) for t in (True, False) for r in (False, True)}
    hip.check(L.usot_batchnorm_fwd_f32(st, C.byref(ds[True, False])))          # save_mean / save_invstd for the backward calls
    out = [('fwd_train', lambda: hip.check(L.usot_batchnorm_fwd_f32(st, C.byref(ds[True, False])))),
           ('fwd_train_relu', lambda: hip.check(L.usot_batchnorm_fwd_f32(st, C.byref(ds[True, True])))),
           ('bwd_train', lambda: hip.check(L.usot_batchnorm_bwd_f32(st, C.byref(ds[True, False])))),
           ('bwd_train_relu', lambda: hip.check(L.usot_batchnorm_bwd_f32(st, C.byref(ds[True, True])))),
           ('fwd_eval', lambda: hip.check(L.usot_batchnorm_fwd_f32(st, C.byref(ds[False, False]))))]
    if with_torch:
        xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)        # NCHW-shaped views of the same channels-last memory
        assert xt.is_contiguous(memory_format=torch.channels_last) or n == 1
        trm, trv = rm.clone(), rv.clone()
        keep += [trm, trv]
        aten = torch.ops.aten
        _, tmean, tinv = aten.native_batch_norm(xt, gamma, beta, trm, trv, True, MOMENTUM, EPS)
        keep += [tmean, tinv]
        out.append(('torch_fwd_train', lambda: aten.native_batch_norm(xt, gamma, beta, trm, trv, True, MOMENTUM, EPS)))
        out.append(('torch_bwd_train', lambda: aten.native_batch_norm_backward(dyt, xt, gamma, trm, trv, tmean, tinv, True, EPS,
                                                                                [True, True, True])))
        out.append(('torch_fwd_eval', lambda: aten.native_batch_norm(xt, gamma, beta, trm, trv, False, MOMENTUM, EPS)))
    extra = dict(M=m, C=ch, slices=int(L.usot_batchnorm_slices(C.byref(d0))), map_bytes=4 * m * ch)
    return out, extra, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.3)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    rows = []
    for name, c in CASES:
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
    r, cb = hip.batchnorm_geometry()
    print(json.dumps(dict(probe='batchnorm', unit='us per call (two timed passes each)', device=torch.cuda.get_device_name(0),
                          seconds_per_point=a.seconds, geometry=dict(rows_per_step=r, channels_per_workgroup=cb),
                          maps_moved_per_call=MAPS, torch=torch.__version__, rows=rows)))


if __name__ == '__main__':
    main()
