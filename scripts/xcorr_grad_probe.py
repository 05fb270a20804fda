"""Forward + both gradients of the depthwise cross-correlation on the head's three shapes, (a) through
usot_amd.autograd.xcorr_depthwise (csrc/xcorr.hip + csrc/xcorr_grad.hip) and (b) through the reference's formulation on
PyTorch-ROCm (one grouped F.conv2d with a channel per group, under autograd on the device), in one process; and the two
gradient kernels (and the forward) alone, with their algorithmic bytes per call over time against the box's copy ceiling
(usot_bw_probe, as bench.py measures it).  Prints ONE JSON line.

Points: shapes 29x29 * 5x5, 27x29 * 3x5, 29x27 * 5x3 at P = 3 072 (12 x 256) and P = 21 504 (12 x 7 x 256) planes.  Every
point is timed for >= --seconds after a warm-up, twice, the contenders of one point alternating (the second pass reversed),
so the two numbers show the spread.  A call = forward, then torch.autograd.grad for both inputs.

    timeout -k 10 900 python scripts/xcorr_grad_probe.py > profiles/xcorr_grad_probe_gfx950.json
"""
import argparse
import json
import os
import socket
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from usot_amd import autograd, hip  # noqa: E402

DEV = 'cuda:0'
SHAPES = ((29, 29, 5, 5), (27, 29, 3, 5), (29, 27, 5, 3))
PLANES = (12 * 256, 12 * 7 * 256)


def _timed(step, seconds):
    """seconds per call of `step`: warm-up, then batches that end in a synchronise until `seconds` have passed"""
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    batch = max(1, int(0.05 / max(time.perf_counter() - t0, 1e-6)))
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(batch):
            step()
        torch.cuda.synchronize()
        n += batch
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def copy_ceiling(gib=2, iters=10):
    """GB/s of bytes moved (read + written) by the library's copy probe, far beyond the Infinity Cache"""
    n = gib << 30
    src = torch.empty(n // 4, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty(n // 4, dtype=torch.float32, device=DEV)
    run = lambda: hip.check(hip.lib().usot_bw_probe(hip.stream(), hip.ptr(src), hip.ptr(dst), n, 1), 'usot_bw_probe')
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 2 * n / (e0.elapsed_time(e1) / iters * 1e-3) / 1e9


def point(shape, P, seconds, ceiling):
    hx, wx, hk, wk = shape
    oh, ow = hx - hk + 1, wx - wk + 1
    g = torch.Generator(device=DEV).manual_seed(P + hx * wk)
    x = torch.randn(P // 256, 256, hx, wx, device=DEV, generator=g)
    k = torch.randn(P // 256, 256, hk, wk, device=DEV, generator=g)
    dout = torch.randn(P // 256, 256, oh, ow, device=DEV, generator=g)
    xa, ka = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    xb, kb = x.view(1, P, hx, wx).clone().requires_grad_(True), k.view(P, 1, hk, wk).clone().requires_grad_(True)
    db = dout.view(1, P, oh, ow)

    def ours():
        return torch.autograd.grad(autograd.xcorr_depthwise(xa, ka), (xa, ka), dout)

    def grouped():
        return torch.autograd.grad(F.conv2d(xb, kb, groups=P), (xb, kb), db)

    # the two formulations compute the same thing (float32 against float32: summation orders differ)
    (ga, gka), (gb, gkb) = ours(), grouped()
    agree = [float((ga.view(-1) - gb.view(-1)).abs().max() / gb.abs().max()), float((gka.view(-1) - gkb.view(-1)).abs().max() / gkb.abs().max())]
    del ga, gka, gb, gkb
    contenders = [('hip_autograd', ours), ('grouped_conv2d_autograd', grouped),
                  ('kernel_forward', lambda: hip.xcorr_depthwise(x, k)),
                  ('kernel_bwd_x', lambda: hip.xcorr_depthwise_backward_x(dout, k, x.shape)),
                  ('kernel_bwd_k', lambda: hip.xcorr_depthwise_backward_k(dout, x, k.shape))]
    got = {}
    for order in (contenders, contenders[::-1]):
        for name, fn in order:
            got.setdefault(name, []).append(_timed(fn, seconds) * 1e6)
    nx, nk, no = P * hx * wx * 4, P * hk * wk * 4, P * oh * ow * 4
    bytes_ = {'kernel_forward': nx + nk + no, 'kernel_bwd_x': no + nk + nx, 'kernel_bwd_k': no + nx + nk}
    row = dict(shape='%dx%d*%dx%d' % shape, planes=P, us_per_call={n: [round(v, 2) for v in t] for n, t in got.items()},
               ratio_grouped_over_hip=[round(b / a, 3) for a, b in zip(got['hip_autograd'], got['grouped_conv2d_autograd'])],
               max_abs_diff_over_max=dict(dx=agree[0], dk=agree[1]), algorithmic_bytes=bytes_, kernels={})
    for n, nbytes in bytes_.items():
        gbs = [nbytes / (t * 1e-6) / 1e9 for t in got[n]]
        row['kernels'][n] = dict(gb_per_s=[round(v, 1) for v in gbs], frac_of_copy_ceiling=[round(v / ceiling, 3) for v in gbs])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--planes', type=int, nargs='+', default=list(PLANES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('xcorr_grad_probe: no GPU (nothing is measured on a CPU)')
    ceiling = copy_ceiling()
    torch.cuda.empty_cache()
    rows = []
    for P in a.planes:
        for shape in SHAPES:
            rows.append(point(shape, P, a.seconds, ceiling))
            print('%s P %d: %s' % (rows[-1]['shape'], P, rows[-1]['us_per_call']), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(dict(probe='xcorr_grad', unit='us per call, two timed passes each (a call of the *_autograd rows = forward + both gradients)',
                          device=torch.cuda.get_device_name(0), host=socket.gethostname(), seconds_per_point=a.seconds,
                          copy_ceiling_gb_per_s=round(ceiling, 1),
                          note='working sets: %.0f MB at P = 3072, %.0f MB at P = 21504 (29x29*5x5): inside the 256 MiB Infinity Cache, '
                               'so a fraction of the HBM copy ceiling above 1 is possible' % (3072 * 1491 * 4 / 1e6, 21504 * 1491 * 4 / 1e6),
                          rows=rows)))


if __name__ == '__main__':
    main()
