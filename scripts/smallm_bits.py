#!/usr/bin/env python3
"""Every output of the small-M fp32 kernels (csrc/smallm_f32.hip) on seeded inputs, for the library given by USOT_HIP_LIB, written
as one torch file {case: [tensors]}: the default build (pinned ring, hoisted prefetches) and the -DUSOT_RING_UNPINNED build must
write the same BITS (tests/test_gpu_smallm_ring.py).  The smallest shapes that reach every path: M = 17 = one full and one ragged
16-pixel tile, M = 16 = an exact tile, M = 31 = a 15-row tail; 5 x 5 and 4 x 4 maps (M = 25, 16); the sliced forms run twice on
one workspace, so a ticket that was not reset shows.  A case name carries its size (_m16, _m31, _4x4); the names without one are
M = 17 and the 5 x 5 map.
    python scripts/smallm_bits.py OUT.pt"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from usot_amd import hip
DEV = 'cuda:0'
MS = (17, 16, 31)
MAPS = (5, 4)
PAIRS_UNSLICED = [(64, 256, 64), (64, 256, 128), (128, 512, 256)]
PAIRS_SLICED = [(128, 512, 128), (256, 1024, 256)]
TRIPLES = [(64, 64, 256, 64), (64, 64, 256, 128), (128, 128, 512, 128)]
SINGLES = [(1024, 256), (256, 1024), (512, 128), (128, 512)]
STREAMED = [(128, 128), (256, 256)]


def m_tag(M):
    return '' if M == 17 else '_m%d' % M


def map_tag(hw):
    return '' if hw == 5 else '_%dx%d' % (hw, hw)


REPEATED = ('pair_sliced_128_512_128', 'pair_sliced_256_1024_256', 'pair_deferred_256_1024_256', 'pair_split16_256_1024_256')


def repeated_cases():
    """The cases launched twice on one workspace: [y0, t0, y1, t1, ...]."""
    return [n + m_tag(M) for M in MS for n in REPEATED]


def cases():
    """Names of everything main() writes, in order (the test's parametrisation)."""
    out = []
    for M in MS:
        out += ['pair_%d_%d_%d' % s + m_tag(M) for s in PAIRS_UNSLICED]
        out += ['pair_sliced_%d_%d_%d' % s + m_tag(M) for s in PAIRS_SLICED]
        out += [n + m_tag(M) for n in ('pair_no_ws_128_512_128', 'pair_deferred_256_1024_256', 'pair_split16_256_1024_256')]
        out += ['single_%d_%d_%s' % (s + (r,)) + m_tag(M) for s in SINGLES for r in ('plain', 'res')]
    for hw in MAPS:
        out += ['triple_%d_%d_%d_%d_pd%d' % (s + (pd,)) + map_tag(hw) for s in TRIPLES for pd in (1, 2)]
        out += ['streamed_%d_%d_pd%d' % (s + (pd,)) + map_tag(hw) for s in STREAMED for pd in (1, 2)]
    return out


def main(path):
    g = torch.Generator().manual_seed(20250)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    res = {}

    def pair(M, cm, co, cn, ws=False, parts=0, rparts=0, split16=False, launches=1):
        """the pair through its descriptor; returns y and t of every launch (the same workspace for all of them)"""
        w3, w1 = rnd(co, cm) / cm ** 0.5, rnd(cn, co) / co ** 0.5
        b3, b1 = rnd(co), rnd(cn)
        t2 = rnd(max(parts, 1), M, cm) if parts else rnd(M, cm).abs()
        r = rnd(max(rparts, 1), M, co)
        tb, rb = rnd(cm), rnd(co)
        pack = hip.pw_pair_s16_pack if split16 else hip.pw_pair_f32_pack
        w3p, w1p = pack(w3), pack(w1)
        wsp = hip.pw_pair_f32_ws(M, cm, co, cn, DEV) if ws else None
        assert (wsp is not None) == ws
        ovf = torch.zeros(4, dtype=torch.int32, device=DEV)
        outs = []
        for _ in range(launches):
            y, t = torch.zeros(M, co, device=DEV), torch.zeros(M, cn, device=DEV)
            d = hip.pw_pair_desc(t2.data_ptr(), w3p.data_ptr(), b3.data_ptr(), r.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1.data_ptr(),
                                 t.data_ptr(), M, cm, co, cn, hip.ACT_RELU, wsp.data_ptr() if ws else None,
                                 t2_parts=parts, t2_bias=tb.data_ptr() if parts else None,
                                 res_parts=rparts, res_bias=rb.data_ptr() if rparts else None, ovf=ovf.data_ptr() if split16 else None)
            fn = hip.lib().usot_pw_pair_f32s if split16 else hip.lib().usot_pw_pair_f32
            hip.check(fn(hip.stream(), C.byref(d)), 'pw_pair_f32')
            torch.cuda.synchronize()
            outs += [y, t]
        if split16:
            assert int(ovf[0]) == 0                   # values inside the split-fp16 window
            outs.append(ovf)
        return outs

    for M in MS:
        tag = m_tag(M)
        for s in PAIRS_UNSLICED:
            res['pair_%d_%d_%d' % s + tag] = pair(M, *s)
        for s in PAIRS_SLICED:
            res['pair_sliced_%d_%d_%d' % s + tag] = pair(M, *s, ws=True, launches=2)
        res['pair_no_ws_128_512_128' + tag] = pair(M, 128, 512, 128)
        res['pair_deferred_256_1024_256' + tag] = pair(M, 256, 1024, 256, ws=True, parts=2, rparts=2, launches=2)
        res['pair_split16_256_1024_256' + tag] = pair(M, 256, 1024, 256, ws=True, split16=True, launches=2)
        for k, n in SINGLES:
            for r in ('plain', 'res'):
                x, w, b = rnd(M, k), rnd(n, k) / k ** 0.5, rnd(n)
                res['single_%d_%d_%s' % (k, n, r) + tag] = [hip.pw_single_f32(x, w, b, res=rnd(M, n) if r == 'res' else None, act=hip.ACT_RELU)]
    for hw in MAPS:
        tag = map_tag(hw)
        for cin, cm, co, cn in TRIPLES:
            for pd in (1, 2):
                x = rnd(1, hw, hw, cin).relu()
                args = (x, rnd(cm, 9 * cin) / (9 * cin) ** 0.5, rnd(cm), rnd(co, cm) / cm ** 0.5, rnd(co), rnd(1, hw, hw, co),
                        rnd(cn, co) / co ** 0.5, rnd(cn))
                res['triple_%d_%d_%d_%d_pd%d' % (cin, cm, co, cn, pd) + tag] = list(hip.pw_triple_f32(*args, pad=(pd, pd), dil=(pd, pd)))
        for cin, n in STREAMED:
            for pd in (1, 2):
                x, w, b = rnd(1, hw, hw, cin), rnd(n, 9 * cin) / (9 * cin) ** 0.5, rnd(n)
                res['streamed_%d_%d_pd%d' % (cin, n, pd) + tag] = [hip.stream_conv3x3_f32(x, w, b, (pd, pd), (pd, pd), act=hip.ACT_RELU)]
    torch.cuda.synchronize()
    assert list(res) == cases()
    torch.save({k: [t.cpu() for t in v] for k, v in res.items()}, path)
    print('smallm_bits', len(res), 'cases ->', path)


if __name__ == '__main__':
    main(sys.argv[1])
