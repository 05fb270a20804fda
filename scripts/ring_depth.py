#!/usr/bin/env python3
"""How deep is the filter ring of usot_amd/csrc/smallm_f32.hip in the BUILT code?  Compiles the file to gfx950 assembly as
usot_amd/build.py does and, per kernel, prints the histogram of the `s_waitcnt vmcnt(n)` that stand in front of MFMA groups:
n is the number of vector-memory operations the wave may still have in flight when it starts a fragment's MFMAs - the ring
depth the hardware sees (the source asks for USOT_RING - 1 or more; docs/LAB_NOTEBOOK.md A.5).  Only v_mfma, global_load and
vmcnt are parsed.
    python scripts/ring_depth.py [-DUSOT_RING_UNPINNED] [-DUSOT_RING=12] [...]
Beside the histogram: per MFMA group, whether its wait allows what the source's issue order leaves in flight behind it (needs()).
tests/test_smallm_ring_schedule.py imports this file."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIT = 'smallm_f32.hip'
KERNELS = ('pw_pair_f32_kernel', 'pw_triple_f32_kernel', 'pw_single_f32_kernel', 'stream_conv3x3_f32_kernel')
# the instantiations the launchers route to (template arguments as the mangled name spells them, defaults included)
ROUTED = [
    'pw_pair_f32_kernel<256,1024,256,4,0>', 'pw_pair_f32_kernel<128,512,128,4,0>',
    'pw_pair_f32_kernel<64,256,64,1,0>', 'pw_pair_f32_kernel<64,256,128,1,0>', 'pw_pair_f32_kernel<128,512,256,1,0>',
    'pw_triple_f32_kernel<64,64,256,64>', 'pw_triple_f32_kernel<64,64,256,128>', 'pw_triple_f32_kernel<128,128,512,128>',
    'pw_single_f32_kernel<1024,256,4,%d>', 'pw_single_f32_kernel<256,1024,8,%d>', 'pw_single_f32_kernel<512,128,2,%d>',
    'pw_single_f32_kernel<128,512,4,%d>',
    'stream_conv3x3_f32_kernel<256,256,4>', 'stream_conv3x3_f32_kernel<128,128,4>',
]


def routed(ring=8):
    return [k % ring if '%d' in k else k for k in ROUTED]


def assembly(flags=()):
    """gfx950 assembly of smallm_f32.hip under the library's flags + `flags`."""
    from usot_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'smallm_f32.s')
        subprocess.check_call([b._hipcc()] + b.FLAGS + b.FILE_FLAGS.get(UNIT, []) + list(flags) +
                              ['--cuda-device-only', '-S', os.path.join(b.CSRC, UNIT), '-o', out])
        with open(out) as f:
            return f.read()


def _name(sym):
    """'pw_pair_f32_kernel<256,1024,256,4,0>' from the mangled symbol of a kernel in the anonymous namespace (or None)."""
    for k in KERNELS:
        i = sym.find('%d%sI' % (len(k), k))
        if i >= 0:
            args = re.findall(r'L[ib](\d+)E', sym[i:].split('EEv')[0] + 'E')
            return '%s<%s>' % (k, ','.join(args))
    return None


def histograms(asm):
    """{kernel: Counter{n: waits}} over the `s_waitcnt .. vmcnt(n)` that are followed by a v_mfma before the next vmcnt wait
    (waits in front of MFMA groups), counted from the kernel's first global_load on."""
    out = {}
    cur, pending, started = None, None, False
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r'^(_Z\w+):', s)
        if m:
            cur = _name(m.group(1))
            if cur is not None:
                out[cur] = collections.Counter()
            pending, started = None, False
            continue
        if cur is None:
            continue
        if s.startswith('s_endpgm'):
            cur = None
        elif s.startswith('global_load'):
            started = True
        elif s.startswith('s_waitcnt'):
            m = re.search(r'vmcnt\((\d+)\)', s)
            if m and started:
                pending = int(m.group(1))
        elif s.startswith('v_mfma'):
            if pending is not None:
                out[cur][pending] += 1
                pending = None
    return out


def groups(asm):
    """{kernel: [wait or None per MFMA group, in program order]}: a group is one fragment's MFMAs (four v_mfma_f32_16x16x4_f32, or
    the three v_mfma_f32_16x16x32_f16 of a split-fp16 fragment pair); its wait is the smallest vmcnt(n) between the previous
    group's last MFMA and its own last one, None when there is none (everything it reads has landed already)."""
    out = {}
    cur, pending, count = None, None, 0
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r'^(_Z\w+):', s)
        if m:
            cur = _name(m.group(1))
            if cur is not None:
                out[cur] = []
            pending, count = None, 0
            continue
        if cur is None:
            continue
        if s.startswith('s_endpgm'):
            cur = None
        elif s.startswith('s_waitcnt'):
            m = re.search(r'vmcnt\((\d+)\)', s)
            if m:
                pending = int(m.group(1)) if pending is None else min(pending, int(m.group(1)))
        elif s.startswith('v_mfma'):
            count += 1
            if count == (3 if '16x16x32' in s else 4):
                out[cur].append(pending)
                pending, count = None, 0
    return out


def gemms(kernel, ring=8):
    """[(fragments N, ring depth PF, fragments per MFMA group)] of the ring GEMMs of a kernel, in program order: the constants of
    smallm_f32.hip (GemmRing, pair_tail, the kernels) from the template arguments."""
    name, args = kernel[:-1].split('<')
    a = [int(v) for v in args.split(',')]

    def one(K, NB, pfd=ring, step=1):             # NB column blocks of a workgroup over K: waves x k-slices (KS) x blocks per wave (CBW)
        ks = 1 if NB >= 8 else 8 // NB
        cbw = NB // 8 if NB >= 8 else 1
        n = cbw * (K // 16 // ks)
        return (n, min(n, pfd), step)

    def pair(cm, cot, cn, s=1, h16=0):
        co = cot // s
        return [(co // 16 // 8 * (cm // 16), min(co // 16 // 8 * (cm // 16), ring), 2 if h16 else 1), one(co, cn // 16, step=2 if h16 else 1)]
    if name == 'pw_pair_f32_kernel':
        return pair(*a)
    if name == 'pw_triple_f32_kernel':
        return [one(9 * a[0], a[1] // 16)] + pair(a[1], a[2], a[3])
    if name == 'pw_single_f32_kernel':
        return [one(a[0], a[1] // 16 // a[2], pfd=a[3])]
    if name == 'stream_conv3x3_f32_kernel':
        return [one(9 * a[0], a[1] // 16 // a[2])]
    raise ValueError(kernel)


def needs(kernel, ring=8):
    """Per MFMA group, the loads the SOURCE leaves in flight behind the fragment(s) the group consumes, capped at PF - 1: the
    refill of the slot is issued in front of the group, so PF - 1 or more in the steady state; in the drain of a ring (its last
    PF - 1 fragments) only what is left of the GEMM.  A wait in front of the group that allows fewer has lost part of the ring."""
    out = []
    for n, pf, step in gemms(kernel, ring):
        out += [min(pf - 1, n - step - g) for g in range(0, n, step)]
    return out


def first_groups(kernel, ring=8):
    """index of the first MFMA group of every ring GEMM: what stands in front of it is the full wait of the barrier that publishes
    its B operand (the pixel tile's loads are younger than the prefetched ring), not a wait of the ring"""
    out, at = [], 0
    for n, pf, step in gemms(kernel, ring):
        out.append(at)
        at += n // step
    return out


def shallow(waits, need, skip=()):
    """[(group, wait, need)] of the groups that wait for more than the source makes them"""
    return [(i, w, d) for i, (w, d) in enumerate(zip(waits, need)) if w is not None and w < d and i not in skip]


def majority_is_reachable(kernel, ring=8):
    """Whether 'most waits allow PF - 1 loads in flight' can hold for this instantiation whatever lands early: the fragments
    beyond the prefetched PF that still have a full ring behind them outnumber the drains (PF - 1 waits per GEMM, shallower
    by the source's own order) and the GEMMs' first groups."""
    sure = sum(max(0, n - 2 * pf + 1) // step for n, pf, step in gemms(kernel, ring))
    drain = sum((pf - 1) // step + 1 for n, pf, step in gemms(kernel, ring))
    return sure > drain


def deep_share(hist, depth):
    """(waits that allow >= depth operations in flight, all counted waits)"""
    return sum(c for n, c in hist.items() if n >= depth), sum(hist.values())


def main(argv):
    flags = [a for a in argv if a.startswith('-D')]
    ring = 8
    for a in flags:
        if a.startswith('-DUSOT_RING='):
            ring = int(a.split('=')[1])
    asm = assembly(flags)
    hs, gs = histograms(asm), groups(asm)
    names = routed(ring) + sorted(k for k in hs if k not in routed(ring))
    for k in names:
        if k not in hs:
            print('%-46s not in the assembly' % k)
            continue
        deep, n = deep_share(hs[k], ring - 1)
        try:
            need = needs(k, ring)
            lost = 'groups %3d, %3d shallower than the source' % (len(gs[k]), len(shallow(gs[k], need, first_groups(k, ring)))) if len(need) == len(gs[k]) else 'groups ?'
        except ValueError:
            lost = ''
        print('%-46s waits %3d  >= %d in flight: %3d  %s   vmcnt %s' % (k, n, ring - 1, deep, lost, dict(sorted(hs[k].items()))))


if __name__ == '__main__':
    main(sys.argv[1:])
