#!/usr/bin/env python3
"""Did a source change leave the device code alone?  Compares two gfx950 assembly listings (`hipcc --cuda-device-only -S`) kernel
by kernel, as TEXT: for every kernel symbol the function body and its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor block.
    python scripts/kernel_diff.py A.s B.s
    python scripts/kernel_diff.py --emit conv_igemm.hip out.s [-DUSOT_EXPERIMENTS ...]     # a listing under the library's flags
Local labels carry the index of the function in its translation unit (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>): the index is
normalised, so kernels that are emitted in another order - a template instantiated from another place - still compare equal.
Prints the symbols only in A, only in B, and every differing symbol with its first differing line; exit status 1 on any
difference.  The comparison looks for nothing in particular: equal text is equal code."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LABEL = re.compile(r'\.(LBB|Lfunc_begin|Lfunc_end|Ltmp)\d+')


def emit(unit, out, flags=()):
    """gfx950 assembly of usot_amd/csrc/<unit> under the library's flags + `flags` (as scripts/ring_depth.py: assembly())."""
    sys.path.insert(0, ROOT)
    from usot_amd import build as b
    flags = [f for f in flags if f not in b.FLAGS]
    subprocess.check_call([b._hipcc()] + b.FLAGS + b.FILE_FLAGS.get(unit, []) + list(flags) +
                          ['--cuda-device-only', '-S', os.path.join(b.CSRC, unit), '-o', out])


def _norm(line):
    line = line.split('//')[0].split(';')[0].rstrip()       # trailing comments (the compiler's notes: `; %bb.0:`, `; encoding`)
    return _LABEL.sub(lambda m: '.' + m.group(1) + 'N', line)


def kernels(asm):
    """{symbol: (body lines, descriptor lines)} of every kernel of a listing: a kernel is a symbol with an .amdhsa_kernel block;
    its body runs from its label to its .Lfunc_end label."""
    bodies, descs = {}, {}
    cur, body, cur_desc, desc = None, None, None, None
    for raw in asm.splitlines():
        s = raw.strip()
        if desc is not None:
            if s.startswith('.end_amdhsa_kernel'):
                descs[cur_desc] = desc
                desc = None
            elif _norm(s):
                desc.append(_norm(s))
            continue
        m = re.match(r'^\.amdhsa_kernel\s+(\S+)', s)
        if m:
            cur_desc, desc = m.group(1), []
            continue
        m = re.match(r'^([A-Za-z_][\w$.]*):', raw)
        if m:                                               # a global symbol (local labels start with a dot): a new body
            cur, body = m.group(1), []
            continue
        if body is None:
            continue
        if re.match(r'^\.Lfunc_end\d+:', s):
            bodies[cur] = body
            cur, body = None, None
            continue
        t = _norm(s)
        if t:
            body.append(t)
    return {k: (bodies.get(k, []), d) for k, d in descs.items()}


def first_difference(a, b):
    """(index, line of a or None, line of b or None) of the first place two line lists differ, None when they are equal"""
    for i in range(max(len(a), len(b))):
        la = a[i] if i < len(a) else None
        lb = b[i] if i < len(b) else None
        if la != lb:
            return i, la, lb
    return None


def compare(asm_a, asm_b):
    """(symbols only in A, symbols only in B, [(symbol, 'body' | 'descriptor', index, line A, line B)])"""
    ka, kb = kernels(asm_a), kernels(asm_b)
    only_a = sorted(set(ka) - set(kb))
    only_b = sorted(set(kb) - set(ka))
    differ = []
    for k in sorted(set(ka) & set(kb)):
        for part, name in ((0, 'body'), (1, 'descriptor')):
            d = first_difference(ka[k][part], kb[k][part])
            if d:
                differ.append((k, name) + d)
                break
    return only_a, only_b, differ


def main(argv):
    if argv and argv[0] == '--emit':
        emit(argv[1], argv[2], argv[3:])
        return 0
    if len(argv) != 2:
        print(__doc__)
        return 2
    with open(argv[0]) as f:
        asm_a = f.read()
    with open(argv[1]) as f:
        asm_b = f.read()
    only_a, only_b, differ = compare(asm_a, asm_b)
    print('%d kernels in %s, %d in %s' % (len(kernels(asm_a)), argv[0], len(kernels(asm_b)), argv[1]))
    for k in only_a:
        print('only in A: %s' % k)
    for k in only_b:
        print('only in B: %s' % k)
    for k, part, i, la, lb in differ:
        print('differs: %s (%s, line %d)\n    A: %s\n    B: %s' % (k, part, i + 1, la, lb))
    if only_a or only_b or differ:
        return 1
    print('no difference')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
