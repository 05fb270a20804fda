#!/usr/bin/env python3
"""How long is a kernel's start-up in the BUILT code?  Compiles a translation unit of usot_amd/csrc to gfx950 assembly as
usot_amd/build.py does (build.FLAGS + FILE_FLAGS) and prints, per kernel, for the path of a wave that STAGES k-tile 0 - from the
kernel's entry to its first barrier, following the branches (start_up_path(): in conv_igemm_f32_v3 the common index
prologue and the PRODUCER waves' block, which the listing holds behind the consumers' whole path):
    instr    instructions in front of the first tile load (vector-memory load of 16 bytes a lane)
    div      integer-division expansions (v_rcp_iflag_f32: one per `/` or `%` by a run-time divisor) up to the fourth tile load
    rounds   s_load groups that are followed by a full wait, s_waitcnt lgkmcnt(0), up to the fourth tile load: the DEPENDENT
             scalar-memory round trips
    between  s_load instructions between the first and the fourth tile load (the x and w loads of k-tiles 0 and 1 of a conv
             tile: a scalar fetch between them keeps the cold round trips from being in flight together)
    vloads   tile loads found on the path, up to four
Parsed: block labels and branch targets, instruction mnemonics (s_load, vector loads, wide ds_write, s_barrier, s_endpgm,
v_rcp_iflag_f32) and lgkmcnt(0); nothing else (docs/LAB_NOTEBOOK.md A.9).
    python scripts/prologue_depth.py [conv_igemm.hip | smallm_f32.hip] [-DUSOT_EXPERIMENTS ...]
tests/test_conv_prologue_schedule.py imports this file."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VLOAD = ('global_load', 'buffer_load', 'flat_load', 'scratch_load')


def assembly(unit, flags=()):
    """gfx950 assembly of usot_amd/csrc/<unit> under the library's flags + `flags`."""
    from usot_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit[:-4] + '.s')
        subprocess.check_call([b._hipcc()] + b.FLAGS + b.FILE_FLAGS.get(unit, []) + list(flags) +
                              ['--cuda-device-only', '-S', os.path.join(b.CSRC, unit), '-o', out])
        with open(out) as f:
            return f.read()


def demangle(syms):
    """{mangled: readable} through llvm-cxxfilt / c++filt where one is there, else the mangled names themselves"""
    from usot_amd import build as b
    for tool in (os.path.join(os.path.dirname(os.path.realpath(b._hipcc())), '..', 'lib', 'llvm', 'bin', 'llvm-cxxfilt'), 'llvm-cxxfilt', 'c++filt'):
        try:
            out = subprocess.run([tool] + list(syms), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode().splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
        if len(out) == len(syms):
            names = {}
            for s, d in zip(syms, out):
                d = re.sub(r'^void \(anonymous namespace\)::', '', d)
                d = re.sub(r'\(.*\)$', '', d).replace('(anonymous namespace)::', '').replace(' ', '')
                names[s] = re.sub(r'\((?:int|bool)\)', '', d)
            return names
    return {s: s for s in syms}


def kernels(asm):
    """[(mangled symbol, [instruction lines and `.Lname:` block labels])] of every kernel (.amdhsa_kernel symbols) in listing order"""
    entry = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M))
    out, cur = [], None
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r'^(\w+):', s)
        if m and not s.startswith('.L'):
            cur = None
            if m.group(1) in entry:
                cur = []
                out.append((m.group(1), cur))
            continue
        if cur is None or not s:
            continue
        lab = re.match(r'^(\.L\w+):', s)
        if lab:
            cur.append(lab.group(1) + ':')        # a basic-block label (start_up_path follows the branches)
            continue
        if s[0] in '.;' or s.endswith(':'):
            continue
        cur.append(s.split(';')[0].strip())
    return out


WIDE_STORE = ('ds_write_b64', 'ds_write_b128', 'ds_write2', 'ds_store_b64', 'ds_store_b128')      # tile rows (a split-K ticket flag is a b32)


def _op(s):
    return s.split()[0]


def _is_sload(op):
    return op.startswith('s_load') or op.startswith('s_buffer_load')


def start_up_path(body):
    """The instructions a STAGING wave runs from the kernel's entry to its first barrier, in listing order: the basic blocks that are
    reachable from the entry without passing an s_barrier AND lead to, hold or follow a wide LDS store (ds_write_b64 / _b128: the
    rows of k-tiles 0 and 1).  In the producer / consumer kernels (v3) this is
    the common index prologue plus the producer waves' block - which the listing holds far behind the consumers' path - and none of
    the consumers' or DMA waves' code, which never stores tile rows; in v1 / v2 and the small-M kernels every wave stages.  Both arms
    of an if / else on the path are counted.  None: the kernel stores no tile rows before its first barrier."""
    blocks, cur = [], {'label': None, 'ins': []}              # split at labels and behind branches / barriers / s_endpgm
    for s in body:
        if s.endswith(':') and s.startswith('.L'):
            if cur['ins'] or cur['label']:
                blocks.append(cur)
            cur = {'label': s[:-1], 'ins': []}
            continue
        cur['ins'].append(s)
        if _op(s).startswith(('s_branch', 's_cbranch', 's_endpgm', 's_setpc', 's_barrier')):
            blocks.append(cur)
            cur = {'label': None, 'ins': []}
    if cur['ins']:
        blocks.append(cur)
    at = {b['label']: i for i, b in enumerate(blocks) if b['label']}
    succ = []
    for i, b in enumerate(blocks):
        last = b['ins'][-1] if b['ins'] else ''
        op = _op(last) if last else ''
        if op.startswith(('s_endpgm', 's_setpc', 's_barrier')):
            nxt = []
        elif op.startswith('s_branch'):
            nxt = [at[last.split()[-1]]] if last.split()[-1] in at else []
        else:
            nxt = [i + 1] if i + 1 < len(blocks) else []
            if op.startswith('s_cbranch') and last.split()[-1] in at:
                nxt.append(at[last.split()[-1]])
        succ.append(nxt)

    def closure(seeds, edges):
        seen, todo = set(seeds), list(seeds)
        while todo:
            for j in edges[todo.pop()]:
                if j not in seen:
                    seen.add(j)
                    todo.append(j)
        return seen
    fwd = closure([0], succ)
    stores = [i for i in fwd if any(_op(s).startswith(WIDE_STORE) for s in blocks[i]['ins'])]
    if not stores:
        return None
    pred = [[] for _ in blocks]
    for i, nxt in enumerate(succ):
        for j in nxt:
            pred[j].append(i)
    on_path = (fwd & closure(stores, pred)) | closure(stores, succ)      # ... and on from the stores to the barrier
    return [s for i in sorted(on_path) for s in blocks[i]['ins']]


def _count(ins):
    """(instructions, division expansions, s_load groups followed by a full lgkmcnt wait) of an instruction list"""
    instr = div = rounds = 0
    open_loads = False
    for s in ins:
        op = _op(s)
        instr += 1
        if op.startswith('v_rcp_iflag_f32'):
            div += 1
        if _is_sload(op):
            open_loads = True
        elif op == 's_waitcnt' and 'lgkmcnt(0)' in s and open_loads:
            rounds += 1
            open_loads = False
    return instr, div, rounds


def depth(body):
    """Start-up counts of one kernel on start_up_path().  The TILE loads are the vector-memory loads of 16 bytes a lane (dwordx4: a
    conv tile's x and w rows; the one-word `*n_dyn` fetch of a build that makes it a vector load is not one):
      instr    instructions in front of the first tile load
      div      division expansions up to the fourth tile load
      rounds   s_load groups followed by a full lgkmcnt wait, up to the fourth tile load
      between  s_load between the first and the fourth tile load
      vloads   tile loads on the path, counted up to four"""
    path = start_up_path(body)
    if path is None:                              # no tile rows stored before a barrier: the listing up to its first barrier
        ins = [s for s in body if not s.endswith(':')]
        bar = next((i for i, s in enumerate(ins) if _op(s) == 's_barrier'), len(ins))
        path = ins[:bar]
    loads = [i for i, s in enumerate(path) if _op(s).startswith(VLOAD) and 'dwordx4' in _op(s)][:4]
    first = loads[0] if loads else len(path)
    last = loads[-1] if loads else len(path)
    instr, _, _ = _count(path[:first])
    _, div, rounds = _count(path[:last])
    between = sum(_is_sload(_op(s)) for s in path[first:last])
    return {'instr': instr, 'div': div, 'rounds': rounds, 'between': between, 'vloads': len(loads)}


def named_kernels(asm):
    """{readable kernel name: instruction list} of a listing"""
    ks = kernels(asm)
    names = demangle([k for k, _ in ks])
    return {names[k]: body for k, body in ks}


def table(unit, flags=()):
    """{readable kernel name: depth()} of a unit"""
    return {k: depth(body) for k, body in named_kernels(assembly(unit, flags)).items()}


def main(argv):
    flags = [a for a in argv if a.startswith('-')]
    units = [a for a in argv if not a.startswith('-')] or ['conv_igemm.hip', 'smallm_f32.hip']
    for unit in units:
        print('%s   (start-up path of a staging wave: instr to the first tile load / div / rounds; s_load between tile loads 1 and 4)' % unit)
        for name, d in sorted(table(unit, flags).items()):
            print('  %-64s instr %4d  div %2d  rounds %2d  between %2d  vloads %d' % (name, d['instr'], d['div'], d['rounds'], d['between'], d['vloads']))

if __name__ == '__main__':
    main(sys.argv[1:])
