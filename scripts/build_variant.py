#!/usr/bin/env python3
"""Builds usot_amd/csrc/alt/lib_<name>.so: the library with ONE translation unit recompiled under extra -D flags (timing /
ablation builds; usot_amd/csrc/alt/ is git-ignored but travels to the GPU box).  The other objects are the up-to-date ones
of the normal build.  A variant whose record (lib_<name>.json: source tree, unit, flags) matches is not built again.
    python scripts/build_variant.py <name> <file.hip> -DUSOT_ABL_NOW [...]
The unit is the .hip file even where the switch stands in one of its headers: USOT_ABL_* / USOT_TRACE are read by csrc/conv_f32_v3.h,
USOT_WS_* / USOT_WSTAT_* by csrc/lab/conv_f32_wstream.h / conv_f32_wstat.h (with -DUSOT_EXPERIMENTS), all built as conv_igemm.hip."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usot_amd import build as b
name, unit, flags = sys.argv[1], sys.argv[2], sys.argv[3:]
alt = os.path.join(b.CSRC, 'alt')
os.makedirs(alt, exist_ok=True)
lib = os.path.join(alt, 'lib_%s.so' % name)
rec, want = lib[:-3] + '.json', {'csrc_tree': b.csrc_tree(), 'unit': unit, 'flags': flags}
try:
    with open(rec) as f:
        if json.load(f) == want and os.path.exists(lib):
            print(lib)
            sys.exit(0)
except (OSError, ValueError):
    pass
b.build()
obj = os.path.join(alt, '%s_%s.o' % (name, unit[:-4]))
subprocess.check_call([b._hipcc()] + b.FLAGS + b.FILE_FLAGS.get(unit, []) + flags + ['-c', os.path.join(b.CSRC, unit), '-o', obj])
objs = [obj if os.path.basename(s) == unit else s[:-4] + '.o' for s in b.sources()]
subprocess.check_call([b._hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs)
with open(rec, 'w') as f:
    json.dump(want, f)
print(lib)
