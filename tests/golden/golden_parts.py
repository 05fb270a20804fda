"""A fixture larger than a committed file may be (1 MiB) is stored as parts: <name>.npz is written as <name>.0.npz, <name>.1.npz,
... (each a compressed .npz of whole arrays, in key order) and read back as one dict.  Callers keep naming the fixture <name>.npz."""
import glob
import os
import zlib

import numpy as np

PART_BYTES = 896 << 10          # compressed bytes per part, below the 1 MiB limit with room for the zip directory


def parts(path):
    """The part files of fixture `path` (.../<name>.npz), in order."""
    stem = path[:-len('.npz')]
    found = glob.glob(glob.escape(stem) + '.*.npz')
    return sorted((f for f in found if f[len(stem) + 1:-len('.npz')].isdigit()), key=lambda f: int(f[len(stem) + 1:-len('.npz')]))


def load(path):
    """Every array of fixture `path`, merged from its parts."""
    files = parts(path)
    if not files:
        raise FileNotFoundError('no parts of %s (%s.0.npz, ...)' % (path, path[:-len('.npz')]))
    out = {}
    for f in files:
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out


def save(path, arrays):
    """Write `arrays` as the parts of fixture `path` (old parts removed first); returns the part files."""
    for f in parts(path):
        os.remove(f)
    groups, cur, size = [], {}, 0
    for k in sorted(arrays):
        a = np.asarray(arrays[k])
        n = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + 256
        if cur and size + n > PART_BYTES:
            groups.append(cur)
            cur, size = {}, 0
        cur[k], size = a, size + n
    groups.append(cur)
    stem = path[:-len('.npz')]
    files = []
    for i, g in enumerate(groups):
        files.append('%s.%d.npz' % (stem, i))
        np.savez_compressed(files[-1], **g)
        assert os.path.getsize(files[-1]) < 1 << 20, (files[-1], os.path.getsize(files[-1]))
    return files
