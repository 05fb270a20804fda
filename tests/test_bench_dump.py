"""CPU: bench.py --dump-outputs writes float32 / float64 .npy files, and an output too large to write whole becomes a sample at
positions that depend on its size only (two builds of the project compare element for element)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_write_outputs_dtypes_and_fixed_sample(tmp_path):
    import bench
    big = torch.arange(bench.DUMP_LIMIT + 5, dtype=torch.float32)
    arrays = {'result': np.arange(8, dtype=np.float64), 'feat': torch.ones(2, 3, dtype=torch.bfloat16), 'big': big}
    bench.write_outputs(str(tmp_path / 'a'), arrays)
    bench.write_outputs(str(tmp_path / 'b'), arrays)
    got = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in arrays}
    assert got['result'].dtype == np.float64 and np.array_equal(got['result'], np.arange(8))
    assert got['feat'].dtype == np.float32 and got['feat'].shape == (2, 3) and (got['feat'] == 1).all()
    s = got['big']
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(s) >= 0) and s.max() < big.numel()
    assert np.array_equal(s, np.load(str(tmp_path / 'b' / 'big.npy')))          # the same positions on every call
    assert sum(os.path.getsize(str(f)) for f in (tmp_path / 'a').iterdir()) < 64 << 20


def test_plumbing_only_refuses_to_dump(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--plumbing-only', '--dump-outputs', str(tmp_path)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b'runs no frames' in r.stderr
