"""The small-M fp32 kernels (csrc/smallm_f32.hip) pin the issue order of their filter ring and start the filter streams before the
barriers that do not concern them.  Neither touches a floating-point operation or its order: the default library and the
-DUSOT_RING_UNPINNED build (the schedule without pins and hoisting) must produce the same BITS on every output, y and t
(scripts/smallm_bits.py has the cases: M = 17 = a full and a ragged pixel tile, M = 16 = an exact tile, M = 31 = a 15-row tail,
5 x 5 and 4 x 4 maps, the sliced pairs twice on one workspace).  Each library is loaded in a child process of its own; the variant is built once per session."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import smallm_bits  # noqa: E402


@pytest.fixture(scope='session')
def both_builds(tmp_path_factory):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'build_variant.py'), 'ring_unpinned', 'smallm_f32.hip', '-DUSOT_RING_UNPINNED'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode(errors='replace')[-2000:]
    unpinned = r.stdout.decode().strip().splitlines()[-1]
    tmp = tmp_path_factory.mktemp('smallm_bits')
    outs = []
    for name, lib in (('pinned', None), ('unpinned', unpinned)):
        env = dict(os.environ)
        env.pop('USOT_HIP_LIB', None)
        if lib:
            env['USOT_HIP_LIB'] = lib
        path = str(tmp / (name + '.pt'))
        q = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'smallm_bits.py'), path], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert q.returncode == 0, q.stderr.decode(errors='replace')[-2000:]
        outs.append(torch.load(path))
    return outs


@pytest.mark.parametrize('case', smallm_bits.cases())
def test_pinned_ring_is_bit_identical_to_the_unpinned_build(both_builds, case):
    pinned, unpinned = both_builds
    assert len(pinned[case]) == len(unpinned[case]) > 0
    for i, (a, b) in enumerate(zip(pinned[case], unpinned[case])):
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0 or a.dtype == torch.int32, (case, i)
        assert torch.equal(a, b), (case, i, int((a != b).sum()))


def test_sliced_pairs_repeat_on_the_same_workspace(both_builds):
    """second launch on the workspace of the first (tickets reset by the last arriver): the same bits again"""
    for outs in both_builds:
        for case in smallm_bits.repeated_cases():
            y0, t0, y1, t1 = outs[case][:4]
            assert torch.equal(y0, y1) and torch.equal(t0, t1), case
