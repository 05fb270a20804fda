"""The start-up of the fp32 conv tiles in the BUILT code: csrc/conv_igemm.hip is compiled to gfx950 assembly under the library's
flags and scripts/prologue_depth.py follows the path of a wave that stages k-tiles 0 and 1 - from the kernel's entry through the
branches to the first barrier; in conv_igemm_f32_v3 that is the common index prologue and the PRODUCER waves' block, not the
consumers' bias / residual prefetch the listing shows first - and counts on it the integer-division expansions and the dependent
scalar-memory rounds up to the fourth tile load (the x and w loads of k-tiles 0 and 1), and the s_load that stand between the first
and the fourth.  The prologue block (conv_f32_common.h: ConvPro, conv_pro_fetch) and the host-made division constants (fastdiv.h)
are there so that these stay at zero divisions, at most three rounds and nothing between the loads; a compiler that sinks the
fetches back to their uses, or a new `/` by a run-time value in the index prologue, the row / pixel split or the first tap, shows
here.  No GPU needed; skipped where hipcc is absent.  (The small-M kernels of csrc/smallm_f32.hip start with ONE scalar round and
no division - docs/LAB_NOTEBOOK.md A.9 - and were not changed; they are held to the same bar so that it stays that way.)"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import prologue_depth  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('hipcc') or os.environ.get('HIPCC')),
                                reason='hipcc not found')

# the v2 / v3 rows of kTiles outside XT(...) (csrc/conv_igemm.hip): template arguments as the demangled name spells them
ROUTED = ['conv_igemm_f32_v2<32,64,2,2,32,1>', 'conv_igemm_f32_v2<32,64,2,2,64,1>', 'conv_igemm_f32_v2<32,32,2,2,64,1>',
          'conv_igemm_f32_v2<16,64,1,4,64,1>', 'conv_igemm_f32_v2<16,64,1,4,64,2>',
          'conv_igemm_f32_v3<64,64,2,2,32,1,4,1>', 'conv_igemm_f32_v3<32,64,2,2,64,1,4,1>', 'conv_igemm_f32_v3<32,32,2,2,64,1,4,1>',
          'conv_igemm_f32_v3<32,64,2,2,64,2,4,1>', 'conv_igemm_f32_v3<32,32,2,2,64,2,4,1>', 'conv_igemm_f32_v3<32,32,2,2,64,3,4,1>',
          'conv_igemm_f32_v3<32,32,2,2,64,2,8,1>', 'conv_igemm_f32_v3<32,32,2,2,64,3,8,1>', 'conv_igemm_f32_v3<32,64,2,2,64,2,8,1>',
          'conv_igemm_f32_v3<32,64,2,2,64,3,8,1>', 'conv_igemm_f32_v3<64,64,2,2,64,2,8,1>',
          'conv_igemm_f32_v3<32,64,2,2,64,2,8,4>', 'conv_igemm_f32_v3<32,64,2,2,64,3,8,4>', 'conv_igemm_f32_v3<32,32,2,2,64,2,8,4>',
          'conv_igemm_f32_v3<32,32,2,2,64,3,8,4>', 'conv_igemm_f32_v3<64,64,2,2,64,2,8,4>', 'conv_igemm_f32_v3<32,64,2,2,64,2,4,4>',
          'conv_igemm_f32_v3<32,32,2,2,64,2,4,4>', 'conv_igemm_f32_v3<32,64,2,2,64,3,4,5>', 'conv_igemm_f32_v3<32,64,2,2,64,2,8,5>',
          'conv_igemm_f32_v3<32,32,2,2,64,3,4,5>']
SMALLM = ('pw_pair_f32_kernel', 'pw_triple_f32_kernel', 'pw_single_f32_kernel', 'stream_conv3x3_f32_kernel')


@pytest.fixture(scope='module')
def conv_bodies():
    return prologue_depth.named_kernels(prologue_depth.assembly('conv_igemm.hip'))


@pytest.fixture(scope='module')
def conv(conv_bodies):
    return {k: prologue_depth.depth(body) for k, body in conv_bodies.items()}


@pytest.fixture(scope='module')
def smallm():
    return prologue_depth.table('smallm_f32.hip')


def test_every_routed_v2_and_v3_tile_is_in_the_listing(conv):
    built = sorted(k for k in conv if k.startswith(('conv_igemm_f32_v2<', 'conv_igemm_f32_v3<')))
    assert built == sorted(ROUTED)


@pytest.mark.parametrize('kernel', ROUTED)
def test_conv_tile_start_up(conv, kernel):
    d = conv[kernel]
    print(kernel, d)
    assert d['vloads'] == 4, d                     # the path reached the x and w loads of k-tiles 0 and 1
    assert d['div'] == 0, d
    assert d['rounds'] <= 3, d
    assert d['between'] == 0, d


def test_small_m_kernels_start_up(smallm):
    ks = {k: d for k, d in smallm.items() if k.startswith(SMALLM)}
    assert len(ks) >= 14, sorted(smallm)
    for k, d in sorted(ks.items()):
        print(k, d)
        assert d['vloads'] == 4 and d['div'] == 0 and d['rounds'] <= 3 and d['between'] == 0, (k, d)


def test_the_v3_path_is_the_producers(conv_bodies):
    """... and the counts above are taken where they are named for: on the dominant tile the path holds the row / pixel split and
    the tap walk of the producer waves, so it is longer than the stretch in front of the consumers' first prefetch load (148
    instructions in listing order), and its first four tile loads come in two groups (k-tile 0, k-tile 1) of adjacent loads"""
    path = prologue_depth.start_up_path(conv_bodies['conv_igemm_f32_v3<32,64,2,2,64,2,8,1>'])
    loads = [i for i, s in enumerate(path) if s.startswith(prologue_depth.VLOAD) and 'dwordx4' in s.split()[0]]
    assert len(loads) >= 6 and loads[0] > 180, loads
    assert loads[1] - loads[0] == 1 and loads[2] - loads[1] == 1, loads      # x and the two w rows of k-tile 0, back to back
    assert any(s.startswith(prologue_depth.WIDE_STORE) for s in path[loads[5]:])
    assert not any(s.startswith('ds_read') for s in path)                    # no consumer code on it
