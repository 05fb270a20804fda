"""The filter ring of csrc/smallm_f32.hip in the BUILT code: the file is compiled to gfx950 assembly and the `s_waitcnt vmcnt(n)`
in front of the MFMA groups are read (scripts/ring_depth.py; only v_mfma, global_load and vmcnt are parsed).  hipcc's scheduler
once sank every refill of the ring to its use - one to three fragments in flight where the source asks for eight - without any
test noticing; this one does.  No GPU needed; skipped where hipcc is absent."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import ring_depth  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('hipcc') or os.environ.get('HIPCC')),
                                reason='hipcc not found')
PF = 8              # USOT_RING of the default build
LAYER3_PAIR = 'pw_pair_f32_kernel<256,1024,256,4,0>'


@pytest.fixture(scope='module')
def pinned_asm():
    return ring_depth.assembly()


@pytest.fixture(scope='module')
def pinned(pinned_asm):
    return ring_depth.histograms(pinned_asm)


@pytest.fixture(scope='module')
def unpinned():
    asm = ring_depth.assembly(['-DUSOT_RING_UNPINNED'])
    return ring_depth.histograms(asm), ring_depth.groups(asm)


def test_routed_list_matches_the_issue_of_the_launchers():
    ks = ring_depth.routed(PF)
    count = lambda p: sum(k.startswith(p) for k in ks)
    assert (count('pw_pair_f32_kernel'), count('pw_triple_f32_kernel'), count('pw_single_f32_kernel'), count('stream_conv3x3_f32_kernel')) == (5, 3, 4, 2)


@pytest.mark.parametrize('kernel', ring_depth.routed(PF))
def test_a_majority_of_the_waits_leaves_the_ring_in_flight(pinned, kernel):
    """Among the vmcnt waits in front of MFMA groups, most allow PF - 1 or more loads in flight - wherever arithmetic lets that
    hold: a GEMM of N fragments drains its ring over its last PF - 1 (waits PF - 2 .. 0 by the source's own order), and its first PF
    need no wait at all once a barrier has landed them, so an instantiation with N < 3 PF or so (layer2's pair: N = PF = 8, every
    wait is a drain) has no majority to show however well it is scheduled.  Those are held to the per-group rule below alone."""
    assert kernel in pinned, sorted(pinned)
    deep, waits = ring_depth.deep_share(pinned[kernel], PF - 1)
    print(kernel, dict(sorted(pinned[kernel].items())))
    assert waits > 0
    if ring_depth.majority_is_reachable(kernel, PF):
        assert 2 * deep > waits, (kernel, deep, waits, dict(sorted(pinned[kernel].items())))


def test_the_majority_rule_covers_the_kernels_the_time_is_in():
    reach = [k for k in ring_depth.routed(PF) if ring_depth.majority_is_reachable(k, PF)]
    assert LAYER3_PAIR in reach and 'pw_triple_f32_kernel<128,128,512,128>' in reach and 'stream_conv3x3_f32_kernel<256,256,4>' in reach


@pytest.fixture(scope='module')
def pinned_groups(pinned_asm):
    return ring_depth.groups(pinned_asm)


@pytest.mark.parametrize('kernel', ring_depth.routed(PF) + ['pw_pair_f32_kernel<128,512,128,1,0>', 'pw_pair_f32_kernel<256,1024,256,4,1>'])
def test_no_wait_is_shallower_than_the_source(pinned_groups, kernel):
    """Every instantiation, the unsliced fallback and the split-fp16 pair included: the MFMA groups in the assembly are the
    fragments of the source's GEMMs, in order, and the wait in front of group n allows min(PF - 1, fragments left behind it) loads
    in flight or more - the refill of its slot was issued first, nothing was sunk behind the MFMAs.  (The first group of a GEMM
    stands behind the barrier that publishes its B operand: exempt.)"""
    waits, need = pinned_groups[kernel], ring_depth.needs(kernel, PF)
    assert len(waits) == len(need), (len(waits), len(need))
    lost = ring_depth.shallow(waits, need, ring_depth.first_groups(kernel, PF))
    assert not lost, lost[:8]


def test_the_unpinned_build_of_layer3s_pair_does_not(unpinned):
    """... so the tests above measure the thing they are named for"""
    hist, groups = unpinned
    deep, waits = ring_depth.deep_share(hist[LAYER3_PAIR], PF - 1)
    assert waits > 0 and 2 * deep <= waits, (deep, waits, dict(sorted(hist[LAYER3_PAIR].items())))
    lost = ring_depth.shallow(groups[LAYER3_PAIR], ring_depth.needs(LAYER3_PAIR, PF), ring_depth.first_groups(LAYER3_PAIR, PF))
    assert len(lost) > len(groups[LAYER3_PAIR]) // 2
