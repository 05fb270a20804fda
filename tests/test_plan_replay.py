"""CPU: the launch-plan runtime (usot_amd/csrc/plan.hip) replayed against recording stubs, and the ctypes signatures of hip.lib().

The plan adders and an eager usot_plan_run make no HIP call, so tests/plan_replay/replay.cpp links plan.hip against stub launchers
that print what they receive.  tests/golden/plan_replay.txt is that program's output on the plan runtime as it was BEFORE its ops
became typed closures (the untyped argument-slot Op with a switch in issue()): every adder accepted once with all-distinct
arguments, every rejection with its status, op_info of every op, two eager runs, a run whose third launch fails.
tests/golden/hip_argtypes.json is {symbol: [argtypes, restype]} of every hip.EXPORTS entry as hip.lib() set them before the
(immediate, plan_add) pair table replaced the doubled statements."""
import json
import os
import subprocess

from usot_amd import build, hip

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def test_plan_replay_matches_the_recording(tmp_path):
    exe = str(tmp_path / 'replay')
    cmd = [build._hipcc()] + build.FLAGS + [os.path.join(HERE, 'plan_replay', 'replay.cpp'), os.path.join(build.CSRC, 'plan.hip'),
                                            '-o', exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors='replace')
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode(errors='replace')
    with open(os.path.join(GOLD, 'plan_replay.txt'), 'rb') as f:
        want = f.read()
    got = run.stdout
    if got != want:
        g, w = got.split(b'\n'), want.split(b'\n')
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        raise AssertionError('replay differs from the recording at line %d (%d vs %d lines):\n  got  %r\n  want %r'
                             % (first + 1, len(g), len(w), g[first:first + 1], w[first:first + 1]))


def _signature(fn):
    name = lambda t: None if t is None else t.__name__
    return [None if fn.argtypes is None else [name(t) for t in fn.argtypes], name(fn.restype)]


def test_hip_signatures_are_the_recorded_ones_and_pairs_agree():
    build.build(force=False)
    L = hip.lib()
    assert len(hip.PAIRS) >= 40
    seen = set()
    for immediate, plan_add, sig in hip.PAIRS:
        assert immediate in hip.EXPORTS and plan_add in hip.EXPORTS and plan_add.startswith('usot_plan_add_'), (immediate, plan_add)
        assert not {immediate, plan_add} & seen, (immediate, plan_add)          # one signature per name
        seen |= {immediate, plan_add}
        a, b = getattr(L, immediate), getattr(L, plan_add)
        assert a.argtypes is not None and list(a.argtypes) == list(b.argtypes) == list(sig), (immediate, plan_add)
        assert a.restype is b.restype, (immediate, plan_add)
    with open(os.path.join(GOLD, 'hip_argtypes.json')) as f:
        want = json.load(f)
    assert sorted(want) == sorted(hip.EXPORTS)
    got = {name: _signature(getattr(L, name)) for name in hip.EXPORTS}
    assert got == want, sorted(n for n in want if got[n] != want[n])
