"""CPU: the fp32 conv tile table (csrc/conv_igemm.hip: kTiles) answers every host query as recorded in
tests/golden/conv_tile_table.json, and the profile scripts' symbol -> name mapping agrees with it.

The fixture holds one block per build ('default', 'experiments'): per tile id the name, bm, bn, built, wfrag, dyn, xsplit, kreq,
kpanel, streamk, threads and lds_bytes.  Tile names are keys of profiles/pmc_*.json and the launch shape is what keeps a kernel
inside its LDS allocation, so a change of either must be a decision, not a side effect: regenerate with

    USOT_EXPERIMENTS=0|1 python tests/test_conv_tile_table.py

(rewrites the block of the library that is built; the other block is kept)."""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_tile_table.json')
FIELDS = ('name', 'bm', 'bn', 'built', 'wfrag', 'dyn', 'xsplit', 'kreq', 'kpanel', 'streamk', 'threads', 'lds_bytes')
STATS = ('mem_dedupe_kernel_stats.txt', 'mem_dedupe_parent_kernel_stats.txt')        # rocprofv3 kernel stats of the frame


def table():
    """(build key, {tile id: {field: value}}) of the loaded library."""
    from usot_amd import hip
    L = hip.lib()
    rows = {}
    for t in range(1, L.usot_conv_tile_count() + 1):
        bm, bn, kp, th, lds = (C.c_int(0) for _ in range(5))
        assert L.usot_conv_tile_info(t, C.byref(bm), C.byref(bn)) == 0
        kreq = L.usot_conv_tile_kreq(t, C.byref(kp))
        assert L.usot_conv_tile_launch(t, C.byref(th), C.byref(lds)) == 0
        rows[t] = dict(zip(FIELDS, (hip.tile_name(t), bm.value, bn.value, L.usot_conv_tile_built(t), L.usot_conv_tile_wfrag(t),
                                    L.usot_conv_tile_dyn(t), L.usot_conv_tile_xsplit(t), kreq, kp.value, L.usot_conv_tile_streamk(t),
                                    th.value, lds.value)))
    return ('experiments' if L.usot_experiments_built() else 'default'), rows


def test_tile_table_matches_the_recorded_one():
    from usot_amd import build, hip
    build.build(force=False)
    key, rows = table()
    with open(FIXTURE) as f:
        want = {int(t): r for t, r in json.load(f)[key].items()}
    assert sorted(rows) == sorted(want) == list(range(1, 118))
    for t in sorted(want):
        for field in FIELDS:
            assert rows[t][field] == want[t][field], (key, t, field)
        if rows[t]['built']:
            assert rows[t]['threads'] % 64 == 0 and 0 < rows[t]['threads'] <= 1024, t
            assert 0 < rows[t]['lds_bytes'] <= 160 * 1024, t
        else:
            assert rows[t]['name'] == '(tile %d: experiments build only)' % t
            assert (rows[t]['threads'], rows[t]['lds_bytes']) == (0, 0)
    L = hip.lib()
    for bad in (0, -1, len(want) + 1):
        assert L.usot_conv_tile_launch(bad, None, None) == -1            # USOT_EINVAL
    assert hip.tile_launch(1) == (rows[1]['threads'], rows[1]['lds_bytes'])


def test_profile_scripts_share_one_symbol_to_name_mapping():
    from usot_amd import build
    build.build(force=False)
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        from pmc_lp_traffic import f32_tile_name
    finally:
        sys.path.pop(0)
    _, rows = table()
    built = [r['name'] for r in rows.values() if r['built']]
    lines = []
    for name in STATS:
        with open(os.path.join(ROOT, 'profiles', name)) as f:
            lines += [ln for ln in f if ln.startswith('conv_igemm_f32')]
    assert len(lines) >= 16
    for ln in lines:
        assert built.count(f32_tile_name(ln)) == 1, ln
    assert f32_tile_name('stem_pool_kernel(StemArgs)') is None
    for script in ('pmc_busy.py', 'pmc_to_traffic.py'):                 # the one definition is pmc_lp_traffic's
        with open(os.path.join(ROOT, 'scripts', script)) as f:
            text = f.read()
        assert 'conv_igemm_f32' not in text.split('"""', 2)[2] and not re.search(r'^def (norm|f32_tile_name)\b', text, re.M), script
        assert re.search(r'^from pmc_lp_traffic import .*\bf32_tile_name\b', text, re.M), script


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from usot_amd import build
    if 'USOT_HIP_LIB' not in os.environ:
        build.build(force=False)
    key, rows = table()
    try:
        with open(FIXTURE) as f:
            doc = json.load(f)
    except FileNotFoundError:
        doc = {}
    doc[key] = {str(t): r for t, r in rows.items()}
    with open(FIXTURE, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%s: %d tiles recorded' % (key, len(rows)))
