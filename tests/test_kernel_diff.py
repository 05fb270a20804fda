"""CPU: scripts/kernel_diff.py on short synthetic listings - the per-kernel text comparison that shows a refactor of a
translation unit left its device code alone (same bodies, same .amdhsa_kernel descriptors, whatever the emission order)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_diff as kd  # noqa: E402


def _kernel(name, index, add='v_add_f32_e32 v1, v0, v0', vgprs=8):
    """one kernel as hipcc prints it: body with local labels that carry the function's index, then its descriptor block"""
    return '''\t.text
\t.globl\t{n}
\t.p2align\t8
\t.type\t{n},@function
{n}:                                    ; @{n}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\ts_cmp_lg_u32 s0, 0
\ts_cbranch_scc1 .LBB{i}_2
; %bb.1:
\t{add}
.LBB{i}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {n}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {v}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{i}:
\t.size\t{n}, .Lfunc_end{i}-{n}
'''.format(n=name, i=index, add=add, v=vgprs)


def test_swapped_order_and_renumbered_labels_compare_equal():
    a = _kernel('_Z5alphav', 0) + _kernel('_Z4betav', 1, add='v_mul_f32_e32 v1, v0, v0')
    b = _kernel('_Z4betav', 0, add='v_mul_f32_e32 v1, v0, v0') + _kernel('_Z5alphav', 1)
    assert a != b
    assert sorted(kd.kernels(a)) == ['_Z4betav', '_Z5alphav']
    body, desc = kd.kernels(a)['_Z5alphav']
    assert 's_endpgm' in body and 'v_add_f32_e32 v1, v0, v0' in body and '.amdhsa_next_free_vgpr 8' in desc
    assert kd.compare(a, b) == ([], [], [])


def test_a_changed_instruction_is_reported_under_its_symbol():
    a = _kernel('_Z5alphav', 0) + _kernel('_Z4betav', 1)
    b = _kernel('_Z5alphav', 0) + _kernel('_Z4betav', 1, add='v_sub_f32_e32 v1, v0, v0')
    only_a, only_b, differ = kd.compare(a, b)
    assert only_a == [] and only_b == []
    assert [(d[0], d[1]) for d in differ] == [('_Z4betav', 'body')]
    assert differ[0][3] == 'v_add_f32_e32 v1, v0, v0' and differ[0][4] == 'v_sub_f32_e32 v1, v0, v0'


def test_a_missing_kernel_is_reported():
    a = _kernel('_Z5alphav', 0) + _kernel('_Z4betav', 1)
    b = _kernel('_Z5alphav', 0)
    assert kd.compare(a, b) == (['_Z4betav'], [], [])
    assert kd.compare(b, a) == ([], ['_Z4betav'], [])


def test_a_changed_descriptor_line_is_reported():
    a = _kernel('_Z5alphav', 0)
    b = _kernel('_Z5alphav', 0, vgprs=12)
    only_a, only_b, differ = kd.compare(a, b)
    assert only_a == [] and only_b == []
    assert [(d[0], d[1]) for d in differ] == [('_Z5alphav', 'descriptor')]
    assert differ[0][3] == '.amdhsa_next_free_vgpr 8' and differ[0][4] == '.amdhsa_next_free_vgpr 12'


def test_command_line_exit_status(tmp_path, capsys):
    pa, pb = tmp_path / 'a.s', tmp_path / 'b.s'
    pa.write_text(_kernel('_Z5alphav', 0))
    pb.write_text(_kernel('_Z5alphav', 3))
    assert kd.main([str(pa), str(pb)]) == 0
    pb.write_text(_kernel('_Z5alphav', 3, add='v_sub_f32_e32 v1, v0, v0'))
    assert kd.main([str(pa), str(pb)]) == 1
    assert 'differs: _Z5alphav (body' in capsys.readouterr().out
