"""tools/asm_compare.py --exact: the gate of refactors that must leave every kernel's instructions alone.  Pure text processing on
synthetic assembly written here: label ordinals and kernel order must not matter, one changed instruction or one changed
.amdhsa_ value must."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "asm_compare.py")


def kernel(name, n, tmp, op="v_add_f32_e32 v0, v1, v2", vgpr=12):
    """One kernel as the compiler prints it: function ordinal n in its labels, .Ltmp numbers starting at tmp."""
    return """
\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                   ; @{name}
.Lfunc_begin{n}:
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\ts_cbranch_scc1 .LBB{n}_2
.Ltmp{tmp}:
; %bb.1:
\t{op}                                    ; encoding comment {n}
.LBB{n}_2:
\ts_endpgm
.Ltmp{tmp1}:
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t\t.amdhsa_accum_offset 12
\t.end_amdhsa_kernel
\t.text
; NumVgprs: {vgpr}
; Occupancy: 8
""".format(name=name, n=n, tmp=tmp, tmp1=tmp + 1, op=op, vgpr=vgpr)


def run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text("\t.text\n" + a + '\t.ident\t"clang A"\n')
    pb.write_text("\t.text\n" + b + '\t.ident\t"clang B"\n')
    return subprocess.run([sys.executable, TOOL, "--exact", str(pa), str(pb)], capture_output=True, text=True)


def test_label_ordinals_and_order_do_not_matter(tmp_path):
    # `after` lost the kernel in the middle: the survivors' ordinals and .Ltmp numbers shift, and they come in another order
    before = kernel("_Z2k0v", 0, 0) + kernel("_Z4gonev", 1, 2) + kernel("_Z2k1v", 2, 4, op="v_mul_f32_e32 v0, v1, v2")
    after = kernel("_Z2k1v", 0, 0, op="v_mul_f32_e32 v0, v1, v2") + kernel("_Z2k0v", 1, 2)
    r = run(tmp_path, before, after)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "RESULT: 2 kernels in both, 0 different, 1 only in the first, 0 only in the second" in r.stdout
    assert "gone()" in r.stdout
    # the other way round the second file has a kernel the first has not
    r = run(tmp_path, after, before)
    assert r.returncode == 1 and "0 different, 0 only in the first, 1 only in the second" in r.stdout


def test_changed_instruction_is_reported(tmp_path):
    r = run(tmp_path, kernel("_Z2k0v", 0, 0) + kernel("_Z2k1v", 1, 2), kernel("_Z2k0v", 0, 0) + kernel("_Z2k1v", 1, 2, op="v_add_f32_e32 v0, v1, v3"))
    assert r.returncode == 1
    assert "DIFFERS k1()" in r.stdout and "v_add_f32_e32 v0, v1, v3" in r.stdout and "DIFFERS k0()" not in r.stdout
    assert "RESULT: 2 kernels in both, 1 different" in r.stdout


def test_changed_amdhsa_value_is_reported(tmp_path):
    r = run(tmp_path, kernel("_Z2k0v", 0, 0), kernel("_Z2k0v", 0, 0, vgpr=13))
    assert r.returncode == 1
    assert "DIFFERS k0()" in r.stdout and ".amdhsa_next_free_vgpr 13" in r.stdout
