"""scripts/diff_device_asm.py: splitting assembly text per kernel and comparing two builds (no compiler involved)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("diff_device_asm", os.path.join(ROOT, "scripts", "diff_device_asm.py"))
dda = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dda)


def _kernel(name, body):
    code = "\n".join(f"\t{ins}" for ins in body)
    return f"""\t.protected\t{name}
\t.globl\t{name}
\t.type\t{name},@function
{name}: ; @{name}
{code}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {len(body)}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end_{name}:
\t.size\t{name}, .Lfunc_end_{name}-{name}
\t.set {name}.num_vgpr, {len(body)}
"""


def _asm(kernels, cuid="0123456789abcdef"):
    head = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.text\n'
    tail = f"""\t.type\t__hip_cuid_{cuid},@object
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.size\t__hip_cuid_{cuid}, 1
\t.amdgpu_metadata
---
amdhsa.kernels:
{"".join(f"  - .name: {n}{chr(10)}" for n in kernels)}...
\t.end_amdgpu_metadata
"""
    return head + "".join(_kernel(n, b) for n, b in kernels.items()) + tail


KA = ["v_add_f32 v0, v1, v2", "v_mul_f32 v0, v0, v3"]
KB = ["v_mov_b32 v0, 0", "global_load_dword v1, v[2:3], off", "s_waitcnt vmcnt(0)"]


def test_split_puts_code_and_descriptor_with_their_kernel():
    pieces = dda.split_kernels(_asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB}))
    assert set(pieces) == {"_Z2k1Pf", "_Z2k2Pf", dda.OUTSIDE}
    k1 = "\n".join(pieces["_Z2k1Pf"])
    assert "v_add_f32 v0, v1, v2" in k1 and ".amdhsa_next_free_vgpr 2" in k1 and "s_endpgm" in k1
    assert "v_mov_b32" not in k1 and "global_load_dword" in "\n".join(pieces["_Z2k2Pf"])
    outside = "\n".join(pieces[dda.OUTSIDE])
    assert ".amdgpu_metadata" in outside and "v_add_f32" not in outside and "amdhsa_next_free_vgpr" not in outside


def test_identical_input():
    text = _asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB})
    ok, report = dda.compare(text, text)
    assert ok
    assert sum(line.startswith("identical") for line in report) == 3  # two kernels and the rest of the file


def test_one_changed_instruction_is_reported_for_its_kernel_only():
    a = _asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB})
    b = _asm({"_Z2k1Pf": KA, "_Z2k2Pf": [KB[0], "global_load_dwordx2 v[4:5], v[2:3], off", KB[2]]})
    ok, report = dda.compare(a, b)
    assert not ok
    assert any(line.startswith("identical") and "_Z2k1Pf" in line for line in report)
    assert any(line.startswith("DIFFERENT") and "_Z2k2Pf" in line for line in report)
    assert any("A| " in line and "global_load_dword v1" in line for line in report)
    assert any("B| " in line and "global_load_dwordx2" in line for line in report)


def test_missing_kernel():
    a = _asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB})
    b = _asm({"_Z2k1Pf": KA})
    ok, report = dda.compare(a, b)
    assert not ok and any(line.startswith("MISSING in B") and "_Z2k2Pf" in line for line in report)
    ok, report = dda.compare(b, a)
    assert not ok and any(line.startswith("MISSING in A") and "_Z2k2Pf" in line for line in report)


def test_kernels_moved_to_a_second_file_compare_against_the_union():
    """``a.hip=b1.hip+b2.hip``: a kernel of A's one file that B defines in its second file is identical; a kernel
    that both of B's files define is an error."""
    import pytest
    assert dda.parse_spec("a.hip") == (["a.hip"], ["a.hip"])
    assert dda.parse_spec("a.hip=b1.hip+b2.hip") == (["a.hip"], ["b1.hip", "b2.hip"])
    a = _asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB})
    b1, b2 = _asm({"_Z2k1Pf": KA}, cuid="1111111111111111"), _asm({"_Z2k2Pf": KB}, cuid="2222222222222222")
    ok, report = dda.compare([a], [b1, b2])
    assert ok, report
    assert sorted(line.split()[1] for line in report if line.startswith("identical")) == ["_Z2k1Pf", "_Z2k2Pf"]
    assert not any(dda.OUTSIDE in line for line in report)  # one file against two: kernels only
    # ... which includes a kernel's register figures, written behind its .size
    assert any(".num_vgpr, 3" in line for line in dda.split_kernels(b2)["_Z2k2Pf"])
    ok, report = dda.compare([a], [b1, b2.replace("_Z2k2Pf.num_vgpr, 3", "_Z2k2Pf.num_vgpr, 4")])
    assert not ok and any(line.startswith("DIFFERENT") and "_Z2k2Pf" in line for line in report)
    # a changed instruction in the moved kernel is still found, and a kernel left behind in neither file is missing
    b2x = _asm({"_Z2k2Pf": [KB[0], "global_load_dwordx2 v[4:5], v[2:3], off", KB[2]]})
    ok, report = dda.compare([a], [b1, b2x])
    assert not ok and any(line.startswith("DIFFERENT") and "_Z2k2Pf" in line for line in report)
    ok, report = dda.compare([a], [b1, _asm({})])
    assert not ok and any(line.startswith("MISSING in B") and "_Z2k2Pf" in line for line in report)
    with pytest.raises(ValueError, match="_Z2k1Pf"):
        dda.compare([a], [b1, _asm({"_Z2k1Pf": KA, "_Z2k2Pf": KB})])


def test_differing_hip_cuid_is_ignored():
    kernels = {"_Z2k1Pf": KA, "_Z2k2Pf": KB}
    ok, report = dda.compare(_asm(kernels, cuid="0123456789abcdef"), _asm(kernels, cuid="fedcba9876543210"))
    assert ok, report
