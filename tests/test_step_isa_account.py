"""scripts/step_isa_account.py: cutting a kernel at its barriers, prefix classes and path walks (no compiler involved)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_isa_account", os.path.join(ROOT, "scripts", "step_isa_account.py"))
sia = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sia)

NAME = "_Z4stepPf"
# segment 0: a wave-uniform branch (wave 0 runs the "head", the others the "M" block); segment 1: an exec-masked region
BODY = """\
\tv_and_b32_e32 v1, 15, v0
\ts_cmp_lg_u32 s2, 0
\ts_cbranch_scc1 .LBB3_2
; %bb.1: ; head
\tv_exp_f32_e32 v2, v1
\tv_log_f32_e32 v2, v2
\tds_write_b32 v1, v2
\ts_branch .LBB3_3
.LBB3_2: ; M
\tds_read_b64 v[4:5], v1
\tv_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], 0
.LBB3_3:
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\tv_cmp_gt_u32_e32 vcc, 4, v0
\ts_and_saveexec_b64 s[4:5], vcc
\ts_cbranch_execz .LBB3_5
; %bb.4:
\tv_mul_f32_e32 v3, v2, v2
\tglobal_store_dword v1, v3, s[0:1]
\tbuffer_store_dword v3, v1, s[8:11], 0 offen
.LBB3_5:
\ts_or_b64 exec, exec, s[4:5]
\ts_endpgm
"""


def _asm():
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.text
\t.globl\t{NAME}
\t.type\t{NAME},@function
{NAME}: ; @{NAME}
{BODY}\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {NAME}
\t\t.amdhsa_next_free_vgpr 12
\t.end_amdhsa_kernel
\t.text
.Lfunc_end3:
\t.size\t{NAME}, .Lfunc_end3-{NAME}
\t.set {NAME}.num_vgpr, 12
"""


def _segments():
    pieces = sia.dda.split_kernels(_asm())
    return sia.split_segments(sia.parse_body(pieces[sia.find_kernel(pieces, "stepPf")]))


def test_classes_come_from_the_prefix():
    assert sia.classify("v_mfma_f32_16x16x32_bf16") == "mfma"
    assert sia.classify("v_cvt_pk_bf16_f32") == "valu"
    assert sia.classify("ds_read_b128") == "lds"
    assert sia.classify("buffer_load_dwordx4") == "vmem" and sia.classify("global_load_dword") == "vmem"
    assert sia.classify("s_waitcnt") == "salu" and sia.classify("s_anything_at_all") == "salu"
    assert sia.classify("flat_load_dword") == "other"


def test_body_is_cut_behind_each_barrier_and_counted_by_class():
    segs = _segments()
    assert len(segs) == 2
    c0, c1 = sia.count(segs[0]), sia.count(segs[1])
    assert c0 == {"mfma": 1, "valu": 3, "lds": 2, "vmem": 0, "salu": 5, "other": 0}
    assert c1 == {"mfma": 0, "valu": 2, "lds": 0, "vmem": 2, "salu": 4, "other": 0}
    # the descriptor and the directives behind the code are not instructions
    assert sum(sum(c.values()) for c in (c0, c1)) == sum(
        1 for line in BODY.splitlines() if line.startswith("\t"))


def test_paths_follow_the_decisions():
    seg0, seg1 = _segments()
    head, trace = sia.walk(seg0, "n")
    assert head == {"mfma": 0, "valu": 3, "lds": 1, "vmem": 0, "salu": 5, "other": 0}
    assert len(trace) == 1 and "s_cbranch_scc1" in trace[0] and " n " in trace[0]
    m_wave, _ = sia.walk(seg0, "t")
    assert m_wave == {"mfma": 1, "valu": 1, "lds": 1, "vmem": 0, "salu": 4, "other": 0}
    assert sia.walk(seg0, "")[0] == head  # decisions used up: fall through
    active, _ = sia.walk(seg1, "n")
    skipped, _ = sia.walk(seg1, "t")
    assert active["vmem"] == 2 and active["valu"] == 2
    assert skipped["vmem"] == 0 and skipped["valu"] == 1 and skipped["salu"] == 4
    with pytest.raises(ValueError):
        sia.walk(seg0, "x")


def test_report_and_kernel_choice():
    lines = sia.account(_asm(), "stepPf", ["head=0:n", "M=0:t"], trace=True)
    text = "\n".join(lines)
    assert f"kernel {NAME}" in text and "2 segments" in text
    assert any(line.strip().startswith("seg 0 head") for line in lines)
    assert any(line.strip().startswith("seg 0 M") for line in lines)
    with pytest.raises(ValueError):
        sia.find_kernel(sia.dda.split_kernels(_asm()), "no_such_kernel")
