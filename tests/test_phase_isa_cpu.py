"""tools/phase_isa.py on a few lines of made-up assembly: the kernel is found by its name, its text is cut at the shader-clock reads, the
slot comes from the store behind the read, and every instruction lands in the columns its mnemonic says."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("phase_isa", os.path.join(ROOT, "tools", "phase_isa.py"))
phase_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(phase_isa)

ASM = """
	.text
_Zother:                                ; @_Zother
	s_memtime s[0:1]
	v_mov_b32_e32 v0, 0
	s_endpgm
.Lfunc_end0:
_Zkern_d10:                             ; @_Zkern_d10
; %bb.0:
	v_writelane_b32 v40, s4, 0
	v_writelane_b32 v41, s5, 1
	v_mov_b32_e32 v9, 1                     ; in front of the first stamp: counted nowhere
	s_memtime s[2:3]
	s_waitcnt lgkmcnt(0)
	v_mov_b64_e32 v[2:3], s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:8
.LBB1_2:
	v_add_f64 v[4:5], v[4:5], v[6:7]
	v_mul_f64 v[4:5], v[4:5], v[4:5]
	v_fma_f64 v[4:5], v[4:5], v[6:7], v[8:9]
	v_cndmask_b32_e64 v1, 0, v4, s[6:7]
	v_readlane_b32 s6, v40, 0
	v_readlane_b32 s7, v10, 3
	s_nop 1
	v_mov_b32_dpp v1, v2 row_shr:1 row_mask:0xf bank_mask:0xf
	v_add_f64 v[4:5], v[4:5], v[6:7] row_shr:2 row_mask:0xf bank_mask:0xf
	s_and_b64 exec, exec, s[6:7]
	ds_read_b64 v[2:3], v0
	s_memtime s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:16
	v_permlane32_swap_b32_e32 v1, v2
	v_accvgpr_write_b32 a0, v1
	s_memtime s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:32
	v_mov_b32_e32 v0, 0
	s_endpgm
.Lfunc_end1:
"""


def test_kernel_is_found_by_prefix_and_ends_at_its_end_marker():
    lines = phase_isa.kernel_text(ASM, "_Zkern")
    assert any("v_writelane_b32 v40" in ln for ln in lines) and not any("_Zother" in ln for ln in lines)
    assert lines[-1].strip() == "s_endpgm"
    try:
        phase_isa.kernel_text(ASM, "_Znone")
    except ValueError:
        pass
    else:
        raise AssertionError("a missing kernel must be an error")


def test_stamps_and_their_slots():
    lines = phase_isa.kernel_text(ASM, "_Zkern")
    assert [s for _, s in phase_isa.stamps(lines)] == [1, 2, 4]
    assert phase_isa.spill_vgprs(lines) == {"v40", "v41"}


def test_counts_between_stamps():
    tab = phase_isa.phase_table(ASM, "_Zkern")
    assert tab["spill_vgprs"] == ["v40", "v41"]
    a, b = tab["phases"]
    assert (a["from"], a["to"], b["from"], b["to"]) == (1, 2, 2, 4)
    # 1 -> 2: the v_mov_b64 behind the clock read, 3 FP64, the select, 2 lane reads, the DPP move, the DPP add = 9 vector instructions
    assert a == {"from": 1, "to": 2, "valu": 9, "select": 1, "mov": 1, "xlane": 4, "reload": 1, "s_nop": 1, "fp64": 4}
    assert b == {"from": 2, "to": 4, "valu": 2, "select": 0, "mov": 1, "xlane": 1, "reload": 0, "s_nop": 0, "fp64": 0}
    assert tab["loop"] == {c: a[c] + b[c] for c in phase_isa.COLUMNS}


def test_render_has_one_line_per_phase():
    out = phase_isa.render(phase_isa.phase_table(ASM, "_Zkern")).splitlines()
    assert out[0].split() == ["stamps"] + list(phase_isa.COLUMNS)
    assert out[1].split()[0] == "1->2" and out[2].split()[0] == "2->4" and out[3].split()[0] == "first->last"
    assert out[4] == "spill VGPRs: v40 v41"
