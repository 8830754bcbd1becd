"""tools/phase_isa.py --blocks on a few lines of made-up assembly: one phase is cut at its labels, the text in front of the first label counts
under "(entry)", and LDS reads and expanded divisions have columns of their own."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("phase_isa", os.path.join(ROOT, "tools", "phase_isa.py"))
phase_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(phase_isa)

ASM = """
_Zkern_d10:                             ; @_Zkern_d10
	s_memtime s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:32
	v_mov_b32_e32 v9, 1
	ds_read_b64 v[2:3], v0
.LBB0_7:                                ; %a.block
	ds_read_b128 v[4:7], v0 offset:16
	ds_read2_b64 v[8:11], v0 offset0:4 offset1:5
	v_cmp_le_f64_e32 vcc, v[2:3], v[4:5]
	v_cndmask_b32_e64 v1, 0, 1, vcc
	v_div_scale_f64 v[12:13], vcc, v[4:5], v[6:7], v[4:5]
	v_rcp_f64_e32 v[14:15], v[12:13]
	v_fma_f64 v[14:15], v[14:15], v[12:13], v[14:15]
	v_div_fmas_f64 v[14:15], v[14:15], v[12:13], v[14:15]
	v_div_fixup_f64 v[14:15], v[14:15], v[6:7], v[4:5]
	s_cbranch_execz .LBB0_9
.LBB0_9:
	v_add_f64 v[4:5], v[4:5], v[6:7]
	s_memtime s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:40
	v_mov_b32_e32 v0, 0
	s_memtime s[2:3]
	global_store_dwordx2 v0, v[2:3], s[4:5] offset:48
	s_endpgm
.Lfunc_end0:
"""


def test_one_phase_cut_at_its_labels():
    rows = phase_isa.block_table(ASM, "_Zkern", 4, 5)
    assert [r["label"] for r in rows] == ["(entry)", ".LBB0_7", ".LBB0_9"]
    entry, a, b = rows
    assert (entry["valu"], entry["mov"], entry["lds_read"], entry["div"]) == (1, 1, 1, 0)
    assert (a["valu"], a["select"], a["fp64"], a["lds_read"], a["div"]) == (7, 1, 1, 2, 1)
    assert (b["valu"], b["fp64"], b["lds_read"]) == (1, 1, 0)
    # the blocks add up to the phase's row of the plain table
    whole = phase_isa.phase_table(ASM, "_Zkern")["phases"][0]
    assert (whole["from"], whole["to"]) == (4, 5)
    for c in phase_isa.COLUMNS:
        assert sum(r[c] for r in rows) == whole[c], c


def test_a_phase_that_is_not_there_is_an_error():
    try:
        phase_isa.block_table(ASM, "_Zkern", 4, 6)
    except ValueError:
        pass
    else:
        raise AssertionError("a missing phase must be an error")
    assert [r["label"] for r in phase_isa.block_table(ASM, "_Zkern", 5, 6)] == ["(entry)"]


def test_render_blocks_ends_with_the_phase_total():
    out = phase_isa.render_blocks(phase_isa.block_table(ASM, "_Zkern", 4, 5)).splitlines()
    assert out[0].split() == ["block"] + list(phase_isa.BLOCK_COLUMNS)
    assert out[-1].split()[0] == "phase" and int(out[-1].split()[1]) == 9
