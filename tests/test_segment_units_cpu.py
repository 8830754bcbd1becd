"""The compiler's resource report (csrc/resource_usage.txt, kept next to the library by csrc/Makefile) for the two units of the α = 1,
two-hand-over, one-handle, one-chunk segment kernel: the default-run unit (smcmi::defrun::k3_segment, csrc/stage3.hpp SMCMI_K3_RUN) exists to
hold fewer registers across the stage loop than the general unit of the same build - a relation within one build, for every n_para built."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIELDS = {"vgprs": r"    VGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "sgpr_spill": r"SGPRs Spill: (\d+)", "vgpr_spill": r"VGPRs Spill: (\d+)"}


def _kernels(txt, prefix):
    """{n_para: {field: value}} of the kernels whose mangled name is `prefix` + k3_segment<n_para, true, false, 1, false>"""
    out = {}
    for m in re.finditer(r"Function Name: " + prefix + r"10k3_segmentILi(\d+)ELb1ELb0ELi1ELb0EE[^\n]*\n((?:[^\n]*\n){0,14}?[^\n]*LDS Size[^\n]*)", txt):
        out[int(m.group(1))] = {k: int(re.search(p, m.group(2)).group(1)) for k, p in _FIELDS.items()}
    return out


def test_the_default_run_unit_holds_fewer_registers_than_the_general_unit():
    rep = os.path.join(ROOT, "smc.jl_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(rep):
        pytest.skip("library was built without the resource report")
    txt = open(rep).read()
    run, general = _kernels(txt, "_ZN5smcmi6defrun"), _kernels(txt, "_ZN5smcmi")
    assert sorted(run) == sorted(general) == list(range(1, 11)), (sorted(run), sorted(general))
    for d in sorted(run):
        r, g = run[d], general[d]
        print("n_para %2d  default-run %s   general %s" % (d, r, g))
        assert r["vgpr_spill"] == 0 and r["scratch"] <= 64, (d, r)
        assert r["vgprs"] < g["vgprs"], (d, r["vgprs"], g["vgprs"])
        assert r["sgpr_spill"] < g["sgpr_spill"], (d, r["sgpr_spill"], g["sgpr_spill"])
