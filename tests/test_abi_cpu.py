"""CPU-only checks of the C-ABI library: it loads, exports every symbol include/smcmi.h declares, and refuses to compute
without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libmod():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "smc.jl_amd", "csrc", "libsmcmi.so")):
        ge.build()
    from smc_jl_amd.host import _lib

    return _lib


def test_every_declared_symbol_is_exported(libmod):
    hdr = open(os.path.join(ROOT, "include", "smcmi.h")).read()
    declared = set(re.findall(r"\b(smcmi_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"smcmi_handle"}
    L = libmod.lib()
    missing = [n for n in sorted(declared) if not hasattr(L, n)]
    assert not missing, missing
    bound = {n for n, _, _ in libmod.SYMBOLS}
    assert declared <= bound, sorted(declared - bound)      # the Python binding covers the whole header


def test_no_cpu_fallback(libmod):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = libmod.lib()
    cfg = libmod.Config(100, 100, 0, 3, 0, 1, 10, 0)
    h = C.c_void_p()
    rc = L.smcmi_create(C.byref(cfg), C.byref(h))
    assert rc == -2                                           # SMCMI_ERR_HIP
    assert b"no CPU fallback" in L.smcmi_last_error()


def test_product_does_not_import_oracle():
    """The shipped package must never route through oracle/ (test infrastructure)."""
    pkg = os.path.join(ROOT, "smc.jl_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".jl")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.replace("oracle-backed", "").replace("the oracle", "").replace("oracle's", "").replace("oracle (", ""), os.path.join(dp, f)


def test_mutation_kernel_keeps_three_waves_per_simd(libmod):
    """k_mutate_reg<10, α=1> (the kernel `roofline` is quoted on) sits two registers below an occupancy step: at 170 VGPRs only two
    wavefronts fit a SIMD and the kernel loses a quarter of its speed at N >= 1e6 (VALU-issue bound there).  The build keeps
    the compiler's resource report next to the library (csrc/Makefile); a change that pushes the kernel over the step, or into
    scratch, fails here instead of in a benchmark three rounds later."""
    rep = os.path.join(ROOT, "smc.jl_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(rep):
        pytest.skip("library was built without the resource report")
    txt = open(rep).read()
    # (round 4: four wavefronts per SIMD since the main translation unit is compiled without machine LICM - 127 / 128 VGPRs, one below
    # the step; the segment kernels without a spilled VGPR since they are, Makefile MAINFLAGS / SEGFLAGS)
    # (<n_para 10, α = 1?, riding?>: the two-hand-over variants - the headline's - and the riding α = 1 variant without a spilled VGPR; the riding
    # mixture variant may keep a couple)
    # (<n_para 10, α = 1?, riding?, chunks per worker, several handles?>; round 6: the two-chunk variants carry the call of their in-place
    # selection - k3_select_two - and with it 32 spilled VGPRs outside the per-particle phases: 48.0-48.7 µs per stage as before)
    for key, max_spill, max_scratch in (("k3_segmentILi10ELb1ELb0ELi1ELb0E", 0, 64), ("k3_segmentILi10ELb0ELb0ELi1ELb0E", 0, 64), ("k3_segmentILi10ELb1ELb1ELi1ELb0E", 0, 64),
                                        ("k3_segmentILi10ELb0ELb1ELi1ELb0E", 4, 96), ("k3_segmentILi10ELb1ELb0ELi1ELb1E", 0, 64), ("k3_segmentILi10ELb1ELb1ELi1ELb1E", 0, 64),
                                        ("k3_segmentILi10ELb1ELb0ELi2ELb0E", 32, 192), ("k3_segmentILi10ELb1ELb1ELi2ELb0E", 32, 192)):
        m = re.search(r"Function Name: _ZN5smcmi\d+" + key + r"[^\n]*\n(?:[^\n]*\n){0,12}?[^\n]*VGPRs Spill: (\d+)", txt)
        assert m, key
        assert int(m.group(1)) <= max_spill, (key, m.group(1))
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", txt[m.start():m.end()]).group(1)) <= max_scratch, key
    for key, min_occ, max_scratch in (("k_mutate_regILi10ELb1E", 4, 64), ("k_mutate_regILi9ELb1E", 4, 64)):
        m = re.search(r"Function Name: _ZN5smcmi\d+" + key + r"[^\n]*\n(?:[^\n]*\n){0,12}?[^\n]*Occupancy \[waves/SIMD\]: (\d+)", txt)
        assert m, key
        blk = txt[m.start():m.end()]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        assert int(m.group(1)) >= min_occ, (key, m.group(1))
        assert scratch <= max_scratch, (key, scratch)


def test_dpp_operands_of_the_kalman_filters_respect_the_hazard_rule(libmod):
    """The Kalman filters read their wave-uniform structure values through the DPP operand of `v_fmac_f64_dpp ... row_newbcast` written
    as inline assembly (csrc/model.hpp): the compiler does not know that operand is a DPP source, so it inserts none of the two wait
    states gfx9 needs between a VALU write of a VGPR and a DPP read of it.  The registers are loaded once, far in front of the loops -
    unless a later compiler reloads or copies one right before a use.  The build keeps the device assembly of the main translation
    unit (csrc/Makefile); this walks it: no VALU instruction within two wait states in front of such an FMA may write its DPP source,
    and the filters' kernels must not have fallen back to scratch."""
    asm = os.path.join(ROOT, "smc.jl_amd", "csrc", "build", "smcmi_device.s")
    if not os.path.exists(asm):
        pytest.skip("library was built without keeping the device assembly")

    def regs(tok):
        m = re.match(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return {int(m.group(1))} if m else set()

    code = []
    for ln in open(asm):
        t = ln.strip()
        if t and not t.startswith((";", ".")) and not t.endswith(":") and not re.match(r"^[._A-Za-z0-9$]+:", t):
            code.append(t)
    total, bad = 0, []
    for n, t in enumerate(code):
        if not t.startswith("v_fmac_f64_dpp"):
            continue
        total += 1
        src = regs(t.split()[2].strip(","))
        ws, k = 0, n - 1
        while k >= 0 and ws < 2:
            p = code[k]
            op = p.split()[0]
            if op == "s_nop":
                ws += int(p.split()[1]) + 1
            else:
                if op.startswith("v_") and len(p.split()) > 1 and regs(p.split()[1].strip(",")) & src:
                    bad.append((p, t))
                ws += 1
            k -= 1
    assert total > 1000, total              # the three places the filters are compiled into
    assert not bad, bad[:3]


def test_header_is_plain_c_and_the_c_example_links(libmod, tmp_path):
    """include/smcmi.h is C99 (-pedantic), and examples/c_abi_config2.c - the boundary used from plain C, no Python / torch -
    compiles and links against libsmcmi.so."""
    import subprocess

    t = tmp_path / "t.c"
    t.write_text('#include "smcmi.h"\nint main(void) { return (int)sizeof(smcmi_run_config) == 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(t)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "c_abi_config2"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_config2.c"), "-L", os.path.join(ROOT, "smc.jl_amd", "csrc"), "-lsmcmi", "-lm",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_routing_table_is_the_one_the_hand_written_predicates_gave(tmp_path):
    """csrc/route.hpp decides where a run goes (driver, engine 2's geometry, Kalman lanes, segment shape).  tests/route_check.hip prints
    its table for every boundary of the geometry under six switch sets - host code, no device - and the table must equal the one
    recorded from the predicates route.hpp replaced (tests/golden/routing_table.txt)."""
    import subprocess

    exe = tmp_path / "route_check"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17",
                        os.path.join(ROOT, "tests", "route_check.hip"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "routing_table.txt")).read().splitlines()
    assert len(want) > 1500
    diff = [(a, b) for a, b in zip(want, got) if a != b]
    assert not diff, "%d of %d lines differ, the first:\n%s\n%s" % (len(diff), len(want), diff[0][0], diff[0][1])
    assert len(got) == len(want), (len(got), len(want))


def test_switches_hpp_is_the_only_reader_of_the_environment_and_matches_the_design_table():
    """DESIGN §7b lists the development switches; csrc/switches.hpp reads exactly those names and nothing else under csrc/ reads the
    environment for one."""
    csrc = os.path.join(ROOT, "smc.jl_amd", "csrc")
    read = set(re.findall(r'\("(SMCMI_[A-Z0-9_]+)"', open(os.path.join(csrc, "switches.hpp")).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 7b\. (.*?)\n(.*?)^## ", design, re.S | re.M)
    assert m, "DESIGN.md has no section 7b"
    count = re.search(r"(\d+) names", m.group(1))
    rows = [ln for ln in m.group(2).splitlines() if ln.startswith("| `SMCMI_")]
    listed = set(re.findall(r"SMCMI_[A-Z0-9_]+", "\n".join(ln.split("|")[1] for ln in rows)))
    assert read == listed, (sorted(read - listed), sorted(listed - read))
    assert count and int(count.group(1)) == len(listed), (count and count.group(1), len(listed))
    others = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hpp", ".hip")) and f != "switches.hpp" and re.search(r'getenv\s*\(\s*"SMCMI_', open(os.path.join(csrc, f)).read()):
            others.append(f)
    assert not others, others


def test_devmem_hpp_is_the_only_caller_of_the_allocators():
    """csrc/devmem.hpp owns every device and pinned allocation: the runtime's five allocator and free calls occur there and nowhere else
    under csrc/ (a buffer allocated beside the owner is one nothing gives back on an error path).  So do the event constructors; the stall
    rules' state occurs in csrc/stagepolicy.hpp alone; and no call of enqueue_stage passes a bare true / false."""
    csrc = os.path.join(ROOT, "smc.jl_amd", "csrc")
    calls = ("hipMalloc", "hipExtMallocWithFlags", "hipHostMalloc", "hipFree", "hipHostFree")
    pat = re.compile(r"\b(%s)\b" % "|".join(calls))
    found = {f: set(pat.findall(open(os.path.join(csrc, f)).read())) for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip"))}
    assert found.pop("devmem.hpp") == set(calls)
    others = {f: sorted(v) for f, v in found.items() if v}
    assert not others, others
    assert len(found) > 20, sorted(found)
    # likewise the events (devmem.hpp Handles destroys what it made on every return), and the stall rules live in stagepolicy.hpp alone
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip"))}
    assert [f for f, t in src.items() if "hipEventCreate" in t] == ["devmem.hpp"]
    for word in ("spec_strikes", "last_solver_stall"):
        assert [f for f, t in src.items() if word in t] == ["stagepolicy.hpp"], word
    # ... and a stage is requested by named fields: no call of enqueue_stage carries a bare true / false
    calls = [m.group(0) for t in src.values() for m in re.finditer(r"\benqueue_stage\s*\(([^;{]*)\)\s*;", t)]
    assert len(calls) >= 4, calls
    bare = [c for c in calls if any(a.strip() in ("true", "false") for a in re.split(r"[(),]", c))]
    assert not bare, bare


def test_the_owner_gives_everything_back_under_fault_injection(tmp_path):
    """tests/devmem_check.hip drives csrc/devmem.hpp's Owner on a counting allocator that fails on its k-th call, for every k of three scripted
    sequences (one shaped like smcmi_create, a regrow that fails after the release, a scoped temporary with an early return) - host code
    under AddressSanitizer and UBSan, no device: exit status 0 and nothing on stderr."""
    import subprocess

    exe = tmp_path / "devmem_check"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17",
                        "-Xarch_host", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "devmem_check.hip"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr


def test_stage_policy_states_the_rules_the_drivers_had(tmp_path):
    """tests/policy_check.cpp drives csrc/stagepolicy.hpp - the resample forecast, the stall book, the stages-left estimate and batch bound the
    host drivers share - with plain numbers against the rules as the drivers' own copies stated them; host code under AddressSanitizer and
    UBSan, no HIP: exit status 0 and nothing on stderr."""
    import subprocess

    exe = tmp_path / "policy_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "policy_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def _lds_check(tmp_path):
    """tests/lds_check.cpp built with AddressSanitizer and UBSan and run: its standard output."""
    import subprocess

    exe = tmp_path / "lds_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "lds_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok" and r.stderr == "", r.stdout + r.stderr
    return r.stdout


def test_lds_layouts_state_the_sizes_the_launch_sites_had(tmp_path):
    """tests/lds_check.cpp holds csrc/ldslayout.hpp - the one description of every stage kernel's dynamic LDS - against the size formulas the
    launch sites stated by hand before (every total equal, at every n_para the layout is built for), checks every member's alignment, that no
    two live members overlap and that all end inside the total, and the equivalences between the layouts; host code under AddressSanitizer
    and UBSan, no HIP: exit status 0, "ok", nothing on stderr."""
    _lds_check(tmp_path)


def test_segment_kernels_fit_a_cu_with_the_static_lds_the_compiler_reports(tmp_path):
    """Every k3_segment instantiation in the compiler's resource report: its static LDS plus the largest dynamic size launch_k3_seg asks for
    (whole KB, as the kernel is opted in; printed by tests/lds_check.cpp from the layouts) fits a CU's 160 KB, and a mixture kernel's static
    LDS is within what k3_sel_cols takes it to be when it decides whether the particle in transit stays in LDS: its z columns and dense
    mixture block (counted by the rule itself) and 24 KB for all the rest."""
    rep = os.path.join(ROOT, "smc.jl_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(rep):
        pytest.skip("library was built without the resource report")
    dyn = {}
    for m in re.finditer(r"^k3_segment D=(\d+) alpha1=(\d) chunks=(\d) max_dynamic=(\d+) assumed_static=(\d+)$", _lds_check(tmp_path), re.M):
        dyn[tuple(int(x) for x in m.group(1, 2, 3))] = (int(m.group(4)), int(m.group(5)))
    assert len(dyn) == 30, sorted(dyn)
    txt = open(rep).read()
    seen = set()
    for m in re.finditer(r"Function Name: _ZN5smcmi\d+k3_segmentILi(\d+)ELb([01])ELb([01])ELi(\d)ELb([01])E[^\n]*\n(?:[^\n]*\n){0,14}?[^\n]*LDS Size \[bytes/block\]: (\d+)", txt):
        d, a1, ride, ch, sys_, static = (int(x) for x in m.groups())
        max_dynamic, assumed_static = dyn[(d, a1, ch)]
        print(f"k3_segment<{d}, {a1}, {ride}, {ch}, {sys_}>: static {static} + dynamic {max_dynamic} = {static + max_dynamic}")
        assert static + max_dynamic <= 160 * 1024, (d, a1, ride, ch, sys_, static, max_dynamic)
        if not a1:
            assert static <= assumed_static, (d, a1, ride, ch, sys_, static, assumed_static)
        seen.add((d, a1, ride, ch, sys_))
    assert len(seen) == 100, len(seen)                        # 10 n_para x (4 one-handle + 4 several-handle + 2 two-chunk) instantiations
