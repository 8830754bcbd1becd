"""CPU-only checks of likelihoods compiled from HIP source FOR ENSEMBLES (smcmi_program_compile_ensemble): the run-time compiler
cross-compiles for gfx950 without a device, so what the code object holds, the n_para range, the compiler log's line numbers, the option
refusals, the header isolation and the ensemble kernel's registers are checked here - and, as a stand-alone program under
AddressSanitizer / UBSan, the pure text functions of csrc/enssrc.hpp."""
import ctypes as C
import os
import subprocess
import tempfile
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smc.jl_amd", "csrc")
ERR_ARG, ERR_COMPILE = -1, -11

GAUSS_SRC = """__device__ double loglik(const double *theta, long long ld, int d, const double *data, long long rows, long long cols,
                         const double *par, long long n_par) {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const double e = theta[k * ld] - data[k];
        acc += e * e;
    }
    return par[0] - acc / par[1];
}
"""


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(CSRC, "libsmcmi.so")):
        ge.build()
    from smc_jl_amd.host import _lib

    lib = _lib.lib()
    opened = None
    for name in ("libhiprtc.so", "libhiprtc.so.7"):
        try:
            opened = C.CDLL(name)
            break
        except OSError:
            pass
    if opened is None:
        pytest.skip("the run-time compiler (libhiprtc) cannot be opened on this machine")
    return lib


def _compile(L, source, n_para=3, entry=None, options=None):
    p = C.c_void_p()
    enc = lambda s: None if s is None else s.encode()
    rc = L.smcmi_program_compile_ensemble(enc(source), enc(entry), enc(options), n_para, C.byref(p))
    return rc, p


def _code(L, p):
    ptr, size = C.c_void_p(), C.c_int64()
    assert L.smcmi_program_code(p, C.byref(ptr), C.byref(size)) == 0
    return C.string_at(ptr, size.value)


def _para(L, p):
    v = C.c_int32(-1)
    assert L.smcmi_program_ensemble_para(p, C.byref(v)) == 0
    return v.value


def kernel_notes(code, name):
    """registers, scratch and LDS of kernel `name` from the code object's notes (llvm-readelf --notes), as tools/program_bench.py reads them"""
    tool = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    assert os.path.exists(tool), tool
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        txt = subprocess.run([tool, "--notes", f.name], capture_output=True, text=True).stdout
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:                 # (one block per kernel; .agpr_count is its first key)
        blk = ".agpr_count:" + blk
        vals = {}
        for ln in blk.splitlines():
            ln = ln.strip().lstrip("- ")
            if ln.startswith(".") and ":" in ln:
                k, v = ln.split(":", 1)
                vals.setdefault(k.strip(), v.strip())
        if vals.get(".name") == name:
            for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
                      ".group_segment_fixed_size"):
                out[k[1:]] = int(vals[k]) if k in vals else None
    return out


@pytest.fixture(scope="module")
def compiled(L):
    """GAUSS_SRC compiled for n_para 1, 3 and 10: {n_para: (program, seconds)}"""
    out = {}
    for d in (1, 3, 10):
        t0 = time.perf_counter()
        rc, p = _compile(L, GAUSS_SRC, n_para=d)
        dt = time.perf_counter() - t0
        assert rc == 0, (d, L.smcmi_last_error(), L.smcmi_program_log(p) if p else None)
        out[d] = (p, dt)
    yield out
    for p, _ in out.values():
        L.smcmi_program_destroy(p)


def test_an_ensemble_code_object_holds_both_kernels_and_a_plain_one_only_the_wrapper(L, compiled):
    for d, (p, dt) in compiled.items():
        code = _code(L, p)
        print("n_para %d: compile time %.3f s, code object %d bytes" % (d, dt, len(code)))
        assert code[:4] == b"\x7fELF"
        assert b"smcmi_program_kernel" in code and b"smcmi_program_ensemble" in code and b"smcmi_program_ens_abi" in code
        assert b"smcmi_program_mutate" not in code
        assert _para(L, p) == d
        assert L.smcmi_program_log(p) == b""
        v = C.c_int32(-1)
        assert L.smcmi_program_is_fused(p, C.byref(v)) == 0 and v.value == 0
    q = C.c_void_p()
    assert L.smcmi_program_compile(GAUSS_SRC.encode(), None, None, C.byref(q)) == 0
    plain = _code(L, q)
    assert b"smcmi_program_kernel" in plain and b"smcmi_program_ensemble" not in plain
    assert _para(L, q) == 0
    L.smcmi_program_destroy(q)
    assert L.smcmi_program_compile_ex(GAUSS_SRC.encode(), None, None, 1, C.byref(q)) == 0          # a fused program is no ensemble program
    assert _para(L, q) == 0 and b"smcmi_program_ensemble" not in _code(L, q)
    L.smcmi_program_destroy(q)
    assert L.smcmi_program_ensemble_para(None, None) == ERR_ARG


@pytest.mark.parametrize("n_para", [0, 11, -1])
def test_n_para_outside_the_kernel_s_range_is_refused(L, n_para):
    rc, p = _compile(L, GAUSS_SRC, n_para=n_para)
    assert rc == ERR_ARG and not p.value
    assert b"n_para" in L.smcmi_last_error()


@pytest.mark.parametrize("flags", [2, 3])
def test_compile_ex_keeps_refusing_other_flag_bits(L, flags):
    p = C.c_void_p()
    assert L.smcmi_program_compile_ex(GAUSS_SRC.encode(), None, None, flags, C.byref(p)) == ERR_ARG and not p.value


def test_a_syntax_error_is_reported_at_the_users_line(L):
    src = GAUSS_SRC.splitlines()
    assert "double acc = 0.0;" in src[2]
    src[2] = "    double acc = 0.0 +;"                        # the user's line 3
    for text in ("\n".join(src) + "\n", "\n".join(src)):       # with and without a trailing newline
        rc, p = _compile(L, text)
        assert rc == ERR_COMPILE and p.value
        log = L.smcmi_program_log(p).decode()
        assert "likelihood.hip:3" in log, log
        assert "error" in log
        ptr, sz = C.c_void_p(), C.c_int64()
        assert L.smcmi_program_code(p, C.byref(ptr), C.byref(sz)) == ERR_ARG
        assert L.smcmi_program_destroy(p) == 0


def test_a_source_without_the_entry_function_does_not_compile(L):
    rc, p = _compile(L, GAUSS_SRC.replace("loglik", "something_else"))
    assert rc == ERR_COMPILE and p.value
    assert "loglik" in L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)


def test_the_library_s_own_loglik_does_not_stand_in_for_a_custom_entry(L):
    rc, p = _compile(L, GAUSS_SRC, entry="other_entry")
    assert rc == ERR_COMPILE and "other_entry" in L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)
    rc, p = _compile(L, GAUSS_SRC.replace("loglik", "other_entry"), entry="other_entry")
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)


@pytest.mark.parametrize("options", ["--offload-arch=gfx942", "-mcpu=gfx90a", "--offload-arch=gfx950:xnack+", "-mxnack"])
def test_options_that_name_a_target_are_refused(L, options):
    rc, p = _compile(L, GAUSS_SRC, options=options)
    assert rc == ERR_ARG and not p.value
    assert b"refused" in L.smcmi_last_error()


@pytest.mark.parametrize("options", ["-I/usr/include", "-isystem /usr/include", "-include stdio.h", "--sysroot=/", "-ffp-contract=fast", "-ffast-math",
                                     "-DSMCMI_PROGRAM_ENTRY=f", "-DSMCMI_PROGRAM_ENS=0", "-USMCMI_INST_UNIT", "-DSMCMI_STRICT_FP",
                                     "-DA=1 -idirafter /usr/include"])
def test_options_that_would_reach_the_engine_s_kernel_are_refused(L, options):
    rc, p = _compile(L, GAUSS_SRC, options=options)
    assert rc == ERR_ARG and not p.value
    assert b"refused" in L.smcmi_last_error()


def test_a_define_in_the_options_reaches_the_source(L):
    rc, p = _compile(L, GAUSS_SRC + "\nstatic_assert(NAME == 3.5, \"NAME did not arrive\");\n", options="-DNAME=3.5")
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)


MACHINE_PATHS = ("/usr", "/opt", "/lib", "/bin", "/include/", "gcc", "x86_64")


def test_a_system_header_the_library_does_not_supply_is_file_not_found(L):
    rc, p = _compile(L, "#include <vector>\n" + GAUSS_SRC)
    assert rc == ERR_COMPILE and p.value
    log = L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)
    assert "likelihood.hip:1" in log and "'vector' file not found" in log, log
    assert not [w for w in MACHINE_PATHS if w in log], log


def test_the_ensemble_kernel_keeps_the_proposal_in_registers(L, compiled):
    """smcmi_program_ensemble for GAUSS_SRC at n_para = 10: no scratch memory and no spilled VGPR - the user's loop over k < d unrolled over
    the private proposal.  Its VGPR count and the compile time are printed, not bounded (DESIGN.md 4h has them)."""
    p, dt = compiled[10]
    notes = kernel_notes(_code(L, p), "smcmi_program_ensemble")
    print("smcmi_program_ensemble, n_para = 10: %r; compile time %.3f s" % (notes, dt))
    assert notes, "the code object's notes do not list smcmi_program_ensemble"
    assert notes["private_segment_fixed_size"] == 0
    assert notes["vgpr_spill_count"] in (0, None)
    for d in (1, 3):
        small = kernel_notes(_code(L, compiled[d][0]), "smcmi_program_ensemble")
        print("smcmi_program_ensemble, n_para = %d: %r" % (d, small))
        assert small["private_segment_fixed_size"] == 0 and small["vgpr_spill_count"] in (0, None)


def test_the_python_wrappers_pass_ensemble_para(L):
    import numpy as np

    import smc_jl_amd as S
    from smc_jl_amd.host import _lib

    p = S.Engine.compile_program(GAUSS_SRC, ensemble_para=2)
    assert p.ensemble_para == 2 and p.fused is False
    p.close()
    assert S.Engine.compile_program(GAUSS_SRC).ensemble_para == 0
    with pytest.raises(_lib.SMCMIError) as ei:
        S.Engine.compile_program(GAUSS_SRC, ensemble_para=11)
    assert ei.value.code == ERR_ARG
    with pytest.raises(S.CompileError) as ei:
        S.Engine.compile_program("__device__ double loglik(const double *theta) {\n  return theta[0]\n}\n", ensemble_para=1)
    assert "likelihood.hip:2" in ei.value.log
    lik = S.HIPLikelihood(GAUSS_SRC, par=[0.0, 2.0], ensemble=True)
    assert lik.ensemble is True and S.HIPLikelihood(GAUSS_SRC).ensemble is False
    assert lik.ensemble_program(2).ensemble_para == 2 and lik.ensemble_program(2) is lik.ensemble_program(2)
    # without ensemble=True smc_ensemble still says where a HIPLikelihood runs, before any handle is made
    pars = [S.parameter("a", 0.0, (-5.0, 5.0), prior=S.Normal(0.0, 1.0))]
    with pytest.raises(NotImplementedError, match="HIPLikelihood"):
        S.smc_ensemble(S.HIPLikelihood(GAUSS_SRC, par=[0.0, 2.0]), pars, np.zeros(1), seeds=[1, 2], n_parts=100)


def test_enssrc_on_its_own_under_the_sanitizers(tmp_path):
    """tests/enssrc_check.cpp: the ensemble text's #line arithmetic, the header table against the #include lines of the embedded text, and the
    two embedded ensemble headers against the files - host code, no run-time compiler in that process.  The embedded text is the one the
    library's build left in csrc/build; only where the library came without its build directory are the files made here."""
    incs = ["build/embedded_headers.inc", "build/embedded_ens_headers.inc"]
    if not all(os.path.exists(os.path.join(CSRC, f)) for f in incs):
        subprocess.check_call(["make", "-C", CSRC] + incs, stdout=subprocess.DEVNULL)
    exe = tmp_path / "enssrc_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(CSRC, "build"), os.path.join(ROOT, "tests", "enssrc_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), CSRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    assert "enssrc_check ok" in r.stdout
