"""Likelihoods compiled at run time from HIP source (include/smcmi.h smcmi_program_*), the half that needs no GPU: the compile itself
(the run-time compiler cross-compiles for gfx950 without a device), the compiler log's line numbers, the refusals, and - as a stand-alone
program under AddressSanitizer / UBSan - the pure text functions of csrc/progsrc.hpp."""
import ctypes as C
import os
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ERR_ARG, ERR_COMPILE = -1, -11

GAUSS = """__device__ double loglik(const double *theta, long long ld, int d, const double *data, long long rows, long long cols,
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

    if not os.path.exists(os.path.join(ROOT, "smc.jl_amd", "csrc", "libsmcmi.so")):
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


def _compile(L, source, entry=None, options=None):
    p = C.c_void_p()
    enc = lambda s: None if s is None else s.encode()
    rc = L.smcmi_program_compile(enc(source), enc(entry), enc(options), C.byref(p))
    return rc, p


def _code_size(L, p):
    ptr, size = C.c_void_p(), C.c_int64()
    assert L.smcmi_program_code(p, C.byref(ptr), C.byref(size)) == 0
    assert ptr.value
    return size.value


def test_a_valid_source_compiles_to_a_code_object(L):
    t0 = time.perf_counter()
    rc, p = _compile(L, GAUSS)
    t1 = time.perf_counter()
    print("compile time %.3f s" % (t1 - t0))
    assert rc == 0, (L.smcmi_last_error(), L.smcmi_program_log(p) if p else None)
    assert p.value
    size = _code_size(L, p)
    assert size > 0
    assert L.smcmi_program_log(p) == b""
    ptr, sz = C.c_void_p(), C.c_int64()
    L.smcmi_program_code(p, C.byref(ptr), C.byref(sz))
    assert C.string_at(ptr, 4) == b"\x7fELF"
    # the same text again: a code object of the same size
    rc2, p2 = _compile(L, GAUSS)
    assert rc2 == 0 and _code_size(L, p2) == size
    # a custom entry
    rc3, p3 = _compile(L, GAUSS.replace("loglik", "my_model_7"), entry="my_model_7")
    assert rc3 == 0 and _code_size(L, p3) > 0 and L.smcmi_program_log(p3) == b""
    for q in (p, p2, p3):
        assert L.smcmi_program_destroy(q) == 0
    assert L.smcmi_program_destroy(None) == 0


def test_a_syntax_error_is_reported_at_the_users_line(L):
    src = GAUSS.splitlines()
    assert "double acc = 0.0;" in src[2]
    src[2] = "    double acc = 0.0 +;"                        # the user's line 3
    for text in ("\n".join(src) + "\n", "\n".join(src)):       # with and without a trailing newline
        rc, p = _compile(L, text)
        assert rc == ERR_COMPILE
        assert p.value                                         # still set: the log can be read
        log = L.smcmi_program_log(p).decode()
        assert "likelihood.hip:3" in log, log
        assert "error" in log
        ptr, sz = C.c_void_p(), C.c_int64()
        assert L.smcmi_program_code(p, C.byref(ptr), C.byref(sz)) == ERR_ARG
        assert L.smcmi_program_destroy(p) == 0


def test_a_source_without_the_entry_function_does_not_compile(L):
    rc, p = _compile(L, GAUSS.replace("loglik", "something_else"))
    assert rc == ERR_COMPILE and p.value
    log = L.smcmi_program_log(p).decode()
    assert "loglik" in log, log
    L.smcmi_program_destroy(p)
    rc, p = _compile(L, GAUSS, entry="other_entry")
    assert rc == ERR_COMPILE and p.value
    assert "other_entry" in L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)


@pytest.mark.parametrize("options", ["--offload-arch=gfx942", "-mcpu=gfx90a", "--offload-arch=gfx950:xnack+", "-mxnack"])
def test_options_that_name_a_target_are_refused(L, options):
    rc, p = _compile(L, GAUSS, options=options)
    assert rc == ERR_ARG and not p.value
    assert b"refused" in L.smcmi_last_error()


@pytest.mark.parametrize("entry", ["9x", "a b", ""])
def test_an_entry_that_is_no_identifier_is_refused(L, entry):
    rc, p = _compile(L, GAUSS, entry=entry)
    assert rc == ERR_ARG and not p.value


def test_a_null_source_is_refused(L):
    rc, p = _compile(L, None)
    assert rc == ERR_ARG and not p.value
    assert L.smcmi_program_compile(GAUSS.encode(), None, None, None) == ERR_ARG
    assert L.smcmi_program_log(None) == b""


def test_a_define_in_the_options_reaches_the_source(L):
    src = GAUSS + "\nstatic_assert(NAME == 3.5, \"NAME did not arrive\");\n"
    rc, p = _compile(L, src)
    assert rc == ERR_COMPILE and "NAME" in L.smcmi_program_log(p).decode()          # without the option: undeclared
    L.smcmi_program_destroy(p)
    rc, p = _compile(L, src, options="  -DNAME=3.5 \t -DUNUSED=1 ")
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)
    rc, p = _compile(L, src, options="-DNAME=3.25")
    assert rc == ERR_COMPILE and "NAME did not arrive" in L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)


def test_the_python_wrapper_compiles_and_raises_with_the_log(L):
    import smc_jl_amd as S

    prog = S.Engine.compile_program(GAUSS)
    assert prog.log == "" and prog.code[:4] == b"\x7fELF"
    prog.close()
    prog.close()
    with pytest.raises(S.CompileError) as ei:
        S.Engine.compile_program("__device__ double loglik(const double *theta) {\n  return theta[0]\n}\n")
    assert "likelihood.hip:2" in ei.value.log and ei.value.code == ERR_COMPILE
    with pytest.raises(S._lib.SMCMIError) as ei:
        S.Engine.compile_program(GAUSS, options="-mcpu=gfx90a")
    assert ei.value.code == ERR_ARG and not isinstance(ei.value, S.CompileError)
    lik = S.HIPLikelihood(GAUSS, par=[0.0, 2.0])
    assert lik.program() is lik.program()


def test_the_library_has_no_link_time_dependency_on_the_run_time_compiler(L):
    for so in ("libsmcmi.so", "libsmcmi_strict.so"):
        path = os.path.join(ROOT, "smc.jl_amd", "csrc", so)
        if not os.path.exists(path):
            continue
        out = subprocess.run(["readelf", "-d", path], capture_output=True, text=True).stdout
        needed = [ln for ln in out.splitlines() if "NEEDED" in ln]
        assert needed and not [ln for ln in needed if "hiprtc" in ln], needed


def test_progsrc_on_its_own_under_the_sanitizers(tmp_path):
    """tests/progsrc_check.cpp: the assembled text's #line arithmetic (sources with and without a trailing newline), entry validation,
    option splitting and refusals (empty, very long, white-space-only strings) - host code, no run-time compiler in that process."""
    exe = tmp_path / "progsrc_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "progsrc_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    assert "progsrc_check ok" in r.stdout
