"""Fused run-time compiled likelihoods (include/smcmi.h smcmi_program_compile_ex, SMCMI_PROGRAM_FUSED), the half that needs no GPU: the
compile of the user's function together with the generic mutation kernel (the run-time compiler cross-compiles for gfx950 without a
device), what the code object holds, the compiler log's line numbers, the refusals, that nothing is read from this machine's include
directories - and, as a stand-alone program under AddressSanitizer / UBSan, the pure text functions of csrc/fusedsrc.hpp."""
import ctypes as C
import os
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smc.jl_amd", "csrc")

ERR_ARG, ERR_COMPILE = -1, -11
FUSED = 1

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


def _compile(L, source, entry=None, options=None, flags=FUSED):
    p = C.c_void_p()
    enc = lambda s: None if s is None else s.encode()
    rc = L.smcmi_program_compile_ex(enc(source), enc(entry), enc(options), flags, C.byref(p))
    return rc, p


def _code(L, p):
    ptr, size = C.c_void_p(), C.c_int64()
    assert L.smcmi_program_code(p, C.byref(ptr), C.byref(size)) == 0
    return C.string_at(ptr, size.value)


def _is_fused(L, p):
    v = C.c_int32(-1)
    assert L.smcmi_program_is_fused(p, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def fused_gauss(L):
    """the one clean fused compile of this file"""
    t0 = time.perf_counter()
    rc, p = _compile(L, GAUSS_SRC)
    print("fused compile time %.3f s" % (time.perf_counter() - t0))
    assert rc == 0, (L.smcmi_last_error(), L.smcmi_program_log(p) if p else None)
    yield p
    L.smcmi_program_destroy(p)


def test_a_fused_code_object_holds_both_kernels_and_a_plain_one_only_the_wrapper(L, fused_gauss):
    code = _code(L, fused_gauss)
    print("fused code object: %d bytes" % len(code))
    assert code[:4] == b"\x7fELF"
    assert b"smcmi_program_kernel" in code and b"smcmi_program_mutate" in code and b"smcmi_program_abi" in code
    assert _is_fused(L, fused_gauss) == 1
    assert L.smcmi_program_log(fused_gauss) == b""
    rc, p = _compile(L, GAUSS_SRC, flags=0)
    assert rc == 0
    plain = _code(L, p)
    assert b"smcmi_program_kernel" in plain and b"smcmi_program_mutate" not in plain
    assert _is_fused(L, p) == 0
    # smcmi_program_compile is flags = 0: the same code object
    q = C.c_void_p()
    assert L.smcmi_program_compile(GAUSS_SRC.encode(), None, None, C.byref(q)) == 0
    assert _code(L, q) == plain and _is_fused(L, q) == 0
    L.smcmi_program_destroy(p)
    L.smcmi_program_destroy(q)
    assert L.smcmi_program_is_fused(None, None) == ERR_ARG


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
    """the mutation kernel lives in a namespace that has a function called loglik of its own: the hook names the user's function at global scope"""
    rc, p = _compile(L, GAUSS_SRC, entry="other_entry")
    assert rc == ERR_COMPILE and "other_entry" in L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)


@pytest.mark.parametrize("options", ["--offload-arch=gfx942", "-mcpu=gfx90a", "--offload-arch=gfx950:xnack+", "-mxnack"])
def test_options_that_name_a_target_are_refused_in_fused_mode_too(L, options):
    rc, p = _compile(L, GAUSS_SRC, options=options)
    assert rc == ERR_ARG and not p.value
    assert b"refused" in L.smcmi_last_error()


@pytest.mark.parametrize("flags", [2, 3, 1 << 30, -2])
def test_unknown_flag_bits_are_refused(L, flags):
    rc, p = _compile(L, GAUSS_SRC, flags=flags)
    assert rc == ERR_ARG and not p.value


MACHINE_PATHS = ("/usr", "/opt", "/lib", "/bin", "/include/", "gcc", "x86_64")


@pytest.mark.parametrize("header", ["vector", "string.h", "features.h", "stdio.h", "cmath"])
def test_a_system_header_the_library_does_not_supply_is_file_not_found(L, header):
    """the run-time compiler must not reach into this machine's include directories (-nostdinc -nostdinc++): every one of these exists on
    it - <string.h> and <features.h> would compile cleanly - and none is in the header table.  The diagnostic is the compiler's own
    'file not found' on the user's line, and no path of the machine appears in the log."""
    rc, p = _compile(L, "#include <%s>\n" % header + GAUSS_SRC)
    assert rc == ERR_COMPILE and p.value
    log = L.smcmi_program_log(p).decode()
    L.smcmi_program_destroy(p)
    assert "likelihood.hip:1" in log and "'%s' file not found" % header in log, log
    assert not [w for w in MACHINE_PATHS if w in log], log


def test_the_machine_s_c_library_is_not_visible(L):
    """<features.h> is what defines __GLIBC__: were it read, the probe below would stop the compile with its own message"""
    rc, p = _compile(L, "#if __has_include(<features.h>) || __has_include(<vector>) || __has_include(<string.h>)\n#error a header of the machine is visible\n#endif\n" + GAUSS_SRC)
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)
    # the stand-ins are what the library's own headers include, and a user may include them too
    rc, p = _compile(L, "#include <stdint.h>\n#include <math.h>\n#include <stddef.h>\n" + GAUSS_SRC)
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)


@pytest.mark.parametrize("options", ["-I/usr/include", "-isystem /usr/include", "-include stdio.h", "--sysroot=/", "-ffp-contract=fast", "-ffast-math",
                                     "-DSMCMI_PROGRAM_ENTRY=f", "-USMCMI_INST_UNIT", "-DSMCMI_STRICT_FP", "-DA=1 -idirafter /usr/include"])
def test_options_that_would_reach_the_engine_s_kernel_are_refused_in_fused_mode(L, options):
    """a fused program's options apply to the whole mutation kernel: include paths (the header isolation), contraction and fast math (the
    bits of the split path) and the library's own names are refused; a plain program takes them as before"""
    rc, p = _compile(L, GAUSS_SRC, options=options)
    assert rc == ERR_ARG and not p.value
    assert b"refused for a fused program" in L.smcmi_last_error()


def test_a_define_in_the_options_reaches_a_fused_source(L):
    rc, p = _compile(L, GAUSS_SRC + "\nstatic_assert(NAME == 3.5, \"NAME did not arrive\");\n", options="-DNAME=3.5")
    assert rc == 0, L.smcmi_program_log(p)
    L.smcmi_program_destroy(p)


def test_the_python_wrapper_passes_the_flag(L, fused_gauss):
    import smc_jl_amd as S

    assert S.Engine.compile_program(GAUSS_SRC).fused is False
    lik = S.HIPLikelihood(GAUSS_SRC, par=[0.0, 2.0], fused=True)
    assert lik.fused is True and S.HIPLikelihood(GAUSS_SRC).fused is False
    with pytest.raises(S.CompileError) as ei:
        S.Engine.compile_program("__device__ double loglik(const double *theta) {\n  return theta[0]\n}\n", fused=True)
    assert "likelihood.hip:2" in ei.value.log


def test_fusedsrc_on_its_own_under_the_sanitizers(tmp_path):
    """tests/fusedsrc_check.cpp: the fused text's #line arithmetic, the header table against the #include lines of the embedded text, and
    the embedded headers against the files - host code, no run-time compiler in that process.  The embedded text is the one the library's
    build left (csrc/build/embedded_headers.inc, what program.o was compiled from): a header edited since then fails the comparison, as it
    should.  Only where the library came without its build directory is the file made here."""
    if not os.path.exists(os.path.join(CSRC, "build", "embedded_headers.inc")):
        subprocess.check_call(["make", "-C", CSRC, "build/embedded_headers.inc"], stdout=subprocess.DEVNULL)
    exe = tmp_path / "fusedsrc_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(CSRC, "build"), os.path.join(ROOT, "tests", "fusedsrc_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), CSRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    assert "fusedsrc_check ok" in r.stdout
