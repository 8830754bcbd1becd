"""The device-pointer likelihood callback (smcmi_set_likelihood_device, include/smcmi.h) as far as it can be checked without a GPU:
the header declares it, the library exports it, the ctypes binding and the Python layers carry it, the plain-HIP example
cross-compiles and links, and the header stays C99."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "smcmi.h")
LIBDIR = os.path.join(ROOT, "smc.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_header_declares_and_library_exports_the_entry_point():
    txt = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    assert re.search(r"\bint\s+smcmi_set_likelihood_device\s*\(\s*smcmi_handle\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*const\s+smcmi_device_likelihood\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*smcmi_lik_device_fn\s*\)", txt)
    # (loaded by path with ctypes alone: resolving a symbol needs no GPU)
    lib = C.CDLL(os.path.join(LIBDIR, "libsmcmi.so"))
    assert hasattr(lib, "smcmi_set_likelihood_device")


def test_binding_declares_it_with_a_plain_pointer():
    from smc_jl_amd.host import _lib

    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert "smcmi_set_likelihood_device" in sym
    res, args = sym["smcmi_set_likelihood_device"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, C.c_void_p]
    # the struct the pointer refers to: a function pointer and the user's pointer, as the header lays it out
    assert [f[0] for f in _lib.DeviceLik._fields_] == ["fn", "user_data"]
    assert C.sizeof(_lib.DeviceLik) == 2 * C.sizeof(C.c_void_p)


def test_python_layers_carry_it():
    import smc_jl_amd as S

    assert callable(getattr(S.Engine, "set_likelihood_device"))
    assert "TorchLikelihood" in S.__all__
    from smc_jl_amd.host import api

    t = S.TorchLikelihood(lambda theta, data: theta.sum(dim=1))
    assert callable(t.fn) and not isinstance(t, api.DeviceLikelihood)
    assert api._lik_spec(t, None)[0] == "device_callback" and api._lik_kind(api._lik_spec(t, None)) == "device"
    assert api._lik_kind(api._lik_spec(lambda th, d: 0.0, None)) == "host"


def test_mixed_host_and_torch_likelihoods_are_refused_before_any_engine_exists():
    import numpy as np
    import pytest

    import smc_jl_amd as S

    pars = [S.parameter("a", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0)), S.parameter("b", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0))]
    data = np.zeros((40, 2))
    host = lambda th, dat: 0.0
    dev = S.TorchLikelihood(lambda th, dat: th.sum(dim=1))
    for new, old in ((host, dev), (dev, host)):
        with pytest.raises(NotImplementedError, match="both"):
            S.smc(new, pars, data, old_data=data[:20], old_loglikelihood=old, old_cloud=S.Cloud(2, 10), n_parts=100, verbose="none")


def test_the_hip_example_cross_compiles_and_links(tmp_path):
    exe = str(tmp_path / "c_abi_device_callback")
    src = os.path.join(ROOT, "examples", "c_abi_device_callback.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L", LIBDIR, "-lsmcmi", "-Wl,-rpath," + LIBDIR])
    assert os.path.getsize(exe) > 0


def test_header_with_a_device_likelihood_is_c99(tmp_path):
    src = tmp_path / "use_device_likelihood.c"
    src.write_text("""
#include <stddef.h>
#include "smcmi.h"
static int lik(const double *theta, int64_t m, int64_t ld, int64_t d, double *out, void *stream, void *user_data) {
    (void)theta; (void)m; (void)ld; (void)d; (void)out; (void)stream; (void)user_data;
    return 0;
}
int use(smcmi_handle *h) {
    smcmi_device_likelihood l;
    l.fn = lik;
    l.user_data = NULL;
    return smcmi_set_likelihood_device(h, SMCMI_WHICH_NEW, &l) + smcmi_set_likelihood_device(h, SMCMI_WHICH_OLD, NULL);
}
""")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
