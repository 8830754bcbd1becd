"""CPU-only checks of the ensemble run (smcmi_run_ensemble: many small runs in one launch, one workgroup per run): the launch-shape function,
the binding of the new entry point through every layer, and its refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libmod():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "smc.jl_amd", "csrc", "libsmcmi.so")):
        ge.build()
    from smc_jl_amd.host import _lib

    return _lib


def test_launch_shape_covers_every_particle_once_and_fits_a_cu(tmp_path):
    """tests/ensemble_check.cpp drives csrc/ensshape.hpp for n_para 1..10 at n_parts 1, 63, 64, 65, T - 1, T, T + 1, 2 T + 77 and 8 192: LDS within
    160 KiB, every particle covered exactly once, alignment; 8 193 is refused.  Host code under AddressSanitizer and UBSan, no HIP: exit
    status 0, "ok", nothing on stderr."""
    exe = tmp_path / "ensemble_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "ensemble_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_binding_mirrors_the_header(libmod):
    hdr = open(os.path.join(ROOT, "include", "smcmi.h")).read()
    m = re.search(r"int\s+smcmi_run_ensemble\s*\(\s*smcmi_handle\s*\*\*\s*hs\s*,\s*int32_t\s+n\s*,\s*const\s+smcmi_run_config\s*\*\s*rc\s*,"
                  r"\s*smcmi_result\s*\*\s*res[^,]*,\s*int32_t\s*\*\s*status[^)]*\)\s*;", hdr)
    assert m, "include/smcmi.h does not declare smcmi_run_ensemble as the issue states it"
    cap = re.search(r"#define\s+SMCMI_ENS_MAX_PARTS\s+(\d+)", hdr)
    assert cap and int(cap.group(1)) == 8192 == libmod.ENS_MAX_PARTS
    sym = {n: (res, args) for n, res, args in libmod.SYMBOLS}
    assert "smcmi_run_ensemble" in sym
    res, args = sym["smcmi_run_ensemble"]
    assert res is C.c_int
    assert len(args) == 5
    assert args[0]._type_ is C.c_void_p and args[1] is C.c_int32
    assert args[2]._type_ is libmod.RunConfig and args[3]._type_ is libmod.Result and args[4]._type_ is C.c_int32
    L = libmod.lib()
    assert hasattr(L, "smcmi_run_ensemble")
    # the header says whether mixture proposals are served
    doc = hdr[:m.start()]
    assert re.search(r"alpha < 1: refused", doc)


def test_python_wrappers_take_the_keywords_of_engine_run(libmod):
    import smc_jl_amd
    from smc_jl_amd.host import api, engine

    run_kw = list(inspect.signature(engine.Engine.run).parameters)[1:]
    ens_kw = list(inspect.signature(engine.run_ensemble).parameters)
    assert ens_kw[0] == "engines" and ens_kw[1:] == run_kw
    for k in run_kw:          # ... with the same defaults
        assert inspect.signature(engine.run_ensemble).parameters[k].default == inspect.signature(engine.Engine.run).parameters[k].default, k
    assert smc_jl_amd.run_ensemble is engine.run_ensemble and smc_jl_amd.smc_ensemble is api.smc_ensemble
    sig = inspect.signature(api.smc_ensemble)
    assert list(sig.parameters)[:4] == ["loglikelihood", "parameters", "data", "seeds"]
    smc_sig = inspect.signature(api.smc)
    for k, p in sig.parameters.items():
        if k in smc_sig.parameters and k != "verbose":
            assert p.default == smc_sig.parameters[k].default, k
    with pytest.raises(ValueError):
        engine.run_ensemble([])


def test_smc_ensemble_refuses_a_python_callable():
    from smc_jl_amd.host import api

    pars = [api.parameter("a", 0.0, (-5.0, 5.0), prior=api.Normal(0.0, 1.0))]
    with pytest.raises(NotImplementedError, match=r"smc\(\)"):
        api.smc_ensemble(lambda th, data: 0.0, pars, np.zeros(1), seeds=[1, 2], n_parts=100)
    with pytest.raises(NotImplementedError, match=r"smc\(\)"):
        api.smc_ensemble(api.TorchLikelihood(lambda th, data: th.sum(1)), pars, np.zeros(1), seeds=[1], n_parts=100)
    # what the ensemble does not serve is said before a handle is made
    with pytest.raises(NotImplementedError, match=r"smc\(\)"):
        api.smc_ensemble(api.GaussIso(1.0), pars, np.zeros(1), seeds=[1], n_parts=8193)
    with pytest.raises(NotImplementedError, match=r"smc\(\)"):
        api.smc_ensemble(api.GaussIso(1.0), pars, np.zeros(1), seeds=[1], n_parts=100, alpha=0.9)
    with pytest.raises(ValueError):
        api.smc_ensemble(api.GaussIso(1.0), pars, np.zeros(1), seeds=[], n_parts=100)


def test_refusal_without_a_device(libmod):
    """smcmi_run_ensemble(NULL, 0, ...) is SMCMI_ERR_ARG before any HIP call: it returns the same on a machine without a GPU"""
    L = libmod.lib()
    rc = libmod.RunConfig(1, 1, 2.1, 20, 0, 0.5, 0.5, 1.0, 0.25, 1, 0.97, 0.0, 0.0, 0, 0, 0, 0.0, 0.0)
    res = (libmod.Result * 1)()
    assert L.smcmi_run_ensemble(None, 0, C.byref(rc), res, None) == -1
    assert L.smcmi_run_ensemble(None, 3, C.byref(rc), res, None) == -1
    arr = (C.c_void_p * 2)(None, None)
    assert L.smcmi_run_ensemble(arr, 2, C.byref(rc), res, None) == -1          # null handles
    assert L.smcmi_run_ensemble(arr, -1, C.byref(rc), res, None) == -1
    assert L.smcmi_last_error()


def test_julia_shim_binds_the_entry_point():
    src = open(os.path.join(ROOT, "smc.jl_amd", "julia", "SMCMI.jl")).read()
    assert re.search(r"ccall\(\(:smcmi_run_ensemble, LIB\), Cint, \(Ptr\{Handle\}, Int32, Ref\{RunConfig\}, Ref\{Result\}, Ptr\{Int32\}\)", src)


def test_the_ensemble_kernel_is_in_the_resource_report_and_adds_no_segment_kernel(libmod):
    """ten kens_run instantiations (n_para 1..10) without scratch memory; the static LDS they carry is within the bound the launch shape counts"""
    rep = os.path.join(ROOT, "smc.jl_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(rep):
        pytest.skip("library was built without the resource report")
    txt = open(rep).read()
    seen = {}
    for m in re.finditer(r"Function Name: _ZN5smcmi8kens_runILi(\d+)EE[^\n]*\n(?:[^\n]*\n){0,14}?[^\n]*LDS Size \[bytes/block\]: (\d+)", txt):
        blk = txt[m.start():m.end()]
        seen[int(m.group(1))] = (int(m.group(2)), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)))
    assert sorted(seen) == list(range(1, 11)), sorted(seen)
    for d, (static_lds, scratch) in seen.items():
        assert static_lds <= 1024, (d, static_lds)            # csrc/ensshape.hpp ENS_STATIC_LDS
        assert scratch == 0, (d, scratch)
