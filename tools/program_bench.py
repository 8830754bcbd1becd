#!/usr/bin/env python
"""What a likelihood compiled at run time from HIP source costs next to the two alternatives a user has on the GPU.

Workload: config 2 (10-dim isotropic Gaussian, adaptive tempering, one MH step x one block), N = 100 000 and 1 000 000.  Three legs on the
same Philox seed and the same starting cloud, alternating in ONE process, medians of five runs each after a warm-up run of every leg:

  (a) program  - the likelihood as a string of HIP source (smcmi_program_compile / smcmi_set_likelihood_program): one launch per score
  (b) callback - a device callback whose function launches a user-written kernel of the same likelihood (tools/program_bench_cb.hip:
                 what examples/c_abi_device_callback.hip does): count -> scan -> copy -> synchronise -> [pack] -> call -> scatter
  (c) family   - the built-in device family (the mutation kernel evaluates it itself)

A run's time is smcmi_result.seconds: the host clock around the whole loop, which ends in a stream synchronise.  Per leg and N: ms per
stage, particle-stages/s, smcmi_callback_phases per stage, likelihood launches per stage; once: compile and module-load times.
The yardstick for (a) is (b) measured here, in the same job.  There is no CPU fallback: without a GPU the tool fails.

  python tools/program_bench.py --out profiles/r15_program_likelihood.json
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCE = """__device__ double loglik(const double *theta, long long ld, int d, const double *data, long long rows, long long cols,
                         const double *par, long long n_par) {
    double acc = 0.0;
    for (int j = 0; j < d; ++j) {
        const double e = theta[j * ld] - data[j];
        acc += e * e;
    }
    return par[0] - acc / par[1];
}
"""
D, SIGMA = 10, 0.25


def callback_library():
    """tools/libprogram_bench_cb.so, built next to its source when it is not there"""
    so = os.path.join(ROOT, "tools", "libprogram_bench_cb.so")
    src = os.path.join(ROOT, "tools", "program_bench_cb.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", src, "-o", so])
    return C.CDLL(so)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_program_likelihood.json"))
    args = ap.parse_args()

    import smc_jl_amd as S
    from smc_jl_amd.host import _lib
    from smc_jl_amd.host import workloads

    spec = workloads.gauss_spec(D, SIGMA)
    mean = np.asarray(spec["lik"][2], dtype=np.float64).ravel()
    c0 = -0.5 * D * math.log(2.0 * math.pi * SIGMA * SIGMA)
    L = _lib.lib()
    cb = callback_library()
    cb.pb_setup.argtypes = [C.POINTER(C.c_double), C.c_double, C.c_double]
    cb.pb_setup(mean.ctypes.data_as(C.POINTER(C.c_double)), SIGMA, c0)
    dl = _lib.DeviceLik(C.cast(cb.pb_gauss_loglik, _lib.LIK_DEVICE_FN), None)

    t0 = time.perf_counter()
    prog = S.Engine.compile_program(SOURCE)
    compile_s = time.perf_counter() - t0
    kw = dict(use_fixed_schedule=False, tempering_target=0.97)
    out = dict(workload="config 2: gauss_iso d=10, adaptive (tempering_target 0.97), 1 MH step x 1 block", repeats=args.repeats,
               method="three legs alternating in one process, medians of smcmi_result.seconds after one warm-up run per leg",
               compile_ms=1e3 * compile_s, code_object_bytes=len(prog.code), sizes={})
    for n in args.sizes:
        engines, load_ms = {}, None
        P0 = None
        for leg in ("program", "callback", "family"):
            e = S.Engine(n, D, seed=1, max_stages=1500, store_history=False)
            e.set_model(spec)
            if P0 is None:
                e.init_from_prior()
                P0 = e.download_cloud()
            if leg == "program":
                t0 = time.perf_counter()
                e.set_likelihood_program(prog, data=mean.reshape(-1, 1), par=[c0, 2.0 * SIGMA * SIGMA])
                load_ms = 1e3 * (time.perf_counter() - t0)
            elif leg == "callback":
                _lib.check(L.smcmi_set_likelihood_device(e._h, 0, C.byref(dl)))
            engines[leg] = e
        runs = {leg: [] for leg in engines}
        last = {}
        for rep in range(args.repeats + 1):                  # (rep 0: warm-up - code objects load, buffers are made)
            for leg, e in engines.items():
                e.upload_cloud(P0)
                r = e.run(**kw)
                last[leg] = (r, e.callback_phases() if leg != "family" else None, e.callback_stats() if leg != "family" else None)
                if rep > 0:
                    runs[leg].append(r["seconds"])
        ra, rb, rc = last["program"][0], last["callback"][0], last["family"][0]
        assert ra["n_stages"] == rb["n_stages"] == rc["n_stages"] and ra["resamples"] == rb["resamples"] == rc["resamples"], (ra, rb, rc)
        assert ra["logmdd"] == rb["logmdd"], (ra["logmdd"], rb["logmdd"])          # the same operations in the same order
        assert abs(ra["logmdd"] - rc["logmdd"]) < 1e-9
        st = ra["n_stages"] - 1
        entry = dict(n_stages=ra["n_stages"], logmdd=ra["logmdd"], module_load_and_register_ms=load_ms, legs={})
        for leg in engines:
            secs = runs[leg]
            med = statistics.median(secs)
            r, ph, cs = last[leg]
            entry["legs"][leg] = dict(ms_per_stage=1e3 * med / st, ms_per_stage_min=1e3 * min(secs) / st, ms_per_stage_max=1e3 * max(secs) / st,
                                      particle_stages_per_s=n * st / med,
                                      phases_ms_per_stage=None if ph is None else {k: v / st for k, v in ph.items()},
                                      likelihood_launches_per_stage=None if cs is None else cs["calls"] / st,
                                      evaluations=None if cs is None else cs["evaluations"])
        a, b = entry["legs"]["program"], entry["legs"]["callback"]
        entry["program_over_callback"] = a["ms_per_stage"] / b["ms_per_stage"]
        entry["callback_minus_program_ms_per_stage"] = b["ms_per_stage"] - a["ms_per_stage"]
        entry["callback_count_wait_ms_per_stage"] = b["phases_ms_per_stage"]["count_wait"]
        entry["callback_spread_ms_per_stage"] = b["ms_per_stage_max"] - b["ms_per_stage_min"]
        out["sizes"][str(n)] = entry
        print("N=%d: program %.4f  callback %.4f  family %.4f ms/stage (ratio a/b %.3f; b's count wait %.4f, b's spread %.4f)" %
              (n, a["ms_per_stage"], b["ms_per_stage"], entry["legs"]["family"]["ms_per_stage"], entry["program_over_callback"],
               entry["callback_count_wait_ms_per_stage"], entry["callback_spread_ms_per_stage"]), flush=True)
        for e in engines.values():
            e.close()
    prog.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, compile_ms=out["compile_ms"])))


if __name__ == "__main__":
    main()
