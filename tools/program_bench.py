#!/usr/bin/env python
"""What a likelihood compiled at run time from HIP source costs next to the two alternatives a user has on the GPU.

Workload: config 2 (10-dim isotropic Gaussian, adaptive tempering, one MH step x one block), N = 100 000 and 1 000 000.  Four legs on the
same Philox seed and the same starting cloud, alternating in ONE process, medians of five runs each after a warm-up run of every leg:

  (a) program  - the likelihood as a string of HIP source (smcmi_program_compile / smcmi_set_likelihood_program): one launch per score
  (b) callback - a device callback whose function launches a user-written kernel of the same likelihood (tools/program_bench_cb.hip:
                 what examples/c_abi_device_callback.hip does): count -> scan -> copy -> synchronise -> [pack] -> call -> scatter
  (c) family   - the built-in device family (the mutation kernel evaluates it itself)
  (d) fused    - the source of (a) compiled with SMCMI_PROGRAM_FUSED: the function inside the generic mutation kernel, one launch per stage

A run's time is smcmi_result.seconds: the host clock around the whole loop, which ends in a stream synchronise.  Per leg and N: ms per
stage, particle-stages/s, smcmi_callback_phases per stage, likelihood launches per stage; once: compile and module-load times, plain and
fused, the code objects' sizes and the fused kernel's registers, scratch and LDS from the code object's notes.
The yardstick for (a) is (b) measured here, in the same job; the one for (d) is (a), by more than (a)'s run-to-run spread, and (c) is what
is left to gain.  The whole comparison then runs once more in a child process with SMCMI_FUSED_AHEAD=1 (the switch is read once per
process): there leg (d) sends its launch ahead of the stage's verdict; the profile holds both (d)s, each next to the (a) of its own process.
There is no CPU fallback: without a GPU the tool fails.

  python tools/program_bench.py --out profiles/r16_fused_program.json
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


def kernel_notes(code, name):
    """registers, scratch and LDS of kernel `name` from the code object's notes (llvm-readelf --notes), or None without the tool"""
    import tempfile

    tool = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(tool):
        return None
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
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-ahead", action="store_true", help="do not repeat the comparison in a child process with SMCMI_FUSED_AHEAD=1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_fused_program.json"))
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
    t0 = time.perf_counter()
    fprog = S.Engine.compile_program(SOURCE, fused=True)
    fused_compile_s = time.perf_counter() - t0
    kw = dict(use_fixed_schedule=False, tempering_target=0.97)
    out = dict(workload="config 2: gauss_iso d=10, adaptive (tempering_target 0.97), 1 MH step x 1 block", repeats=args.repeats,
               method="four legs alternating in one process, medians of smcmi_result.seconds after one warm-up run per leg",
               compile_ms=1e3 * compile_s, code_object_bytes=len(prog.code), fused_compile_ms=1e3 * fused_compile_s,
               fused_code_object_bytes=len(fprog.code), fused_kernel_notes=kernel_notes(fprog.code, "smcmi_program_mutate"), sizes={})
    for n in args.sizes:
        engines, load_ms, fused_load_ms = {}, None, None
        P0 = None
        for leg in ("program", "callback", "family", "fused"):
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
            elif leg == "fused":
                t0 = time.perf_counter()
                e.set_likelihood_program(fprog, data=mean.reshape(-1, 1), par=[c0, 2.0 * SIGMA * SIGMA])
                fused_load_ms = 1e3 * (time.perf_counter() - t0)
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
        ra, rb, rc, rd = last["program"][0], last["callback"][0], last["family"][0], last["fused"][0]
        assert rd["n_stages"] == ra["n_stages"] and rd["resamples"] == ra["resamples"] and rd["logmdd"] == ra["logmdd"], (ra, rd)   # (d) is (a) bit for bit
        assert last["fused"][2]["evaluations"] == last["program"][2]["evaluations"]
        assert ra["n_stages"] == rb["n_stages"] == rc["n_stages"] and ra["resamples"] == rb["resamples"] == rc["resamples"], (ra, rb, rc)
        assert ra["logmdd"] == rb["logmdd"], (ra["logmdd"], rb["logmdd"])          # the same operations in the same order
        assert abs(ra["logmdd"] - rc["logmdd"]) < 1e-9
        st = ra["n_stages"] - 1
        entry = dict(n_stages=ra["n_stages"], logmdd=ra["logmdd"], module_load_and_register_ms=load_ms,
                     fused_module_load_and_register_ms=fused_load_ms, legs={})
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
        dd, cc = entry["legs"]["fused"], entry["legs"]["family"]
        entry["fused_over_program"] = dd["ms_per_stage"] / a["ms_per_stage"]
        entry["fused_over_family"] = dd["ms_per_stage"] / cc["ms_per_stage"]
        entry["program_minus_fused_ms_per_stage"] = a["ms_per_stage"] - dd["ms_per_stage"]
        entry["program_spread_ms_per_stage"] = a["ms_per_stage_max"] - a["ms_per_stage_min"]
        entry["fused_spread_ms_per_stage"] = dd["ms_per_stage_max"] - dd["ms_per_stage_min"]
        entry["fused_beats_program_by_more_than_its_spread"] = entry["program_minus_fused_ms_per_stage"] > entry["program_spread_ms_per_stage"]
        out["sizes"][str(n)] = entry
        print("N=%d: program %.4f  callback %.4f  family %.4f ms/stage (ratio a/b %.3f; b's count wait %.4f, b's spread %.4f)" %
              (n, a["ms_per_stage"], b["ms_per_stage"], entry["legs"]["family"]["ms_per_stage"], entry["program_over_callback"],
               entry["callback_count_wait_ms_per_stage"], entry["callback_spread_ms_per_stage"]), flush=True)
        print("N=%d: fused %.4f ms/stage (d/a %.3f, d/c %.3f; a's spread %.4f, d's spread %.4f)" %
              (n, dd["ms_per_stage"], entry["fused_over_program"], entry["fused_over_family"], entry["program_spread_ms_per_stage"],
               entry["fused_spread_ms_per_stage"]), flush=True)
        for e in engines.values():
            e.close()
    prog.close()
    fprog.close()
    out["fused_ahead_in_this_process"] = int(os.environ.get("SMCMI_FUSED_AHEAD", "0") or 0)
    if not args.no_ahead:
        assert out["fused_ahead_in_this_process"] == 0, "the parent measures launch-after-verdict: unset SMCMI_FUSED_AHEAD"
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            child = os.path.join(tmp, "ahead.json")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--no-ahead", "--repeats", str(args.repeats), "--out", child, "--sizes"] +
                                  [str(n) for n in args.sizes], env=dict(os.environ, SMCMI_FUSED_AHEAD="1"))
            ah = json.load(open(child))
        assert ah["fused_ahead_in_this_process"] == 1
        cmp_ = {}
        for n in out["sizes"]:
            here, there = out["sizes"][n], ah["sizes"][n]
            assert there["logmdd"] == here["logmdd"] and there["n_stages"] == here["n_stages"]
            d0, d1, a0, a1 = here["legs"]["fused"], there["legs"]["fused"], here["legs"]["program"], there["legs"]["program"]
            spread = max(d0["ms_per_stage_max"] - d0["ms_per_stage_min"], d1["ms_per_stage_max"] - d1["ms_per_stage_min"])
            cmp_[n] = dict(after_verdict=dict(fused=d0, program_same_process_ms_per_stage=a0["ms_per_stage"], fused_over_program=d0["ms_per_stage"] / a0["ms_per_stage"]),
                           ahead_of_verdict=dict(fused=d1, program_same_process_ms_per_stage=a1["ms_per_stage"], fused_over_program=d1["ms_per_stage"] / a1["ms_per_stage"],
                                                 program_spread_ms_per_stage=there["program_spread_ms_per_stage"],
                                                 fused_beats_program_by_more_than_its_spread=there["fused_beats_program_by_more_than_its_spread"]),
                           after_minus_ahead_ms_per_stage=d0["ms_per_stage"] - d1["ms_per_stage"], larger_spread_ms_per_stage=spread,
                           ahead_faster_by_more_than_the_spread=(d0["ms_per_stage"] - d1["ms_per_stage"]) > spread)
            print("N=%s: fused after the verdict %.4f, ahead of it %.4f ms/stage (spread %.4f); ahead: d/a %.3f" %
                  (n, d0["ms_per_stage"], d1["ms_per_stage"], spread, cmp_[n]["ahead_of_verdict"]["fused_over_program"]), flush=True)
        out["launch_ahead"] = dict(method="the same tool in a child process with SMCMI_FUSED_AHEAD=1, after this one; each (d) next to the (a) of its own process",
                                   sizes=cmp_, keep=all(c["ahead_faster_by_more_than_the_spread"] for c in cmp_.values()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, compile_ms=out["compile_ms"])))


if __name__ == "__main__":
    main()
