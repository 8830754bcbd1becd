"""Ensembles whose members carry a likelihood compiled from HIP source (smcmi_program_compile_ensemble): E small clouds in ONE launch
against (a) the same E handles driven one after another by smcmi_run with the same program - the split path, what a user had before - and
(b) the device-family ensemble of the same model.

    python tools/ensemble_program_bench.py [--members 1 16 64 256] [--sizes 1000 5000] [--reps 5] [--out profiles/r17_ensemble_program.json]
    python tools/ensemble_program_bench.py --ab-library OTHER/libsmcmi.so      (adds: the built-in ensemble, this build against another)

Workload: config 2's 10-dim Gaussian as HIP source on the fixed 300-stage schedule.  Every repetition starts all paths from the same
uploaded clouds (the uploads are not timed); a timing is the host clock around a call that ends in a stream synchronisation; the paths
alternate in one process, after one warm-up of each, and the medians of `reps` repetitions are written per (n_parts, E) with every
repetition kept next to them, and the largest |Δ log-MDD| between the program ensemble and each other path over the members.
--ab-library: the device-family ensemble (E = 64 and 256 at 1 000 particles) timed in fresh child processes that alternate between this
build's library and the other one (SMCMI_LIBRARY), `reps` children each, one median per child.  Not part of bench.py."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
KW = dict(n_phi=300, use_fixed_schedule=True)


def timed_ensemble(es, starts):
    from smc_jl_amd import run_ensemble

    for e, P in zip(es, starts):
        e.upload_cloud(P)
    t0 = time.perf_counter()
    rs = run_ensemble(es, **KW)
    dt = time.perf_counter() - t0
    assert all(r["status"] == 0 for r in rs)
    return dt, [r["logmdd"] for r in rs]


def timed_sequential(es, starts):
    for e, P in zip(es, starts):
        e.upload_cloud(P)
    t0 = time.perf_counter()
    rs = [e.run(**KW) for e in es]
    return time.perf_counter() - t0, [r["logmdd"] for r in rs]


def family_child(members, n, reps):
    """child of --ab-library: the device-family ensemble under whatever library SMCMI_LIBRARY names; prints one JSON line"""
    from smc_jl_amd.host import _lib

    import ctypes

    probe = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]          # (an older build lacks the newest entry points; none is used here)
    from smc_jl_amd import Engine
    from smc_jl_amd.host import workloads as w

    spec = w.gauss_spec()
    out = {}
    engines, starts = [], []
    for k in range(max(members)):
        e = Engine(n, 10, seed=1 + k, max_stages=300, store_history=False)
        e.set_model(spec)
        e.init_from_prior()
        starts.append(e.download_cloud())
        engines.append(e)
    for E in members:
        timed_ensemble(engines[:E], starts)
        out[str(E)] = 1e3 * statistics.median(timed_ensemble(engines[:E], starts)[0] for _ in range(reps))
    for e in engines:
        e.close()
    print(json.dumps(dict(library=_lib.LIB_PATH, n_parts=n, family_ensemble_ms=out)), flush=True)


def ab(other, reps):
    from smc_jl_amd.host import _lib

    runs = {"this": [], "other": []}
    for _ in range(reps):
        for which, path in (("other", os.path.abspath(other)), ("this", _lib.LIB_PATH)):
            env = dict(os.environ, SMCMI_LIBRARY=path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-family"], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
            runs[which].append(json.loads(r.stdout.strip().splitlines()[-1])["family_ensemble_ms"])
            print(which, runs[which][-1], flush=True)
    out = {}
    for E in runs["this"][0]:
        a, b = [x[E] for x in runs["this"]], [x[E] for x in runs["other"]]
        out[E] = dict(this_ms=statistics.median(a), other_ms=statistics.median(b), this_ms_all=a, other_ms_all=b,
                      other_spread_ms=max(b) - min(b), this_minus_other_ms=statistics.median(a) - statistics.median(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab-library", default=None)
    ap.add_argument("--child-family", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_ensemble_program.json"))
    a = ap.parse_args()
    if a.child_family:
        family_child([64, 256], 1000, 5)
        return
    from smc_jl_amd import Engine
    from smc_jl_amd.host import workloads as w

    spec = w.gauss_spec()
    d = 10
    m, sig = spec["lik"][2].reshape(-1, 1), float(spec["lik"][1][0])
    par = [-0.5 * d * math.log(2.0 * math.pi * sig * sig), 2.0 * sig * sig]
    t0 = time.perf_counter()
    prog = Engine.compile_program(GAUSS_SRC, ensemble_para=d)
    compile_s = time.perf_counter() - t0
    rows = []
    result = dict(tool="tools/ensemble_program_bench.py", compile_seconds=compile_s, rows=rows)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    for n in a.sizes:
        emax = max(a.members)
        progs, fams, starts = [], [], []
        for k in range(emax):
            f = Engine(n, d, seed=1 + k, max_stages=300, store_history=False)
            f.set_model(spec)
            f.init_from_prior()
            starts.append(f.download_cloud())
            fams.append(f)
            e = Engine(n, d, seed=1 + k, max_stages=300, store_history=False)
            e.set_model(spec)
            e.set_likelihood_program(prog, data=m, par=par)
            progs.append(e)
        for E in a.members:
            paths = dict(program_ensemble=lambda: timed_ensemble(progs[:E], starts), program_sequential=lambda: timed_sequential(progs[:E], starts),
                         family_ensemble=lambda: timed_ensemble(fams[:E], starts))
            for f in paths.values():
                f()                                                # warm-up of every path
            t = {k: [] for k in paths}
            worst = dict(program_sequential=0.0, family_ensemble=0.0)
            for _ in range(a.reps):
                lm = {}
                for k, f in paths.items():
                    dt, lm[k] = f()
                    t[k].append(dt)
                for k in worst:
                    worst[k] = max(worst[k], max(abs(x - y) for x, y in zip(lm["program_ensemble"], lm[k])))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = dict(workload="gauss10_fixed300_as_hip_source", n_parts=n, n_para=d, stages=300, members=E, reps=a.reps,
                       program_ensemble_ms=1e3 * med["program_ensemble"], program_sequential_ms=1e3 * med["program_sequential"],
                       family_ensemble_ms=1e3 * med["family_ensemble"],
                       program_ensemble_over_program_sequential=med["program_ensemble"] / med["program_sequential"],
                       program_ensemble_over_family_ensemble=med["program_ensemble"] / med["family_ensemble"],
                       all_ms={k: [1e3 * x for x in v] for k, v in t.items()},
                       max_abs_logmdd_difference_to_program_sequential=worst["program_sequential"],
                       max_abs_logmdd_difference_to_family_ensemble=worst["family_ensemble"])
            print(json.dumps({k: v for k, v in row.items() if k != "all_ms"}), flush=True)
            rows.append(row)
            save()
        for e in progs + fams:
            e.close()
    if a.ab_library:
        result["builtin_ensemble_this_build_against_other"] = dict(other_library=os.path.basename(os.path.dirname(os.path.abspath(a.ab_library))),
                                                                   n_parts=1000, reps=a.reps, members=ab(a.ab_library, a.reps))
        print(json.dumps(result["builtin_ensemble_this_build_against_other"]), flush=True)
    save()


if __name__ == "__main__":
    main()
