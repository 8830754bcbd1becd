"""Ensemble runs: E small clouds in ONE launch (smcmi_run_ensemble, one workgroup per run) against the same E handles driven one after
another by smcmi_run in the same process and build.

    python tools/ensemble_bench.py [--members 1 16 64 256] [--reps 5] [--out profiles/r09_ensemble.json]

Workloads: the README's small-cloud workload - the 10-dim Gaussian on the fixed 300-stage schedule at 1 000 and 5 000 particles - and
config 1, the regression at 1 000 particles.  Every repetition starts both paths from the same uploaded clouds (the uploads are not
timed); a timing is the host clock around a call that ends in a stream synchronisation; the two paths alternate, after one warm-up of
each, and the medians of `reps` repetitions and their ratio are written per (workload, E), every repetition kept next to them.  The
largest |Δ log-MDD| between the two paths over the members is recorded as well.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workloads():
    from smc_jl_amd.host import workloads as w

    return [("gauss10_fixed300", w.gauss_spec(), 1000), ("gauss10_fixed300", w.gauss_spec(), 5000), ("regression_config1", w.regression_spec(), 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_ensemble.json"))
    a = ap.parse_args()
    from smc_jl_amd import Engine, run_ensemble

    kw = dict(n_phi=300, use_fixed_schedule=True)
    rows = []
    for name, spec, n in workloads():
        d = len(spec["priors"])
        emax = max(a.members)
        engines, starts = [], []
        for k in range(emax):
            e = Engine(n, d, seed=1 + k, max_stages=300, store_history=False)
            e.set_model(spec)
            e.init_from_prior()
            starts.append(e.download_cloud())
            engines.append(e)
        for E in a.members:
            es = engines[:E]

            def reset():
                for e, P in zip(es, starts):
                    e.upload_cloud(P)

            def ensemble():
                reset()
                t0 = time.perf_counter()
                rs = run_ensemble(es, **kw)
                dt = time.perf_counter() - t0
                assert all(r["status"] == 0 for r in rs)
                return dt, [r["logmdd"] for r in rs]

            def sequential():
                reset()
                t0 = time.perf_counter()
                rs = [e.run(**kw) for e in es]
                return time.perf_counter() - t0, [r["logmdd"] for r in rs]

            ensemble()                                          # warm-up of both paths: code objects, the engines' buffers
            sequential()
            te, ts, worst = [], [], 0.0
            for _ in range(a.reps):
                dt, le = ensemble()
                te.append(dt)
                dt, ls = sequential()
                ts.append(dt)
                worst = max(worst, max(abs(x - y) for x, y in zip(le, ls)))
            me, ms = statistics.median(te), statistics.median(ts)
            row = dict(workload=name, n_parts=n, n_para=d, stages=300, members=E, reps=a.reps, ensemble_ms=1e3 * me, sequential_ms=1e3 * ms,
                       ensemble_over_sequential=me / ms, ensemble_ms_all=[1e3 * x for x in te], sequential_ms_all=[1e3 * x for x in ts],
                       max_abs_logmdd_difference=worst)
            print(json.dumps(row), flush=True)
            rows.append(row)
        for e in engines:
            e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/ensemble_bench.py", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
