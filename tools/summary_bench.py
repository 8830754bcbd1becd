"""Posterior summaries: the device call against what a user did before it existed - download_cloud() and the numpy mirror.

    python tools/summary_bench.py [--sizes 100000 1000000 10000000] [--reps 5] [--out profiles/r08_summaries.json]
    python tools/summary_bench.py --device-only 10000000        # one device call per repetition, nothing else (for a kernel trace)

d = 10, probs = (0.05, 0.95), every parameter column.  The cloud is a 10-dim Gaussian run paused after a few adaptive stages (general
weights).  The two paths alternate; the medians of `reps` runs and their ratio are written per size.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = (0.05, 0.95)


def make_engine(n):
    from smc_jl_amd import Engine
    from smc_jl_amd.host import workloads

    e = Engine(n, 10, seed=1, max_stages=400, store_history=False)
    e.set_model(workloads.gauss_spec())
    e.init_from_prior()
    r = e.run(use_fixed_schedule=False, tempering_target=0.97, stop_after_stage=5)
    assert r["paused"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_summaries.json"))
    ap.add_argument("--device-only", type=int, default=0, metavar="N")
    a = ap.parse_args()
    from smc_jl_amd.host import api

    if a.device_only:
        e = make_engine(a.device_only)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e.weighted_quantiles(probs=PROBS)
            print("device call at N = %d: %.3f ms" % (a.device_only, 1e3 * (time.perf_counter() - t0)), flush=True)
        return
    rows = []
    for n in a.sizes:
        e = make_engine(n)
        e.weighted_quantiles(probs=PROBS)                       # warm-up: code objects, the first allocation
        dev, host, worst = [], [], 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            q_dev = e.weighted_quantiles(probs=PROBS)
            t1 = time.perf_counter()
            q_host = api.weighted_quantiles(e.download_cloud(), PROBS)
            t2 = time.perf_counter()
            dev.append(t1 - t0)
            host.append(t2 - t1)
            worst = max(worst, float(np.max(np.abs(q_dev - q_host))))
        row = dict(n=n, d=10, probs=list(PROBS), reps=a.reps, device_ms=1e3 * statistics.median(dev), download_numpy_ms=1e3 * statistics.median(host),
                   ratio=statistics.median(host) / statistics.median(dev), device_ms_all=[1e3 * x for x in dev],
                   download_numpy_ms_all=[1e3 * x for x in host], max_abs_difference=worst)
        print(json.dumps(row), flush=True)
        rows.append(row)
        e.close()
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/summary_bench.py", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
