#!/usr/bin/env python
"""What the device-pointer likelihood callback is worth: config 2 (10-dim isotropic Gaussian, adaptive tempering, bench.py's schedule)
at N = 100 000 and at N = 1 000 000, three ways on the same initial cloud and Philox seed -

    family  : the built-in device family (the likelihood inside the mutation kernel)
    host    : the host callback (numpy, batched, as api._batch hands a `batched` callable over)
    device  : a native torch likelihood through Engine.set_likelihood_device

Whole runs, one warm-up round, then --rounds rounds with the three modes alternating; per mode the median and the spread of the
particle-stages per second, and the callback phases (Engine.callback_phases, ms per stage) of the last round.

    python tools/device_callback_bench.py [--rounds 5] [--sizes 100000,1000000] [--modes family,host,device] [--out FILE.json]

Prints one JSON line; --out also writes it to a file.  --modes host times the host callback alone: run on two builds of the library
(SMCMI_LIBRARY selects one) it shows whether a change moved the host path.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")

D = 10
RUN_KW = dict(use_fixed_schedule=False, tempering_target=0.97, n_phi=300, lam=2.1, resampling_method="systematic",
              n_blocks=1, n_mh_steps=1, alpha=1.0, c=0.5, target=0.25, threshold_ratio=0.5)


def numpy_gauss(m, sig):
    c0 = -0.5 * len(m) * math.log(2.0 * math.pi * sig * sig)

    def f(th):
        acc = np.zeros(th.shape[0])
        for k in range(th.shape[1]):
            e = th[:, k] - m[k]
            acc += e * e
        return c0 - acc / (2.0 * sig * sig)
    return f


def torch_gauss(m, sig):
    import torch

    c0 = -0.5 * len(m) * math.log(2.0 * math.pi * sig * sig)
    mt = torch.as_tensor(np.asarray(m, dtype=np.float64), device="cuda")

    def f(th):
        e = th - mt[None, :]
        return c0 - (e * e).sum(dim=1) / (2.0 * sig * sig)
    return f


def one_run(mode, n, spec, P0, seed):
    from smc_jl_amd import Engine

    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    e = Engine(n, D, seed=seed, max_stages=1500, store_history=False)
    e.set_model(spec)
    if mode == "host":
        e.set_likelihood_callback(numpy_gauss(m, sig), which=0)
    elif mode == "device":
        e.set_likelihood_device(torch_gauss(m, sig), which=0)
    e.upload_cloud(P0)
    r = e.run(**RUN_KW)
    out = dict(n_stages=r["n_stages"], resamples=r["resamples"], logmdd=r["logmdd"], seconds=r["seconds"],
               particle_stages_per_s=n * (r["n_stages"] - 1) / r["seconds"])
    if mode != "family":
        st = r["n_stages"] - 1
        out["phases_ms_per_stage"] = {k: v / st for k, v in e.callback_phases().items()}
        out["stats"] = e.callback_stats()
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--modes", default="family,host,device")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from smc_jl_amd import Engine
    from smc_jl_amd.host import _lib, workloads

    modes = args.modes.split(",")
    spec = workloads.gauss_spec(D)
    res = dict(what="config 2 (10-dim Gaussian, adaptive, tempering target 0.97) three ways; whole runs, modes alternating, 1 warm-up round",
               library=os.path.basename(_lib.LIB_PATH), rounds=args.rounds, sizes={})
    for n in [int(x) for x in args.sizes.split(",")]:
        e = Engine(n, D, seed=args.seed, max_stages=4, store_history=False)
        e.set_model(spec)
        e.init_from_prior()
        P0 = e.download_cloud()
        e.close()
        runs = {m: [] for m in modes}
        for rnd in range(args.rounds + 1):
            for m in modes:
                r = one_run(m, n, spec, P0, args.seed)
                if rnd > 0:
                    runs[m].append(r)
                sys.stderr.write("n=%d round %d %-6s %.4f s  %.4g particle-stages/s\n" % (n, rnd, m, r["seconds"], r["particle_stages_per_s"]))
        entry = {}
        for m in modes:
            ps = [r["particle_stages_per_s"] for r in runs[m]]
            last = runs[m][-1]
            entry[m] = dict(particle_stages_per_s_median=statistics.median(ps), particle_stages_per_s_min=min(ps), particle_stages_per_s_max=max(ps),
                            seconds_all=[r["seconds"] for r in runs[m]], n_stages=last["n_stages"], resamples=last["resamples"], logmdd=last["logmdd"])
            if "phases_ms_per_stage" in last:
                entry[m]["phases_ms_per_stage"] = last["phases_ms_per_stage"]
                entry[m]["stats"] = last["stats"]
                entry[m]["ms_per_stage"] = 1e3 * last["seconds"] / (last["n_stages"] - 1)
        res["sizes"][str(n)] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
