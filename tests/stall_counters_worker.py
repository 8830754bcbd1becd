"""One case of tests/test_gpu_stall_counters.py in a process of its own (the development switches are read once per process):
`python tests/stall_counters_worker.py <case>` runs it on cuda:0 and prints one JSON line of what the host drivers decided - stage, resample,
pass, stall and segment counts -, the log-MDD and a position-weighted checksum of the cloud.  tools/record_stall_counters.py records the
fixture with the same cases."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what every case compares with the fixture, exactly
KEYS = ("n_stages", "resamples", "solver_passes", "solver_stalls", "select_stalls", "spec_stalls", "n_segments", "shift_fallback_stage",
        "logmdd", "checksum")

# driver -> the switches that select it (a single handle; route.hpp)
DRIVERS = {"engine1": {"SMCMI_ENGINE": "1"}, "launches": {"SMCMI_ENGINE3": "0"}, "segments": {}, "segments_leave": {"SMCMI_SEG_SELECT": "0"}}
ADAPTIVE = dict(use_fixed_schedule=False, tempering_target=0.9, n_phi=100)
SETTINGS = {
    "adaptive": (ADAPTIVE, {}),
    # phi_rtol < 0 asks for the root to adjacent floats: more passes than the one enqueued -> solver stalls
    "short_solver": (dict(ADAPTIVE, solver_passes=1, phi_rtol=-1.0, sync_every=4), {}),
    # the host deliberately predicts "never resamples": every resample stage stalls - as a missing selection where no prediction of ϕ_n is
    # made (phi_rtol < 0: nothing to verify one against), else as a prediction that does not verify (spec stalls, their strikes, the switch-off)
    "never_select": (dict(ADAPTIVE, phi_rtol=-1.0), {"SMCMI_NO_SELECT_PREDICT": "2"}),
    "never_select_spec": (ADAPTIVE, {"SMCMI_NO_SELECT_PREDICT": "2"}),
    # nobody can foresee a fixed schedule's resamples: the host-note stall path of engine 1, the leaving segment
    "fixed": (dict(use_fixed_schedule=True, n_phi=100), {}),
}


def _cases():
    out = {}
    for drv, denv in DRIVERS.items():
        for st, (kw, senv) in SETTINGS.items():
            if (drv, st) != ("segments", "never_select_spec"):       # (a segment that resamples in place does not ask the forecast: no stall)
                out["gauss6_%s_%s" % (drv, st)] = dict(kind="single", d=6, seed=21, env=dict(denv, **senv), kw=kw)
    # two parameters: predictions stop verifying - the spec strikes and the switch-off
    for drv in ("engine1", "segments"):
        out["gauss2_%s_adaptive" % drv] = dict(kind="single", d=2, seed=21, env=DRIVERS[drv], kw=ADAPTIVE)
    # two handles of 4 096 through run_group on run_sharded_impl (run_group has no sync_every): twenty parameters - no resample forecast at
    # that size, so no wrong one either - and, with engine 2 switched away, six (the forecast, its stalls) and two (the spec strikes)
    for st, (kw, senv) in SETTINGS.items():
        kw = {k: v for k, v in kw.items() if k != "sync_every"}
        if not st.startswith("never_select"):
            out["gauss20_group_%s" % st] = dict(kind="group", d=20, seed=21, env=senv, kw=kw)
        out["gauss6_group_engine1_%s" % st] = dict(kind="group", d=6, seed=21, env=dict(DRIVERS["engine1"], **senv), kw=kw)
    out["gauss2_group_engine1_adaptive"] = dict(kind="group", d=2, seed=21, env=DRIVERS["engine1"], kw=ADAPTIVE)
    for st in ("adaptive", "short_solver"):
        out["gauss6_closure_%s" % st] = dict(kind="closure", d=6, seed=21, env={}, kw=SETTINGS[st][0])
    # profile mode: HIP events around the mutation launches, voided behind every stall
    for drv in ("engine1", "launches"):
        out["gauss6_%s_profile" % drv] = dict(kind="single", d=6, seed=21, env=DRIVERS[drv], kw=dict(SETTINGS["short_solver"][0], use_graph=2))
    return out


CASES = _cases()
N_PARTS = 8192


def conditions(name, r):
    """what the commit the fixture is recorded from must show, for the case to test what it is there for: the unmet ones"""
    bad = []
    if name.endswith(("_short_solver", "_profile")) and not r["solver_stalls"] > 0:
        bad.append("solver_stalls > 0")
    if name.endswith("_never_select") and not r["select_stalls"] >= r["resamples"] > 0:
        bad.append("select_stalls >= resamples > 0")
    if name.endswith("_never_select_spec") and not r["select_stalls"] + r["spec_stalls"] >= r["resamples"] > 0:
        bad.append("select_stalls + spec_stalls >= resamples > 0")
    if name.startswith("gauss2_") and not r["spec_stalls"] > 0:
        bad.append("spec_stalls > 0")
    return bad


def case_env(name):
    """the environment a case's process runs in"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("SMCMI_") and k != "SMCMI_LIBRARY")}
    env.update(CASES[name]["env"])
    return env


def run_case(name):
    import numpy as np

    sys.path.insert(0, ROOT)
    from smc_jl_amd import Engine, run_group
    from smc_jl_amd.host import workloads as models

    c = CASES[name]
    d, seed = c["d"], c["seed"]
    spec = models.gauss_spec(d=d)
    if c["kind"] == "group":
        engs = []
        for r in range(2):
            e = Engine(N_PARTS, d, seed=seed, max_stages=2000, store_history=False, n_local=N_PARTS // 2, gid0=r * (N_PARTS // 2))
            e.set_model(spec)
            e.init_from_prior()
            engs.append(e)
        res = run_group(engs, **c["kw"])
        P = np.concatenate([e.download_cloud() for e in engs], axis=0)
    else:
        e = Engine(N_PARTS, d, seed=seed, max_stages=2000, store_history=False)
        e.set_model(spec)
        e.init_from_prior()
        if c["kind"] == "closure":
            m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
            c0 = -0.5 * d * math.log(2.0 * math.pi * sig * sig)

            def lik(th):
                acc = np.zeros(th.shape[0])
                for k in range(th.shape[1]):
                    acc += (th[:, k] - m[k]) ** 2
                return c0 - acc / (2.0 * sig * sig)
            P0 = e.download_cloud()
            e.set_likelihood_callback(lik, which=0)
            e.upload_cloud(P0)
        res = e.run(**c["kw"])
        P = e.download_cloud()
    rows = 1.0 + (np.arange(P.shape[0]) % 251)[:, None]
    cols = np.arange(1, P.shape[1] + 1)[None, :]
    out = {k: res[k] for k in KEYS if k in res}
    out["checksum"] = float(np.sum(P * rows * cols))
    out["n_mutate_launches"] = res["n_mutate_launches"]
    out["kernel_ms_mutate"] = res["kernel_ms_mutate"]
    return out


if __name__ == "__main__":
    print(json.dumps(run_case(sys.argv[1])))
