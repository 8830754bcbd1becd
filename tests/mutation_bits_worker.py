"""One driver of tests/test_gpu_mutation_bits.py in a process of its own (the development switches are read once per process):
`python tests/mutation_bits_worker.py <driver>` runs every case on cuda:0 and prints one JSON line: per case the SHA-256 of the downloaded
cloud's bytes and of the stage records, with the stage, resample and segment counts.  tools/record_mutation_bits.py records the fixture
with the same cases."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# driver -> the switches that select it (one handle; route.hpp), and the register kernel it runs
DRIVERS = {
    "engine1": {"SMCMI_ENGINE": "1"},                                  # k_mutate_reg
    "launches": {"SMCMI_ENGINE3": "0"},                                # k2_mutate
    "segments": {},                                                    # k3_segment
    "reduced": {"SMCMI_ENGINE": "2", "SMCMI_E2_REDUCED": "1"},         # k2b_mutate, the ZPART loads
}
N_PARTS = 2000          # no multiple of 256 or 512: the last block has dead lanes that take the !live path through the barriers
SEED = 3
_ADAPT = dict(use_fixed_schedule=False, tempering_target=0.8)
_TWO_FIXED = [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]                             # tests/test_gpu_proposal_paths.py: nf = 8 != d

RUNS = {
    "a1_d1": dict(d=1, kw=_ADAPT),                                                            # one Box-Muller pair, half used
    "mix_d2": dict(d=2, kw=dict(_ADAPT, alpha=0.9)),
    "a1_d9_3x2": dict(d=9, kw=dict(_ADAPT, n_blocks=3, n_mh_steps=2)),                        # odd D, the unpaired normal, t > 0 tags
    "mix_d10_3x2": dict(d=10, kw=dict(_ADAPT, alpha=0.9, n_blocks=3, n_mh_steps=2)),          # blocks of 4, 4 and 2
    "a1_d10_two_fixed": dict(d=10, kw=_ADAPT, fixed=_TWO_FIXED),
    "a1_d10_fixed_schedule": dict(d=10, kw=dict(use_fixed_schedule=True, n_phi=20)),          # the riding segment variant
    "other_priors": dict(d=5, kw=_ADAPT, other=True),                                         # has_other
}
# stand-alone mutate calls on a cloud from init_from_prior: k_mutate_reg's in-kernel draws (in a run of this size engine 1 draws ahead).
# They run k_mutate_reg whatever the switches say: MUTATE_DRIVER alone runs them.
MUTATES = {
    "mutate_a1_d9": dict(d=9, alpha=1.0, block_ptr=[0, 9], n_mh=1),
    "mutate_mix_d10_3": dict(d=10, alpha=0.9, block_ptr=[0, 4, 8, 10], n_mh=2),
}
MUTATE_DRIVER = "engine1"
RECORDS = ("schedule", "ess", "c_hist", "accept_hist", "resampled")


def driver_env(driver):
    """the environment a driver's process runs in"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("SMCMI_") and k != "SMCMI_LIBRARY")}
    env.update(DRIVERS[driver])
    return env


def run_worker(driver):
    """every case of one driver in a fresh process: {case: what run_driver() recorded}"""
    import subprocess

    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mutation_bits_worker.py"), driver], env=driver_env(driver),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, "%s: exit status %d\n%s" % (driver, res.returncode, res.stderr[-2000:])
    return json.loads(res.stdout.strip().splitlines()[-1])


def _spec(case):
    import smc_jl_amd as S
    from smc_jl_amd.host import api
    from smc_jl_amd.host import workloads as models

    if case.get("other"):               # the model of tests/test_gpu_parity.py::test_other_prior_families_device_draw_and_mutation
        import numpy as np
        pars = [S.parameter("g", 1.0, (1e-8, 1e5), prior=S.Gamma(2.0, 1.0)),
                S.parameter("b", 0.5, (0.0, 1.0), prior=S.Beta(2.0, 2.0)),
                S.parameter("ig", 1.0, (1e-8, 1e5), prior=S.InverseGamma(3.0, 2.0)),
                S.parameter("rig", 0.5, (1e-8, 1e5), prior=S.RootInverseGamma(4.0, 0.5)),
                S.parameter("n", 0.0, prior=S.Normal(0.0, 2.0))]
        return api._spec_from(pars, S.GaussIso(0.3).spec(np.array([1.5, 0.4, 1.2, 0.6, -0.3])), None)
    spec = models.gauss_spec(d=case["d"])
    if case.get("fixed"):
        spec["fixed"] = list(case["fixed"])
    return spec


def _sha(*arrays):
    import numpy as np

    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_driver(driver):
    import numpy as np

    sys.path.insert(0, ROOT)
    from smc_jl_amd import Engine

    out = {}
    for name, case in RUNS.items():
        e = Engine(N_PARTS, case["d"], seed=SEED, max_stages=400, store_history=False)
        e.set_model(_spec(case))
        e.init_from_prior()
        r = e.run(**case["kw"])
        rec = e.stage_records(r["n_stages"])
        out[name] = dict(cloud=_sha(e.download_cloud()), records=_sha(*[rec[k] for k in RECORDS], np.float64(r["logmdd"])),
                         n_stages=int(r["n_stages"]), resamples=int(r["resamples"]), n_segments=int(r["n_segments"]))
        e.close()
    for name, case in (MUTATES if driver == MUTATE_DRIVER else {}).items():
        d = case["d"]
        e = Engine(N_PARTS, d, seed=SEED, max_stages=4, store_history=False)
        e.set_model(_spec(case))
        e.init_from_prior()
        k = np.arange(d, dtype=np.float64)
        mu = -0.5 + 0.125 * k                                              # exact in binary: the same proposal wherever this runs
        Sigma = 0.25 * np.eye(d) + 0.0625                                  # 0.0625 everywhere, 0.3125 on the diagonal
        blocks_free = [(3 * j) % d if d == 10 else (2 * j) % d for j in range(d)]        # a permutation (3 ⟂ 10, 2 ⟂ 9)
        acc = e.mutate(mu, Sigma, case["block_ptr"], blocks_free, 0.25, 0.0, 0.5, case["alpha"], case["n_mh"], 2)
        out[name] = dict(cloud=_sha(e.download_cloud()), accept=float(acc))
        e.close()
    return out


if __name__ == "__main__":
    os.environ.update(DRIVERS[sys.argv[1]])        # (run_worker has set them already)
    print(json.dumps(run_driver(sys.argv[1])))
