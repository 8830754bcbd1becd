"""Fused run-time compiled likelihoods (smcmi_program_compile_ex with SMCMI_PROGRAM_FUSED / Engine.compile_program(fused=True) /
HIPLikelihood(fused=True)): the user's function compiled into the generic mutation kernel, one launch per mutated stage.

The reference of every test is the SPLIT program run (fused=False) of the same source - propose, wrapper kernel, accept per MH step x block -
which tests/test_gpu_program.py holds to the host callback.  The sources use exactly rounded operations only and both paths compile with
-ffp-contract=off, so the comparison is _assert_same_bits: no tolerance.  Helpers and sources are those of tests/test_gpu_program.py, copied.
Two distinct sources are compiled fused in this file, three compiles in all: GAUSS_SRC and NAN_SRC once per module, and GAUSS_SRC once
more where the test is about a program the binding compiles and destroys by itself."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, D = 2085, 6
KWS = [dict(use_fixed_schedule=False, tempering_target=0.95),
       dict(use_fixed_schedule=True, n_phi=40, n_blocks=2, n_mh_steps=2, alpha=0.9)]

SIG = "(const double *theta, long long ld, int d, const double *data, long long rows, long long cols, const double *par, long long n_par)"

# data = the d means, par = { c0, 2 sigma^2 }: model.hpp's GAUSS_ISO order
GAUSS_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const double e = theta[k * ld] - data[k];
        acc += e * e;
    }
    return par[0] - acc / par[1];
}
"""
# ... NaN where theta_0 > par[2]
NAN_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const double e = theta[k * ld] - data[k];
        acc += e * e;
    }
    const double zero = par[0] - par[0];
    if (theta[0] > par[2]) return zero / zero;
    return par[0] - acc / par[1];
}
"""


def _gauss_par(m, sig):
    return [-0.5 * len(m) * math.log(2.0 * math.pi * sig * sig), 2.0 * sig * sig]


def _run(spec, n, d, seed, kw, register, max_stages=800, history=True):
    """initial cloud by the device family (the same for every mode), then `register(engine)` swaps the likelihood, then the run"""
    from smc_jl_amd import Engine

    e = Engine(n, d, seed=seed, max_stages=max_stages, store_history=history)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()
    if register is not None:
        register(e)
        e.upload_cloud(P0)
    r = e.run(**kw)
    out = dict(r=r, rec=e.stage_records(r["n_stages"]), P=e.download_cloud(), st=e.callback_stats(), ph=e.callback_phases(),
               hist=e.history(r["n_stages"]) if history else None)
    e.close()
    return out


def _assert_same_bits(a, b):
    assert a["r"]["n_stages"] == b["r"]["n_stages"] and a["r"]["resamples"] == b["r"]["resamples"]
    assert a["r"]["logmdd"] == b["r"]["logmdd"]
    for k in a["rec"]:
        assert np.array_equal(a["rec"][k], b["rec"][k]), k
    assert np.array_equal(a["P"], b["P"])
    if a["hist"] is not None:
        assert np.array_equal(a["hist"][0], b["hist"][0]) and np.array_equal(a["hist"][1], b["hist"][1])


def _gauss_case(d=D):
    spec = models.gauss_spec(d)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    return spec, m, sig


@pytest.fixture(scope="module")
def progs():
    """every program of this file, compiled once: (source name, fused?) -> Program"""
    import smc_jl_amd as S

    p = {("gauss", False): S.Engine.compile_program(GAUSS_SRC), ("gauss", True): S.Engine.compile_program(GAUSS_SRC, fused=True),
         ("nan", False): S.Engine.compile_program(NAN_SRC), ("nan", True): S.Engine.compile_program(NAN_SRC, fused=True)}
    for (name, fused), prog in p.items():
        assert prog.fused == fused, name
    yield p
    for prog in p.values():
        prog.close()


def _pair(progs, name, spec, n, d, seed, kw, data, par, **run_kw):
    """(split run, fused run) of program `name` on the same starting cloud"""
    out = []
    for fused in (False, True):
        out.append(_run(spec, n, d, seed, kw, lambda e: e.set_likelihood_program(progs[(name, fused)], data=data, par=par, which=0), **run_kw))
    return out


@pytest.mark.parametrize("case", [0, 1])
def test_a_fused_run_is_the_split_run_bit_for_bit_in_one_launch_per_stage(progs, case):
    """1. whole runs, n = 2 085 (eight 256-row blocks and a 37-row tail), d = 6: adaptive, and fixed with 2 blocks x 2 MH steps, alpha = 0.9"""
    kw = KWS[case]
    spec, m, sig = _gauss_case()
    split, fused = _pair(progs, "gauss", spec, N, D, 7, kw, m.reshape(-1, 1), _gauss_par(m, sig))
    print("fused: stages %d calls %d evaluations %d phases %r" % (fused["r"]["n_stages"], fused["st"]["calls"], fused["st"]["evaluations"], fused["ph"]))
    print("split: stages %d calls %d evaluations %d phases %r" % (split["r"]["n_stages"], split["st"]["calls"], split["st"]["evaluations"], split["ph"]))
    _assert_same_bits(split, fused)
    steps = kw.get("n_mh_steps", 1) * kw.get("n_blocks", 1)
    stages = fused["r"]["n_stages"]
    assert stages > 5
    assert fused["st"]["calls"] == stages - 1
    assert split["st"]["calls"] == steps * (stages - 1)
    assert fused["st"]["evaluations"] == split["st"]["evaluations"] == steps * (stages - 1) * N
    assert fused["ph"]["count_wait"] == 0.0 and fused["ph"]["callback"] == 0.0 and fused["ph"]["enqueue"] > 0.0


@pytest.mark.parametrize("d", [12, 14])
def test_either_side_of_the_staged_constants_limit(progs, d):
    """2. d = 12 and 14 (above the register kernels' range; the proposal constants are staged in LDS up to n_para = 13), n = 600, 3 blocks"""
    n = 600
    spec, m, sig = _gauss_case(d)
    kw = dict(use_fixed_schedule=True, n_phi=20, n_blocks=3)
    split, fused = _pair(progs, "gauss", spec, n, d, 5, kw, m.reshape(-1, 1), _gauss_par(m, sig), max_stages=40)
    _assert_same_bits(split, fused)
    assert fused["st"]["evaluations"] == split["st"]["evaluations"] == 3 * 19 * n
    assert fused["st"]["calls"] == 19 and split["st"]["calls"] == 3 * 19


def test_forty_parameters_at_the_largest_block_stride(progs):
    """3. d = 40, n = 300, 4 blocks: 64-thread blocks whose per-thread vectors ask for more than 64 KiB of dynamic LDS.  (A flat likelihood,
    sigma = 2 under priors of standard deviation 1: with config 2's sigma = 0.25 under priors of 5 the 12-stage schedule leaves 300
    particles in 40 dimensions with an effective sample size near 1, and the split reference itself ends in a PosDefException.)"""
    d, n = 40, 300
    spec = models.gauss_spec(d, sigma=2.0, prior_sd=1.0)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    kw = dict(use_fixed_schedule=True, n_phi=12, n_blocks=4)
    split, fused = _pair(progs, "gauss", spec, n, d, 5, kw, m.reshape(-1, 1), _gauss_par(m, sig), max_stages=40)
    _assert_same_bits(split, fused)
    assert fused["st"]["calls"] == 11 and fused["st"]["evaluations"] == split["st"]["evaluations"]


def test_the_gate_keeps_out_of_bounds_proposals_from_the_function(progs):
    """4. test_the_function_is_called_on_exactly_the_in_bounds_rows's case: uniform priors on [-0.5, 0.5]^3 and c = 2.0"""
    d = 3
    spec = models.gauss_spec(d)
    spec = dict(spec, bounds=[(-0.5, 0.5)] * d, priors=[("uniform", -0.5, 0.5)] * d)
    m, sig = np.asarray(spec["lik"][2]).ravel()[:d], float(spec["lik"][1][0])
    kw = dict(use_fixed_schedule=True, n_phi=20, c=2.0)
    split, fused = _pair(progs, "gauss", spec, N, d, 3, kw, m.reshape(-1, 1), _gauss_par(m, sig), max_stages=200)
    print("bounds: evaluations %d (fused) %d (split) of %d" % (fused["st"]["evaluations"], split["st"]["evaluations"], 19 * N))
    _assert_same_bits(split, fused)
    assert fused["st"]["evaluations"] == split["st"]["evaluations"]
    assert 0 < fused["st"]["evaluations"] < (fused["r"]["n_stages"] - 1) * N


def test_nan_from_the_source_is_minus_inf_as_in_the_split_run(progs):
    """5. 0 / 0 on half the space"""
    spec, m, sig = _gauss_case()
    kw = dict(use_fixed_schedule=True, n_phi=25, n_mh_steps=2)
    split, fused = _pair(progs, "nan", spec, N, D, 13, kw, m.reshape(-1, 1), _gauss_par(m, sig) + [-0.9])
    assert np.all(np.isfinite(fused["P"][:, D]))
    _assert_same_bits(split, fused)
    assert fused["st"]["evaluations"] == split["st"]["evaluations"]


def test_a_tempered_update_keeps_the_split_path(progs):
    """6a. the fused program at the new vintage and a program at the old one (the Gaussian around other means): the run is the split
    run, launch for launch"""
    import smc_jl_amd as S

    spec, m, sig = _gauss_case()
    m_old = 0.5 * m
    par = _gauss_par(m, sig)
    kw = dict(use_fixed_schedule=True, n_phi=12)
    out = []
    for fused in (False, True):
        e = S.Engine(N, D, seed=5, max_stages=20, store_history=False)
        e.set_model(spec)
        e.init_from_prior()
        P0 = e.download_cloud()
        e.set_likelihood_program(progs[("gauss", fused)], data=m.reshape(-1, 1), par=par, which=0)
        e.set_likelihood_program(progs[("gauss", False)], data=m_old.reshape(-1, 1), par=par, which=1)
        e.upload_cloud(P0)
        e.initialize_likelihoods()
        r = e.run(**kw)
        out.append((r, e.download_cloud(), e.callback_stats()))
        e.close()
    (r0, P0_, st0), (r1, P1_, st1) = out
    assert r0["n_stages"] == r1["n_stages"] == 12 and r0["logmdd"] == r1["logmdd"]
    assert np.array_equal(P0_, P1_)
    assert np.any(P1_[:, D + 2] != 0.0)                              # (the old vintage was scored: the update is tempered)
    assert st0 == st1 and st1["calls"] == 2 * 11                     # the new and the old vintage's wrapper launch per stage


def test_init_from_prior_and_eval_cloud_with_a_fused_program_are_the_plain_programs(progs):
    """6b. the stand-alone entry points run a fused program through its wrapper kernel"""
    import smc_jl_amd as S

    spec, m, sig = _gauss_case()
    out = []
    for fused in (False, True):
        e = S.Engine(N, D, seed=3, max_stages=4, store_history=False)
        e.set_parameters(spec["priors"], spec["bounds"], spec["fixed"])
        e.set_likelihood_program(progs[("gauss", fused)], data=m.reshape(-1, 1), par=_gauss_par(m, sig), which=0)
        e.set_likelihood("none", which=1)
        e.init_from_prior()
        P = e.download_cloud()
        st = e.callback_stats()
        Q = P.copy(order="F")
        Q[:, D] = 7.0
        e.upload_cloud(Q)
        e.eval_cloud_callback(which=0)
        out.append((P, st, e.download_cloud()))
        e.close()
    (Pa, sta, Qa), (Pb, stb, Qb) = out
    assert np.array_equal(Pa, Pb) and np.array_equal(Qa, Qb) and sta == stb
    assert np.array_equal(Qb[:, D], Pb[:, D]) and sta["evaluations"] >= N


def test_lifetime_and_replacement(progs):
    """7. a fused program destroyed right after registration; one fused program on two handles with different data; a fused program
    replaced by a device family and back - a fresh run after each equals its reference"""
    import smc_jl_amd as S

    spec, m, sig = _gauss_case()
    kw = dict(use_fixed_schedule=True, n_phi=6, n_blocks=2)
    data, par = m.reshape(-1, 1), _gauss_par(m, sig)
    data2 = data + 0.25
    fam = _run(spec, N, D, 9, kw, lambda x: None, max_stages=8, history=False)
    ref = _run(spec, N, D, 9, kw, lambda e: e.set_likelihood_program(progs[("gauss", False)], data=data, par=par), max_stages=8, history=False)
    ref2 = _run(spec, N, D, 9, kw, lambda e: e.set_likelihood_program(progs[("gauss", False)], data=data2, par=par), max_stages=8, history=False)
    assert not np.array_equal(ref["P"], ref2["P"])

    def same(a, b):
        assert a["r"]["n_stages"] == b["r"]["n_stages"] == 6 and a["r"]["logmdd"] == b["r"]["logmdd"] and np.array_equal(a["P"], b["P"])

    # (source text: the binding compiles it, registers it and destroys the program before it returns)
    got = _run(spec, N, D, 9, kw, lambda e: e.set_likelihood_program(GAUSS_SRC, data=data, par=par, fused=True), max_stages=8, history=False)
    same(got, ref)
    assert got["st"]["calls"] == 5
    # one program, two handles, different data
    same(_run(spec, N, D, 9, kw, lambda e: e.set_likelihood_program(progs[("gauss", True)], data=data, par=par), max_stages=8, history=False), ref)
    same(_run(spec, N, D, 9, kw, lambda e: e.set_likelihood_program(progs[("gauss", True)], data=data2, par=par), max_stages=8, history=False), ref2)
    # fused program -> device family -> fused program on one handle
    e = S.Engine(N, D, seed=9, max_stages=8, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()

    def run_and_compare(want):
        e.upload_cloud(P0)
        r = e.run(**kw)
        assert r["n_stages"] == 6 and r["logmdd"] == want["r"]["logmdd"] and np.array_equal(e.download_cloud(), want["P"])

    e.set_likelihood_program(progs[("gauss", True)], data=data, par=par)
    run_and_compare(ref)
    lk = spec["lik"]
    e.set_likelihood(lk[0], lk[1], lk[2], lk[3], which=0)
    run_and_compare(fam)
    e.set_likelihood_program(progs[("gauss", True)], data=data, par=par)
    run_and_compare(ref)
    assert e.callback_stats() == dict(calls=5, evaluations=2 * 5 * N)
    e.close()


def test_run_group_of_two_handles_with_the_fused_program(progs):
    """8. two shards of 1 040 particles on one GPU, each handle with the fused program, against the same group with the split program - NOT
    against a one-handle run of 2 080 particles: a group adds the shards' sums in another order than one handle adds its blocks', so no
    group run, split or fused, has a one-handle run's bits (tests/test_gpu_program.py compares its group the same way), and the group's
    own split run is the reference that can agree bit for bit"""
    from smc_jl_amd import Engine, run_group

    d, world, seed, nl = 5, 2, 21, 1040
    n = nl * world
    base = models.gauss_spec(d=d)
    m, sig = np.asarray(base["lik"][2]).ravel(), float(base["lik"][1][0])
    kw = dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, n_mh_steps=2, alpha=0.9)
    out = []
    for fused in (False, True):
        engs = []
        for r in range(world):
            e = Engine(n, d, seed=seed, max_stages=600, store_history=False, n_local=nl, gid0=r * nl)
            e.set_model(base)
            e.init_from_prior()
            P0 = e.download_cloud()
            e.set_likelihood_program(progs[("gauss", fused)], data=m.reshape(-1, 1), par=_gauss_par(m, sig), which=0)
            e.upload_cloud(P0)
            engs.append(e)
        r = run_group(engs, **kw)
        rec = engs[0].stage_records(r["n_stages"])
        P = np.concatenate([e.download_cloud() for e in engs], axis=0)
        st = [e.callback_stats() for e in engs]
        for e in engs:
            e.close()
        out.append((r, rec, P, st))
    (r0, rec0, P0_, st0), (r1, rec1, P1_, st1) = out
    assert r0["n_stages"] == r1["n_stages"] and r0["resamples"] == r1["resamples"] and r0["logmdd"] == r1["logmdd"]
    for k in rec0:
        assert np.array_equal(rec0[k], rec1[k]), k
    assert np.array_equal(P0_, P1_)
    assert all(s["calls"] == r1["n_stages"] - 1 for s in st1)            # the group fuses: one launch per stage and handle
    assert [s["evaluations"] for s in st1] == [s["evaluations"] for s in st0]


def test_smc_with_a_fused_hip_likelihood():
    """9. smc(HIPLikelihood(GAUSS_SRC, fused=True), ...) against smc(HIPLikelihood(GAUSS_SRC), ...)"""
    import smc_jl_amd as S

    d = 4
    m = np.linspace(-1.0, 1.0, d)
    pars = [S.parameter("p%d" % k, 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 5.0)) for k in range(d)]
    kw = dict(n_parts=1000, n_phi=15, use_fixed_schedule=True, seed=11, verbose="none")
    res = []
    for fused in (False, True):
        lik = S.HIPLikelihood(GAUSS_SRC, par=_gauss_par(m, 0.25), fused=fused)
        assert lik.program().fused == fused
        res.append(S.smc(lik, pars, m.reshape(-1, 1), **kw))
    (ca, wa, Wa), (cb, wb, Wb) = res
    assert ca.stage_index == cb.stage_index == 15 and ca.logmdd == cb.logmdd
    assert np.array_equal(ca.particles, cb.particles) and np.array_equal(wa, wb) and np.array_equal(Wa, Wb)


_AHEAD_WORKER = """
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests import test_gpu_program_fused as T
import smc_jl_amd as S
spec, m, sig = T._gauss_case()
progs = {False: S.Engine.compile_program(T.GAUSS_SRC), True: S.Engine.compile_program(T.GAUSS_SRC, fused=True)}
for kw in T.KWS + [dict(use_fixed_schedule=False, tempering_target=0.95, solver_passes=1, phi_rtol=-1.0)]:
    runs = [T._run(spec, T.N, T.D, 7, kw, lambda e: e.set_likelihood_program(progs[f], data=m.reshape(-1, 1), par=T._gauss_par(m, sig)))
            for f in (False, True)]
    T._assert_same_bits(*runs)
    stages = runs[1]["r"]["n_stages"]
    assert runs[1]["st"]["calls"] == stages - 1 and runs[1]["st"]["evaluations"] == runs[0]["st"]["evaluations"], (runs[0]["st"], runs[1]["st"])
    print("stages %%d solver stalls %%d" %% (stages, runs[1]["r"]["solver_stalls"]))
assert runs[1]["r"]["solver_stalls"] > 0          # (the last configuration: launches sent ahead were dropped and repeated)
print("AHEAD OK")
"""


def test_the_launch_ahead_of_the_verdict_gives_the_same_bits():
    """10. SMCMI_FUSED_AHEAD=1 (read once per process, hence the child): the fused launch goes out before the stage's verdict is read, no-ops
    on a stage that did not go ahead and is repeated after a resumed stall.  Both entries of KWS, and an adaptive run with one solver pass
    per stage and adjacent-float brackets, which stalls; calls count the stages that were mutated, not the launches"""
    p = subprocess.run([sys.executable, "-c", _AHEAD_WORKER % dict(root=ROOT)], env=dict(os.environ, SMCMI_FUSED_AHEAD="1"), capture_output=True, text=True,
                       timeout=300)
    print(p.stdout[-600:])
    assert p.returncode == 0 and "AHEAD OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
