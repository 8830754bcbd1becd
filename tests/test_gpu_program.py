"""Likelihoods given as HIP source, compiled at run time and called from a kernel of the engine's own (smcmi_program_* /
smcmi_set_likelihood_program / Engine.set_likelihood_program / HIPLikelihood).

The sources below use exactly rounded operations only (-, *, +, /, comparisons; constants such as the Gaussian's c0 arrive through `par`)
and the library compiles them with -ffp-contract=off, so a HOST-callback run with the same operations in numpy, in the same order, is an
independent reference that must agree bit for bit: every difference would be the engine's (the bounds gate, NaN -> -Inf and the
evaluation count inside the wrapper kernel instead of on the host).  This is the construction of tests/test_gpu_device_callback.py
(_gauss_batch, _run, _assert_same_bits), copied here.  Shapes: n = 2 085 = eight 256-row blocks and a 37-row tail (the last block has one
partial wavefront), d = 6, unless a test says otherwise.  Every source touches only theta[j * ld], j < d, data[0 .. rows * cols) and
par[0 .. n_par)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, D = 2085, 6
KWS = [dict(use_fixed_schedule=False, tempering_target=0.95),
       dict(use_fixed_schedule=True, n_phi=40, n_blocks=2, n_mh_steps=2, alpha=0.9)]

SIG = "(const double *theta, long long ld, int d, const double *data, long long rows, long long cols, const double *par, long long n_par)"

# data = the d means, par = { c0, 2 sigma^2 }: model.hpp's GAUSS_ISO order, as _gauss_batch
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


def _gauss_batch(m, sig):
    c0 = -0.5 * len(m) * math.log(2.0 * math.pi * sig * sig)

    def f(th):
        acc = np.zeros(th.shape[0])
        for k in range(th.shape[1]):                # the device's summation order (model.hpp loglik GAUSS_ISO)
            e = th[:, k] - m[k]
            acc += e * e
        return c0 - acc / (2.0 * sig * sig)
    return f


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
def gauss_host_runs():
    """the host-callback reference of the two whole runs, computed once"""
    spec, m, sig = _gauss_case()
    f = _gauss_batch(m, sig)
    return [_run(spec, N, D, 7, kw, lambda e: e.set_likelihood_callback(f, which=0)) for kw in KWS]


@pytest.mark.parametrize("case", [0, 1])
def test_a_program_run_is_the_host_callback_run_bit_for_bit(gauss_host_runs, case):
    """1. whole runs, adaptive and fixed with 2 blocks x 2 MH steps and a mixture proposal"""
    kw = KWS[case]
    spec, m, sig = _gauss_case()
    host = gauss_host_runs[case]
    dev = _run(spec, N, D, 7, kw, lambda e: e.set_likelihood_program(GAUSS_SRC, data=m.reshape(-1, 1), par=_gauss_par(m, sig), which=0))
    st = dev["st"]
    print("program: stages %d calls %d evaluations %d phases %r" % (dev["r"]["n_stages"], st["calls"], st["evaluations"], dev["ph"]))
    _assert_same_bits(host, dev)
    steps = kw.get("n_mh_steps", 1) * kw.get("n_blocks", 1)
    assert dev["r"]["n_stages"] > 5
    assert st["calls"] == steps * (dev["r"]["n_stages"] - 1)              # one launch per MH step x block
    assert st["evaluations"] == st["calls"] * N                            # every proposal is inside the bounds and was scored
    assert dev["ph"]["count_wait"] == 0.0 and dev["ph"]["callback"] == 0.0  # no host read per step, nothing of the user's on the host
    assert dev["ph"]["enqueue"] > 0.0


def test_the_function_is_called_on_exactly_the_in_bounds_rows():
    """2. wide proposals under uniform priors on [-0.5, 0.5]^3: many leave the bounds; the wrapper's gate keeps them from the function"""
    d = 3
    spec = models.gauss_spec(d)
    spec = dict(spec, bounds=[(-0.5, 0.5)] * d, priors=[("uniform", -0.5, 0.5)] * d)
    m, sig = np.asarray(spec["lik"][2]).ravel()[:d], float(spec["lik"][1][0])
    f = _gauss_batch(m, sig)
    kw = dict(use_fixed_schedule=True, n_phi=20, c=2.0)
    host = _run(spec, N, d, 3, kw, lambda e: e.set_likelihood_callback(f, which=0), max_stages=200)
    hs = host["st"]
    print("bounds (host): calls %d evaluations %d of %d" % (hs["calls"], hs["evaluations"], hs["calls"] * N))
    assert hs["calls"] == host["r"]["n_stages"] - 1 and 0 < hs["evaluations"] < hs["calls"] * N      # the reference itself skipped rows
    dev = _run(spec, N, d, 3, kw, lambda e: e.set_likelihood_program(GAUSS_SRC, data=m.reshape(-1, 1), par=_gauss_par(m, sig)), max_stages=200)
    st = dev["st"]
    print("bounds (program): calls %d evaluations %d" % (st["calls"], st["evaluations"]))
    _assert_same_bits(host, dev)
    assert st["calls"] == hs["calls"]
    assert st["evaluations"] == hs["evaluations"]


def test_nan_from_the_source_is_minus_inf_as_on_the_host():
    """3. 0 / 0 on half the space"""
    spec, m, sig = _gauss_case()
    base = _gauss_batch(m, sig)
    count = [0]

    def f(th):
        out = base(th)
        bad = th[:, 0] > -0.9
        count[0] += int(bad.sum())
        out[bad] = np.nan
        return out

    kw = dict(use_fixed_schedule=True, n_phi=25, n_mh_steps=2)
    host = _run(spec, N, D, 13, kw, lambda e: e.set_likelihood_callback(f, which=0))
    assert count[0] > 0
    dev = _run(spec, N, D, 13, kw, lambda e: e.set_likelihood_program(NAN_SRC, data=m.reshape(-1, 1), par=_gauss_par(m, sig) + [-0.9]))
    assert np.all(np.isfinite(dev["P"][:, D]))                        # no proposal with a NaN score was accepted
    _assert_same_bits(host, dev)
    assert dev["st"] == host["st"]


REJECT_SRC = "__device__ double loglik" + SIG + """ {
    if (theta[0] < par[1]) return par[2];
    double acc = 0.0;
    for (long long t = 0; t < rows; ++t) {
        const double e = (data[t] - theta[0]) - theta[ld];
        acc += e * e;
    }
    return par[0] * acc;
}
"""


def test_initial_draw_with_rejected_draws_is_the_host_callbacks_bit_for_bit():
    """4. a Gamma prior and a likelihood that is -Inf on a third of the draws: the redraw loop above the wrapper kernel against the host
    loop - cloud, attempts (the evaluation count) and the score column; initialize_likelihoods() and eval_cloud_callback() likewise"""
    import smc_jl_amd as S
    from smc_jl_amd.host import api

    data = np.full((5, 1), 2.5)

    def batch(th):
        acc = np.zeros(th.shape[0])
        for t in range(data.shape[0]):
            e = (data[t, 0] - th[:, 0]) - th[:, 1]
            acc += e * e
        out = -0.5 * acc
        out[th[:, 0] < 0.6] = -math.inf
        return out

    pars = [S.parameter("g", 1.0, (1e-8, 1e5), prior=S.Gamma(2.0, 1.0)), S.parameter("b", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 2.0))]
    n = N
    spec = api._spec_from(pars, ("host_callback", [], None, None), None)
    out = []
    for mode in ("host", "program"):
        eng = S.Engine(n, 2, seed=3, max_stages=4, store_history=False)
        eng.set_parameters(spec["priors"], spec["bounds"], spec["fixed"])
        if mode == "host":
            eng.set_likelihood_callback(batch, which=0)
        else:
            eng.set_likelihood_program(REJECT_SRC, data=data, par=[-0.5, 0.6, -math.inf], which=0)
        eng.set_likelihood("none", which=1)
        eng.init_from_prior()
        P = eng.download_cloud()
        st = eng.callback_stats()
        eng.initialize_likelihoods()
        P1 = eng.download_cloud()
        Q = P.copy(order="F")
        Q[:, 2] = 0.0
        Q[:, 4] = 7.0
        eng.upload_cloud(Q)
        eng.eval_cloud_callback(which=0, column=4)
        P2 = eng.download_cloud()
        eng.close()
        out.append((P, P1, P2, st))
    (Ph, P1h, P2h, sth), (Pd, P1d, P2d, std) = out
    assert np.all(np.isfinite(Ph[:, 2])) and np.all(Ph[:, 0] >= 0.6)
    assert np.array_equal(Ph, Pd) and np.array_equal(P1h, P1d) and np.array_equal(P2h, P2d)
    assert np.array_equal(P2d[:, 4], Pd[:, 2])                       # the requested column holds the scores
    print("initial draw: evaluations %d (host %d) for %d particles" % (std["evaluations"], sth["evaluations"], n))
    assert n < std["evaluations"] < 2 * n and std["evaluations"] == sth["evaluations"]   # each round scored only what it redrew


# every element of data and par with a weight of its own: element i of data weighs i + 1, entry k of par weighs k + 2
WEIGHTS_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    for (long long c = 0; c < cols; ++c)
        for (long long r = 0; r < rows; ++r) {
            const long long i = r + rows * c;
            acc += ((double)(i + 1) * data[i]) * theta[((r + c) % d) * ld];
        }
    for (long long k = 0; k < n_par; ++k) acc += ((double)(k + 2) * par[k]) * theta[(k % d) * ld];
    return acc;
}
"""


def _weights_ref(th, data, par):
    rows, cols = data.shape
    d = th.shape[1]
    acc = np.zeros(th.shape[0])
    for c in range(cols):
        for r in range(rows):
            i = r + rows * c
            acc += (float(i + 1) * data[r, c]) * th[:, (r + c) % d]
    for k in range(len(par)):
        acc += (float(k + 2) * par[k]) * th[:, k % d]
    return acc


def test_data_and_parameters_reach_the_function_per_handle():
    """5. a 7 x 3 data matrix and 4 parameters, each element with a weight of its own; one program on two handles with different data"""
    import smc_jl_amd as S

    rng = np.random.default_rng(11)
    spec, _, _ = _gauss_case()
    prog = S.Engine.compile_program(WEIGHTS_SRC)
    th = rng.normal(size=(N, D))
    Q = np.zeros((N, D + 5), order="F")
    Q[:, :D] = th
    Q[:, D] = 99.0
    par = rng.normal(size=4)
    engines, datas = [], []
    for k in range(2):
        data = rng.normal(size=(7, 3))
        e = S.Engine(N, D, seed=1, max_stages=4, store_history=False)
        e.set_parameters(spec["priors"], spec["bounds"], spec["fixed"])
        e.set_likelihood_program(prog, data=data, par=par, which=0)
        engines.append(e)
        datas.append(data)
    prog.close()                                                     # (the handles keep their own modules)
    for e, data in zip(engines, datas):
        e.upload_cloud(Q)
        e.eval_cloud_callback(which=0)
        got = e.download_cloud()[:, D]
        want = _weights_ref(th, data, par)
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert e.callback_stats()["evaluations"] >= N
    assert not np.array_equal(_weights_ref(th, datas[0], par), _weights_ref(th, datas[1], par))
    for e in engines:
        e.close()


REG_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    for (long long t = 0; t < rows; ++t) {
        const double e = (data[t] - theta[0]) - theta[ld] * data[t + rows];
        acc += e * e;
    }
    return par[0] - par[1] * acc;
}
"""


def _reg_batch():
    def f(th, dat):                                  # th (m, 2), dat (T, 2) = [y X]
        acc = np.zeros(th.shape[0])
        for t in range(dat.shape[0]):
            e = (dat[t, 0] - th[:, 0]) - th[:, 1] * dat[t, 1]
            acc += e * e
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * acc
    f.batched = True
    return f


class _RegLik:
    """HIPLikelihood whose c0 depends on the vintage's length: par = { -T/2 log(2 pi), 1/2 }"""

    def __init__(self, T):
        import smc_jl_amd as S

        self.lik = S.HIPLikelihood(REG_SRC, par=[-0.5 * T * math.log(2.0 * math.pi), 0.5])


def test_tempered_update_with_programs_on_both_vintages():
    """6. the scenario and the sizes of test_tempered_update_with_torch_likelihoods_on_both_vintages; the host pair is the same operations in
    numpy, so the comparison is bit for bit"""
    import smc_jl_amd as S

    rng = np.random.default_rng(0)
    X = rng.normal(size=60)
    y = 1.0 + 1.0 * X + rng.normal(size=60)
    data = np.column_stack([y, X])
    f = _reg_batch()
    pars = [S.parameter("a", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0)), S.parameter("b", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0))]
    kw = dict(n_parts=4000, n_phi=50, verbose="none", seed=5)
    c_old, _, _ = S.smc(f, pars, data[:30], **kw)
    c_py, w_py, W_py = S.smc(f, pars, data, old_data=data[:30], old_cloud=c_old, **kw)
    c_p, w_p, W_p = S.smc(_RegLik(60).lik, pars, data, old_data=data[:30], old_loglikelihood=_RegLik(30).lik, old_cloud=c_old, **kw)
    print("tempered update: log-MDD %.17g (programs) %.17g (host callbacks)" % (c_p.logmdd, c_py.logmdd))
    assert c_p.stage_index == c_py.stage_index == 50
    assert c_p.logmdd == c_py.logmdd
    assert np.array_equal(c_p.particles, c_py.particles)
    assert np.array_equal(w_p, w_py) and np.array_equal(W_p, W_py)
    # a host callback next to a program is refused before anything runs
    with pytest.raises(NotImplementedError, match="both"):
        S.smc(f, pars, data, old_data=data[:30], old_loglikelihood=_RegLik(30).lik, old_cloud=c_old, **kw)


def test_run_group_of_two_handles_with_the_program():
    """7. two shards of one population on one GPU, each handle with the program, against the same two handles with host callbacks on the
    same operations - the comparison of the device-callback group test (a group adds the shards' sums in another order than one handle
    adds its blocks', so the group's own host-callback run is the reference that can agree bit for bit)"""
    from smc_jl_amd import Engine, run_group

    d, world, seed = 5, 2, 21
    nl = N
    n = nl * world
    base = models.gauss_spec(d=d)
    m, sig = np.asarray(base["lik"][2]).ravel(), float(base["lik"][1][0])
    f = _gauss_batch(m, sig)
    prog = Engine.compile_program(GAUSS_SRC)
    kw = dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, n_mh_steps=2, alpha=0.9)
    out = []
    for mode in ("host", "program"):
        engs = []
        for r in range(world):
            e = Engine(n, d, seed=seed, max_stages=600, store_history=False, n_local=nl, gid0=r * nl)
            e.set_model(base)
            e.init_from_prior()
            P0 = e.download_cloud()
            if mode == "host":
                e.set_likelihood_callback(f, which=0)
            else:
                e.set_likelihood_program(prog, data=m.reshape(-1, 1), par=_gauss_par(m, sig), which=0)
            e.upload_cloud(P0)
            engs.append(e)
        r = run_group(engs, **kw)
        rec = engs[0].stage_records(r["n_stages"])
        P = np.concatenate([e.download_cloud() for e in engs], axis=0)
        st = [e.callback_stats() for e in engs]
        for e in engs:
            e.close()
        out.append((r, rec, P, st))
    prog.close()
    (r0, rec0, P0_, st0), (r1, rec1, P1_, st1) = out
    assert r0["n_stages"] == r1["n_stages"] and r0["resamples"] == r1["resamples"] and r0["logmdd"] == r1["logmdd"]
    for k in rec0:
        assert np.array_equal(rec0[k], rec1[k]), k
    assert np.array_equal(P0_, P1_)
    assert all(s["calls"] == 4 * (r1["n_stages"] - 1) for s in st1)      # 2 MH steps x 2 blocks per stage, per handle
    assert [s["evaluations"] for s in st1] == [s["evaluations"] for s in st0]
    assert all(s["evaluations"] == s["calls"] * nl for s in st1)


def test_replacement_and_lifetime():
    """8. family -> program -> device callback -> program -> NULL on one handle, each followed by a 5-stage run that equals its own
    reference (after NULL the handle has no likelihood: the run says so, and the family runs again); the program destroyed right after
    it was registered; 20 create / register / destroy cycles"""
    import torch

    from smc_jl_amd import Engine, _lib

    spec, m, sig = _gauss_case()
    f = _gauss_batch(m, sig)
    kw = dict(use_fixed_schedule=True, n_phi=5)
    fam = _run(spec, N, D, 9, kw, lambda x: None, max_stages=8, history=False)       # (uploads its starting cloud like the others)
    host = _run(spec, N, D, 9, kw, lambda e: e.set_likelihood_callback(f, which=0), max_stages=8, history=False)
    data, par = m.reshape(-1, 1), _gauss_par(m, sig)

    def staged(th):
        return torch.as_tensor(np.asarray(f(th.cpu().numpy()), dtype=np.float64), device=th.device)

    e = Engine(N, D, seed=9, max_stages=8, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()

    def run_and_compare(ref):
        e.upload_cloud(P0)
        r = e.run(**kw)
        assert r["n_stages"] == 5 and r["logmdd"] == ref["r"]["logmdd"] and np.array_equal(e.download_cloud(), ref["P"])

    run_and_compare(fam)
    e.set_likelihood_program(GAUSS_SRC, data=data, par=par)          # (compiled, registered, and the program destroyed at once)
    run_and_compare(host)
    e.set_likelihood_device(staged)
    run_and_compare(host)
    e.set_likelihood_program(GAUSS_SRC, data=data, par=par)
    run_and_compare(host)
    assert e.callback_stats() == dict(calls=4, evaluations=4 * N)
    e.set_likelihood_program(None)
    e.upload_cloud(P0)
    with pytest.raises(_lib.SMCMIError) as ei:
        e.run(**kw)
    assert ei.value.code == -8                                        # SMCMI_ERR_STATE: no likelihood set
    lk = spec["lik"]
    e.set_likelihood(lk[0], lk[1], lk[2], lk[3], which=0)
    run_and_compare(fam)
    # a program replaced by a host callback, and the other way round
    e.set_likelihood_program(GAUSS_SRC, data=data, par=par)
    e.set_likelihood_callback(f)
    run_and_compare(host)
    assert e.callback_phases()["callback"] > 0.0                      # (the host path ran)
    e.close()
    prog = Engine.compile_program(GAUSS_SRC)
    for _ in range(20):
        x = Engine(N, D, seed=1, max_stages=4, store_history=False)
        x.set_model(spec)
        x.set_likelihood_program(prog, data=data, par=par, which=0)
        x.set_likelihood_program(prog, data=data, par=par, which=1)
        x.close()
    prog.close()


def test_refusals():
    """9. sharded and ensemble runs refuse a handle with a program and the handle runs afterwards; a host callback on the other vintage;
    a program that did not compile cannot be registered and the handle's previous likelihood still runs"""
    from smc_jl_amd import Engine, _lib, run_ensemble

    UNSUPPORTED, STATE, ARG, COMPILE = -7, -8, -1, -11
    spec, m, sig = _gauss_case()
    data, par = m.reshape(-1, 1), _gauss_par(m, sig)
    kw = dict(use_fixed_schedule=True, n_phi=5)
    host = _run(spec, N, D, 9, kw, lambda x: x.set_likelihood_callback(_gauss_batch(m, sig), which=0), max_stages=8, history=False)
    fam = _run(spec, N, D, 9, kw, lambda x: None, max_stages=8, history=False)       # (uploads its starting cloud like the others)
    e = Engine(N, D, seed=9, max_stages=8, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()
    L = _lib.lib()
    # a program with a compile error: SMCMI_ERR_ARG, the family stays
    p = C.c_void_p()
    assert L.smcmi_program_compile(b"__device__ double loglik(const double *theta) { return theta[0] }", None, None, C.byref(p)) == COMPILE
    assert p.value
    assert L.smcmi_set_likelihood_program(e._h, 0, p, None, 0, 0, None, 0) == ARG
    L.smcmi_program_destroy(p)
    e.upload_cloud(P0)
    r = e.run(**kw)
    assert r["logmdd"] == fam["r"]["logmdd"] and np.array_equal(e.download_cloud(), fam["P"])
    # the world-1 host communicator: smcmi_run_sharded refuses the program
    e.set_likelihood_program(GAUSS_SRC, data=data, par=par)
    e.upload_cloud(P0)
    with pytest.raises(_lib.SMCMIError) as ei:
        run_ensemble([e], **kw)
    assert ei.value.code == UNSUPPORTED
    e.comm_init_host(0, 1, allgather=lambda send: send)
    with pytest.raises(_lib.SMCMIError) as ei:
        e.run_sharded(**kw)
    assert ei.value.code == UNSUPPORTED
    r = e.run(**kw)
    assert r["logmdd"] == host["r"]["logmdd"] and np.array_equal(e.download_cloud(), host["P"])
    # a host callback on the other vintage: SMCMI_ERR_STATE from the run; a device callback there is accepted by the same check
    e.set_likelihood_callback(_gauss_batch(m, sig), which=1)
    e.upload_cloud(P0)
    with pytest.raises(RuntimeError) as ei:
        e.run(**kw)
    assert getattr(ei.value, "code", None) == STATE
    e.close()


def _result_line(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "OK" in p.stdout
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])


def test_c_example_with_the_source_as_a_string_matches_the_c_callback_example():
    """10a. examples/c_abi_program.c (gcc only; the likelihood a string literal) against examples/c_abi_callback.c on the same seed.  The
    source's arithmetic is the C callback's - the same IEEE operations in the same order, contraction off in both - so the fields
    test_hip_example_with_a_user_kernel_matches_the_c_callback_example compares (stages, resamples, log-MDD printed with 17 digits) are
    compared exactly, as there.  Both run 20 000 particles (the examples take n as their argument) to keep the test short."""
    lib = os.path.join(ROOT, "smc.jl_amd", "csrc")
    inc = os.path.join(ROOT, "include")
    exe_c = os.path.join(ROOT, "examples", "c_abi_callback")
    exe_p = os.path.join(ROOT, "examples", "c_abi_program")
    for exe in (exe_c, exe_p):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-ffp-contract=off", "-I", inc, "-o", exe, exe + ".c", "-L", lib, "-lsmcmi", "-lm",
                               "-Wl,-rpath," + lib])
    a, b = _result_line([exe_c, "20000"]), _result_line([exe_p, "20000"])
    print("host callback %r\nprogram %r" % (a["callback"], b["callback"]))
    assert a["n_parts"] == b["n_parts"] == 20000
    for sec in ("device", "callback"):
        for k in ("n_stages", "resamples", "logmdd"):
            assert a[sec][k] == b[sec][k], (sec, k, a[sec][k], b[sec][k])
    assert b["callback"]["calls"] == b["callback"]["n_stages"] - 1


def test_smc_with_a_hip_likelihood_on_the_regression_example():
    """10b. examples/estimate_regression.py's model through smc(HIPLikelihood(source), parameters, data) against the Python callable, with
    the tolerances of test_smc_with_a_torch_likelihood_on_the_regression_example (the callable sums with a dot product)"""
    import smc_jl_amd as S

    data = np.load(os.path.join(ROOT, "tests", "golden", "reg_data.npz"))["data"]          # 100 x 2 = [y X]
    pars = [S.parameter("α1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False),
            S.parameter("β1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False)]

    def loglik(theta, dat):
        e = dat[:, 0] - theta[0] - theta[1] * dat[:, 1]
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * float(e @ e)

    kw = dict(n_parts=1000, use_fixed_schedule=True, seed=1793, verbose="none")
    c_py, _, _ = S.smc(loglik, pars, data, **kw)
    c_h, _, _ = S.smc(_RegLik(data.shape[0]).lik, pars, data, **kw)
    print("regression: mean %r (HIP source) %r (python)" % (S.weighted_mean(c_h), S.weighted_mean(c_py)))
    assert c_h.stage_index == c_py.stage_index
    np.testing.assert_allclose(S.weighted_mean(c_h), S.weighted_mean(c_py), atol=1e-6)
    assert abs(S.weighted_mean(c_h)[0] - 1.00018685) < 0.05 and abs(S.weighted_mean(c_h)[1] - 0.99936133) < 0.1
    with pytest.raises(NotImplementedError, match="HIPLikelihood"):
        S.smc_ensemble(_RegLik(data.shape[0]).lik, pars, data, [1, 2], n_parts=1000)
