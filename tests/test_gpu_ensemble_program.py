"""smcmi_run_ensemble with members that carry a likelihood compiled from HIP source FOR ENSEMBLES (smcmi_program_compile_ensemble /
Engine.compile_program(ensemble_para=d) / HIPLikelihood(ensemble=True)) on a real MI355X: the user's function called from inside the
ensemble kernel, one launch and one workgroup per member.

The reference of every member is a solo smcmi_run of a handle with the SAME code object registered - the split path through the wrapper
kernel - from the same cloud with the same seed.  Tolerances are those of tests/test_gpu_ensemble.py::assert_same_run for ensemble against
solo (copied): stage count, resample count and flags equal; schedule, ESS and c to rtol 1e-9; acceptance history to atol 3 / n + 1e-12;
log-MDD to 1e-8 absolute; clouds to rtol 1e-7, atol 1e-9.
All of these fail on a library without the entry point."""
import math
import os

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -7
SIG = "(const double *theta, long long ld, int d, const double *data, long long rows, long long cols, const double *par, long long n_par)"
# config 2's isotropic Gaussian: data = m (d x 1), par = { c0, 2 sigma^2 }
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
# ... +1e300 where any theta lies outside [par[2], par[3]]: the engine's bounds - a value no run survives if the function is ever asked there
BOUNDS_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    bool out = false;
    for (int k = 0; k < d; ++k) {
        const double x = theta[k * ld], e = x - data[k];
        out = out || x < par[2] || x > par[3];
        acc += e * e;
    }
    if (out) return 1e300;
    return par[0] - acc / par[1];
}
"""
# the regression example (tests/test_gpu_program.py REG_SRC): data = [y X] (rows x 2), par = { -rows / 2 log(2 pi), 1 / 2 }
REG_SRC = "__device__ double loglik" + SIG + """ {
    double acc = 0.0;
    for (long long t = 0; t < rows; ++t) {
        const double e = (data[t] - theta[0]) - theta[ld] * data[t + rows];
        acc += e * e;
    }
    return par[0] - par[1] * acc;
}
"""
SOURCES = dict(gauss=GAUSS_SRC, nan=NAN_SRC, bounds=BOUNDS_SRC, reg=REG_SRC)


@pytest.fixture(scope="module")
def progs():
    """progs(name, d): SOURCES[name] compiled for ensembles of d parameters (d = 0: a plain program), once per module"""
    import smc_jl_amd as S

    made = {}

    def get(name, d):
        if (name, d) not in made:
            made[(name, d)] = S.Engine.compile_program(SOURCES[name], ensemble_para=d) if d else S.Engine.compile_program(SOURCES[name])
            assert made[(name, d)].ensemble_para == d
        return made[(name, d)]

    yield get
    for p in made.values():
        p.close()


def gauss_par(spec, *more):
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    return m.reshape(-1, 1), [-0.5 * len(m) * math.log(2.0 * math.pi * sig * sig), 2.0 * sig * sig] + list(more)


def reg_par(rows):
    return [-0.5 * rows * math.log(2.0 * math.pi), 0.5]


def start_cloud(spec, n, seed):
    """the initial cloud by the spec's device family: the same start for the member and for its solo reference"""
    from smc_jl_amd import Engine

    e = Engine(n, len(spec["priors"]), seed=seed, max_stages=2, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()
    e.close()
    return P0


def prog_engine(spec, n, seed, max_stages, prog, data, par, P0, store_history=False):
    from smc_jl_amd import Engine

    e = Engine(n, len(spec["priors"]), seed=seed, max_stages=max_stages, store_history=store_history)
    e.set_model(spec)
    e.set_likelihood_program(prog, data=data, par=par, which=0)
    e.upload_cloud(P0)
    return e


def run_ensemble(engines, **kw):
    from smc_jl_amd import run_ensemble as f

    return f(engines, **kw)


def assert_same_run(n, what, got, ref):
    """got / ref: dict(n_stages, resamples, logmdd, schedule, ess, c_hist, accept_hist, resampled, particles)"""
    assert got["n_stages"] == ref["n_stages"], what
    assert got["resamples"] == ref["resamples"], what
    ns = got["n_stages"]
    np.testing.assert_array_equal(got["resampled"][:ns], ref["resampled"][:ns], err_msg=what)
    np.testing.assert_allclose(got["schedule"][:ns], ref["schedule"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["ess"][:ns], ref["ess"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["c_hist"][:ns], ref["c_hist"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["accept_hist"][:ns], ref["accept_hist"][:ns], atol=3.0 / n + 1e-12, rtol=0, err_msg=what)
    assert abs(got["logmdd"] - ref["logmdd"]) <= 1e-8, (what, got["logmdd"], ref["logmdd"])
    np.testing.assert_allclose(got["particles"], ref["particles"], rtol=1e-7, atol=1e-9, err_msg=what)


def collect(e, res):
    out = dict(n_stages=res["n_stages"], resamples=res["resamples"], logmdd=res["logmdd"], particles=e.download_cloud(), stats=e.callback_stats())
    out.update(e.stage_records(res["n_stages"]))
    return out


def bits(e, r):
    rec = e.stage_records(r["n_stages"])
    return (r["n_stages"], r["resamples"], r["logmdd"], r["c"], r["accept"], e.download_cloud().tobytes(),
            tuple(rec[k].tobytes() for k in ("schedule", "ess", "c_hist", "accept_hist", "resampled")))


class Member:
    """one member's description: everything an ensemble engine and its solo twin are made from"""

    def __init__(self, spec, n, seed, max_stages, prog, data, par, store_history=False):
        self.spec, self.n, self.seed, self.max_stages, self.prog, self.data, self.par = spec, n, seed, max_stages, prog, data, par
        self.store_history = store_history
        self.P0 = start_cloud(spec, n, seed)

    def engine(self):
        return prog_engine(self.spec, self.n, self.seed, self.max_stages, self.prog, self.data, self.par, self.P0, self.store_history)

    def solo(self, kw, keep=False):
        e = self.engine()
        out = collect(e, e.run(**kw))
        if keep:
            return e, out
        e.close()
        return out


def check_members(members, kw, what, keep=False):
    """the members as one ensemble, each against its solo run; returns the engines (keep) or closes them, and the members' collected runs"""
    es = [m.engine() for m in members]
    rs = run_ensemble(es, **kw)
    outs = []
    for k, (m, e, r) in enumerate(zip(members, es, rs)):
        assert r["status"] == 0 and r["call_status"] == 0, (what, k, r)
        got = collect(e, r)
        ref = m.solo(kw)
        print("%s member %d: stages %d log-MDD %.17g (ensemble) %.17g (solo), evaluations %d / %d" %
              (what, k, got["n_stages"], got["logmdd"], ref["logmdd"], got["stats"]["evaluations"], ref["stats"]["evaluations"]))
        assert_same_run(m.n, "%s member %d vs its solo run" % (what, k), got, ref)
        assert got["stats"]["calls"] == 1
        got["ref"] = ref
        outs.append(got)
    if not keep:
        for e in es:
            e.close()
    return es, rs, outs


def fixed_column_spec():
    spec = models.gauss_spec(d=6)
    spec["fixed"] = [0, 0, 1, 0, 0, 0]
    spec["priors"] = [("normal", 0.3 * k, 5.0) for k in range(6)]
    return spec


CELLS = {
    "gauss10_adaptive": (models.gauss_spec, 1000, [1, 2, 3], 400, dict(use_fixed_schedule=False, tempering_target=0.95), False),
    "gauss3_tail_of_9": (lambda: models.gauss_spec(d=3), 777, [11, 12, 13], 20, dict(n_phi=20, n_blocks=3, n_mh_steps=2, resampling_method="multinomial"), False),
    "gauss1_below_a_block": (lambda: models.gauss_spec(d=1), 200, [3, 4], 10, dict(n_phi=10), False),
    "gauss6_one_fixed_column": (fixed_column_spec, 600, [31, 32], 24, dict(n_phi=24, n_blocks=2), True),
}


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_members_equal_their_solo_runs(progs, cell):
    """1."""
    mk, n, seeds, ms, kw, hist = CELLS[cell]
    spec = mk()
    d = len(spec["priors"])
    data, par = gauss_par(spec)
    members = [Member(spec, n, s, ms, progs("gauss", d), data, par, store_history=hist) for s in seeds]
    es, rs, outs = check_members(members, kw, cell, keep=hist)
    assert len({o["logmdd"] for o in outs}) == len(seeds)
    assert all(o["n_stages"] > 5 for o in outs)
    if hist:                         # w / W as well, and the fixed column never moves
        for m, e, r, o in zip(members, es, rs, outs):
            tw, _ = m.solo(kw, keep=True)
            w, W = e.history(r["n_stages"])
            ws, Ws = tw.history(r["n_stages"])
            np.testing.assert_allclose(w, ws, rtol=1e-7, atol=1e-9)
            np.testing.assert_allclose(W, Ws, rtol=1e-7, atol=1e-9)
            assert np.all(o["particles"][:, 2] == m.P0[0, 2])
            tw.close()
            e.close()


@pytest.mark.parametrize("n", [3000, 8192])
def test_above_64_kib_of_dynamic_lds(progs, n):
    """2. d = 10, n = 3000: lds::ens asks for 69 KiB, more than the 64 KiB a launch gets by default - a module's function is launched with it as
    the library's own kernel is; n = 8192, the largest cloud an ensemble serves: 150 KiB"""
    spec = models.gauss_spec()
    data, par = gauss_par(spec)
    members = [Member(spec, n, s, 8, progs("gauss", 10), data, par) for s in (21, 22)]
    check_members(members, dict(n_phi=8), "n = %d" % n)


def test_vintages_side_by_side_in_any_order_and_twice(progs):
    """3. one program, four data vintages (40, 60, 80, 100 rows of the regression data, each with its own par): each member equals its solo
    run; reversed order, one of them alone and a second identical call give the same bits"""
    full = np.load(os.path.join(ROOT, "tests", "golden", "reg_data.npz"))["data"]
    members = []
    for k, rows in enumerate((40, 60, 80, 100)):
        spec = dict(priors=[("normal", 0.0, 10.0)] * 2, bounds=[(-1e5, 1e5)] * 2, fixed=[0, 0], lik=("linreg", [1.0], full[:rows], None), old_lik=None)
        members.append(Member(spec, 500, 100 + k, 30, progs("reg", 2), full[:rows], reg_par(rows)))
    kw = dict(n_phi=30, n_mh_steps=2)
    es, rs, outs = check_members(members, kw, "vintages", keep=True)
    want = [bits(e, r) for e, r in zip(es, rs)]
    for e in es:
        e.close()
    assert len({o["logmdd"] for o in outs}) == 4
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2]):
        es = [members[k].engine() for k in order]
        rs = run_ensemble(es, **kw)
        for k, e, r in zip(order, es, rs):
            assert bits(e, r) == want[k], (order, k)
            e.close()


def test_more_members_than_cus(progs):
    """4. 300 members: the grid queues; every status is 0; members 0, 150 and 299 are the bits of the same three run as an ensemble of three"""
    spec = models.gauss_spec(d=3)
    data, par = gauss_par(spec)
    n, E, kw = 256, 300, dict(n_phi=6)
    P0s = {k: start_cloud(spec, n, 1000 + k) for k in (0, 150, 299)}
    base = start_cloud(spec, n, 999)                          # (the start of every other member: its own seed makes its run its own)

    def member(k):
        return prog_engine(spec, n, 1000 + k, 6, progs("gauss", 3), data, par, P0s.get(k, base))

    es = [member(k) for k in range(E)]
    rs = run_ensemble(es, **kw)
    assert [r["status"] for r in rs] == [0] * E
    assert all(r["n_stages"] == 6 for r in rs)
    three = [member(k) for k in (0, 150, 299)]
    r3 = run_ensemble(three, **kw)
    for j, k in enumerate((0, 150, 299)):
        assert bits(es[k], rs[k]) == bits(three[j], r3[j]), k
    for e in es + three:
        e.close()


def test_nan_is_minus_infinity(progs):
    """5a. NaN where theta_0 > par[2] = 0.2"""
    spec = models.gauss_spec(d=3)
    data, par = gauss_par(spec, 0.2)
    members = [Member(spec, 500, s, 20, progs("nan", 3), data, par) for s in (5, 6)]
    check_members(members, dict(n_phi=20, n_blocks=2), "nan")


def test_the_gate_keeps_out_of_bounds_proposals_from_the_function(progs):
    """5b. uniform priors on [-0.5, 0.5]^3 and c = 2.0, so that many proposals leave the bounds: a function that answers +1e300 outside them is
    never asked there - the run equals its solo run, its log-MDD is finite, and fewer rows than proposals were scored"""
    d, n = 3, 500
    spec = models.gauss_spec(d)
    spec = dict(spec, bounds=[(-0.5, 0.5)] * d, priors=[("uniform", -0.5, 0.5)] * d)
    data, par = gauss_par(spec, -0.5, 0.5)
    members = [Member(spec, n, s, 15, progs("bounds", d), data, par) for s in (7, 8)]
    _, _, outs = check_members(members, dict(n_phi=15, c=2.0), "gate")
    for o in outs:
        assert math.isfinite(o["logmdd"]) and abs(o["logmdd"]) < 1e6
        assert 0 < o["stats"]["evaluations"] < 14 * n
        assert o["stats"]["evaluations"] == o["ref"]["stats"]["evaluations"]


def test_counts(progs):
    """6. bounds no proposal leaves (+-1e5 under priors of standard deviation 5): the function scores every proposal of every mutated stage"""
    spec = models.gauss_spec(d=3)
    data, par = gauss_par(spec)
    n, kw = 777, dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=3, n_mh_steps=2)
    members = [Member(spec, n, s, 200, progs("gauss", 3), data, par) for s in (41, 42, 43)]
    _, _, outs = check_members(members, kw, "counts")
    for o in outs:
        ref = o["ref"]
        assert ref["stats"]["evaluations"] == 6 * (ref["n_stages"] - 1) * n          # the reference itself: steps x (stages - 1) x n
        assert o["stats"]["evaluations"] == 6 * (o["n_stages"] - 1) * n
        assert o["stats"]["calls"] == 1


def test_the_handle_afterwards(progs):
    """7. stages_held, records and the summaries as after a solo run; a fresh smcmi_run on the member - the split path of the same code
    object - is bit-identical to one on a handle the ensemble never touched"""
    from smc_jl_amd.host import api

    spec = models.gauss_spec(d=4)
    data, par = gauss_par(spec)
    n, ms = 600, 200
    kw = dict(use_fixed_schedule=False, tempering_target=0.92, n_mh_steps=2)
    members = [Member(spec, n, s, ms, progs("gauss", 4), data, par, store_history=True) for s in (71, 72)]
    es, rs, outs = check_members(members, kw, "afterwards", keep=True)
    for m, e, r, o in zip(members, es, rs, outs):
        assert e.stages_held() == r["n_stages"] == o["ref"]["n_stages"]
        a = e.get_loop_state()
        assert a["stage_index"] == r["n_stages"] and a["phi_n"] == 1.0 and a["logmdd"] == r["logmdd"]
        q = e.weighted_quantiles(probs=(0.05, 0.5, 0.95))
        np.testing.assert_allclose(q, api.weighted_quantiles(o["particles"], probs=(0.05, 0.5, 0.95)), rtol=1e-9, atol=1e-12)
        fresh = m.engine()
        kw2 = dict(n_phi=25, n_blocks=2)
        got = []
        for h in (e, fresh):
            h.upload_cloud(m.P0)
            g = h.run(**kw2)
            rec = h.stage_records(g["n_stages"])
            got.append((g["n_stages"], g["resamples"], g["logmdd"], h.download_cloud().tobytes(), tuple(rec[x].tobytes() for x in sorted(rec)),
                        tuple(x.tobytes() for x in h.history(g["n_stages"])), h.callback_stats()["evaluations"]))
        assert got[0] == got[1]
        assert got[0][-1] == 2 * 24 * n
        fresh.close()
        e.close()


def test_refusals(progs):
    """8. every refusal returns its code and leaves clouds and loop states bit-identical; afterwards the same handles run"""
    from smc_jl_amd.host import _lib

    spec = models.gauss_spec(d=3)
    data, par = gauss_par(spec)
    n, ms = 200, 20

    def member(seed, prog, **kw):
        return Member(spec, n, seed, ms, prog, data, par, **kw).engine()

    def refused(engines, code, **kw):
        before = [e.download_cloud() for e in engines]
        states = [e.get_loop_state() for e in engines]
        with pytest.raises(_lib.SMCMIError) as ei:
            run_ensemble(engines, **dict(dict(n_phi=10), **kw))
        assert ei.value.code == code, (ei.value.code, code, str(ei.value))
        for e, b, s in zip(engines, before, states):
            assert e.download_cloud().tobytes() == b.tobytes()
            assert e.get_loop_state() == s

    a, b = member(1, progs("gauss", 3)), member(2, progs("gauss", 3))
    family = member(3, None)                                       # (set_likelihood_program(None) ...
    family.set_model(spec)                                         # ... and the device family back)
    refused([a, family], ARG)                                      # a program member beside a family member
    refused([family, a], ARG)
    family.close()
    other = member(4, progs("nan", 3))
    refused([a, other], ARG)                                       # two different ensemble programs
    other.close()
    wrong = member(5, progs("gauss", 4))
    refused([a, wrong], ARG)                                       # compiled for n_para = 4 on n_para = 3 handles
    refused([wrong], ARG)
    wrong.close()
    plain = member(6, progs("gauss", 0))
    refused([a, plain], UNSUPPORTED)                               # a plain program: no ensemble kernel
    refused([plain], UNSUPPORTED)
    plain.close()
    old = member(7, progs("gauss", 3))
    old.set_likelihood_program(progs("gauss", 3), data=data, par=par, which=1)
    refused([a, old], UNSUPPORTED)                                 # an ensemble program at SMCMI_WHICH_OLD
    old.close()
    refused([a, b], UNSUPPORTED, alpha=0.9)                        # mixture proposals
    rs = run_ensemble([a, b], n_phi=10)
    assert [r["status"] for r in rs] == [0, 0] and all(r["n_stages"] == 10 for r in rs)
    assert a.callback_stats() == dict(calls=1, evaluations=9 * n)
    a.close()
    b.close()


def test_smc_ensemble_with_a_hip_likelihood():
    """9. smc_ensemble(HIPLikelihood(REG_SRC, ensemble=True), ...) over three seeds against smc(HIPLikelihood(REG_SRC), ..., seed=s): the
    weighted means within the atol 1e-6 of test_smc_with_a_hip_likelihood_on_the_regression_example, equal stage counts"""
    import smc_jl_amd as S

    data = np.load(os.path.join(ROOT, "tests", "golden", "reg_data.npz"))["data"]          # 100 x 2 = [y X]
    pars = [S.parameter("α1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False),
            S.parameter("β1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False)]
    seeds = [1, 2, 3]
    outs = S.smc_ensemble(S.HIPLikelihood(REG_SRC, par=reg_par(100), ensemble=True), pars, data, seeds, n_parts=1000)
    assert len(outs) == 3
    for s, (cloud, w, W) in zip(seeds, outs):
        c_ref, _, _ = S.smc(S.HIPLikelihood(REG_SRC, par=reg_par(100)), pars, data, n_parts=1000, use_fixed_schedule=True, seed=s, verbose="none")
        print("seed %d: mean %r (ensemble) %r (smc)" % (s, S.weighted_mean(cloud), S.weighted_mean(c_ref)))
        assert cloud.status == 0 and cloud.stage_index == c_ref.stage_index
        np.testing.assert_allclose(S.weighted_mean(cloud), S.weighted_mean(c_ref), atol=1e-6)
        assert abs(cloud.logmdd - c_ref.logmdd) <= 1e-8
    with pytest.raises(NotImplementedError, match="HIPLikelihood"):
        S.smc_ensemble(S.HIPLikelihood(REG_SRC, par=reg_par(100)), pars, data, [1, 2], n_parts=1000)
