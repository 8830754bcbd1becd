"""tests/mutation_ref.py is pinned before it is trusted: Philox against the three known-answer vectors Random123 publishes (and with it the oracle's
export and host/hostmath.py's copy); normals, step-size factor and densities against second, differently written mpmath statements; the Julia
reference's own numbers in tests/golden/proposal_densities.npz and the all-rejected tests/golden/mutation.npz; the conditions and caps every input
class states, for the reference alone; and the FP64 restatement (oracle/smc_oracle.c) on every class: no decided decision differs, and its worst
errors in θ' (units of s_k), log q0 - log q1 and log η (units of max(1, S)) - printed per class - are the yardsticks tests/test_gpu_mutation_range.py
sizes its bars with (restatement_yardsticks below, run there in the worker before the device's values are looked at).

Measured (n = 300 rows per case), the restatement's worst errors per class - θ', log q0 - log q1, log η:
  benign            4.2e-15  9.1e-16  1.1e-14        density_scale     2.3e-14  1.3e-16  7.6e-17
  ill_conditioned   1.3e-11  1.2e-10  6.8e-12        alpha             8.9e-14  1.1e-15  6.0e-15
  far               1.1e-16  5.3e-14  2.9e-11        tight_bounds      2.8e-15  4.2e-16  1.5e-16
  mu_far            2.8e-14  0        1.3e-16        dead_rows         3.0e-15  2.4e-16  4.4e-15
  phi               2.4e-16  9.0e-16  2.7e-16        blocks            1.2e-14  9.4e-16  2.5e-13
(θ': the restatement forms the angle as the FP64 product 2π ub, so a normal next to an axis crossing is off by up to 1e-15 of r - in units of
s_k that is the 1e-14; ill_conditioned: the FP64 Cholesky factor of a matrix of condition 1e7 and the solves with it; far: θ_b - θ'_b and the
log-likelihood's residuals cancel eight digits of a cloud 1e8 standard deviations from the origin.)  No flip anywhere; undecided + band + dropped
decisions: 0 in every case."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

from oracle import oracle as orc
from smc_jl_amd.host import hostmath
from tests import models
from tests import mutation_ref as mr
from tests import target_ref as tr

LD = np.longdouble


# ------------------------------------------------------------------------------------------------ Philox
def _orc_philox(ctr, key):
    out = (C.c_uint32 * 4)()
    orc.lib().orc_philox4x32_10(*(C.c_uint32(v) for v in ctr + key), out)
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("k", range(3))
def test_philox_known_answers(k):
    ctr, key, want = mr.KAT[k]
    assert mr.philox_int(ctr, key) == want
    assert tuple(int(v) for v in mr.philox(*ctr, *key)) == want
    assert _orc_philox(ctr, key) == want
    assert tuple(hostmath.philox4x32_10(*ctr, *key)) == want


def test_tag_and_u53():
    assert mr.rng_tag(mr.P_MUT, 0xFFFFF, 0) == 0x0FFFFF00 and mr.rng_tag(mr.P_INIT, 1, 2) == 0x30000102 and mr.rng_tag(mr.P_BLK, 1 << 20, 0x1FF) == 0x200000FF
    assert mr.rng_tag(mr.P_MUT, 29, 33) == hostmath.rng_tag(0, 29, 33) == (29 << 8 | 33)
    # (x >> 11) + 0.5 is exact below 2^52 and a tie above: to the even neighbour, so u = 1 - 2^-53 is the largest and 2^-54 the smallest uniform
    assert mr.u53_int(0, 0) == 2.0 ** -54 and mr.u53_int(MASK, MASK) == 1.0 and mr.u53_int(0x7FFFFFFF, MASK) == 0.5 - 2.0 ** -54
    x_odd, x_even = (1 << 52) + 1, (1 << 52) + 2             # x + 0.5 -> x + 1 (odd x: up to the even), x (even x: down)
    for x, want in ((x_odd, float(x_odd + 1)), (x_even, float(x_even))):
        hi, lo = (x << 11) >> 32, (x << 11) & MASK
        assert mr.u53_int(hi, lo) == want * 2.0 ** -53 == float(mr.u53(np.uint64(hi), np.uint64(lo)))
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, (2, 4096), dtype=np.uint64)
    assert np.array_equal(mr.u53(w[0], w[1]), [mr.u53_int(int(a), int(b)) for a, b in zip(w[0], w[1])])
    # the ids' high word is a counter word of its own
    ids = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) + 5]
    ua, ub = mr.uniform_pair(77, np.array(ids, dtype=np.uint64), 299, mr.rng_tag(0, 3, 1))
    for i, pid in enumerate(ids):
        assert (ua[i], ub[i]) == hostmath.uniform_pair(77, pid, 299, mr.rng_tag(0, 3, 1))
        o = mr.philox_int((pid & MASK, pid >> 32, 299, mr.rng_tag(0, 3, 1)), (77, 0))
        assert (ua[i], ub[i]) == (mr.u53_int(o[0], o[1]), mr.u53_int(o[2], o[3]))
    assert len({float(v) for v in ua}) == len(ids)


MASK = mr.MASK32


def test_stream_layout_and_blocks():
    pid = np.arange(5, dtype=np.uint64) + np.uint64((1 << 32) - 2)
    for t, db in ((0, 1), (0, 4), (1, 3), (29, 9)):
        st = mr.stream(9, pid, 4, t, db)
        assert st.ua.shape == (5, (db + 1) // 2)
        for i, p in enumerate(int(v) for v in pid):
            dec = hostmath.uniform_pair(9, p, 4, hostmath.rng_tag(0, 0xFFFFF, 0))[0] if t == 0 else hostmath.uniform_pair(9, p, 4, hostmath.rng_tag(0, t - 1, 0))[1]
            assert st.u_dec[i] == dec and st.uc[i] == hostmath.uniform_pair(9, p, 4, hostmath.rng_tag(0, t, 0))[0]
            for q in range((db + 1) // 2):
                assert (st.ua[i, q], st.ub[i, q]) == hostmath.uniform_pair(9, p, 4, hostmath.rng_tag(0, t, 1 + q))
        assert mr.block_normals(st, db).shape == (5, db)
    for nf, nb, seed, stage in ((1, 1, 3, 1), (8, 3, 123, 7), (10, 10, 5, 299), (64, 7, 1 << 40, (1 << 32) - 1), (9, 2, 0, 0)):
        free = np.arange(nf, dtype=np.int32) + 2
        a, b, c = mr.generate_blocks(nf, nb, free, seed, stage), hostmath.generate_blocks(nf, nb, free, seed, stage), orc.generate_blocks(nf, nb, free, seed, stage)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert sorted(a[0]) == list(range(nf)) and a[2][-1] == nf and np.all(np.diff(a[2]) >= 1)


def test_search_ids():
    tag = mr.rng_tag(0, 0, 1)
    r = mr.search_ids(123, 7, tag, n_ids=1 << 18, chunk=1 << 16)
    ids = np.arange(1 << 18, dtype=np.uint64)
    ua, ub = mr.uniform_pair(123, ids, 7, tag)
    assert r["ua_min"][0] == int(np.argmin(ua)) and r["ua_max"][0] == int(np.argmax(ua)) and r["ub_2/4"][0] == int(np.argmin(np.abs(ub - 0.5)))
    assert r["ua_min"][1] < 2e-5 and r["ua_max"][1] > 1 - 2e-5 and all(abs(r["ub_%d/4" % k][2] - 0.25 * k) < 2e-5 for k in range(5))


# ------------------------------------------------------------------------------------------------ second statements
def test_normals_against_mpmath():
    rng = np.random.default_rng(2)
    ua = np.concatenate([rng.random(300), [2.0 ** -54, 1 - 2.0 ** -53, 0.5, 7.1e-8], 1 - 10.0 ** rng.uniform(-16, -1, 40)])
    ub = np.concatenate([rng.random(300), [2.0 ** -54, 1 - 2.0 ** -53, 0.5 - 2.0 ** -54, 0.25 + 2.0 ** -54], rng.integers(0, 5, 40) / 4.0 + 10.0 ** rng.uniform(-16, -3, 40) * rng.choice([-1, 1], 40)])
    ub = np.clip(ub, 2.0 ** -54, 1 - 2.0 ** -53)
    z0, z1 = mr.normals_ld(ua, ub)
    worst = 0.0
    with mp.workdps(50):
        for i in range(len(ua)):
            m0, m1 = mr.normal_pair_mp(ua[i], ub[i])
            r = mp.sqrt(-2 * mp.log(mp.mpf(float(ua[i]))))
            for got, want in ((z0[i], m0), (z1[i], m1)):
                # relative to the value where the angle sits next to an axis (the reduction's point), to r elsewhere
                worst = max(worst, float(abs(mr._mp_ld(want) - got) / mr._mp_ld(max(abs(want), r * mp.mpf(2) ** -30))))
    print("normals: worst error %.3g of their scale" % worst)
    assert worst <= 1e-17
    assert float(mr.ulps(tr.f64(z0), z0).max()) <= 0.5 and float(mr.ulps(tr.f64(z1), z1).max()) <= 0.5


def test_factor_against_second_statement_and_hostmath():
    with mp.workdps(50):
        for target in (0.25, 0.4):
            for a in (0.0, target, 1.0, 3.0, 0.1234, 1e-300, 2.0 / 3.0):
                f1, f2 = mr.factor_mp(a, target), mr.factor_mp2(a, target)
                assert abs(f1 - f2) <= mp.mpf(10) ** -45
                for got in (hostmath.update_c(0.37, a, target), orc.update_c(0.37, a, target)):
                    assert abs(mp.mpf(got) / mp.mpf(0.37) - f1) <= 4 * mp.mpf(2) ** -53 * f1, (a, target, got)
        assert mr.factor_mp(0.25, 0.25) == 1 and abs(mr.factor_mp(0.0, 0.25) - mp.mpf("0.95") - mp.mpf("0.1") / (1 + mp.exp(4))) < mp.mpf(10) ** -45


def test_the_literal_factor_turns_nan_from_45_mh_steps_on():
    """e^x / (1 + e^x) is Inf / Inf once 16 (a - t) > 709.78: a > 44.61 with target 0.25.  The accept column is Σ accepted d_b / n_free <= n_mh_steps
    (quirk Q2), so only runs of 45 MH steps or more reach it.  It is the reference's formula (src/smc_main.jl:453-455); the restatement, host/hostmath.py
    and the six device copies keep it."""
    assert 44.6 < mr.NAN_ACCEPT < 44.62
    below, above = math.nextafter(mr.NAN_ACCEPT, 0.0) - 1e-9, mr.NAN_ACCEPT + 1e-9
    assert math.isfinite(orc.update_c(0.5, below, 0.25)) and math.isnan(orc.update_c(0.5, above, 0.25))
    assert math.isfinite(hostmath.update_c(0.5, below, 0.25))
    with pytest.raises(OverflowError):                          # (Python's math.exp raises where C returns Inf)
        hostmath.update_c(0.5, above, 0.25)
    with mp.workdps(50):
        assert abs(mr.factor_mp(above, 0.25) - mp.mpf("1.05")) < mp.mpf(10) ** -45


@mr.dps50
def densities_mp(F, x, xn, alpha):
    """second statement (one move): the quadratic forms from LU solves with the matrix itself, the determinant from mp.det, the mixtures summed as
    densities, not in log space -> the three exponents' counterparts and log q0, log q1 (no FP64 rule)"""
    A = mp.matrix([[mp.mpf(float(v)) for v in row] for row in F.A])
    n = F.db
    M = lambda v: mp.matrix([mp.mpf(float(t)) for t in v])
    cst = n * mp.log(2 * mp.pi) + mp.log(mp.det(A))

    def nd(a, b):
        r = M(a) - M(b)
        return mp.exp(-(cst + (r.T * mp.lu_solve(A, r))[0]) / 2)

    ind = mp.mpf(1)
    for i in range(n):
        sd = mp.sqrt(mp.mpf(float(F.Sig[i, i])))
        ind = ind / (sd * mp.sqrt(2 * mp.pi)) * mp.exp(-((mp.mpf(float(x[i])) - mp.mpf(float(xn[i]))) / sd) ** 2 / 2)
    a = mp.mpf(float(alpha))
    q0 = a * nd(x, xn) + (1 - a) / 2 * ind + (1 - a) / 2 * nd(x, F.mu)
    q1 = a * nd(xn, x) + (1 - a) / 2 * ind + (1 - a) / 2 * nd(xn, F.mu)
    return mp.log(nd(x, xn)), mp.log(ind), mp.log(q0), mp.log(q1)


@pytest.mark.parametrize("name", list(mr.CLASSES))
def test_densities_and_draw_against_a_second_statement(name):
    """a subsample of every class: the exponents and the mixtures to 1e-17 of max(1, S), and θ' = centre + L z against the factor's defining product
    L Lᵀ = (c c) Σ_b.  The ill-conditioned class alone is asserted to 1e-17 x the condition number of its unit-diagonal factor - 1.8e3, 1.6e6 and
    3.0e6 in the three cases of the subsample, so an effective bar of up to 3.0e-11 (printed) - since a longdouble solve with that factor keeps
    no more; measured there: 6e-16."""
    worst = dict(e0=0.0, e1=0.0, q=0.0, chol=0.0)
    y = restatement_yardsticks(name)
    for case, res in list(zip(y["cases"], y["results"]))[::2]:
        s = res.steps[-1]
        F = mr.block_factor(case.mu, case.Sigma, s.idx, case.c)
        with mp.workdps(50):
            Lm = mp.matrix([[mr_mp(v) for v in row] for row in F.L])
            R = Lm * Lm.T
            worst["chol"] = max(worst["chol"], max(float(abs(R[i, j] - mp.mpf(float(F.A[i, j]))) / mp.sqrt(mp.mpf(float(F.A[i, i])) * mp.mpf(float(F.A[j, j])))) for i in range(F.db) for j in range(F.db)))
        cond = float(np.linalg.cond(tr.f64(F.L / np.diag(F.L)[:, None]))) if name == "ill_conditioned" else 1.0
        if name == "ill_conditioned":
            print("%s: condition number %.3g, effective bar %.3g" % (case.label, cond, 1e-17 * cond))
        rows = [i for i in range(0, case.cloud.shape[0], 37) if s.active[i] and not np.isnan(s.state_theta[i]).any()]
        for i in rows:
            x, xn = s.state_theta[i, s.pos], tr.f64(s.theta_new)[i]
            e0, e1, q0, q1 = densities_mp(F, x, xn, case.alpha)
            D = s.dens
            with mp.workdps(50):
                scale = max(1.0, float(D.S[i]))
                worst["e0"] = max(worst["e0"], float(abs(e0 - mr_mp(D.e0[i]))) / max(1.0, abs(float(e0))) / cond)
                worst["e1"] = max(worst["e1"], float(abs(e1 - mr_mp(D.e1[i]))) / max(1.0, abs(float(e1))))
                if not D.band[i] and np.isfinite(tr.f64(D.logq0[i])) and np.isfinite(tr.f64(D.logq1[i])) and min(D.e0[i], D.e1[i], D.e2_0[i], D.e2_1[i]) > mr.EXP_SUBN:
                    worst["q"] = max(worst["q"], float(abs((q0 - q1) - mr_mp(D.diff[i]))) / scale / cond)
    print(name, worst)
    assert worst["chol"] <= 1e-18 and worst["e0"] <= 1e-17 and worst["e1"] <= 1e-17 and worst["q"] <= 1e-17, worst


def mr_mp(v):
    """a longdouble as an mpf, exactly"""
    v = LD(v)
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


# ------------------------------------------------------------------------------------------------ golden fixtures
def test_reference_reproduces_the_julia_proposal_densities():
    z = np.load(models.GOLDEN + "/proposal_densities.npz")
    d = len(z["mu"])
    F = mr.block_factor(z["mu"], z["Sigma"], range(d), float(z["c"]))
    D = mr.densities(F, z["para_subset"][None, :], z["para_draw"][None, :], float(z["alpha"]))
    print("log q0 %.17g (Julia %.17g), log q1 %.17g (Julia %.17g)" % (float(D.logq0[0]), float(z["q0"]), float(D.logq1[0]), float(z["q1"])))
    assert not D.band[0]
    assert float(D.logq0[0]) == pytest.approx(float(z["q0"]), rel=1e-14) and float(D.logq1[0]) == pytest.approx(float(z["q1"]), rel=1e-14)


def test_reference_reproduces_the_all_rejected_julia_mutation():
    z = np.load(models.GOLDEN + "/mutation.npz")
    spec = models.linmodel_spec(T=100, old_T=100)
    spec["old_lik"] = ("linmodel3", [], z["old_data"], np.load(models.GOLDEN + "/linmodel.npz")["X"])
    P = np.asfortranarray(z["particles_in"])
    bf, ba = (z["blocks_free"] - 1).astype(np.int32), (z["blocks_all"] - 1).astype(np.int32)
    bp = np.concatenate([[0], np.cumsum(z["block_sizes"])]).astype(np.int32)
    case = mr.Case("julia", spec, P, z["mu"], z["Sigma"], float(z["c"]), float(z["alpha"]), float(z["phi_n"]), 1, 1, 2, 42, {})
    res = mr.mutate(case, blocks=(bf, ba, bp))
    # the fixture's log-prior column is the reference target's at its θ, and nothing moves: the Julia output is the input
    T = tr.target(spec, P[:, :9])
    assert float(tr.nerr(P[:, 10], T.lp, T.lp_S).max()) < 1e-13          # (its loglh column is 0: what rejects every proposal)
    o = res.steps[0].outcome
    assert np.all((o == mr.REJECT) | (o == mr.NAN_REJECT)), np.bincount(o)
    assert np.array_equal(res.theta, z["particles_out"][:, :9]) and np.all(res.accept_col == 0.0) and np.all(z["particles_out"][:, 12] == 0.0)
    assert res.rate == 0


# ------------------------------------------------------------------------------------------------ the restatement
def oracle_target(spec, theta):
    """(loglh, logprior, old_loglh) of the FP64 oracle at the rows of theta, bounds rule included; -Inf on the new data takes the prior with it"""
    d = theta.shape[1]
    P = np.zeros((len(theta), d + 5), order="F")
    P[:, :d], P[:, d + 4] = theta, 1.0
    Q = orc.initialize_likelihoods(models.oracle_model(spec), P)
    ll, lp = Q[:, d].copy(), Q[:, d + 1].copy()
    lp[ll == -np.inf] = -np.inf
    if spec.get("old_lik") is None:
        return ll, lp, np.where(tr.in_bounds(spec, theta), 0.0, -np.inf)
    Qo = orc.initialize_likelihoods(models.oracle_model(dict(spec, lik=spec["old_lik"], old_lik=None)), P)
    return ll, lp, Qo[:, d].copy()


def restatement_errors(case, res, pid0=0):
    """the oracle's pieces at the reference's state of every proposal -> its worst errors (θ', log q0 - log q1, log η, and the log-prior at its own
    θ') over the rows the reference decides, and the number of rows whose decision differs"""
    worst, flips = dict(theta=0.0, q=0.0, eta=0.0, lp=0.0), 0
    n, d = case.cloud.shape[0], case.cloud.shape[1] - 5
    for s in res.steps:
        mu_b, Sig_b = np.ascontiguousarray(case.mu[s.idx]), np.ascontiguousarray(case.Sigma[np.ix_(s.idx, s.idx)])
        use = s.active & (s.outcome != mr.BAND)
        thn, qd = np.full((n, len(s.pos)), np.nan), np.full(n, np.nan)
        for i in np.flatnonzero(use):
            xb = np.ascontiguousarray(s.state_theta[i, s.pos])
            thn[i] = orc.mixture_draw(xb, mu_b, Sig_b, case.c, case.alpha, case.seed, pid0 + int(i), case.stage, s.t)
            q0, q1 = orc.proposal_densities(thn[i], xb, mu_b, Sig_b, case.c, case.alpha)
            with np.errstate(all="ignore"):
                qd[i] = np.float64(q0) - np.float64(q1)
        para = s.state_theta.copy()
        para[:, s.pos] = np.where(use[:, None], thn, para[:, s.pos])
        ll, lp, old = oracle_target(case.spec, para)
        with np.errstate(all="ignore"):
            arg = case.phi * (ll - s.state_cols[:, 0]) + (1.0 - case.phi) * (old - s.state_cols[:, 2]) + (lp - s.state_cols[:, 1]) + qd
            acc = s.u_dec < np.exp(arg)
        worst["theta"] = max(worst["theta"], float(mr.nerr_theta(thn, s.theta_new, s.scale)[use].max(initial=0.0)))
        worst["q"] = max(worst["q"], float(mr.nerr_log(qd, s.dens.diff, s.dens.S)[use].max(initial=0.0)))
        worst["eta"] = max(worst["eta"], float(mr.nerr_log(arg, s.log_eta, s.S_eta)[use].max(initial=0.0)))
        worst["lp"] = max(worst["lp"], float(mr.nerr_log(lp, s.lp, s.lp_S)[use].max(initial=0.0)))
        decided = use & (s.outcome != mr.UNDECIDED)
        flips += int((acc != (s.outcome == mr.ACCEPT))[decided].sum())
    return worst, flips


_YARD = {}


def restatement_yardsticks(name, n=mr.N_CLASS):
    """{theta, q, eta: the restatement's worst error over the class; bars: the bars of the GPU file; tol: the undecided rule's; results: the
    reference's call per case; flips; whole: rows whose accept column from the whole restated call differs}"""
    if (name, n) in _YARD:
        return _YARD[(name, n)]
    cs = mr.cases(name, n)
    results = [mr.mutate(c) for c in cs]
    errs = [restatement_errors(c, r) for c, r in zip(cs, results)]
    worst = {k: max(e[0][k] for e in errs) for k in ("theta", "q", "eta", "lp")}
    tol = max(mr.FLOOR_DECIDE, mr.FACTOR * worst["eta"])
    if tol > mr.FLOOR_DECIDE:                                   # the undecided rule with the class's own yardstick: the calls again
        results = [mr.mutate(c, tol=tol) for c in cs]
        errs = [restatement_errors(c, r) for c, r in zip(cs, results)]
        worst = {k: max(worst[k], max(e[0][k] for e in errs)) for k in worst}
    out = dict(worst, tol=tol, cases=cs, results=results, flips=sum(e[1] for e in errs),
               bars=dict(theta=max(mr.FLOOR_THETA, mr.FACTOR * worst["theta"]), q=max(mr.FLOOR_LOG, mr.FACTOR * worst["q"]), eta=max(mr.FLOOR_LOG, mr.FACTOR * worst["eta"]),
                         lp=max(mr.FLOOR_LOG, mr.FACTOR * worst["lp"])))
    _YARD[(name, n)] = out
    return out


@pytest.mark.parametrize("name", list(mr.CLASSES))
def test_restatement_agrees_on_every_decided_decision(name):
    y = restatement_yardsticks(name)
    print("%-16s restatement worst: theta' %.2g  q0-q1 %.2g  log eta %.2g  log-prior %.2g   undecided rule %.2g   flips %d" % (name, y["theta"], y["q"], y["eta"], y["lp"], y["tol"], y["flips"]))
    assert y["flips"] == 0
    whole = 0
    for case, res in zip(y["cases"], y["results"]):
        bf, ba, bp = mr.own_blocks(case)
        Q = orc.mutate_cloud(models.oracle_model(case.spec), case.cloud, case.mu, case.Sigma, bf, ba, bp, case.phi, 0.0, case.c, case.alpha, case.n_mh, case.seed, case.stage)
        d = case.cloud.shape[1] - 5
        keep = ~res.dropped
        whole += int((Q[keep, d + 3] != res.accept_col[keep]).sum())
        moved = keep & (res.count > 0)
        assert np.allclose(Q[moved, :d], res.theta[moved], rtol=1e-6, atol=0.0, equal_nan=True), case.label
        assert np.array_equal(Q[keep & (res.count == 0), :d], case.cloud[keep & (res.count == 0), :d], equal_nan=True), case.label
    assert whole == 0, "%d rows whose accept column differs after the whole restated call" % whole


@pytest.mark.parametrize("name", list(mr.CLASSES))
def test_every_class_keeps_its_conditions_and_caps(name):
    """for the reference alone: at most 1e-3 of a case's decisions are undecided, in a band or dropped, and the case is what its class says"""
    y = restatement_yardsticks(name)
    for case, res in zip(y["cases"], y["results"]):
        und, band, drop, total = mr.left_out(res)
        o = np.concatenate([s.outcome for s in res.steps])
        inb = np.concatenate([s.inb for s in res.steps])
        comp = np.concatenate([s.comp for s in res.steps])
        fig = dict(accept=float((o == mr.ACCEPT).mean()), outside=float(1 - inb.mean()), nan_reject=float((o == mr.NAN_REJECT).mean()), comps=sorted(set(comp.tolist())))
        print("%-16s %-36s decisions %5d undecided %d band %d dropped %d  %s" % (name, case.label, total, und, band, drop, fig))
        assert und + band + drop <= mr.CAP * total, case.label
        for key in ("accept", "outside", "nan_reject"):
            if key in case.cond:
                assert case.cond[key][0] <= fig[key] <= case.cond[key][1], (case.label, key, fig[key])
        if "comps" in case.cond:
            assert fig["comps"] == list(case.cond["comps"]), (case.label, fig["comps"])
        if "row" in case.cond:
            assert res.steps[0].comp[case.cond["row"]] == case.cond["comp"], case.label
        assert res.rate is None or res.rate == mp.mpf(int(res.count.sum())) / (len(mr._free(case.spec)) * len(res.count))
    if name == "density_scale":
        by = {c.label: np.bincount(np.concatenate([s.outcome for s in r.steps]), minlength=6) for c, r in zip(y["cases"], y["results"])}
        n = mr.N_CLASS
        assert by["s=1e+30 alpha=1"][mr.NAN_REJECT] == 0 and 0 < by["s=1.5e+32 alpha=1"][mr.NAN_REJECT] < n and by["s=1e+40 alpha=1"][mr.NAN_REJECT] == n     # nobody / some / everybody
        # the other end: nobody / some / everybody rejected by the q0 = 0 quirk (both densities +Inf: log η = -Inf) or, at α = 1, by 0 x Inf
        for a in ("1", "0.9"):
            assert by["s=1e-29 alpha=" + a][mr.ACCEPT] > 0 and by["s=1e-40 alpha=" + a][mr.ACCEPT] == 0
            assert 0 < by["s=1e-31 alpha=" + a][mr.ACCEPT] + by["s=5e-32 alpha=" + a][mr.ACCEPT] and by["s=5e-32 alpha=" + a][mr.ACCEPT] < by["s=1e-29 alpha=" + a][mr.ACCEPT]
    if name == "mu_far":
        for case, res in zip(y["cases"], y["results"]):
            s = res.steps[0]
            c2 = s.comp == 2
            assert np.all(s.dens.e2_0[c2] < mr.EXP_UNDER) and np.all(s.dens.e2_1[c2] > mr.EXP_SUBN), case.label       # vanishes for q0 only
            assert np.all(s.dens.e2_0[~c2] < mr.EXP_UNDER) and np.all(s.dens.e2_1[~c2] < mr.EXP_UNDER), case.label    # for both
