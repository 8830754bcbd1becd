"""tests/target_ref.py pinned (no GPU): the prior densities against scipy.stats and against a second mpmath statement (the density, then its
log), the likelihoods against an mpmath evaluation written per period, the edge table literally - and the condition every input class of
tests/test_gpu_target_range.py rests on: the reference is finite where the class says so, the FP64 oracle (oracle.logprior / oracle.loglik behind
orc_initialize_likelihoods) returns the same infinities, is finite where the reference is and is off by more than 1e-10 (normalised) on at most 3
of the 24 θ.  The oracle's worst normalised error per class is printed: 16 x that (floor 1e-13) is the device's bar.

With the prior_logpdf of the parent commit test_family_edges_on_the_oracle_and_on_cloudio fails: the oracle returns NaN for Gamma(1, 2) at 0,
Beta(1, 3) at 0, Beta(3, 1) at 1, Beta(1, 1) at 0 and 1 and RootInverseGamma(4, 0.5) at 1e-170 and 1e-162, -Inf for RootInverseGamma at 1e155,
and host/cloudio.py raises ValueError (math.log(0)).

scipy.stats works in FP64: a sum of at most four correctly rounded terms and lnΓ / lnB to a few ulp cannot agree with a 50-digit value better than
8 x 2^-53 S; that is its bar here.  The second mpmath statement and the per-period likelihoods are held to 1e-17 S.
"""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import models
from tests import target_ref as tr

EXACT = 1e-17                 # normalised: what two statements of the same formula in extended precision agree to
SCIPY = 8.0 * 2.0 ** -53      # see the module docstring


def oracle_columns(spec, theta):
    """(loglh, logprior) of the FP64 oracle's initialize_likelihoods (bounds rule included) on the rows of theta"""
    from oracle import oracle as orc

    d = theta.shape[1]
    P = np.zeros((len(theta), d + 5), order="F")
    P[:, :d], P[:, d + 4] = theta, 1.0
    Q = orc.initialize_likelihoods(models.oracle_model(spec), P)
    return Q[:, d].copy(), Q[:, d + 1].copy()


INTERIOR = [(("normal", 0.5, 2.0), (-3.0, 0.5, 7.25)), (("gamma", 0.6, 2.0), (1e-3, 0.7, 30.0)), (("gamma", 7.5, 0.25), (0.2, 1.9, 8.0)), (("gamma", 200.0, 2.0), (300.0, 400.0)),
            (("beta", 0.5, 0.5), (1e-4, 0.5, 0.999)), (("beta", 400.0, 400.0), (0.45, 0.5)), (("beta", 1.0, 3.0), (0.2, 0.9)), (("invgamma", 3.0, 2.0), (0.05, 1.0, 40.0)),
            (("invgamma", 1e-3, 2.0), (0.5, 3.0)), (("uniform", -3.0, 3.0), (-3.0, 0.1, 3.0)), (("rootinvgamma", 4.0, 0.5), (0.1, 0.5, 3.0)), (("rootinvgamma", 400.0, 0.5), (0.45, 0.55))]


def _density_mp(fam, a, b, x):
    """the density itself (not its log), mpmath"""
    a, b, x = mp.mpf(a), mp.mpf(b), mp.mpf(x)
    if fam == "normal":
        return mp.npdf(x, a, b)
    if fam == "uniform":
        return 1 / (b - a)
    if fam == "gamma":
        return x ** (a - 1) * mp.exp(-x / b) / (mp.gamma(a) * b ** a)
    if fam == "beta":
        return x ** (a - 1) * (1 - x) ** (b - 1) / mp.beta(a, b)
    if fam == "invgamma":
        return b ** a / mp.gamma(a) * x ** (-a - 1) * mp.exp(-b / x)
    # σ with ν τ² / σ² ~ χ²(ν): the χ² density times |d(ν τ² / σ²) / dσ|
    u = a * b * b / (x * x)
    return u ** (a / 2 - 1) * mp.exp(-u / 2) / (2 ** (a / 2) * mp.gamma(a / 2)) * 2 * u / x


def test_priors_against_scipy_and_a_second_mpmath_statement():
    from scipy import stats

    worst = dict(scipy=0.0, mp=0.0)
    with mp.workdps(tr.DPS):
        for (fam, a, b), xs in INTERIOR:
            ref = dict(normal=lambda: stats.norm(a, b), uniform=lambda: stats.uniform(a, b - a), gamma=lambda: stats.gamma(a, scale=b), beta=lambda: stats.beta(a, b),
                       invgamma=lambda: stats.invgamma(a, scale=b), rootinvgamma=lambda: None)[fam]()
            for x in xs:
                v, S = tr.prior_logpdf_mp(fam, a, b, x)
                e2 = float(abs(mp.log(_density_mp(fam, a, b, x)) - v) / max(1, S))
                worst["mp"] = max(worst["mp"], e2)
                assert e2 <= EXACT, (fam, a, b, x, e2)
                if ref is not None:
                    e1 = float(abs(mp.mpf(float(ref.logpdf(x))) - v) / max(1, S))
                    worst["scipy"] = max(worst["scipy"], e1)
                    assert e1 <= SCIPY, (fam, a, b, x, e1, float(v), float(ref.logpdf(x)))
    print("worst normalised difference: scipy.stats %.3g (bar %.3g), mpmath density-then-log %.3g (bar %.3g)" % (worst["scipy"], SCIPY, worst["mp"], EXACT))


def test_edge_table_literally():
    for (fam, a, b), x, want in tr.EDGE_TABLE:
        v = tr._to_f64(tr.prior_logpdf_mp(fam, a, b, x)[0])
        if want is None:
            assert math.isfinite(v), (fam, a, b, x, v)
        elif isinstance(want, str):
            assert v == float(want), (fam, a, b, x, v)
        else:
            assert abs(v - want) <= 2.0 ** -52 * max(1.0, abs(want)), (fam, a, b, x, v, want)
    # the four rows of the issue's table by their numbers
    assert tr._to_f64(tr.prior_logpdf_mp("gamma", 1.0, 2.0, 0.0)[0]) == -math.log(2.0)
    assert tr._to_f64(tr.prior_logpdf_mp("beta", 1.0, 3.0, 0.0)[0]) == pytest.approx(math.log(3.0), abs=3e-16)
    assert tr._to_f64(tr.prior_logpdf_mp("beta", 3.0, 1.0, 1.0)[0]) == pytest.approx(math.log(3.0), abs=3e-16)
    v = tr.prior_logpdf_mp("rootinvgamma", 4.0, 0.5, 1e-170)[0]
    assert v < -mp.mpf("1e300") and mp.isfinite(v) and tr._to_f64(v) == -math.inf
    # outside the support, NaN, and the model's rules
    for fam, a, b, x in (("gamma", 2.0, 1.0, -1e-300), ("beta", 2.0, 2.0, np.nextafter(1.0, 2.0)), ("beta", 2.0, 2.0, -5e-324), ("invgamma", 3.0, 2.0, 0.0),
                         ("rootinvgamma", 4.0, 0.5, 0.0), ("uniform", -1.0, 1.0, np.nextafter(1.0, 2.0))):
        assert tr._to_f64(tr.prior_logpdf_mp(fam, a, b, x)[0]) == -math.inf, (fam, x)
    sp = tr.ten()
    th = tr.prior_draws(sp, 4, 1)
    th[1, 1], th[2, 1], th[3, 0] = 1.5, np.nextafter(2.0, 3.0), np.nan       # outside the narrow Uniform prior but inside the bounds; outside; NaN
    T = tr.target(sp, th)
    assert T.inb.tolist() == [True, True, False, False]
    assert np.isfinite(tr.f64(T.lp[0])) and tr.f64(T.lp)[1] == -np.inf and np.isfinite(tr.f64(T.ll)[1])
    assert np.all(tr.f64(T.lp)[2:] == -np.inf) and np.all(tr.f64(T.ll)[2:] == -np.inf) and np.all(tr.f64(T.old)[2:] == -np.inf)
    free = tr.logprior_mp(sp, th[:1])[0][0]
    sp2 = dict(sp, fixed=[0] * 10)
    assert tr.logprior_mp(sp2, th[:1])[0][0] != free                              # the fixed parameter's density is not in the sum


@pytest.mark.parametrize("name", list(tr.CLASSES))
def test_likelihoods_against_mpmath_per_period_and_the_longdouble_priors_against_mpmath(name):
    worst = dict(lik=0.0, prior=0.0)
    for c in tr.cases(name) + ([tr.det_underflow_case()] if name == "far" else []):
        safe = c.theta[tr.in_bounds(c.spec, c.theta)]                  # (all 24 θ of the case: the GPU bars rest on every one)
        ll, S = tr.loglik(c.spec["lik"], safe)
        for i, th in enumerate(safe):
            v, s = tr.loglik_mp(c.spec["lik"], th)
            if mp.isinf(v) or abs(v) > tr.DBL_MAX:                     # (beyond the FP64 range: the column holds that infinity)
                assert tr.f64(ll[i:i + 1])[0] == -np.inf, (c.label, i)
                continue
            with mp.workdps(tr.DPS):
                e = float(abs(mp.mpf(float(ll[i])) + mp.mpf(float(ll[i] - tr.LD(float(ll[i])))) - v) / max(1, s))
            es = float(abs(tr._to_ld(s) - S[i]) / S[i])
            worst["lik"] = max(worst["lik"], e)
            assert e <= EXACT and es <= 1e-15, (c.label, i, e, es)
        a, Sa = tr.logprior_mp(c.spec, c.theta)
        b, Sb = tr.logprior_ld(c.spec, c.theta)
        e = tr.nerr(tr.f64(b), a, Sa)
        fin = np.isfinite(tr.f64(a))
        with np.errstate(all="ignore"):
            e = np.where(fin, (np.abs(b - a) / np.maximum(1, Sa)).astype(np.float64), e)
        assert np.all(np.isfinite(e)), (c.label, "an infinity differs")
        worst["prior"] = max(worst["prior"], float(e.max()))
        assert e.max() <= EXACT, (c.label, float(e.max()))
    print("%s: longdouble likelihood against mpmath per period %.3g, longdouble priors against mpmath %.3g (bar %.3g)" % (name, worst["lik"], worst["prior"], EXACT))


def _class_errors(c):
    """per column: (reference as doubles, the oracle's normalised error)"""
    T = tr.target(c.spec, c.theta)
    oll, olp = oracle_columns(c.spec, c.theta)
    return T, oll, olp, tr.nerr(oll, T.ll, T.ll_S), tr.nerr(olp, T.lp, T.lp_S)


@pytest.mark.parametrize("name", list(tr.CLASSES))
def test_input_conditions_of_every_class_and_spec(name):
    cs = tr.cases(name)
    assert all(c.theta.shape == (tr.N_CLASS, len(c.spec["priors"])) for c in cs)
    worst, why = dict(loglh=0.0, logprior=0.0), []
    for c in cs:
        T, oll, olp, ell, elp = _class_errors(c)
        for col, ref, orc_v, err, says in (("loglh", T.ll, oll, ell, c.ll_finite), ("logprior", T.lp, olp, elp, c.lp_finite)):
            ref64 = tr.f64(ref)
            for i in range(tr.N_CLASS):
                if says[i] is not None and bool(np.isfinite(ref64[i])) != says[i]:
                    why.append("%s %s row %d: the reference is %r, the class says finite = %r" % (c.label, col, i, ref64[i], says[i]))
            fin = np.isfinite(ref64)
            if np.isnan(orc_v).any() or not np.all(np.isfinite(orc_v[fin])) or not np.array_equal(orc_v[~fin], ref64[~fin]):
                why.append("%s %s: the oracle is NaN, not finite where the reference is, or another infinity: %r against %r" % (c.label, col, orc_v[~np.isfinite(orc_v) | ~fin], ref64[~np.isfinite(orc_v) | ~fin]))
                continue
            out = int((err > tr.ORC_LIMIT).sum())
            inc_worst = float(err[err <= tr.ORC_LIMIT].max())
            worst[col] = max(worst[col], inc_worst)
            print("%-13s %-48s %-8s oracle's worst normalised error %.2e, %d of %d beyond 1e-10" % (name, c.label, col, inc_worst, out, tr.N_CLASS))
            if out > tr.MAX_LEFT_OUT:
                why.append("%s %s: the oracle is off by more than 1e-10 on %d of %d" % (c.label, col, out, tr.N_CLASS))
    print("%s: the oracle's worst normalised error: loglh %.2e, logprior %.2e" % (name, worst["loglh"], worst["logprior"]))
    assert not why, "\n".join(why)


def test_nan_rows_are_outside_the_bounds_in_the_reference_and_in_the_oracle():
    """The rows tests/test_gpu_target_range.py uploads with NaN parameters: -Inf in all three columns of the reference and in the oracle's two;
    the control rows are finite in both."""
    for c in tr.nan_cases():
        T, oll, olp, ell, elp = _class_errors(c)
        out = np.array([i % 4 != 0 for i in range(tr.N_CLASS)])
        assert np.isnan(c.theta[out]).any(axis=1).all() and not np.isnan(c.theta[~out]).any(), c.label
        assert np.isnan(c.theta[3::4]).all() and (np.isnan(c.theta[1::4]).sum(axis=1) == 1).all(), c.label
        if any(c.spec["fixed"]):
            assert np.isnan(c.theta[2::4, c.spec["fixed"].index(1)]).all()
        assert T.inb.tolist() == (~out).tolist(), c.label
        for col in (T.ll, T.lp, T.old, oll, olp):
            assert np.all(tr.f64(col)[out] == -np.inf), c.label
        assert np.all(np.isfinite(tr.f64(T.ll)[~out])) and np.all(np.isfinite(tr.f64(T.lp)[~out])) and np.all(np.isfinite(oll[~out])) and np.all(np.isfinite(olp[~out])), c.label
        assert max(ell[~out].max(), elp[~out].max()) <= 1e-13, c.label


def test_two_vintage_specs_sit_on_both_sides_of_the_lds_cap():
    sp = tr.two_vintage_specs()
    got = {st for _, st in sp.values()}
    assert got == {(True, True), (True, False), (False, False)}, got
    for fam in ("linreg", "linmodel3"):
        own = [(k, st) for k, (s, st) in sp.items() if s["lik"][0] == fam]
        assert {st for _, st in own} == {(True, True), (True, False), (False, False)}, own
    s, st = sp["linmodel3 64+64 X 3x64 (cap filled exactly)"]
    assert sum(tr.lik_doubles(s["lik"])) + sum(tr.lik_doubles(s["old_lik"])) == tr.LIK_LDS_CAP and st == (True, True)
    s, st = sp["linmodel3 64+64 X 3x65 (one double over)"]
    assert sum(tr.lik_doubles(s["lik"])) + sum(tr.lik_doubles(s["old_lik"])) == tr.LIK_LDS_CAP + 3 and st == (True, False)
    s, st = sp["linreg 192+193 (one row over)"]
    assert sum(tr.lik_doubles(s["lik"])) + sum(tr.lik_doubles(s["old_lik"])) == tr.LIK_LDS_CAP + 2 and st == (True, False)
    assert tr.staged(tr.linreg(384)) == (True, None) and tr.staged(tr.linreg(385)) == (False, None)
    assert tr.staged(tr.linmodel3(128)) == (True, None) and tr.staged(tr.linmodel3(129)) == (False, None)
    assert tr.staged(tr.capm(5)) == (False, None)                          # capm_literal is never staged (it reads its data as scalars)
    # the old vintage is evaluated the same way: on a spec whose two vintages are the same data the two columns are the same numbers
    s = sp["linmodel3 64, old T periods"][0]
    T = tr.target(s, tr.prior_draws(s, 8, 3))
    assert np.array_equal(T.ll, T.old)


def test_family_edges_on_the_oracle_and_on_cloudio():
    """After the fix: the oracle and host/cloudio.py return the reference's values at every family edge - no NaN, no exception."""
    import smc_jl_amd as S
    from smc_jl_amd.host import cloudio

    mk = dict(gamma=S.Gamma, beta=S.Beta, invgamma=S.InverseGamma, rootinvgamma=S.RootInverseGamma, normal=S.Normal, uniform=S.Uniform)
    why = []
    for c in tr.cases("family_edges"):
        T, oll, olp, ell, elp = _class_errors(c)
        ref64 = tr.f64(T.lp)
        fin = np.isfinite(ref64)
        if np.isnan(olp).any() or not np.array_equal(olp[~fin], ref64[~fin]) or not np.all(elp <= 1e-13):
            why.append("oracle, %s: %r against %r" % (c.label, olp[:2], ref64[:2]))
        for i in range(2):
            try:
                v = sum(cloudio.prior_logpdf(mk[p[0]](p[1], p[2]), float(c.theta[i, k])) for k, p in enumerate(c.spec["priors"]))
            except Exception as ex:   # noqa: BLE001
                why.append("cloudio, %s: %r" % (c.label, ex))
                continue
            if not (v == ref64[i] or (fin[i] and abs(v - ref64[i]) <= 1e-13 * max(1.0, float(T.lp_S[i])))):
                why.append("cloudio, %s: %r against %r" % (c.label, v, ref64[i]))
    assert not why, "\n".join(why)


def test_det_quirk_is_the_oracle_s_and_stays_outside_the_shipped_bounds():
    """linmodel3 / capm_literal form det = Π σ_i² before its log: it underflows (the value turns +Inf) for σ products below 1e-154 and overflows
    (-Inf) above 1e154.  The reference sums logs and stays finite; the oracle shares the quirk with the device.  Inside the shipped
    bounds [1e-5, 1e5] the product is within 1e-30 .. 1e30: nothing finite turns infinite there (the far class: σ at both bounds)."""
    c = tr.det_underflow_case()
    T, oll, olp, ell, elp = _class_errors(c)
    assert np.all(np.isfinite(tr.f64(T.ll)))
    assert np.all(oll[0::2] == np.inf) and np.all(oll[1::2] == -np.inf), oll
    for c in tr.cases("far"):
        if c.spec["lik"][0] in ("linmodel3", "capm_literal"):
            assert {1e-5, 1e5} <= set(c.theta[:, 2::3].ravel().tolist())
            assert np.all(np.isfinite(oracle_columns(c.spec, c.theta)[0]))
