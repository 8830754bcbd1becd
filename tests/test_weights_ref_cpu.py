"""tests/weights_ref.py pinned from two sides: against the CPU oracle where the oracle's unshifted exp is finite (all three
prior_weight forms), and against Python's `decimal` at 60 digits on small clouds with common offsets out to δ e = -2e7, where no
FP64 restatement of the reference survives.  Also here, because it is a condition on inputs and not a measurement: every cloud of
tests/test_gpu_weight_range.py keeps the reference's ESS above 50 n_para (a PosDef abort cannot be the cloud's fault) and the
matrix holds both resample outcomes.

Measured (x86-64, longdouble = 80-bit): largest relative error against 60-digit decimal over the cases below - ESS 2.5e-16,
normalised weights 2.1e-16, log-MDD increment 1.1e-16; the assertions ask 1e-13."""
import decimal
import math

import numpy as np
import pytest

from tests import weights_ref as wr


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def _cloud(rng, n, d=2):
    P = np.zeros((n, d + 5), order="F")
    P[:, d] = -50.0 * rng.random(n) - 3.0
    P[:, d + 2] = -40.0 * rng.random(n)
    P[:, d + 4] = rng.random(n) * 2.0
    P[:, d + 4] *= n / P[:, d + 4].sum()
    return P


@pytest.mark.parametrize("pw", [0.0, 1.0, 0.3])
def test_correct_ref_agrees_with_the_oracle_where_the_oracle_is_finite(orc, pw):
    rng = np.random.default_rng(11)
    n, d = 30000, 2
    P = _cloud(rng, n, d)
    P[::7, d + 4] = 0.0                                                  # zero weights stay zero
    P[5::1001, d] = -np.inf                                              # and a -Inf likelihood carries none
    P[:, d + 4] *= n / P[:, d + 4].sum()
    Q, inc, nw, ess, su = orc.correct(P, 0.35, 0.3, pw, -20.0)
    r = wr.correct_ref(P[:, d], P[:, d + 2], P[:, d + 4], 0.35, 0.3, pw, -20.0)
    assert r["ess"] == pytest.approx(ess, rel=1e-12)
    np.testing.assert_allclose(r["W"], nw, rtol=1e-12)
    np.testing.assert_allclose(r["w"], inc, rtol=1e-12)
    assert r["logz_inc"] == pytest.approx(math.log(su / n), rel=1e-12)
    assert r["resample"] == (ess < 0.5 * n)
    assert np.all(r["W"][::7] == 0.0) and np.all(r["W"][5::1001] == 0.0)
    if pw == 0.0:
        assert wr.ess_ref(P[:, d], P[:, d + 2], P[:, d + 4], 0.35, 0.3) == pytest.approx(
            orc.compute_ess(P[:, d], P[:, d + 4], 0.35, 0.3, P[:, d + 2]), rel=1e-12)


def _decimal_correct(loglh, old, W, phi_n, phi_prev, pw, logp_old):
    D = decimal.Decimal
    delta = D(phi_n) - D(phi_prev)
    L = []
    for ll, o, w in zip(loglh, old, W):
        if w == 0.0 or ll == -np.inf:
            L.append(None)
            continue
        if pw == 0.0:
            g = D(float(ll)) - D(float(o))
        elif pw == 1.0:
            g = D(float(ll))
        else:
            g = D(float(ll)) - ((D(float(o)) - D(logp_old) + (D(1) - D(pw)).ln()).exp() + D(pw)).ln()
        L.append(D(float(w)).ln() + delta * g)
    m = max(x for x in L if x is not None)
    wt = [D(0) if x is None else (x - m).exp() for x in L]
    s1, s2 = sum(wt), sum(x * x for x in wt)
    n = D(len(L))
    return s1 * s1 / s2, [x * n / s1 for x in wt], m + (s1 / n).ln()


@pytest.mark.parametrize("pw", [0.0, 1.0, 0.3])
def test_correct_ref_agrees_with_60_digit_decimal_at_any_offset(pw):
    worst = dict(ess=0.0, W=0.0, logz=0.0)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -decimal.MAX_EMAX, decimal.MAX_EMAX
        for k, dB in enumerate((0.0, 372.0, 745.0, 1e4, 2e7)):
            for sign in (1.0, -1.0):
                rng = np.random.default_rng(100 + k)
                n, delta = 600, 0.0625
                phi_prev, phi_n = 0.25, 0.25 + delta
                loglh = -sign * dB / delta - (5.0 / delta) * rng.random(n)
                old = -40.0 * rng.random(n) if pw != 1.0 else np.zeros(n)
                W = 2.0 * rng.random(n)
                W[3::50] = 0.0
                loglh[7::90] = -np.inf
                W *= n / W.sum()
                r = wr.correct_ref(loglh, old, W, phi_n, phi_prev, pw, -20.0)
                ess, Wn, logz = _decimal_correct(loglh, old, W, phi_n, phi_prev, pw, -20.0)
                worst["ess"] = max(worst["ess"], abs(float((decimal.Decimal(r["ess"]) - ess) / ess)))
                worst["logz"] = max(worst["logz"], abs(float((decimal.Decimal(r["logz_inc"]) - logz) / logz)))
                for a, b in zip(r["W"], Wn):
                    if b > decimal.Decimal("1e-290"):
                        worst["W"] = max(worst["W"], abs(float((decimal.Decimal(float(a)) - b) / b)))
                    else:
                        assert a <= 1e-289
                assert np.all(r["W"][3::50] == 0.0) and np.all(r["W"][7::90] == 0.0)
    print("weights_ref against 60-digit decimal, prior_weight %g: largest relative errors %r" % (pw, worst))
    assert worst["ess"] < 1e-13 and worst["W"] < 1e-13 and worst["logz"] < 1e-13, worst


def test_a_common_offset_changes_nothing_but_the_log_mdd_increment():
    delta = 0.125
    base = None
    for dB in wr.OFFSETS:
        for sign in (1.0, -1.0):
            ll, W = wr.knob_cloud(3000, delta, sign * dB, 5.0, seed=3, weights="random")
            r = wr.correct_ref(ll, None, W, 0.5 + delta, 0.5)
            if base is None:
                base = r
            # (the cloud itself moves in the last bits of e_i = -B - S u_i when B grows: ulp(B / δ) / S per particle)
            tol = 1e-13 + 4 * np.spacing(dB / delta) / (5.0 / delta) * 5.0
            assert r["ess"] == pytest.approx(base["ess"], rel=10 * tol)
            np.testing.assert_allclose(r["W"], base["W"], rtol=10 * tol)
            assert r["logz_inc"] + sign * dB == pytest.approx(base["logz_inc"], abs=1e-12 * max(1.0, dB))
            assert r["resample"] == base["resample"]


@pytest.mark.parametrize("case", ["first_stage", "mid_run", "after_resample", "reach_one", "long_scan"])
def test_solve_phi_ref_agrees_with_the_oracle(orc, case):
    rng = np.random.default_rng(7)
    n, d = 20000, 2
    P = _cloud(rng, n, d)
    P[:, d + 2] = 0.0
    n_phi = 300
    sched = (np.arange(n_phi) / (n_phi - 1.0)) ** 2.1
    if case == "first_stage":
        P[:, d + 4] = 1.0
        a = dict(j=2, phi_prop=0.0, phi_prev=0.0, ess_prev=float(n), rl=False)
    elif case == "mid_run":
        a = dict(j=140, phi_prop=sched[138], phi_prev=0.2, ess_prev=orc.compute_ess(P[:, d], P[:, d + 4], 0.2, 0.2), rl=False)
    elif case == "after_resample":
        P[:, d + 4] = 1.0
        a = dict(j=150, phi_prop=sched[148], phi_prev=0.23, ess_prev=0.4 * n, rl=True)
    elif case == "reach_one":
        P[:, d] = -1e-7 * rng.random(n)
        P[:, d + 4] = 1.0
        a = dict(j=290, phi_prop=sched[288], phi_prev=0.9, ess_prev=float(n), rl=True)
    else:
        P[:, d] = -0.05 * rng.random(n)
        P[:, d + 4] = 1.0
        a = dict(j=2, phi_prop=0.0, phi_prev=0.0, ess_prev=float(n), rl=False)
    want = orc.solve_adaptive_phi(P, a["ess_prev"], sched, a["j"], a["phi_prop"], a["phi_prev"], 0.97, a["rl"])
    got = wr.solve_phi_ref(P[:, d], P[:, d + 2], P[:, d + 4], sched, a["j"], a["phi_prop"], a["phi_prev"], 0.97, a["ess_prev"], a["rl"])
    assert got[0] == pytest.approx(want[0], rel=1e-10)
    assert got[1:] == (want[1], want[2], want[3])
    # and the root moves with 1 / scale when the energies are scaled, not at all with a common offset
    got2 = wr.solve_phi_ref(P[:, d] - 1e6, P[:, d + 2], P[:, d + 4], sched, a["j"], a["phi_prop"], a["phi_prev"], 0.97, a["ess_prev"], a["rl"])
    assert got2[0] == pytest.approx(got[0], rel=1e-9) and got2[1:] == got[1:]


def test_the_gpu_matrix_keeps_the_reference_ess_above_50_n_para_and_holds_both_resample_outcomes():
    """Condition on the inputs of tests/test_gpu_weight_range.py, checked with the helper alone: n_para = 10 there."""
    from tests import test_gpu_weight_range as T

    outcomes = set()
    n_cases = 0
    for name, make in T.input_clouds():
        loglh, old, W, phi_n, phi_prev, pw, logp_old, thr = make()
        r = wr.correct_ref(loglh, old, W, phi_n, phi_prev, pw, logp_old, thr)
        assert r["ess"] >= 50 * T.N_PARA, (name, r["ess"])
        outcomes.add(r["resample"])
        n_cases += 1
    assert outcomes == {True, False} and n_cases >= 100, (outcomes, n_cases)
