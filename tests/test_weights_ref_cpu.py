"""tests/weights_ref.py pinned from two sides: against the CPU oracle where the oracle's unshifted exp is finite (all three
prior_weight forms), and against Python's `decimal` at 60 digits on small clouds with common offsets out to δ e = -2e7, where no
FP64 restatement of the reference survives.  Also here, because it is a condition on inputs and not a measurement: every cloud of
tests/test_gpu_weight_range.py keeps the reference's ESS above 50 n_para (a PosDef abort cannot be the cloud's fault) and the
matrix holds both resample outcomes.  The same for tests/test_gpu_ensemble_range.py, with the two helpers it rests on: chain_ref (the whole adaptive
run of a frozen cloud) against the oracle's own loop, zero_high_cloud (rows of weight 0 with the largest energy) against the cloud without those rows.

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


# ------------------------------------------------------------------------------------------------ the frozen chain and the zero-weight structure
def _sched30():
    return (np.arange(30) / 29.0) ** 2.1


def test_chain_ref_is_the_oracles_loop_on_a_frozen_cloud(orc):
    """chain_ref against the restatement's own solve_adaptive_ϕ + correction, stage after stage, on a cloud the restatement's unshifted exp holds
    (300 particles, spread 3): the same stages, the same schedule indices, ϕ to 1e-10, ESS / W / increments to 1e-12."""
    n, d = 300, 2
    e = wr.knob_cloud(n, 1.0, 0.0, 3.0, 43)[0]
    sched = _sched30()
    ch = wr.chain_ref(e, None, np.ones(n), sched, 0.9)
    P = np.zeros((n, d + 5), order="F")
    P[:, d], P[:, d + 4] = e, 1.0
    j, phi_prop, phi, ess_prev, rl = 2, 0.0, 0.0, float(n), False
    for s in ch:
        assert s["j_in"] == j
        phi_n, rl, j, phi_prop = orc.solve_adaptive_phi(P, ess_prev, sched, j, phi_prop, phi, 0.9, rl)[:4]
        Q, inc, nw, ess, su = orc.correct(P, phi_n, phi, 0.0, 0.0)
        assert s["phi"] == pytest.approx(phi_n, rel=1e-10) and (s["j"], s["phi_prop"]) == (j, phi_prop)
        # (the sums at the restatement's ϕ: the reference evaluated there)
        at = wr.correct_ref(e, None, P[:, d + 4], phi_n, phi)
        assert at["ess"] == pytest.approx(ess, rel=1e-12) and at["logz_inc"] == pytest.approx(math.log(su / n), rel=1e-12, abs=1e-15)
        np.testing.assert_allclose(at["W"], nw, rtol=1e-12)
        np.testing.assert_allclose(s["w"], inc, rtol=1e-9)
        P[:, d + 4], ess_prev, phi = nw, ess, phi_n
    assert phi == 1.0 and ch[-1]["phi"] == 1.0
    # evaluated at its own ϕ the chain repeats itself, bit for bit; and it refuses to resample
    at = wr.chain_at(e, None, np.ones(n), [s["phi"] for s in ch])
    assert [s["ess"] for s in at] == [s["ess"] for s in ch] and all(np.array_equal(a["W"], b["W"]) for a, b in zip(at, ch))
    with pytest.raises(ValueError):
        wr.chain_ref(e, None, np.ones(n), sched, 0.9, threshold_ratio=0.99)


def test_frozen_chains_of_the_issue_table():
    """knob_cloud(n, 1, 0, S, 43), n_phi = 30, λ = 2.1, never resampling (stages as a run counts them: the chain's + 1)"""
    for n, S, target, stages, min_ess in ((1024, 8.0, 0.9, 15, 249.9), (1000, 8.0, 0.95, 29, 244.5), (300, 3.0, 0.9, 6, 181.0)):
        ch = wr.chain_ref(wr.knob_cloud(n, 1.0, 0.0, S, 43)[0], None, np.ones(n), _sched30(), target)
        print(n, S, target, len(ch) + 1, min(s["ess"] for s in ch), ch[0]["phi"])
        assert len(ch) + 1 == stages and min(s["ess"] for s in ch) == pytest.approx(min_ess, abs=0.5)
        if n == 1024:
            assert ch[0]["phi"] == pytest.approx(0.14625, abs=1e-5)


def test_zero_high_cloud_is_the_cloud_without_those_rows():
    """Rows of weight 0 with the largest energy: the reference's ESS, W and increment are those of the cloud with the rows removed (the increment
    corrected for N), their W is exactly 0, every output is finite - at every δΔ, far past the range of a shifted exp."""
    assert list(wr.default_zero_rows(100)) == list(range(8)) + [97, 98, 99]
    assert list(wr.default_zero_rows(1024)) == list(range(8)) + [255, 256, 1021, 1022, 1023]
    assert wr.default_zero_rows(8192).size == 13 + 512 and set(range(1536, 2048)) <= set(wr.default_zero_rows(8192))
    for n in (100, 1024, 8192):
        rows = wr.default_zero_rows(n)
        live = np.ones(n, dtype=bool)
        live[rows] = False
        for delta in (1.0, 0.125):
            for dD in (0.0, 300.0, 700.0, 709.0, 710.0, 745.0, 800.0, 1e4, 1e6):
                ll, W = wr.zero_high_cloud(n, delta, dD, 0.5 / delta, 46)
                assert np.all(W[rows] == 0.0) and np.all(ll[rows] == 0.0) and W.sum() == pytest.approx(n) and np.all(W[live] > 0.0)
                assert ll[live].mean() == pytest.approx(-dD / delta, abs=0.5 / delta)
                r = wr.correct_ref(ll, None, W, 0.5 + delta, 0.5)
                q = wr.correct_ref(ll[live], None, W[live], 0.5 + delta, 0.5)
                nl = int(live.sum())
                assert r["ess"] == pytest.approx(q["ess"], rel=1e-14)
                np.testing.assert_allclose(r["W"][live], q["W"] * (n / nl), rtol=1e-14)
                assert r["logz_inc"] == pytest.approx(q["logz_inc"] + math.log(nl / n), rel=1e-14, abs=1e-14)
                assert np.all(r["W"][rows] == 0.0) and np.all(r["w"][rows] == 1.0)
                assert np.isfinite(r["ess"]) and np.isfinite(r["logz_inc"]) and np.all(np.isfinite(r["W"])) and np.all(np.isfinite(r["w"]))


def test_the_ensemble_matrix_keeps_the_reference_ess_above_50_n_para():
    """Conditions on the inputs of tests/test_gpu_ensemble_range.py, with the helper alone: every one-stage cloud, and every stage of every frozen
    chain; the chains have the shapes the file's docstring says (stage counts, the walk across solver passes, the walk off the schedule's end)."""
    from tests import test_gpu_ensemble_range as T

    n_cases, outcomes = 0, set()
    for name, n_para, make in T.input_clouds():
        loglh, old, W, thr = make()
        r = wr.correct_ref(loglh, old, W, 1.0, 0.0, 0.0, 0.0, thr)
        assert r["ess"] >= 50 * n_para, (name, r["ess"])
        outcomes.add(r["resample"])
        n_cases += 1
    assert outcomes == {True, False} and n_cases >= 700, (outcomes, n_cases)
    want = {"n1024_S8": (15, 249.9), "n1000_S8_target095": (29, 244.5), "n300_S3_walk_across_passes": (6, 181.4), "n257_S3": (6, 153.6), "n100_S3": (6, 59.1),
            "n8192_S8_npara10": (15, 2051.8), "n8192_S200_many_small_steps": (44, 95.2)}
    assert set(want) == set(T.FROZEN)
    n_phi = T.ADAPT["n_phi"]
    for name, f in T.FROZEN.items():
        ch = T.frozen_chain(name)
        ess = min(s["ess"] for s in ch)
        print(name, len(ch) + 1, ess, [(s["j_in"], s["j"]) for s in ch[:3]], [(s["j_in"], s["j"]) for s in ch[-2:]])
        assert ess >= 50 * f["d"], (name, ess)
        assert (len(ch) + 1, pytest.approx(want[name][1], abs=0.06)) == (want[name][0], ess), (name, len(ch) + 1, ess)
        # the last stage walks off the end of the schedule: j = n_phi + 1 on entry (no point left) or reached within the stage, and ϕ = 1
        assert ch[-1]["phi"] == 1.0 and ch[-1]["j"] == n_phi + 1 and ch[-1]["phi_prop"] == 1.0
    walk = T.frozen_chain("n300_S3_walk_across_passes")[0]
    assert walk["j_in"] == 2 and walk["j"] >= 18                      # past the 8th and the 16th schedule point within one stage
    assert any(s["j_in"] == n_phi + 1 for s in T.frozen_chain("n1024_S8"))
    eq = T.frozen_chain("n1024_S8", "equal")
    assert len(eq) == 1 and eq[0]["phi"] == 1.0 and eq[0]["ess"] == 1024.0
