"""tests/moments_ref.py pinned against mpmath at 50 digits on clouds of a few hundred particles, at every knob; and, because they are
conditions on inputs and measurements of the reference's own arithmetic rather than of an engine:
  - the restatement's FP64 two-pass (oracle.weighted_cov) against tests/moments_ref.py on EVERY cloud tests/test_gpu_moment_range.py
    generates: its largest error sets that file's TOL (16 x, floor 1e-13), and each cloud stays within TOL / 16;
  - the reference factor of every stage cloud exists with pivots >= 1e-9 of the diagonal: a PosDef abort cannot be the cloud's fault.

Measured (x86-64, longdouble = 80-bit): tests/moments_ref.py against mpmath - mean 8.6e-20 of max(|mean|, σ), R 4.1e-19 of
sqrt(R_aa R_bb); the restatement against tests/moments_ref.py - 1.45e-9 at the most (tests/test_gpu_moment_range.py ORC_WORST), its
factor's steps 1.82e-11 (FACTOR_ORC_WORST); the smallest pivot of a stage cloud's factor is 1.0e-6 of its diagonal."""
import numpy as np
import pytest

from tests import moments_ref as mr
from tests import test_gpu_moment_range as T

LD = mr.LD


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def _against_mp(theta, W):
    import mpmath as mp

    m, R = mr.weighted_moments(theta, W)
    mm, RR = mr.mp_moments(theta, W)
    d = len(mm)
    with mp.workdps(50):
        sd = [mp.sqrt(RR[a][a]) for a in range(d)]
        e_mean = max(abs(mr._mpf_ld(m[a]) - mm[a]) / max(abs(mm[a]), sd[a]) for a in range(d))
        e_cov = max(abs(mr._mpf_ld(R[a, b]) - RR[a][b]) / (sd[a] * sd[b]) for a in range(d) for b in range(d))
        return float(e_mean), float(e_cov)


@pytest.mark.parametrize("weights", mr.WEIGHTS)
def test_reference_against_mpmath_at_every_knob(weights):
    worst = [0.0, 0.0]
    cases = [(k, "ones", 0.0) for k in mr.KAPPAS] + [((1e8, 1), "ones", 0.0)] + [(k, "spread", c) for k in (0.0, 1e4) for c in mr.CORRS[1:]]
    for i, (kappa, scales, corr) in enumerate(cases):
        n, d = (300, 4) if i % 2 else (257, 3)
        theta, W = mr.knob_cloud(n if weights != "degenerate" else 2000, d, kappa, scales, corr, weights, seed=i)
        e_mean, e_cov = _against_mp(theta, W)
        print(kappa, scales, corr, e_mean, e_cov)
        worst = [max(worst[0], e_mean), max(worst[1], e_cov)]
        assert e_mean <= 1e-18 and e_cov <= 1e-17, (kappa, scales, corr, e_mean, e_cov)
    print("largest errors against mpmath:", worst)


def test_the_sums_do_not_depend_on_the_order_of_the_particles():
    theta, W = mr.knob_cloud(4099, 5, 1e6, "spread", 0.99, "random", seed=3)
    m, R = mr.weighted_moments(theta, W)
    p = np.random.default_rng(0).permutation(4099)
    m2, R2 = mr.weighted_moments(theta[p], W[p])
    assert np.array_equal(m, m2)
    # (the covariance's chunk sums are rounded at 2^-64 of their terms: 1.4e-17 at the most, see the module docstring of tests/moments_ref.py)
    sd = np.sqrt(np.diag(R))
    assert float(np.max(np.abs(R - R2) / np.outer(sd, sd))) <= 1e-17
    x = (np.random.default_rng(1).standard_normal(1000) * 1e8).astype(LD) + LD(1) / LD(3)
    assert mr.exact_sum(x) == mr.exact_sum(x[::-1]) == mr.exact_sum(np.sort(x))


def test_knob_cloud_is_what_it_says():
    theta, W = mr.knob_cloud(20480, 6, (1e4, 2), "spread", 1.0 - 1e-6, "degenerate", seed=1)
    assert np.count_nonzero(W == 0.0) == 20480 - 205 and W.max() == pytest.approx(0.5 * 20480) and W.sum() == pytest.approx(20480.0)
    s = mr.column_scales(6, "spread")
    assert s[0] == pytest.approx(1e-6) and s[-1] == pytest.approx(1e6)
    z = theta / s[None, :]
    assert abs(z[:, 2].mean() - 1e4) < 0.1 and abs(z[:, 1].mean()) < 0.1
    assert np.corrcoef(z[:, 0], z[:, 1])[0, 1] == pytest.approx(1.0 - 1e-6, abs=2e-7)
    theta, W = mr.knob_cloud(5, 64, -1e8, weights="random")
    assert theta.shape == (5, 64) and np.all(theta < -9e7) and np.all(W > 0.0)


def _measure(i):
    """(name, the restatement's error, smallest pivot of the reference factor / its diagonal or None) of cloud i of T.input_clouds()"""
    name, is_stage, make = list(T.input_clouds())[i]
    theta, W = make()
    rm, rR = mr.weighted_moments(theta, W)
    e_cov = T.orc_error(theta, W, rm, rR)
    if not is_stage:
        return name, e_cov, None
    f = mr.chol_ref(rR)
    return name, e_cov, (f[2] if f is not None else -1.0)


def test_the_restatement_on_every_cloud_of_the_gpu_file_sets_its_tolerance(orc):
    """FP64 two-pass, the reference's own arithmetic: its largest error over every generated cloud is ORC_WORST (TOL = 16 x, floor 1e-13), each
    cloud within TOL / 16; every stage cloud's reference factor exists with pivots >= 1e-9 of the diagonal.  (Side by side in child processes.)"""
    from concurrent.futures import ProcessPoolExecutor

    n_clouds = sum(1 for _ in T.input_clouds())
    with ProcessPoolExecutor(max_workers=8) as ex:
        rows = list(ex.map(_measure, range(n_clouds), chunksize=4))
    worst, worst_name = max((e, name) for name, e, _ in rows)
    for name, e_cov, pivot in rows:
        assert e_cov <= T.TOL / 16.0, (name, e_cov)
        assert pivot is None or pivot >= 1e-9, (name, pivot)
    small_pivot = min(p for _, _, p in rows if p is not None)
    print("the restatement's largest error over %d clouds: %.3g (%s); smallest pivot of a stage cloud's factor: %.3g" % (n_clouds, worst, worst_name, small_pivot))
    # the recorded figure is the measured one (to the two digits it is written with): a change of the clouds has to move TOL with it
    assert worst <= T.ORC_WORST <= 1.25 * worst, (worst, T.ORC_WORST)


def test_the_restatements_factor_on_the_matrices_of_the_gpu_file_sets_the_step_tolerance(orc):
    """c L z with the restatement's own FP64 factor against the mpmath factor, on the matrices and draws tests/test_gpu_moment_range.py uses:
    the largest error is FACTOR_ORC_WORST (the device's tolerance is 16 x).  The matrix with a pivot of -1e-6 is not positive definite to the
    restatement either."""
    worst = 0.0
    for d in T.FACTOR_D:
        z = T.factor_draws(orc, d)
        for name, S in T.factor_matrices(d):
            f = mr.chol_ref(S)
            assert f is not None and f[2] >= 1e-9, (name, f and f[2])
            steps = np.array([orc.mixture_draw(np.zeros(d), np.zeros(d), S, T.FACTOR_C, 1.0, T.FACTOR_SEED, pid, T.FACTOR_STAGE, 0) for pid in range(T.FACTOR_N)])
            e = T.factor_error(steps, S, z)
            print(name, e, f[2])
            worst = max(worst, e)
    print("the restatement's largest step error: %.3g" % worst)
    assert worst <= T.FACTOR_ORC_WORST <= 1.25 * worst, (worst, T.FACTOR_ORC_WORST)
    S = T.not_positive_definite()
    assert mr.chol_ref(S) is None
    with pytest.raises(Exception, match="positive definite"):
        orc.mixture_draw(np.zeros(12), np.zeros(12), S, T.FACTOR_C, 1.0, T.FACTOR_SEED, 0, T.FACTOR_STAGE, 0)


def _measure_ensemble(i):
    from tests import test_gpu_ensemble_range as E

    name, make = list(E.moment_clouds())[i]
    theta, W = make()
    rm, rR = mr.weighted_moments(theta, W)
    f = mr.chol_ref(rR)
    return name, T.orc_error(theta, W, rm, rR), (f[2] if f is not None else -1.0)


def test_the_restatement_on_the_ensemble_clouds(orc):
    """The clouds of tests/test_gpu_ensemble_range.py (100 .. 8 192 particles, n_para 1 .. 10): every reference factor exists with pivots >= 1e-9
    of the diagonal, every cloud is within TOL / 16 (TOL stays the cap of the per-cloud bound), and the restatement's largest error over them is
    the figure recorded there as ENS_ORC_WORST."""
    from concurrent.futures import ProcessPoolExecutor

    from tests import test_gpu_ensemble_range as E

    n_clouds = sum(1 for _ in E.moment_clouds())
    with ProcessPoolExecutor(max_workers=8) as ex:
        rows = list(ex.map(_measure_ensemble, range(n_clouds), chunksize=4))
    worst, worst_name = max((e, name) for name, e, _ in rows)
    print("the restatement's largest error over %d ensemble clouds: %.3g (%s); smallest pivot: %.3g" % (n_clouds, worst, worst_name, min(p for _, _, p in rows)))
    for name, e_cov, pivot in rows:
        assert e_cov <= T.TOL / 16.0, (name, e_cov)
        assert pivot >= 1e-9, (name, pivot)
    assert worst <= E.ENS_ORC_WORST <= 1.25 * worst, (worst, E.ENS_ORC_WORST)
