"""tests/kalman_ref.py pinned against mpmath at 40 digits, and the conditions on the inputs of tests/test_gpu_kalman_range.py that need no
GPU: on every class and variant the FP64 oracle (oracle/smc_oracle.c orc_kalman_lgss - the oracle itself, no restatement) returns a finite value
for every θ, and at most 3 of the 24 θ are left out of the device checks because the oracle is off by more than 1e-10 there.

Normalised errors |Δll| / max(1, S), S as tests/kalman_ref.py defines it.  Measured (x86-64, longdouble = 80-bit; 24 θ per class for the oracle,
two θ per class for the pin, at the class's longest T):

  class / variant            oracle worst          left out   longdouble against mpmath
  prior T=80 / 400           2.5e-15 / 3.4e-15     0          2.2e-18
  snr T=80 / 400             1.1e-13 / 4.7e-13     0          1.4e-17
  quiet T=80                 5.2e-16               0          9.3e-19
  roots_mixed T=80           1.1e-15               0          7.2e-19
  roots_pos T=80 / 400       1.3e-14 / 2.7e-11     0 / 1      4.7e-18   (the θ left out at T = 400: the oracle is off by 5.0e-9)
  all_edges T=80             3.9e-14               0          4.9e-19
  mu_far T=80 / 400          3.4e-13 / 2.0e-13     0          3.9e-18
  short T=1 / 2 / 3 / 41     4.7e-16 .. 2.6e-15    0          3.6e-19   (T = 41)
  data_scale y*1e6 / y*1e-6  2.8e-15 / 2.2e-15     0          1.7e-18
  dense_structure (both κ)   2.4e-14 / 7.7e-15     0          8.3e-19
  diagonal T=80              7.0e-16               0          6.0e-19   (the same against three scalar AR(1)-plus-noise recursions in mpmath)

The pin asked of the reference in every class: 6.25e-17 = 1e-3 of the floor 1e-12 of the device bar over its factor 16, so 1e-3 of the smallest
oracle error that can set a bar - the reference's own error is invisible in every device check, and far below the oracle's error in every class but
the two where the oracle itself is at a few 1e-16 (quiet, diagonal: still a factor 500 and more)."""
import mpmath
import numpy as np
import pytest

from tests import kalman_ref as kr

PIN = 1e-3 * kr.FLOOR / kr.FACTOR


def _mp_filter(th, y, C, R, Z, kappa, nt_mid=0):
    """the textbook filter on one θ in mpmath (the working precision is the caller's): (ll, ll_mid, S)"""
    mp, f = mpmath.mp, mpmath.mpf
    th = [f(float(v)) for v in th]
    T = y.shape[1]
    Cm = [[f(float(C[i, j])) for j in range(8)] for i in range(8)]
    Rm = [[f(float(R[i, m])) for m in range(3)] for i in range(8)]
    Zm = [[f(float(Z[a, j])) for j in range(8)] for a in range(3)]
    k = f(float(kappa))
    Tm = [[k * Cm[i][j] + (th[i] if i == j else 0) for j in range(8)] for i in range(8)]
    Q = [[mp.fsum(Rm[i][m] * th[8 + m] ** 2 * Rm[j][m] for m in range(3)) for j in range(8)] for i in range(8)]
    se2, mu = th[11] ** 2, th[12]
    x = [f(0)] * 8
    P = [[f(1 if i == j else 0) for j in range(8)] for i in range(8)]
    ll, S, ll_mid = f(0), f(0), None
    c = f(3) / 2 * mp.log(2 * mp.pi)
    for t in range(T):
        x = [mp.fdot(Tm[i], x) for i in range(8)]
        PT = list(zip(*P))
        TP = [[mp.fdot(Tm[i], PT[j]) for j in range(8)] for i in range(8)]
        P = [[mp.fdot(TP[i], Tm[j]) + Q[i][j] for j in range(8)] for i in range(8)]
        P = [[(P[i][j] + P[j][i]) / 2 for j in range(8)] for i in range(8)]
        v = [f(float(y[a, t])) - mu - mp.fdot(Zm[a], x) for a in range(3)]
        PZ = [[mp.fdot(P[i], Zm[a]) for a in range(3)] for i in range(8)]
        PZT = list(zip(*PZ))
        F = [[mp.fdot(Zm[a], PZT[b]) + (se2 if a == b else 0) for b in range(3)] for a in range(3)]
        l00 = mp.sqrt(F[0][0])
        l10, l20 = F[1][0] / l00, F[2][0] / l00
        l11 = mp.sqrt(F[1][1] - l10 * l10)
        l21 = (F[2][1] - l20 * l10) / l11
        l22 = mp.sqrt(F[2][2] - l20 * l20 - l21 * l21)
        w0 = v[0] / l00
        w1 = (v[1] - l10 * w0) / l11
        w2 = (v[2] - l20 * w0 - l21 * w1) / l22
        hld = mp.log(l00 * l11 * l22)
        q = (w0 * w0 + w1 * w1 + w2 * w2) / 2
        ll -= c + hld + q
        S += c + abs(hld) + q
        if t + 1 == nt_mid:
            ll_mid = ll
        G = []
        for i in range(8):
            g0 = PZ[i][0] / l00
            g1 = (PZ[i][1] - l10 * g0) / l11
            G.append((g0, g1, (PZ[i][2] - l20 * g0 - l21 * g1) / l22))
        x = [x[i] + G[i][0] * w0 + G[i][1] * w1 + G[i][2] * w2 for i in range(8)]
        P = [[P[i][j] - (G[i][0] * G[j][0] + G[i][1] * G[j][1] + G[i][2] * G[j][2]) for j in range(8)] for i in range(8)]
    return ll, ll_mid, S


def _mp_scalar_ar1(rho, q, se2, mu, ys):
    """log-likelihood of y_t = μ + x_t + u_t, x_t = ρ x_{t-1} + e_t, var e = q, var u = se2, x_0 = 0, p_0 = 1"""
    mp, f = mpmath.mp, mpmath.mpf
    x, p, ll = f(0), f(1), f(0)
    for yt in ys:
        x, p = rho * x, rho * rho * p + q
        fv, v = p + se2, f(float(yt)) - mu - x
        ll -= (mp.log(2 * mp.pi * fv) + v * v / fv) / 2
        x, p = x + p / fv * v, p - p * p / fv
    return ll


def _ld_err(a_ld, b_mp, S_mp):
    """|a - b| / max(1, S), a longdouble (split exactly into two doubles), b and S mpmath"""
    hi = float(a_ld)
    lo = float(a_ld - np.longdouble(hi))
    return float(abs(mpmath.mpf(hi) + mpmath.mpf(lo) - b_mp) / max(mpmath.mpf(1), S_mp))


_ORC = {}


def oracle_errors(name):
    """{variant label: (oracle values, normalised errors against the reference)} over the class's 24 θ, computed once"""
    if name not in _ORC:
        th = kr.thetas(name)
        out = {}
        for v in kr.variants(name):
            ref = kr.loglik(th, v.y, v.C, v.R, v.Z, v.kappa)
            got = kr.oracle_loglik(v, th)
            out[v.label] = (got, kr.nerr(got, ref.ll, ref.S), ref)
        _ORC[name] = out
    return _ORC[name]


@pytest.mark.parametrize("name", kr.CLASSES)
def test_oracle_is_finite_and_close_on_every_class(name):
    """The condition on the inputs: no θ at which the oracle returns -Inf, at most 3 of 24 left out (oracle off by more than 1e-10)."""
    for label, (got, err, ref) in oracle_errors(name).items():
        inc, b, worst = kr.bar(err)
        print("%s %s: oracle worst %.3g (all: %.3g), left out %d, bar %.3g, S in [%.3g, %.3g]" % (name, label, worst, err.max(), int((~inc).sum()), b, float(ref.S.min()), float(ref.S.max())))
        assert np.all(np.isfinite(got)), (name, label, got)
        assert np.all(np.isfinite(ref.ll.astype(np.float64))), (name, label)
        assert int((~inc).sum()) <= kr.MAX_LEFT_OUT, (name, label, err)


@pytest.mark.parametrize("name", kr.CLASSES)
def test_longdouble_filter_against_mpmath_at_40_digits(name):
    """Two θ per class at the class's longest data (T = 400 where it has one), every variant of the classes with their own data or structure;
    the value after nt_mid steps with it."""
    th = kr.thetas(name)[:2]
    vs = kr.variants(name)
    if name in kr.CLASS_T:
        vs = vs[-1:]
    with mpmath.workdps(40):
        for v in vs:
            T = v.y.shape[1]
            mid = max(1, T // 2)
            ref = kr.loglik(th, v.y, v.C, v.R, v.Z, v.kappa, nt_mid=mid)
            pin = PIN
            for i in range(2):
                ll, ll_mid, S = _mp_filter(th[i], v.y, v.C, v.R, v.Z, v.kappa, nt_mid=mid)
                e, em = _ld_err(ref.ll[i], ll, S), _ld_err(ref.ll_mid[i], ll_mid, S)
                es = float(abs(mpmath.mpf(float(ref.S[i])) - S) / S)
                print("%s %s theta %d: ll %.6g S %.4g  error %.3g (mid %.3g), pin %.3g, S off %.3g" % (name, v.label, i, float(ll), float(S), e, em, pin, es))
                assert e <= pin and em <= pin, (name, v.label, i, e, em, pin)
                assert es <= 1e-12
                if name == "diagonal":                     # three independent scalar filters: states 0, 3, 6 with shocks 0, 1, 2
                    f = mpmath.mpf
                    tot = f(0)
                    for a, s in enumerate((0, 3, 6)):
                        r = f(float(v.R[s, a]))
                        tot += _mp_scalar_ar1(f(float(th[i, s])), (r * f(float(th[i, 8 + a]))) ** 2, f(float(th[i, 11])) ** 2, f(float(th[i, 12])), v.y[a])
                    es = _ld_err(ref.ll[i], tot, S)
                    print("   against the scalar recursions: %.3g" % es)
                    assert es <= pin and abs(tot - ll) / max(1, S) <= 1e-30


def test_generators_are_deterministic_and_in_bounds():
    from tests import models

    bnd = np.array(models.kalman_spec()["bounds"])
    for name in kr.CLASSES:
        a, b = kr.thetas(name), kr.thetas(name, 300)
        assert np.array_equal(a, b[:kr.N_CLASS]) and np.array_equal(a, kr.thetas(name))
        assert np.all(b >= bnd[:, 0]) and np.all(b <= bnd[:, 1]), name
        for i, th in enumerate(b):
            for k, (lo, hi) in kr.BOXES[name][i % len(kr.BOXES[name])].items():
                assert lo <= th[k] <= hi, (name, i, k)
    assert np.all(np.abs(kr.thetas("mu_far")[:, 12]) >= 1e3) and np.abs(kr.thetas("mu_far")[:, 12]).max() == 1e5
    C, R, Z = kr.dense_structure()
    assert np.abs(C).max() <= 0.5 and np.all(R != 0.0)
    assert np.array_equal(models.kalman_data(400)[:, :80], models.kalman_data(80))


def test_reference_prefix_value_is_the_value_of_a_separate_pass():
    th = kr.thetas("prior")[:4]
    v = kr.variants("prior")[0]
    for mid in (1, 40, 79, 80):
        a = kr.loglik(th, v.y, v.C, v.R, v.Z, v.kappa, nt_mid=mid)
        b = kr.loglik(th, v.y[:, :mid], v.C, v.R, v.Z, v.kappa)
        assert np.array_equal(a.ll_mid, b.ll) and np.array_equal(a.S_mid, b.S)
