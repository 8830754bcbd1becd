"""An independent reference for the target of every MH decision - the log-prior of the six prior families and the log-likelihood of the four
closed-form families (csrc/model.hpp prior_logpdf / logprior / logprior_s, loglik / loglik_s; restated in oracle/smc_oracle.c and, for the priors,
in host/cloudio.py) - and the seeded inputs the tests evaluate it on.  No device, no oracle: mpmath at 50 digits for the priors (and, vectorised
for the large clouds, numpy longdouble with mpmath's constants - pinned against the mpmath statement by tests/test_target_ref_cpu.py), numpy
longdouble for the likelihoods (pinned against a per-period mpmath evaluation there).

Priors, as Distributions.jl / ModelConstructors define them (the ModelConstructors formula of RootInverseGamma: host/cloudio.py):
  Normal(μ, σ)            -log σ - log(2π)/2 - ((x - μ)/σ)²/2
  Uniform(a, b)           -log(b - a) on [a, b]
  Gamma(a, scale b)       -lnΓ(a) - a log b + (a - 1) log x - x/b              x >= 0
  Beta(a, b)              -lnB(a, b) + (a - 1) log x + (b - 1) log(1 - x)      0 <= x <= 1
  InverseGamma(a, b)      a log b - lnΓ(a) - (a + 1) log x - b/x               x > 0
  RootInverseGamma(ν, τ)  log 2 - lnΓ(ν/2) + (ν/2) log(ν τ²/2) - (ν + 1) log x - ν τ²/(2 x²)     x > 0
Edges (xlogy, xlog1py): a factor 0 times log 0 is 0; outside the support -Inf; a negative factor times log 0 is +Inf (Gamma(a < 1) at 0,
Beta(a < 1, .) at 0, Beta(., b < 1) at 1) and a positive one -Inf.  A value beyond the FP64 range is that infinity.

Model rules: logprior sums over the free parameters; in_bounds is closed and NaN is outside; outside the bounds all three columns are -Inf.

Every value comes with its scale S, the sum of the absolute values of the terms its formula adds (prior: each parameter's constant and its
x-dependent terms; likelihood: Σ_t |term1| + |q_t|/2 or the family's equivalent), and every error is |Δ| / max(1, S) (tests/kalman_ref.py's
convention).
"""
import collections
import math
import zlib

import mpmath as mp
import numpy as np

from tests import models

DPS = 50
dps50 = mp.workdps(DPS)         # every mpmath entry point below runs at 50 digits whatever the process-wide precision is (a decorator; callers
                                # that go on computing with the returned mpf values do so inside `with mp.workdps(DPS)` themselves)
LD = np.longdouble
DBL_MAX = 1.7976931348623157e308
N_CLASS = 24                  # θ per class
ORC_LIMIT = 1e-10             # a θ at which the FP64 oracle is off by more than this (normalised) is left out: conditioning, not a kernel's fault
MAX_LEFT_OUT = 3              # of 24 (the same share of a larger cloud)
FLOOR = 1e-13                 # tests/test_gpu_moment_range.py's floor
FACTOR = 16.0                 # another summation order, the device's log / exp
LIK_LDS_CAP = 768             # doubles of likelihood data csrc/kernels.hpp stage_lik keeps in LDS


def _seed(*what):
    return zlib.crc32(repr(what).encode())


# ------------------------------------------------------------------------------------------------ priors
def _xlogy(c, y):
    """c log y for y >= 0 with 0 log 0 = 0"""
    if c == 0:
        return mp.mpf(0)
    if y == 0:
        return -mp.sign(c) * mp.inf
    return c * mp.log(y)


@dps50
def prior_terms_mp(fam, a, b, x):
    """(constant, [x-dependent terms]) of one prior's log-density at the double x, mpmath; ([-inf]) outside the support"""
    x = float(x)
    if x != x:
        return mp.mpf(0), [mp.nan]
    a, b, xm = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(x)
    out = (mp.mpf(0), [-mp.inf])
    if fam == "normal":
        return -mp.log(b) - mp.log(2 * mp.pi) / 2, [-((xm - a) / b) ** 2 / 2]
    if fam == "uniform":
        return (-mp.log(b - a), [mp.mpf(0)]) if a <= xm <= b else out
    if fam == "gamma":
        return (-mp.loggamma(a) - a * mp.log(b), [_xlogy(a - 1, xm), -xm / b]) if x >= 0 else out
    if fam == "beta":
        if not 0 <= x <= 1:
            return out
        t1 = mp.mpf(0) if b == 1 else (-mp.sign(b - 1) * mp.inf if x == 1 else (b - 1) * mp.log1p(-xm))
        return -(mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)), [_xlogy(a - 1, xm), t1]
    if fam == "invgamma":
        return (a * mp.log(b) - mp.loggamma(a), [-(a + 1) * mp.log(xm), -b / xm]) if x > 0 else out
    if fam == "rootinvgamma":
        return (mp.log(2) - mp.loggamma(a / 2) + (a / 2) * mp.log(a * b * b / 2), [-(a + 1) * mp.log(xm), -a * b * b / (2 * xm * xm)]) if x > 0 else out
    raise KeyError(fam)


def _to_f64(v):
    """the double nearest to an mpf; beyond the FP64 range that infinity"""
    if mp.isnan(v):
        return math.nan
    if mp.isinf(v) or abs(v) > DBL_MAX:
        return math.inf if v > 0 else -math.inf
    return float(v)


@dps50
def _to_ld(v):
    f = _to_f64(v)
    if not math.isfinite(f):
        return LD(f)
    return LD(f) + LD(float(v - mp.mpf(f)))


@dps50
def prior_logpdf_mp(fam, a, b, x):
    """(log-density, S) of one prior at x: mpf (or ±inf / nan) and mpf"""
    c, ts = prior_terms_mp(fam, a, b, x)
    v, S = c, abs(c)
    for t in ts:
        v, S = v + t, S + abs(t)
    return v, S


def in_bounds(spec, theta):
    """closed intervals; NaN is outside"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    lo, hi = np.array([b[0] for b in spec["bounds"]]), np.array([b[1] for b in spec["bounds"]])
    with np.errstate(invalid="ignore"):
        return np.all((lo <= theta) & (theta <= hi), axis=1)


def _free(spec):
    fx = spec.get("fixed") or [0] * len(spec["priors"])
    return [k for k in range(len(spec["priors"])) if not fx[k]]


@dps50
def logprior_mp(spec, theta):
    """Σ over the free parameters, in mpmath -> (values, S) as longdouble arrays; the bounds are NOT applied"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    val, S = np.empty(len(theta), dtype=LD), np.empty(len(theta), dtype=LD)
    for i, th in enumerate(theta):
        v, s = mp.mpf(0), mp.mpf(0)
        for k in _free(spec):
            fam, a, b = spec["priors"][k]
            vk, sk = prior_logpdf_mp(fam, a, b, th[k])
            v, s = v + vk, s + sk
        val[i], S[i] = _to_ld(v), (_to_ld(s) if mp.isfinite(s) else LD(np.inf))
    return val, S


@dps50
def logprior_ld(spec, theta):
    """the same sum vectorised in longdouble (the constants from mpmath) for clouds too large for mpmath"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    val, S = np.zeros(len(theta), dtype=LD), np.zeros(len(theta), dtype=LD)
    inf = LD(np.inf)
    with np.errstate(all="ignore"):
        for k in _free(spec):
            fam, a, b = spec["priors"][k]
            x = theta[:, k].astype(LD)
            c = _to_ld(prior_terms_mp(fam, a, b, {"beta": 0.5, "uniform": a}.get(fam, 1.0))[0])
            a, b = LD(a), LD(b)

            def xlogy(f, y):
                return np.zeros_like(y) if f == 0 else np.where(y == 0, -np.sign(f) * inf, f * np.log(np.where(y > 0, y, 1)))

            if fam == "normal":
                ts, ok = [-((x - a) / b) ** 2 / 2], np.ones(len(x), dtype=bool)
            elif fam == "uniform":
                ts, ok = [np.zeros_like(x)], (a <= x) & (x <= b)
            elif fam == "gamma":
                ts, ok = [xlogy(a - 1, x), -x / b], x >= 0
            elif fam == "beta":
                ok = (x >= 0) & (x <= 1)
                ts = [xlogy(a - 1, x), np.zeros_like(x) if b == 1 else np.where(x == 1, -np.sign(b - 1) * inf, (b - 1) * np.log1p(-np.where(ok & (x < 1), x, 0)))]
            elif fam == "invgamma":
                ok = x > 0
                xs = np.where(ok, x, 1)
                ts = [-(a + 1) * np.log(xs), -b / xs]
            elif fam == "rootinvgamma":
                ok = x > 0
                xs = np.where(ok, x, 1)
                ts = [-(a + 1) * np.log(xs), -a * b * b / (2 * xs * xs)]
            else:
                raise KeyError(fam)
            v, s = c + sum(ts), abs(c) + sum(np.abs(t) for t in ts)
            val, S = val + np.where(ok, v, -inf), S + np.where(ok, s, inf)
            val = np.where(np.isnan(theta[:, k]), LD(np.nan), val)
    return val, S


def logprior(spec, theta):
    """(values, S): mpmath up to 2048 rows, longdouble beyond; bounds not applied"""
    theta = np.atleast_2d(theta)
    return logprior_mp(spec, theta) if len(theta) <= 2048 else logprior_ld(spec, theta)


# ------------------------------------------------------------------------------------------------ likelihoods
_LOG2PI = LD(0)


@dps50
def _log2pi():
    global _LOG2PI
    if _LOG2PI == 0:
        _LOG2PI = _to_ld(mp.log(2 * mp.pi))
    return _LOG2PI


def loglik(lik, theta):
    """(values, S) of the rows of theta under lik = (family, par, data, aux), as csrc/model.hpp documents the families; longdouble.
    linreg: data = [y X] (n x 2).  linmodel3: data 3 x T, aux = X, 3 x (>= T), of which X[:, 1:T] is read.  capm_literal (quirk Q12):
    T term1 - T S / 2 with S = Σ_t Σ_i (y_it - α_i - α_i mk_t)² / σ_i² over ALL periods, mk_t the first row of aux."""
    fam, par, data, aux = lik
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64)).astype(LD)
    n, l2p = len(th), _log2pi()
    with np.errstate(all="ignore"):
        if fam == "gauss_iso":
            sig, m = LD(float(par[0])), np.asarray(data, dtype=np.float64).ravel(order="F").astype(LD)
            d = th.shape[1]
            c0 = -(LD(d) / 2) * (l2p + 2 * np.log(sig))
            t = (th - m[None, :d]) ** 2 / (2 * sig * sig)
            return c0 - t.sum(axis=1), abs(c0) + t.sum(axis=1)
        if fam == "linreg":
            D = np.asarray(data, dtype=np.float64)
            y, X, s2, N = D[:, 0].astype(LD), D[:, 1].astype(LD), LD(float(par[0])), LD(D.shape[0])
            e = y[None, :] - th[:, :1] - th[:, 1:2] * X[None, :]
            q = (e * e).sum(axis=1) / (2 * s2)
            return -(N / 2) * l2p - (N / 2) * np.log(s2) - q, (N / 2) * l2p + abs((N / 2) * np.log(s2)) + q
        if fam in ("linmodel3", "capm_literal"):
            Y = np.asarray(data, dtype=np.float64).astype(LD)
            T = Y.shape[1]
            A = np.asarray(aux, dtype=np.float64).astype(LD)
            a, b, s = th[:, 0::3], th[:, 1::3], th[:, 2::3]
            dead = np.any(s == 0, axis=1)
            s = np.where(s == 0, 1, s)
            logdet = 2 * np.log(np.abs(s)).sum(axis=1)
            if fam == "linmodel3":
                e = Y[None, :, :] - a[:, :, None] - b[:, :, None] * A[None, :3, :T]
            else:
                e = Y[None, :, :] - a[:, :, None] - a[:, :, None] * A[None, :1, :T]
            q = ((e / s[:, :, None]) ** 2).sum(axis=(1, 2)) / 2
            if fam == "capm_literal":
                q = q * T
            v = -LD(T) * (LD(1.5) * l2p + logdet / 2) - q
            S = LD(T) * (LD(1.5) * l2p + abs(logdet / 2)) + q
            return np.where(dead, -LD(np.inf), v), np.where(dead, LD(np.inf), S)
    raise KeyError(fam)


@dps50
def loglik_mp(lik, th):
    """one row, written per period in mpmath -> (value, S) as mpf (the second statement tests/test_target_ref_cpu.py pins loglik against)"""
    fam, par, data, aux = lik
    th = [mp.mpf(float(x)) for x in th]
    l2p = mp.log(2 * mp.pi)
    M = lambda x: mp.mpf(float(x))
    if fam == "gauss_iso":
        m, sig = np.asarray(data, dtype=np.float64).ravel(order="F"), M(par[0])
        c0 = -mp.mpf(len(th)) / 2 * mp.log(2 * mp.pi * sig * sig)
        ts = [(th[k] - M(m[k])) ** 2 / (2 * sig * sig) for k in range(len(th))]
        return c0 - mp.fsum(ts), abs(c0) + mp.fsum(ts)
    if fam == "linreg":
        D, s2 = np.asarray(data, dtype=np.float64), M(par[0])
        v = S = mp.mpf(0)
        for t in range(D.shape[0]):
            q = (M(D[t, 0]) - th[0] - th[1] * M(D[t, 1])) ** 2 / (2 * s2)
            v, S = v - l2p / 2 - mp.log(s2) / 2 - q, S + l2p / 2 + abs(mp.log(s2) / 2) + q
        return v, S
    Y, A = np.asarray(data, dtype=np.float64), np.asarray(aux, dtype=np.float64)
    T = Y.shape[1]
    if any(th[3 * i + 2] == 0 for i in range(3)):
        return -mp.inf, mp.inf
    term1 = -mp.mpf(3) / 2 * l2p - mp.fsum(mp.log(th[3 * i + 2] ** 2) for i in range(3)) / 2
    a1 = mp.mpf(3) / 2 * l2p + abs(mp.fsum(mp.log(th[3 * i + 2] ** 2) for i in range(3)) / 2)
    qs = []
    for t in range(T):
        if fam == "linmodel3":
            qs.append(mp.fsum((M(Y[i, t]) - th[3 * i] - th[3 * i + 1] * M(A[i, t])) ** 2 / th[3 * i + 2] ** 2 for i in range(3)))
        else:
            qs.append(mp.fsum((M(Y[i, t]) - th[3 * i] - th[3 * i] * M(A[0, t])) ** 2 / th[3 * i + 2] ** 2 for i in range(3)))
    if fam == "capm_literal":
        Sq = mp.fsum(qs)
        qs = [Sq] * T
    return mp.fsum(term1 - q / 2 for q in qs), mp.fsum(a1 + q / 2 for q in qs)


Target = collections.namedtuple("Target", "inb ll ll_S lp lp_S old old_S")


def target(spec, theta):
    """the three columns at the rows of theta: loglh, logprior and old_loglh (0 without an old vintage), each with its scale; rows outside the
    bounds hold -Inf in all three"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if len(theta) > 8192:                                   # (blocks: the likelihoods hold rows x periods longdoubles at a time)
        parts = [target(spec, theta[i:i + 8192]) for i in range(0, len(theta), 8192)]
        return Target(*[np.concatenate([p[j] for p in parts]) for j in range(7)])
    inb = in_bounds(spec, theta)
    safe = np.where(inb[:, None], theta, np.array([b[0] for b in spec["bounds"]])[None, :])
    ll, ll_S = loglik(spec["lik"], safe)
    lp, lp_S = logprior(spec, safe)
    if spec.get("old_lik") is not None:
        old, old_S = loglik(spec["old_lik"], safe)
    else:
        old, old_S = np.zeros(len(theta), dtype=LD), np.zeros(len(theta), dtype=LD)
    ninf = -LD(np.inf)
    return Target(inb, np.where(inb, ll, ninf), ll_S, np.where(inb, lp, ninf), lp_S, np.where(inb, old, ninf), old_S)


def f64(v):
    """a longdouble reference as the FP64 column it is compared with: beyond the FP64 range that infinity"""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=LD).astype(np.float64)


def nerr(got, ref, S):
    """|got - ref| / max(1, S) per row (float64).  Where the reference is ±Inf (as a double): 0 if `got` is the same infinity, Inf if not;
    where it is finite and `got` is not: Inf."""
    got, ref64 = np.asarray(got, dtype=np.float64), f64(ref)
    with np.errstate(all="ignore"):
        e = (np.abs(got.astype(LD) - ref) / np.maximum(LD(1.0), np.where(np.isfinite(S), S, LD(1.0)))).astype(np.float64)
    fin = np.isfinite(ref64)
    return np.where(fin, np.where(np.isfinite(got), e, np.inf), np.where(got == ref64, 0.0, np.inf))


def bar(orc_err):
    """(included mask, the bar, the oracle's worst included error): FACTOR x the oracle's worst normalised error on the same θ, floor FLOOR;
    θ at which the oracle is off by more than ORC_LIMIT are left out"""
    orc_err = np.asarray(orc_err, dtype=np.float64)
    inc = orc_err <= ORC_LIMIT
    worst = float(orc_err[inc].max()) if inc.any() else 0.0
    return inc, max(FLOOR, FACTOR * worst), worst


# ------------------------------------------------------------------------------------------------ specs
WIDE = (-1e5, 1e5)
POS = (0.0, 1e5)


def _spec(priors, bounds, lik, old=None, fixed=None):
    return dict(priors=list(priors), bounds=list(bounds), fixed=list(fixed) if fixed is not None else [0] * len(priors), lik=lik, old_lik=old)


def _gauss(m, sigma=0.5):
    return ("gauss_iso", [sigma], np.asarray(m, dtype=np.float64).reshape(-1, 1), None)


def sixpriors():
    """d = 6, gauss_iso, one parameter of each prior family"""
    pri = [("normal", 0.5, 2.0), ("uniform", -3.0, 3.0), ("gamma", 2.0, 1.5), ("beta", 2.0, 3.0), ("invgamma", 3.0, 2.0), ("rootinvgamma", 4.0, 0.5)]
    bnd = [WIDE, (-3.0, 3.0), POS, (0.0, 1.0), (1e-8, 1e5), (1e-8, 1e5)]
    return _spec(pri, bnd, _gauss([0.3, -1.0, 2.5, 0.4, 1.2, 0.6]))


def ten():
    """d = 10: the same families, parameter 4 FIXED (its value in prior_a), parameter 1 a Uniform(-1, 1) prior inside bounds (-2, 2)"""
    pri = [("normal", 0.0, 3.0), ("uniform", -1.0, 1.0), ("gamma", 0.6, 2.0), ("beta", 0.5, 0.5), ("normal", 0.75, 1.0), ("invgamma", 3.0, 2.0),
           ("rootinvgamma", 4.0, 0.5), ("beta", 3.0, 1.0), ("normal", -1.0, 0.5), ("gamma", 7.5, 0.25)]
    # (the two priors that are +Inf at an end of their support are bounded away from it: with the Uniform's -Inf the sum would be Inf - Inf)
    bnd = [WIDE, (-2.0, 2.0), (1e-8, 1e5), (1e-6, 1.0 - 1e-6), WIDE, (1e-8, 1e5), (1e-8, 1e5), (0.0, 1.0), WIDE, POS]
    return _spec(pri, bnd, _gauss([0.2, 0.1, 1.0, 0.5, 0.75, 1.1, 0.5, 0.7, -1.0, 1.8]), fixed=[0, 0, 0, 0, 1, 0, 0, 0, 0, 0])


def wide12():
    """d = 12, mixed priors: beyond the register kernels (d <= 10), the generic mutation body"""
    pri = [("normal", 0.0, 2.0), ("gamma", 2.0, 1.0), ("uniform", 0.0, 4.0), ("beta", 2.0, 2.0), ("normal", 1.0, 1.0), ("invgamma", 3.0, 2.0),
           ("rootinvgamma", 4.0, 0.5), ("normal", -2.0, 3.0), ("gamma", 0.6, 2.0), ("beta", 0.5, 3.0), ("uniform", -1.0, 1.0), ("normal", 0.0, 1.0)]
    bnd = [WIDE, POS, (0.0, 4.0), (0.0, 1.0), WIDE, (1e-8, 1e5), (1e-8, 1e5), WIDE, (1e-8, 1e5), (1e-6, 1.0), (-1.0, 1.0), WIDE]
    return _spec(pri, bnd, _gauss([0.1, 1.5, 2.0, 0.5, 1.0, 1.0, 0.5, -2.0, 1.0, 0.2, 0.0, 0.3]))


def reg_data(n, scale=1.0):
    """[y X], n x 2: the committed example data (100 rows), beyond it seeded rows from the same line"""
    base = models.regression_spec()["lik"][2]
    if n > len(base):
        rng = np.random.default_rng(_seed("reg", n))
        X = rng.normal(0.0, 1.0, n - len(base))
        base = np.vstack([base, np.column_stack([1.0 + 2.0 * X + rng.normal(0.0, 1.0, len(X)), X])])
    return np.asfortranarray(base[:n] * scale)


def linreg(n=100, s2=1.0, scale=1.0, old_n=None):
    old = None if old_n is None else ("linreg", [s2], reg_data(old_n, scale), None)
    return _spec([("normal", 0.0, 10.0)] * 2, [WIDE] * 2, ("linreg", [s2], reg_data(n, scale), None), old)


def lm_data(T, xcols=None, scale=1.0):
    """(data 3 x T, X 3 x xcols): the committed test model's (100 periods), beyond it seeded columns"""
    sp = models.linmodel_spec()
    Y, X = np.asarray(sp["lik"][2]), np.asarray(sp["lik"][3])
    xcols = T if xcols is None else xcols
    if max(T, xcols) > Y.shape[1]:
        rng = np.random.default_rng(_seed("lm", T, xcols))
        extra = max(T, xcols) - Y.shape[1]
        X2 = rng.normal(0.0, 1.0, (3, extra))
        Y = np.hstack([Y, 1.0 + 2.0 * X2 + rng.normal(0.0, 1.0, (3, extra))])
        X = np.hstack([X, X2])
    return np.asfortranarray(Y[:, :T] * scale), np.asfortranarray(X[:, :xcols] * scale)


def _nine(sig_lo=1e-5):
    """the nine parameters of the test model and of the CAPM example, the σ's Uniform prior widened to the bounds (the far class puts σ on both)"""
    pri, bnd = [], []
    for _ in range(3):
        pri += [("normal", 0.0, 1e3), ("normal", 0.0, 1e3), ("uniform", 0.0, 1e5)]
        bnd += [WIDE, WIDE, (sig_lo, 1e5)]
    return pri, bnd


def linmodel3(T=100, xcols=None, scale=1.0, old_T=None, old_xcols=None, sig_lo=1e-5):
    pri, bnd = _nine(sig_lo)
    old = None if old_T is None else ("linmodel3", [],) + lm_data(old_T, old_xcols, scale)
    return _spec(pri, bnd, ("linmodel3", [],) + lm_data(T, xcols, scale), old)


def capm(T=36, aux_rows=1, scale=1.0):
    """capm_literal: the committed example data (36 periods), beyond it seeded columns; aux_rows = 2: a second row under the market's, so that
    the stride of the market block matters"""
    sp = models.capm_spec()
    Y, mk = np.asarray(sp["lik"][2]), np.asarray(sp["lik"][3])
    if T > Y.shape[1]:
        rng = np.random.default_rng(_seed("capm", T))
        m2 = rng.normal(0.01, 0.04, (1, T - Y.shape[1]))
        Y, mk = np.hstack([Y, 0.01 * (1.0 + m2) + rng.normal(0.0, 0.05, (3, m2.shape[1]))]), np.hstack([mk, m2])
    Y, mk = Y[:, :T] * scale, mk[:, :T] * scale
    if aux_rows == 2:
        mk = np.vstack([mk, 7.0 + np.arange(T)[None, :]])
    pri, bnd = _nine()
    return _spec(pri, bnd, ("capm_literal", [], np.asfortranarray(Y), np.asfortranarray(mk)))


def lik_doubles(lik):
    """(data doubles, aux doubles) a likelihood hands to stage_lik"""
    if lik is None:
        return 0, 0
    return int(np.asarray(lik[2]).size), 0 if lik[3] is None else int(np.asarray(lik[3]).size)


def staged(spec):
    """(first vintage staged in LDS, second vintage staged): stage_lik keeps a vintage's data and regressors in LDS while used + nd + na <=
    LIK_LDS_CAP, the new vintage first; None for a second vintage that is not there"""
    nd, na = lik_doubles(spec["lik"])
    if spec["lik"][0] == "capm_literal":                     # never staged: the family reads its data as scalars from global memory
        return False, None
    first = nd + na <= LIK_LDS_CAP
    used = nd + na if first else 0
    if spec.get("old_lik") is None:
        return first, None
    od, oa = lik_doubles(spec["old_lik"])
    return first, used + od + oa <= LIK_LDS_CAP


LINREG_N = (1, 2, 3, 5, 100, 384, 385)        # 2 n = 768 is the last size that is staged
LINREG_S2 = (1e-8, 1.0, 1e8)
NINE_T = (1, 2, 3, 5, 100, 128, 129)


def base_specs():
    """label -> spec: every single-vintage spec the scoring vehicle runs"""
    out = collections.OrderedDict(sixpriors=sixpriors(), ten=ten(), wide12=wide12())
    for n in LINREG_N:
        for s2 in LINREG_S2:
            out["linreg n=%d s2=%g" % (n, s2)] = linreg(n, s2)
    for T in NINE_T:
        out["linmodel3 T=%d" % T] = linmodel3(T)
        out["capm T=%d" % T] = capm(T)
    out["linmodel3 T=40 X 3x100"] = linmodel3(40, 100)
    out["capm T=36 aux_rows=2"] = capm(36, 2)
    return out


def two_vintage_specs():
    """label -> (spec, (first staged, second staged)): both sides of the LDS boundary for both vintages"""
    out = collections.OrderedDict()
    out["linmodel3 64+64 X 3x64 (cap filled exactly)"] = linmodel3(64, 64, old_T=64, old_xcols=64)
    out["linmodel3 64+64 X 3x65 (one double over)"] = linmodel3(64, 64, old_T=64, old_xcols=65)
    out["linmodel3 100+40 (first staged, second not)"] = linmodel3(100, 100, old_T=40, old_xcols=100)
    out["linmodel3 129+129 (neither staged)"] = linmodel3(129, 129, old_T=129, old_xcols=129)
    out["linmodel3 100, old 1 period"] = linmodel3(100, 100, old_T=1, old_xcols=1)
    out["linmodel3 64, old T periods"] = linmodel3(64, 64, old_T=64, old_xcols=64)
    out["linreg 192+192 (cap filled exactly)"] = linreg(192, old_n=192)
    out["linreg 192+193 (one row over)"] = linreg(192, old_n=193)
    out["linreg 384+100 (first staged, second not)"] = linreg(384, old_n=100)
    out["linreg 385+385 (neither staged)"] = linreg(385, old_n=385)
    out["linreg 100, old 1 row"] = linreg(100, old_n=1)
    out["linreg 100, old n rows"] = linreg(100, old_n=100)
    return collections.OrderedDict((k, (v, staged(v))) for k, v in out.items())


# ------------------------------------------------------------------------------------------------ the clouds
Case = collections.namedtuple("Case", "label spec theta lp_finite ll_finite")
# lp_finite / ll_finite: what the class says of the reference per θ - True: finite, False: not finite (±Inf), None: not stated


def _draw_prior(rng, fam, a, b, n):
    if fam == "normal":
        return a + b * rng.standard_normal(n)
    if fam == "uniform":
        return a + (b - a) * rng.random(n)
    if fam == "gamma":
        return rng.gamma(a, b, n)
    if fam == "beta":
        return rng.beta(a, b, n)
    if fam == "invgamma":
        return b / rng.gamma(a, 1.0, n)
    if fam == "rootinvgamma":
        return np.sqrt(a * b * b / rng.chisquare(a, n))
    raise KeyError(fam)


def prior_draws(spec, n, seed):
    """n draws of the spec's priors strictly inside the bounds (fixed parameters at their value)"""
    rng = np.random.default_rng(seed)
    d = len(spec["priors"])
    th = np.empty((n, d))
    for k, ((fam, a, b), (lo, hi)) in enumerate(zip(spec["priors"], spec["bounds"])):
        if spec["fixed"][k]:
            th[:, k] = a
            continue
        x = _draw_prior(rng, fam, a, b, n)
        for _ in range(1000):
            bad = ~((lo < x) & (x < hi))
            if not bad.any():
                break
            x[bad] = _draw_prior(rng, fam, a, b, int(bad.sum()))
        th[:, k] = x
    return th


def _all(n, v):
    return np.full(n, v, dtype=object)


def _cases_prior_like(n):
    return [Case(lab, sp, prior_draws(sp, n, _seed("prior", lab)), _all(n, True), _all(n, True)) for lab, sp in base_specs().items()]


def _cases_corners(n):
    """row 2j: every parameter at a bound (inside: the likelihood is finite); row 2j + 1: the same row with one parameter one nextafter
    beyond its bound (-Inf in all three columns)"""
    out = []
    for lab, sp in (("sixpriors", sixpriors()), ("ten", ten()), ("wide12", wide12()), ("linreg n=5 s2=1", linreg(5)), ("linmodel3 T=5", linmodel3(5)), ("capm T=5", capm(5))):
        rng = np.random.default_rng(_seed("corners", lab))
        d = len(sp["priors"])
        lo, hi = np.array([b[0] for b in sp["bounds"]]), np.array([b[1] for b in sp["bounds"]])
        th = np.empty((n, d))
        fin = np.empty(n, dtype=object)
        for i in range(0, n, 2):
            side = rng.random(d) < 0.5 if i >= 4 else np.full(d, i == 0)
            th[i] = np.where(side, lo, hi)
            for k in range(d):
                if sp["fixed"][k]:
                    th[i, k] = sp["priors"][k][1]
            fin[i] = True
            if i + 1 < n:
                th[i + 1] = th[i]
                k = (i // 2) % d
                th[i + 1, k] = np.nextafter(lo[k], -np.inf) if th[i, k] == lo[k] else np.nextafter(hi[k], np.inf)     # (a fixed parameter: beyond hi)
                fin[i + 1] = False
        out.append(Case(lab, sp, th, np.where(fin == False, False, None), fin))   # noqa: E712
    return out


def _cases_far(n, inset=False):
    """location parameters at ±1e5 (the bound), the scales σ of linmodel3 / capm_literal at 1e-5 and 1e5; inset (the mutation vehicle, whose
    proposals must be able to stay inside the bounds): the locations up to a thousandth inside ±1e5, the scales up to a factor 2 inside theirs"""
    out = []
    for lab, sp in (("sixpriors", sixpriors()), ("ten", ten()), ("wide12", wide12()), ("linreg n=100 s2=1", linreg(100)), ("linreg n=385 s2=1e-08", linreg(385, 1e-8)),
                    ("linmodel3 T=100", linmodel3(100)), ("linmodel3 T=129", linmodel3(129)), ("capm T=36", capm(36)), ("capm T=129", capm(129))):
        rng = np.random.default_rng(_seed("far", lab))
        th = prior_draws(sp, n, _seed("farbase", lab))
        nine = sp["lik"][0] in ("linmodel3", "capm_literal")
        for i in range(n):
            for k, (fam, a, b) in enumerate(sp["priors"]):
                if sp["fixed"][k]:
                    continue
                if nine and k % 3 == 2:
                    th[i, k] = (1e-5, 1e5)[(i + k // 3 + (i >> 2)) % 2]
                    if inset:
                        th[i, k] *= (1.0 + rng.random()) ** (1 if th[i, k] < 1 else -1)
                elif fam == "normal" and (nine or sp["lik"][0] == "linreg" or rng.random() < 0.7):
                    th[i, k] = (1e5, -1e5)[(i + k) % 2] if i % 3 else (1e5, -1e5)[i // 3 % 2]
                    if inset:
                        th[i, k] *= 1.0 - 1e-3 * rng.random()
        out.append(Case(lab, sp, th, _all(n, True), _all(n, True)))
    return out


def _ols(y, X):
    A = np.column_stack([np.ones(len(X)), X])
    return np.linalg.lstsq(A, y, rcond=None)[0]


def _cases_cancelling(n):
    """θ at (and a few ulps around) the least-squares solution of data that lie on a line up to rounding: the residuals are rounding-sized
    relative to y"""
    out = []
    for s2 in LINREG_S2:
        D = reg_data(100).copy()
        D[:, 0] = 1.25 - 0.75 * D[:, 1]
        sp = linreg(100, s2)
        sp["lik"] = ("linreg", [s2], np.asfortranarray(D), None)
        th = np.tile(_ols(D[:, 0], D[:, 1]), (n, 1))
        for i in range(1, n):
            th[i, i % 2] = np.nextafter(th[i, i % 2], np.inf if i % 4 < 2 else -np.inf)
            if i >= 8:
                th[i, (i + 1) % 2] *= 1.0 + (i - 7) * 2.0 ** -50
        out.append(Case("linreg n=100 s2=%g" % s2, sp, th, _all(n, True), _all(n, True)))
    for fam in ("linmodel3", "capm_literal"):
        sp = linmodel3(100) if fam == "linmodel3" else capm(36)
        Y, A = np.array(sp["lik"][2]), np.array(sp["lik"][3])
        coef = np.array([[1.5, -0.5], [-2.0, 0.25], [0.125, 3.0]])
        rng = np.random.default_rng(_seed("cancel", fam))
        th = np.empty((n, 9))
        for i in range(3):
            Y[i] = coef[i, 0] + coef[i, 1] * A[i] if fam == "linmodel3" else coef[i, 0] * (1.0 + A[0])
        for r in range(n):
            for i in range(3):
                a, b = _ols(Y[i], A[i] if fam == "linmodel3" else A[0])
                if fam == "capm_literal":
                    a = coef[i, 0]
                th[r, 3 * i], th[r, 3 * i + 1], th[r, 3 * i + 2] = a * (1.0 + (r % 5) * 2.0 ** -51), b * (1.0 - (r % 3) * 2.0 ** -51), 10.0 ** rng.uniform(-5, 5)
        sp["lik"] = (fam, [], np.asfortranarray(Y), sp["lik"][3])
        out.append(Case(fam, sp, th, _all(n, True), _all(n, True)))
    sp = sixpriors()
    th = np.tile(np.asarray(sp["lik"][2]).ravel(), (n, 1))
    for i in range(1, n):
        th[i, i % 6] = np.nextafter(th[i, i % 6], np.inf if i % 2 else -np.inf)
    out.append(Case("sixpriors", sp, th, _all(n, True), _all(n, True)))
    return out


def _cases_data_scale(n):
    out = []
    for sc in (1e6, 1e-6):
        for lab, sp in (("linreg n=100 s2=1", linreg(100, 1.0, sc)), ("linreg n=385 s2=1e+08", linreg(385, 1e8, sc)), ("linmodel3 T=100", linmodel3(100, scale=sc)),
                        ("linmodel3 T=129", linmodel3(129, scale=sc)), ("capm T=36", capm(36, scale=sc)), ("capm T=129 aux_rows=2", capm(129, 2, scale=sc))):
            th = prior_draws(sp, n, _seed("scale", lab))
            out.append(Case("%s x%g" % (lab, sc), sp, th, _all(n, True), _all(n, True)))
    return out


SHAPES = (1e-3, 0.6, 1.0, 7.5, 200.0)
BETAS = ((0.5, 0.5), (1.0, 1.0), (1.0, 3.0), (3.0, 1.0), (400.0, 400.0))
NUS = (1.0, 4.0, 400.0)


def shapes_spec(j):
    """d = 6: Gamma and InverseGamma of shape SHAPES[j], Beta BETAS[j], RootInverseGamma ν = NUS[j % 3], a Normal and a Uniform; the positive
    parameters are bounded by [1e-160, 1e160]"""
    big = (1e-160, 1e160)
    pri = [("gamma", SHAPES[j], 2.0), ("invgamma", SHAPES[j], 2.0), ("beta",) + BETAS[j], ("rootinvgamma", NUS[j % 3], 0.5), ("normal", 0.0, 2.0), ("uniform", -3.0, 3.0)]
    return _spec(pri, [big, big, (0.0, 1.0), big, WIDE, (-3.0, 3.0)], _gauss([1.0, 1.0, 0.5, 0.5, 0.0, 0.0], 1e3))


def _cases_prior_shapes(n, decades=None):
    """x log-uniform over 1e-150 .. 1e150 where the support allows (Beta: 1e-150 .. 1 - 2^-53, both tails); decades (the mutation vehicle, whose
    proposal is the cloud's own covariance): case j keeps its positive parameters within the one decade above 10^decades[j]"""
    out = []
    for j in range(len(SHAPES)):
        sp = shapes_spec(j)
        rng = np.random.default_rng(_seed("shapes", j))
        th = np.empty((n, 6))
        for k in (0, 1, 3):
            th[:, k] = 10.0 ** rng.uniform(-150, 150, n)
            th[:3, k] = (1e-150, 1e150, 1.0)
            if decades is not None:
                th[:, k] = 10.0 ** (decades[j] + rng.random(n))
        t = 10.0 ** rng.uniform(-150, np.log10(0.5), n)
        th[:, 2] = np.where(rng.random(n) < 0.5, t, 1.0 - np.maximum(t, 2.0 ** -53))
        th[:, 4], th[:, 5] = 2.0 * rng.standard_normal(n), rng.uniform(-3, 3, n)
        # where a term overflows the FP64 range the value is -Inf (InverseGamma: b / x, RootInverseGamma: ν τ² / (2 x²) at small x)
        out.append(Case("shapes %g, Beta%r, nu %g" % (SHAPES[j], BETAS[j], NUS[j % 3]), sp, th, _all(n, None), _all(n, True)))
    return out


# (prior, x, the value: a number, "+inf", "-inf", or None = finite, taken from the reference)
EDGE_TABLE = [
    (("gamma", 1.0, 2.0), 0.0, -math.log(2.0)),
    (("beta", 1.0, 3.0), 0.0, math.log(3.0)),
    (("beta", 3.0, 1.0), 1.0, math.log(3.0)),
    (("rootinvgamma", 4.0, 0.5), 1e-170, "-inf"),
    (("beta", 1.0, 1.0), 0.0, 0.0),
    (("beta", 1.0, 1.0), 1.0, 0.0),
    (("gamma", 0.6, 2.0), 0.0, "+inf"),
    (("gamma", 2.0, 2.0), 0.0, "-inf"),
    (("beta", 2.0, 3.0), 0.0, "-inf"),
    (("beta", 3.0, 2.0), 1.0, "-inf"),
    (("beta", 0.5, 3.0), 0.0, "+inf"),
    (("beta", 3.0, 0.5), 1.0, "+inf"),
    (("rootinvgamma", 4.0, 0.5), 1e-162, "-inf"),
    (("rootinvgamma", 4.0, 0.5), 1e155, None),
]


def edge_spec(prior, sigma=1e3):
    """d = 2: the prior under test on [0, 1e160] ([0, 1] for Beta) and a Normal"""
    return _spec([prior, ("normal", 0.0, 1.0)], [(0.0, 1.0) if prior[0] == "beta" else (0.0, 1e160), WIDE], _gauss([0.5, 0.0], sigma))


def _cases_family_edges(n):
    out = []
    for prior, x, want in EDGE_TABLE:
        rng = np.random.default_rng(_seed("edge", prior, x))
        th = np.column_stack([np.full(n, x), rng.standard_normal(n)])
        fin = not isinstance(want, str)
        # (x = 1e155: x² is beyond the FP64 range in every likelihood family; with σ = 1e-3 the log-likelihood's true value is too: -Inf)
        out.append(Case("%s(%g, %g) at %g" % (prior + (x,)), edge_spec(prior, 1e-3 if x > 1e150 else 1e3), th, _all(n, fin), _all(n, x <= 1e150)))
    sp = linmodel3(5, sig_lo=0.0)
    th = prior_draws(sp, n, _seed("edge", "sigma0"))
    for i in range(n):
        th[i, 3 * (i % 3) + 2] = 0.0
    out.append(Case("linmodel3 T=5, a sigma bound of 0 and sigma = 0", sp, th, _all(n, True), _all(n, False)))
    return out


CLASSES = collections.OrderedDict(prior_like=_cases_prior_like, corners=_cases_corners, far=_cases_far, cancelling=_cases_cancelling,
                                  data_scale=_cases_data_scale, prior_shapes=_cases_prior_shapes, family_edges=_cases_family_edges)


def cases(name, n=N_CLASS, **kw):
    """the cases (label, spec, θ (n x d), what the class says of the reference's finiteness) of a class; seeded: the same every time"""
    return CLASSES[name](n, **kw)


def nan_cases(n=N_CLASS):
    """NaN is outside the bounds (both comparisons of a closed interval are false): rows 4j a prior draw (inside: the control), 4j + 1 the draw
    with a NaN in one free parameter (every free parameter in turn), 4j + 2 with a NaN in the fixed parameter (a spec without one: in its last
    parameter, the others on their bounds), 4j + 3 all NaN.  Outside rows hold -Inf in all three columns."""
    out = []
    for lab, sp in (("sixpriors", sixpriors()), ("ten", ten()), ("wide12", wide12()), ("linreg n=5 s2=1", linreg(5)), ("linmodel3 T=5", linmodel3(5)), ("capm T=5", capm(5))):
        d = len(sp["priors"])
        th = prior_draws(sp, n, _seed("nan", lab))
        free = _free(sp)
        fixed = [k for k in range(d) if sp["fixed"][k]]
        for i in range(n):
            if i % 4 == 1:
                th[i, free[(i // 4) % len(free)]] = np.nan
            elif i % 4 == 2:
                if fixed:
                    th[i, fixed[0]] = np.nan
                else:
                    th[i] = [b[(i // 4 + k) % 2] for k, b in enumerate(sp["bounds"])]
                    th[i, d - 1] = np.nan
            elif i % 4 == 3:
                th[i] = np.nan
        fin = np.array([i % 4 == 0 for i in range(n)], dtype=object)
        out.append(Case(lab, sp, th, fin, fin))
    return out


def det_underflow_case(n=N_CLASS):
    """the reproduced quirk: linmodel3 / capm_literal form det = Π σ_i², which underflows for σ products below 1e-154 and overflows
    above 1e154 - outside the shipped bounds of [1e-5, 1e5]; the reference sums logs and does not.  σ down to 1e-60 and up to 1e60."""
    pri, bnd = _nine()
    bnd = [(-1e5, 1e5), (-1e5, 1e5), (1e-80, 1e80)] * 3
    Y, X = lm_data(5)
    sp = _spec(pri, bnd, ("linmodel3", [], Y, X))
    rng = np.random.default_rng(_seed("det"))
    th = prior_draws(linmodel3(5), n, _seed("detbase"))
    for i in range(n):
        for j in range(3):
            th[i, 3 * j + 2] = 10.0 ** (rng.uniform(-60, -52) if i % 2 == 0 else rng.uniform(52, 60))
    return Case("linmodel3 T=5, sigma 1e-60 .. 1e60", sp, th, _all(n, True), _all(n, True))
