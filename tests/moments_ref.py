"""A high-precision reference for the weighted mean and covariance every mutation step rests on (src/smc_main.jl:457-469,
src/particle.jl:481-483, 526-529), in plain numpy + math.fsum (+ mpmath for the factor): no GPU, no oracle.

As the reference package defines them: weights normalised by their sum, the mean, then Σ w (x - m)(x - m)' (StatsBase.cov with
corrected = false), then (R + R') / 2.  TWO passes, in numpy longdouble (64 mantissa bits on x86-64), and sums whose result does not
depend on the order of the terms:
  - Σ W and the d sums of the mean are exact: every longdouble term is split into two doubles (exactly), math.fsum adds all of them
    without rounding, and the residual against the rounded total is taken the same way - the total is good to ~2^-100.
  - the d (d + 1) / 2 sums of the covariance run over deviations from the mean, so nothing cancels: they are taken in chunks of
    256 particles in longdouble (each chunk's rounding <= 256 x 2^-64 = 1.4e-17 of its Σ |term|) and the chunk totals are added exactly.
tests/test_moments_ref_cpu.py pins the whole against mpmath at 50 digits.

Also here: the Cholesky factor and log-determinant of a block in mpmath (chol_ref), and the generator of the test clouds (knob_cloud)
with the knobs that matter for a one-pass formulation: the distance of the cloud from the origin in standard deviations (κ), the
spread of the columns' scales, the correlation of one column pair, and the weights."""
import math

import numpy as np

LD = np.longdouble
CHUNK = 256


def _split(x):
    """longdouble array -> (hi, lo) doubles with hi + lo == x exactly (64 mantissa bits fit 53 + 53)"""
    x = np.asarray(x, dtype=LD)
    hi = x.astype(np.float64)
    lo = (x - hi.astype(LD)).astype(np.float64)
    return hi, lo


def exact_sum(x):
    """Σ x over a 1-D longdouble array, whatever the order: the exact sum rounded to a double, plus the exact residual rounded to a double"""
    hi, lo = _split(np.ravel(x))
    terms = hi.tolist() + lo.tolist()
    s = math.fsum(terms)
    r = math.fsum(terms + [-s])
    return LD(s) + LD(r)


def weighted_moments(theta, w):
    """(mean, R) of the n x d array theta under weights w, as longdouble arrays; R is symmetrised."""
    X = np.asarray(theta, dtype=np.float64).astype(LD)
    if X.ndim == 1:
        X = X[:, None]
    n, d = X.shape
    w = np.asarray(w, dtype=np.float64).astype(LD)
    assert w.shape == (n,)
    sw = exact_sum(w)
    wn = w / sw                                                        # normalize: Weights(W / ΣW)
    swn = exact_sum(wn)
    mean = np.array([exact_sum(wn * X[:, a]) for a in range(d)], dtype=LD) / swn
    Xc = X - mean[None, :]
    Y = Xc * wn[:, None]
    iu = np.triu_indices(d)
    chunks = []
    for b in range(0, n, CHUNK):
        chunks.append((Y[b:b + CHUNK].T @ Xc[b:b + CHUNK])[iu])
    chunks = np.array(chunks, dtype=LD)                                # (n / CHUNK) x d (d + 1) / 2
    R = np.zeros((d, d), dtype=LD)
    for p, (a, b) in enumerate(zip(*iu)):
        R[a, b] = R[b, a] = exact_sum(chunks[:, p]) / swn              # corrected = false; an entry and its mirror are one sum: (R + R') / 2 = R
    return mean, R


def mp_moments(theta, w, dps=50):
    """the same in mpmath at `dps` digits (a few hundred particles): (mean list, R as a list of lists) of mpf"""
    import mpmath as mp

    with mp.workdps(dps):
        X = np.asarray(theta, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        n, d = X.shape
        ww = [mp.mpf(float(v)) for v in w]
        sw = mp.fsum(ww)
        wn = [v / sw for v in ww]
        cols = [[mp.mpf(float(v)) for v in X[:, a]] for a in range(d)]
        mean = [mp.fsum(wi * xi for wi, xi in zip(wn, cols[a])) for a in range(d)]
        dev = [[xi - mean[a] for xi in cols[a]] for a in range(d)]
        R = [[mp.fsum(wi * xa * xb for wi, xa, xb in zip(wn, dev[a], dev[b])) for b in range(d)] for a in range(d)]
        R = [[(R[a][b] + R[b][a]) / 2 for b in range(d)] for a in range(d)]
        return mean, R


def chol_ref(S, dps=50):
    """Lower Cholesky factor of the symmetric matrix S (any real dtype; taken as exact) in mpmath at `dps` digits.
    Returns (L as a longdouble array, log det S as a float, smallest pivot / its diagonal entry as a float) or None if a pivot is <= 0."""
    import mpmath as mp

    S = np.asarray(S)
    d = S.shape[0]
    with mp.workdps(dps):
        A = [[mp.mpf(S[a, b].item()) if S.dtype != LD else _mpf_ld(S[a, b]) for b in range(d)] for a in range(d)]
        L = [[mp.mpf(0)] * d for _ in range(d)]
        logdet, worst = mp.mpf(0), mp.inf
        for j in range(d):
            s = A[j][j] - mp.fsum(L[j][k] ** 2 for k in range(j))
            if not s > 0:
                return None
            worst = min(worst, s / A[j][j])
            L[j][j] = mp.sqrt(s)
            logdet += mp.log(s)
            for i in range(j + 1, d):
                L[i][j] = (A[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        out = np.zeros((d, d), dtype=LD)
        for i in range(d):
            for j in range(i + 1):
                out[i, j] = _ld_mpf(L[i][j])
        return out, float(logdet), float(worst)


def _mpf_ld(x):
    """longdouble -> mpf, exactly"""
    import mpmath as mp

    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(LD(x) - LD(hi)))


def _ld_mpf(v):
    """mpf -> longdouble, to 2^-64"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


# ------------------------------------------------------------------------------------------------ test clouds
KAPPAS = (0.0, 1e2, -1e2, 1e4, -1e4, 1e6, -1e6, 1e8, -1e8)
CORRS = (0.0, 0.99, 1.0 - 1e-6)
WEIGHTS = ("ones", "random", "degenerate")


def column_scales(d, scales):
    if scales == "ones" or d == 1:
        return np.ones(d)
    assert scales == "spread"
    return 10.0 ** np.linspace(-6.0, 6.0, d)                          # geometric, 1e-6 .. 1e6


def knob_cloud(n, d, kappa, scales="ones", corr=0.0, weights="ones", seed=0):
    """θ_k = s_k (κ_k + z_k), z standard normal with corr(z_0, z_1) = corr (d >= 2).  kappa: a number (every column) or (number, column)
    (that column alone).  scales: "ones" or "spread" (1e-6 .. 1e6 over the columns).  weights: "ones", "random" (uniform, mean 1) or
    "degenerate" (99 % exact zeros, one particle carrying half of the mass).  Returns (theta n x d, W of mean 1), doubles."""
    rng = np.random.default_rng([seed, n, d])
    z = rng.standard_normal((n, d))
    if d >= 2 and corr != 0.0:
        z[:, 1] = corr * z[:, 0] + math.sqrt(1.0 - corr * corr) * z[:, 1]
    k = np.zeros(d)
    if isinstance(kappa, (tuple, list)):
        k[kappa[1] % d] = kappa[0]
    else:
        k[:] = kappa
    theta = column_scales(d, scales)[None, :] * (k[None, :] + z)
    if weights == "ones":
        W = np.ones(n)
    elif weights == "random":
        W = 2.0 * rng.random(n) + 1e-12
    else:
        assert weights == "degenerate"
        live = rng.permutation(n)[:max(2, -(-n // 100))]
        W = np.zeros(n)
        W[live] = rng.random(live.size) + 0.5
        W[live[0]] = W[live[1:]].sum()
    W *= n / W.sum()
    return np.asfortranarray(theta), W


def rel_errors(mean, R, ref_mean, ref_R):
    """(largest |mean - ref| in ulps of max(|ref|, σ_ref) per column, largest |R - ref|_ab / sqrt(ref_aa ref_bb), largest asymmetry of R on
    the same scale), as floats; inf where the candidate is not finite"""
    mean, R = np.asarray(mean, dtype=np.float64), np.asarray(R, dtype=np.float64)
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(R))):
        return float("inf"), float("inf"), float("inf")
    sd = np.sqrt(np.diag(ref_R))
    scale = np.maximum(np.abs(ref_mean), sd).astype(np.float64)
    ulp = np.spacing(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_mean = np.abs(mean.astype(LD) - ref_mean) / ulp
        den = np.outer(sd, sd)
        e_cov = np.abs(R.astype(LD) - ref_R) / den
        e_sym = np.abs(R - R.T) / den.astype(np.float64)
    f = lambda x: float(np.max(np.where(np.isnan(x), np.inf, x)))
    return f(e_mean), f(e_cov), f(e_sym)
