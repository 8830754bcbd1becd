"""A high-precision reference for ONE correction step (src/smc_main.jl:401-435) and for the adaptive ϕ root (src/helpers.jl:9-56),
in plain numpy + math.fsum: no GPU, no oracle.

The reference package forms exp(a_i) unshifted and is NaN once every |a_i| passes ~745; the engines shift by an energy they have
at hand.  This helper shifts by the EXACT maximum of the per-particle log-weight log W_i + a_i, forms every difference in extended
precision (numpy longdouble: 64 mantissa bits on x86-64) and sums with math.fsum, so that its ESS, normalised weights and log-MDD
increment do not depend on a common offset of the log-likelihoods.  tests/test_weights_ref_cpu.py pins it against the oracle where
the oracle is finite and against 60-digit `decimal` arithmetic out to offsets of 2e7.

The three exponents, with δ = ϕ_n - ϕ_{n-1} (as oracle/smc_oracle.c orc_correct states them):
    prior_weight == 0:   a_i = δ (loglh_i - old_loglh_i)
    prior_weight == 1:   a_i = δ loglh_i
    otherwise:           a_i = δ (loglh_i - log(exp(old_loglh_i - log_prob_old_data + log(1 - pw)) + pw))
Particles with W_i == 0 or a_i == -Inf carry weight 0."""
import math

import numpy as np

LD = np.longdouble


def generalised_energy(loglh, old_loglh, prior_weight=0.0, log_prob_old_data=0.0):
    """(loglh, h) in extended precision with a_i = δ g_i, g_i = loglh_i - h_i.  The two parts stay apart: with a large common offset in
    loglh, loglh_i - h_i would be rounded at the offset's size, while (loglh_i - loglh_m) - (h_i - h_m) is not."""
    ll = np.asarray(loglh, dtype=np.float64).astype(LD)
    old = np.zeros_like(ll) if old_loglh is None else np.asarray(old_loglh, dtype=np.float64).astype(LD)
    if prior_weight == 0.0:
        return ll, old
    if prior_weight == 1.0:
        return ll, np.zeros_like(ll)
    pw = LD(prior_weight)
    with np.errstate(over="ignore"):
        h = np.log(np.exp(old - LD(log_prob_old_data) + np.log(LD(1.0) - pw)) + pw)
    return ll, h


def _shifted(g, W, delta):
    """(W̃ as longdouble with max 1, the log of the common factor left out, the live mask)"""
    ll, h = g
    W = np.asarray(W, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        logW = np.log(W.astype(LD))
        L = logW + LD(delta) * (ll - h)                           # -Inf where W == 0 or g == -Inf; only the argmax is taken from it
    live = (W > 0) & np.isfinite(L)
    if not live.any():
        raise ValueError("no particle with a positive weight and a finite exponent")
    m = int(np.argmax(np.where(live, L, -np.inf)))
    # differences first, the product with δ after: a common offset of the energies cancels before anything is rounded to its size
    with np.errstate(invalid="ignore"):
        t = (logW - logW[m]) + LD(delta) * ((ll - ll[m]) - (h - h[m]))
    t = np.where(live, t, -np.inf)
    m2 = int(np.argmax(t))                                        # the exact maximum: L's own rounding may have picked a neighbour
    if m2 != m:
        m = m2
        with np.errstate(invalid="ignore"):
            t = np.where(live, (logW - logW[m]) + LD(delta) * ((ll - ll[m]) - (h - h[m])), -np.inf)
    with np.errstate(under="ignore"):
        wt = np.exp(t)
    return wt, logW[m] + LD(delta) * (ll[m] - h[m]), live


def _sums(wt):
    with np.errstate(under="ignore"):
        x = np.asarray(wt, dtype=np.float64)                       # max 1: the cast rounds at 2^-53, squares below 1e-308 are < 1e-308 / N of s2
    s1 = math.fsum(x.tolist())
    s2 = math.fsum((x * x).tolist())
    return s1, s2


def ess_ref(loglh, old_loglh, W, phi_n, phi_prev, prior_weight=0.0, log_prob_old_data=0.0):
    g = generalised_energy(loglh, old_loglh, prior_weight, log_prob_old_data)
    wt, _, _ = _shifted(g, W, float(phi_n) - float(phi_prev))
    s1, s2 = _sums(wt)
    return s1 * s1 / s2


def correct_ref(loglh, old_loglh, W, phi_n, phi_prev, prior_weight=0.0, log_prob_old_data=0.0, threshold_ratio=0.5):
    """One correction.  Returns dict(ess, W (normalised weights, mean 1), logz_inc (log Σ W_i exp(a_i) / N: the log-MDD increment for
    weights of mean 1), resample (ESS < threshold_ratio N), w (the unshifted incremental weights exp(a_i) in FP64: 0 where they
    underflow, inf where they overflow), log_shift (the common factor's log))."""
    n = len(loglh)
    delta = float(phi_n) - float(phi_prev)
    g = generalised_energy(loglh, old_loglh, prior_weight, log_prob_old_data)
    wt, log_shift, _ = _shifted(g, W, delta)
    s1, s2 = _sums(wt)
    ess = s1 * s1 / s2
    with np.errstate(under="ignore", over="ignore"):
        Wn = np.asarray(wt * (LD(n) / LD(s1)), dtype=np.float64)
        w = np.asarray(np.exp(LD(delta) * (g[0] - g[1])), dtype=np.float64)
    logz = float(log_shift + np.log(LD(s1) / LD(n)))
    return dict(ess=ess, W=Wn, logz_inc=logz, resample=bool(ess < threshold_ratio * n), w=w, log_shift=float(log_shift), s1=s1, s2=s2)


def solve_phi_ref(loglh, old_loglh, W, sched, j, phi_prop, phi_prev, target, ess_prev, resampled_last):
    """solve_adaptive_ϕ (src/helpers.jl:9-56) on ess_ref: the walk over the proposed schedule, then bisection to adjacent floats
    (Roots.fzero with xtol = 0).  j is the reference's 1-based index.  Returns (ϕ_n, resampled_last, j, ϕ_prop)."""
    n = len(loglh)
    sched = np.asarray(sched, dtype=np.float64)
    g = generalised_energy(loglh, old_loglh)

    def G(phi):
        wt, _, _ = _shifted(g, W, float(phi) - float(phi_prev))
        s1, s2 = _sums(wt)
        return s1 * s1 / s2 - ess_bar

    ess_bar = target * (float(n) if resampled_last else float(ess_prev))
    while G(phi_prop) >= 0.0 and j <= sched.size:
        phi_prop = float(sched[j - 1])
        j += 1
    if phi_prop != 1.0 or G(phi_prop) < 0.0:
        a, b = float(phi_prev), float(phi_prop)
        fa, fb = G(a), G(b)
        if fa == 0.0:
            root = a
        elif fb == 0.0:
            root = b
        else:
            assert (fa > 0) != (fb > 0), ("the bracket does not change sign", a, b, fa, fb)
            while True:
                mid = a + (b - a) / 2
                if mid <= a or mid >= b:
                    break
                fm = G(mid)
                if fm == 0.0:
                    a = b = mid
                    fa = fb = 0.0
                    break
                if (fm > 0) != (fa > 0):
                    b, fb = mid, fm
                else:
                    a, fa = mid, fm
            root = a if abs(fa) <= abs(fb) else b
        return root, False, j, phi_prop
    return 1.0, False, j, phi_prop


# ------------------------------------------------------------------------------------------------ test clouds with two knobs
# δB as the issue lists them; the lagged shift sees the same magnitudes with the other sign (the overflow side)
OFFSETS = (0.0, 300.0, 350.0, 360.0, 365.0, 368.0, 370.0, 372.0, 373.0, 380.0, 500.0, 700.0, 740.0, 800.0, 1e4, 1e6)
OFFSETS_REDUCED = (0.0, 360.0, 370.0, 373.0, 700.0, 800.0, 1e6)


def knob_cloud(n, delta, dB, dS, seed, weights="ones"):
    """e_i = -B - S u_i with δ B = dB, δ S = dS, u seeded uniform on [0, 1); W all 1 or seeded in (0, 2) with mean 1.
    Returns (loglh, W).  δ S sets the ESS (2: ≈ 0.76 N, 5: ≈ 0.39 N); δ B changes nothing but the log-MDD increment."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    loglh = -(dB / delta) - (dS / delta) * u
    if weights == "ones":
        W = np.ones(n)
    else:
        W = 2.0 * rng.random(n) + 1e-12
        W *= n / W.sum()
    return loglh, W


def chain_ref(loglh, old_loglh, W, sched, target, threshold_ratio=0.0, phis=None, max_stages=400):
    """The whole adaptive run of a FROZEN cloud (src/smc_main.jl:377-508 with every proposal rejected: the energies never change), as a chain
    of solve_phi_ref + correct_ref until ϕ = 1, carrying j, ϕ_prop, ESS_prev and W as the reference loop does (start: j = 2, ϕ_prop = ϕ = 0,
    ESS_prev = N, not resampled).  phis = None: ϕ_k is the reference's root.  phis given (a run's recorded ones, ϕ_2 first): every stage is
    evaluated AT those values - a tolerance on ϕ then does not leak into the tolerances on the sums.  A frozen chain cannot resample (the
    cloud would change): a stage whose ESS falls below threshold_ratio N raises ValueError; with threshold_ratio = 0 none does.
    Returns one dict per stage: phi, ess, logz_inc, W (normalised, mean 1), w (incremental weights), resample (False), j_in / j (the schedule
    index before / after the stage's walk, 1-based as the reference's), phi_prop."""
    n = len(loglh)
    Wc = np.asarray(W, dtype=np.float64).copy()
    j, phi_prop, phi, ess_prev, rl = 2, 0.0, 0.0, float(n), False
    out = []
    while phi < 1.0:
        if len(out) >= max_stages:
            raise ValueError("the chain does not reach 1 within %d stages" % max_stages)
        j_in = j
        if phis is None:
            phi_n, rl, j, phi_prop = solve_phi_ref(loglh, old_loglh, Wc, sched, j, phi_prop, phi, target, ess_prev, rl)
        else:
            phi_n = float(phis[len(out)])
        r = correct_ref(loglh, old_loglh, Wc, phi_n, phi, 0.0, 0.0, threshold_ratio)
        if r["resample"]:
            raise ValueError("stage %d of a frozen chain would resample (ESS %r)" % (len(out) + 2, r["ess"]))
        out.append(dict(phi=phi_n, ess=r["ess"], logz_inc=r["logz_inc"], W=r["W"], w=r["w"], resample=False, j_in=j_in, j=j, phi_prop=phi_prop))
        Wc, ess_prev, phi = r["W"], r["ess"], phi_n
    return out


def chain_at(loglh, old_loglh, W, phis, threshold_ratio=0.0):
    """chain_ref evaluated at given ϕ values (ϕ_2, ϕ_3, ... ending in 1): no solver"""
    return chain_ref(loglh, old_loglh, W, None, None, threshold_ratio, phis=phis)


def default_zero_rows(n):
    """the first 8 rows, the two rows straddling index 255 / 256 (a wavefront and block boundary), the last 3 and - clouds of 4 096 and more -
    one whole interior 512-chunk"""
    rows = list(range(min(8, n))) + [r for r in (255, 256) if r < n] + list(range(max(n - 3, 0), n))
    if n >= 4096:
        rows += list(range(512 * 3, 512 * 4))
    return np.unique(np.asarray(rows, dtype=np.int64))


def zero_high_cloud(n, delta, dDelta, spread, seed, rows=None):
    """Rows of weight 0 that hold the LARGEST energy of the cloud.  Live rows: e_i = -Δ + spread z_i with δ Δ = dDelta, z seeded standard
    normal, weights normalised to sum n (ESS ≈ n_live exp(-(δ spread)²)).  Rows in `rows` (default_zero_rows): W = 0 and energy 0.  By the
    reference's arithmetic those rows contribute exactly 0 (0 x a finite exp) and the cloud is the live rows alone.  Returns (loglh, W)."""
    rng = np.random.default_rng(seed)
    rows = default_zero_rows(n) if rows is None else np.asarray(rows, dtype=np.int64)
    loglh = -(dDelta / delta) + spread * rng.standard_normal(n)
    W = np.ones(n)
    loglh[rows] = 0.0
    W[rows] = 0.0
    W *= n / W.sum()
    return loglh, W


def outlier_cloud(n, delta, dS, dDelta, seed):
    """knob_cloud at offset 0 with one more thing: particle n // 3 has the largest energy of the live cloud, above everyone else's by
    Δ (δ Δ = dDelta), and a negligible weight W = 1e-200.  By the reference's arithmetic it changes nothing."""
    loglh, W = knob_cloud(n, delta, 0.0, dS, seed)
    k = n // 3
    loglh[k] = dDelta / delta
    W[k] = 1e-200
    return loglh, W
