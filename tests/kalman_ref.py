"""A high-precision reference for the linear-Gaussian state-space log-likelihood of config 5 (csrc/model.hpp, the lgss_kalman family), in
plain numpy longdouble (64 mantissa bits on x86-64): no GPU, no oracle, no device filter's statement order.

The model as model.hpp states it: 8 states, 3 observables, 3 shocks, θ = (ρ_0..7, σ_0..2, σ_e, μ);
    x_t = Tm x_{t-1} + R ε_t,  ε ~ N(0, diag σ²),   Tm = diag ρ + κ C
    y_t = μ + Z x_t + u_t,     u ~ N(0, σ_e² I),    x_0 = 0, P_0 = I
    log L = Σ_t -1.5 log 2π - ½ log det F_t - ½ v_t' F_t⁻¹ v_t,   F_t = Z P_{t|t-1} Z' + σ_e² I,  v_t = y_t - μ - Z x_{t|t-1}
Structure (C, R, Z), κ and the data are the caller's.  The inputs are the doubles the device sees - θ, y and the structure are taken as
given, nothing is re-derived - and everything from there on is longdouble, vectorised over the particles.  loglik() also returns the
value after nt_mid steps and the scale S = Σ_t (1.5 log 2π + |½ log det F_t| + ½ v' F⁻¹ v): every error of a filter is taken as
|Δll| / max(1, S), the "normalised error" (nerr).  tests/test_kalman_ref_cpu.py pins loglik() against mpmath at 40 digits.

Also here: the seeded generators of the test classes (tests/test_gpu_kalman_range.py, tests/test_kalman_ref_cpu.py).  A class fixes a
region of the parameter space ("boxes": parameter index -> interval, everything else a prior draw of models.kalman_spec) and a list of
variants (number of periods, data, structure, κ)."""
import collections
import zlib

import numpy as np

from tests import models

LD = np.longdouble
LOG2PI = np.log(LD(2.0) * LD("3.14159265358979323846264338327950288"))

Result = collections.namedtuple("Result", "ll ll_mid S S_mid")


def pack_aux(C, R, Z):
    """[C 8x8 | R 8x3 | Z 3x8] row-major, the `aux` block of the lgss_kalman family"""
    return np.concatenate([np.asarray(C, dtype=np.float64).ravel(), np.asarray(R, dtype=np.float64).ravel(), np.asarray(Z, dtype=np.float64).ravel()]).reshape(1, -1)


def loglik(theta, y, C, R, Z, kappa, nt_mid=0):
    """Result(ll, ll_mid, S, S_mid) as longdouble arrays over the rows of theta (n x 13); y is 3 x T.  ll_mid / S_mid: after the first nt_mid
    periods (-Inf / 0 when nt_mid is not in 1..T).  A pivot of F that is not positive gives -Inf from that period on."""
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64)).astype(LD)
    y = np.asarray(y, dtype=np.float64).astype(LD)
    C, R, Z = (np.asarray(a, dtype=np.float64).astype(LD) for a in (C, R, Z))
    n, T = th.shape[0], y.shape[1]
    assert th.shape[1] == 13 and y.shape[0] == 3 and C.shape == (8, 8) and R.shape == (8, 3) and Z.shape == (3, 8)
    Tm = np.broadcast_to(LD(float(kappa)) * C, (n, 8, 8)).copy()
    Tm[:, np.arange(8), np.arange(8)] += th[:, :8]
    TmT = np.ascontiguousarray(np.swapaxes(Tm, 1, 2))
    Q = np.einsum("im,nm,jm->nij", R, th[:, 8:11] ** 2, R)
    se2, mu = th[:, 11] ** 2, th[:, 12]
    ZT = np.ascontiguousarray(Z.T)
    x = np.zeros((n, 8), dtype=LD)
    P = np.broadcast_to(np.eye(8, dtype=LD), (n, 8, 8)).copy()
    ll, S = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    dead = np.zeros(n, dtype=bool)
    ll_mid, S_mid = np.full(n, -np.inf, dtype=LD), np.zeros(n, dtype=LD)
    half = LD(0.5)
    with np.errstate(all="ignore"):
        for t in range(T):
            x = np.einsum("nij,nj->ni", Tm, x)
            P = Tm @ P @ TmT + Q
            P = half * (P + np.swapaxes(P, 1, 2))
            v = y[None, :, t] - mu[:, None] - x @ ZT
            PZ = P @ ZT                                                   # n x 8 x 3
            F = Z[None] @ PZ
            F = half * (F + np.swapaxes(F, 1, 2))
            F[:, [0, 1, 2], [0, 1, 2]] += se2[:, None]
            dead |= ~(F[:, 0, 0] > 0)
            l00 = np.sqrt(F[:, 0, 0])
            l10, l20 = F[:, 1, 0] / l00, F[:, 2, 0] / l00
            p11 = F[:, 1, 1] - l10 * l10
            dead |= ~(p11 > 0)
            l11 = np.sqrt(p11)
            l21 = (F[:, 2, 1] - l20 * l10) / l11
            p22 = F[:, 2, 2] - l20 * l20 - l21 * l21
            dead |= ~(p22 > 0)
            l22 = np.sqrt(p22)
            w0 = v[:, 0] / l00
            w1 = (v[:, 1] - l10 * w0) / l11
            w2 = (v[:, 2] - l20 * w0 - l21 * w1) / l22
            hld = np.log(l00) + np.log(l11) + np.log(l22)                 # ½ log det F
            q = half * (w0 * w0 + w1 * w1 + w2 * w2)
            ll = ll - LD(1.5) * LOG2PI - hld - q
            S = S + LD(1.5) * LOG2PI + np.abs(hld) + q
            if t + 1 == nt_mid:
                ll_mid, S_mid = np.where(dead, -np.inf, ll), S.copy()
            g0 = PZ[:, :, 0] / l00[:, None]
            g1 = (PZ[:, :, 1] - l10[:, None] * g0) / l11[:, None]
            g2 = (PZ[:, :, 2] - l20[:, None] * g0 - l21[:, None] * g1) / l22[:, None]
            x = x + g0 * w0[:, None] + g1 * w1[:, None] + g2 * w2[:, None]          # K v = P Z' L⁻ᵀ L⁻¹ v
            P = P - (g0[:, :, None] * g0[:, None, :] + g1[:, :, None] * g1[:, None, :] + g2[:, :, None] * g2[:, None, :])
    ll = np.where(dead, -np.inf, ll)
    return Result(ll, ll_mid, S, S_mid)


def nerr(got, ll, S):
    """the normalised error |got - ll| / max(1, S) per particle (float64; Inf where `got` is not finite)"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = (np.abs(got.astype(LD) - ll) / np.maximum(LD(1.0), S)).astype(np.float64)
    return np.where(np.isfinite(got), e, np.inf)


# ------------------------------------------------------------------------------------------------ the classes
N_CLASS = 24                  # θ per class
ORC_LIMIT = 1e-10             # a θ at which the FP64 oracle is off by more than this (normalised) is left out: conditioning, not a filter's fault
MAX_LEFT_OUT = 3              # of 24 (the same share of a larger cloud)
FLOOR = 1e-12                 # the agreement model.hpp states for its filters
FACTOR = 16.0                 # a different summation order, products of Newton-refined reciprocals in place of sqrt and division

SNR = {8: (1.5, 2.0), 9: (1.5, 2.0), 10: (1.5, 2.0), 11: (1e-3, 2e-3)}
QUIET = {8: (1e-3, 2e-3), 9: (1e-3, 2e-3), 10: (1e-3, 2e-3), 11: (1.0, 2.0)}
ROOTS_POS = {k: (0.9, 0.95) for k in range(8)}
_SIGNS = ((1, -1, 1, 1, -1, 1, -1, -1), (-1, -1, 1, -1, 1, 1, -1, 1), (1, 1, -1, 1, 1, -1, 1, -1), (-1, 1, 1, -1, -1, -1, 1, 1))
ROOTS_MIXED = [{k: ((0.9, 0.95) if s > 0 else (-0.95, -0.9)) for k, s in enumerate(sg)} for sg in _SIGNS]
# μ = ±1e3, ±1e5: a drawn cloud takes μ from the unit interval inside the value (the bound of the model is |μ| <= 1e5), a generated one sits on it
MU_FAR = [{12: (999.0, 1000.0)}, {12: (-1000.0, -999.0)}, {12: (1e5 - 1.0, 1e5)}, {12: (-1e5, -(1e5 - 1.0))}]
_MU_PIN = (1e3, -1e3, 1e5, -1e5)


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def thetas(name, n=N_CLASS):
    """n parameter vectors of class `name` (n x 13 doubles); the first rows do not depend on n.  Prior draws (ρ uniform in ±0.95, σ and σ_e
    uniform in (1e-3, 2), μ normal(0, 5)) with the class's boxes laid over them, row i in box i mod len(boxes)."""
    boxes = BOXES[name]
    u = np.random.default_rng(_seed("theta", name)).random((n, 16))
    th = np.empty((n, 13))
    th[:, :8] = -0.95 + 1.9 * u[:, :8]
    th[:, 8:12] = 1e-3 + (2.0 - 1e-3) * u[:, 8:12]
    th[:, 12] = 5.0 * np.sqrt(-2.0 * np.log1p(-u[:, 12])) * np.cos(2.0 * np.pi * u[:, 13])
    for i in range(n):
        for k, (lo, hi) in boxes[i % len(boxes)].items():
            th[i, k] = lo + (hi - lo) * u[i, k if k < 12 else 14]
        if name == "mu_far":
            th[i, 12] = _MU_PIN[i % 4]
    return th


def box_spec(box, y, aux, kappa, old=None):
    """models.kalman_spec with priors and bounds narrowed onto one box (init_from_prior then draws the class's region); old: the old vintage's
    (y, aux) or None"""
    sp = models.kalman_spec()
    pri, bnd = list(sp["priors"]), list(sp["bounds"])
    for k, (lo, hi) in box.items():
        pri[k] = ("uniform", lo, hi)
        bnd[k] = (max(lo, bnd[k][0]), min(hi, bnd[k][1]))
    return dict(priors=pri, bounds=bnd, fixed=[0] * 13, lik=("lgss_kalman", [kappa], np.ascontiguousarray(y), aux),
                old_lik=None if old is None else ("lgss_kalman", [kappa], np.ascontiguousarray(old[0]), old[1]))


def dense_structure():
    """C, R, Z dense random: |C| <= 0.5 with a diagonal, no zero in R (every one of the 108 packed R[i][m] R[j][m] products counts), every
    row of Z different"""
    rng = np.random.default_rng(_seed("dense"))
    C = rng.uniform(-0.5, 0.5, size=(8, 8))
    R = rng.uniform(0.2, 1.0, size=(8, 3)) * rng.choice([-1.0, 1.0], size=(8, 3))
    Z = rng.uniform(-1.0, 1.0, size=(3, 8))
    return C, R, Z


def diagonal_structure():
    """C = 0, Z rows e_0, e_3, e_6, and states 0, 3, 6 driven by shocks 0, 1, 2: three independent AR(1)-plus-noise filters"""
    R = np.zeros((8, 3))
    for k in range(8):
        R[k, (k + k // 3) % 3] = 1.0 / (1.0 + k // 3)
    Z = np.zeros((3, 8))
    Z[0, 0] = Z[1, 3] = Z[2, 6] = 1.0
    return np.zeros((8, 8)), R, Z


def simulate(C, R, Z, kappa, T, seed):
    """observations from the model at models.KALMAN_TRUTH"""
    th = models.KALMAN_TRUTH
    Tm = np.diag(th[:8]) + kappa * C
    rs = np.random.RandomState(seed)
    x, y = np.zeros(8), np.zeros((3, T))
    for t in range(T):
        x = Tm @ x + R @ (th[8:11] * rs.standard_normal(3))
        y[:, t] = th[12] + Z @ x + th[11] * rs.standard_normal(3)
    return y


Variant = collections.namedtuple("Variant", "label y C R Z kappa")
BOXES = dict(prior=[{}], snr=[SNR], quiet=[QUIET], roots_mixed=ROOTS_MIXED, roots_pos=[ROOTS_POS], all_edges=[{**ROOTS_POS, **SNR}], mu_far=MU_FAR,
             short=[{}], data_scale=[{}], dense_structure=[{}], diagonal=[{}])
CLASS_T = dict(prior=(80, 400), snr=(80, 400), quiet=(80,), roots_mixed=(80,), roots_pos=(80, 400), all_edges=(80,), mu_far=(80, 400), short=(1, 2, 3, 41))
CLASSES = tuple(BOXES)
_Y400 = None


def variants(name):
    """the (label, y, C, R, Z, κ) a class is evaluated at"""
    global _Y400
    if _Y400 is None:
        _Y400 = models.kalman_data(400)                     # (its first 80 periods are models.kalman_data(80))
    C, R, Z = models.kalman_structure()
    k = models.KALMAN_KAPPA
    if name in CLASS_T:
        return [Variant("T=%d" % T, np.ascontiguousarray(_Y400[:, :T]), C, R, Z, k) for T in CLASS_T[name]]
    y = np.ascontiguousarray(_Y400[:, :80])
    if name == "data_scale":
        return [Variant("y*1e6", y * 1e6, C, R, Z, k), Variant("y*1e-6", y * 1e-6, C, R, Z, k)]
    if name == "dense_structure":
        Cd, Rd, Zd = dense_structure()
        return [Variant("kappa=%g" % kk, simulate(Cd, Rd, Zd, kk, 80, 7), Cd, Rd, Zd, kk) for kk in (0.2, -0.3)]
    if name == "diagonal":
        Cd, Rd, Zd = diagonal_structure()
        return [Variant("T=80", simulate(Cd, Rd, Zd, k, 80, 8), Cd, Rd, Zd, k)]
    raise KeyError(name)


def oracle_loglik(v, theta, T=None):
    """the FP64 oracle's log-likelihoods (oracle/smc_oracle.c orc_kalman_lgss) of the rows of theta on variant v (its first T periods)"""
    from oracle import oracle as orc

    y = v.y if T is None else np.ascontiguousarray(v.y[:, :T])
    lik = orc.Lik("lgss_kalman", [v.kappa], y, pack_aux(v.C, v.R, v.Z))
    return np.array([orc.loglik(lik, np.ascontiguousarray(th)) for th in np.atleast_2d(theta)])


def bar(orc_err):
    """(included mask, the bar of the value check) from the oracle's normalised errors on a class: FACTOR x the worst included one, floor FLOOR"""
    orc_err = np.asarray(orc_err, dtype=np.float64)
    inc = orc_err <= ORC_LIMIT
    worst = float(orc_err[inc].max()) if inc.any() else 0.0
    return inc, max(FLOOR, FACTOR * worst), worst
