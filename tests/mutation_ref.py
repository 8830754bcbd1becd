"""An independent reference for the Metropolis-Hastings move (src/mutation.jl:56-138, src/helpers.jl:87-164, :215-260 and the RNG contract of
DESIGN.md; on the device csrc/philox.hpp, bmmath.hpp, kernels.hpp mh_draw / mix_propose / mix_densities / mh_step / mutate_generic and their
copies in stage2.hpp, stage3.hpp, enskernel.hpp; restated in oracle/smc_oracle.c and host/hostmath.py) and the seeded input classes the tests run
it on.  No device, no oracle, no library: integers for Philox, numpy longdouble for the bulk, mpmath at 50 digits for the Cholesky factor, the
step-size factor and the pins of tests/test_mutation_ref_cpu.py.  The target comes from tests/target_ref.py (bounds rule included).

Exact step by step: each step takes the FP64 numbers the previous step produced and returns that step's exact value.
  uniforms    Philox4x32-10, key = seed, counter = (id lo, id hi, stage, tag), tag = purpose << 28 | t << 8 | q; u = ((x >> 11) + 0.5) 2^-53 with the sum
              rounded to nearest even.  Proposal t of a particle: its decision's uniform is ub of tag (t - 1, 0) - ua of tag (0xFFFFF, 0) for t = 0 -,
              its component's uniform ua of tag (t, 0), the normals of elements e, e + 1 the pair of tag (t, 1 + e / 2); at odd d_b the last
              pair's second normal is dropped.
  normals     r = sqrt(-2 log ua), (r cos 2π ub, r sin 2π ub): the angle reduced exactly (2 ub - q / 2, q = round(4 ub)) before π is applied.
  draw        component 0 if uc < α, 1 if uc < α + (1 - α) / 2 (that FP64 sum), else 2.  L: the exact Cholesky factor of the FP64 matrix
              (c c) Σ_b.  θ' = centre + L z (centre θ_b, or θ̄_b for component 2), θ' = θ_b + sqrt((c c) Σ_ii) z for component 1; its scale
              s_k = |centre_k| + Σ_e |L_ke| |z_e| (component 1: |θ_k| + sd_k |z_k|).
  densities   in log space: the exponents e0 = -(d_b log 2π + log|c²Σ_b| + |L⁻¹(θ_b - θ'_b)|²) / 2 (weight α, in q0 and q1), e1 = Σ_i -log(sd_i
              sqrt(2π)) - ((θ_i - θ'_i) / sd_i)² / 2 with sd_i = sqrt(Σ_ii) UNSCALED (quirk Q1; weight (1 - α) / 2, in both), e2 = the first with
              θ_b - θ̄_b (q0) or θ'_b - θ̄_b (q1) (weight (1 - α) / 2).  The reference's FP64 rules: a component whose exponent is below the
              underflow point of exp is 0, above the overflow point +Inf - and NaN with a weight of 0; the diagonal component is a running
              product in the reference (ind / (sd_i sqrt(2π)) * exp(-z_i² / 2) coordinate by coordinate), so the rules hold at each of its
              quotients and products (running_product); both densities 0: log 0 - log 0 = NaN (reject); both +Inf: q0 = 0 (the reference's
              quirk), so q0 - q1 = -Inf.
  decision    log η = ϕ (loglh' - loglh) + (1 - ϕ) (old' - old) + (logprior' - logprior) + (log q0 - log q1), IEEE rules for ±Inf and NaN; accept
              iff log u < log η.  S_η: ϕ (S(loglh') + |loglh|) + (1 - ϕ) (S(old') + |old|) + S(logprior') + |logprior| + |log q0| + |log q1|.
  column      Σ accepted d_b / n_free (quirk Q2), exact; the acceptance rate the exact mean; the step-size factor 0.95 + 0.10 e^x / (1 + e^x),
              x = 16 (a - t), from mpmath.
A proposal is `band` when a component that carries more than 2^-53 of its sum (or has weight 0 and sits at the overflow point) has its exponent
within 1e-9 relative of one of the two thresholds or - at α < 1; at α = 1 q0 and q1 are one number whatever its precision - inside the subnormal
range of exp; `undecided` when |log u - log η| <= tol max(1, S_η).  A
particle is dropped from the later proposals of the same call once one of its decisions is undecided or in a band."""
import collections
import math
import zlib

import mpmath as mp
import numpy as np

from tests import target_ref as tr

LD = np.longdouble
dps50 = tr.dps50
MASK32 = 0xFFFFFFFF
P_MUT, P_RES, P_BLK, P_INIT = 0, 1, 2, 3
T_FIRST = 0xFFFFF                       # the t of the tag whose ua decides proposal 0
EXP_UNDER = -745.1332191019412          # exp(x) rounds to 0 below log(2^-1075)
EXP_SUBN = -708.3964185322641           # exp(x) is subnormal below log(2^-1022)
EXP_OVER = 709.782712893384             # exp(x) is +Inf above log(DBL_MAX (1 + 2^-54))
BAND_REL = 1e-9
FLOOR_THETA, FLOOR_LOG, FLOOR_DECIDE, FACTOR = 1e-13, 1e-13, 1e-12, 16.0
CAP = 1e-3                              # undecided + band + dropped decisions of a case
ACCEPT, REJECT, NAN_REJECT, UNDECIDED, BAND, DROPPED = 0, 1, 2, 3, 4, 5
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
# the three known-answer vectors Random123 publishes for philox4x32-10 (counter, key, output)


def _seed(*what):
    return zlib.crc32(repr(what).encode())


# ------------------------------------------------------------------------------------------------ Philox
def rng_tag(purpose, t, q):
    return ((purpose << 28) | ((t & 0xFFFFF) << 8) | (q & 0xFF)) & MASK32


def philox_int(ctr, key):
    """Philox4x32-10 on Python integers: (c0, c1, c2, c3), (k0, k1) -> four words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def u53_int(hi, lo):
    """((x >> 11) + 0.5) 2^-53 for x = hi : lo, the sum rounded to nearest even: the odd integer 2 (x >> 11) + 1 converted (correctly rounded) and scaled"""
    return float(2 * (((hi << 32) | lo) >> 11) + 1) * 2.0 ** -54


def philox(c0, c1, c2, c3, k0, k1):
    """the same on numpy uint64 arrays that hold 32-bit words (broadcast)"""
    U = np.uint64
    c0, c1, c2, c3 = (np.asarray(c, dtype=U) for c in np.broadcast_arrays(np.asarray(c0, dtype=U), np.asarray(c1, dtype=U), np.asarray(c2, dtype=U), np.asarray(c3, dtype=U)))
    m, s32 = U(MASK32), U(32)
    for _ in range(10):
        p0, p1 = U(0xD2511F53) * c0, U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ U(k0), p1 & m, (p0 >> s32) ^ c3 ^ U(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def u53(hi, lo):
    x = ((hi << np.uint64(32)) | lo) >> np.uint64(11)
    return (x.astype(np.float64) + 0.5) * 2.0 ** -53         # x < 2^53 converts exactly; the FP64 sum rounds to nearest even


def uniform_pair(seed, pid, stage, tag):
    """(ua, ub) of the ids pid (any integers below 2^64; array or scalar)"""
    pid = np.asarray(pid, dtype=np.uint64)
    o = philox(pid & np.uint64(MASK32), pid >> np.uint64(32), stage & MASK32, tag, seed & MASK32, (seed >> 32) & MASK32)
    return u53(o[0], o[1]), u53(o[2], o[3])


Stream = collections.namedtuple("Stream", "u_dec uc ua ub")


def stream(seed, pid, stage, t, db):
    """the random numbers of proposal t of the particles pid for a block of db elements: the decision's uniform, the component's, the pairs'
    (ua, ub) as n x ceil(db / 2)"""
    if t == 0:
        u_dec, _ = uniform_pair(seed, pid, stage, rng_tag(P_MUT, T_FIRST, 0))
    else:
        _, u_dec = uniform_pair(seed, pid, stage, rng_tag(P_MUT, t - 1, 0))
    uc, _ = uniform_pair(seed, pid, stage, rng_tag(P_MUT, t, 0))
    prs = [uniform_pair(seed, pid, stage, rng_tag(P_MUT, t, 1 + q)) for q in range((db + 1) // 2)]
    return Stream(u_dec, uc, np.stack([p[0] for p in prs], axis=-1), np.stack([p[1] for p in prs], axis=-1))


def generate_blocks(n_free, n_blocks, free_inds, seed, stage):
    """generate_free_blocks / generate_all_blocks: Fisher-Yates from the top, j = min(trunc(ua (i + 1)), i) with the FP64 product, ua of id 0 and
    tag (P_BLK, i, 0); blocks of ceil(n_free / n_blocks), the last one shorter -> (blocks_free, blocks_all, block_ptr), 0-based"""
    bf = list(range(n_free))
    for i in range(n_free - 1, 0, -1):
        o = philox_int((0, 0, stage & MASK32, rng_tag(P_BLK, i, 0)), (seed & MASK32, (seed >> 32) & MASK32))
        j = min(int(u53_int(o[0], o[1]) * float(i + 1)), i)
        bf[i], bf[j] = bf[j], bf[i]
    sub = -(-n_free // n_blocks)
    bp = [b * sub for b in range(n_blocks)] + [n_free]
    bf = np.array(bf, dtype=np.int32)
    return bf, np.asarray(free_inds, dtype=np.int32)[bf], np.array(bp, dtype=np.int32)


def search_ids(seed, stage, tag, n_ids=1 << 26, chunk=1 << 21):
    """the ids below n_ids whose pair of `tag` has the smallest ua, the ua nearest 1, and the ub nearest each quadrant boundary k / 4 (k = 0 .. 4)
    -> {name: (id, ua, ub)}"""
    best = {}

    def keep(name, score, ids, ua, ub):
        k = int(np.argmin(score))
        if name not in best or score[k] < best[name][0]:
            best[name] = (float(score[k]), int(ids[k]), float(ua[k]), float(ub[k]))

    for lo in range(0, n_ids, chunk):
        ids = np.arange(lo, min(lo + chunk, n_ids), dtype=np.uint64)
        ua, ub = uniform_pair(seed, ids, stage, tag)
        keep("ua_min", ua, ids, ua, ub)
        keep("ua_max", 1.0 - ua, ids, ua, ub)
        for k in range(5):
            keep("ub_%d/4" % k, np.abs(ub - 0.25 * k), ids, ua, ub)
    return {k: v[1:] for k, v in best.items()}


# ------------------------------------------------------------------------------------------------ normals
@dps50
def _mp_ld(v):
    return tr._to_ld(v)


_PI = None


def pi_ld():
    global _PI
    if _PI is None:
        with mp.workdps(tr.DPS):
            _PI = _mp_ld(+mp.pi)
    return _PI


def normals_ld(ua, ub):
    """(z0, z1) of the FP64 uniforms, longdouble"""
    ua, ub = np.asarray(ua, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    r = np.sqrt(-2 * np.log(ua.astype(LD)))
    q = np.rint(4.0 * ub)                                    # 4 ub is exact
    t = 2.0 * ub - 0.5 * q                                   # exact: a multiple of 2^-53 within [-1/4, 1/4]
    a = pi_ld() * t.astype(LD)
    c, s = np.cos(a), np.sin(a)
    k = q.astype(np.int64) % 4
    cc = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s)))
    ss = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c)))
    return r * cc, r * ss


@dps50
def normal_pair_mp(ua, ub):
    """one pair, mpmath, written without the reduction"""
    ua, ub = mp.mpf(float(ua)), mp.mpf(float(ub))
    r = mp.sqrt(-2 * mp.log(ua))
    return r * mp.cos(2 * mp.pi * ub), r * mp.sin(2 * mp.pi * ub)


def block_normals(st, db):
    """n x db longdouble normals of a Stream (block order); the second normal of the last pair is dropped at odd db"""
    z0, z1 = normals_ld(st.ua, st.ub)
    z = np.empty(z0.shape[:-1] + (2 * z0.shape[-1],), dtype=LD)
    z[..., 0::2], z[..., 1::2] = z0, z1
    return z[..., :db]


def ulps(got, ref):
    """|got - ref| in units of the spacing of FP64 at ref"""
    ref = np.asarray(ref, dtype=LD)
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / np.spacing(np.abs(tr.f64(ref))).astype(LD)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the factor
@dps50
def chol_mp(A):
    """exact (50 digits) lower Cholesky factor of the FP64 matrix A -> (L as mpf rows, log det A); None if A is not positive definite"""
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        s = mp.mpf(float(A[j][j])) - mp.fsum(L[j][k] ** 2 for k in range(j))
        if not s > 0:
            return None
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, n):
            L[i][j] = (mp.mpf(float(A[i][j])) - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return L, 2 * mp.fsum(mp.log(L[j][j]) for j in range(n))


Factor = collections.namedtuple("Factor", "db idx mu Sig A L logdet sd_draw sd_dens log_ic")
# idx: the block's positions among the free parameters; A = (c c) Σ_b (FP64); L, logdet: longdouble roundings of the exact factor; sd_draw
# sqrt(A_ii), sd_dens sqrt(Σ_ii) (longdouble); log_ic = Σ -log(sd_dens sqrt(2π))


@dps50
def block_factor(mu_free, Sigma_free, idx, c):
    idx = [int(i) for i in idx]
    Sig = np.asarray(Sigma_free, dtype=np.float64)[np.ix_(idx, idx)]
    A = (np.float64(c) * np.float64(c)) * Sig                 # the FP64 product as the contract states it: (c c) Σ
    f = chol_mp(A.tolist())
    if f is None:
        raise ValueError("c²Σ_b is not positive definite")
    L = np.array([[_mp_ld(v) for v in row] for row in f[0]], dtype=LD)
    sdn = np.array([_mp_ld(mp.sqrt(mp.mpf(float(Sig[i, i])))) for i in range(len(idx))], dtype=LD)
    sdd = np.array([_mp_ld(mp.sqrt(mp.mpf(float(A[i, i])))) for i in range(len(idx))], dtype=LD)
    log_ic = _mp_ld(-mp.fsum(mp.log(mp.sqrt(mp.mpf(float(Sig[i, i])))) + mp.log(2 * mp.pi) / 2 for i in range(len(idx))))
    return Factor(len(idx), np.array(idx), np.asarray(mu_free, dtype=np.float64)[idx], Sig, A, L, _mp_ld(f[1]), sdd, sdn, log_ic)


def solve_lower(L, r):
    """L⁻¹ r for the rows of r (n x db longdouble)"""
    v = np.zeros_like(r)
    for e in range(L.shape[0]):
        s = r[:, e].copy()
        for k in range(e):
            s -= L[e, k] * v[:, k]
        v[:, e] = s / L[e, e]
    return v


# ------------------------------------------------------------------------------------------------ draw
def component(uc, alpha):
    a = np.float64(alpha)
    return np.where(uc < a, 0, np.where(uc < a + (1.0 - a) / 2.0, 1, 2))


def draw(F, xb, z, comp):
    """θ'_b (longdouble) and its scale: xb n x db FP64 (block order), z n x db FP64 normals, comp n"""
    xb, zl = np.asarray(xb, dtype=np.float64).astype(LD), np.asarray(z, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        centre = np.where((comp == 2)[:, None], F.mu.astype(LD)[None, :], xb)
        full, sc = centre + zl @ F.L.T, np.abs(centre) + np.abs(zl) @ np.abs(F.L).T
        diag, scd = xb + F.sd_draw[None, :] * zl, np.abs(xb) + F.sd_draw[None, :] * np.abs(zl)
    one = (comp == 1)[:, None]
    return np.where(one, diag, full), np.where(one, scd, sc)


# ------------------------------------------------------------------------------------------------ densities
Dens = collections.namedtuple("Dens", "e0 e1 e2_0 e2_1 logq0 logq1 diff S band")


@dps50
def _log2pi():
    return _mp_ld(mp.log(2 * mp.pi))


def _mix(ws, es, exact=None, extra_band=None):
    """log Σ_j w_j exp(e_j) under the FP64 rules (per row) and the band flag.  exact[j]: the exponent the component's share is taken from where
    e_j already carries a rule's outcome (±Inf, NaN); extra_band[j]: rows in which the component, if it carries, puts the proposal in the band"""
    n = len(es[0])
    inf = LD(np.inf)
    exact = [None] * len(es) if exact is None else exact
    extra_band = [None] * len(es) if extra_band is None else extra_band
    with np.errstate(all="ignore"):
        lw = [np.log(LD(w)) if w > 0 else -inf for w in ws]
        ex = [e if x is None else x for e, x in zip(es, exact)]
        tot = np.full(n, -inf, dtype=LD)                       # the exact log of the sum, no FP64 rule: the components' shares
        for l, e in zip(lw, ex):
            if l > -inf:
                tot = np.logaddexp(tot, np.where(np.isnan(e), -inf, l + e))
        val, nan, pinf, band = np.full(n, -inf, dtype=LD), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for w, l, e, x, xb in zip(ws, lw, es, ex, extra_band):
            over, under = e > EXP_OVER, e < EXP_UNDER
            near = (np.abs(e - EXP_OVER) <= BAND_REL * EXP_OVER) | (np.abs(e - EXP_UNDER) <= BAND_REL * -EXP_UNDER)
            if w > 0:
                nan |= np.isnan(e)
                carries = (l + x) - tot > LD(-53 * math.log(2.0))
                band |= carries & near
                if xb is not None:
                    band |= carries & xb
                if w < 1:                                       # (weight 1: q0 and q1 are the same number whatever its precision)
                    band |= carries & (((e >= EXP_UNDER) & (e < EXP_SUBN)) | ((l + e >= EXP_UNDER) & (l + e < EXP_SUBN)))
                pinf |= over
                val = np.logaddexp(val, np.where(over | under | np.isnan(e), -inf, l + e))
            else:
                nan |= over | np.isnan(x)                       # 0 x Inf; a NaN parameter
                band |= np.abs(e - EXP_OVER) <= BAND_REL * EXP_OVER
                if xb is not None:
                    band |= xb & (e > EXP_SUBN)                 # (weight 0: only its overflow matters)
        val = np.where(pinf, inf, val)
        val = np.where(nan, LD(np.nan), val)
    return val, band


def running_product(F, x, xn):
    """the diagonal component as the reference forms it (helpers.jl:145-149): ind = ind / (sd_i sqrt(2π)) * exp(-z_i² / 2), coordinate by
    coordinate in block order, under the FP64 rules at every quotient and product - an intermediate beyond the overflow point stays +Inf (times
    an exponential that has vanished: NaN), one below the underflow point stays 0 -> (the exponent: a number, ±Inf or NaN; band: an intermediate
    within 1e-9 relative of a threshold, or an intermediate or one of the exponentials inside the subnormal range)"""
    n = x.shape[0]
    inf = LD(np.inf)
    val, zero, pinf, nan, band = np.zeros(n, dtype=LD), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    lossy = np.zeros(n, dtype=bool)                           # digits lost on the way: matters only if the product does not end as 0
    l2p = _log2pi()

    def rules():
        nonlocal zero, pinf, band, lossy
        live = ~(zero | pinf | nan)
        band |= live & ((np.abs(val - EXP_OVER) <= BAND_REL * EXP_OVER) | (np.abs(val - EXP_UNDER) <= BAND_REL * -EXP_UNDER))
        lossy |= live & (val >= EXP_UNDER) & (val < EXP_SUBN)
        pinf |= live & (val > EXP_OVER)
        zero |= live & (val < EXP_UNDER)

    with np.errstate(all="ignore"):
        for i in range(F.db):
            val = val - (np.log(F.sd_dens[i]) + l2p / 2)
            rules()
            q = ((x[:, i] - xn[:, i]) / F.sd_dens[i]) ** 2 / 2
            nan |= np.isnan(q)
            gone = -q < EXP_UNDER
            band |= ~(zero | nan) & (np.abs(-q - EXP_UNDER) <= BAND_REL * -EXP_UNDER)
            lossy |= ~(zero | nan) & (-q >= EXP_UNDER) & (-q < EXP_SUBN)
            nan |= pinf & gone
            zero |= ~pinf & gone
            val = val - q
            rules()
        out = np.where(nan, LD(np.nan), np.where(pinf, inf, np.where(zero, -inf, val)))
    return out, band | (lossy & ~zero & ~nan)


def densities(F, xb, xnb, alpha):
    """the proposal densities of the move xb -> xnb (n x db FP64, block order)"""
    x, xn = np.asarray(xb, dtype=np.float64).astype(LD), np.asarray(xnb, dtype=np.float64).astype(LD)
    mu = F.mu.astype(LD)[None, :]
    with np.errstate(all="ignore"):
        cst = LD(F.db) * _log2pi() + F.logdet
        quad = lambda r: (solve_lower(F.L, r) ** 2).sum(axis=1)
        e0 = -(cst + quad(x - xn)) / 2
        e1 = F.log_ic - (((x - xn) / F.sd_dens[None, :]) ** 2).sum(axis=1) / 2
        e2_0, e2_1 = -(cst + quad(x - mu)) / 2, -(cst + quad(xn - mu)) / 2
        a = float(alpha)
        ws = (a, (1.0 - a) / 2.0, (1.0 - a) / 2.0)
        e1_lit, b_lit = running_product(F, x, xn)
        q0, b0 = _mix(ws, (e0, e1_lit, e2_0), (None, e1, None), (None, b_lit, None))
        q1, b1 = _mix(ws, (e0, e1_lit, e2_1), (None, e1, None), (None, b_lit, None))
        q0 = np.where((q0 == np.inf) & (q1 == np.inf), LD(0), q0)
        diff = q0 - q1
        S = np.where(np.isfinite(q0), np.abs(q0), 0) + np.where(np.isfinite(q1), np.abs(q1), 0)
    return Dens(e0, e1, e2_0, e2_1, q0, q1, diff, S, b0 | b1)


# ------------------------------------------------------------------------------------------------ the factor of the step size
@dps50
def factor_mp(accept, target):
    """0.95 + 0.10 e^x / (1 + e^x), x = 16 (accept - target), of the FP64 (or rational: an mpf) accept -> mpf"""
    x = 16 * (mp.mpf(accept) - mp.mpf(float(target)))
    return mp.mpf("0.95") + mp.mpf("0.10") * mp.exp(x) / (1 + mp.exp(x))


@dps50
def factor_mp2(accept, target):
    """written differently: 1 - 0.05 tanh(-x / 2) ... = 0.95 + 0.10 / (1 + e^-x) = 1 + 0.05 tanh(x / 2)"""
    x = 16 * (mp.mpf(accept) - mp.mpf(float(target)))
    return 1 + mp.tanh(x / 2) / 20


NAN_ACCEPT = 0.25 + 709.782712893384 / 16.0     # with target 0.25: e^x overflows above this accept and the literal FP64 formula is Inf / Inf = NaN;
                                                # the accept column is at most n_mh_steps (quirk Q2), so from 45 MH steps on


# ------------------------------------------------------------------------------------------------ one call
Step = collections.namedtuple("Step", "t block pos idx comp active theta_new scale z u_dec uc dens inb ll ll_S lp lp_S old old_S log_eta S_eta log_u outcome state_theta state_cols")
Result = collections.namedtuple("Result", "steps theta cols count dropped accept_col rate")


def own_blocks(case):
    sp = case.spec
    free = [k for k in range(len(sp["priors"])) if not sp["fixed"][k]]
    return generate_blocks(len(free), case.n_blocks, free, case.seed, case.stage)


def mutate(case, tol=FLOOR_DECIDE, blocks=None, pid0=0):
    """the whole call on the cloud of `case` (columns d .. d + 2: the particle's loglh, logprior, old_loglh as FP64) -> Result; every proposal's
    figures in .steps.  A particle leaves the call (DROPPED) after an UNDECIDED or BAND decision of its own."""
    sp, P0 = case.spec, case.cloud
    n, d = P0.shape[0], P0.shape[1] - 5
    free = [k for k in range(d) if not sp["fixed"][k]]
    bf, ba, bp = own_blocks(case) if blocks is None else blocks
    nb = len(bp) - 1
    Fs = [block_factor(case.mu, case.Sigma, bf[bp[b]:bp[b + 1]], case.c) for b in range(nb)]
    theta, cols = np.array(P0[:, :d], dtype=np.float64, order="C"), np.array(P0[:, d:d + 3], dtype=np.float64)
    count, active = np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    pid = np.arange(n, dtype=np.uint64) + np.uint64(pid0)
    phi = LD(np.float64(case.phi))
    steps = []
    for step in range(case.n_mh):
        for b in range(nb):
            F, t = Fs[b], step * nb + b
            pos = ba[bp[b]:bp[b + 1]]
            st = stream(case.seed, pid, case.stage, t, F.db)
            z = tr.f64(block_normals(st, F.db))
            comp = component(st.uc, case.alpha)
            xb = theta[:, pos]
            thn_ld, scale = draw(F, xb, z, comp)
            thn = tr.f64(thn_ld)
            D = densities(F, xb, thn, case.alpha)
            para_new = theta.copy()
            para_new[:, pos] = thn
            T = tr.target(sp, para_new)
            with np.errstate(all="ignore"):
                ll, lp, old = T.ll, T.lp, T.old
                dead = T.inb & (tr.f64(ll) == -np.inf)                                  # -Inf on the new data takes the prior with it
                lp = np.where(dead, -LD(np.inf), lp)
                c0, c1, c2 = cols[:, 0].astype(LD), cols[:, 1].astype(LD), cols[:, 2].astype(LD)
                log_eta = phi * (ll - c0) + (1 - phi) * (old - c2) + (lp - c1) + D.diff
                fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0)
                S_eta = phi * (fin(T.ll_S) + fin(c0)) + (1 - phi) * (fin(T.old_S) + fin(c2)) + fin(T.lp_S) + fin(c1) + D.S
                log_u = np.log(st.u_dec.astype(LD))
                out = np.where(np.isnan(log_eta), NAN_REJECT, np.where(log_u < log_eta, ACCEPT, REJECT))
                close = np.isfinite(log_eta) & (np.abs(log_u - log_eta) <= LD(tol) * np.maximum(LD(1), S_eta))
            out = np.where(close, UNDECIDED, out)
            out = np.where(D.band, BAND, out)
            out = np.where(active, out, DROPPED)
            steps.append(Step(t, b, np.asarray(pos), F.idx, comp, active.copy(), thn_ld, scale, z, st.u_dec, st.uc, D, T.inb, ll, T.ll_S, lp, T.lp_S, old, T.old_S, log_eta, S_eta, log_u, out,
                              theta.copy(), cols.copy()))
            acc = out == ACCEPT
            theta[np.ix_(acc, pos)] = thn[acc]
            cols[acc, 0], cols[acc, 1], cols[acc, 2] = tr.f64(ll)[acc], tr.f64(lp)[acc], tr.f64(old)[acc]
            count[acc] += F.db
            active = active & (out != UNDECIDED) & (out != BAND)
    dropped = ~active
    col = count.astype(np.float64) / float(len(free))         # one correctly rounded division of two exact integers
    return Result(steps, theta, cols, count, dropped, col, None if dropped.any() else mp.mpf(int(count.sum())) / (len(free) * n))


def left_out(res):
    """(undecided, band, dropped, decisions) of a call"""
    o = np.concatenate([s.outcome for s in res.steps])
    return int((o == UNDECIDED).sum()), int((o == BAND).sum()), int((o == DROPPED).sum()), int(o.size)


def nerr_theta(got, ref, scale):
    """|Δ_k| / s_k per element; where the reference is NaN `got` must be NaN (0, else Inf), and nowhere else"""
    got, rn = np.asarray(got, dtype=np.float64), np.isnan(tr.f64(ref))
    with np.errstate(all="ignore"):
        e = (np.abs(got.astype(LD) - ref) / np.where(scale > 0, scale, LD(1))).astype(np.float64)
    return np.where(rn, np.where(np.isnan(got), 0.0, np.inf), np.where(np.isnan(got), np.inf, e))


def nerr_log(got, ref, S):
    """|got - ref| / max(1, S); NaN and ±Inf must come back as themselves"""
    got, ref64 = np.asarray(got, dtype=np.float64), tr.f64(ref)
    rn = np.isnan(ref64)
    e = tr.nerr(np.where(rn, 0.0, got), np.where(rn, LD(0), ref), S)
    return np.where(rn, np.where(np.isnan(got), 0.0, np.inf), np.where(np.isnan(got), np.inf, e))


# ------------------------------------------------------------------------------------------------ the classes
Case = collections.namedtuple("Case", "label spec cloud mu Sigma c alpha phi n_blocks n_mh stage seed cond")
# cond: what the class says of the case, asserted for the reference alone by tests/test_mutation_ref_cpu.py - keys: accept (lo, hi): the share of
# accepted decisions; outside (lo, hi): the share of proposals outside the bounds; nan_reject (lo, hi); comps: the components that must be drawn
N_CLASS = 300
SEED, STAGE = 123, 7


def gspec(d, m=0.0, sigma=1.0, prior_sd=10.0, lo=-1e5, hi=1e5, fixed=None):
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), (d,))
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,))
    pri = [("normal", float(m[k]), float(prior_sd)) for k in range(d)]
    return tr._spec(pri, [(float(lo[k]), float(hi[k])) for k in range(d)], tr._gauss(m, sigma), fixed=fixed)


def cloud_of(spec, theta, old_spec=False):
    """the cloud whose columns d .. d + 2 are the FP64 roundings of the reference target at its θ (old_loglh 0 without an old vintage), weights 1"""
    theta = np.asarray(theta, dtype=np.float64)
    n, d = theta.shape
    T = tr.target(spec, theta)
    P = np.zeros((n, d + 5), order="F")
    P[:, :d], P[:, d], P[:, d + 1], P[:, d + 2], P[:, d + 4] = theta, tr.f64(T.ll), tr.f64(T.lp), tr.f64(T.old), 1.0
    return P


def own_moments(theta, free, rows=None):
    """the equally weighted mean and covariance of the free columns, summed in longdouble, rounded to FP64 (symmetric)"""
    X = np.asarray(theta, dtype=np.float64)[:, free].astype(LD)
    if rows is not None:
        X = X[rows]
    m = X.mean(axis=0)
    C = (X - m).T @ (X - m) / LD(len(X))
    C = (C + C.T) / 2
    return tr.f64(m), tr.f64(C)


def _free(spec):
    return [k for k in range(len(spec["priors"])) if not spec["fixed"][k]]


def _case(label, spec, theta, c=0.4, alpha=1.0, phi=0.3, n_blocks=1, n_mh=1, mu=None, Sigma=None, cloud=None, cond=None, stage=STAGE, seed=SEED):
    free = _free(spec)
    m, S = own_moments(theta, free)
    return Case(label, spec, cloud_of(spec, theta) if cloud is None else cloud, m if mu is None else mu, S if Sigma is None else Sigma, float(c), float(alpha), float(phi),
                int(n_blocks), int(n_mh), stage, seed, dict(cond or {}))


def _normal_cloud(rng, n, m, sd):
    m, sd = np.asarray(m, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    return m[None, :] + sd[None, :] * rng.standard_normal((n, len(m)))


def _benign(n):
    out = []
    for name, nb, alpha in (("sixpriors", 1, 1.0), ("sixpriors", 2, 0.9), ("ten", 1, 0.9), ("ten", 3, 1.0), ("wide12", 1, 1.0), ("wide12", 3, 0.9)):
        sp = getattr(tr, name)()
        out.append(_case("%s n_blocks=%d alpha=%g" % (name, nb, alpha), sp, tr.prior_draws(sp, n, _seed("benign", name)), alpha=alpha, n_blocks=nb, cond=dict(accept=(0.02, 0.9))))
    for nb, alpha in ((1, 1.0), (3, 0.9)):                    # d = 20: the generic body's wider columns
        rng = np.random.default_rng(_seed("benign", 20))
        out.append(_case("gauss20 n_blocks=%d alpha=%g" % (nb, alpha), gspec(20, 0.0, 1.0, 10.0), _normal_cloud(rng, n, np.zeros(20), np.ones(20)), c=0.3, alpha=alpha, n_blocks=nb,
                         cond=dict(accept=(0.02, 0.9))))
    return out


def _ill(n):
    """correlations up to 1 - 1e-6 and column scales 1e-6 .. 1e6 (tests/moments_ref.py's ranges) under a flat target"""
    out = []
    for d, rho, alpha, nb in ((6, 1 - 1e-3, 1.0, 1), (6, 1 - 1e-6, 0.9, 1), (10, 1 - 1e-6, 1.0, 2), (10, 1 - 1e-4, 0.9, 3), (12, 1 - 1e-6, 0.9, 1)):
        rng = np.random.default_rng(_seed("ill", d, rho, alpha))
        sc = 10.0 ** np.linspace(-6, 6, d)[rng.permutation(d)]
        g = rng.standard_normal((n, 1)) * np.sqrt(rho) + rng.standard_normal((n, d)) * np.sqrt(1 - rho)
        sp = gspec(d, 0.0, 1e12, 1e12, -1e15, 1e15)
        out.append(_case("d=%d rho=1-%.0e alpha=%g n_blocks=%d" % (d, 1 - rho, alpha, nb), sp, g * sc[None, :], alpha=alpha, n_blocks=nb, cond=dict(accept=(0.5, 1.0))))
    return out


def _far(n):
    """the cloud 1e4 and 1e8 standard deviations from the origin (the target's centre with it)"""
    out = []
    for d, k, alpha, nb in ((6, 1e4, 1.0, 1), (6, 1e8, 0.9, 2), (10, 1e8, 1.0, 1), (10, 1e4, 0.9, 3), (12, 1e8, 0.9, 1)):
        rng = np.random.default_rng(_seed("far", d, k, alpha))
        sd = 10.0 ** rng.uniform(-1, 1, d)
        m = k * sd * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        sp = gspec(d, m, float(np.exp(np.mean(np.log(sd)))), 1e10, -1e12, 1e12)
        out.append(_case("d=%d %g sd alpha=%g n_blocks=%d" % (d, k, alpha, nb), sp, _normal_cloud(rng, n, m, sd), alpha=alpha, n_blocks=nb, cond=dict(accept=(0.02, 0.95))))
    return out


def _mu_far(n):
    """θ̄ tens of standard deviations from the cloud: the third component vanishes for q0 (a draw of component 0 or 1, and for q1 with it) or for
    q0 only (a draw of component 2, which lands at θ̄)"""
    out = []
    for d, k, alpha in ((6, 30.0, 0.5), (10, 60.0, 0.5), (6, 45.0, 0.0), (12, 30.0, 0.5)):
        rng = np.random.default_rng(_seed("mufar", d, k))
        sd = 10.0 ** rng.uniform(-1, 1, d)
        th = _normal_cloud(rng, n, np.zeros(d), sd)
        sp = gspec(d, 0.0, 3.0 * float(sd.max()), 1e3, -1e5, 1e5)
        m, S = own_moments(th, list(range(d)))
        out.append(_case("d=%d mu %g sd off alpha=%g" % (d, k, alpha), sp, th, alpha=alpha, mu=tr.f64(m + k * sd), cond=dict(comps=(0, 1, 2) if alpha > 0 else (1, 2))))
    return out


FLAT_S = (1e30, 1.5e32, 1e40)         # tests/test_gpu_proposal_paths.py: nobody / some / everybody rejected by underflow (d = 10, c = 0.5)
SMALL_S = (1e-29, 2e-31, 1e-31, 5e-32, 1e-33, 1e-40)        # the other end: -(d log 2π + log|c²Σ|) / 2 from below to beyond the overflow point of exp


def _density_scale(n):
    """the cloud (and with it c²Σ) scaled by decades under a flat target: log|c²Σ_b| runs to both ends of what the literal FP64 form survives"""
    out = []
    # (α < 1 on the underflow side: 1e26 and 1e34 - between them the carrying exponents lie in the subnormal range, which is the band)
    for s, alpha in [(s, 1.0) for s in FLAT_S + SMALL_S] + [(s, 0.9) for s in (1e26, 1e34) + SMALL_S]:
        rng = np.random.default_rng(_seed("scale", s, alpha))
        sp = gspec(10, 0.0, 1e45, s, -1e45, 1e45)
        th = _normal_cloud(rng, n, np.zeros(10), np.full(10, s))
        out.append(_case("s=%g alpha=%g" % (s, alpha), sp, th, c=0.5, alpha=alpha, Sigma=np.diag(np.full(10, s)) @ np.diag(np.full(10, s)), mu=np.zeros(10)))
    return out


def _alpha(n):
    out = []
    sp = gspec(6, 0.0, 1.0, 10.0, -1e9, 1e9)
    rng = np.random.default_rng(_seed("alpha"))
    th = _normal_cloud(rng, n, np.zeros(6), 10.0 ** rng.uniform(-1, 1, 6))
    for alpha in (1.0, 0.9, 0.5, 0.0):
        for c in (1e-8, 0.4, 1e4):
            out.append(_case("alpha=%g c=%g" % (alpha, c), sp, th, c=c, alpha=alpha, cond=dict(comps=(0,) if alpha == 1 else ((1, 2) if alpha == 0 else (0, 1, 2)))))
    # α within an ulp of a component uniform: rows 5 and 17 of proposal 0 - below α the row draws component 0, at and above it component 1
    uc = stream(SEED, np.arange(n, dtype=np.uint64), STAGE, 0, 6).uc
    for row in (5, 17):
        for k, a in enumerate((np.nextafter(uc[row], 0.0), uc[row], np.nextafter(uc[row], 1.0))):
            out.append(_case("alpha=uc[%d]%+d ulp" % (row, k - 1), sp, th, alpha=float(a), cond=dict(row=row, comp=0 if k == 2 else 1)))
    return out


def _tight(n):
    """a cloud that fills its bounds evenly (every bound within a standard deviation of cloud): between a sixth and a half of the proposals leave them"""
    out = []
    for d, alpha, nb, w, c in ((6, 1.0, 1, 1.8, 0.4), (6, 0.9, 2, 1.5, 0.5), (10, 1.0, 1, 2.1, 0.25), (12, 0.9, 3, 1.5, 0.5)):
        rng = np.random.default_rng(_seed("tight", d, alpha))
        sd = 10.0 ** rng.uniform(-1, 1, d)
        m = rng.uniform(-3, 3, d)
        th = m[None, :] + sd[None, :] * rng.uniform(-w, w, (n, d)) * 0.999
        sp = gspec(d, m, 2.0 * float(sd.max()), 10.0, m - w * sd, m + w * sd)
        out.append(_case("d=%d alpha=%g n_blocks=%d" % (d, alpha, nb), sp, th, c=c, alpha=alpha, n_blocks=nb, cond=dict(outside=(0.15, 0.6))))
    return out


def _dead(n):
    """rows with loglh = -Inf (every seventh) and rows with a NaN parameter (every eleventh; their three columns -Inf, as scoring leaves them); the
    proposal's moments are those of the other rows"""
    out = []
    for name, alpha, nb in (("sixpriors", 1.0, 1), ("ten", 0.9, 2), ("wide12", 0.9, 3)):
        sp = getattr(tr, name)()
        th = tr.prior_draws(sp, n, _seed("dead", name))
        free = _free(sp)
        ok = np.ones(n, dtype=bool)
        P = cloud_of(sp, th)
        d = th.shape[1]
        for i in range(n):
            if i % 7 == 3:
                P[i, d], ok[i] = -np.inf, False
            if i % 11 == 5:
                P[i, free[(i // 11) % len(free)]], ok[i] = np.nan, False
                P[i, d:d + 3] = -np.inf
        m, S = own_moments(th, free, ok)
        out.append(_case("%s alpha=%g n_blocks=%d" % (name, alpha, nb), sp, th, alpha=alpha, n_blocks=nb, mu=m, Sigma=S, cloud=P, cond=dict(nan_reject=(0.02, 0.5))))
    return out


def _phi(n):
    out = []
    for old_n in (None, 50):
        sp = tr.linreg(100, old_n=old_n)
        rng = np.random.default_rng(_seed("phi", old_n))
        th = np.column_stack([rng.normal(1.0, 0.3, n), rng.normal(2.0, 0.3, n)])
        for phi in (1e-12, 0.3, 1.0):
            out.append(_case("linreg old=%s phi=%g" % (old_n, phi), sp, th, c=0.4, alpha=0.9 if phi < 1 else 1.0, phi=phi, cond=dict(accept=(0.02, 0.995))))
    return out


def _blocks(n):
    """d = 10 with two fixed parameters (n_free = 8): n_blocks 1, 2, 3 (blocks of 3, 3, 2: odd and even), 8; 1 and 3 MH steps"""
    out = []
    sp = tr.ten()
    sp["fixed"] = [0, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    th = tr.prior_draws(sp, n, _seed("blocks"))
    for nb in (1, 2, 3, 8):
        for n_mh in (1, 3):
            alpha = 0.9 if (nb + n_mh) % 2 else 1.0
            out.append(_case("n_blocks=%d n_mh=%d alpha=%g" % (nb, n_mh, alpha), sp, th, alpha=alpha, n_blocks=nb, n_mh=n_mh, cond=dict(accept=(0.02, 0.95))))
    return out


CLASSES = collections.OrderedDict([("benign", _benign), ("ill_conditioned", _ill), ("far", _far), ("mu_far", _mu_far), ("density_scale", _density_scale), ("alpha", _alpha),
                                   ("tight_bounds", _tight), ("dead_rows", _dead), ("phi", _phi), ("blocks", _blocks)])


def cases(name, n=N_CLASS):
    """the cases of a class; seeded: the same every time"""
    return CLASSES[name](n)
