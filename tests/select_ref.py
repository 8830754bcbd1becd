"""An exact reference for the selection step, and the clouds the selection tests run on.

Doubles are exact rationals: the weights become Python integers on the common scale 2^-1074, the prefix sums C_j and the total
S are exact, and slot k's threshold t - the FP64 value of (k + u) / n_out for systematic, u_k for multinomial, the same two correctly
rounded operations the reference package and the device perform - is compared with the boundary C_j / S by integer
cross-multiplication.  No rounding enters anywhere, so the ancestor (the first j with C_j / S > t, src/resample.jl:33-70) carries no
tolerance.

THE RULE (here, in the restatement oracle/smc_oracle.c and in the device's gathers): if the row found has weight 0, or the search
falls through, the ancestor is the nearest row before it with positive weight.  In exact arithmetic a zero-weight row is never found
(C_j = C_{j-1}) and nothing falls through (t < 1 = C_{n-1} / S); in FP64 both happen (a threshold that rounds to 1.0, a cum column
that ends below 1 or steps up across a zero-weight row) and the rule says what is then right.

No GPU, no oracle library: tests/test_select_ref_cpu.py pins this file to a brute-force fractions.Fraction search.
"""
import bisect
import math

import numpy as np

SCALE = 1074                    # 2^-1074: the smallest subnormal, every finite double is an integer multiple of it
SMALL_SIZES = (5, 257, 1024, 4099)
STAGE_FAMILIES = ("random", "collapse_ends", "collapse_apart", "dust", "zero_ends", "chunk_ends")
FAMILIES = STAGE_FAMILIES + ("exact",)
DEGENERATE = ("all_on_first", "all_on_last", "all_on_mid", "single")
MARGIN_FLOOR = 2.0 ** -43       # 1 024 ulp of 1: the longest chain of additions behind any cum value (the carry over <= 1 024 chunk sums)


def exact_int(x):
    """the double x >= 0 as an integer multiple of 2^-1074"""
    m, e = math.frexp(float(x))                     # x = m 2^e, 0.5 <= m < 1
    q = int(m * 9007199254740992.0)                 # m 2^53: an integer, exactly
    s = e - 53 + SCALE
    return q << s if s >= 0 else q >> -s            # (s < 0 only for subnormals, whose low bits are 0)


def thresholds(method, n_out, offsets):
    """the FP64 thresholds of the n_out slots"""
    if method == "multinomial":
        t = np.ascontiguousarray(offsets, dtype=np.float64)
        assert t.size == n_out
        return t
    u = float(np.atleast_1d(offsets)[0])
    return (np.arange(n_out, dtype=np.float64) + u) / float(n_out)


class Cloud:
    """Exact prefix sums of one weight vector; select() then serves any number of offset sets."""

    def __init__(self, weights):
        self.w = np.ascontiguousarray(weights, dtype=np.float64)
        assert self.w.ndim == 1 and self.w.size >= 1 and np.all(np.isfinite(self.w)) and np.all(self.w >= 0)
        self.n = self.w.size
        self.C, run = [], 0
        for x in self.w.tolist():
            run += exact_int(x)
            self.C.append(run)
        self.S = run
        assert self.S > 0
        pos = self.w > 0
        idx = np.arange(self.n)
        self.prev_pos = np.maximum.accumulate(np.where(pos, idx, -1))                 # last positive row <= j (-1: none)
        self.next_pos = np.minimum.accumulate(np.where(pos, idx, self.n)[::-1])[::-1]  # first positive row >= j (n: none)

    def cum_float(self):
        """C_j / S correctly rounded: what a cum column approximates"""
        S = self.S
        return np.array([c / S for c in self.C])

    def cum_error(self, cum):
        """largest |cum_j - C_j / S| of an FP64 cum column, as a float (exact difference, rounded once)"""
        S, worst = self.S, 0.0
        for c, x in zip(self.C, np.asarray(cum, dtype=np.float64).tolist()):
            worst = max(worst, _absdiff(c, S, x))
        return worst

    def interval_distance(self, j, t):
        """distance from the threshold t to row j's interval [C_{j-1}, C_j) / S (0 inside), exact, rounded once"""
        tn, td = float(t).as_integer_ratio()
        lo, hi, num = (self.C[j - 1] if j > 0 else 0) * td, self.C[j] * td, tn * self.S
        return (lo - num) / (td * self.S) if num < lo else ((num - hi) / (td * self.S) if num >= hi else 0.0)

    def select(self, method, n_out, offsets):
        """-> dict(anc, dist, side, lower, upper, thr): per slot the ancestor, the distance from the threshold to the nearer of the two
        boundaries C_{a-1} / S (side -1) and C_a / S (side +1) that have a positive-weight row beyond them (inf: neither has), and the
        positive-weight rows next to the ancestor (-1 / n: none)."""
        thr = thresholds(method, n_out, offsets)
        C, S, n = self.C, self.S, self.n
        anc = np.empty(n_out, dtype=np.int64)
        dist = np.empty(n_out)
        side = np.zeros(n_out, dtype=np.int64)
        lower = np.empty(n_out, dtype=np.int64)
        upper = np.empty(n_out, dtype=np.int64)
        for k, t in enumerate(thr.tolist()):
            assert 0.0 <= t <= 1.0
            tn, td = t.as_integer_ratio()
            num = tn * S                                            # t = num / (td S) on the boundaries' scale
            j = bisect.bisect_right(C, num // td)                   # first j with C_j td > num  <=>  C_j > floor(num / td)
            if j >= n:                                              # fall-through (t == 1.0): the rule
                j = n - 1
            a = int(self.prev_pos[j])                               # (exact search never finds a zero-weight row; fall-through may)
            lo = int(self.prev_pos[a - 1]) if a > 0 else -1
            up = int(self.next_pos[a + 1]) if a + 1 < n else n
            anc[k], lower[k], upper[k] = a, lo, up
            den = td * S
            d_lo = (num - (C[a - 1] if a > 0 else 0) * td) / den if lo >= 0 else math.inf
            d_up = (C[a] * td - num) / den if up < n else math.inf
            dist[k] = min(abs(d_lo), abs(d_up))
            side[k] = 0 if dist[k] == math.inf else (-1 if abs(d_lo) <= abs(d_up) else 1)
        return dict(anc=anc, dist=dist, side=side, lower=lower, upper=upper, thr=thr)


def _absdiff(c, S, x):
    """|x - c / S| for the double x, exactly, rounded once"""
    xn, xd = float(x).as_integer_ratio()
    return abs(xn * S - c * xd) / (xd * S)


def brute_force(weights, thr):
    """first j with C_j / S > t by fractions.Fraction, then the rule: O(n) per slot, for small clouds"""
    from fractions import Fraction

    w = [Fraction(float(x)) for x in weights]
    S = sum(w)
    out = []
    for t in thr:
        t = Fraction(float(t))
        run, j = Fraction(0), len(w)
        for i, x in enumerate(w):
            run += x
            if run / S > t:
                j = i
                break
        j = min(j, len(w) - 1)
        while w[j] == 0:
            j -= 1
        out.append(j)
    return np.array(out, dtype=np.int64)


def margin(ref_cloud, restatement_cum, exact=False):
    """MARGIN of a cloud: 16 x the restatement's largest cum error (the project's usual factor over the restatement's own arithmetic),
    at least 2^-43; 0 on exact clouds"""
    if exact:
        return 0.0
    return max(16.0 * ref_cloud.cum_error(restatement_cum), MARGIN_FLOOR)


def restatement_cum(weights):
    """the cum column of oracle/smc_oracle.c orc_resample_with_offsets: run += w / s, sequentially"""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    s = 0.0
    for x in w.tolist():
        s += x
    return np.cumsum(w / s)         # (numpy's cumsum of a 1-d double array is the sequential sum)


def judge(ref, got, weights, mg, method, cap=2, exempt=None, cloud=None):
    """The assertions per slot -> (list of failures, figures).  decided: the reference's ancestor; undecided (threshold within mg of a
    boundary): the reference's or the neighbouring positive-weight row on the threshold's side - and, with `cloud` (the exact Cloud of the
    weights), any positive-weight row whose whole interval lies within mg of the threshold: rows of dust or of weight 1e-12 are narrower
    than mg, and a cum column that is off by less than mg may land several of them away; always: positive weight, systematic ancestors
    non-decreasing, undecided slots within the cap."""
    got = np.asarray(got, dtype=np.int64)
    w = np.asarray(weights)
    und = ref["dist"] <= mg if mg > 0 else np.zeros(got.size, dtype=bool)
    nb = np.where(ref["side"] < 0, ref["lower"], ref["upper"])
    ok = (got == ref["anc"]) | (und & (got == nb))
    why = []
    inb = (got >= 0) & (got < w.size)
    if cloud is not None:
        for k in np.flatnonzero(und & ~ok & inb).tolist():
            ok[k] = bool(w[got[k]] > 0 and cloud.interval_distance(int(got[k]), float(ref["thr"][k])) <= mg)
    if not inb.all():
        why.append("%d ancestors outside the cloud" % int((~inb).sum()))
        got = np.clip(got, 0, w.size - 1)
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        why.append("%d slots differ from the reference; first: slot %d got %d want %d (threshold %r, distance %.3g, weight of got %r)"
                   % (int((~ok).sum()), k, int(got[k]), int(ref["anc"][k]), float(ref["thr"][k]), float(ref["dist"][k]), float(w[got[k]])))
    if not np.all(w[got] > 0):
        why.append("%d ancestors of weight 0" % int(np.count_nonzero(w[got] <= 0)))
    if method == "systematic" and not np.all(np.diff(got) >= 0):
        why.append("systematic ancestors decrease")
    counted = und if exempt is None else und & ~np.asarray(exempt)       # (exempt: offsets placed on or next to boundaries on purpose)
    if int(counted.sum()) > cap:
        why.append("%d undecided slots (input condition: at most %d)" % (int(counted.sum()), cap))
    fig = dict(undecided=int(und.sum()), wrong=int((~ok).sum()), zero=int(np.count_nonzero(w[got] <= 0)),
               min_dist=float(ref["dist"].min()) if got.size else math.inf)
    return why, fig


def ess(weights):
    """(Σ w)^2 / Σ w^2 with correctly rounded sums"""
    w = np.asarray(weights, dtype=np.float64)
    return math.fsum(w.tolist()) ** 2 / math.fsum((w * w).tolist())


def widest_tile_span(anc, tile=512):
    """largest anc[last slot of a tile] - anc[first] + 1 over the tiles of `tile` consecutive slots"""
    a = np.asarray(anc)
    return int(max(a[min(i + tile, a.size) - 1] - a[i] + 1 for i in range(0, a.size, tile)))


# ------------------------------------------------------------------------------------------------ the clouds
def exact_size(n):
    """the exact family needs a power of two: the largest one <= n"""
    return 1 << (int(n).bit_length() - 1)


def make_cloud(family, n, seed=0):
    """The weight vector of one family at size n (one generator for every test file).  The figures of the families are those of the
    stage sizes (16 384 and up); below they shrink in proportion so that every family exists at the stand-alone sizes too."""
    rng = np.random.default_rng([seed, n, sum(map(ord, family))])
    w = np.zeros(n)
    if family == "random":                                      # as tests/test_gpu_parity.py test_resample_vs_oracle: one in seven rows zero
        w = rng.random(n) * 2.0
        w[rng.integers(0, n, n // 7)] = 0.0
        if not w.any():
            w[0] = 1.0
    elif family in ("collapse_ends", "collapse_apart"):         # two clusters of weight 1, of different sizes: the crossing falls inside a tile
        c1, c2 = min(300, max(1, n // 8)), min(340, max(1, n // 7))
        if family == "collapse_ends":
            w[:] = 1e-12
            w[:c1] = 1.0
            w[n - c2:] = 1.0
        else:
            gap = min(3000, max(0, n - c1 - c2))
            s0 = (n - c1 - c2 - gap) // 2
            w[s0:s0 + c1] = 1.0
            w[s0 + c1 + gap:s0 + c1 + gap + c2] = 1.0
    elif family == "dust":                                      # 1 024 rows of order 1 in log-uniform dust, subnormals included
        big = min(1024, max(2, n // 4))
        w = 10.0 ** rng.uniform(-320.0, -10.0, n)
        at = rng.choice(n, big, replace=False)
        at[:2] = (0, n - 1)                                     # (the first and the last row are large ones: a threshold at an end of [0, 1)
        w[at] = 0.5 + rng.random(big)                           # is then inside a wide interval, not within MARGIN of a run of dust)
    elif family == "zero_ends":                                 # whole chunks and a whole virtual shard of nothing
        head, tail = min(1000, n // 4), min(n // 8 + 7, n // 2)
        w = rng.random(n) * 2.0 + 1e-3
        w[:head] = 0.0
        w[n - tail:] = 0.0
    elif family == "chunk_ends":
        i = np.arange(n)
        w[(i % 512 == 0) | (i % 512 == 511)] = 1.0
        w[i % 512 == 255] = 2.0 ** -30
        w[rng.choice(n, min(600, max(1, n // 8)), replace=False)] += 0.25
    elif family == "exact":                                     # multiples of 2^-11 that total n exactly: every sum in every order is exact
        assert n & (n - 1) == 0, "the exact family needs a power of two"
        m = rng.integers(1, 4097, n)
        m[rng.random(n) < 0.3] = 0
        if not m.any():
            m[0] = 1
        live = np.flatnonzero(m)
        diff = int(n * 2048 - m.sum())
        q, r = divmod(diff, live.size)                          # spread the difference, then walk off what clipping at 1 left over
        m[live] += q
        m[live[:r]] += 1
        m[live] = np.maximum(m[live], 1)
        k = 0
        while m.sum() != n * 2048:
            j = live[k % live.size]
            step = int(n * 2048 - m.sum())
            m[j] = max(1, m[j] + step)
            k += 1
        w = m / 2048.0
        assert w.sum() == n and np.all(w * 2048 == np.round(w * 2048))
    elif family == "all_on_first":
        w[0] = 1.0
    elif family == "all_on_last":
        w[n - 1] = 1.0
    elif family == "all_on_mid":
        w[(n // 2) | 1 if n > 2 else 0] = 1.0
    elif family == "single":
        w = np.ones(1)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(w, dtype=np.float64)


def has_zero_rows(w):
    return bool(np.any(np.asarray(w) == 0))


def fixed_offsets():
    """offsets at the ends of [0, 1) and in the middle"""
    return [2.0 ** -53, 0.5, 1.0 - 2.0 ** -45, 1.0 - 2.0 ** -53]


def ulp_sweep(ref_cloud, max_rows=60, seed=0):
    """Multinomial offsets: for each of up to max_rows zero-weight rows j (with a positive row before them), the 17 doubles within
    +-8 ulp of fl(C_{j-1} / S); the same around the final boundary when trailing rows are zero."""
    w, n, C, S = ref_cloud.w, ref_cloud.n, ref_cloud.C, ref_cloud.S
    rows = np.flatnonzero((w == 0) & (np.arange(n) > 0) & (ref_cloud.prev_pos >= 0))
    if rows.size > max_rows:
        rng = np.random.default_rng(seed)
        rows = np.sort(rng.choice(rows, max_rows, replace=False))
    rows = list(rows)
    if w[n - 1] == 0 and (n - 1) not in rows:
        rows.append(n - 1)
    out = []
    for j in rows:
        c = C[j - 1] / S
        x = c
        for _ in range(8):
            x = np.nextafter(x, 0.0)
        for _ in range(17):
            if 0.0 <= x < 1.0:
                out.append(float(x))
            x = np.nextafter(x, 2.0)
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the cases both test files walk
SEED, STAGE = 5, 2              # the handles' seed and the bracketed stage: the Philox offset of the stage vehicle
STAGE_N, EXACT_STAGE_N, TWO_CHUNK_N = 20480, 16384, 150004
TWO_CHUNK_FAMILIES = ("collapse_ends", "zero_ends")
ENSEMBLE_SIZES = ((8192, 10), (4096, 10), (1000, 3))


def small_cases():
    """(family, n) of the stand-alone calls: every family at the four small sizes (exact: the power of two below), the degenerate ones"""
    out = []
    for n in SMALL_SIZES:
        out += [(f, exact_size(n) if f == "exact" else n) for f in FAMILIES]
        out += [(f, n) for f in DEGENERATE[:3]]
    return out + [("single", 1)]


def stage_cases():
    return [(f, STAGE_N) for f in STAGE_FAMILIES] + [("exact", EXACT_STAGE_N)]


def systematic_offsets(family):
    """the given offsets of a stand-alone systematic call; exact clouds add 0 and multiples of 2^-11 (thresholds ON boundaries: > against >=)"""
    off = fixed_offsets()
    if family == "exact":
        off += [0.0, 3.0 / 2048.0, 1024.0 / 2048.0, 2047.0 / 2048.0]
    return off


def multinomial_offsets(ref_cloud, family, n_out, seed=0, max_calls=12):
    """the given offsets of the stand-alone multinomial calls: a list of (n_out offsets, mask of the slots placed on purpose).  Pool: the fixed offsets, on exact clouds
    0 and multiples of 2^-11, the ulp sweep where the cloud has zero rows, random ones."""
    rng = np.random.default_rng([seed, n_out, ref_cloud.n])
    pool = list(fixed_offsets())
    if family == "exact":
        pool += [0.0] + list(rng.integers(0, 2048, 40) / 2048.0)
    sweep = []
    if has_zero_rows(ref_cloud.w):
        room = max(17, max_calls * n_out - len(pool) - n_out)
        sweep = list(ulp_sweep(ref_cloud, max_rows=max(1, min(60, room // 17 - 1)), seed=seed))[:max(0, max_calls * n_out - len(pool))]
    mask = [True] * len(pool) + [True] * len(sweep)     # (placed on or next to boundaries on purpose: not counted towards the cap of undecided slots)
    pool += sweep
    fill = -len(pool) % n_out
    pool += list(rng.random(fill))
    mask += [False] * fill
    return [(np.array(pool[i:i + n_out]), np.array(mask[i:i + n_out])) for i in range(0, len(pool), n_out)]


def ensemble_cases():
    """size -> (n_para, families): the members of one ensemble launch.  1 000 particles: no power of two, and the chunk_ends family has
    fewer than 50 n_para distinct ancestors there."""
    return {8192: (10, FAMILIES), 4096: (10, FAMILIES), 1000: (3, ("random", "collapse_ends", "collapse_apart", "dust", "zero_ends"))}


MP_N, MP_FAMILIES = 16384, ("collapse_ends", "zero_ends")      # two processes on one GPU, world = 2
