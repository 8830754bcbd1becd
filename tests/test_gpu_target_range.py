"""The target of every MH decision as the device evaluates it - the loglh, logprior and old_loglh columns - against the extended-precision
reference of tests/target_ref.py (pinned by tests/test_target_ref_cpu.py), through every separately written copy of the formulas:
  loglik / logprior (run-time d)      k_initialize_likelihoods<0>, k_init_prior, the generic mutation body, the closure path's proposals
  loglik_s<D> / logprior_s<D>         k_mutate_reg (d <= 10), k2_mutate, k2b_mutate, k3_segment, kens_run; `has_other`, capm_literal's scalar reads
  stage_lik                           both vintages on both sides of the 768-double LDS cap
Every error is |Δ| / max(1, S) of tests/target_ref.py.  The bar of a case and column: max(1e-13, 16 x the worst normalised error of the FP64
oracle over the same θ), θ at which the oracle is off by more than 1e-10 left out (at most an eighth); the oracle's error is computed in the worker,
on the CPU, before the device's values are looked at.  Wherever the reference is finite the device is finite, wherever it is ±Inf the device
returns the same infinity, and nothing is NaN.  Every test is a child process with its own time limit; a child that dies ends the session.

Vehicles, smallest first: scoring an uploaded cloud (initialize_likelihoods; 200 and 300 rows, the class's 24 θ repeated down the cloud: the last
wavefront and the last block are partial, each θ is scored in several lanes and must give the same bits in each; column d + 2 keeps the bits of
the uploaded loglh) - every class and spec, and rows with NaN parameters (one free parameter, the fixed parameter, every parameter: -Inf in
columns d and d + 1, the same in every lane); the prior draw (init_from_prior on sixpriors and ten: the cloud is the oracle's draw, the scored
columns the reference's at the θ that come back - NOT per class: the draw redraws until it is inside the bounds, and the far, corners, edge and
prior-shapes regions have no or next to no mass under these priors, so there is one draw on the spec's own bounds and one on a hand-picked box
of central mass per spec; those classes reach the device through the other vehicles); the proposals of the closure path (Engine.propose: logprior_out is the reference's, -Inf outside the bounds and outside
the narrow Uniform); a stand-alone mutation (Engine.mutate with the cloud's own weighted moments, c chosen on the CPU with oracle.mutate_cloud so
that a tenth of the rows move and a tenth stay - asserted on what the device did; afterwards every row's three columns are the reference's at that
row's θ, every row is inside the bounds, no row that started finite holds -Inf or NaN); one bracketed stage per engine path (stage 2 on an uploaded
cloud, the PATHS rows of tests/test_gpu_weight_range.py); the ensemble kernel (whole runs of the shortest fixed schedule).

Reproduced quirk: linmodel3 / capm_literal form det = Π σ_i² before its log; for σ products below 1e-154 / above 1e154 - outside the
shipped bounds of [1e-5, 1e5] - the value turns +Inf / -Inf where the reference stays finite.  The device returns what the oracle returns there.

Measured on an MI355X, worst normalised error over the included rows (oracle: the FP64 oracle on the same θ; cases: specs x row counts).  The
bar is its floor, 1e-13, in every line (16 x the oracle's worst error is 5.8e-14 at most); no θ is left out anywhere; every infinity of the
reference (2 000 rows of the corners class, 5 000 of the family edges) comes back as the same infinity; nothing is NaN.

  vehicle            class / spec            likelihood    cases   loglh: oracle  device   logprior: oracle  device   moved
  scoring            prior_like              gauss_iso       6            5.8e-16  5.8e-16            1.7e-16  1.7e-16
  scoring            prior_like              linreg         42            1.3e-15  1.3e-15            2.5e-16  2.5e-16
  scoring            prior_like              linmodel3      16            6.7e-16  6.7e-16            2.7e-16  2.7e-16
  scoring            prior_like              capm_literal   16            3.5e-15  3.5e-15            2.3e-16  2.3e-16
  scoring            corners                 all four       12            2.5e-16  2.5e-16            3.8e-17  3.8e-17
  scoring            far                     gauss_iso       6            2.7e-16  2.7e-16            2.5e-16  2.5e-16
  scoring            far                     linreg          4            6.6e-16  6.6e-16            2.9e-17  2.9e-17
  scoring            far                     linmodel3       4            5.0e-16  5.0e-16            3.8e-17  3.8e-17
  scoring            far                     capm_literal    4            1.3e-15  1.3e-15            3.8e-17  3.8e-17
  scoring            cancelling              linreg          6            8.4e-17  8.4e-17            6.2e-17  6.2e-17
  scoring            cancelling              linmodel3       2            2.6e-15  2.6e-15            1.9e-16  1.9e-16
  scoring            cancelling              capm_literal    2            8.6e-16  8.6e-16            6.8e-17  6.8e-17
  scoring            cancelling              gauss_iso       2            5.3e-17  5.3e-17            1.6e-17  1.6e-17
  scoring            data_scale              linreg          8            9.6e-16  9.6e-16            1.6e-16  1.6e-16
  scoring            data_scale              linmodel3       8            9.1e-16  9.1e-16            2.1e-16  2.1e-16
  scoring            data_scale              capm_literal    8            3.6e-15  3.6e-15            1.9e-16  1.9e-16
  scoring            prior_shapes            gauss_iso      10            1.6e-16  1.6e-16            3.5e-16  3.5e-16
  scoring            family_edges            gauss_iso      28            7.4e-17  7.4e-17            1.6e-16  1.6e-16
  scoring            family_edges (σ = 0)    linmodel3       2            -Inf     -Inf               2.0e-16  2.0e-16
  scoring            NaN rows (2 250: -Inf)  all four       12            3.4e-16  3.4e-16            2.4e-16  2.4e-16
  prior draw         sixpriors, ten (+ box)  gauss_iso       4            5.4e-16  5.4e-16            1.4e-16  1.9e-16
  propose            sixpriors, ten, wide12                 12                                        3.2e-16  3.2e-16
  mutation           prior_like              gauss_iso      12            4.5e-16  4.5e-16            1.9e-16  1.9e-16   0.33 .. 0.83
  mutation           prior_like              linreg          4            5.3e-16  5.3e-16            2.1e-16  2.1e-16   0.28 .. 0.47
  mutation           prior_like              linmodel3       4            9.5e-16  9.5e-16            2.5e-16  2.5e-16   0.27 .. 0.42
  mutation           prior_like              capm_literal    4            1.4e-15  1.4e-15            2.5e-16  2.5e-16   0.25 .. 0.45
  mutation           far                     gauss_iso       6            5.5e-16  5.5e-16            5.3e-16  5.3e-16   0.30 .. 0.71
  mutation           far                     linreg          2            8.5e-16  8.5e-16            2.8e-16  2.8e-16   0.25 .. 0.47
  mutation           far                     linmodel3       2            9.9e-16  9.9e-16            2.6e-16  2.6e-16   0.26 .. 0.57
  mutation           far                     capm_literal    2            4.0e-15  4.0e-15            3.1e-16  3.1e-16   0.26 .. 0.59
  mutation           prior_shapes            gauss_iso       6            3.0e-16  3.0e-16            5.3e-16  3.8e-16   0.25 .. 0.59
  mutation           two vintages            linmodel3       6            9.1e-16  9.1e-16            2.4e-16  2.4e-16   0.30 .. 0.39   old_loglh 9.1e-16 / 9.1e-16
  mutation           two vintages            linreg          6            9.5e-16  9.5e-16            2.1e-16  2.1e-16   0.25 .. 0.53   old_loglh 9.5e-16 / 9.5e-16
  stage, every path  sixpriors / ten         gauss_iso       7            6.1e-16  6.1e-16            1.8e-16  1.9e-16   0.31 .. 0.55
  stage, every path  linmodel3               linmodel3       5            1.1e-15  1.1e-15            3.0e-16  3.0e-16   0.98
  stage, every path  capm                    capm_literal    5            1.8e-15  1.8e-15            2.9e-16  2.9e-16   0.98
  stage two_chunk    linreg (150 004 rows)   linreg          1            6.9e-16  6.9e-16            2.2e-16  2.2e-16   1.00
  stage wide         wide12                  gauss_iso       1            6.4e-16  6.4e-16            2.0e-16  2.0e-16   0.27
  ensemble           sixpriors               gauss_iso       3            2.8e-16  2.8e-16            1.1e-16  1.1e-16   0.68 .. 0.74
  ensemble           linreg                  linreg          3            1.1e-16  1.1e-16            2.1e-16  2.1e-16   0.84 .. 0.85
  ensemble           linmodel3               linmodel3       3            1.0e-15  1.0e-15            2.5e-16  2.5e-16   0.75 .. 0.79

The segments and two_chunk_segments rows completed their stage inside one segment with no stall ([1, 1], stalls [0, 0, 0, 0]); no path refused a
spec.  The device agrees with the oracle to the last figure printed nearly everywhere: the formulas are the same FP64 expressions, and what the
reference adds is that both are right - which, at the family edges, they were not: the parent's oracle (measured on the CPU; the device's expressions were the same, not measured)
returns NaN at Gamma(1, 2) and Beta(1, .) at 0, Beta(., 1) at 1 and RootInverseGamma at 1e-170 / 1e-162, and -Inf for RootInverseGamma at 1e155.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import target_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEFT_OUT_SHARE = tr.MAX_LEFT_OUT / tr.N_CLASS
SEED, MUT_PHI, MUT_STAGE = 23, 0.3, 3
SCORE_N = (200, 300)
SHAPE_DECADES = (-45, -20, 0, 20, 45)       # the prior-shapes clouds of the mutation vehicle: one decade each (the determinant of the cloud's 6 x 6 covariance, 10^(6 E), must stay a normal number)
C_GRID = [10.0 ** (-0.5 * k) for k in range(-4, 31)]          # the scales oracle.mutate_cloud is tried at, largest first


# ------------------------------------------------------------------------------------------------ worker side
def oracle_columns(spec, theta, old=False):
    """(loglh, logprior[, old_loglh]) of the FP64 oracle on the rows of theta, bounds rule included (orc_initialize_likelihoods)"""
    from oracle import oracle as orc
    from tests import models

    d = theta.shape[1]
    P = np.zeros((len(theta), d + 5), order="F")
    P[:, :d], P[:, d + 4] = theta, 1.0
    Q = orc.initialize_likelihoods(models.oracle_model(spec), P)
    if not old:
        return Q[:, d].copy(), Q[:, d + 1].copy()
    if spec.get("old_lik") is None:
        return Q[:, d].copy(), Q[:, d + 1].copy(), np.zeros(len(theta))
    Qo = orc.initialize_likelihoods(models.oracle_model(dict(spec, lik=spec["old_lik"], old_lik=None)), P)
    return Q[:, d].copy(), Q[:, d + 1].copy(), Qo[:, d].copy()


def _summary(got, ref, S, orc_v):
    """one line of figures: the oracle's and the device's worst normalised error over the included rows, what is left out, what is not finite"""
    got = np.asarray(got, dtype=np.float64)
    ref64 = tr.f64(ref)
    orc_err = tr.nerr(orc_v, ref, S)
    inc, b, orc_worst = tr.bar(orc_err)
    err = tr.nerr(got, ref, S)
    fin = np.isfinite(ref64)
    worst = int(np.argmax(np.where(inc, err, -1.0)))
    return dict(n=int(len(got)), left_out=int((~inc).sum()), orc_worst=orc_worst, bar=b, dev_worst=float(err[inc].max()) if inc.any() else 0.0, worst_row=worst,
                n_nan=int(np.isnan(got).sum()), n_not_finite=int((~np.isfinite(got[fin])).sum()), n_inf=int((~fin).sum()),
                inf_same=bool(np.array_equal(got[~fin], ref64[~fin])), got_worst=float(got[worst]) if np.isfinite(got[worst]) else str(got[worst]),
                ref_worst=float(ref64[worst]) if np.isfinite(ref64[worst]) else str(ref64[worst]))


def _cloud(theta, loglh=None):
    d = theta.shape[1]
    P = np.zeros((theta.shape[0], d + 5), order="F")
    P[:, :d], P[:, d + 4] = theta, 1.0
    if loglh is not None:
        P[:, d] = loglh
    return P


_ENGINES = {}


def _engine(n, d, seed=SEED, fresh=False, **kw):
    """one handle per (n, d) and worker (set_model replaces the model); fresh: a handle of its own"""
    from smc_jl_amd import Engine

    if fresh:
        return Engine(n, d, seed=seed, max_stages=8, store_history=False, **kw)
    if (n, d, seed) not in _ENGINES:
        _ENGINES[(n, d, seed)] = Engine(n, d, seed=seed, max_stages=8, store_history=False)
    return _ENGINES[(n, d, seed)]


def _class_cases(name, n=tr.N_CLASS, **kw):
    if name == "det_quirk":
        return [tr.det_underflow_case(n)]
    if name == "nan_rows":
        return tr.nan_cases(n)
    return tr.cases(name, n, **kw)


def work_score(cfg):
    """every case of a class through initialize_likelihoods at n rows -> per case a summary of column d and of column d + 1"""
    name, n = cfg["name"], cfg["n"]
    out = []
    for c in _class_cases(name):
        d = c.theta.shape[1]
        th = np.ascontiguousarray(c.theta[np.arange(n) % tr.N_CLASS])
        T = tr.target(c.spec, c.theta)
        oll, olp = oracle_columns(c.spec, c.theta)
        rep = lambda v: np.asarray(v)[np.arange(n) % tr.N_CLASS]
        marker = -1.0 - 0.5 * np.arange(n)
        e = _engine(n, d)
        e.set_model(c.spec)
        e.upload_cloud(_cloud(th, marker))
        e.initialize_likelihoods()
        P = e.download_cloud()
        o = dict(label=c.label, lik=c.spec["lik"][0], priors=sorted({p[0] for k, p in enumerate(c.spec["priors"]) if not c.spec["fixed"][k]}), staged=list(tr.staged(c.spec)),
                 loglh=_summary(P[:, d], rep(T.ll), rep(T.ll_S), rep(oll)), logprior=_summary(P[:, d + 1], rep(T.lp), rep(T.lp_S), rep(olp)),
                 old_bits=bool(np.array_equal(P[:, d + 2], marker)), theta_kept=bool(np.array_equal(P[:, :d], th, equal_nan=True)),
                 lanes_agree=bool(all(np.array_equal(P[i::tr.N_CLASS, d:d + 2], np.broadcast_to(P[i, d:d + 2], P[i::tr.N_CLASS, d:d + 2].shape), equal_nan=True) for i in range(tr.N_CLASS))),
                 outside_neg_inf=bool(np.all(P[~rep(T.inb), d:d + 2] == -np.inf)), n_outside=int((~rep(T.inb)).sum()))
        if name == "det_quirk":                               # the quirk: the device's value is the oracle's, whatever the reference says
            o["same_as_oracle"] = bool(np.array_equal(P[:, d], rep(oll)))
        out.append(o)
    return out


BOX = {"sixpriors": [(-1.0, 2.0), (-2.0, 0.5), (0.5, 4.0), (0.2, 0.7), (0.4, 2.0), (0.3, 0.9)],
       "ten": [(-3.0, 3.0), (-0.5, 0.75), (0.05, 3.0), (0.1, 0.9), None, (0.4, 2.0), (0.3, 0.9), (0.5, 0.99), (-1.5, -0.5), (1.0, 3.0)]}


def draw_spec(name, boxed):
    """sixpriors / ten; boxed: the bounds narrowed onto a box (the draw then redraws until inside it)"""
    sp = getattr(tr, name)()
    if boxed:
        sp["bounds"] = [b if box is None else box for b, box in zip(sp["bounds"], BOX[name])]
    return sp


def work_draw(cfg):
    from oracle import oracle as orc
    from tests import models

    out = []
    for name in ("sixpriors", "ten"):
        for boxed in (False, True):
            sp = draw_spec(name, boxed)
            d, n = len(sp["priors"]), cfg["n"]
            e = _engine(n, d)
            e.set_model(sp)
            e.init_from_prior()
            P = e.download_cloud()
            Q = orc.initial_draw(models.oracle_model(sp), n, seed=SEED)
            th = np.ascontiguousarray(P[:, :d])
            T = tr.target(sp, th)
            oll, olp = oracle_columns(sp, th)
            out.append(dict(label="%s%s" % (name, " boxed" if boxed else ""), same_draws=bool(np.allclose(P, Q, rtol=1e-10, atol=1e-12)), inside=bool(T.inb.all()),
                            loglh=_summary(P[:, d], T.ll, T.ll_S, oll), logprior=_summary(P[:, d + 1], T.lp, T.lp_S, olp)))
    return out


def proposal(P, spec, n_blocks, stage=MUT_STAGE):
    """the cloud's own weighted moments over the free parameters and the oracle's blocks"""
    from oracle import oracle as orc
    from tests import models

    m = models.oracle_model(spec)
    fr = m.free_inds
    mean, cov = orc.weighted_mean(P), orc.weighted_cov(P)
    bf, ba, bp = orc.generate_blocks(len(fr), n_blocks, fr, SEED, stage)
    cov = (cov + cov.T) / 2.0
    return m, mean[fr], cov[np.ix_(fr, fr)], bf, ba, bp


def work_propose(cfg):
    out = []
    n = cfg["n"]
    for name in ("sixpriors", "ten", "wide12"):
        sp = getattr(tr, name)()
        d = len(sp["priors"])
        e = _engine(n, d)
        e.set_model(sp)
        e.upload_cloud(_cloud(tr.prior_draws(sp, n, tr._seed("propose", name))))
        e.initialize_likelihoods()
        P0 = e.download_cloud()
        for nb, alpha, c in ((1, 1.0, 0.5), (3, 0.9, 2.0)):
            m, mean, cov, bf, ba, bp = proposal(P0, sp, nb)
            for blk in range(nb):
                prop, lpr, _ = e.propose(mean, cov, bp, bf, blk, 0, c, alpha, MUT_STAGE)
                th = np.ascontiguousarray(prop)
                T = tr.target(sp, th)
                _, olp = oracle_columns(sp, th)
                o = dict(label="%s n_blocks=%d block=%d alpha=%g c=%g" % (name, nb, blk, alpha, c), logprior=_summary(lpr, T.lp, T.lp_S, olp), n_outside=int((~T.inb).sum()),
                         outside_neg_inf=bool(np.all(lpr[~T.inb] == -np.inf)), n_prior_neg_inf_inside=int((T.inb & (tr.f64(T.lp) == -np.inf)).sum()),
                         moved_only_block=bool(np.all(np.delete(prop, ba[bp[blk]:bp[blk + 1]], axis=1) == np.delete(P0[:, :d], ba[bp[blk]:bp[blk + 1]], axis=1))))
                out.append(o)
    return out


def mutation_spec(label):
    if label in ("sixpriors", "ten", "wide12"):
        return getattr(tr, label)()
    if label.startswith("shapes"):
        return tr.shapes_spec(int(label.split()[1]))
    both = dict(tr.base_specs())
    both.update({k: v[0] for k, v in tr.two_vintage_specs().items()})
    return both[label]


def mutation_cloud(label, cls, spec, n):
    """n θ of the class for the spec: prior draws; the far class's clouds (inset: a proposal can stay inside the bounds); the prior-shapes
    class's; for the nine-parameter likelihoods and linreg a cloud around the least-squares fit (the prior draws of N(0, 1e3) leave the MH ratio
    no chance at any scale)"""
    if cls == "far":
        return [c for c in tr.cases("far", n, inset=True) if c.label == label][0].theta
    if cls == "prior_shapes":
        return tr.cases("prior_shapes", n, decades=SHAPE_DECADES)[int(label.split()[1])].theta
    th = tr.prior_draws(spec, n, tr._seed("mut", label))
    rng = np.random.default_rng(tr._seed("mutfit", label))
    fam = spec["lik"][0]
    if fam == "linreg":
        th = np.column_stack([rng.normal(1.0, 0.5, n), rng.normal(2.0, 0.5, n)])
    elif fam in ("linmodel3", "capm_literal"):
        for i in range(3):
            th[:, 3 * i], th[:, 3 * i + 1], th[:, 3 * i + 2] = rng.normal(0.0, 0.5, n), rng.normal(0.0, 0.5, n), rng.uniform(0.5, 2.0, n)
    return th


def posterior_cloud(spec, n, seed):
    """linmodel3: n θ around the per-equation least-squares fit at the posterior's own spread - a cloud whose weights survive ϕ: 0 -> 1 in one
    stage (the ensemble's shortest schedule)"""
    Y, X = np.asarray(spec["lik"][2]), np.asarray(spec["lik"][3])
    T = Y.shape[1]
    rng = np.random.default_rng(seed)
    th = np.empty((n, 9))
    for i in range(3):
        a, b = tr._ols(Y[i], X[i, :T])
        sd = float(np.std(Y[i] - a - b * X[i, :T]))
        th[:, 3 * i], th[:, 3 * i + 1] = a + sd / np.sqrt(T) * rng.standard_normal(n), b + sd / np.sqrt(T) * rng.standard_normal(n)
        th[:, 3 * i + 2] = sd * (1.0 + rng.standard_normal(n) / np.sqrt(2.0 * T))
    return th


def choose_c(m, P0, mean, cov, bf, ba, bp, alpha, n_mh, lo=0.25, hi=0.75):
    """the largest scale of C_GRID at which oracle.mutate_cloud (CPU) moves between lo and hi of the rows; else the one nearest to a half"""
    from oracle import oracle as orc

    d = P0.shape[1] - 5
    best = None
    for c in C_GRID:
        Q = orc.mutate_cloud(m, P0, mean, cov, bf, ba, bp, MUT_PHI, 0.0, c, alpha, n_mh, SEED, MUT_STAGE)
        share = float(np.any(Q[:, :d] != P0[:, :d], axis=1).mean())
        if lo <= share <= hi:
            return c, share
        if best is None or abs(share - 0.5) < abs(best[1] - 0.5):
            best = (c, share)
    return best


def _rows_check(sp, P0, P1):
    """every row of the cloud P1 against the reference at that row's θ: the three columns, the bounds, nothing finite lost"""
    d = P1.shape[1] - 5
    th1 = np.ascontiguousarray(P1[:, :d])
    T = tr.target(sp, th1)
    oll, olp, oold = oracle_columns(sp, th1, old=True)
    o = dict(inside=bool(T.inb.all()), loglh=_summary(P1[:, d], T.ll, T.ll_S, oll), logprior=_summary(P1[:, d + 1], T.lp, T.lp_S, olp))
    if sp.get("old_lik") is None:
        o["old_zero"] = bool(np.all(P1[:, d + 2] == 0.0))
    else:
        o["old"] = _summary(P1[:, d + 2], T.old, T.old_S, oold)
    if P0 is not None:
        moved = np.any(th1 != P0[:, :d], axis=1)
        o["moved"] = float(moved.mean())
        started = np.isfinite(P0[:, d]) & np.isfinite(P0[:, d + 1])
        o["finite_lost"] = int((started & ~(np.isfinite(P1[:, d]) & np.isfinite(P1[:, d + 1]))).sum())
        o["stayed_bits"] = bool(np.array_equal(P1[~moved, d:d + 3], P0[~moved, d:d + 3]))
    return o


def work_mutation(cfg):
    out = []
    n = cfg["n"]
    for label, cls, nb, alpha, n_mh in cfg["cases"]:
        sp = mutation_spec(label)
        d = len(sp["priors"])
        th = mutation_cloud(label, cls, sp, n)
        e = _engine(n, d)
        if sp.get("old_lik") is not None:
            e.set_model(dict(sp, lik=sp["old_lik"], old_lik=None))
            e.upload_cloud(_cloud(th))
            e.initialize_likelihoods()                        # column d: the old vintage's log-likelihoods
            e.set_model(sp)
            e.initialize_likelihoods()                        # column d + 2 <- column d, column d: the new data's
        else:
            e.set_model(sp)
            e.upload_cloud(_cloud(th))
            e.initialize_likelihoods()
            P = e.download_cloud()
            P[:, d + 2] = 0.0
            e.upload_cloud(P)
        P0 = e.download_cloud()
        nb = min(nb, len([f for f in sp["fixed"] if not f]))
        m, mean, cov, bf, ba, bp = proposal(P0, sp, nb)
        c, share = choose_c(m, P0, mean, cov, bf, ba, bp, alpha, n_mh)
        acc = e.mutate(mean, cov, bp, bf, MUT_PHI, 0.0, c, alpha, n_mh, MUT_STAGE)
        P1 = e.download_cloud()
        o = dict(case=[label, cls, nb, alpha, n_mh], c=c, oracle_share=share, accept=float(acc), lik=sp["lik"][0], staged=list(tr.staged(sp)), d=d,
                 priors=sorted({p[0] for k, p in enumerate(sp["priors"]) if not sp["fixed"][k]}))
        o.update(_rows_check(sp, P0, P1))
        out.append(o)
    return out


def stage_spec(label):
    return dict(sixpriors=tr.sixpriors, ten=tr.ten, wide12=tr.wide12, linreg=lambda: tr.linreg(100), linmodel3=lambda: tr.linmodel3(100), capm=lambda: tr.capm(36))[label]()


STAGE_KW = dict(use_fixed_schedule=True, n_phi=100, lam=2.0, n_blocks=1, c=0.3)


def work_stage(cfg):
    """stage 2 on an uploaded cloud (the fresh vehicle) through one engine path, every row afterwards against the reference"""
    from smc_jl_amd import Engine
    from smc_jl_amd.host import engine as eng
    from smc_jl_amd.host._lib import SMCMIError

    out = []
    n, shards = cfg.get("n", 20480), cfg.get("shards", 1)
    for label in cfg["specs"]:
        sp = stage_spec(label)
        d = len(sp["priors"])
        o = dict(label=label, error="", lik=sp["lik"][0], d=d, n=n)
        out.append(o)
        es = []
        try:
            for r in range(shards):
                e = Engine(n, d, seed=SEED, max_stages=STAGE_KW["n_phi"], store_history=True, n_local=n // shards, gid0=r * (n // shards))
                e.set_model(sp)
                es.append(e)
            P = _cloud(mutation_cloud(label, "prior_like", sp, n))
            for r, e in enumerate(es):
                e.upload_cloud(np.asfortranarray(P[r * (n // shards):(r + 1) * (n // shards)]))
                e.initialize_likelihoods()
            P0 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            P0[:, d + 2] = 0.0
            for r, e in enumerate(es):
                e.upload_cloud(np.asfortranarray(P0[r * (n // shards):(r + 1) * (n // shards)]))
            r = eng.run_group(es, stop_after_stage=2, **STAGE_KW) if shards > 1 else es[0].run(stop_after_stage=2, **STAGE_KW)
            P1 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            rec = es[0].stage_records(r["n_stages"])
            o.update(n_stages=r["n_stages"], resampled=int(rec["resampled"][1]), accept=float(rec["accept_hist"][1]), fallback=r["shift_fallback_stage"],
                     segments=[r["n_segments"], r["segment_stages"]], stalls=[r["solver_stalls"], r["select_stalls"], r["spec_stalls"], r["segment_timeouts"]])
            # a stage that resampled permutes the rows: the moved share is the share of rows whose θ is no row of the uploaded cloud
            keys = {P0[i, :d].tobytes() for i in range(n)}
            o.update(_rows_check(sp, None, P1))
            o["moved"] = float(np.mean([P1[i, :d].tobytes() not in keys for i in range(n)]))
        except SMCMIError as ex:
            o["error"], o["code"] = str(ex)[:300], int(ex.code)
        finally:
            for e in es:
                e.close()
    return out


ENS_KW = dict(use_fixed_schedule=True, n_phi=2, lam=1.0, n_blocks=1, c=0.3)      # the shortest fixed schedule: stage 2 alone (ϕ: 0 -> 1)


def work_ensemble(cfg):
    from smc_jl_amd import Engine, run_ensemble
    from smc_jl_amd.host._lib import SMCMIError

    out = []
    n = cfg["n"]
    for label in cfg["specs"]:                                  # one launch per spec, its members on different seeds and clouds
        sp = stage_spec(label)
        d = len(sp["priors"])
        es, P0s = [], []
        try:
            for m in range(cfg["members"]):
                e = Engine(n, d, seed=SEED + m, max_stages=8, store_history=True)
                e.set_model(sp)
                th = posterior_cloud(sp, n, SEED + m) if label == "linmodel3" else mutation_cloud(label + " member %d" % m if m else label, "prior_like", sp, n)
                e.upload_cloud(_cloud(th))
                e.initialize_likelihoods()
                P = e.download_cloud()
                P[:, d + 2] = 0.0
                e.upload_cloud(P)
                es.append(e)
                P0s.append(P)
            rs = run_ensemble(es, **ENS_KW)
            for m, (e, r) in enumerate(zip(es, rs)):
                P1 = e.download_cloud()
                o = dict(label="%s member %d" % (label, m), error="", lik=sp["lik"][0], d=d, status=[r["status"], r["call_status"]], n_stages=r["n_stages"])
                o.update(_rows_check(sp, None, P1))
                keys = {P0s[m][i, :d].tobytes() for i in range(n)}
                o["moved"] = float(np.mean([P1[i, :d].tobytes() not in keys for i in range(n)]))
                out.append(o)
        except SMCMIError as ex:
            out.append(dict(label=label, error=str(ex)[:300], code=int(ex.code), lik=sp["lik"][0], d=d))
        finally:
            for e in es:
                e.close()
    return out


def worker_main(kind, cfg):
    res = dict(score=work_score, draw=work_draw, propose=work_propose, mutation=work_mutation, stage=work_stage, ensemble=work_ensemble)[kind](json.loads(cfg))
    print("RESULT " + json.dumps(res))


# ------------------------------------------------------------------------------------------------ test side
_CHILD = "import sys; sys.path.insert(0, %r); from tests import test_gpu_target_range as T; T.worker_main(%r, %r)"
SMCMI_ERR_ARG = -1            # include/smcmi.h: what the router answers a spec it does not serve with; any other error fails the test
# What ran, for test_everything_was_exercised.  The likelihood and prior families are the specs' own.  The staged pairs are tr.staged's
# restatement of stage_lik's rule on the host and the kernels "k_mutate_reg" (n_para <= 10) / "generic body" are read from smcmi.hip
# use_reg_mutate - neither is reported by the device: the record says which INPUTS were run, not which instructions.
EXERCISED = dict(lik=set(), priors=set(), staged=set(), paths=set(), vehicles=set())


def _spawn(kind, cfg, env_extra=None, timeout=300):
    env = dict(os.environ)
    env.update(env_extra or {})
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, kind, json.dumps(cfg))], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired as ex:                  # a hang: nothing more is started on that GPU by this file either
        pytest.exit("a worker of tests/test_gpu_target_range.py (%s) did not end within %d s:\n%s" % (kind, timeout, (ex.stderr or "")[-3000:]), returncode=3)
    # the worker died of a signal or met a GPU fault: nothing more is started on that GPU by this file
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:
        pytest.exit("a worker of tests/test_gpu_target_range.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _check_summary(s, why, what):
    """Every figure was printed before this is called."""
    if s["left_out"] > MAX_LEFT_OUT_SHARE * s["n"]:
        why.append("%s: %d of %d rows left out" % (what, s["left_out"], s["n"]))
    if s["n_nan"]:
        why.append("%s: %d NaN" % (what, s["n_nan"]))
    if s["n_not_finite"]:
        why.append("%s: %d values not finite where the reference is" % (what, s["n_not_finite"]))
    if not s["inf_same"]:
        why.append("%s: another value where the reference is ±Inf (%d rows)" % (what, s["n_inf"]))
    if not s["dev_worst"] <= s["bar"]:
        why.append("%s: off by %.3g (bar %.3g, oracle %.3g) at row %d: %r against %r" % (what, s["dev_worst"], s["bar"], s["orc_worst"], s["worst_row"], s["got_worst"], s["ref_worst"]))


def _note(o):
    EXERCISED["lik"].add(o.get("lik"))
    EXERCISED["priors"].update(o.get("priors", ()))
    if "staged" in o:
        EXERCISED["staged"].add((o["lik"], tuple(o["staged"])))


@pytest.mark.parametrize("n", SCORE_N)
@pytest.mark.parametrize("name", list(tr.CLASSES))
def test_scoring_an_uploaded_cloud(name, n):
    res = _spawn("score", dict(name=name, n=n))
    for o in res:
        print(name, n, json.dumps(o))
    why = []
    for o in res:
        what = "%s, %s" % (name, o["label"])
        _check_summary(o["loglh"], why, what + " loglh")
        _check_summary(o["logprior"], why, what + " logprior")
        for key, msg in (("old_bits", "column d + 2 is not the bits of the uploaded loglh"), ("theta_kept", "the parameters changed"), ("lanes_agree", "the same θ gives other bits in another lane"),
                         ("outside_neg_inf", "a θ outside the bounds does not hold -Inf in columns d and d + 1")):
            if not o[key]:
                why.append("%s: %s" % (what, msg))
        _note(o)
    if name == "corners":
        assert all(o["n_outside"] >= n // 2 - 1 for o in res), "the corners class has no row beyond a bound"
    EXERCISED["vehicles"].add("score")
    assert len(res) == len(tr.cases(name)) and not why, "\n".join(why)


@pytest.mark.parametrize("n", SCORE_N)
def test_nan_parameters_score_as_outside_the_bounds(n):
    """in_bounds holds NaN outside only because both comparisons of the closed interval are false: a NaN in one free parameter, in the fixed
    parameter and in every parameter gives -Inf in columns d and d + 1 - in every lane the row is scored in; the control rows are the reference's."""
    res = _spawn("score", dict(name="nan_rows", n=n))
    why = []
    for o in res:
        print(n, json.dumps(o))
        what = "nan rows, %s" % o["label"]
        _check_summary(o["loglh"], why, what + " loglh")
        _check_summary(o["logprior"], why, what + " logprior")
        if o["n_outside"] != sum(1 for i in range(n) if (i % tr.N_CLASS) % 4 != 0) or o["loglh"]["n_inf"] != o["n_outside"] or o["logprior"]["n_inf"] != o["n_outside"]:
            why.append("%s: %d rows outside, %d / %d infinities in the reference" % (what, o["n_outside"], o["loglh"]["n_inf"], o["logprior"]["n_inf"]))
        for key, msg in (("outside_neg_inf", "a NaN θ does not hold -Inf in columns d and d + 1"), ("lanes_agree", "the same θ gives other bits in another lane"),
                         ("theta_kept", "the parameters changed"), ("old_bits", "column d + 2 is not the bits of the uploaded loglh")):
            if not o[key]:
                why.append("%s: %s" % (what, msg))
    assert len(res) == len(tr.nan_cases()) and not why, "\n".join(why)


def test_the_det_quirk_is_the_oracle_s():
    """σ products below 1e-154 / above 1e154 (outside the shipped bounds): det = Π σ_i² underflows / overflows before its log and the value is
    +Inf / -Inf where the reference is finite - on the device as in the oracle, the same infinity row by row.  Inside the shipped bounds nothing
    finite turns infinite: the far class above puts every σ on 1e-5 and on 1e5."""
    res = _spawn("score", dict(name="det_quirk", n=200))
    for o in res:
        print(json.dumps(o))
    o = res[0]
    assert o["same_as_oracle"] and o["lanes_agree"] and o["loglh"]["n_nan"] == 0 and o["loglh"]["n_not_finite"] == 200, o
    why = []
    _check_summary(o["logprior"], why, "logprior")
    assert not why, "\n".join(why)


def test_the_prior_draw():
    res = _spawn("draw", dict(n=1000))
    why = []
    for o in res:
        print(json.dumps(o))
        _check_summary(o["loglh"], why, o["label"] + " loglh")
        _check_summary(o["logprior"], why, o["label"] + " logprior")
        if not o["same_draws"]:
            why.append("%s: the cloud is not the oracle's draw" % o["label"])
        if not o["inside"]:
            why.append("%s: a draw outside the bounds" % o["label"])
    EXERCISED["vehicles"].add("draw")
    assert len(res) == 4 and not why, "\n".join(why)


def test_proposals_of_the_closure_path():
    res = _spawn("propose", dict(n=300))
    why = []
    for o in res:
        print(json.dumps(o))
        _check_summary(o["logprior"], why, o["label"])
        if not o["outside_neg_inf"]:
            why.append("%s: a proposal outside the bounds without -Inf" % o["label"])
        if not o["moved_only_block"]:
            why.append("%s: a parameter outside the block changed" % o["label"])
    # the inputs hold: some proposals leave the bounds, and on `ten` some leave the narrow Uniform prior inside the bounds
    assert sum(o["n_outside"] for o in res) > 0 and sum(o["n_prior_neg_inf_inside"] for o in res if o["label"].startswith("ten")) > 0
    EXERCISED["vehicles"].add("propose")
    assert len(res) == 3 * 4 and not why, "\n".join(why)


COMBOS = [(1, 1.0, 1), (3, 0.9, 1), (1, 0.9, 2), (3, 1.0, 2)]          # (n_blocks, α, n_mh_steps)
MUT_GROUPS = {
    "prior_like d<=10": [(lab, "prior_like") + cb for lab in ("sixpriors", "ten", "linreg n=100 s2=1", "linmodel3 T=100", "capm T=36 aux_rows=2") for cb in COMBOS],
    "prior_like wide12": [("wide12", "prior_like") + cb for cb in COMBOS],
    "far": [(lab, "far") + cb for lab in ("sixpriors", "ten", "wide12", "linreg n=100 s2=1", "linmodel3 T=129", "capm T=129") for cb in COMBOS[:2]],
    "prior_shapes": [("shapes %d" % j, "prior_shapes") + COMBOS[j % 4] for j in range(5)] + [("shapes 1", "prior_shapes") + COMBOS[0]],
    "two vintages linmodel3": [(lab, "prior_like") + COMBOS[i % 4] for i, lab in enumerate(k for k in tr.two_vintage_specs() if k.startswith("linmodel3"))],
    "two vintages linreg": [(lab, "prior_like") + COMBOS[i % 4] for i, lab in enumerate(k for k in tr.two_vintage_specs() if k.startswith("linreg"))],
}


def _check_rows(o, why, what, moved_lo=0.1, moved_hi=0.9):
    if not moved_lo <= o["moved"] <= moved_hi:
        why.append("%s: %.3g of the rows moved - the input does not hold" % (what, o["moved"]))
    if not o["inside"]:
        why.append("%s: a row outside the bounds" % what)
    if o.get("finite_lost"):
        why.append("%s: %d rows that started finite hold -Inf or NaN" % (what, o["finite_lost"]))
    if not o.get("stayed_bits", True):
        why.append("%s: a row that did not move changed one of its three columns" % what)
    if not o.get("old_zero", True):
        why.append("%s: old_loglh is not 0 without an old vintage" % what)
    for col in ("loglh", "logprior", "old"):
        if col in o:
            _check_summary(o[col], why, "%s %s" % (what, col))


@pytest.mark.parametrize("group", list(MUT_GROUPS))
def test_rows_stay_consistent_through_a_mutation(group):
    res = _spawn("mutation", dict(n=300, cases=MUT_GROUPS[group]))
    why = []
    for o in res:
        print(group, json.dumps(o))
    for o in res:
        _check_rows(o, why, "%r" % (o["case"],))
        _note(o)
        EXERCISED["paths"].add("k_mutate_reg" if o["d"] <= 10 else "generic body")
    EXERCISED["vehicles"].add("mutation")
    assert len(res) == len(MUT_GROUPS[group]) and not why, "\n".join(why)


def _paths():
    from tests.test_gpu_weight_range import PATHS

    return PATHS


STAGE_SPECS = {"segments": ["sixpriors", "ten", "linmodel3", "capm"], "launches": ["sixpriors", "linmodel3", "capm"], "engine1": ["ten", "linmodel3", "capm"],
               "large_shard_stage": ["sixpriors", "linmodel3", "capm"], "two_shards": ["ten", "linmodel3", "capm"], "two_chunk_segments": ["sixpriors", "linreg"], "wide": ["wide12"]}


@pytest.mark.parametrize("path", list(STAGE_SPECS))
def test_one_bracketed_stage_per_engine_path(path):
    env, over, seg = _paths()[path]
    cfg = dict(specs=STAGE_SPECS[path], n=over.get("n", 20480), shards=over.get("shards", 1))
    res = _spawn("stage", cfg, env, timeout=600)
    why, ran = [], 0
    for o in res:
        print(path, json.dumps(o))
    for o in res:
        what = "%s %s" % (path, o["label"])
        if o["error"]:                                        # the router refuses the pair: recorded, not a failure (a crash or a silent fallback is)
            print("%s: refused: %s" % (what, o["error"]))
            if o.get("code") != SMCMI_ERR_ARG:
                why.append("%s: %s" % (what, o["error"]))
            continue
        ran += 1
        _check_rows(o, why, what, moved_hi=1.0)
        if o["n_stages"] != 2:
            why.append("%s: %d stages" % (what, o["n_stages"]))
        if seg and not (o["segments"][1] >= seg and o["stalls"] == [0, 0, 0, 0] and o["fallback"] == 0):
            why.append("%s: the stage did not (provably) complete inside a segment: segments %r stalls %r fallback %r" % (what, o["segments"], o["stalls"], o["fallback"]))
        if seg is False and o["segments"][0] != 0:
            why.append("%s: the bracket ran segments: %r" % (what, o["segments"]))
        _note(o)
    EXERCISED["paths"].add(path)
    EXERCISED["vehicles"].add("stage")
    assert ran >= 1 and not why, "\n".join(why)


def test_the_ensemble_kernel():
    res = _spawn("ensemble", dict(n=1024, members=3, specs=["sixpriors", "linreg", "linmodel3"]), timeout=600)
    why, ran = [], set()
    for o in res:
        print(json.dumps(o))
    for o in res:
        if o["error"]:
            print("%s: refused: %s" % (o["label"], o["error"]))
            if o.get("code") != SMCMI_ERR_ARG:
                why.append("%s: %s" % (o["label"], o["error"]))
            continue
        ran.add(o["lik"])
        _check_rows(o, why, o["label"], moved_lo=0.0, moved_hi=1.0)
        if o["status"] != [0, 0] or o["n_stages"] != 2:
            why.append("%s: status %r, %d stages" % (o["label"], o["status"], o["n_stages"]))
        _note(o)
    EXERCISED["paths"].add("ensemble")
    EXERCISED["vehicles"].add("ensemble")
    assert {"gauss_iso", "linreg"} <= ran and not why, "\n".join(why)


def test_everything_was_exercised():
    """What the cases above cover, from their tables - and, when the whole file ran in this process, from what the workers reported."""
    liks = {c.spec["lik"][0] for name in tr.CLASSES for c in tr.cases(name)}
    pris = {p[0] for name in tr.CLASSES for c in tr.cases(name) for p in c.spec["priors"]}
    assert liks == {"gauss_iso", "linreg", "linmodel3", "capm_literal"} and pris == {"normal", "uniform", "gamma", "beta", "invgamma", "rootinvgamma"}
    two = [(mutation_spec(c[0])["lik"][0], tr.staged(mutation_spec(c[0]))) for g in MUT_GROUPS.values() for c in g]
    for fam in ("linreg", "linmodel3"):
        assert {(True, True), (True, False), (False, False), (True, None), (False, None)} <= {st for f, st in two + [(c.spec["lik"][0], tr.staged(c.spec)) for c in tr.cases("prior_like")] if f == fam}, fam
    assert set(STAGE_SPECS) == {"segments", "launches", "engine1", "large_shard_stage", "two_shards", "two_chunk_segments", "wide"} <= set(_paths())
    if EXERCISED["vehicles"] >= {"score", "draw", "propose", "mutation", "stage", "ensemble"}:
        assert EXERCISED["lik"] >= liks and EXERCISED["priors"] >= pris, EXERCISED
        for fam in ("linreg", "linmodel3"):
            assert {(fam, st) for st in ((True, True), (True, False), (False, False), (True, None), (False, None))} <= EXERCISED["staged"], EXERCISED["staged"]
        assert EXERCISED["paths"] >= set(STAGE_SPECS) | {"k_mutate_reg", "generic body", "ensemble"}, EXERCISED["paths"]
