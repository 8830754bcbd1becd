"""The Metropolis-Hastings move as the device makes it - Philox coordinates, Box-Muller normals, mixture draw, proposal densities, decision, accept
column, acceptance rate - against the step-by-step exact reference of tests/mutation_ref.py (pinned by tests/test_mutation_ref_cpu.py), vehicle by
vehicle.  Every test is one child process with its own time limit; a child that dies or times out ends the session.  The restatement's errors (the
yardsticks: tests/test_mutation_ref_cpu.py restatement_yardsticks) are computed in the worker, on the CPU, before the device's values are looked at.

Bars.  θ': |Δ_k| <= max(1e-13, 16 x the restatement's worst error on the class) s_k.  log q0 - log q1, log η and the proposal's log-prior: the same
rule in units of max(1, S).  A decision is undecided only when |log u - log η| <= max(1e-12, 16 x the restatement's worst |Δ log η| on the class)
max(1, S_η); a proposal is in the band as tests/mutation_ref.py defines it; a particle is dropped from the rest of a call after either.  Undecided,
band and dropped decisions together: at most 1e-3 of a case's.  Everything else - uniforms (through the normals, which are the proposal bit for bit
at θ = 0, Σ = I, c = 1, α = 1), components, bounds verdicts, decisions, accept columns, NaN and ±Inf outcomes - without tolerance.  Normals: within
3 ulp of the exact normal (csrc/bmmath.hpp's figure).

Vehicles:
  normals, propose   Engine.propose (k_mutate<1>, the generic body), d 1 .. 64, n = 2 368 on a handle whose ids straddle 2^32 (gid0 = 2^32 - 1 184;
                     smcmi_create takes n_parts = 2^33 with a small n_local), n = 1 and 63, stages 1, 299, 2^32 - 1, t = 0 .. 29, and n = 1 handles on
                     the ids a search of the reference over 2^26 ids finds for the smallest ua, the ua nearest 1 and the ub nearest k / 4
  normals, mutate    Engine.mutate on a flat target (every proposal accepted: the accept column is 1), k_mutate_reg, d 1, 2, 3, 9, 10, one MH step (a
                     second would add two normals: not the bits any more), every parameter a block of its own: t = 0 .. d - 1
  densities          debug_proposal_densities (k_debug_mix_densities: the dense mixture form) on the reference's own moves of every class whose
                     block is the whole vector (d <= 10), and on points no draw reaches: the move stretched 3, 10 and 40 times
  closure            Engine.propose / Engine.accept per (step, block) of every case: θ', log-prior, q0 - q1, then - fed the reference's
                     log-likelihoods rounded to FP64 - the decision (MODE 1 and MODE 2 of the generic body; d <= 10, 12 and 20)
  mutate             Engine.mutate on every case: k_mutate_reg at α = 1 and α < 1, k_mutate<0> at d = 12 and 20; the accept column of every row that
                     was not dropped is the reference's, a moved row's θ the reference's to the bar, the returned rate the mean of the column
  stages             stage 2 on an uploaded cloud through every engine path (the PATHS rows of tests/test_gpu_weight_range.py at their sizes: 20 480
                     rows, two_chunk_segments 150 004 and one case only), at α = 1 and α = 0.9 (inside segments: with parked normals), on a stage
                     that does not resample and one that does (threshold ratios 0 and 1; the ancestors are the restatement's).  The reference
                     starts from the uploaded cloud with ϕ and c from the stage records, the moments of Engine.stage_moments() and its own
                     block; which kernels ran is asserted as that file's _check does (segments: the stage completed inside one, no stall, no
                     fallback; launches / engine 1 / large shards: no segment); then stage 3's c_hist entry against the exact factor of the
                     exact acceptance rate (rtol 1e-14)
  ensemble           whole runs of the shortest fixed schedule (ϕ: 0 -> 1) in one launch of kens_run, three members of n = 1 024 on sixpriors,
                     linreg and linmodel3, each member as a stage above

Measured on an MI355X (n = 300 rows per case; rst: the restatement on the same inputs; normalised errors as above).  No decision is undecided, in a
band or dropped in any case (0 of 43 500 per vehicle); no flip and no wrong accept column anywhere.

  normals           vehicle                      normals   worst ulp   correctly rounded
                    propose (generic body)       908 096        2.49   64.2 %
                    propose, searched ids             14        0.74   (ua = 5.5e-11 and 1 - 4.3e-8, ub within 2.7e-8 of every k / 4)
                    mutate (k_mutate_reg)         60 352        2.11   64.0 %
  densities         class            points   left out   rst      device
                    benign               96          0   3.3e-16  2.5e-16
                    ill_conditioned     192          0   1.6e-09  1.6e-09
                    far                 192          0   0        0
                    mu_far              288          1   2.9e-16  2.5e-16
                    density_scale     1 632         28   1.2e-14  1.2e-14
                    alpha             1 728         13   8.6e-16  1.4e-15
                    tight_bounds        192          0   0        0
                    phi                 576          5   5.6e-16  7.9e-16
  closure, mutate   class           decisions   θ': rst  propose  mutate    q0 - q1: rst  propose   log-prior   flips   columns wrong (mutate)
                    benign              4 500   4.2e-15  4.4e-16  3.0e-16        9.1e-16  4.8e-16     1.2e-14       0   0
                    ill_conditioned     2 400   1.3e-11  1.3e-11  1.3e-11        1.2e-10  1.2e-10     2.4e-16       0   0
                    far                 2 400   1.1e-16  1.1e-16  1.1e-16        5.3e-14  5.3e-14     1.2e-16       0   0
                    mu_far              1 200   2.8e-14  3.6e-16  3.6e-16        0        0           3.0e-16       0   0
                    density_scale       5 100   2.3e-14  3.6e-16  3.4e-16        1.3e-16  1.3e-16     3.9e-16       0   0
                    alpha               5 400   8.9e-14  4.4e-16  3.6e-16        1.1e-15  1.1e-15     1.1e-15       0   0
                    tight_bounds        2 100   2.8e-15  4.4e-16  4.4e-16        4.2e-16  3.4e-16     4.2e-16       0   0
                    dead_rows           1 800   3.0e-15  3.4e-16  3.3e-16        2.4e-16  2.4e-16     2.2e-15       0   0
                    phi                 1 800   2.4e-16  2.0e-16  2.0e-16        9.0e-16  4.7e-16     2.2e-16       0   0
                    blocks             16 800   1.2e-14  1.3e-15  8.3e-16        9.4e-16  9.4e-16     1.2e-13       0   0
  stages, ensemble  path                 cases  decisions  left out   θ': rst  device   columns wrong   next c off by   kernels
                    segments                 4     81 920         0   1.2e-14  4.5e-16              0         5.5e-17   1 segment, 1 stage in it, no stall
                    launches                 4     81 920         0   1.2e-14  4.5e-16              0         5.5e-17   no segment
                    engine1                  4     81 920         0   1.2e-14  4.3e-16              0         5.5e-17   no segment
                    large_shard_stage        4     81 920         0   1.2e-14  4.5e-16              0         5.5e-17   no segment
                    two_shards               4     81 920         0   1.2e-14  4.5e-16              0         5.5e-17
                    two_chunk_segments       1    150 004         0   2.5e-14  3.9e-16              0         8.1e-18   1 segment, 1 stage in it, no stall
                    wide (d = 12)            4     81 920         0   4.5e-14  5.0e-16              0         1.5e-16   no segment
                    ensemble (kens_run)      9      9 216         0   3.8e-15  2.7e-16              0                   all members resampled
No path refused a pair; every stage's recorded acceptance rate is the mean of its column bit for bit; the restatement flips nothing.
The returned acceptance rate is the mean of the downloaded column to 1.4e-16 relative at worst (the bar: 300 x 2^-53 = 3.3e-14), and equals the
reference's exact rate to the same bar wherever no row was dropped (everywhere).  Components are also checked directly (no proposal is another
component's draw); the densities vehicle leaves out at most a quarter of a case's points and a twentieth of a class's (measured: 16 of 96, 28 of 1 632).

Found and fixed in csrc/kernels.hpp, both at the ends of the density-scale class:
  mh_step       the α = 1 shortcut of the register kernels tested the symmetric log-density against the underflow point of exp only.  Above the
                overflow point (709.78; c²Σ_b of about 1e-62 per parameter at d_b = 10) both densities are +Inf, the reference sets q0 = 0 and rejects
                with q0 - q1 = -Inf; the kernels accepted.  On the parent's library test_stand_alone_mutations[density_scale] shows it as 2, 120, 137
                and 123 wrong accept columns of 300 in the α = 1 cases s = 1e-31, 5e-32, 1e-33 and 1e-40.
  mix_densities the dense mixture form (the register kernels at α < 1, k_debug_mix_densities) formed the diagonal component as (Π 1 / (sd_i sqrt(2π)))
                exp(-Σ z_i² / 2) where the reference - and the generic body - interleaves quotient and exponential coordinate by coordinate.  The
                product of the quotients alone overflowed from Π sd_i sqrt(2π) < 1e-308 on (sd = 5e-32 at d_b = 10) although the reference's running
                product stays finite, and the exponential alone underflowed for moves longer than 38.6 unscaled standard deviations although the
                running product does not.  On the parent's library: test_dense_densities_at_chosen_points[density_scale] 52 of 1 632 values (NaN or
                ±Inf where the reference is finite, 0 where it is +Inf: s <= 5e-32 at both α, the moves stretched 10 and 40 times at α = 0.9), and
                test_stand_alone_mutations[density_scale] 8 wrong accept columns of 300 in `s=5e-32 alpha=0.9`.  mix_expand now leaves the ssq below
                which every intermediate of the running product is a normal number (there the one product is the running product up to rounding);
                at and beyond it mix_densities forms the product in the reference's order.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mutation_ref as mr
from tests import target_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ULP_BAR = 3.0
STRADDLE = (1 << 32) - 1184
N_PARTS = 1 << 33
SEARCH_IDS = 1 << 26
PROPOSE_D = (1, 2, 9, 10, 11, 13, 20, 40, 64)
MUTATE_D = (1, 2, 3, 9, 10)
STRETCH = (3.0, 10.0, 40.0)


# ------------------------------------------------------------------------------------------------ worker side
def _flat_spec(d):
    return mr.gspec(d, 0.0, 1e45, 1e30, -1e45, 1e45)


def _engine(n, d, seed, gid0=0):
    from smc_jl_amd import Engine

    return Engine(N_PARTS if gid0 else n, d, seed=seed, max_stages=4, store_history=False, n_local=n, gid0=gid0)


def _zero_cloud(n, d):
    P = np.zeros((n, d + 5), order="F")
    P[:, d + 4] = 1.0
    return P


def _normals_ref(seed, pid, stage, t, db):
    return mr.block_normals(mr.stream(seed, pid, stage, t, db), db)


def _ulp_fig(got, ref):
    u = mr.ulps(got, ref)
    k = int(np.argmax(u))
    return dict(worst=float(u.max()), over=int((u > ULP_BAR).sum()), n=int(u.size), exact=int((np.asarray(got) == tr.f64(ref)).sum()), at=[int(v) for v in np.unravel_index(k, u.shape)])


def work_normals_propose(cfg):
    out = []
    for d, n, stage, gid0, seed, ts in cfg["cases"]:
        sp = _flat_spec(d)
        e = _engine(n, d, seed, gid0)
        e.set_model(sp)
        e.upload_cloud(_zero_cloud(n, d))
        nb = min(3, d)
        bf, ba, bp = mr.generate_blocks(d, nb, list(range(d)), seed, stage)
        pid = np.arange(n, dtype=np.uint64) + np.uint64(gid0)
        fig = dict(worst=0.0, over=0, n=0, exact=0)
        rest_zero = True
        for t in ts:
            b, step = t % nb, t // nb
            pos = ba[bp[b]:bp[b + 1]]
            ref = _normals_ref(seed, pid, stage, t, len(pos))
            prop, _, qd = e.propose(np.zeros(d), np.eye(d), bp, bf, b, step, 1.0, 1.0, stage)
            f = _ulp_fig(prop[:, pos], ref)
            fig = dict(worst=max(fig["worst"], f["worst"]), over=fig["over"] + f["over"], n=fig["n"] + f["n"], exact=fig["exact"] + f["exact"])
            rest_zero &= bool(np.all(np.delete(prop, pos, axis=1) == 0.0)) and bool(np.all(qd == 0.0))
        e.close()
        out.append(dict(case=[d, n, stage, gid0, seed, len(ts)], rest_zero=rest_zero, **fig))
    return out


def work_normals_search(cfg):
    """n = 1 handles on the ids the reference's search finds (proposal 0 of a block of two: the pair of tag (0, 1))"""
    seed, stage = cfg["seed"], cfg["stage"]
    found = mr.search_ids(seed, stage, mr.rng_tag(mr.P_MUT, 0, 1), cfg["n_ids"])
    out = []
    for name, (pid, ua, ub) in found.items():
        e = _engine(1, 2, seed, pid)
        e.set_model(_flat_spec(2))
        e.upload_cloud(_zero_cloud(1, 2))
        prop, _, _ = e.propose(np.zeros(2), np.eye(2), [0, 2], [0, 1], 0, 0, 1.0, 1.0, stage)
        e.close()
        ref = _normals_ref(seed, np.array([pid], dtype=np.uint64), stage, 0, 2)
        out.append(dict(name=name, id=pid, ua=ua, ub=ub, got=[float(v) for v in prop[0]], ref=[float(v) for v in ref[0]], **_ulp_fig(prop, ref)))
    return out


def work_normals_mutate(cfg):
    out = []
    for d, n, stage, gid0, seed in cfg["cases"]:
        sp = _flat_spec(d)
        e = _engine(n, d, seed, gid0)
        e.set_model(sp)
        e.upload_cloud(_zero_cloud(n, d))
        e.initialize_likelihoods()
        bf, ba, bp = mr.generate_blocks(d, d, list(range(d)), seed, stage)
        acc = e.mutate(np.zeros(d), np.eye(d), bp, bf, 1.0, 0.0, 1.0, 1.0, 1, stage)
        P = e.download_cloud()
        e.close()
        pid = np.arange(n, dtype=np.uint64) + np.uint64(gid0)
        ref = np.empty((n, d), dtype=LD)
        for b in range(d):
            ref[:, ba[b]] = _normals_ref(seed, pid, stage, b, 1)[:, 0]
        out.append(dict(case=[d, n, stage, gid0, seed], accept=float(acc), all_accepted=bool(np.all(P[:, d + 3] == 1.0)), **_ulp_fig(P[:, :d], ref)))
    return out


def _whole_vector_cases(name):
    """the cases of a class whose one block is the whole vector (what debug_proposal_densities takes), d <= 10"""
    for case in mr.cases(name):
        d = case.cloud.shape[1] - 5
        if d <= 10 and case.n_blocks == 1 and case.n_mh == 1 and not any(case.spec["fixed"]) and not np.isnan(case.cloud[:, :d]).any():
            yield name, case


def work_densities(cfg):
    from oracle import oracle as orc
    from smc_jl_amd.host.engine import debug_proposal_densities

    out = []
    for name, case in _whole_vector_cases(cfg["name"]):
        d = case.cloud.shape[1] - 5
        res = mr.mutate(case)
        s = res.steps[0]
        F = mr.block_factor(case.mu, case.Sigma, range(d), case.c)
        rows = np.arange(0, case.cloud.shape[0], cfg["every"])
        x = s.state_theta[rows]
        pts = [(x, tr.f64(s.theta_new)[rows])] + [(x, x + k * (tr.f64(s.theta_new)[rows] - x)) for k in STRETCH]
        X, XN = np.concatenate([p[0] for p in pts]), np.concatenate([p[1] for p in pts])
        D = mr.densities(F, X, XN, case.alpha)
        rst = np.array([orc.proposal_densities(XN[i], X[i], case.mu, case.Sigma, case.c, case.alpha) for i in range(len(X))])
        # (a density that is itself a subnormal number has lost digits whatever α is: the band of a single value)
        use = ~(D.band | (tr.f64(D.logq0) < mr.EXP_SUBN) & np.isfinite(tr.f64(D.logq0)) | (tr.f64(D.logq1) < mr.EXP_SUBN) & np.isfinite(tr.f64(D.logq1)))
        fig = {}
        for j, (key, ref) in enumerate((("q0", D.logq0), ("q1", D.logq1))):
            S = np.where(np.isfinite(ref), np.abs(ref), 0)
            fig["rst_" + key] = float(mr.nerr_log(rst[:, j], ref, S)[use].max(initial=0.0))
        bar = max(mr.FLOOR_LOG, mr.FACTOR * max(fig["rst_q0"], fig["rst_q1"]))
        dev = np.array([debug_proposal_densities(XN[i], X[i], case.mu, case.Sigma, case.c, case.alpha) for i in range(len(X))])
        bad = []
        for j, (key, ref) in enumerate((("q0", D.logq0), ("q1", D.logq1))):
            S = np.where(np.isfinite(ref), np.abs(ref), 0)
            err = mr.nerr_log(dev[:, j], ref, S)
            fig["dev_" + key] = float(err[use].max(initial=0.0))
            bad += [dict(point=int(i), which=key, got=repr(float(dev[i, j])), ref=repr(float(ref[i])), rst=repr(float(rst[i, j])), e=[float(D.e0[i]), float(D.e1[i]), float(D.e2_0[i]), float(D.e2_1[i])])
                    for i in np.flatnonzero(use & ~(err <= bar))[:4]]
        r64 = tr.f64(D.logq0)
        out.append(dict(label="%s / %s" % (name, case.label), n=int(len(X)), band=int((~use).sum()), bar=bar, n_bad=len(bad), bad=bad[:6], nan=int(np.isnan(r64).sum()),
                        pinf=int((r64 == np.inf).sum()), ninf=int((r64 == -np.inf).sum()), zero_quirk=int(((r64 == 0.0) & (tr.f64(D.logq1) == np.inf)).sum()), **fig))
    return out


def _yard(name, n):
    from tests.test_mutation_ref_cpu import restatement_yardsticks

    return restatement_yardsticks(name, n)


def work_closure(cfg):
    """Engine.propose / Engine.accept per (step, block) of every case of a class"""
    name, n = cfg["name"], cfg["n"]
    y = _yard(name, n)
    out = []
    for case, res in zip(y["cases"], y["results"]):
        d = case.cloud.shape[1] - 5
        bf, ba, bp = mr.own_blocks(case)
        nb = len(bp) - 1
        lp_bar = y["bars"]["lp"]
        e = _engine(n, d, case.seed)
        e.set_model(case.spec)
        e.upload_cloud(case.cloud)
        o = dict(label=case.label, d=d, steps=len(res.steps), theta=0.0, lp=0.0, q=0.0, bad_theta=0, bad_lp=0, bad_q=0, flips=0, decided=0, comp_wrong=0, inb_wrong=0, examples=[])
        und, band, drop, total = mr.left_out(res)
        o.update(undecided=und, band=band, dropped=drop, decisions=total)
        old = case.spec.get("old_lik") is not None
        P = case.cloud
        for k, s in enumerate(res.steps):
            prop, lpr, qd = e.propose(case.mu, case.Sigma, bp, bf, s.block, s.t // nb, case.c, case.alpha, case.stage)
            use = s.active & (s.outcome != mr.BAND)
            et = mr.nerr_theta(prop[:, s.pos], s.theta_new, s.scale)
            el = mr.nerr_log(lpr, np.where(s.inb, s.lp, -LD(np.inf)), s.lp_S)
            # (a bounds verdict within the θ' bar of a bound is the device's own: such rows - none in these classes - would show as a log-prior of another infinity)
            eq = mr.nerr_log(qd, s.dens.diff, s.dens.S)
            # the component, directly: a proposal that is not the reference's component's draw but another component's
            F = mr.block_factor(case.mu, case.Sigma, s.idx, case.c)
            other = np.zeros(n, dtype=bool)
            for comp in range(3):
                alt, alt_s = mr.draw(F, s.state_theta[:, s.pos], s.z, np.full(n, comp))
                other |= (s.comp != comp) & np.all(mr.nerr_theta(prop[:, s.pos], alt, alt_s) <= y["bars"]["theta"], axis=1)
            o["comp_wrong"] += int((use & other & ~np.all(et <= y["bars"]["theta"], axis=1)).sum())
            o["theta"], o["lp"], o["q"] = max(o["theta"], float(et[use].max(initial=0.0))), max(o["lp"], float(el[use].max(initial=0.0))), max(o["q"], float(eq[use].max(initial=0.0)))
            bt, bl, bq = use[:, None] & ~(et <= y["bars"]["theta"]), use & ~(el <= lp_bar), use & ~(eq <= y["bars"]["q"])
            o["bad_theta"] += int(bt.sum()); o["bad_lp"] += int(bl.sum()); o["bad_q"] += int(bq.sum())
            o["inb_wrong"] += int((use & ((lpr == -np.inf) != (tr.f64(np.where(s.inb, s.lp, -LD(np.inf))) == -np.inf))).sum())
            o["unmoved"] = bool(np.array_equal(np.delete(prop, s.pos, axis=1), np.delete(P[:, :d], s.pos, axis=1), equal_nan=True)) and o.get("unmoved", True)
            for i in np.flatnonzero(bq | bl | bt.any(axis=1))[:2]:
                o["examples"].append(dict(step=k, row=int(i), comp=int(s.comp[i]), q=[repr(float(qd[i])), repr(float(s.dens.diff[i]))], lp=[repr(float(lpr[i])), repr(float(s.lp[i]))], et=float(et[i].max())))
            e.accept(tr.f64(s.ll), tr.f64(s.old) if old else None, case.phi, s.block, s.t // nb, nb, case.stage, k == len(res.steps) - 1)
            P1 = e.download_cloud()
            with np.errstate(invalid="ignore"):
                moved = np.any(P1[:, s.pos] != P[:, s.pos], axis=1) & ~np.isnan(P1[:, s.pos]).any(axis=1)
            decided = use & (s.outcome != mr.UNDECIDED)
            wrong = decided & (moved != (s.outcome == mr.ACCEPT))
            o["flips"] += int(wrong.sum()); o["decided"] += int(decided.sum())
            for i in np.flatnonzero(wrong)[:2]:
                o["examples"].append(dict(step=k, row=int(i), flip=True, outcome=int(s.outcome[i]), log_eta=repr(float(s.log_eta[i])), log_u=float(s.log_u[i]), q=[repr(float(qd[i])), repr(float(s.dens.diff[i]))]))
            P = P1
        keep = ~res.dropped
        o["column_wrong"] = int((P[keep, d + 3] != res.accept_col[keep]).sum())
        o["bars"] = [y["bars"]["theta"], lp_bar, y["bars"]["q"]]
        o["rst"] = [y["theta"], y["q"], y["eta"]]
        o["examples"] = o["examples"][:6]
        e.close()
        out.append(o)
    return out


def _final_fig(case, res, P1, bar):
    """a mutated cloud against the reference's call: accept columns of the rows that were not dropped, θ of the moved rows, rows that stayed"""
    n, d = case.cloud.shape[0], case.cloud.shape[1] - 5
    # the scale of every element of the reference's final θ: that of the last accepted proposal that wrote it
    scale, ref = np.ones((n, d), dtype=LD), case.cloud[:, :d].astype(LD)
    for s in res.steps:
        acc = s.outcome == mr.ACCEPT
        scale[np.ix_(acc, s.pos)], ref[np.ix_(acc, s.pos)] = s.scale[acc], s.theta_new[acc]
    keep = ~res.dropped
    und, band, drop, total = mr.left_out(res)
    col = P1[:, d + 3]
    wrong = keep & (col != res.accept_col)
    moved, stayed = keep & (res.count > 0), keep & (res.count == 0)
    et = mr.nerr_theta(P1[:, :d], ref, scale)
    comps = sorted({int(c) for s in res.steps for c in np.unique(s.comp)})
    return dict(decisions=total, undecided=und, band=band, dropped=drop, column_wrong=int(wrong.sum()), wrong_rows=[[int(i), float(col[i]), float(res.accept_col[i])] for i in np.flatnonzero(wrong)[:5]],
                theta=float(et[moved].max(initial=0.0)), bad_theta=int((moved[:, None] & ~(et <= bar)).sum()), bar=bar, comps=comps,
                stayed_bits=bool(np.array_equal(P1[stayed, :d + 3], case.cloud[stayed, :d + 3], equal_nan=True)), accepted_share=float((res.count > 0).mean()),
                column_mean=float(np.sum(col.astype(LD)) / LD(n)), exact_rate=None if res.rate is None else float(res.rate), n=n)


def _case_yardstick(case):
    """the reference's call on one case and the restatement's errors on it (the bars of a vehicle whose case exists only once the device has run a
    stage's correction: the case is built from what the stage records and the moments say, not from a class)"""
    from tests.test_mutation_ref_cpu import restatement_errors

    res = mr.mutate(case)
    worst, flips = restatement_errors(case, res)
    tol = max(mr.FLOOR_DECIDE, mr.FACTOR * worst["eta"])
    if tol > mr.FLOOR_DECIDE:
        res = mr.mutate(case, tol=tol)
        w2, flips = restatement_errors(case, res)
        worst = {k: max(worst[k], w2[k]) for k in worst}
    return res, worst, flips, max(mr.FLOOR_THETA, mr.FACTOR * worst["theta"])


STAGE_KW = dict(use_fixed_schedule=True, n_phi=100, lam=2.0, n_blocks=1, c=0.3, target=0.25)
STAGE_SEED = 23


def _stage_case(sp, P0, rec, mean, cov, alpha, seed, label):
    """the mutation of stage 2 as the reference sees it: the uploaded cloud (after the restatement's selection if the stage resampled), ϕ and c
    from the stage records, the moments the engine used, the reference's own block"""
    from oracle import oracle as orc

    n, d = P0.shape[0], P0.shape[1] - 5
    phi, c = float(rec["schedule"][1]), float(rec["c_hist"][1])
    pre = np.array(P0, order="F")
    if int(rec["resampled"][1]):
        _, _, nw, _, _ = orc.correct(P0, phi, 0.0)
        idx = orc.resample(nw / float(n), "systematic", seed, 2)
        pre = np.asfortranarray(P0[idx])
    free = mr._free(sp)
    S = np.asarray(cov)[np.ix_(free, free)]
    return mr.Case(label, sp, pre, np.asarray(mean)[free].copy(), S.copy(), c, float(alpha), phi, 1, 1, 2, seed, {})


def _prepared_cloud(e_list, sp, th, shards):
    """θ scored on the device (columns d, d + 1; old_loglh 0), uploaded again -> the cloud as one array"""
    n, d = th.shape
    P = _zero_cloud(n, d)
    P[:, :d] = th
    m = n // shards
    for r, e in enumerate(e_list):
        e.upload_cloud(np.asfortranarray(P[r * m:(r + 1) * m]))
        e.initialize_likelihoods()
    P0 = np.asfortranarray(np.concatenate([e.download_cloud() for e in e_list], axis=0))
    P0[:, d + 2] = 0.0
    for r, e in enumerate(e_list):
        e.upload_cloud(np.asfortranarray(P0[r * m:(r + 1) * m]))
    return P0


def work_stages(cfg):
    """stage 2 on an uploaded cloud through one engine path (the environment of the worker chooses it), then stage 3's c"""
    from smc_jl_amd import Engine
    from smc_jl_amd.host import engine as eng
    from smc_jl_amd.host._lib import SMCMIError

    out = []
    n, shards = cfg["n"], cfg.get("shards", 1)
    for name, alpha, resample in cfg["cases"]:
        sp = getattr(tr, name)()
        d = len(sp["priors"])
        o = dict(label="%s alpha=%g %s" % (name, alpha, "resampling" if resample else "no resampling"), error="", alpha=alpha, resample=bool(resample))
        out.append(o)
        es = []
        try:
            for r in range(shards):
                e = Engine(n, d, seed=STAGE_SEED, max_stages=STAGE_KW["n_phi"], store_history=True, n_local=n // shards, gid0=r * (n // shards))
                e.set_model(sp)
                es.append(e)
            P0 = _prepared_cloud(es, sp, tr.prior_draws(sp, n, mr._seed("stage", name)), shards)
            kw = dict(STAGE_KW, alpha=alpha, threshold_ratio=1.0 if resample else 0.0)
            run = (lambda **k: eng.run_group(es, **k)) if shards > 1 else es[0].run
            r2 = run(stop_after_stage=2, **kw)
            P1 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            rec = es[0].stage_records(r2["n_stages"])
            mean, cov = es[0].stage_moments()
            r3 = run(stop_after_stage=3, continue_run=True, **kw)
            rec3 = es[0].stage_records(r3["n_stages"])
            o.update(n_stages=[r2["n_stages"], r3["n_stages"]], resampled=int(rec["resampled"][1]), fallback=r2["shift_fallback_stage"], segments=[r2["n_segments"], r2["segment_stages"]],
                     stalls=[r2["solver_stalls"], r2["select_stalls"], r2["spec_stalls"], r2["segment_timeouts"]], accept=float(rec["accept_hist"][1]), c=[float(v) for v in rec3["c_hist"][:3]])
            case = _stage_case(sp, P0, rec, mean, cov, alpha, STAGE_SEED, o["label"])
            res, worst, flips, bar = _case_yardstick(case)
            o.update(_final_fig(case, res, P1, bar))
            o.update(rst=[worst["theta"], worst["q"], worst["eta"]], rst_flips=flips)
            o["rate_err"] = abs(o["accept"] - o["column_mean"]) / max(abs(o["column_mean"]), 1e-300)
            if res.rate is not None:
                import mpmath as mp
                with mp.workdps(50):
                    want = mp.mpf(o["c"][1]) * mr.factor_mp(res.rate, STAGE_KW["target"])
                    o["c_next_err"] = float(abs(mp.mpf(o["c"][2]) - want) / want)
        except SMCMIError as ex:
            o["error"], o["code"] = str(ex)[:300], int(ex.code)
        finally:
            for e in es:
                e.close()
    return out


ENS_KW = dict(use_fixed_schedule=True, n_phi=2, lam=1.0, n_blocks=1, c=0.3)      # the shortest fixed schedule: stage 2 alone (ϕ: 0 -> 1)


def work_ensemble(cfg):
    """whole runs of the shortest fixed schedule in one launch (kens_run), every member against the reference's call"""
    from smc_jl_amd import Engine, run_ensemble
    from smc_jl_amd.host._lib import SMCMIError
    from tests.test_gpu_target_range import mutation_cloud, posterior_cloud, stage_spec

    out = []
    n = cfg["n"]
    for label in cfg["specs"]:
        sp = stage_spec(label)
        d = len(sp["priors"])
        es, P0s = [], []
        try:
            for m in range(cfg["members"]):
                e = Engine(n, d, seed=STAGE_SEED + m, max_stages=8, store_history=True)
                e.set_model(sp)
                th = posterior_cloud(sp, n, STAGE_SEED + m) if label == "linmodel3" else mutation_cloud(label + " member %d" % m if m else label, "prior_like", sp, n)
                P0s.append(_prepared_cloud([e], sp, th, 1))
                es.append(e)
            rs = run_ensemble(es, **ENS_KW)
            for m, (e, r) in enumerate(zip(es, rs)):
                P1 = e.download_cloud()
                rec = e.stage_records(r["n_stages"])
                mean, cov = e.stage_moments()
                o = dict(label="%s member %d" % (label, m), error="", status=[r["status"], r["call_status"]], n_stages=r["n_stages"], resampled=int(rec["resampled"][1]), accept=float(rec["accept_hist"][1]))
                case = _stage_case(sp, P0s[m], rec, mean, cov, 1.0, STAGE_SEED + m, o["label"])
                res, worst, flips, bar = _case_yardstick(case)
                o.update(_final_fig(case, res, P1, bar))
                o.update(rst=[worst["theta"], worst["q"], worst["eta"]], rst_flips=flips)
                o["rate_err"] = abs(o["accept"] - o["column_mean"]) / max(abs(o["column_mean"]), 1e-300)
                out.append(o)
        except SMCMIError as ex:
            out.append(dict(label=label, error=str(ex)[:300], code=int(ex.code)))
        finally:
            for e in es:
                e.close()
    return out


def work_mutate(cfg):
    """Engine.mutate on every case of a class"""
    name, n = cfg["name"], cfg["n"]
    y = _yard(name, n)
    out = []
    for case, res in zip(y["cases"], y["results"]):
        d = case.cloud.shape[1] - 5
        bf, ba, bp = mr.own_blocks(case)
        e = _engine(n, d, case.seed)
        e.set_model(case.spec)
        e.upload_cloud(case.cloud)
        rate = e.mutate(case.mu, case.Sigma, bp, bf, case.phi, 0.0, case.c, case.alpha, case.n_mh, case.stage)
        P1 = e.download_cloud()
        e.close()
        o = dict(label=case.label, d=d, kernel="k_mutate_reg" if d <= 10 else "k_mutate<0>", alpha=case.alpha, rst=[y["theta"], y["q"], y["eta"]], rate=float(rate))
        o.update(_final_fig(case, res, P1, y["bars"]["theta"]))
        o["rate_err"] = abs(float(rate) - o["column_mean"]) / max(abs(o["column_mean"]), 1e-300) if o["column_mean"] else abs(float(rate))
        # (no row dropped: the exact rate is known, and the returned one is its FP64 mean)
        o["exact_rate_err"] = None if o["exact_rate"] is None else abs(float(rate) - o["exact_rate"]) / max(o["exact_rate"], 1e-300) if o["exact_rate"] else abs(float(rate))
        out.append(o)
    return out


def work_class(cfg):
    """both vehicles of a class in one worker: the reference and the yardsticks are computed once"""
    return dict(closure=work_closure(cfg), mutate=work_mutate(cfg))


def worker_main(kind, cfg):
    res = dict(classes=work_class, normals_propose=work_normals_propose, normals_search=work_normals_search, normals_mutate=work_normals_mutate, densities=work_densities,
               stages=work_stages, ensemble=work_ensemble)[kind](json.loads(cfg))
    print("RESULT " + json.dumps(res))


# ------------------------------------------------------------------------------------------------ test side
_CHILD = "import sys; sys.path.insert(0, %r); from tests import test_gpu_mutation_range as T; T.worker_main(%r, %r)"


def _spawn(kind, cfg, env_extra=None, timeout=300):
    env = dict(os.environ)
    env.update(env_extra or {})
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, kind, json.dumps(cfg))], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired as ex:                  # a hang: nothing more is started on that GPU by this file either
        pytest.exit("a worker of tests/test_gpu_mutation_range.py (%s) did not end within %d s:\n%s" % (kind, timeout, (ex.stderr or "")[-3000:]), returncode=3)
    # the worker died of a signal or met a GPU fault: nothing more is started on that GPU by this file
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:
        pytest.exit("a worker of tests/test_gpu_mutation_range.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


T_ALL = list(range(30))


def _propose_cases():
    cs = [(d, 2368, 299, STRADDLE, 123, [0, 1, 2, 7, 29] if d > 2 else [0, 1, 29]) for d in PROPOSE_D]
    cs += [(9, 2368, st, 0, 5, T_ALL if st == 299 else [0, 29]) for st in (1, 299, (1 << 32) - 1)]
    cs += [(9, n, st, g, 77, [0, 5, 29]) for n in (1, 63) for st, g in ((1, 0), ((1 << 32) - 1, STRADDLE + 1184 - 31))]
    return cs


def _check_normals(res, why, what):
    for o in res:
        print(what, json.dumps(o))
        if o["over"] or not o["worst"] <= ULP_BAR:
            why.append("%s %r: %d of %d normals beyond %g ulp, the worst %.3g" % (what, o.get("case", o.get("name")), o["over"], o["n"], ULP_BAR, o["worst"]))
        if not o.get("rest_zero", True):
            why.append("%s %r: something outside the block moved, or q0 - q1 is not 0" % (what, o["case"]))
        if not o.get("all_accepted", True):
            why.append("%s %r: a proposal on the flat target was not accepted" % (what, o["case"]))


def test_normals_through_the_proposals_of_the_generic_body():
    cases = _propose_cases()
    res = _spawn("normals_propose", dict(cases=cases))
    why = []
    _check_normals(res, why, "propose")
    assert len(res) == len(cases) and not why, "\n".join(why)


def test_normals_at_the_ids_a_search_of_the_reference_finds():
    res = _spawn("normals_search", dict(seed=123, stage=7, n_ids=SEARCH_IDS))
    why = []
    _check_normals(res, why, "search")
    # the inputs hold: the search reaches the tails it is there for
    by = {o["name"]: o for o in res}
    assert by["ua_min"]["ua"] < 1e-7 and by["ua_max"]["ua"] > 1 - 1e-7 and all(abs(by["ub_%d/4" % k]["ub"] - 0.25 * k) < 1e-7 for k in range(5)), by
    assert len(res) == 7 and not why, "\n".join(why)


def test_normals_through_the_register_kernel_on_a_flat_target():
    cases = [(d, 2368, 299, STRADDLE, 123) for d in MUTATE_D] + [(9, n, st, 0, 77) for n in (1, 63, 2368) for st in (1, (1 << 32) - 1)]
    res = _spawn("normals_mutate", dict(cases=cases))
    why = []
    _check_normals(res, why, "mutate")
    assert len(res) == len(cases) and not why, "\n".join(why)


DENSITY_CLASSES = ("benign", "ill_conditioned", "far", "mu_far", "density_scale", "alpha", "tight_bounds", "phi")     # (dead_rows: NaN rows; blocks: fixed parameters)


@pytest.mark.parametrize("name", DENSITY_CLASSES)
def test_dense_densities_at_chosen_points(name):
    res = _spawn("densities", dict(name=name, every=13))
    why = []
    for o in res:
        print(json.dumps(o))
        if o["n_bad"]:
            why.append("%s: %d values beyond the bar %.3g (restatement %.3g / %.3g, device %.3g / %.3g): %r" % (o["label"], o["n_bad"], o["bar"], o["rst_q0"], o["rst_q1"], o["dev_q0"], o["dev_q1"], o["bad"][:3]))
    # Left out (band, or a density that is itself a subnormal number): the chosen points include moves stretched up to 40 times, whose densities
    # are subnormal by construction where the class sits at the underflow end (s = 1e30: 16 of 96), so the cap is not the decisions' 1e-3 but a
    # quarter of a case's points and a twentieth of the class's
    for o in res:
        if o["band"] > o["n"] // 4:
            why.append("%s: %d of %d points left out" % (o["label"], o["band"], o["n"]))
    if sum(o["band"] for o in res) > sum(o["n"] for o in res) // 20:
        why.append("%s: %d of %d points left out" % (name, sum(o["band"] for o in res), sum(o["n"] for o in res)))
    assert res and not why, "\n".join(why)
    if name == "density_scale":                              # the inputs hold: both rules' outcomes are among the points
        assert sum(o["nan"] for o in res) > 0 and sum(o["zero_quirk"] for o in res) > 0


_CLASS_RUNS = {}


def _class_run(name):
    if name not in _CLASS_RUNS:
        _CLASS_RUNS[name] = _spawn("classes", dict(name=name, n=mr.N_CLASS), timeout=300)
    return _CLASS_RUNS[name]


def _check_left_out(o, why):
    if o["undecided"] + o["band"] + o["dropped"] > mr.CAP * o["decisions"]:
        why.append("%s: %d undecided, %d band, %d dropped of %d decisions" % (o["label"], o["undecided"], o["band"], o["dropped"], o["decisions"]))


@pytest.mark.parametrize("name", list(mr.CLASSES))
def test_the_closure_path(name):
    res = _class_run(name)["closure"]
    why = []
    for o in res:
        print(name, json.dumps(o))
        _check_left_out(o, why)
        for key, msg in (("bad_theta", "θ' beyond the bar"), ("bad_lp", "log-priors beyond the bar"), ("bad_q", "q0 - q1 beyond the bar"), ("flips", "decided decisions that are not the reference's"),
                         ("column_wrong", "accept columns that are not the reference's"), ("inb_wrong", "bounds verdicts that are not the reference's"),
                         ("comp_wrong", "proposals drawn from another component than the reference's")):
            if o[key]:
                why.append("%s: %d %s (worst θ' %.3g, log-prior %.3g, q %.3g; bars %r): %r" % (o["label"], o[key], msg, o["theta"], o["lp"], o["q"], o["bars"], o["examples"][:3]))
        if not o["unmoved"]:
            why.append("%s: a parameter outside the block changed" % o["label"])
    assert res and not why, "\n".join(why)


@pytest.mark.parametrize("name", list(mr.CLASSES))
def test_stand_alone_mutations(name):
    res = _class_run(name)["mutate"]
    why = []
    for o in res:
        print(name, json.dumps(o))
        _check_left_out(o, why)
        if o["column_wrong"]:
            why.append("%s (%s): %d accept columns are not the reference's: %r" % (o["label"], o["kernel"], o["column_wrong"], o["wrong_rows"]))
        if o["bad_theta"]:
            why.append("%s (%s): %d elements of moved rows beyond the bar %.3g, the worst %.3g" % (o["label"], o["kernel"], o["bad_theta"], o["bar"], o["theta"]))
        if not o["stayed_bits"]:
            why.append("%s: a row that did not move changed" % o["label"])
        if not o["rate_err"] <= o["n"] * 2.0 ** -53:
            why.append("%s: the returned rate %.17g is not the column's mean %.17g" % (o["label"], o["rate"], o["column_mean"]))
        if o["exact_rate_err"] is not None and not o["exact_rate_err"] <= o["n"] * 2.0 ** -53:
            why.append("%s: the returned rate %.17g is not the reference's exact rate %.17g" % (o["label"], o["rate"], o["exact_rate"]))
    assert res and not why, "\n".join(why)
    kernels = {(o["kernel"], o["alpha"] == 1.0) for o in res}
    if name == "benign":
        assert kernels >= {("k_mutate_reg", True), ("k_mutate_reg", False), ("k_mutate<0>", True), ("k_mutate<0>", False)}, kernels


SMCMI_ERR_ARG = -1            # include/smcmi.h: what the router answers a pair it does not serve with; any other error fails the test
_FOUR = [("sixpriors", 1.0, 0), ("sixpriors", 1.0, 1), ("sixpriors", 0.9, 0), ("sixpriors", 0.9, 1)]
STAGE_CASES = {"segments": _FOUR, "launches": _FOUR, "engine1": _FOUR, "large_shard_stage": _FOUR, "two_shards": _FOUR, "two_chunk_segments": [("sixpriors", 1.0, 0)],
               "wide": [("wide12", a, r) for _, a, r in _FOUR]}


def _check_stage(o, why, what, seg=None):
    _check_left_out(o, why)
    if o["column_wrong"]:
        why.append("%s: %d accept columns are not the reference's: %r" % (what, o["column_wrong"], o["wrong_rows"]))
    if o["bad_theta"]:
        why.append("%s: %d elements of moved rows beyond the bar %.3g, the worst %.3g" % (what, o["bad_theta"], o["bar"], o["theta"]))
    if not o["stayed_bits"]:
        why.append("%s: a row that did not move changed" % what)
    if o["rst_flips"]:
        why.append("%s: the restatement flips %d decisions" % (what, o["rst_flips"]))
    if not o["rate_err"] <= o["n"] * 2.0 ** -53:
        why.append("%s: the recorded acceptance rate %.17g is not the column's mean %.17g" % (what, o["accept"], o["column_mean"]))
    if "c_next_err" in o and not o["c_next_err"] <= 1e-14:
        why.append("%s: the next stage's c %.17g is off the exact factor of the exact rate by %.3g" % (what, o["c"][2], o["c_next_err"]))
    if not 0.02 <= o["accepted_share"] <= 0.98:
        why.append("%s: %.3g of the rows moved - the input does not hold" % (what, o["accepted_share"]))


@pytest.mark.parametrize("path", list(STAGE_CASES))
def test_one_bracketed_stage_per_engine_path(path):
    """stage 2 on an uploaded cloud at α = 1 and α = 0.9, without and with resampling (threshold ratios 0 and 1; the ancestors are the
    restatement's), against the reference's call started from that cloud with the stage's recorded ϕ and c, the moments the engine used and
    the reference's own block; then stage 3's c against the exact factor of the exact acceptance rate"""
    from tests.test_gpu_weight_range import PATHS

    env, over, seg = PATHS[path]
    res = _spawn("stages", dict(cases=STAGE_CASES[path], n=over.get("n", 20480), shards=over.get("shards", 1)), env, timeout=300)
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
        _check_stage(o, why, what)
        if o["n_stages"] != [2, 3] or o["resampled"] != int(o["resample"]):
            why.append("%s: stages %r, resampled %d" % (what, o["n_stages"], o["resampled"]))
        if seg and not (o["segments"][1] >= seg and o["stalls"] == [0, 0, 0, 0] and o["fallback"] == 0):
            why.append("%s: the stage did not (provably) complete inside a segment: segments %r stalls %r fallback %r" % (what, o["segments"], o["stalls"], o["fallback"]))
        if seg is False and o["segments"][0] != 0:
            why.append("%s: the bracket ran segments: %r" % (what, o["segments"]))
    assert ran >= 1 and not why, "\n".join(why)


def test_the_ensemble_kernel():
    res = _spawn("ensemble", dict(n=1024, members=3, specs=["sixpriors", "linreg", "linmodel3"]), timeout=600)
    why, ran = [], 0
    for o in res:
        print(json.dumps(o))
    for o in res:
        if o["error"]:
            print("%s: refused: %s" % (o["label"], o["error"]))
            if o.get("code") != SMCMI_ERR_ARG:
                why.append("%s: %s" % (o["label"], o["error"]))
            continue
        ran += 1
        _check_stage(o, why, o["label"])
        if o["status"] != [0, 0] or o["n_stages"] != 2:
            why.append("%s: status %r, %d stages" % (o["label"], o["status"], o["n_stages"]))
    assert ran >= 6 and not why, "\n".join(why)
