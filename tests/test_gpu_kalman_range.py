"""The three device Kalman filters (csrc/model.hpp kalman_lgss2, kalman_lgss_quad, kalman_lgss_wave) against the extended-precision
reference of tests/kalman_ref.py (pinned against mpmath by tests/test_kalman_ref_cpu.py), at the edges of the region the model declares.

Reaching each filter: kalman_lgss_quad and kalman_lgss_wave score an uploaded cloud in initialize_likelihoods (SMCMI_KALMAN_LANES = 4 / 1) -
200 / 300 particles, the class's 24 θ repeated down the cloud, so neither the last wavefront nor the last block is full and every θ is
scored in several lanes; kalman_lgss2 scores the draws of init_from_prior, with the priors and bounds of the spec narrowed onto the class's
boxes, and the reference is evaluated at the θ that come back (they must be the oracle's draws: a finite value turned into -Inf would show as
a redraw).  Every test is a child process (the switches are read once per process; a worker that dies ends the session).

Every error is the normalised error |Δll| / max(1, S) of tests/kalman_ref.py.  The bar of a class and variant: max(1e-12, 16 x the worst
normalised error of the FP64 oracle over the same θ), θ at which the oracle is off by more than 1e-10 left out (at most an eighth); 1e-12 is
what model.hpp states for its filters, 16 allows for another summation order and for products of Newton-refined reciprocals in place of
correctly rounded sqrt and division.  The oracle's error is computed in the worker, on the CPU, before the device's values are looked at.  Where
the oracle is finite (everywhere: asserted) the device value must be finite; no value may be NaN.

Rows through a mutation (Engine.mutate with the cloud's own weighted moments as the proposal, c such that at least a tenth of the rows move and
at least a tenth stay - asserted): afterwards column 13 of every row is the reference's log-likelihood of that row's 13 parameters and column 15
the old vintage's, under the same bar - both filters, n_blocks 1 and 3, α 1 and 0.9, on the prior, snr and roots_pos clouds; and on the prior cloud
with the old vintage the first 1, 40, 79 and 80 of the 80 periods (one filter pass, the value taken at step nt_mid) and y[:, 1:41] (no prefix:
two passes).

Measured on an MI355X, worst normalised error over the included rows (oracle: the FP64 oracle on the same θ; kalman_lgss2 has its own column
because it is scored on the device's draws, not on the class's 24 θ):

  class            variant      oracle    quad      wave      bar       | oracle    lgss2     bar      (on the draws)
  prior            T=80         2.5e-15   7.9e-16   4.8e-16   1.0e-12   | 7.7e-14   6.4e-14   1.2e-12
  prior            T=400        3.4e-15   1.3e-15   8.8e-16   1.0e-12   | 1.8e-13   1.9e-13   2.8e-12
  snr              T=80         1.1e-13   2.6e-13   1.3e-13   1.8e-12   | 5.4e-12   6.4e-12   8.7e-11
  snr              T=400        4.7e-13   5.1e-13   5.8e-13   7.5e-12   | 6.1e-12   7.1e-12   9.8e-11
  quiet            T=80         5.2e-16   4.6e-16   2.7e-16   1.0e-12   | 6.8e-16   6.8e-16   1.0e-12
  roots_mixed      T=80         1.1e-15   1.7e-15   2.0e-15   1.0e-12   | 1.8e-14   1.7e-14   1.0e-12
  roots_pos        T=80         1.3e-14   4.7e-15   4.3e-15   1.0e-12   | 1.1e-14   9.2e-15   1.0e-12
  roots_pos        T=400        2.7e-11   1.9e-12   5.1e-15   4.3e-10   | 6.0e-11   1.1e-13   9.5e-10
  all_edges        T=80         3.9e-14   5.8e-15   1.7e-15   1.0e-12   | 2.8e-14   2.7e-15   1.0e-12
  mu_far           T=80         3.4e-13   7.2e-13   1.7e-13   5.4e-12   | 6.4e-14   8.9e-14   1.0e-12
  mu_far           T=400        2.0e-13   6.4e-13   2.9e-13   3.1e-12   | 1.5e-13   1.9e-13   2.3e-12
  short            T=1          4.7e-16   2.5e-16   2.6e-16   1.0e-12   | 8.5e-16   8.6e-16   1.0e-12
  short            T=2          2.6e-15   6.6e-16   2.0e-15   1.0e-12   | 8.6e-15   2.1e-14   1.0e-12
  short            T=3          1.7e-15   1.3e-14   5.8e-15   1.0e-12   | 2.8e-14   2.6e-14   1.0e-12
  short            T=41         2.3e-15   1.7e-14   2.1e-14   1.0e-12   | 4.8e-14   2.9e-14   1.0e-12
  data_scale       y*1e6        2.7e-15   6.9e-15   6.9e-15   1.0e-12   | 9.1e-14   8.1e-14   1.5e-12
  data_scale       y*1e-6       2.2e-15   5.6e-15   5.2e-15   1.0e-12   | 3.1e-14   1.5e-14   1.0e-12
  dense_structure  kappa=0.2    2.4e-14   1.6e-14   1.2e-14   1.0e-12   | 1.8e-14   6.5e-14   1.0e-12
  dense_structure  kappa=-0.3   7.7e-15   1.3e-14   1.8e-15   1.0e-12   | 1.2e-13   3.5e-14   1.9e-12
  diagonal         T=80         7.0e-16   5.0e-16   4.6e-16   1.0e-12   | 1.0e-15   1.0e-15   1.0e-12

  through a mutation (worst of n_blocks 1, 3 and α 1, 0.9; 0.43 .. 0.75 of the rows moved)
  filter class      old vintage   column 13: oracle  device    column 15: oracle  device
  quad   prior      y[:, :40]                3.2e-14   9.1e-14              2.1e-14   7.3e-14
  quad   snr        y[:, :40]                2.9e-12   2.4e-12              7.5e-12   2.2e-12
  quad   roots_pos  y[:, :40]                8.9e-15   1.2e-14              7.0e-15   1.4e-14
  wave   prior      y[:, :40]                2.4e-13   2.4e-13              2.7e-13   2.4e-13
  wave   snr        y[:, :40]                8.6e-12   4.2e-12              5.1e-12   2.7e-12
  wave   roots_pos  y[:, :40]                9.8e-15   2.1e-15              1.1e-14   1.8e-14
  quad   prior      y[:, :1]                 3.2e-14   1.3e-14              1.5e-15   8.7e-16
  quad   prior      y[:, :79]                3.2e-14   1.3e-14              3.1e-14   1.3e-14
  quad   prior      y[:, :80]                3.2e-14   1.3e-14              3.2e-14   1.3e-14
  quad   prior      y[:, 1:41]               3.2e-14   1.3e-14              1.9e-14   6.7e-15
  wave   prior      y[:, :1]                 2.4e-13   1.5e-13              1.0e-15   1.2e-15
  wave   prior      y[:, :79]                2.4e-13   1.5e-13              2.4e-13   1.5e-13
  wave   prior      y[:, :80]                2.4e-13   1.5e-13              2.4e-13   1.5e-13
  wave   prior      y[:, 1:41]               2.4e-13   1.5e-13              1.2e-13   2.0e-13

Nothing is NaN or -Inf; the same θ gives the same bits in every lane it was scored in; every cloud of init_from_prior is the oracle's draw.  roots_pos at
T = 400 leaves out one of the 24 θ (the oracle is off by 5.0e-9 there; 5 of kalman_lgss2's 200 draws): on the included θ the lane-split filter, which does
not symmetrise its covariance, is at 1.9e-12 where the one-thread filter is at 5.1e-15 and the oracle at 2.7e-11 - inside its bar, no defect; every other
class is within a factor 5 of the oracle.  No filter needed a change.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kalman_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILTERS = dict(quad=dict(n=200, env={"SMCMI_KALMAN_LANES": "4"}), wave=dict(n=300, env={"SMCMI_KALMAN_LANES": "1"}), lgss2=dict(n=200, env={}))
MAX_LEFT_OUT_SHARE = kr.MAX_LEFT_OUT / kr.N_CLASS

# ---- the mutation: ϕ_n and, per n_blocks, the scale c at which the oracle's mutation (oracle.mutate_cloud, on the CPU) of the same clouds moves 0.44 .. 0.64
# (one block) and 0.68 .. 0.75 (three blocks) of the rows; the test asserts the condition - a tenth move, a tenth stay - on what the device did
MUT_PHI, MUT_STAGE, MUT_SEED, MUT_OLD_T = 0.3, 3, 23, 40
MUT_C = {1: 0.05, 3: 0.5}


def _engine(n, spec, seed=MUT_SEED):
    from smc_jl_amd import Engine

    e = Engine(n, 13, seed=seed, max_stages=4, store_history=False)
    e.set_model(spec)
    return e


def _cloud(theta):
    P = np.zeros((theta.shape[0], 18), order="F")
    P[:, :13], P[:, 17] = theta, 1.0
    return P


def _summary(got, ref_ll, ref_S, orc):
    """one line of figures: the oracle's and the device's worst normalised error over the included rows, what is left out, what is not finite"""
    orc_err = kr.nerr(orc, ref_ll, ref_S)
    inc, b, orc_worst = kr.bar(orc_err)
    err = kr.nerr(got, ref_ll, ref_S)
    worst = int(np.argmax(np.where(inc, err, -1.0)))
    return dict(n=int(len(got)), orc_finite=bool(np.all(np.isfinite(orc))), ref_finite=bool(np.all(np.isfinite(np.asarray(ref_ll, dtype=np.float64)))),
                left_out=int((~inc).sum()), orc_worst=orc_worst, bar=b, dev_worst=float(err[inc].max()) if inc.any() else 0.0, worst_row=worst,
                n_nan=int(np.isnan(got).sum()), n_not_finite=int((~np.isfinite(got)).sum()), ll_range=[float(np.min(got)), float(np.max(got))])


def work_values(cfg):
    """the class's variants through one filter -> a summary per variant"""
    from oracle import oracle as orc
    from tests import models

    name, filt = cfg["name"], cfg["filter"]
    n = FILTERS[filt]["n"]
    out = []
    for v in kr.variants(name):
        aux = kr.pack_aux(v.C, v.R, v.Z)
        o = dict(label=v.label)
        if filt == "lgss2":
            boxes = kr.BOXES[name]
            th, got, same = [], [], True
            for b, box in enumerate(boxes):
                sp = kr.box_spec(box, v.y, aux, v.kappa)
                e = _engine(n // len(boxes), sp, seed=MUT_SEED + b)
                e.init_from_prior()
                P = e.download_cloud()
                e.close()
                Q = orc.initial_draw(models.oracle_model(sp), n // len(boxes), seed=MUT_SEED + b)
                same = same and bool(np.allclose(P[:, :13], Q[:, :13], rtol=1e-12, atol=1e-14))
                th.append(P[:, :13])
                got.append(P[:, 13])
            th, got = np.ascontiguousarray(np.concatenate(th, axis=0)), np.concatenate(got)
            o["same_draws"] = same
        else:
            base = kr.thetas(name)
            th = np.ascontiguousarray(base[np.arange(n) % kr.N_CLASS])
            e = _engine(n, kr.box_spec({}, v.y, aux, v.kappa))
            e.upload_cloud(_cloud(th))
            e.initialize_likelihoods()
            got = e.download_cloud()[:, 13].copy()
            e.close()
            # (the same θ in another lane gives the same bits)
            o["lanes_agree"] = bool(all(np.array_equal(got[i::kr.N_CLASS], np.full(len(got[i::kr.N_CLASS]), got[i])) for i in range(kr.N_CLASS)))
        ref = kr.loglik(th, v.y, v.C, v.R, v.Z, v.kappa)
        o.update(_summary(got, ref.ll, ref.S, kr.oracle_loglik(v, th)))
        o["worst_theta"] = th[o["worst_row"]].tolist()
        out.append(o)
    return out


def old_vintage(y, old):
    """(old data, nt_mid or 0): old = k: the first k periods; "shift": y[:, 1:41]"""
    if old == "shift":
        return np.ascontiguousarray(y[:, 1:41]), 0
    return np.ascontiguousarray(y[:, :int(old)]), int(old)


def mutation_inputs(name, n, old):
    v = kr.variants(name)[0]
    assert v.y.shape[1] == 80
    aux = kr.pack_aux(v.C, v.R, v.Z)
    y_old, mid = old_vintage(v.y, old)
    return v, aux, y_old, mid, kr.box_spec({}, y_old, aux, v.kappa), kr.box_spec({}, v.y, aux, v.kappa, old=(y_old, aux)), kr.thetas(name, n)


def proposal(P, n_blocks, spec):
    """the cloud's own weighted moments and the oracle's blocks for MUT_STAGE"""
    from oracle import oracle as orc
    from tests import models

    m = models.oracle_model(spec)
    mean, cov = orc.weighted_mean(P), orc.weighted_cov(P)
    bf, ba, bp = orc.generate_blocks(13, n_blocks, m.free_inds, MUT_SEED, MUT_STAGE)
    return m, mean, (cov + cov.T) / 2.0, bf, ba, bp


def work_mutation(cfg):
    """cases of (class, old vintage, n_blocks, α) through one filter: the tempered cloud as the device scores it, one mutation, every row against the
    reference"""
    filt = cfg["filter"]
    n = FILTERS[filt]["n"]
    out = []
    for name, old, nb, alpha in cfg["cases"]:
        v, aux, y_old, mid, sp_old, sp, th = mutation_inputs(name, n, old)
        e = _engine(n, sp_old)
        e.upload_cloud(_cloud(th))
        e.initialize_likelihoods()                            # column 13: the old vintage's log-likelihoods
        e.set_model(sp)
        e.initialize_likelihoods()                            # column 15 <- column 13, column 13: the new data's
        P0 = e.download_cloud()
        m, mean, cov, bf, ba, bp = proposal(P0, nb, sp)
        acc = e.mutate(mean, cov, bp, bf, MUT_PHI, 0.0, MUT_C[nb], alpha, 1, MUT_STAGE)
        P1 = e.download_cloud()
        e.close()
        th1 = np.ascontiguousarray(P1[:, :13])
        moved = np.any(th1 != P0[:, :13], axis=1)
        ref = kr.loglik(th1, v.y, v.C, v.R, v.Z, v.kappa, nt_mid=mid)
        orc_new = kr.oracle_loglik(v, th1)
        if mid:
            ref_old, S_old = ref.ll_mid, ref.S_mid
        else:
            r2 = kr.loglik(th1, y_old, v.C, v.R, v.Z, v.kappa)
            ref_old, S_old = r2.ll, r2.S
        orc_old = kr.oracle_loglik(v._replace(y=y_old), th1)
        ref0 = kr.loglik(th, v.y, v.C, v.R, v.Z, v.kappa)
        o = dict(case=[name, old, nb, alpha], accept=float(acc), moved=float(moved.mean()), before=_summary(P0[:, 13], ref0.ll, ref0.S, kr.oracle_loglik(v, th)),
                 new=_summary(P1[:, 13], ref.ll, ref.S, orc_new), old=_summary(P1[:, 15], ref_old, S_old, orc_old))
        # the rows that moved and those that stayed, apart: a result that landed in another row shows in one of them
        for key, mask in (("moved", moved), ("stayed", ~moved)):
            if mask.any():
                o["new_" + key] = float(kr.nerr(P1[mask, 13], ref.ll[mask], ref.S[mask]).max())
                o["old_" + key] = float(kr.nerr(P1[mask, 15], ref_old[mask], S_old[mask]).max())
        out.append(o)
    return out


def worker_main(kind, cfg):
    res = dict(values=work_values, mutation=work_mutation)[kind](json.loads(cfg))
    print("RESULT " + json.dumps(res))


_CHILD = "import sys; sys.path.insert(0, %r); from tests import test_gpu_kalman_range as T; T.worker_main(%r, %r)"


def _spawn(kind, cfg, env_extra, timeout=600):
    env = dict(os.environ)
    env.pop("SMCMI_KALMAN_LANES", None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, kind, json.dumps(cfg))], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    # the worker died of a signal or met a GPU fault: nothing more is started on that GPU by this file
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:
        pytest.exit("a worker of tests/test_gpu_kalman_range.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _check_summary(s, why, what):
    """Every figure was printed before this is called."""
    if not (s["orc_finite"] and s["ref_finite"]):
        why.append("%s: the oracle or the reference is not finite on an input" % what)
    if s["left_out"] > MAX_LEFT_OUT_SHARE * s["n"]:
        why.append("%s: %d of %d rows left out" % (what, s["left_out"], s["n"]))
    if s["n_nan"]:
        why.append("%s: %d NaN" % (what, s["n_nan"]))
    if s["n_not_finite"]:
        why.append("%s: %d values not finite where the oracle is" % (what, s["n_not_finite"]))
    if not s["dev_worst"] <= s["bar"]:
        why.append("%s: off by %.3g (bar %.3g, oracle %.3g) at row %d" % (what, s["dev_worst"], s["bar"], s["orc_worst"], s["worst_row"]))


@pytest.mark.parametrize("name", kr.CLASSES)
@pytest.mark.parametrize("filt", list(FILTERS))
def test_filter_values_against_the_reference(filt, name):
    res = _spawn("values", dict(name=name, filter=filt), FILTERS[filt]["env"])
    for o in res:
        print(filt, name, json.dumps(o))
    why = []
    for o in res:
        _check_summary(o, why, "%s %s %s" % (filt, name, o["label"]))
        if not o.get("same_draws", True):
            why.append("%s: the draws are not the oracle's (a redraw: a finite value came out -Inf)" % o["label"])
        if not o.get("lanes_agree", True):
            why.append("%s: the same θ gives other bits in another lane" % o["label"])
    assert len(res) == len(kr.variants(name)) and not why, "\n".join(why)


def _check_mutation(res, filt):
    for o in res:
        print(filt, json.dumps(o))
    why = []
    for o in res:
        what = "%s %r" % (filt, o["case"])
        if not 0.1 <= o["moved"] <= 0.9:
            why.append("%s: %.3g of the rows moved - the input does not hold" % (what, o["moved"]))
        _check_summary(o["before"], why, what + " before")
        _check_summary(o["new"], why, what + " column 13")
        _check_summary(o["old"], why, what + " column 15")
    assert not why, "\n".join(why)


MUT_CASES = [(name, MUT_OLD_T, nb, alpha) for name in ("prior", "snr", "roots_pos") for nb in (1, 3) for alpha in (1.0, 0.9)]
PREFIX_CASES = [("prior", old, 1, 0.9) for old in (1, 40, 79, 80, "shift")]


@pytest.mark.parametrize("name", ["prior", "snr", "roots_pos"])
@pytest.mark.parametrize("filt", ["quad", "wave"])
def test_rows_stay_consistent_through_a_mutation(filt, name):
    cases = [c for c in MUT_CASES if c[0] == name]
    res = _spawn("mutation", dict(filter=filt, cases=cases), FILTERS[filt]["env"])
    assert len(res) == 4
    _check_mutation(res, filt)


@pytest.mark.parametrize("filt", ["quad", "wave"])
def test_prefix_values_at_every_nt_mid_and_a_vintage_that_is_no_prefix(filt):
    res = _spawn("mutation", dict(filter=filt, cases=PREFIX_CASES), FILTERS[filt]["env"])
    assert len(res) == 5
    _check_mutation(res, filt)
