"""The correction's weight sums at the edges of the FP64 range.

Everything a run reports - ESS, the resample decision, the normalised weights, log-MDD, the adaptive ϕ - comes out of
s1 = Σ W̃, s2 = Σ W̃², W̃ = W exp(δ (e - shift)), and whether those sums are right depends on the shift.  The engines shift by the
largest energy of the live cloud, by the one a mutation earlier (fixed schedules: RunParams::shift_lag), or - before this file existed -
not at all (prior_weight != 0, the stand-alone calls).  Here every path runs ONE bracketed stage on clouds whose energies carry a
common offset B (δ B from 0 to 1e6, both signs), which by the reference's arithmetic changes nothing but the log-MDD increment, and
is compared with tests/weights_ref.py (extended precision, exact maximum; pinned on the CPU by tests/test_weights_ref_cpu.py).

Vehicles (the stage engines have no stand-alone entry: a stage is bracketed between two pauses, as tests/test_gpu_strict.py does):
  fresh      init_from_prior, the loglh / old_loglh / weight columns set to the case's values, upload, run(stop_after_stage=2):
             stage 2 is the first correction, on exactly that cloud.
  continued  a benign run paused after stage k - 1, loglh lowered or raised by B, upload, continue to stage k.
  lagged     no upload: SMCMI_SHIFT_LAG=-k / =k (development) raises / lowers stage k's lagged shift by 1e6, and λ of the fixed
             schedule is solved so that δ_k 1e6 is the case's offset - the lagged shift's own window (s2 denormal before anything
             is NaN) with no upload in between.  Stage k is the first stage of its call and does not ride; the RIDING stage
             (correction row formed behind the previous mutation row) is a whole run:
             test_squares_that_underflow_under_a_riding_lagged_shift_switch_the_run_to_exact_shifts.
  three      adaptive schedules only (an adaptive call's first two stages take certificate passes: engine 2's launches on every
             row): the continued vehicle with the cloud RAISED by B and stages k .. k + 2 bracketed - every proposal is rejected,
             so stage k + 2, k3_segment's own predicted-and-verified correction, works on a known cloud.
Which kernels a bracket ran is asserted from the bracket's result (_check: n_segments == 0 on the launch rows; on the rows that claim
the segment kernel, the stages completed inside segments and no stall of any kind).

Tolerances: ESS, log-MDD increment, normalised weights rtol 1e-11 at every offset (the component tests' own; the device exp carries
|x| 2^-53 <= 8e-14 of argument rounding at |x| <= 745); incremental weights rtol 1e-11, atol 1e-300; adaptive ϕ rel 1e-9
(test_solve_phi_vs_oracle); decisions, flags and shift_fallback_stage exact.

Rows of weight 0 with the cloud's largest energy (wr.zero_high_cloud, δΔ = 0 .. 1e6 above the shift, fresh vehicle, fixed schedule and adaptive first
correction, every row of PATHS): before the fix this case came with, 0 x exp(δΔ) = 0 x inf = NaN in every correction and solver pass and the history's
inc x unshift was inf x 0 - measured on the parent's library (segments, launches, engine 1): SMCMI_ERR_NAN_ESS from δΔ = 745 on the fixed schedule (710 is
still 708 above the live cloud's largest energy), SMCMI_ERR_BRACKET from δΔ = 700 on the adaptive first correction (the solver's candidates beyond the
root); now such a row adds exactly 0 and stores the reference's exp(δ e) (kernels.hpp weight_times / row_shift): ESS 7.5e-16, W 7.6e-16, w 2.7e-14,
log-MDD increment 2.5e-15, adaptive ϕ 2.2e-15 over all rows and δΔ.

Measured on an MI355X (largest relative errors over all paths and cases): ESS 6.5e-16, W 4.6e-14, w 7.3e-14, log-MDD increment 5.5e-14, adaptive ϕ
2.3e-15, at every offset; the lagged vehicle carries on at G = ±300 and falls back from ±350 on.  Before the fixes this file came with,
measured on the continued vehicle's cloud (launches row: 20 480 particles of the 10-parameter Gaussian, stage 5 of the fixed schedule n_phi = 40,
λ = 2, reference ESS 10 415.08): ESS off by 2.5e-9 / 3.7e-6 / 0.65 % at δB = 365 / 368 / 370, 21 349.67 (twice its value) at 372 and +inf at 373
and 380, a fallback from ±350 on; prior_weight != 0 and the stand-alone calls: wrong ESS over the same window, NaN-ESS errors beyond.  DESIGN §5
has the table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import weights_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_PARA = 10
N = 20480
DELTA = 0.125                       # fresh vehicle, fixed schedule: n_phi = 9, λ = 1 -> ϕ_2 = 1 / 8
FRESH_KW = dict(use_fixed_schedule=True, n_phi=9, lam=1.0)
ADAPT_KW = dict(use_fixed_schedule=False, n_phi=30, lam=2.1, tempering_target=0.9)
ADAPT_S = 8.0                       # spread of the adaptive clouds' energies (the root then sits near δ = 0.15)
LOGP_OLD = -20.0
RTOL = 1e-11


def _signed(offsets):
    return [s * b for b in offsets for s in ((1.0,) if b == 0.0 else (1.0, -1.0))]


def fresh_cloud(dB, dS, pw, weights, seed=42, n=N):
    """(loglh, old_loglh, W) of a fixed-schedule fresh case"""
    loglh, W = wr.knob_cloud(n, DELTA, dB, dS, seed, weights)
    old = np.zeros(n) if pw == 0.0 else -40.0 * np.random.default_rng(seed + 1).random(n)
    return loglh, old, W


def adaptive_delta(n=N):
    """the root the reference finds on the adaptive clouds (it does not depend on the offset): ESS(δ) = 0.9 N"""
    loglh, W = wr.knob_cloud(n, 1.0, 0.0, ADAPT_S, 43)
    sched = (np.arange(ADAPT_KW["n_phi"]) / (ADAPT_KW["n_phi"] - 1.0)) ** ADAPT_KW["lam"]
    return wr.solve_phi_ref(loglh, None, W, sched, 2, 0.0, 0.0, ADAPT_KW["tempering_target"], float(n), False)[0]


def adaptive_cloud(dB, delta_star, pw, n=N):
    loglh, W = wr.knob_cloud(n, 1.0, 0.0, ADAPT_S, 43)
    loglh = loglh - dB / delta_star
    old = np.zeros(n) if pw != 0.3 else -40.0 * np.random.default_rng(44).random(n)
    return loglh, old, W


def outlier_cloud(dD, n=N):
    loglh, W = wr.outlier_cloud(n, DELTA, 5.0, dD, 45)
    return loglh, np.zeros(n), W


# rows of weight 0 that hold the cloud's LARGEST energy, δΔ above the live rows' (wr.zero_high_cloud): the reference's ESS is the live rows' alone
ZERO_DD = (0.0, 300.0, 700.0, 709.0, 710.0, 745.0, 800.0, 1e4, 1e6)
ZERO_DS = 0.5                       # δ x spread of the live rows on the fixed schedule: ESS ≈ 0.78 of the live rows
ZERO_ADAPT_S = 2.0                  # spread of the adaptive zero-weight clouds (the root then sits near δ = 0.14)


def zero_cloud(dD, n=N):
    loglh, W = wr.zero_high_cloud(n, DELTA, dD, ZERO_DS / DELTA, 47)
    return loglh, np.zeros(n), W


def zero_adaptive_delta(n=N):
    """the reference's root on the adaptive zero-weight clouds (the rows of weight 0 and the common offset do not enter it)"""
    loglh, W = wr.zero_high_cloud(n, 1.0, 0.0, ZERO_ADAPT_S, 48)
    sched = (np.arange(ADAPT_KW["n_phi"]) / (ADAPT_KW["n_phi"] - 1.0)) ** ADAPT_KW["lam"]
    return wr.solve_phi_ref(loglh, None, W, sched, 2, 0.0, 0.0, ADAPT_KW["tempering_target"], float(n), False)[0]


def zero_adaptive_cloud(dD, delta_star, n=N):
    loglh, W = wr.zero_high_cloud(n, delta_star, dD, ZERO_ADAPT_S, 48)
    return loglh, np.zeros(n), W


def zero_cases(kind="zero"):
    return [dict(kind=kind, dD=dD, thr=0.5) for dD in ZERO_DD]


def fresh_cases(offsets, pws=(0.0, 1.0, 0.3)):
    out = []
    for pw in pws:
        for dS, weights, thr in ((2.0, "ones", 0.5), (5.0, "random", 0.5)):
            for dB in _signed(offsets):
                out.append(dict(kind="fresh", dB=dB, dS=dS, pw=pw, weights=weights, thr=thr))
    return out


def adaptive_cases(offsets, pws=(0.0, 1.0, 0.3)):
    return [dict(kind="adaptive", dB=dB, pw=pw, thr=thr) for pw in pws for thr in (0.5, 0.95) for dB in _signed(offsets)]


def outlier_cases():
    return [dict(kind="outlier", dD=dD, thr=0.5) for dD in OUTLIER_DD]


def input_clouds():
    """Every cloud this file uploads that is made on the host: (name, make) with make() -> (loglh, old, W, ϕ_n, ϕ_{n-1}, prior_weight,
    log_prob_old_data, threshold_ratio).  tests/test_weights_ref_cpu.py checks the reference's ESS on each (>= 50 n_para) and that both
    resample outcomes occur."""
    ds = adaptive_delta()
    for c in fresh_cases(wr.OFFSETS):
        yield ("fresh %r" % c, lambda c=c: fresh_cloud(c["dB"], c["dS"], c["pw"], c["weights"]) + (DELTA, 0.0, c["pw"], LOGP_OLD, c["thr"]))
    for c in adaptive_cases(wr.OFFSETS):
        yield ("adaptive %r" % c, lambda c=c: adaptive_cloud(c["dB"], ds, c["pw"]) + (ds, 0.0, c["pw"], LOGP_OLD, c["thr"]))
    for c in outlier_cases():
        yield ("outlier %r" % c, lambda c=c: outlier_cloud(c["dD"]) + (DELTA, 0.0, 0.0, 0.0, c["thr"]))
    dz = zero_adaptive_delta()
    for c in zero_cases():
        yield ("zero %r" % c, lambda c=c: zero_cloud(c["dD"]) + (DELTA, 0.0, 0.0, 0.0, c["thr"]))
        yield ("zero, adaptive %r" % c, lambda c=c: zero_adaptive_cloud(c["dD"], dz) + (dz, 0.0, 0.0, 0.0, c["thr"]))
    n2 = PATHS["two_chunk_segments"][1]["n"]                            # the two-chunk row's clouds (n_para 10 as well; the wide row: n_para 12 < 50 * 10 / 40)
    ds2 = adaptive_delta(n2)
    for c in fresh_cases(wr.OFFSETS_REDUCED):
        yield ("fresh, n = %d %r" % (n2, c), lambda c=c: fresh_cloud(c["dB"], c["dS"], c["pw"], c["weights"], n=n2) + (DELTA, 0.0, c["pw"], LOGP_OLD, c["thr"]))
    for c in adaptive_cases(wr.OFFSETS_REDUCED):
        yield ("adaptive, n = %d %r" % (n2, c), lambda c=c: adaptive_cloud(c["dB"], ds2, c["pw"], n=n2) + (ds2, 0.0, c["pw"], LOGP_OLD, c["thr"]))


_WORKER = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from smc_jl_amd.host import engine as eng
from smc_jl_amd.host._lib import SMCMIError
from tests import models, weights_ref as wr
from tests import test_gpu_weight_range as T
cfg = json.loads(%(cfg)r)
spec = models.gauss_spec(*cfg.get("spec_args", [10]))
d = len(spec["priors"])
n = cfg.get("n", T.N)
shards = cfg.get("shards", 1)
es = []
for r in range(shards):
    e = Engine(n, d, seed=cfg.get("seed", 5), max_stages=400, store_history=True, n_local=n // shards, gid0=r * (n // shards))
    e.set_model(spec)
    es.append(e)
ds = T.adaptive_delta(n) if any(c["kind"] == "adaptive" for c in cfg["cases"]) else None
dz = T.zero_adaptive_delta(n) if any(c["kind"] == "zero_adaptive" for c in cfg["cases"]) else None

def run(**kw):
    return eng.run_group(es, **kw) if shards > 1 else es[0].run(**kw)
def download():
    return np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
def upload(P):
    for r, e in enumerate(es):
        e.upload_cloud(np.asfortranarray(P[r * (n // shards):(r + 1) * (n // shards)]))
def history(k):
    hs = [e.history(k) for e in es]
    return np.concatenate([h[0] for h in hs], axis=0), np.concatenate([h[1] for h in hs], axis=0)
def relmax(got, want, floor):
    m = np.isfinite(want) & (np.abs(want) > floor)
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0

out = []
for case in cfg["cases"]:
    kw = dict(cfg["kw"]); kw.update(case.get("kw", {}))
    kw["threshold_ratio"] = case.get("thr", 0.5)
    o = dict(case=case, error="", n_para=d)
    out.append(o)
    try:
        for e in es:
            e.init_from_prior()
        kind = case["kind"]
        if kind in ("fresh", "adaptive", "outlier", "zero", "zero_adaptive"):
            k = 2
            P = download()
            if kind == "fresh":
                loglh, old, W = T.fresh_cloud(case["dB"], case["dS"], case["pw"], case["weights"], n=n)
            elif kind == "adaptive":
                loglh, old, W = T.adaptive_cloud(case["dB"], ds, case["pw"], n=n)
            elif kind == "zero":
                loglh, old, W = T.zero_cloud(case["dD"], n=n)
            elif kind == "zero_adaptive":
                loglh, old, W = T.zero_adaptive_cloud(case["dD"], dz, n=n)
            else:
                loglh, old, W = T.outlier_cloud(case["dD"], n=n)
            pw = case.get("pw", 0.0)
            kw["prior_weight"] = pw
            kw["log_prob_old_data"] = T.LOGP_OLD if pw == 0.3 else 0.0
            P[:, d], P[:, d + 2], P[:, d + 4] = loglh, old, W
            upload(P)
            ls0 = dict(j=2, phi_prop=0.0, phi_n=0.0, ess=float(n), resampled_last_period=0, logmdd=0.0)
        else:                                  # continued / lagged: a benign run to stage k - 1; continued: the loglh column moved by B, uploaded
            k = case["k"]
            pw = 0.0
            r = run(stop_after_stage=k - 1, **kw)
            assert r["paused"], r
            ls0 = es[0].get_loop_state()
            P = download()
            if kind == "continued":
                sched = (np.arange(kw["n_phi"]) / (kw["n_phi"] - 1.0)) ** kw["lam"]
                dk = (sched[k - 1] - sched[k - 2]) if kw["use_fixed_schedule"] else case["delta_guess"]
                P[:, d] -= case["dB"] / dk
                upload(P)
        kt = k + case.get("extra", 0)             # extra > 0: stages k .. kt are bracketed and stage kt is compared (see test_adaptive_correction_inside_a_segment...)
        r = run(stop_after_stage=kt, continue_run=kind in ("continued", "lagged"), **kw)
        ls1 = es[0].get_loop_state()
        rec = es[0].stage_records(r["n_stages"])
        w, W = history(r["n_stages"])
        sched = (np.arange(kw["n_phi"]) / (kw["n_phi"] - 1.0)) ** kw["lam"]
        assert float(rec["schedule"][k - 2]) == ls0["phi_n"], (rec["schedule"][k - 2], ls0["phi_n"])
        # the reference, stage after stage: as long as no stage before kt resampled or moved a particle, the cloud of stage s + 1 is the uploaded one
        # with the normalised weights of stage s
        Wc, jj, pp, essp, rl = P[:, d + 4], ls0["j"], ls0["phi_prop"], ls0["ess"], bool(ls0["resampled_last_period"])
        logz_ref, o["phi_rel"], o["cloud_unchanged"] = 0.0, 0.0, True
        for st in range(k, kt + 1):
            phi1, phi0 = float(rec["schedule"][st - 1]), float(rec["schedule"][st - 2])
            if kw["use_fixed_schedule"]:
                o["phi_rel"] = max(o["phi_rel"], abs(phi1 - sched[st - 1]) / sched[st - 1])
            else:                              # the solver's ESS function is compute_ESS: the prior_weight == 0 exponent whatever the correction uses
                want = wr.solve_phi_ref(P[:, d], P[:, d + 2], Wc, sched, jj, pp, phi0, kw["tempering_target"], essp, rl)
                o["phi_rel"] = max(o["phi_rel"], abs(phi1 - want[0]) / want[0])
                o["phi"] = [phi1, want[0]]
                jj, pp, rl = want[2], want[3], False
            ref = wr.correct_ref(P[:, d], P[:, d + 2], Wc, phi1, phi0, pw, kw.get("log_prob_old_data", 0.0), kw["threshold_ratio"])
            logz_ref += ref["logz_inc"]
            if st < kt:
                o["cloud_unchanged"] = o["cloud_unchanged"] and rec["resampled"][st - 1] == 0 and not ref["resample"] and rec["accept_hist"][st - 1] == 0.0
                Wc, essp = ref["W"], float(rec["ess"][st - 1])
        o["cloud_unchanged"] = bool(o["cloud_unchanged"])
        k = kt
        o["ref_ess"] = ref["ess"]
        o["ess"] = float(rec["ess"][k - 1])
        o["ess_rel"] = abs(o["ess"] - ref["ess"]) / ref["ess"] if np.isfinite(o["ess"]) else float("inf")
        o["resampled"] = [int(rec["resampled"][k - 1]), int(ref["resample"])]
        Wk = W[:, k - 1]
        if rec["resampled"][k - 1]:            # W_matrix[:, i] .= 1 at a resample (smc_main.jl:445)
            o["W_rel"] = float(np.max(np.abs(Wk - 1.0)))
        else:
            o["W_rel"] = relmax(Wk, ref["W"], 1e-290)
            o["W_ok"] = bool(np.all(np.abs(Wk - ref["W"]) <= 1e-300 + T.RTOL * np.abs(ref["W"])))
        o["dead_W_zero"] = bool(rec["resampled"][k - 1] or np.all(Wk[P[:, d + 4] == 0.0] == 0.0))      # (a row of weight 0 keeps weight 0)
        wk = w[:, k - 1]
        o["w_rel"] = relmax(wk, ref["w"], 1e-289)
        with np.errstate(invalid="ignore"):
            o["w_ok"] = bool(np.all((wk == ref["w"]) | (np.abs(wk - ref["w"]) <= 1e-300 + T.RTOL * np.abs(ref["w"]))))
        o["logz"] = [ls1["logmdd"] - ls0["logmdd"], logz_ref]
        o["logz_rel"] = abs(o["logz"][0] - o["logz"][1]) / max(abs(o["logz"][1]), 1e-300)
        o["fallback"] = r["shift_fallback_stage"]
        o["segments"] = [r["n_segments"], r["segment_stages"]]
        o["stalls"] = [r["solver_stalls"], r["select_stalls"], r["spec_stalls"], r["segment_timeouts"]]
        o["n_stages"] = r["n_stages"]
    except SMCMIError as ex:
        o["error"] = str(ex)[:200]
print("RESULT " + json.dumps(out))
'''


def _run(cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    code = _WORKER % dict(root=ROOT, cfg=json.dumps(cfg))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    if p.returncode < 0 or p.returncode in (134, 139):              # the worker died of a signal: nothing more is started on that GPU by this file
        pytest.exit("a worker of tests/test_gpu_weight_range.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _check(res, fallback=0, segments=None, need_both=False):
    """Every figure is printed before anything is asserted; then every case is held to the tolerances of the module docstring."""
    bad = []
    for o in res:
        print(json.dumps(o))
    for o in res:
        why = []
        if o["error"]:
            bad.append((o["case"], ["error: " + o["error"]]))
            continue
        assert o["ref_ess"] >= 50 * o["n_para"], o                     # a condition on the input, not on the engine
        if not o["ess_rel"] <= RTOL:
            why.append("ESS %r against %r" % (o["ess"], o["ref_ess"]))
        if o["resampled"][0] != o["resampled"][1]:
            why.append("resample decision %r" % (o["resampled"],))
        if o["resampled"][0]:
            if o["W_rel"] != 0.0:
                why.append("W column not 1 after a resample")
        elif not (o["W_ok"] and o["W_rel"] <= RTOL):
            why.append("normalised weights off by %.3g" % o["W_rel"])
        if not (o["w_ok"] and o["w_rel"] <= RTOL):
            why.append("incremental weights off by %.3g" % o["w_rel"])
        if not o["logz_rel"] <= RTOL:
            why.append("log-MDD increment %r" % (o["logz"],))
        if not o["dead_W_zero"]:
            why.append("a row of weight 0 has weight")
        if not o["phi_rel"] <= (1e-9 if "phi" in o else 1e-14):
            why.append("phi off by %.3g" % o["phi_rel"])
        if fallback is not None and o["fallback"] != fallback:
            why.append("shift_fallback_stage %d" % o["fallback"])
        if not o["cloud_unchanged"]:
            why.append("a stage before the compared one resampled or moved a particle: the vehicle does not hold")
        # run2.hpp run2_impl: a stage that needs no certificate passes (every stage of a fixed schedule; an adaptive call's third stage on) is
        # enqueued WHOLE into a segment - begin, correction, decision, selection, mutation - and only a stall hands it back to the launches
        # (select: the segment left for the selection launches; spec: a predicted ϕ_n did not verify; solver; a time-out).  `segments` = s:
        # at least s stages completed inside segments and nothing stalled, so the compared stage's correction ran in k3_segment.
        if segments and not (o["segments"][1] >= segments and o["stalls"] == [0, 0, 0, 0] and o["fallback"] == 0):
            why.append("the compared stage's correction did not (provably) run inside a segment: segments %r stalls %r fallback %r" % (o["segments"], o["stalls"], o["fallback"]))
        if segments is False and o["segments"][0] != 0:
            why.append("the bracket ran segments: %r" % (o["segments"],))
        if why:
            bad.append((o["case"], why))
    worst = {k: max((o.get(k, 0.0) for o in res if not o["error"]), default=0.0) for k in ("ess_rel", "W_rel", "w_rel", "logz_rel", "phi_rel")}
    print("largest relative errors of %d cases: %r; %d cases fail" % (len(res), worst, len(bad)))
    assert not bad, "%d of %d cases:\n" % (len(bad), len(res)) + "\n".join("%r: %s" % (c, "; ".join(w)) for c, w in bad)
    if need_both:
        assert {o["resampled"][1] for o in res} == {0, 1}


# path -> (environment, worker overrides, stages of a one-stage bracket that must complete inside a segment / False: no segment at all / None: not asserted)
PATHS = {
    "segments": ({}, {}, 1),
    "launches": ({"SMCMI_ENGINE3": "0"}, {}, False),
    "engine1": ({"SMCMI_ENGINE": "1"}, {}, False),
    "large_shard_stage": ({"SMCMI_ENGINE": "2", "SMCMI_E2_REDUCED": "1"}, {}, False),
    "two_shards": ({}, {"shards": 2}, None),
    "two_chunk_segments": ({}, {"n": 150_004}, 1),
    "wide": ({}, {"spec_args": [12]}, None),
}
FULL = ("segments", "launches", "engine1", "two_shards")
CONT_KW = dict(use_fixed_schedule=True, n_phi=40, lam=2.0)
CONT_K = 5


def _offsets(path):
    return wr.OFFSETS if path in FULL else wr.OFFSETS_REDUCED


@pytest.mark.parametrize("path", list(PATHS))
def test_continued_stage_after_an_upload_with_a_common_offset_fixed_schedule(path):
    """Pause -> the loglh column lowered / raised by B -> upload -> one more stage (fixed schedule, k = 5: the lagged shift is in force).
    ESS, W, w and the decision are those of the unmoved cloud, the log-MDD increment moves by -δ_k B, and no fallback was needed: the
    upload forgets the energy maximum the handle had learnt (Begin2::e_seen)."""
    env, over, seg = PATHS[path]
    cases = [dict(kind="continued", k=CONT_K, dB=dB) for dB in _signed(wr.OFFSETS if path == "two_chunk_segments" else _offsets(path))]
    cfg = dict(kw=CONT_KW, cases=cases, **over)
    # inside segments a one-stage continuation is a segment of one stage
    _check(_run(cfg, env), fallback=0, segments=seg)


@pytest.mark.parametrize("path", ["segments", "launches", "engine1", "two_shards", "two_chunk_segments", "large_shard_stage", "wide"])
def test_continued_stage_after_an_upload_with_a_common_offset_adaptive(path):
    env, over, seg = PATHS[path]
    kw = dict(use_fixed_schedule=False, n_phi=40, lam=2.0, tempering_target=0.9)
    # (the offset is sized with a guess of the stage's step, 2e-3: the case's δ B is then nominal; the reference is computed at the ϕ the run took)
    # The first two stages of every adaptive call take certificate passes: their begin, solver passes and correction are engine 2's LAUNCHES on
    # every row (run2.hpp: cert = adaptive && launched < 2) and a segment only enters at the mutation - the [segments] and [two_chunk_segments]
    # rows here measure the launches' correction in the segment rows' geometry, not k3_segment's (that is the test below).
    cases = [dict(kind="continued", k=CONT_K, dB=dB, delta_guess=2e-3) for dB in _signed(_offsets(path))]
    _check(_run(dict(kw=kw, cases=cases, **over), env), fallback=0, segments=False if seg is False else None)


@pytest.mark.parametrize("path", ["segments", "two_chunk_segments"])
def test_adaptive_correction_inside_a_segment_on_a_cloud_with_a_common_offset(path):
    """k3_segment's own adaptive correction (predicted ϕ_n, verified by decide2) is the THIRD stage of a call at the earliest.  Vehicle: pause after
    stage k - 1, RAISE the loglh column by B, upload, continue through stages k .. k + 2 with a threshold no stage reaches.  Every proposal of stages
    k and k + 1 is then rejected (its log-likelihood is the model's, B below the stored ones: MH ratio exp(-ϕ B), ϕ B >= 500), so the cloud that stage
    k + 2 corrects is the uploaded one with the weights of stage k + 1 - known without a download (asserted: no resample, acceptance rate exactly 0).
    Compared: stage k + 2 against the reference chained over the three stages, the log-MDD increment of all three.  Only raised offsets: a lowered
    cloud accepts every proposal and loses its offset in stage k's mutation; under the exact shift of adaptive schedules the sign of B does not
    enter the arithmetic.  Asserted: three stages completed inside segments, nothing stalled."""
    env, over, seg = PATHS[path]
    kw = dict(use_fixed_schedule=False, n_phi=40, lam=2.0, tempering_target=0.9)
    cases = [dict(kind="continued", k=CONT_K, extra=2, dB=-dB, delta_guess=2e-3, thr=0.02) for dB in _offsets(path) if dB >= 300.0]
    _check(_run(dict(kw=kw, cases=cases, **over), env), fallback=0, segments=3)


def _lam_for(G, k, n_phi):
    """λ with δ_k 1e6 = G on the schedule ((i - 1) / (n_phi - 1))^λ: bisection (δ_k falls in λ for k << n_phi)"""
    f = lambda lam: ((k - 1.0) / (n_phi - 1.0)) ** lam - ((k - 2.0) / (n_phi - 1.0)) ** lam
    lo, hi = 1.0, 4.0
    assert f(lo) * 1e6 > G > f(hi) * 1e6, (G, f(lo), f(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) * 1e6 > G else (lo, mid)
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("sign", ["-", ""], ids=["too_high", "too_low"])
@pytest.mark.parametrize("path", ["segments", "launches", "two_shards", "two_chunk_segments"])
def test_a_lagged_shift_off_by_G_leaves_the_sums_right_or_falls_back(path, sign):
    """The lagged shift's own window, with no upload in between: stage k's shift is raised (the underflow side: s2 goes denormal, then 0,
    long before anything is NaN) or lowered (the overflow side) by 1e6, and δ_k 1e6 = G runs through the offsets.  Whatever the run does -
    carry on, or redo the stage with the exact shift (shift_fallback_stage = k) - what it records is the reference's."""
    env, over, seg = PATHS[path]
    k, n_phi = CONT_K, 60
    cases = [dict(kind="lagged", k=k, G=G, kw=dict(lam=_lam_for(G, k, n_phi))) for G in wr.OFFSETS if 300.0 <= G <= 800.0]
    cfg = dict(kw=dict(use_fixed_schedule=True, n_phi=n_phi, lam=2.0), cases=cases, **over)
    res = _run(cfg, dict(env, SMCMI_SHIFT_LAG=sign + str(k)))
    _check(res, fallback=None, segments=None)              # (stage k is the first stage of its call: it does not ride - the riding stage is the test below)
    for o in res:
        assert o["fallback"] in (0, k), o
        if seg:
            assert o["segments"][1] >= 1 and o["stalls"][3] == 0, o
    assert any(o["fallback"] == k for o in res)                     # the development switch did act


@pytest.mark.parametrize("path", list(PATHS))
def test_first_correction_on_knob_clouds_fixed_schedule(path):
    """Fresh vehicle, fixed schedule (δ = 1 / 8), prior_weight 0 / 1 / 0.3: the cloud's largest energy is exact at a run's first stage, so
    prior_weight == 0 holds at every offset; prior_weight != 0 must hold inside the reference's own range (|δ B| <= 700 here: the reference
    normalises before it squares, oracle/smc_oracle.c orc_correct) and, shifted by the generalised energy, beyond it."""
    env, over, seg = PATHS[path]
    cfg = dict(kw=FRESH_KW, cases=fresh_cases(_offsets(path)), **over)
    _check(_run(cfg, env), fallback=0, segments=seg, need_both=True)


@pytest.mark.parametrize("path", list(PATHS))
def test_first_correction_on_knob_clouds_adaptive(path):
    env, over, seg = PATHS[path]
    # (the reference's root is a bisection in extended precision per case: the full offset list at prior_weight 0, the reduced one at 1 and 0.3;
    # the two-chunk row - 150 004 particles per evaluation - at prior_weight 0 alone)
    cases = adaptive_cases(_offsets(path), pws=(0.0,))
    if path != "two_chunk_segments":
        cases += adaptive_cases(wr.OFFSETS_REDUCED, pws=(1.0, 0.3))
    # (an adaptive call's first correction is engine 2's launches on every row - see test_continued_stage...adaptive)
    cfg = dict(kw=ADAPT_KW, cases=cases, **over)
    _check(_run(cfg, env), fallback=0, segments=False if seg is False else None, need_both=True)


@pytest.mark.parametrize("path", list(PATHS))
def test_rows_of_weight_zero_with_the_largest_energy_add_nothing_fixed_schedule(path):
    """Fresh vehicle, δ = 1 / 8: rows of weight 0 whose energy lies δΔ = 0 .. 1e6 above the live cloud's largest (the shift).  The reference's
    exponent is unshifted and finite, 0 x finite = 0: ESS, W, the log-MDD increment are the live rows' alone, those rows keep weight exactly 0,
    their stored incremental weight is exp(δ e) = 1, nothing is NaN (_check: NaN fails every comparison)."""
    env, over, seg = PATHS[path]
    _check(_run(dict(kw=FRESH_KW, cases=zero_cases(), **over), env), fallback=0, segments=seg)


@pytest.mark.parametrize("path", list(PATHS))
def test_rows_of_weight_zero_with_the_largest_energy_add_nothing_adaptive(path):
    """The same on an adaptive call's first correction: the solver's passes see those rows at every candidate ϕ."""
    env, over, seg = PATHS[path]
    _check(_run(dict(kw=ADAPT_KW, cases=zero_cases("zero_adaptive"), **over), env), fallback=0, segments=False if seg is False else None)


# δΔ up to which each path was measured right (engines 2 / 3: decide2 asks s2 >= 1e-290 and returns SMCMI_ERR_NAN_ESS beyond, from δΔ ≈ 340;
# engine 1's post_write only asks isnan(ess): 2e-13 at 360, silently wrong from 365)
OUTLIER_OK = {"segments": 300.0, "launches": 300.0, "engine1": 360.0}
OUTLIER_DD = (0.0, 300.0, 350.0, 360.0, 365.0, 368.0, 370.0, 372.0, 373.0, 380.0)       # (W = 1e-200 = e^-460.5: negligible while δΔ << 460)


@pytest.mark.parametrize("path", list(OUTLIER_OK))
def test_a_negligible_particle_with_the_largest_energy_changes_nothing_in_range(path):
    env, over, seg = PATHS[path]
    cases = [dict(kind="outlier", dD=dD, thr=0.5) for dD in OUTLIER_DD if dD <= OUTLIER_OK[path]]
    _check(_run(dict(kw=FRESH_KW, cases=cases, **over), env), fallback=0, segments=seg)


@pytest.mark.parametrize("path,dD", [(p, dD) for p in OUTLIER_OK for dD in OUTLIER_DD if dD > OUTLIER_OK[p]])
@pytest.mark.xfail(strict=True, reason="the shift is the largest ENERGY of the live cloud, not the largest log-weight: a live particle of weight 1e-200 whose "
                   "energy is Δ above everyone else's pushes the others' squares out of range - engines 2 / 3 return SMCMI_ERR_NAN_ESS from δΔ ≈ 340, "
                   "engine 1 is silently wrong from 365 (DESIGN §5, shift rules)")
def test_a_negligible_particle_with_the_largest_energy_changes_nothing(path, dD):
    env, over, seg = PATHS[path]
    _check(_run(dict(kw=FRESH_KW, cases=[dict(kind="outlier", dD=dD, thr=0.5)], **over), env), fallback=0)


def test_squares_that_underflow_under_a_riding_lagged_shift_switch_the_run_to_exact_shifts():
    """The mirror of tests/test_gpu_segments.py::test_sums_that_overflow_under_the_lagged_shift...: a whole fixed-schedule run in which stage 12 RIDES
    (its correction row is formed right behind stage 11's mutation row, from Post2::e_seen) and SMCMI_SHIFT_LAG=-12 raises that stage's shift
    by 1e6, with λ such that δ_12 1e6 = 372: every W̃ is scaled by e^-372, Σ W̃² is denormal, nothing is NaN - the window in which ESS came out
    twice its value and the run went on.  decide2 sends the stage to the fallback: nothing of it is committed, the run goes on with exact shifts
    (shift_fallback_stage = 12), segments and launches alike, same bits - and is the run exact shifts give from the start: same stages, same
    resample decisions, log-MDD to rounding."""
    from tests.test_gpu_segments import _KEYS, _run as run_whole

    cfg = dict(n=20_000, d=10, seed=3, kw=dict(use_fixed_schedule=True, n_phi=200, lam=_lam_for(372.0, 12, 200)))
    a = run_whole(cfg, {"SMCMI_SHIFT_LAG": "-12"})[0]
    b = run_whole(cfg, {"SMCMI_SHIFT_LAG": "0"})[0]
    c = run_whole(cfg, {"SMCMI_SHIFT_LAG": "-12", "SMCMI_ENGINE3": "0"})[0]
    print(a["shift_fallback_stage"], b["shift_fallback_stage"], c["shift_fallback_stage"], a["n_segments"], a["logmdd_f"], b["logmdd_f"], a["resamples"])
    assert a["shift_fallback_stage"] == 12 and b["shift_fallback_stage"] == 0 and c["shift_fallback_stage"] == 12
    assert a["n_segments"] >= 2 and c["n_segments"] == 0
    assert (a["n_stages"], a["resamples"], a["resampled"]) == (b["n_stages"], b["resamples"], b["resampled"]) and a["n_stages"] == 200
    assert abs(a["logmdd_f"] - b["logmdd_f"]) <= 1e-9 * abs(b["logmdd_f"]), (a["logmdd_f"], b["logmdd_f"])
    for k in _KEYS:
        assert a[k] == c[k], (k, a[k], c[k])


# ------------------------------------------------------------------------------------------------ the stand-alone calls
def _engine(n, d=2):
    from smc_jl_amd import Engine

    spec = dict(priors=[("normal", 0.0, 1.0)] * d, bounds=[(-1e9, 1e9)] * d, fixed=[0] * d, lik=("gauss_iso", [1.0], np.zeros((d, 1)), None), old_lik=None)
    e = Engine(n, d)
    e.set_model(spec)
    return e


@pytest.mark.parametrize("pw", [0.0, 1.0, 0.3])
def test_smcmi_correct_at_any_offset(pw):
    d = 2
    e = _engine(N, d)
    bad = []
    for c in fresh_cases(wr.OFFSETS, pws=(pw,)):
        loglh, old, W = fresh_cloud(c["dB"], c["dS"], pw, c["weights"])
        P = np.zeros((N, d + 5), order="F")
        P[:, d], P[:, d + 2], P[:, d + 4] = loglh, old, W
        e.upload_cloud(P)
        ref = wr.correct_ref(loglh, old, W, 0.5 + DELTA, 0.5, pw, LOGP_OLD)
        assert ref["ess"] >= 50 * N_PARA
        st = e.correct(0.5 + DELTA, 0.5, prior_weight=pw, log_prob_old_data=LOGP_OLD)
        got = e.download_cloud()[:, d + 4]
        m = ref["W"] > 1e-290
        errs = dict(ess=abs(st["ess"] - ref["ess"]) / ref["ess"], logz=abs(st["logz_inc"] - ref["logz_inc"]) / max(abs(ref["logz_inc"]), 1e-300),
                    W=float(np.max(np.abs(got[m] - ref["W"][m]) / ref["W"][m])) if np.all(np.isfinite(got)) else float("inf"))
        print(c, st["ess"], ref["ess"], errs)
        # Σ W w̃ = N exp(log-MDD increment): 0 / inf where it leaves the FP64 range, as the reference's own sum (the exponent carries up to 745 2^-53)
        with np.errstate(over="ignore", under="ignore"):
            su = float(np.asarray(N * np.exp(wr.LD(ref["logz_inc"])), dtype=np.float64))
        errs["sum"] = 0.0 if st["sum_unnorm"] == su else abs(st["sum_unnorm"] - su) / max(su, 1e-300 / RTOL)
        if not (errs["ess"] <= RTOL and errs["W"] <= RTOL and errs["logz"] <= RTOL and errs["sum"] <= RTOL and st["resample"] == ref["resample"]):
            bad.append((c, errs))
    assert not bad, "%d cases:\n" % len(bad) + "\n".join(map(repr, bad))


def test_smcmi_ess_at_and_solve_phi_at_any_offset():
    d = 2
    e = _engine(N, d)
    n_phi = 30
    sched = (np.arange(n_phi) / (n_phi - 1.0)) ** 2.1
    ds = adaptive_delta()
    bad = []
    for dB in _signed(wr.OFFSETS):
        loglh, old, W = adaptive_cloud(dB, ds, 0.0)
        P = np.zeros((N, d + 5), order="F")
        P[:, d], P[:, d + 2], P[:, d + 4] = loglh, old, W
        e.upload_cloud(P)
        phis = np.array([0.5 * ds, ds, 2.0 * ds])
        got = e.ess_at(phis, 0.0)
        want = np.array([wr.ess_ref(loglh, old, W, ph, 0.0) for ph in phis])
        got_phi = e.solve_phi(sched, 2, 0.0, 0.0, 0.9, float(N), False)
        want_phi = wr.solve_phi_ref(loglh, old, W, sched, 2, 0.0, 0.0, 0.9, float(N), False)
        errs = dict(ess=float(np.max(np.abs(got - want) / want)) if np.all(np.isfinite(got)) else float("inf"), phi=abs(got_phi[0] - want_phi[0]) / want_phi[0])
        print(dB, got, want, got_phi, want_phi, errs)
        if not (errs["ess"] <= RTOL and errs["phi"] <= 1e-9 and tuple(got_phi[1:]) == tuple(want_phi[1:])):
            bad.append((dB, errs))
    assert not bad, "%d cases:\n" % len(bad) + "\n".join(map(repr, bad))


# ------------------------------------------------------------------------------------------------ zero-weight structure through every selection
# The selections work on 512-particle chunks, chunk sums and a cum column: chunks whose sum is exactly 0, -Inf likelihoods and all the weight
# at one end of the cloud.  Continued vehicle on the strict build (tests/test_gpu_strict.py): a benign run paused after stage k - 1, the
# weight / loglh columns given the structure, upload, stage k forced to resample (threshold_ratio 0.99); the oracle repeats the stage on the
# same cloud - ancestors from oracle.resample on the REFERENCE's normalised weights (Philox stage k, the handle's seed).
STRICT = os.path.join(ROOT, "smc.jl_amd", "csrc", "libsmcmi_strict.so")
STRUCTURES = ("zero_chunks", "minus_inf_third", "all_weight_last_3pc", "all_weight_first_3pc")

_SELECT = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from oracle import oracle as orc
from smc_jl_amd import Engine
from smc_jl_amd.host import engine as eng
from tests import models, weights_ref as wr
cfg = json.loads(%(cfg)r)
spec = models.gauss_spec(10)
m = models.oracle_model(spec)
n, d, seed, k = cfg["n"], 10, 5, cfg["k"]
shards = cfg.get("shards", 1)
nl = n // shards
es = []
for r in range(shards):
    e = Engine(n, d, seed=seed, max_stages=400, store_history=True, n_local=nl, gid0=r * nl)
    e.set_model(spec)
    es.append(e)
run = lambda **kw: eng.run_group(es, **kw) if shards > 1 else es[0].run(**kw)
out = []
for method in ("systematic", "multinomial"):
    for structure in cfg["structures"]:
        kw = dict(use_fixed_schedule=True, n_phi=200, lam=2.0, resampling_method=method, threshold_ratio=0.99)
        for e in es:
            e.init_from_prior()
        r = run(stop_after_stage=k - 1, **kw)
        assert r["paused"], r
        P = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
        W = P[:, d + 4].copy()
        if structure == "zero_chunks":                       # particles 0 .. 511 and one whole interior 512-chunk
            W[:512] = 0.0; W[512 * 7:512 * 8] = 0.0
        elif structure == "minus_inf_third":                 # a third of the cloud, the last particle and a whole virtual shard's first chunk
            P[::3, d] = -np.inf; P[-1, d] = -np.inf
            v = -(-n // 8) * 3
            P[v:v + 512, d] = -np.inf
        elif structure == "all_weight_last_3pc":
            W[:] = 0.0; W[n - (3 * n) // 100:] = 1.0
        else:
            W[:] = 0.0; W[:(3 * n) // 100] = 1.0
        P[:, d + 4] = W * (n / W.sum())
        for q, e in enumerate(es):
            e.upload_cloud(np.asfortranarray(P[q * nl:(q + 1) * nl]))
        r = run(stop_after_stage=k, continue_run=True, **kw)
        P1 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
        rec = es[0].stage_records(r["n_stages"])
        phi1, phi0, c = float(rec["schedule"][k - 1]), float(rec["schedule"][k - 2]), float(rec["c_hist"][k - 1])
        ref = wr.correct_ref(P[:, d], P[:, d + 2], P[:, d + 4], phi1, phi0, 0.0, 0.0, 0.99)
        idx = orc.resample(ref["W"] / n, method, seed=seed, stage=k)
        Pc = np.asfortranarray(P[idx]); Pc[:, d + 4] = 1.0
        mean, cov = orc.weighted_mean(Pc), orc.weighted_cov(Pc)
        fi = m.free_inds
        mu_f, S_f = mean[fi], (cov[np.ix_(fi, fi)] + cov[np.ix_(fi, fi)].T) / 2
        bf, ba, bp = orc.generate_blocks(len(fi), 1, fi, seed, k)
        want = orc.mutate_cloud(m, Pc, mu_f, S_f, bf, ba, bp, phi1, phi0, c, 1.0, 1, seed, k, n_threads=8)
        same = P1[:, d + 3] == want[:, d + 3]
        live = (P[:, d + 4] > 0) & np.isfinite(P[:, d])
        # rows the oracle's mutation did not move are the ancestors' rows, bit for bit (the cloud may hold a row several times after an earlier
        # resample: contents are compared, not indices); no row of the new cloud is the row of a particle without weight
        stay = want[:, d + 3] == 0.0
        anc_differ = int(np.count_nonzero(np.any(P1[stay][:, :d] != P[idx[stay]][:, :d], axis=1)))
        live = (P[:, d + 4] > 0) & np.isfinite(P[:, d])
        live_keys = {P[i, :d].tobytes() for i in np.flatnonzero(live)}
        dead_keys = {P[i, :d].tobytes() for i in np.flatnonzero(~live)} - live_keys
        from_dead = sum(1 for i in range(n) if P1[i, :d].tobytes() in dead_keys)
        out.append(dict(structure=structure, method=method, ref_ess=ref["ess"], ref_resample=int(ref["resample"]), resampled=int(rec["resampled"][k - 1]),
                        ess_rel=abs(float(rec["ess"][k - 1]) - ref["ess"]) / ref["ess"], flips=int(np.count_nonzero(~same)),
                        max_rel=float(np.max(np.abs(P1[same][:, :d + 3] - want[same][:, :d + 3]) / (1.0 + np.abs(want[same][:, :d + 3])))) if same.any() else 0.0,
                        rows_equal=int(np.count_nonzero(np.all(P1[:, :d] == want[:, :d], axis=1))), unmoved=int(np.count_nonzero(stay)),
                        unmoved_from_dead=int(from_dead), ancestors_differ=anc_differ, idx_dead=int(np.count_nonzero(~live[idx])),
                        w_after=[float(P1[:, d + 4].min()), float(P1[:, d + 4].max())], segments=[r["n_segments"], r["segment_stages"]], n=n))
print("RESULT " + json.dumps(out))
'''

SELECT_PATHS = {
    "segments": ({}, {}, True),
    "segments_leave_for_the_selection": ({"SMCMI_SEG_SELECT": "0"}, {}, None),
    "launches": ({"SMCMI_ENGINE3": "0"}, {}, False),
    "engine1": ({"SMCMI_ENGINE": "1"}, {}, False),
    "two_chunk_segments": ({}, {"n": 150_004}, True),
    "two_shards": ({}, {"shards": 2}, None),
}


@pytest.mark.parametrize("path", list(SELECT_PATHS))
def test_zero_weight_structure_through_the_selection(path):
    assert os.path.exists(STRICT), "libsmcmi_strict.so missing: python __graft_entry__.py builds it"
    env, over, seg = SELECT_PATHS[path]
    cfg = dict(n=N, k=CONT_K, structures=STRUCTURES)
    cfg.update(over)
    code = _SELECT % dict(root=ROOT, cfg=json.dumps(cfg))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SMCMI_LIBRARY=STRICT, **env), capture_output=True, text=True, timeout=1500, cwd=ROOT)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("a worker of tests/test_gpu_weight_range.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for o in res:
        print(json.dumps(o))
    assert len(res) == 2 * len(STRUCTURES)
    for o in res:
        assert o["ref_ess"] >= 50 * N_PARA and o["ref_resample"] == 1, o      # conditions on the input
        assert o["resampled"] == 1 and o["ess_rel"] <= RTOL, o
        assert o["unmoved_from_dead"] == 0 and o["idx_dead"] == 0 and o["ancestors_differ"] == 0, o    # no ancestor has zero weight; the oracle's ancestors
        # strict build: the oracle's stage, decision for decision; values of the moved rows as tests/test_gpu_strict.py at its 30 000 particles, and
        # in proportion beyond (the oracle totals the moments one particle after the other: its own rounding grows with N u).  Measured: 1.7e-12 at
        # 20 480 particles, 1.6e-11 at 150 004.
        assert o["flips"] == 0 and o["max_rel"] < 1e-11 * max(1.0, o["n"] / 30000.0), o
        assert o["unmoved"] >= o["n"] // 4 and o["w_after"] == [1.0, 1.0], o
        if seg is True:
            assert o["segments"][1] >= 1, o
        if seg is False:
            assert o["segments"][0] == 0, o
