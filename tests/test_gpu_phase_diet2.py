"""The default-run unit of the segment kernel (csrc/stage3.hpp SMCMI_K3_RUN) with the mutation row's energy maximum taken through lane
swaps and DPP moves (K3H_EMAX: csrc/kernels.hpp wave_max_swap, csrc/stage2.hpp k2_mut_row_f SWAPMAX), not six LDS-crossbar rounds.

No operation on a live value and no order of operations changes, so a job must leave the same bits three ways: by the default dispatch (the
default-run unit), as engine 2's launches (SMCMI_ENGINE3=0) and forced onto the general unit (SMCMI_K3_GENERAL=1), which keeps the rounds:
schedule, ESS, c, acceptance, resample flags, cloud, both histories, log-MDD.  The segments ran, none timed out, and smcmi_segment_unit
reports the default-run unit for the default dispatch.

Shapes: the smallest clouds the unit takes (more than two rows per shard) with dead lanes of each kind; adaptive schedules of 30-40 stages
with at least one resample inside the segment.  Switches are read once per process: every run is a child process.

Not here: a likelihood that is -Inf on part of the prior's support as a MODEL - no likelihood family the default-run unit evaluates is -Inf
on a region of moderate size (gauss_iso only where the squared distance overflows).  The rows of weight 0 and the -Inf energies such a model
gives are put into the starting cloud instead, on a fixed schedule (test_neg_inf_likelihoods_and_rows_of_weight_zero)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RUN, GENERAL = 0, 1, 2          # include/smcmi.h SMCMI_SEG_UNIT_*

_WORKER = r'''
import json, sys, hashlib
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from tests import models
cfg = json.loads(%(cfg)r)
d = cfg["d"]
spec = models.gauss_spec(d, cfg.get("sigma", 0.25), cfg.get("prior_sd", 5.0))
if "bounds" in cfg:
    spec["bounds"] = [tuple(b) for b in cfg["bounds"]]
if "fixed" in cfg:
    spec["fixed"] = cfg["fixed"]
e = Engine(cfg["n"], d, seed=cfg["seed"], max_stages=400, store_history=True)
e.set_model(spec)
e.init_from_prior()
n_neg = 0
if cfg.get("neg_inf"):          # the likelihood is -Inf where θ_0 > neg_inf: those rows get weight 0 at the first correction and hold energy -Inf
    P = e.download_cloud()
    rows = P[:, 0] > cfg["neg_inf"]
    P[rows, d] = -np.inf
    n_neg = int(rows.sum())
    e.upload_cloud(P)
r = e.run(**cfg["kw"])
unit = e.segment_unit()
rec = e.stage_records(r["n_stages"])
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
w, W = e.history(r["n_stages"])
P = e.download_cloud()
print("RESULT " + json.dumps(dict(
    n_stages=r["n_stages"], resamples=r["resamples"], logmdd=float(r["logmdd"]).hex(), c=float(r["c"]).hex(), accept=float(r["accept"]).hex(),
    schedule=h(rec["schedule"]), ess=h(rec["ess"]), c_hist=h(rec["c_hist"]), accept_hist=h(rec["accept_hist"]), resampled=h(rec["resampled"]),
    cloud=h(P), w=h(w), W=h(W), flags="".join(str(int(x)) for x in rec["resampled"]), accepts=[float(a) for a in rec["accept_hist"]],
    theta_min=[float(x) for x in P[:, :d].min(axis=0)], theta_max=[float(x) for x in P[:, :d].max(axis=0)], n_neg=n_neg,
    zero_weights=int((W == 0.0).sum()), n_segments=r["n_segments"], segment_stages=r["segment_stages"], segment_blocks=r["segment_blocks"],
    segment_state=r["segment_state"], segment_timeouts=r["segment_timeouts"], stalls=[r["solver_stalls"], r["select_stalls"], r["spec_stalls"]],
    unit=unit)))
'''

_KEYS = ("n_stages", "resamples", "logmdd", "c", "accept", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud", "w", "W")


def _run(cfg, env_extra=None):
    env = dict(os.environ)
    for k in ("SMCMI_K3_GENERAL", "SMCMI_PROF2", "SMCMI_ENGINE3"):
        env.pop(k, None)
    env.update(env_extra or {})
    code = _WORKER % dict(root=ROOT, cfg=json.dumps(cfg))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _three_ways(cfg, min_stages=12, env=None):
    """The default dispatch, engine 2's launches and the forced general unit: the same bits."""
    seg = _run(cfg, env)
    ref = _run(cfg, dict(env or {}, SMCMI_ENGINE3="0"))
    gen = _run(cfg, dict(env or {}, SMCMI_K3_GENERAL="1"))
    print(cfg, "stages", seg["n_stages"], "resampled", seg["flags"], "segments", seg["n_segments"], "segment stages", seg["segment_stages"],
          "blocks", seg["segment_blocks"], "stalls", seg["stalls"], "units", seg["unit"], ref["unit"], gen["unit"])
    assert ref["n_segments"] == 0 and ref["unit"] == NONE, (ref["n_segments"], ref["unit"])
    for r in (seg, gen):
        assert r["n_segments"] > 0 and r["segment_timeouts"] == 0 and r["segment_state"] == 1, r
    assert seg["unit"] == RUN and gen["unit"] == GENERAL, (seg["unit"], gen["unit"])
    for k in _KEYS:
        assert seg[k] == ref[k], ("launches", k, seg[k], ref[k], seg["stalls"], ref["stalls"])
        assert seg[k] == gen[k], ("general unit", k, seg[k], gen[k], seg["stalls"], gen["stalls"])
    assert seg["n_stages"] >= min_stages and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
    # (a stage that resampled without a select stall did so inside a segment)
    assert seg["flags"][1:].count("1") - seg["stalls"][1] >= 1, (seg["flags"], seg["stalls"])
    return seg


# (30-40 stages: the Gaussian of d parameters at these tempering targets)
_TARGET = {1: 0.96, 3: 0.88, 4: 0.87, 7: 0.82, 10: 0.78}


def _adaptive(d, **more):
    return dict(use_fixed_schedule=False, tempering_target=_TARGET[d], **more)


@pytest.mark.parametrize("n", [12_292, 12_548, 14_332], ids=["one_live_lane", "wavefront_with_one_live_lane", "one_dead_lane"])
@pytest.mark.parametrize("d", [1, 4, 7, 10, 3])
def test_dead_lanes_of_each_kind(n, d):
    """n_para 1, 4, 7, 10, 3: the correction row's 5, 17, 38, 68 and 12 sums.  12 292 = 4 x 3 073: every shard's
    last block holds ONE particle - seven of its wavefronts are wholly dead, the energy maximum of each is -Inf.  12 548 = 4 x 3 137: 65
    live lanes, wavefront 1 has one.  14 332 = 4 x 3 583: one dead lane, in the last wavefront."""
    seg = _three_ways(dict(n=n, d=d, seed=3, kw=_adaptive(d)))
    assert seg["segment_blocks"] == 4 * 7 + 4, seg["segment_blocks"]


def test_tight_bounds_refuse_proposals_on_either_side():
    """Bounds a few posterior standard deviations (0.25) wide around the likelihood's centre, off-centre, on parameters 0, 4, 8 and 9 of ten:
    proposals leave them on either side throughout the run, the others never come near theirs."""
    d = 10
    m = [-1.0 + 2.0 * j / (d - 1) for j in range(d)]
    bounds = [(-1e5, 1e5)] * d
    bounds[0] = (m[0] - 0.1, m[0] + 0.4)
    bounds[4] = (m[4] - 0.3, m[4] + 0.15)
    bounds[8] = (m[8] - 0.2, m[8] + 0.2)
    bounds[9] = (m[9] - 0.5, m[9] + 0.05)
    seg = _three_ways(dict(n=12_292, d=d, seed=11, prior_sd=1.0, bounds=bounds, kw=dict(use_fixed_schedule=False, tempering_target=0.92)))
    # the final cloud reaches within a tenth of a posterior standard deviation of both bounds of every bounded parameter, and stays inside
    for k in (0, 4, 8, 9):
        lo, hi = bounds[k]
        assert lo <= seg["theta_min"][k] <= lo + 0.025 and hi - 0.025 <= seg["theta_max"][k] <= hi, (k, bounds[k], seg["theta_min"][k], seg["theta_max"][k])


def test_one_fixed_parameter():
    """Parameter 2 of seven is fixed: n_free = 6 < n_para, a particle's acceptance value is a multiple of 1 / 6."""
    seg = _three_ways(dict(n=12_548, d=7, seed=13, fixed=[0, 0, 1, 0, 0, 0, 0], kw=_adaptive(7)))
    assert seg["theta_min"][2] == seg["theta_max"][2]


def test_neg_inf_likelihoods_and_rows_of_weight_zero():
    """A starting cloud whose likelihood is -Inf wherever θ_0 > 6.5 = 1.3 prior standard deviations (a tenth of the prior draws): the first
    correction gives those rows weight 0 - they stay in the cloud, weight 0 in the rows' sums and energy -Inf in the mutation row's maximum,
    until a stage resamples.  On a FIXED schedule with exact shifts (SMCMI_SHIFT_LAG=0 in all three runs: two hand-overs per stage, this
    kernel): the adaptive solver refuses such a cloud at stage 1 under either engine (its bracket's lower end is 0 x -Inf)."""
    seg = _three_ways(dict(n=12_292, d=10, seed=17, neg_inf=6.5, kw=dict(use_fixed_schedule=True, n_phi=40)), env={"SMCMI_SHIFT_LAG": "0"})
    assert seg["n_stages"] == 40
    assert 0.05 * 12_292 < seg["n_neg"] < 0.15 * 12_292 and seg["zero_weights"] >= seg["n_neg"], (seg["n_neg"], seg["zero_weights"])


def test_sigma_that_is_no_power_of_two():
    _three_ways(dict(n=14_332, d=10, seed=19, sigma=0.3, kw=_adaptive(10)))


def test_a_stage_that_accepts_nothing():
    """An initial step size of 1e7: the first mutations' proposals all leave the bounds (±1e5) - acceptance exactly 0."""
    seg = _three_ways(dict(n=12_292, d=4, seed=23, kw=_adaptive(4, c=1e7)))
    print("acceptance of the first stages", seg["accepts"][:5])
    assert min(seg["accepts"][1:4]) == 0.0, seg["accepts"][:5]


def test_a_stage_that_accepts_everything():
    """An initial step size of 1e-9: a proposal changes the log-posterior by ~1e-7 at the most, the first mutation refuses (nearly) none."""
    seg = _three_ways(dict(n=12_292, d=4, seed=29, kw=_adaptive(4, c=1e-9)))
    print("acceptance of the first stages", seg["accepts"][:5])
    assert max(seg["accepts"][1:4]) > 0.999, seg["accepts"][:5]
