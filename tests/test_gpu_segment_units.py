"""The two units of the α = 1, two-hand-over, one-handle, one-chunk segment kernel (csrc/stage3.hpp SMCMI_K3_RUN, csrc/launch2.hpp
launch_k3_segment): the DEFAULT-RUN unit is the general kernel's text with three things fixed at compile time that the default run of one
cloud of more than 8 192 particles never varies - no development stamps, gatherer geometry only, one random block - and is
launched exactly when a launch is that; everything else takes the GENERAL unit.  The units differ in text no such launch reaches, never in
an operation on a value, so the default dispatch and a run forced onto the general unit (SMCMI_K3_GENERAL=1) must leave the same bits:
cloud, stage records, log-MDD, both histories.  (The ancestors of a whole-loop run are not host-visible; the resampled cloud is a copy of
the rows they name.)  smcmi_segment_unit says which unit the last segment launch took.

Every shape is the smallest at which the dispatch or the specialised text can go wrong; 30-60 stages, at least two of which resample
inside the segment.  Switches are read once per process: every run is a child process."""
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
spec = getattr(models, cfg.get("spec", "gauss_spec"))(*cfg.get("spec_args", [cfg["d"]]))
history = cfg.get("history", True)
e = Engine(cfg["n"], cfg["d"], seed=cfg["seed"], max_stages=400, store_history=history)
e.set_model(spec)
if cfg.get("old_run"):                      # a tempered update: the cloud of an estimation on the old data is the starting point
    e0 = Engine(cfg["n"], cfg["d"], seed=cfg["seed"] + 1, max_stages=200, store_history=False)
    e0.set_model(getattr(models, cfg["spec"])(*cfg["old_run"]["spec_args"])); e0.init_from_prior()
    e0.run(**cfg["old_run"]["kw"])
    P_old = e0.download_cloud(); e0.close()
    e.upload_cloud(P_old); e.initialize_likelihoods()
else:
    e.init_from_prior()
kw = dict(cfg["kw"]); stop = kw.pop("pause_at", 0)
units = []
if stop:
    r = e.run(stop_after_stage=stop, **kw); assert r["paused"]
    units.append(e.segment_unit())
    r = e.run(continue_run=True, **kw)
else:
    r = e.run(**kw)
units.append(e.segment_unit())
rec = e.stage_records(r["n_stages"])
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
o = dict(n_stages=r["n_stages"], resamples=r["resamples"], logmdd=float(r["logmdd"]).hex(), c=float(r["c"]).hex(), accept=float(r["accept"]).hex(),
         schedule=h(rec["schedule"]), ess=h(rec["ess"]), c_hist=h(rec["c_hist"]), accept_hist=h(rec["accept_hist"]), resampled=h(rec["resampled"]),
         cloud=h(e.download_cloud()), flags="".join(str(int(x)) for x in rec["resampled"]), phi_last=float(rec["schedule"][-1]),
         n_segments=r["n_segments"], segment_stages=r["segment_stages"], segment_blocks=r["segment_blocks"], segment_state=r["segment_state"],
         segment_timeouts=r["segment_timeouts"], stalls=[r["solver_stalls"], r["select_stalls"], r["spec_stalls"]], units=units)
if history:
    w, W = e.history(r["n_stages"])
    o["w"], o["W"] = h(w), h(W)
print("RESULT " + json.dumps(o))
'''

_KEYS = ("n_stages", "resamples", "logmdd", "c", "accept", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud", "w", "W")


def _run(cfg, env_extra=None):
    env = dict(os.environ)
    for k in ("SMCMI_K3_GENERAL", "SMCMI_PROF2"):
        env.pop(k, None)
    env.update(env_extra or {})
    code = _WORKER % dict(root=ROOT, cfg=json.dumps(cfg))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _same_bits(a, b):
    for k in _KEYS:
        if k in a or k in b:
            assert a[k] == b[k], (k, a[k], b[k], a["stalls"], b["stalls"])


def _pair(cfg, unit, env=None, min_inside=2):
    """The default dispatch against the forced general unit: the same bits; the default dispatch took `unit` in its last segment launch(es),
    the forced run the general unit; the segments ran and none timed out."""
    a = _run(cfg, env)
    g = _run(cfg, dict(env or {}, SMCMI_K3_GENERAL="1"))
    print(cfg, env, "stages", a["n_stages"], "resampled", a["flags"], "segments", a["n_segments"], "segment stages", a["segment_stages"],
          "blocks", a["segment_blocks"], "stalls", a["stalls"], "units", a["units"], g["units"])
    for r in (a, g):
        assert r["n_segments"] > 0 and r["segment_timeouts"] == 0 and r["segment_state"] == 1, r
    assert a["units"] == [unit] * len(a["units"]), a["units"]
    assert g["units"] == [GENERAL] * len(g["units"]), g["units"]
    _same_bits(a, g)
    assert a["n_segments"] == g["n_segments"] and a["segment_stages"] == g["segment_stages"] and a["stalls"] == g["stalls"]
    assert a["phi_last"] == 1.0
    # (a stage that resampled without a select stall did so inside a segment)
    assert a["flags"][1:].count("1") - a["stalls"][1] >= min_inside, (a["flags"], a["stalls"])
    return a


def _adaptive(d, **more):
    # (30-40 stages: the 3-parameter Gaussian at a tempering target of 0.96, the 10-parameter one at 0.86; the threshold above them: nearly
    # every stage resamples, inside the segment)
    return dict(use_fixed_schedule=False, tempering_target=0.96 if d == 3 else 0.86, threshold_ratio=0.98 if d == 3 else 0.95, **more)


# (segment blocks: V * rows workers + V gatherers where gatherers are launched - csrc/route.hpp plan_run, launch2.hpp)
@pytest.mark.parametrize("n,blocks,unit", [(12_288, 8 * 3 + 8, RUN), (8_192, 8 * 2, GENERAL), (4_096, 8 * 1, GENERAL), (12_289, None, RUN),
                                           (67_588, 4 * 34 + 4, RUN)],
                         ids=["n12288_smallest_default_run", "n8192_rows_two", "n4096_rows_direct", "n12289_uneven", "n67588_gather_wide"])
@pytest.mark.parametrize("d", [3, 10])
def test_geometry_decides_the_unit_and_never_the_bits(n, blocks, unit, d):
    """12 288 = 8 virtual shards of 3 blocks: the smallest cloud with gatherers, hence the smallest the default-run unit serves.  8 192 / 4 096:
    two / one block per shard - the workers take each other's rows (rows_two / rows_direct), text the default-run unit does not have: the
    general unit.  12 289: the uneven geometry (a last shard one particle longer).  67 588 = 4 x 16 897: 34 rows per shard, beyond k3_gather's
    32 (k3_gather_wide) and more than the workers' LDS allocation holds of them (the launcher's gather_bytes)."""
    a = _pair(dict(n=n, d=d, seed=3, kw=_adaptive(d)), unit)
    if blocks is not None:
        assert a["segment_blocks"] == blocks, a["segment_blocks"]
    assert 30 <= a["n_stages"] <= 60 and a["segment_stages"] >= (a["n_stages"] - 1) // 2


def test_one_parameter_on_a_fixed_schedule_with_exact_shifts():
    """n_para 1 (the generic Cholesky with one row; an adaptive schedule's predictions rarely verify there, so a fixed one: every stage runs
    inside segments).  Exact shifts (SMCMI_SHIFT_LAG=0): two hand-overs per stage - this kernel, not the riding one."""
    a = _pair(dict(n=12_288, d=1, seed=5, kw=dict(use_fixed_schedule=True, n_phi=40, threshold_ratio=0.9)), RUN, {"SMCMI_SHIFT_LAG": "0"})
    assert a["n_stages"] == 40


@pytest.mark.parametrize("method", ["multinomial"])
@pytest.mark.parametrize("history", [True, False], ids=["history", "no_history"])
def test_multinomial_resampling_and_history_off(method, history):
    """(Systematic resampling with history: every other case.)  Without history the kernel's two history stores are skipped - a run-time
    branch both units have."""
    _pair(dict(n=12_288, d=10, seed=7, history=history, kw=_adaptive(10, resampling_method=method)), RUN)


def test_systematic_resampling_without_history():
    _pair(dict(n=12_289, d=3, seed=8, history=False, kw=_adaptive(3)), RUN)


def test_two_random_blocks_take_the_general_unit_and_the_bits_of_the_launches():
    """n_blocks = 2: the several-blocks proposal and the MH step's block loop, which the default-run unit does not have.  The general unit is
    the kernel as it was: the bits of engine 2's launches (SMCMI_ENGINE3=0), as before."""
    cfg = dict(n=12_288, d=10, seed=9, kw=_adaptive(10, n_blocks=2))
    a = _pair(cfg, GENERAL)
    ref = _run(cfg, {"SMCMI_ENGINE3": "0"})
    assert ref["n_segments"] == 0 and ref["units"] == [NONE]
    _same_bits(a, ref)


def test_a_tempered_update_stays_on_the_default_run_unit():
    """A tempered update (prior weight 0.5, an old-data likelihood beside the new one: RunParams::pw != 1 in the correction and the MH
    step's target) is a matter of run-time values in both units."""
    cfg = dict(n=16_000, d=9, seed=8, spec="linmodel_spec", spec_args=[100, 60], old_run=dict(spec_args=[60], kw=dict(n_phi=100, lam=2.0)),
               kw=dict(use_fixed_schedule=False, tempering_target=0.995, threshold_ratio=0.999, prior_weight=0.5, log_prob_old_data=-300.0))
    _pair(cfg, RUN)


def test_a_launch_that_enters_at_a_mutation():
    """SMCMI_NO_SELECT_PREDICT=2 with SMCMI_SEG_SELECT=0: every resample stage is met inside a segment, which leaves with nothing of the stage
    committed; the host runs correction and selection as launches and a segment ENTERS at the stage's mutation (Seg3Args::enter_mut: the
    prologue's other branch, rs0, v_entered).  Nothing resamples inside a segment here."""
    cfg = dict(n=12_288, d=10, seed=13, kw=dict(use_fixed_schedule=False, tempering_target=0.8))
    env = {"SMCMI_NO_SELECT_PREDICT": "2", "SMCMI_SEG_SELECT": "0"}
    a = _pair(cfg, RUN, env, min_inside=-10**9)
    assert a["resamples"] >= 2 and a["stalls"][1] >= a["resamples"] - 1 and a["n_segments"] > a["resamples"]
    ref = _run(cfg, dict(env, SMCMI_ENGINE3="0"))
    _same_bits(a, ref)


def test_a_paused_and_continued_run_on_a_fixed_schedule_with_exact_shifts():
    """stop_after_stage = 15 of 40: the first call's segment ends at the pause (begin2_wave's exit), the second call's begins from the loop
    state the handle holds and ends at ϕ = 1 inside the segment.  Both calls' last launches took the unit under test."""
    a = _pair(dict(n=12_288, d=3, seed=21, kw=dict(use_fixed_schedule=True, n_phi=40, threshold_ratio=0.9, pause_at=15)), RUN, {"SMCMI_SHIFT_LAG": "0"})
    assert a["n_stages"] == 40 and len(a["units"]) == 2


def test_a_profiled_run_takes_the_general_unit_and_leaves_the_same_bits():
    """SMCMI_PROF2=<stage>: the launch that holds the profiled stage carries the stamp pointers, which the default-run unit has no text for -
    it takes the general unit (here the run's only segment launch: a fixed schedule with exact shifts), and the stamps touch no result."""
    cfg = dict(n=12_288, d=10, seed=23, kw=dict(use_fixed_schedule=True, n_phi=40, threshold_ratio=0.9))
    a = _run(cfg, {"SMCMI_SHIFT_LAG": "0"})
    p = _run(cfg, {"SMCMI_SHIFT_LAG": "0", "SMCMI_PROF2": "20"})
    print("segments", a["n_segments"], p["n_segments"], "units", a["units"], p["units"], "resampled", a["flags"])
    assert a["units"] == [RUN] and a["n_segments"] >= 1
    assert p["n_segments"] == 1 and p["units"] == [GENERAL], (p["n_segments"], p["units"])
    _same_bits(a, p)
