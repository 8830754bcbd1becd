"""The two chip-wide hand-overs of a segment stage (csrc/stage3.hpp): which code fetches the shard totals (k3_totals in the two-hand-over
one-handle kernels, gather_totals / gather_totals_pair elsewhere), who totals a shard's rows (a gatherer block, or the workers themselves
where a virtual shard is one or two blocks) and where the begin's schedule window is filled (behind the stage's post2, under the hand-over)
are matters of WHEN a word is looked at and WHICH code looks - never of an operation on a value.  So every path must leave the bits a run of
engine 2's launches leaves (SMCMI_ENGINE3=0): schedule, ESS, c, acceptance, resample flags, cloud, both histories, log-MDD.

The shapes are the smallest that reach each path: 8 virtual shards of one, two or three 512-particle rows, an uneven last shard, 30-40
stages with at least one resample inside the segment.  Switches are read once per process: every run is a child process."""
import hashlib  # noqa: F401  (the worker's)
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import json, sys, hashlib
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from tests import models
cfg = json.loads(%(cfg)r)
e = Engine(cfg["n"], cfg["d"], seed=cfg["seed"], max_stages=400, store_history=True)
e.set_model(models.gauss_spec(cfg["d"]))
e.init_from_prior()
r = e.run(**cfg["kw"])
rec = e.stage_records(r["n_stages"])
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
w, W = e.history(r["n_stages"])
print("RESULT " + json.dumps(dict(
    n_stages=r["n_stages"], resamples=r["resamples"], logmdd=float(r["logmdd"]).hex(), schedule=h(rec["schedule"]), ess=h(rec["ess"]),
    c_hist=h(rec["c_hist"]), accept_hist=h(rec["accept_hist"]), resampled=h(rec["resampled"]), cloud=h(e.download_cloud()), w=h(w), W=h(W),
    flags="".join(str(int(x)) for x in rec["resampled"]), n_segments=r["n_segments"], segment_stages=r["segment_stages"],
    segment_blocks=r["segment_blocks"], segment_state=r["segment_state"], segment_timeouts=r["segment_timeouts"],
    stalls=[r["solver_stalls"], r["select_stalls"], r["spec_stalls"]])))
'''

_KEYS = ("n_stages", "resamples", "logmdd", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud", "w", "W")


def _run(cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    code = _WORKER % dict(root=ROOT, cfg=json.dumps(cfg))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _pair(cfg):
    """The job with segments and as launches: the same bits; the segments ran, none timed out, the handle keeps its segment geometry."""
    seg = _run(cfg)
    ref = _run(cfg, {"SMCMI_ENGINE3": "0"})
    print(cfg, "stages", seg["n_stages"], "resampled", seg["flags"], "segments", seg["n_segments"], "segment stages", seg["segment_stages"],
          "blocks", seg["segment_blocks"], "stalls", seg["stalls"])
    assert ref["n_segments"] == 0
    assert seg["n_segments"] > 0 and seg["segment_timeouts"] == 0 and seg["segment_state"] == 1, seg
    for k in _KEYS:
        assert seg[k] == ref[k], (k, seg[k], ref[k], seg["stalls"], ref["stalls"])
    return seg


def _adaptive(d, **more):
    # (30-40 stages: the 3-parameter Gaussian at a tempering target of 0.88, the 10-parameter one at 0.78)
    return dict(use_fixed_schedule=False, tempering_target=0.88 if d == 3 else 0.78, **more)


@pytest.mark.parametrize("n,blocks", [(12_288, 8 * 3 + 8), (12_301, 25 + 1), (33_001, 8 * 9 + 8)], ids=["even", "n12301", "uneven_last_shard"])
@pytest.mark.parametrize("d", [3, 10])
def test_gatherers_and_one_canonical_group(n, blocks, d):
    """One gatherer per virtual shard sweeps the shard's rows, every block fetches the V totals - the headline's path (k3_segment<D, true,
    false>: k3_totals, the window filled ahead).  12 288: 8 shards x 3 rows.  12 301 has no divisor among 8 / 4 / 2 and few enough rows for ONE
    virtual shard (csrc/route.hpp make_geo2): 25 rows - the headline's count per shard, the last one partly filled - and one total, k3_totals'
    loop for V other than 8.  33 001: too many rows for one shard, so 8 shards of ceil(n / 8) particles, the last one shorter (make_geo2_uneven):
    9 rows each, the last shard's last row partly filled."""
    seg = _pair(dict(n=n, d=d, seed=3, kw=_adaptive(d)))
    assert seg["segment_blocks"] == blocks, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["n_stages"] >= 12 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


@pytest.mark.parametrize("n,rows", [(4_096, 1), (8_192, 2)], ids=["one_row_per_shard", "two_rows_per_shard"])
def test_workers_take_the_rows_themselves(n, rows):
    """A virtual shard of one block: its total is its only row, every worker fetches the 8 rows (k3_totals on the row tables); of two blocks:
    gather_totals<2> totals the two rows as a gatherer would.  No gatherer is launched."""
    seg = _pair(dict(n=n, d=3, seed=5, kw=_adaptive(3)))
    assert seg["segment_blocks"] == 8 * rows, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


@pytest.mark.parametrize("alpha", [1.0, 0.9], ids=["alpha1", "mixture"])
def test_riding_stages_fetch_both_tables_at_once(alpha):
    """Fixed schedules: one hand-over per stage, gather_totals_pair (the riding kernels keep the text they had)."""
    seg = _pair(dict(n=12_288, d=3, seed=7, kw=dict(use_fixed_schedule=True, n_phi=40, alpha=alpha)))
    assert seg["n_stages"] == 40 and seg["resamples"] >= 1 and seg["segment_blocks"] == 8 * 3 + 8


def test_mixture_proposals_on_two_hand_overs():
    """k3_segment<3, false, false>: the mixture kernel takes the same hand-over code as the α = 1 kernel."""
    seg = _pair(dict(n=12_288, d=3, seed=9, kw=_adaptive(3, alpha=0.9)))
    assert seg["resamples"] >= 1 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


def test_the_schedule_window_filled_ahead_survives_a_selection():
    """A resampling threshold above the tempering target: the run resamples at stage after stage, inside the segment.  The window of the
    proposed schedule that stage n + 1's begin walks is filled behind stage n's post2; stage n's selection took the same LDS words as
    scratch just before that post2, stage n + 1's takes them right behind the begin that read them."""
    seg = _pair(dict(n=12_288, d=3, seed=11, kw=dict(use_fixed_schedule=False, tempering_target=0.88, threshold_ratio=0.92)))
    assert "11" in seg["flags"] and seg["stalls"][1] == 0, seg["flags"]
    assert seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
