"""The per-particle phases of the two-hand-over, one-handle, one-chunk segment kernels (csrc/stage3.hpp, SMCMI_K3HO bits 16 and up) with
lanes that hold no particle: the correction row's sums are formed without the `live` select (a dead lane's operands are +0.0, so its sums
are +0.0 - csrc/stage2.hpp k2_cm_row_one DEADZERO), and the `live` mask is formed anew from a flag in a vector register at each use
(K3H_LIVE).  No operation on a live value moves, so every shape must leave the bits a run of
engine 2's launches leaves (SMCMI_ENGINE3=0): schedule, ESS, c, acceptance, resample flags, cloud, both histories, log-MDD.

The shapes are the smallest clouds in which a worker's block (512 lanes, 8 wavefronts) has dead lanes of each kind, at n_para 1, 3 and 10 (the
correction row has 5, 12 and 68 sums).  30-40 adaptive stages with at least one resample inside the segment.  Switches are read once per
process: every run is a child process."""
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
e = Engine(cfg["n"], cfg["d"], seed=cfg["seed"], max_stages=400, store_history=cfg["history"])
e.set_model(models.gauss_spec(cfg["d"]))
e.init_from_prior()
r = e.run(**cfg["kw"])
rec = e.stage_records(r["n_stages"])
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
w, W = e.history(r["n_stages"]) if cfg["history"] else (np.zeros(0), np.zeros(0))
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


def _pair(cfg, env_both=None):
    """The job with segments and as launches: the same bits; the segments ran, none timed out, the handle keeps its segment geometry."""
    cfg = {"history": True, **cfg}
    seg = _run(cfg, env_both)
    ref = _run(cfg, dict(env_both or {}, SMCMI_ENGINE3="0"))
    print(cfg, "stages", seg["n_stages"], "resampled", seg["flags"], "segments", seg["n_segments"], "segment stages", seg["segment_stages"],
          "blocks", seg["segment_blocks"], "stalls", seg["stalls"])
    assert ref["n_segments"] == 0
    assert seg["n_segments"] > 0 and seg["segment_timeouts"] == 0 and seg["segment_state"] == 1, seg
    for k in _KEYS:
        assert seg[k] == ref[k], (k, seg[k], ref[k], seg["stalls"], ref["stalls"])
    return seg


# (30-40 stages: the Gaussian of 1 / 3 / 10 parameters at these tempering targets)
_TARGET = {1: 0.96, 3: 0.88, 10: 0.78}


def _adaptive(d, **more):
    return dict(use_fixed_schedule=False, tempering_target=_TARGET[d], **more)


# (segment blocks: V * rows workers + V gatherers; where a shard has one or two rows the workers take the rows themselves: csrc/route.hpp plan_run)
_SHAPES = [(12_292, 4 * 7 + 4), (12_548, 4 * 7 + 4), (14_332, 4 * 7 + 4), (1_000, None), (5_000, None)]


@pytest.mark.parametrize("n,blocks", _SHAPES, ids=["one_live_lane", "wavefront_with_one_live_lane", "one_dead_lane", "n1000_one_block_per_shard",
                                                   "n5000_two_blocks_per_shard"])
@pytest.mark.parametrize("d", [1, 3, 10])
def test_dead_lanes_of_each_kind(n, blocks, d):
    """12 292 = 4 x 3 073: every shard's last row holds ONE particle - seven wavefronts of that block are wholly dead.
    12 548 = 4 x 3 137: 65 live lanes - wavefront 1 has one live lane, wavefronts 2-7 none.
    14 332 = 4 x 3 583: 511 live lanes - one dead lane, in the last wavefront.
    1 000 and 5 000: the workers take the rows themselves, one and two blocks per shard, the last block of every shard partly filled."""
    seg = _pair(dict(n=n, d=d, seed=3, kw=_adaptive(d)))
    if blocks is not None:
        assert seg["segment_blocks"] == blocks, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["n_stages"] >= 12 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
    assert "1" in seg["flags"][1:], seg["flags"]


def test_fixed_schedule_on_two_hand_overs():
    """A fixed schedule with exact energy shifts (SMCMI_SHIFT_LAG=0, in both runs) takes the two-hand-over kernel - the one these bits
    change; with lagged shifts it would take the riding kernel, whose text is the one it was."""
    seg = _pair(dict(n=12_292, d=3, seed=7, kw=dict(use_fixed_schedule=True, n_phi=40)), {"SMCMI_SHIFT_LAG": "0"})
    assert seg["n_stages"] == 40 and seg["resamples"] >= 1 and seg["segment_blocks"] == 4 * 7 + 4


def test_without_history():
    """store_history=False: the correction under the re-formed `live` mask writes no history column."""
    seg = _pair(dict(n=12_292, d=3, seed=3, history=False, kw=_adaptive(3)))
    assert seg["resamples"] >= 1 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
