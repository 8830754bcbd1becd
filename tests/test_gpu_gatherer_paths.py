"""The gatherer blocks' sweep of a virtual shard's rows in the two-hand-over, one-handle, one-chunk segment kernels (csrc/stage3.hpp k3_gather,
SMCMI_K3HO bit 8): every wavefront polls and fetches the rows it owns as they land, the reduction walks the rows present in whole steps of
8 rows instead of 64 row slots, the totals go out as 16-byte stores - WHEN a word is looked at and WHICH code looks, never an operation on a
value.  So every path must leave the bits a run of engine 2's launches leaves (SMCMI_ENGINE3=0): schedule, ESS, c, acceptance, resample
flags, cloud, both histories, log-MDD.

Each shape is the smallest that reaches a distinct path of k3_gather (8 wavefronts; wavefront w owns rows w, w + 8, ...), at n_para 3 and 10
(the correction row's width differs); tests/test_gpu_handover_paths.py has 3, 25 and 9 rows per shard.  30-40 stages with at least one
resample inside the segment.  Switches are read once per process: every run is a child process."""
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


# (segment blocks: V * rows workers + V gatherers, csrc/route.hpp plan_run)
@pytest.mark.parametrize("n,blocks", [(12_292, 4 * 7 + 4), (12_290, 2 * 13 + 2), (126_976, 8 * 31 + 8), (67_588, 4 * 34 + 4)],
                         ids=["rows7_fewer_than_wavefronts", "rows13_one_or_two_per_wavefront", "rows31_largest_fast_path", "rows34_gather_vshard"])
@pytest.mark.parametrize("d", [3, 10])
def test_rows_per_wavefront(n, blocks, d):
    """12 292 = 4 x 3 073: 4 virtual shards of 7 rows - wavefront 7 owns no row, and every shard's last row holds ONE particle.
    12 290 = 2 x 6 145: 2 shards of 13 rows - wavefronts 0-4 own two rows, 5-7 one; the reduction's two steps of 8 rows, the second partly
    filled.  126 976 = 8 x 31 x 512: 31 rows, four per wavefront but the last, 256 blocks - the largest cloud k3_gather serves.
    67 588 = 4 x 16 897: 34 rows, beyond k3_gather's 32 - the call site's dispatch to the unchanged gather_vshard."""
    seg = _pair(dict(n=n, d=d, seed=3, kw=_adaptive(d)))
    assert seg["segment_blocks"] == blocks, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["n_stages"] >= 12 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
    assert "1" in seg["flags"][1:], seg["flags"]


@pytest.mark.parametrize("d", [3, 10])
def test_selection_sweeps_alternate_with_the_stage_sweeps(d):
    """A resampling threshold above the tempering target: the run resamples at stage after stage, inside the segment.  The selection's two
    sweeps (gather_vshard: the "everything is written" row, the moment row) and the stage's two (k3_gather) take turns on the same staging
    area, with nothing but the barriers of the totals' fetches between them."""
    seg = _pair(dict(n=12_288, d=d, seed=11, kw=_adaptive(d, threshold_ratio=0.92)))
    assert seg["segment_blocks"] == 8 * 3 + 8, seg["segment_blocks"]
    assert "11" in seg["flags"] and seg["stalls"][1] == 0, seg["flags"]
    assert seg["segment_stages"] >= (seg["n_stages"] - 1) // 2
