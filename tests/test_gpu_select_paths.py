"""The selection inside the one-handle, one-chunk segment kernels (csrc/stage3.hpp k3_select_inside and the gatherer's dec == 1 branch of
k3_segment): the workers resample the particles they hold between two stages of one launch, over two more chip-wide hand-overs - "every
particle and cum value is written" (two payload-free granules per worker in g_sel) and the moment rows of the resampled cloud (g_gm).  Who
polls which word, and through which table the totals travel, decides WHEN a value is looked at, never an operation on it.  So every path
must leave the bits a run of engine 2's launches leaves (SMCMI_ENGINE3=0, where k2_scan + k2_gather resample between two launches):
schedule, ESS, c, acceptance, resample flags, cloud, both histories, log-MDD.

Each shape is the smallest that reaches a distinct path of the selection's two hand-overs, at n_para 3 and 10 (the moment row's width,
pad2(NP), differs: 10 and 66 granules).  Every case resamples at least once behind stage 1, that is inside a segment, and no selection may
stall (select_stalls == 0).  Switches are read once per process: every run is a child process."""
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
    select_stalls=r["select_stalls"], stalls=[r["solver_stalls"], r["select_stalls"], r["spec_stalls"]])))
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
    """The job with segments and as launches: the same bits.  The segments ran, none timed out, the handle keeps its segment geometry, no
    selection stalled, and at least one stage behind stage 1 resampled."""
    seg = _run(cfg)
    ref = _run(cfg, {"SMCMI_ENGINE3": "0"})
    print(cfg, "stages", seg["n_stages"], "resampled", seg["flags"], "segments", seg["n_segments"], "segment stages", seg["segment_stages"],
          "blocks", seg["segment_blocks"], "stalls", seg["stalls"])
    assert ref["n_segments"] == 0
    assert seg["n_segments"] > 0 and seg["segment_timeouts"] == 0 and seg["segment_state"] == 1, seg
    assert seg["select_stalls"] == 0, seg["stalls"]
    for k in _KEYS:
        assert seg[k] == ref[k], (k, seg[k], ref[k], seg["stalls"], ref["stalls"])
    assert "1" in seg["flags"][1:], seg["flags"]
    return seg


def _adaptive(d, **more):
    # (30-40 stages: the 3-parameter Gaussian at a tempering target of 0.88, the 10-parameter one at 0.78)
    return dict(use_fixed_schedule=False, tempering_target=0.88 if d == 3 else 0.78, **more)


@pytest.mark.parametrize("d", [3, 10])
def test_a_selection_at_stage_after_stage(d):
    """12 288 = 8 shards x 3 rows, a resampling threshold above the tempering target: the run resamples at stage after stage inside the
    segment, so the selection's polls of g_sel and g_gm and the stage's own sweeps alternate on the same tables and the same staging area
    with nothing but the barriers of the totals' fetches between them, and each selection's tag follows the last one's by one."""
    seg = _pair(dict(n=12_288, d=d, seed=11, kw=_adaptive(d, threshold_ratio=0.92)))
    assert seg["segment_blocks"] == 8 * 3 + 8, seg["segment_blocks"]
    assert "11" in seg["flags"], seg["flags"]
    assert seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


# (segment blocks: V * rows workers + V gatherers, csrc/route.hpp plan_run)
@pytest.mark.parametrize("n,blocks", [(12_292, 4 * 7 + 4), (33_001, 8 * 9 + 8), (67_588, 4 * 34 + 4), (126_976, 8 * 31 + 8)],
                         ids=["rows7_last_row_one_particle", "uneven_last_shard", "rows34_gather_vshard", "rows31_256_blocks"])
@pytest.mark.parametrize("d", [3, 10])
def test_shard_shapes(n, blocks, d):
    """12 292 = 4 x 3 073: 4 virtual shards of 7 rows, every shard's last row holds ONE particle - its worker's tile scan, search and moment
    row run on one live lane.  33 001: 8 shards of ceil(n / 8) particles, the last one shorter (make_geo2_uneven), its last row partly
    filled.  67 588 = 4 x 16 897: 34 rows per shard, beyond the 32 of the fast sweep - the moment rows go through gather_vshard, and
    W = 136 workers' flags say "everything is written".  126 976 = 8 x 31 x 512: 256 blocks, the largest one-chunk cloud."""
    seg = _pair(dict(n=n, d=d, seed=3, kw=_adaptive(d)))
    assert seg["segment_blocks"] == blocks, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["n_stages"] >= 12 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


@pytest.mark.parametrize("d", [3, 10])
def test_two_rows_per_shard_take_the_rows_themselves(d):
    """5 000 particles (the reference's default): shards of two blocks, no gatherer is launched - both of the selection's hand-overs are
    gather_totals<2> on the row tables."""
    seg = _pair(dict(n=5_000, d=d, seed=5, kw=_adaptive(d)))
    assert seg["resamples"] >= 1 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


@pytest.mark.parametrize("d", [3, 10])
def test_multinomial_two_blocks(d):
    """Multinomial resampling (every output slot draws its own threshold; the search is not staged) with the parameters mutated in two blocks."""
    seg = _pair(dict(n=12_288, d=d, seed=7, kw=_adaptive(d, resampling_method="multinomial", n_blocks=2)))
    assert seg["segment_blocks"] == 8 * 3 + 8, seg["segment_blocks"]
    assert seg["resamples"] >= 1 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2


@pytest.mark.parametrize("d", [3, 10])
def test_a_fixed_schedule_that_rides(d):
    """A fixed schedule of 40 stages: the riding kernels (one hand-over per stage, the correction rows ride the mutation rows) call the same
    k3_select_inside when a stage resamples."""
    seg = _pair(dict(n=12_288, d=d, seed=7, kw=dict(use_fixed_schedule=True, n_phi=40)))
    assert seg["n_stages"] == 40 and seg["resamples"] >= 1 and seg["segment_blocks"] == 8 * 3 + 8
