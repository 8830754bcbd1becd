"""How a single-handle run of engines 2 / 3 starts and ends (csrc/prologue.hpp, csrc/run2.hpp): a fresh run puts its loop state, schedule, first
records, history columns, cleared tickets and engine 3's small inputs on the device with ONE launch (k2_run_prologue, which also takes the
centre of the cloud) and reads its result from host-mapped memory behind ONE sync (k2_run_result); the prior draw reports "no finite
likelihood" through a host-mapped word.  None of it is an operation on a value: every run must leave the bits it left before.

What can go wrong is state that survives from one run to the next on a handle - a table or ticket the launch no longer clears, a history
column or schedule left by another run, the host's copy of the loop state falling behind the device's - so the cases are repeats on ONE
handle, with another kind of run in between, against a fresh handle; a continued run (it takes the old start: pull, push, launches) against
the uninterrupted one; and the whole job with SMCMI_RUN_PROLOGUE=0 (the copies and launches as before) in a child process.  12 288
particles = 8 shards of 3 rows: the smallest one-chunk segment shape; 30-40 adaptive stages with resamples inside the segment."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, SEED = 12_288, 10, 7
KW = dict(use_fixed_schedule=False, tempering_target=0.78)
_KEYS = ("n_stages", "resamples", "logmdd", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud")


def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _engine(history=True):
    from smc_jl_amd import Engine
    from tests import models

    e = Engine(N, D, seed=SEED, max_stages=400, store_history=history)
    e.set_model(models.gauss_spec(D))
    return e


def _digest(e, r):
    rec = e.stage_records(r["n_stages"])
    out = dict(n_stages=r["n_stages"], resamples=r["resamples"], logmdd=float(r["logmdd"]).hex(), schedule=_h(rec["schedule"]), ess=_h(rec["ess"]),
               c_hist=_h(rec["c_hist"]), accept_hist=_h(rec["accept_hist"]), resampled=_h(rec["resampled"]), cloud=_h(e.download_cloud()),
               flags="".join(str(int(x)) for x in rec["resampled"]), n_segments=r["n_segments"], segment_stages=r["segment_stages"],
               segment_timeouts=r["segment_timeouts"], c=float(r["c"]).hex(), accept=float(r["accept"]).hex())
    if e.store_history:
        w, W = e.history(r["n_stages"])
        out.update(w=_h(w), W=_h(W))
    return out


def _job(e, **kw):
    e.init_from_prior()
    return _digest(e, e.run(**dict(KW, **kw)))


@pytest.fixture(scope="module")
def fresh():
    """The job on a handle that has run nothing else: computed once, compared by every test."""
    e = _engine()
    ref = _job(e)
    e.close()
    print("fresh handle:", ref["n_stages"], "stages, resampled", ref["flags"], "segments", ref["n_segments"], "segment stages", ref["segment_stages"])
    assert ref["n_segments"] > 0 and ref["segment_timeouts"] == 0 and ref["segment_stages"] >= (ref["n_stages"] - 1) // 2
    assert "1" in ref["flags"][1:] and 20 <= ref["n_stages"] <= 60, ref
    return ref


def _same(a, b, keys):
    for k in keys:
        assert a[k] == b[k], (k, a[k], b[k])


def test_repeats_on_one_handle_leave_the_first_runs_bits(fresh):
    """Three runs on one handle, a fixed schedule of another length (its own schedule upload, history columns, records and stage counts) between
    the first and the second: every repeat leaves what the first left, which is what a fresh handle leaves."""
    e = _engine()
    first = _job(e)
    other = _job(e, use_fixed_schedule=True, n_phi=40)
    assert other["n_stages"] == 40 and other["logmdd"] != first["logmdd"]
    second, third = _job(e), _job(e)
    e.close()
    for r in (first, second, third):
        _same(r, fresh, _KEYS + ("w", "W", "c", "accept", "n_segments", "segment_stages"))


def test_repeats_without_history(fresh):
    """store_history = False: the prologue launch has no history columns to write; records, cloud and log-MDD are the fresh handle's."""
    e = _engine(history=False)
    runs = [_job(e) for _ in range(3)]
    e.close()
    for r in runs:
        _same(r, fresh, _KEYS + ("c", "accept", "n_segments", "segment_stages"))


def _paused_and_continued(e, **kw):
    e.init_from_prior()
    p = e.run(**dict(KW, stop_after_stage=9, **kw))
    assert p["paused"] == 1 and p["n_stages"] == 9, p
    r = e.run(**dict(KW, continue_run=True, **kw))
    assert r["paused"] == 0
    return _digest(e, r)


def test_a_continued_run_equals_the_uninterrupted_one():
    """Paused at stage 9 and continued: the continuation starts the old way (the handle's state is pulled and pushed) and ends the new one -
    the host's copy of the loop state the pause leaves must be complete enough to go on from.  A fixed schedule: there a continuation computes
    what the uninterrupted run computes (an adaptive one certifies the roots of its first two stages instead of taking the predicted ones, which
    agree to phi_rtol only - its bits are compared with the old start's below)."""
    fixed = dict(use_fixed_schedule=True, n_phi=40)
    e = _engine()
    whole = _job(e, **fixed)
    got = _paused_and_continued(e, **fixed)
    e.close()
    assert whole["n_stages"] == 40 and "1" in whole["flags"][9:], whole["flags"]
    _same(got, whole, _KEYS + ("w", "W", "c", "accept"))


_WORKER = r'''
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_gpu_run_prologue as t
e = t._engine()
print("RESULT " + json.dumps(dict(job=t._job(e), continued=t._paused_and_continued(e))))
'''


def test_the_copies_and_launches_of_before_leave_the_same_bits(fresh):
    """SMCMI_RUN_PROLOGUE=0 (read once per process: a child): the push, the copies, k_center_one, the fills and k2_state at the start, the
    copy of DevState and of the stage counts at the end - for the job, and for the same job paused at stage 9 and continued."""
    env = dict(os.environ, SMCMI_RUN_PROLOGUE="0")
    p = subprocess.run([sys.executable, "-c", _WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    old = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    _same(old["job"], fresh, _KEYS + ("w", "W", "c", "accept", "n_segments", "segment_stages"))
    e = _engine()
    got = _paused_and_continued(e)
    e.close()
    assert got["n_stages"] >= 20 and "1" in got["flags"][9:], got["flags"]
    _same(got, old["continued"], _KEYS + ("w", "W", "c", "accept", "n_segments", "segment_stages"))


def test_no_finite_likelihood_draw_is_still_an_error():
    """A Gaussian likelihood centred at +inf is -inf on the whole support of the prior: every particle gives up after its last attempt and the
    prior draw itself returns the error - now read from a host-mapped word instead of a copied flag.  (tests/models.py can express the model:
    no existing test covered this error on the device path.)  One parameter, 64 particles: 100 001 attempts each, tens of milliseconds."""
    from smc_jl_amd import Engine
    from tests import models

    spec = models.gauss_spec(1)
    spec["lik"] = ("gauss_iso", [0.25], np.full((1, 1), np.inf), None)
    e = Engine(64, 1, seed=1, max_stages=50, store_history=False)
    e.set_model(spec)
    with pytest.raises(Exception, match="no finite-likelihood draw"):
        e.init_from_prior()
    # the word is cleared by the next draw: the same handle draws from a proper model afterwards
    e.set_model(models.gauss_spec(1))
    e.init_from_prior()
    assert np.isfinite(e.download_cloud()[:, 1]).all()
    e.close()
