"""The loop's failure paths on every stage engine.

check_nan_ess (src/helpers.jl:270-305, called at src/smc_main.jl:427-432): a correction that leaves no usable weight ends the run with
the reference's assertion text.  With the adaptive schedule the reference never reaches it - `fzero` throws on the NaN objective first
(src/helpers.jl:49) - so the guard is exercised on fixed schedules; the adaptive counterpart is the solver's bracket error.
PosDefException (src/mutation.jl:81: `MvNormal(θ̄_b, c²Σ_b)` outside the try block) aborts the run: a cloud whose particles coincide has
a zero covariance.  Inside an engine-3 segment the error must come back at once, not after the hand-over time-out.

Engines: 3 = persistent segments (small cloud, default), 2 = two launches per stage (SMCMI_ENGINE3=0), 1 = round-1 pipeline
(SMCMI_ENGINE=1); a 2-shard in-process group runs engine 2's sharded driver."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_W = r'''
import json, sys, time
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from smc_jl_amd.host import engine as eng
from smc_jl_amd.host._lib import SMCMIError
from tests import models
cfg = json.loads(%(cfg)r)
n, d = cfg["n"], cfg["d"]
spec = models.gauss_spec(d)
shards = cfg.get("shards", 1)
es = []
for r in range(shards):
    e = Engine(n, d, seed=3, max_stages=400, store_history=True, n_local=n // shards, gid0=r * (n // shards))
    e.set_model(spec); e.init_from_prior()
    es.append(e)
P = [e.download_cloud() for e in es]
out = []
if cfg.get("warm"):                                                   # first-use costs (allocations, residency self-test) out of the timings
    kw = dict(cfg["kw"])
    eng.run_group(es, **kw) if shards > 1 else es[0].run(**kw)
for case in cfg["cases"]:
    for e, P0 in zip(es, P):
        Q = P0.copy()
        if case == "nan_loglh":
            if e.gid0 == 0: Q[123, d] = np.nan                         # one particle's log-likelihood is NaN
        elif case == "all_minus_inf":
            Q[:, d] = -np.inf                                          # no particle has a usable likelihood
        elif case == "degenerate":
            Q[:, :] = P[0][7, :][None, :]; Q[:, d + 4] = 1.0            # every particle the same point: Σ = 0
        e.upload_cloud(Q)
    t0 = time.time()
    try:
        kw = dict(cfg["kw"])
        if shards > 1:
            r = eng.run_group(es, **kw)
        else:
            r = es[0].run(**kw)
        out.append(dict(case=case, code=0, msg="", seconds=time.time() - t0, n_stages=r["n_stages"], segments=r["n_segments"]))
    except SMCMIError as ex:
        out.append(dict(case=case, code=ex.code, msg=str(ex), seconds=time.time() - t0))
    if cfg.get("then_good"):                                          # the handle is usable afterwards
        for e, P0 in zip(es, P):
            e.upload_cloud(P0)
        r = eng.run_group(es, **kw) if shards > 1 else es[0].run(**kw)
        out[-1]["good_after"] = [r["n_stages"], bool(np.isfinite(r["logmdd"])), r["n_segments"]]
print("RESULT " + json.dumps(out))
'''


def _run(cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, "-c", _W % dict(root=ROOT, cfg=json.dumps(cfg))], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


ENGINES = [("segments", {}, 1), ("launches", {"SMCMI_ENGINE3": "0"}, 1), ("engine1", {"SMCMI_ENGINE": "1"}, 1), ("two_shards", {}, 2)]


@pytest.mark.parametrize("name,env,shards", ENGINES, ids=[e[0] for e in ENGINES])
def test_nan_ess_guard_on_every_engine(name, env, shards):
    cfg = dict(n=20480, d=10, shards=shards, cases=["nan_loglh", "all_minus_inf"], kw=dict(use_fixed_schedule=True, n_phi=40), then_good=True)
    res = _run(cfg, env)
    for r in res:
        assert r["code"] == -3, r                                                    # SMCMI_ERR_NAN_ESS
        assert "No particles have non-zero weight." in r["msg"] and "ESS is NaN" in r["msg"], r
        assert r["seconds"] < 5.0, r
        assert r["good_after"][0] == 40 and r["good_after"][1], r                    # the next run on the same handle is fine
    assert "NaN log-likelihoods" in res[0]["msg"], res[0]                            # helpers.jl:281-283
    assert "returning a NaN" in res[0]["msg"] and "returning a NaN" in res[1]["msg"], res     # helpers.jl:287-292
    if name == "segments":
        assert res[0]["good_after"][2] >= 1                                          # ... and still on engine 3


def test_nan_objective_on_an_adaptive_schedule_is_the_solvers_error():
    """`fzero` on a NaN objective (src/helpers.jl:49): the reference throws from the root finder before the NaN guard is reached."""
    cfg = dict(n=20480, d=10, cases=["nan_loglh"], kw=dict(use_fixed_schedule=False, tempering_target=0.95))
    for env in ({}, {"SMCMI_ENGINE": "1"}):
        r = _run(cfg, env)[0]
        assert r["code"] in (-6, -3), r                                              # SMCMI_ERR_BRACKET (or the guard, if a stage got that far)


@pytest.mark.parametrize("name,env,shards", ENGINES, ids=[e[0] for e in ENGINES])
def test_posdef_exception_aborts_the_run(name, env, shards):
    cfg = dict(n=20480, d=10, shards=shards, cases=["degenerate"], kw=dict(use_fixed_schedule=True, n_phi=40), then_good=True, warm=True)
    r = _run(cfg, env)[0]
    assert r["code"] == -4 and "PosDefException" in r["msg"], r                      # SMCMI_ERR_POSDEF
    assert r["seconds"] < 0.15 + (2.0 if name != "segments" else 0.0), r             # segments: no 200 ms hand-over time-out on the way out
    assert r["good_after"][0] == 40 and r["good_after"][1], r
    if name == "segments":
        assert r["good_after"][2] >= 1


def test_the_sharded_all_reduce_driver_rejects_an_unknown_resampler():
    """run_sharded_impl (n_para > 16 behind a group: two handles x 512 particles, n_para = 17) validates the resampler like the other three
    drivers: resampling_method = 7, set directly on the run configuration, is SMCMI_ERR_ARG with the reference's message before any stage
    runs - the handles' stage records stay untouched and the next run on the same handles is fine."""
    import ctypes as C

    import numpy as np

    from smc_jl_amd import Engine, run_group
    from smc_jl_amd.host import _lib
    from tests import models

    d, n, nl = 17, 1024, 512
    spec = models.gauss_spec(d=d, sigma=0.5, prior_sd=2.0)
    engs = []
    for k in range(2):
        e = Engine(n, d, seed=5, max_stages=40, store_history=False, n_local=nl, gid0=k * nl)
        e.set_model(spec)
        e.init_from_prior()
        engs.append(e)
    kw = dict(use_fixed_schedule=True, n_phi=12)
    good = run_group(engs, **kw)
    before = [e.stage_records(good["n_stages"]) for e in engs]
    rc = engs[0]._run_config(1, 1, 2.1, 12, "systematic", 0.5, 0.5, 1.0, 0.25, True, 0.97, 0.0, 0.0, 0, 0, 0, 0.0)
    rc.resampling_method = 7
    res = _lib.Result()
    arr = (C.c_void_p * 2)(*[e._h for e in engs])
    code = _lib.lib().smcmi_run_group(arr, 2, C.byref(rc), C.byref(res))
    msg = _lib.lib().smcmi_last_error().decode()
    print("code", code, "message", msg)
    assert code == -1, (code, msg)                                                   # SMCMI_ERR_ARG
    assert msg == "Invalid resampler in SMC. Options are systematic or multinomial", msg
    for e, b in zip(engs, before):                                                   # nothing ran: the records are the last run's
        a = e.stage_records(good["n_stages"])
        for key in ("schedule", "ess", "c_hist", "accept_hist", "resampled"):
            np.testing.assert_array_equal(a[key], b[key])
    again = run_group(engs, **kw)
    assert again["n_stages"] == 12 and np.isfinite(again["logmdd"])
    for e in engs:
        e.close()


# ---- who owns a handle's memory (csrc/devmem.hpp): under SMCMI_POISON_ALLOC=2 the library reports every allocation and every release with
# one process-wide index; tests/handle_lifetime_child.py leaves that report on stderr, a "[scenario] <name>" line in front of each scenario
def _lifetime_child(args, env_extra=None):
    import re

    env = dict(os.environ, SMCMI_POISON_ALLOC="2")
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handle_lifetime_child.py"), ROOT] + args, env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    report, name = {}, None                                   # scenario -> (indices allocated, indices released, poisoned allocations)
    for ln in p.stderr.splitlines():
        if ln.startswith("[scenario] "):
            name = ln[11:]
            report[name] = ([], [], 0)
            continue
        made, gone = re.match(r"\[smcmi\] (?:poisoned )?allocation #(\d+) ", ln), re.match(r"\[smcmi\] released #(\d+)$", ln)
        if made:
            report[name][0].append(int(made.group(1)))
            report[name] = report[name][:2] + (report[name][2] + ln.startswith("[smcmi] poisoned"),)
        elif gone:
            report[name][1].append(int(gone.group(1)))
    for name, (made, gone, poisoned) in report.items():
        print("scenario %s: %d allocations (%d of them poisoned device memory), %d releases" % (name, len(made), poisoned, len(gone)))
    return res, report


def _assert_all_given_back(report):
    made = [i for m, _, _ in report.values() for i in m]
    gone = [i for _, g, _ in report.values() for i in g]
    assert len(set(made)) == len(made), "an allocation index was reported twice"
    assert len(set(gone)) == len(gone), "an allocation was released twice"
    assert set(made) == set(gone), (sorted(set(made) - set(gone)), sorted(set(gone) - set(made)))
    for name, (m, g, _) in report.items():                    # every scenario closes its own handles
        assert set(m) == set(g), (name, sorted(set(m) ^ set(g)))


def test_a_failed_create_returns_everything_and_the_next_create_works():
    """smcmi_create with n_local = 2^40, n_para = 3: the first cloud buffer cannot be allocated - an error return of the allocator, nothing is
    launched.  SMCMI_ERR_HIP, the caller's handle pointer as it was, every reported allocation released; the next create in the same process
    (4 096 particles) succeeds and runs."""
    res, report = _lifetime_child(["create_failure"])
    assert res["rc"] == -2, res                                                       # SMCMI_ERR_HIP
    assert res["handle_untouched"], res
    assert res["message"], res
    _assert_all_given_back(report)
    assert len(report["next"][0]) > 30, report["next"]                                # (the report is on: the working create shows in it)
    assert res["next"][0] > 2 and res["next"][1], res


def test_everything_a_handle_took_is_given_back():
    """Create, use, destroy, four times: (a) one handle of 4 096 particles, n_para = 3 - an adaptive run on the default route (engine 2's buffers,
    the segment tables, the note, the snapshot), a second run with n_mh_steps = n_blocks = 2 (the drawn-ahead buffer regrows), a fixed schedule
    longer than the first (the schedule buffer regrows); (b) the same under SMCMI_ENGINE=1; (c) a group of two handles of 2 048 through
    run_group; (d) a host-callback and a device-callback run at 2 048 particles.  After the last close() the set of allocation indices on
    stderr equals the set of release indices.  (The library reads SMCMI_ENGINE once per process, so (b) is a child of its own.)"""
    res, report = _lifetime_child(["lifetime", "acd"])
    _assert_all_given_back(report)
    assert not report["end"][0] and not report["end"][1], report["end"]
    for s in "acd":
        assert len(report[s][0]) > 30, (s, len(report[s][0]))
        for n_stages, finite, _ in res[s]:
            assert n_stages > 2 and finite, (s, res[s])
    assert res["a"][2][0] == 320, res["a"]
    res, report = _lifetime_child(["lifetime", "a"], {"SMCMI_ENGINE": "1"})           # (b)
    _assert_all_given_back(report)
    assert len(report["a"][0]) > 30 and res["a"][2][0] == 320, (res, len(report["a"][0]))
