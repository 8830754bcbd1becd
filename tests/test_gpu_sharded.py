"""Shard-level HIP entry points (the multi-GPU path) on ONE MI355X: two / four shards of one population run as threads of a
single process, exchanging partial sums through an in-process communicator, and must reproduce the single-shard device
loop.  Also runs the real torch.distributed/RCCL code path with one rank."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import dist_helpers, models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def _run_sharded_threads(spec, n, seed, world, kw):
    from smc_jl_amd import Engine
    from tests.shard_orchestrator import ShardedSMC

    import torch

    torch.zeros(1, device="cuda")          # initialise torch's HIP context on the main thread first
    shared = dist_helpers.ThreadComm._Shared(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            nl = n // world
            eng = Engine(n, len(spec["priors"]), seed=seed, max_stages=1500, store_history=False, n_local=nl, gid0=rank * nl)
            eng.set_model(spec)
            sm = ShardedSMC(spec, n, seed=seed, engine=eng, comm=dist_helpers.ThreadComm(shared, rank), max_stages=1500)
            sm.n_local, sm.gid0 = nl, rank * nl
            sm.init_from_prior()
            r = sm.run(**kw)
            r["cloud"] = sm.download_cloud()
            out[rank] = r
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)
            shared.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_hip_shards_match_single_engine(world):
    from smc_jl_amd import Engine

    spec = models.gauss_spec(d=6)
    n, seed = 40000, 13
    kw = dict(use_fixed_schedule=False, tempering_target=0.95, n_blocks=2, alpha=0.9)
    e = Engine(n, 6, seed=seed, max_stages=1500, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    g = e.run(**kw)
    rec = e.stage_records(g["n_stages"])
    P = e.download_cloud()
    outs = _run_sharded_threads(spec, n, seed, world, kw)
    for r in outs:
        assert r["n_stages"] == g["n_stages"] and r["resamples"] == g["resamples"]
        np.testing.assert_allclose(r["schedule"], rec["schedule"], rtol=1e-9)
        np.testing.assert_allclose(r["ess"], rec["ess"], rtol=1e-8)
        assert r["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    full = np.concatenate([r["cloud"] for r in outs], axis=0)
    np.testing.assert_allclose(full, P, rtol=1e-7, atol=1e-9)


def test_bench_sharded_path_one_rank_rccl():
    """bench.py through torch.distributed.run with one rank and the sharded orchestrator forced on: exercises the
    nccl(=RCCL) process group, device-tensor all-reduce / all-gather and the zero-copy cloud tensors."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SMCMI_FORCE_SHARDED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29653", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--nparts", "20000",
           "--no-cpu"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    import json

    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert abs(d["logmdd_gpu"] - d["logmdd_exact"]) < 0.3


@pytest.mark.parametrize("world", [2, 4])
def test_cpp_group_driver_matches_single_engine(world):
    """csrc/sharded.hpp (the driver behind smcmi_run_sharded / RCCL) with in-process shards on one GPU."""
    from smc_jl_amd import Engine, run_group

    spec = models.gauss_spec(d=6)
    n, seed = 40000, 13
    kw = dict(use_fixed_schedule=False, tempering_target=0.95, n_blocks=2, alpha=0.9)
    e = Engine(n, 6, seed=seed, max_stages=1500, store_history=True)
    e.set_model(spec)
    e.init_from_prior()
    g = e.run(**kw)
    rec = e.stage_records(g["n_stages"])
    P = e.download_cloud()
    w1, W1 = e.history(g["n_stages"])
    nl = n // world
    engs = []
    for r in range(world):
        s = Engine(n, 6, seed=seed, max_stages=1500, store_history=True, n_local=nl, gid0=r * nl)
        s.set_model(spec)
        s.init_from_prior()
        engs.append(s)
    r = run_group(engs, **kw)
    assert r["n_stages"] == g["n_stages"] and r["resamples"] == g["resamples"]
    assert r["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    for s in engs:
        rs = s.stage_records(r["n_stages"])
        np.testing.assert_allclose(rs["schedule"], rec["schedule"], rtol=1e-9)
        np.testing.assert_allclose(rs["ess"], rec["ess"], rtol=1e-8)
        np.testing.assert_array_equal(rs["resampled"], rec["resampled"])
    full = np.concatenate([s.download_cloud() for s in engs], axis=0)
    np.testing.assert_allclose(full, P, rtol=1e-7, atol=1e-9)
    W = np.concatenate([s.history(r["n_stages"])[1] for s in engs], axis=0)
    np.testing.assert_allclose(W, W1, rtol=1e-7, atol=1e-12)


def test_cpp_group_single_shard_equals_the_plain_driver():
    """Same kernels; only the order in which block partials are combined differs (extra reduce kernels), i.e. rounding."""
    from smc_jl_amd import Engine, run_group

    spec = models.gauss_spec(d=4)
    out = []
    for mode in ("run", "group"):
        e = Engine(20000, 4, seed=3, max_stages=800, store_history=False)
        e.set_model(spec)
        e.init_from_prior()
        r = e.run(use_fixed_schedule=False) if mode == "run" else run_group([e], use_fixed_schedule=False)
        out.append((r["n_stages"], r["logmdd"], e.download_cloud()))
    assert out[0][0] == out[1][0] and out[0][1] == pytest.approx(out[1][1], abs=1e-10)
    np.testing.assert_allclose(out[0][2], out[1][2], rtol=1e-8, atol=1e-10)


def test_alltoall_resample_exchange_equals_allgather():
    """Resample redistribution as an all-to-all-v (only the rows inside a shard's ancestor range travel,
    SMCMI_RESAMPLE_EXCHANGE=alltoall) must reproduce the all-gather path bit for bit: the gather kernel sees the same rows."""
    code = r'''
import json, sys, numpy as np
sys.path.insert(0, %r)
from tests import models
from smc_jl_amd import Engine, run_group
spec = models.gauss_spec(d=6)
n, seed, world = 40000, 13, 4
engs = []
for r in range(world):
    s = Engine(n, 6, seed=seed, max_stages=1500, store_history=False, n_local=n // world, gid0=r * (n // world))
    s.set_model(spec); s.init_from_prior(); engs.append(s)
r = run_group(engs, use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, alpha=0.9, n_phi=100)
full = np.concatenate([s.download_cloud() for s in engs], axis=0)
print(json.dumps(dict(n=r["n_stages"], rs=r["resamples"], logmdd=r["logmdd"], chk=float(np.sum(full * np.arange(1, full.shape[1] + 1)[None, :])),
                      chk2=float(np.sum(full[::7] ** 2)))))
''' % ROOT
    out = {}
    for mode in ("allgather", "alltoall"):
        env = dict(os.environ, SMCMI_RESAMPLE_EXCHANGE=mode)
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        out[mode] = __import__("json").loads(res.stdout.strip().splitlines()[-1])
    assert out["alltoall"]["rs"] > 3
    assert out["alltoall"] == out["allgather"]


def test_group_driver_shares_one_energy_shift_across_shards():
    """The large-energy bridge of test_gpu_tempered (loglh - old_loglh ~ -600 everywhere) on two in-process shards: every shard
    must correct with the SAME energy shift (the largest energy over all shards travels in the epilogue all-reduce), or the
    summed weights of the shards would carry different factors."""
    from smc_jl_amd import Engine, run_group

    n, d, seed = 4096, 9, 779
    spec = models.linmodel_spec(T=100, old_T=60)
    e = Engine(n, d, seed=seed, max_stages=400)
    e.set_model(models.linmodel_spec(T=60))
    e.init_from_prior()
    r_old = e.run(n_phi=60, use_fixed_schedule=True, n_mh_steps=2)
    ess_old = float(e.stage_records(r_old["n_stages"])["ess"][-1])
    P_old = e.download_cloud()
    e.close()
    e = Engine(n, d, seed=seed + 1, max_stages=400)
    e.set_model(spec)
    e.upload_cloud(P_old)
    e.initialize_likelihoods()
    P0 = e.download_cloud()
    kw = dict(n_blocks=3, n_mh_steps=2, alpha=0.5, use_fixed_schedule=False, n_phi=30, tempering_target=0.95,
              resampling_method="systematic", threshold_ratio=0.8, initial_ess=ess_old)
    g = e.run(**kw)
    rec = e.stage_records(g["n_stages"])
    P = e.download_cloud()
    e.close()
    # make the shards' maxima differ: the best particle lives in shard 1
    assert np.argmax(P0[:, d] - P0[:, d + 2]) >= n // 2 or np.max((P0[:, d] - P0[:, d + 2])[: n // 2]) != np.max((P0[:, d] - P0[:, d + 2])[n // 2:])
    engs = []
    for r in range(2):
        s = Engine(n, d, seed=seed + 1, max_stages=400, n_local=n // 2, gid0=r * (n // 2))
        s.set_model(spec)
        s.upload_cloud(np.asfortranarray(P0[r * (n // 2):(r + 1) * (n // 2)]))
        engs.append(s)
    rg = run_group(engs, **kw)
    assert rg["n_stages"] == g["n_stages"] and rg["resamples"] == g["resamples"]
    assert rg["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    np.testing.assert_allclose(engs[0].stage_records(rg["n_stages"])["ess"], rec["ess"], rtol=1e-8)
    full = np.concatenate([s.download_cloud() for s in engs], axis=0)
    np.testing.assert_allclose(full, P, rtol=1e-7, atol=1e-9)
    for s in engs:
        s.close()


@pytest.mark.parametrize("fixed", [True, False])
def test_group_driver_pause_and_continue(fixed):
    """Intermediate save points with shards (smc_main.jl:499-507, 334-361): the lock-stepped shards pause at the same stage and
    continue in place, or in fresh handles restored from what the paused ones hand out; the run is the uninterrupted one."""
    from smc_jl_amd import Engine, run_group

    spec = models.gauss_spec(d=4)
    n, seed, world = 20000, 3, 2
    kw = dict(use_fixed_schedule=fixed, n_phi=40, tempering_target=0.9, n_blocks=2)

    def shards():
        out = []
        for r in range(world):
            s = Engine(n, 4, seed=seed, max_stages=600, n_local=n // world, gid0=r * (n // world))
            s.set_model(spec)
            out.append(s)
        return out

    ref = shards()
    for s in ref:
        s.init_from_prior()
    g = run_group(ref, **kw)
    rec = ref[0].stage_records(g["n_stages"])
    full = np.concatenate([s.download_cloud() for s in ref], axis=0)

    a = shards()
    for s in a:
        s.init_from_prior()
    r = run_group(a, stop_after_stage=9, **kw)
    assert r["paused"] and r["n_stages"] == 9
    states = [s.get_loop_state() for s in a]
    assert states[0] == states[1]
    # (1) continue in place
    saved = [(s.download_cloud(), s.stage_records(9), s.history(9)) for s in a]
    r1 = run_group(a, continue_run=True, **kw)
    assert not r1["paused"] and r1["n_stages"] == g["n_stages"] and r1["resamples"] == g["resamples"]
    assert r1["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    np.testing.assert_allclose(a[0].stage_records(r1["n_stages"])["ess"], rec["ess"], rtol=1e-8)
    np.testing.assert_allclose(np.concatenate([s.download_cloud() for s in a], axis=0), full, rtol=1e-7, atol=1e-9)
    # (2) continue in fresh handles from the saved pieces
    b = shards()
    for s, (P, rc9, (w9, W9)) in zip(b, saved):
        s.upload_cloud(P)
        s.set_stage_records(rc9["schedule"], rc9["ess"], rc9["c_hist"], rc9["accept_hist"], rc9["resampled"])
        s.set_history(w9, W9)
        s.set_loop_state(**states[0])
    r2 = run_group(b, continue_run=True, **kw)
    assert r2["n_stages"] == g["n_stages"] and r2["resamples"] == g["resamples"]
    assert r2["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    np.testing.assert_allclose(b[1].stage_records(r2["n_stages"])["schedule"], rec["schedule"], rtol=1e-9)
    np.testing.assert_allclose(np.concatenate([s.download_cloud() for s in b], axis=0), full, rtol=1e-7, atol=1e-9)
    for s in ref + a + b:
        s.close()


def test_two_rank_rccl_run_when_two_gpus_are_visible():
    """The real thing - one process per GPU, smcmi_run_sharded over an RCCL communicator with world size 2 - whenever the box has
    two devices (a gpurun box has one: skipped there; the driver's multi-GPU tier runs it).  bench.py --gpus 2 spawns the ranks
    itself, runs config 3's workload (scaled down) sharded and the same workload on rank 0 alone: the log-MDDs must agree to the
    bit (engine 2's shard-count invariance; the reference run uses the same engine at this size)."""
    import json

    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SMCMI_ENGINE="2")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--nparts", "80000",
                        "--no-cpu", "--full"], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["n_parts_per_gpu"] == 40000
    assert d["logmdd_abs_diff_vs_single_gpu"] == 0.0
    assert abs(d["logmdd_gpu"] - d["logmdd_exact"]) < 0.3


def test_host_closures_on_shards_match_one_handle():
    """The reference's `parallel = true` with a user closure: every worker scores the particles it holds (smc_main.jl:472-476).  Two
    shards of one population, the likelihood a host closure on each (ShardedSMC: propose -> closure -> accept per shard), against ONE
    handle running the same closure through smcmi_run's callback path: same stages and resample decisions, log-MDD to 1e-8, same cloud
    (particle ids are global: a shard proposes exactly what the single handle proposes for its rows)."""
    from smc_jl_amd import Engine
    from tests.shard_orchestrator import ShardedSMC

    import torch

    d, n, seed, world = 5, 20000, 21, 2
    base = models.gauss_spec(d=d)
    m, sigma = base["lik"][2].ravel(), base["lik"][1][0]
    const = -0.5 * d * np.log(2.0 * np.pi * sigma * sigma)

    def closure(theta):                                        # (m, d) -> (m,)
        return const - 0.5 * (((theta - m) / sigma) ** 2).sum(axis=1)

    spec = dict(base, lik=("host_callback", [], None, None))
    kw = dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, n_mh_steps=2, alpha=0.9)
    e = Engine(n, d, seed=seed, max_stages=600, store_history=False)
    e.set_model(spec)
    e.set_likelihood_callback(closure, which=0)
    e.init_from_prior()
    g = e.run(**kw)
    rec = e.stage_records(g["n_stages"])
    P = e.download_cloud()
    e.close()

    torch.zeros(1, device="cuda")
    shared = dist_helpers.ThreadComm._Shared(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            nl = n // world
            eng = Engine(n, d, seed=seed, max_stages=600, store_history=False, n_local=nl, gid0=rank * nl)
            eng.set_model(spec)
            sm = ShardedSMC(spec, n, seed=seed, engine=eng, comm=dist_helpers.ThreadComm(shared, rank), max_stages=600, loglikelihood=closure)
            sm.n_local, sm.gid0 = nl, rank * nl
            sm.init_from_prior()
            r = sm.run(**kw)
            r["cloud"] = sm.download_cloud()
            out[rank] = r
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)
            shared.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    for r in out:
        assert r["n_stages"] == g["n_stages"] and r["resamples"] == g["resamples"]
        np.testing.assert_allclose(r["schedule"], rec["schedule"], rtol=1e-9)
        assert r["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    full = np.concatenate([r["cloud"] for r in out], axis=0)
    np.testing.assert_allclose(full, P, rtol=1e-7, atol=1e-9)
    assert g["n_stages"] > 10 and g["resamples"] >= 1


def test_host_closures_on_shards_tempered_update():
    """The same with an old vintage: `loglikelihood` and `old_loglikelihood` both host closures (generalized tempering,
    src/mutation.jl:96-106), every shard scoring its own proposals with both; against one handle with the two callbacks."""
    from smc_jl_amd import Engine
    from tests.shard_orchestrator import ShardedSMC

    import torch

    d, n, seed, world = 4, 12000, 5, 2
    base = models.gauss_spec(d=d)
    m, sigma = base["lik"][2].ravel(), base["lik"][1][0]

    def new_lik(theta):
        return -0.5 * (((theta - m) / sigma) ** 2).sum(axis=1)

    def old_lik(theta):                                        # a flatter likelihood around a shifted mean: the "old data"
        return -0.5 * (((theta - (m + 0.3)) / (3.0 * sigma)) ** 2).sum(axis=1)

    spec = dict(base, lik=("host_callback", [], None, None), old_lik=("host_callback", [], None, None))
    kw = dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=1, n_mh_steps=1, alpha=1.0)
    rng = np.random.default_rng(11)
    P0 = np.zeros((n, d + 5), order="F")
    P0[:, :d] = m + 0.3 + 3.0 * sigma * rng.standard_normal((n, d))       # a cloud distributed like the old posterior (flat prior)
    P0[:, d] = old_lik(P0[:, :d])
    P0[:, d + 4] = 1.0

    def start(eng, rows):
        eng.upload_cloud(np.asfortranarray(P0[rows]))
        eng.initialize_likelihoods()                                       # old_loglh <- loglh, loglh / logprior on the new data

    e = Engine(n, d, seed=seed, max_stages=600, store_history=False)
    e.set_model(spec)
    e.set_likelihood_callback(new_lik, which=0)
    e.set_likelihood_callback(old_lik, which=1)
    start(e, slice(0, n))
    g = e.run(**kw)
    rec = e.stage_records(g["n_stages"])
    P = e.download_cloud()
    e.close()

    torch.zeros(1, device="cuda")
    shared = dist_helpers.ThreadComm._Shared(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            nl = n // world
            eng = Engine(n, d, seed=seed, max_stages=600, store_history=False, n_local=nl, gid0=rank * nl)
            eng.set_model(spec)
            sm = ShardedSMC(spec, n, seed=seed, engine=eng, comm=dist_helpers.ThreadComm(shared, rank), max_stages=600, loglikelihood=new_lik,
                            old_loglikelihood=old_lik)
            sm.n_local, sm.gid0 = nl, rank * nl
            start(eng, slice(rank * nl, (rank + 1) * nl))
            r = sm.run(**kw)
            r["cloud"] = sm.download_cloud()
            out[rank] = r
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)
            shared.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    for r in out:
        assert r["n_stages"] == g["n_stages"] and r["resamples"] == g["resamples"]
        np.testing.assert_allclose(r["schedule"], rec["schedule"], rtol=1e-9)
        assert r["logmdd"] == pytest.approx(g["logmdd"], abs=1e-8)
    full = np.concatenate([r["cloud"] for r in out], axis=0)
    np.testing.assert_allclose(full, P, rtol=1e-7, atol=1e-9)
    assert g["n_stages"] > 5


@pytest.mark.parametrize("kw", [dict(use_fixed_schedule=False, tempering_target=0.95, n_blocks=3, alpha=0.9),
                                dict(use_fixed_schedule=True, n_phi=60, n_blocks=3, n_mh_steps=2, resampling_method="multinomial"),
                                dict(use_fixed_schedule=True, n_phi=80, n_blocks=1)],
                         ids=["adaptive_mixture_3blocks", "fixed_multinomial_3blocks_2steps", "fixed_systematic_1block"])
def test_forty_parameters_on_one_handle_and_on_two_shards_against_the_oracle(orc, kw):
    """n_para > 16 (Smets-Wouters size: 40 parameters, examples/dsge_models/dsge_model.jl; regime-switching vectors,
    src/smc_main.jl:206-216) runs on engine 1's kernels - one handle (run type R3) and, sharded, round 1's all-reduce driver (R7,
    csrc/sharded.hpp run_sharded_impl) - which until now were compared with each other only.  Here both against the ORACLE on the same Philox
    streams: ϕ schedule, ESS path, resample stages, c path, acceptance rates, log-MDD, fixed schedules and multinomial resampling included."""
    from smc_jl_amd import Engine, run_group

    d, n, seed = 40, 16384, 23
    spec = models.gauss_spec(d=d, sigma=0.5, prior_sd=2.0)
    m = models.oracle_model(spec)
    P0 = orc.initial_draw(m, n, seed=seed)
    r = orc.smc_run(m, P0, seed=seed, n_threads=8, history=False, **kw)
    assert r["resamples"] >= 2

    def check(g, recs):
        assert (g["n_stages"], g["resamples"]) == (r["n_stages"], r["resamples"])
        for rec in recs:
            np.testing.assert_allclose(rec["schedule"], r["schedule"], rtol=1e-9)
            np.testing.assert_allclose(rec["ess"], r["ess"], rtol=1e-8)
            np.testing.assert_array_equal(rec["resampled"], r["resampled"])
            np.testing.assert_allclose(rec["c_hist"], r["c_hist"], rtol=1e-9)
            np.testing.assert_allclose(rec["accept_hist"], r["accept_hist"], atol=3.0 / n + 1e-12)
        assert g["logmdd"] == pytest.approx(r["logmdd"], abs=1e-7)

    e = Engine(n, d, seed=seed, max_stages=max(r["n_stages"] + 50, 300), store_history=False)
    e.set_model(spec)
    e.upload_cloud(P0)
    g = e.run(**kw)
    check(g, [e.stage_records(g["n_stages"])])
    e.close()
    nl = n // 2
    engs = []
    for k in range(2):
        s = Engine(n, d, seed=seed, max_stages=max(r["n_stages"] + 50, 300), store_history=False, n_local=nl, gid0=k * nl)
        s.set_model(spec)
        s.upload_cloud(np.asfortranarray(P0[k * nl:(k + 1) * nl]))
        engs.append(s)
    g2 = run_group(engs, **kw)
    check(g2, [s.stage_records(g2["n_stages"]) for s in engs])
    for s in engs:
        s.close()
