"""The device-pointer likelihood callback (smcmi_set_likelihood_device / Engine.set_likelihood_device / TorchLikelihood): the closure
path of smc(loglikelihood::Function, ...) with the proposals and the scores staying on the GPU.

Two kinds of device callback are used:
  staged - copies theta to the host, applies a numpy function, copies the result back.  Against a host-callback run with the SAME numpy
           function the likelihood values are identical by construction, so every difference would be the engine's (count, pack,
           scatter, NaN pass, redraw loop on the device instead of the host): these comparisons are bit for bit.
  native - the likelihood written in torch on the device.  Its arithmetic may round differently from numpy's, so these comparisons use
           the tolerances of tests/test_gpu_callback.py::test_callback_run_matches_the_device_likelihood.
A whole run exposes no ancestor vector; the ancestors of its resampling steps are covered by the bit-for-bit comparison of the clouds and
of the w / W history matrices they permute."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KWS = [dict(use_fixed_schedule=False, tempering_target=0.95),
       dict(use_fixed_schedule=True, n_phi=40, n_blocks=2, n_mh_steps=2, alpha=0.9)]


def _gauss_batch(m, sig):
    c0 = -0.5 * len(m) * math.log(2.0 * math.pi * sig * sig)

    def f(th):
        acc = np.zeros(th.shape[0])
        for k in range(th.shape[1]):                # the device's summation order (model.hpp loglik GAUSS_ISO)
            e = th[:, k] - m[k]
            acc += e * e
        return c0 - acc / (2.0 * sig * sig)
    return f


def _staged(fn, watch=None):
    """device callback: theta -> host -> the numpy function -> device"""
    import torch

    def f(th):
        if watch is not None:
            watch(th)
        return torch.as_tensor(np.asarray(fn(th.cpu().numpy()), dtype=np.float64), device=th.device)
    return f


def _torch_gauss(m, sig):
    import torch

    c0 = -0.5 * len(m) * math.log(2.0 * math.pi * sig * sig)
    mt = [float(x) for x in m]

    def f(th):
        acc = torch.zeros(th.shape[0], dtype=torch.float64, device=th.device)
        for k in range(th.shape[1]):                # the same operations in the same order
            e = th[:, k] - mt[k]
            acc += e * e
        return c0 - acc / (2.0 * sig * sig)
    return f


def _run(spec, n, d, seed, kw, register, max_stages=800, history=True):
    """initial cloud by the device family (the same for every mode), then `register(engine)` swaps the likelihood, then the run"""
    from smc_jl_amd import Engine

    e = Engine(n, d, seed=seed, max_stages=max_stages, store_history=history)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()
    if register is not None:
        register(e)
        e.upload_cloud(P0)
    r = e.run(**kw)
    out = dict(r=r, rec=e.stage_records(r["n_stages"]), P=e.download_cloud(), st=e.callback_stats(), ph=e.callback_phases(),
               hist=e.history(r["n_stages"]) if history else None)
    e.close()
    return out


def _assert_same_bits(a, b):
    assert a["r"]["n_stages"] == b["r"]["n_stages"] and a["r"]["resamples"] == b["r"]["resamples"]
    assert a["r"]["logmdd"] == b["r"]["logmdd"]
    for k in a["rec"]:
        assert np.array_equal(a["rec"][k], b["rec"][k]), k
    assert np.array_equal(a["P"], b["P"])
    if a["hist"] is not None:
        assert np.array_equal(a["hist"][0], b["hist"][0]) and np.array_equal(a["hist"][1], b["hist"][1])


def _assert_close(dev, cb):
    """the tolerances of test_callback_run_matches_the_device_likelihood"""
    r0, r1 = dev["r"], cb["r"]
    assert r0["n_stages"] == r1["n_stages"] and r0["resamples"] == r1["resamples"]
    np.testing.assert_allclose(cb["rec"]["schedule"], dev["rec"]["schedule"], rtol=1e-8)
    np.testing.assert_allclose(cb["rec"]["ess"], dev["rec"]["ess"], rtol=1e-7)
    assert abs(r1["logmdd"] - r0["logmdd"]) < 1e-7
    same = np.all(np.abs(cb["P"] - dev["P"]) <= 1e-9 * (1 + np.abs(dev["P"])), axis=1)
    assert same.mean() > 0.999                       # (an MH decision within an ulp of its threshold may flip)


@pytest.mark.parametrize("kw", KWS)
def test_staged_device_callback_is_the_host_callback_run_bit_for_bit(kw):
    """Case 1, and the no-pack half of case 3: bounds of +-1e5 around a prior of standard deviation 5 - nothing leaves them, so the
    user's function gets the engine's own proposal buffer (the same pointer at every call) and scores every row."""
    d, n, seed = 6, 20000, 7
    spec = models.gauss_spec(d)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    f = _gauss_batch(m, sig)
    ptrs, shapes = set(), set()

    def watch(th):
        ptrs.add(th.data_ptr())
        shapes.add((tuple(th.shape), tuple(th.stride()), str(th.dtype), th.is_cuda))

    host = _run(spec, n, d, seed, kw, lambda e: e.set_likelihood_callback(f, which=0))
    dev = _run(spec, n, d, seed, kw, lambda e: e.set_likelihood_device(_staged(f, watch), which=0))
    _assert_same_bits(host, dev)
    steps = kw.get("n_mh_steps", 1) * kw.get("n_blocks", 1)
    st = dev["st"]
    print("device callback: calls %d evaluations %d phases %r" % (st["calls"], st["evaluations"], dev["ph"]))
    assert st["calls"] == steps * (dev["r"]["n_stages"] - 1)            # one invocation per MH step x block, no chunks
    assert st["evaluations"] == st["calls"] * n                          # every proposal passed: nothing was packed
    assert len(ptrs) == 1
    assert shapes == {((n, d), (1, n), "torch.float64", True)}
    assert dev["ph"]["first_chunk_wait"] == 0.0 and dev["ph"]["later_chunk_wait"] == 0.0 and dev["ph"]["callback"] > 0.0


@pytest.mark.parametrize("kw", KWS)
def test_native_torch_likelihood_matches_the_device_family(kw):
    """Case 2"""
    d, n, seed = 6, 20000, 7
    spec = models.gauss_spec(d)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    fam = _run(spec, n, d, seed, kw, None)
    nat = _run(spec, n, d, seed, kw, lambda e: e.set_likelihood_device(_torch_gauss(m, sig), which=0))
    _assert_close(fam, nat)
    steps = kw.get("n_mh_steps", 1) * kw.get("n_blocks", 1)
    assert nat["st"]["calls"] == steps * (nat["r"]["n_stages"] - 1) and nat["st"]["evaluations"] == nat["st"]["calls"] * n


def test_device_callback_sees_only_in_bounds_proposals_packed_in_particle_order():
    """Case 3: wide proposals under uniform priors on [-0.5, 0.5]^3 - many leave the bounds, the rest is packed on the device."""
    import torch

    d, n = 3, 4096
    spec = models.gauss_spec(d)
    spec = dict(spec, bounds=[(-0.5, 0.5)] * d, priors=[("uniform", -0.5, 0.5)] * d)
    m, sig = np.asarray(spec["lik"][2]).ravel()[:d], float(spec["lik"][1][0])
    f = _gauss_batch(m, sig)
    kw = dict(use_fixed_schedule=True, n_phi=20, c=2.0)
    seen = dict(ok=None, sizes=[])

    def watch(th):
        inb = ((th >= -0.5) & (th <= 0.5)).all()                   # checked on the device, read after the run
        seen["ok"] = inb if seen["ok"] is None else seen["ok"] & inb
        seen["sizes"].append(th.shape[0])
        assert th.stride() == (1, th.shape[0])                     # a packed batch: leading dimension m

    host = _run(spec, n, d, 3, kw, lambda e: e.set_likelihood_callback(f, which=0), max_stages=200)
    dev = _run(spec, n, d, 3, kw, lambda e: e.set_likelihood_device(_staged(f, watch), which=0), max_stages=200)
    torch.cuda.synchronize()
    assert bool(seen["ok"])
    st = dev["st"]
    print("bounds: calls %d evaluations %d of %d" % (st["calls"], st["evaluations"], st["calls"] * n))
    assert st["calls"] == len(seen["sizes"]) == dev["r"]["n_stages"] - 1
    assert st["evaluations"] == sum(seen["sizes"])
    assert st["evaluations"] < st["calls"] * n                         # the pack path ran
    assert st["evaluations"] == host["st"]["evaluations"]
    _assert_same_bits(host, dev)


def test_nan_from_the_likelihood_is_minus_inf_on_the_device_as_on_the_host():
    """Case 4"""
    d, n, seed = 6, 8192, 13
    spec = models.gauss_spec(d)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    base = _gauss_batch(m, sig)
    count = [0]

    def f(th):
        out = base(th)
        bad = th[:, 0] > -0.9
        count[0] += int(bad.sum())
        out[bad] = np.nan
        return out

    kw = dict(use_fixed_schedule=True, n_phi=25, n_mh_steps=2)
    host = _run(spec, n, d, seed, kw, lambda e: e.set_likelihood_callback(f, which=0))
    n_host = count[0]
    dev = _run(spec, n, d, seed, kw, lambda e: e.set_likelihood_device(_staged(f), which=0))
    assert n_host > 0 and count[0] == 2 * n_host                     # NaNs were returned, the same number in both runs
    assert np.all(np.isfinite(dev["P"][:, d]))                       # no proposal with a NaN score was accepted
    _assert_same_bits(host, dev)


def test_errors_in_a_device_callback_surface_on_the_host_and_the_handle_runs_again():
    """Case 5: every failure is raised on the host, inside the trampoline, before anything of the batch is used - no GPU fault involved."""
    import torch

    from smc_jl_amd import Engine

    d, n = 4, 4096
    spec = models.gauss_spec(d)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    e = Engine(n, d, seed=5, max_stages=200, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    P0 = e.download_cloud()

    def boom(th):
        raise FloatingPointError("user likelihood failed")

    e.set_likelihood_device(boom, which=0)
    with pytest.raises(FloatingPointError):
        e.run(use_fixed_schedule=True, n_phi=20)
    e.set_likelihood_device(lambda th: torch.zeros(th.shape[0] + 1, dtype=torch.float64, device=th.device), which=0)
    e.upload_cloud(P0)
    with pytest.raises(ValueError, match="log-likelihoods"):
        e.run(use_fixed_schedule=True, n_phi=20)
    e.set_likelihood_device(lambda th: torch.zeros(th.shape[0], dtype=torch.float32, device=th.device), which=0)
    e.upload_cloud(P0)
    with pytest.raises(TypeError, match="float64"):
        e.run(use_fixed_schedule=True, n_phi=20)
    # the handle runs again, and gives the run a fresh handle gives
    e.set_likelihood_device(_torch_gauss(m, sig), which=0)
    e.upload_cloud(P0)
    r = e.run(use_fixed_schedule=True, n_phi=20)
    P = e.download_cloud()
    e.close()
    ref = _run(spec, n, d, 5, dict(use_fixed_schedule=True, n_phi=20), lambda x: x.set_likelihood_device(_torch_gauss(m, sig), which=0),
               max_stages=200, history=False)
    assert r["n_stages"] == 20 and r["logmdd"] == ref["r"]["logmdd"] and np.array_equal(P, ref["P"])
    # a host callback on one vintage next to a device callback on the other is refused by the run
    e = Engine(256, d, seed=1, max_stages=8, store_history=False)
    e.set_model(spec)
    e.init_from_prior()
    e.set_likelihood_device(_torch_gauss(m, sig), which=0)
    e.set_likelihood_callback(_gauss_batch(m, sig), which=1)
    with pytest.raises(RuntimeError, match="both be host callbacks or both device callbacks"):
        e.run(n_phi=5)
    e.close()


def test_tempered_update_with_torch_likelihoods_on_both_vintages():
    """Case 6: the scenario and the tolerance of test_smc_entry_point_with_a_python_closure_tempered_update"""
    import smc_jl_amd as S

    rng = np.random.default_rng(0)
    X = rng.normal(size=60)
    y = 1.0 + 1.0 * X + rng.normal(size=60)
    data = np.column_stack([y, X])

    def loglik(theta, dat):
        e = dat[:, 0] - theta[0] - theta[1] * dat[:, 1]
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * float(e @ e)

    def tloglik(theta, dat):                        # theta (m, 2), dat (T, 2): both device tensors
        e = dat[:, 0][None, :] - theta[:, 0:1] - theta[:, 1:2] * dat[:, 1][None, :]
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * (e * e).sum(dim=1)

    pars = [S.parameter("a", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0)), S.parameter("b", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 10.0))]
    kw = dict(n_parts=4000, n_phi=50, verbose="none", seed=5)
    c_old, _, _ = S.smc(loglik, pars, data[:30], **kw)
    c_py, _, _ = S.smc(loglik, pars, data, old_data=data[:30], old_cloud=c_old, **kw)
    c_t, w, W = S.smc(S.TorchLikelihood(tloglik), pars, data, old_data=data[:30], old_cloud=c_old, **kw)
    print("tempered update: log-MDD %.12f (torch) %.12f (python)" % (c_t.logmdd, c_py.logmdd))
    assert c_t.stage_index == c_py.stage_index == 50
    assert c_t.logmdd == pytest.approx(c_py.logmdd, abs=1e-6)
    np.testing.assert_allclose(S.weighted_mean(c_t), S.weighted_mean(c_py), atol=1e-6)
    assert w.shape == (4000, 50) and W.shape == (4000, 50)
    # ... with a prior-weighted bridge: the prior draws are scored by the OLD likelihood as a device callback (prior_engine)
    kb = dict(kw, tempered_update_prior_weight=0.3)
    c_pb, _, _ = S.smc(loglik, pars, data, old_data=data[:30], old_cloud=c_old, **kb)
    c_tb, _, _ = S.smc(S.TorchLikelihood(tloglik), pars, data, old_data=data[:30], old_cloud=c_old, **kb)
    assert c_tb.stage_index == c_pb.stage_index == 50
    assert c_tb.logmdd == pytest.approx(c_pb.logmdd, abs=1e-6)
    np.testing.assert_allclose(S.weighted_mean(c_tb), S.weighted_mean(c_pb), atol=1e-6)
    for new, old in ((loglik, S.TorchLikelihood(tloglik)), (S.TorchLikelihood(tloglik), loglik)):
        with pytest.raises(NotImplementedError, match="both"):
            S.smc(new, pars, data, old_data=data[:30], old_loglikelihood=old, old_cloud=c_old, **kw)


def test_initial_draw_with_rejected_draws_is_the_host_callbacks_bit_for_bit():
    """Case 7: a Gamma prior and a likelihood that rejects a third of the draws - the redraw loop with its attempt counters, gate and
    kept scores on the device against the host loop; initialize_likelihoods() and eval_cloud_callback() likewise."""
    import smc_jl_amd as S
    from smc_jl_amd.host import api

    def loglik(theta, dat):
        if theta[0] < 0.6:                           # a third of the Gamma(2, 1) draws
            return -math.inf
        e = dat[:, 0] - theta[0] - theta[1]
        return -0.5 * float(e @ e)

    pars = [S.parameter("g", 1.0, (1e-8, 1e5), prior=S.Gamma(2.0, 1.0)), S.parameter("b", 0.0, (-1e5, 1e5), prior=S.Normal(0.0, 2.0))]
    data = np.full((5, 1), 2.5)
    n = 1500
    spec = api._spec_from(pars, ("host_callback", [], None, None), None)
    batch = api._batch(loglik, data)
    out = []
    for mode in ("host", "device"):
        eng = S.Engine(n, 2, seed=3, max_stages=4, store_history=False)
        eng.set_parameters(spec["priors"], spec["bounds"], spec["fixed"])
        if mode == "host":
            eng.set_likelihood_callback(batch, which=0)
        else:
            eng.set_likelihood_device(_staged(batch), which=0)
        eng.set_likelihood("none", which=1)
        eng.init_from_prior()
        P = eng.download_cloud()
        st = eng.callback_stats()
        eng.initialize_likelihoods()
        P1 = eng.download_cloud()
        Q = P.copy(order="F")
        Q[:, 2] = 0.0
        Q[:, 4] = 7.0
        eng.upload_cloud(Q)
        eng.eval_cloud_callback(which=0, column=4)
        P2 = eng.download_cloud()
        eng.close()
        out.append((P, P1, P2, st))
    (Ph, P1h, P2h, sth), (Pd, P1d, P2d, std) = out
    assert np.all(np.isfinite(Ph[:, 2])) and np.all(Ph[:, 0] >= 0.6)
    np.testing.assert_array_equal(Pd[:, 4], 0.0)
    assert np.array_equal(Ph, Pd) and np.array_equal(P1h, P1d) and np.array_equal(P2h, P2d)
    assert np.array_equal(P2d[:, 4], Pd[:, 2])                       # the requested column holds the scores
    assert n < std["evaluations"] < 2 * n and std["evaluations"] == sth["evaluations"]   # each round scored only what it redrew


def test_run_group_of_two_handles_with_device_callbacks():
    """Case 8: two shards of one population on one GPU, against the same two handles with host callbacks on the same numpy function"""
    from smc_jl_amd import Engine, run_group

    d, n, seed, world = 5, 20000, 21, 2
    base = models.gauss_spec(d=d)
    m, sig = np.asarray(base["lik"][2]).ravel(), float(base["lik"][1][0])
    f = _gauss_batch(m, sig)
    kw = dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, n_mh_steps=2, alpha=0.9)
    out = []
    for mode in ("host", "device"):
        nl = n // world
        engs = []
        for r in range(world):
            e = Engine(n, d, seed=seed, max_stages=600, store_history=False, n_local=nl, gid0=r * nl)
            e.set_model(base)
            e.init_from_prior()
            P0 = e.download_cloud()
            if mode == "host":
                e.set_likelihood_callback(f, which=0)
            else:
                e.set_likelihood_device(_staged(f), which=0)
            e.upload_cloud(P0)
            engs.append(e)
        r = run_group(engs, **kw)
        rec = engs[0].stage_records(r["n_stages"])
        P = np.concatenate([e.download_cloud() for e in engs], axis=0)
        st = [e.callback_stats() for e in engs]
        for e in engs:
            e.close()
        out.append((r, rec, P, st))
    (r0, rec0, P0_, st0), (r1, rec1, P1_, st1) = out
    assert r0["n_stages"] == r1["n_stages"] and r0["resamples"] == r1["resamples"] and r0["logmdd"] == r1["logmdd"]
    for k in rec0:
        assert np.array_equal(rec0[k], rec1[k]), k
    assert np.array_equal(P0_, P1_)
    assert all(s["calls"] == 4 * (r1["n_stages"] - 1) for s in st1)      # 2 MH steps x 2 blocks per stage, per handle
    assert [s["evaluations"] for s in st1] == [s["evaluations"] for s in st0]


def _result_line(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "OK" in p.stdout
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])


def test_hip_example_with_a_user_kernel_matches_the_c_callback_example():
    """Case 9: examples/c_abi_device_callback.hip (the likelihood a user-written __global__ kernel on the callback's stream) against
    examples/c_abi_callback.c (the same Gaussian on the host).  With contraction off both are the same IEEE operations in the same
    order: the numerical fields of the two result lines - stages, resamples, log-MDD printed with 17 digits - are compared exactly
    (the lines also carry wall-clock figures, which are not results)."""
    lib = os.path.join(ROOT, "smc.jl_amd", "csrc")
    inc = os.path.join(ROOT, "include")
    exe_c = os.path.join(ROOT, "examples", "c_abi_callback")
    exe_h = os.path.join(ROOT, "examples", "c_abi_device_callback")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-I", inc, "-o", exe_c, os.path.join(ROOT, "examples", "c_abi_callback.c"),
                           "-L", lib, "-lsmcmi", "-lm", "-Wl,-rpath," + lib])
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-I", inc, "-o", exe_h,
                           os.path.join(ROOT, "examples", "c_abi_device_callback.hip"), "-L", lib, "-lsmcmi", "-Wl,-rpath," + lib])
    a, b = _result_line([exe_c]), _result_line([exe_h])
    print("host callback %r\ndevice callback %r" % (a["callback"], b["callback"]))
    assert a["n_parts"] == b["n_parts"] == 100000
    for sec in ("device", "callback"):
        for k in ("n_stages", "resamples", "logmdd"):
            assert a[sec][k] == b[sec][k], (sec, k, a[sec][k], b[sec][k])
    assert b["callback"]["calls"] == b["callback"]["n_stages"] - 1


def test_smc_with_a_torch_likelihood_on_the_regression_example():
    """Case 10: examples/estimate_regression.py's model through smc(TorchLikelihood(f), parameters, data) against the Python callable"""
    import smc_jl_amd as S

    data = np.load(os.path.join(ROOT, "tests", "golden", "reg_data.npz"))["data"]          # 100 x 2 = [y X]
    pars = [S.parameter("α1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False),
            S.parameter("β1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False)]

    def loglik(theta, dat):
        e = dat[:, 0] - theta[0] - theta[1] * dat[:, 1]
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * float(e @ e)

    def tloglik(theta, dat):
        e = dat[:, 0][None, :] - theta[:, 0:1] - theta[:, 1:2] * dat[:, 1][None, :]
        return -0.5 * dat.shape[0] * math.log(2.0 * math.pi) - 0.5 * (e * e).sum(dim=1)

    kw = dict(n_parts=1000, use_fixed_schedule=True, seed=1793, verbose="none")
    c_py, _, _ = S.smc(loglik, pars, data, **kw)
    c_t, _, _ = S.smc(S.TorchLikelihood(tloglik), pars, data, **kw)
    print("regression: mean %r (torch) %r (python)" % (S.weighted_mean(c_t), S.weighted_mean(c_py)))
    assert c_t.stage_index == c_py.stage_index
    np.testing.assert_allclose(S.weighted_mean(c_t), S.weighted_mean(c_py), atol=1e-6)
    assert abs(S.weighted_mean(c_t)[0] - 1.00018685) < 0.05 and abs(S.weighted_mean(c_t)[1] - 0.99936133) < 0.1
