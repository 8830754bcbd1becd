"""smcmi_run_ensemble (many small SMC runs in ONE launch, one workgroup per run) on a real MI355X.

Every member is compared twice: against a twin handle run alone through smcmi_run on the same uploaded cloud and seed, and against the
CPU restatement (oracle.smc_run) on that cloud and seed.  Tolerances are the project's own: tests/test_gpu_parity.py::_compare_runs
(stage count, resample count and flags equal; schedule, ESS and c to rtol 1e-9; acceptance history to atol 3 / n + 1e-12), the log-MDD to
1e-8 absolute (the README's parity statement), final clouds to rtol 1e-7, atol 1e-9 (as the sharded tests compare clouds).
All of these fail on a library without the entry point."""
import ctypes as C

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu

T = 256            # csrc/ensshape.hpp ENS_T: the block of a member's workgroup


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def make_engine(spec, n, seed, max_stages, store_history=False, **kw):
    from smc_jl_amd import Engine

    e = Engine(n, len(spec["priors"]), seed=seed, max_stages=max_stages, store_history=store_history, **kw)
    e.set_model(spec)
    return e


def run_ensemble(engines, **kw):
    from smc_jl_amd import run_ensemble as f

    return f(engines, **kw)


def assert_same_run(n, what, got, ref):
    """got / ref: dict(n_stages, resamples, logmdd, schedule, ess, c_hist, accept_hist, resampled, particles)"""
    assert got["n_stages"] == ref["n_stages"], what
    assert got["resamples"] == ref["resamples"], what
    ns = got["n_stages"]
    np.testing.assert_array_equal(got["resampled"][:ns], ref["resampled"][:ns], err_msg=what)
    np.testing.assert_allclose(got["schedule"][:ns], ref["schedule"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["ess"][:ns], ref["ess"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["c_hist"][:ns], ref["c_hist"][:ns], rtol=1e-9, err_msg=what)
    np.testing.assert_allclose(got["accept_hist"][:ns], ref["accept_hist"][:ns], atol=3.0 / n + 1e-12, rtol=0, err_msg=what)
    assert abs(got["logmdd"] - ref["logmdd"]) <= 1e-8, (what, got["logmdd"], ref["logmdd"])
    np.testing.assert_allclose(got["particles"], ref["particles"], rtol=1e-7, atol=1e-9, err_msg=what)


def collect(e, res):
    out = dict(n_stages=res["n_stages"], resamples=res["resamples"], logmdd=res["logmdd"], particles=e.download_cloud())
    out.update(e.stage_records(res["n_stages"]))
    return out


def solo_run(spec, n, seed, P0, max_stages, kw, store_history=False):
    tw = make_engine(spec, n, seed, max_stages, store_history)
    tw.upload_cloud(P0)
    return tw, collect(tw, tw.run(**kw))


def check_member(orc, spec, n, seed, P0, max_stages, kw, e, res, what):
    """member (e, res) of an ensemble against its solo twin and against the CPU restatement"""
    assert res["status"] == 0, (what, res["status"])
    got = collect(e, res)
    tw, solo = solo_run(spec, n, seed, P0, max_stages, kw)
    tw.close()
    assert_same_run(n, what + " vs its solo run", got, solo)
    r = orc.smc_run(models.oracle_model(spec), P0, seed=seed, n_threads=8, history=False, max_stages=max_stages, **kw)
    assert_same_run(n, what + " vs the CPU restatement", got, r)
    return got


def start_clouds(orc, specs, n, seeds):
    return [orc.initial_draw(models.oracle_model(s), n, seed=sd) for s, sd in zip(specs, seeds)]


def ensemble_of(specs, n, seeds, P0s, max_stages, store_history=False):
    es = [make_engine(s, n, sd, max_stages, store_history) for s, sd in zip(specs, seeds)]
    for e, P in zip(es, P0s):
        e.upload_cloud(P)
    return es


def fixed_columns_spec():
    """8 columns of which three are fixed, as tests/test_gpu_parity.py::test_run_with_fixed_and_free_regime_columns_vs_oracle"""
    spec = models.gauss_spec(d=8)
    spec["fixed"] = [0, 0, 1, 0, 0, 1, 0, 1]
    spec["priors"] = [("normal", 0.3 * k, 5.0) if not f else ("normal", -1.0 + 2.0 * k / 7.0, 5.0) for k, f in enumerate(spec["fixed"])]
    return spec


CELLS = {
    "regression_config1": (models.regression_spec, 1000, [1793, 7, 8], 300, dict()),
    "gauss10_adaptive": (models.gauss_spec, 1000, [1, 2, 3], 400, dict(use_fixed_schedule=False, tempering_target=0.95)),
    "gauss3_odd_pair": (lambda: models.gauss_spec(d=3), T + 1, [11, 12, 13, 14], 20,
                        dict(n_phi=20, n_blocks=2, n_mh_steps=2, resampling_method="multinomial")),
    "gauss1": (lambda: models.gauss_spec(d=1), 65, [3, 4, 5], 15, dict(n_phi=15)),
    "gauss8_fixed_columns": (fixed_columns_spec, 1000, [31, 32, 33], 24, dict(n_phi=24, n_blocks=2)),
    "capm_literal": (models.capm_spec, 1000, [5, 6, 7], 20, dict(n_phi=20, n_mh_steps=3)),
    "gauss10_at_the_cap": (models.gauss_spec, 8192, [21, 22], 16, dict(n_phi=16)),
}


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_members_equal_their_solo_runs(orc, cell):
    mk, n, seeds, max_stages, kw = CELLS[cell]
    spec = mk()
    specs = [spec] * len(seeds)
    P0s = start_clouds(orc, specs, n, seeds)
    es = ensemble_of(specs, n, seeds, P0s, max_stages)
    rs = run_ensemble(es, **kw)
    assert [r["call_status"] for r in rs] == [0] * len(seeds)
    logmdds = set()
    for k, sd in enumerate(seeds):
        got = check_member(orc, spec, n, sd, P0s[k], max_stages, kw, es[k], rs[k], "%s member %d (seed %d)" % (cell, k, sd))
        logmdds.add(got["logmdd"])
        if cell == "gauss8_fixed_columns":
            for col in (2, 5, 7):
                assert np.all(got["particles"][:, col] == P0s[k][0, col])          # fixed columns never move
        if cell == "regression_config1":
            assert got["n_stages"] == 300
    assert len(logmdds) == len(seeds)                        # distinct seeds, distinct runs
    for e in es:
        e.close()


def test_more_members_than_cus(orc):
    """300 members on a 256-CU chip: the grid queues; every status is 0; members 0, 255 and 299 equal their solo runs"""
    spec = models.gauss_spec(d=2)
    n, E, kw = 128, 300, dict(n_phi=12)
    seeds = list(range(1000, 1000 + E))
    m = models.oracle_model(spec)
    P0s = [orc.initial_draw(m, n, seed=sd) for sd in seeds]
    es = ensemble_of([spec] * E, n, seeds, P0s, 12)
    rs = run_ensemble(es, **kw)
    assert [r["status"] for r in rs] == [0] * E
    assert all(r["n_stages"] == 12 for r in rs)
    for k in (0, 255, 299):
        check_member(orc, spec, n, seeds[k], P0s[k], 12, kw, es[k], rs[k], "member %d of %d" % (k, E))
    for e in es:
        e.close()


def test_position_and_company_do_not_matter(orc):
    """a member's cloud, records and log-MDD are the same bits alone and as member 3 of 5, and two identical calls give the same bits"""
    spec = models.gauss_spec(d=4)
    n, kw, ms = 500, dict(use_fixed_schedule=False, tempering_target=0.9, n_blocks=2, resampling_method="multinomial"), 200
    seeds = [41, 42, 43, 44, 45]
    P0s = start_clouds(orc, [spec] * 5, n, seeds)

    def bits(e, r):
        rec = e.stage_records(r["n_stages"])
        return (r["n_stages"], r["resamples"], r["logmdd"], r["c"], r["accept"], e.download_cloud().tobytes(),
                tuple(rec[k].tobytes() for k in ("schedule", "ess", "c_hist", "accept_hist", "resampled")))

    alone = ensemble_of([spec], n, [seeds[3]], [P0s[3]], ms)
    ra = run_ensemble(alone, **kw)
    want = bits(alone[0], ra[0])
    assert ra[0]["status"] == 0 and ra[0]["n_stages"] > 5
    for _ in range(2):                                        # ... and the same call twice
        five = ensemble_of([spec] * 5, n, seeds, P0s, ms)
        rf = run_ensemble(five, **kw)
        assert bits(five[3], rf[3]) == want
        for e in five:
            e.close()
    alone[0].close()


def test_different_models_side_by_side(orc):
    """three members with different likelihood data, likelihood parameters, priors and bounds: each equals its own solo run"""
    specs = []
    for k, (sigma, prior_sd, shift) in enumerate([(0.25, 5.0, 0.0), (0.5, 3.0, 1.5), (0.1, 8.0, -2.0)]):
        s = models.gauss_spec(d=4, sigma=sigma, prior_sd=prior_sd)
        s["lik"] = ("gauss_iso", [sigma], np.asarray(s["lik"][2]) + shift, None)
        s["priors"] = [("normal", 0.1 * k, prior_sd)] * 3 + [("uniform", -6.0 - k, 6.0 + k)]
        s["bounds"] = [(-1e5, 1e5)] * 3 + [(-6.0 - k, 6.0 + k)]
        specs.append(s)
    n, seeds, kw, ms = 600, [51, 52, 53], dict(n_phi=25, n_blocks=2), 25
    P0s = start_clouds(orc, specs, n, seeds)
    es = ensemble_of(specs, n, seeds, P0s, ms)
    rs = run_ensemble(es, **kw)
    outs = [check_member(orc, specs[k], n, seeds[k], P0s[k], ms, kw, es[k], rs[k], "model %d" % k) for k in range(3)]
    assert abs(outs[0]["logmdd"] - outs[1]["logmdd"]) > 0.1 and abs(outs[0]["logmdd"] - outs[2]["logmdd"]) > 0.1
    for e in es:
        e.close()


def test_a_failing_member_stands_alone(orc):
    """one of three members starts from a cloud whose log-likelihood column holds a NaN: its status is SMCMI_ERR_NAN_ESS and the call returns
    that code; the other two equal their solo runs"""
    spec = models.gauss_spec(d=3)
    n, seeds, kw, ms = 400, [61, 62, 63], dict(n_phi=18), 18
    P0s = start_clouds(orc, [spec] * 3, n, seeds)
    P0s[1] = np.array(P0s[1], order="F")
    P0s[1][17, 3] = np.nan
    es = ensemble_of([spec] * 3, n, seeds, P0s, ms)
    rs = run_ensemble(es, **kw)
    assert [r["status"] for r in rs] == [0, -3, 0]
    assert [r["call_status"] for r in rs] == [-3] * 3
    for k in (0, 2):
        check_member(orc, spec, n, seeds[k], P0s[k], ms, kw, es[k], rs[k], "member %d next to a failing one" % k)
    for e in es:
        e.close()


def test_capacity_is_a_members_own_error(orc):
    """an adaptive run that needs more stages than the handles hold records for ends with SMCMI_ERR_CAPACITY like the solo run, the records of
    the max_stages stages it completed in place (nothing is written beyond them)"""
    from smc_jl_amd.host import _lib

    spec = models.gauss_spec(d=2)
    n, seeds, ms = 300, [81, 82], 6
    kw = dict(use_fixed_schedule=False, tempering_target=0.97)
    P0s = start_clouds(orc, [spec] * 2, n, seeds)
    es = ensemble_of([spec] * 2, n, seeds, P0s, ms, store_history=True)
    rs = run_ensemble(es, **kw)
    assert [r["status"] for r in rs] == [-5, -5] and rs[0]["call_status"] == -5
    for k in range(2):
        assert rs[k]["n_stages"] == ms and es[k].stages_held() == ms
        tw = make_engine(spec, n, seeds[k], ms, store_history=True)
        tw.upload_cloud(P0s[k])
        with pytest.raises(_lib.SMCMIError) as ei:
            tw.run(**kw)
        assert ei.value.code == -5
        a, b = es[k].stage_records(ms), tw.stage_records(ms)
        np.testing.assert_allclose(a["schedule"], b["schedule"], rtol=1e-9)
        np.testing.assert_allclose(a["ess"], b["ess"], rtol=1e-9)
        np.testing.assert_array_equal(a["resampled"], b["resampled"])
        assert 0.0 < a["schedule"][-1] < 1.0
        np.testing.assert_allclose(es[k].download_cloud(), tw.download_cloud(), rtol=1e-7, atol=1e-9)
        tw.close()
    for e in es:
        e.close()


def test_the_handle_afterwards(orc):
    """with store_history: records, history, loop state and stages_held as the solo twin's; the summaries work; a fresh smcmi_run on the same
    handle from a re-uploaded cloud is bit-identical to that run on a handle the ensemble never touched"""
    from smc_jl_amd.host import api

    spec = models.gauss_spec(d=5)
    n, seeds, ms = 700, [71, 72], 300
    kw = dict(use_fixed_schedule=False, tempering_target=0.92, n_mh_steps=2)
    P0s = start_clouds(orc, [spec] * 2, n, seeds)
    es = ensemble_of([spec] * 2, n, seeds, P0s, ms, store_history=True)
    rs = run_ensemble(es, **kw)
    for k in range(2):
        e, r = es[k], rs[k]
        got = check_member(orc, spec, n, seeds[k], P0s[k], ms, kw, e, r, "member %d" % k)
        tw, solo = solo_run(spec, n, seeds[k], P0s[k], ms, kw, store_history=True)
        ns = r["n_stages"]
        assert e.stages_held() == tw.stages_held() == ns
        w, W = e.history(ns)
        ws, Ws = tw.history(ns)
        # (a history column is what the cloud's weight column was at that stage: the clouds' tolerance.  A single weight answers a change
        # δϕ of the stage's root with δϕ (e_i - ē), so the schedule's 1e-9 does not bound it for a particle far out in energy)
        np.testing.assert_allclose(w, ws, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(W, Ws, rtol=1e-7, atol=1e-9)
        assert np.all(w[:, 0] == 0) and np.array_equal(W[:, 0], P0s[k][:, -1])
        # the log-MDD formula from the stored histories (SURVEY a-9)
        assert np.sum(np.log(np.sum(w[:, 1:] * W[:, :-1], axis=0) / n)) == pytest.approx(r["logmdd"], abs=1e-8)
        a, b = e.get_loop_state(), tw.get_loop_state()
        for key in ("stage_index", "j", "resampled_last_period", "resamples"):
            assert a[key] == b[key], (key, a, b)
        for key in ("phi_n", "phi_prop", "c", "ess"):
            assert a[key] == pytest.approx(b[key], rel=1e-9), (key, a, b)
        assert abs(a["accept"] - b["accept"]) <= 3.0 / n + 1e-12
        assert abs(a["logmdd"] - b["logmdd"]) <= 1e-8
        assert a["stage_index"] == ns and a["phi_n"] == 1.0 and a["logmdd"] == r["logmdd"] and a["c"] == r["c"] and a["accept"] == r["accept"]
        mean_e, cov_e = e.stage_moments()
        mean_t, cov_t = tw.stage_moments()
        np.testing.assert_allclose(mean_e, mean_t, rtol=1e-9, atol=1e-12)
        # the summaries, against the numpy mirror on the downloaded cloud
        q = e.weighted_quantiles(probs=(0.05, 0.5, 0.95))
        np.testing.assert_allclose(q, api.weighted_quantiles(got["particles"], probs=(0.05, 0.5, 0.95)), rtol=1e-9, atol=1e-12)
        idx, val, para = e.best_particle("loglh")
        assert idx == int(np.argmax(got["particles"][:, 5])) and val == got["particles"][idx, 5]
        np.testing.assert_array_equal(para, got["particles"][idx, :5])
        # a fresh run on the same handle
        kw2 = dict(n_phi=30, n_blocks=2)
        fresh = make_engine(spec, n, seeds[k], ms, store_history=True)
        outs = []
        for h in (e, fresh):
            h.upload_cloud(P0s[k])
            g = h.run(**kw2)
            rec = h.stage_records(g["n_stages"])
            outs.append((g["n_stages"], g["resamples"], g["logmdd"], h.download_cloud().tobytes(), tuple(rec[x].tobytes() for x in sorted(rec)),
                         tuple(x.tobytes() for x in h.history(g["n_stages"]))))
        assert outs[0] == outs[1]
        fresh.close()
        tw.close()
    for e in es:
        e.close()


def test_refusals(orc):
    """every row of the header's refusal table returns its code, and a cloud downloaded before and after is bit-identical"""
    from smc_jl_amd import Engine
    from smc_jl_amd.host import _lib

    ARG, UNSUPPORTED = -1, -7
    spec = models.gauss_spec(d=3)
    n, ms = 200, 20
    m = models.oracle_model(spec)
    P0 = orc.initial_draw(m, n, seed=9)

    def good(seed=9, nn=n, stages=ms, hist=False, sp=spec):
        e = make_engine(sp, nn, seed, stages, hist)
        e.upload_cloud(orc.initial_draw(models.oracle_model(sp), nn, seed=seed))
        return e

    def refused(engines, code, **kw):
        before = [e.download_cloud() for e in engines]
        states = [e.get_loop_state() for e in engines]
        with pytest.raises(_lib.SMCMIError) as ei:
            run_ensemble(engines, **dict(dict(n_phi=10), **kw))
        assert ei.value.code == code, (ei.value.code, code, str(ei.value))
        for e, b, s in zip(engines, before, states):
            assert e.download_cloud().tobytes() == b.tobytes()
            assert e.get_loop_state() == s

    a, b = good(1), good(2)
    # ---- SMCMI_ERR_ARG: n < 1, a NULL or repeated handle, differing shapes
    L = _lib.lib()
    rc = a._run_config(1, 1, 2.1, 10, "systematic", 0.5, 0.5, 1.0, 0.25, True, 0.97, 0.0, 0.0, 0, 0, 0, 0.0, 0.0)
    res, status = (_lib.Result * 2)(), (C.c_int32 * 2)()
    before = a.download_cloud()
    assert L.smcmi_run_ensemble((C.c_void_p * 2)(a._h, b._h), 0, C.byref(rc), res, status) == ARG
    assert L.smcmi_run_ensemble((C.c_void_p * 2)(a._h, b._h), -2, C.byref(rc), res, status) == ARG
    assert L.smcmi_run_ensemble((C.c_void_p * 2)(a._h, None), 2, C.byref(rc), res, status) == ARG
    assert L.smcmi_run_ensemble(None, 2, C.byref(rc), res, status) == ARG
    assert a.download_cloud().tobytes() == before.tobytes()
    refused([a, b, a], ARG)
    for other in (good(3, nn=n + 1), good(3, stages=ms + 1), good(3, hist=True), good(3, sp=models.gauss_spec(d=4))):
        refused([a, other], ARG)
        other.close()
    # ---- SMCMI_ERR_UNSUPPORTED
    shard = Engine(2 * n, 3, seed=4, max_stages=ms, store_history=False, n_local=n, gid0=0)
    shard.set_model(spec)
    shard.upload_cloud(P0)
    refused([shard], UNSUPPORTED)
    shard2 = Engine(2 * n, 3, seed=4, max_stages=ms, store_history=False, n_local=n, gid0=n)
    shard2.set_model(spec)
    shard2.upload_cloud(P0)
    refused([shard, shard2], UNSUPPORTED)
    shard.close()
    shard2.close()
    cb = good(5)
    cb.set_likelihood_callback(lambda th: -0.5 * (th ** 2).sum(axis=1))
    refused([a, cb], UNSUPPORTED)                                   # a host callback
    cb.close()
    dcb = good(6)
    fn = _lib.LIK_DEVICE_FN(lambda *args: 0)                        # (never called: the registration alone makes the handle a closure handle)
    dl = _lib.DeviceLik(fn, None)
    _lib.check(L.smcmi_set_likelihood_device(dcb._h, 0, C.byref(dl)))
    refused([dcb, a], UNSUPPORTED)                                  # a device callback
    _lib.check(L.smcmi_set_likelihood_device(dcb._h, 0, None))
    dcb.close()
    old = dict(spec)
    old["old_lik"] = ("gauss_iso", [0.75], np.asarray(spec["lik"][2]), None)
    od = make_engine(old, n, 7, ms)
    od.upload_cloud(P0)
    refused([a, od], UNSUPPORTED)                                   # an old-data likelihood
    od.close()
    refused([a, b], UNSUPPORTED, prior_weight=0.3)                  # tempered_update_prior_weight != 0
    refused([a, b], UNSUPPORTED, stop_after_stage=5)
    refused([a, b], UNSUPPORTED, continue_run=True)
    refused([a, b], UNSUPPORTED, alpha=0.9)                         # mixture proposals: refused, not served (include/smcmi.h)
    wide = good(8, sp=models.gauss_spec(d=11))
    refused([wide], UNSUPPORTED)                                    # n_para > 10
    wide.close()
    big = good(8, nn=8193)
    refused([big], UNSUPPORTED)                                     # n_parts above SMCMI_ENS_MAX_PARTS
    big.close()
    # ... and the two handles every refusal left alone still run
    rs = run_ensemble([a, b], n_phi=10)
    assert [r["status"] for r in rs] == [0, 0] and all(r["n_stages"] == 10 for r in rs)
    a.close()
    b.close()
