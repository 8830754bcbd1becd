"""The α = 1 fast path of the proposal (csrc/stage2.hpp proposal2 / k2_mh_steps with the A1F_* bits, taken by the segment kernel's α = 1
variants, csrc/stage3.hpp): the block shuffle runs in front of the wait for the correction totals, no mixture scales are formed, every
wavefront of the MH step forms the log-determinant itself, and with one random block the Cholesky wavefront stores its rows where the
MH step reads them.  None of it changes an operation or its order, so

  1. a run on segments leaves the bits a run of launches leaves (SMCMI_ENGINE3=0, which runs proposal2 as it always was) and both agree
     with the CPU oracle to tests/test_gpu_parity.py's tolerances;
  2. the paths that must not take it (α < 1, several random blocks, several MH steps) keep their bits as well;
  3. the log-determinant's only α = 1 reader - the reference's underflow quirk, one comparison in the MH step - decides as the oracle's.

Every device run of the module is made once, by two worker processes (the engines are chosen by an environment variable the library reads
once per process: segments, launches), and the oracle runs once per case."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ADAPT = dict(use_fixed_schedule=False, tempering_target=0.8)          # a resample about every fourth stage
_FLAT = dict(use_fixed_schedule=True, n_phi=6, lam=2.1, c=0.5)
_TWO_FIXED = [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]                             # nf = 8 != d: the generic Cholesky, the fi / ball maps


def _case(d, n, kw, seed=3, fixed=None, flat_s=None):
    return dict(d=d, n=n, kw=kw, seed=seed, fixed=fixed, flat_s=flat_s)


CASES = {}
for _n in (2048, 20_000):                   # 2 048: the workers take each other's rows; 20 000: the gatherers total them
    for _d in (2, 3, 10):                   # n_para 2: the smallest chol_full
        CASES["a1_d%d_n%d" % (_d, _n)] = _case(_d, _n, _ADAPT)
    CASES["a1_d10_two_fixed_n%d" % _n] = _case(10, _n, _ADAPT, fixed=_TWO_FIXED)
CASES["a1_d10_fixed_schedule"] = _case(10, 2048, dict(use_fixed_schedule=True, n_phi=20))       # the riding variant
FAST_IDS = list(CASES)
CASES["mix_d3"] = _case(3, 2048, dict(_ADAPT, alpha=0.9))
CASES["mix_d10"] = _case(10, 2048, dict(_ADAPT, alpha=0.9))
CASES["three_blocks_d10"] = _case(10, 2048, dict(_ADAPT, n_blocks=3))
CASES["two_steps_d10"] = _case(10, 2048, dict(_ADAPT, n_mh_steps=2))
SLOW_IDS = ["mix_d3", "mix_d10", "three_blocks_d10", "two_steps_d10"]
# a flat likelihood under Normal(0, s) priors: the proposal's covariance is the prior's, log det ~ 20 log(c s) - s decides whether the
# underflow quirk rejects nobody (1e30), the particles with large |z|² (1.5e32) or everybody (1e40)
FLAT_S = {"1e30": 1e30, "1.5e32": 1.5e32, "1e40": 1e40}
for _n in (2048, 20_000):
    for _k, _s in FLAT_S.items():
        CASES["flat_s%s_n%d" % (_k, _n)] = _case(10, _n, _FLAT, seed=1, flat_s=_s)
FLAT_IDS = [k for k in CASES if k.startswith("flat_")]


def _spec(case):
    if case["flat_s"] is not None:
        spec = models.gauss_spec(case["d"], 1e45, case["flat_s"])
        spec["bounds"] = [(-1e45, 1e45)] * case["d"]
        return spec
    spec = models.gauss_spec(case["d"])
    if case["fixed"]:
        spec["fixed"] = list(case["fixed"])
    return spec


_WORKER = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from oracle import oracle as orc
from tests import models
from tests.test_gpu_proposal_paths import CASES, _spec
out_dir = %(out)r
for name, case in CASES.items():
    spec = _spec(case)
    P0 = orc.initial_draw(models.oracle_model(spec), case["n"], seed=case["seed"])
    e = Engine(case["n"], case["d"], seed=case["seed"], max_stages=300, store_history=True)
    e.set_model(spec)
    e.upload_cloud(P0)
    r = e.run(**case["kw"])
    rec = e.stage_records(r["n_stages"])
    w, W = e.history(r["n_stages"])
    np.savez(os.path.join(out_dir, name + ".npz"), cloud=e.download_cloud(), w=w, W=W, schedule=rec["schedule"], ess=rec["ess"], c_hist=rec["c_hist"],
             accept_hist=rec["accept_hist"], resampled=rec["resampled"], logmdd=np.float64(r["logmdd"]), c=np.float64(r["c"]), accept=np.float64(r["accept"]),
             n_stages=r["n_stages"], resamples=r["resamples"], n_segments=r["n_segments"], segment_stages=r["segment_stages"])
    e.close()
print("DONE")
'''


def _device_runs(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    with tempfile.TemporaryDirectory() as out:
        p = subprocess.run([sys.executable, "-c", _WORKER % dict(root=ROOT, out=out)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0 and "DONE" in p.stdout, p.stderr[-3000:]
        res = {}
        for name in CASES:
            with np.load(os.path.join(out, name + ".npz")) as z:
                res[name] = {k: z[k] for k in z.files}
        return res


@pytest.fixture(scope="module")
def segments():
    return _device_runs({})


@pytest.fixture(scope="module")
def launches():
    return _device_runs({"SMCMI_ENGINE3": "0"})


@pytest.fixture(scope="module")
def oracle_run():
    from oracle import oracle as orc

    orc.build()
    done = {}

    def run(name):
        if name not in done:
            case = CASES[name]
            m = models.oracle_model(_spec(case))
            P0 = orc.initial_draw(m, case["n"], seed=case["seed"])
            done[name] = orc.smc_run(m, P0, seed=case["seed"], n_threads=8, history=True, **case["kw"])
        return done[name]

    return run


_BITS = ("n_stages", "resamples", "logmdd", "c", "accept", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud", "w", "W")


def _same_bits(a, b):
    for k in _BITS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _against_oracle(g, r, n):
    """tests/test_gpu_parity.py _compare_runs, its tolerances"""
    assert int(g["n_stages"]) == r["n_stages"] and int(g["resamples"]) == r["resamples"]
    np.testing.assert_allclose(g["schedule"], r["schedule"], rtol=1e-9)
    np.testing.assert_allclose(g["ess"], r["ess"], rtol=1e-9)
    np.testing.assert_array_equal(g["resampled"], r["resampled"])
    np.testing.assert_allclose(g["c_hist"], r["c_hist"], rtol=1e-9)
    np.testing.assert_allclose(g["accept_hist"], r["accept_hist"], atol=3.0 / n + 1e-12)


@pytest.mark.parametrize("name", FAST_IDS)
def test_fast_path_segments_leave_the_bits_of_the_launches(name, segments, launches, oracle_run):
    a, b, r = segments[name], launches[name], oracle_run(name)
    assert int(b["n_segments"]) == 0 and int(a["n_segments"]) >= 1 and int(a["segment_stages"]) >= (int(a["n_stages"]) - 1) // 2
    if not CASES[name]["kw"]["use_fixed_schedule"]:
        assert int(a["n_stages"]) >= 12 and int(a["resamples"]) >= 2
    else:
        assert int(a["n_stages"]) == 20
    _same_bits(a, b)
    _against_oracle(a, r, CASES[name]["n"])
    _against_oracle(b, r, CASES[name]["n"])
    assert float(a["logmdd"]) == pytest.approx(r["logmdd"], abs=1e-6)


@pytest.mark.parametrize("name", SLOW_IDS)
def test_other_proposal_paths_keep_their_bits(name, segments, launches):
    a, b = segments[name], launches[name]
    assert int(b["n_segments"]) == 0 and int(a["n_segments"]) >= 1
    _same_bits(a, b)


@pytest.mark.parametrize("name", FLAT_IDS)
def test_log_determinant_decides_the_underflow_quirk_as_the_oracle(name, segments, launches, oracle_run):
    """-(d log 2π + log det + |z|²) / 2 < -745.13: the proposal density underflows in the reference and the move is rejected (kernels.hpp
    mh_step).  Oracle acceptance after the first record (N = 20 000): s = 1e30 ordinary (1.0, 0.40, 0.35, ...); s = 1.5e32: 0.05, 0.09, 0.17,
    0.20, 0.18 - the particles with large |z|², a log-determinant off by one moves these by several points; s = 1e40: exactly 0 everywhere."""
    a, b, r = segments[name], launches[name], oracle_run(name)
    n, s = CASES[name]["n"], CASES[name]["flat_s"]
    assert int(a["n_segments"]) >= 1 and int(b["n_segments"]) == 0
    for g in (a, b):
        assert int(g["n_stages"]) == r["n_stages"] == 6 and int(g["resamples"]) == r["resamples"]
        np.testing.assert_allclose(g["accept_hist"], r["accept_hist"], atol=3.0 / n + 1e-12)
        if s == 1e40:
            assert np.all(g["accept_hist"][1:] == 0.0) and np.all(np.asarray(r["accept_hist"])[1:] == 0.0)
    if s == 1.5e32:
        acc = np.asarray(r["accept_hist"])[1:]
        assert r["resamples"] == 0 and np.all(acc > 0.02) and np.all(acc < 0.3)           # the branch takes a part of the particles, not all, not none
    if s == 1e30:
        assert np.asarray(r["accept_hist"])[2] > 0.3
    _same_bits(a, b)
