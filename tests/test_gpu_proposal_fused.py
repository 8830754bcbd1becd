"""The fused proposal of the α = 1, one-random-block segment stage (csrc/stage2.hpp proposal2_fused, the A1F_FUSE bit, taken by the
two-hand-over, one-handle, one-chunk segment units alone, csrc/stage3.hpp): the zero fill of the factor's padded form and the map of the
shuffled free set run in front of the wait for the correction totals, wavefront 0 forms its rows of c²Σ from the totals itself, factors
them and stores what the MH step reads, the other wavefronts write the covariance and the mean beside it, and one barrier ends it where
three stood.  No operation on a value and no order of operations changes, so

  1. a run on segments leaves the bits a run of launches leaves (SMCMI_ENGINE3=0: proposal2 as it always was), and both agree with the
     CPU oracle to tests/test_gpu_parity.py's tolerances;
  2. the paths that must not take it (several random blocks, α < 1, the riding unit of a fixed schedule) keep their bits as well;
  3. a cloud whose proposal covariance has a non-positive pivot ends both kinds of run with the same error at the same stage.

Every adaptive run has one stage that enters its segment at the mutation (the first stage of a launch: its correction ran as launches),
the stage whose proposal nothing in front of it publishes; the result does not report it, so nothing here can assert it beyond the bits.

Every device run of the module is made once, by two worker processes (the engines are chosen by an environment variable the library reads
once per process: segments, launches), and the oracle runs once per case."""
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
_FIRST_FIXED = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
_LAST_FIXED = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
_TWO_FIXED = [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]                             # nf = 8 != d: the fi / ball maps, the generic Cholesky


def _case(d, n, kw, seed=3, fixed=None, identical=False):
    return dict(d=d, n=n, kw=kw, seed=seed, fixed=fixed, identical=identical)


CASES = {}
for _n in (2048, 20_000):                   # 2 048: the workers take each other's rows; 20 000: the gatherers total them
    for _d in (1, 2, 3, 7, 10):             # n_para 1: the generic Cholesky with one row; 2: the smallest chol_full
        CASES["d%d_n%d" % (_d, _n)] = _case(_d, _n, _ADAPT)
    CASES["d10_two_fixed_n%d" % _n] = _case(10, _n, _ADAPT, fixed=_TWO_FIXED)
CASES["d10_first_fixed"] = _case(10, 2048, _ADAPT, fixed=_FIRST_FIXED)
CASES["d10_last_fixed"] = _case(10, 2048, _ADAPT, fixed=_LAST_FIXED)
CASES["d3_two_fixed"] = _case(3, 2048, _ADAPT, fixed=[1, 0, 1])        # nf = 1
CASES["d10_two_steps"] = _case(10, 2048, dict(_ADAPT, n_mh_steps=2))   # the factor is built once and read by two steps
CASES["d10_n512"] = _case(10, 512, _ADAPT)                              # one full block
CASES["d10_n513"] = _case(10, 513, _ADAPT)                              # ... and a block with a single live lane beside it
FUSED_IDS = list(CASES)
CASES["two_blocks_d10"] = _case(10, 2048, dict(_ADAPT, n_blocks=2))
CASES["three_blocks_d10"] = _case(10, 2048, dict(_ADAPT, n_blocks=3))
CASES["mix_d3"] = _case(3, 2048, dict(_ADAPT, alpha=0.9))
CASES["mix_d10"] = _case(10, 2048, dict(_ADAPT, alpha=0.9))
CASES["fixed_schedule_d10"] = _case(10, 2048, dict(use_fixed_schedule=True, n_phi=20))         # the riding unit
OTHER_IDS = ["two_blocks_d10", "three_blocks_d10", "mix_d3", "mix_d10", "fixed_schedule_d10"]
# 2 048 copies of one particle: every centred moment of the cloud is a rounding error or zero, the first pivot is not positive
CASES["identical_d3"] = _case(3, 2048, _ADAPT, identical=True)


def _spec(case):
    spec = models.gauss_spec(case["d"])
    if case["fixed"]:
        spec["fixed"] = list(case["fixed"])
    return spec


def _cloud(case, orc):
    P0 = orc.initial_draw(models.oracle_model(_spec(case)), case["n"], seed=case["seed"])
    if case["identical"]:
        P0 = np.ascontiguousarray(np.repeat(P0[:1], case["n"], axis=0))
    return P0


_WORKER = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from smc_jl_amd.host import _lib
from oracle import oracle as orc
from tests.test_gpu_proposal_fused import CASES, _spec, _cloud
out_dir = %(out)r
for name, case in CASES.items():
    e = Engine(case["n"], case["d"], seed=case["seed"], max_stages=300, store_history=True)
    e.set_model(_spec(case))
    e.upload_cloud(_cloud(case, orc))
    try:
        r = e.run(**case["kw"])
    except _lib.SMCMIError as err:
        np.savez(os.path.join(out_dir, name + ".npz"), failed=1, code=err.code, message=str(err), stage=e.get_loop_state()["stage_index"])
        e.close()
        continue
    rec = e.stage_records(r["n_stages"])
    w, W = e.history(r["n_stages"])
    np.savez(os.path.join(out_dir, name + ".npz"), failed=0, cloud=e.download_cloud(), w=w, W=W, schedule=rec["schedule"], ess=rec["ess"], c_hist=rec["c_hist"],
             accept_hist=rec["accept_hist"], resampled=rec["resampled"], logmdd=np.float64(r["logmdd"]), c=np.float64(r["c"]), accept=np.float64(r["accept"]),
             n_stages=r["n_stages"], resamples=r["resamples"], n_segments=r["n_segments"], segment_stages=r["segment_stages"],
             segment_state=r["segment_state"], segment_timeouts=r["segment_timeouts"])
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
            done[name] = orc.smc_run(m, _cloud(case, orc), seed=case["seed"], n_threads=8, history=True, **case["kw"])
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


def _segments_against_launches(name, segments, launches, oracle_run):
    a, b, r = segments[name], launches[name], oracle_run(name)
    assert int(a["failed"]) == 0 and int(b["failed"]) == 0
    print(name, "stages", int(a["n_stages"]), "resamples", int(a["resamples"]), "segments", int(a["n_segments"]), "segment stages", int(a["segment_stages"]))
    assert int(b["n_segments"]) == 0 and int(a["n_segments"]) >= 1 and int(a["segment_timeouts"]) == 0 and int(a["segment_state"]) == 1
    assert int(a["resamples"]) >= 1
    _same_bits(a, b)
    _against_oracle(a, r, CASES[name]["n"])
    _against_oracle(b, r, CASES[name]["n"])
    return a, r


@pytest.mark.parametrize("name", FUSED_IDS)
def test_fused_proposal_segments_leave_the_bits_of_the_launches(name, segments, launches, oracle_run):
    a, r = _segments_against_launches(name, segments, launches, oracle_run)
    # the run's stages ran in the segment kernel, not beside it.  (One free parameter: the predicted ϕ_n does not verify in the early stages of
    # an adaptive schedule at n_para 1-2 - DESIGN §9 item 10, a property of the predictor, not of the proposal - and the segments leave for
    # launches; what the fused path needs is a stage inside a segment at all.)
    case = CASES[name]
    nf = case["d"] - sum(case["fixed"] or [])
    assert int(a["segment_stages"]) >= ((int(a["n_stages"]) - 1) // 2 if nf >= 2 else 1)
    assert float(a["logmdd"]) == pytest.approx(r["logmdd"], abs=1e-6)


@pytest.mark.parametrize("name", OTHER_IDS)
def test_paths_that_do_not_fuse_keep_their_bits(name, segments, launches, oracle_run):
    a, _ = _segments_against_launches(name, segments, launches, oracle_run)
    if CASES[name]["kw"]["use_fixed_schedule"]:
        assert int(a["n_stages"]) == 20


def test_non_positive_pivot_is_the_same_error_at_the_same_stage(segments, launches):
    """An error status of the library (SMCMI_ERR_POSDEF, the reference's PosDefException), not a fault of the device.  Should neither
    kind of run fail on this cloud, the runs are held to the same bits instead.  (Both report POSDEF at stage 1 - a stage that runs as
    launches under either engine: the case holds the two to one answer, it does not reach the fused proposal's own failure word.)"""
    a, b = segments["identical_d3"], launches["identical_d3"]
    print("segments:", {k: a[k] for k in ("failed", "code", "stage", "message") if k in a})
    print("launches:", {k: b[k] for k in ("failed", "code", "stage", "message") if k in b})
    assert int(a["failed"]) == int(b["failed"])
    if int(a["failed"]):
        assert int(a["code"]) == int(b["code"]) and int(a["stage"]) == int(b["stage"])
    else:
        _same_bits(a, b)
