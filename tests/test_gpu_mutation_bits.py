"""The Metropolis-Hastings move of the register kernels (n_para <= 10) leaves the bits it left before its proposal step and its draws were
written once for all of them (csrc/kernels.hpp mh_draw / mh_step): every case of tests/mutation_bits_worker.py - engine 1's k_mutate_reg,
engine 2's k2_mutate and k2b_mutate, the segment kernel; α = 1 and mixture proposals, one and three blocks, odd and even n_para, fixed
parameters, a fixed schedule, the other prior families, and two stand-alone mutate calls (k_mutate_reg's in-kernel draws) - gives the
SHA-256 of the downloaded cloud and of the stage records (schedule, ess, c_hist, accept_hist, resampled, logmdd) recorded from the commit
before it (tests/golden/mutation_bits.json, tools/record_mutation_bits.py), exactly.  One worker process per driver runs all its cases."""
import json
import os

import pytest

from tests import mutation_bits_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mutation_bits.json")


@pytest.fixture(scope="module")
def recorded():
    assert os.path.exists(FIXTURE), "tests/golden/mutation_bits.json is missing (tools/record_mutation_bits.py records it on a GPU)"
    return json.load(open(FIXTURE))["drivers"]


@pytest.mark.parametrize("driver", sorted(worker.DRIVERS))
def test_mutation_leaves_the_recorded_bits(recorded, driver):
    want = recorded[driver]
    assert sorted(want) == sorted(list(worker.RUNS) + (list(worker.MUTATES) if driver == worker.MUTATE_DRIVER else []))
    got = worker.run_worker(driver)
    for case in sorted(want):
        print(driver, case, got[case])
    for case in worker.RUNS:            # each case runs the kernel it is there for (recorded from the parent, and now)
        for r in (want[case], got[case]):
            assert (r["n_segments"] >= 1) if driver == "segments" else (r["n_segments"] == 0), (case, r)
    for case in sorted(want):
        assert got[case] == want[case], case
