"""The host drivers decide what they decided before csrc/stagepolicy.hpp took their stall and batching rules over: every case of
tests/stall_counters_worker.py - engine 1, engine 2's launches, segments (resampling inside and leaving), the sharded group driver and the
host-closure loop; adaptive, with a starved solver, with a deliberately wrong resample forecast, on a fixed schedule - gives the stage,
resample, pass, stall and segment counts, the log-MDD and the cloud checksum recorded from the commit before it
(tests/golden/stall_counters.json, tools/record_stall_counters.py), exactly."""
import json
import os
import subprocess
import sys

import pytest

from tests import stall_counters_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "stall_counters.json")


@pytest.fixture(scope="module")
def recorded():
    assert os.path.exists(FIXTURE), "tests/golden/stall_counters.json is missing (tools/record_stall_counters.py records it on a GPU)"
    return json.load(open(FIXTURE))["cases"]


@pytest.mark.parametrize("name", sorted(worker.CASES))
def test_driver_decides_as_recorded(recorded, name):
    want = recorded[name]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stall_counters_worker.py"), name], env=worker.case_env(name),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    print(name, got)
    assert {k: got[k] for k in want} == want
    assert not worker.conditions(name, want)          # the case stalls the way its name says (recorded from the parent)
    if name.endswith("_profile"):
        assert "n_mutate_launches" in want and got["kernel_ms_mutate"] > 0.0
