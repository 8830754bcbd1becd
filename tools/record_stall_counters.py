#!/usr/bin/env python
"""Record tests/golden/stall_counters.json: what the host drivers decide - stages, resamples, solver passes, the three kinds of stall,
segments - with the log-MDD and a checksum of the cloud, for every case of tests/stall_counters_worker.py, each in a fresh process on cuda:0.

    SMCMI_LIBRARY=<libsmcmi.so of the commit to record from> python tools/record_stall_counters.py --commit <its hash>

Every case runs twice; a value that differs between the two recordings is left out of the fixture and listed under "unstable".  The
conditions a case is there for (it stalls the way its name says) are checked on what was recorded: a case that misses its condition
needs another seed or target in the worker's table."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import stall_counters_worker as worker  # noqa: E402


def run(name):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stall_counters_worker.py"), name], env=worker.case_env(name),
                         capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "stall_counters.json"))
    ap.add_argument("--commit", default="", help="the commit the library was built from (kept in the fixture)")
    ap.add_argument("cases", nargs="*", help="default: all")
    a = ap.parse_args()
    cases, unstable, unmet = {}, {}, []
    for name in a.cases or sorted(worker.CASES):
        r1, r2 = run(name), run(name)
        keys = worker.KEYS + (("n_mutate_launches",) if name.endswith("_profile") else ())
        diff = [k for k in keys if r1[k] != r2[k]]
        cases[name] = {k: r1[k] for k in keys if k not in diff}
        if diff:
            unstable[name] = {k: [r1[k], r2[k]] for k in diff}
        unmet += [(name, c) for c in worker.conditions(name, r1) + worker.conditions(name, r2)]
        print(name, json.dumps(cases[name]), "UNSTABLE %s" % unstable[name] if diff else "", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(recorded_from=a.commit, cases=cases, unstable=unstable), f, indent=1, sort_keys=True)
        f.write("\n")
    if unmet:
        raise SystemExit("conditions not met on the recorded commit: %s" % sorted(set(unmet)))


if __name__ == "__main__":
    main()
