#!/usr/bin/env python
"""Record tests/golden/mutation_bits.json: SHA-256 digests of the cloud and of the stage records every register mutation kernel leaves,
for every case of tests/mutation_bits_worker.py, one fresh process per driver on cuda:0.

    SMCMI_LIBRARY=<libsmcmi.so of the commit to record from> python tools/record_mutation_bits.py --commit <its hash>

Every driver runs twice; a case whose two recordings differ is a finding: the recorder lists it and fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mutation_bits_worker as worker  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "mutation_bits.json"))
    ap.add_argument("--commit", default="", help="the commit the library was built from (kept in the fixture)")
    a = ap.parse_args()
    drivers, unstable = {}, []
    for drv in sorted(worker.DRIVERS):
        r1, r2 = worker.run_worker(drv), worker.run_worker(drv)
        unstable += ["%s/%s" % (drv, c) for c in r1 if r1[c] != r2[c]]
        drivers[drv] = r1
        print(drv, json.dumps(r1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(recorded_from=a.commit, n_parts=worker.N_PARTS, drivers=drivers), f, indent=1, sort_keys=True)
        f.write("\n")
    if unstable:
        raise SystemExit("two recordings differ: %s" % unstable)


if __name__ == "__main__":
    main()
