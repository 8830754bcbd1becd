"""Child process of the handle-lifetime tests (tests/test_gpu_errors.py): creates, uses and destroys handles under SMCMI_POISON_ALLOC=2 and
leaves the library's allocation report on stderr, one "[scenario] <name>" line in front of each scenario; the last stdout line is
"RESULT <json>".  Usage: handle_lifetime_child.py <repository root> create_failure | lifetime <scenario letters>."""
import ctypes as C
import json
import math
import sys

import numpy as np

root, mode = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from smc_jl_amd import Engine, run_group  # noqa: E402
from smc_jl_amd.host import _lib  # noqa: E402
from smc_jl_amd.host.workloads import gauss_spec  # noqa: E402

D = 3
out = {}


def scenario(name):
    sys.stderr.write("[scenario] %s\n" % name)
    sys.stderr.flush()


def engine(n, n_local=None, gid0=0):
    e = Engine(n, D, seed=3, max_stages=400, store_history=True, n_local=n_local, gid0=gid0)
    e.set_model(gauss_spec(D))
    e.init_from_prior()
    return e


def summary(r):
    return [r["n_stages"], bool(math.isfinite(r["logmdd"])), r["n_segments"]]


def one_handle():
    """adaptive run; more proposals per particle (the drawn-ahead buffer regrows); a fixed schedule longer than the adaptive runs' (the schedule buffer regrows)"""
    e = engine(4096)
    runs = [summary(e.run(use_fixed_schedule=False, tempering_target=0.95))]
    e.init_from_prior()
    runs.append(summary(e.run(use_fixed_schedule=False, tempering_target=0.95, n_mh_steps=2, n_blocks=2)))
    e.init_from_prior()
    runs.append(summary(e.run(use_fixed_schedule=True, n_phi=320)))
    e.close()
    return runs


def group():
    es = [engine(4096, n_local=2048, gid0=k * 2048) for k in range(2)]
    r = summary(run_group(es, use_fixed_schedule=True, n_phi=40))
    for e in es:
        e.close()
    return [r]


def callbacks():
    import torch

    spec = gauss_spec(D)
    m, sig = np.asarray(spec["lik"][2]).ravel(), float(spec["lik"][1][0])
    c0 = -0.5 * D * math.log(2.0 * math.pi * sig * sig)
    mt = torch.as_tensor(m, device="cuda")
    runs = []
    for dev in (False, True):
        e = engine(2048)
        P0 = e.download_cloud()
        if dev:
            e.set_likelihood_device(lambda th: c0 - ((th - mt) ** 2).sum(dim=1) / (2.0 * sig * sig))
        else:
            e.set_likelihood_callback(lambda th: c0 - ((th - m) ** 2).sum(axis=1) / (2.0 * sig * sig))
        e.upload_cloud(P0)
        runs.append(summary(e.run(use_fixed_schedule=True, n_phi=20)))
        e.close()
    return runs


if mode == "create_failure":
    scenario("failure")
    L = _lib.lib()
    cfg = _lib.Config(2 ** 40, 2 ** 40, 0, D, 0, 1, 10, 0)           # the first cloud buffer is 2^40 x 8 doubles: the allocator refuses
    h = C.c_void_p(0x5A5A5A5A)
    out["rc"] = L.smcmi_create(C.byref(cfg), C.byref(h))
    out["message"] = L.smcmi_last_error().decode()
    out["handle_untouched"] = h.value == 0x5A5A5A5A
    scenario("next")
    e = engine(4096)
    out["next"] = summary(e.run(use_fixed_schedule=False, tempering_target=0.95))
    e.close()
else:
    for s in sys.argv[3]:
        scenario(s)
        out[s] = {"a": one_handle, "c": group, "d": callbacks}[s]()
    scenario("end")
print("RESULT " + json.dumps(out))
