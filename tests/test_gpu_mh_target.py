"""The MH step's target in the two-hand-over, one-handle, one-chunk segment kernels (csrc/stage2.hpp A1F_BOUNDS, A1F_PRIOR; csrc/model.hpp
in_bounds_flat, logprior_normal_rb): the bounds check without its chain of branches, and - where no parameter is fixed and every prior is
Normal - the log-prior from the reciprocal standard deviations the host formed (csrc/bmmath.hpp bm_div_rb_core; tests/test_divrb_cpu.py
holds the helper itself against the division).  Both are the same operations on the same values, so a run through the segment kernel must
leave the bits a run of engine 2's launches leaves (SMCMI_ENGINE3=0: k2_mutate keeps in_bounds_s / logprior_s, which makes it an
independent reference): cloud, stage records, both histories, log-MDD.

Shapes: n_para 1, 3, 10; 513 and 1 025 particles (a block with one live lane), 1 023 (one dead lane), 4 096; a short adaptive schedule and
a short fixed one (with exact energy shifts, SMCMI_SHIFT_LAG=0: lagged shifts would take the riding kernel, whose text is the one it was).
Models (an isotropic Gaussian likelihood throughout):
  normal            every prior Normal: the reciprocal path
  mixed             Normal and Uniform alternating: logprior_s behind the flat bounds check
  uniform           n_para 1: the one prior Uniform
  fixed_first/last  one fixed parameter whose value EQUALS its lower / upper bound (a fixed parameter is the one a proposal leaves where it
                    is, so `lo <= x` / `x <= hi` are decided by equality in every proposal)
  gamma             one Gamma prior: the rolled copy of prior_logpdf (PRIOR_HAS_OTHER)
  sd_1e-200, sd_1e200   a Normal whose standard deviation bm_div_rb does not admit: the host clears PRIOR_NORMAL_RB, the model divides
                    (sd 1e-200 at n_para 3 only, see below)
  mean_1e160        a Normal(1e160, 1e10): its standard deviation is admitted, x - 1e160 is beyond the admitted dividends in every lane - the
                    reciprocal path's own `/` branch
  tight_first/middle/last   bounds of +- 0.2 about the likelihood's mean on that parameter alone: a large share of the proposals falls
                    outside on it and on no other
A cloud the model's own prior cannot draw inside its bounds (sd 1e200) or not usefully (sd 1e-200, mean 1e160) is drawn from the plain
Gaussian model's prior and uploaded; the segment run and the reference start from the same array.
One child process per (engine, environment) runs every case: switches are read once per process."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TARGET = {1: 0.96, 3: 0.88, 10: 0.78}             # 30-40 adaptive stages of the Gaussian at 1 / 3 / 10 parameters
_A, _F = "adaptive", "fixed"


def _kw(d, sched):
    return dict(use_fixed_schedule=False, tempering_target=_TARGET[d]) if sched == _A else dict(use_fixed_schedule=True, n_phi=20)


def spec_of(model, d):
    """(spec, proxy): proxy = draw the cloud from the plain Gaussian model's prior."""
    from tests import models
    spec = models.gauss_spec(d)
    pri, bnd, fx = list(spec["priors"]), list(spec["bounds"]), [0] * d
    m = [float(v) for v in spec["lik"][2].ravel()]
    proxy = False
    mid = {"first": 0, "middle": d // 2, "last": d - 1}
    if model == "normal":
        pass
    elif model == "mixed":
        for k in range(1, d, 2):
            pri[k], bnd[k] = ("uniform", -6.0, 6.0), (-6.0, 6.0)
    elif model == "uniform":
        pri[0], bnd[0] = ("uniform", -6.0, 6.0), (-6.0, 6.0)
    elif model == "fixed_first":
        fx[0], pri[0], bnd[0] = 1, ("normal", 0.5, 5.0), (0.5, 1e5)
    elif model == "fixed_last":
        fx[d - 1], pri[d - 1], bnd[d - 1] = 1, ("normal", 0.5, 5.0), (-1e5, 0.5)
    elif model == "gamma":
        pri[d - 1], bnd[d - 1] = ("gamma", 2.0, 1.0), (1e-9, 1e5)
    elif model == "sd_1e-200":
        pri[0], proxy = ("normal", 0.0, 1e-200), True
    elif model == "sd_1e200":
        pri[d - 1], proxy = ("normal", 0.0, 1e200), True
    elif model == "mean_1e160":
        pri[0], proxy = ("normal", 1e160, 1e10), True
    elif model.startswith("tight_"):
        k = mid[model[6:]]
        pri[k], bnd[k] = ("normal", m[k], 0.25), (m[k] - 0.2, m[k] + 0.2)
    else:
        raise KeyError(model)
    spec["priors"], spec["bounds"], spec["fixed"] = pri, bnd, fx
    return spec, proxy


CASES = {}


def _add(model, d, n, sched):
    CASES["%s-d%d-n%d-%s" % (model, d, n, sched)] = dict(model=model, d=d, n=n, sched=sched, seed=3)


for _d in (1, 3, 10):
    for _n in (513, 1025, 1023, 4096):
        _add("normal", _d, _n, _A)
    _add("normal", _d, 1025, _F)
for _m in ("mixed", "fixed_first", "fixed_last", "gamma", "sd_1e200", "mean_1e160", "tight_first", "tight_middle", "tight_last"):
    _add(_m, 3, 1025, _A)
    _add(_m, 10, 1023, _A)
    _add(_m, 10, 4096, _F)
for _m in ("uniform", "gamma", "sd_1e200", "mean_1e160"):
    _add(_m, 1, 513, _A)
# sd 1e-200: z = x / 1e-200 overflows when squared, every log-prior is -Inf, -Inf - -Inf = NaN refuses every proposal.  At 10 parameters the
# cloud then degenerates under resampling and either engine ends with the reference's PosDefException: the case runs at n_para 3
_add("sd_1e-200", 3, 1025, _A)

_KEYS = ("n_stages", "resamples", "logmdd", "schedule", "ess", "c_hist", "accept_hist", "resampled", "cloud", "w", "W")

_WORKER = r'''
import json, sys, hashlib
import numpy as np
sys.path.insert(0, %(root)r)
from smc_jl_amd import Engine
from tests import models
from tests.test_gpu_mh_target import CASES, spec_of, _kw
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}
for name, c in CASES.items():
    if c["sched"] != %(sched)r:
        continue
    spec, proxy = spec_of(c["model"], c["d"])
    P0 = None
    if proxy:
        e0 = Engine(c["n"], c["d"], seed=c["seed"], max_stages=400)
        e0.set_model(models.gauss_spec(c["d"]))
        e0.init_from_prior()
        P0 = e0.download_cloud()
        e0.close()
        # the rows carry the plain model's log-prior (column n_para + 1): this model's - every prior of these models is Normal
        pa, pb = (np.array([p[i] for p in spec["priors"]], dtype=np.float64) for i in (1, 2))
        with np.errstate(over="ignore"):
            P0[:, c["d"] + 1] = np.sum(-(((P0[:, :c["d"]] - pa) / pb) ** 2 + np.log(2.0 * np.pi)) / 2.0 - np.log(pb), axis=1)
    e = Engine(c["n"], c["d"], seed=c["seed"], max_stages=400, store_history=True)
    e.set_model(spec)
    if P0 is None:
        e.init_from_prior()
    else:
        e.upload_cloud(P0)
    try:
        r = e.run(**_kw(c["d"], c["sched"]))
    except Exception as ex:                 # (reported with the case's name by the test)
        out[name] = dict(error=repr(ex))
        e.close()
        continue
    rec = e.stage_records(r["n_stages"])
    w, W = e.history(r["n_stages"])
    P = e.download_cloud()
    out[name] = dict(
        n_stages=r["n_stages"], resamples=r["resamples"], logmdd=float(r["logmdd"]).hex(), schedule=h(rec["schedule"]), ess=h(rec["ess"]),
        c_hist=h(rec["c_hist"]), accept_hist=h(rec["accept_hist"]), resampled=h(rec["resampled"]), cloud=h(P), w=h(w), W=h(W),
        n_segments=r["n_segments"], segment_stages=r["segment_stages"], segment_timeouts=r["segment_timeouts"],
        accept_mean=float(np.mean(rec["accept_hist"][1:])))
    e.close()
print("RESULT " + json.dumps(out))
'''


def _runs(sched, engine3_off):
    env = dict(os.environ)
    if sched == _F:
        env["SMCMI_SHIFT_LAG"] = "0"
    if engine3_off:
        env["SMCMI_ENGINE3"] = "0"
    p = subprocess.run([sys.executable, "-c", _WORKER % dict(root=ROOT, sched=sched)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def segments():
    return {**_runs(_A, False), **_runs(_F, False)}


@pytest.fixture(scope="module")
def launches():
    return {**_runs(_A, True), **_runs(_F, True)}


@pytest.mark.parametrize("name", list(CASES))
def test_segment_run_leaves_the_launches_bits(segments, launches, name):
    seg, ref, c = segments[name], launches[name], CASES[name]
    assert "error" not in seg and "error" not in ref, (seg.get("error"), ref.get("error"))
    print(name, "stages", seg["n_stages"], "resamples", seg["resamples"], "segments", seg["n_segments"], "segment stages", seg["segment_stages"],
          "mean acceptance", seg["accept_mean"])
    assert ref["n_segments"] == 0
    assert seg["n_segments"] > 0 and seg["segment_timeouts"] == 0 and seg["segment_stages"] >= (seg["n_stages"] - 1) // 2, seg
    assert seg["n_stages"] >= 12
    for k in _KEYS:
        assert seg[k] == ref[k], (k, seg[k], ref[k])
    # proposals are accepted: the target is evaluated inside the bounds, not only refused
    if c["model"] != "sd_1e-200":
        assert seg["accept_mean"] > 0.02, seg["accept_mean"]
