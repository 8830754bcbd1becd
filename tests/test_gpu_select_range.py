"""Every resampler against the exact reference of tests/select_ref.py.

Selection is the one step whose result is an integer per particle, implemented about ten times over (k_resample_gather, k_bridge_gather,
k_anc_ranges; k2_scan / k2_owner_ranges / k2_gather / k2_gather_wide / sel_search_tile; k3_select_inside / k3_select_two; the selection
block of kens_run) on three scan orders and a staged search with two caps (2 048 and 4 096 rows).  The reference holds the weights as exact
integers, so the expected ancestor of every slot is known without a tolerance; what remains open is the slots whose threshold lies within
MARGIN = max(16 x the restatement's cum error, 2^-43) of a boundary (0 on the exact family), where the device may take the neighbouring
positive-weight row on the threshold's side.  tests/test_select_ref_cpu.py pins the reference and checks the clouds' input conditions.

The rule the project follows: a search that falls through, or finds a row of weight 0, takes the nearest row before it with
positive weight.  In force in the restatement, the stand-alone calls, engine 1, engine 2's launches (one handle; several handles that
all-gather), the selection inside segments and the ensemble kernel; not in the all-to-all-v exchange of several handles.
An undecided slot may also take any positive-weight row whose whole interval lies within MARGIN of its threshold (dust rows are narrower).

Stand-alone entries (given offsets and Philox offsets, both methods): Engine.resample, bridge_resample_from with n_out =, < and > n_src,
shard_resample on two handles, api.resample - every family at 5, 257, 1 024 and 4 099 particles (the exact family at the power of two
below), offsets 2^-53, 0.5, 1 - 2^-45, 1 - 2^-53, on exact clouds 0 and multiples of 2^-11 (thresholds ON boundaries), and on clouds with
zero rows the ULP SWEEP: multinomial offsets within +-8 ulp of fl(C_{j-1}) for up to 60 zero-weight rows j and around the final boundary.
Systematic bridging with n_out < n_src keeps quirk Q5 and is compared with the restatement only.  shard_resample and api.resample take no
offsets: they run under Philox offsets alone.

One bracketed stage per engine: the "resample" vehicle of tests/test_gpu_moment_range.py (init_from_prior, download, loglh = 1e6, columns
d+1 .. d+3 = 0, the family's weights, upload, run(stop_after_stage=2, threshold_ratio=0.99)): the stage resampled, acceptance exactly 0, the
w column +inf in every row and the stage's ESS that of the family's weights to 1e-11 (the history keeps the reference's unshifted
increment, exp(δ 1e6) = +inf, not 1.0; the stage works with increments shifted by the common 1e6: exp(0)), the W column 1 - the downloaded rows are P[anc], and every ancestor is recovered by matching all d θ columns bit for
bit (a row travelled whole; columns d .. d+3 are the ancestor's).  Rows: PATHS of tests/test_gpu_weight_range.py, a mixture row (α = 0.9 at
n_para 10: the transit parked in device memory), a multinomial row, and a continued vehicle at k = 5 of the fixed schedule (a riding segment
selects).  Which kernels ran is asserted from the result as tests/test_gpu_weight_range.py _check does.  Sizes: 20 480 (exact: 16 384);
two_chunk_segments: 150 004, no exact family there (150 004 is no power of two), families collapse_ends and zero_ends.

Ensemble (kens_run): one launch per size - 8 192 and 4 096 particles at n_para 10, 1 000 at n_para 3 - whose members carry different families
and seeds; each member is a whole run of the shortest fixed schedule (n_phi = 2).  Two processes on one GPU (world = 2, 16 384 particles,
tests/mp_shard_worker.py with cfg["upload"]): host communicator (mailbox asserted), comm = "rccl" over tests/fake_rccl, and
SMCMI_RESAMPLE_EXCHANGE=allgather, on the collapse_ends and zero_ends families.

Measured on an MI355X (26 tests, 60 s; 1 740 stand-alone calls, 86 bracketed stages, 38 ensemble members, 6 two-process runs):
  * undecided slots: 0 on every bracketed stage, ensemble member and two-process run, every family and path (the closest boundary over all of
    them: 1.9e-9, MARGIN <= 1.1e-10); 0 on the exact family everywhere.  Stand-alone calls under Philox offsets and the given systematic
    offsets: collapse_ends 34, collapse_apart 62 and chunk_ends 28 over all sizes and entries (at most 2 per call: thresholds k / n_out on
    boundaries j / (c1 + c2) of these structured clouds), 0 on the other families; the offsets placed on purpose (ulp sweep, ends of [0, 1))
    are undecided by construction - about 12 000 slots per size - and every one of them took the reference's row or the neighbour on the
    threshold's side, none a row of weight 0.
  * widest 512-slot tile of a stage: collapse_ends 19 856 rows (beyond both caps), collapse_apart 3 016 (between G_CAP and SEL_CAP); two-chunk
    segments (150 004 particles): collapse_ends 149 367.
  * no path row fell back to another size: every row reached its path at 20 480 / 16 384 particles (segments: 1 segment, 1 stage, no stall;
    launches / engine 1 / large-shard stage: no segment); two_chunk_segments runs at the 150 004 particles tests/test_gpu_weight_range.py uses
    and drops the exact family.
  * on the parent's library (the clamp to the last row, no look at the weight): test_stand_alone_entries fails at all four sizes - 205 of 1 740
    calls.  The end offsets 1 - 2^-45 and 1 - 2^-53 (systematic) and the ulp sweep around a trailing boundary (multinomial, zero_ends: up to 121
    slots of a call) select the last row, weight 0; the ulp sweep around INTERIOR zero-weight rows of the random family selects such rows too (1 to 7
    slots per call at 257, 1 024 and 4 099 particles: the scan's step across a zero-weight row does survive the division by the total).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import select_ref as sr
from tests.test_gpu_weight_range import CONT_K, CONT_KW, FRESH_KW, PATHS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tests/test_gpu_select_range.py"

_COMMON = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from oracle import oracle as orc
from smc_jl_amd import Engine
from smc_jl_amd.host import api, engine as eng
from smc_jl_amd.host._lib import SMCMIError
from tests import models, select_ref as sr
cfg = json.loads(%(cfg)r)
orc.build()
_clouds = {}
def cloud(family, n):
    """(weights, exact reference, MARGIN): once per worker"""
    if (family, n) not in _clouds:
        w = sr.make_cloud(family, n)
        c = sr.Cloud(w)
        _clouds[(family, n)] = (w, c, sr.margin(c, sr.restatement_cum(w), exact=family == "exact"))
    return _clouds[(family, n)]
out = []
def report(entry, family, n, method, label, why, fig, **extra):
    out.append(dict(entry=entry, family=family, n=n, method=method, label=label, why=why, fig=fig, **extra))
'''

_STANDALONE = _COMMON + r'''
d = 2
spec = dict(priors=[("normal", 0.0, 1.0)] * d, bounds=[(-1e9, 1e9)] * d, fixed=[0] * d, lik=("gauss_iso", [1.0], np.zeros((d, 1)), None), old_lik=None)
def engine(n, n_parts=None, gid0=0):
    """a handle of n rows: a whole cloud, or (n_parts given) the shard [gid0, gid0 + n) of a cloud of n_parts"""
    e = Engine(n_parts or n, d, seed=sr.SEED, max_stages=4, store_history=False, n_local=n if n_parts else None, gid0=gid0)
    e.set_model(spec)
    return e
def particles(n, w, rng):
    P = np.zeros((n, d + 5), order="F")
    P[:, :d + 4] = rng.normal(size=(n, d + 4))
    P[:, d + 4] = w
    return P
for family, n in cfg["cases"]:
    w, c, mg = cloud(family, n)
    rng = np.random.default_rng(n)
    P = particles(n, w, rng)
    e = engine(n)
    sizes = sorted({n, n // 2 + 1, n + n // 3 + 1})
    dsts = {m: engine(m) for m in sizes}
    for method in ("systematic", "multinomial"):
        # ---- Engine.resample and bridge_resample_from: given offsets, then Philox
        for n_out in sizes:
            if method == "systematic":
                sets = [("u=%%r" %% u, [u], None) for u in sr.systematic_offsets(family)]
            else:
                sets = [("given %%d" %% i, o, m) for i, (o, m) in enumerate(sr.multinomial_offsets(c, family, n_out))]
            sets.append(("philox", None, None))
            q5 = method == "systematic" and n_out < n
            for label, off, exempt in sets:
                given = off if off is not None else orc.resample_offsets(method, n_out, seed=sr.SEED, stage=sr.STAGE)
                ref = c.select(method, n_out, given)
                if q5:                                   # quirk Q5 (search range 1:n_out): the restatement alone, wherever the slot is decided
                    want = orc.resample(w, method, n_parts=n_out, offsets=given)
                    dec = ~(ref["dist"] <= mg)
                entries = [("bridge", n_out)] + ([("resample", n)] if n_out == n else [])
                for entry, _ in entries:
                    e.upload_cloud(P)
                    if entry == "resample":
                        anc = e.resample(method, stage=sr.STAGE, offsets=off)
                        Q = e.download_cloud()
                        rows_ok = bool(np.array_equal(Q[:, :d + 4], P[anc.clip(0, n - 1), :d + 4]) and np.all(Q[:, d + 4] == 1.0))
                    else:
                        dst = dsts[n_out]
                        anc = dst.bridge_resample_from(e, n_out, method=method, stage=sr.STAGE, offsets=off)
                        Q = dst.download_cloud()
                        rows_ok = bool(np.array_equal(Q[:n_out], P[anc.clip(0, n - 1)]))      # whole rows, old weights included
                    if q5:
                        wrong = int(np.count_nonzero((anc != want) & dec))
                        why = ["%%d decided slots differ from the restatement (Q5)" %% wrong] if wrong else []
                        fig = dict(undecided=int(np.count_nonzero(~dec)), wrong=wrong, zero=int(np.count_nonzero(w[anc.clip(0, n - 1)] <= 0)))
                        # (rows n_out .. n - 1 are out of reach: a cloud with no weight in front of them leaves only rows of weight 0)
                        if (fig["zero"] and np.any(w[:n_out] > 0)) or np.any(np.diff(anc) < 0) or anc.min() < 0 or anc.max() >= n_out:
                            why.append("Q5: an ancestor of weight 0, out of 1:n_out, or a decreasing sequence")
                    else:
                        why, fig = sr.judge(ref, anc, w, mg, method, exempt=exempt, cloud=c)
                    if not rows_ok:
                        why.append("the gathered rows are not the ancestors' rows")
                    report(entry, family, n, method, "%%s n_out=%%d" %% (label, n_out), why, fig)
        # ---- api.resample (Philox; seed / stage of the call)
        for n_out in sizes:
            anc = api.resample(w, n_parts=n_out, method=method, seed=sr.SEED, stage=sr.STAGE)
            given = orc.resample_offsets(method, n_out, seed=sr.SEED, stage=sr.STAGE)
            ref = c.select(method, n_out, given)
            if method == "systematic" and n_out < n:
                want = orc.resample(w, method, n_parts=n_out, offsets=given)
                wrong = int(np.count_nonzero((anc != want) & ~(ref["dist"] <= mg)))
                why = ["%%d decided slots differ from the restatement (Q5)" %% wrong] if wrong else []
                fig = dict(undecided=int(np.count_nonzero(ref["dist"] <= mg)), wrong=wrong, zero=int(np.count_nonzero(w[anc.clip(0, n - 1)] <= 0)))
                if (fig["zero"] and np.any(w[:n_out] > 0)) or np.any(np.diff(anc) < 0) or anc.min() < 0 or anc.max() >= n_out:
                    why.append("Q5: an ancestor of weight 0, out of 1:n_out, or a decreasing sequence")
            else:
                why, fig = sr.judge(ref, anc, w, mg, method, cloud=c)
            report("api", family, n, method, "philox n_out=%%d" %% n_out, why, fig)
        # ---- shard_resample on two handles (Philox): the all-gathered cloud as a torch tensor [R, N]
        if n >= 2:
            import torch
            full = torch.as_tensor(np.ascontiguousarray(P.T), device="cuda")
            ref = c.select(method, n, orc.resample_offsets(method, n, seed=sr.SEED, stage=sr.STAGE))
            got, rows_ok = [], True
            for g0, nl in ((0, n // 2), (n // 2, n - n // 2)):
                s = engine(nl, n_parts=n, gid0=g0)
                s.upload_cloud(P[g0:g0 + nl])
                a = s.shard_resample(full[d + 4], full, method, sr.STAGE)
                Q = s.download_cloud()
                rows_ok = rows_ok and bool(np.array_equal(Q[:, :d + 4], P[a.clip(0, n - 1), :d + 4]) and np.all(Q[:, d + 4] == 1.0))
                got.append(a)
                s.close()
            why, fig = sr.judge(ref, np.concatenate(got), w, mg, method, cloud=c)
            if not rows_ok:
                why.append("the gathered rows are not the ancestors' rows")
            report("shard", family, n, method, "philox", why, fig)
    for x in dsts.values():
        x.close()
print("RESULT " + json.dumps(out))
'''

_STAGE = _COMMON + r'''
spec = models.gauss_spec(*cfg.get("spec_args", [10]))
d = len(spec["priors"])
shards = cfg.get("shards", 1)
def run(es, **kw):
    return eng.run_group(es, **kw) if shards > 1 else es[0].run(**kw)
for family, n in cfg["cases"]:
    w, c, mg = cloud(family, n)
    for method in cfg["methods"]:
        o = dict(error="")
        es = []
        try:
            for r in range(shards):
                e = Engine(n, d, seed=sr.SEED, max_stages=48, store_history=True, n_local=n // shards, gid0=r * (n // shards))
                e.set_model(spec)
                e.init_from_prior()
                es.append(e)
            kw = dict(cfg["kw"], resampling_method=method)
            k = cfg["k"]
            P0 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            if k > 2:                                   # continued vehicle: a benign run paused after stage k - 1
                r = run(es, stop_after_stage=k - 1, **kw)
                assert r["paused"], r
            P = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            P[:, :d] = P0[:, :d]                        # (a cloud that has resampled repeats rows: the prior draw's θ, distinct row by row)
            P[:, d], P[:, d + 1], P[:, d + 2], P[:, d + 3], P[:, d + 4] = 1e6, 0.0, 0.0, 0.0, w
            for q, e in enumerate(es):
                e.upload_cloud(np.asfortranarray(P[q * (n // shards):(q + 1) * (n // shards)]))
            r = run(es, stop_after_stage=k, threshold_ratio=0.99, continue_run=k > 2, **kw)
            P1 = np.asfortranarray(np.concatenate([e.download_cloud() for e in es], axis=0))
            rec = es[0].stage_records(r["n_stages"])
            hs = [e.history(r["n_stages"]) for e in es]
            wh = np.concatenate([h[0] for h in hs], axis=0)[:, k - 1]
            Wh = np.concatenate([h[1] for h in hs], axis=0)[:, k - 1]
            o["vehicle"] = dict(n_stages=r["n_stages"], resampled=int(rec["resampled"][k - 1]), accept=float(rec["accept_hist"][k - 1]),
                                ess=[float(rec["ess"][k - 1]), sr.ess(w)],
                                w_col=[float(wh.min()), float(wh.max())], W_col=[float(Wh.min()), float(Wh.max())],
                                W_cloud=[float(P1[:, d + 4].min()), float(P1[:, d + 4].max())])
            o["segments"] = [r["n_segments"], r["segment_stages"]]
            o["stalls"] = [r["solver_stalls"], r["select_stalls"], r["spec_stalls"], r["segment_timeouts"]]
            o["fallback"] = r["shift_fallback_stage"]
            # the ancestors: all d θ columns matched bit for bit
            keys = {P[i, :d].tobytes(): i for i in range(n)}
            assert len(keys) == n, "the prior draw repeats a row"
            anc = np.array([keys.get(P1[i, :d].tobytes(), -1) for i in range(n)], dtype=np.int64)
            o["unmatched"] = int(np.count_nonzero(anc < 0))
            o["tail_ok"] = bool(np.array_equal(P1[:, d:d + 4], P[anc.clip(0, n - 1), d:d + 4]))
            given = orc.resample_offsets(method, n, seed=sr.SEED, stage=k)
            ref = c.select(method, n, given)
            why, fig = sr.judge(ref, anc, w, mg, method, cloud=c)
            fig["span"] = sr.widest_tile_span(ref["anc"]) if method == "systematic" else 0
            fig["distinct"] = int(np.unique(ref["anc"]).size)
        except SMCMIError as ex:
            o["error"] = str(ex)[:200]
            why, fig = ["error"], {}
        for e in es:
            e.close()
        report("stage", family, n, method, cfg["label"], why, fig, n_para=d, **o)
print("RESULT " + json.dumps(out))
'''


def _spawn(code, cfg, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, "-c", code % dict(root=ROOT, cfg=json.dumps(cfg))], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if p.returncode < 0 or p.returncode in (134, 139):              # the worker died of a signal: nothing more is started on that GPU by this file
        pytest.exit("a worker of %s died with status %d:\n%s" % (NAME, p.returncode, p.stderr[-3000:]), returncode=3)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _check(res):
    """Every figure is printed before anything is asserted."""
    for o in res:
        print(json.dumps(o))
    bad = [(o["entry"], o["family"], o["n"], o["method"], o["label"], o["why"]) for o in res if o["why"]]
    print("%d calls, %d fail; undecided slots in all: %d" % (len(res), len(bad), sum(o["fig"].get("undecided", 0) for o in res)))
    assert res
    for o in res:
        if o["family"] == "exact":
            assert o["fig"].get("undecided", 0) == 0, o
    assert not bad, "%d of %d calls:\n" % (len(bad), len(res)) + "\n".join(map(repr, bad))


# ------------------------------------------------------------------------------------------------ the stand-alone entries
@pytest.mark.parametrize("n", sr.SMALL_SIZES)
def test_stand_alone_entries(n):
    """Engine.resample, bridge_resample_from (n_out =, <, > n_src), shard_resample on two handles and api.resample: every family and the
    degenerate clouds at one size, given offsets (the ends of [0, 1), thresholds on boundaries, the ulp sweep) and Philox offsets."""
    cases = [(f, m) for f, m in sr.small_cases() if (m == n and f != "exact") or (f == "exact" and m == sr.exact_size(n))]
    if n == sr.SMALL_SIZES[0]:
        cases.append(("single", 1))
    _check(_spawn(_STANDALONE, dict(cases=cases)))


# ------------------------------------------------------------------------------------------------ one bracketed stage per engine
def _stage(path, label, cases, methods=("systematic",), kw=None, k=2, env_extra=None):
    env, over, seg = PATHS[path]
    cfg = dict(cases=cases, methods=list(methods), kw=dict(FRESH_KW if k == 2 else CONT_KW, **(kw or {})), k=k, label=label, **over)
    res = _spawn(_STAGE, cfg, dict(env, **(env_extra or {})))
    _check(res)
    for o in res:
        v = o["vehicle"]
        # the vehicle holds: the stage resampled, no proposal was accepted, the incremental weights are ONE constant (exp(δ 1e6) = +inf as the
        # history keeps them) - so the selection saw the family's weights: the stage's ESS is that of the family's weights - the W history column and the cloud's weights are 1: the downloaded
        # rows are then P[anc].  (The w history column holds the reference's UNSHIFTED increment exp(δ 1e6) = +inf in every row, not 1.0; the
        # increments the stage works with are shifted by the cloud's largest energy, the common 1e6, and are exp(0).)
        assert v["n_stages"] == k and v["resampled"] == 1 and v["accept"] == 0.0, o
        assert v["w_col"] == [float("inf"), float("inf")], o
        assert abs(v["ess"][0] - v["ess"][1]) <= 1e-11 * v["ess"][1], o
        assert v["W_col"] == [1.0, 1.0] and v["W_cloud"] == [1.0, 1.0], o
        assert o["unmatched"] == 0 and o["tail_ok"], o
        assert o["fig"]["distinct"] >= 50 * o["n_para"], o                     # a condition on the input
        if seg:
            assert o["segments"][1] >= seg and o["stalls"] == [0, 0, 0, 0] and o["fallback"] == 0, o
        if seg is False:
            assert o["segments"][0] == 0, o
    return res


def _cases(path):
    n = PATHS[path][1].get("n")
    if n:                                               # two_chunk_segments: 150 004 particles, no exact family (no power of two)
        return [(f, n) for f in sr.TWO_CHUNK_FAMILIES]
    return sr.stage_cases()


@pytest.mark.parametrize("path", list(PATHS))
def test_one_stage_selects_the_reference_ancestors(path):
    res = _stage(path, path, _cases(path))
    spans = {o["family"]: o["fig"]["span"] for o in res}
    print("widest tile spans", spans)
    assert spans["collapse_ends"] > 4096                                        # beyond both staging caps
    if "collapse_apart" in spans:
        assert 2048 < spans["collapse_apart"] <= 4096                           # between G_CAP and SEL_CAP


def test_one_stage_mixture_proposals_with_the_transit_in_device_memory():
    _stage("segments", "mixture", sr.stage_cases(), kw=dict(alpha=0.9))


@pytest.mark.parametrize("path", ["segments", "launches", "engine1"])
def test_one_stage_multinomial(path):
    _stage(path, path + " multinomial", sr.stage_cases(), methods=("multinomial",))


@pytest.mark.parametrize("path", ["segments", "launches"])
def test_continued_stage_selects_the_reference_ancestors(path):
    """A benign run paused after stage 4 of the fixed schedule, the vehicle's columns, upload, stage 5: inside segments the stage rides."""
    _stage(path, path + " continued", sr.stage_cases(), k=CONT_K)


# ------------------------------------------------------------------------------------------------ the ensemble kernel
ENS_KW = dict(use_fixed_schedule=True, n_phi=2, lam=1.0, threshold_ratio=0.99)      # the shortest fixed schedule: stage 2 alone (ϕ: 0 -> 1)

_ENSEMBLE = _COMMON + r'''
from smc_jl_amd import run_ensemble
n, d, families = cfg["n"], cfg["d"], cfg["families"]
spec = models.gauss_spec(d)
for method in ("systematic", "multinomial"):
    es, Ps = [], []
    for m, family in enumerate(families):               # members of one launch carry different families and seeds
        e = Engine(n, d, seed=sr.SEED + m, max_stages=8, store_history=True)
        e.set_model(spec)
        e.init_from_prior()
        P = e.download_cloud()
        P[:, d], P[:, d + 1], P[:, d + 2], P[:, d + 3], P[:, d + 4] = 1e6, 0.0, 0.0, 0.0, cloud(family, n)[0]
        e.upload_cloud(P)
        es.append(e); Ps.append(P)
    rs = run_ensemble(es, resampling_method=method, **cfg["kw"])
    for m, family in enumerate(families):
        w, c, mg = cloud(family, n)
        e, P, r = es[m], Ps[m], rs[m]
        P1 = e.download_cloud()
        rec = e.stage_records(r["n_stages"])
        wh, Wh = e.history(r["n_stages"])
        o = dict(status=[r["status"], r["call_status"]], n_stages=r["n_stages"], resampled=[int(x) for x in rec["resampled"][:r["n_stages"]]],
                 ess=[float(rec["ess"][1]), sr.ess(w)],
                 accept=[float(x) for x in rec["accept_hist"][:r["n_stages"]]], w_col=[float(wh[:, 1].min()), float(wh[:, 1].max())],
                 W_col=[float(Wh[:, 1].min()), float(Wh[:, 1].max())], W_cloud=[float(P1[:, d + 4].min()), float(P1[:, d + 4].max())])
        keys = {P[i, :d].tobytes(): i for i in range(n)}
        assert len(keys) == n, "the prior draw repeats a row"
        anc = np.array([keys.get(P1[i, :d].tobytes(), -1) for i in range(n)], dtype=np.int64)
        o["unmatched"] = int(np.count_nonzero(anc < 0))
        o["tail_ok"] = bool(np.array_equal(P1[:, d:d + 4], P[anc.clip(0, n - 1), d:d + 4]))
        ref = c.select(method, n, orc.resample_offsets(method, n, seed=sr.SEED + m, stage=2))
        why, fig = sr.judge(ref, anc, w, mg, method, cloud=c)
        fig["distinct"] = int(np.unique(ref["anc"]).size)
        report("ensemble", family, n, method, "member %%d" %% m, why, fig, n_para=d, **o)
    for e in es:
        e.close()
print("RESULT " + json.dumps(out))
'''


@pytest.mark.parametrize("n", list(sr.ensemble_cases()))
def test_ensemble_members_select_the_reference_ancestors(n):
    """run_ensemble neither pauses nor continues: each member is a whole run of the shortest fixed schedule (n_phi = 2: stage 2 alone), its
    cloud uploaded as in the stage vehicle - stage 2 resamples, acceptance 0, so the final cloud is P[anc].  Members of one launch carry
    different families and seeds."""
    d, families = sr.ensemble_cases()[n]
    res = _spawn(_ENSEMBLE, dict(n=n, d=d, families=list(families), kw=ENS_KW))
    _check(res)
    for o in res:
        assert o["status"] == [0, 0] and o["n_stages"] == ENS_KW["n_phi"], o
        assert o["resampled"][1] == 1 and not any(o["resampled"][2:]) and not any(o["accept"][1:]), o  # stage 2 resamples, no later stage does; (accept[0]: the start value)
        assert o["w_col"] == [float("inf"), float("inf")] and abs(o["ess"][0] - o["ess"][1]) <= 1e-11 * o["ess"][1], o    # (see _stage)
        assert o["W_col"] == [1.0, 1.0] and o["W_cloud"] == [1.0, 1.0], o
        assert o["unmatched"] == 0 and o["tail_ok"], o
        assert o["fig"]["distinct"] >= 50 * o["n_para"], o


# ------------------------------------------------------------------------------------------------ two processes on one GPU
def mp_cloud(family, n=sr.MP_N, d=10, seed=77):
    """the cloud a two-process run uploads: the stage vehicle's columns on θ drawn here (N(0, 1): inside the Gaussian workload's prior)"""
    P = np.zeros((n, d + 5), order="F")
    P[:, :d] = np.random.default_rng(seed).normal(size=(n, d))
    P[:, d], P[:, d + 4] = 1e6, sr.make_cloud(family, n)
    return P


@pytest.mark.parametrize("family", sr.MP_FAMILIES)
@pytest.mark.parametrize("transport", ["host", "rccl", "allgather"])
def test_two_processes_select_the_reference_ancestors(transport, family, tmp_path):
    """world = 2, 16 384 particles in all, each rank uploads its rows of a cloud this test wrote and runs the one bracketed stage: over the
    host communicator (mailbox active), over comm = "rccl" on tests/fake_rccl, and with SMCMI_RESAMPLE_EXCHANGE=allgather."""
    from tests.test_gpu_multiproc import _spawn as spawn_ranks

    n, d = sr.MP_N, 10
    P = mp_cloud(family)
    path = str(tmp_path / "upload.npy")
    np.save(path, P)
    env = {}
    if transport == "rccl":
        fake = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
        subprocess.check_call(["make", "-C", os.path.dirname(fake), "libfake_rccl.so"], stdout=subprocess.DEVNULL, timeout=120)
        env["SMCMI_RCCL_PATH"] = fake
    if transport == "allgather":
        env["SMCMI_RESAMPLE_EXCHANGE"] = "allgather"
    cfg = dict(n=n, d=d, seed=sr.SEED, comm="rccl" if transport == "rccl" else "host", upload=path, stop_at=2, full_records=True, max_stages=48,
               kw=dict(FRESH_KW, threshold_ratio=0.99))
    try:
        runs, P1 = spawn_ranks(2, cfg, tmp_path, env_extra=env, timeout=300)
    except AssertionError as ex:                        # a rank that died of a signal: nothing more is started on that GPU by this file
        if any("rc %d" % c in str(ex) for c in (-6, -11, 134, 139)):
            pytest.exit("a rank of %s died of a signal:\n%s" % (NAME, str(ex)[-3000:]), returncode=3)
        raise
    w = P[:, d + 4].copy()
    c = sr.Cloud(w)
    mg = sr.margin(c, sr.restatement_cum(w))
    from oracle import oracle as orc

    orc.build()
    ref = c.select("systematic", n, orc.resample_offsets("systematic", n, seed=sr.SEED, stage=2))
    keys = {P[i, :d].tobytes(): i for i in range(n)}
    anc = np.array([keys.get(P1[i, :d].tobytes(), -1) for i in range(n)], dtype=np.int64)
    why, fig = sr.judge(ref, anc, w, mg, "systematic", cloud=c)
    print(transport, family, fig, "span", sr.widest_tile_span(ref["anc"]), [r[0]["mailbox"] for r in runs], [r[0]["segments"] for r in runs], why)
    for rr in runs:
        r = rr[0]
        assert r["n_stages"] == 2 and r["resampled_values"][1] == 1 and r["accept_values"][1] == 0.0, r
        if transport == "host":
            assert r["mailbox"] is True, r
    assert int(np.count_nonzero(anc < 0)) == 0 and np.array_equal(P1[:, d:d + 4], P[anc, d:d + 4]) and np.all(P1[:, d + 4] == 1.0)
    assert np.unique(ref["anc"]).size >= 50 * d
    assert not why, why
