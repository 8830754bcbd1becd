"""Posterior summaries on the device (csrc/summary.hip; DESIGN.md "Posterior summaries"): weighted quantiles by selection and the best
particle, against tests/quantile_ref.py (exact rational arithmetic) and numpy.

Sizes: n = 1, 2, 63, 64, 65 (around one wavefront), 1000, 4097, and 6221 = 3 x 2048 + 77 - the kernels give a block of 256 threads 2048
particles, so that is four blocks, the last with a ragged tail of 77; d = 1 and 10, a column subset, probs = (0, 0.05, 0.5, 0.95, 1).

Exact cases carry integer weights in [1, 1024] (every partial sum is exact in any order): the device must return float(reference) bit for
bit.  General weights are compared through bracket(delta = 2^-40 wsum) widened by 2 ulp: 2^-40 allows 8192 roundings of 2^-53 in the
summation tree and is five orders of magnitude below one particle's share at N = 1e7."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

from tests import models
from tests import quantile_ref as qr

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
SIZES = (1, 2, 63, 64, 65, 1000, 4097, 6221)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def exact_cloud(n, d, seed):
    """n x (d + 5): values with ties, negatives, denormals, +-1e300 and a chain of 40 adjacent doubles (no zeros: +0.0 and -0.0 are not
    mixed in a column), integer weights in [1, 1024] with some zeros"""
    rng = np.random.default_rng(seed)
    chain = [1.0]
    for _ in range(39):
        chain.append(math.nextafter(chain[-1], math.inf))
    pool = np.array([-1e300, 1e300, -3.5, 2.5, -5e-324, 5e-324, 2.5e-310, -2.5e-310, -1.0] + chain)
    P = np.zeros((n, d + 5), order="F")
    for j in range(d):
        col = rng.normal(size=n)
        pick = rng.random(n) < 0.6
        col[pick] = rng.choice(pool, size=int(pick.sum()))
        col[rng.random(n) < 0.2] = col[0]                     # a large tie group
        P[:, j] = col
    w = rng.integers(1, 1025, size=n).astype(np.float64)
    w[rng.random(n) < 0.15] = 0.0
    if not w.any():
        w[0] = 7.0
    P[:, d] = rng.normal(size=n)
    P[:, d + 1] = rng.normal(size=n)
    P[:, d + 4] = w
    return P


def engine_with(P, d, **kw):
    from smc_jl_amd import Engine

    e = Engine(P.shape[0] if "n_parts" not in kw else kw.pop("n_parts"), d, seed=1, max_stages=8, store_history=False, **kw)
    e.upload_cloud(P)
    return e


def shard_engines(P, d, cuts):
    n, out, at = P.shape[0], [], 0
    for m in cuts:
        out.append(engine_with(np.asfortranarray(P[at:at + m]), d, n_parts=n, n_local=m, gid0=at))
        at += m
    assert at == n
    return out


def reference_exact(P, d, cols=None, probs=PROBS):
    cols = range(d) if cols is None else cols
    out = np.empty((len(cols), len(probs)))
    for r, j in enumerate(cols):
        ref = qr.Ref(P[:, j].tolist(), P[:, d + 4].tolist())
        out[r] = [ref.quantile_float(p) for p in probs]
    return out


@pytest.mark.parametrize("d", [1, 10])
@pytest.mark.parametrize("n", SIZES)
def test_exact_cases_bit_for_bit(n, d):
    P = exact_cloud(n, d, seed=100 * d + n)
    e = engine_with(P, d)
    got = e.weighted_quantiles(probs=PROBS)
    want = reference_exact(P, d)
    print("n=%d d=%d differing entries: %d" % (n, d, int((bits(got) != bits(want)).sum())))
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(bits(e.weighted_quantiles(probs=PROBS)), bits(got))            # two calls in a row: identical bits
    sub = [d - 1, 0] if d > 1 else [0]
    assert np.array_equal(bits(e.weighted_quantiles(columns=sub, probs=(0.95, 0.05))), bits(got[sub][:, [3, 1]]))
    assert np.array_equal(bits(e.weighted_quantiles()), bits(got[:, [1, 3]]))             # the reference's 5 % / 95 %
    assert np.array_equal(bits(e.download_cloud()), bits(P))                             # the cloud is only read
    e.close()


def test_zero_weights_and_all_weight_on_one_particle():
    P = exact_cloud(1000, 3, seed=5)
    P[:, 7] = 0.0
    P[417, 7] = 1024.0
    e = engine_with(P, 3)
    got = e.weighted_quantiles(probs=PROBS)
    assert np.array_equal(bits(got), bits(np.repeat(P[417, :3, None], 5, axis=1)))
    assert np.array_equal(bits(got), bits(reference_exact(P, 3)))
    e.close()


@pytest.mark.parametrize("cuts", [(1000, 3097), (63, 64, 3970)])
def test_group_over_uneven_handles_gives_the_same_bits(cuts):
    from smc_jl_amd import weighted_quantiles_group

    P = exact_cloud(4097, 10, seed=77)
    want = reference_exact(P, 10)
    es = shard_engines(P, 10, cuts)
    got = weighted_quantiles_group(es, probs=PROBS)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(weighted_quantiles_group(es, columns=[9, 2], probs=PROBS)), bits(want[[9, 2]]))
    with pytest.raises(RuntimeError) as ei:                        # a lone shard is not a cloud
        es[0].weighted_quantiles()
    assert ei.value.code == -7
    with pytest.raises(RuntimeError) as ei:
        es[1].best_particle()
    assert ei.value.code == -7
    with pytest.raises(RuntimeError) as ei:                        # ... nor are handles out of rank order
        weighted_quantiles_group(es[::-1])
    assert ei.value.code == -1
    for e in es:
        e.close()


def in_bracket(ref, p, got, wsum):
    lo, hi = ref.bracket(p, wsum / 2 ** 40)
    return F(qr.nextafter_n(float(lo), -2)) <= F(float(got)) <= F(qr.nextafter_n(float(hi), 2)), (float(lo), float(hi))


def check_general(P, d, got, label):
    from smc_jl_amd.host import api

    w = P[:, d + 4].tolist()
    wsum = sum(F(x) for x in w)
    mirror = api.weighted_quantiles(P, PROBS)
    for j in range(d):
        ref = qr.Ref(P[:, j].tolist(), w)
        for q, p in enumerate(PROBS):
            ok_m, br = in_bracket(ref, p, mirror[j, q], wsum)
            assert ok_m, ("numpy mirror outside the bracket", label, j, p, mirror[j, q], br)
            ok, br = in_bracket(ref, p, got[j, q], wsum)
            print("%s column %d p=%g device %r bracket %r" % (label, j, p, got[j, q], br))
            assert ok, (label, j, p, got[j, q], br)


def test_general_weights_after_a_short_adaptive_run():
    """the cloud of a config-2-style run (10-dim Gaussian, adaptive schedule) paused after a few stages, N = 4097"""
    from smc_jl_amd import Engine

    e = Engine(4097, 10, seed=3, max_stages=400, store_history=False)
    e.set_model(models.gauss_spec())
    e.init_from_prior()
    r = e.run(use_fixed_schedule=False, tempering_target=0.97, stop_after_stage=6)
    assert r["paused"]
    got = e.weighted_quantiles(probs=PROBS)
    P = e.download_cloud()
    assert np.unique(P[:, 14]).size > 100                        # general weights indeed
    check_general(P, 10, got, "run")
    e.close()


def test_general_weights_spanning_300_decades():
    rng = np.random.default_rng(8)
    n, d = 4097, 2
    P = np.zeros((n, d + 5), order="F")
    P[:, 0] = rng.normal(size=n)
    P[:, 1] = np.round(rng.normal(size=n), 1) + 0.05             # ties
    P[:, d + 4] = 10.0 ** rng.uniform(-300, 0, size=n)
    e = engine_with(P, d)
    got = e.weighted_quantiles(probs=PROBS)
    check_general(P, d, got, "decades")
    es = shard_engines(P, d, (2000, 97, 2000))
    from smc_jl_amd import weighted_quantiles_group

    check_general(P, d, weighted_quantiles_group(es, probs=PROBS), "decades, 3 handles")
    for x in es + [e]:
        x.close()


def test_error_paths():
    P = exact_cloud(1000, 3, seed=9)
    e = engine_with(P, 3)

    def code(fn):
        with pytest.raises(RuntimeError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: e.weighted_quantiles(probs=(0.5, 1.5))) == -1
    assert code(lambda: e.weighted_quantiles(probs=(-0.1,))) == -1
    assert code(lambda: e.weighted_quantiles(probs=(math.nan,))) == -1
    assert code(lambda: e.weighted_quantiles(probs=np.linspace(0, 1, 17))) == -1
    assert code(lambda: e.weighted_quantiles(columns=[3])) == -1
    assert code(lambda: e.weighted_quantiles(columns=[-1])) == -1
    assert e.weighted_quantiles(probs=np.linspace(0, 1, 16)).shape == (3, 16)
    for bad in (math.nan, -1.0, math.inf):
        Q = P.copy()
        Q[500, 7] = bad
        e.upload_cloud(Q)
        assert code(lambda: e.weighted_quantiles()) == -1, bad
    Q = P.copy()
    Q[:, 7] = 0.0
    e.upload_cloud(Q)
    assert code(lambda: e.weighted_quantiles()) == -1              # wsum == 0
    Q = P.copy()
    Q[123, 1] = math.nan                                           # a NaN in a column, even under a zero weight: that column is NaN
    Q[123, 7] = 0.0
    e.upload_cloud(Q)
    got = e.weighted_quantiles(probs=PROBS)
    assert np.isnan(got[1]).all()
    want = reference_exact(Q, 3, cols=[0, 2])
    assert np.array_equal(bits(got[[0, 2]]), bits(want))
    e.close()


def numpy_best(P, d, logpost):
    c = P[:, d] + P[:, d + 1] if logpost else P[:, d]
    i = qr.best(c.tolist())
    return i, c[i], P[i, :d]


@pytest.mark.parametrize("n", [1, 65, 6221])
def test_best_particle_on_one_handle_and_on_three(n):
    from smc_jl_amd import best_particle_group

    d = 10
    P = exact_cloud(n, d, seed=31 + n)
    variants = [("plain", P)]
    if n > 1:
        T = P.copy()                                               # a planted tie at the top: the lower id wins
        hi, lo = n - 2, n // 3
        T[[lo, hi], d] = 50.0
        T[[lo, hi], d + 1] = 0.25
        variants.append(("tie", T))
        N = T.copy()                                               # planted NaNs rank above everything, the first one wins
        N[[n // 2, n - 1], d] = math.nan
        variants.append(("nan", N))
    for label, C in variants:
        e = engine_with(C, d)
        es = shard_engines(C, d, (n // 3, n // 3, n - 2 * (n // 3))) if n >= 3 else []
        for crit in ("loglh", "logpost"):
            i, val, para = numpy_best(C, d, crit == "logpost")
            got = [e.best_particle(crit)] + ([best_particle_group(es, crit)] if es else [])
            for gi, gv, gp in got:
                assert gi == i, (label, crit, gi, i)
                assert np.array_equal(bits([gv]), bits([val])) or (math.isnan(gv) and math.isnan(val)), (label, crit, gv, val)
                assert np.array_equal(bits(gp), bits(para)), (label, crit)
        if label == "tie":
            assert e.best_particle("loglh")[0] == n // 3
        if label == "nan":
            assert e.best_particle("logpost")[0] == n // 2
        for x in es + [e]:
            x.close()


def test_summaries_between_a_pause_and_its_continuation_change_nothing():
    """stop_after_stage, summaries, continue_run: the same cloud bits, records and log-MDD as without the summary calls"""
    from smc_jl_amd import Engine

    kw = dict(use_fixed_schedule=False, tempering_target=0.97)
    ends = []
    for summarise in (False, True):
        e = Engine(4097, 10, seed=12, max_stages=600, store_history=True)
        e.set_model(models.gauss_spec())
        e.init_from_prior()
        r = e.run(stop_after_stage=7, **kw)
        assert r["paused"]
        if summarise:
            q = e.weighted_quantiles(probs=PROBS)
            assert np.isfinite(q).all() and (np.diff(q, axis=1) >= 0).all()
            e.best_particle("loglh")
            e.best_particle("logpost")
        r = e.run(continue_run=True, **kw)
        assert not r["paused"]
        rec = e.stage_records(r["n_stages"])
        ends.append((r["n_stages"], r["resamples"], float(r["logmdd"]).hex(), float(r["c"]).hex(), bits(e.download_cloud()),
                     {k: np.asarray(v).tobytes() for k, v in rec.items()}, [bits(h) for h in e.history(r["n_stages"])]))
        e.close()
    a, b = ends
    assert a[:4] == b[:4], (a[:4], b[:4])
    assert np.array_equal(a[4], b[4])
    assert a[5] == b[5]
    assert all(np.array_equal(x, y) for x, y in zip(a[6], b[6]))
