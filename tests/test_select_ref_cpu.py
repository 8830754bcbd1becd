"""tests/select_ref.py pinned on the CPU, the restatement held to the selection rule, and the input conditions of every cloud
tests/test_gpu_select_range.py uses.

  * the exact reference against a brute-force fractions.Fraction search on clouds of at most 64 particles, thresholds exactly on
    boundaries, 0 and 1.0 included;
  * the reference against the restatement (oracle/smc_oracle.c orc_resample_with_offsets) on every cloud of the GPU file: equal
    ancestors wherever the slot is decided;
  * the two fall-through cases the restatement's clamp got wrong (a zero-weight last row selected) held to the rule;
  * the input conditions: at most 2 undecided slots per case, and on the clouds that go through a stage at least 50 n_para distinct
    ancestors (n_para 10; the wide row's 12), so that the resampled cloud's factor exists.

MARGIN = max(16 x the restatement's largest cum error on the cloud, 2^-43); 0 on exact clouds (tests/select_ref.py margin).

The restatement's largest cum error, measured (printed by test_reference_against_the_restatement; 20 480 particles, exact 16 384):
random 6.9e-15, collapse_ends 8.9e-13, collapse_apart 1.0e-14, dust 8.6e-16, zero_ends 4.7e-15, chunk_ends 6.5e-15, exact 0;
at 150 004 particles: collapse_ends 6.6e-12 (MARGIN 1.1e-10), zero_ends 1.5e-14; at the small sizes at most 1.5e-13 (collapse_ends,
4 099).  Undecided slots under the stages' Philox offsets: 0 on every cloud; distinct ancestors: collapse 640, chunk_ends 680 (527 at
4 096 particles), dust 1 024, the others thousands; widest 512-slot tile: collapse_ends 19 856 rows, collapse_apart 3 016.  Offsets
placed on purpose - the ends of [0, 1), multiples of 2^-11 on the exact family, the ulp sweep - sit on or next to boundaries and are
not counted towards the cap of undecided slots (tests/select_ref.py multinomial_offsets).
"""
import numpy as np
import pytest

from tests import select_ref as sr

N_PARA_MAX = 12


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


_CACHE = {}


def cloud(family, n):
    """(weights, exact Cloud, restatement's cum error, MARGIN), once per module"""
    key = (family, n)
    if key not in _CACHE:
        w = sr.make_cloud(family, n)
        c = sr.Cloud(w)
        err = c.cum_error(sr.restatement_cum(w))
        _CACHE[key] = (w, c, err, 0.0 if family == "exact" else max(16.0 * err, sr.MARGIN_FLOOR))
    return _CACHE[key]


def test_exact_int_is_exact():
    from fractions import Fraction

    for x in (0.0, 5e-324, 2.0 ** -1022, 1e-320, 1e-12, 0.1, 1.0, 1.5, 2.0 ** -30, 1e300):
        assert Fraction(sr.exact_int(x), 2 ** sr.SCALE) == Fraction(x), x


@pytest.mark.parametrize("family", sr.FAMILIES + sr.DEGENERATE[:3])
@pytest.mark.parametrize("n", [5, 33, 64])
def test_reference_against_brute_force(family, n):
    if family == "exact":
        n = sr.exact_size(n)
    w = sr.make_cloud(family, n, seed=1)
    c = sr.Cloud(w)
    rng = np.random.default_rng(n)
    # thresholds: 0, 1.0, the ends of [0, 1), every boundary C_j / S correctly rounded (exact on the exact family) and its two neighbours
    b = c.cum_float()
    t = np.concatenate([[0.0, 1.0], sr.fixed_offsets(), b, np.nextafter(b, 0.0), np.minimum(np.nextafter(b, 2.0), 1.0), rng.random(40)])
    got = c.select("multinomial", t.size, t)
    np.testing.assert_array_equal(got["anc"], sr.brute_force(w, t))
    assert np.all(w[got["anc"]] > 0)
    for u in sr.systematic_offsets(family) + [0.0, float(rng.random())]:
        for n_out in (n, 2 * n + 1):
            got = c.select("systematic", n_out, [u])
            np.testing.assert_array_equal(got["anc"], sr.brute_force(w, sr.thresholds("systematic", n_out, [u])))
    if family == "exact":                       # thresholds ON boundaries: the boundary's own row is not taken (> against >=)
        on = c.select("multinomial", n, b)
        live = np.flatnonzero(w > 0)
        assert np.all(on["anc"][live[:-1]] == live[1:]) and np.all(on["dist"][live[:-1]] == 0.0)


def test_single_particle():
    c = sr.Cloud(sr.make_cloud("single", 1))
    for u in (0.0, 0.5, 1.0 - 2.0 ** -53):
        assert c.select("systematic", 1, [u])["anc"].tolist() == [0]
        assert c.select("systematic", 3, [u])["anc"].tolist() == [0, 0, 0]


def _fall_through_cases():
    w1 = np.ones(400)
    w1[-3:] = 0.0
    rng = np.random.default_rng(4098)                   # (a seed whose sequential cum ends at 1 - 2.3e-15)
    w2 = rng.random(4097) * 2.0
    w2[-5:] = 0.0
    u2 = rng.random(4097)
    u2[7] = 1.0 - 2.0 ** -53
    return [("systematic", w1, [1.0 - 2.0 ** -53]), ("systematic", w1, [1.0 - 2.0 ** -45]), ("multinomial", w2, u2)]


@pytest.mark.parametrize("case", range(3))
def test_fall_through_takes_the_last_positive_row(orc, case):
    """(399 + u) / 400 rounds to 1.0; the sequential cum of 4 097 random weights ends below 1 - 2^-53: the restatement's clamp took the
    last row, weight 0.  The rule: the nearest row before it with positive weight."""
    method, w, off = _fall_through_cases()[case]
    ref = sr.Cloud(w).select(method, w.size, off)
    got = orc.resample(w, method, offsets=off)          # (the same weights as the reference's: the restatement normalises them itself)
    print(method, "last slots: restatement", got[-3:], "reference", ref["anc"][-3:])
    assert np.all(w[ref["anc"]] > 0)
    assert np.all(w[got] > 0), "the restatement selected rows of weight 0: %r" % np.flatnonzero(w[got] <= 0)
    und = ref["dist"] <= sr.MARGIN_FLOOR
    np.testing.assert_array_equal(got[~und], ref["anc"][~und])


def _offsets_of(orc, c, family, method, n_out):
    """every offset set the GPU file gives a stand-alone call of this cloud: (label, offsets, exempt mask or None)"""
    out = []
    if method == "systematic":
        out += [("u=%r" % u, [u], None) for u in sr.systematic_offsets(family)]
    else:
        out += [("given %d" % i, o, m) for i, (o, m) in enumerate(sr.multinomial_offsets(c, family, n_out))]
    out.append(("philox", orc.resample_offsets(method, n_out, seed=sr.SEED, stage=sr.STAGE), None))
    return out


@pytest.mark.parametrize("family,n", sr.small_cases() + sr.stage_cases() + [(f, sr.TWO_CHUNK_N) for f in sr.TWO_CHUNK_FAMILIES])
def test_reference_against_the_restatement(orc, family, n):
    """Equal ancestors wherever the slot is decided, at most 2 undecided slots per case (the ulp sweep's own slots apart), and on the
    stage sizes at least 50 n_para distinct ancestors."""
    w, c, err, mg = cloud(family, n)
    print("%s n=%d: restatement's cum error %.3g, MARGIN %.3g" % (family, n, err, mg))
    stage = n >= sr.EXACT_STAGE_N
    for method in ("systematic", "multinomial"):
        sets = _offsets_of(orc, c, family, method, n)
        if stage:                                   # a stage takes its offset from Philox alone
            sets = sets[-1:]
        for label, off, exempt in sets:
            ref = c.select(method, n, off)
            got = orc.resample(w, method, offsets=off)
            why, fig = sr.judge(ref, got, w, mg, method, exempt=exempt, cloud=c)
            distinct = np.unique(ref["anc"]).size
            print("  %s %s: %r distinct %d" % (method, label, fig, distinct))
            assert not why, (family, n, method, label, why)
            if family == "exact":
                assert fig["undecided"] == 0
            if stage:
                assert distinct >= 50 * N_PARA_MAX, distinct
    if stage and family.startswith("collapse"):     # the widest 512-slot tile spans more rows than the staging caps (2 048 / 4 096)
        span = sr.widest_tile_span(c.select("systematic", n, orc.resample_offsets("systematic", n, sr.SEED, sr.STAGE))["anc"])
        print("  widest tile span", span)
        assert span > (4096 if family == "collapse_ends" else 2048)
        if family == "collapse_apart":
            assert span <= 4096


@pytest.mark.parametrize("n_out", [100, 257, 700])
@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_bridge_sizes(orc, method, n_out):
    """n_out != n_src.  Multinomial and systematic with n_out >= n_src: the exact reference; systematic with n_out < n_src keeps quirk
    Q5 (search range 1:n_out) as the restatement states it and is compared with the restatement only - here: it stays in range."""
    w, c, err, mg = cloud("random", 257)
    off = orc.resample_offsets(method, n_out, seed=sr.SEED, stage=0)
    got = orc.resample(w, method, n_parts=n_out, offsets=off)
    if method == "systematic" and n_out < w.size:
        assert got.max() < n_out and np.all(np.diff(got) >= 0)
        return
    why, fig = sr.judge(c.select(method, n_out, off), got, w, mg, method, cloud=c)
    assert not why, why


@pytest.mark.parametrize("n", list(sr.ensemble_cases()) + [sr.MP_N])
def test_input_conditions_of_the_ensemble_and_two_process_clouds(orc, n):
    """the clouds of the ensemble launches (member m: seed SEED + m, stage 2) and of the two-process runs: at most 2 undecided slots, at
    least 50 n_para distinct ancestors, the restatement's ancestors wherever the slot is decided"""
    n_para, families = sr.ensemble_cases().get(n, (10, sr.MP_FAMILIES))
    for m, family in enumerate(families):
        w, c, err, mg = cloud(family, n)
        for method in ("systematic", "multinomial"):
            off = orc.resample_offsets(method, n, seed=sr.SEED + (m if n != sr.MP_N else 0), stage=2)
            ref = c.select(method, n, off)
            why, fig = sr.judge(ref, orc.resample(w, method, offsets=off), w, mg, method, cloud=c)
            distinct = np.unique(ref["anc"]).size
            print("%s n=%d %s: cum error %.3g %r distinct %d" % (family, n, method, err, fig, distinct))
            assert not why, (family, n, method, why)
            assert distinct >= 50 * n_para, (family, n, method, distinct)
