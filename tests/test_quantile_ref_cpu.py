"""The weighted quantiles and best particles off the device (DESIGN.md "Posterior summaries"): the exact reference pinned on hand-worked
cases, the numpy mirror of smc_jl_amd.host.api against it, and the host side of the device's selection (csrc/quantsel.hpp) driven by a
stand-alone program with plain loops in place of the kernels, under AddressSanitizer and UBSan."""
import math
import os
import random
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests import quantile_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference, by hand
def test_three_particles_with_weights_1_2_1():
    v, w = [10.0, 20.0, 30.0], [1.0, 2.0, 1.0]
    # wsum = 4, w1 = 1, h = 3 p + 1; S = 1, 3, 4
    assert qr.quantile(v, w, 0.5) == F(10) + F(3, 2) / 2 * 10            # h = 2.5: k = 2, 10 + (2.5 - 1) / 2 * 10 = 17.5
    assert qr.quantile(v, w, 0.5) == F(35, 2)
    assert qr.quantile(v, w, 0.0) == 10                                 # h = 1: S_1 = 1 is not > h, k = 2, 10 + 0
    assert qr.quantile(v, w, F(2, 3)) == 20                             # h = 3: S_2 = 3 is not > h, k = 3, 20 + 0 / 1 * 10
    assert qr.quantile(v, w, 0.9) == F(20) + (F(0.9) * 3 + 1 - 3) * 10  # h = 3.7: k = 3
    assert qr.quantile(v, w, 1.0) == 30                                 # h = 4 = wsum: no k
    assert qr.quantile_float(v, w, 0.5) == 17.5


def test_a_tie_group_that_straddles_h():
    # sorted pairs (1, 1) (2, 1) (2, 3) (2, 5) (3, 1): S = 1, 2, 5, 10, 11; wsum = 11, w1 = 1, h = 10 p + 1
    v, w = [2.0, 1.0, 2.0, 3.0, 2.0], [5.0, 1.0, 1.0, 1.0, 3.0]
    assert qr.quantile(v, w, F(1, 20)) == 1 + F(1, 2)    # h = 1.5: k = 2 is the tie group's lightest pair: 1 + (1.5 - 1) / 1 * (2 - 1)
    assert qr.quantile(v, w, F(3, 10)) == 2             # h = 4: k = 3, inside the group: v_{k-1} = v_k = 2
    assert qr.quantile(v, w, 0.5) == 2                 # h = 6: k = 4
    assert qr.quantile(v, w, F(19, 20)) == 2 + F(1, 2)    # h = 10.5: k = 5, 2 + (10.5 - 10) / 1 * 1
    # zero weights do not count, whatever their value
    assert qr.quantile(v + [-7.0, 99.0], w + [0.0, 0.0], F(1, 20)) == 1 + F(1, 2)


def test_p_0_p_1_and_one_particle():
    assert qr.quantile([5.0], [0.25], 0.0) == 5 and qr.quantile([5.0], [0.25], 0.3) == 5 and qr.quantile([5.0], [0.25], 1.0) == 5
    v, w = [3.0, -1.0, 2.0], [0.5, 0.25, 0.25]
    assert qr.quantile(v, w, 0.0) == -1                # h = w1 = 0.25 = S_1: k = 2 with h - S_1 = 0
    assert qr.quantile(v, w, 1.0) == 3
    assert math.isnan(qr.quantile([1.0, math.nan], [1.0, 0.0], 0.5))
    for bad in ([1.0, -1.0], [math.nan, 1.0], [0.0, 0.0]):
        with pytest.raises(ValueError):
            qr.quantile([1.0, 2.0], bad, 0.5)
    with pytest.raises(ValueError):
        qr.quantile([1.0, 2.0], [1.0, 1.0], 1.5)
    lo, hi = qr.bracket(v, w, 0.5, F(1, 1024))
    assert lo < qr.quantile(v, w, 0.5) < hi
    assert qr.best([1.0, 3.0, 3.0, 2.0]) == 1 and qr.best([1.0, math.nan, 9.0, math.nan]) == 1 and qr.best([-0.0, 0.0]) == 1


# ------------------------------------------------------------------------------------------------ the numpy mirror
def golden_cloud():
    """A host cloud made of the golden replay's columns: four incremental-weight columns as parameters (they carry ties), the last
    stage's normalised weights as weights."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "replay_as1000.npz"))
    w, W = z["w"], z["W"]
    n = w.shape[0]
    P = np.empty((n, 4 + 5), order="F")
    P[:, :4] = w[:, [10, 40, 70, 99]]
    P[:, 3] = np.round(P[:, 3], 2)                       # ... and one column with many ties
    with np.errstate(divide="ignore"):
        P[:, 4] = np.log(w[:, 99])
    P[:, 5] = -w[:, 50]
    P[:, 6] = 0.0
    P[:, 7] = z["accept_col"]
    P[:, 8] = W[:, -1]
    return P


def local_gap(v, w, q):
    """the distance between the distinct weighted values around q (the scale an error of the selection would have)"""
    vals = np.unique(np.asarray(v)[np.asarray(w) != 0])
    k = int(np.searchsorted(vals, q))
    lo, hi = vals[max(k - 1, 0)], vals[min(k, vals.size - 1)]
    return max(hi - lo, abs(q) * 2.0 ** -52, 5e-324)


def test_api_quantiles_and_best_particles_on_the_golden_cloud():
    import smc_jl_amd as S

    P = golden_cloud()
    c = S.Cloud(4, P.shape[0])
    c.particles[:] = P
    w = P[:, 8]
    probs = (0.0, 0.05, 0.5, 0.95, 1.0)
    Q = S.weighted_quantiles(c, probs)
    assert Q.shape == (4, 5)
    for j in range(4):
        for q, p in enumerate(probs):
            want = qr.quantile(P[:, j], w, p)
            assert abs(F(Q[j, q]) - want) <= F(1e-12) * F(local_gap(P[:, j], w, float(want))), (j, p, Q[j, q], float(want))
        lb, ub = S.weighted_quantile(c, j + 1)                      # 1-based like the reference
        assert (lb, ub) == (Q[j, 1], Q[j, 3])
        assert S.weighted_quantile(P, j + 1) == (lb, ub)            # a matrix is a cloud's particles
    with pytest.raises(AssertionError):
        S.weighted_quantile(c, 5)
    loglh, logpost = P[:, 4], P[:, 4] + P[:, 5]
    assert np.array_equal(S.get_likeliest_particle_value(c), P[np.argmax(loglh), :4])
    assert np.array_equal(S.get_likeliest_particle_value(c), P[qr.best(list(loglh)), :4])
    assert np.array_equal(S.get_highest_posterior_particle_value(c), P[np.argmax(logpost), :4])
    assert np.array_equal(S.get_highest_posterior_particle_value(c), P[qr.best(list(logpost)), :4])
    P2 = P.copy()
    P2[[700, 300], 4] = np.nan                                     # the first NaN wins (Julia's argmax)
    assert np.array_equal(S.get_likeliest_particle_value(P2), P2[300, :4])
    assert np.array_equal(S.get_highest_posterior_particle_value(P2), P2[300, :4])
    with pytest.raises(ValueError):
        S.weighted_quantiles(c, (0.5, 1.01))
    P2[5, 8] = -1.0
    with pytest.raises(ValueError):
        S.weighted_quantiles(P2, (0.5,))
    P2[:, 8] = 0.0
    with pytest.raises(ValueError):
        S.weighted_quantiles(P2, (0.5,))
    P2[:, 8] = 1.0
    P2[3, 1] = np.nan
    Q2 = S.weighted_quantiles(P2, (0.5,))
    assert np.isnan(Q2[1, 0]) and not np.isnan(Q2[0, 0])


# ------------------------------------------------------------------------------------------------ the selection's host side
ADJ = [1.0]
for _ in range(39):
    ADJ.append(math.nextafter(ADJ[-1], math.inf))          # a chain of 40 adjacent doubles


def selection_cases():
    """(values, weights, probs): integer weights (every sum exact in any order, so the program's doubles must reproduce
    quantile_float bit for bit) and general ones (compared through the bracket)"""
    rng = random.Random(11)
    P5 = (0.0, 0.05, 0.5, 0.95, 1.0)
    cases = [
        ([10.0, 20.0, 30.0], [1.0, 2.0, 1.0], P5),
        ([2.0, 1.0, 2.0, 3.0, 2.0], [5.0, 1.0, 1.0, 1.0, 3.0], P5),
        ([5.0], [3.0], P5),                                                          # one particle
        ([7.0, 7.0, 7.0], [1.0, 2.0, 3.0], P5),                                      # one value: lo == hi from the start
        (ADJ[:2], [1.0, 1.0], P5),                                                   # adjacent doubles: an interval of two keys
        (ADJ[:7], [3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0], P5),                          # hi - lo < C
        (ADJ, [float(1 + (i * 7) % 5) for i in range(40)], P5),
        ([-1e300, 1e300, -5e-324, 5e-324, 2.5e-310, -2.5e-310, 1.0, -1.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], P5),
        ([-1.7976931348623157e308, 1.7976931348623157e308, 0.0], [1.0, 1.0, 2.0], P5),    # the finite keys nearest 0 and 2^64 - 1
        ([1.0, 2.0, 3.0, 4.0], [0.0, 1024.0, 0.0, 0.0], P5),                         # all weight on one particle
        ([4.0, 1.0, 3.0, 2.0], [1.0, 1.0, 1.0, 1.0], tuple(i / 15 for i in range(16))),   # 16 levels: two thresholds each
    ]
    pool = [-1e300, -3.5, -1e-310, 5e-324, 1.0, ADJ[1], 2.5, 1e300]
    for _ in range(40):
        n = rng.choice([2, 3, 5, 17, 64, 65, 200])
        v = [rng.choice(pool + [rng.gauss(0, 1)]) for _ in range(n)]
        w = [float(rng.choice([0, 0, 1, 2, 3, rng.randint(1, 1024)])) for _ in range(n)]
        if not any(w):
            w[0] = 1.0
        cases.append((v, w, P5 + (rng.random(),)))
    general = []
    for _ in range(20):
        n = rng.choice([3, 17, 65, 200])
        v = [rng.choice(pool + [rng.gauss(0, 1), rng.gauss(0, 1)]) for _ in range(n)]
        w = [rng.choice([0.0, rng.random(), rng.random() * 1e-300, 0.5]) for _ in range(n)]
        if not any(w):
            w[0] = 0.25
        general.append((v, w, (0.05, 0.5, 0.95, rng.random())))
    return cases, general


CAND = [(0, 2 ** 64 - 1, 32), (0, 2 ** 64 - 1, 16), (0, 2 ** 64 - 1, 2), (0, 2 ** 64 - 1, 3), (0, 0, 16), (2 ** 64 - 1, 2 ** 64 - 1, 16),
        (0, 1, 2), (0, 5, 16), (2 ** 64 - 6, 2 ** 64 - 1, 32), (2 ** 64 - 33, 2 ** 64 - 1, 32), (2 ** 64 - 32, 2 ** 64 - 1, 32), (0, 31, 32), (0, 32, 32),
        (7, 2 ** 63 + 11, 10), (2 ** 63 - 1, 2 ** 63, 16), (1, 2 ** 64 - 2, 7), (123456789, 123456789 + 1000, 32)]


def test_selection_host_side_under_sanitizers(tmp_path):
    """tests/quantsel_check.cpp: csrc/quantsel.hpp with plain loops for the two functions the kernels provide.  Candidate generation at the
    ends of the key range and on intervals narrower than C; the selection on exact cases (bit for bit) and general ones (bracket)."""
    exe = tmp_path / "quantsel_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "quantsel_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exact, general = selection_cases()
    lines = ["cand %d %d %d" % c for c in CAND]
    for v, w, probs in exact + general:
        lines.append("case %d %d %s %s" % (len(v), len(probs), " ".join(float(p).hex() for p in probs),
                                           " ".join("%s %s" % (float(a).hex(), float(b).hex()) for a, b in zip(v, w))))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    for (lo, hi, C), ln in zip(CAND, out):
        t = [int(x) for x in ln.split()[1:]]
        n_keys = hi - lo + 1
        assert len(t) == min(C, n_keys), (lo, hi, C, t)
        assert t[-1] == hi and t[0] >= lo and all(a < b for a, b in zip(t, t[1:])), (lo, hi, C, t)
        runs = [b - a for a, b in zip([lo - 1] + t, t)]
        assert max(runs) - min(runs) <= 1 and max(runs) == -(-n_keys // len(t)), (lo, hi, C, runs)
    most = 0
    for (v, w, probs), ln in zip(exact, out[len(CAND):]):
        got = [float.fromhex(x) for x in ln.split()[1:-1]]
        most = max(most, int(ln.split()[-1]))
        for p, g in zip(probs, got):
            want = qr.quantile_float(v, w, p)
            assert g == want and math.copysign(1, g) == math.copysign(1, want), (v, w, p, g, want)
    for (v, w, probs), ln in zip(general, out[len(CAND) + len(exact):]):
        got = [float.fromhex(x) for x in ln.split()[1:-1]]
        most = max(most, int(ln.split()[-1]))
        wsum = sum(F(b) for b in w)
        for p, g in zip(probs, got):
            lo, hi = qr.bracket(v, w, p, wsum / 2 ** 40)
            assert F(qr.nextafter_n(float(lo), -2)) <= F(g) <= F(qr.nextafter_n(float(hi), 2)), (v, w, p, g, float(lo), float(hi))
    assert 1 <= most <= 64                      # 64 key bits at one bit per pass at the worst (16 levels); 13 at one level, 16 at two


def test_numpy_mirror_stays_inside_the_bracket_on_the_general_cases():
    from smc_jl_amd.host.api import _weighted_quantiles_1d

    _, general = selection_cases()
    for v, w, probs in general:
        got = _weighted_quantiles_1d(v, w, probs)
        wsum = sum(F(b) for b in w)
        for p, g in zip(probs, got):
            lo, hi = qr.bracket(v, w, p, wsum / 2 ** 40)
            assert F(qr.nextafter_n(float(lo), -2)) <= F(float(g)) <= F(qr.nextafter_n(float(hi), 2)), (v, w, p, g, float(lo), float(hi))
