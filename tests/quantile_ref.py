"""Exact reference for the weighted quantiles (DESIGN.md "Posterior summaries"): StatsBase's quantile(v, Weights(w), p) for
non-frequency weights in its sequential form - sort the (value, weight) pairs, walk them - in fractions.Fraction.  It is neither the
numpy mirror of smc_jl_amd.host.api (float cumulative sums) nor the device's algorithm (selection on keys, grouped by value).

    quantile(v, w, p)            the exact value as a Fraction; h = p (wsum - w1) + w1 exact unless `h` is given
    quantile_float(v, w, p)      what a double-precision evaluation gives when every partial sum is exactly representable (integer
                                 weights): h formed in double, the pair k selected exactly, the interpolation in the formula's operation order
    bracket(v, w, p, delta)      (Q(h - delta), Q(h + delta)) with the exact h: Q is monotone in h
    Ref(v, w)                    the same four on one column whose sorted pairs and running sums are kept
    best(values)                 Julia's argmax: the first NaN if there is one, else the first largest value (isless order: -0.0 < +0.0)
"""
import bisect
import math
import struct
from fractions import Fraction as F


def _key(x):
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return u ^ (0xFFFFFFFFFFFFFFFF if u >> 63 else 1 << 63)


def _pairs(v, w):
    """the pairs with w != 0, sorted by (value, weight); values ordered by isless (-0.0 below +0.0)"""
    vw = [(float(a), float(b)) for a, b in zip(v, w) if b != 0]
    for a, b in vw:
        if math.isnan(b) or b < 0 or math.isinf(b):
            raise ValueError("weight vector cannot contain NaN / negative / infinite entries")
    if not vw or sum(F(b) for _, b in vw) == 0:
        raise ValueError("weight vector cannot sum to zero")
    return sorted(vw, key=lambda t: (_key(t[0]), t[1]))


class Ref:
    """one column: the sorted pairs and their exact running sums, shared by every probability asked of it"""

    def __init__(self, v, w):
        self.nan = any(math.isnan(x) for x in v)
        self.vw = _pairs(v, w)
        self.S = []
        s = F(0)
        for _, b in self.vw:
            s += F(b)
            self.S.append(s)
        self.wsum, self.w1 = s, F(self.vw[0][1])

    def _walk(self, h):
        """(k, S_{k-1}, S_k) with k the first 1-based index with S_k > h, or None; exact"""
        k = bisect.bisect_right(self.S, h)
        if k >= len(self.S):
            return None
        return k + 1, (self.S[k - 1] if k else F(0)), self.S[k]

    def exact_h(self, p):
        return F(p) * (self.wsum - self.w1) + self.w1

    def quantile(self, p, h=None):
        if not 0 <= p <= 1:
            raise ValueError("input probability out of [0,1] range")
        if self.nan:
            return math.nan
        h = self.exact_h(p) if h is None else F(h)
        hit = self._walk(h)
        if hit is None:
            return F(self.vw[-1][0])
        k, S_old, S = hit
        if k == 1:            # (h < w1: cannot happen for an h of the definition; Q continued to the left for bracket())
            return F(self.vw[0][0])
        v_old, v_k = F(self.vw[k - 2][0]), F(self.vw[k - 1][0])
        return v_old + (h - S_old) / (S - S_old) * (v_k - v_old)

    def quantile_float(self, p):
        if self.nan:
            return math.nan
        assert F(float(self.wsum)) == self.wsum, "quantile_float is for weights whose sums are exact in double"
        h = p * (float(self.wsum) - float(self.w1)) + float(self.w1)
        hit = self._walk(F(h))
        if hit is None:
            return self.vw[-1][0]
        k, S_old, S = hit
        assert k > 1
        return self.vw[k - 2][0] + (h - float(S_old)) / float(S - S_old) * (self.vw[k - 1][0] - self.vw[k - 2][0])

    def bracket(self, p, delta):
        h = self.exact_h(p)
        return self.quantile(p, h=h - F(delta)), self.quantile(p, h=h + F(delta))


def exact_h(v, w, p):
    return Ref(v, w).exact_h(p)


def quantile(v, w, p, h=None):
    if not 0 <= p <= 1:
        raise ValueError("input probability out of [0,1] range")
    return Ref(v, w).quantile(p, h)


def quantile_float(v, w, p):
    return Ref(v, w).quantile_float(p)


def bracket(v, w, p, delta):
    return Ref(v, w).bracket(p, delta)


def nextafter_n(x, n):
    """x moved by n units in the last place (n < 0: down)"""
    x = float(x)
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def best(values):
    win = 0
    for i, x in enumerate(values):
        if math.isnan(x):
            return i
        if _key(x) > _key(values[win]):
            win = i
    return win
