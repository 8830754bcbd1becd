// quantsel.hpp - the host side of the weighted-quantile selection (DESIGN.md "Posterior summaries").  No HIP in here: whoever drives it
// supplies two functions over the cloud - "the sums S(t) = Σ w·[key ≤ t] for these thresholds" and "the smallest non-zero weight at this key
// and the largest key below it" - and gets the quantiles.  csrc/summary.hip supplies them as kernel launches over one or several handles,
// tests/quantsel_check.cpp as plain loops.
//
// Definition (StatsBase's quantile(v, Weights(w), p), grouped by value): h = p (wsum - w1) + w1 with w1 the smallest weight at the
// smallest value; v* the smallest value with S_≤(v*) > h; the result v_prev + (h - S_<) / wmin · (v* - v_prev) when S_< + wmin > h and v*
// otherwise; the largest value when S_≤(max) ≤ h.  Only particles with w ≠ 0 count.
//
// Selection: K-section on the order-preserving 64-bit key of a double.  An open (column, level) holds a key interval [lo, hi] with
// S(lo - 1) ≤ h < S(hi); a pass cuts it into C runs of near-equal length, the last threshold being hi itself, and keeps the first run whose
// threshold's sum exceeds h.  S is monotone in t whatever its rounding (every S comes out of the same summation tree and round-to-nearest
// addition is monotone), so the choice is self-consistent.  A column's open levels share the SLOTS thresholds of a pass.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace quantsel {

constexpr int SLOTS = 32;            // thresholds per column and pass (the candidate kernel keeps one running sum per slot in registers)
constexpr int MAX_LEVELS = 16;       // = SMCMI_MAX_QUANT: SLOTS / MAX_LEVELS = 2 thresholds per level at the least, so every pass narrows

// order-preserving key: a < b as doubles (Julia's isless: -0.0 below +0.0) <=> key(a) < key(b) as unsigned integers
inline uint64_t key_of(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
inline double value_of(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ (1ull << 63)) : ~k;
    double x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

// Up to C ascending thresholds that cut the keys lo..hi into runs of near-equal length; the last one is hi.  An interval of fewer than C keys
// gives every key of it once.  The interval holds hi - lo + 1 keys - 2^64 of them for [0, 2^64 - 1], so that count is never formed: quotient
// and remainder are taken of hi - lo and stepped by one.  Unsigned arithmetic below may wrap; every threshold's true value lies in [lo, hi].
inline int candidates(uint64_t lo, uint64_t hi, int C, uint64_t *t) {
    const uint64_t width = hi - lo, c64 = (uint64_t)C;
    uint64_t q = width / c64, r = width % c64;
    if (r + 1 == c64) { q += 1; r = 0; } else r += 1;           // (q, r) = divmod(width + 1, C)
    if (q == 0) {
        for (uint64_t c = 0; c < r; ++c) t[c] = lo + c;
        return (int)r;
    }
    for (uint64_t c = 0; c < c64; ++c) t[c] = lo + ((c + 1) * q + (c + 1 < r ? c + 1 : r) - 1);
    return C;
}

struct Prepass {                     // what the first passes over a column leave (particles with w ≠ 0 only)
    uint64_t kmin = 0, kmax = 0;     // smallest and largest key
    double w1 = 0.0;                 // smallest weight at kmin
    double wsum = 0.0;               // Σ w, out of the same tree as every S(t)
    bool has_nan = false;            // a NaN anywhere in the column: every quantile of it is NaN
};

struct Level {
    double h = 0.0;
    uint64_t lo = 0, hi = 0;
    double s_lt = 0.0;               // S(lo - 1)
    bool open = false;               // lo < hi: still to be narrowed
    bool top = false;                // S(max) ≤ h: the largest value (p = 1, one particle)
    int off = 0, cnt = 0;            // its thresholds of the pass under way: slots [off, off + cnt)
};

struct Column {
    Prepass pre;
    int n_levels = 0;
    Level lv[MAX_LEVELS];

    void init(const Prepass &p, const double *probs, int L) {
        pre = p;
        n_levels = L;
        for (int l = 0; l < L; ++l) {
            Level &v = lv[l];
            v = Level();
            v.h = probs[l] * (p.wsum - p.w1) + p.w1;
            v.top = !(p.wsum > v.h);
            v.lo = p.kmin;
            v.hi = p.kmax;
            v.open = !p.has_nan && !v.top && v.lo < v.hi;
        }
    }
    int n_open() const {
        int k = 0;
        for (int l = 0; l < n_levels; ++l) k += lv[l].open;
        return k;
    }
    // the thresholds of the next pass into thr[0, SLOTS); unused slots repeat the largest key (their sums are not read)
    void plan(uint64_t *thr) {
        const int C = SLOTS / n_open();
        int off = 0;
        for (int l = 0; l < n_levels; ++l) {
            Level &v = lv[l];
            if (!v.open) continue;
            v.off = off;
            v.cnt = candidates(v.lo, v.hi, C, thr + off);
            off += v.cnt;
        }
        for (; off < SLOTS; ++off) thr[off] = pre.kmax;
    }
    // narrow every open level to the first run whose threshold's sum exceeds h
    void update(const uint64_t *thr, const double *S) {
        for (int l = 0; l < n_levels; ++l) {
            Level &v = lv[l];
            if (!v.open) continue;
            int c = 0;
            while (c < v.cnt - 1 && !(S[v.off + c] > v.h)) ++c;         // (the last threshold is hi, and S(hi) > h holds from the pass before)
            if (c > 0) {
                v.lo = thr[v.off + c - 1] + 1;
                v.s_lt = S[v.off + c - 1];
            }
            v.hi = thr[v.off + c];
            v.open = v.lo < v.hi;
        }
    }
    // wmin: the smallest non-zero weight at the level's key; prev1: the largest key below it + 1, 0 when there is none
    double result(int l, double wmin, uint64_t prev1) const {
        const Level &v = lv[l];
        if (pre.has_nan) return std::nan("");
        if (v.top) return value_of(pre.kmax);
        const double x = value_of(v.lo);
        if (prev1 != 0 && v.s_lt + wmin > v.h) {
            const double xp = value_of(prev1 - 1);
            return xp + (v.h - v.s_lt) / wmin * (x - xp);
        }
        return x;
    }
};

// All requested columns at once.  sums(cols, thr, S): for every listed column k (an index into the caller's column list) the SLOTS sums of
// thr[k' * SLOTS + j] into S[k' * SLOTS + j], k' the position in `cols`.  atkey(cols, keys, wmin, prev1): the same addressing with MAX_LEVELS
// keys per column.  Both return 0 or an error code, which ends the selection.  out[k * L + l]; *passes counts the calls of `sums`.
template <class Sums, class AtKey>
int select(int n_col, const Prepass *pre, const double *probs, int L, Sums &&sums, AtKey &&atkey, double *out, int *passes = nullptr) {
    std::vector<Column> col((size_t)n_col);
    for (int k = 0; k < n_col; ++k) col[(size_t)k].init(pre[k], probs, L);
    std::vector<int> cols;
    std::vector<uint64_t> thr;
    std::vector<double> S;
    int n_pass = 0;
    for (;;) {
        cols.clear();
        for (int k = 0; k < n_col; ++k)
            if (col[(size_t)k].n_open() > 0) cols.push_back(k);
        if (cols.empty()) break;
        thr.assign(cols.size() * SLOTS, 0);
        S.assign(cols.size() * SLOTS, 0.0);
        for (size_t j = 0; j < cols.size(); ++j) col[(size_t)cols[j]].plan(&thr[j * SLOTS]);
        if (int e = sums(cols, thr.data(), S.data())) return e;
        for (size_t j = 0; j < cols.size(); ++j) col[(size_t)cols[j]].update(&thr[j * SLOTS], &S[j * SLOTS]);
        ++n_pass;
    }
    if (passes) *passes = n_pass;
    // the finishing pass: columns with a level that may interpolate
    cols.clear();
    for (int k = 0; k < n_col; ++k) {
        const Column &c = col[(size_t)k];
        bool any = false;
        for (int l = 0; l < L; ++l) any = any || !c.lv[l].top;
        if (any && !c.pre.has_nan) cols.push_back(k);
    }
    std::vector<uint64_t> keys(cols.size() * MAX_LEVELS, 0), prev1(cols.size() * MAX_LEVELS, 0);
    std::vector<double> wmin(cols.size() * MAX_LEVELS, 0.0);
    for (size_t j = 0; j < cols.size(); ++j)
        for (int l = 0; l < L; ++l) keys[j * MAX_LEVELS + (size_t)l] = col[(size_t)cols[j]].lv[l].lo;
    if (!cols.empty())
        if (int e = atkey(cols, keys.data(), wmin.data(), prev1.data())) return e;
    std::vector<int> pos((size_t)n_col, -1);
    for (size_t j = 0; j < cols.size(); ++j) pos[(size_t)cols[j]] = (int)j;
    for (int k = 0; k < n_col; ++k)
        for (int l = 0; l < L; ++l) {
            const int j = pos[(size_t)k];
            out[(size_t)k * L + l] = j < 0 ? col[(size_t)k].result(l, 0.0, 0) : col[(size_t)k].result(l, wmin[(size_t)j * MAX_LEVELS + l], prev1[(size_t)j * MAX_LEVELS + l]);
        }
    return 0;
}

}      // namespace quantsel
