/* bm_div_rb (csrc/bmmath.hpp: y / b from the divisor's reciprocal) against the host's IEEE division, bit for bit.
 * usage: divrb_check <random pairs>; prints one line per group "name tried mismatches" and a last line "total tried mismatches".
 * Compile with -ffp-contract=off (the helper's FMAs are explicit; nothing else may be fused). */
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../smc.jl_amd/csrc/bmmath.hpp"

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {                       /* splitmix64 */
    uint64_t z = (rng_s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double from_bits(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }
/* a double with a random sign and mantissa and the binary exponent e (normal range) */
static double rnd_double(int e) { return from_bits((rnd() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(e + 1023) << 52)); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }
static double step_ulps(double x, int k) {        /* k ulps away (k of either sign) */
    for (; k > 0; --k) x = nextafter(x, INFINITY);
    for (; k < 0; ++k) x = nextafter(x, -INFINITY);
    return x;
}

static long long tried, wrong, g_tried, g_wrong;
static void check(double y, double b) {
    const double rb = 1.0 / b;
    const double got = bm_div_rb(y, b, rb, bm_div_rb_admits(b)), want = y / b;
    ++tried;
    if (bits(got) != bits(want)) {                /* (NaN included: the helper takes `/` itself there) */
        if (++wrong <= 10) printf("  MISMATCH y=%a b=%a rb=%a got=%a want=%a\n", y, b, rb, got, want);
    }
}
static void group(const char *name) {
    printf("%s %lld %lld\n", name, tried, wrong);
    g_tried += tried; g_wrong += wrong; tried = wrong = 0;
}

int main(int argc, char **argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 10000000;
    /* 1. random pairs over the admitted exponent ranges */
    for (long long i = 0; i < n; ++i) check(rnd_double(rnd_int(-460, 499)), rnd_double(rnd_int(-500, 499)));
    group("random");
    /* ... and with exponents close together (quotients around one, where a Normal prior's z lives) */
    for (long long i = 0; i < n / 4; ++i) { const int e = rnd_int(-40, 40); check(rnd_double(e + rnd_int(-3, 3)), rnd_double(e)); }
    group("random_near");
    /* 2. hard cases: y = RN(b q) for a random q, and the doubles 1..3 ulp either side of it - quotients next to a double or next to the
     * midpoint of two */
    for (long long i = 0; i < n / 16; ++i) {
        const double b = rnd_double(rnd_int(-200, 200)), q = rnd_double(rnd_int(-200, 200)), y = b * q;
        for (int k = -3; k <= 3; ++k) check(step_ulps(y, k), b);
    }
    group("constructed");
    /* midpoints: q = (an odd multiple of half an ulp) needs 54 bits, so b q is hit exactly only with short mantissas: b of 26 bits, q of 27 */
    for (long long i = 0; i < n / 16; ++i) {
        const double b = (double)((rnd() >> 38) | (1ull << 25)), qh = (double)((rnd() >> 37) | (1ull << 26) | 1ull);
        const double y = b * qh;                  /* exact: 53 bits */
        for (int k = -2; k <= 2; ++k) check(step_ulps(ldexp(y, rnd_int(-300, 300)), k), ldexp(b, rnd_int(-100, 100)));
    }
    group("short_mantissas");
    /* 3. quotients at a binade edge: q = 2^e (1 - k 2^-53) and 2^e (1 + k 2^-52) */
    for (long long i = 0; i < n / 32; ++i) {
        const double b = rnd_double(rnd_int(-200, 200));
        const double one = ldexp(1.0, rnd_int(-200, 200));
        for (int k = -4; k <= 4; ++k) {
            const double q = step_ulps(one, k), y = b * q;
            for (int j = -2; j <= 2; ++j) check(step_ulps(y, j), b);
        }
    }
    group("binade_edge");
    /* 4. powers of two as divisor, dividend, both; mantissas of all ones */
    for (int eb = -500; eb <= 500; eb += 1) {
        const double b = ldexp(1.0, eb), ones = step_ulps(ldexp(1.0, eb < 500 ? eb + 1 : eb), -1);
        for (int j = 0; j < 64; ++j) {
            const int ey = rnd_int(-460, 499);
            check(rnd_double(ey), b); check(-ldexp(1.0, ey), b); check(ldexp(1.0, ey), -b);
            check(rnd_double(ey), ones); check(step_ulps(ldexp(1.0, ey + 1), -1), ones); check(ldexp(1.0, ey), ones);
        }
    }
    group("powers_of_two");
    /* 5. zeros, infinities, NaN as dividend */
    {
        const double sp[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, -NAN};
        for (int i = 0; i < 100000; ++i)
            for (int s = 0; s < 6; ++s) check(sp[s], rnd_double(rnd_int(-500, 499)));
        for (int s = 0; s < 6; ++s)
            for (int t = 0; t < 6; ++t) check(sp[s], sp[t]);                    /* (such divisors are not admitted) */
    }
    group("special_dividends");
    /* 6. subnormal quotients and subnormal operands (dividends below the admitted range: the helper must take `/`) */
    for (long long i = 0; i < n / 16; ++i) {
        const double b = rnd_double(rnd_int(0, 500));
        const double y = rnd_double(rnd_int(-1022, -1000) + (int)(rnd() % 24));
        check(y, b);
        check(from_bits(rnd() & 0x800FFFFFFFFFFFFFull), rnd_double(rnd_int(-500, 500)));      /* subnormal dividend */
        check(rnd_double(rnd_int(-1022, -600)), rnd_double(rnd_int(400, 500)));
    }
    group("subnormal_quotients");
    /* 7. both ends of the admitted ranges, and the doubles just outside them; divisors outside the range altogether */
    {
        const double be[] = {BM_DIV_B_MIN, BM_DIV_B_MAX}, ye[] = {BM_DIV_Y_MIN, BM_DIV_Y_MAX};
        double bs[2 * 2 * 7], ys[2 * 2 * 7];
        int nb = 0, ny = 0;
        for (int e = 0; e < 2; ++e)
            for (int k = -3; k <= 3; ++k)
                for (int sg = 0; sg < 2; ++sg) {
                    bs[nb++] = (sg ? -1.0 : 1.0) * step_ulps(be[e], k);
                    ys[ny++] = (sg ? -1.0 : 1.0) * step_ulps(ye[e], k);
                }
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j < ny; ++j) check(ys[j], bs[i]);
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j < 20000; ++j) { check(rnd_double(rnd_int(-460, 499)), bs[i]); check(rnd_double(rnd_int(-1022, 1023)), bs[i]); }
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < 20000; ++i) { check(ys[j], rnd_double(rnd_int(-500, 499))); check(ys[j], rnd_double(rnd_int(-1022, 1023))); }
        /* the extreme quotients of the admitted box: 2^-960 and 2^1000, random mantissas */
        for (int i = 0; i < 200000; ++i) {
            check(rnd_double(-460), rnd_double(499)); check(rnd_double(499), rnd_double(-500));
            check(rnd_double(-460), rnd_double(-500)); check(rnd_double(499), rnd_double(499));
        }
        /* divisors that are not admitted: tiny (1e-200: a Normal prior's sd of that size), huge (1e200), subnormal, zero, infinite, NaN */
        const double out[] = {1e-200, 1e200, -1e-200, -1e200, 0x1p-1060, 0.0, -0.0, INFINITY, NAN, 0x1p-501, 0x1p+501, 0x1p+1023};
        for (unsigned i = 0; i < sizeof out / sizeof out[0]; ++i) {
            if (bm_div_rb_admits(out[i])) { printf("  divisor %a must not be admitted\n", out[i]); ++wrong; }
            for (int j = 0; j < 20000; ++j) check(rnd_double(rnd_int(-1022, 1023)), out[i]);
        }
        if (!bm_div_rb_admits(BM_DIV_B_MIN) || !bm_div_rb_admits(-BM_DIV_B_MAX) || bm_div_rb_admits(step_ulps(BM_DIV_B_MIN, -1)) ||
            bm_div_rb_admits(step_ulps(BM_DIV_B_MAX, 1)) || !bm_div_rb_admits_y(BM_DIV_Y_MIN) || !bm_div_rb_admits_y(-BM_DIV_Y_MAX) ||
            bm_div_rb_admits_y(step_ulps(BM_DIV_Y_MIN, -1)) || bm_div_rb_admits_y(step_ulps(BM_DIV_Y_MAX, 1)) || bm_div_rb_admits_y(0.0) ||
            bm_div_rb_admits_y(INFINITY) || bm_div_rb_admits_y(NAN)) { printf("  the admitted ranges are not as documented\n"); ++wrong; }
    }
    group("range_ends");
    printf("total %lld %lld\n", g_tried, g_wrong);
    return g_wrong != 0;
}
