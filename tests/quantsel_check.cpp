// quantsel_check.cpp - drives csrc/quantsel.hpp (the host side of the weighted-quantile selection) with plain double-precision loops in
// place of the kernels.  Stand-alone: tests/test_quantile_ref_cpu.py builds it with -fsanitize=address,undefined, feeds it a text file of
// cases and compares what it prints with tests/quantile_ref.py.
//
// Input, whitespace-separated tokens:
//   cand <lo> <hi> <C>                                   -> "cand t_0 t_1 ..."             the thresholds of one interval (decimal)
//   case <n> <L> p_0 .. p_{L-1} v_0 w_0 .. v_{n-1} w_{n-1} -> "case q_0 .. q_{L-1} passes"   doubles as hexadecimal floats (%a)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../smc.jl_amd/csrc/quantsel.hpp"

static bool token(FILE *f, std::string &s) {
    char buf[128];
    if (fscanf(f, "%127s", buf) != 1) return false;
    s = buf;
    return true;
}
static double number(FILE *f) {
    std::string s;
    if (!token(f, s)) { fprintf(stderr, "unexpected end of input\n"); exit(2); }
    return strtod(s.c_str(), nullptr);
}
static uint64_t integer(FILE *f) {
    std::string s;
    if (!token(f, s)) { fprintf(stderr, "unexpected end of input\n"); exit(2); }
    return strtoull(s.c_str(), nullptr, 10);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::string kind;
    while (token(f, kind)) {
        if (kind == "cand") {
            const uint64_t lo = integer(f), hi = integer(f);
            const int C = (int)integer(f);
            std::vector<uint64_t> t((size_t)C);
            const int cnt = quantsel::candidates(lo, hi, C, t.data());
            printf("cand");
            for (int c = 0; c < cnt; ++c) printf(" %" PRIu64, t[(size_t)c]);
            printf("\n");
            continue;
        }
        if (kind != "case") { fprintf(stderr, "unknown record %s\n", kind.c_str()); return 2; }
        const int n = (int)integer(f), L = (int)integer(f);
        std::vector<double> probs((size_t)L), v((size_t)n), w((size_t)n), out((size_t)L);
        for (double &p : probs) p = number(f);
        for (int i = 0; i < n; ++i) { v[(size_t)i] = number(f); w[(size_t)i] = number(f); }
        std::vector<uint64_t> key((size_t)n);
        for (int i = 0; i < n; ++i) key[(size_t)i] = quantsel::key_of(v[(size_t)i]);
        // the two functions the selection asks for, over one column
        auto sums = [&](const std::vector<int> &cols, const uint64_t *thr, double *S) {
            for (size_t j = 0; j < cols.size() * quantsel::SLOTS; ++j) {
                double s = 0.0;
                for (int i = 0; i < n; ++i) s += key[(size_t)i] <= thr[j] ? w[(size_t)i] : 0.0;
                S[j] = s;
            }
            return 0;
        };
        auto atkey = [&](const std::vector<int> &cols, const uint64_t *keys, double *wmin, uint64_t *prev1) {
            for (size_t j = 0; j < cols.size() * quantsel::MAX_LEVELS; ++j) {
                bool any = false;
                wmin[j] = 0.0;
                prev1[j] = 0;
                for (int i = 0; i < n; ++i) {
                    if (w[(size_t)i] == 0.0) continue;
                    if (key[(size_t)i] == keys[j] && (!any || w[(size_t)i] < wmin[j])) { wmin[j] = w[(size_t)i]; any = true; }
                    if (key[(size_t)i] < keys[j] && key[(size_t)i] + 1 > prev1[j]) prev1[j] = key[(size_t)i] + 1;
                }
            }
            return 0;
        };
        // the prepass
        quantsel::Prepass pre;
        pre.kmin = ~0ull;
        for (int i = 0; i < n; ++i) {
            if (v[(size_t)i] != v[(size_t)i]) pre.has_nan = true;
            if (w[(size_t)i] == 0.0) continue;
            if (key[(size_t)i] < pre.kmin) pre.kmin = key[(size_t)i];
            if (key[(size_t)i] > pre.kmax) pre.kmax = key[(size_t)i];
        }
        {
            const std::vector<int> one(1, 0);
            std::vector<uint64_t> keys(quantsel::MAX_LEVELS, 0), prev1(quantsel::MAX_LEVELS), thr(quantsel::SLOTS, ~0ull);
            std::vector<double> wmin(quantsel::MAX_LEVELS), S(quantsel::SLOTS);
            keys[0] = pre.kmin;
            atkey(one, keys.data(), wmin.data(), prev1.data());
            pre.w1 = wmin[0];
            sums(one, thr.data(), S.data());
            pre.wsum = S[0];
        }
        int passes = 0;
        if (quantsel::select(1, &pre, probs.data(), L, sums, atkey, out.data(), &passes)) return 1;
        printf("case");
        for (double q : out) printf(" %a", q);
        printf(" %d\n", passes);
    }
    fclose(f);
    return 0;
}
