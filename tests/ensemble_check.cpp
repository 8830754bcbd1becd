// ensemble_check.cpp - csrc/ensshape.hpp, the launch shape of an ensemble member (one workgroup = one whole run), as a pure function of
// (n_parts, n_para): for every n_para 1..10 at n_parts = 1, 63, 64, 65, T - 1, T, T + 1, 2 T + 77 and 8 192 (T the block) the shape is
// granted, the dynamic LDS (lds::ens) plus the bound on the kernel's static words stays within a CU's 160 KiB, both walks over the cloud -
// strided (ens_particle) and contiguous (ens_chunk) - cover every particle exactly once and none beyond it, and every member of the layout
// is aligned, inside the total and disjoint from the others; at 8 193 particles, at n_para 0 and 11 and at n_parts 0 the shape is refused.
// No HIP.  Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <vector>

#include "../smc.jl_amd/csrc/ensshape.hpp"

using namespace smcmi;

static int failures = 0;
static long long g_n = 0;
static int g_d = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        if (!(cond)) { std::printf("line %d (n_parts %lld, n_para %d): %s\n", __LINE__, g_n, g_d, #cond); ++failures; } \
    } while (0)

static void check_shape(long long n, int d) {
    g_n = n; g_d = d;
    const EnsShape s = ens_shape(n, d);
    CHECK(s.ok == 1);
    if (!s.ok) return;
    CHECK(s.block == ENS_T && s.block % 64 == 0 && s.block <= 1024);
    CHECK((long long)s.per_thread * s.block >= n && (long long)(s.per_thread - 1) * s.block < n);
    // LDS: the dynamic part is the layout's, and with the static words it fits a CU
    const auto l = lds::ens(d, n);
    CHECK(s.lds_bytes == l.bytes);
    CHECK(s.lds_bytes + ENS_STATIC_LDS <= 160 * 1024);
    CHECK(l[lds::X_body] == 0);                                     // (MutBodyLds::place_body carves from sm[0])
    CHECK(l.m[lds::X_body].count >= lds::mut2(d, 4, LIK_LDS_CAP, false).bytes);
    CHECK(l.m[lds::X_en].count == (size_t)n && l.m[lds::X_wv].count == (size_t)n);
    CHECK(l.m[lds::X_Ls].count >= (size_t)d * d * d);
    CHECK(l.m[lds::X_red].count >= (size_t)(ENS_T / 64) * 64 && l.m[lds::X_tot].count >= 64);
    for (int a = 0; a < lds::X_N; ++a) {
        const lds::Member &m = l.m[a];
        CHECK(m.count > 0);
        CHECK(m.off % m.align == 0 && m.off % (m.elem < 8 ? m.elem : 8) == 0);
        CHECK(m.end() <= l.bytes);
        for (int b = a + 1; b < lds::X_N; ++b) CHECK(m.end() <= l.m[b].off || l.m[b].end() <= m.off);
    }
    // the strided walk: every particle exactly once, nothing beyond the cloud
    std::vector<int> seen((size_t)n, 0);
    for (int t = 0; t < s.block; ++t)
        for (int q = 0; q < s.per_thread; ++q) {
            const long long p = ens_particle(s, n, t, q);
            CHECK(p >= -1 && p < n);
            if (p >= 0 && p < n) seen[(size_t)p] += 1;
        }
    bool once = true;
    for (long long p = 0; p < n; ++p) once = once && seen[(size_t)p] == 1;
    CHECK(once);
    // the contiguous walk: consecutive stretches in thread order that tile [0, n)
    long long at = 0;
    for (int t = 0; t < s.block; ++t) {
        long long beg = -1, end = -1;
        ens_chunk(s, n, t, beg, end);
        CHECK(beg <= end && end - beg <= s.per_thread);
        CHECK(beg == at || (beg == n && end == n));
        if (end > at) at = end;
    }
    CHECK(at == n);
}

int main() {
    const long long T = ENS_T;
    const long long sizes[] = {1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 77, 8192};
    static_assert(SMCMI_ENS_MAX_PARTS == 8192, "the cap the header states");
    for (int d = 1; d <= 10; ++d)
        for (long long n : sizes) check_shape(n, d);
    g_n = 0; g_d = 0;
    for (int d = 1; d <= 10; ++d) {
        CHECK(ens_shape(8193, d).ok == 0);
        CHECK(ens_shape(0, d).ok == 0);
        CHECK(ens_shape(-5, d).ok == 0);
    }
    CHECK(ens_shape(1000, 0).ok == 0);
    CHECK(ens_shape(1000, 11).ok == 0);
    // the derivation of the cap: two particle-length FP64 arrays are 128 KiB at 8 192 particles
    CHECK(2 * sizeof(double) * (size_t)SMCMI_ENS_MAX_PARTS == 128 * 1024);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
