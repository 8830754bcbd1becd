// lds_check.cpp - csrc/ldslayout.hpp against the rule before the header took it over: every layout's total equals the size formula its
// launch site used to state by hand (copied below, verbatim), every member is aligned and inside the total, no two live members overlap,
// and the equivalences the kernels rely on hold.  Prints the segment kernels' largest dynamic request, one line per instantiation
// (tests/test_abi_cpu.py adds the compiler's static figure), then "ok".  No HIP.  Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cstdio>

#include "../smc.jl_amd/csrc/ldslayout.hpp"

using namespace smcmi;
using lds::Layout;
using lds::Member;

static int failures = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::printf("line %d (%s): %s\n", __LINE__, g_what, #cond); ++failures; }     \
    } while (0)
static char g_what[96] = "";

// ---- the rule before: the launch sites' formulas
namespace old {
constexpr size_t k2_lds_bytes_body(int D, int lik_cap = LIK_LDS_CAP) {
    return (size_t)(2 * D * D + 12 * D + 8 + 2 * LIK_PAR_MAX + lik_cap) * sizeof(double) + (size_t)(6 * D + 8) * sizeof(int) + 32;
}
constexpr size_t k2_lds_bytes(int D, int lik_cap = LIK_LDS_CAP) {
    const size_t np = (size_t)(D + 1) * (D + 2) / 2, npf = np + 2;
    return (size_t)(2 * D * D + 12 * D + 8 + 2 * LIK_PAR_MAX + lik_cap) * sizeof(double) + (size_t)(6 * D + 8) * sizeof(int) + 32 +
           (V2_MAXV * (npf + 1) + npf + 5 + 4 * D * D + 2 * D) * sizeof(double) + (size_t)(3 * D + 4) * sizeof(int) + 32;
}
constexpr int mutate_wave_bytes_ls4(int d) {
    return (2 * d * 16 * 8 + ((2 * d * 16 * 8 > 16 * KALMAN4_SLOT_BYTES) ? 2 * d * 16 * 8 : 16 * KALMAN4_SLOT_BYTES) + 15) / 16 * 16;
}
constexpr size_t k2w_lds_bytes(int D, int LS) {
    const size_t pro = (k2_lds_bytes(D, 0) + 15) / 16 * 16;
    return pro + (LS == 4 ? (size_t)4 * mutate_wave_bytes_ls4(13) : (size_t)4 * D * 256 * sizeof(double)) + 64;
}
static size_t reg_lds_bytes(int D) {
    return (size_t)(2 * D * D + 12 * D + 4 + 2 * LIK_PAR_MAX + LIK_LDS_CAP) * sizeof(double) + (size_t)(6 * D + 8) * sizeof(int) + 32;
}
static size_t mut_lds(int d, int T) { return (size_t)(4 * d * T + T / 64) * sizeof(double) + (d <= 13 ? 64 + sizeof(MutStage) : 0); }
static size_t mut_lds_ls4() { return 4 * mutate_wave_bytes_ls4(13) + 64 + sizeof(MutStage); }
static size_t mom_lds(int d) { const int npairs = (d + 1) * (d + 2) / 2; return (size_t)((d + 2) * (MT + 1)) * sizeof(double) + 2 * (size_t)npairs + 16; }
static size_t prep_lds(int d) { const int npairs = (d + 1) * (d + 2) / 2; return (size_t)(((npairs + 63) / 64) * 64 + 4 * d * d + 8) * sizeof(double); }
constexpr size_t k3_gather_lds_bytes(int D) {
    const size_t npf = (size_t)(D + 1) * (D + 2) / 2 + 2, mcm = npf + (npf & 1);
    return (size_t)2 * GRP * (mcm > (size_t)RMUT ? mcm : (size_t)RMUT) * sizeof(double);
}
constexpr size_t k3_park_offset(int D) { return (k2_lds_bytes(D) + 15) / 16 * 2; }          // in doubles, 16-byte aligned
constexpr size_t k3_lds_bytes(int D, int sel_cols = 0) {
    return k3_park_offset(D) * sizeof(double) + (size_t)(D + 2) * T3 * sizeof(double) + (size_t)sel_cols * T3 * sizeof(double);
}
constexpr int k3_sel_cols(int D, bool alpha1) {
    return (alpha1 || 24 * 1024 + ((size_t)T3 * D + 3 * D * D + 3 * D + 2) * sizeof(double) + k3_lds_bytes(D, D + 5) <= 160 * 1024) ? D + 5 : 0;
}
}  // namespace old

// placement of members 0 .. n-1: aligned as asked and at least to the element, inside `limit`, live members disjoint, overlays on their host
template <int N>
static void placement(const Layout<N> &l, int n, size_t limit) {
    for (int i = 0; i < n; ++i) {
        const Member &a = l.m[i];
        CHECK(a.align >= 1 && a.off % a.align == 0);
        CHECK(a.elem == 1 || a.elem > 8 || a.align % a.elem == 0);        // (a double on 8, an int on 4; a struct on the 8 of its doubles)
        CHECK(a.elem <= 8 || a.align % 8 == 0);
        if (a.over < 0) CHECK(a.end() <= limit);
        else CHECK(a.off == l.m[a.over].off && l.m[a.over].over < 0);
        for (int j = 0; j < i; ++j) {
            const Member &b = l.m[j];
            if (a.over >= 0 || b.over >= 0 || a.count == 0 || b.count == 0) continue;
            CHECK(a.end() <= b.off || b.end() <= a.off);
        }
    }
    CHECK(l.at <= l.bytes || l.bytes == 0);
}

int main() {
    using namespace lds;
    // ---- Mut2Lds (k2_mutate, k2_prepare, k2_prepare_block, k2b_mutate, k3_segment; without likelihood data: k2w_mutate) and k2w
    for (int D = 1; D <= 16; ++D)
        for (int cap : {LIK_LDS_CAP, 0}) {
            std::snprintf(g_what, sizeof g_what, "mut2 D=%d cap=%d", D, cap);
            const Mut2Layout l = mut2(D, 8, cap);
            CHECK(l.bytes == old::k2_lds_bytes(D, cap));
            CHECK(l.body_bytes == old::k2_lds_bytes_body(D, cap));
            placement(l, M_N, l.bytes);
            CHECK(l[M_svt] % 16 == 0 && l[M_Ls] % 16 == 0);             // (16-byte loads)
            for (int i = 0; i < M_BODY_N; ++i) CHECK(l.m[i].end() <= l.body_bytes);
            CHECK(l[M_svt] <= l.body_bytes && l[M_svt] >= l.m[M_ballr].end());       // the scratch starts inside the body's slack
            const Mut2Layout b = mut2(D, 8, cap, false);                // the body alone: the same prefix
            CHECK(b.bytes == old::k2_lds_bytes_body(D, cap) && b.bytes == l.body_bytes);
            for (int i = 0; i < M_BODY_N; ++i) CHECK(b.m[i].off == l.m[i].off && b.m[i].count == l.m[i].count && b.m[i].elem == l.m[i].elem);
            placement(b, M_BODY_N, b.bytes);
        }
    for (int D = 1; D <= 16; ++D)
        for (int LS : {1, 4}) {
            std::snprintf(g_what, sizeof g_what, "k2w D=%d LS=%d", D, LS);
            const Layout<W_N> l = k2w(D, LS);
            CHECK(l.bytes == old::k2w_lds_bytes(D, LS));
            placement(l, W_N, l.bytes);
            CHECK(l[W_cols] % 16 == 0 && l[W_cols] == (old::k2_lds_bytes(D, 0) + 15) / 16 * 16);
            CHECK(l.m[W_mut2].count == mut2(D, 8, 0).bytes);
        }
    // ---- k_mutate_reg: the body with red of 4
    for (int D = 1; D <= 10; ++D) {
        std::snprintf(g_what, sizeof g_what, "reg D=%d", D);
        const Mut2Layout r = mut2(D, 4, LIK_LDS_CAP, false), b = mut2(D, 8, LIK_LDS_CAP, false);
        CHECK(r.bytes == old::reg_lds_bytes(D));
        placement(r, M_BODY_N, r.bytes);
        CHECK(r.m[M_red].count == 4 && b.m[M_red].count == 8);
        for (int i = 0; i < M_BODY_N; ++i) {
            CHECK(r.m[i].elem == b.m[i].elem && r.m[i].align == b.m[i].align && (i == M_red || r.m[i].count == b.m[i].count));
            CHECK(r.m[i].off + (i > M_red ? 4 * sizeof(double) : 0) == b.m[i].off);
        }
    }
    // ---- the per-particle vectors and the four-lane wavefront areas; k_mutate
    for (int d = 1; d <= MAXD; ++d) {
        std::snprintf(g_what, sizeof g_what, "cols d=%d", d);
        CHECK(mutate_wave_bytes_ls4(d) == old::mutate_wave_bytes_ls4(d));
        const Layout<C_N> w = mut_cols(d, 16, 4);
        placement(w, C_N, w.bytes);
        CHECK(w.m[C_slots].over == C_y && w[C_slots] % 16 == 0 && w.m[C_slots].end() <= w.bytes && w.bytes % 16 == 0);      // the declared overlay
        CHECK(w.m[C_slots].count == (size_t)16 * KALMAN4_SLOT_BYTES && KALMAN4_SLOT_BYTES % 16 == 0);
        for (int T : {256, 128, 64}) {
            std::snprintf(g_what, sizeof g_what, "mutate d=%d T=%d", d, T);
            const Layout<C_N> c = mut_cols(d, T, 1);
            placement(c, C_slots, c.bytes);
            CHECK(c.bytes == (size_t)4 * d * T * sizeof(double) && c[C_tn] == (size_t)d * T * 8 && c[C_y] == (size_t)2 * d * T * 8 && c[C_v] == (size_t)3 * d * T * 8);
            const Layout<G_N> l = mutate(d, T, 1, d <= 13);
            CHECK(l.bytes == old::mut_lds(d, T));
            placement(l, G_N, l.bytes);
            CHECK(l[G_red] == c.bytes);
            if (d <= 13) CHECK(l[G_stage] == l[G_red] + 8 * sizeof(double) && l.m[G_stage].end() <= l.bytes);
            const Layout<G_N> u = mutate(d, T, 1, false);               // (modes that stage nothing in a launch sized for the stage)
            CHECK(u[G_red] == l[G_red] && u.m[G_red].end() <= l.bytes);
        }
    }
    {
        std::snprintf(g_what, sizeof g_what, "mutate LS=4");
        const Layout<G_N> l = mutate(LS4_D, 16, 4, true);
        CHECK(l.bytes == old::mut_lds_ls4());
        placement(l, G_N, l.bytes);
        CHECK(l[G_red] == (size_t)4 * old::mutate_wave_bytes_ls4(13) && l[G_stage] == l[G_red] + 64 && l.m[G_stage].end() == l.bytes);
    }
    // ---- k_prepare_mutation and k_moments
    for (int d = 1; d <= MAXD; ++d) {
        for (int nf = 1; nf <= d; ++nf) {
            std::snprintf(g_what, sizeof g_what, "prep d=%d nf=%d", d, nf);
            const Layout<P_N> l = prep(d, nf);
            CHECK(l.bytes == old::prep_lds(d));
            placement(l, P_N, l.bytes);
            CHECK(l[P_tot] == 0 && l[P_covl] % 16 == 0);
        }
        std::snprintf(g_what, sizeof g_what, "moments d=%d", d);
        const Layout<O_N> l = moments(d);
        CHECK(l.bytes == old::mom_lds(d));
        placement(l, O_N, l.bytes);
        CHECK(l.m[O_pa].count == (size_t)(d + 1) * (d + 2) / 2 && l.m[O_pb].off == l.m[O_pa].end());
    }
    // ---- k3_segment
    for (int D = 1; D <= 10; ++D) {
        for (bool a1 : {true, false}) {
            std::snprintf(g_what, sizeof g_what, "seg3 D=%d alpha1=%d", D, (int)a1);
            CHECK(k3_sel_cols(D, a1) == old::k3_sel_cols(D, a1));
            for (int CH : {1, 2}) {
                if (CH == 2 && !a1) continue;
                const int cols = CH == 2 ? D + 6 : old::k3_sel_cols(D, a1);
                const Seg3Layout l = k3_layout(D, a1, CH);
                CHECK(l.bytes == old::k3_lds_bytes(D, cols));
                CHECK(l.gather_bytes == old::k3_gather_lds_bytes(D));
                CHECK(l[S_park] == old::k3_park_offset(D) * sizeof(double) && l[S_park] % 16 == 0);
                CHECK(l[S_cols] == l[S_park] + (size_t)(D + 2) * T3 * sizeof(double) && l.m[S_cols].count == (size_t)cols * T3);
                CHECK(l.m[S_mut2].count == mut2(D).bytes);
                placement(l, S_N, l.bytes);
                CHECK(l.m[S_gather].over == S_mut2 && l.m[S_gather].end() == l.gather_bytes);
                const size_t want = CH == 2 ? (old::k3_lds_bytes(D, D + 6) + 1023) / 1024 * 1024
                                            : (std::max(old::k3_lds_bytes(D, old::k3_sel_cols(D, a1)), old::k3_gather_lds_bytes(D)) + 1023) / 1024 * 1024;
                CHECK(k3_max_lds_bytes(D, a1, CH) == want);
                // the fixed text form tests/test_abi_cpu.py reads: the largest dynamic request (whole KB, as the kernel is opted in) and,
                // for the mixture kernels, the static LDS k3_sel_cols takes the kernel to have at most
                std::printf("k3_segment D=%d alpha1=%d chunks=%d max_dynamic=%zu assumed_static=%zu\n", D, (int)a1, CH, k3_max_lds_bytes(D, a1, CH),
                            a1 ? (size_t)0 : K3_STATIC_REST + k3_mix_static_bytes(D));
            }
        }
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
