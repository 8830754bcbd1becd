// route_check.hip - prints the routing table of csrc/route.hpp: one line per (shape, run kind, switch set) with the driver, engine 2's
// geometry, the Kalman lanes and the segment shape at 256 CUs.  Host code only, no device needed:
//     hipcc --offload-arch=gfx950 --offload-host-only -O1 -std=c++17 tests/route_check.hip -o route_check
// tests/test_abi_cpu.py builds it, runs it and compares the output with tests/golden/routing_table.txt, which was recorded from the
// hand-written predicates route.hpp replaced (make_geo2, eng2_eligible, two_chunk_run, seg3_ready, run2_guarded at commit 3245866).
#include "../smc.jl_amd/csrc/handle.hpp"
#include "../smc.jl_amd/csrc/switches.hpp"
#include "../smc.jl_amd/csrc/route.hpp"

enum Entry { RUN, RCCL, GROUP };                 // smcmi_run, smcmi_run_sharded (one handle per process), smcmi_run_group
struct Kind { const char *name; double alpha; int n_blocks, n_mh_steps, lik0; bool closure; };
static const Kind KINDS[] = {
    {"alpha1", 1.0, 1, 1, SMCMI_LIK_GAUSS_ISO, false},
    {"alpha09", 0.9, 1, 1, SMCMI_LIK_GAUSS_ISO, false},
    {"capm3mh", 1.0, 1, 3, SMCMI_LIK_CAPM_LITERAL, false},
    {"closure", 1.0, 1, 1, SMCMI_LIK_HOST_CALLBACK, true},
    {"kalman", 1.0, 1, 1, SMCMI_LIK_LGSS_KALMAN, false},
};
struct Case { Entry entry; long long n; int world, rank, d; const Kind *kind; int max_stages; };
struct Row { const char *driver; int geo_ok; Geo2 g; int ls4, ch, grid, agree, snap; };
static const int N_CU = 256;

static Row evaluate(const Case &c, const Switches &s) {
    RunShape r;
    r.n = c.n; r.N = c.n * c.world; r.d = c.d; r.world = c.world; r.rank = c.rank;
    r.n_handles = c.entry == GROUP ? c.world : 1;
    r.rccl = c.entry == RCCL; r.single = r.n_handles == 1 && !r.rccl; r.group_call = c.entry != RUN;
    r.lik0 = c.kind->lik0; r.lik1 = SMCMI_LIK_NONE; r.closure = c.kind->closure; r.max_stages = c.max_stages;
    const RunPlan p = plan_run(r, c.kind->alpha, c.kind->n_blocks, c.kind->n_mh_steps, s, N_CU);
    static const char *names[] = {"CALLBACK", "ENGINE1", "SHARDED1", "ENGINE2"};
    Row o{};
    o.driver = names[p.driver];
    o.ls4 = p.ls4;
    if (p.driver != DRIVER_ENGINE2) return o;
    o.geo_ok = p.geo_ok; o.g = p.geo; o.ch = p.seg_chunks; o.grid = p.seg_grid; o.agree = p.seg_agree; o.snap = p.snapshot;
    return o;
}

// columns: switch set, entry, n per handle, world, rank, n_para, run kind, max_stages | driver, Kalman lanes (ls4) | for engine 2: V Vl v0 nv nb1
// nb2 nbg per1 perg t2 direct inker wide | segment chunks, grid, agreement round, snapshot
static void line(const char *set, const Case &c, const Switches &s) {
    static const char *entries[] = {"run", "rccl", "group"};
    const Row o = evaluate(c, s);
    const Geo2 &g = o.g;
    printf("%s %s %lld %d %d %d %s %d | %s %d", set, entries[c.entry], c.n, c.world, c.rank, c.d, c.kind->name, c.max_stages, o.driver, o.ls4);
    if (o.geo_ok) printf(" | %d %d %d %lld %d %d %d %lld %lld %d %d %d %d | %d %d %d %d", g.V, g.Vl, g.v0, g.nv, g.nb1, g.nb2, g.nbg, g.per1, g.perg, g.t2,
                         g.direct, g.inker, g.wide, o.ch, o.grid, o.agree, o.snap);
    printf("\n");
}
static void table(const char *set, const Switches &s) {
    const Kind *A = &KINDS[0], *KAL = &KINDS[4];
    // one handle, and the communicator / the group of one rank: both sides of every boundary of the geometry, the uneven cut, small and huge clouds
    const long long NS[] = {4096, 5000, 32768, 32769, 100000, 100001, 126976, 126977, 131072, 131073, 150004, 250000, 253952, 253953, 1000000, 10000000};
    for (long long n : NS) {
        for (Entry e : {RUN, RCCL, GROUP})
            for (int d : {10, 11}) line(set, Case{e, n, 1, 0, d, A, 1200}, s);
        for (int k = 1; k <= 3; ++k) line(set, Case{RUN, n, 1, 0, 10, &KINDS[k], 1200}, s);
    }
    for (long long n : {5000ll, 100000ll, 1000000ll})
        for (Entry e : {RUN, RCCL, GROUP})
            for (int d : {16, 17, 40}) line(set, Case{e, n, 1, 0, d, A, 1200}, s);
    for (long long n : {100000ll, 250000ll})
        for (Entry e : {RCCL, GROUP})
            for (int k = 1; k <= 3; ++k) line(set, Case{e, n, 1, 0, 10, &KINDS[k], 1200}, s);
    for (long long n : {32768ll, 32769ll})
        for (Entry e : {RUN, RCCL, GROUP}) line(set, Case{e, n, 1, 0, 13, KAL, 1200}, s);
    line(set, Case{RUN, 100000, 1, 0, 10, A, 65536}, s);                 // (a segment counts its stages in 16 bits)
    // several handles: n per handle on both sides of the in-kernel and the segment limits
    for (int world : {2, 4, 8})
        for (long long n : {65536ll, 65537ll, 131072ll, 131073ll})
            for (Entry e : {RCCL, GROUP}) {
                for (int rank : {0, world - 1}) line(set, Case{e, n, world, rank, 10, A, 1200}, s);
                line(set, Case{e, n, world, 0, 11, A, 1200}, s);
                line(set, Case{e, n, world, 0, 10, &KINDS[1], 1200}, s);
            }
    for (long long n : {32768ll, 32769ll})
        for (Entry e : {RCCL, GROUP})
            for (int rank : {0, 1}) line(set, Case{e, n, 2, rank, 13, KAL, 1200}, s);
    for (Entry e : {RCCL, GROUP}) line(set, Case{e, 65536, 2, 0, 10, &KINDS[3], 1200}, s);
}

int main() {
    Switches none, eng1, eng2, reduced, e3off, lanes1;
    eng1.engine = 1; eng2.engine = 2; reduced.e2_reduced = true; e3off.engine3 = 0; lanes1.kalman_lanes = 1;
    table("none", none);
    table("ENGINE=1", eng1);
    table("ENGINE=2", eng2);
    table("E2_REDUCED=1", reduced);
    table("ENGINE3=0", e3off);
    table("KALMAN_LANES=1", lanes1);
    return 0;
}
