// route.hpp - where a run goes: ONE pure function from the shape of a run (RunShape), its proposal settings and the development switches
// to the driver that serves it, the virtual-shard geometry of engine 2, the lanes of the Kalman mutation and the shape of engine 3's
// persistent segments (RunPlan).  No handle, no environment, no HIP call: tests/route_check.hip prints the table without a GPU
// (tests/golden/routing_table.txt), and DESIGN §0's "Stage engines" rows are decided here.  The entry points (smcmi.hip), ensure_eng2,
// seg3_ready and run2_guarded consume the plan; what a self-test or an earlier time-out decides (Eng2::e3_state, mbox_ok, the mailbox
// itself) stays with them.  Included by smcmi.hip behind handle.hpp (Geo2 and the block constants) and switches.hpp.
#pragma once

struct RunShape {
    long long N = 0, n = 0;          // particles of the cloud / of this handle
    int d = 0;                       // n_para
    int world = 1, rank = 0;         // shards of the cloud, this handle's
    int n_handles = 1;               // handles of the run in this process
    bool single = true;              // one handle of one process without a communicator: not a communicator of one rank, whose handle keeps
                                     // the geometry its larger worlds have
    bool rccl = false;               // one handle per process (smcmi_run_sharded)
    bool group_call = false;         // came through smcmi_run_sharded / smcmi_run_group: what engine 2 does not serve is run_sharded_impl's
    int lik0 = SMCMI_LIK_NONE, lik1 = SMCMI_LIK_NONE;       // the two likelihood families
    bool closure = false;            // a user likelihood, host callback or device callback (nothing routes on which of the two)
    int max_stages = 0;
};
enum RunDriver { DRIVER_CALLBACK, DRIVER_ENGINE1, DRIVER_SHARDED1, DRIVER_ENGINE2 };     // run_callback, run1_impl, run_sharded_impl, run2_guarded
struct RunPlan {
    RunDriver driver = DRIVER_ENGINE1;
    bool geo_ok = false;             // engine 2 has a geometry for this handle (`geo`)
    Geo2 geo{};
    bool ls4 = false;                // lgss_kalman: four lanes per particle
    int seg_chunks = 0;              // 512-particle chunks per segment worker: 0 = the shape (or SMCMI_ENGINE3) admits no segments, 1 or 2
    int seg_grid = 0;                // ... and the segment's grid: workers + one gatherer per virtual shard, one CU each
    bool seg_agree = false;          // several handles / a communicator: the ranks agree on segments through an all-reduce - entered by
                                     // switch and handle count alone, never by what one device's CU count admits (every rank must enter alike)
    bool snapshot = false;           // the run keeps the cloud it started from: a segment time-out repeats it as launches (run2_guarded)
};

// lgss_kalman on both vintages (or no old vintage) and at most 32 768 particles on the handle: four lanes per particle (kernels.hpp
// k_mutate<0, 4>) - up to two of its wavefronts per SIMD; beyond that one thread per particle (fewer instructions per particle) is
// faster (measured: §6 of DESIGN.md).  SMCMI_KALMAN_LANES=1 / 4 forces one or the other (development / comparison).
static bool kalman_model(const RunShape &r) {
    return r.d == 13 && r.lik0 == SMCMI_LIK_LGSS_KALMAN && (r.lik1 == SMCMI_LIK_NONE || r.lik1 == SMCMI_LIK_LGSS_KALMAN);
}
static bool route_ls4(const RunShape &r, const Switches &s) {
    return kalman_model(r) && (s.kalman_lanes == 4 || (s.kalman_lanes != 1 && r.n <= 32768));
}

// virtual-shard geometry of a handle that is shard `rank` of `world` (a function of N and the shard count's divisibility only)
static bool make_geo2(const RunShape &r, const Switches &s, Geo2 *out) {
    const int world = r.world;
    Geo2 g{};
    g.N = r.N; g.n = r.n;
    if (world < 1 || g.n * world != g.N) return false;
    int V = 0;
    for (int cand : {8, 4, 2, 1})
        if (cand % world == 0 && g.n % (cand / world) == 0) { V = cand; break; }
    if (!V) { if (world <= V2_MAXV) V = world; else return false; }
    g.V = V; g.Vl = V / world; g.v0 = r.rank * g.Vl; g.nv = g.n / g.Vl;
    if (g.nv < 1) return false;
    // n_para > 10: the generic mutation body behind engine 2's prologues (stage2.hpp k2w_mutate) - 256 particles per block with one
    // thread per particle, 64 with four lanes per particle (lgss_kalman on small clouds); rows always totalled per virtual shard (Tail2)
    g.wide = r.d > 10 ? (route_ls4(r, s) ? 4 : 1) : 0;
    if (g.wide) {
        g.t2 = g.wide == 4 ? 64 : 256;
        g.nb2 = (int)((g.nv + g.t2 - 1) / g.t2);
        if (g.nv > 65536 || (long long)g.nb2 * g.Vl > 1024) return false;      // (a correction row is 512 particles, one per thread: nb1 <= 128)
        g.direct = 0; g.inker = 1;
        g.nb1 = (int)std::max<long long>(1, (g.nv + 511) / 512);
        g.per1 = T1;
        g.nbg = (int)std::max<long long>(1, std::min<long long>((g.nv + 511) / 512, 256));
        g.perg = ((g.nv + g.nbg - 1) / g.nbg + 255) / 256 * 256;
        *out = g;
        return true;
    }
    g.t2 = 512;
    g.nb2 = (int)((g.nv + g.t2 - 1) / g.t2);
    // direct: every block totals the per-block rows itself - one handle, <= GRP rows per virtual shard, and the 512-thread mutation
    // blocks (one per CU) resident at once
    // (beyond 256 blocks - up to 62 per virtual shard - the persistent segments give every worker two chunks: stage3.hpp k3_segment<D, true, RIDE, 2>;
    // plan_run keeps such a cloud on engine 1 unless its run qualifies for them)
    g.direct = (r.single && world == 1 && g.nb2 <= GRP && (long long)g.nb2 * V <= 2 * (256 - V2_MAXV)) ? 1 : 0;
    if (s.e2_reduced) g.direct = 0;                                    // development: force the k2_reduce path on one handle
    // several handles with small shards: one 512-thread mutation block per CU as well, prologues in the kernels, fed by the gathered totals
    g.inker = (g.direct || (!r.single && (long long)g.nb2 * g.Vl <= 256)) ? 1 : 0;
    // large shards (stage2b.hpp k2b_mutate): the same 512-particle mutation blocks at half the registers - two per CU, 4 wavefronts per SIMD
    // (256-thread blocks - 489 raw rows per virtual shard at 125 000 particles, paired into canonical rows by whoever totals them - cost
    // the block that totals a shard's rows ~10 µs at the END of every mutation launch: twice the loads, a quarter of them in flight)
    // correction blocks per virtual shard: 1024 particles per block (two passes of its 512 threads), at most 16 rows per virtual shard for
    // K2's prologue to total while the cloud is small
    // (the direct geometry: one correction row per 512 particles, the same particles as a mutation row - the persistent segment kernel
    // of stage3.hpp holds one particle per thread and writes exactly these rows, so both engines total the same numbers)
    // every geometry cuts a virtual shard the same way, so all of them total the same rows (<= 128 rows per virtual shard: the blocks
    // grow beyond 512 particles for nv > 65 536, where the direct geometry does not exist)
    g.nb1 = (int)std::max<long long>(1, g.direct ? g.nb2 : std::min<long long>((g.nv + 511) / 512, 128));
    if (s.e2_nb1.set) g.nb1 = std::max(1, std::min(s.e2_nb1.v, g.direct ? 64 : 128));   // development only (tools/shard_rank_prof.sh: one rank's share of a larger run)
    g.per1 = ((g.nv + g.nb1 - 1) / g.nb1 + T1 - 1) / T1 * T1;                        // whole passes of the block
    // (one 512-slot tile per gather block up to GRP rows per virtual shard on one handle as on several: a cloud of 4 x odd or 2 x odd particles -
    // 33 .. 64 rows per shard - had two-tile blocks on one handle until round 6, i.e. moment rows summed in another order than its sharded runs')
    g.nbg = (int)std::max<long long>(1, std::min<long long>((g.nv + 511) / 512, g.direct ? GRP : 256));
    g.perg = ((g.nv + g.nbg - 1) / g.nbg + 255) / 256 * 256;
    // (a virtual shard of at most 256 particles: one gather block of ONE 512-slot tile all the same - the block a segment worker is, so that
    // clouds of a few thousand particles resample inside their segments too)
    if (g.direct && g.perg < 512) g.perg = 512;
    if ((long long)g.V * g.nb1 > 1024) return false;
    *out = g;
    return true;
}
// One handle whose particle count has no divisor among 8 / 4 / 2 that leaves it the direct geometry (100 001 particles: one virtual
// shard of 196 rows - engine 1's stage at twice the time): virtual shards of ceil(n / V) particles, the last one shorter (vchunk and
// k2_scan clamp at n; a block beyond the end holds no particle and publishes zero rows).  Only where no sharded run of the same
// cloud shares the canonical order anyway (such a cloud runs on engine 1 today, which has another order).
static bool make_geo2_uneven(const RunShape &r, const Switches &s, Geo2 *out) {
    if (r.d > 10 || s.e2_reduced) return false;
    for (int V : {8, 4, 2}) {
        Geo2 g{};
        g.N = r.N; g.n = r.n;
        if (g.n != g.N) return false;
        g.V = V; g.Vl = V; g.v0 = 0; g.nv = (g.n + V - 1) / V;
        if ((long long)(V - 1) * g.nv >= g.n) continue;                              // (no empty virtual shard)
        g.wide = 0; g.t2 = 512;
        g.nb2 = (int)((g.nv + g.t2 - 1) / g.t2);
        if (!(g.nb2 <= GRP && (long long)g.nb2 * V <= 2 * (256 - V2_MAXV))) continue;
        g.direct = 1; g.inker = 1;
        g.nb1 = g.nb2;
        g.per1 = ((g.nv + g.nb1 - 1) / g.nb1 + T1 - 1) / T1 * T1;
        g.nbg = (int)std::max<long long>(1, std::min<long long>((g.nv + 511) / 512, GRP));      // (one tile per gather block, like make_geo2's: in-place selection beyond 32 rows)
        g.perg = ((g.nv + g.nbg - 1) / g.nbg + 255) / 256 * 256;
        if (g.perg < 512) g.perg = 512;
        *out = g;
        return true;
    }
    return false;
}
// The geometry a handle gets: ONE rule for building it (ensure_eng2) and for asking whether engine 2 serves the run (plan_run).  The uneven
// cut replaces only a geometry that would send the handle to engine 1; a cloud forced onto engine 2 (SMCMI_ENGINE=2) keeps the canonical cut
// a sharded run of the same cloud has, so run2.hpp's contract - results do not depend on the number of handles - holds for it.
static bool route_geo2(const RunShape &r, const Switches &s, Geo2 *out) {
    if (!make_geo2(r, s, out)) return false;
    if (r.single && r.world == 1 && !out->wide && !out->direct && s.engine != 2) { Geo2 gu; if (make_geo2_uneven(r, s, &gu)) *out = gu; }
    return true;
}

// Two chunks per segment worker (one handle of 126 977 .. 253 952 particles) pay where a stage is hand-overs and serial work, not likelihood
// evaluations: α = 1, one block, one MH step, a likelihood that is a handful of flops per datum.  (Measured in round 5: the 10-dim Gaussian at
// 250 000 particles 47.5 against engine 1's 63 µs per stage; config 4 - CAPM, three MH steps - 30.6 against 29.6 ms per run: MH-bound runs stay on engine 1.)
static bool two_chunk_run(const RunShape &r, double alpha, int n_blocks, int n_mh_steps) {
    auto cheap = [](int fam) { return fam == SMCMI_LIK_GAUSS_ISO || fam == SMCMI_LIK_LINREG || fam == SMCMI_LIK_NONE; };
    return alpha == 1.0 && r.d <= 10 && n_blocks == 1 && n_mh_steps == 1 && cheap(r.lik0) && cheap(r.lik1);
}

// Engine 2 serves n_para <= 10: one handle while its cloud is small enough for the direct geometry (every block totals the rows
// itself: the latency-bound regime engine 2 was built for), and every multi-handle run (one all-gather of V rows per hand-over,
// results independent of the number of handles).  A single handle with a larger cloud keeps engine 1: its kernels fill the chip
// there and one-block set-up launches are cheap next to them (engine 2's reduced geometry measured 10-15 % behind at N >= 1e6).
// SMCMI_ENGINE=1 / =2 force one engine wherever it can run (development, tests).
// Engine 3 serves a handle in the direct (or in-kernel) geometry whose blocks are all resident at one per CU (`n_cu`); SMCMI_ENGINE3=0
// leaves every handle on engine 2's launches, =2 the handles of a group, =3 admits in-process groups of any size.
static RunPlan plan_run(const RunShape &r, double alpha, int n_blocks, int n_mh_steps, const Switches &s, int n_cu) {
    RunPlan p;
    p.ls4 = route_ls4(r, s);
    p.geo_ok = route_geo2(r, s, &p.geo);
    const Geo2 &g = p.geo;
    const bool two_ok = two_chunk_run(r, alpha, n_blocks, n_mh_steps);
    const bool alone = r.single && r.world == 1;
    bool e2 = !r.closure && s.engine != 1 && r.d <= 16 && p.geo_ok;
    // (one handle with more than 256 - V blocks: only the two-chunk segments make engine 2's geometry worth it there)
    if (e2 && alone && g.direct && (long long)g.nb2 * g.V > 256 - V2_MAXV && !two_ok && s.engine != 2) e2 = false;
    // n_para 11 .. 16: the same two-launch stage around the generic mutation body (SMCMI_ENGINE=1: engine 1's stage)
    // (a communicator of one rank is a sharded run: the measurement vehicle for one rank's share)
    if (e2 && !g.wide && !(s.engine == 2 || r.world > 1 || !r.single || g.direct)) e2 = false;
    // n_para > 10 behind a communicator or in a group, and every run with a user likelihood there: run_sharded_impl
    p.driver = e2 ? DRIVER_ENGINE2 : (r.group_call ? DRIVER_SHARDED1 : (r.closure ? DRIVER_CALLBACK : DRIVER_ENGINE1));
    if (!e2) return p;
    // ---- engine 3's segments: workers + one gatherer per virtual shard, one CU each; a cloud with more 512-particle blocks than that gives
    // every worker two of them (one handle, a run two_chunk_run admits)
    const bool one = alone && !r.rccl && r.n_handles == 1;
    // (handles of ONE process share the device's few hardware queues: beyond two of them a handle's persistent launch can sit in a queue
    // in front of the launch it waits for - the in-process group driver, a test vehicle, keeps to launches there; SMCMI_ENGINE3=3 forces segments)
    p.seg_agree = !one && s.engine3 != 2 && (r.n_handles <= 2 || s.engine3 == 3);
    const bool admitted = s.engine3 != 0 && (one || p.seg_agree);
    const int ch = (g.Vl * g.nb2 + g.Vl <= n_cu) ? 1 : 2;
    const int grid = g.Vl * ((g.nb2 + ch - 1) / ch) + g.Vl;
    // (the tables a segment needs exist where the rows of K1 and K2 are the same 512 particles: ensure_eng2; a gatherer totals at most two
    // canonical groups of rows: stage3.hpp gather_vshard)
    const bool tables = g.direct || (g.inker && !g.wide && g.t2 == T3 && g.nb1 == g.nb2);
    if (admitted && (ch == 1 || (one && two_ok)) && tables && !g.wide && g.nb1 == g.nb2 && g.nb2 <= 2 * GRP && g.per1 == T3 && g.t2 == T3 &&
        grid <= n_cu && r.max_stages < 65536) { p.seg_chunks = ch; p.seg_grid = grid; }
    // (the snapshot's limits are those of the segment kernels: two chunks of 62 rows in 8 virtual shards on one handle, 128 rows per handle of a group)
    p.snapshot = s.engine3 != 0 && r.d <= 10 && (one || s.engine3 != 2) && r.n <= (one ? 253952 : 131072);
    return p;
}
