// launch2.hpp - host launchers of the engine 2 kernels that are templates over n_para (stage2.hpp).  Each n_para is compiled in its
// own translation unit (inst2.hip with -DSMCMI_INST_D=<d>), so the sixty-odd instantiations build in parallel; every other
// translation unit sees the launchers as extern templates and instantiates none of the kernels.
#pragma once
#include "handle.hpp"

// opt a kernel in to `bytes` of dynamic LDS per block (beyond the default 64 KB)
template <class K>
static inline int set_max_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess ? 0 : SMCMI_ERR_HIP;
}

// pb.enable: the launch carries the helper block of stage2b.hpp (decision + proposal from this launch's own totals; large shards with the mailbox)
template <int D>
void launch_k2_correct(smcmi_handle *h, int n, int begin_done, int spec_expected, const Rows2 &mrows, const Tail2 &tail, const Prep2Args &pb) {
    Eng2 *e = h->e2;
    Rng2 ra{};
    unsigned grid = (unsigned)(e->g.Vl * e->g.nb1);
    const bool helper = pb.enable && tail.tick && D <= 10;
    if (e->rng_ahead) {              // extra blocks, one per mutation block, draw the stage's random numbers on the idle CUs
        ra.zbuf = h->d_zbuf; ra.n_steps = e->n_steps; ra.nb = e->n_blocks; ra.nf = h->h_model.n_free; ra.seed = h->cfg.seed; ra.gid0 = h->cfg.gid0;
        ra.t_lim = e->z_ahead;
        // (large shards: the drawing blocks follow the correction blocks onto the CUs - one 512-thread block each - and run under the helper's serial work)
        if (e->g.inker) grid += (unsigned)std::max(1, std::min(e->g.Vl * e->g.nb2, 256 - (int)grid));
        else grid += (unsigned)std::max<long long>(1, std::min<long long>((e->g.n + T1 - 1) / T1, 256));
    }
    if (helper) grid += 1;
    const size_t lds = helper ? lds::mut2(D).bytes : 0;
    Prep2Args pa = pb;
    pa.enable = helper ? 1 : 0;
    if (tail.tick) k2_correct<D, true><<<grid, T1, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, e->g, n, begin_done, spec_expected, mrows, h->d_sched, h->rec,
                                                           e->rows_cm, e->csum, h->d_wt, h->d_hist_w, h->n, ra, tail, pa, (e->d_prof && n == e->prof_stage) ? e->d_prof : nullptr);
    else k2_correct<D, false><<<grid, T1, 0, h->stream>>>(h->cl, h->d_st, e->d_ctl, e->g, n, begin_done, spec_expected, mrows, h->d_sched, h->rec,
                                                           e->rows_cm, e->csum, h->d_wt, h->d_hist_w, h->n, ra, tail, pa, (e->d_prof && n == e->prof_stage) ? e->d_prof : nullptr);
}
template <int D>
void launch_k2_gather(smcmi_handle *h, int n, const Rows2 &cmrows, const double *cum, int method, const double *full, long long s_lo, long long s_hi,
                      const double *wsel) {
    Eng2 *e = h->e2;
    if constexpr (D <= 10)
        k2_gather<D><<<e->g.Vl * e->g.nbg, TS, 0, h->stream>>>(h->cl, e->d_ctl, h->d_st, e->g, n, cmrows, cum, method, h->cfg.seed, h->cfg.gid0, h->d_anc, full,
                                                              h->n, e->rows_gm, s_lo, s_hi, wsel);
    else
        k2_gather_wide<D><<<e->g.Vl * e->g.nbg, TB, 0, h->stream>>>(h->cl, e->d_ctl, h->d_st, e->g, n, cmrows, cum, method, h->cfg.seed, h->cfg.gid0, h->d_anc, full,
                                                                   h->n, e->rows_gm, s_lo, s_hi, wsel);
}
template <int D>
int launch_k2_mutate(smcmi_handle *h, const Mut2Args &ma, int nb, bool alpha1) {
    Eng2 *e = h->e2;
    if constexpr (D > 10) {          // the generic mutation body behind K2's prologue (stage2.hpp k2w_mutate); e->g.wide = lanes per particle
        const unsigned gw = (unsigned)(e->g.Vl * e->g.nb2);
        if (!e->wide_attr_set) {     // (more than the default 64 KB of dynamic LDS per block: the per-particle vectors of 256 particles)
            if (set_max_lds(k2w_mutate<D, 1>, lds::k2w(D, 1).bytes)) return SMCMI_ERR_HIP;
            if constexpr (D == 13) { if (set_max_lds(k2w_mutate<13, 4>, lds::k2w(13, 4).bytes)) return SMCMI_ERR_HIP; }
            e->wide_attr_set = true;
        }
        if constexpr (D == 13) {
            if (e->g.wide == 4) { k2w_mutate<13, 4><<<gw, 256, lds::k2w(13, 4).bytes, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free); return 0; }
        }
        k2w_mutate<D, 1><<<gw, 256, lds::k2w(D, 1).bytes, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free);
        return 0;
    } else {
    const size_t lds = lds::mut2(D).bytes;
    const unsigned grid = (unsigned)(e->g.Vl * e->g.nb2);
    // (every block runs the prologue: the direct geometry and small shards of several handles; large shards are k2b_mutate's - launch_k2b_mutate)
    if (!ma.tail.tick) {             // the direct geometry (config 2): no hand-over code in the instantiation
        if (alpha1) k2_mutate<D, true, 512, false><<<grid, 512, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free);
        else k2_mutate<D, false, 512, false><<<grid, 512, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free);
    } else {
        if (alpha1) k2_mutate<D, true, 512, true><<<grid, 512, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free);
        else k2_mutate<D, false, 512, true><<<grid, 512, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, nb, h->h_model.n_free);
    }
    return 0;
    }
}
// the mutation launch of large shards (stage2b.hpp), compiled in translation units of its own (inst2b.hip, Makefile BIGFLAGS)
template <int D>
void launch_k2b_mutate(smcmi_handle *h, const Mut2Args &ma, const Beg2Args &bb, int nb, bool alpha1) {
    Eng2 *e = h->e2;
    if constexpr (D <= 10) {
        const size_t lds = lds::mut2(D).body_bytes;       // (the prologue's scratch behind it is never touched: 13 instead of 22 KB per block)
        const unsigned grid = (unsigned)(e->g.Vl * e->g.nb2) + (bb.enable ? 1u : 0u);
        if (alpha1) k2b_mutate<D, true><<<grid, T2B, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, bb, nb, h->h_model.n_free);
        else k2b_mutate<D, false><<<grid, T2B, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, bb, nb, h->h_model.n_free);
    }
}
template <int D>
void launch_k2_prepare(smcmi_handle *h, const Mut2Args &mp, int nb) {
    Eng2 *e = h->e2;
    if constexpr (D <= 10) k2_prepare<D><<<1, 256, lds::mut2(D).bytes, h->stream>>>(h->d_st, e->d_ctl, h->d_model, mp, nb, h->h_model.n_free, e->d_pre);
}
// one instantiation per (n_para, α = 1?, riding?): the proposal kinds are compiled with different flags (Makefile SEGFLAGS / SEGFLAGS_MIX).
// RIDE: fixed schedules under RunParams::shift_lag on one handle - a stage's correction row rides the mutation row in front of it (stage3.hpp k3_rides)
// CH = 2: two 512-particle chunks per worker (α = 1, one handle of up to 253 952 particles: run2.hpp seg3_ready), translation units of their own (inst3c / inst3cr)
// SYS: several handles (Seg3Args::peers set): translation units of their own as well (inst3s / inst3ms / inst3rs / inst3mrs)
template <int D, bool A1, bool RIDE, int CH = 1, bool SYS = false>
int launch_k3_seg(smcmi_handle *h, const Mut2Args &ma, const Seg3Args &sa, int nb) {
    Eng2 *e = h->e2;
    if constexpr (D <= 10 && CH == 2) {
        static_assert(A1, "two chunks per worker: the α = 1 kernel only");
        constexpr size_t lds2 = k3_layout(D, true, 2).bytes;     // (the parked chunk where the one-chunk kernel keeps the particle in transit)
        const unsigned grid2 = (unsigned)(e->g.Vl * ((e->g.nb2 + 1) / 2) + e->g.Vl);
        constexpr int bit2 = RIDE ? 32 : 16;
        if (!(e->seg_attr_set & bit2)) {
            if (set_max_lds(k3_segment<D, true, RIDE, 2>, k3_max_lds_bytes(D, true, 2))) return SMCMI_ERR_HIP;
            e->seg_attr_set |= bit2;
        }
        k3_segment<D, true, RIDE, 2><<<grid2, T3, lds2, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, ma, sa, nb, h->h_model.n_free);
    } else if constexpr (D <= 10) {
    // (a gatherer stages its shard's rows in the dynamic LDS: beyond GRP rows per virtual shard - several handles with 32 769 .. 65 536
    // particles per virtual shard - the small-n_para and the large mixture kernels' allocation would not hold them)
    constexpr lds::Seg3Layout O3 = k3_layout(D, A1, 1);
    const size_t lds = std::max(O3.bytes, e->g.nb2 > GRP ? O3.gather_bytes : (size_t)0);
    // workers + one gatherer per virtual shard.  One handle whose virtual shards are one or two blocks (stage3.hpp rows_direct / rows_two): the
    // workers take each other's rows themselves and nobody reads a gatherer's totals - none is launched (a gatherer that nothing waits for has
    // no flow control: one stage behind, it would poll for a tag its rows have already left and raise the waits' abort word)
    const bool gatherers = !(e->g.nb2 <= 2 && sa.peers == nullptr);
    const unsigned grid = (unsigned)(e->g.Vl * e->g.nb2 + (gatherers ? e->g.Vl : 0));
    constexpr int attr_bit = ((A1 ? 1 : 2) << (RIDE ? 2 : 0)) << (SYS ? 6 : 0);
    if (!(e->seg_attr_set & attr_bit)) {       // (per handle = per device: a function attribute belongs to the device's copy of the kernel)
        // (opt in to more than the default 64 KB per block: the kernel's static arrays come on top of `lds`; a CU has 160 KB)
        if (set_max_lds(k3_segment<D, A1, RIDE, 1, SYS>, k3_max_lds_bytes(D, A1, 1))) return SMCMI_ERR_HIP;
        e->seg_attr_set |= attr_bit;
    }
    Mut2Args mk = ma;
    if constexpr ((k3_fast_bits(A1, RIDE, 1, SYS) & A1F_PRIOR) != 0) mk.has_other = h->h_model.prior_shape;      // (this unit's MH step reads the PRIOR_* bits)
    k3_segment<D, A1, RIDE, 1, SYS><<<grid, T3, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, mk, sa, nb, h->h_model.n_free);
    }
    return 0;
}
// THE DEFAULT-RUN UNIT of k3_segment<D, true, false> (stage3.hpp SMCMI_K3_RUN: no stamps, gatherer geometry, one random block),
// translation units of its own (inst3_d<D>, next to the general unit's inst3g_d<D>): defined there alone, a symbol to everyone else
template <int D>
int launch_k3_seg_run(smcmi_handle *h, const Mut2Args &ma, const Seg3Args &sa, int nb);
#ifdef SMCMI_K3_RUN
template <int D>
int launch_k3_seg_run(smcmi_handle *h, const Mut2Args &ma, const Seg3Args &sa, int nb) {
    Eng2 *e = h->e2;
    constexpr lds::Seg3Layout O3 = k3_layout(D, true, 1);
    const size_t lds = std::max(O3.bytes, e->g.nb2 > GRP ? O3.gather_bytes : (size_t)0);      // (as launch_k3_seg)
    const unsigned grid = (unsigned)(e->g.Vl * e->g.nb2 + e->g.Vl);                            // workers + one gatherer per virtual shard, always
    constexpr int attr_bit = 1 << 10;
    if (!(e->seg_attr_set & attr_bit)) {
        if (set_max_lds(defrun::k3_segment<D, true, false>, k3_max_lds_bytes(D, true, 1))) return SMCMI_ERR_HIP;
        e->seg_attr_set |= attr_bit;
    }
    Mut2Args mk = ma;
    if constexpr ((k3_fast_bits(true, false, 1, false) & A1F_PRIOR) != 0) mk.has_other = h->h_model.prior_shape;
    defrun::k3_segment<D, true, false><<<grid, T3, lds, h->stream>>>(h->cl, h->d_st, e->d_ctl, h->d_model, e->g, mk, sa, nb, h->h_model.n_free);
    return 0;
}
#endif
// which unit a launch of the α = 1, two-hand-over, one-handle, one-chunk kernel takes: the default-run unit exactly when the launch is what that
// unit was compiled for (stage3.hpp K3U_*); anything else - and everything under SMCMI_K3_GENERAL=1 (Eng2::seg_general) - the general unit.
// Both leave memory alike: the batches of one run may differ in it.  (SMCMI_K3_KEEP & 1, development builds: the unit has its stamps)
inline bool k3_takes_run_unit(const Eng2 *e, const Seg3Args &sa, int nb) {
#if defined(SMCMI_K3_KEEP) && ((SMCMI_K3_KEEP) & 1)
    const bool stamps_ok = true;
#else
    const bool stamps_ok = sa.prof == nullptr && sa.gprof == nullptr;
#endif
    return !e->seg_general && nb == 1 && e->g.nb2 > 2 && stamps_ok;
}
template <int D>
inline int launch_k3_segment(smcmi_handle *h, const Mut2Args &ma, const Seg3Args &sa, int nb, bool alpha1, bool ride) {
    h->e2->seg_unit = SMCMI_SEG_UNIT_GENERAL;
    if constexpr (D <= 10) {
        if (h->e2->seg_ch != 2 && sa.peers == nullptr && alpha1 && !ride && k3_takes_run_unit(h->e2, sa, nb)) {
            h->e2->seg_unit = SMCMI_SEG_UNIT_RUN;
            return launch_k3_seg_run<D>(h, ma, sa, nb);
        }
    }
    if (h->e2->seg_ch == 2)               // (seg3_ready grants two chunks to α = 1 runs only)
        return ride ? launch_k3_seg<D, true, true, 2>(h, ma, sa, nb) : launch_k3_seg<D, true, false, 2>(h, ma, sa, nb);
    if (sa.peers != nullptr) {            // several handles
        if (alpha1) return ride ? launch_k3_seg<D, true, true, 1, true>(h, ma, sa, nb) : launch_k3_seg<D, true, false, 1, true>(h, ma, sa, nb);
        return ride ? launch_k3_seg<D, false, true, 1, true>(h, ma, sa, nb) : launch_k3_seg<D, false, false, 1, true>(h, ma, sa, nb);
    }
    if (alpha1) return ride ? launch_k3_seg<D, true, true>(h, ma, sa, nb) : launch_k3_seg<D, true, false>(h, ma, sa, nb);
    return ride ? launch_k3_seg<D, false, true>(h, ma, sa, nb) : launch_k3_seg<D, false, false>(h, ma, sa, nb);
}

#define SMCMI_LAUNCH2_INSTANCES(X, D)                                                                                              \
    X template void launch_k2_correct<D>(smcmi_handle *, int, int, int, const Rows2 &, const Tail2 &, const Prep2Args &);            \
    X template void launch_k2_gather<D>(smcmi_handle *, int, const Rows2 &, const double *, int, const double *, long long, long long, const double *); \
    X template int launch_k2_mutate<D>(smcmi_handle *, const Mut2Args &, int, bool);                                                \
    X template void launch_k2_prepare<D>(smcmi_handle *, const Mut2Args &, int);
// the persistent segment kernel lives in translation units of its own (inst3.hip, one per n_para and proposal kind) with their own flags
// (Makefile SEGFLAGS / SEGFLAGS_MIX).  History of the α = 1 variant at n_para 10: default flags 256 VGPRs / 216 B of scratch per lane, 36.4 µs per
// stage; hoisted computations sunk back into the stage loop (-sink-insts-to-avoid-spills) 72 B, 35.6 µs; no machine LICM instead 229 VGPRs,
// no spill, 35.2 µs (both together: 36.6).  The mixture variant needs both (251 VGPRs, no spill, 42.5 µs; LICM off alone: 77 spilled
// registers, 45.3 µs).  K1 / K2 and the generic mutation kernels lose 1-2 % to the sinking and are indifferent to the LICM switch.
#define SMCMI_LAUNCH3_INSTANCES(X, D) X template int launch_k3_seg<D, true, false>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, false, false>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, true, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, false, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, true, false, 2>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, true, true, 2>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, true, false, 1, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, false, false, 1, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, true, true, 1, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int); \
                                      X template int launch_k3_seg<D, false, true, 1, true>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int);
#define SMCMI_LAUNCH3_ONE(D, A, R, C, S) template int launch_k3_seg<D, A, R, C, S>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int);
#define SMCMI_LAUNCH2B_INSTANCES(X, D) X template void launch_k2b_mutate<D>(smcmi_handle *, const Mut2Args &, const Beg2Args &, int, bool);
#define SMCMI_LAUNCH_ALL_D(M, X)                                                                                                          \
    M(X, 1) M(X, 2) M(X, 3) M(X, 4) M(X, 5) M(X, 6) M(X, 7) M(X, 8) M(X, 9) M(X, 10) M(X, 11) M(X, 12) M(X, 13) M(X, 14) M(X, 15) M(X, 16)
// (the large-shard mutation kernel and the segment kernel exist for n_para <= 10: beyond that the launchers are empty and instantiated where they are called)
#define SMCMI_LAUNCH_B_D(M, X) M(X, 1) M(X, 2) M(X, 3) M(X, 4) M(X, 5) M(X, 6) M(X, 7) M(X, 8) M(X, 9) M(X, 10)
#if defined(SMCMI_INST_D)
SMCMI_LAUNCH2_INSTANCES(, SMCMI_INST_D)
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH3_INSTANCES, extern)
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH2B_INSTANCES, extern)
#elif defined(SMCMI_INST3_D)
SMCMI_LAUNCH_ALL_D(SMCMI_LAUNCH2_INSTANCES, extern)
#ifdef SMCMI_K3_RUN
template int launch_k3_seg_run<SMCMI_INST3_D>(smcmi_handle *, const Mut2Args &, const Seg3Args &, int);
#else
SMCMI_LAUNCH3_ONE(SMCMI_INST3_D, (SMCMI_INST3_A != 0), (SMCMI_INST3_R != 0), SMCMI_INST3_C, (SMCMI_INST3_S != 0))
#endif
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH2B_INSTANCES, extern)
#elif defined(SMCMI_INST2B_D)
SMCMI_LAUNCH_ALL_D(SMCMI_LAUNCH2_INSTANCES, extern)
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH3_INSTANCES, extern)
SMCMI_LAUNCH2B_INSTANCES(, SMCMI_INST2B_D)
#else
SMCMI_LAUNCH_ALL_D(SMCMI_LAUNCH2_INSTANCES, extern)
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH3_INSTANCES, extern)
SMCMI_LAUNCH_B_D(SMCMI_LAUNCH2B_INSTANCES, extern)
#endif
