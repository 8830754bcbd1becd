// runsetup.hpp - how a run starts and ends, once: argument checks, schedule, RunParams, the fresh or continued DevState, the stage-1 records
// and history columns, the result fill, and the profile events with their overhead calibration.  What the four drivers share around their
// stage loops (run1_impl, run_callback, run_sharded_impl, run2_impl); what they decide between stages is in stagepolicy.hpp.  Included by
// smcmi.hip in front of run1.hpp.
#pragma once
#include "stagepolicy.hpp"

static int check_run_config(const smcmi_handle *h, const smcmi_run_config *rc) {
    const int nf = h->h_model.n_free;
    if (rc->n_blocks < 1 || rc->n_blocks > nf || ((nf + rc->n_blocks - 1) / rc->n_blocks) * (rc->n_blocks - 1) >= nf)
        return set_err(SMCMI_ERR_ARG, "n_blocks incompatible with the number of free parameters");
    if (rc->n_phi < 2 || rc->n_mh_steps < 1) return set_err(SMCMI_ERR_ARG, "bad n_phi / n_mh_steps");
    if (rc->resampling_method != SMCMI_RESAMPLE_SYSTEMATIC && rc->resampling_method != SMCMI_RESAMPLE_MULTINOMIAL)
        return set_err(SMCMI_ERR_ARG, "Invalid resampler in SMC. Options are systematic or multinomial");
    if (rc->use_fixed_schedule && rc->n_phi > h->cfg.max_stages) return set_err(SMCMI_ERR_CAPACITY, "max_stages < n_phi");
    return 0;
}
// proposed fixed schedule ((k-1)/(n_Φ-1))^λ, smc_main.jl:348-352
static std::vector<double> make_schedule(const smcmi_run_config *rc) {
    std::vector<double> sched(rc->n_phi);
    for (int k = 0; k < rc->n_phi; ++k) sched[k] = pow((double)k / (double)(rc->n_phi - 1), rc->lambda);
    return sched;
}
// (shift_lag stays 0: run2_impl, whose stages know the lagged energy shift, sets it on the result)
static RunParams make_run_params(const smcmi_handle *h, const smcmi_run_config *rc) {
    RunParams rp{};
    rp.n_parts = h->cfg.n_parts; rp.n_blocks = rc->n_blocks; rp.n_mh_steps = rc->n_mh_steps; rp.n_phi = rc->n_phi;
    rp.resampling_method = rc->resampling_method; rp.use_fixed_schedule = rc->use_fixed_schedule;
    rp.threshold = rc->threshold_ratio * (double)h->cfg.n_parts;
    rp.alpha = rc->alpha; rp.target = rc->target; rp.tempering_target = rc->tempering_target;
    rp.pw = rc->tempered_update_prior_weight; rp.logp_old = rc->log_prob_old_data;
    rp.max_stages = h->cfg.max_stages; rp.store_history = h->cfg.store_history;
    rp.stall_on_exhaust = 1;
    rp.phi_rtol = rc->phi_rtol > 0.0 ? rc->phi_rtol : (rc->phi_rtol < 0.0 ? 0.0 : DEFAULT_PHI_RTOL);
    rp.stop_stage = rc->stop_after_stage > 0 ? rc->stop_after_stage : 0;
    return rp;
}
// ESS of the cloud a run starts from (tempered update: the old cloud's, initialization.jl:199-200)
static double initial_ess(const smcmi_handle *h, const smcmi_run_config *rc) { return rc->initial_ess > 0.0 ? rc->initial_ess : (double)h->cfg.n_parts; }

// The loop state a run starts from, in h->h_st and on the device.  continue_run (continue_intermediate, smc_main.jl:334-335,355-361) keeps the
// loop scalars, records and history the handle holds (left by a paused run, or put there by smcmi_set_loop_state / _set_stage_records /
// _set_history); the caller has pulled them.  keep_e_seen: engines 2 / 3 go on from the largest energy their last begin saw (stage2.hpp
// Begin2::e_seen); the other drivers keep none, and a later continuation on engines 2 / 3 takes the cloud's own maximum.
// push = false: the state stays in the handle - the caller's prologue launch puts it on the device (run2.hpp run_prologue: a fresh run).
static int start_state(smcmi_handle *h, const smcmi_run_config *rc, const RunParams &rp, bool keep_e_seen, bool push = true) {
    DevState &s = h->h_st;
    if (rc->continue_run) {
        if (s.stage < 1 || s.stage >= h->cfg.max_stages) return set_err(SMCMI_ERR_STATE, "no loop state to continue from");
        if (s.phi_n >= 1.0) return set_err(SMCMI_ERR_STATE, "the run to continue has already reached phi = 1");
        s.rp = rp; s.done = 0; s.err = 0; s.skip_fold = 1; s.do_resample = 0;
        if (!keep_e_seen) s.e_seen = __builtin_nan("");
    } else {
        const int cur = s.cur;
        memset(&s, 0, sizeof(DevState));
        s.e_seen = __builtin_nan("");
        s.rp = rp; s.cur = cur;
        s.stage = 1; s.j = 2;                                   // i = 1, j = 2 (smc_main.jl:198-199)
        s.c = rc->c; s.accept = rc->target;                     // initialize_cloud_settings!, initialization.jl:196-211
        s.ess_prev = initial_ess(h, rc);
    }
    return push ? push_state(h) : 0;
}
// A fresh run's stage-1 records, resample flags and history columns (w[:,1] = 0, W[:,1] = weights; smc_main.jl:363-366).  on_import:
// run2_impl's variant - the four records ride on its import kernel (k2_state) and the column is copied by a kernel: no host copies, no
// sync (a measured saving); everything here is in stream order.
static int first_records(smcmi_handle *h, const smcmi_run_config *rc, bool on_import = false) {
    const double v0[4] = {0.0, initial_ess(h, rc), rc->c, rc->target};
    double *const dst[4] = {h->rec.phi, h->rec.ess, h->rec.c, h->rec.accept};
    for (int k = 0; k < 4 && !on_import; ++k) HIP_TRY(hipMemcpyAsync(dst[k], &v0[k], sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->rec.resampled, 0, sizeof(int) * h->cfg.max_stages, h->stream));
    if (h->cfg.store_history) {
        const double *W = h->cl.buf[h->h_st.cur] + (long long)(h->R - 1) * h->n;
        HIP_TRY(hipMemsetAsync(h->d_hist_w, 0, sizeof(double) * h->n, h->stream));
        if (on_import) launch_copy_f64(h->d_hist_W, W, h->n, h->stream);
        else HIP_TRY(hipMemcpyAsync(h->d_hist_W, W, sizeof(double) * h->n, hipMemcpyDeviceToDevice, h->stream));
    }
    if (!on_import) HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

typedef std::chrono::steady_clock::time_point run_clock_t;
static void finish_result(smcmi_result *res, const DevState &s, run_clock_t t0, run_clock_t t1) {
    res->n_stages = s.stage; res->resamples = s.resamples; res->logmdd = s.logz; res->c = s.c; res->accept = s.accept;
    res->seconds = std::chrono::duration<double>(t1 - t0).count();
    res->solver_passes = s.solver_passes;
    res->paused = (s.done == 5) ? 1 : 0;
}
// what the closed loop state says of the run (engine 1's drivers; run2_impl reads its own Ctl2)
static int finish_error(const DevState &s) {
    if (s.err) return err_from_state(s.err);
    if (!s.done) return set_err(SMCMI_ERR_CAPACITY, "max_stages exceeded before the tempering schedule reached 1");
    return 0;
}
static int bracket_error() { return set_err(SMCMI_ERR_BRACKET, "adaptive tempering solver: the search for phi_n does not terminate (the ESS objective is not a number?)"); }
// An event pair brackets [previous kernel done -> this kernel done]: dispatch of the kernel included.  Calibrate that fixed part with pairs
// around an empty kernel of the mutation kernel's grid (its predecessor of comparable size) and subtract it, so the figure is the kernel's
// own duration (what rocprofv3 --kernel-trace reports).
static double event_overhead_ms(smcmi_handle *h) {
    devmem::Handles made;
    hipEvent_t c0 = nullptr, c1 = nullptr;
    if (made.event(&c0) != hipSuccess || made.event(&c1) != hipSuccess) return 0.0;
    double acc_ms = 0.0;
    int got = 0;
    for (int r = 0; r < 64; ++r) {
        k_fill<<<(unsigned)((h->n + 255) / 256), 256, 0, h->stream>>>(nullptr, 0, 0.0);
        hipEventRecord(c0, h->stream);
        k_fill<<<(unsigned)((h->n + 255) / 256), 256, 0, h->stream>>>(nullptr, 0, 0.0);
        hipEventRecord(c1, h->stream);
        hipStreamSynchronize(h->stream);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c0, c1) == hipSuccess) { acc_ms += ms; ++got; }
    }
    // an empty kernel of this grid itself lasts ~2.5 µs in a rocprofv3 kernel trace (wave launch + drain): leave that in
    return got ? std::max(0.0, acc_ms / got - 0.0025) : 0.0;
}
// Profile mode (use_graph == 2: direct launches with HIP events around the mutation kernel): the event pairs of a run, each tagged with the
// stage or iteration it belongs to; destroyed on every return.
struct MutationEvents {
    bool on;
    explicit MutationEvents(bool profile) : on(profile) {}
    // a pair for a launch of stage / iteration `tag` (off, or no event to be had: two nulls - the launch goes untimed)
    void pair(int tag, hipEvent_t *e0, hipEvent_t *e1) {
        *e0 = *e1 = nullptr;
        if (!on) return;
        hipEvent_t a = nullptr, b = nullptr;
        if (made_.event(&a) != hipSuccess || made_.event(&b) != hipSuccess) return;
        pairs_.push_back({a, b, tag});
        *e0 = a; *e1 = b;
    }
    // a stage stalled: its mutation launch and everything behind it were no-ops
    void void_from(int tag) { for (Pair &p : pairs_) if (p.tag >= tag) p.tag = -1; }
    // kernel_ms_mutate / n_mutate_launches from the pairs that stand with a tag below `bound` (the stages the run completed), each minus the
    // calibrated overhead
    int tally(smcmi_handle *h, int bound, smcmi_result *res) const {
        res->kernel_ms_mutate = 0.0; res->n_mutate_launches = 0;
        if (pairs_.empty()) return 0;
        HIP_TRY(hipSetDevice(h->cfg.device));
        const double over = event_overhead_ms(h);
        for (const Pair &p : pairs_) {
            float ms = 0.f;
            if (p.tag >= 0 && p.tag < bound && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) { res->kernel_ms_mutate += std::max(0.0, (double)ms - over); res->n_mutate_launches += 1; }
        }
        return 0;
    }
private:
    struct Pair { hipEvent_t e0, e1; int tag; };
    devmem::Handles made_;
    std::vector<Pair> pairs_;
};
// the stalls a run's book counted (stagepolicy.hpp); StallReport: they reach the result on every return, an early one included
static void put_stalls(smcmi_result *res, const stagepolicy::StallBook &b) { res->solver_stalls = b.solver_stalls; res->select_stalls = b.select_stalls; res->spec_stalls = b.spec_stalls; }
struct StallReport { smcmi_result *res; const stagepolicy::StallBook &book; ~StallReport() { put_stalls(res, book); } };
