// run1.hpp - engine 1's driver: the stage as a fixed kernel sequence (enqueue_stage) and run1_impl, the run of one handle on it (smcmi_run,
// the entry point every one-handle run comes through, is in smcmi.hip behind all drivers).  Included by smcmi.hip behind the stage primitives
// it enqueues.
#pragma once

// ------------------------------------------------------------------------------------------------ whole loop
// One stage = a fixed kernel sequence (no host decision inside): see the header of kernels.hpp.
struct StageRun { bool adaptive; int method, n_blocks; double alpha; int acc_nb; };      // what all stages of a run share
// what varies from one enqueue to the next; every caller sets only what it means
struct StageReq {
    int passes = 0;             // solver passes to enqueue
    // p0 > 0 resumes a stage whose solver ran out of passes after p0 of them (st->done == 2 stall, see solver_prologue): the
    // search continues with passes p0 .. p0 + passes - 1 exactly as if the original list had been that much longer.
    int p0 = 0;
    // the host expects no resampling in this stage: k_post_correct and k_resample_gather are not launched, the moments
    // kernel takes the decision itself and stalls the run (done = 3) if selection is needed after all.
    bool no_select = false;
    bool tail_only = false;     // resume such a stage from k_post_correct on (the correction is already done)
    bool spec = false;          // predict -> correct -> verify (kernels.hpp k_stage_begin): no certificate pass is enqueued at all - 4 launches
    bool skip_begin = false;    // resume of such a stage through the certificate path: its begin has run
    bool host_mut = false;      // the mutation runs through the host callback (callback.hpp): none is launched
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // profile mode: recorded around the mutation launch
};
// What resumes stage st, stalled with DevState::done = 2 (its solver ran out of passes: the same search continues with more), 3 (enqueued
// without selection kernels it must resample after all: nothing past its correction has run - the rest of it through the full path) or 4
// (enqueued without a certificate pass, its prediction did not verify: nothing is committed, W̃ went to scratch - the caller re-arms the solver
// and the stage runs through the certificate path); booked in `book`.  false: the search of a done = 2 stage does not terminate.
static bool resume_request(stagepolicy::StallBook &book, int done, int st, StageReq *q) {
    if (done == 4) { q->passes = book.first_passes; q->skip_begin = true; book.spec_stall(st); }
    else if (done == 2) {
        const auto more = book.solver_stall(st);
        if (!more.ok) return false;
        q->p0 = more.p0; q->passes = more.p1 - more.p0;
    } else { q->p0 = book.had(st); q->tail_only = true; book.select_stall(); }
    return true;
}
static void enqueue_stage(smcmi_handle *h, const StageRun &run, const StageReq &q) {
    const bool adaptive = run.adaptive, no_select = q.no_select, tail_only = q.tail_only, host_mut = q.host_mut;
    const int p0 = q.p0, acc_nb = run.acc_nb;
    const long long n = h->n;
    hipStream_t s = h->stream;
    const int P = (adaptive && !q.spec) ? p0 + q.passes : 0;
    h->run_adaptive = adaptive;
    const int fin_slot = P == 0 ? 0 : (P & 1);
    // no selection expected and the register kernels apply: the correction pass gathers the moments too, k_prepare_mutation
    // takes the post-correction decision, the mutation kernel normalises the weights (5 launches per stage)
    const bool cm = no_select && !tail_only && can_fuse_cm(h);
    h->fused_cm = cm;
    h->spec_stage = q.spec && cm;
    if (!tail_only) {
    if (p0 == 0 && !q.skip_begin) {
        // (a host-callback mutation without cb_energy - sharded closure runs, fixed schedules - leaves neither energy sums nor energy maxima:
        // plain schedule walk, unshifted weights)
        const bool hm_plain = host_mut && !h->cb_energy;
        const double *es = (adaptive && !sw().no_predictor && !hm_plain) ? h->d_esum_part : nullptr;
        int es_nb = acc_nb, em_nb = acc_nb;
        const double *em = hm_plain ? nullptr : h->d_emax_part;
        // tens of thousands of rows are not for one block: blocks 1..ESUM_RED_ROWS of the same launch total a chunk each (k_stage_begin)
        PrepRed rr{};
        unsigned grid = 1;
        // (reducer blocks: ~96 rows each - 40 blocks at N = 1e6, the full 128 from 3e6 on; block 0 adds one group row per reducer)
        if (es && acc_nb > 2048 && em) { rr.rows = h->d_esum_red; rr.tick = h->d_prep_tick + 1; grid = 1u + (unsigned)std::min(ESUM_RED_ROWS, std::max(16, acc_nb / 96)); }
        else if (es && acc_nb > 2048) {
            k_reduce_rows<<<ESUM_RED_ROWS, TB, 0, s>>>(h->d_esum_part, acc_nb, ES, h->d_esum_red, nullptr, nullptr);
            es = h->d_esum_red; es_nb = ESUM_RED_ROWS;
        }
        k_stage_begin<<<grid, BT, 0, s>>>(h->d_st, h->d_sched, h->d_acc_part, es ? es_nb : acc_nb, h->rec, es, h->d_prof ? h->d_prof + 9 : nullptr,
                                          h->spec_stage ? 1 : 0, em, em_nb, rr, h->note_on ? h->d_note : nullptr);
    }
    if (adaptive && !h->spec_stage) enqueue_solver(h, P, p0);
    if (cm) launch_correct_moments(h, P);
    else k_pass<1, true><<<h->nb_e, TB, 0, s>>>(h->cl, h->d_st, h->d_sched, h->d_part_ess[(P + 1) & 1], h->d_part_fin, h->nb_e, P, h->d_hist_w, n);
    }
    int nbm = 0;
    if (cm) {
        launch_prepare_in_run(h, h->d_part_cm, h->nb_e, 3, fin_slot);
        if (q.ev0) hipEventRecord(q.ev0, s);
        launch_mutate(h, run.n_blocks, 0, run.alpha);
        if (q.ev1) hipEventRecord(q.ev1, s);
        return;
    }
    if (no_select && !tail_only && can_fuse_post(h)) nbm = launch_moments(h, h->d_hist_W, 0, fin_slot);
    else {
        k_post_correct<<<h->nb_e, TB, 0, s>>>(h->d_st, h->d_part_fin, h->nb_e, nullptr, h->rec, fin_slot, h->cl, h->d_cum);
        k_resample_gather<<<(unsigned)std::min<long long>((n + TB - 1) / TB, 4 * h->noop_grid), TB, 0, s>>>(h->cl, h->d_st, h->d_cum, n, 0, h->cfg.n_parts, run.method,
                                                                     h->cfg.seed, 0u, nullptr, h->d_anc, nullptr, 0);
        nbm = launch_moments(h, h->d_hist_W, 0);
    }
    launch_prepare_in_run(h, h->d_part_mom, nbm, 1);
    if (host_mut) return;
    if (q.ev0) hipEventRecord(q.ev0, s);
    launch_mutate(h, run.n_blocks, 0, run.alpha);
    if (q.ev1) hipEventRecord(q.ev1, s);
}

// a (host closure, device family) pair in a tempered update: the callback path would score the old likelihood as 0, the device path
// would call a device family that does not exist - refuse instead of sampling the wrong posterior
static int check_lik_pair(const smcmi_handle *h) {
    const int f1 = h->h_model.lik[1].family;
    const bool old_dev = f1 != SMCMI_LIK_NONE && f1 != SMCMI_LIK_HOST_CALLBACK, old_cb = closure_lik(h, 1);
    if ((closure_lik(h) && old_dev) || (!closure_lik(h) && old_cb))
        return set_err(SMCMI_ERR_UNSUPPORTED, "the new and the old likelihood must both be device families or both host callbacks");
    // (a host callback next to a device callback: one mutation would need both paths)
    if ((h->cb[0] && device_lik(h, 1)) || (device_lik(h, 0) && h->cb[1]))
        return set_err(SMCMI_ERR_STATE, "the new and the old likelihood must both be host callbacks or both device callbacks / programs");
    return 0;
}
// engine 1's run of one handle (smcmi_run sends it the runs that are neither closure runs nor engine 2's)
static int run1_impl(smcmi_handle *h, const smcmi_run_config *rc, smcmi_result *res) {
    if (int e = check_run_config(h, rc)) return e;
    const bool adaptive = !rc->use_fixed_schedule;
    if (pull_state(h)) return SMCMI_ERR_HIP;
    const std::vector<double> sched = make_schedule(rc);
    if (upload_sched(h, sched.data(), rc->n_phi)) return SMCMI_ERR_HIP;
    DevState &s = h->h_st;
    const RunParams rp = make_run_params(h, rc);
    const bool cont = rc->continue_run != 0;
    if (int e = start_state(h, rc, rp, false)) return e;
    const int base = cont ? s.stage - 1 : 0;                // stages completed before this call
    if (int e = center_single(h, !cont)) return e;           // the chain's first moments are centred on the cloud (kernels.hpp k_center_probe)
    // the arrival counters of the two-level totals (PrepRed) start every run at zero: a launch whose wait timed out (SMCMI_ERR_TIMEOUT,
    // the run is void) may have left late arrivals behind - in stream order they precede this fill
    HIP_TRY(hipMemsetAsync(h->d_prep_tick, 0, 8 * sizeof(double), h->stream));
    if (!cont) { if (int e = first_records(h, rc)) return e; }
    if (sw().prof2.set && !h->d_prof) { if (dmalloc(h->mem, &h->d_prof, 32)) return SMCMI_ERR_HIP; }
    if (int e = ensure_zbuf(h, rc->n_mh_steps, rc->n_blocks)) return e;
    const int first_passes = std::max(rc->solver_passes >= 1 ? rc->solver_passes : DEFAULT_SOLVER_PASSES, FIRST_SOLVER_PASSES);
    const int sync_every = rc->sync_every > 0 ? rc->sync_every : 32;     // (16 until round 4: 36.75 vs 36.45 ms per run at N = 1e6)
    const int acc_nb = mut_blocks(h);
    // largest energy of the initial cloud, in the layout the mutation epilogue uses afterwards (stage 1's energy shift)
    k_energy_max<<<acc_nb, TB, 0, h->stream>>>(h->cl, h->d_st, h->d_emax_part);
    const StageRun run{adaptive, rc->resampling_method, rc->n_blocks, rc->alpha, acc_nb};
    MutationEvents evs(rc->use_graph == 2);     // tagged with the iteration of the launch
    // The selection kernels go only where a resample is forecast (stagepolicy.hpp Forecast; k_moments_reg checks the expectation).
    // SMCMI_NO_SELECT_PREDICT=1 (development) keeps the full list everywhere, =2 deliberately predicts "never" to exercise the stall path.
    const int sel_mode = sw().no_select_predict;
    // (Fixed schedules: extrapolating the ESS decay was tried and dropped - CAPM-like posteriors collapse within two or three
    // stages, 19 of 20 resamples stalled, and the per-batch sync it needs makes short stages host-bound.)
    const bool predict_select = adaptive && can_fuse_post(h) && sel_mode != 1;
    // Fixed schedules: the host cannot foresee which stages resample, so EVERY stage is enqueued without the selection kernels
    // (begin, correction + moments, prepare, mutation: four launches instead of seven) and a stage that resamples after all stalls
    // (done = 3) and is resumed through the full path, exactly as a mispredicted stage of an adaptive run.  What made this a loss
    // before was the drain - the whole schedule is enqueued at once, a stall left hundreds of idle launches behind it - and a sync
    // per batch makes short stages host-bound.  Instead the host stays `run_ahead` stages in front of the device WITHOUT a sync:
    // k_stage_begin posts its stage index and the stalling k_prepare_mutation a flag into host-mapped words (handle.hpp h_note)
    // which the enqueue loop polls; a drained stream (an error, a pause, phi = 1) also ends the wait.
    const int run_ahead = 1;      // (config 4: 30.6 ms at 1, 30.8 at 2, 31.1 at 4 - fewer idle launches behind a stall; measured in round 4, the switch retired in round 6)
    bool fixed_ns = !adaptive && can_fuse_cm(h) && sel_mode != 1 && sw().fixed_no_select != 0;        // (development: SMCMI_FIXED_NO_SELECT=0 = the seven-launch stage)
    if (fixed_ns && !h->h_note) {
        int *hp = nullptr, *dp = nullptr;
        if (h->mem.alloc(&hp, 16, devmem::Kind::Mapped, &dp) == hipSuccess) {
            h->h_note = hp; h->d_note = dp;
        } else {
            (void)hipGetLastError();
            fixed_ns = false;
        }
    }
    struct NoteGuard { smcmi_handle *h; ~NoteGuard() { h->note_on = false; } } note_guard{h};
    h->note_on = fixed_ns;
    if (fixed_ns) { h->h_note[0] = s.stage; h->h_note[1] = 0; }
    // (with a prior weight the correction's incremental weight differs from the solver's objective - quirk Q4 - so the ESS it
    // produces cannot verify a predicted root: those runs keep the certificate pass)
    const bool spec_ok = predict_select && can_fuse_cm(h) && !sw().no_predictor &&
                         rc->tempered_update_prior_weight == 0.0 && rp.phi_rtol > 0.0;
    stagepolicy::Forecast forecast(rc->tempering_target, (double)h->cfg.n_parts, rp.threshold, cont ? s.ess_prev : initial_ess(h, rc), cont ? s.resampled_last : 0);
    stagepolicy::StallBook book(first_passes, stagepolicy::starting_passes(rc->solver_passes, DEFAULT_SOLVER_PASSES, rc->tempering_target), 8, base, spec_ok);
    stagepolicy::StagesLeft left;
    const auto t0 = std::chrono::steady_clock::now();
    int launched = 0, done = 0;
    const StallReport stall_report{res, book};
    const int max_iter = (adaptive ? h->cfg.max_stages : rc->n_phi - 1) - base;
    while (launched < max_iter && !done) {
        int batch = adaptive ? left.batch(sync_every, max_iter - launched) : max_iter - launched;
        for (int b = 0; b < batch; ++b) {
            bool no_select = false;
            if (fixed_ns) {
                // iteration `launched` begins stage base + launched + 2: wait until the device has begun the stage run_ahead before it
                const int need = base + launched + 2 - run_ahead;
                bool leave = false;
                while (h->h_note[0] < need) {
                    if (h->h_note[1] != 0) break;
                    if (hipStreamQuery(h->stream) != hipErrorNotReady) { leave = h->h_note[0] < need; break; }   // nothing left in flight: look at the state
                }
                if (h->h_note[1] != 0) {
                    // Stage h_note[0] resamples after all (the begins behind it returned at once and posted nothing).  No sync: clear
                    // the stall behind the idle launches already in the stream, run the rest of that stage through the full path
                    // (tail_only: the correction is done) and go on enqueuing from the stage after it.
                    const int st_i = h->h_note[0];
                    h->h_note[1] = 0;
                    HIP_TRY(hipMemsetAsync(&h->d_st->done, 0, sizeof(int), h->stream));
                    StageReq q; q.tail_only = true;
                    evs.void_from(st_i - 2 - base);
                    evs.pair(st_i - 2 - base, &q.ev0, &q.ev1);
                    enqueue_stage(h, run, q);
                    book.select_stall();
                    launched = st_i - 1 - base;
                    batch = max_iter - launched; b = -1;
                    continue;
                }
                if (leave) break;
                no_select = true;
            }
            if (predict_select) no_select = !forecast.step() || sel_mode == 2;
            StageReq q;
            q.passes = book.fresh(launched);
            q.no_select = no_select;
            q.spec = book.spec_on && no_select && launched >= 2;
            evs.pair(launched, &q.ev0, &q.ev1);
            enqueue_stage(h, run, q);
            ++launched;
        }
        // one copy per sync: the loop scalars from `stage` to `ess_prev` are contiguous in DevState (64 bytes) - the done flag, the
        // last stage's resample decision and its ESS used to be three copies (each a ~2.5 µs copy kernel plus a host round trip)
        DevState head;
        constexpr size_t head_off = offsetof(DevState, stage), head_len = offsetof(DevState, ess) - offsetof(DevState, stage);
        HIP_TRY(hipMemcpyAsync((char *)&head + head_off, (const char *)h->d_st + head_off, head_len, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        done = head.done;
        bool resumed = false;
        while (done == 2 || done == 3 || done == 4) {
            resumed = true;
            if (pull_state(h)) return SMCMI_ERR_HIP;
            if (fixed_ns) h->h_note[1] = 0;               // (the stream is drained: no post is in flight)
            const int st_i = s.stage;
            const int zero = 0;
            HIP_TRY(hipMemcpyAsync(&h->d_st->done, &zero, sizeof(int), hipMemcpyHostToDevice, h->stream));
            StageReq q;
            evs.void_from(st_i - 2 - base);
            evs.pair(st_i - 2 - base, &q.ev0, &q.ev1);
            if (done == 4) k_solver_rearm<<<1, 64, 0, h->stream>>>(h->d_st, h->d_sched);       // (with the plain schedule walk)
            if (!resume_request(book, done, st_i, &q)) return bracket_error();
            enqueue_stage(h, run, q);                      // ... and go on from the stage after it
            launched = st_i - 1 - base;
            HIP_TRY(hipMemcpyAsync(&done, &h->d_st->done, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        if (resumed) {               // a resumed stage ran after the copy above
            HIP_TRY(hipMemcpyAsync((char *)&head + head_off, (const char *)h->d_st + head_off, head_len, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        // The stage that reaches ϕ = 1 raises `done` only through the NEXT stage's k_stage_begin.  When it was the last one of its
        // batch (config 2: 256 stages = 16 batches of 16) nothing has raised it yet - do not enqueue a whole batch of no-ops (64
        // launches and a sync) to find out: the closing k_stage_begin below does the same bookkeeping.
        if (!done && head.phi_n >= 1.0) break;
        left.observe(head.phi_n, head.phi_n - head.phi_prev);
        if (predict_select) {
            s.resampled_last = head.do_resample;       // did the last stage resample
            s.ess_prev = head.ess_prev;
            forecast.anchor(s.ess_prev, s.resampled_last);
        }
        if (sw().trace) {   // development only
            static long long last_passes = 0;
            if (pull_state(h)) return SMCMI_ERR_HIP;
            fprintf(stderr, "[smcmi] stage %d phi %.12e dphi %.6e pred %.6e relerr %.2e passes %lld ess %.1f rs %d\n", s.stage, s.phi_n,
                    s.phi_n - s.phi_prev, s.pred_delta, (s.pred_delta - (s.phi_n - s.phi_prev)) / (s.phi_n - s.phi_prev),
                    s.solver_passes - last_passes, s.ess, s.do_resample);
            last_passes = s.solver_passes;
            if (h->d_prof) {
                long long pr[16];
                hipMemcpy(pr, h->d_prof, sizeof(pr), hipMemcpyDeviceToHost);
                long long pq[32];
                hipMemcpy(pq, h->d_prof, sizeof(pq), hipMemcpyDeviceToHost);
                fprintf(stderr, "[smcmi]    prepare phase ticks: %lld %lld %lld %lld %lld %lld\n", pq[26] - pq[25], pq[27] - pq[26], pq[28] - pq[27], pq[29] - pq[28], pq[30] - pq[29], pq[31] - pq[30]);
                fprintf(stderr, "[smcmi]    mutate phase ticks (block 0):");
                for (int q = 1; q <= 8; ++q) fprintf(stderr, " %lld", pq[q] - pq[q - 1]);
                fprintf(stderr, "  total %lld\n", pq[8] - pq[0]);
                fprintf(stderr, "[smcmi]    begin phase ticks: %lld %lld %lld %lld %lld\n", pr[10] - pr[9], pr[11] - pr[10], pr[12] - pr[11], pr[14] - pr[12], 0ll);
            }
            for (int q = 0; q < 2; ++q)
                fprintf(stderr, "[smcmi]    sol[%d] mode %d nv %d lo-phi %.3e hi-phi %.3e glo %.3e ghi %.3e\n", q, s.sol[q].mode, s.sol[q].n_valid,
                        s.sol[q].lo - s.phi_n, s.sol[q].hi - s.phi_n, s.sol[q].glo, s.sol[q].ghi);
        }
    }
    // fold the last mutation's acceptance rate and close the run
    k_stage_begin<<<1, BT, 0, h->stream>>>(h->d_st, h->d_sched, h->d_acc_part, acc_nb, h->rec);
    if (pull_state(h)) return SMCMI_ERR_HIP;
    const auto t1 = std::chrono::steady_clock::now();
    if (int e = evs.tally(h, s.stage - 1 - base, res)) return e;
    finish_result(res, s, t0, t1);
    h->last_n_stages = s.stage;
    if (s.err == SMCMI_ERR_NAN_ESS) return nan_ess_error(h, h->spec_stage ? h->d_wt : h->cl.buf[0] + (long long)(h->R - 1) * h->n);
    return finish_error(s);
}

