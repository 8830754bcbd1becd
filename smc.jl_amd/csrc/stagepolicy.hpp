// stagepolicy.hpp - what the host decides between the stages of a run, once: which stage is expected to resample, what a stalled stage is
// resumed with and what repeated stalls change, and how many stages go out before the next sync.  No HIP in here, no handle, no environment:
// run1_impl, run2_impl, run_sharded_impl and run_callback construct these from their run's numbers and enqueue what they answer;
// tests/policy_check.cpp drives them with plain numbers.
#pragma once
#include <algorithm>

namespace stagepolicy {

// Resampling is predictable on an adaptive schedule: every stage ends at ESS = tempering target x the previous ESS, or x N after a resample
// (helpers.jl:14-20).  So the host enqueues the selection kernels only where it expects a resample; the device checks the expectation and
// stalls the run if it was wrong.  The margin: a wrong "resample" guess only costs two idle launches.
struct Forecast {
    double target, n_parts, threshold;      // tempering target, particles of the whole cloud, ESS below which a stage resamples
    double pred_ess;                        // ESS after the last stage forecast (or anchored)
    int pred_rl;                            // ... and whether it resampled (resampled_last_period)
    Forecast(double tempering_target, double n, double thr, double ess, int resampled)
        : target(tempering_target), n_parts(n), threshold(thr), pred_ess(ess), pred_rl(resampled) {}
    // will the next stage resample?
    bool step() {
        const double ess_bar = target * (pred_rl ? n_parts : pred_ess);
        const bool rs = ess_bar < threshold * (1.0 + 1e-6);
        pred_ess = ess_bar; pred_rl = rs ? 1 : 0;
        return rs;
    }
    // every sync re-anchors the expectation on the device's ESS and flag
    void anchor(double ess, int resampled) { pred_ess = ess; pred_rl = resampled; }
};

// A bracketing search halves its interval at least every pass: 1100 passes exhaust the exponent range of a double - whatever keeps a stage
// asking for more is not a search any more, and the host must not feed it for ever.
constexpr int MAX_SEARCH_PASSES = 1200;

// The stalls of a run.  A stage (counted as the device counts them; `base` stages were complete before this call, so a run's first two
// stages are base + 2 and base + 3) is enqueued with first_passes solver passes when it is one of the first two and with dyn_P otherwise.
struct StallBook {
    int first_passes, dyn_P;                // dyn_P: raised when stalls are frequent (poorly predictable models)
    int more, base;                         // passes a stage that ran out of them gets on top
    int stall_stage = -1, stall_p = 0;      // the stage resumed last with a certificate search, and the passes it has had so far
    // Predict-correct-verify pays only while predictions verify: three failures, each within four stages of the one before (heavy-tailed
    // energies, steps too long for the 16-term model), switch the rest of the run to the certificate path, where a miss costs an extra pass
    // instead of a host round trip.  Once off they stay off.
    bool spec_on;
    int spec_strikes = 0, last_spec_stall = -100, last_solver_stall = -100;
    int solver_stalls = 0, select_stalls = 0, spec_stalls = 0;      // what was reported (smcmi_result)
    StallBook(int first, int dyn, int more_passes, int stages_before, bool spec) : first_passes(first), dyn_P(dyn), more(more_passes), base(stages_before), spec_on(spec) {}

    // solver passes of a stage enqueued afresh, `launched` stages of this call in front of it
    int fresh(int launched) const { return launched < 2 ? first_passes : dyn_P; }
    // solver passes stage `st` has been given so far
    int had(int st) const { return st == stall_stage ? stall_p : fresh(st - base - 2); }
    // Stage st is (re)run through the certificate path from its first pass, with first_passes of them.
    void rerun(int st) { stall_stage = st; stall_p = first_passes; }
    // Stage st exhausted its solver passes: it and everything enqueued behind it did nothing.  The same search continues with passes
    // p0 .. p1 - 1; ok = false: it does not terminate (SMCMI_ERR_BRACKET), nothing is booked.  A stall flushes the rest of its batch and costs a
    // host round trip, an idle pass launch costs 3 µs: two stalls within four stages -> one more pass per stage from here on, up to 4.
    struct Passes { int p0, p1; bool ok; };
    Passes solver_stall(int st) {
        const int p0 = had(st);
        if (p0 > MAX_SEARCH_PASSES) return {p0, p0, false};
        stall_stage = st; stall_p = p0 + more;
        solver_stalls += 1;
        if (st - last_solver_stall <= 4 && dyn_P < 4) ++dyn_P;
        last_solver_stall = st;
        return {p0, p0 + more, true};
    }
    // Stage st, enqueued without a certificate pass, had no usable prediction or the ESS its correction produced did not verify it: nothing of
    // the stage is committed, the caller reruns it in full.
    void spec_stall(int st) {
        rerun(st);
        spec_stalls += 1;
        if (st - last_spec_stall <= 4) { if (++spec_strikes >= 2) spec_on = false; }
        else spec_strikes = 0;
        last_spec_stall = st;
    }
    // A stage enqueued without selection kernels has to resample after all (the caller runs the rest of it).
    void select_stall() { select_stalls += 1; }
};
// passes per stage a run starts with: what was asked for, else the driver's default - but larger steps (a tempering target below 0.95) leave
// the 8-term model good to ~1e-3 only: two passes are the norm there
inline int starting_passes(int asked, int dflt, double tempering_target) { return asked >= 1 ? asked : (tempering_target < 0.95 ? 2 : dflt); }

// Stages left at the last sync: (1 - ϕ_n) / (ϕ_n - ϕ_{n-1}), an over-estimate while the steps grow.  Near the end of the run the batch shrinks
// to what is left, so that few no-op stages trail the one that reaches ϕ = 1.
struct StagesLeft {
    static constexpr int UNKNOWN = 1 << 30;
    int est = UNKNOWN;
    void observe(double phi_n, double last_step) {
        if (!(last_step > 0.0 && phi_n < 1.0)) return;
        const double left = (1.0 - phi_n) / last_step;
        est = left < 1e6 ? (int)left + 1 : UNKNOWN;
    }
    // stages to enqueue before the next sync: at most sync_every, at most `room` (what the capacity leaves), at least 4 while room allows
    int batch(int sync_every, int room) const { return std::min(std::min(sync_every, std::max(est, 4)), room); }
};

}      // namespace stagepolicy
