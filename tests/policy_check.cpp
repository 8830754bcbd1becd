// policy_check.cpp - csrc/stagepolicy.hpp driven with plain numbers: the resample forecast, the stall book and the stages-left estimate, each
// against the rule as the three host drivers stated it before the header took it over.  No HIP.  Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../smc.jl_amd/csrc/stagepolicy.hpp"

using namespace stagepolicy;

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; }    \
    } while (0)

// predictions after spec stalls at these stages
static bool spec_on_after(std::initializer_list<int> stages) {
    StallBook b(6, 1, 8, 0, true);
    for (int st : stages) b.spec_stall(st);
    return b.spec_on;
}

int main() {
    // ---- forecast: target 0.95, N = 1000, threshold ratio 0.5, starting ESS 1000
    {
        Forecast f(0.95, 1000.0, 0.5 * 1000.0, 1000.0, 0);
        double ess = 1000.0;
        for (int k = 1; k <= 13; ++k) {
            CHECK(!f.step());                                  // 0.95^13 * 1000 = 513.3 is above 500.0005
            ess *= 0.95;
            CHECK(f.pred_ess == ess && f.pred_rl == 0);
        }
        CHECK(std::fabs(f.pred_ess - 513.3) < 0.05);
        CHECK(f.step());                                       // step 14: 487.7 < 500.0005
        CHECK(std::fabs(f.pred_ess - 487.7) < 0.05 && f.pred_rl == 1);
        CHECK(!f.step());                                      // step 15 restarts from N
        CHECK(f.pred_ess == 0.95 * 1000.0 && f.pred_rl == 0);
        f.anchor(600.0, 0);
        CHECK(!f.step());
        CHECK(f.pred_ess == 0.95 * 600.0);                     // 570
        f.anchor(600.0, 1);                                    // the device says the last stage resampled: from N again
        CHECK(!f.step() && f.pred_ess == 950.0);
        // inside the 1e-6 margin above the threshold: "resample"
        Forecast m(1.0, 1000.0, 500.0, 500.0002, 0);
        CHECK(m.step() && m.pred_rl == 1);
        Forecast e(1.0, 1000.0, 500.0, 500.0, 0);              // at the threshold itself
        CHECK(e.step());
        Forecast o(1.0, 1000.0, 500.0, 500.001, 0);            // outside the margin
        CHECK(!o.step());
    }
    // ---- had: first_passes within base + 3, dyn_P later, the accumulated passes of the stage that stalled last
    for (int base : {0, 7}) {
        StallBook b(6, 1, 8, base, true);
        CHECK(b.had(base + 2) == 6 && b.had(base + 3) == 6);
        CHECK(b.had(base + 4) == 1 && b.had(base + 40) == 1);
        CHECK(b.fresh(0) == 6 && b.fresh(1) == 6 && b.fresh(2) == 1);
        const StallBook::Passes p = b.solver_stall(base + 9);
        CHECK(p.ok && p.p0 == 1 && p.p1 == 9);
        CHECK(b.had(base + 9) == 9 && b.had(base + 10) == 1 && b.had(base + 8) == 1);
        b.spec_stall(base + 12);                               // rerun from the first pass with first_passes
        CHECK(b.had(base + 12) == 6 && b.had(base + 9) == 1);
        b.rerun(base + 20);
        CHECK(b.had(base + 20) == 6 && b.had(base + 12) == 1);
    }
    // ---- solver stalls
    {
        StallBook b(6, 1, 8, 0, false);
        b.solver_stall(10);
        CHECK(b.dyn_P == 1);                                   // the first stall of a run raises nothing
        b.solver_stall(14);                                    // 4 stages apart
        CHECK(b.dyn_P == 2);
        b.solver_stall(19);                                    // 5 apart
        CHECK(b.dyn_P == 2);
        b.solver_stall(20); b.solver_stall(21); b.solver_stall(22); b.solver_stall(23);
        CHECK(b.dyn_P == 4);                                   // never above 4
        CHECK(b.solver_stalls == 7 && b.select_stalls == 0 && b.spec_stalls == 0);
        StallBook hi(9, 7, 8, 0, false);                       // a run that asked for more than 4 keeps what it asked for
        hi.solver_stall(10); hi.solver_stall(11);
        CHECK(hi.dyn_P == 7);
    }
    for (int more : {8, 4}) {
        StallBook b(6, 2, more, 0, false);
        int want = 2, n = 0;
        for (;;) {
            const StallBook::Passes p = b.solver_stall(30);    // the same stage again and again: passes p0 .. p1 - 1, p0 growing by `more`
            if (!p.ok) { CHECK(p.p0 > 1200 && p.p0 == want); break; }
            CHECK(p.p0 == want && p.p1 == want + more && b.had(30) == want + more);
            want += more; ++n;
            if (n > 1000) { CHECK(!"the book never reports the bracket condition"); break; }
        }
        CHECK(want > 1200 && want - more <= 1200);             // the last range granted starts at or below 1200
        CHECK(b.solver_stalls == n);                           // the refusal is not counted
        CHECK(!b.solver_stall(30).ok && b.solver_stalls == n && b.had(30) == want);
    }
    // ---- spec stalls: a strike is a stall within four stages of the one before; the second strike switches predictions off
    // (three failures, each within four stages of the one before: `if (st - last <= 4) { if (++strikes >= 2) off; } else strikes = 0;`)
    CHECK(spec_on_after({5}));
    CHECK(spec_on_after({5, 8}));                              // one strike
    CHECK(!spec_on_after({5, 8, 11}));                         // two
    CHECK(!spec_on_after({5, 9, 13}));                         // exactly four apart still counts
    CHECK(spec_on_after({5, 10}));                             // five apart: no strike
    CHECK(spec_on_after({5, 10, 13}));                         // ... and the count had started over: one strike
    CHECK(!spec_on_after({5, 10, 13, 16}));
    CHECK(spec_on_after({5, 8, 20, 23}));                      // a stall further away forgets the strike before it
    {
        StallBook b(6, 1, 8, 0, true);
        for (int st : {5, 8, 11}) b.spec_stall(st);
        CHECK(!b.spec_on);
        b.spec_stall(40); b.solver_stall(41); b.select_stall(); b.rerun(50);
        CHECK(!b.spec_on);                                     // once off they stay off
        CHECK(b.spec_stalls == 4 && b.solver_stalls == 1 && b.select_stalls == 1);
        StallBook off(6, 1, 8, 0, false);                      // a run that never predicted
        off.spec_stall(5);
        CHECK(!off.spec_on);
    }
    // ---- counters count what was reported
    {
        StallBook b(6, 1, 4, 0, true);
        CHECK(b.solver_stalls == 0 && b.select_stalls == 0 && b.spec_stalls == 0);
        b.select_stall(); b.select_stall(); b.select_stall();
        b.spec_stall(9);
        b.solver_stall(12); b.solver_stall(30);
        CHECK(b.solver_stalls == 2 && b.select_stalls == 3 && b.spec_stalls == 1);
    }
    // ---- starting passes per stage
    CHECK(starting_passes(0, 1, 0.97) == 1 && starting_passes(0, 1, 0.95) == 1 && starting_passes(0, 1, 0.9) == 2);
    CHECK(starting_passes(3, 1, 0.9) == 3 && starting_passes(1, 1, 0.9) == 1 && starting_passes(-1, 1, 0.5) == 2);
    // ---- stages left and the batch bound
    {
        StagesLeft l;
        CHECK(l.est == StagesLeft::UNKNOWN);
        l.observe(0.5, 0.5 - 0.4);
        CHECK(l.est == 6);
        l.observe(0.5, 0.0);                                   // ϕ_n = ϕ_prev: left alone
        CHECK(l.est == 6);
        l.observe(1.0, 0.1);                                   // the run is at its end: left alone
        CHECK(l.est == 6);
        l.observe(0.5, 0.5e-6);                                // ratio 1e6
        CHECK(l.est == StagesLeft::UNKNOWN);
        l.observe(0.5, 0.5000001e-6);                          // just below
        CHECK(l.est == 1000000);
        l.observe(0.5, std::nan(""));
        CHECK(l.est == 1000000);
        for (int est : {1, 3, 4, 5, 20, 1000, StagesLeft::UNKNOWN})
            for (int sync : {1, 2, 4, 16, 32, 96})
                for (int room : {1, 2, 3, 4, 5, 31, 1200}) {
                    l.est = est;
                    const int b = l.batch(sync, room);
                    CHECK(b <= sync && b <= room);
                    CHECK(b >= std::min(std::min(4, room), sync));     // never below min(4, room) where sync_every allows as much
                    CHECK(b == std::min(std::min(sync, std::max(est, 4)), room));
                }
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
