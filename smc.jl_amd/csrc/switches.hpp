// switches.hpp - the development switches of DESIGN §7b: one field per name, one place that reads the environment, one place per default.
// None is needed in production.  Everything is read once per process (sw()), except the two names a caller may change between runs of one
// process - the mailbox transport and the bound of its waits (include/smcmi.h) - which Switches::per_run() reads again at every run.
// Included by smcmi.hip only; plain host C++ without a HIP call, so tests/route_check.hip can fill a Switches by hand.
#pragma once
#include <cstdlib>
#include <string>

struct Switches {
    struct OptInt { bool set = false; int v = 0; };      // a name whose presence matters next to its value
    // ---- stage engines
    int engine = 0;                 // SMCMI_ENGINE: 1 = engine 1 everywhere, 2 = engine 2 beyond the direct geometry
    int engine3 = 1;                // SMCMI_ENGINE3: 0 segments off, 1 default, 2 one handle only, 3 also for in-process groups of any size
    bool e2_reduced = false;        // SMCMI_E2_REDUCED (set): the k2_reduce path on one small handle
    OptInt e2_nb1;                  // SMCMI_E2_NB1=<n>: correction rows per virtual shard
    int e2_helpers = 1;             // SMCMI_E2_HELPERS: 0 = k2_begin / k2_prepare as launches
    int seg_select = 1;             // SMCMI_SEG_SELECT: 0 = a segment leaves at a stage that must resample
    int k3_general = 0;             // SMCMI_K3_GENERAL: 1 = the segment kernel's general unit where the default-run unit would run (launch2.hpp)
    int run_prologue = 1;          // SMCMI_RUN_PROLOGUE: 0 = a fresh single-handle run starts and ends with the copies and launches it used to
    double seg_timeout_ms = 0.0;    // SMCMI_SEG_TIMEOUT_MS: <= 0 = the driver's bound (200 ms, 1 s across handles)
    // ---- hand-over transport: read at every run (per_run)
    int mailbox = -1;               // SMCMI_MAILBOX: -1 default, 0 off, 1 on, 2 also with one rank
    double mailbox_timeout_ms = 0.0; // SMCMI_MAILBOX_TIMEOUT_MS: <= 0 = the transport's default (stage2.hpp MB_TIMEOUT_TICKS_DEFAULT)
    // ---- solver and schedule
    int no_predictor = 0;           // SMCMI_NO_PREDICTOR: 1 = the solver without the energy-sum predictor
    int no_select_predict = 0;      // SMCMI_NO_SELECT_PREDICT: 1 = always, 2 = never expect a resample
    int shift_lag = 1;              // SMCMI_SHIFT_LAG: 0 exact shifts, k >= 3 / -k: stage k's lagged shift overflows / underflows
    int center = 1;                 // SMCMI_CENTER: 0 = the one-pass moments keep the shift the handle holds
    int fixed_no_select = 1;        // SMCMI_FIXED_NO_SELECT: 0 = engine 1's seven-launch fixed stage
    long long rng_ahead_part = 250000;   // SMCMI_RNG_AHEAD_PART: draws per stage the set-up launch makes ahead
    bool resample_allgather = false; // SMCMI_RESAMPLE_EXCHANGE=allgather
    // ---- models, closures
    int kalman_lanes = 0;           // SMCMI_KALMAN_LANES: 1 / 4 lanes per particle, 0 = by cloud size
    int no_lik_prefix = 0;          // SMCMI_NO_LIK_PREFIX: 1 = two filter passes
    int cb_chunks = 0;              // SMCMI_CB_CHUNKS: chunks per batch, 0 = by batch size
    int fused_ahead = 0;            // SMCMI_FUSED_AHEAD: 1 = a fused program's mutation launch goes out before the stage's verdict is read
    // ---- diagnostics
    int trace = 0;                  // SMCMI_TRACE
    OptInt prof2;                   // SMCMI_PROF2=<stage>
    int poison_alloc = 0;           // SMCMI_POISON_ALLOC: 1 poisons fresh device memory, 2 also reports allocations and releases (devmem.hpp)
    std::string rccl_path;          // SMCMI_RCCL_PATH: the RCCL to dlopen first

    static Switches read() {
        Switches s;
        auto opt = [](const char *name, OptInt *out) { if (const char *v = getenv(name)) { out->set = true; out->v = atoi(v); } };
        auto integer = [](const char *name, int *out) { if (const char *v = getenv(name)) *out = atoi(v); };
        integer("SMCMI_ENGINE", &s.engine); integer("SMCMI_ENGINE3", &s.engine3);
        s.e2_reduced = getenv("SMCMI_E2_REDUCED") != nullptr;
        opt("SMCMI_E2_NB1", &s.e2_nb1); integer("SMCMI_E2_HELPERS", &s.e2_helpers); integer("SMCMI_SEG_SELECT", &s.seg_select);
        integer("SMCMI_RUN_PROLOGUE", &s.run_prologue); integer("SMCMI_K3_GENERAL", &s.k3_general);
        if (const char *v = getenv("SMCMI_SEG_TIMEOUT_MS")) s.seg_timeout_ms = atof(v);
        integer("SMCMI_NO_PREDICTOR", &s.no_predictor); integer("SMCMI_NO_SELECT_PREDICT", &s.no_select_predict);
        integer("SMCMI_SHIFT_LAG", &s.shift_lag); integer("SMCMI_CENTER", &s.center); integer("SMCMI_FIXED_NO_SELECT", &s.fixed_no_select);
        if (const char *v = getenv("SMCMI_RNG_AHEAD_PART")) s.rng_ahead_part = atoll(v);
        if (const char *v = getenv("SMCMI_RESAMPLE_EXCHANGE")) s.resample_allgather = std::string(v) == "allgather";
        integer("SMCMI_KALMAN_LANES", &s.kalman_lanes); integer("SMCMI_NO_LIK_PREFIX", &s.no_lik_prefix); integer("SMCMI_CB_CHUNKS", &s.cb_chunks);
        integer("SMCMI_FUSED_AHEAD", &s.fused_ahead);
        integer("SMCMI_TRACE", &s.trace); opt("SMCMI_PROF2", &s.prof2); integer("SMCMI_POISON_ALLOC", &s.poison_alloc);
        if (const char *v = getenv("SMCMI_RCCL_PATH")) s.rccl_path = v;
        s.read_per_run();
        return s;
    }
    // the process's switches with the two per-run names as the environment has them now
    Switches per_run() const { Switches s = *this; s.read_per_run(); return s; }

private:
    void read_per_run() {
        const Switches dflt;
        const char *mb = getenv("SMCMI_MAILBOX"), *ms = getenv("SMCMI_MAILBOX_TIMEOUT_MS");
        mailbox = mb ? atoi(mb) : dflt.mailbox;
        mailbox_timeout_ms = ms ? atof(ms) : dflt.mailbox_timeout_ms;
    }
};
static const Switches &sw() { static const Switches s = Switches::read(); return s; }
