/* The reference's entry point smc(loglikelihood::Function, parameters, data; ...) (src/smc_main.jl:118) from plain C with the user's
 * likelihood ON THE GPU and no toolchain: the likelihood is a string of HIP source, compiled by the library at run time
 * (smcmi_program_compile) and registered with smcmi_set_likelihood_program (include/smcmi.h).  Config 2's workload (10-dim isotropic
 * Gaussian, adaptive tempering) twice on the same Philox seed: once with the built-in device family, once with the program; the runs
 * must agree (stage / resample counts, log-MDD to 1e-9).  The result line has the fields of examples/c_abi_callback.c; the likelihood
 * is that example's arithmetic - the same IEEE operations in the same order - so the two examples print the same numbers.
 *
 *   gcc -std=c99 -O2 -ffp-contract=off -Iinclude examples/c_abi_program.c -Lsmc.jl_amd/csrc -lsmcmi -lm -o c_abi_program
 */
#define _USE_MATH_DEFINES
#include <math.h>
#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "smcmi.h"

#define D 10
#define CHECK(call)                                                                    \
    do {                                                                               \
        int rc_ = (call);                                                              \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, smcmi_last_error()); return 1; } \
    } while (0)

/* loglikelihood(parameters, data) for ONE proposal: parameter j at theta[j * ld]; data = the d means, par = { c0, 2 sigma^2 } */
static const char *SOURCE =
    "__device__ double loglik(const double *theta, long long ld, int d, const double *data, long long rows, long long cols,\n"
    "                         const double *par, long long n_par) {\n"
    "    double acc = 0.0;\n"
    "    for (int j = 0; j < d; ++j) {\n"
    "        const double e = theta[j * ld] - data[j];\n"
    "        acc += e * e;\n"
    "    }\n"
    "    return par[0] - acc / par[1];\n"
    "}\n";

int main(int argc, char **argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 100000;
    smcmi_result res[2];
    double secs[2], phases[8] = {0}, mean[D], par[2];
    const double sigma = 0.25;
    int64_t calls = 0, evals = 0;
    for (int k = 0; k < D; ++k) mean[k] = -1.0 + 2.0 * (double)k / (double)(D - 1);
    par[0] = -0.5 * (double)D * log(2.0 * M_PI * sigma * sigma);
    par[1] = 2.0 * sigma * sigma;
    smcmi_program *prog = NULL;
    const int crc = smcmi_program_compile(SOURCE, NULL, NULL, &prog);
    if (crc != 0) {
        fprintf(stderr, "smcmi_program_compile -> %d: %s\n%s\n", crc, smcmi_last_error(), prog ? smcmi_program_log(prog) : "");
        if (prog) smcmi_program_destroy(prog);
        return 1;
    }
    for (int mode = 0; mode < 2; ++mode) {
        smcmi_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_parts = n; cfg.n_local = n; cfg.n_para = D; cfg.seed = 1; cfg.max_stages = 1500; cfg.store_history = 0;
        smcmi_handle *h = NULL;
        CHECK(smcmi_create(&cfg, &h));
        int32_t fixed[D], fam[D];
        double lo[D], hi[D], pa[D], pb[D];
        for (int k = 0; k < D; ++k) { fixed[k] = 0; fam[k] = SMCMI_PRIOR_NORMAL; lo[k] = -1e5; hi[k] = 1e5; pa[k] = 0.0; pb[k] = 5.0; }
        CHECK(smcmi_set_parameters(h, fixed, lo, hi, fam, pa, pb));
        /* the initial draw (initial_draw!, initialization.jl:88-119) by the device family in both modes: the same starting cloud */
        CHECK(smcmi_set_likelihood(h, SMCMI_WHICH_NEW, SMCMI_LIK_GAUSS_ISO, &sigma, 1, mean, D, 1, NULL, 0, 0));
        CHECK(smcmi_set_likelihood(h, SMCMI_WHICH_OLD, SMCMI_LIK_NONE, NULL, 0, NULL, 0, 0, NULL, 0, 0));
        CHECK(smcmi_init_from_prior(h));
        if (mode == 1) {
            CHECK(smcmi_set_likelihood_program(h, SMCMI_WHICH_NEW, prog, mean, D, 1, par, 2));
            CHECK(smcmi_program_destroy(prog));          /* (the handle keeps its own module) */
            prog = NULL;
        }
        smcmi_run_config rc;
        memset(&rc, 0, sizeof rc);
        rc.n_blocks = 1; rc.n_mh_steps = 1; rc.lambda = 2.1; rc.n_phi = 300; rc.resampling_method = SMCMI_RESAMPLE_SYSTEMATIC;
        rc.threshold_ratio = 0.5; rc.c = 0.5; rc.alpha = 1.0; rc.target = 0.25; rc.use_fixed_schedule = 0; rc.tempering_target = 0.97;
        CHECK(smcmi_run(h, &rc, &res[mode]));
        secs[mode] = res[mode].seconds;
        if (mode == 1) {
            CHECK(smcmi_callback_phases(h, phases, 8));
            CHECK(smcmi_callback_stats(h, &calls, &evals));
        }
        CHECK(smcmi_destroy(h));
    }
    const double ps0 = (double)n * (res[0].n_stages - 1) / secs[0], ps1 = (double)n * (res[1].n_stages - 1) / secs[1];
    const double st = (double)(res[1].n_stages - 1);
    printf("{\"n_parts\": %lld, \"device\": {\"n_stages\": %d, \"resamples\": %d, \"logmdd\": %.17g, \"particle_stages_per_s\": %.4g}, "
           "\"callback\": {\"n_stages\": %d, \"resamples\": %d, \"logmdd\": %.17g, \"particle_stages_per_s\": %.4g, \"calls\": %lld, \"callback_threads\": %d, "
           "\"ms_per_stage\": %.4f, \"phases_ms_per_stage\": {\"first_chunk_wait\": %.4f, \"later_chunk_wait\": %.4f, \"pack\": %.4f, \"callback\": %.4f, "
           "\"scatter\": %.4f, \"enqueue\": %.4f, \"stage_device_part\": %.4f}}}\n",
           n, res[0].n_stages, res[0].resamples, res[0].logmdd, ps0, res[1].n_stages, res[1].resamples, res[1].logmdd, ps1, (long long)calls, 0,
           1e3 * secs[1] / st, phases[0] / st, phases[1] / st, phases[2] / st, phases[3] / st, phases[4] / st, phases[5] / st, phases[6] / st);
    /* one launch per stage (1 MH step x 1 block), every proposal inside the bounds and scored */
    if (res[0].n_stages != res[1].n_stages || res[0].resamples != res[1].resamples || fabs(res[0].logmdd - res[1].logmdd) > 1e-9 ||
        calls != res[1].n_stages - 1 || evals != calls * n) {
        printf("MISMATCH\n");
        return 2;
    }
    printf("OK\n");
    return 0;
}
