/* "My own HIP likelihood": the user's likelihood as a __global__ kernel of their own, handed to the engine as a device callback
 * (smcmi_set_likelihood_device, include/smcmi.h) - no run-time compilation, no proposal and no log-likelihood crossing PCIe.  The
 * callback receives device pointers and the handle's stream and launches its kernel on that stream; it does not synchronise.
 * Config 2's workload as in examples/c_abi_callback.c (10-dim isotropic Gaussian, adaptive tempering), twice on the same Philox seed:
 * once with the built-in device family, once with the user's kernel - the Gaussian of csrc/model.hpp GAUSS_ISO in the same summation
 * order, so with contraction off the runs agree (stage / resample counts, log-MDD to 1e-9).  Prints the result line of
 * c_abi_callback.c.
 *
 *   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -Iinclude examples/c_abi_device_callback.hip -Lsmc.jl_amd/csrc -lsmcmi -o c_abi_device_callback
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smcmi.h"

#define D 10
#define CHECK(call)                                                                    \
    do {                                                                               \
        int rc_ = (call);                                                              \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, smcmi_last_error()); return 1; } \
    } while (0)

struct gauss_data { double mean[D], sigma, c0; long long calls, evals; };

/* loglikelihood(parameters, data) for a batch: proposal k, parameter j at theta[k + ld * j]; one thread per proposal, every column a
 * unit-stride stream across the wavefront */
__global__ void __launch_bounds__(256) gauss_loglik_kernel(const double *__restrict__ theta, long long m, long long ld, gauss_data g, double *__restrict__ out) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    double acc = 0.0;
    for (int j = 0; j < D; ++j) { const double e = theta[k + ld * j] - g.mean[j]; acc += e * e; }
    out[k] = g.c0 - acc / (2.0 * g.sigma * g.sigma);
}

static int gauss_loglik(const double *theta, int64_t m, int64_t ld, int64_t d, double *out, void *stream, void *ud) {
    gauss_data *g = (gauss_data *)ud;
    if (d != D || m < 1) return 1;
    gauss_loglik_kernel<<<(unsigned)((m + 255) / 256), 256, 0, (hipStream_t)stream>>>(theta, (long long)m, (long long)ld, *g, out);
    if (hipGetLastError() != hipSuccess) return 2;
    g->calls += 1; g->evals += m;
    return 0;
}

int main(int argc, char **argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 100000;
    smcmi_result res[2];
    double secs[2], phases[8] = {0};
    gauss_data g;
    memset(&g, 0, sizeof g);
    g.sigma = 0.25;
    for (int k = 0; k < D; ++k) g.mean[k] = -1.0 + 2.0 * (double)k / (double)(D - 1);
    g.c0 = -0.5 * (double)D * log(2.0 * M_PI * g.sigma * g.sigma);
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
        /* the initial draw by the device family in both modes: the same starting cloud */
        CHECK(smcmi_set_likelihood(h, SMCMI_WHICH_NEW, SMCMI_LIK_GAUSS_ISO, &g.sigma, 1, g.mean, D, 1, NULL, 0, 0));
        CHECK(smcmi_set_likelihood(h, SMCMI_WHICH_OLD, SMCMI_LIK_NONE, NULL, 0, NULL, 0, 0, NULL, 0, 0));
        CHECK(smcmi_init_from_prior(h));
        smcmi_device_likelihood lik;
        lik.fn = gauss_loglik; lik.user_data = &g;
        if (mode == 1) CHECK(smcmi_set_likelihood_device(h, SMCMI_WHICH_NEW, &lik));
        smcmi_run_config rc;
        memset(&rc, 0, sizeof rc);
        rc.n_blocks = 1; rc.n_mh_steps = 1; rc.lambda = 2.1; rc.n_phi = 300; rc.resampling_method = SMCMI_RESAMPLE_SYSTEMATIC;
        rc.threshold_ratio = 0.5; rc.c = 0.5; rc.alpha = 1.0; rc.target = 0.25; rc.use_fixed_schedule = 0; rc.tempering_target = 0.97;
        CHECK(smcmi_run(h, &rc, &res[mode]));
        secs[mode] = res[mode].seconds;
        if (mode == 1) {
            int64_t calls = 0, evals = 0;
            CHECK(smcmi_callback_phases(h, phases, 8));
            CHECK(smcmi_callback_stats(h, &calls, &evals));
            if (calls != g.calls || evals != g.evals) { fprintf(stderr, "callback statistics disagree\n"); return 3; }
        }
        CHECK(smcmi_destroy(h));
    }
    const double ps0 = (double)n * (res[0].n_stages - 1) / secs[0], ps1 = (double)n * (res[1].n_stages - 1) / secs[1];
    const double st = (double)(res[1].n_stages - 1);
    /* (the PCIe and host-side phases are 0 for a device callback; the wait for the propose kernel and the count is the last value) */
    printf("{\"n_parts\": %lld, \"device\": {\"n_stages\": %d, \"resamples\": %d, \"logmdd\": %.17g, \"particle_stages_per_s\": %.4g}, "
           "\"callback\": {\"n_stages\": %d, \"resamples\": %d, \"logmdd\": %.17g, \"particle_stages_per_s\": %.4g, \"calls\": %lld, \"callback_threads\": %d, "
           "\"ms_per_stage\": %.4f, \"phases_ms_per_stage\": {\"first_chunk_wait\": %.4f, \"later_chunk_wait\": %.4f, \"pack\": %.4f, \"callback\": %.4f, "
           "\"scatter\": %.4f, \"enqueue\": %.4f, \"stage_device_part\": %.4f, \"count_wait\": %.4f}}}\n",
           n, res[0].n_stages, res[0].resamples, res[0].logmdd, ps0, res[1].n_stages, res[1].resamples, res[1].logmdd, ps1, g.calls, 0,
           1e3 * secs[1] / st, phases[0] / st, phases[1] / st, phases[2] / st, phases[3] / st, phases[4] / st, phases[5] / st, phases[6] / st, phases[7] / st);
    /* one invocation per stage (one MH step, one block) */
    if (res[0].n_stages != res[1].n_stages || res[0].resamples != res[1].resamples || fabs(res[0].logmdd - res[1].logmdd) > 1e-9 ||
        g.calls != res[1].n_stages - 1) {
        printf("MISMATCH\n");
        return 2;
    }
    printf("OK\n");
    return 0;
}
