/* tools/program_bench.py, leg (b): config 2's Gaussian as a user-written __global__ kernel behind a device callback
 * (smcmi_set_likelihood_device) - what examples/c_abi_device_callback.hip does, as a shared library so that the three legs of the
 * benchmark run in one process.  The arithmetic is that example's (and csrc/model.hpp GAUSS_ISO's): the same IEEE operations in the
 * same order, contraction off.
 *
 *   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -fPIC -shared tools/program_bench_cb.hip -o tools/libprogram_bench_cb.so
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#define D 10
struct gauss_data { double mean[D], sigma, c0; };
static gauss_data g_data;

__global__ void __launch_bounds__(256) pb_gauss_loglik_kernel(const double *__restrict__ theta, long long m, long long ld, gauss_data g, double *__restrict__ out) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    double acc = 0.0;
    for (int j = 0; j < D; ++j) { const double e = theta[k + ld * j] - g.mean[j]; acc += e * e; }
    out[k] = g.c0 - acc / (2.0 * g.sigma * g.sigma);
}

extern "C" void pb_setup(const double *mean, double sigma, double c0) {
    for (int j = 0; j < D; ++j) g_data.mean[j] = mean[j];
    g_data.sigma = sigma;
    g_data.c0 = c0;
}
/* smcmi_lik_device_fn */
extern "C" int pb_gauss_loglik(const double *theta, int64_t m, int64_t ld, int64_t d, double *out, void *stream, void *ud) {
    (void)ud;
    if (d != D || m < 1) return 1;
    pb_gauss_loglik_kernel<<<(unsigned)((m + 255) / 256), 256, 0, (hipStream_t)stream>>>(theta, (long long)m, (long long)ld, g_data, out);
    return hipGetLastError() != hipSuccess ? 2 : 0;
}
