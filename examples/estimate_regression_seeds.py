"""The regression example (estimate_regression.py) with its likelihood written as HIP source, estimated over 16 seeds in ONE launch:
smc_ensemble(HIPLikelihood(source, ensemble=True), parameters, data, seeds) compiles the function into the ensemble kernel once, runs one
workgroup per seed and returns one (cloud, w, W) per seed - here for the mean and the standard deviation of the log-MDD over seeds.

    python examples/estimate_regression_seeds.py
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import smc_jl_amd as S  # noqa: E402

# y_t = a + b x_t + e_t, e_t ~ N(0, 1); data = [y X] (rows x 2, column-major on the device); par = { -rows / 2 log(2 pi), 1 / 2 }
SOURCE = """
__device__ double loglik(const double *theta, long long ld, int d, const double *data, long long rows, long long cols,
                         const double *par, long long n_par) {
    double acc = 0.0;
    for (long long t = 0; t < rows; ++t) {
        const double e = (data[t] - theta[0]) - theta[ld] * data[t + rows];
        acc += e * e;
    }
    return par[0] - par[1] * acc;
}
"""


def main():
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(S.__file__)), "host", "data", "reg_data.npz"))["data"]          # 100 x 2
    parameters = [S.parameter("α1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False),
                  S.parameter("β1", 0.0, (-1e5, 1e5), (-1e5, 1e5), None, S.Normal(0, 10), fixed=False)]
    lik = S.HIPLikelihood(SOURCE, par=[-0.5 * data.shape[0] * math.log(2.0 * math.pi), 0.5], ensemble=True)
    seeds = list(range(1, 17))
    runs = S.smc_ensemble(lik, parameters, data, seeds, n_parts=1000, use_fixed_schedule=True)
    logmdd = np.array([cloud.logmdd for cloud, _, _ in runs])
    for s, (cloud, _, _) in zip(seeds, runs):
        print("seed %2d: %d stages, log-MDD %.6f, mean %s" % (s, cloud.stage_index, cloud.logmdd, np.array2string(S.weighted_mean(cloud), precision=5)))
    print("log-MDD over %d seeds: mean %.6f, standard deviation %.6f" % (len(seeds), logmdd.mean(), logmdd.std(ddof=1)))


if __name__ == "__main__":
    main()
