"""smc.jl_amd - MI355X-native SMC particle engine behind the FRBNY-DSGE/SMC.jl interface.

The directory name contains a dot, so import it as `smc_jl_amd` (repo-root shim smc_jl_amd.py).
Contents: csrc/ (HIP kernels + C ABI -> libsmcmi.so), host/ (ctypes binding and the Python mirror of the
reference's `smc(...)` / `Cloud` interface), julia/ (the ccall shim a Julia user loads).
"""
from .host import _lib  # noqa: F401
from .host.engine import (CompileError, Engine, Program, best_particle_group, comm_unique_id, run_ensemble, run_group, torch_dist_host_comm,  # noqa: F401
                          weighted_quantiles_group)
from .host.api import (Beta, CapmLiteral, LGSSKalman, Cloud, Gamma, GaussIso, InverseGamma, LinModel3, LinReg, Normal, Parameter,  # noqa: F401
                       RootInverseGamma, TorchLikelihood, HIPLikelihood, Uniform, cloud_isempty, get_accept, get_loglh, get_logpost, get_logprior,
                       get_old_loglh, get_vals, get_weights, parameter, smc, smc_ensemble, weighted_cov, weighted_mean, weighted_std, flatten_regimes, regime_values,
                       weighted_quantile, weighted_quantiles, get_likeliest_particle_value, get_highest_posterior_particle_value,
                       get_cloud, initial_draw, mutation, mvnormal_mixture_draw, resample)
from .host.cloudio import add_parameters_to_cloud, join_cloud, load_cloud, save_cloud, split_cloud  # noqa: F401

__all__ = ["Engine", "_lib", "smc", "smc_ensemble", "run_ensemble", "Cloud", "parameter", "Normal", "Uniform", "Gamma", "Beta", "InverseGamma",
           "RootInverseGamma", "GaussIso", "LinReg", "LinModel3", "CapmLiteral", "LGSSKalman", "TorchLikelihood", "HIPLikelihood", "Program", "CompileError", "get_vals", "get_loglh", "get_logprior",
           "get_old_loglh", "get_logpost", "get_accept", "get_weights", "weighted_mean", "weighted_cov", "weighted_std", "weighted_quantile", "weighted_quantiles",
           "get_likeliest_particle_value", "get_highest_posterior_particle_value", "weighted_quantiles_group", "best_particle_group",
           "cloud_isempty", "get_cloud", "initial_draw", "mutation", "mvnormal_mixture_draw", "resample", "split_cloud", "join_cloud", "add_parameters_to_cloud", "save_cloud", "load_cloud", "flatten_regimes", "regime_values"]
