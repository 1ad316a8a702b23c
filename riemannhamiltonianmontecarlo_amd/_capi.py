"""ctypes binding of the C-ABI declared in include/rmhmc.h.

``RmhmcLib(path)`` binds any shared library exporting that ABI.  The product
uses it with the HIP library only (``load_hip_library``), which raises if the
extension is missing or cannot run — there is no CPU fallback.  The test-suite
binds the CPU oracle with the same class to diff results.
"""
import ctypes as C
import math
import os

import numpy as np

F64 = 0
FLAG_MOMENTUM_LT = 1 << 0
FLAG_GUARDS = 1 << 1
COMPAT = FLAG_MOMENTUM_LT | FLAG_GUARDS
FLAG_FP32_METRIC = 1 << 4
FLAG_INT8_METRIC = 1 << 5
FLAG_MMALA_FULL = 1 << 6
FLAG_INT8_CERTIFY = 1 << 7
FLAG_INT8_INNER_FULL = 1 << 10   # int8 x 6 slices: position iterates before the last also from all 6 slices (default: 5)
FLAG_ESS_WRAP = 1 << 9      # ESS with the reference Python's wrapped FFT length (tools.py:23); default = MATLAB (no wrap)
INT8_CERTIFY_TOL = 1e-9


def int8_metric_flags(slices=6):
    """flags for the int8 matrix-core metric assembly with `slices` byte slices per operand (4..7), include/rmhmc.h"""
    if not 4 <= int(slices) <= 7:
        raise ValueError("slices must be 4..7")
    return FLAG_INT8_METRIC | (int(slices) << 12)


def auto_metric_flags(D, n_chains, slices=None, M=None):
    """None: 6 slices where the int8 path pays: 8 < D <= 256 and enough work to fill its 128 x 128 tiles, n_chains * M * D^2 >= 1e9
    (measured, tools/i8_threshold.py: 1.3-1.7x over the fp64 matrix cores from 128 chains x 10000 rows x D 64 and from 8192 chains of
    the 690 x 15 australian data upwards; 0.76x at 600 chains x 1000 x 25), or n_chains >= 1024 when M is not given; 0: fp64 cores"""
    auto = slices is None
    if slices is None:
        big = (n_chains * float(M) * D * D >= 1e9) if M is not None else (n_chains >= 1024)
        slices = 6 if (8 < D <= 256 and big) else 0
    if not slices:
        return 0
    # chosen by the shim, not by the caller: let rmhmc_set_data check the error bound for the actual data and fall back to fp64
    return int8_metric_flags(slices) | (FLAG_INT8_CERTIFY if auto else 0)


FLAG_ORACLE_LITERAL = 1 << 8

ST_NOT_PD, ST_NONFINITE, ST_GUARD_P, ST_GUARD_W = 1, 2, 4, 8

_PKG = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_PKG, "csrc", "librmhmc_hip.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)

PROGRESS_FN = C.CFUNCTYPE(None, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p)
EV_PROGRESS, EV_BURNIN_DONE = 0, 1



class Option(C.Structure):
    """rmhmc_option of include/rmhmc.h: one (key, value) tuning option"""
    _fields_ = [("key", C.c_char_p), ("value", C.c_int64)]


# every symbol include/rmhmc.h declares, with its signature
SIGNATURES = {
    "rmhmc_create_opts": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_uint32,
                                    C.POINTER(Option), C.c_int32]),
    "rmhmc_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "rmhmc_get_option": (C.c_int, [C.c_void_p, C.c_char_p, _lp]),
    "rmhmc_options": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "rmhmc_version": (C.c_char_p, []),
    "rmhmc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_uint32]),
    "rmhmc_destroy": (None, [C.c_void_p]),
    "rmhmc_last_error": (C.c_char_p, [C.c_void_p]),
    "rmhmc_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "rmhmc_set_data": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double]),
    "rmhmc_log_posterior": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rmhmc_metric": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "rmhmc_metric_terms": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "rmhmc_leapfrog": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double, _ip, _ip, C.c_int32, _dp, _ip]),
    "rmhmc_transition": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp, C.c_int32, C.c_double, C.c_int32,
                                   _ip, _ip, _dp, _dp, _dp, _dp, _dp, _ip]),
    "rmhmc_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                               C.c_int64, _dp, _dp, _lp, _lp, _dp]),
    "rmhmc_chains_init": (C.c_int, [C.c_void_p, _dp, C.c_uint64, C.c_int64, C.c_int32, C.c_double, C.c_int32]),
    "rmhmc_chains_run": (C.c_int, [C.c_void_p, C.c_int64]),
    "rmhmc_chains_state": (C.c_int, [C.c_void_p, _dp, _lp, _lp]),
    "rmhmc_chains_restore": (C.c_int, [C.c_void_p, _lp, _lp]),
    "rmhmc_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, _dp, _lp]),
    "rmhmc_int8_certificate": (C.c_int, [C.c_void_p, _dp, _ip]),
    "rmhmc_set_progress": (C.c_int, [C.c_void_p, PROGRESS_FN, C.c_int64, C.c_int64, C.c_void_p]),
    "rmhmc_ess": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int64, C.c_int32, _dp]),
    "rmhmc_sample_stats": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int64,
                                     _dp, _dp, _dp, _dp, _lp, _lp, _dp]),
    "rmhmc_chains_state_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rmhmc_sample_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                                   C.c_int64, _dp, C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    "rmhmc_sample_stats_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int64,
                                         _dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    "rmhmc_mmala_transition": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_double, _ip, _dp, _dp]),
    "rmhmc_mmala_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_uint64, C.c_int64, _dp, _dp, _lp, _dp]),
    "rmhmc_hmc_transition": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int32, C.c_double, _ip, _ip, _dp, _dp, _dp, _dp]),
    "rmhmc_hmc_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_uint64, C.c_int64, _dp, _dp,
                                   _lp, _lp, _dp]),
}

# include/rmhmc_amh.h: the adaptive Metropolis sampler, exported by the HIP library only (not by the CPU oracle), so bound apart from
# SIGNATURES and only where the library has it
_i8p = C.POINTER(C.c_int8)
AMH_SIGNATURES = {
    "rmhmc_amh_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, _dp, _dp, _lp, _dp, _dp]),
    "rmhmc_amh_replay": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _i8p]),
}
# include/rmhmc_iwls.h: the IWLS Metropolis-Hastings sampler, HIP library only as well
IWLS_SIGNATURES = {
    "rmhmc_iwls_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64, C.c_int64, _dp, _dp, _lp, _lp, _dp]),
    "rmhmc_iwls_replay": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _i8p]),
}
# include/rmhmc_gibbs.h: the auxiliary-variable Gibbs sampler, HIP library only as well
GIBBS_SIGNATURES = {
    "rmhmc_gibbs_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, _dp, _lp, _lp, _dp, _dp, _dp]),
    "rmhmc_gibbs_replay": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _lp, C.c_int64, _dp, _dp, _ip, _dp, _dp, _lp, _ip]),
}


# include/rmhmc_out.h: the output descriptor (every sampler to host or device memory, raw or reduced), HIP library only as well
OUT_HOST, OUT_DEVICE = 0, 1


class Out(C.Structure):
    """rmhmc_out of include/rmhmc_out.h: every pointer in the memory space `where` names, NULL where an output is not wanted"""
    _fields_ = [("where", C.c_int32), ("samples", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p), ("ess", C.c_void_p),
                ("run_mean", C.c_void_p), ("run_ess", C.c_void_p)]


_op = C.POINTER(Out)
_vp = C.c_void_p   # a counter output: host or device memory, as Out.where says
OUT_SIGNATURES = {
    "rmhmc_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int64, _dp, _op,
                                  _vp, _vp, _dp]),
    "rmhmc_hmc_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_uint64, C.c_int64, _dp, _op, _vp, _vp,
                                      _dp]),
    "rmhmc_mmala_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_uint64, C.c_int64, _dp, _op, _vp, _dp]),
    "rmhmc_amh_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, _dp, _op, _vp, _vp, _dp]),
    "rmhmc_iwls_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64, C.c_int64, _dp, _op, _vp, _vp, _dp]),
    "rmhmc_gibbs_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, _op, _vp, _vp, _dp]),
    "rmhmc_ess_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _vp, _vp, _vp]),
}
# sampler -> (entry point, its per-chain counters in the order of its signature: (dict key, [n][D] doubles instead of [n] int64))
SAMPLERS_TO = {
    "rmhmc": ("rmhmc_sample_to", (("accepted", False), ("leapfrog_steps", False))),
    "hmc": ("rmhmc_hmc_sample_to", (("accepted", False), ("leapfrog_steps", False))),
    "mmala": ("rmhmc_mmala_sample_to", (("accepted", False),)),
    "amh": ("rmhmc_amh_sample_to", (("accepted", False), ("sd", True))),
    "iwls": ("rmhmc_iwls_sample_to", (("accepted", False), ("saturated", False))),
    "gibbs": ("rmhmc_gibbs_sample_to", (("capped", False), ("stopped", False))),
}
# the run arguments a sampler has besides n_iter, burn_in, seed, chain_offset (Context.sample_to)
SAMPLER_ARGS = {"rmhmc": ("L", "eps", "K", "theta0"), "hmc": ("L", "eps", "theta0"), "mmala": ("eps", "theta0"), "amh": ("theta0",),
                "iwls": ("compat", "theta0"), "gibbs": ()}
SUMMARY_KEYS = ("mean", "var", "ess", "run_mean", "run_ess")

# include/rmhmc_diag.h: split R-hat and the pooled ESS across chains, HIP library only as well
_dpp = C.POINTER(_dp)
DIAG_SIGNATURES = {
    "rmhmc_diag_partial_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, C.c_int64, _vp]),
    "rmhmc_diag_finish": (C.c_int, [_dpp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, _dp, _lp, _lp]),
}
DIAG_KEYS = ("rhat", "ess_pooled", "pairs", "chains_used")   # what diag_finish returns, [P] each
DIAG_S_MIN, DIAG_S_MAX = 4, 20000

# include/rmhmc_phmc.h: HMC with a fixed dense mass matrix shared by all chains and the Newton search for the posterior mode, HIP
# library only as well.  Not a key of SAMPLERS_TO: the sampler needs its mass matrix first (Context.phmc_set_mass), so it has methods
# of its own (Context.phmc_sample_to) instead of a place in the tables every sampler is run from.
PHMC_SIGNATURES = {
    "rmhmc_phmc_set_mass": (C.c_int, [C.c_void_p, _dp]),
    "rmhmc_phmc_mode": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_double, _dp, _dp, _ip, _dp]),
    "rmhmc_phmc_transition": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int32, C.c_double, _ip, _ip, _dp, _dp, _dp, _dp, _ip]),
    "rmhmc_phmc_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_uint64, C.c_int64, _dp, _op, _vp, _vp,
                                       _dp]),
}
PHMC_COUNTERS = (("accepted", False), ("leapfrog_steps", False))

# include/rmhmc_adapt.h: the warm-up of the fixed-metric HMC sampler (pooled covariance on the device, regularised mass, dual
# averaging of the step size), HIP library only as well
ADAPT_SIGNATURES = {
    "rmhmc_cov_partial_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _vp]),
    "rmhmc_cov_finish": (C.c_int, [_dpp, C.c_int32, C.c_int32, _dp, _dp, _dp, _lp]),
    "rmhmc_adapt_mass": (C.c_int, [_dp, C.c_int64, C.c_int32, _dp]),
    "rmhmc_adapt_init": (C.c_int, [_dp, C.c_double, C.c_double]),
    "rmhmc_adapt_step": (C.c_int, [_dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp]),
    "rmhmc_phmc_warmup": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64,
                                    C.c_int64, C.c_int32, _lp, _ip, C.c_int64, _dp, _dp, _dp, _dp, _dp, _ip, _dp]),
}
COV_MAX_P = 256      # widest sample row of rmhmc_cov_partial_dev
COV_ROWS = 256       # smallest row block of its kernels (csrc/adapt.h)

# include/rmhmc_ais.h: the log marginal likelihood by annealed importance sampling with tempered fixed-metric HMC, HIP library only as
# well.  Like PHMC it has methods of its own (Context.tphmc_sample_to, Context.ais_run) and no place in the sampler tables.
AIS_SIGNATURES = {
    "rmhmc_tphmc_transition": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int32, C.c_double, _ip, _ip, _dp, _dp, _dp, _dp, _ip, C.c_double,
                                         _dp, _dp]),
    "rmhmc_tphmc_sample_to": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_uint64, C.c_int64, _dp, _op, _vp, _vp,
                                        _dp, C.c_double, _dp, _dp]),
    "rmhmc_ais_prior": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, _dp]),
    "rmhmc_ais_partial_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, _vp]),
    "rmhmc_ais_finish": (C.c_int, [_dpp, C.c_int32, _dp, _dp, _dp, _dp, _lp, _lp]),
    "rmhmc_ais_run": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_int32, _dp, _lp, _ip, _dp, C.c_int32, C.c_double, C.c_uint64, C.c_int64,
                                _dp, _dp, _dp, _dp, _dp]),
}
AIS_PRIOR_ITER = 0xFFFFFFFF   # iteration counter of the prior draws (RMHMC_AIS_PRIOR_ITER)
AIS_KEYS = ("log_mean_w", "se", "weight_ess", "m", "n_nan")   # what ais_finish returns besides the merged partial

# include/rmhmc_pred.h: posterior predictive probabilities of new rows from draws on the device, HIP library only as well
PRED_SIGNATURES = {
    "rmhmc_pred_partial_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, C.c_int64, _vp]),
    "rmhmc_pred_finish": (C.c_int, [_dpp, C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, _dp, _lp]),
}
PRED_KEYS = ("prob", "pvar", "lpd", "lpd_total", "draws_used")   # what pred_finish returns besides the merged partial
PRED_MAX_D = 256     # widest draw of rmhmc_pred_partial_dev

# include/rmhmc_smc.h: the log marginal likelihood by adaptive sequential Monte Carlo (conditional-ESS ladder, systematic resampling on
# integers) on top of the tempered sampler of rmhmc_ais.h, HIP library only as well
SMC_SIGNATURES = {
    "rmhmc_smc_cess_dev": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.c_int32, _dp, _vp]),
    "rmhmc_smc_cess_finish": (C.c_int, [_dpp, C.c_int32, C.c_int32, _dp, _dp]),
    "rmhmc_smc_choose_delta_dev": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.c_double, C.c_double, _dp, _dp, _ip]),
    "rmhmc_smc_reweight_dev": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.c_double]),
    "rmhmc_smc_quantise_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_double, _vp]),
    "rmhmc_smc_ancestors_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_uint32, _vp]),
    "rmhmc_smc_run": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_double,
                                C.c_uint64, C.c_int64, _ip, _dp, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
}
SMC_MAX_J = 32            # most candidates of one smc_cess call (RMHMC_SMC_MAX_J)
SMC_J, SMC_ROUNDS = 16, 3     # the search: candidates per round, rounds (RMHMC_SMC_J, RMHMC_SMC_ROUNDS)
SMC_MAX_N = 2 ** 20       # most particles of smc_ancestors (RMHMC_SMC_MAX_N)
SMC_QBITS = 40            # q = 2^40 at the largest weight (RMHMC_SMC_QBITS)
SMC_LAST, SMC_FLOOR, SMC_RESAMPLED = 1, 2, 4      # flags of a stage

# include/rmhmc_quant.h: exact posterior quantiles by a radix select on mergeable integer histograms, HIP library only as well
_up = C.POINTER(C.c_uint64)
QUANT_SIGNATURES = {
    "rmhmc_quant_hist_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _up, C.c_int32, _vp]),
    "rmhmc_quant_plan": (C.c_int, [_lp, _dp, C.c_int32, C.c_int32, _lp, _dp]),
    "rmhmc_quant_step": (C.c_int, [_dpp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _up, _lp]),
    "rmhmc_quant_finish": (C.c_int, [_up, _dp, _lp, C.c_int32, C.c_int32, _dp]),
    "rmhmc_quant_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, _lp]),
}
QUANT_MAX_K, QUANT_MAX_Q, QUANT_BINS, QUANT_ROUNDS = 16, 8, 256, 8    # RMHMC_QUANT_MAX_K, RMHMC_QUANT_MAX_Q; bins of a round, rounds
QUANT_THREADS, QUANT_KEYS, QUANT_MAX_TILE = 256, 64, 64               # the kernel's workgroup, rows per thread, widest column tile (csrc/quant.h)
QUANT_KEYS_OUT = ("quantiles", "quantile_draws")                      # what quantiles=probs adds to a sample_to result


# include/rmhmc_loo.h: PSIS leave-one-out cross-validation and WAIC from draws on the device, HIP library only as well
LOO_SIGNATURES = {
    "rmhmc_loo_loglik_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, C.c_int32, _vp]),
    "rmhmc_loo_moments_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _vp]),
    "rmhmc_loo_plan": (C.c_int, [_lp, C.c_int32, _lp, _lp]),
    "rmhmc_loo_split_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, _lp, C.c_int64, _vp, _vp, _vp]),
    "rmhmc_loo_fit_dev": (C.c_int, [C.c_void_p, _vp, _vp, _dp, _dp, _lp, C.c_int64, C.c_int32, _vp]),
    "rmhmc_loo_finish": (C.c_int, [_dpp, C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _lp, _lp]),
    "rmhmc_loo_dev": (C.c_int, [C.c_void_p, _vp, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp,
                                _dp, _dp, _dp, _dp, _lp, _lp]),
}
LOO_MAX_COLS, LOO_MAX_TAIL, LOO_MAX_D = 64, 16384, 256     # RMHMC_LOO_MAX_COLS, RMHMC_LOO_MAX_TAIL; widest draw
LOO_POINTWISE = ("elpd_loo", "p_loo", "pareto_k", "lppd", "p_waic", "elpd_waic")           # the [C] outputs of loo_finish, in its order
LOO_TOTALS = ("elpd_loo", "se_elpd_loo", "p_loo", "elpd_waic", "se_elpd_waic", "p_waic")   # its totals [6]


def quant_tile(P):
    """(column tile, rows of a workgroup's row block) of the histogram kernel at P columns: quant_tile_width and quant_block_rows of
    csrc/quant.h"""
    tw = 1
    while tw < int(P) and tw < QUANT_MAX_TILE:
        tw *= 2
    return tw, QUANT_THREADS // tw * QUANT_KEYS


def quant_probs(probs):
    """probs as the float64 vector the quantile calls take: one probability or a sequence of them, each in [0, 1].  ValueError otherwise."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if p.ndim != 1 or p.size < 1 or not ((p >= 0.0) & (p <= 1.0)).all():
        raise ValueError("quantiles: probabilities in [0, 1] required, at least one")
    return np.ascontiguousarray(p)


# the optional headers: key (RmhmcLib.has_<key>, RmhmcLib.need(key)) -> (the header's signatures, what it is called in the "does not
# export ..." message).  A library has a feature when it exports every symbol of the header.
FEATURES = {
    "amh": (AMH_SIGNATURES, "the AMH sampler (include/rmhmc_amh.h)"),
    "iwls": (IWLS_SIGNATURES, "the IWLS sampler (include/rmhmc_iwls.h)"),
    "gibbs": (GIBBS_SIGNATURES, "the Gibbs sampler (include/rmhmc_gibbs.h)"),
    "out": (OUT_SIGNATURES, "the output descriptor (include/rmhmc_out.h)"),
    "diag": (DIAG_SIGNATURES, "the cross-chain diagnostics (include/rmhmc_diag.h)"),
    "phmc": (PHMC_SIGNATURES, "the fixed-metric HMC sampler (include/rmhmc_phmc.h)"),
    "adapt": (ADAPT_SIGNATURES, "the warm-up of the fixed-metric HMC sampler (include/rmhmc_adapt.h)"),
    "ais": (AIS_SIGNATURES, "annealed importance sampling (include/rmhmc_ais.h)"),
    "pred": (PRED_SIGNATURES, "the posterior predictive probabilities (include/rmhmc_pred.h)"),
    "smc": (SMC_SIGNATURES, "adaptive sequential Monte Carlo (include/rmhmc_smc.h)"),
    "quant": (QUANT_SIGNATURES, "the posterior quantiles (include/rmhmc_quant.h)"),
    "loo": (LOO_SIGNATURES, "leave-one-out cross-validation (include/rmhmc_loo.h)"),
}


def ais_schedule(n_temps, ladder="power4", mass_every=1, iters_per_temp=1):
    """(beta [T], stage_len [T], stage_mass [T]) of an annealing run of T = n_temps stages (csrc/ais.h): ladder "power<q>" is
    beta_k = ((k + 1) / T)^q, "log<b>" the log-spaced beta_k = b^(1 - (k + 1) / T) with 0 < b < 1 ("log" alone: b = 1e-6); the last
    beta is exactly 1.  stage_mass: 1 every mass_every stages and in the first and the last; mass_every None: no stage installs a mass
    (stage_mass is None).  ValueError for T < 1, an unknown ladder, mass_every < 1 or iters_per_temp < 1."""
    T, K = int(n_temps), int(iters_per_temp)
    if T != n_temps or T < 1:
        raise ValueError("n_temps must be a number of stages >= 1")
    if K != iters_per_temp or K < 1:
        raise ValueError("iters_per_temp must be >= 1")
    if not isinstance(ladder, str) or not (ladder.startswith("power") or ladder.startswith("log")):
        raise ValueError('ladder must be "power<q>" or "log<beta_min>"')
    frac = (np.arange(T, dtype=np.float64) + 1.0) / float(T)
    try:
        if ladder.startswith("power"):
            q = float(ladder[5:])
            if not (np.isfinite(q) and q > 0.0):
                raise ValueError
            beta = np.array([math.pow(f, q) for f in frac])
        else:
            b = float(ladder[3:]) if len(ladder) > 3 else 1e-6
            if not 0.0 < b < 1.0:
                raise ValueError
            beta = np.array([math.exp(math.log(b) * (1.0 - f)) for f in frac])
    except ValueError:
        raise ValueError('ladder must be "power<q>" with q > 0 or "log<beta_min>" with 0 < beta_min < 1') from None
    beta[-1] = 1.0
    stage_mass = None
    if mass_every is not None:
        if int(mass_every) != mass_every or mass_every < 1:
            raise ValueError("mass_every must be None or a number of stages >= 1")
        k = np.arange(T)
        stage_mass = ((k % int(mass_every) == 0) | (k == T - 1)).astype(np.int32)
    return beta, np.full(T, K, dtype=np.int64), stage_mass


def adapt_schedule(warmup, window=25):
    """(win_len, win_kind) of a warm-up of `warmup` iterations in W = warmup // window windows of `window` iterations (what is left over
    is not run): the first max(1, round(0.15 W)) and the last max(1, round(0.1 W)) windows adapt the step size alone (kind 0), those
    between them the step size and the mass (kind 1); halves round up (integer arithmetic, as adapt_schedule of csrc/adapt.h).
    ValueError for W < 3."""
    warmup, window = int(warmup), int(window)
    if window < 1:
        raise ValueError("window must be >= 1")
    W = warmup // window
    if W < 3:
        raise ValueError("a warm-up needs at least 3 windows: warmup >= 3 * window")
    head = max(1, (15 * W + 50) // 100)
    tail = max(1, (10 * W + 50) // 100)
    kind = np.array([0 if (w < head or w >= W - tail) else 1 for w in range(W)], dtype=np.int32)
    return np.full(W, window, dtype=np.int64), kind


def diag_lags(S, max_lag=None):
    """(H, T) of a diagnostics call on S samples per chain: H = S // 2 rows per half chain, T = max_lag + 1 lags; max_lag None or 0:
    every lag, H - 1.  ValueError outside what rmhmc_diag_partial_dev accepts."""
    S = int(S)
    if not DIAG_S_MIN <= S <= DIAG_S_MAX:
        raise ValueError("diagnostics need %d <= S <= %d samples per chain (the centred series is held in LDS)" % (DIAG_S_MIN, DIAG_S_MAX))
    H = S // 2
    max_lag = 0 if max_lag is None else int(max_lag)
    if not 0 <= max_lag <= H - 1:
        raise ValueError("max_lag must be None or 0 (every lag) or 1 .. S // 2 - 1")
    return H, (max_lag if max_lag else H - 1) + 1


def ess_flags(ess_nfft):
    """context flags of the FFT-length convention of the device ESS: "matlab" (no wrap, the default) or "python" (tools.py:23)"""
    if ess_nfft not in ("matlab", "python"):
        raise ValueError('ess_nfft must be "matlab" or "python"')
    return FLAG_ESS_WRAP if ess_nfft == "python" else 0


class RmhmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rmhmc error %d: %s" % (code, msg))
        self.code = code


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a, typ=_dp):
    return None if a is None else a.ctypes.data_as(typ)


class RmhmcLib:
    """A loaded library exporting the rmhmc C-ABI."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError("rmhmc library not built: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
        self.path = path
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        self._bind(SIGNATURES)   # AttributeError if a declared symbol is missing
        for key, (sigs, _) in FEATURES.items():
            has = all(hasattr(self.lib, name) for name in sigs)
            setattr(self, "has_" + key, has)
            if has:
                self._bind(sigs)
        # the HIP library writes its _dev outputs through device pointers of its own GPU; the CPU oracle's "device" is the host
        self.on_gpu = "gfx950" in self.version()

    def _bind(self, sigs):
        for name, (res, args) in sigs.items():
            fn = getattr(self.lib, name)
            fn.restype = res
            fn.argtypes = args

    def need(self, key):
        """RmhmcError -4 unless the library has the optional feature `key` of FEATURES"""
        if not getattr(self, "has_" + key):
            raise RmhmcError(-4, "%s does not export %s" % (self.path, FEATURES[key][1]))

    def ck(self, rc):
        """RmhmcError from a failed call that has no context (rmhmc_last_error(NULL))"""
        if rc != 0:
            raise RmhmcError(rc, self.lib.rmhmc_last_error(None).decode())

    def version(self):
        return self.lib.rmhmc_version().decode()

    def context(self, M, D, n_chains=1, flags=COMPAT, device=0, options=None):
        """options: dict of the tuning options of include/rmhmc.h (rmhmc_create_opts), e.g. {"graph": 0, "medium": 0}"""
        return Context(self, M, D, n_chains, flags, device, options)


class Context:
    """One opaque rmhmc_ctx: M data rows, D dims, n_chains chains on one device."""

    def __init__(self, rl, M, D, n_chains, flags, device, options=None):
        self.rl, self.lib = rl, rl.lib
        self.M, self.D, self.n, self.flags = int(M), int(D), int(n_chains), int(flags)
        self.device = int(device)
        self._h = C.c_void_p()
        if options:
            arr = (Option * len(options))(*[Option(str(k).encode(), int(v)) for k, v in options.items()])
            rc = self.lib.rmhmc_create_opts(C.byref(self._h), device, self.M, self.D, self.n, F64, self.flags, arr, len(options))
        else:
            rc = self.lib.rmhmc_create(C.byref(self._h), device, self.M, self.D, self.n, F64, self.flags)
        rl.ck(rc)

    def close(self):
        if self._h:
            self.lib.rmhmc_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RmhmcError(rc, self.lib.rmhmc_last_error(self._h).decode())

    def device_info(self):
        buf = C.create_string_buffer(1024)
        self._ck(self.lib.rmhmc_device_info(self._h, buf, 1024))
        return buf.value.decode()

    def set_option(self, key, value):
        """a run-time tuning option (include/rmhmc.h); create-time ones go to ``context(..., options={...})``"""
        self._ck(self.lib.rmhmc_set_option(self._h, str(key).encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._ck(self.lib.rmhmc_get_option(self._h, str(key).encode(), C.cast(C.byref(v), _lp)))
        return v.value

    def options(self):
        """the active option set as a dict (empty for the CPU oracle)"""
        buf = C.create_string_buffer(1024)
        self._ck(self.lib.rmhmc_options(self._h, buf, 1024))
        return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split())}

    def set_data(self, XX, t, alpha=100.0):
        XX = _f64(XX)
        t = _f64(t).ravel()
        if XX.shape != (self.M, self.D) or t.shape != (self.M,):
            raise ValueError("XX must be (%d,%d) and t (%d,)" % (self.M, self.D, self.M))
        self._ck(self.lib.rmhmc_set_data(self._h, _ptr(XX), _ptr(t), float(alpha)))

    # ---- unit entry points -------------------------------------------------
    def log_posterior(self, w):
        w = _f64(w, (self.n, self.D))
        out = np.empty(self.n)
        self._ck(self.lib.rmhmc_log_posterior(self._h, _ptr(w), _ptr(out)))
        return out

    def metric(self, w):
        w = _f64(w, (self.n, self.D))
        G = np.empty((self.n, self.D, self.D)); hld = np.empty(self.n); g = np.empty((self.n, self.D))
        self._ck(self.lib.rmhmc_metric(self._h, _ptr(w), _ptr(G), _ptr(hld), _ptr(g)))
        return G, hld, g

    def metric_terms(self, w, p=None):
        w = _f64(w, (self.n, self.D))
        tr = np.empty((self.n, self.D))
        q = None
        if p is not None:
            p = _f64(p, (self.n, self.D))
            q = np.empty((self.n, self.D))
        self._ck(self.lib.rmhmc_metric_terms(self._h, _ptr(w), _ptr(p), _ptr(tr), _ptr(q)))
        return tr, q

    def leapfrog(self, w, p, eps, direction, nsteps, K=4):
        w = _f64(w, (self.n, self.D)).copy(); p = _f64(p, (self.n, self.D)).copy()
        d = np.ascontiguousarray(np.broadcast_to(direction, (self.n,)), dtype=np.int32)
        ns = np.ascontiguousarray(np.broadcast_to(nsteps, (self.n,)), dtype=np.int32)
        hld = np.empty(self.n); st = np.zeros(self.n, dtype=np.int32)
        self._ck(self.lib.rmhmc_leapfrog(self._h, _ptr(w), _ptr(p), float(eps), _ptr(d, _ip), _ptr(ns, _ip), int(K),
                                         _ptr(hld), _ptr(st, _ip)))
        return w, p, hld, st

    def transition(self, w, z, u_len, g_dir, u_acc, L=6, eps=0.5, K=4):
        n, D = self.n, self.D
        w = _f64(w, (n, D)).copy()
        z = _f64(z, (n, D)); u_len = _f64(u_len, (n,)); g_dir = _f64(g_dir, (n,)); u_acc = _f64(u_acc, (n,))
        acc = np.zeros(n, dtype=np.int32); ns = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        Hc = np.empty(n); Hp = np.empty(n); wp = np.empty((n, D)); pp = np.empty((n, D)); hp = np.empty(n)
        self._ck(self.lib.rmhmc_transition(self._h, _ptr(w), _ptr(z), _ptr(u_len), _ptr(g_dir), _ptr(u_acc), int(L),
                                           float(eps), int(K), _ptr(acc, _ip), _ptr(ns, _ip), _ptr(Hc), _ptr(Hp),
                                           _ptr(wp), _ptr(pp), _ptr(hp), _ptr(st, _ip)))
        return dict(w=w, accepted=acc, nsteps=ns, H_cur=Hc, H_prop=Hp, w_prop=wp, p_prop=pp, hld_prop=hp, status=st)

    # ---- bulk entry points -------------------------------------------------
    def sample(self, n_iter, burn_in, L=6, eps=0.5, K=4, seed=0, chain_offset=0, theta0=None):
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        samples = np.empty((n, S, D)); acc = np.zeros(n, dtype=np.int64); steps = np.zeros(n, dtype=np.int64)
        secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_sample(self._h, int(n_iter), int(burn_in), int(L), float(eps), int(K), int(seed),
                                       int(chain_offset), _ptr(th), _ptr(samples), _ptr(acc, _lp), _ptr(steps, _lp),
                                       C.cast(C.byref(secs), _dp)))
        return samples, acc, steps, secs.value

    # ---- ESS on the device (tools.py:32-74) -----------------------------------
    def ess(self, samples):
        samples = _f64(samples)
        if samples.ndim == 2:
            samples = samples[None]
        n, S, P = samples.shape
        out = np.empty((n, P))
        self._ck(self.lib.rmhmc_ess(self._h, _ptr(samples), n, S, P, _ptr(out)))
        return out

    def sample_stats(self, n_iter, burn_in, L=6, eps=0.5, K=4, seed=0, chain_offset=0, theta0=None, run_mean=False):
        if run_mean:  # (include/rmhmc_out.h)
            return self.sample_to("rmhmc", n_iter, burn_in, stats=True, run_mean=True, L=L, eps=eps, K=K, seed=seed,
                                  chain_offset=chain_offset, theta0=theta0)
        n, D = self.n, self.D
        if int(n_iter) - int(burn_in) <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        mean = np.empty((n, D)); var = np.empty((n, D)); ess = np.empty((n, D))
        acc = np.zeros(n, dtype=np.int64); steps = np.zeros(n, dtype=np.int64)
        secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_sample_stats(self._h, int(n_iter), int(burn_in), int(L), float(eps), int(K), int(seed),
                                             int(chain_offset), _ptr(th), _ptr(mean), _ptr(var), _ptr(ess), _ptr(acc, _lp),
                                             _ptr(steps, _lp), C.cast(C.byref(secs), _dp)))
        return dict(mean=mean, var=var, ess=ess, accepted=acc, leapfrog_steps=steps, seconds=secs.value)

    # ---- device-resident write-out: outputs are torch tensors on the context's GPU (host tensors for the CPU oracle) ----------
    def _out_tensors(self, shapes, device):
        """device: a torch.device.  The HIP library writes through device pointers on its own GPU; the oracle's "device" is the host."""
        import torch
        return [torch.empty(shape, dtype=dt, device=device) for shape, dt in shapes]

    def _dev_tensor(self, who, x, what, rank=None, dtype=None):
        """x as the contiguous torch tensor a <name>_dev entry point reads: on the context's GPU (anywhere for the CPU oracle), of
        `dtype` (float64 unless it says otherwise) and of `rank` dimensions (None: any), a vector not empty.  ValueError "<who>: <dtype>
        tensor<what> required" otherwise.  torch's current stream on the tensor's device is synchronised: the library reads the tensor
        at once on a stream of its own, so whatever produced it must have finished."""
        import torch
        dtype = dtype or torch.float64
        if self.rl.on_gpu and not x.is_cuda:
            raise ValueError("%s: a tensor on the context's GPU is required" % who)
        x = x.contiguous()
        if x.dtype != dtype or (rank is not None and x.dim() != rank) or (rank == 1 and x.numel() < 1):
            raise ValueError("%s: %s tensor%s required" % (who, str(dtype).replace("torch.", ""), what))
        if x.is_cuda:
            torch.cuda.current_stream(x.device).synchronize()
        return x

    def chains_state_dev(self, device):
        import torch
        w, it, acc = self._out_tensors([((self.n, self.D), torch.float64), ((self.n,), torch.int64), ((self.n,), torch.int64)], device)
        self._ck(self.lib.rmhmc_chains_state_dev(self._h, w.data_ptr(), it.data_ptr(), acc.data_ptr()))
        return w, it, acc

    def sample_dev(self, device, n_iter, burn_in, L=6, eps=0.5, K=4, seed=0, chain_offset=0, theta0=None):
        import torch
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        smp, acc, steps = self._out_tensors([((n, S, D), torch.float64), ((n,), torch.int64), ((n,), torch.int64)], device)
        secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_sample_dev(self._h, int(n_iter), int(burn_in), int(L), float(eps), int(K), int(seed), int(chain_offset),
                                           _ptr(th), smp.data_ptr(), acc.data_ptr(), steps.data_ptr(), C.cast(C.byref(secs), _dp)))
        return smp, acc, steps, secs.value

    def sample_stats_dev(self, device, n_iter, burn_in, L=6, eps=0.5, K=4, seed=0, chain_offset=0, theta0=None, run_mean=False):
        if run_mean:  # (include/rmhmc_out.h)
            return self.sample_to("rmhmc", n_iter, burn_in, where="device", device=device, stats=True, run_mean=True, L=L, eps=eps, K=K,
                                  seed=seed, chain_offset=chain_offset, theta0=theta0)
        import torch
        n, D = self.n, self.D
        if int(n_iter) - int(burn_in) <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        mean, var, ess, acc, steps = self._out_tensors([((n, D), torch.float64)] * 3 + [((n,), torch.int64)] * 2, device)
        secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_sample_stats_dev(self._h, int(n_iter), int(burn_in), int(L), float(eps), int(K), int(seed), int(chain_offset),
                                                 _ptr(th), mean.data_ptr(), var.data_ptr(), ess.data_ptr(), acc.data_ptr(), steps.data_ptr(),
                                                 C.cast(C.byref(secs), _dp)))
        return dict(mean=mean, var=var, ess=ess, accepted=acc, leapfrog_steps=steps, seconds=secs.value)

    # ---- simplified mMALA (authors_code/.../BLR_mMALA_Simp.m) -------------------
    def mmala_transition(self, w, z, u_acc, eps=1.0):
        n, D = self.n, self.D
        w = _f64(w, (n, D)).copy(); z = _f64(z, (n, D)); u_acc = _f64(u_acc, (n,))
        acc = np.zeros(n, dtype=np.int32); ratio = np.empty(n); wp = np.empty((n, D))
        self._ck(self.lib.rmhmc_mmala_transition(self._h, _ptr(w), _ptr(z), _ptr(u_acc), float(eps), _ptr(acc, _ip), _ptr(ratio), _ptr(wp)))
        return dict(w=w, accepted=acc, ratio=ratio, w_prop=wp)

    def mmala_sample(self, n_iter, burn_in, eps=1.0, seed=0, chain_offset=0, theta0=None):
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        samples = np.empty((n, S, D)); acc = np.zeros(n, dtype=np.int64); secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_mmala_sample(self._h, int(n_iter), int(burn_in), float(eps), int(seed), int(chain_offset), _ptr(th),
                                             _ptr(samples), _ptr(acc, _lp), C.cast(C.byref(secs), _dp)))
        return samples, acc, secs.value

    # ---- plain HMC (code/hmc.py) ---------------------------------------------
    def hmc_transition(self, w, z, u_len, u_acc, L=100, eps=0.14):
        n, D = self.n, self.D
        w = _f64(w, (n, D)).copy()
        z = _f64(z, (n, D)); u_len = _f64(u_len, (n,)); u_acc = _f64(u_acc, (n,))
        acc = np.zeros(n, dtype=np.int32); ns = np.zeros(n, dtype=np.int32)
        Hc = np.empty(n); Hp = np.empty(n); wp = np.empty((n, D)); pp = np.empty((n, D))
        self._ck(self.lib.rmhmc_hmc_transition(self._h, _ptr(w), _ptr(z), _ptr(u_len), _ptr(u_acc), int(L), float(eps),
                                               _ptr(acc, _ip), _ptr(ns, _ip), _ptr(Hc), _ptr(Hp), _ptr(wp), _ptr(pp)))
        return dict(w=w, accepted=acc, nsteps=ns, H_cur=Hc, H_prop=Hp, w_prop=wp, p_prop=pp)

    def hmc_sample(self, n_iter, burn_in, L=100, eps=0.14, seed=0, chain_offset=0, theta0=None):
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0:
            raise ValueError("BurnIn must be < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        samples = np.empty((n, S, D)); acc = np.zeros(n, dtype=np.int64); steps = np.zeros(n, dtype=np.int64)
        secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_hmc_sample(self._h, int(n_iter), int(burn_in), int(L), float(eps), int(seed),
                                           int(chain_offset), _ptr(th), _ptr(samples), _ptr(acc, _lp), _ptr(steps, _lp),
                                           C.cast(C.byref(secs), _dp)))
        return samples, acc, steps, secs.value

    # ---- HMC with a fixed dense mass matrix shared by all chains (include/rmhmc_phmc.h) -----------
    def phmc_set_mass(self, mass=None):
        """the context's mass matrix: (D, D) symmetric positive definite (the lower triangle is read), None: the identity"""
        self.rl.need("phmc")
        m = None if mass is None else _f64(mass, (self.D, self.D))
        self._ck(self.lib.rmhmc_phmc_set_mass(self._h, _ptr(m)))

    def phmc_mode(self, w0=None, max_iter=50, tol=1e-10):
        """posterior mode by damped Newton from w0 (None: zeros): dict(w [D], G [D][D] the metric at w, iters, step: max|s| of the
        last Newton step, converged: step <= tol * max(1, max|w|))"""
        self.rl.need("phmc")
        D = self.D
        w0 = None if w0 is None else _f64(w0, (D,))
        w = np.empty(D); G = np.empty((D, D))
        iters = C.c_int32(0); step = C.c_double(0.0)
        self._ck(self.lib.rmhmc_phmc_mode(self._h, _ptr(w0), int(max_iter), float(tol), _ptr(w), _ptr(G), C.cast(C.byref(iters), _ip),
                                          C.cast(C.byref(step), _dp)))
        return dict(w=w, G=G, iters=iters.value, step=step.value,
                    converged=bool(step.value <= float(tol) * max(1.0, float(np.abs(w).max()))))

    def phmc_transition(self, w, z, u_len, u_acc, L=6, eps=0.5):
        self.rl.need("phmc")
        n, D = self.n, self.D
        w = _f64(w, (n, D)).copy()
        z = _f64(z, (n, D)); u_len = _f64(u_len, (n,)); u_acc = _f64(u_acc, (n,))
        acc = np.zeros(n, dtype=np.int32); ns = np.zeros(n, dtype=np.int32); status = np.zeros(n, dtype=np.int32)
        Hc = np.empty(n); Hp = np.empty(n); wp = np.empty((n, D)); pp = np.empty((n, D))
        self._ck(self.lib.rmhmc_phmc_transition(self._h, _ptr(w), _ptr(z), _ptr(u_len), _ptr(u_acc), int(L), float(eps),
                                                _ptr(acc, _ip), _ptr(ns, _ip), _ptr(Hc), _ptr(Hp), _ptr(wp), _ptr(pp), _ptr(status, _ip)))
        return dict(w=w, accepted=acc, nsteps=ns, H_cur=Hc, H_prop=Hp, w_prop=wp, p_prop=pp, status=status)

    def phmc_sample_to(self, n_iter, burn_in, L=6, eps=0.5, *, where="host", device=None, samples=False, stats=False, run_mean=False,
                       seed=0, chain_offset=0, theta0=None):
        """One run of the sampler with the context's mass matrix, written out as sample_to writes the others: the requested outputs,
        the counters accepted and leapfrog_steps (same memory space) and seconds."""
        self.rl.need("phmc")
        self.rl.need("out")
        return self._call_sample_to("rmhmc_phmc_sample_to", PHMC_COUNTERS, (int(L), float(eps)), n_iter, burn_in, where, device, samples,
                                    stats, run_mean, seed, chain_offset, theta0)

    # ---- warm-up of the fixed-metric HMC sampler (include/rmhmc_adapt.h) -----------
    def cov_partial(self, samples):
        """The mergeable partial [(2 + P), P] (include/rmhmc_adapt.h) of a float64 torch tensor [n][S][P] already on the context's GPU,
        reduced there.  torch's current stream is synchronised first, as in ess_dev."""
        import torch
        self.rl.need("adapt")
        x = self._dev_tensor("cov_partial", samples, " [n][S][P]", 3)
        n, S, P = x.shape
        part = torch.empty((2 + P, P), dtype=torch.float64, device=x.device)
        self._ck(self.lib.rmhmc_cov_partial_dev(self._h, x.data_ptr(), n, S, P, part.data_ptr()))
        return part

    def pooled_cov(self, samples):
        """pooled mean and covariance of the rows of samples [n][S][P] on the context's GPU (rows with a non-finite entry left out):
        dict(mean [P], cov [P][P], rows_used: host; partial: the device tensor of cov_partial)"""
        part = self.cov_partial(samples)
        out = cov_finish([part], lib=self.rl)
        return dict(mean=out["mean"], cov=out["cov"], rows_used=out["rows_used"], partial=part)

    def phmc_warmup(self, win_len, win_kind, L=6, eps0=0.5, *, min_rows=None, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, seed=0,
                    chain_offset=0, theta0=None):
        """The windowed warm-up of phmc_sample_to (rmhmc_phmc_warmup) from the context's mass and eps0: window w runs win_len[w]
        iterations and adapts the step size (win_kind[w] = 0) or the step size and then the mass (1; adapt_schedule builds the usual
        schedule).  min_rows: pooled rows a mass update needs, default 10 D.  Returns dict(step_size, mass [D][D] or None when no
        update happened, theta [n][D] the last positions, eps_trace, accept_trace, mass_updated [W], seconds).  The context is left
        with the adapted mass."""
        self.rl.need("adapt")
        n, D = self.n, self.D
        wl = np.ascontiguousarray(win_len, dtype=np.int64).reshape(-1)
        wk = np.ascontiguousarray(win_kind, dtype=np.int32).reshape(-1)
        if wl.shape != wk.shape or wl.size < 1:
            raise ValueError("phmc_warmup: win_len and win_kind of one length W >= 1 required")
        W = wl.size
        min_rows = 10 * D if min_rows is None else int(min_rows)
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        eps = C.c_double(0.0); secs = C.c_double(0.0)
        mass = np.empty((D, D)); theta = np.empty((n, D))
        eps_trace = np.empty(W); acc_trace = np.empty(W); upd = np.zeros(W, dtype=np.int32)
        self._ck(self.lib.rmhmc_phmc_warmup(self._h, _ptr(th), int(L), float(eps0), float(delta), float(gamma), float(t0), float(kappa),
                                            int(seed) % 2 ** 64, int(chain_offset), W, _ptr(wl, _lp), _ptr(wk, _ip), min_rows,
                                            C.cast(C.byref(eps), _dp), _ptr(mass), _ptr(theta), _ptr(eps_trace), _ptr(acc_trace),
                                            _ptr(upd, _ip), C.cast(C.byref(secs), _dp)))
        return dict(step_size=eps.value, mass=mass if (upd == 1).any() else None, theta=theta, eps_trace=eps_trace,
                    accept_trace=acc_trace, mass_updated=upd, seconds=secs.value)

    # ---- annealed importance sampling with tempered fixed-metric HMC (include/rmhmc_ais.h) -----------
    def tphmc_transition(self, w, z, u_len, u_acc, L=6, eps=0.5, beta=1.0):
        """phmc_transition on the target tempered by beta; the dict gains loglik0 (at the start) and loglik (at the returned w)"""
        self.rl.need("ais")
        n, D = self.n, self.D
        w = _f64(w, (n, D)).copy()
        z = _f64(z, (n, D)); u_len = _f64(u_len, (n,)); u_acc = _f64(u_acc, (n,))
        acc = np.zeros(n, dtype=np.int32); ns = np.zeros(n, dtype=np.int32); status = np.zeros(n, dtype=np.int32)
        Hc = np.empty(n); Hp = np.empty(n); wp = np.empty((n, D)); pp = np.empty((n, D)); ll0 = np.empty(n); ll = np.empty(n)
        self._ck(self.lib.rmhmc_tphmc_transition(self._h, _ptr(w), _ptr(z), _ptr(u_len), _ptr(u_acc), int(L), float(eps), _ptr(acc, _ip),
                                                 _ptr(ns, _ip), _ptr(Hc), _ptr(Hp), _ptr(wp), _ptr(pp), _ptr(status, _ip), float(beta),
                                                 _ptr(ll0), _ptr(ll)))
        return dict(w=w, accepted=acc, nsteps=ns, H_cur=Hc, H_prop=Hp, w_prop=wp, p_prop=pp, status=status, loglik0=ll0, loglik=ll)

    def tphmc_sample_to(self, n_iter, burn_in, L=6, eps=0.5, beta=1.0, *, where="host", device=None, samples=False, stats=False,
                        run_mean=False, seed=0, chain_offset=0, theta0=None):
        """phmc_sample_to on the target tempered by beta (the power posterior p(t|w)^beta p(w)); the result gains loglik0 [n] (the
        log-likelihood at theta0) and loglik [n] (at the last state), host arrays whatever `where` says"""
        self.rl.need("ais")
        self.rl.need("out")
        ll0 = np.empty(self.n); ll = np.empty(self.n)
        res = self._call_sample_to("rmhmc_tphmc_sample_to", PHMC_COUNTERS, (int(L), float(eps)), n_iter, burn_in, where, device, samples,
                                   stats, run_mean, seed, chain_offset, theta0, back=(float(beta), _ptr(ll0), _ptr(ll)))
        res["loglik0"], res["loglik"] = ll0, ll
        return res

    def ais_prior(self, seed=0, chain_offset=0):
        """exact draws from the prior N(0, alpha I), [n][D]: the start of an annealing run"""
        self.rl.need("ais")
        th = np.empty((self.n, self.D))
        self._ck(self.lib.rmhmc_ais_prior(self._h, int(seed) % 2 ** 64, int(chain_offset), _ptr(th)))
        return th

    def ais_partial(self, logw):
        """The mergeable partial [5] = (m, n_nan, max, S1, S2) (include/rmhmc_ais.h) of a float64 torch tensor [n] of log weights already
        on the context's GPU, reduced there.  torch's current stream is synchronised first, as in ess_dev."""
        import torch
        self.rl.need("ais")
        x = self._dev_tensor("ais_partial", logw, " [n], n >= 1,", 1)
        part = torch.empty(5, dtype=torch.float64, device=x.device)
        self._ck(self.lib.rmhmc_ais_partial_dev(self._h, x.data_ptr(), x.numel(), part.data_ptr()))
        return part

    def ais_run(self, beta, stage_len, stage_mass=None, H_lik=None, L=6, eps=0.5, *, beta0=0.0, seed=0, chain_offset=0, theta0=None):
        """rmhmc_ais_run: stage k installs the mass beta[k] H_lik + I / alpha where stage_mass[k] is 1, runs stage_len[k] tempered
        iterations at beta[k] from the last positions and adds (beta[k] - beta[k - 1]) loglik0 to logw; theta0 None: the chains start
        from the prior (beta0 must be 0).  ais_schedule builds the usual (beta, stage_len, stage_mass).  Returns dict(logw [n], theta
        [n][D] the last positions, accept_trace [T], partial [5], seconds, and the AIS_KEYS of ais_finish on the partial).  The context
        is left with the last mass installed."""
        self.rl.need("ais")
        n, D = self.n, self.D
        b = _f64(beta).reshape(-1)
        sl = np.ascontiguousarray(stage_len, dtype=np.int64).reshape(-1)
        sm = None if stage_mass is None else np.ascontiguousarray(stage_mass, dtype=np.int32).reshape(-1)
        if b.size < 1 or sl.shape != b.shape or (sm is not None and sm.shape != b.shape):
            raise ValueError("ais_run: beta, stage_len and stage_mass of one length T >= 1 required")
        H = None if H_lik is None else _f64(H_lik, (D, D))
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        logw = np.empty(n); theta = np.empty((n, D)); trace = np.empty(b.size); part = np.empty(5); secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_ais_run(self._h, _ptr(th), float(beta0), b.size, _ptr(b), _ptr(sl, _lp), _ptr(sm, _ip), _ptr(H), int(L),
                                        float(eps), int(seed) % 2 ** 64, int(chain_offset), _ptr(logw), _ptr(theta), _ptr(trace),
                                        _ptr(part), C.cast(C.byref(secs), _dp)))
        out = dict(logw=logw, theta=theta, accept_trace=trace, partial=part, seconds=secs.value)
        out.update(ais_finish([part], lib=self.rl))
        return out

    # ---- the evidence by adaptive sequential Monte Carlo (include/rmhmc_smc.h) -----------
    def _smc_vec(self, who, x, dtype=None):
        return self._dev_tensor(who, x, " [n], n >= 1,", 1, dtype)

    def smc_cess(self, logw, loglik, delta):
        """The mergeable conditional-ESS partial [2 + 4 J] = (a0, S0, then per candidate a1, S1, a2, S2) (include/rmhmc_smc.h) of the log
        weights and log-likelihoods (float64 torch tensors [n] on the context's GPU) at the J <= 32 candidate steps delta (host)."""
        import torch
        self.rl.need("smc")
        lw, ll = self._smc_vec("smc_cess", logw), self._smc_vec("smc_cess", loglik)
        d = _f64(delta).reshape(-1)
        if ll.shape != lw.shape or not 1 <= d.size <= SMC_MAX_J:
            raise ValueError("smc_cess: logw and loglik of one length and 1 .. %d candidates required" % SMC_MAX_J)
        part = torch.empty(2 + 4 * d.size, dtype=torch.float64, device=lw.device)
        self._ck(self.lib.rmhmc_smc_cess_dev(self._h, lw.data_ptr(), ll.data_ptr(), lw.numel(), d.size, _ptr(d), part.data_ptr()))
        return part

    def smc_choose_delta(self, logw, loglik, remaining, rho):
        """the search for the next temperature step (include/rmhmc_smc.h section 2): dict(delta, frac, flags)"""
        self.rl.need("smc")
        lw, ll = self._smc_vec("smc_choose_delta", logw), self._smc_vec("smc_choose_delta", loglik)
        if ll.shape != lw.shape:
            raise ValueError("smc_choose_delta: logw and loglik of one length required")
        d = C.c_double(0.0); f = C.c_double(0.0); fl = C.c_int32(0)
        self._ck(self.lib.rmhmc_smc_choose_delta_dev(self._h, lw.data_ptr(), ll.data_ptr(), lw.numel(), float(remaining), float(rho),
                                                     C.cast(C.byref(d), _dp), C.cast(C.byref(f), _dp), C.cast(C.byref(fl), _ip)))
        return dict(delta=d.value, frac=f.value, flags=fl.value)

    def smc_reweight(self, logw, loglik, delta):
        """logw += delta loglik in place where loglik is finite, -inf where it is not (NaN stays); returns logw"""
        self.rl.need("smc")
        ll = self._smc_vec("smc_reweight", loglik)
        if not logw.is_contiguous() or self._smc_vec("smc_reweight", logw).shape != ll.shape:
            raise ValueError("smc_reweight: contiguous logw and loglik of one length required")
        self._ck(self.lib.rmhmc_smc_reweight_dev(self._h, logw.data_ptr(), ll.data_ptr(), logw.numel(), float(delta)))
        return logw

    def smc_quantise(self, logw, a):
        """q [n] (int64 tensor holding the uint64 values, all <= 2^40) = floor(2^40 exp(min(logw - a, 0))), 0 for NaN and -inf"""
        import torch
        self.rl.need("smc")
        lw = self._smc_vec("smc_quantise", logw)
        q = torch.empty(lw.numel(), dtype=torch.int64, device=lw.device)
        self._ck(self.lib.rmhmc_smc_quantise_dev(self._h, lw.data_ptr(), lw.numel(), float(a), q.data_ptr()))
        return q

    def smc_ancestors(self, q, U, out=None):
        """anc [n] (int32 tensor) of systematic resampling on the integers q [n] (int64 tensor, entries 0 .. 2^40) with the 32-bit offset U
        (include/rmhmc_smc.h section 4); out: the tensor to write into"""
        import torch
        self.rl.need("smc")
        q = self._smc_vec("smc_ancestors", q, torch.int64)
        if int(U) != U or not 0 <= U < 2 ** 32:
            raise ValueError("smc_ancestors: U is a 32-bit unsigned")
        anc = out if out is not None else torch.empty(q.numel(), dtype=torch.int32, device=q.device)
        if anc.dtype != torch.int32 or anc.shape != q.shape or anc.device != q.device or not anc.is_contiguous():
            raise ValueError("smc_ancestors: out must be a contiguous int32 tensor [n] beside q")
        if anc.is_cuda:
            torch.cuda.current_stream(anc.device).synchronize()
        self._ck(self.lib.rmhmc_smc_ancestors_dev(self._h, q.data_ptr(), q.numel(), int(U), anc.data_ptr()))
        return anc

    def smc_run(self, rho=0.9, tau=0.5, T_max=10000, stage_len=1, mass_every=1, H_lik=None, L=6, eps=0.5, *, beta0=0.0, seed=0, chain_offset=0,
                theta0=None):
        """rmhmc_smc_run: the annealing of ais_run on a ladder chosen stage by stage so that the conditional ESS of the step is rho n,
        resampling (systematic, on integers) when the weight-ESS falls below tau n; mass_every 0: no stage installs a mass.  Returns
        dict(T, beta [T], cess [T], ess [T], flags [T], accept_trace [T], logw [n], theta [n][D], log_z (NaN if T_max stages did not
        reach beta = 1), se (NaN if a stage resampled), partial [5], seconds, and the AIS_KEYS of ais_finish on the partial)."""
        self.rl.need("smc")
        n, D = self.n, self.D
        if int(T_max) != T_max or not 1 <= T_max < 2 ** 31:
            raise ValueError("smc_run: T_max must be a number of stages >= 1")
        T_max = int(T_max)
        H = None if H_lik is None else _f64(H_lik, (D, D))
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        T = C.c_int32(0); lz = C.c_double(0.0); se = C.c_double(0.0); secs = C.c_double(0.0)
        beta = np.full(T_max, np.nan); cess = np.full(T_max, np.nan); ess = np.full(T_max, np.nan); trace = np.full(T_max, np.nan)
        flags = np.zeros(T_max, dtype=np.int32)
        logw = np.empty(n); theta = np.empty((n, D)); part = np.empty(5)
        self._ck(self.lib.rmhmc_smc_run(self._h, _ptr(th), float(beta0), float(rho), float(tau), T_max, int(stage_len), int(mass_every), _ptr(H),
                                        int(L), float(eps), int(seed) % 2 ** 64, int(chain_offset), C.cast(C.byref(T), _ip), _ptr(beta),
                                        _ptr(cess), _ptr(ess), _ptr(flags, _ip), _ptr(trace), _ptr(logw), _ptr(theta),
                                        C.cast(C.byref(lz), _dp), C.cast(C.byref(se), _dp), _ptr(part), C.cast(C.byref(secs), _dp)))
        k = T.value
        out = dict(T=k, beta=beta[:k].copy(), cess=cess[:k].copy(), ess=ess[:k].copy(), flags=flags[:k].copy(), accept_trace=trace[:k].copy(),
                   logw=logw, theta=theta, log_z=lz.value, partial=part, seconds=secs.value)
        out.update(ais_finish([part], lib=self.rl))
        out["se"] = se.value
        return out

    # ---- posterior predictive probabilities of new rows (include/rmhmc_pred.h) -----------
    def predict_partial(self, samples, xnew, tnew=None):
        """The mergeable partial [4, R] = (m, S1, S2, SQ) (include/rmhmc_pred.h) of the draws of a float64 torch tensor [n][S][D] already
        on the context's GPU for the rows xnew [R][D] (host) and the held-out labels tnew [R] (host, 0 or 1) or None, reduced there.
        torch's current stream is synchronised first, as in ess_dev."""
        import torch
        self.rl.need("pred")
        w = self._dev_tensor("predict_partial", samples, " [n][S][D]", 3)
        n, S, D = w.shape
        x = _f64(xnew)
        if x.ndim != 2 or x.shape[1] != D:
            raise ValueError("predict_partial: xnew must be (R, D) with the D of the samples")
        R = x.shape[0]
        t = None if tnew is None else _f64(tnew).reshape(-1)
        if t is not None and t.shape[0] != R:
            raise ValueError("predict_partial: tnew must have R entries")
        part = torch.empty((4, R), dtype=torch.float64, device=w.device)
        self._ck(self.lib.rmhmc_pred_partial_dev(self._h, w.data_ptr(), n, S, D, _ptr(x), _ptr(t), R, part.data_ptr()))
        return part

    def predict(self, samples, xnew, tnew=None):
        """posterior predictive probabilities of the rows xnew [R][D] under the draws samples [n][S][D] on the context's GPU (draws with
        a non-finite entry left out): dict(prob [R] = p(t* = 1 | x*, data), pvar [R] the variance of p over the draws, lpd [R] the log
        pointwise predictive density of tnew (NaN without labels), lpd_total, draws_used: host; partial: the device tensor of
        predict_partial)"""
        part = self.predict_partial(samples, xnew, tnew)
        out = pred_finish([part], lib=self.rl)
        res = {k: out[k] for k in PRED_KEYS}
        res["partial"] = part
        return res

    # ---- leave-one-out cross-validation (include/rmhmc_loo.h) -----------
    @staticmethod
    def _loo_rows(who, x, t, D):
        x = _f64(x)
        if x.ndim != 2 or x.shape[1] != D or x.shape[0] < 1:
            raise ValueError("%s: x must be (C, D) with the D of the samples" % who)
        t = _f64(t).reshape(-1)
        if t.shape[0] != x.shape[0]:
            raise ValueError("%s: t must have one entry per row of x" % who)
        return x, t

    def _loo_cut(self, who, cut, lmin, tail_len, C):
        cut, lmin = _f64(cut).reshape(-1), _f64(lmin).reshape(-1)
        tl = np.ascontiguousarray(tail_len, dtype=np.int64).reshape(-1)
        if not cut.size == lmin.size == tl.size == C:
            raise ValueError("%s: cut, lmin and tail_len must have one entry per column" % who)
        return cut, lmin, tl

    def loo_loglik(self, samples, x, t):
        """The log-likelihood matrix ll [n][S][C] (include/rmhmc_loo.h) of the C <= 64 data rows x [C][D], t [C] (host, 0 or 1) under the
        draws of a float64 torch tensor [n][S][D] already on the context's GPU, a tensor there.  torch's current stream is synchronised
        first, as in ess_dev."""
        import torch
        self.rl.need("loo")
        w = self._dev_tensor("loo_loglik", samples, " [n][S][D]", 3)
        n, S, D = w.shape
        x, t = self._loo_rows("loo_loglik", x, t, D)
        ll = torch.empty((n, S, x.shape[0]), dtype=torch.float64, device=w.device)
        self._ck(self.lib.rmhmc_loo_loglik_dev(self._h, w.data_ptr(), n, S, D, _ptr(x), _ptr(t), x.shape[0], ll.data_ptr()))
        return ll

    def loo_moments(self, ll):
        """The mergeable moments partial [5, C] = (m, mean, M2, SQ, lmin) of ll [n][S][C] on the context's GPU, a tensor there"""
        import torch
        self.rl.need("loo")
        ll = self._dev_tensor("loo_moments", ll, " [n][S][C]", 3)
        n, S, Cc = ll.shape
        part = torch.empty((5, Cc), dtype=torch.float64, device=ll.device)
        self._ck(self.lib.rmhmc_loo_moments_dev(self._h, ll.data_ptr(), n, S, Cc, part.data_ptr()))
        return part

    def loo_split(self, ll, cut, lmin, tail_len, stride=None):
        """The split of ll [n][S][C] at the cutoffs cut [C] (host; lmin [C], tail_len [C] of loo_plan): dict(tail [C][stride] (the first
        n_lt slots of a row hold the values below the cutoff, in no order), counts int64 [2, C] = (n_lt, n_gt), body [2, C] = (A_body,
        B_body)), tensors on the context's GPU.  stride: max(1, the longest tail) unless given."""
        import torch
        self.rl.need("loo")
        ll = self._dev_tensor("loo_split", ll, " [n][S][C]", 3)
        n, S, Cc = ll.shape
        cut, lmin, tl = self._loo_cut("loo_split", cut, lmin, tail_len, Cc)
        stride = max(1, int(tl.max())) if stride is None else int(stride)
        tail = torch.empty((Cc, max(stride, 1)), dtype=torch.float64, device=ll.device)
        counts = torch.empty((2, Cc), dtype=torch.int64, device=ll.device)
        body = torch.empty((2, Cc), dtype=torch.float64, device=ll.device)
        self._ck(self.lib.rmhmc_loo_split_dev(self._h, ll.data_ptr(), n, S, Cc, _ptr(cut), _ptr(lmin), _ptr(tl, _lp), stride, tail.data_ptr(),
                                              counts.data_ptr(), body.data_ptr()))
        return dict(tail=tail, counts=counts, body=body)

    def loo_fit(self, tail, counts, cut, lmin, tail_len):
        """The generalised Pareto fit of every column's tail (tail [C][stride], counts [2, C] of loo_split): fit [4, C] = (khat, sigma,
        A_tail, B_tail), a tensor on the context's GPU"""
        import torch
        self.rl.need("loo")
        tail = self._dev_tensor("loo_fit", tail, " [C][stride]", 2)
        counts = self._dev_tensor("loo_fit", counts, " [2][C]", 2, torch.int64)
        Cc, stride = tail.shape
        if tuple(counts.shape) != (2, Cc):
            raise ValueError("loo_fit: counts must be [2][C]")
        cut, lmin, tl = self._loo_cut("loo_fit", cut, lmin, tail_len, Cc)
        fit = torch.empty((4, Cc), dtype=torch.float64, device=tail.device)
        self._ck(self.lib.rmhmc_loo_fit_dev(self._h, tail.data_ptr(), counts.data_ptr(), _ptr(cut), _ptr(lmin), _ptr(tl, _lp), stride, Cc,
                                            fit.data_ptr()))
        return fit

    def loo(self, samples, x, t, cols_per_block=0):
        """PSIS-LOO and WAIC of the rows x [R][D], t [R] (host) under the draws samples [n][S][D] on the context's GPU (rmhmc_loo_dev), in
        blocks of cols_per_block columns (0: the library chooses).  Returns what loo_finish returns, with partial [5, R], fit [4, R] and
        body [2, R] (host) in place of merged."""
        self.rl.need("loo")
        w = self._dev_tensor("loo", samples, " [n][S][D]", 3)
        n, S, D = w.shape
        x, t = self._loo_rows("loo", x, t, D)
        R = x.shape[0]
        part = np.empty((5, R)); fit = np.empty((4, R)); body = np.empty((2, R))
        pw = [np.empty(R) for _ in LOO_POINTWISE]
        totals = np.empty(6); kc = np.zeros(2, dtype=np.int64); used = np.zeros(R, dtype=np.int64)
        self._ck(self.lib.rmhmc_loo_dev(self._h, w.data_ptr(), n, S, D, _ptr(x), _ptr(t), R, int(cols_per_block), _ptr(part), _ptr(fit), _ptr(body),
                                        *[_ptr(a) for a in pw], _ptr(totals), _ptr(kc, _lp), _ptr(used, _lp)))
        return _loo_result(pw, totals, kc, used, partial=part, fit=fit, body=body)

    # ---- adaptive Metropolis (code/metropolis.py, include/rmhmc_amh.h) -----------
    def amh_sample(self, n_iter, burn_in, seed=0, chain_offset=0, theta0=None):
        """returns (samples [n][n_iter-burn_in][D], accepted proposals [n], final ProposalSD [n][D], seconds after burn-in)"""
        self.rl.need("amh")
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0 or int(burn_in) < 0:
            raise ValueError("need 0 <= BurnIn < NumOfIterations")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        samples = np.empty((n, S, D)); acc = np.zeros(n, dtype=np.int64); sd = np.empty((n, D)); secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_amh_sample(self._h, int(n_iter), int(burn_in), int(seed), int(chain_offset), _ptr(th), _ptr(samples),
                                           _ptr(acc, _lp), _ptr(sd), C.cast(C.byref(secs), _dp)))
        return samples, acc, sd, secs.value

    def amh_replay(self, n_iter, burn_in, z, u, theta0=None):
        """z, u: [n][n_iter][D] recorded draws (u NaN where none was drawn).  Returns dict(w [n][n_iter][D], ljl [n][n_iter],
        sd [n][D], accepted / u_read [n][n_iter][D] bool)"""
        self.rl.need("amh")
        n, D, T = self.n, self.D, int(n_iter)
        z = _f64(z, (n, T, D)); u = _f64(u, (n, T, D))
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        w = np.empty((n, T, D)); ljl = np.empty((n, T)); sd = np.empty((n, D)); dec = np.zeros((n, T, D), dtype=np.int8)
        self._ck(self.lib.rmhmc_amh_replay(self._h, T, int(burn_in), _ptr(z), _ptr(u), _ptr(th), _ptr(w), _ptr(ljl), _ptr(sd),
                                           _ptr(dec, _i8p)))
        return dict(w=w, ljl=ljl, sd=sd, accepted=(dec & 1) != 0, u_read=(dec & 2) != 0)

    # ---- IWLS Metropolis-Hastings (code/iwls.py, include/rmhmc_iwls.h) ----------
    def iwls_sample(self, n_iter, burn_in, compat=True, seed=0, chain_offset=0, theta0=None):
        """returns (samples [n][n_iter-burn_in][D], accepted proposals [n], saturated proposals [n], seconds from iteration burn_in)"""
        self.rl.need("iwls")
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0 or int(burn_in) < 0:
            raise ValueError("need 0 <= burn_in < max_iter")
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        samples = np.empty((n, S, D)); acc = np.zeros(n, dtype=np.int64); sat = np.zeros(n, dtype=np.int64); secs = C.c_double(0.0)
        self._ck(self.lib.rmhmc_iwls_sample(self._h, int(n_iter), int(burn_in), 1 if compat else 0, int(seed), int(chain_offset), _ptr(th),
                                            _ptr(samples), _ptr(acc, _lp), _ptr(sat, _lp), C.cast(C.byref(secs), _dp)))
        return samples, acc, sat, secs.value

    def iwls_replay(self, w_prop, u, compat=True, theta0=None):
        """w_prop [n][T][D] given proposals, u [n][T] uniforms (NaN where none was drawn).  Returns dict(w, mean [n][T][D], ljl,
        ratio [n][T] after every iteration, accepted / u_read / saturated [n][T] bool)"""
        self.rl.need("iwls")
        n, D = self.n, self.D
        w_prop = _f64(w_prop)
        T = w_prop.size // (n * D)
        w_prop = w_prop.reshape(n, T, D); u = _f64(u, (n, T))
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        w = np.empty((n, T, D)); mean = np.empty((n, T, D)); ljl = np.empty((n, T)); ratio = np.empty((n, T))
        dec = np.zeros((n, T), dtype=np.int8)
        self._ck(self.lib.rmhmc_iwls_replay(self._h, T, 1 if compat else 0, _ptr(w_prop), _ptr(u), _ptr(th), _ptr(w), _ptr(mean), _ptr(ljl),
                                            _ptr(ratio), _ptr(dec, _i8p)))
        return dict(w=w, mean=mean, ljl=ljl, ratio=ratio, accepted=(dec & 1) != 0, u_read=(dec & 2) != 0, saturated=(dec & 4) != 0)

    # ---- auxiliary-variable Gibbs sampler (code/gibbs_sampler.py, include/rmhmc_gibbs.h) ----------
    def gibbs_sample(self, n_iter, burn_in, seed=0, chain_offset=0, state=False):
        """returns dict(samples [n][n_iter-burn_in][D], capped [n]: rows that reached a bound (expected 0), stopped [n]: -1, or the
        iteration at which the chain stopped where the reference would have (include/rmhmc_gibbs.h; its later rows are NaN), seconds
        from iteration burn_in; state=True adds Z and lam [n][N] after the last iteration)"""
        self.rl.need("gibbs")
        n, D = self.n, self.D
        S = int(n_iter) - int(burn_in)
        if S <= 0 or int(burn_in) < 0:
            raise ValueError("need 0 <= burn_in < max_iter")
        samples = np.empty((n, S, D)); capped = np.zeros(n, dtype=np.int64); stopped = np.zeros(n, dtype=np.int64); secs = C.c_double(0.0)
        Z = np.zeros((n, self.M)) if state else None
        lam = np.zeros((n, self.M)) if state else None
        self._ck(self.lib.rmhmc_gibbs_sample(self._h, int(n_iter), int(burn_in), int(seed), int(chain_offset), _ptr(samples),
                                             _ptr(capped, _lp), _ptr(stopped, _lp), _ptr(Z), _ptr(lam), C.cast(C.byref(secs), _dp)))
        out = dict(samples=samples, capped=capped, stopped=stopped, seconds=secs.value)
        if state:
            out.update(Z=Z, lam=lam)
        return out

    def gibbs_replay(self, u_init, u_sweep, T, ks_draws, ks_offset):
        """Recorded draws per chain: u_init [n][N], u_sweep [n][T][N], T [n][T][D], ks_draws [n][total][3], ks_offset [n][T][N+1].
        Returns dict(beta, B [n][T][D] after every iteration (B before the T term), attempts [n][T][N], Z, lam [n][N] after the last
        one, capped [n], status [n]: 1 where the tape ran out of attempts, 2 where a lam_j was not positive and finite: the chain stopped)"""
        self.rl.need("gibbs")
        n, D, N = self.n, self.D, self.M
        u_init = _f64(u_init, (n, N))
        u_sweep = _f64(u_sweep); Tn = u_sweep.size // (n * N)
        u_sweep = u_sweep.reshape(n, Tn, N); T = _f64(T, (n, Tn, D))
        ks_draws = _f64(ks_draws).reshape(n, -1, 3); total = ks_draws.shape[1]
        ks_offset = np.ascontiguousarray(ks_offset, dtype=np.int64).reshape(n, Tn, N + 1)
        beta = np.zeros((n, Tn, D)); B = np.zeros((n, Tn, D)); att = np.zeros((n, Tn, N), dtype=np.int32)
        Z = np.zeros((n, N)); lam = np.zeros((n, N)); capped = np.zeros(n, dtype=np.int64); status = np.zeros(n, dtype=np.int32)
        self._ck(self.lib.rmhmc_gibbs_replay(self._h, Tn, _ptr(u_init), _ptr(u_sweep), _ptr(T), _ptr(ks_draws), _ptr(ks_offset, _lp), total,
                                             _ptr(beta), _ptr(B), _ptr(att, _ip), _ptr(Z), _ptr(lam), _ptr(capped, _lp), _ptr(status, _ip)))
        return dict(beta=beta, B=B, attempts=att, Z=Z, lam=lam, capped=capped, status=status)

    # ---- output descriptor: every sampler to host or device memory, raw or reduced (include/rmhmc_out.h) ----------
    def sample_to(self, sampler, n_iter, burn_in, *, where="host", device=None, samples=False, stats=False, run_mean=False,
                  L=None, eps=None, K=None, compat=None, seed=0, chain_offset=0, theta0=None, diagnostics=False, max_lag=None,
                  quantiles=None):
        """One run of `sampler` (a key of SAMPLERS_TO) written out as asked: samples [n][S][D]; stats: mean, var, ess [n][D]; run_mean:
        run_mean [S][D] and run_ess [D].  where="host": NumPy arrays; "device": torch tensors on `device`, the samples written by the
        sampler itself.  Returns a dict of the requested outputs, the sampler's counters (same memory space) and `seconds`.  The run
        arguments are those of the sampler's own method, with its defaults (L, eps, K, compat where it has them); one the sampler does
        not have (theta0 for Gibbs included) is a ValueError.  The library works on a stream of its own: torch's current stream on
        `device` is synchronised before the call, and the library's is idle on return.

        diagnostics=True adds the cross-chain diagnostics of the call's samples (include/rmhmc_diag.h; max_lag as in diag_partial): rhat,
        ess_pooled, pairs, chains_used as host NumPy arrays [D], and diag_partial, the device tensor a sharded job merges.  The sampler
        then writes its samples to a device tensor whatever `where` and `samples` say (they are returned only if asked, and outputs
        asked on the host are copied there); samples and counters are those of the same call without the keyword, bit for bit.

        quantiles=probs (one probability or a sequence of them, each in [0, 1]) adds the exact posterior quantiles of the call's
        samples over all chains (include/rmhmc_quant.h): quantiles [Q][D] and quantile_draws [D], host NumPy arrays.  The samples go to
        a device tensor as for the diagnostics; a bad probability is refused before any sampling work."""
        probs = None if quantiles is None else quant_probs(quantiles)   # refused before any sampling work
        self.rl.need("out")
        if quantiles is not None:
            self.rl.need("quant")
            return self._sample_to_quant(sampler, n_iter, burn_in, where, device, samples, probs,
                                         dict(stats=stats, run_mean=run_mean, L=L, eps=eps, K=K, compat=compat, seed=seed,
                                              chain_offset=chain_offset, theta0=theta0, diagnostics=diagnostics, max_lag=max_lag))
        if diagnostics:
            return self._sample_to_diag(sampler, n_iter, burn_in, where, device, samples, max_lag,
                                        dict(stats=stats, run_mean=run_mean, L=L, eps=eps, K=K, compat=compat, seed=seed,
                                             chain_offset=chain_offset, theta0=theta0))
        name, counters = SAMPLERS_TO[sampler]
        given = dict(L=L, eps=eps, K=K, compat=compat, theta0=theta0)
        extra = sorted(k for k, v in given.items() if v is not None and k not in SAMPLER_ARGS[sampler])
        if extra:
            raise ValueError("sampler %r has no run argument %s" % (sampler, ", ".join(extra)))
        if sampler == "rmhmc":
            front = (int(6 if L is None else L), float(0.5 if eps is None else eps), int(4 if K is None else K))
        elif sampler == "hmc":
            front = (int(100 if L is None else L), float(0.14 if eps is None else eps))
        elif sampler == "mmala":
            front = (float(1.0 if eps is None else eps),)
        elif sampler == "iwls":
            front = (1 if compat or compat is None else 0,)
        else:
            front = ()
        return self._call_sample_to(name, counters, front, n_iter, burn_in, where, device, samples, stats, run_mean, seed, chain_offset,
                                    theta0, has_theta0=sampler != "gibbs")

    def _call_sample_to(self, name, counters, front, n_iter, burn_in, where, device, samples, stats, run_mean, seed, chain_offset, theta0,
                        has_theta0=True, back=()):
        """the descriptor, the buffers and the call of one <sampler>_sample_to entry point: `front` its run arguments between burn_in
        and seed, `back` those after seconds_out, `counters` as in SAMPLERS_TO"""
        n, D = self.n, self.D
        n_iter, burn_in = int(n_iter), int(burn_in)
        S = n_iter - burn_in
        if S <= 0 or burn_in < 0:
            raise ValueError("need 0 <= burn_in < n_iter")
        dev = where in ("device", OUT_DEVICE)
        if dev:
            import torch
            if device is None:
                raise ValueError('where="device" needs the torch device of the context\'s GPU')
            device = torch.device(device)
            if self.rl.on_gpu and device.type != "cuda":
                raise ValueError("the HIP library writes through device pointers: %s is not a GPU" % device)

        def buf(shape, dtype=np.float64):
            if dev:
                # (empty: the library writes every output and counter it is handed, and a fill would run on torch's stream)
                b = torch.empty(shape, dtype=torch.int64 if dtype is np.int64 else torch.float64, device=device)
                return b, b.data_ptr()
            b = np.zeros(shape, dtype=dtype)
            return b, b.ctypes.data

        res = {}
        o = Out(where={"host": OUT_HOST, "device": OUT_DEVICE}.get(where, where))
        want = ([("samples", (n, S, D))] if samples else []) + ([(k, (n, D)) for k in ("mean", "var", "ess")] if stats else []) \
            + ([("run_mean", (S, D)), ("run_ess", (D,))] if run_mean else [])
        for key, shape in want:
            res[key], ptr = buf(shape)
            setattr(o, key, ptr)
        cptr = []
        for key, vec in counters:
            res[key], ptr = buf((n, D) if vec else (n,), np.float64 if vec else np.int64)
            cptr.append(ptr)
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (n, D)))
        tail = (int(seed), int(chain_offset)) + ((_ptr(th),) if has_theta0 else ())
        secs = C.c_double(0.0)
        if dev and device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()   # nothing of torch's is pending on the buffers the library is handed
        self._ck(getattr(self.lib, name)(self._h, n_iter, burn_in, *front, *tail, C.byref(o), *cptr, C.cast(C.byref(secs), _dp), *back))
        res["seconds"] = secs.value
        return res

    def ess_dev(self, samples):
        """ESS, mean and population variance of a torch tensor [n][S][P] (or [S][P]) already on the context's GPU, reduced there: returns
        (ess, mean, var) tensors [n][P] on the same device.  torch's current stream on that device is synchronised first: the
        library reads the tensor at once on a stream of its own, so whatever produced it must have finished."""
        import torch
        self.rl.need("out")
        x = self._dev_tensor("ess_dev", samples, "")
        if x.dim() == 2:
            x = x[None]
        n, S, P = x.shape
        ess, mean, var = self._out_tensors([((n, P), torch.float64)] * 3, x.device)
        self._ck(self.lib.rmhmc_ess_dev(self._h, x.data_ptr(), n, S, P, ess.data_ptr(), mean.data_ptr(), var.data_ptr()))
        return ess, mean, var

    # ---- cross-chain diagnostics: split R-hat and the pooled ESS (include/rmhmc_diag.h) ----------
    def diag_partial(self, samples, max_lag=None):
        """The mergeable partial [(4 + T), P] (include/rmhmc_diag.h) of a float64 torch tensor [n][S][P] already on the context's GPU,
        reduced there; T = max_lag + 1, max_lag None or 0: every lag, S // 2 - 1.  torch's current stream is synchronised first, as in
        ess_dev."""
        import torch
        self.rl.need("diag")
        x = self._dev_tensor("diag_partial", samples, " [n][S][P]", 3)
        n, S, P = x.shape
        max_lag = 0 if max_lag is None else int(max_lag)
        H = S // 2
        T = (max_lag if max_lag else H - 1) + 1 if 0 <= max_lag < H else 1   # (out of range: the library refuses the call)
        part = torch.empty((4 + T, P), dtype=torch.float64, device=x.device)
        self._ck(self.lib.rmhmc_diag_partial_dev(self._h, x.data_ptr(), n, S, P, max_lag, part.data_ptr()))
        return part

    def diagnose(self, samples, max_lag=None):
        """split R-hat and pooled ESS of the chains of samples [n][S][P] on the context's GPU: dict(rhat, ess_pooled, pairs, chains_used:
        host NumPy arrays [P]; partial: the device tensor of diag_partial).  2 * pairs + 1 >= T marks an ESS that is an upper bound."""
        part = self.diag_partial(samples, max_lag)
        out = diag_finish([part], samples.shape[1] // 2, lib=self.rl)
        out["partial"] = part
        return out

    def _sample_to_diag(self, sampler, n_iter, burn_in, where, device, samples, max_lag, kw):
        import torch
        self.rl.need("diag")
        diag_lags(int(n_iter) - int(burn_in), max_lag)   # refused before any sampling work
        host = where in ("host", OUT_HOST)
        if host:
            device = torch.device("cuda", self.device) if self.rl.on_gpu else torch.device("cpu")
        r = self.sample_to(sampler, n_iter, burn_in, where="device" if host else where, device=device, samples=True, **kw)
        dg = self.diagnose(r["samples"], max_lag)
        if not samples:
            del r["samples"]
        if host:
            r = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in r.items()}
        r.update({k: dg[k] for k in DIAG_KEYS})
        r["diag_partial"] = dg["partial"]
        return r

    # ---- posterior quantiles: a radix select on mergeable integer histograms (include/rmhmc_quant.h) ----------
    def quant_hist(self, samples, round, prefix=None, K=None):
        """The histogram partial of one round of the select (include/rmhmc_quant.h) of a float64 torch tensor [n][S][P] already on the
        context's GPU, counted there: a tensor [1][P][256] in round 0 (prefix None) and [K][P][256] afterwards, prefix a uint64 array
        [K][P] (host; quant_step keeps it).  torch's current stream is synchronised first, as in ess_dev."""
        import torch
        self.rl.need("quant")
        x = self._dev_tensor("quant_hist", samples, " [n][S][P]", 3)
        n, S, P = x.shape
        round = int(round)
        pre = None
        if prefix is not None:
            pre = np.ascontiguousarray(prefix, dtype=np.uint64)
            if pre.ndim != 2 or pre.shape[1] != P:
                raise ValueError("quant_hist: prefix must be [K][P] with the P of the samples")
            K = pre.shape[0]
        K = 1 if K is None else int(K)
        Kh = K if round > 0 and 1 <= K <= QUANT_MAX_K else 1   # (out of range: the library refuses the call)
        hist = torch.empty((Kh, P, QUANT_BINS), dtype=torch.float64, device=x.device)
        self._ck(self.lib.rmhmc_quant_hist_dev(self._h, x.data_ptr(), n, S, P, round, _ptr(pre, _up), K, hist.data_ptr()))
        return hist

    def quantiles(self, samples, probs):
        """Exact quantiles (numpy's "linear" rule between the two exact order statistics) of every dimension of samples [n][S][P] on
        the context's GPU over all n S rows, non-finite values left out of their own dimension: dict(quantiles [Q][P], draws_used [P]
        the finite values per dimension), host NumPy arrays.  More than 8 probabilities run in groups of 8 (rmhmc_quant_dev)."""
        self.rl.need("quant")
        p = quant_probs(probs)
        x = self._dev_tensor("quantiles", samples, " [n][S][P]", 3)
        n, S, P = x.shape
        out = np.empty((p.size, P)); used = np.zeros(P, dtype=np.int64)
        for a in range(0, p.size, QUANT_MAX_Q):
            pg = np.ascontiguousarray(p[a:a + QUANT_MAX_Q])
            qg = np.empty((pg.size, P))
            self._ck(self.lib.rmhmc_quant_dev(self._h, x.data_ptr(), n, S, P, _ptr(pg), pg.size, _ptr(qg), _ptr(used, _lp)))
            out[a:a + pg.size] = qg
        return dict(quantiles=out, draws_used=used)

    def _sample_to_quant(self, sampler, n_iter, burn_in, where, device, samples, probs, kw):
        import torch
        host = where in ("host", OUT_HOST)
        if host:
            device = torch.device("cuda", self.device) if self.rl.on_gpu else torch.device("cpu")
        r = self.sample_to(sampler, n_iter, burn_in, where="device" if host else where, device=device, samples=True, **kw)
        q = self.quantiles(r["samples"], probs)
        if not samples:
            del r["samples"]
        if host:
            r = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) and k != "diag_partial" else v for k, v in r.items()}
        r["quantiles"], r["quantile_draws"] = q["quantiles"], q["draws_used"]
        return r

    # the three output modes of RMHMC (sample_dev, sample_stats, sample_stats_dev above) for the other five samplers: *_sample_dev
    # returns what *_sample returns with the arrays as tensors on `device`; *_sample_stats[_dev] return dict(mean, var, ess, the
    # sampler's counters, seconds), run_mean=True adds run_mean and run_ess
    def hmc_sample_dev(self, device, n_iter, burn_in, L=100, eps=0.14, seed=0, chain_offset=0, theta0=None):
        r = self.sample_to("hmc", n_iter, burn_in, where="device", device=device, samples=True, L=L, eps=eps, seed=seed,
                           chain_offset=chain_offset, theta0=theta0)
        return r["samples"], r["accepted"], r["leapfrog_steps"], r["seconds"]

    def hmc_sample_stats(self, n_iter, burn_in, L=100, eps=0.14, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("hmc", n_iter, burn_in, stats=True, run_mean=run_mean, L=L, eps=eps, seed=seed, chain_offset=chain_offset,
                              theta0=theta0)

    def hmc_sample_stats_dev(self, device, n_iter, burn_in, L=100, eps=0.14, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("hmc", n_iter, burn_in, where="device", device=device, stats=True, run_mean=run_mean, L=L, eps=eps,
                              seed=seed, chain_offset=chain_offset, theta0=theta0)

    def mmala_sample_dev(self, device, n_iter, burn_in, eps=1.0, seed=0, chain_offset=0, theta0=None):
        r = self.sample_to("mmala", n_iter, burn_in, where="device", device=device, samples=True, eps=eps, seed=seed,
                           chain_offset=chain_offset, theta0=theta0)
        return r["samples"], r["accepted"], r["seconds"]

    def mmala_sample_stats(self, n_iter, burn_in, eps=1.0, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("mmala", n_iter, burn_in, stats=True, run_mean=run_mean, eps=eps, seed=seed, chain_offset=chain_offset,
                              theta0=theta0)

    def mmala_sample_stats_dev(self, device, n_iter, burn_in, eps=1.0, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("mmala", n_iter, burn_in, where="device", device=device, stats=True, run_mean=run_mean, eps=eps, seed=seed,
                              chain_offset=chain_offset, theta0=theta0)

    def amh_sample_dev(self, device, n_iter, burn_in, seed=0, chain_offset=0, theta0=None):
        r = self.sample_to("amh", n_iter, burn_in, where="device", device=device, samples=True, seed=seed, chain_offset=chain_offset,
                           theta0=theta0)
        return r["samples"], r["accepted"], r["sd"], r["seconds"]

    def amh_sample_stats(self, n_iter, burn_in, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("amh", n_iter, burn_in, stats=True, run_mean=run_mean, seed=seed, chain_offset=chain_offset, theta0=theta0)

    def amh_sample_stats_dev(self, device, n_iter, burn_in, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("amh", n_iter, burn_in, where="device", device=device, stats=True, run_mean=run_mean, seed=seed,
                              chain_offset=chain_offset, theta0=theta0)

    def iwls_sample_dev(self, device, n_iter, burn_in, compat=True, seed=0, chain_offset=0, theta0=None):
        r = self.sample_to("iwls", n_iter, burn_in, where="device", device=device, samples=True, compat=compat, seed=seed,
                           chain_offset=chain_offset, theta0=theta0)
        return r["samples"], r["accepted"], r["saturated"], r["seconds"]

    def iwls_sample_stats(self, n_iter, burn_in, compat=True, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("iwls", n_iter, burn_in, stats=True, run_mean=run_mean, compat=compat, seed=seed, chain_offset=chain_offset,
                              theta0=theta0)

    def iwls_sample_stats_dev(self, device, n_iter, burn_in, compat=True, seed=0, chain_offset=0, theta0=None, run_mean=False):
        return self.sample_to("iwls", n_iter, burn_in, where="device", device=device, stats=True, run_mean=run_mean, compat=compat,
                              seed=seed, chain_offset=chain_offset, theta0=theta0)

    def gibbs_sample_dev(self, device, n_iter, burn_in, seed=0, chain_offset=0):
        return self.sample_to("gibbs", n_iter, burn_in, where="device", device=device, samples=True, seed=seed, chain_offset=chain_offset)

    def gibbs_sample_stats(self, n_iter, burn_in, seed=0, chain_offset=0, run_mean=False):
        return self.sample_to("gibbs", n_iter, burn_in, stats=True, run_mean=run_mean, seed=seed, chain_offset=chain_offset)

    def gibbs_sample_stats_dev(self, device, n_iter, burn_in, seed=0, chain_offset=0, run_mean=False):
        return self.sample_to("gibbs", n_iter, burn_in, where="device", device=device, stats=True, run_mean=run_mean, seed=seed,
                              chain_offset=chain_offset)

    def chains_init(self, theta0=None, seed=0, chain_offset=0, L=6, eps=0.5, K=4):
        th = None if theta0 is None else _f64(np.broadcast_to(theta0, (self.n, self.D)))
        self._ck(self.lib.rmhmc_chains_init(self._h, _ptr(th), int(seed), int(chain_offset), int(L), float(eps), int(K)))

    def chains_run(self, n_steps):
        self._ck(self.lib.rmhmc_chains_run(self._h, int(n_steps)))

    def chains_state(self):
        w = np.empty((self.n, self.D)); it = np.zeros(self.n, dtype=np.int64); acc = np.zeros(self.n, dtype=np.int64)
        self._ck(self.lib.rmhmc_chains_state(self._h, _ptr(w), _ptr(it, _lp), _ptr(acc, _lp)))
        return w, it, acc

    def chains_restore(self, iters, accepted):
        it = np.ascontiguousarray(iters, dtype=np.int64).reshape(self.n)
        acc = np.ascontiguousarray(accepted, dtype=np.int64).reshape(self.n)
        self._ck(self.lib.rmhmc_chains_restore(self._h, _ptr(it, _lp), _ptr(acc, _lp)))

    def set_progress(self, fn, first=49, every=50):
        """fn(event, iterations_done, accepted_total, iterations_total) or None.  The defaults are the reference's schedule: a report
        whenever IterationNum+1 is a multiple of 50, i.e. after 49, 99, ... completed transitions (rmhmc.py:38).  One chain: exactly
        then; several chains: when the slowest chain has got there (include/rmhmc.h)."""
        if fn is None:
            self._progress_cb = PROGRESS_FN(0)
            self._ck(self.lib.rmhmc_set_progress(self._h, self._progress_cb, 1, 1, None))
            return
        self._progress_cb = PROGRESS_FN(lambda ev, it, acc, itot, user: fn(int(ev), int(it), int(acc), int(itot)))   # kept alive with the context
        self._ck(self.lib.rmhmc_set_progress(self._h, self._progress_cb, int(first), int(every), None))

    def int8_certificate(self):
        """(bound, active): worst-case error bound of the int8 metric path for the current data, and whether the int8 kernels are in use"""
        b = C.c_double(0.0); a = C.c_int32(0)
        self._ck(self.lib.rmhmc_int8_certificate(self._h, C.cast(C.byref(b), _dp), C.cast(C.byref(a), _ip)))
        return b.value, bool(a.value)

    def i8_delta_counts(self):
        """delta assemblies of the int8 path since chains_init, by the slice count S' the device picked (rmhmc_kernel_time,
        include/rmhmc.h): {"end": [S'=4, S'=5, S'=6], "inner": [S'=4, S'=5]}"""
        return {"end": [self.kernel_time("i8_delta_end_s%d" % s)[1] for s in (4, 5, 6)],
                "inner": [self.kernel_time("i8_delta_inner_s%d" % s)[1] for s in (4, 5)]}

    def kernel_time(self, which):
        s = C.c_double(0.0); k = C.c_int64(0)
        self._ck(self.lib.rmhmc_kernel_time(self._h, which.encode(), C.cast(C.byref(s), _dp), C.cast(C.byref(k), _lp)))
        return s.value, k.value


def _lib_with(lib, key):
    """lib, or the product library where it is None; either must have the optional feature `key`"""
    lib = lib if lib is not None else load_hip_library()
    lib.need(key)
    return lib


def _finish_call(name, key, partials, lib, ok, refusal):
    """What the *_finish functions share around their own outputs.  The library (_lib_with) must have the feature `key`.  The partials
    (torch tensors on any device or NumPy arrays) become float64 host arrays, refused with ValueError(refusal) unless there is one,
    ok(the first) holds and all have its shape.  Returns (the shape of a partial, call): call(*rest) runs the library's
    `name`(the pointers to the partials, their number, *rest) and raises RmhmcError where that fails."""
    lib = _lib_with(lib, key)
    parts = [_f64(p if isinstance(p, np.ndarray) else p.detach().cpu().numpy()) for p in partials]
    if not parts or not ok(parts[0]) or any(p.shape != parts[0].shape for p in parts):
        raise ValueError(refusal)
    ptrs = (_dp * len(parts))(*[_ptr(p) for p in parts])

    def call(*rest):
        lib.ck(getattr(lib.lib, name)(ptrs, len(parts), *rest))   # (the closure keeps the arrays behind ptrs alive)
    return parts[0].shape, call


def diag_finish(partials, H, lib=None):
    """rmhmc_diag_finish (include/rmhmc_diag.h): the partials ([(4 + T), P] each: torch tensors on any device or NumPy arrays, all of the
    same shape, from series of H rows) merged in the order given and finished on the host.  Returns dict(rhat, ess_pooled, pairs,
    chains_used: NumPy arrays [P]; merged: the merged partial [(4 + T), P])."""
    shape, call = _finish_call("rmhmc_diag_finish", "diag", partials, lib, lambda p: p.ndim == 2,
                               "diag_finish: partials of one shape [(4 + T), P] required")
    T, P = shape[0] - 4, shape[1]
    merged = np.empty((4 + T, P)); rhat = np.empty(P); ess = np.empty(P)
    pairs = np.zeros(P, dtype=np.int64); used = np.zeros(P, dtype=np.int64)
    call(int(H), T, P, _ptr(merged), _ptr(rhat), _ptr(ess), _ptr(pairs, _lp), _ptr(used, _lp))
    return dict(rhat=rhat, ess_pooled=ess, pairs=pairs, chains_used=used, merged=merged)


def diag_info(st, diagnostics):
    """what a shim adds to its info dict: {"diagnostics": the DIAG_KEYS of a sample_to result} when asked, else nothing"""
    return {"diagnostics": {k: st[k] for k in DIAG_KEYS}} if diagnostics else {}


def diag_identity(T, P):
    """the partial of no series at all (an empty shard): the identity of the merge"""
    return np.zeros((4 + int(T), int(P)))


def quant_identity(K, P):
    """the histogram partial of no rows at all (an empty shard): the identity of the merge; K = 1 in round 0"""
    return np.zeros((int(K), int(P), QUANT_BINS))


def quant_plan(m, probs, lib=None):
    """rmhmc_quant_plan (include/rmhmc_quant.h): m [P] finite values per dimension (int64), 1 .. 8 probabilities -> (rank int64 [2Q][P]:
    rows 2j and 2j+1 the two order statistics of probs[j], -1 where m is 0; frac [Q][P]: the weight of the upper one)"""
    lib = _lib_with(lib, "quant")
    m = np.ascontiguousarray(m, dtype=np.int64).reshape(-1)
    p = quant_probs(probs)
    rank = np.zeros((2 * p.size, m.size), dtype=np.int64); frac = np.empty((p.size, m.size))
    lib.ck(lib.lib.rmhmc_quant_plan(_ptr(m, _lp), _ptr(p), p.size, m.size, _ptr(rank, _lp), _ptr(frac)))
    return rank, frac


def quant_step(hists, round, prefix, rank, lib=None):
    """rmhmc_quant_step: the histogram partials of one round ([Kh][P][256] each: torch tensors on any device or NumPy arrays, one per
    shard) merged in the order given; prefix (uint64 [K][P]) and rank (int64 [K][P]), both contiguous NumPy arrays, are updated in
    place.  RmhmcError -1, nothing written, for histograms that do not continue the previous round of these targets."""
    if not (isinstance(prefix, np.ndarray) and prefix.dtype == np.uint64 and prefix.ndim == 2 and prefix.flags.c_contiguous
            and isinstance(rank, np.ndarray) and rank.dtype == np.int64 and rank.shape == prefix.shape and rank.flags.c_contiguous):
        raise ValueError("quant_step: prefix (uint64) and rank (int64) are contiguous arrays of one shape [K][P]")
    K, P = prefix.shape
    Kh = K if int(round) > 0 else 1
    _, call = _finish_call("rmhmc_quant_step", "quant", hists, lib, lambda h: h.shape == (Kh, P, QUANT_BINS),
                           "quant_step: histograms of one shape [K][P][256] ([1][P][256] in round 0) required")
    call(P, K, int(round), _ptr(prefix, _up), _ptr(rank, _lp))


def quant_finish(prefix, frac, m, lib=None):
    """rmhmc_quant_finish: prefix (uint64 [2Q][P]) after round 7, frac [Q][P] and m [P] of quant_plan -> the quantiles [Q][P]"""
    lib = _lib_with(lib, "quant")
    frac = _f64(frac)
    m = np.ascontiguousarray(m, dtype=np.int64).reshape(-1)
    prefix = np.ascontiguousarray(prefix, dtype=np.uint64)
    if frac.ndim != 2 or prefix.shape != (2 * frac.shape[0], frac.shape[1]) or m.size != frac.shape[1]:
        raise ValueError("quant_finish: prefix [2Q][P], frac [Q][P] and m [P] required")
    Q, P = frac.shape
    out = np.empty((Q, P))
    lib.ck(lib.lib.rmhmc_quant_finish(_ptr(prefix, _up), _ptr(frac), _ptr(m, _lp), Q, P, _ptr(out)))
    return out


def quant_totals(hists):
    """the finite values per dimension, int64 [P]: the totals of the round-0 histograms of all shards"""
    return sum(np.asarray(h if isinstance(h, np.ndarray) else h.detach().cpu().numpy(), dtype=np.float64)[0].sum(axis=1) for h in hists).astype(np.int64)


def quant_select(hist, probs, P, lib=None):
    """The eight rounds of the select around any source of histograms: hist(round, prefix, K) returns the list of the shards' partials of
    that round (prefix None in round 0).  Every shard that runs this with the same (merged or gathered) histograms steps identically.
    Returns dict(quantiles [Q][P], draws_used [P]); more than 8 probabilities run in groups of 8 on the one round-0 histogram."""
    p = quant_probs(probs)
    h0 = hist(0, None, 1)
    m = quant_totals(h0)
    out = np.empty((p.size, int(P)))
    for a in range(0, p.size, QUANT_MAX_Q):
        pg = p[a:a + QUANT_MAX_Q]
        rank, frac = quant_plan(m, pg, lib=lib)
        prefix = np.zeros(rank.shape, dtype=np.uint64)
        quant_step(h0, 0, prefix, rank, lib=lib)
        for r in range(1, QUANT_ROUNDS):
            quant_step(hist(r, prefix, prefix.shape[0]), r, prefix, rank, lib=lib)
        out[a:a + pg.size] = quant_finish(prefix, frac, m, lib=lib)
    return dict(quantiles=out, draws_used=m)


def cov_finish(partials, lib=None):
    """rmhmc_cov_finish (include/rmhmc_adapt.h): the partials ([(2 + P), P] each: torch tensors on any device or NumPy arrays) merged in
    the order given and finished on the host.  Returns dict(mean [P], cov [P][P] (NaN for fewer than 2 rows), rows_used, merged)."""
    shape, call = _finish_call("rmhmc_cov_finish", "adapt", partials, lib, lambda p: p.ndim == 2 and p.shape[0] == p.shape[1] + 2,
                               "cov_finish: partials of one shape [(2 + P), P] required")
    P = shape[1]
    merged = np.empty((2 + P, P)); mean = np.empty(P); cov = np.empty((P, P)); used = C.c_int64(0)
    call(P, _ptr(merged), _ptr(mean), _ptr(cov), C.cast(C.byref(used), _lp))
    return dict(mean=mean, cov=cov, rows_used=used.value, merged=merged)


def adapt_mass(cov, rows_used, lib=None):
    """rmhmc_adapt_mass: the inverse of the shrunk covariance m / (m + 5) cov + 1e-3 * 5 / (m + 5) I, or None where the library refuses
    it (fewer than 2 rows, not finite, not positive definite): the caller keeps its mass"""
    lib = _lib_with(lib, "adapt")
    cov = _f64(cov)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("adapt_mass: a square covariance required")
    mass = np.empty_like(cov)
    rc = lib.lib.rmhmc_adapt_mass(_ptr(cov), int(rows_used), cov.shape[0], _ptr(mass))
    return mass if rc == 0 else None


def adapt_init(eps, factor=10.0, lib=None):
    """rmhmc_adapt_init: the dual-averaging state (t, Hbar, log epsbar, mu = log(factor eps)) of a (re)start at step size eps; the
    warm-up starts with factor 10 and restarts with factor 1 after a mass update"""
    lib = _lib_with(lib, "adapt")
    state = np.empty(4)
    lib.ck(lib.lib.rmhmc_adapt_init(_ptr(state), float(eps), float(factor)))
    return state


def adapt_step(state, accept, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, lib=None):
    """rmhmc_adapt_step: one dual-averaging update of `state` (a float64 array of 4, updated in place) with the acceptance statistic
    of a window.  Returns (eps_next, eps_bar)."""
    lib = _lib_with(lib, "adapt")
    if not (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.shape == (4,) and state.flags.c_contiguous):
        raise ValueError("adapt_step: the state is a contiguous float64 array of 4")
    e = C.c_double(0.0); eb = C.c_double(0.0)
    lib.ck(lib.lib.rmhmc_adapt_step(_ptr(state), float(accept), float(delta), float(gamma), float(t0), float(kappa),
                                    C.cast(C.byref(e), _dp), C.cast(C.byref(eb), _dp)))
    return e.value, eb.value


def ais_finish(partials, lib=None):
    """rmhmc_ais_finish (include/rmhmc_ais.h): the weight partials ([5] each: torch tensors on any device or NumPy arrays) merged in the
    order given and finished on the host.  Returns dict(log_mean_w, se (NaN for m < 2), weight_ess, m, n_nan, merged [5])."""
    _, call = _finish_call("rmhmc_ais_finish", "ais", partials, lib, lambda p: p.shape == (5,), "ais_finish: partials of shape [5] required")
    merged = np.empty(5); lm = C.c_double(0.0); se = C.c_double(0.0); ess = C.c_double(0.0); m = C.c_int64(0); nn = C.c_int64(0)
    call(_ptr(merged), C.cast(C.byref(lm), _dp), C.cast(C.byref(se), _dp), C.cast(C.byref(ess), _dp), C.cast(C.byref(m), _lp),
         C.cast(C.byref(nn), _lp))
    return dict(log_mean_w=lm.value, se=se.value, weight_ess=ess.value, m=m.value, n_nan=nn.value, merged=merged)


def smc_cess_finish(partials, lib=None):
    """rmhmc_smc_cess_finish (include/rmhmc_smc.h): the conditional-ESS partials ([2 + 4 J] each: torch tensors on any device or NumPy
    arrays) merged in the order given and finished on the host.  Returns dict(frac [J]: cess / n of every candidate, merged)."""
    shape, call = _finish_call("rmhmc_smc_cess_finish", "smc", partials, lib,
                               lambda p: p.ndim == 1 and (p.size - 2) % 4 == 0 and 1 <= (p.size - 2) // 4 <= SMC_MAX_J,
                               "smc_cess_finish: partials of one shape [2 + 4 J], 1 <= J <= %d, required" % SMC_MAX_J)
    J = (shape[0] - 2) // 4
    merged = np.empty(2 + 4 * J); frac = np.empty(J)
    call(J, _ptr(merged), _ptr(frac))
    return dict(frac=frac, merged=merged)


def smc_resample_u(seed, k):
    """the 32-bit offset of the resampling of stage k of rmhmc_smc_run: the high half of splitmix64(seed + 0x9E3779B97F4A7C15 (k + 1))"""
    m = 2 ** 64 - 1
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return (z ^ (z >> 31)) >> 32


def pred_finish(partials, lib=None):
    """rmhmc_pred_finish (include/rmhmc_pred.h): the partials ([4, R] each: torch tensors on any device or NumPy arrays) merged in the
    order given and finished on the host.  Returns dict(prob, pvar, lpd [R], lpd_total, draws_used, merged [4, R])."""
    shape, call = _finish_call("rmhmc_pred_finish", "pred", partials, lib, lambda p: p.ndim == 2 and p.shape[0] == 4,
                               "pred_finish: partials of one shape [4, R] required")
    R = shape[1]
    merged = np.empty((4, R)); prob = np.empty(R); pvar = np.empty(R); lpd = np.empty(R); total = C.c_double(0.0); used = C.c_int64(0)
    call(R, _ptr(merged), _ptr(prob), _ptr(pvar), _ptr(lpd), C.cast(C.byref(total), _dp), C.cast(C.byref(used), _lp))
    return dict(prob=prob, pvar=pvar, lpd=lpd, lpd_total=total.value, draws_used=used.value, merged=merged)


def pred_identity(R):
    """the partial of no draws at all (an empty shard): the identity of the merge"""
    return np.zeros((4, int(R)))


def loo_identity(C):
    """the moments partial of no draws at all (an empty shard): the identity of the merge, lmin = +inf"""
    p = np.zeros((5, int(C)))
    p[4] = np.inf
    return p


def loo_plan(m, lib=None):
    """rmhmc_loo_plan (include/rmhmc_loo.h): m [C] finite values per column (int64) -> (tail_len int64 [C], rank int64 [C]: the 0-based
    rank of the cutoff, -1 where the tail is shorter than 5).  RmhmcError -4 for a tail longer than LOO_MAX_TAIL."""
    lib = _lib_with(lib, "loo")
    m = np.ascontiguousarray(m, dtype=np.int64).reshape(-1)
    tl = np.zeros(m.size, dtype=np.int64); rank = np.zeros(m.size, dtype=np.int64)
    lib.ck(lib.lib.rmhmc_loo_plan(_ptr(m, _lp), m.size, _ptr(tl, _lp), _ptr(rank, _lp)))
    return tl, rank


def _loo_result(pointwise, totals, k_counts, used, **more):
    out = dict(zip(LOO_POINTWISE, pointwise))
    out["totals"] = dict(zip(LOO_TOTALS, (float(v) for v in totals)))
    out.update(k_mid=int(k_counts[0]), k_high=int(k_counts[1]), draws_used=used)
    out.update(more)
    return out


def loo_finish(partials, fit=None, body=None, lib=None):
    """rmhmc_loo_finish (include/rmhmc_loo.h): the moments partials ([5, C] each: torch tensors on any device or NumPy arrays) merged in
    the order given and finished on the host with fit [4, C] and body [2, C] (both None: WAIC alone).  Returns dict(elpd_loo, p_loo,
    pareto_k, lppd, p_waic, elpd_waic [C]; totals: a dict of LOO_TOTALS; k_mid, k_high: the khat in (0.5, 0.7] and above 0.7;
    draws_used int64 [C]; merged [5, C])."""
    shape, call = _finish_call("rmhmc_loo_finish", "loo", partials, lib, lambda p: p.ndim == 2 and p.shape[0] == 5,
                               "loo_finish: partials of one shape [5, C] required")
    Cc = shape[1]
    host = [None if a is None else _f64(a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()) for a in (fit, body)]
    if (host[0] is None) != (host[1] is None) or (host[0] is not None and (host[0].shape != (4, Cc) or host[1].shape != (2, Cc))):
        raise ValueError("loo_finish: fit [4, C] and body [2, C] together, or neither")
    merged = np.empty((5, Cc)); pw = [np.empty(Cc) for _ in LOO_POINTWISE]
    totals = np.empty(6); kc = np.zeros(2, dtype=np.int64); used = np.zeros(Cc, dtype=np.int64)
    call(Cc, _ptr(host[0]), _ptr(host[1]), _ptr(merged), *[_ptr(a) for a in pw], _ptr(totals), _ptr(kc, _lp), _ptr(used, _lp))
    return _loo_result(pw, totals, kc, used, merged=merged)


_hip = None


def load_hip_library():
    """The product library (HIP kernels for gfx950).  Raises when it is not built.

    PyTorch (used for device plumbing and torch.distributed) bundles its own HIP runtime with the
    same SONAME as the system one.  Importing torch BEFORE dlopen-ing the library makes both share
    that single runtime; the other order would put two HIP/HSA stacks in one process."""
    global _hip
    if _hip is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip = RmhmcLib(os.environ.get("RMHMC_HIP_LIB", HIP_LIB_PATH))   # (override: experiment builds of the same library)
    return _hip
