"""The log marginal likelihood log p(t) of Bayesian logistic regression under the N(0, alpha I) prior, by annealed importance sampling
(Neal 2001) on the GPU (include/rmhmc_ais.h): the quantity that compares models (feature sets, bases) on the same data.

    r = log_evidence(XX, t)          # r["log_evidence"] +- r["se"], r["weight_ess"], r["log_laplace"] beside it

A batch of independent chains is the particle population: every chain starts at an exact draw from the prior, passes through the
tempered targets p(t|w)^beta p(w) of a ladder 0 < beta_1 < .. < beta_T = 1 with fixed-metric HMC transitions, and collects the weight
logw = sum_k (beta_k - beta_{k-1}) loglik(w_{k-1}).  log p(t) is the log of the mean weight.  No CPU fallback.

    r = log_evidence_adaptive(XX, t) # the same on a ladder the run chooses from the conditional ESS of its weights, with resampling
                                     # (adaptive sequential Monte Carlo, include/rmhmc_smc.h): what a sharp likelihood needs
"""
import math

import numpy as np

from . import _capi


def log_laplace(XX, t, w, G, alpha=100.0):
    """the Laplace approximation of log p(t) at the posterior mode w with metric G = -Hessian of the log joint there (on the host)"""
    XX = np.asarray(XX, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    D = XX.shape[1]
    f = XX @ w
    ljl = f @ t - np.logaddexp(0.0, f).sum() - 0.5 * D * math.log(2.0 * math.pi * alpha) - (w @ w) / (2.0 * alpha)
    return float(ljl + 0.5 * D * math.log(2.0 * math.pi) - 0.5 * np.linalg.slogdet(G)[1])


def log_evidence(XX, t, n_chains=8192, n_temps=1000, iters_per_temp=1, ladder="power4", mass="mode", mass_every=1, NumOfLeapFrogSteps=6,
                 StepSize=0.5, alpha=100.0, seed=0, _lib=None):
    """ LOG MARGINAL LIKELIHOOD BY ANNEALED IMPORTANCE SAMPLING (Bayesian logistic regression, N(0, alpha I) prior)

    n_chains particles, n_temps stages of iters_per_temp transitions each; ladder: "power<q>" (beta_k = (k / T)^q) or "log<beta_min>"
    (_capi.ais_schedule).  mass="mode": every mass_every stages (and in the first and the last) the mass matrix becomes
    beta H + I / alpha with H = G(mode) - I / alpha the likelihood's part of the metric at the posterior mode - the exact metric of the
    tempered target were it Gaussian; mass=None: the identity throughout.
    Returns a dict: log_evidence, se (the delta-method standard error of log_evidence), weight_ess (of n_chains), n_nan (chains that
    failed and were left out), log_laplace (the Laplace approximation at the posterior mode, a sanity figure), accept_trace
    [n_temps], seconds (of the annealing run), info (mode, newton_iters, beta, stage_mass, logw, partial, seed)."""
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if int(n_chains) != n_chains or n_chains < 2:
        raise ValueError("n_chains must be >= 2 (the standard error needs two weights)")
    if mass is not None and not (isinstance(mass, str) and mass == "mode"):
        raise ValueError('mass must be "mode" or None')
    if int(NumOfLeapFrogSteps) != NumOfLeapFrogSteps or NumOfLeapFrogSteps < 1:
        raise ValueError("NumOfLeapFrogSteps must be >= 1")
    if not (np.isfinite(StepSize) and StepSize > 0.0):
        raise ValueError("StepSize must be finite and > 0")
    if not (np.isfinite(alpha) and alpha > 0.0):
        raise ValueError("alpha must be finite and > 0")
    beta, stage_len, stage_mass = _capi.ais_schedule(n_temps, ladder, mass_every if mass is not None else None, iters_per_temp)
    lib = _lib if _lib is not None else _capi.load_hip_library()
    with lib.context(N, D, int(n_chains)) as ctx:
        ctx.set_data(XX, t, alpha)
        md = ctx.phmc_mode()
        if not md["converged"]:
            raise RuntimeError("log_evidence: the Newton search for the posterior mode has not converged after %d iterations "
                               "(last step %.3e)" % (md["iters"], md["step"]))
        H = md["G"] - np.eye(D) / alpha if mass is not None else None
        ctx.phmc_set_mass(None)      # (the identity until the first stage installs its own)
        r = ctx.ais_run(beta, stage_len, stage_mass, H, L=NumOfLeapFrogSteps, eps=StepSize, seed=seed)
    return dict(log_evidence=r["log_mean_w"], se=r["se"], weight_ess=r["weight_ess"], n_nan=r["n_nan"],
                log_laplace=log_laplace(XX, t, md["w"], md["G"], alpha), accept_trace=r["accept_trace"], seconds=r["seconds"],
                info=dict(mode=md["w"], newton_iters=md["iters"], beta=beta, stage_mass=stage_mass, logw=r["logw"], partial=r["partial"],
                          seed=seed))


def log_evidence_adaptive(XX, t, n_chains=8192, cess_target=0.9, resample_below=0.5, iters_per_temp=1, mass="mode", mass_every=1,
                          max_temps=10000, repeats=1, NumOfLeapFrogSteps=6, StepSize=0.5, alpha=100.0, seed=0, _lib=None):
    """ LOG MARGINAL LIKELIHOOD BY ADAPTIVE SEQUENTIAL MONTE CARLO (include/rmhmc_smc.h)

    The annealing of log_evidence on a ladder the run chooses itself: every stage takes the largest step of the inverse temperature
    whose conditional ESS stays at cess_target n_chains (Zhou, Johansen and Aston 2016), and the particles are resampled (systematic)
    whenever the weight-ESS falls below resample_below n_chains (0: never - annealed importance sampling on the adaptive ladder).
    mass and mass_every as in log_evidence (a mass also in the last stage); max_temps bounds the number of stages: RuntimeError if they
    do not reach beta = 1.  repeats >= 2 runs the seeds seed, seed + (max_temps + 1), seed + 2 (max_temps + 1), .. and returns the log
    of the mean estimate of p(t) with its delta-method standard error over the repeats; with repeats = 1 se is the run's own: NaN if
    a stage resampled.  (Stage k of a run draws from the streams of seed + 1 + k, so runs of neighbouring seeds share random numbers
    - measured: a lag-1 correlation of 0.3 - 0.45 between their estimates - and a standard error over them would be too small; the
    spacing keeps the streams of the repeats apart.)
    Returns a dict: log_evidence, se, log_laplace, n_temps (stages, per repeat for repeats >= 2), seconds (of the runs), info (mode,
    newton_iters, seed, and per repeat in lists: seeds, log_z, beta, cess, ess, flags, accept_trace, weight_ess, logw)."""
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if int(n_chains) != n_chains or n_chains < 2:
        raise ValueError("n_chains must be >= 2 (the standard error needs two weights)")
    if n_chains > _capi.SMC_MAX_N and resample_below > 0.0:
        raise ValueError("resampling needs n_chains <= 2^20")
    if not 0.0 < cess_target < 1.0:
        raise ValueError("cess_target must be in (0, 1)")
    if not 0.0 <= resample_below <= 1.0:
        raise ValueError("resample_below must be in [0, 1]")
    if int(iters_per_temp) != iters_per_temp or iters_per_temp < 1:
        raise ValueError("iters_per_temp must be >= 1")
    if mass is not None and not (isinstance(mass, str) and mass == "mode"):
        raise ValueError('mass must be "mode" or None')
    if int(mass_every) != mass_every or mass_every < 1:
        raise ValueError("mass_every must be a number of stages >= 1")
    if int(max_temps) != max_temps or not 1 <= max_temps < 2 ** 31:
        raise ValueError("max_temps must be a number of stages >= 1")
    if int(repeats) != repeats or repeats < 1:
        raise ValueError("repeats must be >= 1")
    if int(NumOfLeapFrogSteps) != NumOfLeapFrogSteps or NumOfLeapFrogSteps < 1:
        raise ValueError("NumOfLeapFrogSteps must be >= 1")
    if not (np.isfinite(StepSize) and StepSize > 0.0):
        raise ValueError("StepSize must be finite and > 0")
    if not (np.isfinite(alpha) and alpha > 0.0):
        raise ValueError("alpha must be finite and > 0")
    lib = _lib if _lib is not None else _capi.load_hip_library()
    runs = []
    seeds = [int(seed) + rep * (int(max_temps) + 1) for rep in range(int(repeats))]
    with lib.context(N, D, int(n_chains)) as ctx:
        ctx.set_data(XX, t, alpha)
        md = ctx.phmc_mode()
        if not md["converged"]:
            raise RuntimeError("log_evidence_adaptive: the Newton search for the posterior mode has not converged after %d iterations "
                               "(last step %.3e)" % (md["iters"], md["step"]))
        H = md["G"] - np.eye(D) / alpha if mass is not None else None
        for run_seed in seeds:
            ctx.phmc_set_mass(None)      # (the identity until the first stage installs its own)
            r = ctx.smc_run(cess_target, resample_below, int(max_temps), int(iters_per_temp), int(mass_every) if mass is not None else 0, H,
                            L=NumOfLeapFrogSteps, eps=StepSize, seed=run_seed)
            if math.isnan(r["log_z"]) and r["beta"][-1] < 1.0:
                raise RuntimeError("log_evidence_adaptive: %d stages have reached beta = %.6g only (max_temps)" % (r["T"], r["beta"][-1]))
            runs.append(r)
    lz = np.array([r["log_z"] for r in runs])
    if len(runs) == 1:
        value, se = float(lz[0]), runs[0]["se"]
    else:                                # log of the mean of the Z estimates, and the delta-method standard error of that log
        a = lz.max()
        z = np.exp(lz - a)
        value = float(a + math.log(z.mean())) if np.isfinite(a) else float(a)
        se = float(z.std(ddof=1) / math.sqrt(len(z)) / z.mean()) if np.isfinite(a) else float("nan")
    return dict(log_evidence=value, se=se, log_laplace=log_laplace(XX, t, md["w"], md["G"], alpha),
                n_temps=runs[0]["T"] if len(runs) == 1 else [r["T"] for r in runs], seconds=float(sum(r["seconds"] for r in runs)),
                info=dict(mode=md["w"], newton_iters=md["iters"], seed=seed, seeds=seeds, log_z=lz, beta=[r["beta"] for r in runs],
                          cess=[r["cess"] for r in runs], ess=[r["ess"] for r in runs], flags=[r["flags"] for r in runs],
                          accept_trace=[r["accept_trace"] for r in runs], weight_ess=[r["weight_ess"] for r in runs],
                          logw=[r["logw"] for r in runs]))
