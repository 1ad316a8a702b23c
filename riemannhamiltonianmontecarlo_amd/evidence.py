"""The log marginal likelihood log p(t) of Bayesian logistic regression under the N(0, alpha I) prior, by annealed importance sampling
(Neal 2001) on the GPU (include/rmhmc_ais.h): the quantity that compares models (feature sets, bases) on the same data.

    r = log_evidence(XX, t)          # r["log_evidence"] +- r["se"], r["weight_ess"], r["log_laplace"] beside it

A batch of independent chains is the particle population: every chain starts at an exact draw from the prior, passes through the
tempered targets p(t|w)^beta p(w) of a ladder 0 < beta_1 < .. < beta_T = 1 with fixed-metric HMC transitions, and collects the weight
logw = sum_k (beta_k - beta_{k-1}) loglik(w_{k-1}).  log p(t) is the log of the mean weight.  No CPU fallback.
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
