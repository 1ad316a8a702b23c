"""Leave-one-out cross-validation of Bayesian logistic regression under the N(0, alpha I) prior on the GPU (include/rmhmc_loo.h):
Pareto-smoothed importance sampling (PSIS-LOO) and WAIC over the rows the model was trained on, with the Pareto-k table that says which
rows the posterior hinges on.

    r = psis_loo(XX, t)      # r["elpd_loo"], r["se_elpd_loo"], r["p_loo"], r["pareto_k"] per row, r["elpd_waic"], ...

The draws come from fixed-metric HMC with the metric at the posterior mode as mass, started at the mode (the recipe of
predict.posterior_predictive); they stay in device memory, and so does the log-likelihood matrix, one block of columns at a time
(Context.loo): nothing but a handful of numbers per row crosses PCIe.  No CPU fallback.
"""
import numpy as np

from . import _capi


def psis_loo(XX, t, n_chains=1024, NumOfIterations=600, BurnIn=100, NumOfLeapFrogSteps=6, StepSize=0.5, alpha=100.0, seed=0,
             cols_per_block=0, _lib=None):
    """ PSIS-LOO AND WAIC OVER THE TRAINING ROWS (Bayesian logistic regression, N(0, alpha I) prior)

    XX (M, D), t (M,) with every entry 0 or 1: the training set, every entry of XX finite.  n_chains chains of NumOfIterations
    iterations, the first BurnIn dropped.  cols_per_block: the rows per block of the log-likelihood matrix, 0 .. 64 (0: the library
    chooses); the result does not depend on it.
    Returns a dict: elpd_loo, se_elpd_loo, p_loo, elpd_waic, se_elpd_waic, p_waic (totals); pareto_k [M]; pointwise: a dict of the
    arrays [M] elpd_loo, p_loo, lppd, p_waic, elpd_waic; draws_used [M]; k_mid, k_high (rows with khat in (0.5, 0.7] and above 0.7);
    accept, seconds (of the sampling run), info (mode, newton_iters, accepted [n_chains], seed)."""
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2 or XX.shape[0] < 1:
        raise ValueError("XX must be (M, D) with M >= 1")
    M, D = XX.shape
    if not 1 <= D <= _capi.LOO_MAX_D:
        raise ValueError("1 <= D <= %d" % _capi.LOO_MAX_D)
    if not np.isfinite(XX).all():
        raise ValueError("every entry of XX must be finite")
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != M:
        raise ValueError("t must have M entries")
    if not np.isin(t, (0.0, 1.0)).all():
        raise ValueError("every entry of t must be 0 or 1")
    if int(n_chains) != n_chains or n_chains < 1:
        raise ValueError("n_chains must be >= 1")
    if int(NumOfIterations) != NumOfIterations or int(BurnIn) != BurnIn or not 0 <= BurnIn < NumOfIterations:
        raise ValueError("need 0 <= BurnIn < NumOfIterations")
    if int(NumOfLeapFrogSteps) != NumOfLeapFrogSteps or NumOfLeapFrogSteps < 1:
        raise ValueError("NumOfLeapFrogSteps must be >= 1")
    if not (np.isfinite(StepSize) and StepSize > 0.0):
        raise ValueError("StepSize must be finite and > 0")
    if not (np.isfinite(alpha) and alpha > 0.0):
        raise ValueError("alpha must be finite and > 0")
    if int(cols_per_block) != cols_per_block or not 0 <= cols_per_block <= _capi.LOO_MAX_COLS:
        raise ValueError("0 <= cols_per_block <= %d" % _capi.LOO_MAX_COLS)
    lib = _lib if _lib is not None else _capi.load_hip_library()
    lib.need("loo")
    import torch
    with lib.context(M, D, int(n_chains)) as ctx:
        ctx.set_data(XX, t, alpha)
        md = ctx.phmc_mode()
        if not md["converged"]:
            raise RuntimeError("psis_loo: the Newton search for the posterior mode has not converged after %d iterations (last step %.3e)"
                               % (md["iters"], md["step"]))
        ctx.phmc_set_mass(md["G"])
        dev = torch.device("cuda", ctx.device) if lib.on_gpu else torch.device("cpu")
        st = ctx.phmc_sample_to(int(NumOfIterations), int(BurnIn), L=int(NumOfLeapFrogSteps), eps=float(StepSize), where="device", device=dev,
                                samples=True, seed=seed, theta0=md["w"])
        r = ctx.loo(st["samples"], XX, t, int(cols_per_block))
        accepted = st["accepted"].cpu().numpy()
    out = dict(r["totals"])
    out.update(pareto_k=r["pareto_k"], pointwise={k: r[k] for k in _capi.LOO_POINTWISE if k != "pareto_k"}, draws_used=r["draws_used"],
               k_mid=r["k_mid"], k_high=r["k_high"], accept=float(accepted.sum()) / (float(n_chains) * float(NumOfIterations)),
               seconds=st["seconds"], info=dict(mode=md["w"], newton_iters=md["iters"], accepted=accepted, seed=seed))
    return out
