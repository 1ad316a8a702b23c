"""Posterior predictive probabilities of Bayesian logistic regression under the N(0, alpha I) prior for rows that were not in the
training set, on the GPU (include/rmhmc_pred.h): p(t* = 1 | x*, data) = E_w sigmoid(x* . w) over posterior draws, its spread over the
draws, and the log pointwise predictive density of held-out labels.

    r = posterior_predictive(XX, t, Xnew, tnew)      # r["prob"], r["pvar"], r["lpd"] per row of Xnew, r["lpd_total"]

The draws come from fixed-metric HMC with the metric at the posterior mode as mass, started at the mode; they stay in device memory and
are reduced there (Context.predict): nothing but the [4, R] partial crosses PCIe.  No CPU fallback.
"""
import numpy as np

from . import _capi


def posterior_predictive(XX, t, Xnew, tnew=None, n_chains=1024, NumOfIterations=600, BurnIn=100, NumOfLeapFrogSteps=6, StepSize=0.5,
                         alpha=100.0, seed=0, _lib=None):
    """ POSTERIOR PREDICTIVE PROBABILITIES OF NEW ROWS (Bayesian logistic regression, N(0, alpha I) prior)

    XX (N, D), t (N,): the training set.  Xnew (R, D): the rows to predict, every entry finite.  tnew (R,) or None: held-out labels,
    each 0 or 1.  n_chains chains of NumOfIterations iterations, the first BurnIn dropped: n_chains * (NumOfIterations - BurnIn) draws.
    Returns a dict: prob [R] (p(t* = 1 | x*, data)), pvar [R] (the population variance of sigmoid(x* . w) over the draws), lpd [R] (log
    of the mean likelihood of tnew over the draws; NaN without labels), lpd_total, draws_used (draws with a non-finite entry are left
    out), partial (the mergeable [4, R] partial, a host array), accept (accepted proposals over all transitions), seconds (of the
    sampling run), info (mode, newton_iters, accepted [n_chains], seed)."""
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
    if Xnew.ndim != 2 or Xnew.shape[1] != D or Xnew.shape[0] < 1:
        raise ValueError("Xnew must be (R, D) with R >= 1 and the D of XX")
    if not np.isfinite(Xnew).all():
        raise ValueError("every entry of Xnew must be finite")
    if D > _capi.PRED_MAX_D:
        raise ValueError("D <= %d" % _capi.PRED_MAX_D)
    if tnew is not None:
        tnew = np.ascontiguousarray(tnew, dtype=np.float64).reshape(-1)
        if tnew.shape[0] != Xnew.shape[0]:
            raise ValueError("tnew must have R entries")
        if not np.isin(tnew, (0.0, 1.0)).all():
            raise ValueError("every entry of tnew must be 0 or 1")
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
    lib = _lib if _lib is not None else _capi.load_hip_library()
    import torch
    with lib.context(N, D, int(n_chains)) as ctx:
        ctx.set_data(XX, t, alpha)
        md = ctx.phmc_mode()
        if not md["converged"]:
            raise RuntimeError("posterior_predictive: the Newton search for the posterior mode has not converged after %d iterations "
                               "(last step %.3e)" % (md["iters"], md["step"]))
        ctx.phmc_set_mass(md["G"])
        dev = torch.device("cuda", ctx.device) if lib.on_gpu else torch.device("cpu")
        st = ctx.phmc_sample_to(int(NumOfIterations), int(BurnIn), L=int(NumOfLeapFrogSteps), eps=float(StepSize), where="device", device=dev,
                                samples=True, seed=seed, theta0=md["w"])
        r = ctx.predict(st["samples"], Xnew, tnew)
        accepted = st["accepted"].cpu().numpy()
        out = {k: r[k] for k in _capi.PRED_KEYS}
        out["partial"] = r["partial"].cpu().numpy()
    out.update(accept=float(accepted.sum()) / (float(n_chains) * float(NumOfIterations)), seconds=st["seconds"],
               info=dict(mode=md["w"], newton_iters=md["iters"], accepted=accepted, seed=seed))
    return out
