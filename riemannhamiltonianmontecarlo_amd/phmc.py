"""HMC with a fixed dense mass matrix shared by all chains (include/rmhmc_phmc.h): the sampler between plain HMC
(identity mass, hmc.py) and RMHMC (position-dependent metric, rmhmc.py).

    wSaved, TimeTaken = PHMC(XX, t, NumOfIterations=6000, BurnIn=1000, NumOfLeapFrogSteps=6, StepSize=0.5)

The default mass matrix is the metric G = X' Lambda X + I / alpha at the posterior mode, found by a damped Newton search on
the GPU (Context.phmc_mode).  With a constant metric the generalised leapfrog of RMHMC is this integrator, hence RMHMC's step
size and trajectory length as defaults (rmhmc.py:13).  The reference has no such sampler; theta0 = 0, the trajectory length
ceil(rand*NumOfLeapFrogSteps) and the acceptance rule are plain HMC's (hmc.py:27,48,77), and so are the keyword-only
extensions, the return shapes and the row-0 convention of riemannhamiltonianmontecarlo_amd.hmc.HMC.  No CPU fallback.
"""
import numpy as np

from . import _capi


def PHMC(XX, t, NumOfIterations=6000, BurnIn=1000, NumOfLeapFrogSteps=6, StepSize=0.5, *, mass="mode", n_chains=1, seed=None,
         theta0=None, alpha=100.0, device=0, chain_offset=0, verbose=True, return_info=False, options=None, summary=False,
         ess_nfft="matlab", diagnostics=False, max_lag=None, warmup=0, target_accept=0.8, window=25, _lib=None):
    """ HAMILTONIAN MONTE CARLO WITH A FIXED DENSE MASS MATRIX (Bayesian logistic regression, N(0, alpha I) prior)

    mass: "mode" (the metric at the posterior mode), "identity" (plain HMC) or a (D, D) symmetric positive definite array.
    theta0: None (zeros, as HMC), "mode" (every chain starts at the posterior mode) or an array broadcastable to (n_chains, D).
    info (return_info=True) carries, besides HMC's entries, mode (the posterior mode, or None when it was not searched), mass (the
    matrix in use, None for the identity) and newton_iters.
    warmup > 0: a windowed warm-up (include/rmhmc_adapt.h) of warmup // window windows of `window` iterations runs first, from `mass`,
    StepSize and theta0: dual averaging moves the acceptance rate of a window towards target_accept, and the windows in the middle
    of the schedule (_capi.adapt_schedule) replace the mass by the inverse of the shrunk pooled covariance of all chains once
    10 D rows are pooled.  The sampling run then starts from the last positions of the warm-up (its BurnIn still applies) with the
    adapted step size and mass; info gains step_size, warmup (eps_trace, accept_trace, mass_updated, seconds) and mass is the
    adapted one.  warmup=0: nothing of this runs, and every return value is what it is without the keyword."""
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if not BurnIn < NumOfIterations:
        raise ValueError("BurnIn must be smaller than NumOfIterations")
    if diagnostics and not return_info:
        raise ValueError("diagnostics=True returns its result in the info dict: it needs return_info=True")
    if diagnostics:
        _capi.diag_lags(NumOfIterations - BurnIn, max_lag)
    ess = _capi.ess_flags(ess_nfft)
    schedule = None
    if warmup != 0:
        if int(warmup) != warmup or warmup < 0:
            raise ValueError("warmup must be a number of iterations >= 0")
        if not 0.0 < target_accept < 1.0:
            raise ValueError("target_accept must lie in (0, 1)")
        schedule = _capi.adapt_schedule(warmup, window)
    if isinstance(mass, str):
        if mass not in ("mode", "identity"):
            raise ValueError('mass must be "mode", "identity" or a (D, D) array')
    else:
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        if mass.shape != (D, D):
            raise ValueError('mass must be "mode", "identity" or a (D, D) array')
    if isinstance(theta0, str) and theta0 != "mode":
        raise ValueError('theta0 must be None, "mode" or an array')
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 62))
    lib = _lib if _lib is not None else _capi.load_hip_library()
    with lib.context(N, D, n_chains, flags=ess, device=device, options=options) as ctx:
        ctx.set_data(XX, t, alpha)
        mode, iters = None, 0
        if (isinstance(mass, str) and mass == "mode") or isinstance(theta0, str):
            md = ctx.phmc_mode()
            if not md["converged"]:
                raise RuntimeError("PHMC: the Newton search for the posterior mode has not converged after %d iterations "
                                   "(last step %.3e)" % (md["iters"], md["step"]))
            mode, iters = md["w"], md["iters"]
            if isinstance(mass, str) and mass == "mode":
                mass = md["G"]
        if isinstance(mass, str):   # "identity"
            mass = None
        ctx.phmc_set_mass(mass)
        if isinstance(theta0, str):
            theta0 = mode
        warm = None
        if schedule is not None:   # (before the progress printer is set: the warm-up prints nothing)
            warm = ctx.phmc_warmup(*schedule, L=NumOfLeapFrogSteps, eps0=StepSize, delta=target_accept, seed=seed, chain_offset=chain_offset,
                                   theta0=theta0)
            StepSize, theta0 = warm["step_size"], warm["theta"]
            if warm["mass"] is not None:
                mass = warm["mass"]
        if verbose:  # HMC's stdout, hmc.py:85-89,92-94
            from .rmhmc import progress_printer
            ctx.set_progress(progress_printer(n_chains, hmc_burn_in=BurnIn), first=1, every=50)
        kw = dict(L=NumOfLeapFrogSteps, eps=StepSize, seed=seed, chain_offset=chain_offset, theta0=theta0)
        if diagnostics:   # the samples stay on the device for the cross-chain diagnostics (include/rmhmc_diag.h)
            import torch
            dev = torch.device("cuda", ctx.device) if lib.on_gpu else torch.device("cpu")
            st = ctx.phmc_sample_to(NumOfIterations, BurnIn, where="device", device=dev, samples=True, stats=summary, run_mean=summary, **kw)
            dg = ctx.diagnose(st["samples"], max_lag)
            if summary:
                del st["samples"]
            st = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in st.items()}
            st.update({k: dg[k] for k in _capi.DIAG_KEYS})
        else:
            st = ctx.phmc_sample_to(NumOfIterations, BurnIn, samples=not summary, stats=summary, run_mean=summary, **kw)
        samples, acc, steps, seconds = st.get("samples"), st["accepted"], st["leapfrog_steps"], st["seconds"]
    if verbose:
        print('Time drawing posterior: {}'.format(seconds))
    wSaved = {k: st[k] for k in _capi.SUMMARY_KEYS} if summary else samples[0] if n_chains == 1 else samples
    if return_info:
        extra = {} if warm is None else dict(step_size=StepSize, warmup={k: warm[k] for k in ("eps_trace", "accept_trace", "mass_updated",
                                                                                             "seconds")})
        return wSaved, seconds, dict(accepted=acc, leapfrog_steps=steps, seed=seed, mode=mode, mass=mass, newton_iters=iters,
                                     **_capi.diag_info(st, diagnostics), **extra)
    return wSaved, seconds
