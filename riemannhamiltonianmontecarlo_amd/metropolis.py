"""Drop-in counterpart of the reference's component-wise adaptive Metropolis sampler, code/metropolis.py (AMH, the baseline of the
paper's comparison tables).

    wSaved, TimeTaken = AMH(XX, t, NumOfIterations=10000, BurnIn=5000)

w = 0, ProposalSD = 1 (metropolis.py:24-29), one Gaussian proposal per coordinate per iteration, SD adapted every 100 iterations of
the burn-in (iteration 0 included).  Runs on the MI355X through rmhmc_amh_sample (include/rmhmc_amh.h); same keyword-only extensions
and the same row-0 convention as riemannhamiltonianmontecarlo_amd.hmc.HMC (row 0 = state after iteration BurnIn; the reference never
writes it).  return_info adds the per-chain acceptance rate over the whole run and the final ProposalSD; summary / ess_nfft and diagnostics / max_lag as for RMHMC.  No CPU fallback.
"""
import numpy as np

from . import _capi


def amh_progress_printer():
    """metropolis.py:73-74,92-94: '<i> iterations completed.' after iteration i for i % 1000 == 0, i < BurnIn, then the banner"""
    def report(event, iters, accepted, iters_total):
        if event == _capi.EV_BURNIN_DONE:
            print('Burn-in complete, now drawing posterior samples.')
        else:
            print('{} iterations completed.'.format(iters))
    return report


def AMH(XX, t, NumOfIterations=10000, BurnIn=5000, *, n_chains=1, seed=None, theta0=None, alpha=100.0, device=0, chain_offset=0,
        verbose=True, return_info=False, summary=False, ess_nfft="matlab", diagnostics=False, max_lag=None, _lib=None):
    """ ADAPTIVE METROPOLIS HASTING (Bayesian logistic regression, N(0, alpha I) prior) """
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if not 0 <= BurnIn < NumOfIterations:
        raise ValueError("BurnIn must be smaller than NumOfIterations")  # NameError in the reference (metropolis.py:93)
    if diagnostics and not return_info:
        raise ValueError("diagnostics=True returns its result in the info dict: it needs return_info=True")
    if diagnostics:
        _capi.diag_lags(NumOfIterations - BurnIn, max_lag)
    ess = _capi.ess_flags(ess_nfft)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 62))
    lib = _lib if _lib is not None else _capi.load_hip_library()
    with lib.context(N, D, n_chains, flags=ess, device=device) as ctx:
        ctx.set_data(XX, t, alpha)
        if verbose:
            # (rmhmc_amh_sample reports on the reference's own schedule, include/rmhmc_amh.h: the context's first / every are not used)
            ctx.set_progress(amh_progress_printer())
        st = None
        if diagnostics:   # (include/rmhmc_diag.h; as RMHMC)
            st = ctx.sample_to("amh", NumOfIterations, BurnIn, samples=not summary, stats=summary, run_mean=summary, diagnostics=True,
                               max_lag=max_lag, seed=seed, chain_offset=chain_offset, theta0=theta0)
            samples, acc, sd, seconds = st.get("samples"), st["accepted"], st["sd"], st["seconds"]
        elif summary:
            st = ctx.amh_sample_stats(NumOfIterations, BurnIn, seed=seed, chain_offset=chain_offset, theta0=theta0, run_mean=True)
            samples, acc, sd, seconds = None, st["accepted"], st["sd"], st["seconds"]
        else:
            samples, acc, sd, seconds = ctx.amh_sample(NumOfIterations, BurnIn, seed=seed, chain_offset=chain_offset, theta0=theta0)
    if verbose:
        print('Time drawing posterior: {}'.format(seconds))
    wSaved = {k: st[k] for k in _capi.SUMMARY_KEYS} if summary else samples[0] if n_chains == 1 else samples
    if return_info:
        return wSaved, seconds, dict(acceptance=acc / float(NumOfIterations * D), accepted=acc, ProposalSD=sd, seed=seed, **_capi.diag_info(st, diagnostics))
    return wSaved, seconds
