"""Drop-in counterpart of the reference's IWLS Metropolis-Hastings sampler, code/iwls.py (main.py:15,49).

    beta_saved, time = iwls(XX, t, alpha=100, max_iter=10000, burn_in=5000)

w = 0 (iwls.py:18).  Every iteration proposes from N(m(w), G(w)^-1), G = X'WX + I/alpha, m(w) = w + G^-1 grad(w) (the reference's
current_mean and current_cov, :33-35), and accepts by the Metropolis-Hastings ratio of the two proposal densities (:63-81).  Runs on the
MI355X through rmhmc_iwls_sample (include/rmhmc_iwls.h); the metric is assembled on the fp64 or the int8 matrix cores as for RMHMC
(int8_slices).  compat=True (the default) is the reference: its jittered log-determinant term and the rejection of every proposal with a
saturated row (W_j = 0, the reference's 0/0), which truncates the posterior to states without a row f_j > 36.7;
compat=False is the corrected sampler.  Every row of beta_saved is written (:84-85).  n_chains > 1 returns (n_chains, S, D);
return_info adds the accepted and saturated proposals per chain, the acceptance rate and the seed; summary / ess_nfft and diagnostics / max_lag as for RMHMC.  No CPU fallback.
"""
import numpy as np

from . import _capi


def iwls_progress_printer():
    """iwls.py:39-42: 'Iteration <i>' before iteration i for i % 1000 == 0, the banner before iteration burn_in"""
    def report(event, iters, accepted, iters_total):
        if event == _capi.EV_BURNIN_DONE:
            print("Burn-in complete, now drawing posterior samples.")
        else:
            print("Iteration %d" % iters)
    return report


def iwls(XX, t, alpha=100, max_iter=10000, burn_in=5000, *, n_chains=1, seed=None, theta0=None, compat=True, int8_slices=None,
         device=0, chain_offset=0, verbose=True, return_info=False, summary=False, ess_nfft="matlab", diagnostics=False,
         max_lag=None, _lib=None):
    """ IWLS METROPOLIS-HASTINGS (Bayesian logistic regression, N(0, alpha I) prior) """
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if not 0 <= burn_in < max_iter:
        raise ValueError("need 0 <= burn_in < max_iter")  # NameError in the reference (`start` unbound, iwls.py:88)
    if diagnostics and not return_info:
        raise ValueError("diagnostics=True returns its result in the info dict: it needs return_info=True")
    if diagnostics:
        _capi.diag_lags(max_iter - burn_in, max_lag)
    ess = _capi.ess_flags(ess_nfft)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 62))
    if verbose:
        print("--- Initialization...")
    lib = _lib if _lib is not None else _capi.load_hip_library()
    flags = _capi.auto_metric_flags(D, n_chains, int8_slices, M=N) | ess
    with lib.context(N, D, n_chains, flags=flags, device=device) as ctx:
        ctx.set_data(XX, t, float(alpha))
        if verbose:
            print("--- Iterating...")
            # (rmhmc_iwls_sample reports on the reference's own schedule, include/rmhmc_iwls.h: the context's first / every are not used)
            ctx.set_progress(iwls_progress_printer())
        st = None
        if diagnostics:   # (include/rmhmc_diag.h; as RMHMC)
            st = ctx.sample_to("iwls", max_iter, burn_in, samples=not summary, stats=summary, run_mean=summary, diagnostics=True,
                               max_lag=max_lag, compat=compat, seed=seed, chain_offset=chain_offset, theta0=theta0)
            samples, acc, sat, seconds = st.get("samples"), st["accepted"], st["saturated"], st["seconds"]
        elif summary:
            st = ctx.iwls_sample_stats(max_iter, burn_in, compat=compat, seed=seed, chain_offset=chain_offset, theta0=theta0,
                                       run_mean=True)
            samples, acc, sat, seconds = None, st["accepted"], st["saturated"], st["seconds"]
        else:
            samples, acc, sat, seconds = ctx.iwls_sample(max_iter, burn_in, compat=compat, seed=seed, chain_offset=chain_offset,
                                                         theta0=theta0)
    if verbose:
        print("--- Iterating: done.")
        print("Number of accepted samples: ", int(acc.sum()))
    beta_saved = {k: st[k] for k in _capi.SUMMARY_KEYS} if summary else samples[0] if n_chains == 1 else samples
    if return_info:
        return beta_saved, seconds, dict(accepted=acc, saturated=sat, acceptance=acc / float(max_iter), seed=seed, **_capi.diag_info(st, diagnostics))
    return beta_saved, seconds
