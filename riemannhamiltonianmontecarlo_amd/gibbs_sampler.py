"""Drop-in counterpart of the reference's auxiliary-variable Gibbs sampler, code/gibbs_sampler.py (main.py:13,52).

    beta_saved, time = auxiliary_gibbs(XX, t, v=100, max_iter=10000, burn_in=5000)

The Holmes-Held sampler for Bayesian logistic regression with the prior N(0, v I): latent Z_j and mixing weights lam_j per row; every
iteration draws the rows' Z_j in order from their truncated normals (a joint update with B), beta = B + L T, and the lam_j by the
reference's rejection sampler (gibbs_sampler.py:14-70, both alternating series as the Python file writes them).  Runs on the MI355X
through rmhmc_gibbs_sample (include/rmhmc_gibbs.h), D <= 64, fp64 throughout.  Every row of beta_saved is written (:130-131).
n_chains > 1 returns (n_chains, S, D); return_info adds the capped rows per chain (rows that reached a bound of the mixing-weight
sampler, expected 0), the seed, and `stopped`: -1, or the iteration at which a chain met lam_j = inf from the reference's cancelling proposal
formula (about 3e-9 of all draws of a lam_j: N * max_iter * 3e-9 per chain and run, i.e. about 2 % of the chains of a default run on
australian, 690 rows x 10 000 iterations, and about a quarter of them at 10 000 rows x 10 000 iterations).  The reference ends in a
ValueError there; here that chain stops, its later rows of beta_saved are NaN (check `stopped`), the other chains go on.  summary / ess_nfft as
for RMHMC; the statistics of a stopped chain are NaN, and so are the rows of run_mean it did not reach; diagnostics / max_lag as for RMHMC.  No CPU fallback.
"""
import numpy as np

from . import _capi


def gibbs_progress_printer():
    """gibbs_sampler.py:97-98: 'Iteration <i>' at the top of every iteration i % 100 == 0"""
    def report(event, iters, accepted, iters_total):
        print("Iteration %d" % iters)
    return report


def auxiliary_gibbs(XX, t, v=100, max_iter=10000, burn_in=5000, *, n_chains=1, seed=None, device=0, chain_offset=0, verbose=True,
                    return_info=False, summary=False, ess_nfft="matlab", diagnostics=False, max_lag=None, _lib=None):
    """ AUXILIARY VARIABLE GIBBS SAMPLER (Bayesian logistic regression, N(0, v I) prior) """
    XX = np.ascontiguousarray(XX, dtype=np.float64)
    if XX.ndim != 2:
        raise ValueError("XX must be (N, D)")
    N, D = XX.shape
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] != N:
        raise ValueError("t must have N entries")
    if not 0 <= burn_in < max_iter:
        raise ValueError("need 0 <= burn_in < max_iter")  # NameError in the reference (`start` unbound, gibbs_sampler.py:137)
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
    with lib.context(N, D, n_chains, flags=ess, device=device) as ctx:   # (fp64 assembly: the int8 metric flags do not apply)
        ctx.set_data(XX, t, float(v))
        if verbose:
            print("--- Initialization: done. Iterating...")
            ctx.set_progress(gibbs_progress_printer())
        st = None
        if diagnostics:   # (include/rmhmc_diag.h; as RMHMC.  A stopped chain has NaN rows: it is left out, see chains_used)
            st = ctx.sample_to("gibbs", max_iter, burn_in, samples=not summary, stats=summary, run_mean=summary, diagnostics=True,
                               max_lag=max_lag, seed=seed, chain_offset=chain_offset)
            samples, capped, stopped, seconds = st.get("samples"), st["capped"], st["stopped"], st["seconds"]
        elif summary:
            st = ctx.gibbs_sample_stats(max_iter, burn_in, seed=seed, chain_offset=chain_offset, run_mean=True)
            samples, capped, stopped, seconds = None, st["capped"], st["stopped"], st["seconds"]
        else:
            r = ctx.gibbs_sample(max_iter, burn_in, seed=seed, chain_offset=chain_offset)
            samples, capped, stopped, seconds = r["samples"], r["capped"], r["stopped"], r["seconds"]
    if verbose:
        print("--- Iterating: done.")
        print("--- Auxiliary Variable Gibbs Sampler finished in {}".format(seconds))
    beta_saved = {k: st[k] for k in _capi.SUMMARY_KEYS} if summary else samples[0] if n_chains == 1 else samples
    if return_info:
        return beta_saved, seconds, dict(capped=capped, stopped=stopped, seed=seed, **_capi.diag_info(st, diagnostics))
    return beta_saved, seconds
