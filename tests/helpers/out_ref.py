"""Host references for the tests of the output descriptor (include/rmhmc_out.h): the existing *_sample call of every sampler in one
shape, and the ESS reference with the guard that makes a 1e-9 comparison of an ESS meaningful."""
import numpy as np

from riemannhamiltonianmontecarlo_amd import tools

# sampler of _capi.SAMPLERS_TO -> (the existing Context method, the keys of what it returns after the samples; None: it returns a dict)
EXISTING = {
    "rmhmc": ("sample", ("accepted", "leapfrog_steps", "seconds")),
    "hmc": ("hmc_sample", ("accepted", "leapfrog_steps", "seconds")),
    "mmala": ("mmala_sample", ("accepted", "seconds")),
    "amh": ("amh_sample", ("accepted", "sd", "seconds")),
    "iwls": ("iwls_sample", ("accepted", "saturated", "seconds")),
    "gibbs": ("gibbs_sample", None),
}


def existing_call(ctx, sampler, n_iter, burn_in, **kw):
    """the sampler's existing entry point as a dict(samples, its counters, seconds)"""
    method, keys = EXISTING[sampler]
    r = getattr(ctx, method)(n_iter, burn_in, **kw)
    if keys is None:
        return dict(r)
    return dict(zip(("samples",) + keys, r))


def host(x):
    """a NumPy array of a NumPy array or a torch tensor on any device"""
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def geyer_margin(x, nfft):
    """x (S, P): for every column the smallest |Gamma_j| over the Geyer pairs up to and including the one the sum stops at (the first whose
    running minimum is not positive, tools.py:54-67; all of them when none is).  Two series that differ in their last bits have the
    same stopping pair when this is far from 0 - and only then can their ESS be compared to 1e-9."""
    x = np.asarray(x, dtype=np.float64)
    S, P = x.shape
    acs = np.stack([tools.ac(x[:, i], S - 1, nfft) for i in range(P)], axis=1)
    half = S // 2
    gamma = np.minimum.accumulate(acs[0:2 * half:2] + acs[1:2 * half:2], axis=0)
    out = np.empty(P)
    for i in range(P):
        stop = np.nonzero(~(gamma[:, i] > 0))[0]
        last = stop[0] if len(stop) else half - 1
        out[i] = np.abs(gamma[: last + 1, i]).min()
    return out


def ess_ref(x, nfft, guard=False):
    """tools.CalculateESS(x, S-1, nfft) as a flat (P,) array; guard: the stopping pair of every column is well away from 0"""
    x = np.asarray(x, dtype=np.float64)
    if guard:
        m = geyer_margin(x, nfft)
        assert (m > 1e-6).all(), "a Geyer pair sum within 1e-6 of 0: choose another seed (%r)" % (m,)
    return tools.CalculateESS(x, x.shape[0] - 1, nfft).ravel()
