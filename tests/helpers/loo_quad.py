"""A D = 1 logistic regression whose leave-one-out predictive densities are known by quadrature: about 30 rows under the N(0, 100) prior,
one of them an outlier (x = 6 with the unlikely label).  Exact posterior draws by inverse CDF on a fine grid; the exact elpd_loo of
every row on the same grid.  Used by tests/test_loo_cpu.py (the restatement) and tests/test_gpu_loo.py (the GPU, psis_loo)."""
import numpy as np

import loo_ref as R

ALPHA = 100.0
ROWS = 30
SEED = 3            # of the data and of the draws: fixed, see test_loo_cpu.test_quadrature
N_CHAINS, N_DRAWS = 64, 400


def problem(seed=SEED):
    """x [ROWS][1], t [ROWS]: labels drawn at w = 0.5; the last row is the outlier"""
    rs = np.random.RandomState(1000 + seed)
    x = rs.randn(ROWS, 1)
    t = (rs.rand(ROWS) < 1.0 / (1.0 + np.exp(-0.5 * x[:, 0]))).astype(np.float64)
    x[-1, 0] = 6.0
    t[-1] = 0.0
    return x, t


def grid_loglik(x, t, lo=-6.0, hi=10.0, points=400001):
    """w [points], the log-likelihood of every row at every grid point [points][ROWS], and the log prior [points], in longdouble"""
    w = np.linspace(lo, hi, points).astype(R.LD)
    ll = R.loglik(np.asarray(w, dtype=np.float64)[:, None], x, t)
    return w, ll, -w * w / (2 * R.LD(ALPHA))


def exact_elpd(x, t):
    """elpd_loo_i = log(Z / Z_-i), Z the integral of prior times likelihood, Z_-i the same without row i: [ROWS], longdouble"""
    w, ll, lp = grid_loglik(x, t)
    tot = lp + ll.sum(axis=1)
    mx = tot.max()
    Z = np.exp(tot - mx).sum()
    return np.array([np.log(Z) - np.log(np.exp(tot - ll[:, i] - mx).sum()) for i in range(ll.shape[1])], dtype=R.LD)


def exact_draws(x, t, seed=SEED, n=N_CHAINS, S=N_DRAWS):
    """samples [n][S][1]: exact posterior draws by inverse CDF on the grid, linear between the grid points"""
    w, ll, lp = grid_loglik(x, t, points=40001)
    tot = (lp + ll.sum(axis=1)).astype(np.float64)
    dens = np.exp(tot - tot.max())
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]))])
    cdf /= cdf[-1]
    u = np.random.RandomState(2000 + seed).rand(n * S)
    return np.interp(u, cdf, np.asarray(w, dtype=np.float64)).reshape(n, S, 1)


def conditions(elpd_total_of, pareto_k, samples, x, t):
    """The three conditions of the quadrature test.  elpd_total_of(samples [n'][S'][1]) -> the total elpd_loo of those draws;
    pareto_k [ROWS] of all the draws.  Returns (difference in standard errors, the outlier's khat, the largest other khat) after
    asserting |difference| <= 5 standard errors, the standard error from the spread of eight interleaved eighths of the draws
    (sd / sqrt(8)), the outlier's khat the largest and above 0.5, every other below 0.5."""
    exact = float(exact_elpd(x, t).sum())
    flat = samples.reshape(-1, 1, 1)
    eighths = np.array([float(elpd_total_of(flat[i::8])) for i in range(8)])
    se = eighths.std(ddof=1) / np.sqrt(8.0)
    diff = (float(elpd_total_of(samples)) - exact) / se
    k = np.asarray(pareto_k, dtype=np.float64)
    print("quadrature: exact %.6f, difference %.3f standard errors (se %.4f), khat outlier %.3f, next %.3f" % (exact, diff, se, k[-1], k[:-1].max()))
    assert abs(diff) <= 5.0, (diff, se)
    assert k.argmax() == len(k) - 1 and k[-1] > 0.5 and k[:-1].max() < 0.5, k
    return diff, k[-1], k[:-1].max()
