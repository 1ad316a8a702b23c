"""NumPy restatement of include/rmhmc_adapt.h: the covariance partial and its merge, the regularised mass, dual averaging of the step
size, the schedule and the windowed warm-up.  Written from the specification alone (the header's comment).  The warm-up runs on
phmc_ref.transitions with NumPy's own draws: it shares no random stream with the GPU and is compared with it statistically only.
tests/test_adapt_cpu.py pins csrc/adapt.h to it; tests/test_gpu_adapt.py compares the GPU with it."""
import math
from fractions import Fraction

import numpy as np

import phmc_ref  # (tests/helpers is on sys.path, as for the other helpers)

DEFAULTS = dict(delta=0.8, gamma=0.05, t0=10.0, kappa=0.75)


def partial(x):
    """the partial [(2 + P), P] of rows x [N][P], two passes in float64; rows with a non-finite entry are left out"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    P = x.shape[1]
    x = x[np.isfinite(x).all(axis=1)]
    out = np.zeros((2 + P, P))
    m = x.shape[0]
    out[0] = m
    if m:
        out[1] = x.mean(axis=0)
        xc = x - out[1]
        out[2:] = xc.T @ xc
    return out


def partial_longdouble(x):
    """(m, mean, C) of the finite rows of x [N][P], two passes in np.longdouble, and Sabs = sum_r |xc_ri| |xc_rj| for the error bound"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    x = x[np.isfinite(x).all(axis=1)].astype(np.longdouble)
    m, P = x.shape
    if m == 0:
        z = np.zeros((P, P), dtype=np.longdouble)
        return 0, np.zeros(P, dtype=np.longdouble), z, z
    mean = x.sum(axis=0) / m
    xc = x - mean
    C = np.zeros((P, P), dtype=np.longdouble)
    S = np.zeros((P, P), dtype=np.longdouble)
    ac = np.abs(xc)
    for i in range(P):   # (no BLAS for long double: column by column)
        C[i] = (xc[:, i:i + 1] * xc).sum(axis=0)
        S[i] = (ac[:, i:i + 1] * ac).sum(axis=0)
    return m, mean, C, S


def merge(a, b):
    """Chan's update of two partials; one with m = 0 is the identity"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ma, mb = a[0, 0], b[0, 0]
    if mb == 0:
        return a.copy()
    if ma == 0:
        return b.copy()
    m = ma + mb
    delta = b[1] - a[1]
    out = np.empty_like(a)
    out[0] = m
    out[1] = a[1] + delta * mb / m
    out[2:] = a[2:] + b[2:] + np.outer(delta, delta) * (ma * mb / m)
    return out


def finish(parts):
    """(merged, mean, cov, rows_used) of partials merged in the order given"""
    merged = np.zeros_like(np.asarray(parts[0], dtype=np.float64))
    for p in parts:
        merged = merge(merged, p)
    m = merged[0, 0]
    cov = merged[2:] / (m - 1.0) if m >= 2 else np.full_like(merged[2:], np.nan)
    return merged, merged[1].copy(), cov, int(m)


def shrink(cov, m):
    """Sigma_reg = m / (m + 5) cov + 1e-3 * 5 / (m + 5) I"""
    cov = np.asarray(cov, dtype=np.float64)
    return m / (m + 5.0) * cov + 1e-3 * (5.0 / (m + 5.0)) * np.eye(cov.shape[0])


def mass_from_cov(cov, m):
    """Mass = Sigma_reg^-1, or None where it is refused: m < 2, not finite, not positive definite"""
    if m < 2:
        return None
    sig = shrink(cov, m)
    if not np.isfinite(sig).all():
        return None
    try:
        np.linalg.cholesky(sig)
    except np.linalg.LinAlgError:
        return None
    mass = np.linalg.inv(sig)
    return 0.5 * (mass + mass.T)


def adapt_init(eps, factor=10.0):
    """the (re)start at eps: the iterates shrink towards mu = log(factor eps)"""
    return np.array([0.0, 0.0, 0.0, math.log(factor * eps)])


def adapt_step(state, accept, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75):
    """one dual-averaging update (Hoffman & Gelman 2014, section 3.2) of state = (t, Hbar, log epsbar, mu), in place;
    returns (eps_next, eps_bar)"""
    if not np.isfinite(accept):
        raise ValueError("non-finite acceptance statistic")
    t = state[0] + 1.0
    Hbar = (1.0 - 1.0 / (t + t0)) * state[1] + (delta - accept) / (t + t0)
    leps = state[3] - math.sqrt(t) / gamma * Hbar
    eta = t ** (-kappa)
    lbar = eta * leps + (1.0 - eta) * state[2]
    state[0], state[1], state[2] = t, Hbar, lbar
    return math.exp(leps), math.exp(lbar)


def schedule(warmup, window=25):
    """(win_len, win_kind): W = warmup // window windows; the first max(1, round(0.15 W)) and the last max(1, round(0.1 W)) of kind
    0, the rest of kind 1 (halves round up)"""
    W = warmup // window
    if W < 3:
        raise ValueError("W < 3")
    head = max(1, math.floor(Fraction(15, 100) * W + Fraction(1, 2)))
    tail = max(1, math.floor(Fraction(10, 100) * W + Fraction(1, 2)))
    return [window] * W, [0 if (w < head or w >= W - tail) else 1 for w in range(W)]


def run_window(X, t, Lm, W0, K, L, eps, rs, alpha=100.0):
    """K transitions of every chain from W0 [n][D] with NumPy's draws: (samples [n][K][D], accepted [n])"""
    n, D = W0.shape
    w = np.array(W0, dtype=np.float64)
    samples = np.empty((n, K, D))
    acc = np.zeros(n, dtype=np.int64)
    for k in range(K):
        r = phmc_ref.transitions(X, t, Lm, w, rs.standard_normal((n, D)), rs.random_sample(n), rs.random_sample(n), L, eps, alpha)
        w = r["w"]
        acc += r["accepted"]
        samples[:, k] = w
    return samples, acc


def warmup(X, t, n, win_len, win_kind, L=6, eps0=0.5, mass=None, min_rows=None, seed=0, alpha=100.0, **da):
    """the windowed warm-up of the header on phmc_ref.transitions: dict(step_size, mass, theta, eps_trace, accept_trace, mass_updated)"""
    da = dict(DEFAULTS, **da)
    D = X.shape[1]
    min_rows = 10 * D if min_rows is None else min_rows
    rs = np.random.RandomState(seed)
    Lm = None if mass is None else np.linalg.cholesky(mass)
    theta = np.zeros((n, D))
    state = adapt_init(eps0)
    eps, eps_bar = eps0, eps0
    running = np.zeros((2 + D, D))
    eps_trace, acc_trace, updated = [], [], []
    for K, kind in zip(win_len, win_kind):
        samples, acc = run_window(X, t, Lm, theta, K, L, eps, rs, alpha)
        theta = samples[:, -1].copy()
        a = acc.sum() / float(n * K)
        eps_trace.append(eps); acc_trace.append(a); updated.append(0)
        eps, eps_bar = adapt_step(state, a, **da)
        if kind != 1:
            continue
        running, _, cov, m = finish([running, partial(samples)])
        if m < min_rows:
            continue
        new = mass_from_cov(cov, m)
        if new is None:
            updated[-1] = -1
            continue
        mass, Lm = new, np.linalg.cholesky(new)
        running = np.zeros_like(running)
        state = adapt_init(eps, 1.0)
        updated[-1] = 1
    return dict(step_size=eps_bar, mass=mass, theta=theta, eps_trace=np.array(eps_trace), accept_trace=np.array(acc_trace),
                mass_updated=np.array(updated))
