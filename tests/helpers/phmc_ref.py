"""NumPy restatement of include/rmhmc_phmc.h: HMC with a fixed dense mass matrix, and the damped Newton search for the posterior
mode.  Written from the specification alone (the header's comment), one chain at a time, in float64; its own Cholesky by
numpy.linalg.cholesky and its own triangular solves.  tests/test_phmc_cpu.py pins it to the CPU oracle's plain HMC with the
identity as mass matrix; tests/test_gpu_phmc.py compares the GPU with it."""
import math

import numpy as np

ST_NONFINITE = 2


def ljl_grad(X, t, w, alpha=100.0):
    """log joint and its gradient, the naive log(1 + exp f) included"""
    D = X.shape[1]
    t = np.ravel(t)
    f = X @ w
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = 1.0 / (1.0 + np.exp(-f))
        ljl = f @ t - np.sum(np.log(1.0 + np.exp(f))) - 0.5 * D * math.log(2.0 * math.pi * alpha) - (w @ w) / (2.0 * alpha)
        grad = X.T @ (t - p) - w / alpha
    return ljl, grad


def metric(X, w, alpha=100.0):
    """G = X' Lambda X + I / alpha, Lambda = diag p (1 - p): the metric, and minus the Hessian of the log joint"""
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-(X @ w)))
    return (X * (p * (1.0 - p))[:, None]).T @ X + np.eye(X.shape[1]) / alpha


def solve_lower(L, b):
    """x with L x = b, L lower triangular"""
    x = np.zeros_like(b, dtype=np.float64)
    for i in range(L.shape[0]):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def solve_upper(U, b):
    x = np.zeros_like(b, dtype=np.float64)
    for i in range(U.shape[0] - 1, -1, -1):
        x[i] = (b[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def mass_solve(Lm, p):
    """Mass^-1 p with Mass = Lm Lm'"""
    return solve_upper(Lm.T, solve_lower(Lm, p))


def transition(X, t, Lm, w, z, u_len, u_acc, L, eps, alpha=100.0):
    """one transition of one chain with explicit randomness; Lm None: the identity.  Returns a dict with the outputs of
    rmhmc_phmc_transition and margin = ratio - min(0, log u_acc), the distance of the decision from a tie."""
    D = X.shape[1]
    w = np.array(w, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    if Lm is None:
        Lm = np.eye(D)
    p = Lm @ z
    ljl, grad = ljl_grad(X, t, w, alpha)
    H_cur = -ljl + 0.5 * (z @ z)
    ns = int(math.ceil(u_len * L))
    wn = w.copy()
    status = 0
    for _ in range(ns):
        p = p + eps / 2.0 * grad
        if np.isnan(p).any():
            status |= ST_NONFINITE
            break
        wn = wn + eps * mass_solve(Lm, p)
        ljl, grad = ljl_grad(X, t, wn, alpha)
        p = p + eps / 2.0 * grad
    with np.errstate(invalid="ignore", over="ignore"):
        q = solve_lower(Lm, p)
        H_prop = -ljl + 0.5 * (q @ q)
        ratio = H_cur - H_prop
    if not (np.isfinite(H_cur) and np.isfinite(H_prop)):   # the log joint has overflowed: the chain fails
        status |= ST_NONFINITE
    accept = status == 0 and bool(ratio > 0 or ratio > math.log(u_acc))
    return dict(w=wn if accept else w, accepted=int(accept), nsteps=ns, H_cur=H_cur, H_prop=H_prop, w_prop=wn, p_prop=p, status=status,
                margin=ratio - min(0.0, math.log(u_acc)))


def transitions(X, t, Lm, W, Z, u_len, u_acc, L, eps, alpha=100.0):
    """the batch form: one dict of stacked outputs"""
    rows = [transition(X, t, Lm, W[c], Z[c], u_len[c], u_acc[c], L, eps, alpha) for c in range(len(W))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def mode(X, t, w0=None, max_iter=50, tol=1e-10, alpha=100.0):
    """damped Newton: s = G^-1 grad; stop when max|s| <= tol max(1, max|w|) or after max_iter steps; otherwise w += s / 2^k for the
    first k = 0..20 whose log joint is finite and >= the current one; none: stop.  Returns dict(w, G, iters, step, converged)."""
    D = X.shape[1]
    w = np.zeros(D) if w0 is None else np.array(w0, dtype=np.float64)
    it = 0
    while True:
        ljl, grad = ljl_grad(X, t, w, alpha)
        G = metric(X, w, alpha)
        Lg = np.linalg.cholesky(G)
        s = solve_upper(Lg.T, solve_lower(Lg, grad))
        step = float(np.abs(s).max())
        if not np.isfinite(step) or step <= tol * max(1.0, float(np.abs(w).max())) or it >= max_iter:
            break
        for k in range(21):
            cand = w + s / 2.0 ** k
            lc, _ = ljl_grad(X, t, cand, alpha)
            if np.isfinite(lc) and lc >= ljl:
                break
        else:
            break
        w = cand
        it += 1
    return dict(w=w, G=G, iters=it, step=step, converged=bool(step <= tol * max(1.0, float(np.abs(w).max()))))
