"""NumPy restatement of include/rmhmc_ais.h, written from the header alone on top of phmc_ref.py: the tempered log joint, the tempered
transition (one chain at a time, float64, explicit randomness: what the GPU is compared with), the weight partial and its merge and
finish in np.longdouble, the ladders, and the annealing run vectorised over chains with NumPy's own random numbers (a statistical
restatement: tests/test_ais_cpu.py holds its estimate to a quadrature of the evidence)."""
import math

import numpy as np

import phmc_ref as R

ST_NONFINITE = R.ST_NONFINITE
LD = np.longdouble


# ---- the tempered target ------------------------------------------------------------------------------------------------------------------
def loglik(X, t, w):
    """the likelihood part of the log joint, the naive log(1 + exp f) included"""
    f = X @ w
    with np.errstate(over="ignore", invalid="ignore"):
        return f @ np.ravel(t) - np.sum(np.log(1.0 + np.exp(f)))


def ljl_grad(X, t, w, beta, alpha=100.0):
    """(LJL_beta, grad_beta, loglik); at beta = 1 the first two are phmc_ref.ljl_grad's to the bit"""
    D = X.shape[1]
    t = np.ravel(t)
    f = X @ w
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = 1.0 / (1.0 + np.exp(-f))
        ll = f @ t - np.sum(np.log(1.0 + np.exp(f)))
        ljl = beta * ll - 0.5 * D * math.log(2.0 * math.pi * alpha) - (w @ w) / (2.0 * alpha)
        grad = beta * (X.T @ (t - p)) - w / alpha
    return ljl, grad, ll


def transition(X, t, Lm, w, z, u_len, u_acc, L, eps, beta, alpha=100.0):
    """phmc_ref.transition with LJL_beta and grad_beta; the dict gains loglik0 (at the start) and loglik (at the returned w)"""
    D = X.shape[1]
    w = np.array(w, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    if Lm is None:
        Lm = np.eye(D)
    p = Lm @ z
    ljl, grad, ll0 = ljl_grad(X, t, w, beta, alpha)
    H_cur = -ljl + 0.5 * (z @ z)
    ns = int(math.ceil(u_len * L))
    wn = w.copy()
    ll = ll0
    status = 0
    for _ in range(ns):
        p = p + eps / 2.0 * grad
        if np.isnan(p).any():
            status |= ST_NONFINITE
            break
        wn = wn + eps * R.mass_solve(Lm, p)
        ljl, grad, ll = ljl_grad(X, t, wn, beta, alpha)
        p = p + eps / 2.0 * grad
    with np.errstate(invalid="ignore", over="ignore"):
        q = R.solve_lower(Lm, p)
        H_prop = -ljl + 0.5 * (q @ q)
        ratio = H_cur - H_prop
    if not (np.isfinite(H_cur) and np.isfinite(H_prop)):
        status |= ST_NONFINITE
    accept = status == 0 and bool(ratio > 0 or ratio > math.log(u_acc))
    return dict(w=wn if accept else w, accepted=int(accept), nsteps=ns, H_cur=H_cur, H_prop=H_prop, w_prop=wn, p_prop=p, status=status,
                margin=ratio - min(0.0, math.log(u_acc)), loglik0=ll0, loglik=ll if accept else ll0)


def transitions(X, t, Lm, W, Z, u_len, u_acc, L, eps, beta, alpha=100.0):
    rows = [transition(X, t, Lm, W[c], Z[c], u_len[c], u_acc[c], L, eps, beta, alpha) for c in range(len(W))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def mode(X, t, beta, alpha=100.0, tol=1e-12, max_iter=100):
    """the mode of the tempered target by damped Newton from zero (phmc_ref.mode's scheme with LJL_beta and beta X' Lambda X + I / alpha)"""
    D = X.shape[1]
    w = np.zeros(D)
    for _ in range(max_iter):
        ljl, grad, _ = ljl_grad(X, t, w, beta, alpha)
        s = np.linalg.solve(beta * (R.metric(X, w, alpha) - np.eye(D) / alpha) + np.eye(D) / alpha, grad)
        if np.abs(s).max() <= tol * max(1.0, np.abs(w).max()):
            break
        for k in range(21):
            cand = w + s / 2.0 ** k
            if ljl_grad(X, t, cand, beta, alpha)[0] >= ljl:
                break
        w = cand
    return w


def stage_mass_matrix(beta, H_lik, alpha=100.0):
    return beta * np.asarray(H_lik) + np.eye(len(H_lik)) * (1.0 / alpha)


# ---- weights: the partial, its merge and finish, in np.longdouble -----------------------------------------------------------------------------
def partial(logw):
    """(m, n_nan, a, S1, S2) of include/rmhmc_ais.h as longdoubles"""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    nan = np.isnan(lw)
    used = lw[~nan].astype(LD)
    m, n_nan = used.size, int(nan.sum())
    if m == 0 or np.max(used) == -np.inf:
        return np.array([m, n_nan, -np.inf, 0.0, 0.0], dtype=LD)
    a = np.max(used)
    with np.errstate(under="ignore"):
        return np.array([m, n_nan, a, np.sum(np.exp(used - a)), np.sum(np.exp(2 * (used - a)))], dtype=LD)


def merge(parts):
    acc = np.array([0, 0, -np.inf, 0, 0], dtype=LD)
    for p in parts:
        p = np.asarray(p, dtype=LD)
        acc[1] += p[1]
        if p[0] == 0:
            continue
        if acc[0] == 0:
            acc[[0, 2, 3, 4]] = p[[0, 2, 3, 4]]
            continue
        a = max(acc[2], p[2])
        acc[0] += p[0]
        if a == -np.inf:
            acc[2:] = (a, 0, 0)
            continue
        with np.errstate(under="ignore"):
            acc[3] = acc[3] * np.exp(acc[2] - a) + p[3] * np.exp(p[2] - a)
            acc[4] = acc[4] * np.exp(2 * (acc[2] - a)) + p[4] * np.exp(2 * (p[2] - a))
        acc[2] = a
    return acc


def finish(parts):
    """dict(log_mean_w, se, weight_ess, m, n_nan, merged) as the header defines them"""
    acc = merge(parts)
    m, n_nan, a, S1, S2 = acc
    lm = se = ess = LD(np.nan)
    if m > 0 and S1 > 0:
        lm = a + np.log(S1 / m)
        ess = S1 * S1 / S2
        if m >= 2:
            se = np.sqrt(max(LD(0), (m * S2 / (S1 * S1) - 1) / (m - 1)))
    elif m > 0:
        lm = LD(-np.inf)
    return dict(log_mean_w=lm, se=se, weight_ess=ess, m=int(m), n_nan=int(n_nan), merged=acc)


# ---- ladders ----------------------------------------------------------------------------------------------------------------------------------
def ladder_power(T, q):
    b = ((np.arange(T, dtype=LD) + 1) / T) ** LD(q)
    b[-1] = 1
    return b


def ladder_log(T, beta_min):
    b = np.exp(np.log(LD(beta_min)) * (1 - (np.arange(T, dtype=LD) + 1) / T))
    b[-1] = 1
    return b


def stage_mass(T, every):
    return [1 if (k % every == 0 or k == T - 1) else 0 for k in range(T)]


# ---- the annealing run, vectorised over chains ----------------------------------------------------------------------------------------------
def _eval(X, t, W, beta, alpha):
    """rows of W: (LJL_beta [n], grad_beta [n][D], loglik [n])"""
    F = W @ X.T
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        P = 1.0 / (1.0 + np.exp(-F))
        ll = F @ t - np.log(1.0 + np.exp(F)).sum(axis=1)
        ljl = beta * ll - 0.5 * X.shape[1] * math.log(2.0 * math.pi * alpha) - (W * W).sum(axis=1) / (2.0 * alpha)
        grad = beta * ((t - P) @ X) - W / alpha
    return ljl, grad, ll


def run(X, t, n, beta, stage_len, H_lik, L=6, eps=0.5, alpha=100.0, seed=0):
    """rmhmc_ais_run from the prior (beta0 = 0) with a mass update in every stage (H_lik None: the identity throughout), NumPy's
    random numbers.  Returns dict(logw [n], theta [n][D], accept_trace [T])."""
    rs = np.random.RandomState(seed)
    t = np.ravel(t).astype(np.float64)
    D = X.shape[1]
    W = math.sqrt(alpha) * rs.randn(n, D)
    logw = np.zeros(n)
    prev = 0.0
    trace = np.zeros(len(beta))
    for k, b in enumerate(beta):
        Mass = stage_mass_matrix(b, H_lik, alpha) if H_lik is not None else np.eye(D)
        Lm = np.linalg.cholesky(Mass)
        Minv = np.linalg.inv(Mass)
        ljl, grad, ll = _eval(X, t, W, b, alpha)
        with np.errstate(invalid="ignore"):
            logw = np.where(np.isfinite(ll), logw + (b - prev) * ll, np.nan)
        acc_total = 0
        for _ in range(int(stage_len[k])):
            Z = rs.randn(n, D)
            ns = np.ceil(rs.rand(n) * L).astype(int)
            u_acc = rs.rand(n)
            Pm = Z @ Lm.T
            H_cur = -ljl + 0.5 * (Z * Z).sum(axis=1)
            Wn, gn, ljn, lln = W.copy(), grad.copy(), ljl.copy(), ll.copy()
            for s in range(L):
                act = ns > s
                if not act.any():
                    break
                Pa = Pm[act] + eps / 2.0 * gn[act]
                Wa = Wn[act] + eps * (Pa @ Minv)
                lj, g, l_ = _eval(X, t, Wa, b, alpha)
                Pm[act] = Pa + eps / 2.0 * g
                Wn[act], gn[act], ljn[act], lln[act] = Wa, g, lj, l_
            with np.errstate(invalid="ignore", over="ignore"):
                H_prop = -ljn + 0.5 * ((Pm @ Minv) * Pm).sum(axis=1)
                ratio = H_cur - H_prop
                ok = np.isfinite(H_cur) & np.isfinite(H_prop) & ~np.isnan(Pm).any(axis=1)
                accept = ok & ((ratio > 0) | (ratio > np.log(u_acc)))
            W[accept], grad[accept], ljl[accept], ll[accept] = Wn[accept], gn[accept], ljn[accept], lln[accept]
            acc_total += int(accept.sum())
        trace[k] = acc_total / (n * float(stage_len[k]))
        prev = b
    return dict(logw=logw, theta=W, accept_trace=trace)


# ---- the evidence by quadrature (D = 1, 2) ----------------------------------------------------------------------------------------------------
def log_evidence_quadrature(X, t, alpha=100.0, half_width=12.0, points=1201):
    """log of the integral of exp(LJL) over a grid of `points` per axis spanning +- half_width standard deviations of the Laplace
    approximation about the mode, along the axes of its Cholesky factor (rectangle rule: for a smooth integrand that has died out at
    the border it converges geometrically in the spacing, 0.02 standard deviations here; the tails are heavier than a Gaussian's, and
    tests/test_ais_cpu.py::test_quadrature_is_converged measures what the border and the spacing leave)."""
    D = X.shape[1]
    assert D in (1, 2)
    md = R.mode(X, t, alpha=alpha)
    Lc = np.linalg.cholesky(np.linalg.inv(md["G"]))
    u = np.linspace(-half_width, half_width, points)
    h = u[1] - u[0]
    U = u[:, None] if D == 1 else np.stack(np.meshgrid(u, u, indexing="ij"), axis=-1).reshape(-1, 2)
    W = md["w"] + U @ Lc.T
    t = np.ravel(t).astype(np.float64)
    out = []
    for i in range(0, len(W), 200000):
        F = W[i:i + 200000] @ X.T
        out.append(F @ t - np.logaddexp(0.0, F).sum(axis=1) - 0.5 * D * math.log(2.0 * math.pi * alpha)
                   - (W[i:i + 200000] ** 2).sum(axis=1) / (2.0 * alpha))
    lj = np.concatenate(out).astype(LD)
    a = lj.max()
    return float(a + np.log(np.sum(np.exp(lj - a))) + D * math.log(h) + np.log(np.diag(Lc)).sum())
