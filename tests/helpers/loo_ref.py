"""np.longdouble restatement of include/rmhmc_loo.h, line by line: the log-likelihood matrix, its moments partial and the merge, the tail
length, the cutoff and the split, the generalised Pareto fit, the smoothed weights and the finish.  Written from the specification alone
(the header's comment).  tests/test_loo_cpu.py pins csrc/loo.h and this file's own fit to independent facts; tests/test_gpu_loo.py
compares the GPU with it."""
import numpy as np

LD = np.longdouble
MAX_TAIL = 16384


# ---- log-likelihood ---------------------------------------------------------------------------------------------------------------------
def loglik(samples, x, t):
    """For column c and draw k: f = x_c . w_k, s = f if t_c = 1 else -f, e = exp(-|f|), l = min(s, 0) - log1p(e).  A draw with any
    non-finite entry gets NaN in every column; a NaN f gives NaN.  samples [n][S][D] or [N][D] -> ll [N][C] in longdouble"""
    w = np.asarray(samples, dtype=np.float64)
    w = w.reshape(-1, w.shape[-1])
    ok = np.isfinite(w).all(axis=1)
    wl = np.where(ok[:, None], w, 0.0).astype(LD)
    x = np.asarray(x, dtype=LD)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.zeros((wl.shape[0], x.shape[0]), dtype=LD)
        for d in range(x.shape[1]):       # (no BLAS for long double: column by column)
            f += wl[:, d:d + 1] * x[None, :, d]
        s = np.where((t == 1.0)[None, :], f, -f)
        l = np.minimum(s, LD(0)) - np.log1p(np.exp(-np.abs(f)))
        l = np.where(np.isnan(f), LD(np.nan), l) + LD(0)
    l[~ok] = np.nan
    return l


def abs_product(samples, x):
    """A [N][C] of the error bound: sum_d |x_cd| |w_kd| per (draw, column), 0 for an invalid draw"""
    w = np.asarray(samples, dtype=np.float64)
    w = w.reshape(-1, w.shape[-1])
    ok = np.isfinite(w).all(axis=1)
    wl = np.abs(np.where(ok[:, None], w, 0.0)).astype(LD)
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(LD)
    A = np.zeros((wl.shape[0], x.shape[0]), dtype=LD)
    for d in range(x.shape[1]):
        A += wl[:, d:d + 1] * x[None, :, d]
    return A


# ---- moments ------------------------------------------------------------------------------------------------------------------------------
def identity(C):
    p = np.zeros((5, C), dtype=LD)
    p[4] = np.inf
    return p


def moments(ll):
    """Moments partial [5][C] of ll [N][C], every non-finite l left out of its own column: m, the mean of l, M2 = sum (l - mean)^2,
    SQ = sum exp(l), lmin"""
    ll = np.asarray(ll)
    ll = ll.reshape(-1, ll.shape[-1])
    out = identity(ll.shape[1])
    for c in range(ll.shape[1]):
        v = ll[:, c]
        v = v[np.isfinite(v)].astype(LD)
        if v.size == 0:
            continue
        mean = v.sum() / v.size
        out[:, c] = [v.size, mean, ((v - mean) ** 2).sum(), np.exp(v).sum(), v.min()]
    return out


def merge(a, b):
    """Chan's update for mean and M2, addition for m and SQ, min for lmin, column by column; m = 0 is the identity.  In the dtype of a"""
    a = np.array(a, copy=True)
    b = np.asarray(b)
    for c in range(a.shape[1]):
        ma, mb = a[0, c], b[0, c]
        if mb == 0:
            continue
        if ma == 0:
            a[:, c] = b[:, c]
            continue
        m = ma + mb
        delta = b[1, c] - a[1, c]
        a[:, c] = [m, a[1, c] + delta * (mb / m), (a[2, c] + b[2, c]) + delta * delta * (ma * (mb / m)), a[3, c] + b[3, c], min(a[4, c], b[4, c])]
    return a


# ---- tail length --------------------------------------------------------------------------------------------------------------------------
def tail_len(m):
    """M = min(floor(m / 5), r), r the smallest integer with r^2 >= 9 m (Python integers)"""
    import math
    m = int(m)
    r = math.isqrt(9 * m)
    if r * r < 9 * m:
        r += 1
    return min(m // 5, r)


def plan(m):
    """(tail_len [C], rank [C]: -1 where M < 5); None where an M is above MAX_TAIL"""
    M = [tail_len(v) for v in m]
    if any(v > MAX_TAIL for v in M):
        return None
    return np.array(M, dtype=np.int64), np.array([v if v >= 5 else -1 for v in M], dtype=np.int64)


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def gpd_fit(y):
    """Zhang and Stephens (2009) as PSIS uses it on y_1 <= .. <= y_M (longdouble, >= 0): (khat, sigma), or None where the tail is
    constant or mostly tied (y_M = 0 or y_q = 0, q = floor(M / 4 + 0.5))"""
    y = np.asarray(y, dtype=LD)
    M = y.size
    q = int(np.floor(M / 4 + 0.5))
    yM, yq = y[M - 1], y[q - 1]
    if yM == 0 or yq == 0:
        return None
    import math
    G = 30 + math.isqrt(M)
    i = np.arange(1, G + 1, dtype=LD)
    with np.errstate(all="ignore"):
        theta = 1 / yM + (1 - np.sqrt(G / (i - LD(0.5)))) / (3 * yq)
        kappa = np.array([np.log1p(-th * y).sum() / M for th in theta], dtype=LD)
        L = M * (np.log(-theta / kappa) - kappa - 1)
        omega = np.exp(L - L.max())
        omega = omega / omega.sum()
        th = (omega * theta).sum()
        k = np.log1p(-th * y).sum() / M
        sigma = -k / th
        khat = (k * M + 5) / (LD(M) + 10)
    return khat, sigma


def column(l, smooth=True):
    """One column from its l (any shape; non-finite values are left out): everything between the moments and the finish, in longdouble.
    Returns dict(m, M, cut, lmin, n_lt, n_gt, A_body, B_body, khat, sigma, A_tail, B_tail, elpd_loo)"""
    v = np.asarray(l).reshape(-1)
    v = np.sort(v[np.isfinite(v)]).astype(LD)
    m = v.size
    M = tail_len(m)
    out = dict(m=m, M=M, cut=np.nan, lmin=LD(np.inf), n_lt=0, n_gt=m, khat=LD(np.inf), sigma=LD(np.nan), A_tail=LD(0), B_tail=LD(0),
               A_body=LD(0), B_body=LD(0), elpd_loo=LD(np.nan))
    if m == 0:
        return out
    lmin = v[0]
    out["lmin"] = lmin
    if M < 5:                                  # no tail: every l is body
        out["A_body"] = np.exp(lmin - v).sum()
        out["B_body"] = m * np.exp(lmin)
    else:
        cut = v[M]                             # the order statistic of rank M, 0-based
        n_lt, n_gt = int((v < cut).sum()), int((v > cut).sum())
        n_eq = m - n_lt - n_gt
        r = M - n_lt
        out.update(cut=cut, n_lt=n_lt, n_gt=n_gt)
        out["A_body"] = np.exp(lmin - v[v > cut]).sum() + (n_eq - r) * np.exp(lmin - cut)
        out["B_body"] = (n_gt + n_eq - r) * np.exp(lmin)
        tail_l = np.concatenate([v[:n_lt], np.full(r, cut, dtype=LD)])[::-1]      # by ascending lw = lmin - l: l descending
        lw = lmin - tail_l
        lw_cut = lmin - cut
        y = np.expm1(lw - lw_cut)
        fit = gpd_fit(y) if smooth else None
        if fit is not None and np.isfinite(fit[0]) and np.isfinite(fit[1]):
            khat, sigma = fit
            p = (np.arange(1, M + 1, dtype=LD) - LD(0.5)) / M
            with np.errstate(all="ignore"):
                qj = -sigma * np.log1p(-p) if khat == 0 else sigma * np.expm1(-khat * np.log1p(-p)) / khat
                lw = np.minimum(lw_cut + np.log1p(qj), LD(0))
            out.update(khat=khat, sigma=sigma)
        out["A_tail"] = np.exp(lw).sum()
        out["B_tail"] = np.exp(lw + tail_l).sum()
    out["elpd_loo"] = np.log(out["B_tail"] + out["B_body"]) - np.log(out["A_tail"] + out["A_body"])
    return out


def columns(ll, smooth=True):
    """column() of every column of ll [N][C] -> (fit [4][C] = khat, sigma, A_tail, B_tail; body [2][C]; list of the dicts)"""
    ll = np.asarray(ll)
    ll = ll.reshape(-1, ll.shape[-1])
    cols = [column(ll[:, c], smooth) for c in range(ll.shape[1])]
    fit = np.array([[c[k] for c in cols] for k in ("khat", "sigma", "A_tail", "B_tail")], dtype=LD)
    body = np.array([[c[k] for c in cols] for k in ("A_body", "B_body")], dtype=LD)
    return fit, body, cols


# ---- finish -------------------------------------------------------------------------------------------------------------------------------
def total_se(v):
    v = np.asarray(v)
    dt = v.dtype.type
    total = dt(0)
    for x in v:
        total = total + x
    if v.size < 2:
        return total, dt(np.nan)
    mean = total / v.size
    return total, np.sqrt(v.size * (((v - mean) ** 2).sum() / (v.size - 1)))


def finish(partials, fit=None, body=None):
    """elpd_loo_c = log(B_tail + B_body) - log(A_tail + A_body), lppd_c = log(SQ / m), p_waic_c = M2 / (m - 1) (NaN for m < 2),
    elpd_waic_c = lppd_c - p_waic_c, p_loo_c = lppd_c - elpd_loo_c; totals in column order; se = sqrt(C var); the counts of khat in
    (0.5, 0.7] and above 0.7; m = 0 gives NaN.  In the dtype of the partials."""
    merged = identity(np.asarray(partials[0]).shape[1]).astype(np.asarray(partials[0]).dtype)
    for p in partials:
        merged = merge(merged, p)
    dt = merged.dtype.type
    C = merged.shape[1]
    m = merged[0]
    some = m > 0
    with np.errstate(all="ignore"):
        lppd = np.where(some, np.log(merged[3] / np.where(some, m, 1)), dt(np.nan))
        p_waic = np.where(m >= 2, merged[2] / np.where(m >= 2, m - 1, 1), dt(np.nan))
        if fit is None:
            elpd = np.full(C, np.nan, dtype=dt)
            khat = np.full(C, np.nan, dtype=dt)
        else:
            fit, body = np.asarray(fit, dtype=dt), np.asarray(body, dtype=dt)
            elpd = np.where(some, np.log(fit[3] + body[1]) - np.log(fit[2] + body[0]), dt(np.nan))
            khat = np.where(some, fit[0], dt(np.nan))
    out = dict(merged=merged, elpd_loo=elpd, p_loo=lppd - elpd, pareto_k=khat, lppd=lppd, p_waic=p_waic, elpd_waic=lppd - p_waic,
               draws_used=m.astype(np.int64), k_mid=int(((khat > 0.5) & (khat <= 0.7)).sum()), k_high=int((khat > 0.7).sum()))
    tot = {}
    tot["elpd_loo"], tot["se_elpd_loo"] = total_se(out["elpd_loo"])
    tot["p_loo"], _ = total_se(out["p_loo"])
    tot["elpd_waic"], tot["se_elpd_waic"] = total_se(out["elpd_waic"])
    tot["p_waic"], _ = total_se(out["p_waic"])
    out["totals"] = tot
    return out


def loo(samples, x, t, smooth=True):
    """the whole run: finish of the moments and the columns of loglik"""
    ll = loglik(samples, x, t).astype(np.float64)      # (ll is a matrix of doubles: every later stage starts from those)
    fit, body, _ = columns(ll, smooth)
    return finish([moments(ll)], fit, body)
