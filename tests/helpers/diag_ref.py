"""NumPy restatement of the cross-chain diagnostics of include/rmhmc_diag.h, written as plain float64 loops over the series and the
lags: the partial of samples [n][S][P], the merge of two partials, and the finish (split R-hat, pooled ESS, Geyer pairs) with the margin
that tells whether `pairs` can be compared exactly.  Also the AR(1) inputs of the tests."""
import numpy as np


def ar1(seed, n, S, P, phi=None):
    """x_s = phi x_{s-1} + e_s, e ~ N(0, 1), stationary start, plus a per-dimension offset: [n][S][P] with phi = linspace(-0.4, 0.9, P) and
    offsets linspace(-3, 100, P)"""
    rng = np.random.default_rng(seed)
    phi = np.linspace(-0.4, 0.9, P) if phi is None else np.broadcast_to(np.asarray(phi, dtype=np.float64), (P,))
    e = rng.standard_normal((n, S, P))
    x = np.empty((n, S, P))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x + np.linspace(-3.0, 100.0, P)


def lags(S, max_lag=None):
    H = S // 2
    return H, (max_lag if max_lag else H - 1) + 1


def partial(x, T):
    """[(4 + T), P]: row 0 the series used, 1 the mean of their means, 2 M2, 3 the sum of s2_j, 4 + t the sum of acov_j(t)"""
    x = np.asarray(x, dtype=np.float64)
    n, S, P = x.shape
    H = S // 2
    out = np.zeros((4 + T, P))
    for d in range(P):
        means = []
        for c in range(n):
            for half in (x[c, :H, d], x[c, S - H:, d]):
                if not np.isfinite(half).all():
                    continue
                mu = half.sum() / H
                z = half - mu                                  # centred first, never E[x^2] - E[x]^2
                acov = np.array([np.dot(z[: H - t], z[t:]) / H for t in range(T)])
                means.append(mu)
                out[3, d] += acov[0] * H / (H - 1)
                out[4:, d] += acov
        m = len(means)
        out[0, d] = m
        if m:
            means = np.array(means)
            out[1, d] = means.sum() / m
            out[2, d] = ((means - out[1, d]) ** 2).sum()
    return out


def merge(a, b):
    """Chan's update of rows 1 and 2, the other rows add; a partial with m = 0 is the identity"""
    a = np.array(a, dtype=np.float64)
    for d in range(a.shape[1]):
        ma, mb = a[0, d], b[0, d]
        if mb == 0:
            continue
        if ma == 0:
            a[:, d] = b[:, d]
            continue
        m = ma + mb
        delta = b[1, d] - a[1, d]
        a[0, d] = m
        a[1, d] = a[1, d] + delta * mb / m
        a[2, d] = a[2, d] + b[2, d] + delta * delta * ma * mb / m
        a[3:, d] += b[3:, d]
    return a


def finish(part, H):
    """dict(rhat, ess, pairs, used, margin) [P] each; margin: the smallest of |Gamma_k| and |Gamma_k - running minimum before it| over the
    pairs visited (the stopping one included): `pairs` is comparable exactly only where this is well above rounding"""
    part = np.asarray(part, dtype=np.float64)
    T, P = part.shape[0] - 4, part.shape[1]
    rhat = np.full(P, np.nan); ess = np.full(P, np.nan); margin = np.full(P, np.inf)
    pairs = np.zeros(P, dtype=np.int64); used = part[0].astype(np.int64)
    for d in range(P):
        m = part[0, d]
        if m < 2:
            continue
        W = part[3, d] / m
        if not W > 0:
            continue
        varp = W * (H - 1) / H + part[2, d] / (m - 1)
        rhat[d] = np.sqrt(varp / W)
        rho = 1.0 - (W - part[4:, d] / m) / varp
        rho[0] = 1.0
        prev, total, k = np.inf, 0.0, 0
        while 2 * k + 1 < T:
            g = rho[2 * k] + rho[2 * k + 1]
            margin[d] = min(margin[d], abs(g), abs(g - prev))
            g = min(g, prev)
            if not g > 0:
                break
            total += g
            prev = g
            k += 1
        ess[d] = m * H / max(1.0, -1.0 + 2.0 * total)
        pairs[d] = k
    return dict(rhat=rhat, ess=ess, pairs=pairs, used=used, margin=margin)
