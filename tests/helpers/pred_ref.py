"""np.longdouble restatement of include/rmhmc_pred.h, line by line: the partial of the posterior predictive probabilities, its merge and
its finish.  Written from the specification alone (the header's comment).  tests/test_pred_cpu.py pins csrc/pred.h and this file's own
sigmoid to it; tests/test_gpu_pred.py compares the GPU with it."""
import numpy as np

LD = np.longdouble
TINY = np.ldexp(LD(1), -1075)


def used_draws(samples):
    """Invalid draws: a draw with any non-finite entry is left out of every row.  samples [n][S][D] or [N][D] -> the draws used [m][D]"""
    w = np.asarray(samples, dtype=np.float64)
    w = w.reshape(-1, w.shape[-1])
    return w[np.isfinite(w).all(axis=1)]


def probabilities(w, xnew):
    """Per row r and used draw k: f = x_r . w_k, e = exp(-|f|), hi = 1 / (1 + e), lo = e / (1 + e); p = f >= 0 ? hi : lo and
    1 - p = f >= 0 ? lo : hi, never by subtraction.  Returns (f, p, 1 - p), [R][m] each, in longdouble; a NaN f gives NaN."""
    w = np.asarray(w, dtype=LD)
    x = np.asarray(xnew, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.zeros((x.shape[0], w.shape[0]), dtype=LD)
        for d in range(x.shape[1]):       # (no BLAS for long double: column by column)
            f += x[:, d:d + 1] * w[None, :, d]
        e = np.exp(-np.abs(f))
        hi = 1 / (1 + e)
        lo = e / (1 + e)
        pos = f >= 0
        p = np.where(pos, hi, lo)
        np_ = np.where(pos, lo, hi)
        # the p and 1 - p of the specification are doubles: one that is below half the smallest of them, 2^-1075, has underflowed and
        # is 0 (that is when "every q underflowed" can happen; a long double alone would never say so)
        p = np.where(p < TINY, 0, p)
        np_ = np.where(np_ < TINY, 0, np_)
        nan = np.isnan(f)
        p[nan] = np.nan
        np_[nan] = np.nan
    return f, p, np_


def partial(samples, xnew, tnew=None):
    """Partial: [4][R] in longdouble: row 0 m (in every entry), row 1 S1 = sum_k p, row 2 S2 = sum_k p^2, row 3 SQ = sum_k q with
    q = tnew_r == 1 ? p : 1 - p; without labels row 3 is all zeros, written as -0.0"""
    xnew = np.asarray(xnew, dtype=np.float64)
    w = used_draws(samples)
    R = xnew.shape[0]
    out = np.zeros((4, R), dtype=LD)
    out[0] = w.shape[0]
    _, p, np_ = probabilities(w, xnew)
    out[1] = p.sum(axis=1)
    out[2] = (p * p).sum(axis=1)
    if tnew is None:
        out[3] = -0.0
    else:
        t = np.asarray(tnew, dtype=np.float64).reshape(-1)
        out[3] = np.where((t == 1.0)[:, None], p, np_).sum(axis=1)
    return out


def merge(a, b):
    """Two partials merge by adding all four rows; one with m = 0 is the identity"""
    if b[0, 0] == 0:
        return a.copy()
    if a[0, 0] == 0:
        return b.copy()
    return a + b


def finish(partials):
    """Finished: prob = S1 / m, pvar = max(0, S2 / m - prob^2), lpd = log(SQ / m) (-inf when every q underflowed, NaN without labels: SQ
    is -0.0), lpd_total = sum of lpd in row order; m = 0 gives NaN everywhere.  Computed in the dtype of the partials."""
    merged = np.zeros_like(np.asarray(partials[0]))
    for p in partials:
        merged = merge(merged, np.asarray(p))
    dt = merged.dtype.type
    m = merged[0, 0]
    R = merged.shape[1]
    nan = np.full(R, np.nan, dtype=dt)
    if m == 0:
        return dict(merged=merged, prob=nan, pvar=nan.copy(), lpd=nan.copy(), lpd_total=dt(np.nan), draws_used=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = merged[1] / m
        pvar = merged[2] / m - prob * prob
        pvar = np.where(pvar < 0, dt(0), pvar)
        no_labels = (merged[3] == 0) & np.signbit(merged[3])
        lpd = np.where(no_labels, dt(np.nan), np.log(merged[3] / m))
    total = dt(0)
    for v in lpd:
        total = total + v
    return dict(merged=merged, prob=prob, pvar=pvar, lpd=lpd, lpd_total=total, draws_used=int(m))


def predict(samples, xnew, tnew=None):
    return finish([partial(samples, xnew, tnew)])


def abs_product(samples, xnew):
    """A-bar [R] of the error bounds: the maximum over the used draws of sum_d |x_rd| |w_kd| (0 where no draw is used)"""
    w = np.abs(used_draws(samples)).astype(LD)
    x = np.abs(np.asarray(xnew, dtype=np.float64)).astype(LD)
    if w.shape[0] == 0:
        return np.zeros(x.shape[0], dtype=LD)
    A = np.zeros((x.shape[0], w.shape[0]), dtype=LD)
    for d in range(x.shape[1]):
        A += x[:, d:d + 1] * w[None, :, d]
    return A.max(axis=1)
