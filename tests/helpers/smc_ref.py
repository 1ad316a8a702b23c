"""Restatement of include/rmhmc_smc.h, written from the header on top of ais_ref.py: the conditional-ESS partial, its merge and finish in
np.longdouble; the candidate grids and the bracket rule of the search in float64 (the header fixes every rounding); the reweighting;
the quantised weights and systematic resampling in Python integers; the refusals; and the run vectorised over particles with NumPy's
own random numbers (a statistical restatement: tests/test_smc_cpu.py holds its estimate to a quadrature of the evidence)."""
import math

import numpy as np

import ais_ref as A

LD = np.longdouble
MAX_J, J, ROUNDS, MAX_N, QBITS = 32, 16, 3, 2 ** 20, 40
LAST, FLOOR, RESAMPLED = 1, 2, 4
NEG_INF = LD(-np.inf)


# ---- 1. conditional ESS ---------------------------------------------------------------------------------------------------------------------
def _pair(x):
    """(a, S) of a set of exponents (longdoubles): the maximum and sum exp(x - a); (-inf, 0) for an empty set or one of -inf alone"""
    if x.size == 0 or np.max(x) == -np.inf:
        return NEG_INF, LD(0)
    a = np.max(x)
    with np.errstate(under="ignore"):
        return a, np.sum(np.exp(x - a))


def cess_partial(logw, loglik, delta):
    """the partial [2 + 4 J] in longdouble, the products and sums of the exponents exact to the longdouble's own rounding"""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    ll = np.asarray(loglik, dtype=np.float64).ravel()
    used = ~np.isnan(lw)
    both = used & np.isfinite(ll)
    out = list(_pair(lw[used].astype(LD)))
    x, l = lw[both].astype(LD), ll[both].astype(LD)
    for d in np.asarray(delta, dtype=np.float64).ravel():
        with np.errstate(invalid="ignore", over="ignore"):
            t = LD(d) * l
            out += list(_pair(x + t)) + list(_pair(x + 2 * t))
    return np.array(out, dtype=LD)


def cess_merge(parts):
    parts = [np.asarray(p, dtype=LD) for p in parts]
    acc = np.array([NEG_INF, 0] * (len(parts[0]) // 2), dtype=LD)
    for p in parts:
        for i in range(0, len(p), 2):
            if p[i] == -np.inf:
                continue
            if acc[i] == -np.inf:
                acc[i], acc[i + 1] = p[i], p[i + 1]
                continue
            a = max(acc[i], p[i])
            with np.errstate(under="ignore"):
                acc[i + 1] = acc[i + 1] * np.exp(acc[i] - a) + p[i + 1] * np.exp(p[i] - a)
            acc[i] = a
    return acc


def cess_levels(part):
    """L = a + log S of every pair, -inf where S = 0"""
    part = np.asarray(part, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(part[1::2] > 0, part[0::2] + np.log(part[1::2]), NEG_INF)


def cess_finish(parts):
    """dict(frac [J], merged)"""
    acc = cess_merge(parts)
    L = cess_levels(acc)
    frac = np.full((len(acc) - 2) // 4, np.nan, dtype=LD)
    for j in range(len(frac)):
        if acc[1] > 0 and acc[3 + 4 * j] > 0:
            frac[j] = np.exp(2 * L[1 + 2 * j] - L[0] - L[2 + 2 * j])
    return dict(frac=frac, merged=acc)


def cess_brute(logw, loglik, delta):
    """cess / n of one step from normalised weights: (sum W w)^2 / (sum W w^2), W summing to 1, w = exp(delta l) (0 for a failed particle)"""
    lw = np.asarray(logw, dtype=LD)
    ll = np.asarray(loglik, dtype=np.float64)
    W = np.exp(lw - lw.max())
    W = W / W.sum()
    fin = np.isfinite(ll)
    lmax = ll[fin].max()
    w = np.where(fin, np.exp(LD(delta) * (np.where(fin, ll, 0.0).astype(LD) - lmax)), LD(0))      # (a common factor of w cancels)
    return (W * w).sum() ** 2 / (W * w * w).sum()


# ---- 2. the search ----------------------------------------------------------------------------------------------------------------------------
def grid(rnd, remaining, lo, hi):
    """the J candidates of a round, float64 to the bit"""
    if rnd == 0:
        return np.array([math.ldexp(remaining, -3 * (J - 1 - j)) for j in range(J)])
    lo, hi = np.float64(lo), np.float64(hi)
    out = [lo + (hi - lo) * np.float64((j + 1) / 16.0) for j in range(J)]
    out[-1] = hi
    return np.array(out, dtype=np.float64)


def bracket(rnd, delta, frac, rho, lo, lo_frac, hi):
    """one application of the rule: (js, lo, lo_frac, hi); js = J: no candidate failed"""
    js = 0
    while js < J and frac[js] >= rho:       # (a NaN fails)
        js += 1
    if js == J:
        return js, delta[-1], frac[-1], delta[-1]
    if js > 0:
        lo, lo_frac = delta[js - 1], frac[js - 1]
    return js, lo, lo_frac, delta[js]


def search(frac_of, remaining, rho):
    """frac_of(delta [J]) -> frac [J].  dict(delta, frac, flags, rounds: [(grid, frac, js)])"""
    lo, lo_frac, hi = 0.0, math.nan, remaining
    rounds = []
    for rnd in range(ROUNDS):
        d = grid(rnd, remaining, lo, hi)
        f = np.asarray(frac_of(d), dtype=np.float64)
        if rnd == 0:
            floor_delta, floor_frac = d[0], f[0]
        js, lo, lo_frac, hi = bracket(rnd, d, f, rho, lo, lo_frac, hi)
        rounds.append((d, f, js))
        if rnd == 0 and js == J:
            return dict(delta=remaining, frac=f[-1], flags=LAST, rounds=rounds)
    if lo > 0.0:
        return dict(delta=float(lo), frac=float(lo_frac), flags=0, rounds=rounds)
    return dict(delta=float(floor_delta), frac=float(floor_frac), flags=FLOOR, rounds=rounds)


def choose_delta(logw, loglik, remaining, rho):
    """the search on the longdouble conditional ESS (rounded to float64 as the library's finish returns it)"""
    return search(lambda d: cess_finish([cess_partial(logw, loglik, d)])["frac"].astype(np.float64), remaining, rho)


# ---- 3. reweighting ---------------------------------------------------------------------------------------------------------------------------
def reweight(logw, loglik, delta):
    lw = np.asarray(logw, dtype=np.float64)
    ll = np.asarray(loglik, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(lw), lw, np.where(np.isfinite(ll), lw + np.float64(delta) * ll, -np.inf))


# ---- 4. resampling on integers -----------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    m = 2 ** 64 - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def resample_u(seed, k):
    return splitmix64((seed + 0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)) >> 32


def quantise(logw, a):
    """q as a list of Python integers, from longdouble arithmetic"""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    out = []
    for x in lw:
        if np.isnan(x) or x == -np.inf:
            out.append(0)
        else:
            with np.errstate(under="ignore", invalid="ignore"):
                out.append(int(np.floor(LD(2) ** QBITS * np.exp(min(LD(x) - LD(a), LD(0))))))
    return out


def ancestors_direct(q, U):
    """the definition, one comparison of Python integers after another"""
    n = len(q)
    C, s = [], 0
    for v in q:
        s += int(v)
        C.append(s)
    Q = s
    assert Q > 0
    anc, i = [], 0
    for j in range(n):
        while not C[i] * (n << 32) > ((j << 32) + U) * Q:       # (the right side grows with j: the search resumes where it stood)
            i += 1
        anc.append(i)
    return anc


def ancestors(q, U):
    """the same for long arrays: C_i (n 2^32) > P  <=>  C_i > P // (n 2^32) for integers, the quotient in Python integers (below 2^60), the
    search in exact uint64"""
    n = len(q)
    C = np.cumsum(np.asarray(q, dtype=np.uint64), dtype=np.uint64)
    Q = int(C[-1])
    assert 0 < Q <= 2 ** 60 and n <= MAX_N
    thr = (((np.arange(n, dtype=object) << 32) + int(U)) * Q // (n << 32)).astype(np.uint64)      # (object arrays: Python integers)
    return np.searchsorted(C, thr, side="right").astype(np.int32)


def scan_plan(n):
    return max(1, -(-n // 1024)), 1024


def scan_range(n, block, thread):
    b = block * 1024 + thread * 4
    return min(b, n), min(b + 4, n)


# ---- 5. the run: its refusals, and a statistical restatement --------------------------------------------------------------------------------
def check_run(have_theta0, beta0, rho, tau, T_max, stage_len, mass_every, have_H, L):
    """True where rmhmc_smc_run accepts its arguments"""
    return bool(T_max >= 1 and stage_len >= 1 and L >= 1 and 0.0 < rho < 1.0 and 0.0 <= tau <= 1.0 and math.isfinite(beta0)
                and 0.0 <= beta0 < 1.0 and (have_theta0 or beta0 == 0.0) and mass_every >= 0 and (mass_every == 0 or have_H))


def stage_mass(k, mass_every, flags):
    return mass_every > 0 and (k % mass_every == 0 or bool(flags & LAST))


def _log_mean_and_ess(logw):
    f = A.finish([A.partial(logw)])
    return float(f["log_mean_w"]), float(f["weight_ess"])


def run(X, t, n, rho, tau, stage_len, H_lik, L=6, eps=0.5, alpha=100.0, seed=0, T_max=10000):
    """rmhmc_smc_run from the prior with a mass update in every stage, NumPy's random numbers (the offset of a resampling among them).
    Returns dict(log_z, T, beta, cess, ess, flags, accept_trace, logw, theta)."""
    rs = np.random.RandomState(seed)
    t = np.ravel(t).astype(np.float64)
    D = X.shape[1]
    W = math.sqrt(alpha) * rs.randn(n, D)
    logw = np.zeros(n)
    ll = A._eval(X, t, W, 0.0, alpha)[2]
    beta, logz, k = 0.0, 0.0, 0
    tr = dict(beta=[], cess=[], ess=[], flags=[], accept_trace=[])
    while beta < 1.0 and k < T_max:
        c = choose_delta(logw, ll, 1.0 - beta, rho)
        flags = c["flags"]
        b = 1.0 if flags & LAST else beta + c["delta"]
        logw = reweight(logw, ll, c["delta"])
        lm, ess = _log_mean_and_ess(logw)
        if ess < tau * n:
            logz += lm
            anc = ancestors(quantise(logw, np.nanmax(logw)), int(rs.randint(0, 2 ** 32, dtype=np.uint64)))
            W = W[anc]
            logw = np.zeros(n)
            flags |= RESAMPLED
        Mass = A.stage_mass_matrix(b, H_lik, alpha) if H_lik is not None else np.eye(D)
        Lm = np.linalg.cholesky(Mass)
        Minv = np.linalg.inv(Mass)
        ljl, grad, ll = A._eval(X, t, W, b, alpha)
        acc_total = 0
        for _ in range(int(stage_len)):                 # (the transition of ais_ref.run)
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
                lj, g, l_ = A._eval(X, t, Wa, b, alpha)
                Pm[act] = Pa + eps / 2.0 * g
                Wn[act], gn[act], ljn[act], lln[act] = Wa, g, lj, l_
            with np.errstate(invalid="ignore", over="ignore"):
                H_prop = -ljn + 0.5 * ((Pm @ Minv) * Pm).sum(axis=1)
                ratio = H_cur - H_prop
                ok = np.isfinite(H_cur) & np.isfinite(H_prop) & ~np.isnan(Pm).any(axis=1)
                accept = ok & ((ratio > 0) | (ratio > np.log(u_acc)))
            W[accept], grad[accept], ljl[accept], ll[accept] = Wn[accept], gn[accept], ljn[accept], lln[accept]
            acc_total += int(accept.sum())
        for key, v in zip(("beta", "cess", "ess", "flags", "accept_trace"), (b, c["frac"], ess, flags, acc_total / (n * float(stage_len)))):
            tr[key].append(v)
        beta = b
        k += 1
    lm, _ = _log_mean_and_ess(logw)
    out = {key: np.array(v) for key, v in tr.items()}
    out.update(log_z=logz + lm if beta >= 1.0 else math.nan, T=k, logw=logw, theta=W)
    return out


def combine(log_z):
    """(log of the mean of exp(log_z), its delta-method standard error) over repeats"""
    lz = np.asarray(log_z, dtype=np.float64)
    a = lz.max()
    z = np.exp(lz - a)
    return float(a + math.log(z.mean())), float(z.std(ddof=1) / math.sqrt(len(z)) / z.mean())
