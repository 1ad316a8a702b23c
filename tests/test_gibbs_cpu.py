"""Auxiliary-variable Gibbs sampler (code/gibbs_sampler.py, include/rmhmc_gibbs.h) without a GPU: the C-ABI header, the ctypes binding
and the library exports agree; a NumPy restatement of the reference (gibbs_numpy: Phi and Phi^-1 from torch.special in float64, the
bounds of the device) reproduces every golden Gibbs tape; its truncated normal matches SciPy's recorded values, |m/s| up to 40
included; the tapes cover what they are for; the shim checks its arguments and is wired into experiment.SAMPLERS and dropin/."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, rel_err
from riemannhamiltonianmontecarlo_amd import _capi, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_amh_cpu import M32, _u53, philox4x32_10

GIBBS_TAPES = ["ripley", "heart", "pima", "australian", "syn_m400_d64", "syn_m300_d33", "syn_m150_d5_x30"]
MAX_ATTEMPTS, MAX_TERMS, TAIL = 64, 64, 25.0        # the bounds of gibbs.hip.h
TINY = 2.2250738585072014e-308


def flip_labels(t, frac, seed):
    """the label noise of the outlier tape (tests/golden/make_golden_gibbs.py)"""
    t = np.array(t, dtype=np.float64)
    idx = np.random.RandomState(seed).choice(t.size, int(frac * t.size), replace=False)
    t.reshape(-1)[idx] = 1.0 - t.reshape(-1)[idx]
    return t


def load_gibbs_tape(name):
    g = dict(np.load(os.path.join(GOLDEN, "gibbs_%s.npz" % name)))
    if "data_seed" in g:
        XX, t = synthetic_logreg(int(g["M"]), int(g["D"]), int(g["data_seed"]))
        if float(g["flip"]):
            t = flip_labels(t, float(g["flip"]), int(g["data_seed"]))
        XX = XX * float(g["x_scale"])
    else:
        d = np.load(os.path.join(GOLDEN, "data_%s.npz" % name))
        XX, t = d["XX"], d["t"]
    return XX, t, g


# ---- NumPy restatement of gibbs_sampler.py:14-139 for n chains at once ---------------------------------------------------------------
def _Phi(x):
    return 0.5 * torch.special.erfc(torch.as_tensor(-np.asarray(x, dtype=np.float64) / np.sqrt(2.0))).numpy()


def _ndtri(p):
    return torch.special.ndtri(torch.as_tensor(np.asarray(p, dtype=np.float64))).numpy()


def _mills(y):
    q = 1.0 / (y * y)
    r = np.ones_like(q)
    for k in range(8, 0, -1):
        r = 1.0 - (2 * k - 1) * q * r
    return r


def truncnorm_neg(U, Uc, m, s):
    """N(m, s^2) truncated to (-inf, 0) at the uniform U (Uc = 1 - U, given apart so that a mirrored call keeps the digits of a tiny
    uniform): m + s Phi^-1(p), p = U Phi(-m/s); beyond m/s = 25 the same quantile from the asymptotic series of log Phi (as gibbs.hip.h)"""
    U, Uc, m, s = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (U, Uc, m, s)])
    with np.errstate(all="ignore"):
        a = m / s
        p = U * _Phi(-a)
        # (upper half: the quantile of the complement 1 - p = (1 - U) + U Phi(a), a sum of positive terms, keeps the digits p loses near 1)
        y = np.where(p > 0.5, -_ndtri(Uc + U * _Phi(a)), _ndtri(np.maximum(p, TINY)))
        x = m + s * y
        tail = a > TAIL
        if np.any(tail):
            at = a[tail]
            lu = np.where(U[tail] > 0.5, np.log1p(-Uc[tail]), np.log(U[tail]))
            lr0 = np.log(_mills(at))
            dl = -lu / at
            for _ in range(6):
                y = at + dl
                r = _mills(y)
                g = -(at + 0.5 * dl) * dl - np.log1p(dl / at) + (np.log(r) - lr0) - lu
                dl = dl + g * r / y
            x = x.copy()
            x[tail] = -s[tail] * dl
        return np.fmin(x, -TINY)


def truncnorm(U, m, s, pos):
    """label 1 (pos): (0, inf), label 0: (-inf, 0)"""
    pos = np.asarray(pos, dtype=bool)
    U = np.asarray(U, dtype=np.float64)
    x = truncnorm_neg(np.where(pos, 1.0 - U, U), np.where(pos, U, 1.0 - U), np.where(pos, -np.asarray(m), m), s)
    return np.where(pos, -x, x)


def series_tests(U, Lam):
    """gibbs_sampler.py:14-47 element-wise: (ok bool, depth of the series, bound reached)"""
    U = np.asarray(U, dtype=np.float64); Lam = np.asarray(Lam, dtype=np.float64)
    right = Lam > 4.0 / 3.0
    ok = np.zeros(U.shape, bool); bound = np.zeros(U.shape, bool); depth = np.zeros(U.shape, np.int64)
    with np.errstate(all="ignore"):
        H = 0.5 * np.log(2) + 2.5 * np.log(np.pi) - 2.5 * np.log(Lam) - np.pi ** 2 / (2 * Lam) + 0.5 * Lam
        logU = np.log(U)
        X = np.where(right, np.exp(-0.5 * Lam), np.exp((-np.pi ** 2) / (2 * Lam)))
        K = Lam / (np.pi ** 2)
        Z = np.ones(U.shape)
        pend = np.ones(U.shape, bool)
        j = 0
        for _ in range(MAX_TERMS):
            if not pend.any():
                break
            j += 1
            Z = np.where(pend, Z - np.where(right, (j + 1) ** 2 * X ** float((j + 1) ** 2 - 1), K * X ** float(j ** 2 - 1)), Z)
            acc = pend & np.where(right, Z > U, H + np.log(Z) > logU)
            ok |= acc; depth[acc] = j; pend &= ~acc
            j += 1
            Z = np.where(pend, Z + (j + 1) ** 2 * X ** float((j + 1) ** 2 - 1), Z)
            rej = pend & np.where(right, Z < U, H + np.log(Z) < logU)
            depth[rej] = j; pend &= ~rej
        bound |= pend
    return ok, depth, bound, right


def gibbs_numpy(XX, t, n_iter, draws, n=1, v=100.0, stats=None):
    """draws: u_init() -> (n, N); u_sweep(it) -> (n, N); T(it) -> (n, D); ks(it, attempt, active (n, N) bool) -> normal, u, u (n, N).
    Returns dict(beta, B (n, T, D) after every iteration (B before the T term), attempts (n, T, N), Z, lam (n, N) after the last one,
    capped (n,)).  stats (a dict) collects which series branch was taken and the deepest series."""
    XX = np.asarray(XX, dtype=np.float64); tt = np.asarray(t, dtype=np.float64).reshape(-1)
    N, D = XX.shape
    pos = tt > 0.5
    Z = truncnorm(draws.u_init(), 0.0, 1.0, pos[None, :]) * np.ones((n, 1))
    lam = np.ones((n, N))
    beta_o = np.zeros((n, n_iter, D)); B_o = np.zeros((n, n_iter, D)); att_o = np.zeros((n, n_iter, N), np.int64)
    capped = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for it in range(n_iter):
            G = np.einsum("jd,cj,je->cde", XX, 1.0 / lam, XX) + np.eye(D) / v
            V = np.linalg.inv(G)
            V = 0.5 * (V + np.transpose(V, (0, 2, 1)))
            L = np.linalg.cholesky(V)
            S = np.einsum("cde,je->cdj", V, XX)                    # (n, D, N)
            B = np.einsum("cdj,cj->cd", S, Z / lam)
            U = draws.u_sweep(it)
            for j in range(N):
                z_old = Z[:, j].copy()
                h = S[:, :, j] @ XX[j]
                w = h / (lam[:, j] - h)
                m = B @ XX[j]
                m = m - w * (z_old - m)
                q = lam[:, j] * (w + 1)
                Z[:, j] = truncnorm(U[:, j], m, np.sqrt(q), pos[j])
                B = B + ((Z[:, j] - z_old) / lam[:, j])[:, None] * S[:, :, j]
            T = draws.T(it)
            beta = B + np.einsum("cde,ce->cd", L, T)
            B_o[:, it] = B; beta_o[:, it] = beta
            res = Z - beta @ XX.T
            r = np.sqrt(res * res)
            active = np.ones((n, N), bool)
            bound = np.zeros((n, N), bool)
            for a in range(MAX_ATTEMPTS):
                if not active.any():
                    break
                Y, Ua, Ub = draws.ks(it, a, active)
                Y = Y * Y
                Y = 1 + (Y - np.sqrt(Y * (4 * r + Y))) / (2 * r)
                Lam = np.where(Ua <= 1 / (1 + Y), r / Y, r * Y)
                ok, depth, bnd, right = series_tests(np.where(active, Ub, 0.5), np.where(active, Lam, 1.0))
                lam = np.where(active, Lam, lam)
                att_o[:, it][active] += 1
                bound |= active & bnd
                if stats is not None:
                    stats["right"] = stats.get("right", 0) + int((active & right).sum())
                    stats["left"] = stats.get("left", 0) + int((active & ~right).sum())
                    stats["depth"] = max(stats.get("depth", 0), int(depth[active].max()))
                active = active & ~ok
            bound |= active
            capped += bound.sum(axis=1)
    return dict(beta=beta_o, B=B_o, attempts=att_o, Z=Z, lam=lam, capped=capped)


class TapeDraws:
    """the draws of one tape, for one chain"""
    def __init__(self, g):
        self.g = g

    def u_init(self):
        return self.g["u_init"][None]

    def u_sweep(self, it):
        return self.g["u_sweep"][it][None]

    def T(self, it):
        return self.g["T"][it][None]

    def ks(self, it, a, active):
        off = self.g["ks_offset"][it]
        idx = off[:-1] + a
        have = idx < off[1:]
        assert not np.any(active[0] & ~have), "the restatement wants more attempts than the reference made"
        k = self.g["ks_draws"][np.where(have, idx, 0)]
        return tuple(np.where(have, k[:, q], np.nan)[None] for q in range(3))


class PhiloxDraws:
    """the Philox4x32-10 streams of gibbs.hip.h for the global chain ids `chains`: key = seed, counter = (chain, row, iteration, block)"""
    def __init__(self, seed, chains, N, D):
        self.g = np.asarray(chains, dtype=np.uint64)[:, None]
        self.key = (np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))
        self.N, self.D = N, D

    def _block(self, rows, it, block):
        rows = np.asarray(rows, dtype=np.uint64)[None, :]
        shape = np.broadcast(self.g, rows).shape
        full = lambda x: np.broadcast_to(np.asarray(x, dtype=np.uint64), shape)
        c = philox4x32_10((full(self.g), full(rows), full(it), full(block)), self.key)
        return _u53(c[0], c[1]), _u53(c[2], c[3])

    def u_init(self):
        return self._block(np.arange(self.N), 0, 0x60000000)[0]

    def u_sweep(self, it):
        return self._block(np.arange(self.N), it, 0x61000000)[0]

    def T(self, it):
        d = np.arange(self.D, dtype=np.uint64)
        shape = (self.g.shape[0], self.D)
        full = lambda x: np.broadcast_to(np.asarray(x, dtype=np.uint64), shape)
        c = philox4x32_10((full(self.g), full(0), full(it), full((np.uint64(0x62000000) + (d >> np.uint64(1)))[None, :])), self.key)
        U0, U1 = _u53(c[0], c[1]), _u53(c[2], c[3])
        R = np.sqrt(-2.0 * np.log(U0))
        return np.where((d & np.uint64(1)) == 1, R * np.sin(2 * np.pi * U1), R * np.cos(2 * np.pi * U1))

    def ks(self, it, a, active):
        U0, U1 = self._block(np.arange(self.N), it, 0x63000000 + 2 * a)
        Ua, Ub = self._block(np.arange(self.N), it, 0x63000001 + 2 * a)
        return np.sqrt(-2.0 * np.log(U0)) * np.cos(2 * np.pi * U1), Ua, Ub


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def _header():
    hdr = open(os.path.join(ROOT, "include", "rmhmc_gibbs.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_gibbs_header_binding_and_exports_agree(hip, oracle):
    import ctypes
    hdr = _header()
    syms = sorted(set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == ["rmhmc_gibbs_replay", "rmhmc_gibbs_sample"]
    assert set(syms) == set(_capi.GIBBS_SIGNATURES)
    assert not set(syms) & (set(_capi.SIGNATURES) | set(_capi.AMH_SIGNATURES) | set(_capi.IWLS_SIGNATURES))
    lib = ctypes.CDLL(hip.path)
    for s in syms:
        assert hasattr(lib, s), s
        args = re.search(s + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(args.split(",")) == len(_capi.GIBBS_SIGNATURES[s][1]), s
    assert hip.has_gibbs and not oracle.has_gibbs


def test_oracle_context_has_no_gibbs(oracle):
    with oracle.context(5, 2, 1) as ctx:
        ctx.set_data(np.eye(5, 2), np.zeros(5))
        with pytest.raises(_capi.RmhmcError):
            ctx.gibbs_sample(4, 1)


@pytest.mark.parametrize("name", GIBBS_TAPES)
def test_numpy_restatement_reproduces_tape(name):
    """attempts per row array-equal; beta, B <= 1e-9; Z, lam <= 1e-8 (lam inherits the cancellation in Z_j - x_j.beta)"""
    XX, t, g = load_gibbs_tape(name)
    r = gibbs_numpy(XX, t, int(g["n_iter"]), TapeDraws(g), v=float(g["v"]))
    np.testing.assert_array_equal(r["attempts"][0], g["attempts"])
    errs = {k: rel_err(r[k][0], g[k]) for k in ("beta", "B", "Z", "lam")}
    print(name, errs)
    assert r["capped"][0] == 0
    assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9, errs
    assert errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs
    assert os.path.getsize(os.path.join(GOLDEN, "gibbs_%s.npz" % name)) <= 128 * 1024


def test_tapes_cover_both_series_deep_attempts_and_both_labels():
    right = left = depth = attempts = 0
    for name in GIBBS_TAPES:
        XX, t, g = load_gibbs_tape(name)
        tt = np.asarray(t).reshape(-1)
        assert (tt == 1).any() and (tt == 0).any()
        assert np.all(np.sign(g["Z"]) == np.where(tt == 1, 1.0, -1.0)) and np.all(g["lam"] > 0)
        attempts = max(attempts, int(g["attempts"].max()))
        if name in ("ripley", "syn_m150_d5_x30"):
            st = {}
            gibbs_numpy(XX, t, int(g["n_iter"]), TapeDraws(g), v=float(g["v"]), stats=st)
            right += st["right"]; left += st["left"]; depth = max(depth, st["depth"])
    assert right > 100 and left > 100 and depth >= 3 and attempts >= 5, (right, left, depth, attempts)


def test_truncated_normal_against_scipy_values():
    """SciPy's values (tests/golden/make_golden_gibbs.py): a grid of U and m/s in [-40, 40], both labels, and the 250 calls of a sweep
    of the ripley tape.  Finite, on the label's side of 0, relative error against SciPy's value <= 1e-9 - wherever SciPy's value is one:
    the fixture also holds the exact quantile (multiprecision), and where U is within 1e-12 of the truncated end SciPy's own m + s y is
    rounding noise (off by up to 37 % on 142 of the 1296 grid points).  Those points (SciPy itself further than 1e-10 from the exact
    value) are held against the exact value instead, to 1e-9 relative plus the rounding of the sum m + s y, 16 eps (|m| + s + |x|): p carries
    an absolute rounding of eps / 2, which moves y = Phi^-1(p) by at least 1.25 eps."""
    f = np.load(os.path.join(GOLDEN, "gibbs_truncnorm.npz"))
    g = np.load(os.path.join(GOLDEN, "gibbs_ripley.npz"))
    U, m, s, lab, want, exact = f["u"], f["m"], f["s"], f["t"], f["x"], f["x_exact"]
    x = truncnorm(U, m, s, lab == 1)
    assert np.all(np.isfinite(x)) and np.all(np.where(lab == 1, x > 0, x < 0)) and np.all(np.isfinite(want))
    a = m / s
    usable = np.abs(want - exact) <= 1e-10 * np.abs(exact)
    for sign in (-1, 1):
        for l in (0, 1):
            assert np.any(usable & (sign * a >= 40 - 1e-9) & (lab == l)), (sign, l)      # |m/s| = 40 on both sides, both labels
    err = np.abs(x - want)[usable] / np.abs(want)[usable]
    rest = np.abs(x - exact)[~usable]
    tol = (1e-9 * np.abs(exact) + 16 * np.finfo(float).eps * (np.abs(m) + s + np.abs(exact)))[~usable]
    print("truncated normal, grid to |m/s| = %.0f: max relative error against SciPy %.3e on %d points; against the exact value %.3e on all; "
          "%d points where SciPy's value is noise: max error / tolerance %.3f"
          % (np.abs(a).max(), err.max(), usable.sum(), (np.abs(x - exact) / np.abs(exact))[usable].max(), (~usable).sum(),
             (rest / tol).max()))
    assert err.max() <= 1e-9, err.max()
    assert np.all(rest <= tol)
    x = truncnorm(g["tn_u"], g["tn_m"], g["tn_s"], g["tn_t"] == 1)
    err = np.abs(x - g["tn_x"]) / np.abs(g["tn_x"])
    print("truncated normal, a sweep of the ripley tape: max relative error against SciPy %.3e (|m/s| up to %.1f)"
          % (err.max(), np.abs(g["tn_m"] / g["tn_s"]).max()))
    assert err.max() <= 1e-9, err.max()


def test_truncated_normal_tail_form_agrees_with_two_tail_form():
    """where both forms are valid (25 < m/s < 36) they agree; beyond underflow the tail form stays finite and on the right side"""
    rs = np.random.RandomState(3)
    a = rs.uniform(25.0001, 36, 4000); U = rs.uniform(1e-9, 1 - 1e-9, 4000); s = np.exp(rs.uniform(-2, 2, 4000))
    two_tail = a * s + s * _ndtri(U * _Phi(-a))
    assert rel_err(truncnorm_neg(U, 1.0 - U, a * s, s), two_tail) <= 1e-10
    for a in (38.0, 60.0, 1e3, 1e6):
        x = truncnorm(np.array([1e-16, 0.5, 1 - 1e-16]), np.full(3, -a * 2.0), 2.0, True)
        assert np.all(np.isfinite(x)) and np.all(x > 0)
        x = truncnorm(np.array([1e-16, 0.5, 1 - 1e-16]), np.full(3, a * 2.0), 2.0, False)
        assert np.all(np.isfinite(x)) and np.all(x < 0)


def test_bounds_catch_a_nan_residual():
    ok, depth, bound, right = series_tests(np.array([0.3, 0.3]), np.array([np.nan, 0.7]))
    assert bound[0] and not ok[0] and not bound[1]


def test_numpy_philox_streams_are_valid():
    d = PhiloxDraws(7, [0, 5, 2 ** 32 - 1], 11, 5)
    for a in (d.u_init(), d.u_sweep(3), d.ks(2, 1, None)[1], d.ks(2, 1, None)[2]):
        assert a.shape == (3, 11) and np.all((a > 0) & (a < 1))
    assert d.T(4).shape == (3, 5) and np.all(np.isfinite(d.T(4))) and np.all(np.isfinite(d.ks(0, 0, None)[0]))
    assert not np.array_equal(d.u_sweep(3), d.u_sweep(4)) and not np.array_equal(d.u_init()[0], d.u_init()[1])
    # a chain's stream does not depend on the batch it is drawn in
    np.testing.assert_array_equal(PhiloxDraws(7, [5], 11, 5).T(4)[0], d.T(4)[1])


def test_gibbs_shim_argument_checks():
    from riemannhamiltonianmontecarlo_amd import auxiliary_gibbs
    X = np.zeros((5, 2)); t = np.zeros(5)
    for bad in (dict(max_iter=10, burn_in=10), dict(max_iter=10, burn_in=12), dict(max_iter=10, burn_in=-1)):
        with pytest.raises(ValueError):
            auxiliary_gibbs(X, t, verbose=False, **bad)
    with pytest.raises(ValueError):
        auxiliary_gibbs(X, np.zeros(4))
    assert experiment.SAMPLERS["Gibbs"] is auxiliary_gibbs


def test_dropin_modules_cover_the_reference_drivers_imports():
    """main.py:10-15 imports hmc, metropolis, rmhmc, gibbs_sampler and iwls: all five load from dropin/, gibbs_sampler re-exports the shim"""
    import importlib.util
    mods = {}
    for name in ("hmc", "metropolis", "rmhmc", "gibbs_sampler", "iwls"):
        spec = importlib.util.spec_from_file_location("dropin_" + name, os.path.join(ROOT, "dropin", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    from riemannhamiltonianmontecarlo_amd.gibbs_sampler import auxiliary_gibbs
    assert mods["gibbs_sampler"].auxiliary_gibbs is auxiliary_gibbs
    for name, attr in (("hmc", "HMC"), ("metropolis", "AMH"), ("rmhmc", "RMHMC"), ("iwls", "iwls")):
        assert callable(getattr(mods[name], attr))
