"""IWLS Metropolis-Hastings (code/iwls.py, include/rmhmc_iwls.h) without a GPU: the C-ABI header, the ctypes binding and the library
exports agree; a NumPy restatement of the sampler reproduces every golden IWLS tape; the Philox draws that feed it in the GPU tests;
the shim checks its arguments and is wired into experiment.SAMPLERS and dropin/."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_amh_cpu import M32, _u53, philox4x32_10

IWLS_TAPES = ["australian", "german", "heart", "pima", "ripley", "syn_m3000_d64", "syn_m100_d5_outlier"]


def load_iwls_tape(name):
    g = dict(np.load(os.path.join(GOLDEN, "iwls_%s.npz" % name)))
    if "XX" in g:
        XX, t = g["XX"], g["t"]
    elif "data_seed" in g:
        XX, t = synthetic_logreg(int(g["M"]), int(g["D"]), int(g["data_seed"]))
    else:
        d = np.load(os.path.join(GOLDEN, "data_%s.npz" % name))
        XX, t = d["XX"], d["t"]
    return XX, t, g


# ---- NumPy restatement of iwls.py:13-89 for n chains at once ----------------------------------------------------------------------
def iwls_numpy(XX, t, n_iter, draws, n=1, alpha=100.0, theta0=None, compat=True):
    """draws(it, chol, mean) -> (w_prop (n, D), u (n,)): the proposal given the current factor L (G = L L') and mean.  Returns dict(w,
    mean (n,T,D) and ljl, ratio (n,T) after every iteration, accepted / u_read / saturated (n,T))."""
    XX = np.asarray(XX, dtype=np.float64); t = np.asarray(t, dtype=np.float64).reshape(-1)
    D = XX.shape[1]

    def point(w):  # LJL, G, L, mean, l(w) and the saturation flag at w (n, D)
        f = w @ XX.T
        prior = np.sum(-0.5 * np.log(2 * np.pi * alpha) - w ** 2 / (2 * alpha), axis=1)  # tools.LogNormPDF(0, w, alpha)
        ljl = f @ t - np.sum(np.log(1 + np.exp(f)), axis=1) + prior
        p = 1 / (1 + np.exp(-f))
        W = p * (1 - p)
        sat = np.any((W == 0) | ~np.isfinite(1 / W), axis=1)
        G = np.matmul(XX.T[None] * W[:, None, :], XX) + np.eye(D) / alpha
        grad = (t - p) @ XX - w / alpha
        L = np.linalg.cholesky(G)
        mean = w + np.linalg.solve(G, grad[..., None])[..., 0]
        if compat:
            lq = -np.sum(np.log(np.diagonal(np.linalg.cholesky(np.linalg.inv(G) + 1e-6 * np.eye(D)), axis1=1, axis2=2)), axis=1)
        else:
            lq = np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), axis=1)
        return dict(ljl=ljl, L=L, mean=mean, lq=lq, sat=sat)

    def logq(x, P):  # l(w) - |L'(x - m)|^2 / 2
        y = np.einsum("cij,ci->cj", P["L"], x - P["mean"])
        return P["lq"] - 0.5 * np.sum(y * y, axis=1)

    w = np.zeros((n, D)) if theta0 is None else np.array(np.broadcast_to(theta0, (n, D)), dtype=np.float64)
    out = dict(w=np.zeros((n, n_iter, D)), mean=np.zeros((n, n_iter, D)), ljl=np.zeros((n, n_iter)), ratio=np.zeros((n, n_iter)),
               accepted=np.zeros((n, n_iter), bool), u_read=np.zeros((n, n_iter), bool), saturated=np.zeros((n, n_iter), bool))
    with np.errstate(all="ignore"):
        cur = point(w)
        for it in range(n_iter):
            wp, u = draws(it, cur["L"], cur["mean"])
            prop = point(wp)
            ratio = prop["ljl"] + logq(w, prop) - cur["ljl"] - logq(wp, cur)
            sat = prop["sat"] if compat else np.zeros(n, bool)
            ratio = np.where(sat, np.nan, ratio)
            ur = ~(ratio > 0)
            acc = ~ur | (ratio > np.log(np.where(ur, u, 0.5)))
            w = np.where(acc[:, None], wp, w)
            for k in cur:
                cur[k] = np.where(acc.reshape((n,) + (1,) * (cur[k].ndim - 1)), prop[k], cur[k])
            out["w"][:, it] = w; out["mean"][:, it] = cur["mean"]; out["ljl"][:, it] = cur["ljl"]; out["ratio"][:, it] = ratio
            out["accepted"][:, it] = acc; out["u_read"][:, it] = ur; out["saturated"][:, it] = sat
    return out


# ---- Philox streams of iwls.hip.h -----------------------------------------------------------------------------------------------------
def philox_iwls_draws(seed, chains, D):
    """draws(it, L, mean) for iwls_numpy: z from the momentum-normal blocks d/2 (Box-Muller, cos for even d, sin for odd), w' = mean +
    L^-T z; u = U1 of block 0x40000000; counter (chain lo, chain hi, it, block), key seed"""
    g = np.asarray(chains, dtype=np.uint64)[:, None]
    j = np.arange(D, dtype=np.uint64)[None, :]
    odd = (j & np.uint64(1)) == 1
    key = (np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))

    def block(it, b):
        c = philox4x32_10((g & M32, g >> np.uint64(32), np.full_like(g, it), np.uint64(0) * g + b), key)
        return _u53(c[0], c[1]), _u53(c[2], c[3])

    def draws(it, L, mean):
        U0, U1 = block(it, j >> np.uint64(1))
        z = np.sqrt(-2.0 * np.log(U0)) * np.where(odd, np.sin(2 * np.pi * U1), np.cos(2 * np.pi * U1))
        x = np.linalg.solve(np.swapaxes(L, 1, 2), z[..., None])[..., 0]
        _, u = block(it, np.uint64(0x40000000))
        return mean + x, u[:, 0]
    return draws


def tape_draws(g):
    return lambda it, L, mean: (g["w_prop"][it][None], g["u"][it:it + 1])


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def _iwls_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmhmc_iwls.h")).read(), flags=re.S)


def test_iwls_header_binding_and_exports_agree(hip, oracle):
    import ctypes
    hdr = _iwls_header()
    syms = sorted(set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == ["rmhmc_iwls_replay", "rmhmc_iwls_sample"]
    assert set(syms) == set(_capi.IWLS_SIGNATURES)
    assert not set(syms) & set(_capi.SIGNATURES)      # rmhmc.h stays the oracle's ABI
    lib = ctypes.CDLL(hip.path)
    for s in syms:
        assert hasattr(lib, s), s
    assert hip.has_iwls and not oracle.has_iwls
    for s in syms:
        args = re.search(s + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(args.split(",")) == len(_capi.IWLS_SIGNATURES[s][1]), s


def test_oracle_context_has_no_iwls(oracle):
    with oracle.context(5, 2, 1) as ctx:
        ctx.set_data(np.eye(5, 2), np.zeros(5))
        with pytest.raises(_capi.RmhmcError):
            ctx.iwls_sample(4, 1)


@pytest.mark.parametrize("name", IWLS_TAPES)
def test_numpy_restatement_reproduces_tape(name):
    XX, t, g = load_iwls_tape(name)
    T = int(g["n_iter"])
    r = iwls_numpy(XX, t, T, tape_draws(g))
    np.testing.assert_array_equal(r["accepted"][0], g["accepted"] != 0)
    np.testing.assert_array_equal(r["u_read"][0], ~np.isnan(g["u"]))
    np.testing.assert_array_equal(r["w"][0], g["w"])
    np.testing.assert_array_equal(np.isnan(r["ratio"][0]), np.isnan(g["ratio"]))
    assert _rel(r["ljl"][0], g["ljl"]) <= 1e-12
    assert _rel(r["mean"][0], g["mean"]) <= 1e-12
    fin = np.isfinite(g["ratio"])
    np.testing.assert_array_equal(np.isfinite(r["ratio"][0]), fin)
    # (relative to the larger of |ratio| and max |LJL|: far-out proposals have quadratic terms of 1e7 and more)
    scale = np.maximum(np.abs(g["ratio"][fin]), np.max(np.abs(g["ljl"])))
    assert np.all(np.abs(r["ratio"][0][fin] - g["ratio"][fin]) <= 1e-12 * scale)
    B = int(g["burn_in"])
    np.testing.assert_array_equal(g["beta_saved"], g["w"][B:])     # every row written: row k = beta after iteration burn_in + k


def test_tapes_cover_saturation_overflow_and_both_u_branches():
    saturated = 0
    for name in IWLS_TAPES:
        _, _, g = load_iwls_tape(name)
        saturated += int(np.isnan(g["ratio"]).sum())
        assert (~np.isnan(g["u"])).any() and np.isnan(g["u"]).any(), name    # u read and not read
    assert saturated > 100
    _, _, g = load_iwls_tape("australian")
    assert np.isnan(g["ratio"]).sum() > 50                                   # the reference's 0/0 on australian
    XX, t, g = load_iwls_tape("syn_m100_d5_outlier")
    over = np.isneginf(g["ljl_prop"])
    assert over.sum() > 5 and not g["accepted"][over].any() and not np.isnan(g["u"][over]).any()
    assert (np.max(g["w_prop"][over] @ XX.T, axis=1) > 709.78).all()


def test_numpy_philox_draws():
    from test_amh_cpu import philox_draws
    d = philox_iwls_draws(7, [0, 1, 2 ** 33], 5)
    L = np.broadcast_to(np.eye(5), (3, 5, 5))
    wp, u = d(3, L, np.zeros((3, 5)))
    assert wp.shape == (3, 5) and u.shape == (3,) and np.all((u > 0) & (u < 1)) and np.all(np.isfinite(wp))
    # (the normals are the RMHMC momentum stream: blocks d/2 of the same counter, independent of the AMH blocks)
    z2, _ = philox_draws(7, [0], 5)(3)
    assert not np.allclose(z2[0], wp[0])


def test_iwls_shim_argument_checks():
    from riemannhamiltonianmontecarlo_amd import iwls
    X = np.zeros((5, 2)); t = np.zeros(5)
    for bad in (dict(max_iter=10, burn_in=10), dict(max_iter=10, burn_in=12), dict(max_iter=10, burn_in=-1)):
        with pytest.raises(ValueError):
            iwls(X, t, verbose=False, **bad)
    with pytest.raises(ValueError):
        iwls(X, np.zeros(4))
    assert experiment.SAMPLERS["IWLS"] is iwls


def test_dropin_module_reaches_the_gpu_shim():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_iwls", os.path.join(ROOT, "dropin", "iwls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from riemannhamiltonianmontecarlo_amd.iwls import iwls
    assert mod.iwls is iwls
