"""Adaptive Metropolis (code/metropolis.py, include/rmhmc_amh.h) without a GPU: the C-ABI header, the ctypes binding and the library
exports agree; a NumPy restatement of the reference reproduces every golden AMH tape exactly; the NumPy Philox4x32-10 that feeds it in
the GPU tests is the library's stream; the shim checks its arguments."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

AMH_TAPES = ["australian", "heart", "pima", "ripley", "syn_m3000_d64", "syn_m200_d6_x300"]


def load_amh_tape(name):
    g = dict(np.load(os.path.join(GOLDEN, "amh_%s.npz" % name)))
    if "data_seed" in g:
        XX, t = synthetic_logreg(int(g["M"]), int(g["D"]), int(g["data_seed"]))
        XX = XX * float(g["x_scale"])
    else:
        d = np.load(os.path.join(GOLDEN, "data_%s.npz" % name))
        XX, t = d["XX"], d["t"]
    return XX, t, g


# ---- NumPy restatement of metropolis.py:14-94 for n chains at once -----------------------------------------------------------------
def amh_numpy(XX, t, n_iter, burn_in, draws, n=1, alpha=100.0, theta0=None):
    """draws(it) -> (z, u), each (n, D).  Returns dict(w (n,T,D) and ljl (n,T) after every iteration, sd (n,D) final, accepted /
    u_read (n,T,D))."""
    XX = np.asarray(XX, dtype=np.float64); t = np.asarray(t, dtype=np.float64).reshape(-1)
    D = XX.shape[1]

    def ljl(W):
        f = W @ XX.T
        prior = np.sum(-0.5 * np.log(2 * np.pi * alpha) - W ** 2 / (2 * alpha), axis=1)   # tools.LogNormPDF(0, w, alpha)
        return f @ t - np.sum(np.log(1 + np.exp(f)), axis=1) + prior

    w = np.zeros((n, D)) if theta0 is None else np.array(np.broadcast_to(theta0, (n, D)), dtype=np.float64)
    sd = np.ones((n, D)); accw = np.zeros((n, D))
    W = np.zeros((n, n_iter, D)); L = np.zeros((n, n_iter)); A = np.zeros((n, n_iter, D), bool); U = np.zeros((n, n_iter, D), bool)
    with np.errstate(all="ignore"):
        cur = ljl(w)
        for it in range(n_iter):
            z, u = draws(it)
            for d in range(D):
                wn = w.copy()
                wn[:, d] = w[:, d] + z[:, d] * sd[:, d]
                prop = ljl(wn)
                ratio = prop - cur
                acc = ratio > 0
                ur = ~acc
                acc = acc | (ur & (ratio > np.log(u[:, d])))
                cur = np.where(acc, prop, cur)
                w = np.where(acc[:, None], wn, w)
                accw[:, d] += acc
                A[:, it, d] = acc; U[:, it, d] = ur
            W[:, it] = w; L[:, it] = cur
            if it % 100 == 0 and it < burn_in:
                ar = accw / (1.0 if it == 0 else 100.0)
                sd = np.where(ar > 0.5, sd * 1.2, np.where(ar < 0.2, sd * 0.8, sd))
                accw[:] = 0
    return dict(w=W, ljl=L, sd=sd, accepted=A, u_read=U)


# ---- Philox4x32-10 streams of amh.hip.h ----------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k):
    """c: 4 uint64 arrays holding 32-bit words, k: 2 of them.  Random123's Philox4x32-10."""
    c0, c1, c2, c3 = [np.asarray(x, dtype=np.uint64) & M32 for x in c]
    k0, k1 = [np.asarray(x, dtype=np.uint64) & M32 for x in k]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64) + 0.5) / 9007199254740992.0


def philox_draws(seed, chains, D):
    """draws(it) for amh_numpy: z and u of global chain ids `chains` at iteration it (stream layout in amh.hip.h)"""
    g = np.asarray(chains, dtype=np.uint64)[:, None]
    j = np.arange(D, dtype=np.uint64)[None, :]
    odd = (j & np.uint64(1)) == 1
    key = (np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))

    def block(it, base):
        c = philox4x32_10((g & M32, g >> np.uint64(32), np.full_like(g, it), np.uint64(base) + (j >> np.uint64(1))), key)
        return _u53(c[0], c[1]), _u53(c[2], c[3])

    def draws(it):
        U0, U1 = block(it, 0x50000000)
        V0, V1 = block(it, 0x50001000)
        z = np.sqrt(-2.0 * np.log(U0)) * np.where(odd, np.sin(2 * np.pi * U1), np.cos(2 * np.pi * U1))
        return z, np.where(odd, V1, V0)
    return draws


def tape_draws(g):
    return lambda it: (g["z"][it][None], g["u"][it][None])


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def _amh_header_symbols():
    hdr = open(os.path.join(ROOT, "include", "rmhmc_amh.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", hdr)))


def test_amh_header_binding_and_exports_agree(hip, oracle):
    import ctypes
    syms = _amh_header_symbols()
    assert syms == ["rmhmc_amh_replay", "rmhmc_amh_sample"]
    assert set(syms) == set(_capi.AMH_SIGNATURES)
    assert not set(syms) & set(_capi.SIGNATURES)      # rmhmc.h stays the oracle's ABI
    lib = ctypes.CDLL(hip.path)
    for s in syms:
        assert hasattr(lib, s), s
    assert hip.has_amh and not oracle.has_amh
    # the argument lists of the header and of the binding have the same length
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmhmc_amh.h")).read(), flags=re.S)
    for s in syms:
        args = re.search(s + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(args.split(",")) == len(_capi.AMH_SIGNATURES[s][1]), s


def test_oracle_context_has_no_amh(oracle):
    with oracle.context(5, 2, 1) as ctx:
        ctx.set_data(np.eye(5, 2), np.zeros(5))
        with pytest.raises(_capi.RmhmcError):
            ctx.amh_sample(4, 1)


@pytest.mark.parametrize("name", AMH_TAPES)
def test_numpy_restatement_reproduces_tape(name):
    XX, t, g = load_amh_tape(name)
    T, B = int(g["n_iter"]), int(g["burn_in"])
    r = amh_numpy(XX, t, T, B, tape_draws(g))
    np.testing.assert_array_equal(r["accepted"][0], g["accepted"] != 0)
    np.testing.assert_array_equal(r["u_read"][0], ~np.isnan(g["u"]))
    np.testing.assert_array_equal(r["w"][0], g["w"])
    np.testing.assert_array_equal(r["sd"][0], g["sd"][-1])
    fin = np.isfinite(g["ljl"])
    np.testing.assert_allclose(r["ljl"][0][fin], g["ljl"][fin], rtol=1e-12)
    np.testing.assert_array_equal(g["wSaved"][1:], g["w"][B + 1:])     # the reference's rows 1.. = state after iteration BurnIn + k


def test_tapes_cover_adaptation_and_overflow():
    _, _, g = load_amh_tape("australian")
    assert len({tuple(s) for s in g["sd"]}) >= 3                       # SD changed at iterations 0, 100 and 200
    XX, t, g = load_amh_tape("syn_m200_d6_x300")
    # exp(f) overflowed for many proposals: the reference's LJL was -inf, u was read and the proposal rejected
    w, sd, overflow = np.zeros(6), np.ones(6), 0
    for it in range(int(g["n_iter"])):
        for d in range(6):
            wn = w.copy(); wn[d] += g["z"][it, d] * sd[d]
            if (XX @ wn).max() > 709.79:
                overflow += 1
                assert not g["accepted"][it, d] and not np.isnan(g["u"][it, d])
            if g["accepted"][it, d]:
                w = wn
        sd = g["sd"][it]
    assert overflow > 100 and g["accepted"].sum() > 0


def test_numpy_philox_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = philox4x32_10([np.uint64(x) for x in ctr], [np.uint64(x) for x in key])
        assert tuple(int(x) for x in got) == want
    z, u = philox_draws(7, [0, 1, 2 ** 33], 5)(3)
    assert z.shape == u.shape == (3, 5) and np.all((u > 0) & (u < 1)) and np.all(np.isfinite(z))


def test_amh_shim_argument_checks():
    from riemannhamiltonianmontecarlo_amd import AMH
    X = np.zeros((5, 2)); t = np.zeros(5)
    for bad in (dict(NumOfIterations=10, BurnIn=10), dict(NumOfIterations=10, BurnIn=12), dict(NumOfIterations=10, BurnIn=-1)):
        with pytest.raises(ValueError):
            AMH(X, t, verbose=False, **bad)
    with pytest.raises(ValueError):
        AMH(X, np.zeros(4))
    assert experiment.SAMPLERS["AMH"] is AMH


def test_dropin_module_reaches_the_gpu_shim():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_metropolis", os.path.join(ROOT, "dropin", "metropolis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from riemannhamiltonianmontecarlo_amd.metropolis import AMH
    assert mod.AMH is AMH
