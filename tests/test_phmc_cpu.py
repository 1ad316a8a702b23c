"""CPU-side checks of the fixed-metric HMC sampler, include/rmhmc_phmc.h: the header, the ctypes binding and the library's exports
agree and stay out of every other table; the shim's argument checks raise before a library is touched; the NumPy restatement
tests/helpers/phmc_ref.py with the identity as mass matrix reproduces the CPU oracle's plain HMC transition (which is pinned to the
reference's tapes), so that the GPU tests compare against something that is itself checked; and csrc/mass.h in a stand-alone program
under AddressSanitizer and UBSan (tests/helpers/mass_probe.cpp, a child process: nothing sanitised is loaded into this one)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err
from riemannhamiltonianmontecarlo_amd import PHMC, _capi, experiment, multi_gpu
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import phmc_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

HEADER = os.path.join(ROOT, "include", "rmhmc_phmc.h")
SYMBOLS = {"rmhmc_phmc_set_mass", "rmhmc_phmc_mode", "rmhmc_phmc_transition", "rmhmc_phmc_sample_to"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_and_binding_agree():
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert syms == SYMBOLS == set(_capi.PHMC_SIGNATURES)
    for other in (_capi.SIGNATURES, _capi.AMH_SIGNATURES, _capi.IWLS_SIGNATURES, _capi.GIBBS_SIGNATURES, _capi.OUT_SIGNATURES,
                  _capi.DIAG_SIGNATURES):
        assert not syms & set(other)
    for name, (res, args) in _capi.PHMC_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc_out.h"]


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_phmc and not oracle.has_phmc
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with oracle.context(10, 2, 1) as ctx:           # a library without the sampler says so, with the header's name
        for call in (ctx.phmc_set_mass, ctx.phmc_mode, lambda: ctx.phmc_sample_to(4, 1, samples=True)):
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_phmc.h" in str(e.value)


def test_sampler_tables_unchanged():
    assert set(_capi.SAMPLERS_TO) == set(_capi.SAMPLER_ARGS) == {"rmhmc", "hmc", "mmala", "amh", "iwls", "gibbs"}
    assert set(experiment.SAMPLERS) == {"RMHMC", "HMC", "mMALA", "AMH", "IWLS", "Gibbs"}
    assert _capi.SUMMARY_KEYS == ("mean", "var", "ess", "run_mean", "run_ess")
    assert set(multi_gpu._SHARDED) == set(experiment.SAMPLERS)


class _NoLibrary:
    """stands in for the library: the argument checks must raise before anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the shim touched the library (%s) before refusing its arguments" % name)


def test_shim_argument_checks_need_no_library():
    XX, t = synthetic_logreg(30, 3, 0)
    bad = [dict(XX=XX[0]), dict(t=t[:-1]), dict(BurnIn=10, NumOfIterations=10), dict(diagnostics=True), dict(ess_nfft="numpy"),
           dict(diagnostics=True, return_info=True, NumOfIterations=12, BurnIn=10), dict(mass="hessian"), dict(mass=np.eye(4)),
           dict(theta0="zero")]
    for kw in bad:
        args = dict(XX=XX, t=t, NumOfIterations=20, BurnIn=5, _lib=_NoLibrary())
        args.update(kw)
        with pytest.raises(ValueError):
            PHMC(**args)


# ---- the restatement with the identity as mass matrix is the oracle's plain HMC ------------------------------------------------------
@pytest.mark.parametrize("M,D,n", [(400, 12, 6), (250, 150, 4)])
def test_restatement_with_identity_mass_is_the_oracle_hmc(oracle, M, D, n):
    XX, t = synthetic_logreg(M, D, 0)
    rs = np.random.RandomState(M + D)
    w = 0.1 * rs.randn(n, D); z = rs.randn(n, D)
    u_len = rs.uniform(0.05, 1.0, n); u_acc = rs.uniform(0.05, 1.0, n)
    u_len[0] = 1.0                                     # the longest trajectory
    L, eps = 12, 0.02
    with oracle.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        o = ctx.hmc_transition(w, z, u_len, u_acc, L=L, eps=eps)
    for Lm in (None, np.eye(D)):
        r = R.transitions(XX, t, Lm, w, z, u_len, u_acc, L, eps)
        assert (np.abs(r["margin"]) > 1e-6).all() and (r["status"] == 0).all()
        assert np.array_equal(r["nsteps"], o["nsteps"]) and np.array_equal(r["accepted"], o["accepted"]) and o["nsteps"][0] == L
        err = {k: rel_err(r[k], o[k]) for k in ("w", "w_prop", "p_prop", "H_cur", "H_prop")}
        print(M, D, n, err)
        assert max(err.values()) < 1e-12, err


def test_restatement_mode_is_a_stationary_point():
    XX, t = synthetic_logreg(200, 9, 3)
    m = R.mode(XX, t)
    _, g0 = R.ljl_grad(XX, t, np.zeros(9))
    _, g = R.ljl_grad(XX, t, m["w"])
    assert m["converged"] and 2 <= m["iters"] <= 20 and np.abs(g).max() <= 1e-9 * np.abs(g0).max()
    assert np.allclose(m["G"], R.metric(XX, m["w"]), rtol=0, atol=0)


# ---- csrc/mass.h in a stand-alone program under AddressSanitizer and UBSan -----------------------------------------------------------
def _probe(exe, mass, D, DP):
    body = "identity" if mass is None else " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.ravel(mass))
    r = subprocess.run([exe], input="%d %d\n%s\n" % (D, DP, body), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    rc = int(lines[0].split()[1])
    if rc != 0:
        return rc, lines[0], None, None
    Lm, Mi = (np.array([float.fromhex(v) for v in ln.split()]).reshape(DP, DP) for ln in lines[1:3])
    return rc, lines[0], Lm, Mi


@pytest.mark.parametrize("D,DP", [(1, 16), (7, 16), (64, 64), (256, 256), (65, 128)])
def test_mass_header_under_sanitizers(tmp_path_factory, D, DP):
    exe = probe_exe(tmp_path_factory, "mass_probe")
    rs = np.random.RandomState(D)
    A = rs.randn(D, 2 * D + 3)
    mass = A @ A.T / (2 * D + 3) + 0.5 * np.eye(D)      # condition number of a few tens: 1e-12 leaves room over D eps cond
    upper_garbage = np.tril(mass) + np.triu(rs.randn(D, D), 1)   # only the lower triangle is read
    rc, _, Lm, Mi = _probe(exe, upper_garbage, D, DP)
    assert rc == 0
    assert rel_err(Lm[:D, :D], np.linalg.cholesky(mass)) < 1e-12 and rel_err(Mi[:D, :D], np.linalg.inv(mass)) < 1e-12
    assert np.array_equal(Mi, Mi.T) and not np.triu(Lm, 1).any()
    for img in (Lm, Mi):                                # zero padding
        assert not img[D:].any() and not img[:, D:].any()
    rc, _, Lm, Mi = _probe(exe, None, D, DP)            # NULL: exact zeros and ones
    eye = np.zeros((DP, DP)); eye[:D, :D] = np.eye(D)
    assert rc == 0 and np.array_equal(Lm, eye) and np.array_equal(Mi, eye)


def test_mass_header_refusals(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "mass_probe")
    good = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    assert _probe(exe, good, 3, 16)[0] == 0
    nan = good.copy(); nan[2, 1] = np.nan
    inf = good.copy(); inf[1, 1] = np.inf
    zero = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])     # second pivot exactly 0
    neg = good.copy(); neg[2, 2] = -2.0
    for bad, word in ((nan, "non-finite"), (inf, "non-finite"), (zero, "pivot"), (neg, "pivot")):
        rc, msg, _, _ = _probe(exe, bad, 3, 16)        # (the probe itself checks that a refusal leaves the images untouched)
        assert rc == -1 and word in msg, msg
    ok = good.copy(); ok[0, 2] = np.nan                 # above the diagonal: not read
    assert _probe(exe, ok, 3, 16)[0] == 0
