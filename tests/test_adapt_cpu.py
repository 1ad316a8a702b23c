"""CPU-side checks of the warm-up of the fixed-metric HMC sampler, include/rmhmc_adapt.h: the header, the ctypes binding and the
library's exports agree; csrc/adapt.h (merge and finish of covariance partials, the regularised mass, dual averaging, the schedule,
the row blocks) in a stand-alone program under AddressSanitizer and UBSan (tests/helpers/adapt_probe.cpp, a child process: nothing
sanitised is loaded into this one) against the NumPy restatement tests/helpers/adapt_ref.py; and the restated warm-up on pima, whose
figures set the bands of the statistical GPU test (tests/test_gpu_adapt.py).

Tolerances: merged partials and covariances rtol 1e-13 of the largest entry (a dozen operations per entry); the mass rtol 1e-9 (an
inverse of a matrix of condition < 1e4); dual averaging 4 ulp (five operations and three libm calls per update; measured 0)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from riemannhamiltonianmontecarlo_amd import PHMC, _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adapt_ref as A  # noqa: E402
import phmc_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

SYMBOLS = {"rmhmc_cov_partial_dev", "rmhmc_cov_finish", "rmhmc_adapt_mass", "rmhmc_adapt_init", "rmhmc_adapt_step", "rmhmc_phmc_warmup"}
_cache = {}


def _header():
    return open(os.path.join(ROOT, "include", "rmhmc_adapt.h")).read()


# ---- the header, the binding, the exports -----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert syms == SYMBOLS == set(_capi.ADAPT_SIGNATURES)
    for other in (_capi.SIGNATURES, _capi.AMH_SIGNATURES, _capi.IWLS_SIGNATURES, _capi.GIBBS_SIGNATURES, _capi.OUT_SIGNATURES,
                  _capi.DIAG_SIGNATURES, _capi.PHMC_SIGNATURES):
        assert not syms & set(other)
    for name, (res, args) in _capi.ADAPT_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc_phmc.h"]


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_adapt and not oracle.has_adapt
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with oracle.context(10, 2, 1) as ctx:           # a library without the warm-up says so, with the header's name
        calls = (lambda: ctx.cov_partial(None), lambda: ctx.pooled_cov(None), lambda: ctx.phmc_warmup([1, 1, 1], [0, 1, 0]),
                 lambda: _capi.cov_finish([np.zeros((3, 1))], lib=oracle), lambda: _capi.adapt_mass(np.eye(2), 9, lib=oracle),
                 lambda: _capi.adapt_init(0.5, 10.0, lib=oracle), lambda: _capi.adapt_step(np.zeros(4), 0.5, lib=oracle))
        for call in calls:
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_adapt.h" in str(e.value)


# ---- csrc/adapt.h in a stand-alone program under AddressSanitizer and UBSan ----------------------------------------------------------------
def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _floats(line):
    return np.array([float.fromhex(v) for v in line.split()])


def _hex(a):
    return " ".join(float(v).hex() for v in np.ravel(a))


def _finish(exe, parts, P):
    lines = _run(exe, "finish %d %d\n" % (len(parts), P) + "\n".join(_hex(p) for p in parts) + "\n")
    head = lines[0].split()
    assert head[0] == "finish"
    out = dict(rc=int(head[1]), m=int(head[2]))
    if out["rc"] == 0:
        out.update(merged=_floats(lines[1]).reshape(2 + P, P), mean=_floats(lines[2]), cov=_floats(lines[3]).reshape(P, P))
    return out


def _rows(N, P, seed):
    rs = np.random.RandomState(seed)
    mix = rs.randn(P, P) / np.sqrt(P) + np.eye(P)
    return rs.randn(N, P) @ mix.T + 10.0 * rs.randn(P)


def _close(got, want, rtol):
    want = np.asarray(want)
    return bool(np.all(np.abs(got - want) <= rtol * max(np.abs(want).max(), 1e-300)))


def test_merge_and_finish_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "adapt_probe")
    P = 5
    x = _rows(91, P, 0)
    whole = A.partial(x)
    pieces = [A.partial(x[:7]), A.partial(x[7:8]), A.partial(x[8:60]), A.partial(x[60:])]      # unequal, one of a single row
    empty = np.zeros((2 + P, P))
    for parts in ([whole], pieces, [empty] + pieces[:2] + [empty] + pieces[2:] + [empty]):
        got = _finish(exe, parts, P)
        merged, mean, cov, m = A.finish(parts)
        assert got["rc"] == 0 and got["m"] == m == 91
        assert _close(got["merged"], merged, 1e-13) and _close(got["mean"], mean, 1e-13) and _close(got["cov"], cov, 1e-13)
        assert _close(got["merged"], whole, 1e-13) and _close(got["cov"], np.cov(x.T), 1e-13)
        assert np.array_equal(got["merged"][2:], got["merged"][2:].T) and (got["merged"][0] == 91).all()
    one = [A.partial(x[:1])]                                                                   # m < 2: NaN covariance
    for parts, m in ((one, 1), ([empty, empty], 0)):
        got = _finish(exe, parts, P)
        assert got["rc"] == 0 and got["m"] == m and np.isnan(got["cov"]).all()
    got = _finish(exe, [empty] + one, P)                                                       # the identity, to the bit
    assert got["merged"].tobytes() == one[0].tobytes()
    assert _finish(exe, [], P)["rc"] == -1 and _finish(exe, [np.zeros(0)], 0)["rc"] == -1


def _mass(exe, cov, m):
    P = cov.shape[0]
    lines = _run(exe, "mass %d %d\n%s\n" % (P, m, _hex(cov)))
    rc = int(lines[0].split()[1])
    return rc, (_floats(lines[1]).reshape(P, P) if rc == 0 else None)


def test_regularised_mass_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "adapt_probe")
    P = 6
    cov = np.cov(_rows(40, P, 1).T)
    rc, mass = _mass(exe, cov, 40)
    assert rc == 0 and np.array_equal(mass, mass.T)
    assert _close(mass, A.mass_from_cov(cov, 40), 1e-9)
    assert _close(mass @ A.shrink(cov, 40), np.eye(P), 1e-9)                # the shrinkage rule itself, restated
    flat = np.cov(_rows(3, P, 2).T)                                         # rank 2: the shrinkage makes it positive definite
    rc, mass = _mass(exe, flat, 3)
    assert rc == 0 and _close(mass @ A.shrink(flat, 3), np.eye(P), 1e-6)
    nan = cov.copy(); nan[2, 1] = nan[1, 2] = np.nan
    inf = cov.copy(); inf[0, 0] = np.inf
    neg = cov.copy(); neg[3, 3] = -1.0                                      # not positive definite even after shrinkage
    # singular to the bit: with m = 2^62 the weights are 1 and 1e-21, so Sigma_reg is the matrix of ones and the second pivot is 0
    for bad, m in ((nan, 40), (inf, 40), (neg, 40), (np.ones((P, P)), 2 ** 62), (cov, 1), (cov, 0)):
        assert _mass(exe, bad, m)[0] == -1
        assert A.mass_from_cov(bad, m) is None


ACCEPTS = [0.31, 0.62, 0.95, 0.88, 0.71, "restart", 0.83, 0.79, 1.0, 0.0, 0.8, "restart", 0.55, 0.81, 0.8, 0.79]   # a recorded sequence


def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def test_dual_averaging_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "adapt_probe")
    for eps0, da in ((0.5, A.DEFAULTS), (0.03, dict(delta=0.65, gamma=0.1, t0=5.0, kappa=0.6))):
        head = "da %s %s %s %s %s %d\n" % (float(eps0).hex(), float(da["delta"]).hex(), float(da["gamma"]).hex(), float(da["t0"]).hex(),
                                         float(da["kappa"]).hex(), len(ACCEPTS))
        lines = _run(exe, head + " ".join(a if isinstance(a, str) else float(a).hex() for a in ACCEPTS) + "\n")
        state = A.adapt_init(eps0)
        eps, bar = eps0, eps0
        worst = 0.0
        for a, line in zip(ACCEPTS, lines):
            tok = line.split()
            assert tok[0] == "da" and int(tok[1]) == 0
            got = [float.fromhex(v) for v in tok[2:]]
            if a == "restart":
                state = A.adapt_init(eps, 1.0)
            else:
                eps, bar = A.adapt_step(state, a, **da)
            for g, w in zip(got, [eps, bar] + list(state)):
                worst = max(worst, _ulps(g, w) if w != 0.0 else abs(g))
            assert got[2] == state[0]
        print("dual averaging, eps0 %g: worst difference %.2f ulp" % (eps0, worst))
        assert worst <= 4.0
        assert eps != eps0 and state[0] == 4.0                                # four steps since the last restart
    # refusals: a non-finite statistic, a step size that overflows; the state stays and the sequence goes on
    lines = _run(exe, "da 0.5 0.8 0.05 10 0.75 4\n0.5 nan inf 0.5\n")
    rcs = [int(line.split()[1]) for line in lines]
    assert rcs == [0, -1, -1, 0] and lines[1].split()[2:] == lines[0].split()[2:] == lines[2].split()[2:]
    lines = _run(exe, "da 1e300 0.8 1e-9 10 0.75 1\n0.0\n")                   # log eps = log 1e301 - 7e7: eps underflows to 0
    assert int(lines[0].split()[1]) == -1
    assert _run(exe, "da -1 0.8 0.05 10 0.75 0\n") == []


@pytest.mark.parametrize("W", [3, 4, 10, 40])
def test_schedule(tmp_path_factory, W):
    exe = probe_exe(tmp_path_factory, "adapt_probe")
    want = {3: [0, 1, 0], 4: [0, 1, 1, 0], 10: [0, 0] + [1] * 7 + [0], 40: [0] * 6 + [1] * 30 + [0] * 4}[W]    # by hand
    for warmup, window in ((25 * W, 25), (7 * W + 6, 7)):
        length, kind = _capi.adapt_schedule(warmup, window)
        assert kind.tolist() == want and length.tolist() == [window] * W and kind.dtype == np.int32 and length.dtype == np.int64
        assert A.schedule(warmup, window) == ([window] * W, want)
        assert _run(exe, "sched %d %d\n" % (warmup, window)) == ["sched %d %s" % (W, " ".join(str(k) for k in want))]
    if W == 3:
        assert _run(exe, "sched 74 25\n") == ["sched 0"] and _run(exe, "sched 10 0\n") == ["sched 0"]
        for bad in ((74, 25), (10, 0), (0, 25)):
            with pytest.raises(ValueError):
                _capi.adapt_schedule(*bad)


def test_row_blocks(tmp_path_factory):
    """the row blocks of the covariance kernels, asked of csrc/adapt.h.  By hand: at least 256 rows per block; at most 1024 blocks and
    at most 4 MiB / (8 P^2) of them in the second pass (8 at P = 256, 128 at P = 64); rows per block of the second pass a multiple of 4"""
    exe = probe_exe(tmp_path_factory, "adapt_probe")
    want = {(1, 1): (1, 4, 1, 1), (255, 5): (1, 256, 1, 255), (256, 64): (1, 256, 1, 256), (257, 64): (2, 132, 2, 129),
            (1000, 256): (4, 252, 4, 250), (204800, 64): (128, 1600, 800, 256), (204800, 256): (8, 25600, 800, 256),
            (163840000, 8): (1024, 160000, 1024, 160000)}
    lines = _run(exe, "".join("plan %d %d\n" % k for k in want))
    assert {k: tuple(int(v) for v in line.split()[1:]) for k, line in zip(want, lines)} == want
    assert _capi.COV_ROWS == 256 and _capi.COV_MAX_P == 256


# ---- the shim's checks: before the library is touched ------------------------------------------------------------------------------------
def test_shim_refuses_bad_arguments_before_the_library():
    XX = np.ones((5, 2)); t = np.ones(5)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was touched: " + name)

    for kw in (dict(warmup=-1), dict(warmup=74), dict(warmup=100, window=0), dict(warmup=100, target_accept=1.0),
               dict(warmup=100, target_accept=0.0), dict(warmup=100, target_accept=np.nan), dict(warmup=2.5)):
        with pytest.raises(ValueError):
            PHMC(XX, t, 20, 10, verbose=False, _lib=Untouchable(), **kw)


# ---- the restated warm-up: does the scheme adapt at all, and by how much does it miss its target -------------------------------------------
SEEDS = range(8)


def restated_warmup(seed):
    """pima, 64 chains, warmup = 300 from the identity mass and eps0 = 0.5, then 100 iterations: computed once per seed and shared"""
    if ("warm", seed) not in _cache:
        d = np.load(os.path.join(GOLDEN, "data_pima.npz"))
        XX, t = d["XX"], d["t"]
        n = 64
        length, kind = _capi.adapt_schedule(300, 25)
        r = A.warmup(XX, t, n, length, kind, L=6, eps0=0.5, mass=None, seed=seed)
        rs = np.random.RandomState(1000 + seed)
        _, acc = A.run_window(XX, t, np.linalg.cholesky(r["mass"]) if r["mass"] is not None else None, r["theta"], 100, 6, r["step_size"], rs)
        r["post_accept"] = acc.sum() / (n * 100.0)
        G = R.metric(XX, R.mode(XX, t)["w"])
        if r["mass"] is not None:       # spectrum of mass G^-1: all ones were the adapted mass the metric at the mode
            Lg = np.linalg.cholesky(G)
            r["spectrum"] = np.linalg.eigvalsh(np.linalg.solve(Lg, np.linalg.solve(Lg, r["mass"]).T))
        _cache[("warm", seed)] = r
    return _cache[("warm", seed)]


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_warmup_adapts(seed):
    """Each seed prints its figures.  Measured, seeds 0..7: adapted eps 0.879 .. 0.922; 9 mass updates each; post-warm-up acceptance
    0.8053, 0.8180, 0.8217, 0.8183, 0.8309, 0.8205, 0.8252, 0.8180 (|a - 0.8| at most 0.0309: the band of
    tests/test_gpu_adapt.py::test_warmup_statistics is twice that); spectrum of mass G(mode)^-1 within 0.78 .. 1.28.  With the paper's
    factor 10 at the restarts as well the same runs end at eps = 3457 .. 3710 and accept nothing (include/rmhmc_adapt.h)."""
    r = restated_warmup(seed)
    dev = abs(r["post_accept"] - 0.8)
    print("seed %d: eps %.4f, mass updates %d, post-warm-up acceptance %.4f (|a - 0.8| = %.4f), spectrum of mass G(mode)^-1 %.3f .. %.3f"
          % (seed, r["step_size"], (r["mass_updated"] == 1).sum(), r["post_accept"], dev, r["spectrum"].min(), r["spectrum"].max()))
    assert r["step_size"] != 0.5 and np.isfinite(r["step_size"])
    assert (r["mass_updated"] == 1).sum() >= 1
    assert 0.5 < r["post_accept"] < 0.99
