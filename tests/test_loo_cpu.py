"""CPU-side checks of leave-one-out cross-validation, include/rmhmc_loo.h: the header, the ctypes binding and the library's exports agree;
csrc/loo.h (the tail length, the merge of moments partials, the finish, the host checks, the kernels' plan) through the loaded library
and again in a stand-alone program under AddressSanitizer and UBSan (tests/helpers/loo_probe.cpp, a child process: nothing sanitised is
loaded into this one), both against the np.longdouble restatement tests/helpers/loo_ref.py; the restatement itself against independent
facts (generalised Pareto recovery, scale-freeness, the unsmoothed estimator by brute force, exact leave-one-out by quadrature); the
shim's argument checks.

Bounds of the host half (u = 2^-53; the probe works in doubles on the same double partials the restatement takes in long doubles).
Merge of k partials: m exact; the mean moves by delta m_b / m per step, three roundings on numbers no larger than the means, so
|mean - ref| <= 4 k u max|mean_i|; M2 gains positive terms only, each with a few roundings: (4 k + 2) u relative, plus what the error
of delta does to delta^2 m_a m_b / m: 8 k u max|mean_i| |delta| m, allowed as a relative (4 k + 2) u on M2 + m max|mean|^2; SQ k u
relative; lmin exact.  Finish: lppd = log(SQ / m): (k + 1) u + 2 u max(1, |ref|) as in test_pred_cpu; p_waic: M2's bound plus 2 u
relative; elpd_loo = log(B) - log(A) from sums of two doubles each: 2 u + 2 u (|log B| + |log A|) + u |ref|, allowed as
4 u max(1, |log A| + |log B|)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import riemannhamiltonianmontecarlo_amd as pkg
from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment, multi_gpu
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loo_quad as Q  # noqa: E402
import loo_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

SYMBOLS = {"rmhmc_loo_loglik_dev", "rmhmc_loo_moments_dev", "rmhmc_loo_plan", "rmhmc_loo_split_dev", "rmhmc_loo_fit_dev", "rmhmc_loo_finish",
           "rmhmc_loo_dev"}
U = 2.0 ** -53
EDGE = 29826161          # the largest m whose tail is RMHMC_LOO_MAX_TAIL draws: 9 m <= 16384^2 < 9 (m + 1)


def _header():
    return open(os.path.join(ROOT, "include", "rmhmc_loo.h")).read()


# ---- the header, the binding, the exports -----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", code))
    assert syms == SYMBOLS == set(_capi.LOO_SIGNATURES)
    others = [v for k, v in vars(_capi).items() if k.endswith("SIGNATURES") and k != "LOO_SIGNATURES"]
    assert len(others) >= 10
    for other in others:
        assert not syms & set(other)
    for name, (res, args) in _capi.LOO_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc.h"]
    assert _capi.FEATURES["loo"] == (_capi.LOO_SIGNATURES, "leave-one-out cross-validation (include/rmhmc_loo.h)")
    assert pkg.psis_loo is pkg.loo.psis_loo and "psis_loo" in pkg.__all__
    for name in ("loo_loglik", "loo_moments", "loo_split", "loo_fit", "loo"):
        assert callable(getattr(_capi.Context, name)), name
    # the constants of the header, of the binding and of the host half
    hdr = open(os.path.join(ROOT, "riemannhamiltonianmontecarlo_amd", "csrc", "loo.h")).read()
    for mine, theirs, value in (("LOO_MAX_COLS", "RMHMC_LOO_MAX_COLS", 64), ("LOO_MAX_TAIL", "RMHMC_LOO_MAX_TAIL", 16384)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % mine, hdr).group(1)) == getattr(_capi, mine) == value
        assert int(re.search(r"#define\s+%s\s+(\d+)" % theirs, _header()).group(1)) == value
    assert int(re.search(r"#define\s+LOO_MAX_D\s+(\d+)", hdr).group(1)) == _capi.LOO_MAX_D == 256 and R.MAX_TAIL == 16384


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_loo and not oracle.has_loo
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with pytest.raises(_capi.RmhmcError) as e:
        oracle.need("loo")
    assert e.value.code == -4
    with oracle.context(10, 2, 1) as ctx:           # a library without the calls says so, with the header's name
        calls = (lambda: ctx.loo_loglik(None, None, None), lambda: ctx.loo_moments(None), lambda: ctx.loo_split(None, None, None, None),
                 lambda: ctx.loo_fit(None, None, None, None, None), lambda: ctx.loo(None, None, None),
                 lambda: _capi.loo_finish([np.zeros((5, 3))], lib=oracle), lambda: _capi.loo_plan([5], lib=oracle),
                 lambda: pkg.psis_loo(np.zeros((4, 2)), np.zeros(4), n_chains=2, _lib=oracle))
        for call in calls:
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_loo.h" in str(e.value)
    ident = _capi.loo_identity(3)
    assert ident.shape == (5, 3) and not ident[:4].any() and np.all(ident[4] == np.inf)


def test_sampler_tables_unchanged():
    assert set(_capi.SAMPLERS_TO) == set(_capi.SAMPLER_ARGS) == {"rmhmc", "hmc", "mmala", "amh", "iwls", "gibbs"}
    assert set(experiment.SAMPLERS) == {"RMHMC", "HMC", "mMALA", "AMH", "IWLS", "Gibbs"}
    assert set(multi_gpu._SHARDED) == set(experiment.SAMPLERS)


# ---- the shim's checks: before the library is touched ------------------------------------------------------------------------------------
class _NoLibrary:
    """stands in for the library: the argument checks must raise before anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the shim touched the library (%s) before refusing its arguments" % name)


def test_shim_argument_checks_need_no_library():
    XX, t = synthetic_logreg(30, 3, 0)
    nan_x = XX.copy(); nan_x[1, 2] = np.nan
    half = t.copy(); half[3] = 0.5
    bad = [dict(XX=XX[0]), dict(XX=XX[:0]), dict(XX=nan_x), dict(XX=np.zeros((5, 257)), t=np.zeros(5)), dict(t=t[:-1]), dict(t=half),
           dict(t=np.where(t > 0, 1.0, -1.0)), dict(n_chains=0), dict(n_chains=2.5), dict(NumOfIterations=10, BurnIn=10), dict(BurnIn=-1),
           dict(NumOfIterations=2.5), dict(NumOfLeapFrogSteps=0), dict(StepSize=0.0), dict(StepSize=np.nan), dict(alpha=0.0),
           dict(alpha=np.inf), dict(cols_per_block=-1), dict(cols_per_block=65), dict(cols_per_block=1.5)]
    for kw in bad:
        args = dict(XX=XX, t=t, n_chains=8, _lib=_NoLibrary())
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.psis_loo(**args)


# ---- csrc/loo.h through the library and in a stand-alone program under AddressSanitizer and UBSan --------------------------------------------
def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _floats(line):
    return np.array([float.fromhex(v) if "x" in v else float(v) for v in line.split()])


def _hex(a):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.ravel(a))


def _probe_plan(exe, m):
    lines = _run(exe, "plan %d %s\n" % (len(m), " ".join(str(int(v)) for v in m)))
    rc = int(lines[0].split()[1])
    if rc != 0:
        return rc, None, None
    return rc, np.array(lines[1].split(), dtype=np.int64), np.array(lines[2].split(), dtype=np.int64)


def _lib_plan(hip, m):
    try:
        return (0,) + _capi.loo_plan(m, lib=hip)
    except _capi.RmhmcError as e:
        return e.code, None, None


def test_plan(hip, tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "loo_probe")
    ms = [0, 1, 24, 25, 26, 224, 225, 226, 2 ** 20, EDGE - 1, EDGE]
    # by hand: M = min(floor(m / 5), ceil(3 sqrt(m)))
    by_hand = {0: 0, 1: 0, 24: 4, 25: 5, 26: 5, 224: 44, 225: 45, 226: 45, 2 ** 20: 3072, EDGE: 16384}
    want = R.plan(ms)
    for m, M in by_hand.items():
        assert want[0][ms.index(m)] == M == R.tail_len(m), m
    assert R.tail_len(225) == 225 // 5 == 45 and 45 * 45 == 9 * 225           # both rules give 45
    assert want[1][ms.index(24)] == -1 and want[1][ms.index(25)] == 5
    for ask in (lambda m: _probe_plan(exe, m), lambda m: _lib_plan(hip, m)):
        rc, tl, rank = ask(ms)
        assert rc == 0 and np.array_equal(tl, want[0]) and np.array_equal(rank, want[1])
        # the edge of RMHMC_LOO_MAX_TAIL, and far beyond it: refused as unsupported, nothing written
        assert ask([EDGE])[0] == 0 and ask([EDGE + 1])[0] == -4 and ask([10, 2 ** 40 + 1, 10])[0] == -4
        assert R.tail_len(EDGE + 1) == 16385 and R.plan([EDGE + 1]) is None and R.tail_len(2 ** 40 + 1) == 3 * 2 ** 20 + 1
        assert ask([5, -1])[0] == -1


def _finish_probe(exe, parts, fit=None, body=None):
    Cn = np.asarray(parts[0]).shape[1]
    text = "finish %d %d %d\n" % (len(parts), Cn, fit is not None) + "\n".join(_hex(p) for p in parts) + "\n"
    if fit is not None:
        text += _hex(fit) + "\n" + _hex(body) + "\n"
    lines = _run(exe, text)
    head = lines[0].split()
    assert head[0] == "finish" and int(head[1]) == 0
    out = dict(k_mid=int(head[2]), k_high=int(head[3]), merged=_floats(lines[1]).reshape(5, Cn))
    for key, line in zip(_capi.LOO_POINTWISE, lines[2:8]):
        out[key] = _floats(line)
    out["totals"] = dict(zip(_capi.LOO_TOTALS, _floats(lines[8])))
    out["draws_used"] = np.array(lines[9].split(), dtype=np.int64)
    return out


def check_finish(got, parts, fit=None, body=None, what=""):
    """a finished result (doubles) against the restatement's finish of the same doubles in long doubles, to the module's bounds"""
    k = len(parts)
    lp = [np.asarray(p, dtype=R.LD) for p in parts]
    want = R.finish(lp, None if fit is None else np.asarray(fit, dtype=R.LD), None if body is None else np.asarray(body, dtype=R.LD))
    wm, gm = want["merged"], got["merged"]
    big = max(float(np.abs(p[1]).max()) for p in lp)
    assert np.array_equal(gm[0], wm[0].astype(np.float64)) and np.array_equal(gm[4], wm[4].astype(np.float64)), what
    assert np.array_equal(got["draws_used"], want["draws_used"]), what
    fin = np.isfinite(wm[1].astype(np.float64))
    assert np.array_equal(np.isnan(gm[1:4]), np.isnan(wm[1:4].astype(np.float64))), what
    assert np.all(np.abs(gm[1][fin] - wm[1][fin]) <= 4 * k * U * big), what
    assert np.all(np.abs(gm[2][fin] - wm[2][fin]) <= (4 * k + 2) * U * (wm[2][fin] + wm[0][fin] * big * big)), what
    assert np.all(np.abs(gm[3][fin] - wm[3][fin]) <= k * U * np.abs(wm[3][fin])), what
    for key in _capi.LOO_POINTWISE:
        g, w = got[key], np.asarray(want[key], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, key, g, w)
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), (what, key)
    assert (got["k_mid"], got["k_high"]) == (want["k_mid"], want["k_high"]), what
    tol = {}
    ok = np.isfinite(np.asarray(want["lppd"], dtype=np.float64))
    tol["lppd"] = (k + 1) * U + 2 * U * np.maximum(1.0, np.abs(want["lppd"].astype(np.float64)))
    m = wm[0].astype(np.float64)
    with np.errstate(all="ignore"):
        tol["p_waic"] = ((4 * k + 4) * U * (wm[2] + wm[0] * big * big) / np.maximum(m - 1, 1)).astype(np.float64)
        if fit is not None:
            la, lb = np.log(np.asarray(fit[2] + body[0], dtype=R.LD)), np.log(np.asarray(fit[3] + body[1], dtype=R.LD))
            tol["elpd_loo"] = 4 * U * np.maximum(1.0, (np.abs(la) + np.abs(lb)).astype(np.float64))
            tol["p_loo"] = tol["elpd_loo"] + tol["lppd"]
    tol["elpd_waic"] = tol["lppd"] + tol["p_waic"]
    for key, tl in tol.items():
        w = want[key]
        good = np.isfinite(np.asarray(w, dtype=np.float64))
        assert np.all(np.abs(got[key][good] - w[good]) <= tl[good] * 1.0001), (what, key)
    for key, tl_key in (("elpd_loo", "elpd_loo"), ("p_loo", "p_loo"), ("elpd_waic", "elpd_waic"), ("p_waic", "p_waic")):
        w = want["totals"][key]
        g = got["totals"][key]
        if np.isfinite(np.float64(w)) and tl_key in tol:
            Cn = len(got[key])
            assert abs(g - w) <= tol[tl_key].sum() + Cn * U * np.abs(want[key]).sum(), (what, key)
        else:
            assert np.isnan(g) == bool(np.isnan(w)) and (np.isnan(g) or g == w), (what, key)
    for key, src in (("se_elpd_loo", "elpd_loo"), ("se_elpd_waic", "elpd_waic")):
        w, g = want["totals"][key], got["totals"][key]
        if np.isfinite(np.float64(w)) and src in tol:
            # d se / d v_c <= sqrt(C / (C - 1)) <= sqrt(2) per entry in the 2-norm: the entries' errors add to at most 2 sum tol; the
            # arithmetic of the variance itself is 4 C u relative
            Cn = len(got[src])
            assert abs(g - w) <= 2 * tol[src].sum() + 4 * Cn * U * abs(w) + 4 * Cn * U * np.abs(want[src]).max(), (what, key)
        else:
            assert np.isnan(g) == bool(np.isnan(w)), (what, key)


def _ll_case(seed, N, Cn, scale=3.0):
    rs = np.random.RandomState(seed)
    return -np.abs(rs.randn(N, Cn)) * scale - rs.rand(N, Cn) * 1e-3


def _both(hip, exe):
    def lib(parts, fit=None, body=None):
        return _capi.loo_finish(parts, fit, body, lib=hip)
    return (("probe", lambda parts, fit=None, body=None: _finish_probe(exe, parts, fit, body)), ("library", lib))


def test_merge_and_finish(hip, tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "loo_probe")
    ll = _ll_case(0, 700, 6)
    ll[3, 2] = np.nan                      # left out of its own column only
    ll[5, 2] = -np.inf
    ll[:, 4] = np.nan                      # a column without a finite value: m = 0
    whole = R.moments(ll).astype(np.float64)
    assert whole[0].tolist() == [700, 700, 698, 700, 0, 700] and whole[4, 4] == np.inf
    fit64, body64, _ = R.columns(ll)
    fit64, body64 = fit64.astype(np.float64), body64.astype(np.float64)
    for name, fin in _both(hip, exe):
        for cuts in ([0, 700], [0, 250, 700], [0, 100, 101, 700]):         # k = 1, 2, 3 partials
            parts = [R.moments(ll[a:b]).astype(np.float64) for a, b in zip(cuts[:-1], cuts[1:])]
            got = fin(parts, fit64, body64)
            check_finish(got, parts, fit64, body64, "%s k = %d" % (name, len(parts)))
            # ... and against the partial of all rows at once
            k = len(parts)
            some = whole[0] > 0
            assert np.array_equal(got["merged"][0], whole[0]) and np.array_equal(got["merged"][4], whole[4])
            assert np.all(np.abs(got["merged"][1] - whole[1])[some] <= (4 * k + 2) * U * np.abs(whole[1]).max())
            assert np.all(np.abs(got["merged"][2] - whole[2])[some] <= (8 * k + 8) * U * (whole[2] + whole[0] * whole[1] ** 2)[some])
            check_finish(fin(parts), parts, None, None, "%s WAIC alone k = %d" % (name, k))
        # the identity, in any place, changes no bit; a lone identity is m = 0
        ident = _capi.loo_identity(6)
        got = fin([ident, whole, ident], fit64, body64)
        alone = fin([whole], fit64, body64)
        assert got["merged"].tobytes() == whole.tobytes()
        for key in _capi.LOO_POINTWISE:
            assert got[key].tobytes() == alone[key].tobytes(), key
        assert np.isnan(alone["elpd_loo"][4]) and np.isnan(alone["pareto_k"][4]) and alone["draws_used"][4] == 0
        assert np.isnan(alone["totals"]["elpd_loo"]) and np.isnan(alone["totals"]["se_elpd_waic"])
        none = fin([ident, ident])
        assert not none["draws_used"].any() and all(np.isnan(none[key]).all() for key in _capi.LOO_POINTWISE)
        # C = 1: totals are the one value, the standard errors NaN
        one = fin([whole[:, :1].copy()], fit64[:, :1].copy(), body64[:, :1].copy())
        assert one["totals"]["elpd_loo"] == one["elpd_loo"][0] and np.isnan(one["totals"]["se_elpd_loo"]) and np.isnan(one["totals"]["se_elpd_waic"])
        check_finish(one, [whole[:, :1]], fit64[:, :1], body64[:, :1], name + " C = 1")
        # m = 1: p_waic NaN; khat = inf, 0.6 and NaN columns: counted as above 0.7, between, not at all
        part = whole[:, [0, 1, 3, 5]].copy()
        part[:, 0] = [1.0, -0.5, 0.0, np.exp(-0.5), -0.5]
        f = fit64[:, [0, 1, 3, 5]].copy(); b = body64[:, [0, 1, 3, 5]].copy()
        f[0] = [np.inf, 0.6, np.nan, 0.71]
        got = fin([part], f, b)
        assert np.isnan(got["p_waic"][0]) and np.isfinite(got["lppd"][0]) and (got["k_mid"], got["k_high"]) == (1, 2)
        assert got["pareto_k"][0] == np.inf and np.isnan(got["pareto_k"][2])
        check_finish(got, [part], f, b, name + " khat")
    # every refusal of loo_plan and loo_finish in the probe (it checks that nothing was written) ...
    assert _run(exe, "refusals\n") == ["refusals -1 -1 -1 -1 -1 -1 -1 -1 -1 -1 -1 -4"]
    # ... and through the library, with sentinel-filled outputs
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    part = np.ascontiguousarray(whole[:, :2]); fit2 = np.ascontiguousarray(fit64[:, :2]); body2 = np.ascontiguousarray(body64[:, :2])
    outs = [np.full(10, -7.0)] + [np.full(2, -7.0) for _ in range(6)] + [np.full(6, -7.0)]
    ints = [np.full(2, -7, dtype=np.int64), np.full(2, -7, dtype=np.int64)]

    def raw(k, Cn, f, b, ptr=True):
        ptrs = (dp * 2)(part.ctypes.data_as(dp), part.ctypes.data_as(dp) if ptr else None)
        return hip.lib.rmhmc_loo_finish(ptrs, k, Cn, None if f is None else f.ctypes.data_as(dp), None if b is None else b.ctypes.data_as(dp),
                                        *[o.ctypes.data_as(dp) for o in outs], *[o.ctypes.data_as(lp) for o in ints])
    assert [raw(0, 2, fit2, body2), raw(2, 0, fit2, body2), raw(2, 2, fit2, body2, ptr=False), raw(2, 2, fit2, None), raw(2, 2, None, body2)] == [-1] * 5
    assert all((o == -7.0).all() for o in outs) and all((o == -7).all() for o in ints)
    assert raw(2, 2, fit2, body2) == 0 and not any((o == -7.0).any() for o in outs)
    m = np.array([100, EDGE + 1], dtype=np.int64); tl = np.full(2, -7, dtype=np.int64); rank = np.full(2, -7, dtype=np.int64)
    assert hip.lib.rmhmc_loo_plan(m.ctypes.data_as(lp), 2, tl.ctypes.data_as(lp), rank.ctypes.data_as(lp)) == -4
    assert hip.lib.rmhmc_loo_plan(m.ctypes.data_as(lp), 0, tl.ctypes.data_as(lp), rank.ctypes.data_as(lp)) == -1
    assert hip.lib.rmhmc_loo_plan(None, 2, tl.ctypes.data_as(lp), rank.ctypes.data_as(lp)) == -1
    assert (tl == -7).all() and (rank == -7).all()


def test_host_checks_and_kernel_plan_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "loo_probe")
    x = np.arange(6.0).reshape(2, 3) - 2.5

    def check(x, t):
        return _run(exe, "check 2 3\n%s\n%s\n" % (_hex(x), _hex(t)))[0]
    assert check(x, [0.0, 1.0]) == "check ok" and check(x, [-0.0, 1.0]) == "check ok"
    for v in (np.nan, np.inf, -np.inf):
        bad = x.copy(); bad[1, 2] = v
        assert "x" in check(bad, [0.0, 1.0])
    for v in (0.5, 2.0, -1.0, np.nan, 1.0 + 2 * U):
        assert "t" in check(x, [0.0, v]), v
    names = ("MAX_COLS", "MAX_TAIL", "MAX_D", "BLOCK_ROWS", "MAX_BLOCKS", "ROW_LANES", "DRAWS")
    c = dict(zip(names, (int(v) for v in _run(exe, "consts\n")[0].split()[1:])))
    assert (c["MAX_COLS"], c["MAX_TAIL"], c["MAX_D"]) == (64, 16384, 256) and c["ROW_LANES"] * c["MAX_COLS"] == 256
    Ns = sorted({1, 3, 4, 5, c["DRAWS"] - 1, c["DRAWS"], c["DRAWS"] + 1, c["BLOCK_ROWS"] - 1, c["BLOCK_ROWS"], c["BLOCK_ROWS"] + 1,
                 c["BLOCK_ROWS"] * c["MAX_BLOCKS"], c["BLOCK_ROWS"] * c["MAX_BLOCKS"] + 1, 4096000, EDGE, 2 ** 28, 2 ** 28 + 1, 2 ** 34})
    lines = _run(exe, "".join("kplan %d 64\n" % N for N in Ns))
    for N, line in zip(Ns, lines):
        lb, vb, dpv, rb, rpb, ks, cpb = (int(v) for v in line.split()[1:])
        what = (N, line)
        assert (lb - 1) * c["DRAWS"] < N <= lb * c["DRAWS"], what
        assert 1 <= vb <= c["MAX_BLOCKS"] and (vb - 1) * dpv < N <= vb * dpv, what
        assert 1 <= rb <= c["MAX_BLOCKS"] and (rb - 1) * rpb < N <= rb * rpb and rpb % c["ROW_LANES"] == 0, what
        assert rpb <= c["BLOCK_ROWS"] or rb == c["MAX_BLOCKS"] or rpb == -(-(-(-N // c["MAX_BLOCKS"])) // c["ROW_LANES"]) * c["ROW_LANES"], what
        assert ks == 16, what
        # the largest power of two <= 64 whose block of N x cols doubles stays within 2 GiB, at least 1
        assert cpb in (1, 2, 4, 8, 16, 32, 64) and (cpb == 1 or N * cpb * 8 <= 2 ** 31) and (cpb == 64 or N * cpb * 2 * 8 > 2 ** 31), what
    assert [int(l.split()[-1]) for l in _run(exe, "kplan 4096000 64\nkplan 4194304 64\nkplan 4194305 64\n")] == [64, 64, 32]


# ---- the restatement against independent facts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
def test_gpd_recovery_and_scale_freeness(k):
    """the fit on 6000 exact generalised Pareto draws (sigma = 1) by the quantile transform: within 0.05 (the sampling sd at M = 6000 is
    about (1 + k) / sqrt(M) <= 0.025); khat is unchanged to rounding when y is multiplied by 2^-600, sigma scales with y"""
    u = np.sort(np.random.RandomState(3).rand(6000)).astype(R.LD)
    y = np.expm1(-k * np.log1p(-u)) / k
    khat, sigma = R.gpd_fit(y)
    print("k = %.1f: khat %.4f, sigma %.4f" % (k, khat, sigma))
    assert abs(float(khat) - k) <= 0.05
    s = np.ldexp(R.LD(1), -600)
    khat2, sigma2 = R.gpd_fit(y * s)
    eps = float(np.finfo(R.LD).eps)
    assert abs(float(khat2 - khat)) <= 1e4 * eps and abs(float(sigma2 / s / sigma - 1)) <= 1e4 * eps
    assert R.gpd_fit(np.zeros(20, dtype=R.LD)) is None                                    # a constant tail
    assert R.gpd_fit(np.concatenate([np.zeros(10), np.ones(10)]).astype(R.LD)) is None     # mostly tied: y_q = 0


def test_no_smoothing_is_the_harmonic_mean():
    """with smoothing off, elpd_loo_c = log(m / sum_k 1 / q_k), q_k = exp(l_k): by brute force.  Also a column too short for a tail."""
    ll = _ll_case(4, 900, 3, scale=2.0)
    ll[7, 1] = np.nan
    short = _ll_case(5, 24, 3, scale=2.0)
    for case in (ll, short):
        fit, body, cols = R.columns(case, smooth=False)
        got = R.finish([R.moments(case)], fit, body)
        for c in range(3):
            v = case[:, c][np.isfinite(case[:, c])].astype(R.LD)
            brute = np.log(v.size / np.exp(-v).sum())
            assert abs(got["elpd_loo"][c] - brute) <= 1e3 * float(np.finfo(R.LD).eps) * abs(brute), c
            assert got["pareto_k"][c] == np.inf
    assert all(c["M"] == 4 and c["n_lt"] == 0 and c["n_gt"] == 24 for c in R.columns(short)[2])
    # the cutoff is the order statistic of rank M, the tail the M smallest, ties shared between tail and body
    tied = np.repeat(_ll_case(6, 100, 1, scale=2.0), 7, axis=0)      # every value seven times: 700 rows, M = 80
    col = R.column(tied[:, 0])
    srt = np.sort(tied[:, 0])
    assert col["M"] == 80 and col["cut"] == srt[80] and col["n_lt"] == 77 and col["n_gt"] == 700 - 84


def test_quadrature():
    """The D = 1 problem of tests/helpers/loo_quad.py with its fixed seed: exact posterior draws (64 x 400), the total elpd_loo against
    the exact leave-one-out value by quadrature on the same grid within 5 standard errors (from eight interleaved eighths), the outlier
    row with the largest khat, above 0.5, every other row below 0.5.  (Seeds 0 .. 3 gave differences of 0.2 to 4.9 such standard
    errors and an outlier khat of 0.65 to 0.96 when this was written; seed 3: 0.19, 0.648, next 0.165.)"""
    x, t = Q.problem()
    s = Q.exact_draws(x, t)
    assert s.shape == (Q.N_CHAINS, Q.N_DRAWS, 1) and x.shape == (Q.ROWS, 1) and x[-1, 0] == 6.0 and t[-1] == 0.0
    full = R.loo(s, x, t)
    Q.conditions(lambda w: R.loo(w, x, t)["totals"]["elpd_loo"], full["pareto_k"], s, x, t)
    # WAIC and LOO agree on the well-behaved rows (they differ at second order in the row's influence)
    assert np.abs(full["elpd_loo"][:-1] - full["elpd_waic"][:-1]).max() < 0.01
