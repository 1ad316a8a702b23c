"""CPU-side checks of the posterior predictive probabilities, include/rmhmc_pred.h: the header, the ctypes binding and the library's
exports agree; csrc/pred.h (merge and finish of partials, the host checks, the plan of the kernels) in a stand-alone program under
AddressSanitizer and UBSan (tests/helpers/pred_probe.cpp, a child process: nothing sanitised is loaded into this one) against the
np.longdouble restatement tests/helpers/pred_ref.py; the restatement itself against a brute-force formula; the shim's argument checks.

Bounds of the finish (u = 2^-53; the probe finishes in doubles the same double partials the restatement finishes in long doubles, whose
own error of 2^-64 per operation is nothing).  A merge of k partials adds k - 1 times, one rounding each, so a merged sum is off by a
relative (k - 1) u.  prob = S1 / m: one more rounding, |prob - ref| <= k u ref.  pvar = S2 / m - prob^2: S2 / m <= 1 and prob <= 1 are
each off by at most k u / 2 absolute (a number in [1/2, 1) rounds to u / 2), the square by 2 * k u / 2 + u / 2, the difference, at most
1/4, by u / 8: (3 k / 2 + 5 / 8) u, inside the 4 u of the header for k = 1; the test allows (3 k + 1) u.  lpd = log(SQ / m): the
quotient carries a relative k u, which is an absolute k u in the logarithm, and log itself is good to 1 ulp = 2 u |ref|:
|lpd - ref| <= k u + 2 u |ref|, allowed as (k + 1) u + 2 u max(1, |ref|).  lpd_total adds R numbers in row order: the sum of the rows'
allowances plus R u sum |lpd|."""
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
import pred_ref as P  # noqa: E402
from probe_build import probe_exe  # noqa: E402

SYMBOLS = {"rmhmc_pred_partial_dev", "rmhmc_pred_finish"}
U = 2.0 ** -53


def _header():
    return open(os.path.join(ROOT, "include", "rmhmc_pred.h")).read()


# ---- the header, the binding, the exports -----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", code))
    assert syms == SYMBOLS == set(_capi.PRED_SIGNATURES)
    others = [v for k, v in vars(_capi).items() if k.endswith("SIGNATURES") and k != "PRED_SIGNATURES"]
    assert len(others) >= 9
    for other in others:
        assert not syms & set(other)
    for name, (res, args) in _capi.PRED_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc.h"]
    assert pkg.posterior_predictive is pkg.predict.posterior_predictive and "posterior_predictive" in pkg.__all__
    # the constants of the binding and of the host half
    hdr = open(os.path.join(ROOT, "riemannhamiltonianmontecarlo_amd", "csrc", "pred.h")).read()
    assert int(re.search(r"#define\s+PRED_MAX_D\s+(\d+)", hdr).group(1)) == _capi.PRED_MAX_D == 256


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_pred and not oracle.has_pred
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with oracle.context(10, 2, 1) as ctx:           # a library without the calls says so, with the header's name
        calls = (lambda: ctx.predict_partial(None, None), lambda: ctx.predict_partial(None, None, None), lambda: ctx.predict(None, None),
                 lambda: _capi.pred_finish([np.zeros((4, 3))], lib=oracle))
        for call in calls:
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_pred.h" in str(e.value)
    assert _capi.pred_identity(3).shape == (4, 3) and not _capi.pred_identity(3).any()


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
    Xn, tn = XX[:4], t[:4]
    nan_x = Xn.copy(); nan_x[1, 2] = np.nan
    inf_x = Xn.copy(); inf_x[0, 0] = np.inf
    bad = [dict(XX=XX[0]), dict(t=t[:-1]), dict(Xnew=Xn[0]), dict(Xnew=Xn[:, :2]), dict(Xnew=Xn[:0]), dict(Xnew=nan_x), dict(Xnew=inf_x),
           dict(tnew=tn[:-1]), dict(tnew=np.array([0.0, 1.0, 0.5, 1.0])), dict(tnew=np.array([0.0, 1.0, np.nan, 1.0])),
           dict(tnew=np.array([0.0, 1.0, 2.0, 1.0])), dict(n_chains=0), dict(n_chains=2.5), dict(NumOfIterations=10, BurnIn=10),
           dict(BurnIn=-1), dict(NumOfIterations=2.5), dict(NumOfLeapFrogSteps=0), dict(StepSize=0.0), dict(StepSize=np.nan),
           dict(alpha=0.0), dict(alpha=np.inf)]
    for kw in bad:
        args = dict(XX=XX, t=t, Xnew=Xn, tnew=tn, n_chains=8, _lib=_NoLibrary())
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.posterior_predictive(**args)
    wide = np.zeros((5, 257))
    with pytest.raises(ValueError):
        pkg.posterior_predictive(wide, np.zeros(5), wide[:2], _lib=_NoLibrary())


# ---- csrc/pred.h in a stand-alone program under AddressSanitizer and UBSan -----------------------------------------------------------------
def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _floats(line):
    return np.array([float.fromhex(v) if "x" in v else float(v) for v in line.split()])


def _hex(a):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.ravel(a))


def _finish(exe, parts):
    R = np.asarray(parts[0]).shape[1]
    lines = _run(exe, "finish %d %d\n" % (len(parts), R) + "\n".join(_hex(p) for p in parts) + "\n")
    head = lines[0].split()
    assert head[0] == "finish" and int(head[1]) == 0
    return dict(draws_used=int(head[2]), merged=_floats(lines[1]).reshape(4, R), prob=_floats(lines[2]), pvar=_floats(lines[3]),
                lpd=_floats(lines[4]), lpd_total=float(_floats(lines[5])[0]))


def check_finish(got, parts, what=""):
    """a finished result of the probe (doubles) against the restatement's finish of the same double partials in long doubles, to the
    bounds of the module's docstring"""
    k = len(parts)
    want = P.finish([np.asarray(p, dtype=P.LD) for p in parts])
    assert got["draws_used"] == want["draws_used"], what
    assert np.array_equal(got["merged"][0], np.asarray(want["merged"][0], dtype=np.float64)), what
    for row in (1, 2, 3):
        g, w = got["merged"][row].astype(P.LD), want["merged"][row]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, row)
        fin = ~np.isnan(w)
        assert np.all(np.abs(g[fin] - w[fin]) <= k * U * np.abs(w[fin])), (what, row)
    for key in ("prob", "pvar", "lpd"):
        g, w = got[key], np.asarray(want[key])
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, key, g, w)
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf].astype(np.float64)), (what, key)
    ok = np.isfinite(np.asarray(want["prob"], dtype=np.float64))
    assert np.all(np.abs(got["prob"][ok] - want["prob"][ok]) <= k * U * want["prob"][ok]), what
    assert np.all(np.abs(got["pvar"][ok] - want["pvar"][ok]) <= (3 * k + 1) * U), what
    assert np.all(got["pvar"][ok] >= 0.0), what
    fin = np.isfinite(np.asarray(want["lpd"], dtype=np.float64))
    tol = (k + 1) * U + 2 * U * np.maximum(1.0, np.abs(want["lpd"][fin].astype(np.float64)))
    assert np.all(np.abs(got["lpd"][fin] - want["lpd"][fin]) <= tol), what
    wt = want["lpd_total"]
    if np.isfinite(wt):
        R = len(got["lpd"])
        assert abs(got["lpd_total"] - wt) <= tol.sum() + R * U * np.abs(want["lpd"]).sum(), what
    else:
        assert (np.isnan(got["lpd_total"]) and np.isnan(wt)) or got["lpd_total"] == wt, what


def _case(seed, n, S, D, R, scale=1.0):
    rs = np.random.RandomState(seed)
    w = rs.randn(n, S, D) * scale
    x = rs.randn(R, D)
    t = (rs.rand(R) < 0.5).astype(np.float64)
    return w, x, t


def test_merge_and_finish_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "pred_probe")
    w, x, t = _case(0, 6, 11, 5, 9, scale=4.0)
    w[2, 3, 1] = np.nan                                    # an invalid draw: left out of m
    whole = P.partial(w, x, t).astype(np.float64)
    assert whole[0, 0] == 65
    for cuts in ([0, 6], [0, 2, 6], [0, 1, 4, 6]):         # k = 1, 2, 3 partials
        parts = [P.partial(w[a:b], x, t).astype(np.float64) for a, b in zip(cuts[:-1], cuts[1:])]
        got = _finish(exe, parts)
        check_finish(got, parts, "k = %d" % len(parts))
        # ... and against the partial of all draws at once: every row of a piece carries the half-ulp of its conversion to double
        k = len(parts)
        for row in (1, 2, 3):
            assert np.all(np.abs(got["merged"][row] - whole[row]) <= (2 * k + 1) * U * whole[row])
        assert np.array_equal(got["merged"][0], whole[0])
    # the identity partial, in any place, changes no bit; a lone identity is m = 0
    ident = _capi.pred_identity(9)
    got = _finish(exe, [ident, whole, ident])
    assert got["merged"].tobytes() == whole.tobytes()
    alone = _finish(exe, [whole])
    for key in ("prob", "pvar", "lpd"):
        assert got[key].tobytes() == alone[key].tobytes()
    none = _finish(exe, [ident, ident])
    assert none["draws_used"] == 0 and np.isnan(none["lpd_total"])
    for key in ("prob", "pvar", "lpd"):
        assert np.isnan(none[key]).all()
    check_finish(none, [ident, ident], "m = 0")
    # m = 0 from draws that are all invalid
    dead = P.partial(np.full((2, 3, 5), np.nan), x, t).astype(np.float64)
    assert _finish(exe, [dead])["draws_used"] == 0 and np.isnan(_finish(exe, [dead])["prob"]).all()
    # SQ = 0: every likelihood underflowed, lpd = -inf, and the total with it
    part = whole.copy()
    part[3, 4] = 0.0
    got = _finish(exe, [part])
    assert got["lpd"][4] == -np.inf and np.isfinite(np.delete(got["lpd"], 4)).all() and got["lpd_total"] == -np.inf
    check_finish(got, [part], "SQ = 0")
    # a NaN row (an f that was NaN) stays NaN and leaves its neighbours alone
    part = whole.copy()
    part[1:, 2] = np.nan
    got = _finish(exe, [part])
    assert np.isnan([got["prob"][2], got["pvar"][2], got["lpd"][2], got["lpd_total"]]).all()
    assert np.isfinite(np.delete(got["prob"], 2)).all()
    check_finish(got, [part], "NaN row")
    # no labels: row 3 is -0.0, lpd NaN, the rest as with labels
    nolab = P.partial(w, x, None).astype(np.float64)
    assert not nolab[3].any() and np.signbit(nolab[3]).all() and np.array_equal(nolab[:3], whole[:3])
    got = _finish(exe, [nolab])
    assert np.isnan(got["lpd"]).all() and np.isnan(got["lpd_total"])
    assert got["prob"].tobytes() == alone["prob"].tobytes() and got["pvar"].tobytes() == alone["pvar"].tobytes()
    halves = [P.partial(w[:3], x, None).astype(np.float64), P.partial(w[3:], x, None).astype(np.float64)]
    got = _finish(exe, halves)
    assert np.isnan(got["lpd"]).all() and np.signbit(got["merged"][3]).all()
    check_finish(got, halves, "no labels, merged")
    # pvar is never negative: every p equal
    same = np.zeros((4, 3))
    same[0] = 7.0; same[1] = 7.0 * 0.3; same[2] = 7.0 * (0.3 * 0.3) * (1 - 2 * U); same[3] = 7.0 * 0.3
    assert np.all(_finish(exe, [same])["pvar"] == 0.0)
    # every refusal: k < 1, R < 1, a NULL partial, a NULL list (the probe checks that nothing was written)
    assert _run(exe, "refusals\n") == ["refusals -1 -1 -1 -1"]


def test_host_checks_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "pred_probe")
    x = np.arange(6.0).reshape(2, 3) - 2.5

    def check(x, t):
        return _run(exe, "check 2 3 %d\n%s\n%s\n" % (t is not None, _hex(x), "" if t is None else _hex(t)))[0]
    assert check(x, None) == "check ok" and check(x, [0.0, 1.0]) == "check ok" and check(x, [1.0, 1.0]) == "check ok"
    assert check(x, [-0.0, 1.0]) == "check ok"                # -0.0 == 0.0
    for v in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0), (1, 2)):
            bad = x.copy(); bad[pos] = v
            assert "xnew" in check(bad, [0.0, 1.0])
    for v in (0.5, 2.0, -1.0, np.nan, np.inf, 1.0 + 2 * U, 5e-324):
        for pos in (0, 1):
            t = [0.0, 1.0]; t[pos] = v
            assert "tnew" in check(x, t), v


def _consts(exe):
    names = ("ROW_TILE", "WAVE_ROWS", "DRAWS", "MAX_BLOCKS", "SCRATCH_BYTES", "MAX_D")
    line = _run(exe, "consts\n")[0].split()
    assert line[0] == "consts"
    return dict(zip(names, (int(v) for v in line[1:])))


PLAN_KEYS = ("row_tiles", "nblocks", "draws_per_block", "vblocks", "draws_per_vblock", "ksteps", "rec_doubles", "cnt_doubles", "x_doubles",
             "valid_bytes", "scratch_bytes")


def plans(exe, shapes):
    lines = _run(exe, "".join("plan %d %d %d\n" % s for s in shapes))
    return [dict(zip(PLAN_KEYS, (int(v) for v in line.split()[1:]))) for line in lines]


def test_plan_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "pred_probe")
    c = _consts(exe)
    assert c["ROW_TILE"] % c["WAVE_ROWS"] == 0 and c["WAVE_ROWS"] == 16 and c["DRAWS"] % 16 == 0 and c["MAX_D"] == 256
    # by hand, from the rules in pred.h
    want = {(1, 1, 1): (1, 1, 16, 1, 1, 4), (256, 1, 5): (1, 1, 256, 1, 256, 4), (257, 17, 64): (1, 2, 144, 2, 129, 16),
            (515, 65, 65): (2, 3, 176, 3, 172, 24), (4096000, 10000, 64): (157, 278, 14736, 1024, 4000, 16), (300, 33, 256): (1, 2, 160, 2, 150, 64)}
    for shape, p in zip(want, plans(exe, list(want))):
        assert tuple(p[k] for k in PLAN_KEYS[:6]) == want[shape], (shape, p)
    # the edges of the plan itself: the smallest block, the block limit, the row tile, the R from which the scratch bound cuts the blocks
    tile, draws, maxb = c["ROW_TILE"], c["DRAWS"], c["MAX_BLOCKS"]
    r_cut = c["SCRATCH_BYTES"] // (maxb * 3 * tile * 8) * tile          # the last R with all MAX_BLOCKS blocks
    Ns = sorted({1, 15, 16, 17, draws - 1, draws, draws + 1, 2 * draws, 2 * draws + 3, draws * maxb - 1, draws * maxb, draws * maxb + 1,
                 16 * draws * maxb + 5, 4096000})
    Rs = sorted({1, 15, 16, 17, 33, tile - 1, tile, tile + 1, 2 * tile + 1, r_cut - 1, r_cut, r_cut + 1, r_cut + tile + 1, 10000, 1000000})
    shapes = [(N, R, D) for N in Ns for R in Rs for D in (1, 64)]
    for (N, R, D), p in zip(shapes, plans(exe, shapes)):
        what = (N, R, D, p)
        # the blocks cover 0 .. N exactly once: block b is [b dpb, min((b + 1) dpb, N)), none empty; likewise the tiles and 0 .. R
        for nb, per in ((p["nblocks"], p["draws_per_block"]), (p["vblocks"], p["draws_per_vblock"])):
            assert 1 <= nb <= maxb and (nb - 1) * per < N <= nb * per, what
        assert p["draws_per_block"] % 16 == 0, what
        # blocks of at most PRED_DRAWS draws, unless that would take more blocks than the block limit or the scratch bound allows
        limit = min(maxb, max(1, c["SCRATCH_BYTES"] // (p["row_tiles"] * 3 * tile * 8)))
        assert p["draws_per_block"] <= draws or p["draws_per_block"] == ((N + limit - 1) // limit + 15) // 16 * 16, what
        assert p["draws_per_vblock"] <= draws or p["draws_per_vblock"] == (N + maxb - 1) // maxb, what
        assert (p["row_tiles"] - 1) * tile < R <= p["row_tiles"] * tile, what
        # the scratch size matches, and the records keep to their bound (one block's records are the least there can be)
        assert p["rec_doubles"] == p["row_tiles"] * p["nblocks"] * 3 * tile, what
        assert 8 * p["rec_doubles"] <= max(c["SCRATCH_BYTES"], 8 * p["row_tiles"] * 3 * tile), what
        assert p["cnt_doubles"] == p["vblocks"] and p["x_doubles"] == R * D + R, what
        assert N <= p["valid_bytes"] < N + 8 and p["valid_bytes"] % 8 == 0, what
        assert p["scratch_bytes"] == 8 * (p["rec_doubles"] + p["cnt_doubles"] + p["x_doubles"]) + p["valid_bytes"], what
    # as many blocks as the bounds allow: with few rows the block limit, with many the scratch bound
    full = plans(exe, [(draws * maxb, r_cut, 8), (draws * maxb, r_cut + 1, 8)])
    assert full[0]["nblocks"] == maxb and full[1]["nblocks"] < maxb
    # the steps: 4 up to D = 16, then the next multiple of 8 that holds ceil(D / 4)
    for D, p in zip(range(1, 257), plans(exe, [(1, 1, D) for D in range(1, 257)])):
        need = (D + 3) // 4
        assert p["ksteps"] == (4 if D <= 16 else (need + 7) // 8 * 8) and p["ksteps"] >= need, D


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_against_brute_force():
    """log(mean(exp(t f - logaddexp(0, f)))) in long doubles on a 5 x 7 x 3 case (5 rows, 7 draws, D = 3): exp(t f) / (1 + exp(f)) is the
    likelihood of t under f, written without the header's case distinction"""
    rs = np.random.RandomState(11)
    w = rs.randn(7, 1, 3) * 3.0
    x = rs.randn(5, 3)
    t = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    f = (x.astype(P.LD)[:, None, :] * w.reshape(7, 3).astype(P.LD)[None]).sum(axis=2)
    assert np.abs(f).max() > 5.0
    brute_lpd = np.log(np.exp(t[:, None] * f - np.logaddexp(P.LD(0), f)).mean(axis=1))
    p = 1 / (1 + np.exp(-f))
    got = P.predict(w, x, t)
    eps = np.finfo(P.LD).eps
    assert got["draws_used"] == 7
    assert np.all(np.abs(got["lpd"] - brute_lpd) <= 64 * eps * np.maximum(1, np.abs(brute_lpd)))
    assert np.all(np.abs(got["prob"] - p.mean(axis=1)) <= 64 * eps)
    assert np.all(np.abs(got["pvar"] - p.var(axis=1)) <= 64 * eps)
    assert abs(got["lpd_total"] - brute_lpd.sum()) <= 64 * eps * np.abs(brute_lpd).sum()
    # the complement is not a subtraction: at f = 60, 1 - p = e^-60 / (1 + e^-60) to full relative accuracy, and at -700 p itself;
    # at -800 it is below every double and has underflowed: 0
    _, p1, q1 = P.probabilities(np.array([[60.0], [-700.0], [700.0], [-800.0]]), np.array([[1.0]]))
    assert abs(q1[0, 0] / (np.exp(P.LD(-60)) / (1 + np.exp(P.LD(-60)))) - 1) <= 4 * eps and abs(q1[0, 0] / 8.75651076269652e-27 - 1) < 1e-14
    assert abs(p1[0, 1] / np.exp(P.LD(-700)) - 1) <= 4 * eps and q1[0, 1] == 1 and p1[0, 2] == 1 and q1[0, 2] == p1[0, 1]
    assert p1[0, 3] == 0 and q1[0, 3] == 1
    # invalid draws leave, whatever the entry
    bad = np.concatenate([w, np.array([np.nan, 0, 0, 0, np.inf, 0, 0, 0, -np.inf]).reshape(3, 1, 3)])
    again = P.predict(bad, x, t)
    assert again["draws_used"] == 7 and np.array_equal(again["prob"], got["prob"]) and np.array_equal(again["lpd"], got["lpd"])
    assert np.isnan(P.predict(bad[7:], x, t)["prob"]).all() and P.predict(bad[7:], x, t)["draws_used"] == 0
