"""CPU-side checks of the cross-chain diagnostics, include/rmhmc_diag.h: the header, the ctypes binding and the library's exports
agree; rmhmc_diag_finish (pure host code, csrc/diag.h) through the loaded library against the NumPy restatement
tests/helpers/diag_ref.py, in one piece, in ragged pieces and with an empty piece; its refusals; the AR(1) sanity of the statistic; and
csrc/diag.h once more in a stand-alone program under AddressSanitizer and UBSan (tests/helpers/diag_probe.cpp, a child process: nothing
sanitised is loaded into this one).

Tolerances are those of tests/test_gpu_out.py: mean, sum of s2, R-hat rtol 1e-12 / atol 1e-14; lag rows 1e-12 of row 4; ESS rtol 1e-9;
pairs and chains_used equal, where the reference's Geyer margin is above 1e-6."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment, multi_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import diag_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

HEADER = os.path.join(ROOT, "include", "rmhmc_diag.h")
MEAN_TOL = dict(rtol=1e-12, atol=1e-14)
ESS_RTOL = 1e-9

_cache = {}


def case():
    """one input for the finish tests: 23 chains x 37 rows x 6 dimensions, 18 lags; its partial in one piece and in ragged pieces"""
    if not _cache:
        x = R.ar1(7, 23, 37, 6)
        _cache.update(x=x, H=18, T=18, whole=R.partial(x, 18), pieces=[R.partial(x[a:b], 18) for a, b in ((0, 1), (1, 9), (9, 10), (10, 23))])
    return _cache


def check_finish(got, part, H):
    """a diag_finish result against the reference's finish of `part`"""
    ref = R.finish(part, H)
    assert (ref["margin"] > 1e-6).all(), ref["margin"]
    assert np.array_equal(got["pairs"], ref["pairs"]) and np.array_equal(got["chains_used"], ref["used"])
    assert np.allclose(got["rhat"], ref["rhat"], **MEAN_TOL) and np.allclose(got["ess_pooled"], ref["ess"], rtol=ESS_RTOL, atol=0)
    assert np.isfinite(got["rhat"]).all() and np.isfinite(got["ess_pooled"]).all()


def check_partial(got, want):
    """a partial against the reference's, row by row"""
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got[0], want[0])
    err = dict(mean=np.abs(got[1] - want[1]).max(), m2=np.abs(got[2] - want[2]).max(), s2=np.abs(got[3] / want[3] - 1).max(),
               lags=(np.abs(got[4:] - want[4:]) / want[4]).max())
    print("partial: mean %.1e (abs) M2 %.1e (abs) sum s2 %.1e (rel) lag rows %.1e (of row 4)" % tuple(err.values()))
    assert np.allclose(got[1], want[1], **MEAN_TOL) and np.allclose(got[3], want[3], **MEAN_TOL)
    # M2 is a sum of squares of differences of means, each good to MEAN_TOL: bounded by 2 sqrt(m M2) 1e-12 max|mean| + rounding
    assert (np.abs(got[2] - want[2]) <= 1e-12 * (want[2] + 2 * np.sqrt(want[0] * want[2]) * np.abs(want[1])) + 1e-14).all()
    assert (np.abs(got[4:] - want[4:]) <= 1e-12 * want[4]).all()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_binding_and_exports_agree(hip, oracle):
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert syms == {"rmhmc_diag_partial_dev", "rmhmc_diag_finish"} == set(_capi.DIAG_SIGNATURES)
    assert not syms & (set(_capi.SIGNATURES) | set(_capi.OUT_SIGNATURES))     # out of the ABI the CPU oracle has to export
    # the argument counts of the declarations and of the binding
    for name, (res, args) in _capi.DIAG_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.search(r'#include\s+"rmhmc.h"', _header()) and len(re.findall(r"#include", _header())) == 1
    assert hip.has_diag and not oracle.has_diag
    lib = C.CDLL(hip.path)
    for s in syms:
        assert hasattr(lib, s), s
    assert _capi.SUMMARY_KEYS == ("mean", "var", "ess", "run_mean", "run_ess")      # unchanged
    assert _capi.DIAG_KEYS == ("rhat", "ess_pooled", "pairs", "chains_used")


def test_finish_in_one_piece(hip):
    c = case()
    got = _capi.diag_finish([c["whole"]], c["H"], lib=hip)
    check_finish(got, c["whole"], c["H"])
    assert np.array_equal(got["merged"], c["whole"])                 # one partial merges to itself
    assert (got["chains_used"] == 46).all()


def test_finish_in_ragged_pieces(hip):
    c = case()
    got = _capi.diag_finish(c["pieces"], c["H"], lib=hip)
    check_finish(got, c["whole"], c["H"])
    check_partial(got["merged"], c["whole"])
    ref = c["pieces"][0]
    for p in c["pieces"][1:]:
        ref = R.merge(ref, p)
    assert np.allclose(got["merged"], ref, rtol=1e-14, atol=1e-14)   # the same merge, restated in NumPy
    print("merge against one piece: %.1e (rel)" % np.abs(got["merged"][1:] / c["whole"][1:] - 1).max())


def test_finish_with_an_empty_piece(hip):
    c = case()
    empty = _capi.diag_identity(c["T"], 6)
    assert np.array_equal(empty, R.partial(c["x"][:0], c["T"]))
    for parts in ([empty, c["whole"]], [c["whole"], empty], [empty, c["pieces"][0], empty, c["pieces"][1]]):
        got = _capi.diag_finish(parts, c["H"], lib=hip)
        want = _capi.diag_finish([p for p in parts if p[0].any()], c["H"], lib=hip)
        for k in got:
            assert np.array_equal(got[k], want[k]), k                # the identity, to the bit
    none = _capi.diag_finish([empty, empty], c["H"], lib=hip)
    assert np.isnan(none["rhat"]).all() and np.isnan(none["ess_pooled"]).all() and not none["pairs"].any() and not none["chains_used"].any()


def test_degenerate_dimensions(hip):
    x = R.ar1(3, 4, 20, 3)
    x[:, :, 1] = 2.5                                                 # a constant dimension: W = 0
    x[1, 3, 2] = np.nan                                              # one series of dimension 2 is left out, its other half is used
    p = R.partial(x, 10)
    got = _capi.diag_finish([p], 10, lib=hip)
    assert list(got["chains_used"]) == [8, 8, 7]
    assert np.isnan(got["rhat"][1]) and np.isnan(got["ess_pooled"][1]) and got["pairs"][1] == 0
    assert np.isfinite(got["rhat"][[0, 2]]).all()
    lone = R.partial(x[1:2], 10)                                     # one chain: m = 1 < 2 where a half is missing
    assert list(lone[0]) == [2, 2, 1]
    got = _capi.diag_finish([lone], 10, lib=hip)
    assert np.isnan(got["rhat"][2]) and np.isnan(got["ess_pooled"][2]) and np.isfinite(got["rhat"][0])


def test_refusals(hip):
    f = hip.lib.rmhmc_diag_finish
    p = np.ascontiguousarray(case()["whole"])
    ptrs = (_capi._dp * 1)(_capi._ptr(p))
    null = (_capi._dp * 1)(None)
    rhat = np.full(6, -3.0)
    ok = (ptrs, 1, 18, 18, 6)
    for args in ((ptrs, 0, 18, 18, 6), (ptrs, 1, 1, 1, 6), (ptrs, 1, 18, 1, 6), (ptrs, 1, 18, 19, 6), (ptrs, 1, 18, 18, 0), (null, 1, 18, 18, 6),
                 (None, 1, 18, 18, 6)):
        assert f(*args, None, _capi._ptr(rhat), None, None, None) == -1, args[1:]
        assert (rhat == -3.0).all()
    assert "diag_finish" in hip.lib.rmhmc_last_error(None).decode()
    assert f(*ok, None, _capi._ptr(rhat), None, None, None) == 0 and np.isfinite(rhat).all()
    assert f(*ok, None, None, None, None, None) == 0                 # every output is optional
    with pytest.raises(ValueError, match="one shape"):
        _capi.diag_finish([p, p[:-1]], 18, lib=hip)
    with pytest.raises(_capi.RmhmcError) as e:
        _capi.diag_finish([p], 17, lib=hip)                          # T = 18 > H
    assert e.value.code == -1


def test_argument_checks_need_no_gpu(oracle):
    assert _capi.diag_lags(61) == (30, 30) and _capi.diag_lags(61, 0) == (30, 30) and _capi.diag_lags(37, 5) == (18, 6)
    assert _capi.diag_lags(4) == (2, 2) and _capi.diag_lags(20000, 7) == (10000, 8)
    for S, lag in ((3, None), (20001, None), (60, 30), (60, -1)):
        with pytest.raises(ValueError):
            _capi.diag_lags(S, lag)
    X = np.random.RandomState(0).randn(12, 3); t = (X[:, 0] > 0).astype(float)
    for fn in experiment.SAMPLERS.values():
        with pytest.raises(ValueError, match="return_info"):
            fn(X, t, diagnostics=True, verbose=False)
    with pytest.raises(ValueError, match="batched=True"):
        experiment.run_experiment(X, t, "AMH", n_experiments=2, diagnostics=True)
    for kw in (dict(NumOfIterations=13, BurnIn=10), dict(max_lag=10 ** 6), dict(gather="mean")):   # before any collective: no group here
        with pytest.raises(ValueError):
            multi_gpu.sample_sharded(X, t, 4, sampler="HMC", diagnostics=True, **kw)
    with oracle.context(12, 3, 2) as ctx:                            # a library without the entry points says so
        with pytest.raises(_capi.RmhmcError, match="rmhmc_diag.h"):
            ctx.rl.need("diag")
    with pytest.raises(_capi.RmhmcError, match="rmhmc_diag.h"):
        _capi.diag_finish([np.zeros((6, 2))], 3, lib=oracle)


def test_report_prints_the_diagnostics(capsys):
    res = {"Min": 1.0, "Median": 2.0, "Mean": 2.0, "Max": 3.0, "Time": 0.5, "Time per Min ESS": 0.5}
    experiment.report(res)
    assert "R-hat" not in capsys.readouterr().out
    experiment.report(dict(res, rhat=np.array([1.01, 1.2]), ess_pooled=np.array([300.0, 40.0])))
    out = capsys.readouterr().out
    assert "Max split R-hat: 1.2" in out and "Min pooled ESS: 40.0" in out


def test_ar1_sanity(hip):
    """The statistic itself, finished by the library: n = 64 chains of S = 500, every lag, seed 0.  Pooled ESS within 15 % of the AR(1) theory
    2 n H (1 - phi) / (1 + phi) = 10667 and 1684 for phi = 0.5 and 0.9 (measured +5.8 % and -4.5 %; at phi = 0.9 and H = 250 a chain
    half holds about 13 independent draws, var+ exceeds W by 7 % and the pooled rho_t levels off near 0.07, so over seeds 0 .. 7 the
    figure scatters between -33 % and +8 % and half of them use every lag: the upper-bound case of include/rmhmc_diag.h), R-hat below
    1.05; one of 12 chains shifted by two standard deviations gives R-hat above 1.1 (1.007 -> 1.144)."""
    for phi, theory in ((0.5, 2 * 64 * 250 / 3.0), (0.9, 2 * 64 * 250 * 0.1 / 1.9)):
        part = R.partial(R.ar1(0, 64, 500, 1, phi=phi), 250)
        f = R.finish(part, 250)
        check_finish(_capi.diag_finish([part], 250, lib=hip), part, 250)
        print("phi %.1f: ess %.0f, theory %.0f (%+.1f %%), rhat %.4f, pairs %d" % (phi, f["ess"][0], theory, 100 * (f["ess"][0] / theory - 1),
                                                                                 f["rhat"][0], f["pairs"][0]))
        assert abs(f["ess"][0] / theory - 1) < 0.15 and f["rhat"][0] < 1.05
    x = R.ar1(2, 12, 500, 1, phi=0.5)
    before = R.finish(R.partial(x, 250), 250)
    x[3] += 2 * np.sqrt(1 / 0.75)
    part = R.partial(x, 250)
    after = R.finish(part, 250)
    got = _capi.diag_finish([part], 250, lib=hip)
    assert got["pairs"][0] == after["pairs"][0] == 125 and 2 * got["pairs"][0] + 1 >= 250      # every lag used: the ESS is an upper bound
    assert np.allclose(got["rhat"], after["rhat"], **MEAN_TOL)
    print("rhat %.4f -> %.4f, pairs %d -> %d of 125" % (before["rhat"][0], after["rhat"][0], before["pairs"][0], after["pairs"][0]))
    assert before["rhat"][0] < 1.05 and after["rhat"][0] > 1.1


# ---- csrc/diag.h in a stand-alone program under AddressSanitizer and UBSan ---------------------------------------------------------------
def _probe(exe, parts, H, T, P, tiles=()):
    text = "%d %d %d %d\n" % (len(parts), H, T, P) + "\n".join(" ".join(float(v).hex() for v in np.ravel(p)) for p in parts) + "\n"
    text += "".join("%d %d\n" % hp for hp in tiles)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    rc = int(lines[0].split()[1])
    out = dict(rc=rc, tiles=[tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("tile")])
    if rc == 0:
        fl = [np.array([float.fromhex(v) for v in ln.split()]) for ln in lines[1:4]]
        out.update(merged=fl[0].reshape(4 + T, P), rhat=fl[1], ess_pooled=fl[2], pairs=np.array(lines[4].split(), dtype=np.int64),
                   chains_used=np.array(lines[5].split(), dtype=np.int64))
    return out


def test_diag_header_under_sanitizers(hip, tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "diag_probe")
    c = case()
    empty = _capi.diag_identity(c["T"], 6)
    for parts in ([c["whole"]], c["pieces"], [empty] + c["pieces"] + [empty]):
        got = _probe(exe, parts, c["H"], c["T"], 6)
        assert got["rc"] == 0
        check_finish(got, c["whole"], c["H"])
        lib = _capi.diag_finish(parts, c["H"], lib=hip)              # the library runs the same header
        assert np.allclose(got["merged"], lib["merged"], rtol=1e-14, atol=1e-14) and np.array_equal(got["pairs"], lib["pairs"])
    x = R.ar1(3, 4, 20, 3); x[:, :, 1] = 2.5; x[1, 3, 2] = np.nan
    got = _probe(exe, [R.partial(x, 10)], 10, 10, 3)
    assert np.isnan(got["rhat"][1]) and np.isnan(got["ess_pooled"][1]) and list(got["chains_used"]) == [8, 8, 7]
    for parts, H, T, P in (([], 18, 18, 6), ([c["whole"]], 18, 19, 6), ([c["whole"]], 1, 1, 6), ([c["whole"]], 18, 1, 6)):
        assert _probe(exe, parts if T == 18 else [np.zeros((4 + T, P))], H, T, P)["rc"] == -1


def test_tile_shapes(tmp_path_factory):
    """the tile k_diag_acov works on, asked of csrc/diag.h: width, LDS rows, LDS bytes, lags per workgroup.  By hand: rows =
    (ceil(H / 16) 16 + 32) 17 / 16; bytes = (rows width + 256) 8 + 1024; width the largest power of two <= 64 that P needs, halved
    while the bytes exceed 81920 (two workgroups per CU), and the bytes never above 163840; lags = 256 / width x 16 per set."""
    want = {(250, 64): (32, 306, 81408, 128), (250, 5): (8, 306, 22656, 512), (2, 1): (1, 51, 3480, 4096), (18, 33): (64, 68, 37888, 64),
            (30, 65): (64, 68, 37888, 64), (10000, 2): (1, 10659, 88344, 4096), (10000, 64): (1, 10659, 88344, 4096),
            (300, 64): (16, 357, 48768, 256), (251, 64): (32, 306, 81408, 128), (257, 64): (16, 323, 44416, 256), (5000, 3): (1, 5355, 45912, 4096)}
    got = _probe(probe_exe(tmp_path_factory, "diag_probe"), [np.zeros((6, 1))], 2, 2, 1, tiles=list(want))["tiles"]
    assert {g[:2]: g[2:] for g in got} == want
