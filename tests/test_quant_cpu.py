"""CPU-side checks of the posterior quantiles, include/rmhmc_quant.h: the header, the ctypes binding and the library's exports agree;
the host calls (rmhmc_quant_plan, rmhmc_quant_step, rmhmc_quant_finish: csrc/quant.h) through the loaded library and once more in a
stand-alone program under AddressSanitizer and UBSan (tests/helpers/quant_probe.cpp, a child process: nothing sanitised is loaded into
this one), both against the NumPy restatement tests/helpers/quant_ref.py and against np.sort; the shim's argument checks.

Everything is compared bit for bit: the order statistics with np.sort, the interpolated values with the exact rational value of
g (hi - lo) + lo rounded once.  np.quantile uses another (two-rounding) interpolation: within 2 ulp of the larger of |lo| and |hi|."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, multi_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import diag_ref  # noqa: E402
import quant_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

HEADER = os.path.join(ROOT, "include", "rmhmc_quant.h")
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
DBL_MAX, TINY = np.finfo(np.float64).max, 5e-324
EDGE_VALUES = [0.0, -0.0, TINY, -TINY, 2 * TINY, -2 * TINY, 2.2250738585072014e-308, -2.2250738585072014e-308, 2.225073858507201e-308,
               DBL_MAX, -DBL_MAX, np.nextafter(DBL_MAX, 0), np.nextafter(-DBL_MAX, 0), 1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0), -1.0,
               np.nextafter(-1.0, 0), np.nextafter(-1.0, -2), 3.5, -3.5, 1e-300, -1e300]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_binding_and_exports_agree(hip, oracle):
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert syms == set(_capi.QUANT_SIGNATURES) == {"rmhmc_quant_hist_dev", "rmhmc_quant_plan", "rmhmc_quant_step", "rmhmc_quant_finish",
                                                   "rmhmc_quant_dev"}
    assert not syms & (set(_capi.SIGNATURES) | set(_capi.OUT_SIGNATURES))     # out of the ABI the CPU oracle has to export
    for name, (res, args) in _capi.QUANT_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.search(r'#include\s+"rmhmc.h"', _header()) and len(re.findall(r"#include", _header())) == 1
    assert hip.has_quant and not oracle.has_quant
    lib = C.CDLL(hip.path)
    for s in syms:
        assert hasattr(lib, s), s
    assert _capi.FEATURES["quant"] == (_capi.QUANT_SIGNATURES, "the posterior quantiles (include/rmhmc_quant.h)")
    hdr = open(HEADER).read()
    assert "RMHMC_QUANT_MAX_K %d " % _capi.QUANT_MAX_K in hdr and "RMHMC_QUANT_MAX_Q %d " % _capi.QUANT_MAX_Q in hdr
    src = open(os.path.join(ROOT, "riemannhamiltonianmontecarlo_amd", "csrc", "quant.h")).read()
    for name, v in (("QUANT_THREADS", _capi.QUANT_THREADS), ("QUANT_KEYS", _capi.QUANT_KEYS), ("QUANT_MAX_TILE", _capi.QUANT_MAX_TILE),
                    ("QUANT_BINS", _capi.QUANT_BINS), ("QUANT_MAX_K", _capi.QUANT_MAX_K), ("QUANT_MAX_Q", _capi.QUANT_MAX_Q)):
        assert re.search(r"#define %s %d\b" % (name, v), src), name
    assert _capi.quant_tile(1) == (1, 16384) and _capi.quant_tile(15) == (16, 1024) and _capi.quant_tile(33) == (64, 256)
    assert _capi.quant_tile(64) == _capi.quant_tile(65) == (64, 256)


def test_a_library_without_the_feature_says_so(oracle):
    with pytest.raises(_capi.RmhmcError, match="rmhmc_quant.h") as e:
        oracle.need("quant")
    assert e.value.code == -4
    with oracle.context(12, 3, 2) as ctx:
        for call in (lambda: ctx.quant_hist(None, 0), lambda: ctx.quantiles(None, 0.5)):
            with pytest.raises(_capi.RmhmcError, match="rmhmc_quant.h"):
                call()
    m = np.array([5], dtype=np.int64)
    for call in (lambda: _capi.quant_plan(m, 0.5, lib=oracle),
                 lambda: _capi.quant_step([np.zeros((1, 1, 256))], 0, np.zeros((2, 1), np.uint64), np.zeros((2, 1), np.int64), lib=oracle),
                 lambda: _capi.quant_finish(np.zeros((2, 1), np.uint64), np.zeros((1, 1)), m, lib=oracle)):
        with pytest.raises(_capi.RmhmcError, match="rmhmc_quant.h"):
            call()


def test_shim_argument_checks_need_no_library(oracle):
    for bad in ((), (0.5, 1.5), -0.1, np.nan, ((0.1, 0.2),)):
        with pytest.raises(ValueError, match="probabilities"):
            _capi.quant_probs(bad)
    assert np.array_equal(_capi.quant_probs(0.5), [0.5]) and _capi.quant_probs(range(2)).dtype == np.float64
    assert _capi.quant_identity(3, 5).shape == (3, 5, 256) and not _capi.quant_identity(3, 5).any()
    X = np.random.RandomState(0).randn(12, 3); t = (X[:, 0] > 0).astype(float)
    for kw in (dict(quantiles=1.5), dict(quantiles=()), dict(quantiles=0.5, gather="mean")):          # before any collective: no group here
        with pytest.raises(ValueError):
            multi_gpu.sample_sharded(X, t, 4, sampler="HMC", **kw)
    with oracle.context(12, 3, 2) as ctx:                            # a bad probability is refused before the library is asked anything
        with pytest.raises(ValueError, match="probabilities"):
            ctx.sample_to("rmhmc", 20, 10, quantiles=2.0)
    p = np.zeros((2, 3), dtype=np.uint64); r = np.zeros((2, 3), dtype=np.int64)
    for pre, rank in ((p.astype(np.int64), r), (p, r[:1]), (p[:, ::2], r[:, ::2]), (list(p), r)):
        with pytest.raises(ValueError, match="quant_step"):
            _capi.quant_step([np.zeros((1, 3, 256))], 0, pre, rank, lib=oracle)


# ---- the host calls through the library -------------------------------------------------------------------------------------------------
def _data():
    x = R.edge_data(5, 700, 9)
    x[:, 7] = diag_ref.ar1(3, 1, 700, 1)[0, :, 0]
    return x


def test_plan_against_the_restatement(hip):
    m = np.array([0, 1, 2, 3, 5, 101, 700, 2 ** 40 + 1], dtype=np.int64)
    probs = (0.0, 1.0, 0.5, 0.25, 0.975, 1 / 3)                      # (m - 1) q is an integer for q = 0, 1 and e.g. m = 5, q = 0.25, 0.5
    rank, frac = _capi.quant_plan(m, probs, lib=hip)
    want_rank, want_frac = R.plan(m, probs)
    assert np.array_equal(rank, want_rank) and R.same_bits(frac, want_frac)
    assert (rank[:, 0] == -1).all() and not rank[:, 1].any() and list(rank[:4, 2]) == [0, 1, 1, 1]
    assert rank[6, 4] == 1 and rank[7, 4] == 2 and frac[3, 4] == 0.0  # m = 5, q = 0.25: h = 1 exactly, and hi is lo + 1 all the same
    assert (rank[1::2] <= np.maximum(m - 1, -1)).all() and (rank[1::2] - rank[::2] <= 1).all()
    for j, q in enumerate(probs):                                    # numpy's virtual index
        for d in range(1, 7):
            assert rank[2 * j, d] + frac[j, d] == (m[d] - 1) * q
    out = np.full((2, 1), -5, dtype=np.int64); fr = np.full((1, 1), -5.0)
    f = hip.lib.rmhmc_quant_plan
    one = np.array([3], dtype=np.int64)
    for mm, pp, Q, P in ((one, [1.5], 1, 1), (one, [np.nan], 1, 1), (one, [-0.0001], 1, 1), (one, [0.5] * 9, 9, 1), (one, [0.5], 0, 1),
                         (one, [0.5], 1, 0), (np.array([-1], dtype=np.int64), [0.5], 1, 1)):
        pp = np.array(pp)
        assert f(_capi._ptr(mm, _capi._lp), _capi._ptr(pp), Q, P, _capi._ptr(out, _capi._lp), _capi._ptr(fr)) == -1
        assert (out == -5).all() and (fr == -5.0).all()
    assert "quant_plan" in hip.lib.rmhmc_last_error(None).decode()
    assert f(None, _capi._ptr(fr), 1, 1, _capi._ptr(out, _capi._lp), _capi._ptr(fr)) == -1


def _library_select(hip, x, probs, splits):
    def hist(r, prefix, K):
        return [R.hist(x[a:b], r, prefix) for a, b in splits]
    return _capi.quant_select(hist, probs, x.shape[1], lib=hip)


@pytest.mark.parametrize("splits", [[(0, 700)], [(0, 300), (300, 700)], [(0, 1), (1, 1), (1, 250), (250, 699), (699, 700)]],
                         ids=["one", "two", "five_with_an_empty_one"])
def test_select_is_np_sort_for_any_split(hip, splits):
    x = _data()
    got = _library_select(hip, x, PROBS, splits)
    order, quant, m = R.sorted_stats(x, PROBS)
    ref = R.select(x, PROBS, splits)
    assert np.array_equal(got["draws_used"], m) and m[5] == 0 and m[4] < 700 and (m[[0, 1, 2, 3, 6, 7, 8]] == 700).all()
    assert R.same_bits(ref["order"][:, m > 0], order[:, m > 0])      # the restatement finds np.sort's values ...
    assert R.same_bits(got["quantiles"], quant) and R.same_bits(got["quantiles"], ref["quantiles"])      # ... and the library its quantiles
    assert np.isnan(got["quantiles"][:, 5]).all() and (got["quantiles"][:, 0] == -3.75).all()
    with np.errstate(invalid="ignore"):
        npq = np.array([[np.quantile(x[np.isfinite(x[:, d]), d], q) if m[d] else np.nan for d in range(9)] for q in PROBS])
    ulp = np.spacing(np.maximum(np.abs(order[::2]), np.abs(order[1::2])))
    ok = m > 0
    assert (np.abs(got["quantiles"] - npq)[:, ok] <= 2 * ulp[:, ok]).all()


def test_more_than_eight_probabilities_run_in_groups(hip):
    x = _data()[:, [6, 7]]
    probs = np.linspace(0, 1, 11)
    got = _library_select(hip, x, probs, [(0, 700)])
    assert got["quantiles"].shape == (11, 2) and R.same_bits(got["quantiles"], R.sorted_stats(x, probs)[1])
    assert (got["quantiles"][0] == x.min(0)).all() and (got["quantiles"][10] == x.max(0)).all()


def test_step_refuses_a_histogram_that_is_not_its_own(hip):
    x = _data()[:, [6, 7, 5]]
    m = np.isfinite(x).sum(0)
    rank, _ = _capi.quant_plan(m, (0.25, 0.5), lib=hip)
    prefix = np.zeros(rank.shape, dtype=np.uint64)
    h0 = R.hist(x, 0)
    for bad in (R.hist(x[:50], 0), h0 * 0, h0 + 0.5, -h0):               # too few values for the rank; no counts
        p, r = prefix.copy(), rank.copy()
        with pytest.raises(_capi.RmhmcError) as e:
            _capi.quant_step([bad], 0, p, r, lib=hip)
        assert e.value.code == -1 and "quant_step" in str(e.value) and np.array_equal(p, prefix) and np.array_equal(r, rank)
    _capi.quant_step([h0], 0, prefix, rank, lib=hip)
    assert (rank[:, 2] == -1).all() and not prefix[:, 2].any()        # m = 0: carried through
    h1 = R.hist(x, 1, prefix)
    other = R.hist(x[:650], 1, prefix)                                  # partials of other samples: fewer values in the chosen bin
    skipped = R.hist(x, 2, prefix)                                      # a skipped round
    for r_, bad in ((1, other), (2, skipped), (1, h1 * 2), (1, h0)):
        p, r = prefix.copy(), rank.copy()
        with pytest.raises((_capi.RmhmcError, ValueError)):
            _capi.quant_step([bad], r_, p, r, lib=hip)
        assert np.array_equal(p, prefix) and np.array_equal(r, rank)
    want_p, want_r = prefix.copy(), rank.copy()
    R.step([h1], 1, want_p, want_r)
    _capi.quant_step([h1], 1, prefix, rank, lib=hip)
    assert np.array_equal(prefix, want_p) and np.array_equal(rank, want_r)
    f = hip.lib.rmhmc_quant_step
    ptrs = (_capi._dp * 1)(_capi._ptr(np.ascontiguousarray(h1)))
    for args in ((ptrs, 0, 3, 4, 1), (ptrs, 1, 0, 4, 1), (ptrs, 1, 3, 0, 1), (ptrs, 1, 3, 17, 1), (ptrs, 1, 3, 4, 8), (ptrs, 1, 3, 4, -1),
                 (None, 1, 3, 4, 1), ((_capi._dp * 1)(None), 1, 3, 4, 1)):
        assert f(*args, _capi._ptr(prefix, _capi._up), _capi._ptr(rank, _capi._lp)) == -1, args[1:]
    assert np.array_equal(prefix, want_p) and np.array_equal(rank, want_r)


def test_finish_is_one_rounding(hip):
    rs = np.random.RandomState(2)
    lo = np.concatenate([rs.randn(40), [-0.0, 0.0, -TINY, 1.0, -DBL_MAX / 2, 1e-310, -3.0]])
    hi = np.concatenate([lo[:40] + np.abs(rs.randn(40)) * 10.0 ** rs.randint(-18, 3, 40), [0.0, TINY, TINY, np.nextafter(1.0, 2), DBL_MAX / 2, 3e-310, -3.0]])
    g = np.concatenate([rs.rand(40), [0.5, 0.3, 0.5, 0.7, 0.25, 1 / 3, 0.9]])
    g[:4] = 0.0
    P = lo.size
    prefix = np.stack([R.key(lo), R.key(hi)])
    m = np.full(P, 2, dtype=np.int64)
    got = _capi.quant_finish(prefix, g[None], m, lib=hip)
    want = np.array([[R.finish_exact(a, b, c) for a, b, c in zip(lo + 0.0, hi + 0.0, g)]])
    assert R.same_bits(got, want) and R.same_bits(got[0, :4], lo[:4]) and not np.signbit(got[0, 40])
    m[3] = 0
    assert np.isnan(_capi.quant_finish(prefix, g[None], m, lib=hip)[0, 3])
    out = np.full((1, P), -5.0)
    f = hip.lib.rmhmc_quant_finish
    for Q, PP in ((0, P), (9, P), (1, 0)):
        assert f(_capi._ptr(prefix, _capi._up), _capi._ptr(g), _capi._ptr(m, _capi._lp), Q, PP, _capi._ptr(out)) == -1
    assert f(None, _capi._ptr(g), _capi._ptr(m, _capi._lp), 1, P, _capi._ptr(out)) == -1 and (out == -5.0).all()


# ---- csrc/quant.h in a stand-alone program under AddressSanitizer and UBSan -----------------------------------------------------------
def _hx(a):
    return " ".join(float(v).hex() for v in np.ravel(a))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _floats(line):
    return np.array([float.fromhex(v) for v in line.split()])


def test_key_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "quant_probe")
    vals = np.array(EDGE_VALUES + [np.inf, -np.inf, np.nan])
    lines = _run(exe, "keys %d %s\n" % (vals.size, _hx(vals)))
    rows = [ln.split() for ln in lines]
    keys = np.array([int(r[1], 16) for r in rows], dtype=np.uint64)
    back = np.array([float.fromhex(r[2]) for r in rows])
    finite = np.array([int(r[3]) for r in rows])
    n = len(EDGE_VALUES)
    assert list(finite) == [1] * n + [0, 0, 0]
    assert np.array_equal(keys[:n], R.key(vals[:n]))                     # the restatement's key
    assert R.same_bits(back[:n], vals[:n] + 0.0) and R.same_bits(R.unkey(keys[:n]), back[:n])      # invertible; a zero comes back as +0.0
    assert keys[0] == keys[1] == np.uint64(1 << 63)
    order = np.argsort(vals[:n], kind="stable")
    sk, sv = keys[:n][order], vals[:n][order]
    assert ((sk[1:] > sk[:-1]) == (sv[1:] > sv[:-1])).all() and ((sk[1:] == sk[:-1]) == (sv[1:] == sv[:-1])).all()      # monotone
    assert keys[n + 1] < keys[:n].min() and keys[n] > keys[:n].max()     # the infinities bracket the finite keys
    for r, k in zip(rows, keys):
        assert [int(v) for v in r[4:]] == [(int(k) >> (56 - 8 * i)) & 255 for i in range(8)]


def test_plan_step_finish_under_sanitizers(hip, tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "quant_probe")
    m = np.array([0, 1, 2, 5, 700], dtype=np.int64)
    probs = (0.0, 1.0, 0.25, 0.9)
    lines = _run(exe, "plan 5 4 %s %s\n" % (" ".join(map(str, m)), _hx(probs)))
    assert lines[0] == "rc 0"
    rank = np.array([ln.split() for ln in lines[1:9]], dtype=np.int64)
    frac = np.array([_floats(ln) for ln in lines[9:13]])
    want_rank, want_frac = R.plan(m, probs)
    assert np.array_equal(rank, want_rank) and R.same_bits(frac, want_frac)
    assert _run(exe, "plan 1 1 3 %s\n" % _hx([1.25]))[0] == "rc -1" and _run(exe, "plan 1 9 3 %s\n" % _hx([0.5] * 9))[0] == "rc -1"
    # one step, consistent and not
    x = _data()[:, [6, 4]]
    mm = np.isfinite(x).sum(0)
    rk, _ = R.plan(mm, (0.5,))
    pre = np.zeros(rk.shape, dtype=np.uint64)
    R.step([R.hist(x, 0)], 0, pre, rk)
    pieces = [R.hist(x[a:b], 1, pre) for a, b in ((0, 0), (0, 400), (400, 700))]

    def step(parts, r):
        text = "step 2 2 %d %d %s %s %s\n" % (r, len(parts), " ".join("%x" % int(v) for v in pre.ravel()), " ".join(map(str, rk.ravel())),
                                             " ".join(_hx(p) for p in parts))
        out = _run(exe, text)
        return out[0], np.array([int(v, 16) for v in out[1].split()], dtype=np.uint64).reshape(2, 2), np.array(out[2].split(), dtype=np.int64).reshape(2, 2)
    for parts, r in ((pieces[1:2], 1), ([pieces[1], pieces[1]], 1), ([R.hist(x, 2, pre)], 2), ([], 1)):
        rc, p, k = step(parts, r)
        assert rc == "rc -1" and np.array_equal(p, pre) and np.array_equal(k, rk)
    rc, p, k = step(pieces, 1)
    want_p, want_k = pre.copy(), rk.copy()
    R.step(pieces, 1, want_p, want_k)
    assert rc == "rc 0" and np.array_equal(p, want_p) and np.array_equal(k, want_k)
    lib_p, lib_k = pre.copy(), rk.copy()
    _capi.quant_step(pieces, 1, lib_p, lib_k, lib=hip)                   # the library runs the same header
    assert np.array_equal(lib_p, p) and np.array_equal(lib_k, k)
    # the finish
    lo, hi, g = np.array([1.0, -2.5, 0.0]), np.array([1.5, -2.5, TINY]), np.array([1 / 3, 0.7, 0.0])
    text = "finish 3 1 %s %s 4 4 0\n" % (" ".join("%x" % int(v) for v in np.concatenate([R.key(lo), R.key(hi)])), _hx(g))
    out = _run(exe, text)
    got = _floats(out[1])
    assert out[0] == "rc 0" and got[0] == R.finish_exact(1.0, 1.5, 1 / 3) and got[1] == -2.5 and np.isnan(got[2])


@pytest.mark.parametrize("bounds", [(0, 700), (0, 300, 700), (0, 1, 1, 250, 699, 700)], ids=["one", "two", "five_with_an_empty_one"])
def test_whole_loop_under_sanitizers(tmp_path_factory, bounds):
    exe = probe_exe(tmp_path_factory, "quant_probe")
    x = _data()
    N, P = x.shape
    out = _run(exe, "select %d %d %d %d %s %s %s\n" % (N, P, len(PROBS), len(bounds) - 1, _hx(PROBS), " ".join(map(str, bounds)), _hx(x)))
    assert out[0] == "rc 0"
    m = np.array(out[1].split(), dtype=np.int64)
    order = np.array([_floats(ln) for ln in out[2:12]])
    quant = np.array([_floats(ln) for ln in out[12:17]])
    want_order, want_quant, want_m = R.sorted_stats(x, PROBS)
    assert np.array_equal(m, want_m)
    assert R.same_bits(order, want_order)                                # bit-equal to np.sort
    assert R.same_bits(quant, want_quant)                                # and to the exact interpolation between its values
