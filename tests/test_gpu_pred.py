"""GPU checks of the posterior predictive probabilities (include/rmhmc_pred.h, csrc/pred.hip.h) against the np.longdouble restatement
tests/helpers/pred_ref.py: every shape edge of the kernels, invalid draws, saturation, repeatability and merging, the call without
labels, the refusals, no trace on the context, and the shim end to end.  The block and tile sizes come from csrc/pred.h itself,
through tests/helpers/pred_probe.cpp built with the host compiler.

Bounds (u = 2^-53, gamma = D u / (1 - D u), which holds for a dot product of length D in any order, fma or MFMA; A = sum_d |x_d| |w_d|
per (row, draw), A-bar_r its maximum over the used draws).
  f.     |f^ - f| <= gamma A.
  p.     e = exp(-|f|) is good to 1 ulp = 2 u relative; 1 + e and the division round once each.  d log hi / d log e = -e / (1 + e),
         at most 1/2 in size, and d log lo / d log e = 1 / (1 + e) <= 1: hi carries u + u + u = 3 u relative and is at most 1, lo carries
         2 u + u + u = 4 u relative and is at most 1/2.  |dp / df| <= 1/4.  So |p^ - p| <= gamma A / 4 + 3 u.
  S1.    The lanes' sums and the sum over the blocks are compensated pairs (error O(N u^2), nothing); sum + error is rounded once into
         the record and once into the partial, and S1 / m rounds once more: 3 u on a number that is at most 1.
         |prob - ref| <= gamma A-bar / 4 + 6 u.
  pvar.  To first order the error of mean(p^2) - mean(p)^2 under errors delta_k of the p_k is 2 mean((p_k - p-bar) delta_k), at most
         max |delta| in size because mean |p - p-bar| <= 1/2; the roundings of the squares, of the two sums (3 u each as above, on
         numbers that are at most 1), of prob^2 and of the difference come to less than 12 u.  That is inside the
         |pvar - ref| <= 2 (gamma A-bar / 4 + 6 u) + 4 u that the test uses.
  SQ.    On the small side d log q / df <= 1, so a q carries gamma A + 4 u relative, and all q are positive: the sum inherits the largest
         relative error of a term, plus the two roundings: |SQ - ref| <= (gamma A-bar + 6 u) ref.
  lpd.   SQ / m rounds once (an absolute u in the logarithm) and log is good to 1 ulp = 2 u |ref|:
         |lpd - ref| <= gamma A-bar + 6 u + 3 u max(1, |ref|).
  tiny.  Below 2^-1022 doubles are 2^-1074 apart whatever their size, so an e, and the lo made of it, is good to a spacing each there,
         not to a relative error: SQ is allowed 2 m 2^-1074 on top, and lpd the logarithm of that relative change, -log(1 - rel), in
         place of the first-order rel.  It matters for |f| > 708 alone.
  merge. The product of a draw does not depend on where the draw sits in its block or among the blocks (the same MFMA steps in the same
         order), so the p of a split call are the p of the whole call, bit for bit, and the compensated sums of either differ from the
         exact sum of those numbers by O(N u^2).  What differs is the rounding into the record (u), into the partial (u) on either
         side, and the one addition of the merge (u): |merged - whole| <= 5 u |whole| + O(N u^2), allowed as 6 u |whole|."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, posterior_predictive
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pred_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SPACING = 2.0 ** -1074      # of the doubles below 2^-1022
DEV = torch.device("cuda", 0)
_cache = {}


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- the plan of csrc/pred.h, asked of the header itself ---------------------------------------------------------------------------------
def _probe():
    if "exe" not in _cache:
        import tempfile
        cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        _cache["dir"] = tempfile.TemporaryDirectory(prefix="pred_probe_")
        exe = os.path.join(_cache["dir"].name, "pred_probe")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "helpers", "pred_probe.cpp")])
        _cache["exe"] = exe
    return _cache["exe"]


def _ask(text):
    r = subprocess.run([_probe()], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [[int(v) for v in line.split()[1:]] for line in r.stdout.splitlines()]


def plan(N, R, D):
    """(nblocks, draws_per_block) of the main kernel"""
    p = _ask("plan %d %d %d\n" % (N, R, D))[0]
    return p[1], p[2]


def _define(name):
    import re
    hdr = open(os.path.join(ROOT, "riemannhamiltonianmontecarlo_amd", "csrc", "pred.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)\b" % name, hdr).group(1))


TILE = _define("PRED_WAVE_ROWS") * _define("PRED_WAVES")      # PRED_ROW_TILE, the rows of a workgroup
BLOCK = _define("PRED_DRAWS")                                 # the draws of a block


def test_parsed_constants_are_the_plan_s():
    assert _ask("consts\n")[0][:3] == [TILE, _define("PRED_WAVE_ROWS"), BLOCK]
    assert [plan(N, 3, 5)[0] for N in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3)] == [1, 1, 2, 3]
    assert [_ask("plan 5 %d 5\n" % R)[0][0] for R in (TILE - 1, TILE, TILE + 1)] == [1, 1, 2]


# ---- inputs and the comparison -----------------------------------------------------------------------------------------------------------
def draws(n, S, D, R, seed=0, spread=10.0):
    """samples [n][S][D] ~ N(0, spread^2 / D) and rows [R][D] ~ N(0, 1): f = x . w has standard deviation `spread`, so |f| covers 0 to
    about 4 spread = 40; labels by a coin"""
    rs = np.random.RandomState(100000 * D + 1000 * R + 10 * n + S + seed)
    w = rs.randn(n, S, D) * (spread / np.sqrt(D))
    x = rs.randn(R, D)
    t = (rs.rand(R) < 0.5).astype(np.float64)
    return w, x, t


def run(ctx, w, x, t):
    out = ctx.predict(torch.from_numpy(np.ascontiguousarray(w)).to(DEV), x, t)
    out["partial"] = out["partial"].cpu().numpy()
    return out


def check(got, w, x, t, what="", merges=0):
    """a finished result of the GPU against the restatement on the same samples, to the bounds of the module's docstring, with one more
    u for each merge behind it; returns the largest error over its bound"""
    D = x.shape[1]
    want = P.predict(w, x, t)
    m = want["draws_used"]
    part = got["partial"]
    assert got["draws_used"] == m and (part[0] == m).all(), (what, got["draws_used"], m)
    if m == 0:
        assert not part.any() and np.isnan(got["prob"]).all() and np.isnan(got["pvar"]).all() and np.isnan(got["lpd"]).all(), what
        assert np.isnan(got["lpd_total"]), what
        return 0.0
    g = D * U / (1.0 - D * U)
    A = P.abs_product(w, x)
    tol_p = g * A / 4 + (6 + merges) * U
    err = [np.abs(got["prob"] - want["prob"]) / tol_p, np.abs(got["pvar"] - want["pvar"]) / (2 * tol_p + 4 * U)]
    assert (got["pvar"] >= 0.0).all(), what
    if t is None:
        assert not part[3].any() and np.isnan(got["lpd"]).all() and np.isnan(got["lpd_total"]), what
    else:
        ref_q = want["merged"][3]
        tol_q = (g * A + (6 + merges) * U) * ref_q + 2 * m * SPACING
        err.append(np.abs(part[3] - ref_q) / np.where(tol_q > 0, tol_q, 1.0))
        ref_lpd = np.asarray(want["lpd"], dtype=np.float64)
        inf = np.isinf(ref_lpd)
        assert np.array_equal(got["lpd"][inf], ref_lpd[inf]) and not np.isinf(got["lpd"][~inf]).any(), what
        ref_l = want["lpd"][~inf]
        rel = (tol_q / np.where(ref_q > 0, ref_q, 1))[~inf].astype(np.float64)
        assert (rel < 0.5).all(), what
        tol_l = -np.log1p(-rel) + 3 * U * np.maximum(1.0, np.abs(ref_l))
        err.append(np.abs(got["lpd"][~inf] - ref_l) / tol_l)
        if inf.any():
            assert got["lpd_total"] == -np.inf, what
        else:       # the row-order sum of R numbers, each inside its bound
            assert abs(got["lpd_total"] - want["lpd_total"]) <= tol_l.sum() + len(ref_l) * U * np.abs(ref_l).sum(), what
    worst = max(float(e.max()) for e in err if e.size)
    assert worst <= 1.0, (what, [float(e.max()) for e in err if e.size])
    return worst


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.context(10, 2, 1) as c:     # the predictive calls use the context for its device and stream only
        yield c


# ---- 1. shape edges ------------------------------------------------------------------------------------------------------------------------
RS = [1, 15, 16, 17, 33, TILE - 1, TILE, TILE + 1]
DS = [1, 3, 4, 5, 17, 63, 64, 65, 128, 130, 192, 224, 256]     # every step count of the product: 4, 8, 16, 24, .., 64
NS = [1, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3]


@pytest.mark.parametrize("R", RS)
def test_row_edges(ctx, R):
    w, x, t = draws(3, 11, 5, R)
    print("R = %d: worst error / bound %.3f" % (R, check(run(ctx, w, x, t), w, x, t, R)))


@pytest.mark.parametrize("D", DS)
def test_column_edges(ctx, D):
    w, x, t = draws(3, 11, D, 5)
    print("D = %d: worst error / bound %.3f" % (D, check(run(ctx, w, x, t), w, x, t, D)))


@pytest.mark.parametrize("as_chains", [True, False])
@pytest.mark.parametrize("N", NS)
def test_draw_edges(ctx, N, as_chains):
    n, S = (N, 1) if as_chains else (1, N)
    w, x, t = draws(n, S, 5, 3)
    if N == 2 * BLOCK + 3:
        assert plan(N, 3, 5)[0] == 3
    print("N = %d: worst error / bound %.3f" % (N, check(run(ctx, w, x, t), w, x, t, N)))


def test_all_maximum_corner(ctx):
    N = 2 * BLOCK + 3
    w, x, t = draws(1, N, 256, 33)
    assert plan(N, 33, 256)[0] == 3
    print("corner: worst error / bound %.3f" % check(run(ctx, w, x, t), w, x, t, "corner"))


# ---- 2. invalid draws ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("D", [5, 65])
def test_invalid_draws_are_left_out(ctx, D, bad):
    N = 2 * BLOCK + 3
    per = plan(N, 17, D)[1]
    w, x, t = draws(1, N, D, 17)
    clean = run(ctx, w, x, t)
    places = [(0, 0), (N - 1, D // 2), (per - 1, 1 % D), (per, D - 1), (2 * per - 1, D - 1)]   # first, last, around the block edges; the last column
    for count, (j, d) in enumerate(places, 1):
        w[0, j, d] = bad
        got = run(ctx, w, x, t)
        assert got["draws_used"] == N - count
        check(got, w, x, t, (D, bad, j, d))
    assert not same_bits(got["partial"], clean["partial"])
    # the same numbers as a call on the remaining draws alone, to the merge bound (other positions, other blocks)
    keep = np.isfinite(w[0]).all(axis=1)
    alone = run(ctx, w[:, keep], x, t)
    assert same_bits(alone["partial"][0], got["partial"][0])
    assert (np.abs(alone["partial"][1:] - got["partial"][1:]) <= 6 * U * np.abs(got["partial"][1:])).all()


def test_all_draws_invalid(ctx):
    w, x, t = draws(2, 9, 5, 3)
    w[:, :, 4] = np.nan
    w[1, 3, 0] = np.inf
    got = run(ctx, w, x, t)
    assert got["draws_used"] == 0 and not got["partial"].any()
    check(got, w, x, t, "all invalid")
    assert np.isnan(run(ctx, w, x, None)["prob"]).all()


def test_padding_and_flagged_draws_do_not_leak_one_half(ctx):
    """a row of zeros has f = 0 and p = 1/2 in every draw: S1 = m / 2 exactly.  A flagged draw and the padding of the last tile have
    f = 0 in every row as well; were they added, S1 would be (m + their number) / 2"""
    for N in (1, 15, 17, BLOCK + 1):
        w, x, t = draws(1, N, 5, 3)
        x[1] = 0.0
        flagged = sorted({0, N // 2, N - 1}) if N > 1 else []
        for j in flagged:
            w[0, j, 2] = np.nan
        got = run(ctx, w, x, t)
        m = N - len(flagged)
        assert got["draws_used"] == m
        assert got["partial"][1, 1] == 0.5 * m and got["partial"][2, 1] == 0.25 * m and got["partial"][3, 1] == 0.5 * m
        assert got["prob"][1] == 0.5 and got["pvar"][1] == 0.0 and abs(got["lpd"][1] - np.log(0.5)) <= 2 * U
        check(got, w, x, t, N)


# ---- 3. saturation -------------------------------------------------------------------------------------------------------------------------
def test_saturation(ctx):
    """f = +-800 (e = exp(-800) = 0: p is exactly 1 or 0) and +-40 (p = 1 - 4e-18 rounds to 1; 1 - p = 4.2e-18 does not)"""
    N = 37
    x = np.array([[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [0.0, 1.0], [0.0, -1.0]])
    t = np.array([1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    w = np.empty((1, N, 2))
    w[0, :, 0] = 800.0          # rows 0 - 3: f = +-800 in every draw
    w[0, :, 1] = 800.0          # rows 4 - 7: f = +-800 in every draw but one, where it is +-40
    w[0, 20, 1] = 40.0
    got = run(ctx, w, x, t)
    assert got["draws_used"] == N
    assert got["prob"][[0, 2]].tolist() == [1.0, 1.0] and got["prob"][[1, 3]].tolist() == [0.0, 0.0]
    assert got["pvar"][:4].tolist() == [0.0] * 4 and (got["pvar"] >= 0.0).all()
    assert got["lpd"][[0, 3]].tolist() == [0.0, 0.0]                       # every q is exactly 1
    assert got["lpd"][[1, 2]].tolist() == [-np.inf, -np.inf]              # every q underflowed
    assert got["prob"][4] == 1.0 and got["lpd"][4] == 0.0 and got["lpd"][7] == 0.0
    q40 = np.exp(-40.0) / (1.0 + np.exp(-40.0))
    for r in (5, 6):                                                      # one draw of 37 has q = 4.2e-18, the others 0
        assert np.isfinite(got["lpd"][r]) and abs(got["lpd"][r] - np.log(q40 / N)) < 1e-12
        assert 0.0 < got["prob"][5] < 1e-18
    assert got["lpd_total"] == -np.inf
    check(got, w, x, t, "saturation")
    # denormal likelihoods: f = -740 gives q = 4.2e-322, kept, not flushed
    w2 = np.full((1, 5, 2), 740.0)
    got = run(ctx, w2, x[:2], t[:2])
    assert got["lpd"][0] == 0.0 and abs(got["lpd"][1] + 740.0) < 0.02 and 0.0 < got["prob"][1] < 1e-320
    check(got, w2, x[:2], t[:2], "denormal")


# ---- 4. repeatability and merging ----------------------------------------------------------------------------------------------------------
def test_repeatable_and_mergeable(ctx):
    w, x, t = draws(8, 2 * BLOCK // 8 + 5, 20, TILE + 1)
    w[2, 7, 3] = np.nan
    w[6, 0, 0] = np.inf
    a, b = run(ctx, w, x, t), run(ctx, w, x, t)
    assert same_bits(a["partial"], b["partial"])
    for k in ("prob", "pvar", "lpd", "lpd_total", "draws_used"):
        assert same_bits(a[k], b[k]), k
    check(a, w, x, t, "whole")
    head, tail = run(ctx, w[:3], x, t), run(ctx, w[3:], x, t)
    merged = _capi.pred_finish([head["partial"], tail["partial"]])
    assert merged["draws_used"] == a["draws_used"] == w.shape[0] * w.shape[1] - 2 and same_bits(merged["merged"][0], a["partial"][0])
    assert (np.abs(merged["merged"][1:] - a["partial"][1:]) <= 6 * U * np.abs(a["partial"][1:])).all()
    check(dict(merged, partial=merged["merged"]), w, x, t, "merged", merges=1)
    # the identity changes no bit, wherever it stands; torch tensors and arrays mix
    ident = _capi.pred_identity(x.shape[0])
    again = _capi.pred_finish([ident, torch.from_numpy(a["partial"]), ident])
    assert same_bits(again["merged"], a["partial"])
    for k in ("prob", "pvar", "lpd", "lpd_total", "draws_used"):
        assert same_bits(again[k], a[k]), k


def test_without_labels(ctx):
    w, x, t = draws(2, BLOCK // 2 + 9, 33, 17)
    with_t, without = run(ctx, w, x, t), run(ctx, w, x, None)
    assert not without["partial"][3].any() and np.isnan(without["lpd"]).all() and np.isnan(without["lpd_total"])
    assert same_bits(without["partial"][:3], with_t["partial"][:3])
    assert same_bits(without["prob"], with_t["prob"]) and same_bits(without["pvar"], with_t["pvar"])
    check(without, w, x, None, "no labels")
    halves = _capi.pred_finish([run(ctx, w[:1], x, None)["partial"], run(ctx, w[1:], x, None)["partial"]])
    assert np.isnan(halves["lpd"]).all() and not halves["merged"][3].any()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_partial_untouched(ctx):
    dp = C.POINTER(C.c_double)

    def call(n, S, D, x, t, R, w=None, part=True):
        w = torch.zeros((n, S, max(D, 1)), dtype=torch.float64, device=DEV) if w is None else w
        out = torch.full((4, max(R, 1) + 2), -7.0, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        rc = ctx.lib.rmhmc_pred_partial_dev(ctx._h, w.data_ptr(), n, S, D, None if x is None else x.ctypes.data_as(dp),
                                            None if t is None else t.ctypes.data_as(dp), R, out.data_ptr() if part else None)
        assert (out.cpu().numpy() == -7.0).all()
        return rc

    x = np.ones((3, 4)); t = np.array([0.0, 1.0, 1.0])
    assert call(2, 2, 257, np.ones((3, 257)), t, 3) == -4                     # RMHMC_ERR_UNSUPPORTED
    half = t.copy(); half[1] = 0.5
    nan_x = x.copy(); nan_x[2, 3] = np.nan
    inf_x = x.copy(); inf_x[0, 0] = -np.inf
    for args in ((2, 2, 4, x, half, 3), (2, 2, 4, nan_x, t, 3), (2, 2, 4, inf_x, None, 3), (2, 2, 4, x, t, 0), (0, 2, 4, x, t, 3), (2, 0, 4, x, t, 3),
                 (2, 2, 0, x, t, 3), (2, 2, 4, None, t, 3)):
        assert call(*args) == -1, args[:3] + args[5:]                           # RMHMC_ERR_INVALID
    assert call(2, 2, 4, x, t, 3, part=False) == -1
    assert ctx.lib.rmhmc_pred_partial_dev(ctx._h, None, 2, 2, 4, x.ctypes.data_as(dp), None, 3, torch.zeros(12, dtype=torch.float64, device=DEV).data_ptr()) == -1
    # the binding's own checks, and the library's through it
    good = torch.zeros((2, 2, 4), dtype=torch.float64, device=DEV)
    for bad in (lambda: ctx.predict_partial(good.cpu(), x), lambda: ctx.predict_partial(good.float(), x), lambda: ctx.predict_partial(good[0], x),
                lambda: ctx.predict_partial(good, x[:, :3]), lambda: ctx.predict_partial(good, x, t[:2])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.predict(good, x, half)
    assert e.value.code == -1 and "tnew" in str(e.value)
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.predict(torch.zeros((1, 2, 257), dtype=torch.float64, device=DEV), np.ones((3, 257)))
    assert e.value.code == -4
    assert ctx.predict(good, x, t)["draws_used"] == 4                          # the context works on


# ---- 6. the context keeps no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace_on_the_context(hip):
    M, D, n = 200, 6, 16
    XX, t = synthetic_logreg(M, D, 3)

    def sample(c):
        r = c.phmc_sample_to(12, 2, L=5, eps=0.3, where="device", device=DEV, samples=True, seed=5)
        return r["samples"], r["accepted"].cpu().numpy(), r["leapfrog_steps"].cpu().numpy()

    with hip.context(M, D, n) as c:
        c.set_data(XX, t)
        c.phmc_set_mass(c.phmc_mode()["G"])
        opts = c.options()
        lp = c.log_posterior(np.zeros((n, D)))
        first = sample(c)
        p1 = c.predict(first[0], XX[:70], t[:70])
        p2 = c.predict(first[0][:, :, :3].contiguous(), XX[:5, :3])               # another D than the context's
        assert c.options() == opts
        second = sample(c)
        assert same_bits(lp, c.log_posterior(np.zeros((n, D))))
        p3 = c.predict(second[0], XX[:70], t[:70])
    for a, b in zip(first, second):
        assert same_bits(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, b.cpu().numpy() if isinstance(b, torch.Tensor) else b)
    assert same_bits(p1["partial"].cpu().numpy(), p3["partial"].cpu().numpy()) and p2["draws_used"] == n * 10


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------------
def test_posterior_predictive_end_to_end(hip):
    XX, t = synthetic_logreg(300, 6, 0)
    Xtr, ttr, Xnew, tnew = XX[:200], t[:200], XX[200:], t[200:]
    r = posterior_predictive(Xtr, ttr, Xnew, tnew, n_chains=64, NumOfIterations=120, BurnIn=20)
    assert r["draws_used"] == 64 * 100 and r["prob"].shape == r["pvar"].shape == r["lpd"].shape == (100,)
    assert 0.0 <= r["accept"] <= 1.0 and r["seconds"] > 0.0 and r["partial"].shape == (4, 100)
    with hip.context(200, 6, 64) as c:          # the same sequence by hand
        c.set_data(Xtr, ttr, 100.0)
        md = c.phmc_mode()
        c.phmc_set_mass(md["G"])
        st = c.phmc_sample_to(120, 20, L=6, eps=0.5, where="device", device=DEV, samples=True, seed=0, theta0=md["w"])
        mine = c.predict(st["samples"], Xnew, tnew)
        w = st["samples"].cpu().numpy()
    assert w.shape == (64, 100, 6) and np.isfinite(w).all()
    for k in ("prob", "pvar", "lpd", "lpd_total", "draws_used"):
        assert same_bits(r[k], mine[k]), k
    assert same_bits(r["partial"], mine["partial"].cpu().numpy()) and same_bits(r["info"]["mode"], md["w"])
    assert same_bits(r["info"]["accepted"], st["accepted"].cpu().numpy())
    print("end to end: worst error / bound %.3f, lpd_total %.3f, acceptance %.3f"
          % (check(dict(r), w, Xnew, tnew, "end to end"), r["lpd_total"], r["accept"]))
    none = posterior_predictive(Xtr, ttr, Xnew, None, n_chains=64, NumOfIterations=120, BurnIn=20)
    assert same_bits(none["prob"], r["prob"]) and np.isnan(none["lpd"]).all()
