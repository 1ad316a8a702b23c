"""GPU checks of leave-one-out cross-validation (include/rmhmc_loo.h, csrc/loo.hip.h) against the np.longdouble restatement
tests/helpers/loo_ref.py: the log-likelihood matrix at every shape edge of its kernel, edge values and non-finite draws; the cutoff and
the counts bit for bit against np.sort on the device's own ll; ties; the tail-length edges; the fit; determinism, the whole run against
the composition of its pieces, every cols_per_block; refusals; no trace on the context; psis_loo end to end against quadrature.

Bound of ll (u = 2^-53, gamma = D u / (1 - D u), which holds for a dot product of length D in any order, fma or MFMA; A = sum_d |x_d| |w_d|
per (draw, column)).  |f^ - f| <= gamma A.  l = min(s, 0) - log1p(exp(-|f|)) has |dl / df| <= 1, so the error of f costs gamma A.  exp and
log1p are good to 1 ulp = 2 u relative each; the error of e = exp(-|f|) <= 1 enters log1p(e) <= log 2 with a factor e / (1 + e) <= 1/2 relative
to a number below 1: u; log1p's own 2 u on a number below 0.7; the subtraction rounds once: u |l|.  Together |l^ - l| <= gamma A + 4 u
max(1, |l|), the per-draw bound tests/test_gpu_pred.py derives for lpd.  Where s > 0, l = -log1p(e) alone and every one of those errors
is relative to |l| (d log|l| / df is at most 1 in size): |l^ - l| <= (gamma A + 6 u) |l| + 2^-1074, which is what "relative accuracy
from -1e-300" means; the edge-value test asserts it.  Largest error over the bound seen on the MI355X over all shapes of this file:
see FIT below and DESIGN section 8k.

The fit against the restatement fed the device's own ll bits: tail membership is then identical and only the arithmetic differs (the
device's exp, log1p, expm1 in doubles and its summation order against long doubles).  No bound follows from first principles that
would be tight enough to be worth having: the pass bound is 16 times the largest deviation measured over all shapes of this file
against the np.longdouble restatement (never against the code under test), FIT below, the maximum of rounding noise over a few hundred
columns, which moves by small factors from one input to the next."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from riemannhamiltonianmontecarlo_amd import _capi, psis_loo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import context_history as H  # noqa: E402
import loo_quad as Q  # noqa: E402
import loo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
DEV = torch.device("cuda", 0)
SIGN = 1 << 63
EDGE = 29826161          # the largest m whose tail is RMHMC_LOO_MAX_TAIL draws
# the largest deviations measured on the MI355X over all shapes of this file (khat and elpd_loo absolute, the others relative); the
# tests allow 16 times these
# (khat and sigma at the longest tail, M = 16384; A_tail and elpd_loo at N = 256, C = 3; the ll error over its bound was 0.40 at most)
FIT = dict(khat=5.04e-15, sigma=4.94e-15, A_tail=5.22e-15, B_tail=1.50e-15, A_body=3.31e-16, B_body=1.96e-16, elpd_loo=5.22e-15)
_worst = dict.fromkeys(FIT, 0.0)
_worst["ll"] = 0.0


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unkey(key):
    key = int(key)
    u = key ^ SIGN if key & SIGN else ~key & (2 ** 64 - 1)
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def draws(n, S, D, Cn, seed=0, spread=3.0):
    """samples [n][S][D] ~ N(0, spread^2 / D) and rows [C][D] ~ N(0, 1): f = x . w has standard deviation `spread`; labels by a coin"""
    rs = np.random.RandomState(100000 * D + 1000 * Cn + 10 * n + S + seed)
    w = rs.randn(n, S, D) * (spread / np.sqrt(D))
    x = rs.randn(Cn, D)
    t = (rs.rand(Cn) < 0.5).astype(np.float64)
    return w, x, t


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.context(10, 2, 1) as c:     # the calls use the context for its device and stream only
        yield c


def check_ll(ll, w, x, t, what=""):
    """ll [N][C] of the device against the restatement, to the bound of the module's docstring; returns the largest error over it"""
    D = x.shape[1]
    want = R.loglik(w, x, t)
    assert ll.shape == want.shape, what
    nan = np.isnan(want.astype(np.float64))
    assert np.array_equal(np.isnan(ll), nan), what
    assert not np.signbit(ll[ll == 0.0]).any(), what
    g = D * U / (1.0 - D * U)
    A = R.abs_product(w, x)
    with np.errstate(invalid="ignore"):
        tol = g * A + 4 * U * np.maximum(1.0, np.abs(want))
        ratio = np.where(nan, 0, np.abs(ll - want) / tol)
    worst = float(ratio.max()) if ratio.size else 0.0
    _worst["ll"] = max(_worst["ll"], worst)
    assert worst <= 1.0, (what, worst)
    return worst


def pieces(ctx, w, x, t):
    """the whole run as the composition of the pieces and the select's own calls; everything on the host at the end"""
    return pieces_of_ll(ctx, ctx.loo_loglik(dev(w), x, t))


def pieces_of_ll(ctx, ll):
    """everything after the log-likelihood from ll [n][S][C] on the device"""
    part = ctx.loo_moments(ll)
    ph = part.cpu().numpy()
    Cn = ph.shape[1]
    tl, rank0 = _capi.loo_plan(ph[0].astype(np.int64))
    cut = np.full(Cn, np.nan)
    if (rank0 >= 0).any():
        prefix = np.zeros((1, Cn), dtype=np.uint64); rank = rank0.reshape(1, Cn).copy()
        for r in range(_capi.QUANT_ROUNDS):
            _capi.quant_step([ctx.quant_hist(ll, r, prefix if r else None, 1)], r, prefix, rank)
        for c in range(Cn):
            if tl[c] >= 5:
                cut[c] = unkey(prefix[0, c])
    sp = ctx.loo_split(ll, cut, ph[4], tl)
    fit = ctx.loo_fit(sp["tail"], sp["counts"], cut, ph[4], tl)
    out = _capi.loo_finish([part], fit, sp["body"])
    out.update(ll=ll.cpu().numpy().reshape(-1, Cn), partial=ph, cut=cut, tail_len=tl, counts=sp["counts"].cpu().numpy(),
               fit=fit.cpu().numpy(), body=sp["body"].cpu().numpy(), tail=sp["tail"].cpu().numpy())
    return out


def check_pieces(got, what=""):
    """everything after ll against the restatement fed the device's own ll bits: the cutoff, the counts and the tail bit for bit, the
    moments, the body, the fit and the pointwise values to rounding (FIT); returns the deviations"""
    ll = got["ll"]
    Cn = ll.shape[1]
    mom = R.moments(ll)
    fit, body, cols = R.columns(ll)
    ph = got["partial"]
    assert np.array_equal(ph[0], mom[0].astype(np.float64)) and np.array_equal(ph[4], mom[4].astype(np.float64)), what
    some = ph[0] > 0
    big = np.maximum(1.0, np.abs(mom[1].astype(np.float64)))
    assert np.all(np.abs(ph[1] - mom[1])[some] <= 4 * U * big[some]), what
    assert np.all(np.abs(ph[2] - mom[2])[some] <= 8 * U * (mom[2] + mom[0] * U * big * big)[some] + 1e-300), what
    assert np.all(np.abs(ph[3] - mom[3])[some] <= 4 * U * mom[3][some]), what
    dv = dict.fromkeys(FIT, 0.0)
    for c, col in enumerate(cols):
        srt = np.sort(ll[:, c][np.isfinite(ll[:, c])])
        assert got["tail_len"][c] == col["M"] == R.tail_len(srt.size), (what, c)
        if col["M"] >= 5:
            assert same_bits(got["cut"][c], srt[col["M"]]) and same_bits(got["cut"][c], np.float64(col["cut"])), (what, c)
            assert same_bits(np.sort(got["tail"][c, :col["n_lt"]]), srt[:col["n_lt"]]), (what, c)
        assert (got["counts"][0, c], got["counts"][1, c]) == (col["n_lt"], col["n_gt"]), (what, c, got["counts"][:, c], col["n_lt"], col["n_gt"])
        assert np.isinf(got["fit"][0, c]) == bool(np.isinf(col["khat"])), (what, c, got["fit"][:, c], col["khat"])
        if col["m"] == 0:
            assert np.isnan(got["elpd_loo"][c]) and np.isnan(got["pareto_k"][c]), (what, c)
            continue
        if np.isfinite(col["khat"]):
            dv["khat"] = max(dv["khat"], abs(float(got["fit"][0, c] - col["khat"])))
            dv["sigma"] = max(dv["sigma"], abs(float(got["fit"][1, c] / col["sigma"] - 1)))
        for key, mine, ref in (("A_tail", got["fit"][2, c], col["A_tail"]), ("B_tail", got["fit"][3, c], col["B_tail"]),
                               ("A_body", got["body"][0, c], col["A_body"]), ("B_body", got["body"][1, c], col["B_body"])):
            if ref == 0:
                assert mine == 0, (what, c, key)
            else:
                dv[key] = max(dv[key], abs(float(mine / ref - 1)))
        dv["elpd_loo"] = max(dv["elpd_loo"], abs(float(got["elpd_loo"][c] - col["elpd_loo"])))
    print("%s: deviations from the restatement %s" % (what, " ".join("%s %.2e" % kv for kv in dv.items())))
    for k, v in dv.items():
        _worst[k] = max(_worst[k], v)
        assert v <= 16 * FIT[k], (what, k, v)
    # the finish: the library's against the restatement's on the device's own partial, fit and body
    want = R.finish([ph.astype(R.LD)], got["fit"].astype(R.LD), got["body"].astype(R.LD))
    for key in _capi.LOO_POINTWISE:
        w = np.asarray(want[key], dtype=np.float64)
        assert np.array_equal(np.isnan(got[key]), np.isnan(w)), (what, key)
        fin = np.isfinite(w)
        assert np.all(np.abs(got[key][fin] - w[fin]) <= 64 * U * np.maximum(1.0, np.abs(w[fin]))), (what, key)
    assert (got["k_mid"], got["k_high"]) == (want["k_mid"], want["k_high"]), what
    return dv


def run_all(ctx, w, x, t, what):
    got = pieces(ctx, w, x, t)
    worst = check_ll(got["ll"], w, x, t, what)
    print("%s: ll worst error / bound %.3f" % (what, worst))
    check_pieces(got, what)
    return got


# ---- 1. shape edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 15, 16, 17, 63, 64])
def test_column_edges(ctx, Cn):
    w, x, t = draws(3, 11, 5, Cn)
    run_all(ctx, w, x, t, "C = %d" % Cn)


@pytest.mark.parametrize("D", [1, 3, 4, 5, 17, 63, 64, 65, 128, 130, 192, 224, 256])     # every step count of the product
def test_dimension_edges(ctx, D):
    w, x, t = draws(3, 11, D, 5)
    run_all(ctx, w, x, t, "D = %d" % D)


@pytest.mark.parametrize("as_chains", [True, False])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 255, 256, 257, 515])
def test_draw_edges(ctx, N, as_chains):
    n, S = (N, 1) if as_chains else (1, N)
    w, x, t = draws(n, S, 5, 3)
    run_all(ctx, w, x, t, "N = %d" % N)


def test_many_columns_with_real_tails(ctx):
    """64 columns x 2100 draws (M = 138, G = 41) and 17 x 8200 (two reduction blocks; M = 272): the shapes the fit's figures come from"""
    for n, S, D, Cn in ((7, 300, 20, 64), (4, 2050, 33, 17)):
        w, x, t = draws(n, S, D, Cn, spread=2.0)
        got = run_all(ctx, w, x, t, "%d x %d" % (n * S, Cn))
        assert np.isfinite(got["pareto_k"]).all() and (got["tail_len"] == R.tail_len(n * S)).all()


def test_block_independence(ctx):
    """the l of a (draw, column) pair does not depend on where the draw or the column sits in the call"""
    w, x, t = draws(2, 300, 37, 64)
    whole = ctx.loo_loglik(dev(w), x, t).cpu().numpy()
    for c0, c1 in ((0, 1), (5, 22), (16, 64), (63, 64)):
        assert same_bits(ctx.loo_loglik(dev(w), x[c0:c1], t[c0:c1]).cpu().numpy(), whole[:, :, c0:c1])
    perm = np.random.RandomState(0).permutation(64)
    assert same_bits(ctx.loo_loglik(dev(w), x[perm], t[perm]).cpu().numpy(), whole[:, :, perm])
    flat = w.reshape(1, 600, 37)
    for j0, j1 in ((0, 1), (7, 270), (255, 600), (599, 600)):
        assert same_bits(ctx.loo_loglik(dev(flat[:, j0:j1]), x, t).cpu().numpy().reshape(-1, 64), whole.reshape(600, 64)[j0:j1])


# ---- 2. edge values and non-finite draws ---------------------------------------------------------------------------------------------------
def test_edge_values(ctx):
    """f = +-800, +-40, -740 with either label, and a row of zeros (l = -log 2)"""
    fs = np.array([800.0, -800.0, 40.0, -40.0, 740.0, -740.0, 0.5, -0.5])
    w = np.zeros((1, len(fs), 2)); w[0, :, 0] = fs; w[0, :, 1] = 1.0
    x = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 0.0]]); t = np.array([1.0, 0.0, 1.0, 0.0])
    ll = ctx.loo_loglik(dev(w), x, t).cpu().numpy().reshape(-1, 4)
    check_ll(ll, w, x, t, "edge values")
    assert same_bits(ll[:, 2], np.full(len(fs), -np.log(2.0))) or np.all(np.abs(ll[:, 2:] + np.log(2.0)) <= 2 * U)
    assert ll[0, 0] == 0.0 and ll[1, 1] == 0.0 and ll[0, 1] == -800.0 and ll[1, 0] == -800.0 and not np.signbit(ll[[0, 1], [0, 1]]).any()
    want = R.loglik(w, x, t)
    for j, c in ((2, 0), (3, 1), (4, 0), (5, 1), (6, 0), (7, 1)):       # s > 0: relative accuracy, down to the denormals
        g = 2 * U / (1 - 2 * U)
        assert ll[j, c] < 0.0 and abs(ll[j, c] - want[j, c]) <= (g * abs(fs[j]) + 6 * U) * abs(want[j, c]) + 2.0 ** -1074, (j, c, ll[j, c])
    assert abs(ll[2, 0] / -4.248354255291589e-18 - 1) < 1e-13 and 0 < -ll[4, 0] < 1e-320 and abs(ll[5, 0] + 740.0) < 1e-12


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_invalid_draws(ctx, bad):
    N, D, Cn = 515, 5, 17
    w, x, t = draws(1, N, D, Cn)
    clean = pieces(ctx, w, x, t)
    for j, d in ((0, 0), (N - 1, D // 2), (255, 1), (256, D - 1), (511, D - 1)):      # first, last, around the block edges; the last column of w
        w[0, j, d] = bad
    got = run_all(ctx, w, x, t, "invalid draws %r" % bad)
    assert (got["draws_used"] == N - 5).all() and np.isnan(got["ll"][[0, 255, 256, 511, N - 1]]).all()
    keep = np.isfinite(w[0]).all(axis=1)
    assert same_bits(got["ll"][keep], clean["ll"][keep])
    alone = pieces(ctx, w[:, keep], x, t)            # the same tails as a call on the remaining draws alone: cutoff and counts to the bit
    assert same_bits(alone["cut"], got["cut"]) and same_bits(alone["counts"], got["counts"]) and same_bits(alone["fit"], got["fit"])


def test_non_finite_l_is_left_out_of_its_own_column(ctx):
    """an l of -inf (an f that overflowed: finite draw, finite row) and a NaN l leave their own column only.  (A product of finite
    numbers cannot give a NaN f on the matrix cores: the fused steps do not round a product to infinity before they add it, so
    inf - inf does not arise; the NaN of this test is put into ll itself.)"""
    w, x, t = draws(1, 300, 2, 3)
    w[0, :, 0] = 0.0; w[0, 5, 0] = 1e160; x[:, 0] = [0.0, 1e160, 0.0]; t[1] = 0.0       # f of column 1 at draw 5: 1e320 = +inf, s = -inf
    ll = ctx.loo_loglik(dev(w), x, t)
    h = ll.cpu().numpy().reshape(-1, 3)
    assert h[5, 1] == -np.inf and np.isfinite(h[5, [0, 2]]).all() and np.isfinite(np.delete(h[:, 1], 5)).all()
    h[9, 2] = np.nan
    got = pieces_of_ll(ctx, dev(h.reshape(1, 300, 3)))
    assert got["partial"][0].tolist() == [300.0, 299.0, 299.0]
    check_pieces(got, "non-finite l")
    assert same_bits(got["partial"][:, 0], ctx.loo_moments(ll).cpu().numpy()[:, 0])


def test_all_draws_invalid(ctx):
    w, x, t = draws(2, 9, 5, 3)
    w[:, :, 4] = np.nan
    got = run_all(ctx, w, x, t, "all invalid")
    assert not got["draws_used"].any() and np.isnan(got["ll"]).all() and np.isnan(got["totals"]["elpd_loo"])
    assert same_bits(got["partial"], _capi.loo_identity(3)) and not got["body"].any()
    whole = ctx.loo(dev(w), x, t)
    assert np.isnan(whole["elpd_loo"]).all() and np.isnan(whole["elpd_waic"]).all() and np.isnan(whole["pareto_k"]).all()


# ---- 3. ties and the tail-length edges -----------------------------------------------------------------------------------------------------
def test_ties_straddle_the_cutoff(ctx):
    """every chain a copy of one chain: each value seven times; 700 draws, M = 80, the cutoff value holds ranks 77 .. 83"""
    w, x, t = draws(1, 100, 4, 5)
    w = np.repeat(w, 7, axis=0)
    got = run_all(ctx, w, x, t, "ties")
    assert (got["tail_len"] == 80).all() and (got["counts"][0] == 77).all() and (got["counts"][1] == 700 - 84).all()


def test_all_draws_identical(ctx):
    """a constant tail: no smoothing, khat = inf, elpd_loo_c = l"""
    w, x, t = draws(1, 1, 4, 5)
    w = np.repeat(w, 300, axis=1)
    got = run_all(ctx, w, x, t, "identical")
    l = got["ll"][0]
    assert (got["ll"] == l).all() and np.isinf(got["pareto_k"]).all() and got["k_high"] == 5
    assert np.all(np.abs(got["elpd_loo"] - l) <= 8 * U * np.maximum(1.0, np.abs(l)))
    assert np.all(got["partial"][2] <= 300 * (2 * U * l) ** 2) and np.all(np.abs(got["elpd_waic"] - l) <= 8 * U * np.maximum(1.0, np.abs(l)))


@pytest.mark.parametrize("N,M", [(24, 4), (25, 5), (225, 45)])
def test_tail_length_edges(ctx, N, M):
    w, x, t = draws(1, N, 3, 4)
    got = run_all(ctx, w, x, t, "m = %d" % N)
    assert (got["tail_len"] == M).all()
    assert np.isinf(got["pareto_k"]).all() == (M < 5)
    if M < 5:
        assert not got["fit"][2:].any() and np.isnan(got["cut"]).all() and (got["counts"][1] == N).all()


def test_longest_tail_and_the_refusal_above_it(ctx):
    """one column with D = 1 at M = RMHMC_LOO_MAX_TAIL exactly (m = 29 826 161), and the smallest m above that: refused, outputs
    untouched.  The restatement's fit on the 16384 tail values; cutoff and counts against np.partition."""
    g = torch.Generator(device=DEV); g.manual_seed(7)
    w = torch.randn((1, EDGE + 1, 1), dtype=torch.float64, device=DEV, generator=g)
    x = np.array([[1.5]]); t = np.array([1.0])
    top = w[:, :EDGE].contiguous()
    got = ctx.loo(top, x, t)
    ll = ctx.loo_loglik(top, x, t).cpu().numpy().reshape(-1)
    M = _capi.LOO_MAX_TAIL
    assert got["draws_used"][0] == EDGE and R.tail_len(EDGE) == M
    low = np.sort(np.partition(ll, M)[:M + 1])
    cut = low[M]
    n_lt = int((low[:M] < cut).sum())
    y = np.expm1((cut - np.concatenate([low[:n_lt], np.full(M - n_lt, cut)])[::-1]).astype(R.LD))
    khat, sigma = R.gpd_fit(y)
    print("longest tail: khat %.6f (restatement %.6f), deviation %.2e, sigma deviation %.2e"
          % (got["pareto_k"][0], khat, abs(got["pareto_k"][0] - khat), abs(got["fit"][1, 0] / sigma - 1)))
    _worst["khat"] = max(_worst["khat"], abs(float(got["pareto_k"][0] - khat)))
    _worst["sigma"] = max(_worst["sigma"], abs(float(got["fit"][1, 0] / sigma - 1)))
    assert abs(got["pareto_k"][0] - float(khat)) <= 16 * FIT["khat"] and abs(float(got["fit"][1, 0] / sigma - 1)) <= 16 * FIT["sigma"]
    body = np.exp(ll.min() - ll[ll > cut]).sum() + ((ll == cut).sum() - (M - n_lt)) * np.exp(ll.min() - cut)
    assert abs(got["body"][0, 0] / body - 1) < 1e-10
    outs = [np.full(k, -7.0) for k in (5, 4, 2, 1, 1, 1, 1, 1, 1, 6)]
    ints = [np.full(2, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)]
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rc = ctx.lib.rmhmc_loo_dev(ctx._h, w.data_ptr(), 1, EDGE + 1, 1, x.ctypes.data_as(dp), t.ctypes.data_as(dp), 1, 0,
                               *[o.ctypes.data_as(dp) for o in outs], *[o.ctypes.data_as(lp) for o in ints])
    assert rc == -4 and all((o == -7.0).all() for o in outs) and all((o == -7).all() for o in ints)


# ---- 4. determinism and composition --------------------------------------------------------------------------------------------------------
KEYS = _capi.LOO_POINTWISE + ("draws_used", "partial", "fit", "body")


def test_repeatable_and_equal_to_the_composition(ctx):
    w, x, t = draws(6, 350, 12, 64, spread=2.0)
    w[2, 7, 3] = np.nan
    a, b = ctx.loo(dev(w), x, t), ctx.loo(dev(w), x, t)
    p, q = pieces(ctx, w, x, t), pieces(ctx, w, x, t)
    for k in KEYS:
        assert same_bits(a[k], b[k]) and same_bits(a[k], p[k]) and same_bits(p[k], q[k]), k
    assert a["totals"] == b["totals"] == p["totals"] and (a["k_mid"], a["k_high"]) == (p["k_mid"], p["k_high"])
    assert same_bits(p["ll"], q["ll"]) and same_bits(np.sort(p["tail"], axis=1)[:, :1], np.sort(q["tail"], axis=1)[:, :1])


def test_every_cols_per_block_gives_the_same_bits(ctx):
    w, x, t = draws(5, 300, 9, 65, spread=2.0)
    w[1, 0, 0] = np.inf
    runs = [ctx.loo(dev(w), x, t, cpb) for cpb in (1, 16, 64, 0)]
    for r in runs[1:]:
        for k in KEYS:
            assert same_bits(r[k], runs[0][k]), k
        assert r["totals"] == runs[0]["totals"]
    # ... and the composition of the pieces over the first 64 and the last column
    head, last = pieces(ctx, w, x[:64], t[:64]), pieces(ctx, w, x[64:], t[64:])
    for k in _capi.LOO_POINTWISE:
        assert same_bits(np.concatenate([head[k], last[k]]), runs[0][k]), k
    check_pieces(head, "R = 65, head")


# ---- 5. refusals, and no trace on the context ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    w = torch.zeros((2, 3, 4), dtype=torch.float64, device=DEV)
    x = np.ones((3, 4)); t = np.array([0.0, 1.0, 1.0])
    half = t.copy(); half[1] = 0.5
    nan_x = x.copy(); nan_x[2, 3] = np.nan
    wide_x = np.ones((3, 257)); many_x = np.ones((65, 4)); many_t = np.zeros(65)
    out = torch.full((2 * 3 * 66,), -7.0, dtype=torch.float64, device=DEV)
    iout = torch.full((2 * 66,), -7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def ptr(a, typ=dp):
        return None if a is None else a.ctypes.data_as(typ)

    def clean():
        torch.cuda.synchronize()
        return bool((out == -7.0).all()) and bool((iout == -7).all())
    lib, h = ctx.lib, ctx._h
    # the log-likelihood
    for args, code in (((w.data_ptr(), 2, 3, 4, ptr(x), ptr(half), 3), -1), ((w.data_ptr(), 2, 3, 4, ptr(nan_x), ptr(t), 3), -1),
                       ((w.data_ptr(), 2, 3, 257, ptr(wide_x), ptr(t), 3), -4), ((w.data_ptr(), 2, 3, 4, ptr(many_x), ptr(many_t), 65), -1),
                       ((w.data_ptr(), 0, 3, 4, ptr(x), ptr(t), 3), -1), ((w.data_ptr(), 2, 0, 4, ptr(x), ptr(t), 3), -1),
                       ((w.data_ptr(), 2, 3, 0, ptr(x), ptr(t), 3), -1), ((w.data_ptr(), 2, 3, 4, ptr(x), ptr(t), 0), -1),
                       ((None, 2, 3, 4, ptr(x), ptr(t), 3), -1), ((w.data_ptr(), 2, 3, 4, None, ptr(t), 3), -1),
                       ((w.data_ptr(), 2, 3, 4, ptr(x), None, 3), -1)):
        assert lib.rmhmc_loo_loglik_dev(h, *args, out.data_ptr()) == code and clean(), args[1:4]
    assert lib.rmhmc_loo_loglik_dev(h, w.data_ptr(), 2, 3, 4, ptr(x), ptr(t), 3, None) == -1
    # the moments
    for n, S, Cn in ((0, 3, 3), (2, 0, 3), (2, 3, 0), (2, 3, 65)):
        assert lib.rmhmc_loo_moments_dev(h, w.data_ptr(), n, S, Cn, out.data_ptr()) == -1 and clean()
    assert lib.rmhmc_loo_moments_dev(h, None, 2, 3, 4, out.data_ptr()) == -1 and lib.rmhmc_loo_moments_dev(h, w.data_ptr(), 2, 3, 4, None) == -1
    # the split and the fit
    cut = np.zeros(4); lmin = np.zeros(4); tl = np.array([5, 5, 5, 5], dtype=np.int64)
    for bad_tl, stride in ((np.array([5, -1, 5, 5], dtype=np.int64), 8), (np.array([5, 9, 5, 5], dtype=np.int64), 8), (tl, 0),
                           (np.array([5, 5, 5, 16385], dtype=np.int64), 16385)):
        assert lib.rmhmc_loo_split_dev(h, w.data_ptr(), 2, 3, 4, ptr(cut), ptr(lmin), ptr(bad_tl, lp), stride, out.data_ptr(), iout.data_ptr(),
                                       out.data_ptr()) == -1 and clean()
        assert lib.rmhmc_loo_fit_dev(h, out.data_ptr(), iout.data_ptr(), ptr(cut), ptr(lmin), ptr(bad_tl, lp), stride, 4, out.data_ptr()) == -1 and clean()
    assert lib.rmhmc_loo_split_dev(h, w.data_ptr(), 2, 3, 4, None, ptr(lmin), ptr(tl, lp), 8, out.data_ptr(), iout.data_ptr(), out.data_ptr()) == -1
    assert lib.rmhmc_loo_split_dev(h, w.data_ptr(), 2, 3, 65, ptr(cut), ptr(lmin), ptr(tl, lp), 8, out.data_ptr(), iout.data_ptr(), out.data_ptr()) == -1
    assert lib.rmhmc_loo_fit_dev(h, out.data_ptr(), iout.data_ptr(), ptr(cut), None, ptr(tl, lp), 8, 4, out.data_ptr()) == -1
    assert lib.rmhmc_loo_fit_dev(h, out.data_ptr(), iout.data_ptr(), ptr(cut), ptr(lmin), ptr(tl, lp), 8, 0, out.data_ptr()) == -1 and clean()
    # the whole run: host outputs
    outs = [np.full(k, -7.0) for k in (15, 12, 6, 3, 3, 3, 3, 3, 3, 6)]
    ints = [np.full(2, -7, dtype=np.int64), np.full(3, -7, dtype=np.int64)]

    def whole(wp, n, S, D, xx, tt, Rn, cpb):
        rc = lib.rmhmc_loo_dev(h, wp, n, S, D, ptr(xx), ptr(tt), Rn, cpb, *[ptr(o) for o in outs], *[ptr(o, lp) for o in ints])
        assert all((o == -7.0).all() for o in outs) and all((o == -7).all() for o in ints)
        return rc
    assert whole(w.data_ptr(), 2, 3, 4, x, half, 3, 0) == -1 and whole(w.data_ptr(), 2, 3, 4, nan_x, t, 3, 0) == -1
    assert whole(w.data_ptr(), 2, 3, 257, wide_x, t, 3, 0) == -4 and whole(w.data_ptr(), 2, 3, 4, x, t, 3, 65) == -1
    assert whole(w.data_ptr(), 2, 3, 4, x, t, 3, -1) == -1 and whole(w.data_ptr(), 2, 3, 4, x, t, 0, 0) == -1 and whole(None, 2, 3, 4, x, t, 3, 0) == -1
    # the binding's own checks, and the library's through it
    for bad in (lambda: ctx.loo_loglik(w.cpu(), x, t), lambda: ctx.loo_loglik(w.float(), x, t), lambda: ctx.loo_loglik(w[0], x, t),
                lambda: ctx.loo_loglik(w, x[:, :3], t), lambda: ctx.loo_loglik(w, x, t[:2]), lambda: ctx.loo(w, x, t[:2]),
                lambda: ctx.loo_split(w, cut[:2], lmin, tl), lambda: ctx.loo_fit(w[0], iout[:6].reshape(2, 3), cut, lmin, tl)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.loo(w, x, half)
    assert e.value.code == -1 and " t " in str(e.value)
    assert (ctx.loo(w, x, t)["draws_used"] == 6).all()                         # the context works on


def test_no_trace_on_the_context(hip):
    """the battery of tests/helpers/context_history.py gives the same bits before and after the calls of this header"""
    spec = H.PATHS["fused"]
    M, D, n = spec[:3]
    XX, t = H.data_of(spec)
    inputs = H.make_inputs(spec)
    w, x, tt = draws(3, 200, D + 2, 20)              # another D than the context's
    with hip.context(M, D, n, flags=spec[3]) as c:
        c.set_data(XX, t, 100.0)
        opts = c.options()
        before = H.battery(c, inputs)
        first = c.loo(dev(w), x, tt)
        pieces(c, w, x, tt)
        with pytest.raises(_capi.RmhmcError):
            c.loo(dev(w), x, tt * 0.5)
        assert c.options() == opts
        after = H.battery(c, inputs)
        second = c.loo(dev(w), x, tt)
    H.assert_same_bits(after, before, "after the loo calls")
    for k in KEYS:
        assert same_bits(first[k], second[k]), k


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_psis_loo_end_to_end(hip):
    """psis_loo on the D = 1 problem of tests/helpers/loo_quad.py with its fixed seeds, against the quadrature: the three conditions of
    tests/test_loo_cpu.py::test_quadrature"""
    x, t = Q.problem()
    r = psis_loo(x, t, n_chains=Q.N_CHAINS, NumOfIterations=Q.N_DRAWS + 100, BurnIn=100, seed=Q.SEED)
    assert (r["draws_used"] == Q.N_CHAINS * Q.N_DRAWS).all() and r["pareto_k"].shape == (Q.ROWS,) and 0.0 <= r["accept"] <= 1.0
    with hip.context(Q.ROWS, 1, Q.N_CHAINS) as c:          # the same sequence by hand
        c.set_data(x, t, Q.ALPHA)
        md = c.phmc_mode()
        c.phmc_set_mass(md["G"])
        st = c.phmc_sample_to(Q.N_DRAWS + 100, 100, L=6, eps=0.5, where="device", device=DEV, samples=True, seed=Q.SEED, theta0=md["w"])
        mine = c.loo(st["samples"], x, t)
        s = st["samples"].cpu().numpy()
        assert same_bits(mine["pareto_k"], r["pareto_k"]) and mine["totals"]["elpd_loo"] == r["elpd_loo"]
        for k in ("elpd_loo", "p_loo", "lppd", "p_waic", "elpd_waic"):
            assert same_bits(mine[k], r["pointwise"][k]), k
        assert (r["k_mid"], r["k_high"]) == (mine["k_mid"], mine["k_high"]) and r["se_elpd_loo"] == mine["totals"]["se_elpd_loo"]
        Q.conditions(lambda v: c.loo(dev(v), x, t)["totals"]["elpd_loo"], r["pareto_k"], s, x, t)
    check_ll(c_ll(hip, s, x, t), s, x, t, "end to end")


def c_ll(hip, s, x, t):
    with hip.context(10, 2, 1) as c:
        return c.loo_loglik(dev(s), x, t).cpu().numpy().reshape(-1, x.shape[0])


def test_zz_report_the_largest_deviations():
    """(runs last in the file) the figures of DESIGN section 8k: the largest ll error over its bound and the largest deviations of the
    fit from the restatement over all shapes of this file"""
    print("largest over this file: " + " ".join("%s %.3e" % kv for kv in _worst.items()))
    assert _worst["ll"] <= 1.0
