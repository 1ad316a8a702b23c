"""GPU tests of the warm-up of the fixed-metric HMC sampler (include/rmhmc_adapt.h): the pooled covariance kernels of csrc/adapt.hip.h
against a two-pass reference in np.longdouble, and rmhmc_phmc_warmup against the composition of the public pieces run from Python
(bit for bit) and, statistically, against the NumPy restatement tests/helpers/adapt_ref.py.

Covariance tolerance, per entry: 4 N 2^-53 sum_r |xc_ri| |xc_rj| with xc the rows centred about the long-double mean - the
forward-error bound of a dot product of length N, the factor 4 for the centring and the order of the sums.  Mean: N 2^-53 sum |x|.
Inputs: Gaussian rows with a dense covariance of unit scale and column means from 1e-8 to 1e8 in absolute value."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from riemannhamiltonianmontecarlo_amd import PHMC, _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adapt_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
DEV = torch.device("cuda", 0)
RB = _capi.COV_ROWS            # the smallest row block of the kernels


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def rows(n, S, P, mean_scale=1e8, seed=0):
    """[n][S][P] Gaussian draws, dense covariance of unit scale, column means +-mean_scale * 10^-16 .. mean_scale (log-spaced)"""
    rs = np.random.RandomState(1000 * P + 10 * n + S + seed)
    mix = rs.randn(P, P) / np.sqrt(P) + np.eye(P)
    mean = mean_scale * 10.0 ** (-16.0 * rs.permutation(P) / max(P - 1, 1)) * rs.choice([-1.0, 1.0], P)
    return (rs.randn(n * S, P) @ mix.T + mean).reshape(n, S, P)


def check(got, x, what=""):
    """a finished result (mean, cov or merged partial, rows_used) against the long-double reference of x; returns the worst ratios"""
    m, mean, C, S = A.partial_longdouble(x)
    assert got["rows_used"] == m, what
    merged = got["merged"]
    assert (merged[0] == m).all() and np.array_equal(merged[2:], merged[2:].T), what
    tol_c = 4.0 * m * U * S
    err_c = np.abs(merged[2:].astype(np.longdouble) - C)
    assert (err_c <= tol_c).all(), what
    finite = np.isfinite(x.reshape(-1, x.shape[-1])).all(axis=1)
    tol_m = m * U * np.abs(x.reshape(-1, x.shape[-1])[finite]).astype(np.longdouble).sum(axis=0) / max(m, 1)
    err_m = np.abs(merged[1].astype(np.longdouble) - mean)
    assert (err_m <= tol_m).all(), what
    if m >= 2:
        assert same_bits(got["cov"], merged[2:] / (m - 1.0)) and same_bits(got["mean"], merged[1])
    else:
        assert np.isnan(got["cov"]).all()
    rc = float((err_c[tol_c > 0] / tol_c[tol_c > 0]).max()) if (tol_c > 0).any() else 0.0
    rm = float((err_m[tol_m > 0] / tol_m[tol_m > 0]).max()) if (tol_m > 0).any() else 0.0
    return rc, rm


def finished(ctx, x):
    part = ctx.cov_partial(torch.from_numpy(x).to(DEV))
    out = _capi.cov_finish([part])
    out["partial"] = part.cpu().numpy()
    assert same_bits(out["partial"], out["merged"])          # one partial: the merge is the identity
    return out


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.context(10, 2, 1) as c:     # the covariance calls use the context for its device and stream only
        yield c


# ---- 1. the covariance kernels at every tile, block and padding edge ----------------------------------------------------------------------
PS = [1, 5, 16, 17, 64, 65, 130, 256]
SHAPES = [(1, 1), (1, 2), (3, 1), (1, 4), (5, 1), (17, 3), (2, 33),                      # fewer rows than one MFMA takes, ragged groups of 4
          (1, RB - 1), (RB, 1), (1, RB + 1), (8, 125)]                                   # one row block - 1, one, one + 1, several


@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("P", PS)
def test_covariance_matches_long_double(ctx, P, n, S):
    x = rows(n, S, P)
    got = finished(ctx, x)
    rc, rm = check(got, x)
    print("P %d, n %d, S %d: worst error / bound: covariance %.3f, mean %.3f" % (P, n, S, rc, rm))
    again = ctx.cov_partial(torch.from_numpy(x).to(DEV)).cpu().numpy()                   # the same call, the same bits
    assert same_bits(again, got["partial"])
    pc = ctx.pooled_cov(torch.from_numpy(x).to(DEV))
    assert same_bits(pc["cov"], got["cov"]) and same_bits(pc["mean"], got["mean"]) and pc["rows_used"] == n * S
    assert tuple(pc["partial"].shape) == (2 + P, P)


@pytest.mark.parametrize("P,n,S", [(5, 3, 7), (17, 2, 33), (65, 1, RB + 1), (256, 8, 125)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_row_is_left_out(ctx, P, n, S, bad):
    x = rows(n, S, P)
    whole = finished(ctx, x)
    y = x.copy()
    c, s, d = n - 1, S // 2, P // 3
    y[c, s, d] = bad
    got = finished(ctx, y)
    assert got["rows_used"] == whole["rows_used"] - 1 == n * S - 1
    check(got, y, "planted %r" % bad)                       # the reference of the rows that are left: nothing else has changed


def test_all_rows_non_finite(ctx):
    x = np.full((3, 5, 7), np.nan)
    x[1] = np.inf
    got = finished(ctx, x)
    assert got["rows_used"] == 0 and np.isnan(got["cov"]).all() and (got["merged"] == 0).all()
    one = rows(1, 1, 7)
    merged = _capi.cov_finish([got["partial"], finished(ctx, one)["partial"]])          # the identity of the merge
    assert merged["rows_used"] == 1 and same_bits(merged["mean"], one[0, 0]) and np.isnan(merged["cov"]).all()


@pytest.mark.parametrize("P,n,S", [(17, 9, 57), (130, 6, 100)])
def test_split_by_chains_merges_to_the_whole(ctx, P, n, S):
    """Three shards of the chains, merged on the host, against the long-double reference of all rows, to the bound of the whole.
    Column means up to 1e3 here, not 1e8: a partial carries its mean as a double, so a merge sees the means of its shards rounded to
    |mean| 2^-53 and the merged C an error of 2 |delta_i| |mean_j| 2^-53 m_a m_b / m on top (include/rmhmc_adapt.h).  With shards of
    N / 3 rows of unit spread that is about |mean| 2^-53 sqrt(N) against a bound of 4 N^2 2^-53: inside it for |mean| << 4 N^1.5,
    i.e. 4e4 at N = 500, and outside it by orders of magnitude at 1e8, whatever the kernels do."""
    x = rows(n, S, P, mean_scale=1e3)
    k = n // 3
    parts = [ctx.cov_partial(torch.from_numpy(np.ascontiguousarray(x[a:b])).to(DEV)) for a, b in ((0, k), (k, 2 * k), (2 * k, n))]
    got = _capi.cov_finish(parts)
    rc, rm = check(got, x, "3-way split")
    whole = finished(ctx, x)
    print("P %d: 3-way split, worst error / bound: covariance %.3f, mean %.3f; against the one-piece call %.2e relative"
          % (P, rc, rm, np.abs(got["cov"] - whole["cov"]).max() / np.abs(whole["cov"]).max()))


def test_covariance_refusals(ctx):
    x = torch.zeros((2, 3, 4), dtype=torch.float64, device=DEV)
    part = torch.zeros((6, 4), dtype=torch.float64, device=DEV)
    lib, h = ctx.lib, ctx._h
    for args, code in (((None, 2, 3, 4, part.data_ptr()), -1), ((x.data_ptr(), 2, 3, 4, None), -1), ((x.data_ptr(), 0, 3, 4, part.data_ptr()), -1),
                       ((x.data_ptr(), 2, 0, 4, part.data_ptr()), -1), ((x.data_ptr(), 2, 3, 0, part.data_ptr()), -1),
                       ((x.data_ptr(), 2, 3, 257, part.data_ptr()), -4)):
        assert lib.rmhmc_cov_partial_dev(h, *args) == code, args
    assert lib.rmhmc_cov_partial_dev(None, x.data_ptr(), 2, 3, 4, part.data_ptr()) == -1
    with pytest.raises(ValueError):
        ctx.cov_partial(torch.zeros((2, 3, 4), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ctx.cov_partial(torch.zeros((2, 3, 4), dtype=torch.float64))
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.cov_partial(torch.zeros((1, 2, 257), dtype=torch.float64, device=DEV))
    assert e.value.code == -4
    with pytest.raises(ValueError):
        _capi.cov_finish([np.zeros((5, 4))])


# ---- 2. the warm-up is the composition of the public pieces --------------------------------------------------------------------------------
DA = dict(delta=0.8, gamma=0.05, t0=10.0, kappa=0.75)


def compose(ctx, win_len, win_kind, L, eps0, min_rows, seed, theta0=None, chain_offset=0):
    """rmhmc_phmc_warmup restated with the public calls"""
    n, D = ctx.n, ctx.D
    state = _capi.adapt_init(eps0)
    eps, eps_bar, theta, mass = eps0, eps0, theta0, None
    running = np.zeros((2 + D, D))
    eps_trace, acc_trace, updated = [], [], []
    for w, (K, kind) in enumerate(zip(win_len, win_kind)):
        r = ctx.phmc_sample_to(K, 0, L=L, eps=eps, where="device", device=DEV, samples=True, seed=(seed + 1 + w) % 2 ** 64,
                               chain_offset=chain_offset, theta0=theta)
        theta = r["samples"][:, -1, :].cpu().numpy()
        a = int(r["accepted"].cpu().numpy().sum()) / (n * K)
        eps_trace.append(eps); acc_trace.append(a); updated.append(0)
        eps, eps_bar = _capi.adapt_step(state, a, **DA)
        if kind != 1:
            continue
        f = _capi.cov_finish([running, ctx.cov_partial(r["samples"])])
        running = f["merged"]
        if f["rows_used"] < min_rows:
            continue
        new = _capi.adapt_mass(f["cov"], f["rows_used"])
        try:
            if new is None:
                raise _capi.RmhmcError(-1, "refused")
            ctx.phmc_set_mass(new)
        except _capi.RmhmcError:
            updated[-1] = -1
            continue
        mass = new
        running = np.zeros_like(running)
        state = _capi.adapt_init(eps, 1.0)
        updated[-1] = 1
    return dict(step_size=eps_bar, mass=mass, theta=theta, eps_trace=np.array(eps_trace), accept_trace=np.array(acc_trace),
                mass_updated=np.array(updated, dtype=np.int32))


def assert_same_warmup(a, b):
    assert a["step_size"] == b["step_size"]
    for k in ("theta", "eps_trace", "accept_trace", "mass_updated"):
        assert same_bits(a[k], b[k]), k
    assert (a["mass"] is None) == (b["mass"] is None) and (a["mass"] is None or same_bits(a["mass"], b["mass"]))


WINDOWS = ([8] * 6, [0, 1, 1, 1, 1, 0])


@pytest.mark.parametrize("opts", [None, {"graph": 0, "sorted": 0}])
@pytest.mark.parametrize("M,D,n", [(300, 20, 64), (250, 150, 16)])
def test_warmup_is_the_composition_of_its_pieces(hip, M, D, n, opts):
    XX, t = synthetic_logreg(M, D, 1)
    min_rows = 2 * 8 * n                                    # two windows' rows: the mass is updated after windows 2 and 4
    out = []
    for run in ("call", "pieces", "call again"):
        with hip.context(M, D, n, options=opts) as c:       # a fresh context each
            c.set_data(XX, t)
            c.phmc_set_mass(None)
            if run == "pieces":
                out.append(compose(c, *WINDOWS, L=6, eps0=0.1, min_rows=min_rows, seed=11, chain_offset=5))
            else:
                out.append(c.phmc_warmup(*WINDOWS, L=6, eps0=0.1, min_rows=min_rows, seed=11, chain_offset=5))
                assert out[-1].pop("seconds") > 0
            after = c.phmc_sample_to(5, 1, L=6, eps=out[-1]["step_size"], seed=3, samples=True, theta0=out[-1]["theta"])
            out[-1]["after"] = after["samples"]             # the context is left with the final mass
    assert out[0]["mass_updated"].tolist() == [0, 0, 1, 0, 1, 0]
    # (window 1 runs at about 10 eps0, where dual averaging starts its search, and may accept nothing)
    assert np.isfinite(out[0]["theta"]).all() and out[0]["accept_trace"].max() > 0.5 and len(set(out[0]["eps_trace"])) == 6
    assert_same_warmup(out[0], out[1])
    assert_same_warmup(out[0], out[2])
    assert same_bits(out[0]["after"], out[1]["after"]) and same_bits(out[0]["after"], out[2]["after"])


def test_warmup_leaves_no_trace_on_the_context(hip):
    """the property of tests/test_gpu_phmc.py::test_no_trace_on_the_context with a warm-up interleaved"""
    M, D, n = 300, 20, 6
    XX, t = synthetic_logreg(M, D, 1)

    def others(c):
        return (c.hmc_sample(12, 4, L=5, eps=0.05, seed=1)[:3], c.sample(8, 3, seed=2)[:3], c.mmala_sample(8, 3, seed=3)[:2])

    def warm(c):
        c.phmc_set_mass(None)
        r = c.phmc_warmup([6] * 4, [0, 1, 1, 0], L=5, eps0=0.1, min_rows=30, seed=4)
        r.pop("seconds")
        return r

    with hip.context(M, D, n) as c:
        c.set_data(XX, t)
        opts = c.options()
        first = others(c)
        warm(c)
        assert c.options() == opts
        second = others(c)
        mine = warm(c)
        assert c.options() == opts
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert same_bits(x, y)
    with hip.context(M, D, n) as c:
        c.set_data(XX, t)
        assert_same_warmup(mine, warm(c))
    assert (mine["mass_updated"] == 1).sum() >= 1


def test_refused_covariance_keeps_the_mass(hip):
    M, D = 200, 6
    XX, t = synthetic_logreg(M, D, 2)
    G = A.phmc_ref.metric(XX, np.zeros(D))
    # n K < 2 rows: one chain, windows of one iteration, min_rows = 1: every kind-1 window tries a covariance of one row and is refused
    with hip.context(M, D, 1) as c:
        c.set_data(XX, t)
        c.phmc_set_mass(G)
        before = c.phmc_sample_to(6, 1, L=4, eps=0.3, seed=9, samples=True)["samples"]
        r = c.phmc_warmup([1] * 3, [0, 1, 0], L=4, eps0=0.3, min_rows=1, seed=2)
        assert r["mass_updated"].tolist() == [0, -1, 0] and r["mass"] is None and np.isfinite(r["theta"]).all()
        r3 = c.phmc_warmup([1] * 4, [0, 1, 1, 0], L=4, eps0=0.3, min_rows=3, seed=2)                        # never enough rows: not tried
        assert r3["mass_updated"].tolist() == [0, 0, 0, 0] and r3["mass"] is None
        assert same_bits(c.phmc_sample_to(6, 1, L=4, eps=0.3, seed=9, samples=True)["samples"], before)     # G is still the mass
        # the refused window's row stays in the pool: the next window makes it two rows, whose shrunk covariance is positive definite
        r2 = c.phmc_warmup([1] * 4, [0, 1, 1, 0], L=4, eps0=0.3, min_rows=1, seed=2)
        assert r2["mass_updated"].tolist() == [0, -1, 1, 0] and np.isfinite(r2["mass"]).all() and same_bits(r2["eps_trace"][:2], r["eps_trace"][:2])
    # a chain pinned at a non-finite start: its rows are NaN and drop out of the pool; alone, it leaves the pool empty
    with hip.context(M, D, 1) as c:
        c.set_data(XX, t)
        c.phmc_set_mass(G)
        r = c.phmc_warmup([3] * 3, [1, 1, 1], L=4, eps0=0.3, min_rows=1, seed=2, theta0=np.full((1, D), np.nan))
        assert r["mass_updated"].tolist() == [0, 0, 0] and r["mass"] is None and (r["accept_trace"] == 0).all() and np.isnan(r["theta"]).all()
        assert same_bits(c.phmc_sample_to(6, 1, L=4, eps=0.3, seed=9, samples=True)["samples"], before)
    with hip.context(M, D, 5) as c:
        c.set_data(XX, t)
        c.phmc_set_mass(G)
        th = np.zeros((5, D)); th[3] = np.inf
        r = c.phmc_warmup([4] * 3, [1, 1, 1], L=4, eps0=0.3, min_rows=16, seed=2, theta0=th)
        assert r["mass_updated"].tolist() == [1, 1, 1]      # 16 rows a window from the four chains that move
        assert np.isfinite(r["theta"][[0, 1, 2, 4]]).all() and np.isinf(r["theta"][3]).all() and np.isfinite(r["mass"]).all()


def test_warmup_refusals(hip):
    M, D, n = 60, 3, 2
    XX, t = synthetic_logreg(M, D, 1)
    with hip.context(M, D, n) as c:
        c.set_data(XX, t)
        with pytest.raises(_capi.RmhmcError) as e:
            c.phmc_warmup([2, 2, 2], [0, 1, 0])
        assert e.value.code == -1 and "rmhmc_phmc_set_mass" in str(e.value)
        c.phmc_set_mass(None)
        for kw in (dict(win_len=[2, 0, 2]), dict(win_kind=[0, 2, 0]), dict(L=0), dict(eps0=0.0), dict(eps0=np.inf), dict(min_rows=0)):
            args = dict(win_len=[2, 2, 2], win_kind=[0, 1, 0])
            args.update(kw)
            with pytest.raises(_capi.RmhmcError) as e:
                c.phmc_warmup(**args)
            assert e.value.code == -1, kw
        with pytest.raises(ValueError):
            c.phmc_warmup([2, 2], [0, 1, 0])


# ---- 3. the right distribution, and the shim -------------------------------------------------------------------------------------------------
# |post-warm-up acceptance - 0.8| of the NumPy restatement (pima, 64 chains, warmup 300, then 100 iterations), seeds 0..7, as printed by
# tests/test_adapt_cpu.py::test_restated_warmup_adapts (acceptances 0.805 .. 0.831, adapted eps 0.879 .. 0.922)
RESTATED = (0.0053, 0.0180, 0.0217, 0.0183, 0.0309, 0.0205, 0.0252, 0.0180)


def test_warmup_statistics(hip):
    """pima, 1024 chains, identity mass, eps0 = 0.5, warmup = 300, then 200 iterations.  The band of |acceptance - 0.8| is twice the
    largest deviation the NumPy restatement showed over its 8 seeds (tests/test_adapt_cpu.py::test_restated_warmup_adapts; the factor
    for the different random streams): RESTATED above, largest 0.0309, band 0.0618; the figures are in DESIGN section 8f too.
    Measured on an MI355X: adapted eps 0.8984, acceptance 0.8212 (|a - 0.8| = 0.0212), 9 mass updates, max split R-hat 1.0008, mean
    differences at most 0.34 of their bound.  The posterior means agree with a
    mass = "mode" run within five standard errors, the criterion of tests/test_gpu_phmc.py::test_same_posterior_as_rmhmc."""
    d = np.load(os.path.join(GOLDEN, "data_pima.npz"))
    XX, t = d["XX"], d["t"]
    kw = dict(NumOfIterations=200, BurnIn=0, n_chains=1024, seed=23, verbose=False, summary=True, diagnostics=True, return_info=True)
    sw, _, iw = PHMC(XX, t, mass="identity", StepSize=0.5, warmup=300, **kw)
    sm, _, im = PHMC(XX, t, NumOfIterations=300, BurnIn=100, mass="mode", **{k: v for k, v in kw.items() if k not in ("NumOfIterations", "BurnIn")})
    acc = iw["accepted"].sum() / (1024 * 200.0)
    band = 2.0 * max(RESTATED)
    print("adapted eps %.4f, post-warm-up acceptance %.4f (|a - 0.8| = %.4f, band %.4f), mass updates %d, max rhat %.4f"
          % (iw["step_size"], acc, abs(acc - 0.8), band, (iw["warmup"]["mass_updated"] == 1).sum(), iw["diagnostics"]["rhat"].max()))
    assert abs(acc - 0.8) <= band
    stat = []
    for s, info in ((sw, iw), (sm, im)):
        assert all(np.isfinite(s[k]).all() for k in ("mean", "var", "ess", "run_mean"))
        stat.append((s["mean"].mean(axis=0), s["var"].mean(axis=0) + s["mean"].var(axis=0), info["diagnostics"]["ess_pooled"]))
    (m1, v1, e1), (m2, v2, e2) = stat
    bound = 5.0 * np.sqrt(v1 / e1 + v2 / e2)
    print("mean difference / bound:", np.abs(m1 - m2) / bound)
    assert (np.abs(m1 - m2) <= bound).all()


def test_shim_with_and_without_warmup(hip):
    XX, t = synthetic_logreg(150, 10, 4)
    kw = dict(NumOfIterations=30, BurnIn=10, NumOfLeapFrogSteps=7, StepSize=0.03, n_chains=48, seed=12, verbose=False, return_info=True)
    w0, _, i0 = PHMC(XX, t, **kw)
    w1, _, i1 = PHMC(XX, t, warmup=0, target_accept=0.6, window=7, **kw)         # warmup = 0: today's call, bit for bit
    assert same_bits(w0, w1) and set(i0) == set(i1) == {"accepted", "leapfrog_steps", "seed", "mode", "mass", "newton_iters"}
    for k in i0:
        assert same_bits(i0[k], i1[k]) if isinstance(i0[k], np.ndarray) else i0[k] == i1[k], k
    w2, _, i2 = PHMC(XX, t, mass="identity", warmup=300, **kw)
    assert set(i2) == set(i0) | {"step_size", "warmup"} and w2.shape == w0.shape and np.isfinite(w2).all()
    wu = i2["warmup"]
    assert set(wu) == {"eps_trace", "accept_trace", "mass_updated", "seconds"} and all(len(wu[k]) == 12 for k in ("eps_trace", "accept_trace", "mass_updated"))
    assert wu["eps_trace"][0] == 0.03 and i2["step_size"] != 0.03 and (wu["mass_updated"] == 1).sum() >= 1
    assert wu["mass_updated"][:2].tolist() == [0, 0] and wu["mass_updated"][-1] == 0
    # the adapted mass and step size are the ones a direct call returns, and the ones the sampling run used
    length, kind = _capi.adapt_schedule(300, 25)
    with hip.context(150, 10, 48) as c:
        c.set_data(XX, t)
        c.phmc_set_mass(None)
        r = c.phmc_warmup(length, kind, L=7, eps0=0.03, seed=12)
        assert same_bits(r["mass"], i2["mass"]) and r["step_size"] == i2["step_size"] and same_bits(r["eps_trace"], wu["eps_trace"])
        s = c.phmc_sample_to(30, 10, L=7, eps=r["step_size"], seed=12, theta0=r["theta"], samples=True)
    assert same_bits(s["samples"], w2) and same_bits(s["accepted"], i2["accepted"])
