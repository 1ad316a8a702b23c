"""Cross-chain diagnostics of include/rmhmc_diag.h on the GPU: the partial of k_diag_acov / k_diag_reduce / k_diag_m2 and the finished
split R-hat and pooled ESS against the NumPy restatement tests/helpers/diag_ref.py on AR(1) inputs, at the smallest shapes at which each
edge of the kernel can go wrong; determinism; ragged chain splits merged; non-finite, constant and lone series; every sampler through
sample_to(diagnostics=True); the refusals; and multi_gpu.sample_sharded(diagnostics=True) under three gloo ranks on the one GPU.

Tolerances are those of tests/test_gpu_out.py: mean, sum of s2, R-hat rtol 1e-12 / atol 1e-14; lag rows 1e-12 of row 4; ESS rtol 1e-9;
pairs and chains_used equal, every test asserting that the reference's Geyer margin is above 1e-6.  Needs an MI355X: run with
pytest -m gpu."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, synthetic_logreg
from riemannhamiltonianmontecarlo_amd import AMH, _capi, experiment

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import diag_ref as R  # noqa: E402
import sharded_diag_child as child  # noqa: E402
from test_diag_cpu import ESS_RTOL, MEAN_TOL, check_partial  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (seed, n, S, P, max_lag): T = max_lag + 1
SHAPES = {
    "odd_S": (5, 12, 61, 5, 29),                  # the middle row is unused
    "smallest": (6, 3, 4, 1, 1),                  # H = T = 2, one dimension
    "two_blocks": (7, 130, 37, 33, 17),           # crosses a chain block (32), a ragged dimension tile (33 of 64), every lag
    "two_blocks_capped": (7, 130, 37, 33, 5),     # ... and a capped lag
    "two_tiles": (8, 5, 60, 65, 29),              # P beyond one wavefront: a second dimension tile of one column
    "lag_sets": (10, 2, 133, 33, 65),             # 66 lags: more than the 64 that one set of 16 per thread covers at this tile width
    "lds_limit": (9, 2, 20000, 2, 7),             # H = 10000: one dimension per tile, 86 KB of LDS, without the quadratic cost
    # the other tile widths with one lag set ...
    "width_2": (11, 3, 40, 2, 7),
    "width_4": (12, 3, 40, 3, 7),
    "width_16": (13, 3, 40, 9, 7),
    "width_32": (14, 3, 40, 17, 7),
    # ... and every width below 64 with four: every lag of a half series longer than the 4096 / width lags of one set
    "width_32_lag_sets": (15, 1, 300, 17, 149),
    "width_16_lag_sets": (16, 1, 600, 9, 299),
    "width_8_lag_sets": (17, 1, 1100, 5, 549),
    "width_4_lag_sets": (18, 1, 2100, 3, 1049),
    "width_2_lag_sets": (19, 1, 4200, 2, 2099),
    "width_1_lag_sets": (20, 1, 8400, 1, 4199),
}
_inputs = {}


def inputs(name):
    """the AR(1) tensor of a shape and its reference partial, computed once"""
    seed, n, S, P, max_lag = SHAPES[name]
    if (seed, n, S, P) not in _inputs:
        _inputs[seed, n, S, P] = dict(x=R.ar1(seed, n, S, P), parts={})
    e = _inputs[seed, n, S, P]
    if max_lag not in e["parts"]:
        e["parts"][max_lag] = R.partial(e["x"], max_lag + 1)
    return e["x"], e["parts"][max_lag], S // 2, max_lag


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.context(20, 2, 1) as c:      # the diagnostics read samples of any shape: the context only names the GPU and the stream
        yield c


def check_finished(got, part, H):
    ref = R.finish(part, H)
    print("margin %.1e, pairs %d..%d, rhat %.1e ess %.1e (rel)" % (ref["margin"].min(), ref["pairs"].min(), ref["pairs"].max(),
                                                                  np.nanmax(np.abs(got["rhat"] / ref["rhat"] - 1)),
                                                                  np.nanmax(np.abs(got["ess_pooled"] / ref["ess"] - 1))))
    assert (ref["margin"] > 1e-6).all(), ref["margin"]
    assert np.array_equal(got["pairs"], ref["pairs"]) and np.array_equal(got["chains_used"], ref["used"])
    assert np.allclose(got["rhat"], ref["rhat"], equal_nan=True, **MEAN_TOL)
    assert np.allclose(got["ess_pooled"], ref["ess"], rtol=ESS_RTOL, atol=0, equal_nan=True)
    return ref


@pytest.mark.parametrize("name", list(SHAPES))
def test_partial_and_finish_against_numpy(ctx, name):
    x, want, H, max_lag = inputs(name)
    got = ctx.diagnose(torch.from_numpy(x).to(DEV), max_lag)
    assert got["partial"].is_cuda and got["partial"].shape == want.shape
    assert all(isinstance(got[k], np.ndarray) and got[k].shape == (x.shape[2],) for k in _capi.DIAG_KEYS)
    check_partial(got["partial"].cpu().numpy(), want)
    ref = check_finished(got, want, H)
    assert np.isfinite(ref["rhat"]).all() and (ref["used"] == 2 * x.shape[0]).all()


def test_every_lag_is_the_default(ctx):
    x, want, H, max_lag = inputs("odd_S")
    t = torch.from_numpy(x).to(DEV)
    assert max_lag == H - 1
    a, b, c = ctx.diag_partial(t), ctx.diag_partial(t, 0), ctx.diag_partial(t, max_lag)
    assert torch.equal(a, b) and torch.equal(a, c)
    short = ctx.diag_partial(t, 4)                                   # fewer lags: the same rows, cut
    assert short.shape == (4 + 5, 5) and torch.equal(short, a[:9])


def test_same_call_twice_gives_the_same_bits(ctx):
    for name in ("two_blocks", "two_tiles"):
        x, _, _, max_lag = inputs(name)
        t = torch.from_numpy(x).to(DEV)
        a = ctx.diagnose(t, max_lag)
        b = ctx.diagnose(t, max_lag)
        assert torch.equal(a["partial"], b["partial"])
        for k in _capi.DIAG_KEYS:
            assert np.array_equal(a[k], b[k]), k


def test_ragged_chain_splits_merge_to_one_call(ctx):
    x, want, H, max_lag = inputs("two_blocks")
    t = torch.from_numpy(x).to(DEV)
    parts = [ctx.diag_partial(t[a:b], max_lag) for a, b in ((0, 1), (1, 40), (40, 97), (97, 130))]
    got = _capi.diag_finish(parts, H)
    check_partial(got["merged"], want)
    check_finished(got, want, H)
    one = ctx.diag_partial(t, max_lag).cpu().numpy()
    print("merged against one call: %.1e (rel)" % np.abs(got["merged"][1:] / one[1:] - 1).max())


def test_non_finite_constant_and_lone_series(ctx):
    x = R.ar1(3, 4, 20, 3)
    x[:, :, 1] = 2.5                                                 # a constant dimension: W = 0
    x[1, 3, 2] = np.nan                                              # one series of dimension 2 is left out of it, and of it only
    x[2, 15, 0] = np.inf
    want = R.partial(x, 10)
    got = ctx.diagnose(torch.from_numpy(x).to(DEV))
    assert list(got["chains_used"]) == [7, 8, 7]
    check_partial(got["partial"].cpu().numpy()[:, [0, 2]], want[:, [0, 2]])
    check_finished({k: got[k][[0, 2]] for k in _capi.DIAG_KEYS}, want[:, [0, 2]], 10)
    p = got["partial"].cpu().numpy()
    assert p[0, 1] == 8 and p[1, 1] == 2.5 and not p[2:, 1].any()    # centred first: a constant series has no variance at all
    assert np.isnan(got["rhat"][1]) and np.isnan(got["ess_pooled"][1]) and got["pairs"][1] == 0
    # a stopped Gibbs chain: every row from some point on is NaN, so both halves drop out of every dimension
    y = R.ar1(4, 3, 20, 2)
    y[1, 4:] = np.nan
    got = ctx.diagnose(torch.from_numpy(y).to(DEV))
    assert list(got["chains_used"]) == [4, 4]
    check_finished(got, R.partial(y[[0, 2]], 10), 10)
    # fewer than two usable series
    y[2, 12:] = np.nan; y[0, 0, 1] = np.nan
    got = ctx.diagnose(torch.from_numpy(y).to(DEV))
    assert list(got["chains_used"]) == [3, 2] and np.isfinite(got["rhat"]).all()
    y[0, 19] = np.nan
    got = ctx.diagnose(torch.from_numpy(y).to(DEV))
    assert list(got["chains_used"]) == [2, 1] and np.isfinite(got["rhat"][0])
    assert np.isnan(got["rhat"][1]) and np.isnan(got["ess_pooled"][1]) and got["pairs"][1] == 0
    got = ctx.diagnose(torch.from_numpy(np.full((2, 8, 2), np.nan)).to(DEV))
    assert not got["chains_used"].any() and np.isnan(got["rhat"]).all() and not got["partial"].cpu().numpy().any()


def test_refusals_leave_the_context_usable(ctx):
    x, want, H, max_lag = inputs("odd_S")
    t = torch.from_numpy(x).to(DEV)
    part = torch.full((4 + 30, 5), -3.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    f = ctx.lib.rmhmc_diag_partial_dev
    for args, code in (((t.data_ptr(), 12, 3, 5, 0), -4), ((t.data_ptr(), 1, 20001, 5, 0), -4), ((t.data_ptr(), 12, 61, 5, 30), -1),
                       ((t.data_ptr(), 12, 61, 5, -1), -1), ((None, 12, 61, 5, 0), -1), ((t.data_ptr(), 0, 61, 5, 0), -1),
                       ((t.data_ptr(), 12, 61, 0, 0), -1)):
        t0 = time.perf_counter()
        assert f(ctx._h, *args, part.data_ptr()) == code, args[1:]
        assert time.perf_counter() - t0 < 1.0
    assert f(ctx._h, t.data_ptr(), 12, 61, 5, 0, None) == -1
    assert "20000" in _error(ctx, f, t, 20001)
    assert (part == -3.0).all()                                      # nothing was written
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.diag_partial(t[:, :3])
    assert e.value.code == -4
    with pytest.raises(_capi.RmhmcError) as e:
        ctx.diag_partial(t, 30)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="GPU"):
        ctx.diag_partial(torch.zeros(2, 8, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        ctx.diag_partial(torch.zeros(2, 8, 3, device=DEV))
    check_partial(ctx.diag_partial(t).cpu().numpy(), want)           # ... and the context works as before


def _error(ctx, f, t, S):
    f(ctx._h, t.data_ptr(), 1, S, 5, 0, t.data_ptr())
    return ctx.lib.rmhmc_last_error(ctx._h).decode()


# ---- every sampler: sample_to(diagnostics=True), at the shape of tests/test_gpu_out.py -------------------------------------------------
M, D, N_CH, N_ITER, BURN, SEED = 200, 5, 5, 60, 23, 11
S = N_ITER - BURN


def _probe(c):
    with np.errstate(all="ignore"):
        return c.sample(30, 10, seed=4)[:3]


@pytest.mark.parametrize("sampler", list(_capi.SAMPLERS_TO))
def test_sample_to_with_diagnostics(hip, sampler):
    flags = _capi.COMPAT if sampler == "rmhmc" else 0
    XX, t = synthetic_logreg(M, D, 3)
    counters = [k for k, _ in _capi.SAMPLERS_TO[sampler][1]]
    with hip.context(M, D, N_CH, flags=flags) as c, np.errstate(all="ignore"):
        c.set_data(XX, t)
        fresh = _probe(c)
        plain = c.sample_to(sampler, N_ITER, BURN, samples=True, seed=SEED)
        host = c.sample_to(sampler, N_ITER, BURN, samples=True, stats=True, seed=SEED, diagnostics=True)
        dev = c.sample_to(sampler, N_ITER, BURN, where="device", device=DEV, seed=SEED, diagnostics=True, max_lag=6)
        after = _probe(c)
    x = plain["samples"]
    assert x.shape == (N_CH, S, D) and np.isfinite(x).all()
    assert set(host) == set(plain) | {"mean", "var", "ess", "diag_partial"} | set(_capi.DIAG_KEYS)
    assert set(dev) == (set(plain) - {"samples"}) | {"diag_partial"} | set(_capi.DIAG_KEYS)      # the samples only where asked
    for k in ["samples"] + counters:
        assert isinstance(host[k], np.ndarray) and host[k].dtype == plain[k].dtype and np.array_equal(host[k], plain[k]), k
    for k in counters:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), plain[k]), k
    assert np.allclose(host["mean"], x.mean(1), **MEAN_TOL)
    for r, max_lag in ((host, None), (dev, 6)):
        H, T = R.lags(S, max_lag)
        want = R.partial(x, T)
        assert r["diag_partial"].is_cuda and all(isinstance(r[k], np.ndarray) for k in _capi.DIAG_KEYS)
        check_partial(r["diag_partial"].cpu().numpy(), want)
        check_finished(r, want, H)
    for a, b in zip(after, fresh):                                   # the chain state of the context was not touched
        assert np.array_equal(a, b)


def test_sample_to_refuses_before_sampling(hip):
    with hip.context(M, D, N_CH) as c:
        c.set_data(*synthetic_logreg(M, D, 3))
        t0 = time.perf_counter()
        with pytest.raises(ValueError, match="4 <= S"):
            c.sample_to("hmc", 10 ** 6, 10 ** 6 - 3, diagnostics=True)
        with pytest.raises(ValueError, match="max_lag"):
            c.sample_to("hmc", N_ITER, BURN, diagnostics=True, max_lag=S // 2)
        assert time.perf_counter() - t0 < 1.0


def test_shim_and_run_experiment(hip):
    XX, t = synthetic_logreg(M, D, 3)
    kw = dict(NumOfIterations=N_ITER, BurnIn=BURN, n_chains=4, seed=SEED, verbose=False)
    x, _, info = AMH(XX, t, return_info=True, **kw)
    assert "diagnostics" not in info
    xd, _, dinfo = AMH(XX, t, return_info=True, diagnostics=True, **kw)
    assert np.array_equal(xd, x) and np.array_equal(dinfo["accepted"], info["accepted"]) and np.array_equal(dinfo["ProposalSD"], info["ProposalSD"])
    assert set(dinfo) == set(info) | {"diagnostics"} and set(dinfo["diagnostics"]) == set(_capi.DIAG_KEYS)
    want = R.partial(x, S // 2)
    check_finished(dinfo["diagnostics"], want, S // 2)
    st, _, sinfo = AMH(XX, t, return_info=True, diagnostics=True, summary=True, max_lag=6, **kw)
    assert set(st) == set(_capi.SUMMARY_KEYS) and np.allclose(st["mean"], x.mean(1), **MEAN_TOL)
    check_finished(sinfo["diagnostics"], R.partial(x, 7), S // 2)
    ekw = dict(sampler="AMH", n_experiments=4, batched=True, seed=SEED, NumOfIterations=N_ITER, BurnIn=BURN)
    full = experiment.run_experiment(XX, t, **ekw)
    res = experiment.run_experiment(XX, t, diagnostics=True, **ekw)
    assert set(res) == set(full) | set(_capi.DIAG_KEYS) and np.array_equal(res["results_beta"], full["results_beta"])
    check_finished(res, want, S // 2)
    res = experiment.run_experiment(XX, t, diagnostics=True, summary=True, **ekw)
    check_finished(res, want, S // 2)


# ---- sharded: three gloo ranks on the one GPU ---------------------------------------------------------------------------------------------
def test_sharded_diagnostics_under_gloo(hip, tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "r0.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="3", LOCAL_RANK="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "helpers", "sharded_diag_child.py"), out], cwd=ROOT,
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(3)]
    try:
        logs = [p.communicate(timeout=240)[0] for p in procs]       # every child under a limit of its own
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):                                    # ... and every exit status checked
        assert p.returncode == 0, (r, logs[r][-3000:])
    g = np.load(out)
    XX, t = synthetic_logreg(child.M, child.D, 3)
    H = (child.N_ITER - child.BURN) // 2
    for n_chains, counts in child.CHAINS:
        for name in child.SAMPLERS:
            key = name.lower()
            with hip.context(child.M, child.D, n_chains, flags=_capi.COMPAT if name == "RMHMC" else 0) as c, np.errstate(all="ignore"):
                c.set_data(XX, t)
                one = c.sample_to(key, child.N_ITER, child.BURN, where="device", device=DEV, samples=True, stats=True, seed=child.SEED)
                dg = c.diagnose(one["samples"])
            pre = "%s.%d." % (name, n_chains)
            assert list(g[pre + "counts"]) == counts
            assert np.array_equal(g[pre + "accepted"], one["accepted"].cpu().numpy())
            assert np.array_equal(g[pre + "mean"], one["mean"].cpu().numpy())
            want = R.partial(one["samples"].cpu().numpy(), H)
            got = {k: g[pre + k] for k in _capi.DIAG_KEYS}
            check_finished(got, want, H)                             # against NumPy, and against the one-rank call:
            assert np.array_equal(got["pairs"], dg["pairs"]) and np.array_equal(got["chains_used"], dg["chains_used"])
            assert (got["chains_used"] == 2 * n_chains).all()
            assert np.allclose(got["rhat"], dg["rhat"], **MEAN_TOL) and np.allclose(got["ess_pooled"], dg["ess_pooled"], rtol=ESS_RTOL, atol=0)
