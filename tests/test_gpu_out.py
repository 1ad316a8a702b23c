"""The output descriptor of include/rmhmc_out.h on the GPU: every sampler with its samples left in device memory, reduced on the
device, or both, against the sampler's existing *_sample call (bit for bit), the ESS kernel on the same samples (bit for bit), NumPy and
tools.CalculateESS (the project's tolerances: mean / var rtol 1e-12, atol 1e-14; ESS rtol 1e-9).

Shapes: 200 rows, D = 5, 5 chains, 60 iterations of which 23 burn-in: S = 37 is odd, the ESS kernel's half = 18, n is a multiple of
nothing; IWLS again at D = 33 (three column blocks) and Gibbs at D = 17; one case with RMHMC_FLAG_ESS_WRAP (at S = 37 no wrapped lag
is reached before the sums stop, so it checks the flag's plumbing only: the wrap itself is tested in tests/test_gpu_ess_edges.py).  The older entry points
are the same bodies behind a descriptor of their own: what only they allow (rmhmc_sample_stats without a statistic), what they
refuse themselves (no samples_out) and the statistics limit, refused before any sampling work, at n = 3 and n = 5.  Needs an
MI355X: run with  pytest -m gpu."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

from conftest import synthetic_logreg
from riemannhamiltonianmontecarlo_amd import AMH, _capi, experiment

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import out_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

M, N_CH, N_ITER, BURN = 200, 5, 60, 23
S = N_ITER - BURN
SEED = 11
# case -> (sampler, D, context flags, first global chain id)
# (IWLS accepts little at D = 33 on 200 rows: of the chains 0..4 of this seed, chain 2 does not move once in its 37 rows, and a constant
#  series has no ESS to compare - NumPy's is 0/0; the chains 20..24 all move)
CASES = {
    "rmhmc": ("rmhmc", 5, _capi.COMPAT, 0),
    "hmc": ("hmc", 5, 0, 0),
    "mmala": ("mmala", 5, 0, 0),
    "amh": ("amh", 5, 0, 0),
    "iwls": ("iwls", 5, 0, 0),
    "gibbs": ("gibbs", 5, 0, 0),
    "iwls_d33": ("iwls", 33, 0, 20),
    "gibbs_d17": ("gibbs", 17, 0, 0),
    "hmc_wrap": ("hmc", 5, _capi.FLAG_ESS_WRAP, 0),   # S = 37, nfft = 65: the first wrapped lag is 29, never reached (see the docstring)
}
MEAN_TOL = dict(rtol=1e-12, atol=1e-14)   # (tests/test_gpu_bench.py: the device mean against NumPy)
ESS_RTOL = 1e-9                           # (the ESS kernel against tools.CalculateESS)

_runs = {}
_fresh = {}


def _context(hip, D, flags, n=N_CH):
    ctx = hip.context(M, D, n, flags=flags)
    ctx.set_data(*synthetic_logreg(M, D, 3))
    return ctx


def _history_probe(ctx):
    with np.errstate(all="ignore"):
        return ctx.sample(30, 10, seed=4)[:3]


def fresh_probe(hip, D, flags):
    if (D, flags) not in _fresh:
        with _context(hip, D, flags) as ctx:
            _fresh[D, flags] = _history_probe(ctx)
    return _fresh[D, flags]


def runs(hip, case):
    """once per case, on one context: the existing call; the descriptor with device samples only; with everything on the device; with
    everything on the host; then an RMHMC run whose result must not depend on any of that"""
    if case not in _runs:
        sampler, D, flags, first = CASES[case]
        dev = torch.device("cuda", 0)
        kw = dict(seed=SEED, chain_offset=first)
        with _context(hip, D, flags) as ctx, np.errstate(all="ignore"):
            r = dict(existing=R.existing_call(ctx, sampler, N_ITER, BURN, **kw))
            r["ess_kernel"] = ctx.ess(r["existing"]["samples"])
            r["dev"] = ctx.sample_to(sampler, N_ITER, BURN, where="device", device=dev, samples=True, **kw)
            r["dev_all"] = ctx.sample_to(sampler, N_ITER, BURN, where="device", device=dev, samples=True, stats=True, run_mean=True, **kw)
            r["host"] = ctx.sample_to(sampler, N_ITER, BURN, samples=True, stats=True, run_mean=True, **kw)
            r["after"] = _history_probe(ctx)
        _runs[case] = r
    return _runs[case]


def _counters(case):
    return [k for k, _ in _capi.SAMPLERS_TO[CASES[case][0]][1]]


@pytest.mark.parametrize("case", list(CASES))
def test_device_samples_and_counters_equal_the_existing_call(hip, case):
    r = runs(hip, case)
    want = r["existing"]
    assert want["samples"].shape == (N_CH, S, CASES[case][1]) and np.isfinite(want["samples"]).all()
    assert set(r["dev"]) == {"samples", "seconds"} | set(_counters(case))
    for k in ["samples"] + _counters(case):
        assert r["dev"][k].is_cuda
        for mode in ("dev", "dev_all", "host"):
            got = R.host(r[mode][k])
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (mode, k)
    assert all(r[mode]["seconds"] > 0 for mode in ("dev", "dev_all", "host"))


@pytest.mark.parametrize("case", list(CASES))
def test_statistics_equal_the_ess_kernel_numpy_and_the_reference(hip, case):
    r = runs(hip, case)
    x = r["existing"]["samples"]
    nfft = "python" if CASES[case][2] & _capi.FLAG_ESS_WRAP else "matlab"
    h = r["host"]
    moved = [len(np.unique(x[c], axis=0)) for c in range(N_CH)]
    print("%s: distinct rows per chain %s" % (case, moved))
    assert min(moved) > 1                                       # every chain has an ESS
    assert np.array_equal(h["ess"], r["ess_kernel"])            # launch_ess on the same buffer: rmhmc_ess
    for k in ("mean", "var", "ess", "run_mean", "run_ess"):
        assert isinstance(h[k], np.ndarray) and r["dev_all"][k].is_cuda
        assert np.array_equal(R.host(r["dev_all"][k]), h[k]), k
    ref = np.stack([R.ess_ref(x[c], nfft) for c in range(N_CH)])
    err = dict(mean=np.abs(h["mean"] - x.mean(1)).max(), var=np.abs(h["var"] - x.var(1)).max(), ess=np.abs(h["ess"] / ref - 1).max())
    print("%s: mean %.1e var %.1e (abs), ess %.1e (rel)" % (case, err["mean"], err["var"], err["ess"]))
    assert np.allclose(h["mean"], x.mean(1), **MEAN_TOL) and np.allclose(h["var"], x.var(1), **MEAN_TOL)
    assert np.allclose(h["ess"], ref, rtol=ESS_RTOL, atol=0)


@pytest.mark.parametrize("case", list(CASES))
def test_run_mean_and_its_ess(hip, case):
    r = runs(hip, case)
    x = r["existing"]["samples"]
    D = CASES[case][1]
    nfft = "python" if CASES[case][2] & _capi.FLAG_ESS_WRAP else "matlab"
    h = r["host"]
    assert h["run_mean"].shape == (S, D) and h["run_ess"].shape == (D,)
    avg = x.mean(axis=0)                                             # main.py:54
    ref = R.ess_ref(avg, nfft, guard=True)                           # main.py:71
    print("%s: run_mean %.1e (abs), run_ess %.1e (rel)" % (case, np.abs(h["run_mean"] - avg).max(), np.abs(h["run_ess"] / ref - 1).max()))
    assert np.allclose(h["run_mean"], avg, **MEAN_TOL)
    assert np.allclose(h["run_ess"], ref, rtol=ESS_RTOL, atol=0)
    # the definition: chains summed in order, then one division
    acc = np.zeros((S, D))
    for c in range(N_CH):
        acc += x[c]
    assert np.array_equal(h["run_mean"], acc / N_CH)


@pytest.mark.parametrize("case", list(CASES))
def test_context_history(hip, case):
    """as test_limits_and_context_state: an RMHMC run after the *_sample_to calls equals a fresh context's"""
    _, D, flags, _ = CASES[case]
    for a, b in zip(runs(hip, case)["after"], fresh_probe(hip, D, flags)):
        assert np.array_equal(a, b)


def test_ess_dev_with_a_nan_chain(hip):
    x = np.cumsum(np.random.RandomState(5).randn(3, S, 4), axis=1) * 0.3 + np.random.RandomState(6).randn(3, S, 4)
    with _context(hip, 5, 0) as ctx:
        want = ctx.ess(x)
        bad = x.copy(); bad[1] = np.nan
        t = torch.from_numpy(bad).to("cuda:0")
        ess, mean, var = ctx.ess_dev(t)
        assert ess.is_cuda and ess.shape == (3, 4)
        ess, mean, var = ess.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
        assert np.isnan(ess[1]).all() and np.isnan(mean[1]).all() and np.isnan(var[1]).all()
        assert np.array_equal(ess[[0, 2]], want[[0, 2]]) and np.isfinite(want).all()
        assert np.allclose(mean[[0, 2]], x[[0, 2]].mean(1), **MEAN_TOL) and np.allclose(var[[0, 2]], x[[0, 2]].var(1), **MEAN_TOL)
        one = ctx.ess_dev(t[2])[0].cpu().numpy()                     # a single (S, P) series block
        assert np.array_equal(one, want[2:3])
        with pytest.raises(_capi.RmhmcError) as e:
            ctx._ck(ctx.lib.rmhmc_ess_dev(ctx._h, t.data_ptr(), 3, S, 4, None, None, None))
        assert e.value.code == -1


def test_nan_chain_through_sample_to(hip):
    """NaN propagation through a whole *_sample_to call (the mechanism a stopped Gibbs chain relies on; one cannot be had at this size):
    chain 1 of an AMH run starts at NaN, so every proposal of it is rejected and its rows are NaN.  Its statistics are NaN, every row of
    run_mean is NaN and so is run_ess - as NumPy's are - and the other chains are what they are without it."""
    th = np.zeros((N_CH, 5)); th[1] = np.nan
    dev = torch.device("cuda", 0)
    with _context(hip, 5, 0) as ctx, np.errstate(all="ignore"):
        clean = ctx.sample_to("amh", N_ITER, BURN, samples=True, stats=True, run_mean=True, seed=SEED)
        old = ctx.amh_sample(N_ITER, BURN, seed=SEED, theta0=th)
        h = ctx.sample_to("amh", N_ITER, BURN, samples=True, stats=True, run_mean=True, seed=SEED, theta0=th)
        d = ctx.sample_to("amh", N_ITER, BURN, where="device", device=dev, samples=True, stats=True, run_mean=True, seed=SEED, theta0=th)
    x = h["samples"]
    assert np.isnan(x[1]).all() and np.isfinite(x[[0, 2, 3, 4]]).all()
    assert np.array_equal(x, old[0], equal_nan=True) and np.array_equal(h["accepted"], old[1]) and h["accepted"][1] == 0
    for k in ("mean", "var", "ess"):
        assert np.isnan(h[k][1]).all(), k
        assert np.array_equal(h[k][[0, 2, 3, 4]], clean[k][[0, 2, 3, 4]]), k        # a batched AMH chain equals the chain run alone
    assert np.isnan(h["run_mean"]).all() and np.isnan(x.mean(axis=0)).all() and np.isnan(h["run_ess"]).all()
    assert np.isfinite(clean["run_mean"]).all() and np.isfinite(clean["run_ess"]).all()
    for k in ("samples", "mean", "var", "ess", "run_mean", "run_ess", "accepted", "sd"):
        assert np.array_equal(R.host(d[k]), h[k], equal_nan=True), k


def test_sample_to_argument_checks(hip):
    with _context(hip, 5, 0) as ctx:
        with pytest.raises(ValueError, match="device"):
            ctx.sample_to("amh", N_ITER, BURN, where="device", samples=True)
        with pytest.raises(ValueError, match="not a GPU"):
            ctx.sample_to("amh", N_ITER, BURN, where="device", device="cpu", samples=True)
        with pytest.raises(ValueError, match="theta0"):
            ctx.sample_to("gibbs", N_ITER, BURN, samples=True, theta0=np.zeros(5))
        for sampler, kw in (("amh", dict(L=3)), ("mmala", dict(K=2)), ("hmc", dict(compat=False)), ("gibbs", dict(eps=0.1))):
            with pytest.raises(ValueError, match="no run argument"):
                ctx.sample_to(sampler, N_ITER, BURN, samples=True, **kw)
        with pytest.raises(ValueError, match="GPU"):
            ctx.ess_dev(torch.zeros(2, S, 3, dtype=torch.float64))


# the run arguments between burn_in and the descriptor, per entry point
_FRONT = {"rmhmc": (6, 0.5, 4, 0, 0, None), "hmc": (100, 0.14, 0, 0, None), "mmala": (1.0, 0, 0, None), "amh": (0, 0, None),
          "iwls": (1, 0, 0, None), "gibbs": (0, 0)}


@pytest.mark.parametrize("sampler", list(_capi.SAMPLERS_TO))
def test_refusals(hip, sampler):
    name, counters = _capi.SAMPLERS_TO[sampler]
    with _context(hip, 5, CASES[sampler][2]) as ctx:
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.sample_to(sampler, N_ITER, BURN)                     # an empty descriptor
        assert e.value.code == -1
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.sample_to(sampler, N_ITER, BURN, where=7, samples=True)
        assert e.value.code == -1
        # a statistic of 20001 samples per chain: refused at once, nothing run, nothing written
        fn = getattr(hip.lib, name)
        mean = np.full((N_CH, 5), -3.0)
        secs = C.c_double(-7.0)
        for where in (_capi.OUT_HOST, _capi.OUT_DEVICE):
            o = _capi.Out(where=where, mean=mean.ctypes.data)        # (never dereferenced: refused first)
            t0 = time.perf_counter()
            rc = fn(ctx._h, 20001 + BURN, BURN, *_FRONT[sampler], C.byref(o), *([None] * len(counters)), C.cast(C.byref(secs), _capi._dp))
            assert rc == -4 and time.perf_counter() - t0 < 1.0
            assert secs.value == -7.0 and (mean == -3.0).all()
        assert fn(ctx._h, N_ITER, BURN, *_FRONT[sampler], None, *([None] * len(counters)), None) == -1   # NULL descriptor
        # samples alone have no such limit - and the refusals have left the context usable
        got = ctx.sample_to(sampler, N_ITER, BURN, samples=True, seed=SEED)
        assert np.array_equal(got["samples"], runs(hip, sampler)["existing"]["samples"])


# ---- the older entry points: thin wrappers of the same bodies (each builds its own descriptor) ----
_RMHMC_RUN = (6, 0.5, 4, SEED, 0, None)   # L, eps, K, seed, chain_offset, theta0
_secs = lambda s: C.cast(C.byref(s), _capi._dp)  # noqa: E731


def test_sample_stats_without_a_statistic(hip):
    """mean_out, var_out and ess_out all NULL: a descriptor that asks for nothing, which only rmhmc_sample_stats may pass - the sampler
    runs, the counters and the time come back.  Then with the statistics: the write-out of the older call is the timed write_out."""
    n = 3
    with _context(hip, 5, _capi.COMPAT, n=n) as ctx:
        acc = np.full(n, -5, dtype=np.int64); steps = np.full(n, -5, dtype=np.int64); secs = C.c_double(-7.0)
        rc = hip.lib.rmhmc_sample_stats(ctx._h, N_ITER, BURN, *_RMHMC_RUN, None, None, None, _capi._ptr(acc, _capi._lp),
                                        _capi._ptr(steps, _capi._lp), _secs(secs))
        assert rc == 0 and secs.value > 0
        _, want_acc, want_steps, _ = ctx.sample(N_ITER, BURN, seed=SEED)
        assert np.array_equal(acc, want_acc) and np.array_equal(steps, want_steps) and (steps > 0).all()
        st = ctx.sample_stats(N_ITER, BURN, seed=SEED)
        assert np.array_equal(st["accepted"], want_acc) and np.isfinite(st["ess"]).all()
        assert ctx.kernel_time("write_out")[0] > 0


@pytest.mark.parametrize("S_bad", [1, 20001])
def test_sample_stats_limit_is_refused_before_sampling(hip, S_bad):
    """n_iter - burn_in outside 2..20000: RMHMC_ERR_UNSUPPORTED from rmhmc_sample_stats and rmhmc_sample_stats_dev before any sampling
    work - nothing written, the timer untouched, the context as a fresh one's."""
    nd = (N_CH, 5)
    with _context(hip, 5, _capi.COMPAT) as ctx:
        host = [np.full(nd, -3.0) for _ in range(3)] + [np.full(N_CH, -5, dtype=np.int64) for _ in range(2)]
        dev = [torch.full(nd, -3.0, dtype=torch.float64, device="cuda:0") for _ in range(3)] + \
              [torch.full((N_CH,), -5, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        secs = C.c_double(-7.0)
        front = (ctx._h, S_bad + BURN, BURN) + _RMHMC_RUN
        rc = hip.lib.rmhmc_sample_stats(*front, *[_capi._ptr(a) for a in host[:3]], *[_capi._ptr(a, _capi._lp) for a in host[3:]], _secs(secs))
        assert rc == -4 and hip.lib.rmhmc_last_error(ctx._h).decode().startswith("sample_stats:")
        rc = hip.lib.rmhmc_sample_stats_dev(*front, *[t.data_ptr() for t in dev], _secs(secs))
        assert rc == -4 and hip.lib.rmhmc_last_error(ctx._h).decode().startswith("sample_stats_dev:")
        rc = hip.lib.rmhmc_sample_stats(*front, None, None, None, None, None, _secs(secs))      # nothing requested: the same code
        assert rc == -4
        assert secs.value == -7.0
        for a in host + [t.cpu().numpy() for t in dev]:
            assert (a == (-3.0 if a.dtype == np.float64 else -5)).all()
        for a, b in zip(_history_probe(ctx), fresh_probe(hip, 5, _capi.COMPAT)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("sampler", list(_capi.SAMPLERS_TO))
def test_older_calls_need_samples_out(hip, sampler):
    """samples_out NULL: RMHMC_ERR_INVALID, and the message names the entry point that was called"""
    name = _capi.SAMPLERS_TO[sampler][0][:-len("_to")]
    fn = getattr(hip.lib, name)
    with _context(hip, 5, 0, n=3) as ctx:
        rest = len(fn.argtypes) - 3 - len(_FRONT[sampler])            # samples_out, the counters, seconds_out
        assert fn(ctx._h, N_ITER, BURN, *_FRONT[sampler], *([None] * rest)) == -1
        assert hip.lib.rmhmc_last_error(ctx._h).decode().startswith(name[len("rmhmc_"):] + ":")


@pytest.mark.parametrize("sampler", ["iwls", "gibbs"])
def test_d65_is_still_unsupported(hip, sampler):
    with _context(hip, 65, 0, n=2) as ctx:
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.sample_to(sampler, 6, 2, samples=True)
        assert e.value.code == -4 and "D > 64" in str(e.value)


def _check_summary(st, x, nfft):
    """a shim's summary dict against the statistics of the samples x (n, S, D) of the same run"""
    n, s, D = x.shape
    assert st["mean"].shape == st["var"].shape == st["ess"].shape == (n, D)
    assert st["run_mean"].shape == (s, D) and st["run_ess"].shape == (D,)
    assert np.allclose(st["mean"], x.mean(1), **MEAN_TOL) and np.allclose(st["var"], x.var(1), **MEAN_TOL)
    assert np.allclose(st["ess"], np.stack([R.ess_ref(x[c], nfft) for c in range(n)]), rtol=ESS_RTOL, atol=0)
    assert np.allclose(st["run_mean"], x.mean(0), **MEAN_TOL)
    assert np.allclose(st["run_ess"], R.ess_ref(x.mean(0), nfft, guard=True), rtol=ESS_RTOL, atol=0)


def test_shim_summary(hip):
    XX, t = synthetic_logreg(M, 5, 3)
    kw = dict(NumOfIterations=N_ITER, BurnIn=BURN, n_chains=3, seed=SEED, verbose=False)
    x, _, info = AMH(XX, t, return_info=True, **kw)
    for nfft in ("matlab", "python"):
        st, secs, sinfo = AMH(XX, t, summary=True, ess_nfft=nfft, return_info=True, **kw)
        assert set(st) == set(_capi.SUMMARY_KEYS) and secs > 0
        _check_summary(st, x, nfft)
        assert np.array_equal(sinfo["accepted"], info["accepted"]) and np.array_equal(sinfo["ProposalSD"], info["ProposalSD"])
    st1, _ = AMH(XX, t, summary=True, **dict(kw, n_chains=1))       # one chain: the chain axis stays
    assert st1["mean"].shape == st1["ess"].shape == (1, 5) and st1["run_mean"].shape == (S, 5) and st1["run_ess"].shape == (5,)
    assert np.array_equal(AMH(XX, t, **kw)[0], x)                    # the defaults return what they returned


def test_run_experiment_summary(hip):
    XX, t = synthetic_logreg(M, 5, 3)
    kw = dict(sampler="Gibbs", n_experiments=4, batched=True, seed=SEED, max_iter=N_ITER, burn_in=BURN)
    full = experiment.run_experiment(XX, t, **kw)
    assert R.geyer_margin(full["avg_beta_posterior"], "python").min() > 1e-6
    s = experiment.run_experiment(XX, t, summary=True, **kw)
    assert set(s) == set(full) - {"results_beta"}
    assert np.allclose(s["avg_beta_posterior"], full["avg_beta_posterior"], rtol=1e-12, atol=1e-14)
    assert s["ESS"].shape == full["ESS"].shape and s["ESS_per_run"].shape == full["ESS_per_run"].shape
    assert np.allclose(s["ESS"], full["ESS"], rtol=ESS_RTOL, atol=0) and np.allclose(s["ESS_per_run"], full["ESS_per_run"], rtol=ESS_RTOL, atol=0)
    for k in ("Min", "Median", "Mean", "Max"):
        assert np.isclose(s[k], full[k], rtol=ESS_RTOL, atol=0), k
        assert np.isclose(s["per_run"][k], full["per_run"][k], rtol=ESS_RTOL, atol=0), k
