"""IWLS Metropolis-Hastings on the MI355X (include/rmhmc_iwls.h, csrc/iwls.hip.h): replays of the reference's own proposals, the Philox
sampler against the NumPy restatement of tests/test_iwls_cpu.py in both modes and on both assembly paths, chain independence, the
reference's truncation, agreement in distribution with the RMHMC sampler, limits, and the Python surface."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from riemannhamiltonianmontecarlo_amd import RMHMC, _capi, experiment, iwls
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_iwls_cpu import IWLS_TAPES, iwls_numpy, load_iwls_tape, philox_iwls_draws

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sampler_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("name", IWLS_TAPES)
def test_replay_matches_reference_tape(hip, name):
    XX, t, g = load_iwls_tape(name)
    T = int(g["n_iter"])
    M, D = XX.shape
    n = 2   # the same tape in two chains
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        r = ctx.iwls_replay(np.broadcast_to(g["w_prop"], (n, T, D)), np.broadcast_to(g["u"], (n, T)), compat=True)
    nan = np.isnan(g["ratio"])
    scale = np.maximum(np.abs(np.where(nan, 0.0, g["ratio"])), np.max(np.abs(g["ljl"])))
    for c in range(n):
        np.testing.assert_array_equal(r["accepted"][c], g["accepted"] != 0)
        np.testing.assert_array_equal(r["u_read"][c], ~np.isnan(g["u"]))       # u consumed exactly where the reference drew one
        np.testing.assert_array_equal(r["saturated"][c], nan)                   # the reference's 0/0 is the saturation rule
        np.testing.assert_array_equal(r["w"][c], g["w"])
        np.testing.assert_allclose(r["ljl"][c], g["ljl"], rtol=1e-11)
        assert _rel(r["mean"][c], g["mean"]) <= 1e-9
        np.testing.assert_array_equal(np.isnan(r["ratio"][c]), nan)
        assert np.all(np.abs(r["ratio"][c][~nan] - g["ratio"][~nan]) <= 1e-9 * scale[~nan])


def _sample_vs_numpy(hip, XX, t, n, T, B, seed, compat, flags=0, ref=None):
    """ref: the restatement's run where the caller shares it with other tests (tests/helpers/sampler_edges.py)"""
    M, D = XX.shape
    with hip.context(M, D, n, flags=flags) as ctx:
        ctx.set_data(XX, t)
        if flags & _capi.FLAG_INT8_METRIC:     # the assembly really is the int8 one: no certificate has sent the data to the fp64 kernels
            info = ctx.device_info().split("; options:")[0]
            assert "int8 metric path %d slices: active" % ((flags >> 12) & 7) in info, info
        smp, acc, sat, _ = ctx.iwls_sample(T, B, compat=compat, seed=seed)
    if ref is None:
        ref = iwls_numpy(XX, t, T, philox_iwls_draws(seed, np.arange(n), D), n=n, compat=compat)
    np.testing.assert_array_equal(acc, ref["accepted"].sum(axis=1))
    np.testing.assert_array_equal(sat, ref["saturated"].sum(axis=1))
    assert _rel(smp, ref["w"][:, B:]) <= 1e-9
    return acc, sat


@pytest.mark.parametrize("compat", [True, False])
def test_sample_matches_numpy_philox_australian(hip, compat):
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    acc, sat = _sample_vs_numpy(hip, d["XX"], d["t"], 1, 300, 150, 1234, compat)
    assert acc[0] > 30 and (sat[0] > 0) == compat


@pytest.mark.parametrize("compat", [True, False])
def test_sample_matches_numpy_philox_64_chains(hip, compat):
    XX, t = synthetic_logreg(5000, 32, 11)
    _sample_vs_numpy(hip, XX, t, 64, 30, 15, 99, compat)


@pytest.mark.parametrize("compat", [True, False])
def test_sample_matches_numpy_philox_d64(hip, compat):
    XX, t = synthetic_logreg(3000, 64, 12)
    _sample_vs_numpy(hip, XX, t, 4, 24, 12, 7, compat)


@pytest.mark.parametrize("compat", [True, False])
def test_sample_matches_numpy_philox_int8_metric(hip, compat):
    """the assembly on the int8 matrix cores (6 exact byte slices) behind the same sampler"""
    d = np.load(os.path.join(GOLDEN, "data_german.npz"))
    _sample_vs_numpy(hip, d["XX"], d["t"], 4, 60, 30, 5, compat, flags=_capi.int8_metric_flags(6))


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("case", E.IWLS_EDGE_CASES)
def test_sample_matches_numpy_philox_block_counts_and_edges(hip, case, compat):
    """the block counts and edges no other case runs (tests/helpers/sampler_edges.py): NB = 3 (D 33, 40, 48), D == DP (16, 48), D = 1,
    D = 17 with M = 40 < 64, and 33 chains (a second, partly filled chain block of k_iwls_sat).  No decision of these cases is closer
    than 1e-6 to its threshold on the restatement (tests/test_sampler_edges_cpu.py; measured: 8e-4 and 1.2e-2 at the least)."""
    M, D, n, T, B, seed = case
    k = E.iwls_edge_case(case, compat)
    _sample_vs_numpy(hip, k["XX"], k["t"], n, T, B, seed, compat, ref=k["ref"])


@pytest.mark.parametrize("compat", [True, False])
def test_sample_matches_numpy_philox_int8_metric_nb3(hip, compat):
    """the int8 assembly (6 exact byte slices) at D = 40, 33 chains: NB = 3 behind it (german above: D = 25)"""
    case = E.IWLS_EDGE_CASES[0]
    M, D, n, T, B, seed = case
    assert D == 40 and n == 33
    k = E.iwls_edge_case(case, compat)
    _sample_vs_numpy(hip, k["XX"], k["t"], n, T, B, seed, compat, flags=_capi.int8_metric_flags(6), ref=k["ref"])


def test_saturation_in_a_partly_filled_chain_block_australian(hip):
    """33 chains, compat, 120 iterations on australian: chain 32 sits alone in the second 32-chain block of k_iwls_sat, where the guard
    c0 + j < n covers the LDS fill and the store, and saturates (55 times on the restatement, about 2100 in all: asserted in
    tests/test_sampler_edges_cpu.py).  Accepted and saturated counts per chain array-equal, samples <= 1e-9."""
    k = E.iwls_sat_case()
    ref = k["ref"]
    assert ref["saturated"][32].sum() >= 1
    acc, sat = _sample_vs_numpy(hip, k["XX"], k["t"], E.IWLS_SAT_N, E.IWLS_SAT_T, E.IWLS_SAT_B, E.IWLS_SAT_SEED, True, ref=ref)
    assert sat[32] >= 1 and sat.sum() > 1000


def test_batched_chain_equals_single_chain_with_offset(hip):
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    M, D = XX.shape
    with hip.context(M, D, 8, flags=0) as ctx:
        ctx.set_data(XX, t)
        many = ctx.iwls_sample(200, 100, seed=5)
    for i in (0, 7):
        with hip.context(M, D, 1, flags=0) as ctx:
            ctx.set_data(XX, t)
            one = ctx.iwls_sample(200, 100, seed=5, chain_offset=i)
        np.testing.assert_array_equal(one[0][0], many[0][i])
        assert one[1][0] == many[1][i] and one[2][0] == many[2][i]


def _australian():
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    return d["XX"], d["t"]


def test_compat_truncates_the_posterior_australian():
    """the reference rejects every proposal with a saturated row, so no compat sample has a row with f > 36.7"""
    XX, t = _australian()
    w, _, info = iwls(XX, t, max_iter=10000, burn_in=5000, n_chains=64, seed=31, verbose=False, return_info=True)
    assert np.max(w @ XX.T) < 36.75
    assert info["saturated"].sum() > 0


def test_posterior_agrees_with_rmhmc_australian():
    XX, t = _australian()
    n = 64
    wi, _ = iwls(XX, t, max_iter=4000, burn_in=1000, n_chains=n, seed=21, verbose=False, compat=False)
    # (compat=False on both sides: the corrected samplers leave the same posterior invariant)
    wr, _ = RMHMC(XX, t, NumOfIterations=1000, BurnIn=200, n_chains=n, seed=22, verbose=False, compat=False)
    wr = wr[:, 1:]
    mi, mr = wi.mean(axis=(0, 1)), wr.mean(axis=(0, 1))
    se = np.sqrt(wi.mean(axis=1).var(axis=0, ddof=1) / n + wr.mean(axis=1).var(axis=0, ddof=1) / n)   # chains as batches
    assert np.all(np.abs(mi - mr) <= 5 * se), (np.abs(mi - mr) / se)
    si, sr = wi.reshape(-1, wi.shape[-1]).std(axis=0), wr.reshape(-1, wr.shape[-1]).std(axis=0)
    assert np.all(np.abs(si / sr - 1) <= 0.10), si / sr


def test_limits_and_context_state(hip):
    XX, t = synthetic_logreg(200, 65, 3)
    with hip.context(200, 65, 2, flags=0) as ctx:
        ctx.set_data(XX, t)
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.iwls_sample(10, 5)
        assert e.value.code == -4
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.iwls_replay(np.zeros((2, 3, 65)), np.full((2, 3), np.nan))
        assert e.value.code == -4
    XX, t = _australian()
    M, D = XX.shape
    with hip.context(M, D, 4) as ctx:
        ctx.set_data(XX, t)
        ctx.iwls_sample(50, 25, seed=3)
        after = ctx.sample(30, 10, seed=4)
    with hip.context(M, D, 4) as ctx:
        ctx.set_data(XX, t)
        fresh = ctx.sample(30, 10, seed=4)
    np.testing.assert_array_equal(after[0], fresh[0])
    np.testing.assert_array_equal(after[1], fresh[1])


def test_run_experiment_and_reference_print_out(capsys):
    XX, t = synthetic_logreg(300, 5, 4)
    res = experiment.run_experiment(XX, t, sampler="IWLS", n_experiments=3, batched=True, seed=3, max_iter=400, burn_in=200)
    for k in ("results_beta", "results_time", "ESS", "Min", "Median", "Mean", "Max", "Time", "Time per Min ESS"):
        assert k in res, k
    assert res["results_beta"].shape == (3, 200, 5)
    capsys.readouterr()
    w, secs, info = iwls(XX, t, max_iter=2100, burn_in=1500, seed=1, verbose=True, return_info=True)
    out = capsys.readouterr().out.splitlines()
    assert out == ["--- Initialization...", "--- Iterating...", "Iteration 0", "Iteration 1000",
                   "Burn-in complete, now drawing posterior samples.", "Iteration 2000", "--- Iterating: done.",
                   "Number of accepted samples:  %d" % info["accepted"][0]]
    assert w.shape == (600, 5) and secs > 0 and 0 < info["accepted"][0] <= 2100
