"""Adaptive Metropolis on the MI355X (include/rmhmc_amh.h, csrc/amh.hip.h): replays of the reference's own draws, the Philox sampler
against the NumPy restatement of tests/test_amh_cpu.py, chain independence, agreement in distribution with the RMHMC sampler, and the
Python surface."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from riemannhamiltonianmontecarlo_amd import AMH, RMHMC, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_amh_cpu import AMH_TAPES, amh_numpy, load_amh_tape, philox_draws

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sampler_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("name", AMH_TAPES)
def test_replay_matches_reference_tape(hip, name):
    XX, t, g = load_amh_tape(name)
    T, B = int(g["n_iter"]), int(g["burn_in"])
    M, D = XX.shape
    n = 2   # the same tape in two chains
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        r = ctx.amh_replay(T, B, np.broadcast_to(g["z"], (n, T, D)), np.broadcast_to(g["u"], (n, T, D)))
    for c in range(n):
        np.testing.assert_array_equal(r["accepted"][c], g["accepted"] != 0)
        np.testing.assert_array_equal(r["u_read"][c], ~np.isnan(g["u"]))      # u consumed exactly where the reference drew one
        np.testing.assert_array_equal(r["sd"][c], g["sd"][-1])
        assert _rel(r["w"][c], g["w"]) <= 1e-14
        np.testing.assert_allclose(r["ljl"][c], g["ljl"], rtol=1e-11)


def _sample_vs_numpy(hip, XX, t, n, T, B, seed, follow=None, ref=None):
    """follow: the chain ids the restatement follows (default: all); ref: its run on them, where the caller shares it"""
    M, D = XX.shape
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        smp, acc, sd, _ = ctx.amh_sample(T, B, seed=seed)
    ids = np.arange(n) if follow is None else np.asarray(follow)
    if ref is None:
        ref = amh_numpy(XX, t, T, B, philox_draws(seed, ids, D), n=len(ids))
    assert np.all(np.isfinite(smp))
    np.testing.assert_array_equal(acc[ids], ref["accepted"].sum(axis=(1, 2)))
    assert _rel(smp[ids], ref["w"][:, B:]) <= 1e-10
    np.testing.assert_array_equal(sd[ids], ref["sd"])


def test_sample_matches_numpy_philox_australian(hip):
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    _sample_vs_numpy(hip, d["XX"], d["t"], 4, 300, 150, 1234)


def test_sample_matches_numpy_philox_64_chains(hip):
    XX, t = synthetic_logreg(5000, 32, 11)
    _sample_vs_numpy(hip, XX, t, 64, 40, 20, 99)


def test_sample_matches_numpy_philox_streamed_f(hip):
    """M beyond the on-chip rows (256 threads x 48): f goes through the per-chain global buffers"""
    XX, t = synthetic_logreg(20000, 6, 12)
    _sample_vs_numpy(hip, XX, t, 3, 30, 20, 7)


@pytest.mark.parametrize("case", ["ripley", "pima", "syn_m300_d80"])
def test_sample_matches_numpy_philox_one_wave_per_chain(hip, case):
    """>= 1024 chains with M <= 1024 run one wavefront per chain (k_amh<64, R>, no LDS reduction): R = 4 (ripley, M 250),
    R = 16 (pima, M 532), R = 8 with D = 80, where a lane owns two coordinates (KW = 4)"""
    if case == "syn_m300_d80":
        XX, t = synthetic_logreg(300, 80, 13)
        T, B = 10, 5
    else:
        d = np.load(os.path.join(GOLDEN, "data_%s.npz" % case))
        XX, t = d["XX"], d["t"]
        T, B = 30, 20
    _sample_vs_numpy(hip, XX, t, 1024, T, B, 31)


@pytest.mark.parametrize("name", list(E.AMH_EDGE_CASES))
def test_sample_matches_numpy_philox_wide_d_and_tile_edges(hip, name):
    """the variants and edges no other case runs (tests/helpers/sampler_edges.py; the variant each shape selects is asserted in
    tests/test_sampler_edges_cpu.py): one wavefront per chain with D = 256 (KW = 4, every lane owns four coordinates) and D = 129
    (lane 0 owns three, the last Box-Muller pair is half used); 256 threads per chain with D = 200 and 65 (threads 64..255 own
    coordinates and draw); M = 1024 (R = 16 full at NT = 64), 1025 (falls to NT = 256), 12 288 = AMH_MAX_ONCHIP_ROWS (R = 48 full) and
    12 289 (the first streamed size).  Of a 1024-chain batch the restatement follows the first chain, the last and 16 in between."""
    n, M, D, T, B, seed, _ = E.AMH_EDGE_CASES[name]
    k = E.amh_edge_case(name)
    _sample_vs_numpy(hip, k["XX"], k["t"], n, T, B, seed, follow=k["ids"], ref=k["ref"])


@pytest.mark.parametrize("M", [500, 1500, 4000, 8000, 12000])
def test_sample_matches_numpy_philox_rows_per_thread(hip, M):
    """256 threads per chain with f in R = 2, 8, 16, 32, 48 registers per thread (R = 4: australian above; streamed: M 20 000)"""
    XX, t = synthetic_logreg(M, 6, 14)
    _sample_vs_numpy(hip, XX, t, 3, 20, 10, 17)


@pytest.mark.parametrize("n,M", [(1024, 10000), (512, 20000)])
def test_launch_cuts_leave_results_unchanged(hip, n, M):
    """A segment whose work exceeds AMH_LAUNCH_ROWS (2^34 chain x proposal x row evaluations) runs as several launches with f and
    CurrentLJL carried over (here 26 iterations per launch); one chain alone runs each segment in one launch.  Same bits, on chip
    (R = 48) and streamed."""
    D, T, B = 64, 60, 30
    XX, t = synthetic_logreg(M, D, 15)
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        many = ctx.amh_sample(T, B, seed=8)
    for i in (0, n - 1):
        with hip.context(M, D, 1, flags=0) as ctx:
            ctx.set_data(XX, t)
            one = ctx.amh_sample(T, B, seed=8, chain_offset=i)
        np.testing.assert_array_equal(one[0][0], many[0][i])
        assert one[1][0] == many[1][i]
        np.testing.assert_array_equal(one[2][0], many[2][i])


def test_batched_chain_equals_single_chain_with_offset(hip):
    XX, t = synthetic_logreg(690, 15, 3)
    with hip.context(690, 15, 4, flags=0) as ctx:
        ctx.set_data(XX, t)
        many = ctx.amh_sample(250, 120, seed=5)
    for i in (0, 3):
        with hip.context(690, 15, 1, flags=0) as ctx:
            ctx.set_data(XX, t)
            one = ctx.amh_sample(250, 120, seed=5, chain_offset=i)
        np.testing.assert_array_equal(one[0][0], many[0][i])
        assert one[1][0] == many[1][i]
        np.testing.assert_array_equal(one[2][0], many[2][i])


def test_posterior_agrees_with_rmhmc_australian():
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    n = 64
    wa, _ = AMH(XX, t, NumOfIterations=10000, BurnIn=5000, n_chains=n, seed=21, verbose=False)   # the reference's own run length
    # (compat=False: momentum p = L z with Cov(p) = G; the reference's p = L'z, the default, does not leave the posterior invariant)
    wr, _ = RMHMC(XX, t, NumOfIterations=1000, BurnIn=200, n_chains=n, seed=22, verbose=False, compat=False)
    wa, wr = wa[:, 1:], wr[:, 1:]
    ma, mr = wa.mean(axis=(0, 1)), wr.mean(axis=(0, 1))
    se = np.sqrt(wa.mean(axis=1).var(axis=0, ddof=1) / n + wr.mean(axis=1).var(axis=0, ddof=1) / n)   # chains as batches
    assert np.all(np.abs(ma - mr) <= 5 * se), (np.abs(ma - mr) / se)
    sa, sr = wa.reshape(-1, wa.shape[-1]).std(axis=0), wr.reshape(-1, wr.shape[-1]).std(axis=0)
    assert np.all(np.abs(sa / sr - 1) <= 0.10), sa / sr
    moved = (np.diff(wa, axis=1) != 0).mean(axis=(0, 1))   # post-burn-in acceptance per dimension
    assert np.all((moved >= 0.15) & (moved <= 0.6)), moved


def test_run_experiment_and_reference_print_out(capsys):
    XX, t = synthetic_logreg(300, 5, 4)
    res = experiment.run_experiment(XX, t, sampler="AMH", n_experiments=3, batched=True, seed=3, NumOfIterations=400, BurnIn=200)
    for k in ("results_beta", "results_time", "ESS", "Min", "Median", "Mean", "Max", "Time", "Time per Min ESS"):
        assert k in res, k
    assert res["results_beta"].shape == (3, 200, 5)
    capsys.readouterr()
    w, secs, info = AMH(XX, t, NumOfIterations=2100, BurnIn=1500, seed=1, verbose=True, return_info=True)
    out = capsys.readouterr().out.splitlines()
    assert out[:3] == ["0 iterations completed.", "1000 iterations completed.", "Burn-in complete, now drawing posterior samples."]
    assert out[3].startswith("Time drawing posterior: ") and len(out) == 4
    assert w.shape == (600, 5) and secs > 0 and info["ProposalSD"].shape == (1, 5)
