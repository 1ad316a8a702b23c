"""Auxiliary-variable Gibbs sampler on the MI355X (include/rmhmc_gibbs.h, csrc/gibbs.hip.h): replays of the reference's own draws against
the reference's values, the Philox sampler against the NumPy restatement of tests/test_gibbs_cpu.py, chain and segment independence,
invariants on outlier data, agreement in distribution with the reference's own long runs, the benchmark's shape, limits, and the Python
surface."""
import contextlib
import io
import os
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, rel_err
from riemannhamiltonianmontecarlo_amd import RMHMC, _capi, auxiliary_gibbs, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_gibbs_cpu import GIBBS_TAPES, PhiloxDraws, flip_labels, gibbs_numpy, load_gibbs_tape

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sampler_edges as E  # noqa: E402
from sampler_edges import OneUlpOff as _OneUlpOff, philox_tapes  # noqa: E402

pytestmark = pytest.mark.gpu


def _tapes(g, n):
    T, N = g["u_sweep"].shape
    b = lambda a: np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape))
    return b(g["u_init"]), b(g["u_sweep"]), b(g["T"]), b(g["ks_draws"]), b(g["ks_offset"])


@pytest.mark.parametrize("name", GIBBS_TAPES)
def test_replay_matches_reference_tape(hip, name):
    """the same tape in two chains: attempts per row array-equal to the tape, no row left out; beta, B <= 1e-9, Z, lam <= 1e-8 against
    the tape (the reference's values)"""
    XX, t, g = load_gibbs_tape(name)
    M, D = XX.shape
    n = 2
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t, float(g["v"]))
        r = ctx.gibbs_replay(*_tapes(g, n))
    for c in range(n):
        assert r["status"][c] == 0 and r["capped"][c] == 0
        np.testing.assert_array_equal(r["attempts"][c], g["attempts"])
        errs = {k: rel_err(r[k][c], g[k]) for k in ("beta", "B", "Z", "lam")}
        print(name, c, errs)
        assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9, errs
        assert errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs


def test_replay_stops_a_chain_whose_tape_is_short(hip):
    """chain 1's tape lacks the last attempt of one row: the chain stops and is reported, chain 0 is untouched"""
    XX, t, g = load_gibbs_tape("ripley")
    M, D = XX.shape
    u_init, u_sweep, T, ks, off = _tapes(g, 2)
    off = off.copy()
    j = int(np.argmax(g["attempts"][1] >= 2))           # a row of iteration 1 with at least two attempts
    off[1, 1, j + 1:] -= 1                              # its range loses the accepted attempt; the later rows read shifted draws
    off[1, 2:] -= 1
    with hip.context(M, D, 2, flags=0) as ctx:
        ctx.set_data(XX, t, float(g["v"]))
        r = ctx.gibbs_replay(u_init, u_sweep, T, ks, off)
    assert list(r["status"]) == [0, 1]
    np.testing.assert_array_equal(r["attempts"][0], g["attempts"])
    assert rel_err(r["beta"][0], g["beta"]) <= 1e-9
    np.testing.assert_array_equal(r["attempts"][1, 0], g["attempts"][0])      # iteration 0 ran; nothing after the stop
    assert np.all(r["beta"][1, 2:] == 0)
    bad = off.copy(); bad[0, 0, 3] = -1
    with hip.context(M, D, 2, flags=0) as ctx:
        ctx.set_data(XX, t, float(g["v"]))
        with pytest.raises(_capi.RmhmcError):
            ctx.gibbs_replay(u_init, u_sweep, T, ks, bad)


def _sample_vs_numpy(hip, XX, t, n, T, B, seed, follow=None, v=100.0, known=None):
    """gibbs_sample against gibbs_numpy on the same Philox streams; follow: the chain ids the restatement follows (default: all).
    The reference's proposal Y = 1 + (Y - sqrt(Y (4 r + Y))) / (2 r) (gibbs_sampler.py:59) cancels twice for a small residual r, so one
    rounding error in r comes back as ~ eps (Y / r)^2 in lam_j and, an iteration later, in beta: two correct evaluations of the file differ
    by 1e-10 .. 1e-5 after two or three iterations, depending on the smallest residual the case happens to meet.
    A case can carry the 1e-9 bound only where the restatement itself is stable to that level, so that is checked first, on the
    restatement alone: its samples move by <= 1e-10 when the initial uniforms move by one ulp.  Data, seeds and lengths below were
    chosen by that criterion, before any run on the device.  known: dict(ref, own) where the caller shares them with other tests."""
    M, D = XX.shape
    ids = np.arange(n) if follow is None else np.asarray(follow)
    if known is None:
        ref = gibbs_numpy(XX, t, T, PhiloxDraws(seed, ids, M, D), n=len(ids), v=v)
        own = rel_err(gibbs_numpy(XX, t, T, _OneUlpOff(seed, ids, M, D), n=len(ids), v=v)["beta"], ref["beta"])
    else:
        ref, own = known["ref"], known["own"]
    assert own <= 1e-10, own
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t, v)
        r = ctx.gibbs_sample(T, B, seed=seed)
    smp, capped = r["samples"], r["capped"]
    assert np.all(capped == 0) and np.all(ref["capped"] == 0) and np.all(r["stopped"] == -1)
    err = rel_err(smp[ids], ref["beta"][:, B:])
    print("gibbs_sample vs gibbs_numpy: M %d D %d, %d chains (%d followed), %d iterations: %.3e (the restatement against itself one ulp off: %.3e)"
          % (M, D, n, len(ids), T, err, own))
    assert np.all(np.isfinite(smp))
    assert err <= 1e-9, err
    return smp


def test_sample_matches_numpy_philox_australian(hip):
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    _sample_vs_numpy(hip, d["XX"], d["t"], 4, 30, 10, 1234)


def test_sample_matches_numpy_philox_d64(hip):
    XX, t = synthetic_logreg(200, 64, 5)
    _sample_vs_numpy(hip, XX, t, 64, 2, 0, 84)


def test_sample_matches_numpy_philox_large_batch_ragged_m(hip):
    """1536 chains, M = 203 (13 row blocks of the sweep, the last one of 11 rows; not a multiple of the 256 rows of a mixing-weight
    block either).  The restatement follows 18 chain ids: the first, the last and 16 spread over the batch."""
    XX, t = synthetic_logreg(203, 9, 11)
    n = 1536
    follow = np.unique(np.concatenate([[0, n - 1], np.linspace(1, n - 2, 16).astype(int)]))
    assert len(follow) >= 18
    _sample_vs_numpy(hip, XX, t, n, 3, 1, 109, follow=follow)


@pytest.mark.parametrize("M,D,T", E.GIBBS_EDGE_CASES)
def test_sample_matches_numpy_philox_block_counts_and_edges(hip, M, D, T):
    """every block count of k_gibbs_sweep / k_gibbs_factor and the row-count edges (tests/helpers/sampler_edges.py): NB = 2 (D 17, 24,
    31, 32), NB = 3 with D == DP (48), D == DP (16, 32), D = 1; M = 3, 15, 16, 17 (the sweep's 16-row blocks, the 8-row stride of
    k_gibbs_b's four waves), 256 / 257 (a block of k_gibbs_mix / k_gibbs_init).  Four chains, no burn-in, same bounds as every case
    here; the stability of each case on the restatement is asserted in tests/test_sampler_edges_cpu.py too."""
    k = E.gibbs_edge_case(M, D, T)
    _sample_vs_numpy(hip, k["XX"], k["t"], E.GIBBS_EDGE_CHAINS, T, 0, E.GIBBS_EDGE_SEED, known=k)


@pytest.mark.parametrize("M,D,T", E.GIBBS_EDGE_CASES)
def test_replay_matches_numpy_block_counts_and_edges(hip, M, D, T):
    """the same cases through the replay entry point fed with the restatement's attempts: attempts array-equal, B, beta <= 1e-9, Z, lam
    <= 1e-8 (the state and the attempts, which the sampler's samples do not show)"""
    k = E.gibbs_edge_case(M, D, T)
    ref = k["ref"]
    with hip.context(M, D, E.GIBBS_EDGE_CHAINS, flags=0) as ctx:
        ctx.set_data(k["XX"], k["t"])
        r = ctx.gibbs_replay(*philox_tapes(k["draws"], ref["attempts"]))
    assert np.all(r["status"] == 0) and np.all(r["capped"] == 0)
    np.testing.assert_array_equal(r["attempts"], ref["attempts"])
    errs = {key: rel_err(r[key], ref[key]) for key in ("beta", "B", "Z", "lam")}
    print("replay vs gibbs_numpy: M %d D %d:" % (M, D), errs)
    assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9 and errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs


def test_replay_row_that_reaches_the_attempt_bound(hip):
    """Row 7 of chain 1 has the second uniform of every attempt of iteration 1 at 1 - 2^-53: every attempt is rejected, the row runs
    into GIBBS_MAX_ATTEMPTS, keeps its last proposal and is counted in capped (the path of k_gibbs_mix that no other test reaches:
    they all assert capped == 0).  capped and attempts array-equal to the restatement, no chain stopped, beta, B <= 1e-9 and Z, lam
    <= 1e-8 through the iteration after it, which runs on the kept proposal; chains 0 and 2 bit for bit as without the override."""
    k = E.capped_case()
    ref = k["ref"]
    out = []
    for dr in (k["draws"], k["plain_draws"]):
        with hip.context(E.CAP_M, E.CAP_D, E.CAP_N, flags=0) as ctx:
            ctx.set_data(k["XX"], k["t"])
            out.append(ctx.gibbs_replay(*philox_tapes(dr, (ref if dr is k["draws"] else k["plain"])["attempts"])))
    r, plain = out
    np.testing.assert_array_equal(r["capped"], ref["capped"])
    assert list(r["capped"]) == [0, 1, 0] and np.all(r["status"] == 0)
    np.testing.assert_array_equal(r["attempts"], ref["attempts"])
    assert r["attempts"][E.CAP_CHAIN, E.CAP_IT, E.CAP_ROW] == 64
    errs = {key: rel_err(r[key], ref[key]) for key in ("beta", "B", "Z", "lam")}
    print("capped row:", errs)
    assert np.all(np.isfinite(r["beta"])) and np.all(np.isfinite(r["Z"])) and np.all(r["lam"] > 0)
    assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9 and errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs
    assert np.all(plain["capped"] == 0) and np.all(plain["status"] == 0)
    for c in (0, 2):
        for key in ("beta", "B", "Z", "lam", "attempts"):
            np.testing.assert_array_equal(r[key][c], plain[key][c])


def test_batched_chain_equals_single_chain_and_segments_do_not_matter(hip):
    d = np.load(os.path.join(GOLDEN, "data_pima.npz"))
    XX, t = d["XX"], d["t"]
    M, D = XX.shape

    def run(n, T, B, off=0):
        with hip.context(M, D, n, flags=0) as ctx:
            ctx.set_data(XX, t)
            ctx.set_progress(lambda *a: None)          # the host synchronises at the reports, as in a verbose run
            return ctx.gibbs_sample(T, B, seed=5, chain_offset=off)["samples"]

    full = run(6, 230, 0)
    for c in (0, 3, 5):
        np.testing.assert_array_equal(run(1, 230, 0, off=c)[0], full[c])       # bit for bit
    for B in (100, 57, 201):                                                      # burn_in at, before and after a multiple of 100
        np.testing.assert_array_equal(run(6, 230, B), full[:, B:])
    # an int8-metric context runs the same fp64 assembly
    with hip.context(M, D, 6, flags=_capi.int8_metric_flags(6)) as ctx:
        ctx.set_data(XX, t)
        np.testing.assert_array_equal(ctx.gibbs_sample(230, 200, seed=5)["samples"], full[:, 200:])


def test_invariants_on_outlier_data(hip):
    """5 % flipped labels, x_scale 30, 200 iterations: everything finite, sign(Z_j) matches t_j, lam > 0, no capped row"""
    M, D, n, T = 300, 6, 8, 200
    XX, t = synthetic_logreg(M, D, 4)
    XX = XX * 30.0
    t = flip_labels(t, 0.05, 4)
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        r200 = ctx.gibbs_sample(T, 0, seed=8, state=True)
    smp, capped = r200["samples"], r200["capped"]
    tt = np.asarray(t).reshape(-1)
    assert np.all(np.isfinite(smp)) and np.all(capped == 0) and np.all(r200["stopped"] == -1)
    # the state after the 200 iterations
    assert np.all(np.isfinite(r200["Z"])) and np.all(np.isfinite(r200["lam"])) and np.all(r200["lam"] > 0)
    assert np.all(np.sign(r200["Z"]) == np.where(tt == 1, 1.0, -1.0)[None])
    # the state itself, through the replay entry point fed with the sampler's own streams for a few iterations
    T2 = 5
    dr = PhiloxDraws(8, np.arange(n), M, D)
    ref = gibbs_numpy(XX, t, T2, dr, n=n)
    tapes = philox_tapes(dr, ref["attempts"])
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        r = ctx.gibbs_replay(*tapes)
    assert np.all(r["status"] == 0) and np.all(r["capped"] == 0)
    np.testing.assert_array_equal(r["attempts"], ref["attempts"])
    assert np.all(np.isfinite(r["Z"])) and np.all(np.sign(r["Z"]) == np.where(tt == 1, 1.0, -1.0)[None]) and np.all(r["lam"] > 0)
    assert rel_err(r["beta"], ref["beta"]) <= 1e-9 and rel_err(r["Z"], ref["Z"]) <= 1e-8 and rel_err(r["lam"], ref["lam"]) <= 1e-8
    assert rel_err(smp[:, :T2], ref["beta"]) <= 1e-9


def test_posterior_agrees_with_the_references_long_runs_ripley():
    """Pooled moments of 256 GPU chains of the reference's run length (5500 iterations, 500 of them burn-in) against the per-seed means
    and standard deviations of 12 such runs of the reference itself (tests/golden/gibbs_ripley_moments.npz): means within 5 standard
    errors, the standard error from the spread of the REFERENCE's per-seed means (the GPU side's own error is negligible at 256
    chains); standard deviations within 5 times the relative spread of the reference's per-seed values.  The same comparison against
    RMHMC(compat=False) is computed and printed, not asserted.
    A chain whose draw of some lam_j is inf (the reference's proposal formula cancels for residuals below about 1e-7) has no variance
    to draw from: the reference stops there with a ValueError (seed 106 of the 16 tried, at iteration 5063: the failed seeds of the
    fixture), the device chain stops and reports it.  Such chains are counted, printed and left out of the pooled moments."""
    g = np.load(os.path.join(GOLDEN, "gibbs_ripley_moments.npz"))
    d = np.load(os.path.join(GOLDEN, "data_ripley.npz"))
    XX, t = d["XX"], d["t"]
    assert g["mean"].shape[0] == 12
    n = 256
    smp, secs, info = auxiliary_gibbs(XX, t, v=float(g["v"]), max_iter=int(g["n_iter"]), burn_in=int(g["burn_in"]), n_chains=n, seed=31,
                                      verbose=False, return_info=True)
    alive = info["stopped"] < 0
    np.testing.assert_array_equal(alive, np.all(np.isfinite(smp), axis=(1, 2)))
    assert np.all(info["capped"][alive] == 0)
    print("ripley: %d GPU chains x %d iterations in %.2f s after burn-in; %d chains stopped; the reference stopped on seeds %s of the 16 run"
          % (n, int(g["n_iter"]), secs, int((~alive).sum()), list(g["failed_seeds"])))
    # (256 x 250 x 5500 = 3.5e8 draws of lam_j at about 3e-9 each: one stopped chain expected)
    assert (~alive).sum() <= 8
    smp = smp[alive]
    mean, std = smp.mean(axis=(0, 1)), smp.reshape(-1, smp.shape[-1]).std(axis=0)
    rm, rs = g["mean"].mean(axis=0), g["std"].mean(axis=0)
    se = g["mean"].std(axis=0, ddof=1) / np.sqrt(12)
    spread = g["std"].std(axis=0, ddof=1) / rs
    zm = (mean - rm) / se
    zs = (std / rs - 1) / spread
    print("means: GPU - reference in standard errors of the reference:", np.round(zm, 2))
    print("standard deviations: GPU / reference - 1 in relative spreads of the reference's per-seed values:", np.round(zs, 2), "ratios", np.round(std / rs, 4))
    wr, _ = RMHMC(XX, t, NumOfIterations=3000, BurnIn=500, n_chains=64, seed=22, verbose=False, compat=False)
    wr = wr[:, 1:]
    mr, sr = wr.mean(axis=(0, 1)), wr.reshape(-1, wr.shape[-1]).std(axis=0)
    ser = np.sqrt(se ** 2 + wr.mean(axis=1).var(axis=0, ddof=1) / wr.shape[0])
    print("against RMHMC(compat=False), 64 chains: reference means - RMHMC in standard errors:", np.round((rm - mr) / ser, 2))
    print("                                        GPU Gibbs means - RMHMC in the same units: ", np.round((mean - mr) / ser, 2))
    print("                                        sd ratios reference / RMHMC:", np.round(rs / sr, 4), " GPU Gibbs / RMHMC:", np.round(std / sr, 4))
    assert np.all(np.abs(zm) <= 5), zm
    assert np.all(np.abs(zs) <= 5), zs


_BENCH_SIZE_CHILD = """
import sys, time
import numpy as np
import torch  # noqa: F401  (before the HIP library is loaded, as tests/conftest.py)
sys.path.insert(0, sys.argv[1])
from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
M, D, n = 10000, 64, 8192
XX, t = synthetic_logreg(M, D, 0)
with _capi.load_hip_library().context(M, D, n, flags=0) as ctx:
    ctx.set_data(XX, t)
    r = ctx.gibbs_sample(3, 0, seed=3, state=True)
tt = np.asarray(t).reshape(-1)
alive = r["stopped"] < 0
Z, lam = r["Z"][alive], r["lam"][alive]
np.savez(sys.argv[2], samples=r["samples"], capped=r["capped"], stopped=r["stopped"], seconds=r["seconds"],
         z_finite=np.isfinite(Z).all(), lam_ok=(np.isfinite(lam) & (lam > 0)).all(),
         sign_ok=(np.sign(Z) == np.where(tt == 1, 1.0, -1.0)[None]).all())
"""


def test_one_launch_at_the_benchmark_size(tmp_path):
    """8192 chains x D 64 x M 10 000, 3 iterations, in a process of its own that is ended after 300 s (a hung launch cannot hold the
    suite): finite, sign(Z_j) matches t_j, lam > 0, no capped row, on every chain that did not stop; a stopped chain is finite up to
    the iteration it reports and NaN after it."""
    import subprocess
    import sys
    from conftest import ROOT
    out = str(tmp_path / "bench_size.npz")
    t0 = time.time()
    subprocess.run([sys.executable, "-c", _BENCH_SIZE_CHILD, ROOT, out], check=True, timeout=300)
    wall = time.time() - t0
    r = np.load(out)
    smp, capped, stopped, secs = r["samples"], r["capped"], r["stopped"], float(r["seconds"])
    n, D = 8192, 64
    alive = stopped < 0
    print("8192 x 64 x 10000, 3 iterations: %.2f s in the sampler, %.2f s with set-up and the final state; %d chains stopped on lam_j = inf"
          % (secs, wall, int((~alive).sum())))
    # (2.5e8 draws of lam_j: the reference's cancelling proposal returns inf for about 3e-9 of them, DESIGN section 8d: 0.7 chains expected)
    assert smp.shape == (n, 3, D) and (~alive).sum() <= 8 and np.all(capped[alive] == 0)
    assert np.all((stopped >= -1) & (stopped < 3))
    for c in np.nonzero(~alive)[0]:
        assert np.all(np.isfinite(smp[c, :stopped[c] + 1])) and np.all(np.isnan(smp[c, stopped[c] + 1:]))
    assert bool(r["z_finite"]) and bool(r["lam_ok"]) and bool(r["sign_ok"])
    smp = smp[alive]
    assert np.all(np.isfinite(smp)) and np.abs(smp).max() < 10 and len(np.unique(smp[:, 2, 0])) == len(smp)   # chains differ, no runaway


def _replay_truncated_normal(hip, k, what):
    """replay of the batch k (tests/helpers/sampler_edges.py) against the restatement: attempts equal; beta, B norm-wise <= 1e-9; every Z
    finite, non-zero and on its label's side; Z ELEMENT by element within 1e-8 |Z_ref| + 1e-12 (|m| + s), m and s the restatement's
    values of that row's last draw (the project's Z bound per element; the absolute term is the rounding of the sum m + s y when m
    comes from differently ordered sums).  Prints the worst error / tolerance per m/s bin of the last draw and returns it."""
    ref, t, n = k["ref"], np.asarray(k["t"]).reshape(-1), k["n"]
    with hip.context(E.TN_M, E.TN_D, n, flags=0) as ctx:
        ctx.set_data(k["XX"], k["t"])
        r = ctx.gibbs_replay(*philox_tapes(k["draws"], ref["attempts"]))
    assert np.all(r["status"] == 0) and np.all(r["capped"] == 0)
    np.testing.assert_array_equal(r["attempts"], ref["attempts"])
    assert np.all(np.isfinite(r["Z"])) and np.all(r["Z"] != 0) and np.all(np.sign(r["Z"]) == np.where(t == 1, 1.0, -1.0)[None])
    errs = {key: rel_err(r[key], ref[key]) for key in ("beta", "B", "Z", "lam")}
    ratio, worst = E.tn_report(r["Z"], ref)
    print("%s, %d iteration(s), norm-wise:" % (what, k["T"]), errs)
    for b, (q, cnt) in worst.items():
        print("    m/s in %-12s %5d elements of Z, worst error / tolerance %.3e" % (b, cnt, q))
    if "extreme" in k:
        print("    elements drawn at an extreme uniform: worst error / tolerance %.3e" % ratio[k["extreme"]].max())
        low = ref["p_last"] < E.G.TINY                           # p = U Phi(-m/s) below TINY on the two-tail form: the fmax(p, TINY) clamp
        assert low.sum() == 2
        print("    elements whose p is clamped at TINY (Z = m + s Phi^-1(TINY)): device", r["Z"][low], "restatement", ref["Z"][low],
              "error / tolerance %.3e" % ratio[low].max())
    assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9, errs
    assert np.all(ratio <= 1.0), (float(ratio.max()), np.argwhere(ratio > 1.0)[:8])
    return errs, worst


@pytest.mark.parametrize("T", [E.TN_T, 1])
def test_device_truncated_normal_between_the_tapes_and_the_tail_form(hip, T):
    """gibbs_truncnorm_neg on the device where neither the tapes (|m/s| <= 2.4) nor the far-tail test (m/s > 25) reach: the library
    quantile polished by the Newton step on erfc for p = U Phi(-m/s) down to 1e-137, both sides of the switch to the asymptotic form
    at m/s = 25, the complement branch p > 1/2 at m/s down to -30, and the two clamps.  24 chains of the intercept-dominated data set,
    chain c started at Z = Phi^-1(Phi(-z0_c) / 2) on every label-0 row, z0 from 2.5 to 31 (tests/helpers/sampler_edges.py; the counts
    per bin, the stability of the case and the extreme uniforms are asserted on the restatement in tests/test_sampler_edges_cpu.py).
    The chains relax in one sweep, so the draws beyond m/s = 10 are all in the first one: the run of ONE iteration has them in its Z
    and compares them element by element (34, 30, 29, 37, 75, 10, 9, 7 elements in the bins from (2.4, 5] to (26, 30], 1216 below
    -15); the run of three iterations compares what follows from them.  In the last iteration of either, two rows of each label in
    chains 3 and 13 (and two label-1 rows of chain 22, in the tail form) are drawn at U = 1e-300, 2^-53, 1/2 and 1 - 2^-53: where the
    mirrored uniform of a label-1 row is 1, the draw is the rounding of m + s y and fmin(x, -TINY) holds it on its side.  One
    label-0 row of chains 5 and 16 is drawn at a subnormal uniform (1e-310, 5e-324): p = U Phi(-m/s) is below TINY there and the
    fmax(p, TINY) clamp gives m + s Phi^-1(TINY) (that p < TINY occurs on exactly these two draws is asserted on the restatement).
    Measured on the MI355X, worst error / tolerance per bin of the one-iteration run: (2.4, 5] 9.6e-6, (5, 10] 3.2e-5, (10, 15]
    4.7e-5, (15, 20] 4.6e-5, (20, 24] 2.0e-4, (24, 25] 1.5e-4, (25, 26] 7.9e-8, (26, 30] 3.0e-8, [-25, -15) 2.2e-7, [-40, -25)
    8.7e-8, the extreme uniforms 1.7e-5, the two draws with p clamped at TINY 1.6e-8; of the three-iteration run 1.6e-3 at the most
    (extreme uniforms 5.7e-5, clamped p 1.1e-6).  The restatement's
    own values of these draws lie within 1.7e-4 of the tolerance of the exact quantile (mpmath), in every bin."""
    _replay_truncated_normal(hip, E.tn_mid_case(T), "truncated normal, mid range")


def _far_tail(hip, T):
    k = E.tn_far_case(T)
    ref = k["ref"]
    far = int((ref["a_calls"] > E.G.TAIL).sum())
    assert far >= 20 and np.all(ref["capped"] == 0), far
    errs, worst = _replay_truncated_normal(hip, k, "far tail, %d draws beyond m/s = 25" % far)
    assert errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs
    return ref, worst


def test_device_truncated_normal_far_tail(hip):
    """The device's own truncated normal beyond m/s = 25 (the asymptotic branch, which no tape reaches: |m/s| <= 2.4 there).  An
    intercept-dominated data set, nine labels 0 to one label 1, with the initial uniform of every label-0 row at 1e-300: Z_j = -37
    there, B_0 near -30, and the label-1 rows are drawn at m/s between 25 and 35 (counted on the restatement: at least 20 such
    draws).  Replay of the Philox streams with that u_init against the restatement: attempts equal, beta, B <= 1e-9, Z, lam <= 1e-8,
    every Z finite and on its label's side, and Z element by element within 1e-8 |Z_ref| + 1e-12 (|m| + s): norm-wise, against
    max |Z| = 37, a relative error of 1e-6 in a heavily truncated draw of 0.05 passed."""
    _far_tail(hip, E.TN_T)


def test_device_truncated_normal_far_tail_first_sweep(hip):
    """All 30 far draws of the case above are in its first sweep (the chains relax at once: the Z it compares after three iterations
    holds none of them).  The same batch run for ONE iteration: the far draws are the label-1 elements of Z, compared element by
    element.  Measured on the MI355X: worst error / tolerance 7.4e-8 on the 30 far draws, 9.4e-8 over all of Z."""
    ref, worst = _far_tail(hip, 1)
    assert (ref["m_last"] / ref["s_last"] > E.G.TAIL).sum() >= 20


def test_limits(hip):
    XX, t = synthetic_logreg(200, 65, 3)
    with hip.context(200, 65, 2, flags=0) as ctx:
        ctx.set_data(XX, t)
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.gibbs_sample(4, 1)
        assert e.value.code == -3 or "not supported" in str(e.value)
    XX, t = synthetic_logreg(50, 3, 3)
    with hip.context(50, 3, 2, flags=0) as ctx:
        ctx.set_data(XX, t)
        with pytest.raises(_capi.RmhmcError):
            ctx.gibbs_sample(4, 1, chain_offset=2 ** 32 - 1)
        # the context still serves the other samplers afterwards
        smp = ctx.gibbs_sample(4, 1, seed=1)["samples"]
        w, acc, sd, _ = ctx.amh_sample(20, 10, seed=1)
        assert np.all(np.isfinite(smp)) and np.all(np.isfinite(w))


def test_reference_printout_and_experiment():
    d = np.load(os.path.join(GOLDEN, "data_ripley.npz"))
    XX, t = d["XX"], d["t"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        beta, secs = auxiliary_gibbs(XX, t, max_iter=250, burn_in=120, seed=4)
    lines = buf.getvalue().splitlines()
    assert lines[:2] == ["--- Initialization...", "--- Initialization: done. Iterating..."]
    assert lines[2:5] == ["Iteration 0", "Iteration 100", "Iteration 200"]
    assert lines[5] == "--- Iterating: done." and lines[6] == "--- Auxiliary Variable Gibbs Sampler finished in {}".format(secs)
    assert beta.shape == (130, 7) and secs > 0 and np.all(np.isfinite(beta))
    res = experiment.run_experiment(XX, t, sampler="Gibbs", n_experiments=4, batched=True, seed=9, max_iter=400, burn_in=100)
    assert res["results_beta"].shape == (4, 300, 7) and res["sampler"] == "auxiliary_gibbs" and res["Min"] > 0
    one, _ = auxiliary_gibbs(XX, t, max_iter=400, burn_in=100, seed=9, chain_offset=2, verbose=False)
    np.testing.assert_array_equal(one, res["results_beta"][2])


def test_australian_default_run_shape():
    """auxiliary_gibbs(XX, t) with the reference's defaults on the bundled australian data: (5000, 15) samples and a time"""
    d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
    beta, secs = auxiliary_gibbs(d["XX"], d["t"], seed=12, verbose=False)
    print("australian, one chain, 10000 / 5000: %.2f s after burn-in" % secs)
    assert beta.shape == (5000, 15) and secs > 0 and np.all(np.isfinite(beta))
