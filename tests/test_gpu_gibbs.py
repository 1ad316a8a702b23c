"""Auxiliary-variable Gibbs sampler on the MI355X (include/rmhmc_gibbs.h, csrc/gibbs.hip.h): replays of the reference's own draws against
the reference's values, the Philox sampler against the NumPy restatement of tests/test_gibbs_cpu.py, chain and segment independence,
invariants on outlier data, agreement in distribution with the reference's own long runs, the benchmark's shape, limits, and the Python
surface."""
import contextlib
import io
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN, rel_err
from riemannhamiltonianmontecarlo_amd import RMHMC, _capi, auxiliary_gibbs, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_gibbs_cpu import GIBBS_TAPES, PhiloxDraws, flip_labels, gibbs_numpy, load_gibbs_tape

pytestmark = pytest.mark.gpu


def _tapes(g, n):
    T, N = g["u_sweep"].shape
    b = lambda a: np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape))
    return b(g["u_init"]), b(g["u_sweep"]), b(g["T"]), b(g["ks_draws"]), b(g["ks_offset"])


def philox_tapes(dr, attempts):
    """the replay entry point's five tapes from the sampler's own Philox streams, given the attempts (n, T, N) every row consumes"""
    n, T, N = attempts.shape
    off = np.concatenate([np.zeros((n, T, 1), np.int64), np.cumsum(attempts, axis=2)], axis=2)
    tot = attempts.sum(axis=2)                                          # (n, T) attempts per iteration
    off = off + np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(tot, axis=1)[:, :-1]], axis=1)[:, :, None]
    ks = np.zeros((n, int(tot.sum(axis=1).max()), 3))
    for it in range(T):
        for a in range(int(attempts[:, it].max())):
            Y, Ua, Ub = dr.ks(it, a, None)
            c, j = np.nonzero(attempts[:, it] > a)
            ks[c, off[c, it, j] + a] = np.stack([Y[c, j], Ua[c, j], Ub[c, j]], axis=1)
    return (dr.u_init(), np.stack([dr.u_sweep(i) for i in range(T)], axis=1), np.stack([dr.T(i) for i in range(T)], axis=1), ks, off)


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


class _OneUlpOff(PhiloxDraws):
    def u_init(self):
        return super().u_init() * (1 + 2.0 ** -52)


def _sample_vs_numpy(hip, XX, t, n, T, B, seed, follow=None, v=100.0):
    """gibbs_sample against gibbs_numpy on the same Philox streams; follow: the chain ids the restatement follows (default: all).
    The reference's proposal Y = 1 + (Y - sqrt(Y (4 r + Y))) / (2 r) (gibbs_sampler.py:59) cancels twice for a small residual r, so one
    rounding error in r comes back as ~ eps (Y / r)^2 in lam_j and, an iteration later, in beta: two correct evaluations of the file differ
    by 1e-10 .. 1e-5 after two or three iterations, depending on the smallest residual the case happens to meet.
    A case can carry the 1e-9 bound only where the restatement itself is stable to that level, so that is checked first, on the
    restatement alone: its samples move by <= 1e-10 when the initial uniforms move by one ulp.  Data, seeds and lengths below were
    chosen by that criterion, before any run on the device."""
    M, D = XX.shape
    ids = np.arange(n) if follow is None else np.asarray(follow)
    ref = gibbs_numpy(XX, t, T, PhiloxDraws(seed, ids, M, D), n=len(ids), v=v)
    own = rel_err(gibbs_numpy(XX, t, T, _OneUlpOff(seed, ids, M, D), n=len(ids), v=v)["beta"], ref["beta"])
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


def test_device_truncated_normal_far_tail(hip):
    """The device's own truncated normal beyond m/s = 25 (the asymptotic branch, which no tape reaches: |m/s| <= 2.4 there).  An
    intercept-dominated data set, nine labels 0 to one label 1, with the initial uniform of every label-0 row at 1e-300: Z_j = -37
    there, B_0 near -30, and the label-1 rows are drawn at m/s between 25 and 35 (counted on the restatement: at least 20 such
    draws).  Replay of the Philox streams with that u_init against the restatement: attempts equal, beta, B <= 1e-9, Z, lam <= 1e-8,
    every Z finite and on its label's side."""
    import test_gibbs_cpu as G
    M, D, n, T = 100, 2, 3, 3
    XX = np.c_[np.ones(M), np.random.RandomState(3).randn(M)]
    t = (np.arange(M) % 10 == 0).astype(np.float64)

    class Extreme(PhiloxDraws):
        def u_init(self):
            u = super().u_init().copy()
            u[:, t == 0] = 1e-300
            return u

    far = [0]
    orig = G.truncnorm_neg

    def counting(U, Uc, m, s):
        far[0] += int(np.sum(np.asarray(m) / np.asarray(s) > G.TAIL))
        return orig(U, Uc, m, s)

    G.truncnorm_neg = counting
    try:
        dr = Extreme(5, np.arange(n), M, D)
        ref = gibbs_numpy(XX, t, T, dr, n=n)
    finally:
        G.truncnorm_neg = orig
    assert far[0] >= 20 and np.all(ref["capped"] == 0), far
    with hip.context(M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        r = ctx.gibbs_replay(*philox_tapes(dr, ref["attempts"]))
    assert np.all(r["status"] == 0) and np.all(r["capped"] == 0)
    np.testing.assert_array_equal(r["attempts"], ref["attempts"])
    assert np.all(np.isfinite(r["Z"])) and np.all(np.sign(r["Z"]) == np.where(t == 1, 1.0, -1.0)[None])
    errs = {k: rel_err(r[k], ref[k]) for k in ("beta", "B", "Z", "lam")}
    print("far tail, %d draws beyond m/s = 25:" % far[0], errs)
    assert errs["beta"] <= 1e-9 and errs["B"] <= 1e-9 and errs["Z"] <= 1e-8 and errs["lam"] <= 1e-8, errs


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
