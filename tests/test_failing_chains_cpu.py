"""CPU half of tests/test_gpu_failing_chains.py: the planted batches, sampler regimes and HMC / mMALA plants of
tests/helpers/failing_chains.py on the CPU oracle.  It keeps the GPU tests from becoming vacuous: the plants really raise every status
bit, the chains the GPU file compares to a tolerance are insensitive to the last bits of their inputs, the samplers really run in a
regime where trajectories fail and the chain then carries on, and there the oracle's own sampler is stable enough to be a reference."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import failing_chains as F  # noqa: E402

CASES = [(p, m) for p in F.N_CHAINS for m in F.MODES]
TINY = 1.0 + 2.0 ** -48


@pytest.mark.parametrize("n", sorted(set(F.N_CHAINS.values())) + [129, 300])
def test_plant_positions_cover_the_edges(n):
    pos = F.plant_positions(n)
    assert {0, 15, 16, n - 1} <= set(pos) and len(pos) >= len(F.KINDS) and len(set(pos)) == len(pos)
    if n > 128:
        assert {127, 128} <= set(pos)
    for g in range(n // 16):                                   # (full groups; a ragged last one may hold two required positions)
        assert sum(p // 16 == g for p in pos) <= 8, (n, pos)


@pytest.mark.parametrize("path", list(F.N_CHAINS))
def test_every_kind_is_planted_and_shapes_stay_on_their_path(path):
    assert {k for _, k in F.plants_of(path)} == set(F.KINDS)
    for mode in F.MODES:
        spec, planted, twin, plants = F.make_case(path, mode)
        F.assert_shape_on_path(path, spec)
        rows = [c for c, _ in plants]
        keep = np.setdiff1d(np.arange(spec[2]), rows)
        for k in planted:
            assert np.array_equal(planted[k][keep], twin[k][keep])
        assert np.isfinite(twin["w"]).all() and np.isfinite(twin["z"]).all()
        F.assert_shape_on_path(path, F.sampler_spec(path)[0])


@pytest.mark.parametrize("path,mode", CASES)
def test_plants_raise_every_status_bit_on_the_oracle(oracle, path, mode):
    spec, planted, twin, plants = F.make_case(path, mode)
    r = F.oracle_transition(oracle, path, mode)
    st = r["status"]
    assert np.bitwise_or.reduce(st) == (15 if mode == "compat" else 3)
    planted_rows = np.zeros(spec[2], dtype=bool); planted_rows[[c for c, _ in plants]] = True
    assert (st[~planted_rows] == 0).mean() >= 0.9
    assert r["accepted"][~planted_rows].mean() >= 0.94
    for c, kind in plants:
        if kind in F.POISONED or mode == "plain":
            assert st[c] & F.FAIL and r["accepted"][c] == 0 and np.array_equal(r["w"][c], planted["w"][c], equal_nan=True), (c, kind)
        if kind in F.MOMENTUM_GUARD and mode == "compat":         # renormalised: the trajectory is an ordinary one
            assert st[c] == _capi.ST_GUARD_P and r["accepted"][c] == 1 and np.isfinite(r["H_prop"][c]), (c, kind)
    with F.context(oracle, spec) as ctx:                         # (the twin is a batch of well-behaved chains)
        good = F.transition(ctx, twin)
    assert (good["status"] == 0).mean() >= 0.9 and np.isfinite(good["w_prop"]).all()


@pytest.mark.parametrize("path,mode", CASES)
def test_finite_plants_are_insensitive_to_the_last_bits(oracle, path, mode):
    """The plants the GPU file compares to 1e-8 (no failure bit on the oracle) move by < 1e-10 when w and z are scaled by 1 + 2^-48: what
    separates the libraries there is rounding, not a trajectory on the edge of failing."""
    spec, planted, _, plants = F.make_case(path, mode)
    r = F.oracle_transition(oracle, path, mode)
    moved = dict(planted, w=planted["w"] * TINY, z=planted["z"] * TINY)
    with F.context(oracle, spec) as ctx:
        r2 = F.transition(ctx, moved)
    assert np.array_equal(r2["status"], r["status"]) and np.array_equal(r2["accepted"], r["accepted"])
    for c, kind in plants:
        if r["status"][c] & F.FAIL:
            continue
        s = rel_err(r2["w_prop"][c], r["w_prop"][c])
        print("%s %s chain %d (%s): self-sensitivity %.1e" % (path, mode, c, kind, s))
        assert s < 1e-10, (c, kind, s)


@pytest.mark.parametrize("path", list(F.SAMPLER_CASES))
def test_sampler_regime_fails_and_carries_on(oracle, path):
    """20 transitions from w = 0 with NumPy draws: at least a quarter of the chains see a failed trajectory followed by an accepted one,
    and the chains move (mean acceptance >= 0.05)"""
    mode, eps, _ = F.SAMPLER_CASES[path]
    spec = F.spec_of(path, mode, F.REGIME_N)
    M, D, n = spec[:3]
    rs = np.random.RandomState(6000 + spec[4])
    w = np.zeros((n, D))
    failed = np.zeros(n, dtype=bool); carried_on = np.zeros(n, dtype=bool); acc = 0.0
    with F.context(oracle, spec) as ctx:
        for _ in range(F.REGIME_ITERS):
            with np.errstate(all="ignore"):
                r = ctx.transition(w, rs.randn(n, D), rs.rand(n), rs.randn(n), rs.rand(n), L=F.SAMPLER_L, eps=eps, K=F.SAMPLER_K)
            a = r["accepted"] != 0
            carried_on |= failed & a
            failed |= (r["status"] & F.FAIL) != 0
            assert not (a & ((r["status"] & F.FAIL) != 0)).any()
            acc += a.mean() / F.REGIME_ITERS
            w = r["w"]
    print("%s %s eps %.1f: %.2f of the chains fail and carry on, acceptance %.3f" % (path, mode, eps, carried_on.mean(), acc))
    assert carried_on.mean() >= 0.25 and acc >= 0.05
    assert np.isfinite(w).all()


@pytest.mark.parametrize("path", list(F.SAMPLER_CASES))
def test_oracle_sampler_is_stable_in_that_regime(oracle, path):
    """theta0 scaled by 1 + 2^-48: the same accept decisions and samples within 1e-9, which licenses the 1e-7 of the GPU comparison"""
    spec, eps = F.sampler_spec(path)
    th = F.sampler_theta0(spec)
    with F.context(oracle, spec) as ctx:
        a = F.sample(ctx, eps, th)
        b = F.sample(ctx, eps, th * TINY)
    assert np.array_equal(a["accepted"], b["accepted"]) and np.array_equal(a["leapfrog_steps"], b["leapfrog_steps"])
    assert np.isfinite(a["samples"]).all()
    move = float(np.abs(a["samples"] - b["samples"]).max())
    print("%s: samples move by %.1e" % (path, move))
    assert move < 1e-9
    assert 0 < a["accepted"].sum() < a["accepted"].size * F.SAMPLER_T


@pytest.mark.parametrize("name", list(F.HMC_SHAPES))
def test_hmc_plant_ends_in_a_nan_momentum(oracle, name):
    M, D, n, XX, t, planted, twin, c, eps = F.hmc_case(name)
    with oracle.context(M, D, n) as ctx:
        ctx.set_data(XX, t, 100.0)
        r = F.hmc_transition(ctx, planted, eps)
    assert np.isnan(r["p_prop"][c]).any() and r["accepted"][c] == 0 and np.array_equal(r["w"][c], planted["w"][c])
    keep = np.arange(n) != c
    assert np.isfinite(r["p_prop"][keep]).all() and np.isfinite(r["w"]).all() and r["accepted"][keep].sum() > 0


@pytest.mark.parametrize("name", list(F.MMALA_SHAPES))
def test_mmala_plant_is_rejected_on_the_oracle(oracle, name):
    spec, planted, twin, c = F.mmala_case(name)
    with F.context(oracle, spec) as ctx:
        r = F.mmala_transition(ctx, planted)
        good = F.mmala_transition(ctx, twin)
    assert r["accepted"][c] == 0 and np.array_equal(r["w"][c], planted["w"][c], equal_nan=True)
    keep = np.arange(spec[2]) != c
    for k in r:
        assert F.same_bits(r[k][keep], good[k][keep]), k
    assert good["accepted"].sum() > 0
