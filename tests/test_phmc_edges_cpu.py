"""CPU-side checks of tests/helpers/phmc_edges.py: the conditions that concern the references alone, so that no GPU test of
tests/test_gpu_phmc_edges.py can pass by leaving a case out or by comparing against a reference that hangs on a rounding.

The transition references must be finite, away from a tie (1e-6, the margin of tests/test_gpu_phmc.py) and hold the planted trajectory
lengths; the sampler references must accept and reject, spread their trajectory lengths within an iteration (so that the chains of a
workgroup begin transitions at different global steps) and not move when every momentum normal is one ulp off.
The Philox streams and the iteration convention of the sampler reference are pinned to the CPU oracle's plain HMC sampler."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import phmc_edges as E  # noqa: E402

TRANSITIONS = [(c, b) for c in E.D_CASES + E.N_CASES for b in E.BETAS]


def _tid(p):
    case, beta = p
    return "%s-%s" % (case.id, "phmc" if beta is None else "beta%g" % beta)


def test_tables_are_whole():
    """every edge the tables are there for, each exactly once, and every row parametrised below"""
    assert [c.D for c in E.D_CASES] == [16, 17, 32, 47, 48, 49, 63, 127, 128, 129, 191, 192, 193, 255]
    assert all((c.M, c.n, c.zero_steps) == (300, 18, (5, 16, 17)) for c in E.D_CASES)
    assert sorted(set(E.ndb_of(c.D) for c in E.D_CASES)) == [1, 2, 3, 4, 8, 12, 16]
    assert [(c.M, c.D, c.n) for c in E.N_CASES] == [(200, 20, n) for n in (1, 15, 16, 17, 32, 33, 65)] + [(300, 129, n) for n in (16, 17, 33)]
    assert E.BETAS == (None, 0.3)
    assert [(c.M, c.D, c.n, c.beta) for c in E.SAMPLER_CASES] == [
        (300, 17, 33, None), (300, 49, 18, None), (300, 49, 18, 0.3), (300, 128, 18, None), (300, 129, 18, None), (300, 129, 18, 0.3),
        (300, 255, 18, None)]
    assert (E.SAMPLER_T, E.SAMPLER_BURN_IN, E.L, E.EPS, E.SAMPLER_SEED, E.SAMPLER_OFFSET) == (6, 2, 8, 0.5, 2 ** 40 + 31, 7)
    assert E.PLANT_SHAPES == [(300, 129, 18), (300, 49, 18)] and E.PLANTED == (5, 17) and len(E.PLANT_KINDS) == 3
    assert E.PRIOR_D == (1, 2, 63, 64, 65, 255) and (E.PRIOR_N, E.PRIOR_SEED, E.PRIOR_OFFSET) == (18, 2 ** 40 + 5, 9)
    assert len(TRANSITIONS) == (len(E.D_CASES) + len(E.N_CASES)) * len(E.BETAS) == 48
    ids = [c.id for c in E.D_CASES + E.N_CASES + E.SAMPLER_CASES]
    assert len(set(ids)) == len(ids) and all(c.why for c in E.D_CASES + E.N_CASES + E.SAMPLER_CASES)
    for D, ndb in ((1, 1), (16, 1), (17, 2), (64, 4), (65, 8), (128, 8), (129, 12), (192, 12), (193, 16), (256, 16)):
        assert E.ndb_of(D) == ndb


@pytest.mark.parametrize("case,beta", TRANSITIONS, ids=[_tid(p) for p in TRANSITIONS])
def test_transition_reference(case, beta):
    inp, ref = E.case_inputs(case, beta), E.case_reference(case, beta)
    assert len(ref["w"]) == case.n and inp["u_len"][0] == 1.0
    assert (ref["status"] == 0).all() and np.isfinite(ref["H_prop"]).all() and np.isfinite(ref["H_cur"]).all()
    assert (np.abs(ref["margin"]) > 1e-6).all(), np.abs(ref["margin"]).min()
    assert ref["nsteps"][0] == E.L
    zero = list(case.zero_steps)
    assert np.array_equal(np.flatnonzero(ref["nsteps"] == 0), zero)
    assert (ref["accepted"][zero] == 1).all() and np.array_equal(ref["w_prop"][zero], inp["w"][zero])
    assert np.array_equal(ref["w"][zero], inp["w"][zero])
    if beta is not None:
        assert np.isfinite(ref["loglik0"]).all() and np.array_equal(ref["loglik"][zero], ref["loglik0"][zero])
    if case.n > 1:      # (a batch of one holds the full-length chain alone)
        assert 0 < ref["accepted"].sum() and len(set(ref["nsteps"].tolist())) >= min(case.n, 4)


def test_number_of_cases():
    """the parametrised tests of this file and of tests/test_gpu_phmc_edges.py cover the tables row by row"""
    import test_gpu_phmc_edges as G
    assert len(G.TRANSITIONS) == len(TRANSITIONS) and [(_tid(p)) for p in G.TRANSITIONS] == [_tid(p) for p in TRANSITIONS]
    assert G.SAMPLERS == E.SAMPLER_CASES
    assert len(G.PLANTS) == len(E.PLANT_SHAPES) * len(E.PLANT_KINDS) * len(E.BETAS) == 12
    assert tuple(G.PRIOR_D) == E.PRIOR_D
    for name, count in (("test_transition_at_edges", 48), ("test_sampler_matches_chained_restatement", 7),
                        ("test_planted_chain_is_alone_at_edges", 12), ("test_ais_prior_is_the_philox_stream", 6)):
        marks = [m for m in getattr(G, name).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and len(marks[0].args[1]) == count, name
        assert not [m for m in getattr(G, name).pytestmark if m.name in ("skip", "skipif", "xfail")]


@pytest.mark.parametrize("case", E.SAMPLER_CASES, ids=[c.id for c in E.SAMPLER_CASES])
def test_sampler_reference(case):
    ref = E.sampler_reference(case)
    assert ref["samples"].shape == (case.n, E.SAMPLER_T, case.D) and np.isfinite(ref["samples"]).all() and (ref["status"] == 0).all()
    assert ref["margin"] > 1e-6, ref["margin"]
    assert (ref["accepted"] == 1).any() and (ref["accepted"] == 0).any()
    assert len(set(ref["nsteps"][:, 0].tolist())) >= 4 and ref["nsteps"].min() >= 1 and ref["nsteps"].max() == E.L
    # z one ulp off: the same decisions, samples that do not move (measured: at most 1.1e-15 relative)
    off = E.sampler_reference(case, z_factor=1.0 + 2.0 ** -52)
    moved = rel_err(off["samples"], ref["samples"])
    print(case.id, "margin %.2e, accepted %d of %d, lengths in iteration 0: %s, one ulp in z moves the samples by %.1e" % (
        ref["margin"], ref["accepted"].sum(), ref["accepted"].size, sorted(set(ref["nsteps"][:, 0].tolist())), moved))
    assert np.array_equal(off["accepted"], ref["accepted"]) and np.array_equal(off["nsteps"], ref["nsteps"])
    assert moved < 1e-12
    if case.beta is not None:
        assert np.isfinite(ref["loglik0"]).all() and np.isfinite(ref["loglik"]).all()


def test_streams_are_the_oracle_draws(oracle):
    """hmc_streams against the oracle's own recipe (rmhmc_oracle_draws), the prior's iteration counter included"""
    import ctypes as C
    lib = C.CDLL(oracle.path)
    lib.rmhmc_oracle_draws.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.rmhmc_oracle_draws.restype = None
    seed, D = 2 ** 40 + 31, 17
    chains = [0, 7, 2 ** 32 + 5]
    for it in (0, 5, E.PRIOR_ITER):
        z, u_len, u_acc = E.hmc_streams(seed, chains, D, it)
        for i, c in enumerate(chains):
            zo = np.empty(D + 1); u3 = np.empty(3)
            lib.rmhmc_oracle_draws(seed, c, it, D, zo.ctypes.data_as(C.POINTER(C.c_double)), u3.ctypes.data_as(C.POINTER(C.c_double)))
            assert u_len[i] == u3[0] and u_acc[i] == u3[2]               # the uniforms are exact on both sides
            assert np.abs(z[i] - zo[:D]).max() <= 8 * 2.0 ** -53 * 9.0   # Box-Muller on libm and NumPy: a few ulp of |z| < 9


@pytest.mark.parametrize("eps", [E.EPS, 0.1])
def test_sampler_reference_with_identity_mass_is_the_oracle_hmc(oracle, eps):
    """sampler_ref under the identity mass is rmhmc_hmc_sample: the streams, the iteration counter, which iterations are saved and
    which are counted.  eps 0.5 is the step size of the sampler table, at which plain HMC rejects every proposal on these data (the
    trajectory lengths are still compared); at 0.1 it accepts 26 of 30, so the normals and the acceptance uniforms are compared too."""
    M, D, n = 300, 17, 5
    pr = E.identity_problem(M, D)
    theta0 = 0.1 * np.random.RandomState(M + D).randn(n, D)
    T, B = E.SAMPLER_T, E.SAMPLER_BURN_IN
    with oracle.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        samples, acc, steps, _ = ctx.hmc_sample(T, B, L=E.L, eps=eps, seed=E.SAMPLER_SEED, chain_offset=E.SAMPLER_OFFSET, theta0=theta0)
    ref = E.sampler_ref(pr, theta0, T, E.L, eps, E.SAMPLER_SEED, E.SAMPLER_OFFSET)
    err = rel_err(ref["samples"][:, B:], samples)
    print("eps %g: accepted %s, steps %s, samples %.1e, margin %.2e" % (eps, acc, steps, err, ref["margin"]))
    assert np.array_equal(ref["accepted"].sum(axis=1), acc)               # every iteration counts
    assert np.array_equal(ref["nsteps"][:, B + 1:].sum(axis=1), steps)    # the iterations after burn_in + 1
    assert err < 1e-12
    if eps < E.EPS:
        assert 0 < acc.sum() < n * T and (np.diff(samples, axis=1) != 0).any()
