"""GPU tests of fixed-metric HMC (csrc/phmc.hip.h), its tempered form and the prior draws of annealed importance sampling
(csrc/ais.hip.h) at every chain slot of a 16-chain workgroup and at the tile edges of D, against the NumPy restatements.  The tables,
inputs and references are those of tests/helpers/phmc_edges.py; tests/test_phmc_edges_cpu.py holds the references to their own conditions
(finite, away from a tie, the planted trajectory lengths) and pins the sampler reference's streams to the CPU oracle.

Tolerances are the project's (tests/test_gpu_phmc.py, from tests/test_gpu_parity.py): step counts, decisions and status equal, 1e-9 on
a transition's outputs, 1e-8 on samples.  The transition errors are taken per chain, relative to that chain's own reference, so that a
failure names the chain slot; the batch-wide rel_err of the existing tests is never larger than what is asserted here.

Measured on an MI355X: the worst per-chain error of a transition 1.1e-15 (NDB 1), 2.3e-15 (2), 1.7e-15 (3), 2.0e-15 (4), 3.7e-15 (8),
8.0e-15 (12), 9.0e-15 (16); samples after six iterations 6e-16 ... 5.2e-15, the final loglik 1.1e-15; the prior draws at most 0.05 of
their bound (7.1e-15 absolute).  With the tails reading the product row of chain j & 3 for NDB >= 8 (a scratch build) every D > 64
case of tests 1 and 2 fails and nothing else in this file, tests/test_gpu_phmc.py or tests/test_gpu_ais.py does."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import phmc_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

TRANSITIONS = [(c, b) for c in E.D_CASES + E.N_CASES for b in E.BETAS]
SAMPLERS = E.SAMPLER_CASES
PLANTS = [(s, k, b) for s in E.PLANT_SHAPES for k in E.PLANT_KINDS for b in E.BETAS]
PRIOR_D = E.PRIOR_D
VECTORS, SCALARS = ("w_prop", "p_prop", "w"), ("H_prop", "H_cur")


def _beta_id(beta):
    return "phmc" if beta is None else "beta%g" % beta


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def transition(ctx, inp, beta):
    with np.errstate(all="ignore"):
        if beta is None:
            return ctx.phmc_transition(inp["w"], inp["z"], inp["u_len"], inp["u_acc"], L=E.L, eps=E.EPS)
        return ctx.tphmc_transition(inp["w"], inp["z"], inp["u_len"], inp["u_acc"], L=E.L, eps=E.EPS, beta=beta)


def chain_err(got, ref):
    """the error of every chain relative to its own reference: [n]"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.ndim == 1:
        got, ref = got[:, None], ref[:, None]
    return np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)


def slot(c):
    return "chain %d (workgroup %d, wavefront %d, slot jj %d, product column %d)" % (c, c // 16, c % 4, (c % 16) // 4, c % 16)


# ---- 1. one transition at every chain slot and tile edge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case,beta", TRANSITIONS, ids=["%s-%s" % (c.id, _beta_id(b)) for c, b in TRANSITIONS])
def test_transition_at_edges(hip, case, beta):
    st, inp, ref = E.stage(case.M, case.D, beta), E.case_inputs(case, beta), E.case_reference(case, beta)
    with hip.context(case.M, case.D, case.n) as ctx:
        ctx.set_data(st["XX"], st["t"])
        ctx.phmc_set_mass(st["Mass"])
        got = transition(ctx, inp, beta)
    keys = VECTORS + SCALARS + (() if beta is None else ("loglik0", "loglik"))
    errs = {k: chain_err(got[k], ref[k]) for k in keys}
    worst = max(keys, key=lambda k: errs[k].max())
    print("%s %s NDB %d: worst %s %.1e at %s; margin min %.2e | %s" % (case.id, _beta_id(beta), E.ndb_of(case.D), worst, errs[worst].max(),
                                                                      slot(int(errs[worst].argmax())), np.abs(ref["margin"]).min(), case.why))
    for k in ("nsteps", "accepted", "status"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (k, [slot(int(c)) for c in bad], got[k][bad], ref[k][bad])
    for k in keys:
        bad = np.flatnonzero(~(errs[k] < 1e-9))
        assert bad.size == 0, (k, [(slot(int(c)), errs[k][c]) for c in bad])
    for c in case.zero_steps:        # a trajectory of zero steps: the proposal is the current point itself
        assert got["nsteps"][c] == 0 and got["accepted"][c] == 1, slot(c)
        assert same_bits(got["w"][c], inp["w"][c]) and same_bits(got["w_prop"][c], inp["w"][c]), slot(c)
        if beta is not None:
            assert same_bits(got["loglik"][c], got["loglik0"][c]), slot(c)


# ---- 2. the sampler against the chained restatement ---------------------------------------------------------------------------------------
def run_sampler(hip, case, options=None):
    st = E.stage(case.M, case.D, case.beta)
    kw = dict(L=E.L, eps=E.EPS, seed=E.SAMPLER_SEED, chain_offset=E.SAMPLER_OFFSET, theta0=E.sampler_theta0(case), samples=True)
    with hip.context(case.M, case.D, case.n, options=options) as ctx:
        ctx.set_data(st["XX"], st["t"])
        ctx.phmc_set_mass(st["Mass"])
        if case.beta is None:
            return ctx.phmc_sample_to(E.SAMPLER_T, E.SAMPLER_BURN_IN, **kw)
        return ctx.tphmc_sample_to(E.SAMPLER_T, E.SAMPLER_BURN_IN, beta=case.beta, **kw)


@pytest.mark.parametrize("case", SAMPLERS, ids=[c.id for c in SAMPLERS])
def test_sampler_matches_chained_restatement(hip, case):
    ref = E.sampler_reference(case)
    got = run_sampler(hip, case)
    B = E.SAMPLER_BURN_IN
    want = ref["samples"][:, B:]
    per_chain = np.abs(got["samples"] - want).reshape(case.n, -1).max(axis=1) / np.abs(want).reshape(case.n, -1).max(axis=1)
    ll = "" if case.beta is None else ", loglik0 %.1e, loglik %.1e" % (chain_err(got["loglik0"], ref["loglik0"]).max(),
                                                                      chain_err(got["loglik"], ref["loglik"]).max())
    print("%s: samples %.1e (worst at %s)%s; margin %.2e, accepted %d of %d | %s" % (
        case.id, per_chain.max(), slot(int(per_chain.argmax())), ll, ref["margin"], ref["accepted"].sum(), ref["accepted"].size, case.why))
    assert got["samples"].shape == want.shape
    assert np.array_equal(got["accepted"], ref["accepted"].sum(axis=1))                    # every iteration counts
    assert np.array_equal(got["leapfrog_steps"], ref["nsteps"][:, B + 1:].sum(axis=1))     # the iterations after burn_in + 1
    bad = np.flatnonzero(~(per_chain < 1e-8))
    assert bad.size == 0, [(slot(int(c)), per_chain[c]) for c in bad]
    assert rel_err(got["samples"], want) < 1e-8
    if case.beta is not None:
        for k in ("loglik0", "loglik"):
            e = chain_err(got[k], ref[k])
            assert (e < 1e-9).all(), (k, slot(int(e.argmax())), e.max())
    if case.D == 129:                            # no captured graph, chains in the caller's order: the same bits
        other = run_sampler(hip, case, {"graph": 0, "sorted": 0})
        for k in ("samples", "accepted", "leapfrog_steps") + (() if case.beta is None else ("loglik0", "loglik")):
            assert same_bits(got[k], other[k]), k


# ---- 3. a failing chain is alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,beta", PLANTS, ids=["%dx%dx%d-%s-%s" % (s + (k, _beta_id(b))) for s, k, b in PLANTS])
def test_planted_chain_is_alone_at_edges(hip, shape, kind, beta):
    M, D, n = shape
    st, planted, twin = E.plant_case(M, D, n, kind, beta)
    ref = E.reference(st, planted)
    with hip.context(M, D, n) as ctx:
        ctx.set_data(st["XX"], st["t"])
        ctx.phmc_set_mass(st["Mass"])
        bad = transition(ctx, planted, beta)
        good = transition(ctx, twin, beta)
    others = [c for c in range(n) if c not in E.PLANTED]
    assert (good["status"] == 0).all() and good["accepted"].sum() > 0 and (ref["status"][others] == 0).all()
    for c in E.PLANTED:
        assert bad["accepted"][c] == 0 and bad["status"][c] & 2, (slot(c), bad["status"][c])
        assert same_bits(bad["w"][c], planted["w"][c]), slot(c)
        assert ref["accepted"][c] == 0 and ref["status"][c] & 2
        if beta is not None and kind.startswith("w_"):
            assert np.isnan(bad["loglik0"][c]), (slot(c), bad["loglik0"][c])
    for k in bad:                                 # every other chain: the same bits in every output
        for c in others:
            assert same_bits(bad[k][c], good[k][c]), (k, slot(c))
    assert np.array_equal(bad["nsteps"], ref["nsteps"])
    if kind == "z_nan":
        assert np.array_equal(bad["status"], ref["status"]), (bad["status"], ref["status"])


# ---- 4. the prior draws are the Philox stream -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", PRIOR_D)
def test_ais_prior_is_the_philox_stream(hip, D):
    n, seed, off = E.PRIOR_N, E.PRIOR_SEED, E.PRIOR_OFFSET
    want, bound = E.prior_reference(D)
    XX, t = synthetic_logreg(20, D, 0)
    with hip.context(20, D, n) as ctx:
        ctx.set_data(XX, t)
        got = ctx.ais_prior(seed, off)
    with hip.context(20, D, off + n) as ctx:
        ctx.set_data(XX, t)
        wide = ctx.ais_prior(seed, 0)
    ratio = np.abs(got - want) / bound
    c, d = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print("D %d: worst |error| / bound %.3f at chain %d, d %d; max |error| %.1e" % (D, ratio.max(), c, d, np.abs(got - want).max()))
    assert got.shape == (n, D) and np.isfinite(got).all()
    assert (ratio <= 1.0).all(), (ratio.max(), c, d)
    assert same_bits(wide[off:off + n], got)       # the chain's global id keys the stream, not its place in the batch
