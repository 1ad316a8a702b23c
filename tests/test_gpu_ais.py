"""GPU tests of annealed importance sampling with tempered fixed-metric HMC (include/rmhmc_ais.h, csrc/ais.hip.h): the tempered sampler
at beta = 1 against the fixed-metric HMC sampler (bit for bit), the tempered transition against the NumPy restatement
tests/helpers/ais_ref.py, rmhmc_ais_run against the composition of the public pieces (bit for bit), the weight reduction against
np.longdouble, and the estimate of the evidence against a quadrature.

GPU-versus-restatement tolerances are those of tests/test_gpu_phmc.py (from tests/test_gpu_parity.py): step counts, decisions and
status equal, 1e-9 on w_prop, p_prop, the Hamiltonians and the two log-likelihoods; no decision of the restatement within 1e-6 of a tie.
The bounds of the weight reduction are derived in tests/test_ais_cpu.py."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, rel_err
from riemannhamiltonianmontecarlo_amd import _capi, log_evidence
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ais_ref as A  # noqa: E402
import phmc_ref as R  # noqa: E402
from test_ais_cpu import N_CHAINS, PROBLEMS, check_finish, quadrature, weight_cases  # noqa: E402
from test_gpu_phmc import DENSE, draws, problem, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
ALPHA = 100.0


def H_lik(pr):
    return pr["G"] - np.eye(len(pr["G"])) / ALPHA


# ---- 1. beta = 1 is the fixed-metric HMC sampler, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("M,D,n", [(690, 15, 4), (300, 64, 17), (250, 150, 3)])
def test_beta_one_is_phmc(hip, M, D, n, graph):
    pr = problem(M, D)
    w, z, u_len, u_acc = draws(pr, n, M + D)
    eps = 0.5 if D < 100 else 0.05     # (M = 250 < 2 D: the step size of the other shapes overflows every trajectory, in PHMC itself)
    kw = dict(L=8, eps=eps, seed=8, chain_offset=3, theta0=w, samples=True, stats=True)
    with hip.context(M, D, n, options={"graph": graph}) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        ctx.phmc_set_mass(pr["G"])
        p = ctx.phmc_transition(w, z, u_len, u_acc, L=8, eps=eps)
        q = ctx.tphmc_transition(w, z, u_len, u_acc, L=8, eps=eps, beta=1.0)
        ps = ctx.phmc_sample_to(24, 4, **kw)
        qs = ctx.tphmc_sample_to(24, 4, beta=1.0, **kw)
    assert p["nsteps"][0] == 8 and (p["status"] == 0).all() and p["accepted"].sum() > 0
    for k in p:
        assert same_bits(p[k], q[k]), k
    for k in ("samples", "mean", "var", "ess", "accepted", "leapfrog_steps"):
        assert same_bits(ps[k], qs[k]), k
    assert ps["accepted"].sum() > 0 and ps["leapfrog_steps"].sum() > 0
    # the log-likelihoods beside them: at the start, and at the state the call returned
    ll = np.array([A.loglik(pr["XX"], pr["t"], x) for x in w])
    assert rel_err(q["loglik0"], ll) < 1e-9 and same_bits(qs["loglik0"], q["loglik0"])
    assert rel_err(q["loglik"], np.array([A.loglik(pr["XX"], pr["t"], x) for x in q["w"]])) < 1e-9
    assert rel_err(qs["loglik"], np.array([A.loglik(pr["XX"], pr["t"], x) for x in qs["samples"][:, -1]])) < 1e-9


# ---- 2. the tempered transition against the restatement ---------------------------------------------------------------------------------
def tempered_draws(pr, n, beta, seed):
    """starts from N(mode_beta, Mass^-1), Mass = beta H + I / alpha (beta = 0: the prior itself), momentum normals, the two uniforms"""
    D = pr["XX"].shape[1]
    rs = np.random.RandomState(seed)
    Mass = A.stage_mass_matrix(beta, H_lik(pr))
    Lm = np.linalg.cholesky(Mass)
    centre = A.mode(pr["XX"], pr["t"], beta)
    w = np.stack([centre + R.solve_upper(Lm.T, rs.randn(D)) for _ in range(n)])
    z = rs.randn(n, D)
    u_len = rs.uniform(0.05, 1.0, n); u_acc = rs.uniform(0.05, 1.0, n)
    u_len[0] = 1.0
    return Mass, Lm, w, z, u_len, u_acc


@pytest.mark.parametrize("beta", [0.0, 1e-6, 0.3, 1.0])
@pytest.mark.parametrize("M,D,n,scale", DENSE + [(200, 16, 33, 1.0), (200, 17, 16, 1.0)])
def test_tempered_transition_matches_restatement(hip, M, D, n, scale, beta):
    pr = problem(M, D, scale)
    Mass, Lm, w, z, u_len, u_acc = tempered_draws(pr, n, beta, M + D)
    ref = A.transitions(pr["XX"], pr["t"], Lm, w, z, u_len, u_acc, 8, 0.5, beta)
    assert ref["nsteps"][0] == 8
    with hip.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        ctx.phmc_set_mass(Mass)
        got = ctx.tphmc_transition(w, z, u_len, u_acc, L=8, eps=0.5, beta=beta)
    print("beta %g: margin min %.2e  w_prop %.1e  p_prop %.1e  H_cur %.1e  H_prop %.1e  loglik0 %.1e  loglik %.1e" % (
        beta, np.abs(ref["margin"]).min(), rel_err(got["w_prop"], ref["w_prop"]), rel_err(got["p_prop"], ref["p_prop"]),
        rel_err(got["H_cur"], ref["H_cur"]), rel_err(got["H_prop"], ref["H_prop"]), rel_err(got["loglik0"], ref["loglik0"]),
        rel_err(got["loglik"], ref["loglik"])))
    assert (np.abs(ref["margin"]) > 1e-6).all() and np.isfinite(ref["H_prop"]).all()
    assert np.array_equal(got["nsteps"], ref["nsteps"]) and np.array_equal(got["accepted"], ref["accepted"])
    assert np.array_equal(got["status"], ref["status"])
    for k in ("w_prop", "p_prop", "H_prop", "H_cur", "w", "loglik0", "loglik"):
        assert rel_err(got[k], ref[k]) < 1e-9, k


# ---- 3. the run is the composition of the public pieces, bit for bit --------------------------------------------------------------------
def compose(ctx, theta0, beta0, beta, stage_len, stage_mass, H, L, eps, seed, chain_offset):
    """rmhmc_ais_run as its header describes it, from the caller's side"""
    import torch
    n, D = ctx.n, ctx.D
    theta = ctx.ais_prior(seed, chain_offset) if theta0 is None else np.array(theta0, dtype=np.float64)
    logw = np.zeros(n)
    prev = beta0
    trace = []
    for k, b in enumerate(beta):
        if stage_mass is not None and stage_mass[k]:
            try:
                ctx.phmc_set_mass(b * H + np.eye(D) * (1.0 / ALPHA))
            except _capi.RmhmcError:
                pass                                   # refused: the previous mass stays
        r = ctx.tphmc_sample_to(int(stage_len[k]), 0, L=L, eps=eps, beta=b, seed=(seed + 1 + k) % 2 ** 64, chain_offset=chain_offset,
                                theta0=theta, samples=True)
        with np.errstate(invalid="ignore"):
            logw = np.where(np.isfinite(r["loglik0"]), logw + (b - prev) * r["loglik0"], np.nan)
        theta = r["samples"][:, -1].copy()
        trace.append(r["accepted"].sum() / (n * float(stage_len[k])))
        prev = b
    part = ctx.ais_partial(torch.from_numpy(logw).to(torch.device("cuda", ctx.device))).cpu().numpy()
    return dict(logw=logw, theta=theta, accept_trace=np.array(trace), partial=part)


def mass_probe(ctx, pr):
    """what the context's mass does to one transition: equal bits, equal mass"""
    w, z, u_len, u_acc = draws(pr, ctx.n, 77)
    return ctx.phmc_transition(w, z, u_len, u_acc, L=4, eps=0.5)


@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("M,D,n", [(300, 20, 64), (250, 150, 16)])
def test_run_equals_composition(hip, M, D, n, graph):
    pr = problem(M, D)
    H = H_lik(pr)
    beta = np.array([0.01, 0.1, 0.3, 0.7, 1.0]); stage_len = [1, 2, 1, 3, 1]; stage_mass = [1, 0, 1, 0, 1]
    # stage_len 12 >= 8 global steps: the stage replays a captured graph where the option allows it
    cases = [dict(theta0=None, beta0=0.0), dict(theta0=draws(pr, n, 3)[0], beta0=0.3), dict(theta0=None, beta0=0.0, long=True)]
    for case in cases:
        sl = [12, 2, 1, 3, 1] if case.get("long") else stage_len
        kw = dict(L=6, eps=0.5 if D < 100 else 0.05, seed=2 ** 64 - 3, chain_offset=5)   # (the step size: as in test_beta_one_is_phmc)
        out = []
        for mode in ("run", "compose", "run"):         # a fresh context each: the second run repeats the bits of the first
            with hip.context(M, D, n, options={"graph": graph}) as ctx:
                ctx.set_data(pr["XX"], pr["t"])
                ctx.phmc_set_mass(None)
                if mode == "run":
                    r = ctx.ais_run(beta, sl, stage_mass, H, beta0=case["beta0"], theta0=case["theta0"], **kw)
                else:
                    r = compose(ctx, case["theta0"], case["beta0"], beta, sl, stage_mass, H, **kw)
                r["probe"] = mass_probe(ctx, pr)
                out.append(r)
        run, comp, again = out
        for k in ("logw", "theta", "accept_trace", "partial"):
            assert same_bits(run[k], comp[k]), (k, case["beta0"])
            assert same_bits(run[k], again[k]), k
        for k in run["probe"]:                          # the final mass is the last one installed, beta = 1: the metric at the mode
            assert same_bits(run["probe"][k], comp["probe"][k]), k
        assert np.isfinite(run["logw"]).all() and run["n_nan"] == 0 and run["m"] == n and run["accept_trace"].sum() > 0
        assert run["seconds"] > 0 and run["log_mean_w"] == _capi.ais_finish([run["partial"]])["log_mean_w"]


# ---- 4. a ladder of ones ------------------------------------------------------------------------------------------------------------------
def test_ladder_of_ones(hip):
    M, D, n = 300, 20, 9
    pr = problem(M, D)
    th = draws(pr, n, 4)[0]
    with hip.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        ctx.phmc_set_mass(pr["G"])
        r = ctx.ais_run([1.0, 1.0, 1.0], [2, 1, 3], None, None, L=6, eps=0.5, beta0=1.0, seed=11, chain_offset=1, theta0=th)
        pos = th
        for k, K in enumerate((2, 1, 3)):
            pos = ctx.phmc_sample_to(K, 0, L=6, eps=0.5, seed=12 + k, chain_offset=1, theta0=pos, samples=True)["samples"][:, -1].copy()
    assert same_bits(r["logw"], np.zeros(n)) and same_bits(r["theta"], pos)
    assert r["log_mean_w"] == 0.0 and r["se"] == 0.0 and r["weight_ess"] == n


# ---- 5. the weight reduction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000, 70001])
def test_weight_reduction(hip, n):
    import torch
    rs = np.random.RandomState(n)
    cases = {"narrow": rs.randn(n) * 0.5 + 7.0, "wide": 1e4 * (2.0 * rs.rand(n) - 1.0), "all_neg_inf": np.full(n, -np.inf),
             "all_nan": np.full(n, np.nan)}
    mixed = rs.randn(n) * 3.0 - 40.0
    mixed[rs.rand(n) < 0.1] = -np.inf
    mixed[rs.rand(n) < 0.1] = np.nan
    mixed[n - 1] = np.nan if n % 2 else -np.inf           # the last entry is one of the special ones
    cases["mixed"] = mixed
    if n == 257:
        cases.update({k: v for k, v in weight_cases().items() if len(v) == 257})
    with hip.context(10, 2, 1) as ctx:
        dev = torch.device("cuda", ctx.device)
        for name, lw in cases.items():
            x = torch.from_numpy(lw).to(dev)
            part = ctx.ais_partial(x).cpu().numpy()
            assert same_bits(part, ctx.ais_partial(x).cpu().numpy()), name
            want = A.finish([A.partial(lw)])
            check_finish(_capi.ais_finish([part]), want, "%s n %d" % (name, n))
            if n >= 3:                                    # a 3-way split merged agrees with one piece to the same bound
                cuts = [0, n // 3, n // 3 + max(1, n // 5), n]
                pieces = [ctx.ais_partial(x[a:b].contiguous()).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])]
                check_finish(_capi.ais_finish(pieces), want, "%s n %d split" % (name, n))
        with pytest.raises(ValueError):
            ctx.ais_partial(torch.zeros(0, dtype=torch.float64, device=dev))


# ---- 6. the estimator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_log_evidence_meets_the_quadrature(hip, name):
    """the same inequality and conditions as tests/test_ais_cpu.py::test_restated_ais_meets_the_quadrature, on the GPU"""
    M, D, T = PROBLEMS[name]
    XX, t = synthetic_logreg(M, D, 0)
    r = log_evidence(XX, t, n_chains=N_CHAINS, n_temps=T, ladder="power4", mass="mode", mass_every=1, seed=0)
    ref = quadrature(name)
    print("%s: log Z %.5f, quadrature %.5f, (log Z - quadrature) / se %+.2f, se %.4f, weight-ESS %.0f, Laplace %.5f, acceptance %.3f .. %.3f, "
          "%.3f s" % (name, r["log_evidence"], ref, (r["log_evidence"] - ref) / r["se"], r["se"], r["weight_ess"], r["log_laplace"],
                      r["accept_trace"].min(), r["accept_trace"].max(), r["seconds"]))
    assert r["n_nan"] == 0
    assert r["se"] <= 0.03 and r["weight_ess"] >= N_CHAINS / 4
    assert abs(r["log_evidence"] - ref) <= 5 * r["se"]
    assert abs(r["log_laplace"] - ref) < 0.2 and r["accept_trace"].shape == (T,)


def test_log_evidence_on_pima_is_near_laplace(hip):
    """a sanity band, not a parity claim: the posterior of pima is close to Gaussian"""
    d = np.load(os.path.join(GOLDEN, "data_pima.npz"))
    r = log_evidence(d["XX"], d["t"], n_chains=2048, n_temps=400, seed=1)
    print("pima: log Z %.4f +- %.4f, Laplace %.4f, weight-ESS %.0f of 2048, %.3f s" % (r["log_evidence"], r["se"], r["log_laplace"],
                                                                                     r["weight_ess"], r["seconds"]))
    assert r["n_nan"] == 0 and np.isfinite(r["log_evidence"]) and abs(r["log_evidence"] - r["log_laplace"]) < 1.0


# ---- 7. a failing chain ----------------------------------------------------------------------------------------------------------------------
def test_failing_chain_has_nan_weight_and_is_alone(hip):
    M, D, n = 400, 12, 3
    XX, t = synthetic_logreg(M, D, 0)
    XX = XX * 50.0
    H = R.metric(XX, np.zeros(D)) - np.eye(D) / ALPHA
    w0 = np.zeros((n, D)); w0[1] = 300.0                  # the log-likelihood overflows at this start
    beta = [0.3, 0.6, 1.0]
    out = []
    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(None)
        for th in (w0, np.zeros((n, D))):
            out.append(ctx.ais_run(beta, [2, 2, 2], [1, 1, 1], H, L=4, eps=0.5, beta0=0.1, seed=3, theta0=th))
    bad, good = out
    assert np.isnan(bad["logw"][1]) and bad["n_nan"] == 1 and bad["m"] == 2 and same_bits(bad["theta"][1], w0[1])
    assert good["n_nan"] == 0 and np.isfinite(good["logw"]).all()
    for k in ("logw", "theta"):
        assert same_bits(bad[k][[0, 2]], good[k][[0, 2]]), k
    assert np.isfinite(bad["log_mean_w"])


# ---- 8. refusals, and no trace on the context -------------------------------------------------------------------------------------------------
def test_refusals(hip):
    M, D, n = 60, 3, 2
    pr = problem(M, D)
    H = H_lik(pr)
    w, z, u_len, u_acc = draws(pr, n, 1)
    ok = dict(beta=[0.5, 1.0], stage_len=[1, 1], stage_mass=[1, 1], H_lik=H)
    with hip.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        for call in (lambda: ctx.tphmc_sample_to(6, 2, samples=True), lambda: ctx.tphmc_transition(w, z, u_len, u_acc),
                     lambda: ctx.ais_run(**ok)):
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -1 and "rmhmc_phmc_set_mass" in str(e.value)
        ctx.phmc_set_mass(pr["G"])
        before = mass_probe(ctx, pr)
        bad = [dict(ok, beta=[0.5, -1.0]), dict(ok, beta=[np.nan, 1.0]), dict(ok, beta=[0.5, np.inf]), dict(ok, stage_len=[1, 0]),
               dict(ok, stage_mass=[1, 2]), dict(ok, stage_mass=[-1, 1]), dict(ok, H_lik=None), dict(ok, L=0), dict(ok, beta0=0.3),
               dict(ok, beta0=-0.5, theta0=w), dict(ok, beta0=np.nan, theta0=w)]
        for kw in bad:
            with pytest.raises(_capi.RmhmcError) as e:
                ctx.ais_run(**kw)
            assert e.value.code == -1, kw
        for kw in (dict(beta=[], stage_len=[]), dict(beta=[1.0], stage_len=[1, 1]), dict(beta=[1.0], stage_len=[1], stage_mass=[1, 1])):
            with pytest.raises(ValueError):
                ctx.ais_run(**kw)
        for beta in (-0.1, np.nan, np.inf):
            with pytest.raises(_capi.RmhmcError) as e:
                ctx.tphmc_transition(w, z, u_len, u_acc, beta=beta)
            assert e.value.code == -1
            with pytest.raises(_capi.RmhmcError) as e:
                ctx.tphmc_sample_to(6, 2, beta=beta, samples=True)
            assert e.value.code == -1
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.tphmc_sample_to(5, 4, L=0, samples=True)
        assert e.value.code == -1
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.tphmc_sample_to(5, 4, stats=True)                              # S = 1: unsupported where the PHMC sampler says so
        assert e.value.code == -4
        after = mass_probe(ctx, pr)                                            # no refusal has touched the mass
        for k in before:
            assert same_bits(before[k], after[k]), k
        # a stage whose mass is refused keeps the previous one and the run goes on
        r = ctx.ais_run([0.5, 1.0], [1, 1], [1, 1], -H - np.eye(D), seed=2)
        assert np.isfinite(r["logw"]).all()
        kept = mass_probe(ctx, pr)
        for k in before:
            assert same_bits(before[k], kept[k]), k


def test_no_trace_on_the_context(hip):
    M, D, n = 300, 20, 6
    pr = problem(M, D)
    XX, t, H = pr["XX"], pr["t"], H_lik(pr)

    def others(ctx):
        ctx.phmc_set_mass(pr["G"])
        p = ctx.phmc_sample_to(12, 4, seed=4, samples=True)
        return (ctx.hmc_sample(12, 4, L=5, eps=0.05, seed=1)[:3], ctx.sample(8, 3, seed=2)[:3],
                (p["samples"], p["accepted"], p["leapfrog_steps"]))

    def ais(ctx):
        r = ctx.ais_run(*_capi.ais_schedule(6, "power4", 2), H, seed=9)
        return r["logw"], r["theta"], r["accept_trace"], r["partial"]

    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        opts = ctx.options()
        first = others(ctx)
        ais(ctx)
        assert ctx.options() == opts
        second = others(ctx)
        mine = ais(ctx)
        assert ctx.options() == opts
        last = mass_probe(ctx, pr)
        ctx.phmc_set_mass(pr["G"])                       # the mass after the run is the last installed: beta = 1, the metric at the mode
        want = mass_probe(ctx, pr)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert same_bits(x, y)
    for k in last:
        assert rel_err(last[k].astype(np.float64), want[k].astype(np.float64)) < 1e-9, k
    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(pr["G"])
        fresh = ais(ctx)
    for x, y in zip(mine, fresh):
        assert same_bits(x, y)
