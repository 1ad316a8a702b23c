"""GPU tests of the fixed-metric HMC sampler (include/rmhmc_phmc.h, csrc/phmc.hip.h) against plain HMC on its multi-launch path
(identity mass: bit for bit) and against the NumPy restatement tests/helpers/phmc_ref.py (dense mass), which tests/test_phmc_cpu.py
pins to the CPU oracle.

GPU-versus-restatement tolerances are those of plain HMC against its oracle (tests/test_gpu_parity.py): step counts and decisions
equal, w_prop / p_prop / H_prop 1e-9, samples 1e-8.  No decision of the restatement may be within 1e-6 of a tie, so that rounding
cannot flip one.  Measured on an MI355X: 3e-16 ... 1.4e-14 relative, the smallest tie margin 9e-3.
Every chain slot of a workgroup, the tile edges of D, zero-step trajectories and the sampler against the chained restatement:
tests/test_gpu_phmc_edges.py."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, rel_err
from riemannhamiltonianmontecarlo_amd import PHMC, RMHMC, _capi, experiment
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import phmc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def problem(M, D, scale=1.0):
    """data, the restatement's mode and metric there, its factor: computed once per shape and shared"""
    key = (M, D, scale)
    if key not in _cache:
        XX, t = synthetic_logreg(M, D, 1)
        XX = XX * scale
        m = R.mode(XX, t)
        assert m["converged"]
        _cache[key] = dict(XX=XX, t=t, mode=m["w"], G=m["G"], Lg=np.linalg.cholesky(m["G"]), iters=m["iters"])
    return _cache[key]


def draws(pr, n, seed):
    """starts from N(mode, G^-1), momentum normals, the two uniforms"""
    D = pr["XX"].shape[1]
    rs = np.random.RandomState(seed)
    w = np.stack([pr["mode"] + R.solve_upper(pr["Lg"].T, rs.randn(D)) for _ in range(n)])
    z = rs.randn(n, D)
    u_len = rs.uniform(0.05, 1.0, n); u_acc = rs.uniform(0.05, 1.0, n)
    u_len[0] = 1.0   # one trajectory of full length
    return w, z, u_len, u_acc


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- 1. identity mass is plain HMC ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,n", [(690, 15, 4), (300, 64, 17), (250, 150, 3)])
def test_identity_mass_is_plain_hmc(hip, M, D, n):
    XX, t = synthetic_logreg(M, D, 1)
    rs = np.random.RandomState(M + D)
    w = 0.1 * rs.randn(n, D); z = rs.randn(n, D)
    u_len = rs.uniform(0.05, 1.0, n); u_acc = rs.uniform(0.05, 1.0, n)
    u_len[0] = 1.0
    out = []
    for phmc in (False, True):      # a fresh context each; medium = 0: plain HMC on its multi-launch kernels
        with hip.context(M, D, n, options={"medium": 0}) as ctx:
            ctx.set_data(XX, t)
            if phmc:
                ctx.phmc_set_mass(None)
                out.append(ctx.phmc_transition(w, z, u_len, u_acc, L=12, eps=0.02))
            else:
                out.append(ctx.hmc_transition(w, z, u_len, u_acc, L=12, eps=0.02))
    h, p = out
    assert h["nsteps"][0] == 12 and (p["status"] == 0).all()
    for k in ("w", "w_prop", "p_prop", "nsteps", "accepted", "H_cur", "H_prop"):   # the kinetic sums keep k_hmc_begin's order: H too
        assert same_bits(h[k], p[k]), k
    out = []
    for phmc in (False, True):
        with hip.context(M, D, n, options={"medium": 0}) as ctx:
            ctx.set_data(XX, t)
            if phmc:
                ctx.phmc_set_mass(None)
                r = ctx.phmc_sample_to(20, 5, L=10, eps=0.02, seed=8, chain_offset=3, samples=True)
                out.append((r["samples"], r["accepted"], r["leapfrog_steps"]))
            else:
                out.append(ctx.hmc_sample(20, 5, L=10, eps=0.02, seed=8, chain_offset=3)[:3])
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert out[0][1].sum() > 0 and out[0][2].sum() > 0


# ---- 2. dense mass against the restatement ----------------------------------------------------------------------------------------------
# (M, D, n, scale of X).  M = 120 < D = 256: the data are separable and the prior alone bounds the mode.  With unit-variance columns
# the curvature of the log joint away from the mode is far above the metric at the mode, and the trajectory at eps = 0.5 overflows in
# the restatement as on the GPU (H_prop = inf in both, rejected in both): nothing left to compare.  Rows of unit length (X / sqrt(D))
# keep the integrator stable there: H_prop finite, decisions 2 and 6 away from a tie.
DENSE = [(37, 1, 2, 1.0), (60, 3, 5, 1.0), (200, 33, 17, 1.0), (300, 64, 4, 1.0), (250, 65, 3, 1.0), (300, 130, 3, 1.0),
         (120, 256, 2, 1.0 / 16)]


def check_transition(got, ref):
    print("margin min %.2e  w_prop %.1e  p_prop %.1e  H_cur %.1e  H_prop %.1e" % (
        np.abs(ref["margin"]).min(), rel_err(got["w_prop"], ref["w_prop"]), rel_err(got["p_prop"], ref["p_prop"]),
        rel_err(got["H_cur"], ref["H_cur"]), rel_err(got["H_prop"], ref["H_prop"])))
    assert (np.abs(ref["margin"]) > 1e-6).all() and np.isfinite(ref["H_prop"]).all()
    assert np.array_equal(got["nsteps"], ref["nsteps"]) and np.array_equal(got["accepted"], ref["accepted"])
    assert np.array_equal(got["status"], ref["status"])
    for k in ("w_prop", "p_prop", "H_prop", "H_cur", "w"):
        assert rel_err(got[k], ref[k]) < 1e-9, k


@pytest.mark.parametrize("M,D,n,scale", DENSE)
def test_dense_mass_matches_restatement(hip, M, D, n, scale):
    pr = problem(M, D, scale)
    w, z, u_len, u_acc = draws(pr, n, M + D)
    ref = R.transitions(pr["XX"], pr["t"], pr["Lg"], w, z, u_len, u_acc, 8, 0.5)
    assert ref["nsteps"][0] == 8
    with hip.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        ctx.phmc_set_mass(pr["G"])
        got = ctx.phmc_transition(w, z, u_len, u_acc, L=8, eps=0.5)
    check_transition(got, ref)


def test_dense_mass_in_an_int8_metric_context(hip):
    M, D, n = 300, 64, 130
    pr = problem(M, D)
    w, z, u_len, u_acc = draws(pr, n, 5)
    ref = R.transitions(pr["XX"], pr["t"], pr["Lg"], w, z, u_len, u_acc, 8, 0.5)
    out = []
    for flags in (_capi.COMPAT, _capi.COMPAT | _capi.int8_metric_flags(6)):
        with hip.context(M, D, n, flags=flags) as ctx:
            ctx.set_data(pr["XX"], pr["t"])
            ctx.phmc_set_mass(pr["G"])
            out.append(ctx.phmc_transition(w, z, u_len, u_acc, L=8, eps=0.5))
    check_transition(out[0], ref)
    for k in out[0]:     # the sampler uses the gradient pass alone, which an int8 context does not change
        assert rel_err(out[1][k], out[0][k]) < 1e-12, k


# ---- 3. the sampler is its transitions --------------------------------------------------------------------------------------------------
def test_sampler_modes_agree(hip):
    import torch
    M, D, n = 200, 33, 5
    pr = problem(M, D)
    th = draws(pr, n, 9)[0]
    kw = dict(L=8, eps=0.5, seed=21, chain_offset=2, theta0=th)
    runs = []
    for opts in (None, {"graph": 0, "sorted": 0}):
        with hip.context(M, D, n, options=opts) as ctx:
            ctx.set_data(pr["XX"], pr["t"])
            ctx.phmc_set_mass(pr["G"])
            runs.append(ctx.phmc_sample_to(30, 8, samples=True, **kw))
            if opts is None:
                dev = torch.device("cuda", ctx.device)
                d = ctx.phmc_sample_to(30, 8, where="device", device=dev, samples=True, stats=True, **kw)
                ess, mean, var = ctx.ess_dev(d["samples"])
                assert torch.equal(d["ess"], ess) and torch.equal(d["mean"], mean) and torch.equal(d["var"], var)
                s = ctx.phmc_sample_to(30, 8, stats=True, run_mean=True, **kw)
                assert same_bits(s["ess"], ess.cpu().numpy()) and same_bits(s["mean"], mean.cpu().numpy())
    a, b = runs
    for k in ("samples", "accepted", "leapfrog_steps"):
        assert same_bits(a[k], b[k]), k
        assert same_bits(a[k], d[k].cpu().numpy()), k
    assert a["seconds"] > 0 and d["seconds"] > 0 and np.isfinite(a["samples"]).all()
    changed = (np.diff(a["samples"], axis=1) != 0).any(axis=2).sum(axis=1)
    print("accepted", a["accepted"], "changed rows", changed, "steps", a["leapfrog_steps"])
    assert (changed <= a["accepted"]).all() and (a["accepted"] <= 30).all() and changed.sum() > 0
    assert (a["leapfrog_steps"] >= 21).all() and (a["leapfrog_steps"] <= 21 * 8).all()   # the 21 transitions after burn_in + 1


# ---- 4. the posterior mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("pima", 1), ("australian", 3), ("syn_300_130", 30)])
def test_mode_matches_restatement(hip, name, n):
    if name.startswith("syn"):
        pr = problem(300, 130)
        XX, t, ref = pr["XX"], pr["t"], dict(w=pr["mode"], iters=pr["iters"])
    else:
        d = np.load(os.path.join(GOLDEN, "data_%s.npz" % name))
        XX, t = d["XX"], d["t"]
        ref = R.mode(XX, t)
        assert ref["converged"]
    M, D = XX.shape
    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        m = ctx.phmc_mode()
        G, _, grad = ctx.metric(np.tile(m["w"], (n, 1)))
        _, _, grad0 = ctx.metric(np.zeros((n, D)))
    print(name, "iters", m["iters"], "(restatement %d)" % ref["iters"], "step %.2e" % m["step"], "w err %.2e" % rel_err(m["w"], ref["w"]),
          "grad %.2e of %.2e" % (np.abs(grad).max(), np.abs(grad0).max()))
    assert m["converged"] and 1 <= m["iters"] <= 30
    assert rel_err(m["w"], ref["w"]) < 1e-9
    assert np.abs(grad).max() <= 1e-6 * np.abs(grad0).max()
    assert rel_err(m["G"], G[0]) < 1e-12 and np.array_equal(m["G"], m["G"].T)


# ---- 5. the right distribution -----------------------------------------------------------------------------------------------------------
def test_same_posterior_as_rmhmc(hip):
    d = np.load(os.path.join(GOLDEN, "data_pima.npz"))
    XX, t = d["XX"], d["t"]
    kw = dict(NumOfIterations=400, BurnIn=100, n_chains=64, seed=17, verbose=False, summary=True, diagnostics=True, return_info=True)
    sp, _, ip = PHMC(XX, t, mass="mode", **kw)
    sr, _, ir = RMHMC(XX, t, compat=False, **kw)
    stat = []
    for s, info in ((sp, ip), (sr, ir)):
        assert all(np.isfinite(s[k]).all() for k in ("mean", "var", "ess", "run_mean"))
        pooled_mean = s["mean"].mean(axis=0)
        pooled_var = s["var"].mean(axis=0) + s["mean"].var(axis=0)     # within + between, every chain of the same length
        stat.append((pooled_mean, pooled_var, info["diagnostics"]["ess_pooled"]))
    (m1, v1, e1), (m2, v2, e2) = stat
    bound = 5.0 * np.sqrt(v1 / e1 + v2 / e2)       # five sigma of the Monte-Carlo error of the difference
    print("PHMC acceptance %.3f (RMHMC %.3f), newton iterations %d" % (ip["accepted"].sum() / (64 * 400.0), ir["accepted"].sum() / (64 * 400.0),
                                                                       ip["newton_iters"]))
    print("mean difference / bound:", np.abs(m1 - m2) / bound, "pooled ESS", e1, e2, "max rhat", ip["diagnostics"]["rhat"].max())
    assert (np.abs(m1 - m2) <= bound).all()
    assert ip["mode"].shape == (XX.shape[1],) and ip["mass"].shape == (XX.shape[1],) * 2


def test_shim_mass_and_start_choices(hip, capsys):
    from riemannhamiltonianmontecarlo_amd import HMC
    XX, t = synthetic_logreg(150, 10, 4)
    kw = dict(NumOfIterations=30, BurnIn=10, NumOfLeapFrogSteps=7, StepSize=0.03, n_chains=3, seed=12, verbose=False,
              options={"medium": 0})
    ws, _ = PHMC(XX, t, mass="identity", **kw)                     # plain HMC through the shim, bit for bit
    wh, _ = HMC(XX, t, **kw)
    assert ws.shape == (3, 20, 10) and same_bits(ws, wh)
    m = R.mode(XX, t)
    w1, secs, info = PHMC(XX, t, 30, 10, mass=m["G"], theta0="mode", n_chains=1, seed=12, return_info=True)   # verbose: HMC's lines
    assert w1.shape == (20, 10) and secs > 0 and np.isfinite(w1).all() and "Time drawing posterior" in capsys.readouterr().out
    assert rel_err(info["mode"], m["w"]) < 1e-9 and info["newton_iters"] == m["iters"] and same_bits(info["mass"], m["G"])
    w2, _, info2 = PHMC(XX, t, 30, 10, mass="mode", theta0=m["w"], n_chains=1, seed=12, verbose=False, return_info=True)
    assert rel_err(w2, w1) < 1e-8 and rel_err(info2["mass"], m["G"]) < 1e-12     # the GPU's mode and metric are the restatement's
    _, _, info3 = PHMC(XX, t, 30, 10, mass="identity", n_chains=1, seed=12, verbose=False, return_info=True)
    assert info3["mode"] is None and info3["mass"] is None and info3["newton_iters"] == 0


def test_experiment_takes_the_shim(hip):
    XX, t = synthetic_logreg(120, 4, 2)
    res = experiment.run_experiment(XX, t, PHMC, n_experiments=3, batched=True, seed=5, NumOfIterations=40, BurnIn=10)
    assert res["results_beta"].shape == (3, 30, 4) and res["sampler"] == "PHMC" and np.isfinite(res["results_beta"]).all()


# ---- 6. failing chains and refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [300.0, np.nan])
def test_failing_chain_is_rejected_and_alone(hip, bad):
    M, D, n = 400, 12, 3
    XX, t = synthetic_logreg(M, D, 0)
    XX = XX * 50.0
    mass = R.metric(XX, np.zeros(D))
    w0 = np.zeros((n, D)); w0[1] = bad
    z = np.ones((n, D)); u = np.full(n, 0.5)
    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(mass)
        r = ctx.phmc_transition(w0, z, u, u, L=10, eps=0.5)
        g = ctx.phmc_transition(np.zeros((n, D)), z, u, u, L=10, eps=0.5)
        s = ctx.phmc_sample_to(6, 2, L=4, eps=0.5, seed=3, theta0=w0, samples=True)
        sg = ctx.phmc_sample_to(6, 2, L=4, eps=0.5, seed=3, theta0=np.zeros((n, D)), samples=True)
    assert same_bits(r["w"][1], w0[1]) and r["accepted"][1] == 0 and r["status"][1] & 3
    assert (g["status"] == 0).all()
    for k in r:
        assert same_bits(r[k][[0, 2]], g[k][[0, 2]]), k
    assert same_bits(s["samples"][1], np.tile(w0[1], (4, 1))) and s["accepted"][1] == 0
    for k in ("samples", "accepted", "leapfrog_steps"):
        assert same_bits(s[k][[0, 2]], sg[k][[0, 2]]), k


def test_refusals(hip):
    M, D, n = 60, 3, 2
    pr = problem(M, D)
    w, z, u_len, u_acc = draws(pr, n, 1)
    with hip.context(M, D, n) as ctx:
        ctx.set_data(pr["XX"], pr["t"])
        for call in (lambda: ctx.phmc_sample_to(6, 2, samples=True), lambda: ctx.phmc_transition(w, z, u_len, u_acc)):
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -1 and "rmhmc_phmc_set_mass" in str(e.value)
        ctx.phmc_set_mass(pr["G"])
        before = ctx.phmc_transition(w, z, u_len, u_acc, L=8, eps=0.5)
        nan = pr["G"].copy(); nan[1, 0] = np.nan
        for m in (nan, -pr["G"], np.array([[1.0, 1, 0], [1, 1, 0], [0, 0, 1]])):
            with pytest.raises(_capi.RmhmcError) as e:
                ctx.phmc_set_mass(m)
            assert e.value.code == -1
        after = ctx.phmc_transition(w, z, u_len, u_acc, L=8, eps=0.5)       # the previous mass is still in place
        for k in before:
            assert same_bits(before[k], after[k]), k
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.phmc_sample_to(5, 4, stats=True)                             # S = 1
        assert e.value.code == -4
        with pytest.raises(_capi.RmhmcError) as e:
            ctx.phmc_sample_to(5, 4, L=0, samples=True)
        assert e.value.code == -1


# ---- 7. no trace on the context -----------------------------------------------------------------------------------------------------------
def test_no_trace_on_the_context(hip):
    M, D, n = 300, 20, 6
    XX, t = synthetic_logreg(M, D, 1)

    def others(ctx):
        return (ctx.hmc_sample(12, 4, L=5, eps=0.05, seed=1)[:3], ctx.sample(8, 3, seed=2)[:3], ctx.mmala_sample(8, 3, seed=3)[:2])

    def phmc(ctx):
        m = ctx.phmc_mode()
        assert m["converged"]
        ctx.phmc_set_mass(m["G"])
        r = ctx.phmc_sample_to(12, 4, seed=4, samples=True)
        return r["samples"], r["accepted"], r["leapfrog_steps"]

    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        opts = ctx.options()
        first = others(ctx)
        phmc(ctx)
        assert ctx.options() == opts
        second = others(ctx)
        mine = phmc(ctx)
        assert ctx.options() == opts
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert same_bits(x, y)
    with hip.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        fresh = phmc(ctx)
    for x, y in zip(mine, fresh):
        assert same_bits(x, y)
