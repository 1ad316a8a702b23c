"""Failing, guarded and diverging chains on every stepping path.

include/rmhmc.h promises that a chain which fails (NaN or inf position, overflow along a trajectory, Cholesky pivot <= 0) is rejected
and flagged and never disturbs the other chains of its batch.  The promise is implemented once per stepping path: the fused kernel,
the one-launch medium step, the generic kernels (16 chains share a wavefront and its MFMA tiles), the int8 assembly (128-chain tiles,
delta assemblies whose slice count is a batch-wide maximum) and the blocked large-D kernels.  The batches of
tests/helpers/failing_chains.py (six kinds of plant on the edges of the wavefront groups and tiles) run here on all of them, with and
without RMHMC_COMPAT:

  a. outcome parity   the planted batch against the CPU oracle, chain by chain: status bits, rejection, unchanged state, and the
                      finite chains to the tolerance of the transition tests,
  b. isolation        every unplanted chain bit-identical to the same batch with benign draws in the planted rows (rmhmc_transition
                      and rmhmc_leapfrog),
  c. samplers         step sizes at which trajectories keep failing and the chains carry on (checked on the oracle by
                      tests/test_failing_chains_cpu.py): against the oracle, bit-identical under every scheduling option and to the
                      stepping API, and with two chains that fail forever,
  d. HMC and mMALA    a NaN momentum / a NaN position on the paths the existing checks do not reach.

Needs an MI355X: run with  pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import context_history as H  # noqa: E402
import failing_chains as F  # noqa: E402
from plan_probe import plan  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(p, m) for p in F.N_CHAINS for m in F.MODES]
ISOLATED = ("w", "w_prop", "p_prop", "H_prop", "H_cur", "hld_prop", "accepted", "status", "nsteps")
_gpu = {}


def _assert_path(ctx, path, spec):
    """device_info names the path (context_history.assert_path) and the planning rule agrees (the probe)"""
    M, D, n, flags, seed = spec
    H.assert_path(ctx, path, paths={path: (M, D, n, flags, seed)})
    F.assert_shape_on_path(path, spec)


def gpu_transitions(hip, path, mode):
    """planted batch and twin on a fresh context each, once per module: (planted, twin, delta counts of the two runs)"""
    key = (path, mode)
    if key not in _gpu:
        spec, planted, twin, _ = F.make_case(path, mode)
        out, counts = [], []
        for inp in (planted, twin):
            with F.context(hip, spec) as ctx:
                _assert_path(ctx, path, spec)
                r = F.transition(ctx, inp)
                counts.append(ctx.i8_delta_counts() if spec[3] & _capi.FLAG_INT8_METRIC else None)
            for v in r.values():
                v.setflags(write=False)
            out.append(r)
        _gpu[key] = (out[0], out[1], counts)
    return _gpu[key]


def _scaled(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("path,mode", CASES)
def test_planted_batch_matches_oracle_chain_by_chain(hip, oracle, path, mode):
    """a.  Chains that fail on the oracle: rejected, state untouched, at least one failure bit (which of the two an overflow raises
    first depends on the order of the arithmetic; poisoned inputs must raise exactly the oracle's).  The guard bits of every chain are
    the oracle's.  Chains without a failure bit on the oracle - every unplanted one and the plants the guards rescue - have the
    oracle's status and decision and its proposal to the tolerances of the transition tests (1e-8; H 1e-7; 1e-6 at 5 slices)."""
    spec, planted, _, plants = F.make_case(path, mode)
    n = spec[2]
    kind_of = dict(plants)
    o = F.oracle_transition(oracle, path, mode)
    g = gpu_transitions(hip, path, mode)[0]
    assert np.array_equal(g["nsteps"], o["nsteps"])
    S = (spec[3] >> 12) & 7 if spec[3] & _capi.FLAG_INT8_METRIC else 0
    tol, tol_H = (1e-6, 1e-6) if S == 5 else (1e-8, 1e-7)
    bad, other_bit, worst = [], [], {}
    gst = g["status"] & 15
    for c in range(n):
        tag = "chain %d (%s)" % (c, kind_of.get(c, "unplanted"))
        if (gst[c] & F.GUARDS) != (o["status"][c] & F.GUARDS):
            bad.append("%s: guard bits %d, oracle %d" % (tag, gst[c] & F.GUARDS, o["status"][c] & F.GUARDS))
        if o["status"][c] & F.FAIL:
            if g["accepted"][c] != 0 or not F.same_bits(g["w"][c], planted["w"][c]):
                bad.append("%s: failed on the oracle, not rejected with its state kept" % tag)
            if not gst[c] & F.FAIL:
                bad.append("%s: status %d carries no failure bit (oracle %d)" % (tag, gst[c], o["status"][c]))
            elif kind_of.get(c) in F.POISONED and gst[c] != o["status"][c]:
                bad.append("%s: status %d, oracle %d" % (tag, gst[c], o["status"][c]))
            elif gst[c] != o["status"][c]:
                other_bit.append("%s: %d, oracle %d" % (tag, gst[c], o["status"][c]))
            continue
        if gst[c] != o["status"][c] or g["accepted"][c] != o["accepted"][c]:
            bad.append("%s: status %d accepted %d, oracle %d %d" % (tag, gst[c], g["accepted"][c], o["status"][c], o["accepted"][c]))
            continue
        for k in ("w_prop", "p_prop", "hld_prop", "H_prop", "w"):
            if not np.array_equal(np.isfinite(g[k][c]), np.isfinite(o[k][c])):
                bad.append("%s: %s finite where the oracle's is not, or the reverse" % (tag, k))
        if not (np.isfinite(o["w_prop"][c]).all() and np.isfinite(o["p_prop"][c]).all() and np.isfinite(o["hld_prop"][c])):
            continue
        errs = {"w_prop": (rel_err(g["w_prop"][c], o["w_prop"][c]), tol), "p_prop": (rel_err(g["p_prop"][c], o["p_prop"][c]), tol),
                "hld_prop": (_scaled(g["hld_prop"][c], o["hld_prop"][c]), tol), "w": (rel_err(g["w"][c], o["w"][c]), tol)}
        if np.isfinite(o["H_prop"][c]):
            errs["H_prop"] = (_scaled(g["H_prop"][c], o["H_prop"][c]), tol_H)
        for k, (e, t) in errs.items():
            if not e < t:
                bad.append("%s: %s %.2e >= %.0e" % (tag, k, e, t))
            if e / t > worst.get(k, (0.0, 0, ""))[0]:
                worst[k] = (e / t, e, tag)
    print("%s %s: closest to its bound: %s" % (path, mode, ", ".join("%s %.1e %s" % (k, v[1], v[2]) for k, v in sorted(worst.items()))))
    print("%s %s: failed chains whose failure bits differ from the oracle's: %s" % (path, mode, "; ".join(other_bit) or "none"))
    assert not bad, "%s %s: %s" % (path, mode, "; ".join(bad))


@pytest.mark.parametrize("path,mode", CASES)
def test_planted_chains_do_not_change_a_bit_of_their_neighbours(hip, path, mode):
    """b.  With the delta assemblies on (the default): they are exact integer arithmetic at any slice count that holds the difference,
    so the batch-wide maximum a diverging chain raises must not show in a neighbour."""
    spec, _, _, plants = F.make_case(path, mode)
    planted, twin, counts = gpu_transitions(hip, path, mode)
    keep = np.setdiff1d(np.arange(spec[2]), [c for c, _ in plants])
    if counts[0] is not None:
        print("%s %s: delta assemblies by slice count, planted %s, twin %s" % (path, mode, counts[0], counts[1]))
        if (path, mode) == ("int8", "compat"):   # (the case is not vacuous: here the plants do push the batch to another slice count)
            assert counts[0] != counts[1] and sum(counts[1]["end"]) > 0, counts
    H.assert_same_bits({k: planted[k][keep] for k in ISOLATED}, {k: twin[k][keep] for k in ISOLATED}, "%s %s, unplanted chains" % (path, mode))
    assert np.isfinite(twin["w"]).all() and np.isfinite(planted["w"][keep]).all()


@pytest.mark.parametrize("path,mode", CASES)
def test_leapfrog_planted_chains_do_not_change_a_bit_of_their_neighbours(hip, path, mode):
    """b, rmhmc_leapfrog: two steps with the NaN, inf and far-out positions planted"""
    spec, planted, twin, plants = F.make_case(path, mode, kinds=F.FAR_OUT)
    n = spec[2]
    rs = np.random.RandomState(7)
    dirs = np.where(rs.rand(n) < 0.5, 1, -1).astype(np.int32)
    out = []
    for inp in (planted, twin):
        with F.context(hip, spec) as ctx:
            _assert_path(ctx, path, spec)
            with np.errstate(all="ignore"):
                w, p, hld, st = ctx.leapfrog(inp["w"], inp["z"], F.EPS, dirs, 2, F.K)
            out.append({"w": w, "p": p, "hld": hld, "status": st})
    rows = [c for c, _ in plants]
    keep = np.setdiff1d(np.arange(n), rows)
    assert len(rows) == 3
    for c, kind in plants:                    # (under RMHMC_FLAG_GUARDS the position guard may pull the far-out chain back)
        st = out[0]["status"][c]
        assert st & F.FAIL if kind in F.POISONED else st != 0, (c, kind, st)
    H.assert_same_bits({k: v[keep] for k, v in out[0].items()}, {k: v[keep] for k, v in out[1].items()}, "%s %s leapfrog" % (path, mode))
    assert np.isfinite(out[1]["w"]).all() and (out[1]["status"] & F.FAIL == 0).mean() >= 0.9


def _sample(hip, path, spec, eps, theta0, **options):
    with F.context(hip, spec) as ctx:
        _assert_path(ctx, path, spec)
        for k, v in options.items():
            assert ctx.get_option(k) != v, k
            ctx.set_option(k, v)
        return F.sample(ctx, eps, theta0)


@pytest.mark.parametrize("path", list(F.SAMPLER_CASES))
def test_sampler_that_fails_and_carries_on(hip, oracle, path):
    """c.  Rejected proposals that leave NaN behind meet the c-tile cache and its restore kernel, the work-sorted layout, graph replay
    and the per-iteration state machine: the run agrees with the oracle, does not depend on any of those options, and visits the states
    of the stepping API."""
    spec, eps = F.sampler_spec(path)
    n, T = spec[2], F.SAMPLER_T
    th = F.sampler_theta0(spec)
    with F.context(oracle, spec) as ctx:
        o = F.sample(ctx, eps, th)
    g = _sample(hip, path, spec, eps, th)
    assert np.array_equal(g["accepted"], o["accepted"]) and np.array_equal(g["leapfrog_steps"], o["leapfrog_steps"])
    assert 0 < o["accepted"].sum() < n * T and np.isfinite(g["samples"]).all()
    worst = max(rel_err(g["samples"][c], o["samples"][c]) for c in range(n))
    print("%s: samples against the oracle, worst chain %.1e" % (path, worst))
    assert worst < 1e-7
    for key in ("graph", "sorted", "cdyn", "crestore"):
        H.assert_same_bits(_sample(hip, path, spec, eps, th, **{key: 0}), g, "%s with %s = 0" % (path, key))
    # the stepping API: one global step per call, the state of every chain whenever it completes a transition
    seen = [[] for _ in range(n)]
    last = np.zeros(n, dtype=np.int64)
    with F.context(hip, spec) as ctx:
        with np.errstate(all="ignore"):
            ctx.chains_init(theta0=th, seed=F.SAMPLER_SEED, L=F.SAMPLER_L, eps=eps, K=F.SAMPLER_K)
            for _ in range(T * F.SAMPLER_L):
                ctx.chains_run(1)
                w, it, acc = ctx.chains_state()
                for c in np.where(it > last)[0]:
                    assert it[c] == last[c] + 1
                    seen[c].append(w[c].copy()); last[c] = it[c]
                if last.min() >= T:
                    break
    assert last.min() >= T
    for c in range(n):
        assert np.array_equal(np.array(seen[c][:T]), g["samples"][c]), c


@pytest.mark.parametrize("path", list(F.SAMPLER_CASES))
def test_sampler_with_chains_that_fail_forever(hip, path):
    """c, last item: two chains started at w = 60 (plain flags: every proposal from there overflows) return their start in every sample
    and accept nothing; all other chains are bit-identical to the run without them"""
    _, eps, n = F.SAMPLER_CASES[path]
    spec = F.spec_of(path, "plain", n)
    th = F.sampler_theta0(spec)
    stuck = [1, min(17, n - 1)]
    th_bad = th.copy(); th_bad[stuck] = 60.0
    good = _sample(hip, path, spec, eps, th)
    bad = _sample(hip, path, spec, eps, th_bad)
    for c in stuck:
        assert bad["accepted"][c] == 0 and np.array_equal(bad["samples"][c], np.broadcast_to(th_bad[c], bad["samples"][c].shape)), c
    keep = np.setdiff1d(np.arange(n), stuck)
    H.assert_same_bits({k: v[keep] for k, v in bad.items()}, {k: v[keep] for k, v in good.items()}, path + ", chains next to the stuck ones")
    assert np.array_equal(bad["leapfrog_steps"], good["leapfrog_steps"])
    assert good["accepted"].sum() > 0 and np.isfinite(good["samples"]).all()


@pytest.mark.parametrize("name", list(F.HMC_SHAPES))
def test_hmc_nan_momentum_is_rejected_and_isolated(hip, oracle, name):
    """d.  hmc.py:56-57 on the generic and large-D kernels (k_hmc_pre) and on the one-launch trajectory with the data rows in registers
    and streamed"""
    M, D, n, XX, t, planted, twin, c, eps = F.hmc_case(name)
    p = plan(M, D, n, _capi.COMPAT)
    rows_per_thread = (p["Mp"] + 255) // 256
    assert (p["hmc_traj"], p["big"]) == {"generic": (0, 0), "large": (0, 1)}.get(name, (1, 0)), p
    if p["hmc_traj"]:
        assert (rows_per_thread <= 4) == (name == "traj_rows_in_registers"), p
    with oracle.context(M, D, n) as ctx:
        ctx.set_data(XX, t, 100.0)
        o = F.hmc_transition(ctx, planted, eps)
    assert np.isnan(o["p_prop"][c]).any() and o["accepted"][c] == 0          # (the plant does end in a NaN momentum)
    out = []
    for inp in (planted, twin):
        with hip.context(M, D, n) as ctx:
            ctx.set_data(XX, t, 100.0)
            out.append(F.hmc_transition(ctx, inp, eps))
    g, good = out
    assert g["accepted"][c] == o["accepted"][c] and np.array_equal(g["w"][c], o["w"][c]) and np.array_equal(g["w"][c], planted["w"][c])
    assert np.array_equal(g["nsteps"], o["nsteps"])
    keep = np.arange(n) != c
    H.assert_same_bits({k: v[keep] for k, v in g.items()}, {k: v[keep] for k, v in good.items()}, "HMC %s, neighbours" % name)
    assert np.array_equal(g["accepted"][keep], o["accepted"][keep]) and np.isfinite(g["w"]).all() and o["accepted"][keep].sum() > 0


@pytest.mark.parametrize("name", list(F.MMALA_SHAPES))
def test_mmala_nan_position_is_rejected_and_isolated(hip, name):
    """d.  rmhmc_mmala_transition with one NaN position on the medium, generic and large-D shapes"""
    spec, planted, twin, c = F.mmala_case(name)
    out = []
    for inp in (planted, twin):
        with F.context(hip, spec) as ctx:
            _assert_path(ctx, name, spec)
            out.append(F.mmala_transition(ctx, inp))
    g, good = out
    assert g["accepted"][c] == 0 and F.same_bits(g["w"][c], planted["w"][c])
    keep = np.arange(spec[2]) != c
    H.assert_same_bits({k: v[keep] for k, v in g.items()}, {k: v[keep] for k, v in good.items()}, "mMALA %s, neighbours" % name)
    assert good["accepted"].sum() > 0 and np.isfinite(good["w"]).all()
