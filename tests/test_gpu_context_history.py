"""A context's results must not depend on its earlier calls.

An rmhmc_ctx is long-lived: about forty device buffers (c-tile cache and stale list, int8 slice planes with their per-chain exponents,
partial planes shared by the fp64 row split and the int8 k split, the work-sorted sampler's permutation ...) and a few host-side
fields (lists them).  Every entry point is supposed to overwrite or reset what it reads; INTEGRATION.md promises that one context serves RMHMC, HMC,
mMALA, AMH, IWLS and Gibbs calls in any order.  Here one battery of calls with fixed inputs (tests/helpers/context_history.py) runs on
every stepping path

  1. on two fresh contexts                      -> bit-identical (run-to-run determinism),
  2. after each "polluter" on the same context  -> bit-identical to the fresh battery (history independence),
  3. in reversed order on a fresh context       -> bit-identical, call by call (order independence),
  4. on the CPU oracle with the same data       -> within the tolerances the project's parity tests already use for each call (anchor:
     "equal to fresh" cannot mean "equally wrong").

AMH, IWLS and Gibbs have no oracle entry points: they are covered by 1-3 only (their parity is pinned in test_gpu_amh.py,
test_gpu_iwls.py and test_gpu_gibbs.py).  The certificate cases use the int8 paths' D, n and flags with 6000 rows: below about 3200
rows no data set can fail the 1e-9 certificate (helpers/context_history.py, CERT_PATHS), so they carry a fresh battery of their own,
whose path is confirmed from device_info and whose metric is anchored on the oracle in both modes.  Needs an MI355X: run with  pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi
from test_gpu_int8_metric import G_TOL, STEP_TOL
from test_gpu_int8_stress import _nan_rel
from test_gpu_parity import TOL_STEP, TOL_TRAJ

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import context_history as H  # noqa: E402

pytestmark = pytest.mark.gpu

_fresh = {}
_delta = {}


def _context(lib, spec, variant="own", flags=None):
    M, D, n, fl, _ = spec
    ctx = lib.context(M, D, n, flags=fl if flags is None else flags)
    ctx.set_data(*H.data_of(spec, variant), 100.0)
    return ctx


def _freeze(out):
    for v in out.values():
        v.setflags(write=False)
    return out


def fresh(hip, path):
    """the battery on a fresh context of the path, once per module; asserts that the intended kernels are the ones in use"""
    if path not in _fresh:
        spec = H.PATHS[path]

        def after(name, ctx):
            if name == "sample" and spec[3] & _capi.FLAG_INT8_METRIC:
                _delta[path] = ctx.i8_delta_counts()

        with _context(hip, spec) as ctx:
            H.assert_path(ctx, path)
            _fresh[path] = _freeze(H.battery(ctx, H.make_inputs(spec), after=after))
            H.assert_path(ctx, path)
    return _fresh[path]


@pytest.mark.parametrize("path", list(H.PATHS))
def test_intended_path_is_active_and_battery_is_deterministic(hip, path):
    """assertion 1, and the path checks: device_info names the stepping path, the int8 certificate is active, the 6-slice int8 paths
    have really assembled deltas by the end of the battery's `sample`"""
    spec = H.PATHS[path]
    want = fresh(hip, path)
    assert len(want) > 40
    if path in ("int8", "large_int8"):
        d = _delta[path]
        assert sum(d["end"]) > 0 and sum(d["inner"]) > 0, d
    with _context(hip, spec) as ctx:
        H.assert_same_bits(H.battery(ctx, H.make_inputs(spec)), want, path + ", second fresh context")


@pytest.mark.parametrize("polluter", list(H.POLLUTERS))
@pytest.mark.parametrize("path", list(H.PATHS))
def test_battery_does_not_depend_on_history(hip, path, polluter):
    """assertion 2"""
    spec = H.PATHS[path]
    want = fresh(hip, path)
    inp = H.make_inputs(spec)
    with _context(hip, spec) as ctx:
        H.POLLUTERS[polluter](ctx, spec, inp)
        H.assert_path(ctx, path)
        H.assert_same_bits(H.battery(ctx, inp), want, "%s after %s" % (path, polluter))


@pytest.mark.parametrize("path", list(H.PATHS))
def test_battery_does_not_depend_on_call_order(hip, path):
    """assertion 3"""
    spec = H.PATHS[path]
    want = fresh(hip, path)
    with _context(hip, spec) as ctx:
        H.assert_same_bits(H.battery(ctx, H.make_inputs(spec), order="reversed"), want, path + ", reversed order")


@pytest.mark.parametrize("path", list(H.PATHS))
def test_options_toggled_between_chains_run_calls_do_not_change_the_chains(hip, path):
    """rmhmc_set_option between two rmhmc_chains_run calls of one run (the case its reset of the stale flags and of the list of rejecting
    chains is there for): the scheduling options graph / inflight / cdyn / crestore give the same bits whatever they are, so a run that
    changes them every few steps must visit the states of an untouched run.  This pins that changing the options mid-run does not
    change the bits; it does not pin the reset itself (the flags are exact without it, see the comment at the fill in rmhmc_set_option).  Step size 0.9 (0.5 at D > 64, where 0.9 accepts nothing): proposals are rejected
    and accepted all along."""
    spec = H.PATHS[path]
    eps = 0.5 if spec[1] > 64 else 0.9

    def run(toggles):
        with _context(hip, spec) as ctx:
            with np.errstate(all="ignore"):
                ctx.chains_init(seed=12, chain_offset=2, L=4, eps=eps, K=4)
                for key, val in toggles:
                    ctx.chains_run(9)
                    if key:
                        ctx.set_option(key, val)
                ctx.chains_run(10)
                return ctx.chains_state()

    toggles = [("crestore", 0), ("cdyn", 0), ("crestore", 1), ("graph", 0), ("cdyn", 1), ("inflight", 1), ("graph", 1)]
    plain = run([(None, 0)] * len(toggles))
    iters, acc = plain[1], plain[2]
    assert (acc < iters).any() and acc.sum() > 0            # proposals rejected and accepted
    for a, b in zip(run(toggles), plain):
        assert np.array_equal(a, b, equal_nan=True)


def _fresh_certificate_case(hip, oracle, path, variant):
    """the battery on a fresh context of a certificate shape given one data set alone, once per module.  The path is confirmed from
    device_info (int8 active on the clean data, "NOT certified" and the fp64 matrix cores on the outlier data), and the metric is
    anchored on the oracle: int8 mode with the bounds of test_gpu_int8_metric.py, fp64 mode of the int8-requested context with the
    1e-11 of test_outlier_row_is_sent_to_fp64_by_the_certificate (the whole battery on the oracle would take a minute at these shapes)."""
    key = (path, variant)
    if key not in _fresh:
        spec = H.CERT_PATHS[path]
        M, D, n, flags, _ = spec
        inp = H.make_inputs(spec)
        active = variant == "own"
        with _context(hip, spec, variant) as ctx:
            H.assert_path(ctx, path, certify_active=active, paths=H.CERT_PATHS)
            g = _freeze(H.battery(ctx, inp))
            H.assert_path(ctx, path, certify_active=active, paths=H.CERT_PATHS)
        with _context(oracle, spec, variant, flags=0) as ctx:
            Go, ho, go = ctx.metric(inp["w"])
        assert np.array_equal(g["metric.G"], np.swapaxes(g["metric.G"], 1, 2))
        if active:
            S = (flags >> 12) & 7
            assert _rel_rows(g["metric.G"], Go) < G_TOL[S]
            assert np.abs(g["metric.hld"] - ho).max() < 1e3 * G_TOL[S] and rel_err(g["metric.grad"], go) < 1e-12
        else:
            # (the outlier row overflows e^f for some chains: the reference's gradient is NaN there and so must the kernel's be, as in
            #  test_log_joint_terms_saturate_like_the_reference; _nan_rel is the comparison of the outlier test itself)
            assert _nan_rel(g["metric.G"], Go) < 1e-11 and _nan_rel(g["metric.hld"], ho) < 1e-11 and _nan_rel(g["metric.grad"], go) < 1e-11
        _fresh[key] = g
    return _fresh[key]


@pytest.mark.parametrize("first,then", [("outlier", "own"), ("own", "outlier")])
@pytest.mark.parametrize("path", list(H.CERT_PATHS))
def test_certificate_flip_leaves_no_trace(hip, oracle, path, first, then):
    """int8 -> fp64 -> int8 on one context and its mirror image: a data set the certificate sends to the fp64 kernels (one row 1000 x
    the others, test_outlier_row_is_sent_to_fp64_by_the_certificate), a transition on it, then the other data set and the battery;
    against a fresh context given that data set alone."""
    spec = H.CERT_PATHS[path]
    inp = H.make_inputs(spec)
    want = _fresh_certificate_case(hip, oracle, path, then)
    with _context(hip, spec, first) as ctx:
        bound, active = ctx.int8_certificate()
        assert active == (first == "own") and (bound > _capi.INT8_CERTIFY_TOL) == (first == "outlier")
        H.assert_path(ctx, path, certify_active=first == "own", paths=H.CERT_PATHS)
        with np.errstate(all="ignore"):
            ctx.transition(inp["wt"], inp["z"], inp["ul"], inp["gd"], inp["ua"], L=3, eps=0.4, K=4)
            ctx.chains_init(seed=3, L=3, eps=0.4, K=4)
            ctx.chains_run(5)
        ctx.set_data(*H.data_of(spec, then), 100.0)
        H.assert_path(ctx, path, certify_active=then == "own", paths=H.CERT_PATHS)
        H.assert_same_bits(H.battery(ctx, inp), want, "%s: %s data after %s data" % (path, then, first))


def _rel_rows(a, b):
    """rel_err chain by chain (the int8 tests' convention), worst chain"""
    return max(rel_err(a[c], b[c]) for c in range(len(b)))


@pytest.mark.parametrize("path", list(H.PATHS))
def test_fresh_battery_matches_oracle(hip, oracle, path):
    """assertion 4.  Tolerances, by call: test_callbacks_match_oracle / test_large_d_callbacks_match_oracle (log joint 1e-12, G 1e-12,
    log det and gradient 1e-11, trace and quadratic terms 1e-9, large-D 1e-8), test_leapfrog_matches_oracle (TOL_STEP after <= 1 step,
    TOL_TRAJ after more), test_medium_one_launch_step_matches_generic_and_oracle (transition, sample), test_device_ess_matches_reference_
    and_host (sample_stats; ess against tools.CalculateESS as there), test_fused_small_path_matches_oracle_and_generic (chains),
    test_hmc_one_launch_trajectory_matches_generic_and_oracle (HMC), test_mmala.py's GPU cases (mMALA); int8 paths: G_TOL / STEP_TOL
    of test_gpu_int8_metric.py per chain, whole trajectories 1e-8 at 6 slices and 1e-6 at 5 (its golden-tape test).  Integer outputs are exactly equal."""
    spec = H.PATHS[path]
    M, D, n, flags, _ = spec
    g = fresh(hip, path)
    inp = H.make_inputs(spec)
    with _context(oracle, spec, flags=flags & _capi.COMPAT) as ctx:
        o = H.battery(ctx, inp)
    assert set(o) <= set(g)
    i8 = bool(flags & _capi.FLAG_INT8_METRIC)
    S = (flags >> 12) & 7
    big = D > 64
    for k in sorted(o):
        if o[k].dtype.kind in "iu":
            if k.endswith(".status"):
                assert np.array_equal(g[k] != 0, o[k] != 0), k
            else:
                assert np.array_equal(g[k], o[k]), k
        assert np.array_equal(np.isfinite(g[k]), np.isfinite(o[k])), k
        assert np.isfinite(o[k]).all(), k

    def e(k):
        return rel_err(g[k], o[k])

    def rows(k):
        return _rel_rows(g[k], o[k])

    def scaled(k):
        return float(np.max(np.abs(g[k] - o[k]) / np.maximum(1.0, np.abs(o[k]))))

    err = {}
    # unit entry points
    err["log_posterior.ljl"] = (e("log_posterior.ljl"), 1e-12)
    assert np.array_equal(g["metric.G"], np.swapaxes(g["metric.G"], 1, 2))
    if i8:
        err["metric.G"] = (rows("metric.G"), G_TOL[S])
        err["metric.hld"] = (float(np.abs(g["metric.hld"] - o["metric.hld"]).max()), 1e3 * G_TOL[S])
        err["metric.grad"] = (e("metric.grad"), 1e-12)
        err["metric_terms.tr"] = (rows("metric_terms.tr"), 1e3 * G_TOL[S])
        err["metric_terms.q"] = (rows("metric_terms.q"), 1e3 * G_TOL[S])
    else:
        err["metric.G"] = (e("metric.G"), 1e-12)
        err["metric.hld"] = (e("metric.hld"), 1e-11)
        err["metric.grad"] = (e("metric.grad"), 1e-11)
        err["metric_terms.tr"] = (e("metric_terms.tr"), 1e-8 if big else 1e-9)
        err["metric_terms.q"] = (e("metric_terms.q"), 1e-8 if big else 1e-9)
    step = STEP_TOL[S] if i8 else TOL_STEP
    traj = (1e-6 if S == 5 else 1e-8) if i8 else TOL_TRAJ
    ns = inp["ns"]
    for c in range(n):
        tol = step if ns[c] <= 1 else traj
        err["leapfrog.w[%d]" % c] = (rel_err(g["leapfrog.w"][c], o["leapfrog.w"][c]), tol)
        err["leapfrog.p[%d]" % c] = (rel_err(g["leapfrog.p"][c], o["leapfrog.p"][c]), tol)
        err["leapfrog.hld[%d]" % c] = (abs(g["leapfrog.hld"][c] - o["leapfrog.hld"][c]) / max(1.0, abs(o["leapfrog.hld"][c])), tol)
    assert np.array_equal(g["leapfrog.w"][ns == 0], inp["wl"][ns == 0]) and np.array_equal(g["leapfrog.p"][ns == 0], inp["pl"][ns == 0])
    # one RMHMC transition, whole chains
    for k in ("w_prop", "p_prop", "w", "hld_prop"):
        err["transition." + k] = (e("transition." + k), traj)
    err["transition.H_prop"] = (e("transition.H_prop"), 10 * traj if i8 and S == 5 else 1e-8)
    err["transition.H_cur"] = (scaled("transition.H_cur"), 1e-9)
    err["sample.samples"] = (e("sample.samples"), 1e-7)
    err["sample_stats.mean"] = (e("sample_stats.mean"), 1e-7)
    err["sample_stats.var"] = (e("sample_stats.var"), 1e-6)
    err["sample_stats.ess"] = (e("sample_stats.ess"), 1e-5)
    err["chains.w"] = (e("chains.w"), 1e-7)
    # plain HMC, mMALA, ESS
    for k in ("w_prop", "p_prop", "H_prop", "w"):
        err["hmc_transition." + k] = (e("hmc_transition." + k), 1e-9)
    err["hmc_transition.H_cur"] = (scaled("hmc_transition.H_cur"), 1e-10)          # (check_hmc_against_tape)
    err["hmc_sample.samples"] = (e("hmc_sample.samples"), 1e-8)
    err["mmala_transition.w_prop"] = (rows("mmala_transition.w_prop"), 1e-8)
    err["mmala_transition.w"] = (rows("mmala_transition.w"), 1e-9)                 # (test_gpu_transition_matches_oracle)
    err["mmala_transition.ratio"] = (scaled("mmala_transition.ratio"), 1e-6)
    err["mmala_sample.samples"] = (e("mmala_sample.samples"), 1e-6)
    from riemannhamiltonianmontecarlo_amd import tools
    x = inp["ess_x"]
    ref = np.stack([tools.CalculateESS(x[i], x.shape[1] - 1, nfft="matlab").ravel() for i in range(len(x))])   # (as test_device_ess_...)
    err["ess.ess"] = (float(np.max(np.abs(g["ess.ess"] - ref) / np.abs(ref))), 1e-9)
    unbounded = sorted(k for k in o if o[k].dtype.kind == "f" and k not in {b.split("[")[0] for b in err})
    assert not unbounded, unbounded                              # every float output of the battery has a bound above
    worst = sorted(err.items(), key=lambda kv: -kv[1][0] / kv[1][1])
    print("%s: closest to its bound: %s" % (path, ", ".join("%s %.1e (< %.0e)" % (k, v[0], v[1]) for k, v in worst[:4])))
    bad = ["%s %.2e >= %.0e" % (k, v[0], v[1]) for k, v in worst if not v[0] < v[1]]
    assert not bad, "%s: %s" % (path, "; ".join(bad))
