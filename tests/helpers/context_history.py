"""Harness of tests/test_gpu_context_history.py and tests/test_context_history_cpu.py: one battery of calls with fixed inputs on one
context, and "polluters" that leave a context full of some other call's state before the battery runs.

The invariant under test: what an entry point returns is a function of the data set, the options and its own
arguments, never of what the context was used for before.  The battery therefore starts every call from caller-supplied state.

Both libraries are driven through the same `_capi.Context`; what the CPU oracle cannot express (AMH / IWLS / Gibbs, run-time options,
the int8 certificate) is left out where the library says so (`rl.on_gpu`, `rl.has_*`)."""
import ctypes as C

import numpy as np

from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from plan_probe import plan

I8 = _capi.int8_metric_flags

# id -> M, D, n, flags, data seed: the smallest shape that reaches each stepping path (rmhmc_create_opts)
PATHS = {
    "fused": (150, 6, 5, _capi.COMPAT, 31),
    "medium": (270, 14, 5, _capi.COMPAT, 32),
    "generic": (300, 40, 20, 0, 33),
    "generic_rowsplit": (600, 40, 70, 0, 34),
    "int8": (300, 40, 130, I8(6), 35),
    "int8_s5": (203, 33, 7, I8(5), 36),
    "large": (200, 70, 3, 0, 37),
    "large_int8": (300, 100, 4, I8(6), 38),
}
# The certificate (rmhmc_set_data) bounds the int8 error of G_ab by S M 2^(e_ab - 8 S) / sqrt(G0_aa G0_bb), 2^e_ab <= 2 max_n |x_na x_nb|
# and G0_aa >= sum_n x_na^2 / 4.  By Cauchy-Schwarz max_n |x_na x_nb| <= 4 sqrt(G0_aa G0_bb), so the bound is at most
# 8 S M 2^(-8 S) (x 11/6 with the delta assembly) = 3.1e-13 M at 6 slices, whatever the data: below about 3200 rows NO data set can
# fail the 1e-9 certificate.  The certificate cases therefore run the int8 paths' D, n and flags with M = 6000, the row count of
# test_outlier_row_is_sent_to_fp64_by_the_certificate (bound 1.8e-9 there).
CERT_PATHS = {
    "int8": (6000, 40, 130, I8(6) | _capi.FLAG_INT8_CERTIFY, 35),
    "large_int8": (6000, 100, 4, I8(6) | _capi.FLAG_INT8_CERTIFY, 38),
}
ESS_S = 200
REPLAY_T = 3            # iterations of the replay calls


def assert_path(ctx, path, certify_active=True, paths=None):
    """the stepping path the shape was chosen for is the one the context reports (paths: the table the shape is from, PATHS by default;
    certify_active = False: an int8 context whose data the certificate has sent to the fp64 kernels)"""
    M, D, n, flags, _ = (paths or PATHS)[path]
    info = ctx.device_info().split("; options:")[0]
    suffixes = {"fused": "fused small-problem path", "medium": "one-launch step", "large": "blocked large-D path"}
    want = {"fused": "fused", "medium": "medium", "large": "large", "large_int8": "large"}.get(path)
    for key, text in suffixes.items():
        assert (text in info) == (key == want), (path, info)
    if flags & _capi.FLAG_INT8_METRIC:
        S = (flags >> 12) & 7
        state = "active" if certify_active else "NOT certified"
        assert "int8 metric path %d slices: %s" % (S, state) in info, (path, info)
        assert ctx.int8_certificate()[1] == bool(certify_active)
    else:
        assert "int8" not in info, (path, info)
    if path == "generic":                      # (row ranges of the fp64 assembly: the rule itself, csrc/plan.h)
        assert plan(M, D, n, flags)["fsplit"] == 1
    if path == "generic_rowsplit":
        assert plan(M, D, n, flags)["fsplit"] > 1


def data_of(spec, variant="own"):
    """own: the path's data set; other: a different one of the same shape; outlier: own with one row 1000 x the others"""
    M, D, n, flags, seed = spec
    if variant == "other":
        return synthetic_logreg(M, D, seed + 50)
    XX, t = synthetic_logreg(M, D, seed)
    if variant == "outlier":
        XX = XX.copy(); XX[M // 5] *= 1e3
    return XX, t


def make_inputs(spec):
    """fixed arguments of every call of the battery, drawn like the inputs of tests/test_gpu_parity.py"""
    M, D, n, flags, seed = spec
    rs = np.random.RandomState(1000 + seed)
    inp = dict(M=M, D=D, n=n)
    inp["w"] = 0.3 * rs.randn(n, D) / np.sqrt(D); inp["p"] = rs.randn(n, D)
    inp["wl"] = 0.2 * rs.randn(n, D) / np.sqrt(D); inp["pl"] = 2.0 * rs.randn(n, D)
    ns = rs.randint(0, 4, size=n).astype(np.int32); ns[0] = 1; ns[1] = 0; ns[2] = 3
    inp["ns"] = ns
    dr = np.where(rs.rand(n) < 0.5, 1, -1).astype(np.int32); dr[0] = 1; dr[2] = -1
    inp["dir"] = dr
    inp["wt"] = 0.2 * rs.randn(n, D) / np.sqrt(D); inp["z"] = rs.randn(n, D)
    inp["ul"] = rs.rand(n); inp["gd"] = rs.randn(n); inp["ua"] = rs.rand(n)
    inp["wh"] = 0.1 * rs.randn(n, D); inp["zh"] = rs.randn(n, D); inp["ulh"] = rs.rand(n); inp["uah"] = rs.rand(n)
    inp["wm"] = 0.1 * rs.randn(n, D); inp["zm"] = rs.randn(n, D); inp["uam"] = rs.rand(n)
    inp["ess_x"] = np.cumsum(rs.randn(3, ESS_S, D), axis=1) * 0.05 + rs.randn(3, ESS_S, D)
    inp["eps_lf"] = 0.3 if D > 64 else 0.5
    # the tapes of the three replays (a stream of their own: the inputs above are the ones they always were)
    rr = np.random.RandomState(2000 + seed)
    T = REPLAY_T
    inp["amh_z"] = rr.randn(n, T, D); inp["amh_u"] = rr.rand(n, T, D)
    inp["iwls_wp"] = 0.1 * rr.randn(n, T, D); inp["iwls_u"] = rr.rand(n, T)
    # Gibbs: two attempts per row and iteration (the same ranges in every iteration), the second with the acceptance uniform 0, which
    # every proposal passes (gibbs_sampler.py:21,41: a positive partial sum exceeds it): no chain's tape runs out, status stays 0
    ks = np.stack([rr.randn(n, 2 * M), rr.rand(n, 2 * M), rr.rand(n, 2 * M)], axis=2); ks[:, 1::2, 2] = 0.0
    off = np.ascontiguousarray(np.broadcast_to(2 * np.arange(M + 1, dtype=np.int64), (n, T, M + 1)))
    inp["gibbs_tapes"] = (rr.rand(n, M), rr.rand(n, T, M), rr.randn(n, T, D), ks, off)
    return inp


# ---- the battery -----------------------------------------------------------------------------------------------------------------
def _log_posterior(ctx, i):
    return {"ljl": ctx.log_posterior(i["w"])}


def _metric(ctx, i):
    G, hld, g = ctx.metric(i["w"])
    return {"G": G, "hld": hld, "grad": g}


def _metric_terms(ctx, i):
    tr, q = ctx.metric_terms(i["w"], i["p"])
    return {"tr": tr, "q": q}


def _leapfrog(ctx, i):
    w, p, hld, st = ctx.leapfrog(i["wl"], i["pl"], i["eps_lf"], i["dir"], i["ns"], 4)
    return {"w": w, "p": p, "hld": hld, "status": st}


def _transition(ctx, i):
    return ctx.transition(i["wt"], i["z"], i["ul"], i["gd"], i["ua"], L=3, eps=0.4, K=4)


def _sample(ctx, i):
    s, acc, steps, _ = ctx.sample(12, 4, L=3, eps=0.4, K=4, seed=5, chain_offset=2)
    return {"samples": s, "accepted": acc, "leapfrog_steps": steps}


def _sample_stats(ctx, i):
    r = ctx.sample_stats(12, 4, L=3, eps=0.4, K=4, seed=5, chain_offset=2)
    r.pop("seconds")
    return r


def _chains(ctx, i):
    ctx.chains_init(seed=6, chain_offset=1, L=3, eps=0.4, K=4)
    ctx.chains_run(9)
    w, it, acc = ctx.chains_state()
    return {"w": w, "iters": it, "accepted": acc}


def _hmc_transition(ctx, i):
    return ctx.hmc_transition(i["wh"], i["zh"], i["ulh"], i["uah"], L=8, eps=0.05)


def _hmc_sample(ctx, i):
    s, acc, steps, _ = ctx.hmc_sample(10, 3, L=8, eps=0.05, seed=7, chain_offset=1)
    return {"samples": s, "accepted": acc, "leapfrog_steps": steps}


def _mmala_transition(ctx, i):
    return ctx.mmala_transition(i["wm"], i["zm"], i["uam"], 0.5)


def _mmala_sample(ctx, i):
    s, acc, _ = ctx.mmala_sample(20, 8, 0.5, seed=8, chain_offset=3)
    return {"samples": s, "accepted": acc}


def _ess(ctx, i):
    return {"ess": ctx.ess(i["ess_x"])}


def _amh_sample(ctx, i):
    s, acc, sd, _ = ctx.amh_sample(60, 20, seed=9, chain_offset=1)
    return {"samples": s, "accepted": acc, "sd": sd}


def _iwls_sample(ctx, i):
    s, acc, sat, _ = ctx.iwls_sample(12, 4, seed=10, chain_offset=1)
    return {"samples": s, "accepted": acc, "saturated": sat}


def _gibbs_sample(ctx, i):
    r = ctx.gibbs_sample(8, 3, seed=11, chain_offset=1, state=True)
    r.pop("seconds")
    return r


def _amh_replay(ctx, i):
    return ctx.amh_replay(REPLAY_T, 1, i["amh_z"], i["amh_u"])


def _iwls_replay(ctx, i):
    return ctx.iwls_replay(i["iwls_wp"], i["iwls_u"])


def _gibbs_replay(ctx, i):
    r = ctx.gibbs_replay(*i["gibbs_tapes"])
    assert not r["status"].any(), r["status"]          # (no chain stopped: the records below are those of every iteration)
    return r


CALLS = [("log_posterior", _log_posterior), ("metric", _metric), ("metric_terms", _metric_terms), ("leapfrog", _leapfrog),
         ("transition", _transition), ("sample", _sample), ("sample_stats", _sample_stats), ("chains", _chains),
         ("hmc_transition", _hmc_transition), ("hmc_sample", _hmc_sample), ("mmala_transition", _mmala_transition),
         ("mmala_sample", _mmala_sample), ("ess", _ess), ("amh_sample", _amh_sample), ("iwls_sample", _iwls_sample),
         ("gibbs_sample", _gibbs_sample), ("amh_replay", _amh_replay), ("iwls_replay", _iwls_replay), ("gibbs_replay", _gibbs_replay)]


def calls_for(ctx):
    """the calls of the battery this library and shape support"""
    # (IWLS and Gibbs: D <= 64, RMHMC_ERR_UNSUPPORTED above)
    amh, iwls, gibbs = ctx.rl.has_amh, ctx.rl.has_iwls and ctx.D <= 64, ctx.rl.has_gibbs and ctx.D <= 64
    have = {"amh_sample": amh, "iwls_sample": iwls, "gibbs_sample": gibbs, "amh_replay": amh, "iwls_replay": iwls, "gibbs_replay": gibbs}
    return [(name, fn) for name, fn in CALLS if have.get(name, True)]


def battery(ctx, inputs, order="forward", after=None):
    """Every call of the battery on `ctx`, forward or reversed; returns {"call.output": array}.  `after(name, ctx)` is called after
    each call (used to read the delta-assembly counters after `sample`)."""
    assert order in ("forward", "reversed")
    calls = calls_for(ctx)
    if order == "reversed":
        calls = calls[::-1]
    out = {}
    with np.errstate(all="ignore"):
        for name, fn in calls:
            for k, v in fn(ctx, inputs).items():
                out[name + "." + k] = np.array(v, copy=True)
            if after is not None:
                after(name, ctx)
    return out


def assert_same_bits(got, want, what=""):
    """bit-identical dicts: same keys, same dtypes and shapes, equal values with NaNs compared by position"""
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    bad = []
    for k in sorted(want):
        a, b = got[k], want[k]
        same = a.dtype == b.dtype and a.shape == b.shape and (
            np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))
        if not same:
            d = ""
            if a.shape == b.shape and a.dtype.kind == "f":
                with np.errstate(all="ignore"):
                    diff = np.abs(a - b); diff[np.isnan(a) & np.isnan(b)] = 0.0
                    chains = sorted(set(np.argwhere(~(diff == 0)).T[0].tolist())) if a.ndim else []
                d = " max|diff| %.3e, %d entries, leading indices %s" % (np.nanmax(diff), int((~(diff == 0)).sum()), chains[:8])
            bad.append(k + d)
    assert not bad, "%s: outputs that differ: %s" % (what, "; ".join(bad))


# ---- calls whose arguments the Python wrapper would refuse itself: straight to the C-ABI ------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def raw_sample(ctx, n_iter, burn_in, L, K):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); k = np.zeros(n, dtype=np.int64); secs = C.c_double(0)
    return ctx.lib.rmhmc_sample(ctx._h, n_iter, burn_in, L, 0.4, K, 1, 0, None, _dp(s), _lp(a), _lp(k), C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_sample_stats(ctx, n_iter, burn_in, L, K):
    n, D = ctx.n, ctx.D
    m = np.zeros((n, D)); v = np.zeros((n, D)); e = np.zeros((n, D)); a = np.zeros(n, dtype=np.int64); k = np.zeros(n, dtype=np.int64)
    secs = C.c_double(0)
    return ctx.lib.rmhmc_sample_stats(ctx._h, n_iter, burn_in, L, 0.4, K, 1, 0, None, _dp(m), _dp(v), _dp(e), _lp(a), _lp(k),
                                      C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_hmc_sample(ctx, n_iter, burn_in, L):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); k = np.zeros(n, dtype=np.int64); secs = C.c_double(0)
    return ctx.lib.rmhmc_hmc_sample(ctx._h, n_iter, burn_in, L, 0.05, 1, 0, None, _dp(s), _lp(a), _lp(k), C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_mmala_sample(ctx, n_iter, burn_in, eps):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); secs = C.c_double(0)
    return ctx.lib.rmhmc_mmala_sample(ctx._h, n_iter, burn_in, eps, 1, 0, None, _dp(s), _lp(a), C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_amh_sample(ctx, n_iter, burn_in):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); sd = np.zeros((n, D)); secs = C.c_double(0)
    return ctx.lib.rmhmc_amh_sample(ctx._h, n_iter, burn_in, 1, 0, None, _dp(s), _lp(a), _dp(sd), C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_iwls_sample(ctx, n_iter, burn_in):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); b = np.zeros(n, dtype=np.int64); secs = C.c_double(0)
    return ctx.lib.rmhmc_iwls_sample(ctx._h, n_iter, burn_in, 1, 1, 0, None, _dp(s), _lp(a), _lp(b), C.cast(C.byref(secs), C.POINTER(C.c_double)))


def raw_gibbs_sample(ctx, n_iter, burn_in):
    n, D = ctx.n, ctx.D
    s = np.zeros((n, max(1, n_iter - burn_in), D)); a = np.zeros(n, dtype=np.int64); b = np.zeros(n, dtype=np.int64); secs = C.c_double(0)
    return ctx.lib.rmhmc_gibbs_sample(ctx._h, n_iter, burn_in, 1, 0, _dp(s), _lp(a), _lp(b), None, None, C.cast(C.byref(secs), C.POINTER(C.c_double)))


def _code(fn, *a):
    try:
        fn(*a)
    except _capi.RmhmcError as e:
        return e.code
    return 0


# ---- polluters: (ctx, path spec, inputs) -> None; results are thrown away, the context ends with the path's own data and default options
def _own(ctx, spec):
    XX, t = data_of(spec)
    ctx.set_data(XX, t, 100.0)


def _other_data(ctx, spec, inp, scale, eps):
    X2, t2 = data_of(spec, "other")
    ctx.set_data(X2 * scale, t2, 7.0)
    with np.errstate(all="ignore"):
        ctx.transition(inp["wt"], inp["z"], inp["ul"], inp["gd"], inp["ua"], L=3, eps=eps, K=4)
        ctx.chains_init(seed=3, L=3, eps=eps, K=4)
        ctx.chains_run(5)
    _own(ctx, spec)


def other_data_larger(ctx, spec, inp):
    """another data set of the same shape, 8 x larger than the path's own, with a different prior; then the path's own data.  What the
    larger data set leaves behind (exponents, slice counts, maxima) is not masked by a maximum taken over the smaller one"""
    _other_data(ctx, spec, inp, 8.0, 0.05)


def other_data_smaller(ctx, spec, inp):
    """the same with a data set 64 x smaller than the path's own"""
    _other_data(ctx, spec, inp, 1.0 / 64, 0.4)


def diverged(ctx, spec, inp):
    """chains that end NOT_PD / NONFINITE: the far-out start on strongly scaled data of test_divergent_chain_is_rejected_not_fatal, the
    overflowing HMC chain of test_hmc_sampler_matches_oracle_and_shim, the NaN position of test_nonfinite_chain_is_rejected_and_isolated"""
    M, D, n = inp["M"], inp["D"], inp["n"]
    XX, t = data_of(spec)
    bad = _capi.ST_NOT_PD | _capi.ST_NONFINITE
    rs = np.random.RandomState(2)
    w = 0.01 * rs.randn(n, D); w[1] = 400.0
    z = rs.randn(n, D)
    with np.errstate(all="ignore"):
        ctx.set_data(XX * 30.0, t, 100.0)
        r = ctx.transition(w, z, np.full(n, 0.9), np.full(n, 1.0), np.full(n, 0.5), L=6, eps=0.5, K=4)
        assert r["status"][1] & bad, r["status"]
        assert r["accepted"][1] == 0 and np.array_equal(r["w"][1], w[1])
        ctx.set_data(XX * 50.0, t, 100.0)
        w0 = np.zeros((n, D)); w0[1] = 300.0
        r = ctx.hmc_transition(w0, np.ones((n, D)), np.full(n, 0.5), np.full(n, 0.5), L=10, eps=0.5)
        assert r["accepted"][1] == 0 and np.array_equal(r["w"][1], w0[1])
        _own(ctx, spec)
        c = min(17, n - 1)
        wbad = inp["wt"].copy(); wbad[c, min(3, D - 1)] = np.nan
        r = ctx.transition(wbad, inp["z"], inp["ul"], inp["gd"], inp["ua"], L=3, eps=0.5, K=4)
        assert r["accepted"][c] == 0 and r["status"][c] & bad, r["status"]
        wl = inp["wl"].copy(); wl[c, 0] = np.nan; wl[0] = 400.0
        _, _, _, st = ctx.leapfrog(wl, inp["pl"], 0.5, inp["dir"], np.maximum(inp["ns"], 1), 4)
        assert st[c] & bad and st[0] & bad, st


def other_samplers(ctx, spec, inp):
    """every other sampler of the library, with parameters of its own"""
    n, D = inp["n"], inp["D"]
    th = 0.05 * np.random.RandomState(4).randn(n, D)
    with np.errstate(all="ignore"):
        ctx.hmc_sample(9, 2, L=5, eps=0.03, seed=21, chain_offset=4, theta0=th)
        ctx.mmala_sample(11, 3, 0.7, seed=22, chain_offset=5, theta0=th)
        if ctx.rl.has_amh:
            ctx.amh_sample(45, 15, seed=23, chain_offset=6, theta0=th)
        if ctx.rl.has_iwls and D <= 64:
            ctx.iwls_sample(9, 2, compat=False, seed=24, chain_offset=7, theta0=th)
        if ctx.rl.has_gibbs and D <= 64:
            ctx.gibbs_sample(6, 1, seed=25, chain_offset=8)


def other_run(ctx, spec, inp):
    """a longer sorted run from another start with a progress callback, then a stepping run stopped mid-trajectory and restored"""
    n, D = inp["n"], inp["D"]
    th = 0.02 * np.random.RandomState(5).randn(n, D)
    seen = []
    ctx.set_progress(lambda ev, it, acc, tot: seen.append((ev, it)), first=3, every=4)
    with np.errstate(all="ignore"):
        ctx.sample(24, 10, L=5, eps=0.3, K=3, seed=31, chain_offset=9, theta0=th)
    ctx.set_progress(None)
    if ctx.rl.on_gpu:
        assert (_capi.EV_BURNIN_DONE, 11) in seen, seen
    with np.errstate(all="ignore"):
        ctx.chains_init(theta0=th, seed=32, chain_offset=3, L=5, eps=0.3, K=3)
        ctx.chains_run(7)
        w, it, acc = ctx.chains_state()
        ctx.chains_restore(it + 5, acc + 2)
        ctx.chains_run(2)


def failed_calls(ctx, spec, inp):
    """every bulk entry point once with arguments it must refuse, around one valid plain-HMC run"""
    n, D = inp["n"], inp["D"]
    gpu = ctx.rl.on_gpu
    _own(ctx, spec)                                                        # (chains_ready off: chains_run must be refused)
    assert _code(ctx.chains_run, 3) == -1
    assert raw_sample(ctx, 5, 5, 3, 4) == -1 and raw_sample(ctx, 5, 7, 3, 4) == -1      # burn_in >= n_iter
    assert raw_sample(ctx, 8, 2, 0, 4) == -1                                            # L = 0
    assert raw_sample_stats(ctx, 5, 5, 3, 4) == -1
    assert raw_hmc_sample(ctx, 5, 5, 4) == -1
    with np.errstate(all="ignore"):
        ctx.hmc_sample(8, 2, L=4, eps=0.04, seed=41)
    assert raw_hmc_sample(ctx, 8, 2, 0) == -1                                           # a refusal right after an HMC-mode run
    assert raw_mmala_sample(ctx, 8, 2, 0.0) == -1 and raw_mmala_sample(ctx, 4, 4, 0.5) == -1
    if gpu:   # (the oracle iterates K = 0 times, checks no argument of chains_init and has no length limit on its ESS)
        assert _code(ctx.chains_init, None, 1, 0, 0, 0.4, 4) == -1                      # L = 0
        assert raw_sample(ctx, 8, 2, 3, 0) == -1 and raw_sample_stats(ctx, 8, 2, 3, 0) == -1
        assert _code(ctx.chains_init, None, 1, 0, 3, 0.4, 0) == -1
        assert _code(ctx.ess, np.zeros((1, 20001, 2))) == -4
    assert _code(ctx.ess, np.zeros((1, 1, 2))) != 0                                     # S = 1
    if ctx.rl.has_amh:
        assert raw_amh_sample(ctx, 5, 5) == -1
    if ctx.rl.has_iwls:
        assert raw_iwls_sample(ctx, 5, 5) == -1
        assert raw_iwls_sample(ctx, 8, 2) == (-4 if D > 64 else 0)
    if ctx.rl.has_gibbs:
        assert raw_gibbs_sample(ctx, 5, 5) == -1
        assert raw_gibbs_sample(ctx, 6, 2) == (-4 if D > 64 else 0)
    assert _code(ctx.chains_run, 3) == -1                                               # still no chains_init that succeeded


def option_toggles(ctx, spec, inp):
    """each run-time option at a non-default value for one stepping run, then back to its default"""
    defaults = dict(ctx.options())
    for key, val in (("graph", 0), ("sorted", 0), ("inflight", 2), ("cdyn", 0), ("crestore", 0), ("i8_force_rebase", 1)):
        assert defaults[key] != val, key
        ctx.set_option(key, val)
        with np.errstate(all="ignore"):
            ctx.chains_init(seed=51, L=4, eps=0.6, K=4)
            ctx.chains_run(9)
            if key == "sorted":
                ctx.sample(16, 4, L=4, eps=0.6, K=4, seed=52)
        ctx.set_option(key, defaults[key])
    assert ctx.options() == defaults


def other_params(ctx, spec, inp):
    """the stepping entry points with run parameters the battery never uses: K = 1 and K = 2 (the two values at which the delta
    assemblies of the int8 path switch), L = 1, another step size, a large chain offset"""
    far = (1 << 40) + 12345
    with np.errstate(all="ignore"):
        for K in (1, 2):
            ctx.sample(12, 3, L=1, eps=0.25, K=K, seed=61, chain_offset=far)
            ctx.chains_init(seed=62, chain_offset=far, L=1, eps=0.25, K=K)
            ctx.chains_run(10)
            ctx.transition(inp["wt"], inp["z"], inp["ul"], inp["gd"], inp["ua"], L=1, eps=0.25, K=K)
            ctx.leapfrog(inp["wl"], inp["pl"], 0.25, inp["dir"], inp["ns"], K)


POLLUTERS = {"other_data_larger": other_data_larger, "other_data_smaller": other_data_smaller, "diverged": diverged,
             "other_samplers": other_samplers, "other_run": other_run,
             "failed_calls": failed_calls, "option_toggles": option_toggles, "other_params": other_params}
