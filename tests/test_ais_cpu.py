"""CPU-side checks of annealed importance sampling, include/rmhmc_ais.h: the header, the ctypes binding and the library's exports agree;
csrc/ais.h (merge and finish of weight partials, the ladders, the stage_mass pattern, the refusals of the run, the mass of a stage, the
blocks of the weight kernels) in a stand-alone program under AddressSanitizer and UBSan (tests/helpers/ais_probe.cpp, a child process:
nothing sanitised is loaded into this one) against the np.longdouble restatement tests/helpers/ais_ref.py; the restated tempered
transition against phmc_ref at beta = 1; and the restated annealing run against a quadrature of the evidence.

RTOL, the rounding bound of S1 and S2 of a partial or a merge against exact arithmetic.  A term is exp(x), x = lw - a <= 0 (2 x for S2).
Terms with x < -745.2 are 0 in a double and below 5e-324 exactly, against a sum >= 1 (the maximum's own term): nothing.  Otherwise x
carries the rounding of one subtraction, |x| 2^-53 <= 746 * 2^-53 absolute, which is the relative error it leaves in exp(x); exp itself
is good to 1 ulp = 2 * 2^-53 relative; the doubling 2 x is exact.  All terms are positive, so the sum of the terms inherits the largest
relative error of a term, 748 * 2^-53.  The sums are compensated pairs (error O(n 2^-106), nothing) rounded once at the end, and a merge
multiplies by one more exp of the same kind and adds once: 748 + 748 + 4 = 1500 units of 2^-53 cover a partial, a merge of partials and
their comparison with each other: RTOL = 1500 * 2^-53 = 1.7e-13.  log_mean_w = a + log(S1 / m): RTOL absolute plus 3 roundings of a
result of the size of a.  weight_ess = S1^2 / S2: 3 RTOL.  se^2 = (m S2 / S1^2 - 1) / (m - 1): the bracket's absolute error is
3 RTOL m S2 / S1^2 (the subtraction cancels, so the bound is absolute on se^2, not relative on se)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import riemannhamiltonianmontecarlo_amd as pkg
from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment, multi_gpu
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ais_ref as A  # noqa: E402
import phmc_ref as R  # noqa: E402
from probe_build import probe_exe  # noqa: E402

SYMBOLS = {"rmhmc_tphmc_transition", "rmhmc_tphmc_sample_to", "rmhmc_ais_prior", "rmhmc_ais_partial_dev", "rmhmc_ais_finish", "rmhmc_ais_run"}
RTOL = 1500 * 2.0 ** -53
_cache = {}


def _header():
    return open(os.path.join(ROOT, "include", "rmhmc_ais.h")).read()


def check_finish(got, want, what=""):
    """a finished estimate (dict of _capi.ais_finish or of the probe) against the longdouble restatement, to the bounds above"""
    assert got["m"] == want["m"] and got["n_nan"] == want["n_nan"], what
    gm, wm = np.asarray(got["merged"], dtype=A.LD), want["merged"]
    assert gm[0] == wm[0] and gm[1] == wm[1] and gm[2] == wm[2], (what, gm, wm)
    for i in (3, 4):
        assert abs(gm[i] - wm[i]) <= RTOL * wm[i], (what, i, float(gm[i]), float(wm[i]))
    for key in ("log_mean_w", "se", "weight_ess"):
        g, w = A.LD(got[key]), want[key]
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, key, g, w)
    if np.isfinite(want["log_mean_w"]):
        assert abs(A.LD(got["log_mean_w"]) - want["log_mean_w"]) <= RTOL + 3 * 2.0 ** -53 * max(1.0, abs(float(wm[2]))), what
        assert abs(A.LD(got["weight_ess"]) - want["weight_ess"]) <= 3 * RTOL * want["weight_ess"], what
    if np.isfinite(want["se"]):
        m, S1, S2 = wm[0], wm[3], wm[4]
        assert abs(A.LD(got["se"]) ** 2 - want["se"] ** 2) <= (3 * RTOL * m * S2 / (S1 * S1) + 4 * 2.0 ** -53) / (m - 1), what


# ---- the header, the binding, the exports -----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert syms == SYMBOLS == set(_capi.AIS_SIGNATURES)
    for other in (_capi.SIGNATURES, _capi.AMH_SIGNATURES, _capi.IWLS_SIGNATURES, _capi.GIBBS_SIGNATURES, _capi.OUT_SIGNATURES,
                  _capi.DIAG_SIGNATURES, _capi.PHMC_SIGNATURES, _capi.ADAPT_SIGNATURES):
        assert not syms & set(other)
    for name, (res, args) in _capi.AIS_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc_phmc.h"]
    assert int(re.search(r"#define\s+RMHMC_AIS_PRIOR_ITER\s+(0x[0-9A-Fa-f]+)u", _header()).group(1), 16) == _capi.AIS_PRIOR_ITER == 2 ** 32 - 1
    assert pkg.log_evidence is pkg.evidence.log_evidence and "log_evidence" in pkg.__all__


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_ais and not oracle.has_ais
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with oracle.context(10, 2, 1) as ctx:           # a library without the calls says so, with the header's name
        calls = (lambda: ctx.tphmc_transition(None, None, None, None), lambda: ctx.tphmc_sample_to(2, 0, samples=True),
                 lambda: ctx.ais_prior(), lambda: ctx.ais_partial(None), lambda: ctx.ais_run([1.0], [1]),
                 lambda: _capi.ais_finish([np.zeros(5)], lib=oracle))
        for call in calls:
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_ais.h" in str(e.value)


def test_sampler_tables_unchanged():
    assert set(_capi.SAMPLERS_TO) == set(_capi.SAMPLER_ARGS) == {"rmhmc", "hmc", "mmala", "amh", "iwls", "gibbs"}
    assert set(experiment.SAMPLERS) == {"RMHMC", "HMC", "mMALA", "AMH", "IWLS", "Gibbs"}
    assert set(multi_gpu._SHARDED) == set(experiment.SAMPLERS)


# ---- csrc/ais.h in a stand-alone program under AddressSanitizer and UBSan ------------------------------------------------------------------
def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _floats(line):
    return np.array([float.fromhex(v) if "x" in v else float(v) for v in line.split()])


def _hex(a):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.ravel(a))


def _finish(exe, parts):
    lines = _run(exe, "finish %d\n" % len(parts) + "\n".join(_hex(p) for p in parts) + "\n")
    head = lines[0].split()
    assert head[0] == "finish"
    out = dict(rc=int(head[1]), m=int(head[2]), n_nan=int(head[3]))
    if out["rc"] == 0:
        lm, se, ess = _floats(lines[2])
        out.update(merged=_floats(lines[1]), log_mean_w=lm, se=se, weight_ess=ess)
    return out


def weight_cases():
    """log weights that exercise the reduction: name -> array.  Spreads of +-1e4, -inf and NaN entries, all -inf, all NaN, one entry."""
    rs = np.random.RandomState(5)
    wide = 1e4 * (2.0 * rs.rand(300) - 1.0)
    mixed = rs.randn(257) * 3.0 - 40.0
    mixed[[3, 77, 200]] = -np.inf
    mixed[[0, 100, 256]] = np.nan
    return {"narrow": rs.randn(1000) * 0.5 + 7.0, "wide": wide, "wide_top": np.concatenate([wide, wide.max() - 1e-3 * rs.rand(50)]),
            "mixed": mixed, "equal": np.full(65, -3.25), "all_neg_inf": np.full(64, -np.inf), "all_nan": np.full(63, np.nan),
            "one": np.array([2.5]), "one_neg_inf": np.array([-np.inf]), "pair": np.array([-1e4, 1e4])}


def test_merge_and_finish_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "ais_probe")
    empty = np.array([0.0, 0.0, -np.inf, 0.0, 0.0])
    for name, lw in weight_cases().items():
        whole = A.partial(lw).astype(np.float64)
        got = _finish(exe, [whole])
        assert got["rc"] == 0
        check_finish(got, A.finish([A.partial(lw)]), name)
        if len(lw) >= 60:                               # unequal pieces, one of a single entry, empties in between
            cuts = [0, 7, 8, 40, len(lw)]
            pieces = [A.partial(lw[a:b]).astype(np.float64) for a, b in zip(cuts[:-1], cuts[1:])]
            for parts in (pieces, [empty] + pieces[:2] + [empty] + pieces[2:] + [empty], pieces[::-1]):
                got = _finish(exe, parts)
                check_finish(got, A.finish([A.partial(lw)]), name + " in pieces")
                check_finish(got, A.finish(parts), name + " merged")
        got = _finish(exe, [empty, whole, empty])        # the identity, to the bit
        assert got["merged"].tobytes() == whole.tobytes()
    # m < 2: no standard error; m = 0: nothing at all; every weight zero: -inf
    one = _finish(exe, [A.partial([2.5]).astype(np.float64)])
    assert one["m"] == 1 and one["log_mean_w"] == 2.5 and np.isnan(one["se"]) and one["weight_ess"] == 1.0
    none = _finish(exe, [empty, A.partial([np.nan, np.nan]).astype(np.float64)])
    assert none["m"] == 0 and none["n_nan"] == 2 and np.isnan(none["log_mean_w"]) and np.isnan(none["se"]) and np.isnan(none["weight_ess"])
    zero = _finish(exe, [A.partial([-np.inf] * 4).astype(np.float64)])
    assert zero["m"] == 4 and zero["log_mean_w"] == -np.inf and np.isnan(zero["se"]) and zero["merged"][2] == -np.inf
    eq = _finish(exe, [A.partial(np.full(65, -3.25)).astype(np.float64)])
    assert eq["log_mean_w"] == -3.25 and eq["se"] == 0.0 and eq["weight_ess"] == 65.0
    assert _finish(exe, [])["rc"] == -1


@pytest.mark.parametrize("T", [1, 2, 3, 1000])
def test_schedules(tmp_path_factory, T):
    exe = probe_exe(tmp_path_factory, "ais_probe")
    for cmd, arg, want, name in (("power", 4.0, A.ladder_power(T, 4.0), "power4"), ("power", 1.0, A.ladder_power(T, 1.0), "power1"),
                                 ("log", 1e-6, A.ladder_log(T, 1e-6), "log"), ("log", 0.01, A.ladder_log(T, 0.01), "log0.01")):
        lines = _run(exe, "%s %d %s\n" % (cmd, T, float(arg).hex()))
        assert lines[0] == "ladder 0"
        got = _floats(lines[1])
        py = _capi.ais_schedule(T, name)[0]
        # pow and exp of the C library are good to 1 ulp; their argument carries two roundings, which the power q = 4 turns into 4 ulp and
        # the exponent |log 1e-6 (1 - f)| <= 13.9 into 2 * 13.9 * 2^-53 relative = 14 ulp: 32 spacings cover both
        for b in (got, py):
            assert b.shape == (T,) and b[-1] == 1.0 and np.all(np.diff(b) > 0) and b[0] > 0
            assert np.all(np.abs(b.astype(A.LD) - want) <= 32 * np.spacing(b)), (cmd, T)
        assert np.array_equal(got, py)           # both call the same C library
    if T == 3:
        assert _capi.ais_schedule(3, "power4")[0].tolist() == [(1.0 / 3.0) ** 4, (2.0 / 3.0) ** 4, 1.0]
    by_hand = {1: {1: [1], 2: [1], 5: [1]}, 2: {1: [1, 1], 2: [1, 1], 5: [1, 1]}, 3: {1: [1, 1, 1], 2: [1, 0, 1], 5: [1, 0, 1]}}
    for every in (1, 2, 5):
        want = by_hand[T][every] if T in by_hand else A.stage_mass(T, every)
        assert _run(exe, "smass %d %d\n" % (T, every)) == ["smass 0 " + " ".join(str(v) for v in want)]
        beta, length, sm = _capi.ais_schedule(T, "power4", every, 3)
        assert sm.tolist() == want and sm.dtype == np.int32 and length.tolist() == [3] * T and length.dtype == np.int64
    if T == 1000:
        assert sum(A.stage_mass(T, 5)) == 201 and A.stage_mass(T, 5)[995:] == [1, 0, 0, 0, 1]
    assert _capi.ais_schedule(T, "power4", None)[2] is None


def test_refusals_and_stage_mass_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "ais_probe")
    for line in ("power 0 4", "power 3 0", "power 3 -1", "power 3 nan", "power 3 inf", "log 0 0.5", "log 3 0", "log 3 1", "log 3 nan"):
        assert _run(exe, line + "\n") == ["ladder -1"], line
    for line in ("smass 0 1", "smass 3 0", "smass 3 -2"):
        assert _run(exe, line + "\n") == ["smass -1"], line
    for bad in (dict(n_temps=0), dict(n_temps=2.5), dict(n_temps=3, ladder="linear"), dict(n_temps=3, ladder="power0"),
                dict(n_temps=3, ladder="powerx"), dict(n_temps=3, ladder="log1"), dict(n_temps=3, ladder=4), dict(n_temps=3, mass_every=0),
                dict(n_temps=3, iters_per_temp=0)):
        with pytest.raises(ValueError):
            _capi.ais_schedule(**bad)
    ok = "0.1 1 1 0.5 2 0 1 1 1"

    def check(head, stages=ok):
        return _run(exe, "check %s\n%s\n" % (head, stages))[0]
    #            have_theta0 beta0 T L have_H have_smass
    assert check("0 0 3 6 1 1") == "check ok" and check("1 0.3 3 6 1 1") == "check ok" and check("1 0 3 6 0 0") == "check ok"
    assert check("0 0 0 6 1 1", "") != "check ok"                       # T < 1
    assert check("0 0 3 0 1 1") != "check ok"                           # L < 1
    assert check("0 0.3 3 6 1 1") != "check ok"                         # prior start with beta0 != 0
    assert check("1 -0.1 3 6 1 1") != "check ok" and check("1 nan 3 6 1 1") != "check ok" and check("1 inf 3 6 1 1") != "check ok"
    assert check("0 0 3 6 0 1") != "check ok"                           # a stage installs a mass, no H_lik
    assert check("0 0 3 6 0 1", "0.1 1 0 0.5 2 0 1 1 0") == "check ok"  # ... but none does
    for stages in ("0.1 1 1 -0.5 2 0 1 1 1", "0.1 1 1 nan 2 0 1 1 1", "0.1 1 1 inf 2 0 1 1 1", "0.1 0 1 0.5 2 0 1 1 1", "0.1 1 2 0.5 2 0 1 1 1",
                   "0.1 1 -1 0.5 2 0 1 1 1"):
        assert check("0 0 3 6 1 1", stages) != "check ok", stages
    assert check("0 0 3 6 1 1", "1 1 1 0.5 2 0 0 1 1") == "check ok"    # nothing requires the ladder to be monotone
    # the mass of a stage: a product and a sum per entry, and what the factorisation says of it
    rs = np.random.RandomState(3)
    B = rs.randn(7, 5)
    H = B.T @ B
    for beta in (0.0, 1e-6, 0.3, 1.0):
        lines = _run(exe, "mass %s 5 %s\n%s\n" % (float(beta).hex(), float(0.01).hex(), _hex(H)))
        assert lines[0] == "mass 0"
        assert np.array_equal(_floats(lines[1]).reshape(5, 5), A.stage_mass_matrix(beta, H))
    assert _run(exe, "mass 1 5 0.01\n%s\n" % _hex(-H))[0] == "mass -1"              # not positive definite: refused
    bad = H.copy(); bad[1, 0] = np.nan
    assert _run(exe, "mass 1 5 0.01\n%s\n" % _hex(bad))[0] == "mass -1"
    # the blocks of the weight kernels, by hand: multiples of 256 entries, at most 1024 blocks
    want = {1: (1, 256), 256: (1, 256), 257: (2, 256), 1000: (4, 256), 70001: (274, 256), 262144: (1024, 256), 262145: (513, 512)}
    lines = _run(exe, "".join("plan %d\n" % n for n in want))
    assert {n: tuple(int(v) for v in line.split()[1:]) for n, line in zip(want, lines)} == want


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restated_transition_at_beta_one_is_phmc():
    XX, t = synthetic_logreg(60, 5, 2)
    rs = np.random.RandomState(0)
    G = R.metric(XX, R.mode(XX, t)["w"])
    Lm = np.linalg.cholesky(G)
    for c in range(12):
        w = rs.randn(5) * 0.3; z = rs.randn(5); ul, ua = rs.rand(), rs.rand()
        want = R.transition(XX, t, Lm, w, z, ul, ua, 6, 0.5)
        got = A.transition(XX, t, Lm, w, z, ul, ua, 6, 0.5, 1.0)
        for k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
        assert got["loglik0"] == A.loglik(XX, t, w) and got["loglik"] == A.loglik(XX, t, got["w"])
    # beta = 0: the likelihood has no say - the proposal and the decision are those of the prior alone
    got = A.transition(XX, t, None, w, z, 0.9, 0.5, 6, 0.5, 0.0)
    other = A.transition(XX, 1.0 - np.ravel(t), None, w, z, 0.9, 0.5, 6, 0.5, 0.0)
    assert np.array_equal(got["w_prop"], other["w_prop"]) and got["H_prop"] == other["H_prop"]


PROBLEMS = {"m40_d2": (40, 2, 128), "m25_d1": (25, 1, 64)}     # (M, D, stages); 4096 chains, ladder ((k + 1) / T)^4, a mass per stage
N_CHAINS = 4096


def quadrature(name):
    if ("quad", name) not in _cache:
        M, D, _ = PROBLEMS[name]
        XX, t = synthetic_logreg(M, D, 0)
        _cache[("quad", name)] = A.log_evidence_quadrature(XX, t)
    return _cache[("quad", name)]


def test_quadrature_is_converged():
    """the reference of the estimator tests: the same integral on a grid of twice the spacing and on one half as wide again agrees to
    1e-8, six orders below the standard error of the estimates (measured: 6e-12 and 3e-10; the tails are heavier than a Gaussian's,
    a grid of +-9 standard deviations is off by 2e-7)"""
    for name, (M, D, _) in PROBLEMS.items():
        XX, t = synthetic_logreg(M, D, 0)
        fine = quadrature(name)
        assert abs(A.log_evidence_quadrature(XX, t, points=601) - fine) < 1e-8
        assert abs(A.log_evidence_quadrature(XX, t, half_width=18.0, points=1201) - fine) < 1e-8
        G = R.metric(XX, R.mode(XX, t)["w"])
        w = R.mode(XX, t)["w"]
        laplace = R.ljl_grad(XX, t, w)[0] + 0.5 * D * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(G)[1]
        print("%s: log evidence by quadrature %.5f, Laplace %.5f" % (name, fine, laplace))
        assert abs(laplace - fine) < 0.2


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_restated_ais_meets_the_quadrature(name, seed):
    """|log Z - quadrature| <= 5 se with se <= 0.03, weight-ESS >= n / 4 and no failed chain, each seed printing its figures."""
    M, D, T = PROBLEMS[name]
    XX, t = synthetic_logreg(M, D, 0)
    H = R.metric(XX, R.mode(XX, t)["w"]) - np.eye(D) / 100.0
    r = A.run(XX, t, N_CHAINS, np.asarray(A.ladder_power(T, 4.0), dtype=np.float64), [1] * T, H, seed=seed)
    f = A.finish([A.partial(r["logw"])])
    lz, se, ess = float(f["log_mean_w"]), float(f["se"]), float(f["weight_ess"])
    ref = quadrature(name)
    print("%s seed %d: log Z %.5f, quadrature %.5f, (log Z - quadrature) / se %+.2f, se %.4f, weight-ESS %.0f, acceptance %.3f .. %.3f"
          % (name, seed, lz, ref, (lz - ref) / se, se, ess, r["accept_trace"].min(), r["accept_trace"].max()))
    assert f["n_nan"] == 0 and f["m"] == N_CHAINS
    assert se <= 0.03 and ess >= N_CHAINS / 4
    assert abs(lz - ref) <= 5 * se


# ---- the shim's checks: before the library is touched ------------------------------------------------------------------------------------
class _NoLibrary:
    """stands in for the library: the argument checks must raise before anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the shim touched the library (%s) before refusing its arguments" % name)


def test_shim_argument_checks_need_no_library():
    XX, t = synthetic_logreg(30, 3, 0)
    bad = [dict(XX=XX[0]), dict(t=t[:-1]), dict(n_chains=1), dict(n_chains=2.5), dict(n_temps=0), dict(iters_per_temp=0), dict(ladder="linear"),
           dict(ladder="power-1"), dict(mass="identity"), dict(mass=np.eye(3)), dict(mass_every=0), dict(NumOfLeapFrogSteps=0),
           dict(StepSize=0.0), dict(StepSize=np.nan), dict(alpha=0.0), dict(alpha=np.inf)]
    for kw in bad:
        args = dict(XX=XX, t=t, n_chains=8, n_temps=4, _lib=_NoLibrary())
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.log_evidence(**args)
