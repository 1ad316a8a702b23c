"""CPU-side checks of adaptive sequential Monte Carlo, include/rmhmc_smc.h: the header, the ctypes binding and the library's exports agree;
csrc/smc.h (the candidate grids and the bracket rule of the search, the offset of a resampling, merge and finish of conditional-ESS
partials, the blocks of the prefix sum, every refusal) in a stand-alone program under AddressSanitizer and UBSan
(tests/helpers/smc_probe.cpp, a child process: nothing sanitised is loaded into this one) against the restatement
tests/helpers/smc_ref.py; the restatement itself against a brute-force conditional ESS and against the definition of the ancestors; and
the restated run against a quadrature of the evidence.

CESS_UNITS, the rounding bound of a merged pair's level L = a + log S in units of 2^-53, for partials that the longdouble restatement
made and were rounded to double: S carries half a unit, a merge multiplies by an exp (1 unit, and the rounding of its argument
a' - a: |a' - a| / 2 units where the exp is not below 2^-1075, i.e. at most 373) and adds (1 unit); log S and the sum a + log S are
taken in longdouble by the test.  2 + 373 + 2 per merge, three merges: 1200 units cover it."""
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
import phmc_ref as R  # noqa: E402
import smc_ref as S  # noqa: E402
from probe_build import probe_exe  # noqa: E402
from test_ais_cpu import PROBLEMS, _floats, _hex, quadrature  # noqa: E402

SYMBOLS = {"rmhmc_smc_cess_dev", "rmhmc_smc_cess_finish", "rmhmc_smc_choose_delta_dev", "rmhmc_smc_reweight_dev", "rmhmc_smc_quantise_dev",
           "rmhmc_smc_ancestors_dev", "rmhmc_smc_run"}
CESS_UNITS = 1200


def _header():
    return open(os.path.join(ROOT, "include", "rmhmc_smc.h")).read()


# ---- the header, the binding, the exports -----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    syms = set(re.findall(r"\b(rmhmc_smc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert syms == SYMBOLS == set(_capi.SMC_SIGNATURES)
    for other in (_capi.SIGNATURES, _capi.AMH_SIGNATURES, _capi.IWLS_SIGNATURES, _capi.GIBBS_SIGNATURES, _capi.OUT_SIGNATURES,
                  _capi.DIAG_SIGNATURES, _capi.PHMC_SIGNATURES, _capi.ADAPT_SIGNATURES, _capi.AIS_SIGNATURES, _capi.PRED_SIGNATURES):
        assert not syms & set(other)
    for name, (res, args) in _capi.SMC_SIGNATURES.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) and res is C.c_int, name
    assert re.findall(r'#include\s+"([^"]+)"', _header()) == ["rmhmc_ais.h"]
    defines = {k: int(v) for k, v in re.findall(r"#define\s+RMHMC_SMC_([A-Z_]+)\s+(\d+)", _header())}
    assert defines == dict(MAX_J=_capi.SMC_MAX_J, J=_capi.SMC_J, ROUNDS=_capi.SMC_ROUNDS, MAX_N=_capi.SMC_MAX_N, QBITS=_capi.SMC_QBITS,
                           LAST=_capi.SMC_LAST, FLOOR=_capi.SMC_FLOOR, RESAMPLED=_capi.SMC_RESAMPLED)
    assert defines == dict(MAX_J=S.MAX_J, J=S.J, ROUNDS=S.ROUNDS, MAX_N=S.MAX_N, QBITS=S.QBITS, LAST=S.LAST, FLOOR=S.FLOOR, RESAMPLED=S.RESAMPLED)
    assert pkg.log_evidence_adaptive is pkg.evidence.log_evidence_adaptive and "log_evidence_adaptive" in pkg.__all__


def test_library_exports_and_oracle_does_not(hip, oracle):
    assert hip.has_smc and not oracle.has_smc
    lib = C.CDLL(hip.path)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    with oracle.context(10, 2, 1) as ctx:           # a library without the calls says so, with the header's name
        calls = (lambda: ctx.smc_cess(None, None, [0.5]), lambda: ctx.smc_choose_delta(None, None, 1.0, 0.9),
                 lambda: ctx.smc_reweight(None, None, 0.5), lambda: ctx.smc_quantise(None, 0.0), lambda: ctx.smc_ancestors(None, 0),
                 lambda: ctx.smc_run(), lambda: _capi.smc_cess_finish([np.zeros(6)], lib=oracle))
        for call in calls:
            with pytest.raises(_capi.RmhmcError) as e:
                call()
            assert e.value.code == -4 and "rmhmc_smc.h" in str(e.value)


def test_sampler_tables_unchanged():
    assert set(_capi.SAMPLERS_TO) == set(_capi.SAMPLER_ARGS) == {"rmhmc", "hmc", "mmala", "amh", "iwls", "gibbs"}
    assert set(experiment.SAMPLERS) == {"RMHMC", "HMC", "mMALA", "AMH", "IWLS", "Gibbs"}
    assert set(multi_gpu._SHARDED) == set(experiment.SAMPLERS)


# ---- csrc/smc.h in a stand-alone program under AddressSanitizer and UBSan ------------------------------------------------------------------
def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def test_candidate_grids_bit_for_bit(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    rs = np.random.RandomState(1)
    cases = [(0, rem, 0.0, rem) for rem in (1.0, 0.75, 1.0 / 3.0, 2.0 ** -53, 1.0 - 2.0 ** -53)]
    for _ in range(20):
        hi = rs.rand()
        cases += [(1, 1.0, 0.0, hi), (2, 1.0, hi * rs.rand(), hi), (1, 1.0, hi / 8.0, hi)]
    cases += [(2, 1.0, 0.3, 0.3), (1, 1.0, 0.3, np.nextafter(0.3, 1.0))]
    lines = _run(exe, "".join("grid %d %s %s %s\n" % (r, float(rem).hex(), float(lo).hex(), float(hi).hex()) for r, rem, lo, hi in cases))
    for (r, rem, lo, hi), line in zip(cases, lines):
        got = _floats(line[5:])
        assert _bits(got) == _bits(S.grid(r, rem, lo, hi)), (r, rem, lo, hi)
        assert got[-1] == (rem if r == 0 else hi) and np.all(np.diff(got) >= 0)
        if r == 0:                                   # exact scalings by 8
            assert all(got[j] * 8.0 ** (15 - j) == rem for j in range(16))


def frac_sequences():
    """recorded frac sequences per round (a round is read only if the search asks for it): name -> (remaining, rho, [16 frac] * 3)"""
    dec = np.linspace(0.999, 0.2, 16)
    nan0 = dec.copy(); nan0[0] = np.nan
    nan5 = dec.copy(); nan5[5] = np.nan
    bump = np.array([0.99, 0.95, 0.85, 0.95, 0.99, 0.5, 0.95] + [0.3] * 9)          # fails at 2, passes again later: the first failure counts
    return {"no_failure": (0.4, 0.9, [np.full(16, 0.95)] * 3), "no_failure_exact": (1.0, 0.9, [np.full(16, 0.9)] * 3),
            "floor": (1.0, 0.9, [np.full(16, 0.1)] * 3), "floor_nan": (0.5, 0.9, [np.full(16, np.nan)] * 3),
            "decreasing": (1.0, 0.9, [dec, dec, dec]), "first_round_only": (1.0, 0.9, [dec, np.full(16, 0.1), np.full(16, 0.1)]),
            "later_rounds_pass": (0.7, 0.9, [dec, np.full(16, 0.95), np.full(16, 0.95)]), "nan_first": (1.0, 0.9, [nan0, nan0, nan0]),
            "nan_middle": (1.0, 0.5, [nan5, nan5, nan5]), "non_monotone": (0.9, 0.9, [bump, bump[::-1].copy(), bump]),
            "last_fails": (1.0, 0.9, [np.array([0.95] * 15 + [0.5]), np.array([0.95] * 15 + [0.5]), np.array([0.95] * 15 + [0.5])]),
            "j0_then_pass": (1.0, 0.9, [np.full(16, 0.1), dec, dec])}


def test_bracket_rule_on_recorded_sequences(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    for name, (rem, rho, fracs) in frac_sequences().items():
        it = iter(fracs)
        want = S.search(lambda d: next(it), rem, rho)
        lines = _run(exe, "search %s %s\n%s\n" % (float(rem).hex(), float(rho).hex(), "\n".join(_hex(f) for f in fracs[:len(want["rounds"])])))
        assert len(lines) == len(want["rounds"]) + 1, name
        for line, (d, f, js) in zip(lines, want["rounds"]):
            assert _bits(_floats(line[6:])) == _bits(d), name
        head, delta, frac, flags = lines[-1].split()
        delta, frac = _floats(delta)[0], _floats(frac)[0]
        assert head == "result" and int(flags) == want["flags"], name
        assert _bits(delta) == _bits(want["delta"]) and (_bits(frac) == _bits(want["frac"]) or (np.isnan(frac) and np.isnan(want["frac"]))), name
    by_hand = {"no_failure": (0.4, S.LAST), "no_failure_exact": (1.0, S.LAST), "floor": (8.0 ** -15, S.FLOOR), "floor_nan": (0.5 * 8.0 ** -15, S.FLOOR),
               "nan_first": (8.0 ** -15, S.FLOOR), "j0_then_pass": None}
    for name, expect in by_hand.items():
        rem, rho, fracs = frac_sequences()[name]
        it = iter(fracs)
        got = S.search(lambda d: next(it), rem, rho)
        if expect is not None:
            assert (got["delta"], got["flags"]) == expect, name
        else:                                        # failure at j = 0 in round 0, then a bracket below the smallest candidate: no FLOOR
            assert got["flags"] == 0 and 0.0 < got["delta"] < 8.0 ** -15 and got["frac"] >= rho
    # a delta that is returned without FLOOR or LAST was a candidate that passed
    for name, (rem, rho, fracs) in frac_sequences().items():
        it = iter(fracs)
        got = S.search(lambda d: next(it), rem, rho)
        if got["flags"] == 0:
            assert any(got["delta"] == d[j] and f[j] >= rho and f[j] == got["frac"] for d, f, _ in got["rounds"] for j in range(16)), name


def test_resampling_offset(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    cases = [(0, 0), (0, 1), (1, 0), (12345, 7), (2 ** 64 - 1, 0), (2 ** 64 - 1, 3), (2 ** 64 - 3, 9999), (2 ** 63, 2 ** 31 - 1)]
    lines = _run(exe, "".join("u %d %d\n" % c for c in cases))
    for (seed, k), line in zip(cases, lines):
        assert int(line.split()[1]) == S.resample_u(seed, k) == _capi.smc_resample_u(seed, k) < 2 ** 32, (seed, k)
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF        # the published first output of splitmix64 from state 0
    assert len({S.resample_u(5, k) for k in range(64)}) == 64


def particle_cases():
    """(logw, loglik) that exercise the reduction: name -> pair"""
    rs = np.random.RandomState(11)
    n = 300
    ll3 = -1e5 + 1e4 * rs.randn(n)
    mixed_lw = rs.randn(n) * 3.0 - 40.0
    mixed_lw[[3, 77, 200]] = -np.inf
    mixed_lw[[0, 100, 299]] = np.nan
    mixed_ll = ll3.copy()
    mixed_ll[[5, 77, 150]] = -np.inf
    mixed_ll[[6, 100, 298]] = np.nan
    return {"narrow": (rs.randn(n) * 0.5 + 7.0, -50.0 + 5.0 * rs.randn(n)), "wide": (1e4 * (2.0 * rs.rand(n) - 1.0), ll3),
            "config3": (np.zeros(n), ll3), "mixed": (mixed_lw, mixed_ll), "equal_ll": (rs.randn(n), np.full(n, -3.25)),
            "all_neg_inf": (np.full(n, -np.inf), ll3), "all_nan": (np.full(n, np.nan), ll3), "all_failed": (rs.randn(n), np.full(n, np.nan))}


def _cess(exe, parts, J):
    lines = _run(exe, "cess %d %d\n" % (len(parts), J) + "\n".join(_hex(p) for p in parts) + "\n")
    rc = int(lines[0].split()[1])
    return (rc, _floats(lines[1]), _floats(lines[2])) if rc == 0 else (rc, None, None)


def test_cess_merge_and_finish_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    deltas = {1: [0.37], 3: [1e-6, 1e-3, 0.5], 16: S.grid(0, 1.0, 0.0, 1.0), 32: np.linspace(1e-5, 1.0, 32)}
    tol = CESS_UNITS * 2.0 ** -53
    for name, (lw, ll) in particle_cases().items():
        for J, d in deltas.items():
            whole = S.cess_partial(lw, ll, d)
            want = S.cess_finish([whole])
            cuts = [0, 7, 150, len(lw)]
            pieces = [S.cess_partial(lw[a:b], ll[a:b], d) for a, b in zip(cuts[:-1], cuts[1:])]
            empty = S.cess_partial([], [], d)
            assert np.all(empty[0::2] == -np.inf) and np.all(empty[1::2] == 0)
            two = [S.cess_partial(lw[:150], ll[:150], d), S.cess_partial(lw[150:], ll[150:], d)]
            for parts in ([whole], two, pieces, pieces[::-1], [empty] + pieces + [empty]):
                rc, merged, frac = _cess(exe, [np.asarray(p, dtype=np.float64) for p in parts], J)
                assert rc == 0 and merged.shape == (2 + 4 * J,) and frac.shape == (J,)
                Lg, Lw = S.cess_levels(merged), S.cess_levels(want["merged"])
                assert np.array_equal(np.isinf(Lg), np.isinf(Lw)), name
                fin = np.isfinite(Lw)
                assert np.all(np.abs(Lg[fin] - Lw[fin]) <= tol + 2.0 ** -52 * np.abs(Lw[fin])), (name, J)
                assert np.array_equal(np.isnan(frac), np.isnan(want["frac"])), (name, J)
                ok = ~np.isnan(frac) & (want["frac"] > 1e-300)          # (below that the double underflows: exp of less than -690)
                assert np.all(frac[~np.isnan(frac) & ~ok] < 1e-299)
                # frac = exp(2 L1 - L0 - L2) in double: four levels, each good to tol and rounded, and two roundings of the exponent
                scale = float(np.max(np.abs(Lw[fin]))) if fin.any() else 0.0
                assert np.all(np.abs(np.log(frac[ok].astype(S.LD)) - np.log(want["frac"][ok])) <= 4 * tol + 12 * 2.0 ** -53 * max(1.0, scale)), (name, J)
                assert np.all(frac[ok] <= 1.0 + 1e-9) and np.all(frac[ok] > 0.0)
            rc, merged, _ = _cess(exe, [np.asarray(empty, dtype=np.float64), np.asarray(whole, dtype=np.float64),
                                        np.asarray(empty, dtype=np.float64)], J)                      # the identity, to the bit
            assert rc == 0 and _bits(merged) == _bits(np.asarray(whole, dtype=np.float64))
    assert np.isnan(S.cess_finish([S.cess_partial(*particle_cases()["all_nan"], [0.5])])["frac"]).all()
    assert np.isnan(S.cess_finish([S.cess_partial(*particle_cases()["all_failed"], [0.5])])["frac"]).all()
    assert abs(float(S.cess_finish([S.cess_partial(*particle_cases()["equal_ll"], [0.5])])["frac"][0]) - 1.0) < 1e-15
    for head in ("cess 0 1", "cess 1 0", "cess 1 33"):
        assert _run(exe, head + "\n")[0] == "cess -1", head


def test_scan_plan_covers_every_entry_once(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    sizes = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 70001, 2 ** 20 - 1, 2 ** 20]
    lines = _run(exe, "".join("plan %d\ncover %d\n" % (n, n) for n in sizes))
    for i, n in enumerate(sizes):
        assert lines[2 * i] == "plan %d %d" % S.scan_plan(n), n
        assert lines[2 * i + 1] == "cover ok", n
    by_hand = {1: (1, 1024), 1024: (1, 1024), 1025: (2, 1024), 70001: (69, 1024), 2 ** 20: (1024, 1024)}
    assert {n: S.scan_plan(n) for n in by_hand} == by_hand
    asks = [(n, b, t) for n in (1, 5, 1023, 1024, 1025, 2049, 70001) for b in range(S.scan_plan(n)[0]) if b in (0, 1, S.scan_plan(n)[0] - 1)
            for t in (0, 1, 2, 127, 254, 255)]
    lines = _run(exe, "".join("range %d %d %d\n" % a for a in asks))
    for (n, b, t), line in zip(asks, lines):
        assert tuple(int(v) for v in line.split()[1:]) == S.scan_range(n, b, t), (n, b, t)
    assert S.scan_range(1025, 1, 0) == (1024, 1025) and S.scan_range(1025, 1, 1) == (1025, 1025) and S.scan_range(1025, 0, 255) == (1020, 1024)


def test_every_refusal_under_sanitizers(tmp_path_factory):
    exe = probe_exe(tmp_path_factory, "smc_probe")
    ok = dict(have_theta0=0, beta0=0.0, rho=0.9, tau=0.5, T_max=10, stage_len=1, mass_every=1, have_H=1, L=6)
    cases = [ok, dict(ok, tau=0.0), dict(ok, tau=1.0), dict(ok, have_theta0=1, beta0=0.3), dict(ok, mass_every=0, have_H=0), dict(ok, mass_every=7),
             dict(ok, rho=0.0), dict(ok, rho=1.0), dict(ok, rho=np.nan), dict(ok, rho=-0.5), dict(ok, tau=-0.1), dict(ok, tau=1.1), dict(ok, tau=np.nan),
             dict(ok, T_max=0), dict(ok, T_max=-3), dict(ok, stage_len=0), dict(ok, L=0), dict(ok, beta0=0.3), dict(ok, have_theta0=1, beta0=1.0),
             dict(ok, have_theta0=1, beta0=-0.1), dict(ok, have_theta0=1, beta0=np.nan), dict(ok, have_theta0=1, beta0=np.inf),
             dict(ok, mass_every=-1), dict(ok, have_H=0)]
    text = "".join("checkrun %d %s %s %s %d %d %d %d %d\n" % (c["have_theta0"], repr(float(c["beta0"])), repr(float(c["rho"])), repr(float(c["tau"])),
                                                             c["T_max"], c["stage_len"], c["mass_every"], c["have_H"], c["L"]) for c in cases)
    got = _run(exe, text)
    for c, line in zip(cases, got):
        assert (line == "check ok") == S.check_run(**c), (c, line)
    assert [line == "check ok" for line in got[:7]] == [True] * 6 + [False] and sum(line == "check ok" for line in got) == 6
    d = " ".join(["0.5"] * 32)
    for line, fine in (("checkcess 5 32 " + d, True), ("checkcess 1 1 1e-300", True), ("checkcess 0 1 0.5", False), ("checkcess 5 0", False),
                       ("checkcess 5 33 " + d + " 0.5", False), ("checkcess 5 2 0.5 0", False), ("checkcess 5 2 -0.5 0.5", False),
                       ("checkcess 5 2 0.5 nan", False), ("checkcess 5 2 inf 0.5", False),
                       ("checksearch 5 1 0.9", True), ("checksearch 5 1e-16 0.5", True), ("checksearch 0 1 0.9", False), ("checksearch 5 0 0.9", False),
                       ("checksearch 5 1.5 0.9", False), ("checksearch 5 nan 0.9", False), ("checksearch 5 1 0", False), ("checksearch 5 1 1", False),
                       ("checksearch 5 1 nan", False)):
        assert (_run(exe, line + "\n")[0] == "check ok") == fine, line
    assert _run(exe, "checkanc 1\ncheckanc 1048576\ncheckanc 1048577\ncheckanc 0\ncheckanc -4\n") == ["checkanc 0", "checkanc 0", "checkanc -4",
                                                                                                    "checkanc -1", "checkanc -1"]
    asks = [(k, e, f) for k in (0, 1, 4, 5, 10) for e in (0, 1, 5) for f in (0, S.LAST, S.FLOOR, S.LAST | S.RESAMPLED)]
    lines = _run(exe, "".join("smass %d %d %d\n" % a for a in asks))
    for a, line in zip(asks, lines):
        assert line == "smass %d" % int(S.stage_mass(*a)), a
    assert not S.stage_mass(3, 0, S.LAST) and S.stage_mass(3, 5, S.LAST) and not S.stage_mass(3, 5, 0) and S.stage_mass(10, 5, 0)


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------
def test_restated_cess_is_the_formula_on_normalised_weights():
    rs = np.random.RandomState(2)
    for n in (1, 2, 17, 400):
        lw = rs.randn(n) * 2.0
        ll = -30.0 + 4.0 * rs.randn(n)
        if n >= 17:
            ll[3] = np.nan; ll[9] = -np.inf; lw[5] = -np.inf
        d = [1e-3, 0.1, 0.7, 1.0]
        got = S.cess_finish([S.cess_partial(lw, ll, d)])["frac"]
        want = np.array([S.cess_brute(lw, ll, x) for x in d])
        assert np.all(np.abs(got - want) <= 1e-15 * want), n
        assert np.all(got > 0) and np.all(got <= 1 + 1e-15)
        if n >= 17:
            assert np.all(np.diff(got.astype(np.float64)) < 0)               # a longer step, a smaller conditional ESS
    assert S.cess_finish([S.cess_partial([0.0], [-5.0], [0.5])])["frac"][0] == 1


def test_restated_ancestors_are_the_definition():
    rs = np.random.RandomState(4)
    for n in (1, 2, 3, 64, 257, 1500):
        arrays = {"random": rs.randint(0, 2 ** 40 + 1, n).tolist(), "equal": [2 ** 40] * n, "first": [5] + [0] * (n - 1), "last": [0] * (n - 1) + [1],
                  "sparse": [int(v) if i % 97 == 0 else 0 for i, v in enumerate(rs.randint(1, 2 ** 40, n))]}
        for name, q in arrays.items():
            for U in (0, 1, 2 ** 31, 2 ** 32 - 1):
                anc = S.ancestors(q, U)
                assert anc.tolist() == S.ancestors_direct(q, U), (name, n, U)
                assert np.all(np.diff(anc) >= 0)
                Q = sum(q)
                counts = np.bincount(anc, minlength=n)
                for i in range(n):
                    assert counts[i] - (n * q[i]) // Q in (0, 1), (name, n, U, i)
                if name == "equal":
                    assert anc.tolist() == list(range(n))
    lw = np.array([0.0, -1.0, -np.inf, np.nan, -800.0, 3.0])
    assert S.quantise(lw, 3.0) == [int(np.floor(S.LD(2) ** 40 * np.exp(S.LD(-3)))), int(np.floor(S.LD(2) ** 40 * np.exp(S.LD(-4)))), 0, 0, 0, 2 ** 40]
    assert S.reweight([1.0, np.nan, -np.inf, 2.0, 3.0], [-2.0, -2.0, -2.0, np.nan, -np.inf], 0.5).tolist()[0] == 0.0
    got = S.reweight([1.0, np.nan, -np.inf, 2.0, 3.0], [-2.0, -2.0, -2.0, np.nan, -np.inf], 0.5)
    assert np.isnan(got[1]) and got[2] == -np.inf and got[3] == -np.inf and got[4] == -np.inf


N_REPEATS, N_CHAINS, CESS_TARGET, RESAMPLE_BELOW = 8, 512, 0.9, 0.5     # the conditions of the estimator test, here and on the GPU
SE_LARGEST = {"m25_d1": 0.0334, "m40_d2": 0.0438}                       # the largest se the restatement showed over its 8 seeds


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_restated_smc_meets_the_quadrature(name, seed):
    """|log Z - quadrature| <= 5 se, log Z the log of the mean estimate of 8 repeats of 512 particles (cess_target 0.9, resample_below
    0.5, one transition per stage, a mass per stage) and se its delta-method standard error over the repeats; each seed prints its
    figures.  Over the 8 seeds the restatement showed: m25_d1 largest |log Z - quadrature| / se 4.16 (two seeds above 4, at
    se 0.0102 and 0.0182: an se from 8 repeats is itself uncertain by a quarter), largest se 0.0334, 10 stages, 1-2 of them resampled;
    m40_d2 largest ratio 1.55, largest se 0.0438, 14-15 stages, 2-3 resampled.  All 16 inside 5 se at 512 particles: the number was not
    raised.  96 further runs per setting show no bias: mean Z / Z_quadrature 0.998 +- 0.007 (m25_d1, 512 particles)."""
    M, D, _ = PROBLEMS[name]
    XX, t = synthetic_logreg(M, D, 0)
    H = R.metric(XX, R.mode(XX, t)["w"]) - np.eye(D) / 100.0
    runs = [S.run(XX, t, N_CHAINS, CESS_TARGET, RESAMPLE_BELOW, 1, H, seed=1000 * seed + r) for r in range(N_REPEATS)]
    lz, se = S.combine([r["log_z"] for r in runs])
    ref = quadrature(name)
    print("%s seed %d: log Z %.5f, quadrature %.5f, (log Z - quadrature) / se %+.2f, se %.4f, stages %s, resampled %s, acceptance %.3f .. %.3f"
          % (name, seed, lz, ref, (lz - ref) / se, se, [r["T"] for r in runs], [int((r["flags"] & S.RESAMPLED > 0).sum()) for r in runs],
             min(r["accept_trace"].min() for r in runs), max(r["accept_trace"].max() for r in runs)))
    for r in runs:
        assert r["beta"][-1] == 1.0 and r["flags"][-1] & S.LAST and np.all(np.diff(r["beta"]) > 0) and not (r["flags"] & S.FLOOR).any()
        assert np.all(r["cess"] >= CESS_TARGET) and np.all(r["cess"] <= 1.0 + 1e-12)
    assert se <= SE_LARGEST[name]
    assert abs(lz - ref) <= 5 * se


# ---- the shim's checks: before the library is touched ------------------------------------------------------------------------------------
class _NoLibrary:
    """stands in for the library: the argument checks must raise before anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the shim touched the library (%s) before refusing its arguments" % name)


def test_shim_argument_checks_need_no_library():
    XX, t = synthetic_logreg(30, 3, 0)
    bad = [dict(XX=XX[0]), dict(t=t[:-1]), dict(n_chains=1), dict(n_chains=2.5), dict(n_chains=2 ** 20 + 1), dict(cess_target=0.0),
           dict(cess_target=1.0), dict(cess_target=np.nan), dict(resample_below=-0.1), dict(resample_below=1.5), dict(resample_below=np.nan),
           dict(iters_per_temp=0), dict(iters_per_temp=1.5), dict(mass="identity"), dict(mass=np.eye(3)), dict(mass_every=0), dict(max_temps=0),
           dict(max_temps=2 ** 31), dict(repeats=0), dict(repeats=1.5), dict(NumOfLeapFrogSteps=0), dict(StepSize=0.0), dict(StepSize=np.nan),
           dict(alpha=0.0), dict(alpha=np.inf)]
    for kw in bad:
        args = dict(XX=XX, t=t, n_chains=8, _lib=_NoLibrary())
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.log_evidence_adaptive(**args)
    with pytest.raises(AssertionError):                 # ... and a call that passes them reaches the library
        pkg.log_evidence_adaptive(XX, t, n_chains=8, _lib=_NoLibrary())
